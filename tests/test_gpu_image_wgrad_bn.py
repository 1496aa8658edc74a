"""The image convolution's weight gradient with the BatchNorm(+ReLU) backward
apply in its operand path (csrc/conv_image_wgrad.hip, vu_conv_image_wgrad_bn;
engine.FUSE_IMAGE_WGRAD_BN).

Reference: dy_ref = the bf16 bytes vu_bn_bwd_apply stores for the same inputs,
dW_ref = sum_p dy_ref[p, co] * patch[p, col] in fp64 on the CPU.  A bf16 x bf16
product is exact in fp32, so the only error of any kernel is fp32 accumulation:
for every element

    |dW - dW_ref| <= (P - 1) * 2^-24 * sum_p |dy_ref * patch|,

the order-independent summation bound (derived, not tuned).  An accumulating
launch adds one more term (the old value) and one more rounding: P instead of
P - 1, and |old| joins the sum.  The existing vu_gemm_wgrad path must meet the
same bound on the same inputs."""
import functools

import pytest
import torch
import torch.nn.functional as F

import ref_small as R
from test_gpu_kernels import DEV

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
C = 64
# N, H, W: one wave tile with every pixel on a border; P = 70 (ragged tile, odd
# width, batch seam inside a tile); several waves; more tiles than one block
# takes (with 2 slabs: 54 tiles over 8 waves)
SHAPES = [(1, 8, 8), (2, 5, 7), (1, 16, 40), (3, 24, 24)]


def _k():
    from vaeunet_amd import kernels as K
    return K


def _bf(t):
    return t.to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _inputs(shape, nc, zero_pre):
    """CPU inputs, rounded to bf16 where stored so: y, da [N, 64, H, W]; the
    packed image [N, 8, H, W] whose channels >= nc hold non-zero values
    (cvalid must drop them); coef rows scale, shift, mean, invstd; gamma."""
    N, H, W = shape
    g = torch.Generator().manual_seed(1000 * N + 10 * H + W + nc)
    scale, shift, mean, invstd, gamma = R.bn_coef_inputs(C, seed=31)
    y = _bf(torch.randn(N, C, H, W, generator=g)).float()
    if zero_pre:
        # every pre-activation y * scale + shift is an exact zero of the
        # unfused multiply-add (shift = -fl(y * scale), y constant per
        # channel): the fused one leaves the product's rounding residue, whose
        # sign alone decides the mask
        yc = _bf(torch.randn(C, generator=g) + 2.0).float()
        y = yc.view(1, C, 1, 1).expand(N, C, H, W).contiguous()
        shift = -(yc * scale)
    else:
        y = R.condition_bn_input(y, scale.view(1, C, 1, 1), shift.view(1, C, 1, 1), torch.bfloat16)
    da = _bf(torch.randn(N, C, H, W, generator=g)).float()
    img = _bf(torch.rand(N, 8, H, W, generator=g) + 0.25).float()
    coef = torch.stack([scale, shift, mean, invstd])
    return y, da, img, coef, gamma


def _dev_act(x, strided):
    """CPU [N, C, H, W] -> bf16 NHWC on the device, dense or as the channel
    slice [C, 2C) of a tensor twice as wide."""
    N, Cc, H, W = x.shape
    t, _ = R.guarded_act(N, Cc, H, W, torch.bfloat16, DEV, wide=2 * Cc if strided else None,
                         c0=Cc if strided else 0)
    t.copy_(_bf(x))
    return t


def _reference(dy_ref, img, nc):
    """fp64 dW_ref [64, nc, 3, 3] and sum |dy * patch| of the same shape."""
    N, _, H, W = img.shape
    dy = dy_ref.double().permute(0, 2, 3, 1).reshape(-1, C)                    # [P, 64]
    pt = F.unfold(img[:, :nc].double(), 3, padding=1)                          # [N, nc*9, HW]
    pt = pt.permute(0, 2, 1).reshape(-1, nc * 9)                               # [P, nc*9], col = c*9 + tap
    ref = (dy.t() @ pt).view(C, nc, 3, 3)
    sabs = (dy.abs().t() @ pt.abs()).view(C, nc, 3, 3)
    return ref, sabs


def _check(got, ref, sabs, P, old, what):
    got = got.double().cpu()
    if old is None:
        bound = (P - 1) * U32 * sabs
    else:
        ref = ref + old.double()
        bound = P * U32 * (sabs + old.double().abs())
    err = (got - ref).abs()
    print(f"{what}: max err {float(err.max()):.3e}, max err/bound {float((err / (bound + 1e-300)).max()):.3e}")
    assert bool((err <= bound).all()), (what, float((err / (bound + 1e-300)).max()))


def _run_case(shape, relu, train, strided, nc, accumulate, zero_pre=False, nslab=None, plain=False):
    from vaeunet_amd import _lib
    K = _k()
    N, H, W = shape
    P = N * H * W
    y_c, da_c, img_c, coef_c, gamma_c = _inputs(shape, nc, zero_pre)
    y, da = _dev_act(y_c, strided), _dev_act(da_c, strided)
    img = _dev_act(img_c, False)
    coef, gamma = coef_c.to(DEV), gamma_c.to(DEV)
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    k = K.bn_backward_reduce(da, y, coef, gamma, relu, dg, db, False, _lib.BF16, train=train)
    if not train:
        assert float(k[1:].abs().max()) == 0.0
    dy_ref = torch.empty((N, C, H, W), dtype=torch.bfloat16, device=DEV, memory_format=torch.channels_last)
    K.call("vu_bn_bwd_apply", K.ptr(da), K.pstride(da), K.ptr(y), K.pstride(y), P, C, K.ptr(coef[0]), K.ptr(coef[1]),
           K.ptr(coef[2]), K.ptr(k), 1 if relu else 0, K.ptr(dy_ref), C, _lib.BF16, K.stream())
    torch.cuda.synchronize()
    ref, sabs = _reference(dy_ref.float().cpu(), img_c, nc)
    if zero_pre and relu:
        # the case means what it says: the masks are not all alike
        pre = torch.addcmul(coef_c[1].double().view(1, C, 1, 1), y_c.double(), coef_c[0].double().view(1, C, 1, 1))
        assert bool((pre > 0).any()) and bool((pre <= 0).any()) and float(pre.abs().max()) < 1e-6

    gold = torch.Generator().manual_seed(5)
    old_c = torch.randn(C, nc, 3, 3, generator=gold) if accumulate else None

    def sink():
        g, guard = R.guarded((C, nc, 3, 3), torch.float32, DEV)
        if accumulate:
            g.copy_(old_c)
        return g, guard

    # ---- the fused kernel
    assert K.image_wgrad_bn_ok(da, y, img, _lib.BF16)
    ns = nslab or K.query("vu_conv_image_wgrad_bn_slabs", N, H, W)
    slab, gslab = R.guarded((ns, C, 72), torch.float32, DEV)
    grad, ggrad = sink()
    src = dy_ref if plain else da
    K.call("vu_conv_image_wgrad_bn", K.ptr(src), K.pstride(src), None if plain else K.ptr(y),
           0 if plain else K.pstride(y), K.ptr(coef[0]), K.ptr(coef[1]), K.ptr(coef[2]), K.ptr(k), 1 if relu else 0,
           K.ptr(img), K.pstride(img), N, H, W, K.ptr(slab), ns, K.stream())
    s = grad.stride()
    K.call("vu_slab_reduce", K.ptr(slab), ns, C, 72, 8, nc, s[0], s[3], s[1], K.ptr(grad), 1 if accumulate else 0,
           K.stream())
    torch.cuda.synchronize()
    gslab.check("slabs")
    ggrad.check("gradient")
    assert bool((slab != R.SENTINEL).all()), "a slab element was not written"
    _check(grad, ref, sabs, P, old_c, f"fused {shape} relu={relu} train={train} strided={strided} nc={nc}")

    # ---- the existing path on the same inputs: the bound is fair
    grad2, ggrad2 = sink()
    K.gemm_wgrad(K.gather1x1([dy_ref]), K.gather3x3([img]), C, 72, grad2, (s[0], s[3], s[1]), _lib.BF16,
                 accumulate, cvalid=nc)
    torch.cuda.synchronize()
    ggrad2.check("gradient (vu_gemm_wgrad)")
    _check(grad2, ref, sabs, P, old_c, f"vu_gemm_wgrad {shape}")
    return grad


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("relu", [True, False])
def test_kernel_against_reference(shape, relu):
    _run_case(shape, relu, True, False, 3, False)


@pytest.mark.parametrize("shape", SHAPES)
def test_eval_mode_strided_accumulate_one_channel(shape):
    """train = 0 (k2 = k3 = 0), da and y as channel slices of wider tensors,
    accumulation through vu_slab_reduce, n_channels = 1."""
    _run_case(shape, True, False, True, 1, True)


@pytest.mark.parametrize("strided,accumulate", [(True, False), (False, True)])
def test_strides_and_accumulate_separately(strided, accumulate):
    _run_case((2, 5, 7), True, True, strided, 3, accumulate)


def test_more_tiles_than_a_block_takes_two_slabs():
    """3 x 24 x 24 = 54 tiles on 2 blocks (8 waves): every wave walks 6-7
    tiles, the last one short of the stride; and on 1 block."""
    _run_case((3, 24, 24), True, True, False, 3, False, nslab=2)
    _run_case((3, 24, 24), True, True, True, 3, True, nslab=1)


def test_more_slabs_than_tiles():
    """blocks without a tile write zero slabs"""
    _run_case((1, 8, 8), True, True, False, 3, False, nslab=5)


@pytest.mark.parametrize("relu", [True, False])
def test_exact_zero_preactivations(relu):
    _run_case((1, 16, 40), relu, True, False, 3, False, zero_pre=True)


@pytest.mark.parametrize("shape", SHAPES)
def test_plain_variant_dy_given(shape):
    """y = NULL: the same body over a stored dy."""
    _run_case(shape, True, True, False, 3, False, plain=True)


def test_run_to_run_deterministic():
    a = _run_case((3, 24, 24), True, True, False, 3, False)
    b = _run_case((3, 24, 24), True, True, False, 3, False)
    assert torch.equal(a, b)


def test_refusals():
    from vaeunet_amd import _lib
    K = _k()
    ok = lambda *a: K.query("vu_conv_image_wgrad_bn_ok", *a)  # noqa: E731
    assert ok(64, 8, 64, 64, 8, 2, 16, 16, _lib.BF16) == 1
    assert ok(64, 8, 128, 192, 8, 2, 16, 16, _lib.BF16) == 1
    assert ok(32, 8, 64, 64, 8, 2, 16, 16, _lib.BF16) == 0      # C != 64
    assert ok(128, 8, 128, 128, 8, 2, 16, 16, _lib.BF16) == 0
    assert ok(64, 16, 64, 64, 16, 2, 16, 16, _lib.BF16) == 0    # packed width != 8
    assert ok(64, 8, 68, 64, 8, 2, 16, 16, _lib.BF16) == 0      # misaligned strides
    assert ok(64, 8, 64, 100, 8, 2, 16, 16, _lib.BF16) == 0
    assert ok(64, 8, 64, 64, 12, 2, 16, 16, _lib.BF16) == 0
    assert ok(64, 8, 64, 64, 8, 2, 16, 16, _lib.F32) == 0       # fp32
    # the launch itself refuses what the query refuses
    t = torch.zeros(64, device=DEV)
    rc = K.query("vu_conv_image_wgrad_bn", K.ptr(t), 68, K.ptr(t), 64, K.ptr(t), K.ptr(t), K.ptr(t), K.ptr(t), 1,
                 K.ptr(t), 8, 1, 1, 1, K.ptr(t), 1, K.stream())
    assert rc != 0


# ----------------------------------------------------------------------------
# engine
# ----------------------------------------------------------------------------
def _double_conv_case():
    from vaeunet_amd.unet_parts import DoubleConv
    torch.manual_seed(3)
    dc = DoubleConv(3, 64).to(DEV).train()
    with torch.no_grad():
        for m in (dc.double_conv[1], dc.double_conv[4]):
            m.weight.uniform_(0.5, 1.5)
            m.bias.normal_(0, 0.3)
    gen = torch.Generator().manual_seed(17)
    x = torch.rand(2, 3, 16, 16, generator=gen).to(DEV)
    da2 = _bf(torch.randn(2, 64, 16, 16, generator=gen)).to(DEV).contiguous(memory_format=torch.channels_last)
    return dc, x, da2


def _engine_run(monkeypatch, dc, x, da2, on, audit=None, need_dx=False):
    """(gradients, the C calls as (name, args), saved tensors, packed image,
    input gradient) of one double_conv_bwd."""
    from vaeunet_amd import _lib, engine as E
    K = _k()
    M = E.Mode(_lib.BF16, torch.device(DEV))
    monkeypatch.setattr(E, "FUSE_IMAGE_WGRAD_BN", on)
    for p in dc.parameters():
        p.grad = None
    with torch.no_grad():
        xa = E.to_act(M, x, 8)
        _, saved = E.double_conv_fwd(M, dc.double_conv, [xa], cin_pad=8)
    calls = []
    real_call = K.call

    def spy(name, *a):
        calls.append((name, a))
        return real_call(name, *a)
    monkeypatch.setattr(K, "call", spy)
    monkeypatch.setattr(K, "AUDIT", audit)
    out = E.double_conv_bwd(M, dc.double_conv, saved, da2.clone(), need_dx, cvalid=3)
    monkeypatch.setattr(K, "AUDIT", None)
    monkeypatch.setattr(K, "call", real_call)
    M.join()
    torch.cuda.synchronize()
    assert (out is None) == (not need_dx)
    return {n: p.grad.clone() for n, p in dc.named_parameters()}, calls, saved, xa, out


def _image_launches(calls):
    """per vu_conv_image_wgrad_bn launch: True = BN apply in the operand path
    (y given), False = over a stored dy"""
    return [a[2] is not None for name, a in calls if name == "vu_conv_image_wgrad_bn"]


@pytest.mark.parametrize("small_path,need_dx", [(False, False), (True, False), (False, True)])
def test_engine_switch_on_off(monkeypatch, small_path, need_dx):
    """DoubleConv(3, 64) on 2 x 3 x 16 x 16: everything but conv1's weight
    gradient bit-identical between the switch on and off, conv1's within the
    bound in both.  A tensor this small takes vu_bn_bwd_fused by default, whose
    own reduction the fused path does not reproduce, so it keeps that BatchNorm
    backward and the kernel runs over the stored dy (small_path), as it does
    when the image's gradient is wanted (need_dx); with FUSED_BN_BWD off the
    BatchNorm backward is the reduce + apply pair of the large layers and the
    switch moves the apply into the weight gradient."""
    from vaeunet_amd import _lib, engine as E
    K = _k()
    monkeypatch.setattr(E, "FUSED_BN_BWD", small_path)
    dc, x, da2 = _double_conv_case()
    res = {}
    for on in (False, True):
        grads, calls, saved, xa, dx = _engine_run(monkeypatch, dc, x, da2, on, need_dx=need_dx)
        assert _image_launches(calls) == ([not (small_path or need_dx)] if on else []), [c[0] for c in calls]
        res[on] = grads
        if need_dx:
            res[on] = dict(grads, dx=dx.clone())
    for n in res[False]:
        if n != "double_conv.0.weight":
            assert torch.equal(res[True][n], res[False][n]), n
    # conv1.weight.grad against fp64 from dy1 = vu_bn_bwd_apply's bytes (the
    # unfused path's operand), recomputed here from the saved tensors
    M = E.Mode(_lib.BF16, torch.device(DEV))
    srcs, a1, s1, s2 = saved
    conv1, bn1, _, conv2, bn2, _ = dc.double_conv
    for p in dc.parameters():
        p.grad = None
    monkeypatch.setattr(E, "FUSE_IMAGE_WGRAD_BN", False)
    da1, part = E.conv_bn_relu_bwd(M, [a1], conv2, bn2, s2, da2.clone(), True, feeds=(s1, bn1))
    dy1 = E.bn_bwd(da1, s1[0], s1[1], bn1, True, M, part=part)
    torch.cuda.synchronize()
    ref, sabs = _reference(dy1.float().cpu(), xa.float().cpu(), 3)
    for on in (False, True):
        _check(res[on]["double_conv.0.weight"], ref, sabs, 2 * 16 * 16, None, f"engine conv1.weight.grad on={on}")


def test_engine_under_gemm_audit(monkeypatch):
    """With a GEMM audit installed the unfused launches are reported as
    before: both weight gradients and the input gradient, no fused call."""
    from gemm_audit import GemmAudit
    from vaeunet_amd import engine as E
    monkeypatch.setattr(E, "FUSED_BN_BWD", False)
    dc, x, da2 = _double_conv_case()
    recs = {}
    for on in (False, True):
        audit = GemmAudit(strict=True)
        _, calls, _, _, _ = _engine_run(monkeypatch, dc, x, da2, on, audit=audit)
        assert _image_launches(calls) == []
        recs[on] = [(r["op"], r["kernel"], r["M"], r["N"], r["acc"]) for r in audit.records]
    assert recs[True] == recs[False]
    assert len([r for r in recs[True] if r[0] == "wgrad"]) == 2
