"""The inference-side kernels of csrc/infer.hip, each called through the C ABI
on guarded buffers and compared with a plain CPU reference (tests/ref_small.py).

Bounds (u = 2^-24):

  vu_mean_groups    bitwise: the left-to-right fp32 sum over k, divided by groups
  vu_sigmoid        |y - y_64| <= 4 max(r_cpu, 1) u |y_64| + 2^-126; NaN -> NaN
  vu_patch_blend    wsum bitwise (fp32 CPU); out within u (|p w| + |out|) of the fp32
                    CPU result (the multiply-add may or may not be contracted)
  vu_blend_finish   bitwise: out / (wsum + 1e-8f) in fp32
  vu_uncertainty    each of the five maps within 4 max(r_cpu, 1) u sabs + 2^-126 of
                    fp64; NaN exactly where the reference has it (std, cv at S = 1)
  vu_gather_affine  bitwise: torch.flip / torch.rot90 of the same tensor

r_cpu is the error of the same formulas evaluated by torch in float32 on the
CPU on the same inputs, in the same units (the convention of
test_gpu_ma_loss.py); sabs is the formula on |operands|.  The planted special
values and the random remainder are each held to their own r_cpu, so an
ill-conditioned planted element does not loosen the bound of the rest.

Worst ratios measured on the MI355X (the CPU's float32 figure in brackets),
random elements / planted ones:
  sigmoid      2.47 (2.47) at n = 65535 * 256 + 3 / 0.70 (0.70)
  mean         2.93 (2.93) / 1.19 (1.19)
  std          0.75 (0.84) / 0.60 (0.60)
  cv           1.74 (1.74) / 0.77 (0.77)
  entropy      294 (294) / 8.3e6 (8.3e6)
  mutual info  24.3 (24.3) / 4.1e6 (4.1e6)
The planted entropy figures come from v = 1 - 1e-7, where v + eps rounds to 1 in
float32 and the logarithm loses the whole term on either machine; the random
ones from v close to 1.  Everything else is bitwise or within its stated slack.
"""
import pytest
import torch

import ref_small as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32 = torch.float32
INVALID = 1   # hipErrorInvalidValue
N_LIST = [1, 255, 257, 4099]


def _lib():
    from vaeunet_amd import _lib as L
    return L


def _call(name, *args):
    L = _lib()
    L.call(name, *args, L.stream())
    torch.cuda.synchronize()


def _ptr(t):
    return _lib().ptr(t)


def _put(x, dtype=None):
    """CPU tensor -> guarded contiguous device tensor holding it."""
    t, g = R.guarded(tuple(x.shape), dtype or x.dtype, DEV)
    t.copy_(x)
    return t, g


def _same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


# ----------------------------------------------------------------------------
# vu_mean_groups
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("groups", [1, 3, 8])
def test_mean_groups(groups, n):
    g = torch.Generator().manual_seed(41 + groups + n)
    x = torch.randn(groups, n, generator=g) * torch.tensor([10.0 ** (k % 4 - 2) for k in range(groups)])[:, None]
    xd, gx = _put(x)
    out, go = R.guarded(n, F32, DEV)
    _call("vu_mean_groups", _ptr(xd), groups, n, _ptr(out))
    gx.check("mean_groups x")
    go.check("mean_groups out")
    assert _same_bits(out, R.mean_groups_ref(x))
    assert torch.equal(xd.cpu(), x)


# ----------------------------------------------------------------------------
# vu_sigmoid
# ----------------------------------------------------------------------------
SIG_BIG = 65535 * 256 + 3   # one element more than the capped grid covers in one sweep


@pytest.mark.parametrize("n", N_LIST + [SIG_BIG])
def test_sigmoid(n):
    g = torch.Generator().manual_seed(42)
    x = torch.randn(n, generator=g) * 6.0
    special = torch.tensor([90.0, -90.0, float("inf"), float("-inf"), float("nan"), 0.0, -87.5, 17.0])
    k = min(n, special.numel())
    x[:k] = special[:k]
    if n > 16:
        x[-k:] = special[:k]   # the tail the second sweep of the grid reaches
    xd, gx = _put(x)
    y, gy = R.guarded(n, F32, DEV)
    _call("vu_sigmoid", _ptr(xd), n, _ptr(y))
    gx.check("sigmoid x")
    gy.check("sigmoid y")
    ref64, sabs = R.sigmoid_ref(x)
    ref32, _ = R.sigmoid_ref(x, F32)
    yc = y.cpu()
    assert torch.equal(torch.isnan(yc), torch.isnan(x))
    planted = torch.zeros(n, dtype=torch.bool)
    planted[:k] = True
    if n > 16:
        planted[-k:] = True
    R.assert_trans(yc, ref64, ref32, sabs, f"sigmoid n={n}", split=planted)
    if n >= 4:
        assert float(yc[0]) == 1.0 and float(yc[2]) == 1.0 and float(yc[3]) == 0.0
        assert 0.0 <= float(yc[1]) <= R.TINY


# ----------------------------------------------------------------------------
# vu_patch_blend / vu_blend_finish
# ----------------------------------------------------------------------------
def _blend_setup(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    out0 = torch.randn(B, H, W, generator=g)
    ws0 = torch.rand(B, H, W, generator=g)
    return g, out0, ws0


def _ramp(ov):
    return torch.linspace(0, 1, ov) if ov > 0 else torch.zeros(1)


def _blend_call(pred_d, stride, B, ph, pw, out, wsum, H, W, sh, sw, ramp_d, ov, edges):
    _call("vu_patch_blend", _ptr(pred_d), stride, B, ph, pw, _ptr(out), _ptr(wsum), H, W, sh, sw, _ptr(ramp_d), ov,
          *[int(e) for e in edges])


def _check_blend(out, wsum, out_ref, ws_ref, slack, guards, what):
    for gd in guards:
        gd.check(what)
    assert _same_bits(wsum, ws_ref), f"{what}: wsum"
    diff = (out.cpu().double() - out_ref.double()).abs()
    untouched = slack == 0
    assert _same_bits(out.cpu()[untouched], out_ref[untouched]), f"{what}: out outside the patch"
    assert bool((diff <= R.U32 * slack).all()), f"{what}: out, worst {float((diff / (R.U32 * slack + 1e-300)).max()):.3g}"


EDGES = [(t, b, l, r) for t in (0, 1) for b in (0, 1) for l in (0, 1) for r in (0, 1)]


@pytest.mark.parametrize("edges", EDGES, ids=lambda e: "".join(map(str, e)))
def test_patch_blend_edges(edges):
    """ph = 12, pw = 10, ov = 3: every combination of feathered sides, B = 3
    images whose predictions sit at a stride larger than the patch."""
    B, ph, pw, ov, H, W, sh, sw = 3, 12, 10, 3, 17, 15, 2, 4
    g, out0, ws0 = _blend_setup(B, H, W, 43)
    stride = ph * pw + 7
    pred_buf = torch.randn(B, stride, generator=g)
    pred = pred_buf[:, :ph * pw].reshape(B, ph, pw)
    ramp = _ramp(ov)
    w = R.blend_weight_ref(ph, pw, ov, ramp, *edges)
    out_ref, ws_ref = out0.clone(), ws0.clone()
    slack = R.patch_blend_ref(out_ref, ws_ref, pred, w, sh, sw)
    out, go = _put(out0)
    wsum, gw = _put(ws0)
    pd, gp = _put(pred_buf)
    rd, gr = _put(ramp)
    _blend_call(pd, stride, B, ph, pw, out, wsum, H, W, sh, sw, rd, ov, edges)
    _check_blend(out, wsum, out_ref, ws_ref, slack, (go, gw, gp, gr), f"edges {edges}")
    # the weights themselves: 1 in the interior, the ramp's end values at the feathered borders
    dw = (wsum.cpu() - ws0)[0, sh:sh + ph, sw:sw + pw]
    assert abs(float(dw[ph // 2, pw // 2]) - 1.0) <= 2 * R.U32
    if edges[0]:
        assert _same_bits((ws0[0, sh, sw + 5] + w[0, 5]).reshape(1), wsum.cpu()[0, sh, sw + 5].reshape(1))
        assert float(w[0, 5]) == 0.0 and float(w[1, 5]) == 0.5


@pytest.mark.parametrize("case", [
    # (B, ph, pw, ov, H, W, sh, sw, edges)
    (1, 6, 10, 3, 9, 12, 1, 1, (1, 1, 1, 1)),      # ph = 2 ov: rows unfeathered, columns feathered
    (1, 12, 6, 3, 14, 9, 1, 2, (1, 1, 1, 1)),      # the same on the other axis
    (3, 7, 7, 3, 9, 9, 0, 0, (1, 1, 1, 1)),        # L = 2 ov + 1: feathered, one untouched middle entry
    (1, 5, 4, 0, 6, 6, 1, 1, (1, 1, 1, 1)),        # ov = 0
    (3, 12, 10, 3, 20, 21, 8, 11, (1, 0, 1, 0)),   # flush with the bottom-right corner
    (1, 1, 1, 0, 1, 1, 0, 0, (0, 0, 0, 0)),
], ids=lambda c: "x".join(map(str, c[:8])))
def test_patch_blend_shapes(case):
    B, ph, pw, ov, H, W, sh, sw, edges = case
    g, out0, ws0 = _blend_setup(B, H, W, 44)
    pred = torch.randn(B, ph, pw, generator=g)
    ramp = _ramp(ov)
    w = R.blend_weight_ref(ph, pw, ov, ramp, *edges)
    if ph <= 2 * ov:
        assert torch.equal(w, w[:1].expand(ph, pw))          # constant along the short axis
        assert pw <= 2 * ov or float(w[0, 0]) == 0.0
    if ov == 0:
        assert bool((w == 1).all())
    out_ref, ws_ref = out0.clone(), ws0.clone()
    slack = R.patch_blend_ref(out_ref, ws_ref, pred, w, sh, sw)
    out, go = _put(out0)
    wsum, gw = _put(ws0)
    pd, gp = _put(pred)
    rd, gr = _put(ramp)
    _blend_call(pd, ph * pw, B, ph, pw, out, wsum, H, W, sh, sw, rd, ov, edges)
    _check_blend(out, wsum, out_ref, ws_ref, slack, (go, gw, gp, gr), f"case {case}")


def test_patch_blend_overlap_and_finish():
    """two overlapping patches accumulate into the same out / wsum (from zero,
    as the sampler starts), then vu_blend_finish divides in place"""
    B, ph, pw, ov, H, W = 3, 12, 10, 3, 12, 17
    g = torch.Generator().manual_seed(45)
    zero = torch.zeros(B, H, W)
    out, go = _put(zero)
    wsum, gw = _put(zero)
    rd, gr = _put(_ramp(ov))
    out_ref, ws_ref = zero.clone(), zero.clone()
    for sw, edges in ((0, (0, 0, 0, 1)), (7, (0, 0, 1, 0))):
        pred = torch.randn(B, ph, pw, generator=g)
        pd, gp = _put(pred)
        w = R.blend_weight_ref(ph, pw, ov, _ramp(ov), *edges)
        out_ref = out.cpu().clone()   # each call from the bytes the previous one stored
        slack = R.patch_blend_ref(out_ref, ws_ref, pred, w, 0, sw)
        _blend_call(pd, ph * pw, B, ph, pw, out, wsum, H, W, 0, sw, rd, ov, edges)
        _check_blend(out, wsum, out_ref, ws_ref, slack, (go, gw, gp, gr), f"overlap sw={sw}")
    assert float(ws_ref[0, 0, 8]) > 0 and float(ws_ref.min()) >= 0
    # finish: bitwise out / (wsum + 1e-8f) of the device's own operands
    oc, wc = out.cpu().clone(), wsum.cpu().clone()
    _call("vu_blend_finish", _ptr(out), _ptr(wsum), B * H * W)
    go.check("finish out")
    gw.check("finish wsum")
    assert _same_bits(wsum, wc)
    assert _same_bits(out, oc / (wc + torch.tensor(1e-8, dtype=F32)))


@pytest.mark.parametrize("n", N_LIST)
def test_blend_finish(n):
    g = torch.Generator().manual_seed(46 + n)
    o = torch.randn(n, generator=g)
    w = torch.rand(n, generator=g)
    w[0] = 0.0                      # an uncovered pixel: 0 / 1e-8
    o[0] = 0.0 if n > 1 else 3.0
    out, go = _put(o)
    wsum, gw = _put(w)
    _call("vu_blend_finish", _ptr(out), _ptr(wsum), n)
    go.check("finish out")
    gw.check("finish wsum")
    assert _same_bits(out, o / (w + torch.tensor(1e-8, dtype=F32)))
    assert torch.equal(wsum.cpu(), w)


@pytest.mark.parametrize("sh,sw", [(-1, 0), (0, -1), (6, 0), (0, 6), (5, 5)])
def test_patch_blend_refusals(sh, sw):
    """a window outside the image is hipErrorInvalidValue and writes nothing
    (the last case is the largest offset that still fits: accepted)"""
    B, ph, pw, H, W = 1, 12, 10, 17, 15
    out, go = R.guarded((B, H, W), F32, DEV)
    wsum, gw = R.guarded((B, H, W), F32, DEV)
    pd, gp = _put(torch.ones(B, ph, pw))
    rd, gr = _put(_ramp(3))
    L = _lib()
    rc = L.query("vu_patch_blend", _ptr(pd), ph * pw, B, ph, pw, _ptr(out), _ptr(wsum), H, W, sh, sw, _ptr(rd), 3, 0, 0,
                 0, 0, L.stream())
    torch.cuda.synchronize()
    for gd in (go, gw, gp, gr):
        gd.check("refusal")
    if (sh, sw) == (5, 5):
        assert rc == 0
        assert int((wsum != R.SENTINEL).sum()) == ph * pw
        return
    assert rc == INVALID
    assert bool((out == R.SENTINEL).all()) and bool((wsum == R.SENTINEL).all())


# ----------------------------------------------------------------------------
# vu_uncertainty
# ----------------------------------------------------------------------------
UNC_KEYS = ("mean", "std", "entropy", "mi", "cv")


@pytest.mark.parametrize("n", [1, 257, 4099])
@pytest.mark.parametrize("S", [1, 2, 8])
def test_uncertainty(S, n):
    g = torch.Generator().manual_seed(47 + S)
    seg = torch.rand(S, n, generator=g)
    special = [0.0, 1.0, 1e-7, 1 - 1e-7, 0.5]
    for i, v in enumerate(special):
        if 2 * i + 1 < n:
            seg[:, 2 * i] = v                       # every sample the same value
            seg[0, 2 * i + 1] = v                   # one sample only
    if n == 1:
        seg[:, 0] = torch.tensor(special + [0.25, 0.75, 0.9])[:S]
    sd, gs = _put(seg)
    outs = [R.guarded(n, F32, DEV) for _ in UNC_KEYS]
    _call("vu_uncertainty", _ptr(sd), S, n, *[_ptr(o) for o, _ in outs])
    gs.check("uncertainty seg")
    assert torch.equal(sd.cpu(), seg)
    ref64, mag = R.uncertainty_ref(seg)
    ref32, _ = R.uncertainty_ref(seg, F32)
    for key, (o, gd) in zip(UNC_KEYS, outs):
        gd.check(f"uncertainty {key}")
        oc = o.cpu()
        if S == 1 and key in ("std", "cv"):
            assert bool(torch.isnan(oc).all())
            continue
        assert bool(torch.isfinite(oc).all()), key
        planted = torch.arange(n) < 2 * len(special)
        R.assert_trans(oc, ref64[key], ref32[key], mag[key], f"uncertainty S={S} n={n} {key}", split=planted)
    if S > 1 and n > 10:
        # identical samples: no spread; a lone 1 among randoms: a real one (unbiased: S - 1)
        assert float(outs[1][0][8]) == 0.0
        k = 3
        want = float(seg[:, k].double().std(unbiased=True))
        assert abs(float(outs[1][0][k]) - want) <= 1e-5 * want


# ----------------------------------------------------------------------------
# vu_gather_affine
# ----------------------------------------------------------------------------
def _gather(x, flags, dtype):
    """x [B, C, H, W] CPU (values exact in dtype) -> device result [B, Ho, Wo, C], guards"""
    B, C, H, W = x.shape
    maps = [R.flip_rot_map(H, W, *f) for f in flags]
    Ho, Wo = maps[0][1], maps[0][2]
    assert all((m[1], m[2]) == (Ho, Wo) for m in maps)
    m = torch.tensor([mm[0] for mm in maps], dtype=torch.int32)
    md, gm = R.guarded((B, 6), torch.int32, DEV)
    md.copy_(m)
    xd, gx = R.guarded((B, H, W, C), dtype, DEV)
    xd.copy_(x.permute(0, 2, 3, 1).to(dtype))
    y, gy = R.guarded((B, Ho, Wo, C), dtype, DEV)
    code = _lib().BF16 if dtype == torch.bfloat16 else _lib().F32
    _call("vu_gather_affine", _ptr(xd), B, H, W, C, _ptr(md), _ptr(y), Ho, Wo, code)
    for gd, what in ((gm, "map"), (gx, "x"), (gy, "y")):
        gd.check(f"gather {what}")
    assert torch.equal(md.cpu(), m) and torch.equal(xd.cpu().float(), x.permute(0, 2, 3, 1))
    return y


def test_flip_rot_map_is_the_data_loaders():
    from vaeunet_amd.data import _flip_rot_map
    for f in R.FLIP_ROT:
        assert R.flip_rot_map(16, 16, *f)[0] == _flip_rot_map(16, *f)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 3, 8, 24])
@pytest.mark.parametrize("HW", [(16, 16), (5, 9)], ids=["16x16", "5x9"])
def test_gather_affine(HW, C, dtype):
    """every flip / rot90 combination, a different one per sample (B = 5) and
    alone (B = 1); at 5 x 9 the odd rotations give a 9 x 5 output, so the
    combinations are taken per parity of k"""
    H, W = HW
    g = torch.Generator().manual_seed(48)
    x5 = torch.randint(-120, 120, (5, C, H, W), generator=g).float()    # exact in bf16, all distinct enough
    x5 += torch.arange(H * W).view(1, 1, H, W).float() % 7 * 0.5
    x5 = x5.to(dtype).float()
    groups = [R.FLIP_ROT] if H == W else [[f for f in R.FLIP_ROT if f[2] % 2 == p] for p in (0, 1)]
    for flags_all in groups:
        for lo in range(0, len(flags_all), 5):
            flags = (flags_all + flags_all)[lo:lo + 5]
            y = _gather(x5, flags, dtype)
            for b, f in enumerate(flags):
                want = R.flip_rot_ref(x5[b], *f).permute(1, 2, 0)
                assert torch.equal(y[b].cpu().float(), want), (b, f)
        for f in flags_all:
            y = _gather(x5[2:3], [f], dtype)
            assert torch.equal(y[0].cpu().float(), R.flip_rot_ref(x5[2], *f).permute(1, 2, 0)), f
