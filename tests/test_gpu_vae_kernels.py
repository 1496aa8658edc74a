"""The VAE-U-Net glue kernels of csrc/vae.hip, each called through the C ABI
and compared with a plain fp64 CPU reference (tests/ref_small.py) at the
shapes where they can go wrong: ties, padding, odd sizes, empty splits, tails,
channel slices of a wider tensor, accumulation.  Every output lives in a
guarded buffer (sentinel before, behind and in the neighbouring channels)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import ref_small as R
from test_gpu_kernels import C_SUM, DEV, _code, _dt

pytestmark = pytest.mark.gpu

MODES = ["f32", "bf16"]
U32 = 2.0 ** -24


def _lib():
    from vaeunet_amd import _lib as L
    return L


def _call(name, *args):
    L = _lib()
    L.call(name, *args, L.stream())
    torch.cuda.synchronize()


def _ptr(t):
    return _lib().ptr(t)


def _put_act(x, mode, strided, c0=None):
    """CPU [N, C, H, W] -> device NHWC in the storage dtype, dense or as the
    channel slice [C, 2C) of a tensor twice as wide (pixel stride 2C)."""
    N, C, H, W = x.shape
    t, g = R.guarded_act(N, C, H, W, _dt(mode), DEV, wide=2 * C if strided else None,
                         c0=(C if c0 is None else c0) if strided else 0)
    t.copy_(x.to(_dt(mode)))
    return t, g


def _put_rows(x, mode, strided):
    """CPU [P, C] -> device pixel-major rows (stride C or 2C)."""
    P, C = x.shape
    t, g = R.guarded_rows(P, C, _dt(mode), DEV, wide=2 * C if strided else None, c0=C if strided else 0)
    t.copy_(x.to(_dt(mode)))
    return t, g


def _f32(x, offset=0):
    """CPU tensor -> guarded contiguous fp32 device tensor."""
    t, g = R.guarded(x.shape, torch.float32, DEV, offset=offset)
    t.copy_(x)
    return t, g


# ----------------------------------------------------------------------------
# max pool 3x3 / s2 / p1
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool_case(shape, negative):
    x = R.pool_input(shape, negative=negative)
    y, code = R.pool3_ref(x)
    g = torch.Generator().manual_seed(5)
    dy = torch.randint(-4, 5, y.shape, generator=g).float()
    pre = torch.randint(-4, 5, shape, generator=g).float()
    xr = x.double().requires_grad_(True)
    F.max_pool2d(xr, 3, 2, 1).backward(dy.double())
    return x, y, code, dy, pre, xr.grad


POOL_CASES = [(s, False) for s in R.POOL_SHAPES] + [(R.POOL_SHAPES[0], True)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "x".join(map(str, c[0])) + ("-neg" if c[1] else ""))
def test_maxpool3s2_fwd_bwd(case, strided, mode):
    """vu_maxpool3s2_fwd / _bwd vs F.max_pool2d(x, 3, 2, 1, return_indices)
    and autograd: integer inputs (ties everywhere: the first maximum in
    row-major window order wins), integer dy and pre-fill, so every value is
    exact in both dtypes and the comparison is torch.equal."""
    shape, negative = case
    N, C, H, W = shape
    x, y, code, dy, pre, dx_ref = _pool_case(shape, negative)
    Ho, Wo = y.shape[2], y.shape[3]
    d = _code(mode)
    xd, gx = _put_act(x, mode, strided)
    yd, gy = R.guarded_act(N, C, Ho, Wo, _dt(mode), DEV, wide=2 * C if strided else None, c0=0)
    idx, gi = R.guarded((N, Ho, Wo, C), torch.uint8, DEV)
    s = 2 * C if strided else C
    _call("vu_maxpool3s2_fwd", _ptr(xd), s, N, H, W, C, _ptr(yd), s, _ptr(idx), d)
    for g_, what in ((gx, "x"), (gy, "y"), (gi, "idx")):
        g_.check(f"pool fwd {what}")
    assert torch.equal(yd.double().cpu(), y)
    if negative:
        assert float(yd.float().max()) < 0
    assert torch.equal(idx.cpu().permute(0, 3, 1, 2), code)
    dyd, gdy = _put_act(dy, mode, strided, c0=0)
    for acc in (0, 1):
        dxd, gdx = _put_act(pre, mode, strided)
        _call("vu_maxpool3s2_bwd", _ptr(dyd), s, _ptr(idx), N, H, W, C, _ptr(dxd), s, acc, d)
        gdx.check(f"pool bwd dx acc={acc}")
        gdy.check("pool bwd dy")
        gi.check("pool bwd idx")
        want = dx_ref + pre.double() if acc else dx_ref
        assert torch.equal(dxd.double().cpu(), want), f"acc={acc}"


# ----------------------------------------------------------------------------
# ReLU mask
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("P", [1, 37, 1000])
@pytest.mark.parametrize("C", [8, 24, 64])
def test_relu_mask(C, P, strided, mode):
    """g = where(out > 0, dout, 0), bit for bit; out holds +0.0, -0.0, the
    smallest positive bf16 (a subnormal) and the smallest normal."""
    g = torch.Generator().manual_seed(12)
    out = torch.randn(P, C, generator=g)
    dout = torch.randn(P, C, generator=g)
    special = torch.tensor([0.0, -0.0, R.BF16_TINY, 2.0 ** -126, -R.BF16_TINY])
    pos = torch.randperm(P * C, generator=g)[:min(P * C, 5 * 8)]
    out.view(-1)[pos] = special.repeat(8)[:pos.numel()]
    dt = _dt(mode)
    out, dout = out.to(dt), dout.to(dt)
    assert float(out.float().abs()[out.float() != 0].min()) == R.BF16_TINY
    od, go = _put_rows(out, mode, strided)
    dd, gd = _put_rows(dout, mode, strided)
    gg, ggd = R.guarded_rows(P, C, dt, DEV, wide=2 * C if strided else None, c0=0)
    s = 2 * C if strided else C
    _call("vu_relu_mask", _ptr(dd), s, _ptr(od), s, P, C, _ptr(gg), s, _code(mode))
    for g_ in (go, gd, ggd):
        g_.check("relu mask")
    want = torch.where(out > 0, dout, torch.zeros_like(dout))
    assert torch.equal(gg.cpu(), want)


# ----------------------------------------------------------------------------
# per-sample sums and broadcasts
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("HW", [1, 5, 63, 64, 65, 1000])
@pytest.mark.parametrize("C", [8, 64, 2048])
def test_sample_sum(C, HW, strided, mode):
    """out[n][c] (+)= scale * sum_p x[n, p, c] vs fp64, per element within
    2^-24 |ref| (the fp32 store) + C_SUM |scale| sum |x| (summation order)
    [+ 2^-24 |pre-fill|]; the kernel cuts a sample into 64 splits whatever HW
    (empty splits, one pixel per split, a partial last split)."""
    L = _lib()
    g = torch.Generator().manual_seed(13)
    x3 = torch.randn(3, HW, C, generator=g).to(_dt(mode)).float()
    pre3 = torch.randn(3, C, generator=g)
    s = 2 * C if strided else C
    for N in (1, 3):
        x, pre = x3[:N], pre3[:N]
        xd, gx = _put_rows(x.reshape(N * HW, C), mode, strided)
        ws, gw = R.guarded(L.query("vu_sample_sum_workspace_bytes", N, C) // 4, torch.float32, DEV)
        for scale in (1.0, 1.0 / HW):
            sc32 = float(torch.tensor(scale, dtype=torch.float32))   # the value the kernel is handed
            ref, sabs = R.sample_sum_ref(x, sc32)
            got = []
            for acc in (0, 1, 0):
                out, gout = _f32(pre)
                _call("vu_sample_sum", _ptr(xd), s, N, HW, C, scale, _ptr(out), acc, _ptr(ws), _code(mode))
                for g_ in (gx, gw, gout):
                    g_.check(f"sample_sum N={N} scale={scale} acc={acc}")
                want = ref + pre.double() if acc else ref
                bound = U32 * want.abs() + C_SUM * sabs + (U32 * pre.double().abs() if acc else 0)
                err = (out.double().cpu() - want).abs()
                assert (err <= bound).all(), (N, scale, acc, float((err / bound).max()))
                got.append(out.cpu())
            assert torch.equal(got[0], got[2]), "two launches differ (the order is fixed)"


@pytest.mark.parametrize("bad", ["C24", "odd_stride"])
def test_sample_sum_refuses(bad):
    """C / 8 not a power of two and a pixel stride that is no multiple of 8
    are refused with an error, and nothing is written."""
    C, xs = (24, 24) if bad == "C24" else (8, 9)
    N, HW = 2, 5
    x, gx = R.guarded(N * HW * xs, torch.float32, DEV)
    out, go = R.guarded((N, C), torch.float32, DEV)
    ws, gw = R.guarded(N * 64 * C, torch.float32, DEV)
    with pytest.raises(RuntimeError):
        _call("vu_sample_sum", _ptr(x), xs, N, HW, C, 1.0, _ptr(out), 0, _ptr(ws), 0)
    torch.cuda.synchronize()
    for t, g_ in ((out, go), (ws, gw)):
        g_.check(bad)
        assert (t == R.SENTINEL).all()


def _ulp(ref, mode):
    """Spacing of the storage dtype at |ref| (fp64 tensor)."""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -120)))
    return torch.pow(2.0, e - (23 if mode == "f32" else 7))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("HW", [1, 49])
@pytest.mark.parametrize("C", [5, 8, 512])
def test_sample_broadcast(C, HW, strided, mode):
    """y[n, p, c] (+)= scale * v[n][c].  Overwrite: one fp32 multiply and one
    storage rounding, bit for bit.  Accumulate: equality for scale 1, else
    within one ulp of the storage dtype of the fp64 value (the multiply-add
    may contract); there v and the pre-fill are positive, so no cancellation
    makes the product's own rounding exceed the result's ulp."""
    g = torch.Generator().manual_seed(14)
    N, H = 2, int(HW ** 0.5)
    dt = _dt(mode)
    v = torch.randn(N, C, generator=g)
    pre = torch.randn(N, C, H, H, generator=g).to(dt)
    vd, gv = _f32(v)
    s = 2 * C if strided else C
    for scale in (1.0, 1.0 / 49):
        sc32 = torch.tensor(scale, dtype=torch.float32)
        for acc in (0, 1):
            vv, pp = v, pre
            if acc and scale != 1.0:
                vv, pp = v.abs() + 0.5, (pre.float().abs() + 0.5).to(dt)
            vd.copy_(vv)
            y, gy = _put_act(pp.float(), mode, strided)
            _call("vu_sample_broadcast", _ptr(vd), N, HW, C, scale, _ptr(y), s, acc, _code(mode))
            gy.check(f"broadcast scale={scale} acc={acc}")
            gv.check("broadcast v")
            got = y.cpu()
            val = (vv * sc32)[:, :, None, None].expand(N, C, H, H)
            if not acc:
                assert torch.equal(got, val.to(dt)), (scale, acc)
            elif scale == 1.0:
                assert torch.equal(got, (pp.float() + val).to(dt)), (scale, acc)
            else:
                ref = pp.double() + float(sc32) * vv.double()[:, :, None, None]
                err = (got.double() - ref).abs()
                assert (err <= _ulp(ref, mode)).all(), float((err / _ulp(ref, mode)).max())


def test_sample_broadcast_flat_accumulate():
    """The degenerate call of the VAE backward: N = 1, HW = 1, C = N * L, fp32,
    accumulate -- dz += dzi as one flat vector."""
    g = torch.Generator().manual_seed(15)
    n = 3 * 32
    v, pre = torch.randn(n, generator=g), torch.randn(n, generator=g)
    vd, gv = _f32(v)
    y, gy = _f32(pre)
    _call("vu_sample_broadcast", _ptr(vd), 1, 1, n, 1.0, _ptr(y), n, 1, 0)
    gv.check("v")
    gy.check("y")
    assert torch.equal(y.cpu(), pre + v)


# ----------------------------------------------------------------------------
# the tiny linear map of the mu / logvar heads
# ----------------------------------------------------------------------------
def _linear_inputs(B, K, J):
    g = torch.Generator().manual_seed(16)
    return (torch.randn(B, K, generator=g), torch.randn(J, K, generator=g) / K ** 0.5,
            torch.randn(J, generator=g), torch.randn(B, J, generator=g))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("case", R.LINEAR_FWD_CASES)
def test_linear_small_fwd(case, bias):
    """fp64 accumulation in the kernel: |got - ref64| <= 2^-23 |ref64| +
    1e-12 (|bias| + sum |x||w|)."""
    B, K, J = case
    x, w, b, _ = _linear_inputs(B, K, J)
    ref, sabs = R.linear_fwd_ref(x, w, b if bias else None)
    (xd, gx), (wd, gw), (bd, gb) = _f32(x), _f32(w), _f32(b)
    y, gy = R.guarded((B, J), torch.float32, DEV)
    _call("vu_linear_small_fwd", _ptr(xd), B, K, _ptr(wd), _ptr(bd) if bias else None, J, _ptr(y))
    for g_ in (gx, gw, gb, gy):
        g_.check("linear fwd")
    err = (y.double().cpu() - ref).abs()
    bound = 2.0 ** -23 * ref.abs() + 1e-12 * sabs
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("w_acc", [0, 1])
@pytest.mark.parametrize("dx_acc", [0, 1])
@pytest.mark.parametrize("case", R.LINEAR_BWD_CASES)
def test_linear_small_bwd(case, dx_acc, w_acc):
    """dx, dw, db vs fp64: fp32 sums of <= 64 terms, per element within
    2^-24 |ref| + C_SUM sabs; every accumulate combination; and with dx or
    (dw, db) absent the others are still right and nothing else is written."""
    B, K, J = case
    x, w, _, dy = _linear_inputs(B, K, J)
    g = torch.Generator().manual_seed(17)
    pre = [torch.randn(s, generator=g) for s in ((B, K), (J, K), (J,))]
    refs, sabs = R.linear_bwd_ref(x, w, dy)
    accs = (dx_acc, w_acc, w_acc)
    (xd, gx), (wd, gw), (dyd, gdy) = _f32(x), _f32(w), _f32(dy)
    for present in ((1, 1, 1), (0, 1, 1), (1, 0, 0)):
        outs = [_f32(p) for p in pre]
        ptrs = [_ptr(o[0]) if on else None for o, on in zip(outs, present)]
        _call("vu_linear_small_bwd", _ptr(xd), B, K, _ptr(wd), J, _ptr(dyd), ptrs[0], dx_acc, ptrs[1], ptrs[2],
              w_acc)
        for g_ in (gx, gw, gdy):
            g_.check("linear bwd inputs")
        for name, (o, go), on, ref, sa, p, acc in zip(("dx", "dw", "db"), outs, present, refs, sabs, pre, accs):
            go.check(f"linear bwd {name} {present}")
            if not on:
                assert torch.equal(o.cpu(), p), f"{name} written though absent"
                continue
            want = ref + p.double() if acc else ref
            err = (o.double().cpu() - want).abs()
            bound = U32 * want.abs() + C_SUM * sa + (U32 * p.double().abs() if acc else 0)
            assert (err <= bound).all(), (name, present, float((err / bound).max()))


# ----------------------------------------------------------------------------
# reparameterisation
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.REPARAM_N)
def test_reparam_fwd_bwd(n):
    """z = mu + eps exp(lv / 2) and its backward vs fp64, lv in [-6, 6]:
    |z - ref| <= 1e-6 (|mu| + |eps| exp(lv / 2)) -- one expf at about an ulp
    and three more fp32 roundings are under 4 * 2^-24, the 1e-6 leaves a
    factor of 4 -- and the same form for dlv; dmu is dz (or fl32(pre + dz))
    bit for bit.  eps = NULL: z is mu bitwise, dlv zero or left unchanged."""
    g = torch.Generator().manual_seed(18)
    mu = torch.randn(n, generator=g)
    lv = torch.rand(n, generator=g) * 12 - 6
    lv[0], lv[-1] = -6.0, 6.0
    eps = torch.randn(n, generator=g)
    dz = torch.randn(n, generator=g)
    pre_mu, pre_lv = torch.randn(n, generator=g), torch.randn(n, generator=g)
    (mud, g1), (lvd, g2), (epd, g3), (dzd, g4) = _f32(mu), _f32(lv), _f32(eps), _f32(dz)
    ins = (g1, g2, g3, g4)
    for with_eps in (True, False):
        z, gz = R.guarded(n, torch.float32, DEV)
        _call("vu_reparam_fwd", _ptr(mud), _ptr(lvd), _ptr(epd) if with_eps else None, n, _ptr(z))
        for g_ in ins + (gz,):
            g_.check("reparam fwd")
        ref, mag = R.reparam_fwd_ref(mu, lv, eps if with_eps else None)
        if with_eps:
            err = (z.double().cpu() - ref).abs()
            assert (err <= 1e-6 * mag).all(), float((err / mag).max())
        else:
            assert torch.equal(z.cpu(), mu)
        rmu, rlv = R.reparam_bwd_ref(lv, eps if with_eps else None, dz)
        for acc in (0, 1):
            (dmu, gm), (dlv, gl) = _f32(pre_mu), _f32(pre_lv)
            _call("vu_reparam_bwd", _ptr(lvd), _ptr(epd) if with_eps else None, _ptr(dzd), n, _ptr(dmu), _ptr(dlv),
                  acc)
            for g_ in ins + (gm, gl):
                g_.check("reparam bwd")
            assert torch.equal(dmu.cpu(), pre_mu + dz if acc else dz), (with_eps, acc)
            if not with_eps:
                assert torch.equal(dlv.cpu(), pre_lv if acc else torch.zeros(n)), acc
                continue
            want = rlv + pre_lv.double() if acc else rlv
            err = (dlv.double().cpu() - want).abs()
            bound = 1e-6 * (rlv.abs() + (pre_lv.double().abs() if acc else 0))
            assert (err <= bound).all(), (acc, float((err / bound).max()))
