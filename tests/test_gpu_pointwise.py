"""The OutConv family of csrc/attention.hip (vu_pointwise_fwd / _bwd and the
variants over an on-the-fly BatchNorm + ReLU, vu_pointwise_bn_fwd / _bn_bwd)
called through the C ABI as engine.outconv_* does -- x / dx in the storage
dtype, y / dy fp32 -- against fp64 CPU references (tests/ref_small.py): narrow
and wide channel counts, the C > 512 loop path, pixel counts below, at and
past the 256-pixel tile, the grid cap (a block walking several tiles), column
slices, accumulation, and the per-block BatchNorm-backward partials."""
import functools

import pytest
import torch

import ref_small as R
from test_gpu_kernels import C_SUM, DEV, U_STORE, _code, _dt

pytestmark = pytest.mark.gpu

MODES = ["f32", "bf16"]
U32 = 2.0 ** -24
BIG = R.PW_BWD_CASES[-1]
BWD_CASES = [(c, m) for c in R.PW_BWD_CASES for m in MODES if not (c == BIG and m == "f32")]
_ids = lambda c: f"P{c[0][0]}-C{c[0][1]}-J{c[0][2]}-{c[1]}"  # noqa: E731


def _lib():
    from vaeunet_amd import _lib as L
    return L


def _call(name, *args):
    L = _lib()
    L.call(name, *args, L.stream())
    torch.cuda.synchronize()


def _ptr(t):
    return _lib().ptr(t)


def _f32(x):
    t, g = R.guarded(x.shape, torch.float32, DEV)
    t.copy_(x)
    return t, g


def _rows(x, dtype, wide=None, c0=0):
    t, g = R.guarded_rows(x.shape[0], x.shape[1], dtype, DEV, wide=wide, c0=c0)
    t.copy_(x.to(dtype))
    return t, g


def _bounded(got, ref, bound, what):
    err = (got.detach().double().cpu() - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.where(bad, err - bound, torch.full_like(err, -1.0)).flatten().argmax())
        raise AssertionError(f"{what}: bound exceeded at flat index {i}: got {got.flatten()[i].item():.7g}, "
                             f"ref {ref.flatten()[i].item():.7g}, bound {bound.flatten()[i].item():.3e}; "
                             f"{int(bad.sum())} of {bad.numel()} off")


def _fwd_check(y, x, w, b, what):
    """the bound of test_outconv_pointwise_fwd: 1e-5 (sum |x||w| + |b|) + 1e-6"""
    ref, mag = R.pointwise_fwd_ref(x, w, b)
    _bounded(y, ref, 1e-5 * mag + 1e-6, what)


@functools.lru_cache(maxsize=None)
def _inputs(P, C, J, mode):
    return R.pw_bn_inputs(P, C, J, _dt(mode))


# ----------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------
FWD_CASES = [
    # (C, J, P)
    (8, 2, 3),       # 64 pixels per wave, P below one wave's 256-pixel batch
    (16, 4, 1),      # narrow lane group
    (512, 3, 300),   # 64 lanes per pixel, the widest register path
    (1024, 1, 77),   # C > 512: the loop path
    (1024, 3, 77),
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: f"C{c[0]}-J{c[1]}-P{c[2]}")
def test_pointwise_fwd_edges(case, mode):
    C, J, P = case
    x, w, b, _ = R.pw_inputs(P, C, J, _dt(mode))
    (xd, gx), (wd, gw), (bd, gb) = _rows(x, _dt(mode)), _f32(w), _f32(b)
    y, gy = R.guarded((P, J), torch.float32, DEV)
    _call("vu_pointwise_fwd", _ptr(xd), C, P, C, J, _ptr(wd), _ptr(bd), _ptr(y), J, _code(mode))
    for g_ in (gx, gw, gb, gy):
        g_.check("pointwise fwd")
    _fwd_check(y, x, w, b, f"pointwise fwd {case}")


@pytest.mark.parametrize("mode", MODES)
def test_pointwise_fwd_column_slice(mode):
    """ys = 4, J = 2: y is columns [1, 3) of a 4-column map; columns 0 and 3
    stay untouched."""
    P, C, J = 77, 64, 2
    x, w, b, _ = R.pw_inputs(P, C, J, _dt(mode))
    (xd, gx), (wd, gw), (bd, gb) = _rows(x, _dt(mode)), _f32(w), _f32(b)
    y, gy = R.guarded_rows(P, J, torch.float32, DEV, wide=4, c0=1)
    _call("vu_pointwise_fwd", _ptr(xd), C, P, C, J, _ptr(wd), _ptr(bd), _ptr(y), 4, _code(mode))
    for g_ in (gx, gw, gb, gy):
        g_.check("pointwise fwd slice")
    _fwd_check(y, x, w, b, "pointwise fwd ys=4")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.PW_BN_FWD_CASES, ids=lambda c: f"P{c[0]}-C{c[1]}-J{c[2]}")
def test_pointwise_bn_fwd(case, mode):
    """(a) bit-identical to vu_bn_apply (relu) into a temporary followed by
    vu_pointwise_fwd -- the operand is "the bytes vu_bn_apply would store";
    (b) that unfused result within the forward bound of the fp64 reference
    computed from the temporary.  scale has both signs and every fourth
    channel is all-zero after the ReLU."""
    P, C, J = case
    dt, d = _dt(mode), _code(mode)
    x, w, b, _, (scale, shift, _, _, _) = _inputs(P, C, J, mode)
    (xd, gx), (wd, gw), (bd, gb) = _rows(x, dt), _f32(w), _f32(b)
    (sc, gs), (sh, gh) = _f32(scale), _f32(shift)
    a, ga = R.guarded_rows(P, C, dt, DEV)
    _call("vu_bn_apply", _ptr(xd), C, _ptr(a), C, P, C, _ptr(sc), _ptr(sh), 1, d)
    y0, g0 = R.guarded((P, J), torch.float32, DEV)
    _call("vu_pointwise_fwd", _ptr(a), C, P, C, J, _ptr(wd), _ptr(bd), _ptr(y0), J, d)
    y1, g1 = R.guarded((P, J), torch.float32, DEV)
    _call("vu_pointwise_bn_fwd", _ptr(xd), C, P, C, J, _ptr(sc), _ptr(sh), _ptr(wd), _ptr(bd), _ptr(y1), J, d)
    for g_ in (gx, gw, gb, gs, gh, ga, g0, g1):
        g_.check("pointwise bn fwd")
    acpu = a.float().cpu()
    assert (acpu[:, 3::4] == 0).all() and (acpu >= 0).all()
    assert torch.equal(y1, y0), f"fused != bn_apply + pointwise_fwd: max diff {float((y1 - y0).abs().max()):.3e}"
    _fwd_check(y0, acpu, w, b, f"bn_apply + pointwise fwd {case}")


# ----------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------
def _pre(C, J):
    g = torch.Generator().manual_seed(23)
    return torch.randn(J, C, generator=g), torch.randn(J, generator=g)


def _run_bwd(mode, x_dev, dy_dev, dys, P, C, J, w_dev, acc, pre, bn=None):
    """One launch of vu_pointwise_bwd (bn None) or vu_pointwise_bn_bwd (bn =
    the [4, C] coefficient tensor) into fresh guarded outputs."""
    L = _lib()
    dt = _dt(mode)
    dx, gdx = R.guarded_rows(P, C, dt, DEV)
    (dw, gdw), (db, gdb) = _f32(pre[0]), _f32(pre[1])
    ws, gws = R.guarded(max(1, L.query("vu_pointwise_bwd_workspace_bytes", P, C, J) // 4), torch.float32, DEV)
    guards = [gdx, gdw, gdb, gws]
    if bn is None:
        _call("vu_pointwise_bwd", _ptr(x_dev), C, _ptr(dy_dev), dys, P, C, J, _ptr(w_dev), _ptr(dx), C, _ptr(dw),
              _ptr(db), acc, _ptr(ws), _code(mode))
        bnb = None
    else:
        nblk = L.query("vu_pointwise_bn_bwd_blocks", P)
        bnb, gb = R.guarded((nblk, 2, C), torch.float32, DEV)
        guards.append(gb)
        _call("vu_pointwise_bn_bwd", _ptr(x_dev), C, _ptr(bn), C, _ptr(dy_dev), dys, P, C, J, _ptr(w_dev),
              _ptr(dx), C, _ptr(dw), _ptr(db), acc, _ptr(ws), _ptr(bnb), _code(mode))
    for g_ in guards:
        g_.check(f"pointwise bwd outputs (bn={bn is not None}, acc={acc})")
    return dx, dw, db, bnb


def _check_bwd(mode, dx, dw, db, a, w, dy, acc, pre, what):
    """dx: U_STORE max(|ref|, |got|) + C_SUM sum_j |dy||w|;  dw, db: 2^-24 |ref|
    + C_SUM sabs (sabs = sum_p |dy||a| resp. sum_p |dy|), ref including the
    pre-fill of an accumulating launch."""
    (rdx, rdw, rdb), (adx, adw, adb) = R.pointwise_bwd_ref(a, w, dy)
    g64 = dx.double().cpu()
    _bounded(dx, rdx, U_STORE[mode] * torch.maximum(rdx.abs(), g64.abs()) + C_SUM * adx, f"{what} dx")
    if acc:
        rdw, rdb = rdw + pre[0].double(), rdb + pre[1].double()
    _bounded(dw, rdw, U32 * rdw.abs() + C_SUM * adw, f"{what} dw")
    _bounded(db, rdb, U32 * rdb.abs() + C_SUM * adb, f"{what} db")


@pytest.mark.parametrize("case", BWD_CASES, ids=_ids)
def test_pointwise_bwd(case):
    """vu_pointwise_bwd vs fp64, overwrite and accumulate onto a random
    pre-fill of dw / db; two launches agree bit for bit (fixed order)."""
    (P, C, J), mode = case
    x, w, _, dy = R.pw_inputs(P, C, J, _dt(mode))
    (xd, gx), (wd, gw), (dyd, gdy) = _rows(x, _dt(mode)), _f32(w), _f32(dy)
    pre = _pre(C, J)
    outs = []
    for acc in (0, 1, 0):
        dx, dw, db, _ = _run_bwd(mode, xd, dyd, J, P, C, J, wd, acc, pre)
        for g_ in (gx, gw, gdy):
            g_.check("pointwise bwd inputs")
        if len(outs) < 2:
            _check_bwd(mode, dx, dw, db, x, w, dy, acc, pre, f"pointwise bwd {case} acc={acc}")
        outs.append((dx, dw, db))
    for a_, b_, n in zip(outs[0], outs[2], ("dx", "dw", "db")):
        assert torch.equal(a_, b_), f"{n}: two launches differ"


@pytest.mark.parametrize("mode", MODES)
def test_pointwise_bwd_dy_column_slice(mode):
    """dys = 4, J = 2: dy is columns [1, 3) of a 4-column map."""
    P, C, J = 257, 64, 2
    x, w, _, dy = R.pw_inputs(P, C, J, _dt(mode))
    (xd, _), (wd, _) = _rows(x, _dt(mode)), _f32(w)
    dyd, _ = _rows(dy, torch.float32, wide=4, c0=1)
    pre = _pre(C, J)
    for acc in (0, 1):
        dx, dw, db, _ = _run_bwd(mode, xd, dyd, 4, P, C, J, wd, acc, pre)
        _check_bwd(mode, dx, dw, db, x, w, dy, acc, pre, f"pointwise bwd dys=4 acc={acc}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [512, 24])
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn"])
def test_pointwise_bwd_refuses_unsupported_width(bn, C, mode):
    """C = 512 (more than 32 lanes per pixel) and C = 24 (C / 8 not a power of
    two) are refused with an error and dx, dw, db stay untouched: a
    stand-alone OutConv(512, n) fails cleanly in backward."""
    P, J = 40, 2
    x, w, _, dy = R.pw_inputs(P, C, J, _dt(mode))
    (xd, _), (wd, _), (dyd, _) = _rows(x, _dt(mode)), _f32(w), _f32(dy)
    coef, _ = _f32(torch.ones(4, C))
    dx, gdx = R.guarded_rows(P, C, _dt(mode), DEV)
    dw, gdw = R.guarded((J, C), torch.float32, DEV)
    db, gdb = R.guarded(J, torch.float32, DEV)
    ws, gws = R.guarded(J * C + J, torch.float32, DEV)
    bnb, gbb = R.guarded((1, 2, C), torch.float32, DEV)
    with pytest.raises(RuntimeError):
        if bn:
            _call("vu_pointwise_bn_bwd", _ptr(xd), C, _ptr(coef), C, _ptr(dyd), J, P, C, J, _ptr(wd), _ptr(dx), C,
                  _ptr(dw), _ptr(db), 0, _ptr(ws), _ptr(bnb), _code(mode))
        else:
            _call("vu_pointwise_bwd", _ptr(xd), C, _ptr(dyd), J, P, C, J, _ptr(wd), _ptr(dx), C, _ptr(dw), _ptr(db),
                  0, _ptr(ws), _code(mode))
    torch.cuda.synchronize()
    for t, g_ in ((dx, gdx), (dw, gdw), (db, gdb), (ws, gws), (bnb, gbb)):
        g_.check("refused launch")
        assert (t.float() == torch.full((), R.SENTINEL, dtype=t.dtype).float()).all()


@pytest.mark.parametrize("case", BWD_CASES, ids=_ids)
def test_pointwise_bn_bwd(case):
    """vu_pointwise_bn_bwd on a conditioned input (no BatchNorm output within
    1e-3 of cancelling, so the ReLU mask does not depend on multiply-add
    contraction; nothing is excluded from any comparison):

    * dx, dw, db bit-identical to vu_pointwise_bwd run on a = vu_bn_apply(x)
      (the same kernel template in the same order), overwrite and accumulate;
    * block b of bnb[nblk][2][C] vs the fp64 sums over exactly the pixels
      {p : (p // 256) % nblk == b} of dz and dz * (x - mean) * invstd, dz =
      the stored dx masked by the ReLU, within 2^-24 |ref| + C_SUM sabs;
    * the partials finished by vu_bn_bwd_finish (train) vs the fp64 formulas
      of vu_bn_bwd_reduce: dbeta / dgamma within test_gpu_bnb.py's 2e-6 of
      the largest channel's sum |dz| resp. sum |dz xhat|; k1 = gamma * invstd
      to one fp32 rounding; k2 = -k1 invstd S1 / P and k3 = -k1 S0 / P within
      that tolerance of S1 / S0 carried through the factor, plus 2^-22 |ref|
      (k1's and the result's fp32 roundings, 2^-23, with a factor of two)."""
    (P, C, J), mode = case
    L = _lib()
    dt, d = _dt(mode), _code(mode)
    x, w, _, dy, (scale, shift, mean, invstd, gamma) = _inputs(P, C, J, mode)
    assert int(R.bn_near_zero(x, scale, shift).sum()) == 0
    (xd, gx), (wd, gw), (dyd, gdy) = _rows(x, dt), _f32(w), _f32(dy)
    coef, gc = _f32(torch.stack([scale, shift, mean, invstd]))
    a, ga = R.guarded_rows(P, C, dt, DEV)
    _call("vu_bn_apply", _ptr(xd), C, _ptr(a), C, P, C, _ptr(coef[0]), _ptr(coef[1]), 1, d)
    ga.check("bn_apply")
    pre = _pre(C, J)
    nblk = L.query("vu_pointwise_bn_bwd_blocks", P)
    assert nblk == min((P + R.TILE - 1) // R.TILE, 1024)
    for acc in (0, 1):
        dx0, dw0, db0, _ = _run_bwd(mode, a, dyd, J, P, C, J, wd, acc, pre)
        dx1, dw1, db1, bnb = _run_bwd(mode, xd, dyd, J, P, C, J, wd, acc, pre, bn=coef)
        for g_ in (gx, gw, gdy, gc, ga):
            g_.check("pointwise bn bwd inputs")
        for u, v, n in ((dx0, dx1, "dx"), (dw0, dw1, "dw"), (db0, db1, "db")):
            assert torch.equal(u, v), f"{n} (acc={acc}) differs from vu_pointwise_bwd on vu_bn_apply(x)"
        _check_bwd(mode, dx1, dw1, db1, a.float().cpu(), w, dy, acc, pre, f"pointwise bn bwd {case} acc={acc}")
        part, sabs = R.bnb_partials_ref(dx1.float().cpu(), x, scale, shift, mean, invstd, nblk)
        _bounded(bnb, part, U32 * part.abs() + C_SUM * sabs, f"bnb partials acc={acc}")
    # the finish over the device's partials
    gam, _ = _f32(gamma)
    dgamma, g1 = R.guarded(C, torch.float32, DEV)
    dbeta, g2 = R.guarded(C, torch.float32, DEV)
    k, g3 = R.guarded((3, C), torch.float32, DEV)
    ws, g4 = R.guarded(max(1, L.query("vu_bn_bwd_finish_workspace_bytes", nblk, C) // 4), torch.float32, DEV)
    _call("vu_bn_bwd_finish", _ptr(bnb), nblk, P, C, _ptr(gam), _ptr(coef[3]), 1, _ptr(dgamma), _ptr(dbeta), 0,
          _ptr(k), _ptr(ws))
    for g_ in (g1, g2, g3, g4):
        g_.check("bn_bwd_finish")
    rdg, rdb, rk = R.bn_bwd_finish_ref(part, gamma, invstd, P)
    t0 = 2e-6 * float(sabs[:, 0].sum(0).max())
    t1 = 2e-6 * float(sabs[:, 1].sum(0).max())
    one = torch.ones(C, dtype=torch.float64)
    _bounded(dbeta, rdb, t0 * one, "dbeta")
    _bounded(dgamma, rdg, t1 * one, "dgamma")
    k1 = rk[0].abs()
    _bounded(k[0], rk[0], U32 * k1, "k1")
    _bounded(k[1], rk[1], k1 * invstd.double() / P * t1 + 2.0 ** -22 * rk[1].abs(), "k2")
    _bounded(k[2], rk[2], k1 / P * t0 + 2.0 ** -22 * rk[2].abs(), "k3")
