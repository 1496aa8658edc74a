"""The boundary metrics (vaeunet_amd/csrc/edt.hip, vaeunet_amd/surface.py,
DESIGN.md §4.12) on the GPU against the numpy restatement in tests/edt_ref.py.
The squared distance transform, the boundary and the eight statistics columns
are integers and are compared EXACTLY; the fp64 sums within the bound of a
length-n summation, 2 n 2^-53 relative; square roots and quotients within one
ulp.

Shapes: 1 x 1, 1 x 70, 70 x 1, 67 x 131, 129 x 257; 3 x {63, 64, 65} (the 64
columns of a column-pass block), {15, 16, 17} x 5 and {31, 32, 33} x 5 (its 16
chunks of rows per column: chunks of one and of two rows, with and without empty
and ragged ones), 3 x {255, 256, 257} and {255, 256, 257} x 3 (the 256 threads
of a row-pass block; chunks of 16 and 17 rows), each -1 / 0 / +1; 2 x 600 (a
row of more than twice the row block's threads).  Planes:
edt_ref.adversarial_planes, all of one shape as one batch.  The kernels run through the C ABI on guarded
buffers: the inputs come back unchanged and no guard element is written."""
import functools
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

import edt_ref as ER
import lesions_ref as LR
import ref_small as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
INVALID = 1   # hipErrorInvalidValue
INF = ER.INF

SHAPES = [(1, 1), (1, 70), (70, 1), (67, 131), (129, 257), (3, 63), (3, 64), (3, 65), (15, 5), (16, 5), (17, 5),
          (31, 5), (32, 5), (33, 5), (3, 255), (3, 256), (3, 257), (255, 3), (256, 3), (257, 3), (2, 600)]
PAIR_SHAPES = [(1, 70), (70, 1), (33, 65), (67, 131), (129, 257)]
THR = np.float32(0.5)
MODE_CODE = {"foreground": 0, "background": 1, "boundary": 2}
U = 2.0 ** -53


def _S():
    import vaeunet_amd.surface as S
    return S


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _planes(H, W):
    """(names, uint8 [K, 1, H, W]): every adversarial plane of the shape"""
    d = ER.adversarial_planes(H, W)
    return tuple(d), _ro(np.stack(list(d.values()))[:, None])


@functools.lru_cache(maxsize=None)
def _want_edt(H, W, mode):
    """the reference transform of _planes(H, W): computed once, shared, read-only"""
    return _ro(ER.edt2(_planes(H, W)[1], mode))


@functools.lru_cache(maxsize=None)
def _pairs(H, W):
    """(names, pred uint8 [K, 1, H, W], gt uint8 [K, 1, H, W])"""
    d = ER.pair_planes(H, W)
    return tuple(d), _ro(np.stack([p for p, _ in d.values()])[:, None]), _ro(np.stack([g for _, g in d.values()])[:, None])


@functools.lru_cache(maxsize=None)
def _want_stats(H, W, q, tolerance):
    names, pred, gt = _pairs(H, W)
    st, sm = ER.stats(pred, gt, 0.5, q, tolerance)
    return _ro(st), _ro(sm)


def _as_prob(fg, seed):
    """a float32 map whose foreground at threshold 0.5 is fg: foreground in (0.5, 1], background in [0, 0.5] with
    exact 0.5 and NaN among it"""
    rng = np.random.Generator(np.random.PCG64(seed))
    u = rng.random(fg.shape, dtype=np.float32)
    lo = np.nextafter(THR, np.float32(1))
    p = np.where(fg != 0, lo + u * (np.float32(1) - lo), u * THR).astype(np.float32)
    pick = rng.random(fg.shape)
    p[(fg == 0) & (pick < 0.1)] = THR
    p[(fg == 0) & (pick > 0.9)] = np.nan
    p[(fg != 0) & (pick < 0.05)] = lo
    p[(fg != 0) & (pick > 0.95)] = 1.0
    assert np.array_equal(LR.foreground(p, THR), fg != 0)
    return p


def _code(x):
    from vaeunet_amd import _lib as L
    return L.VU_CCL_F32 if x.dtype == np.float32 else L.VU_CCL_U8


def _put(x):
    """a numpy input inside a guarded device buffer"""
    t, g = R.guarded(x.shape, torch.float32 if x.dtype == np.float32 else torch.uint8, DEV)
    t.copy_(torch.from_numpy(np.array(x)))
    return t, g


def _unchanged(t, x):
    assert np.array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(x).view(np.uint8))


def _edt_raw(x, mode, out_f32=False):
    """vu_edt on guarded buffers -> numpy; the input bitwise unchanged, no guard written"""
    from vaeunet_amd import _lib as L
    B, C, H, W = x.shape
    dx, gx = _put(x)
    out, go = R.guarded(x.shape, torch.float32 if out_f32 else torch.int32, DEV)
    L.call("vu_edt", L.ptr(dx), _code(x), 0.5, MODE_CODE[mode], B * C, H, W, L.ptr(out), int(out_f32), L.stream())
    torch.cuda.synchronize()
    gx.check("vu_edt input")
    go.check("vu_edt output")
    _unchanged(dx, x)
    return out.cpu().numpy()


def _boundary_raw(x):
    from vaeunet_amd import _lib as L
    B, C, H, W = x.shape
    dx, gx = _put(x)
    out, go = R.guarded(x.shape, torch.uint8, DEV)
    L.call("vu_edt_boundary", L.ptr(dx), _code(x), 0.5, B * C, H, W, L.ptr(out), L.stream())
    torch.cuda.synchronize()
    gx.check("vu_edt_boundary input")
    go.check("vu_edt_boundary output")
    _unchanged(dx, x)
    return out.cpu().numpy()


def _stats_raw(pred, gt, q, tolerance):
    """vu_surface_stats on guarded buffers (the workspace included) -> (stats, sums) numpy"""
    from vaeunet_amd import _lib as L
    B, C, H, W = pred.shape
    dp, gp = _put(pred)
    dg, gg = _put(gt)
    st, gs = R.guarded((B, C, 8), torch.int64, DEV)
    sm, gm = R.guarded((B, C, 2), torch.float64, DEV)
    nbytes = L.query("vu_edt_workspace_bytes", B * C, H, W)
    assert nbytes > 0 and nbytes % 4 == 0
    ws, gw = R.guarded(nbytes // 4, torch.int32, DEV)
    L.call("vu_surface_stats", L.ptr(dp), _code(pred), 0.5, L.ptr(dg), _code(gt), B * C, H, W, q,
           ER.tol2_of(tolerance), L.ptr(st), L.ptr(sm), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    for g in (gp, gg, gs, gm, gw):
        g.check("vu_surface_stats")
    _unchanged(dp, pred)
    _unchanged(dg, gt)
    return st.cpu().numpy(), sm.cpu().numpy()


def _sums_within_bound(got, want, n):
    """|sum - want| <= 2 n 2^-53 want, n the set's size: the bound of a length-n fp64 summation (the roots themselves
    are correctly rounded on both sides)"""
    return bool((np.abs(got - want) <= 2.0 * n * U * want).all())


def _ulp_close(got, want, ulps=1):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - want) <= ulps * np.spacing(np.abs(want))
    return bool((ok | both_nan).all())


# ----------------------------------------------------------------------------
# the transform and the boundary
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("HW", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_transform_and_boundary_are_exactly_the_reference(HW):
    H, W = HW
    names, planes = _planes(H, W)
    prob = _as_prob(planes, 1000 * H + W)
    want_b = ER.boundary(planes)
    for x in (planes, prob):
        for mode in ER.MODES:
            got, want = _edt_raw(x, mode), _want_edt(H, W, mode)
            assert got.dtype == np.int32
            bad = [n for k, n in enumerate(names) if not np.array_equal(got[k], want[k])]
            assert not bad, (mode, x.dtype, bad)
        assert np.array_equal(_boundary_raw(x), want_b), x.dtype
    assert (_want_edt(H, W, "foreground")[names.index("none")] == INF).all()
    assert (_want_edt(H, W, "background")[names.index("all")] == INF).all()


def test_float_output_is_the_rounded_root_and_inf_on_a_plane_without_a_site():
    S = _S()
    H, W = 67, 131
    names, planes = _planes(H, W)
    for mode in ER.MODES:
        want2 = _want_edt(H, W, mode)
        with np.errstate(over="ignore"):
            want = np.where(want2 == INF, np.inf, np.sqrt(want2.astype(np.float64))).astype(np.float32)
        got = _edt_raw(planes, mode, out_f32=True)
        assert got.dtype == np.float32 and np.array_equal(got, want), mode
        assert np.isinf(got).any()              # "none" has no foreground or boundary site, "all" no background site
    d = torch.from_numpy(np.array(planes)).to(DEV)
    assert torch.equal(S.distance_transform(d, "boundary", squared=False).cpu(), torch.from_numpy(
        _edt_raw(planes, "boundary", out_f32=True)))


@pytest.mark.parametrize("HW", [(1, 16384), (16384, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_longest_row_and_column_with_the_site_at_one_end(HW):
    """d^2 reaches 16383^2 = 268,402,689; the row search of the far pixel walks the whole row"""
    H, W = HW
    n = H * W
    idx = np.arange(n, dtype=np.int64)
    for end in (0, n - 1):
        x = np.zeros(n, np.uint8)
        x[end] = 1
        want = ((idx - end) ** 2).astype(np.int32).reshape(1, 1, H, W)
        assert want.max() == 16383 ** 2
        for mode in ("foreground", "boundary"):
            assert np.array_equal(_edt_raw(x.reshape(1, 1, H, W), mode), want), (mode, end)
        assert np.array_equal(_edt_raw((1 - x).reshape(1, 1, H, W), "background"), want), end


def test_a_batch_of_different_planes_and_the_api():
    """[2, 3, 67, 131]: six different planes; planes do not interact, and the Python functions and the op give what
    the C ABI gives"""
    import vaeunet_amd.ops  # noqa: F401
    S = _S()
    H, W = 67, 131
    names, planes = _planes(H, W)
    pick = [names.index(k) for k in ("corner11", "bernoulli0.5", "none", "last_row", "bernoulli0.0085", "all")]
    x = np.ascontiguousarray(planes[pick].reshape(2, 3, H, W))
    prob = _as_prob(x, 77)
    d, dp = torch.from_numpy(x).to(DEV), torch.from_numpy(prob).to(DEV)
    for mode in ER.MODES:
        want = _want_edt(H, W, mode)[pick].reshape(2, 3, H, W)
        assert np.array_equal(_edt_raw(x, mode), want), mode
        for got in (S.distance_transform(d, mode), S.distance_transform(d.bool(), mode),
                    S.distance_transform(dp, mode, threshold=0.5), torch.ops.vaeunet.distance_transform(d, mode),
                    torch.ops.vaeunet.distance_transform(dp, mode, 0.5)):
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), mode
    assert torch.equal(S.distance_transform(d), S.distance_transform(d, "background"))
    assert torch.equal(torch.ops.vaeunet.distance_transform(d, "foreground", None, False),
                       S.distance_transform(d, "foreground", squared=False))
    wb = ER.boundary(x)
    for got in (S.boundary(d), S.boundary(d.bool()), S.boundary(dp, threshold=0.5)):
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), wb)
    # another threshold is another foreground; the u8 rule ignores it; a non-contiguous input is densified
    assert np.array_equal(S.distance_transform(dp, "foreground", threshold=0.75).cpu().numpy(),
                          ER.edt2(prob, "foreground", 0.75))
    assert torch.equal(S.distance_transform(d * 200, "foreground", threshold=250.0), S.distance_transform(d, "foreground"))
    wide = torch.zeros(2, 3, H, 2 * W, dtype=torch.uint8, device=DEV)
    wide[..., ::2] = d
    assert torch.equal(S.distance_transform(wide[..., ::2], "boundary"), S.distance_transform(d, "boundary"))


def test_c_abi_rejections_write_nothing():
    from vaeunet_amd import _lib as L
    x = torch.ones(1, 1, 8, 8, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 1, 8, 8), 7, dtype=torch.int32, device=DEV)
    b = torch.full((1, 1, 8, 8), 7, dtype=torch.uint8, device=DEV)
    st = torch.full((8,), 7, dtype=torch.int64, device=DEV)
    sm = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)
    per = torch.full((4,), 7.0, dtype=torch.float64, device=DEV)
    ws = torch.full((L.query("vu_edt_workspace_bytes", 1, 8, 8) // 4,), 7, dtype=torch.int32, device=DEV)
    q, s, p = L.query, L.stream(), L.ptr
    for args in ((p(x), 2, 0.5, 0, 1, 8, 8, p(out), 0, s), (p(x), -1, 0.5, 0, 1, 8, 8, p(out), 0, s),
                 (p(x), 0, 0.5, 3, 1, 8, 8, p(out), 0, s), (p(x), 0, 0.5, -1, 1, 8, 8, p(out), 0, s),
                 (p(x), 0, 0.5, 0, -1, 8, 8, p(out), 0, s), (p(x), 0, 0.5, 0, 1, -8, 8, p(out), 0, s),
                 (p(x), 0, 0.5, 0, 1, 8, 16385, p(out), 0, s), (p(x), 0, 0.5, 0, 1, 16385, 8, p(out), 0, s),
                 (p(x), 0, 0.5, 0, 1, 8, 8, p(out), 2, s), (None, 0, 0.5, 0, 1, 8, 8, p(out), 0, s),
                 (p(x), 0, 0.5, 0, 1, 8, 8, None, 0, s)):
        assert q("vu_edt", *args) == INVALID, args[1:9]
    for n0 in ((0, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert q("vu_edt", p(x), 0, 0.5, 0, *n0, p(out), 0, s) == 0
        assert q("vu_edt_boundary", p(x), 0, 0.5, *n0, p(b), s) == 0
        assert q("vu_surface_stats", p(x), 0, 0.5, p(x), 0, *n0, 95, 1, p(st), p(sm), p(ws), s) == 0
    for args in ((p(x), 2, 0.5, 1, 8, 8, p(b), s), (p(x), 0, 0.5, -1, 8, 8, p(b), s), (p(x), 0, 0.5, 1, 8, 16385, p(b), s),
                 (None, 0, 0.5, 1, 8, 8, p(b), s), (p(x), 0, 0.5, 1, 8, 8, None, s)):
        assert q("vu_edt_boundary", *args) == INVALID
    ok = [p(x), 0, 0.5, p(x), 0, 1, 8, 8, 95, 1, p(st), p(sm), p(ws), s]
    for at, bad in ((1, 2), (4, 2), (5, -1), (6, 16385), (7, 16385), (6, -1), (8, 0), (8, 101), (8, -5), (9, -1),
                    (0, None), (3, None), (10, None), (11, None), (12, None)):
        args = list(ok)
        args[at] = bad
        assert q("vu_surface_stats", *args) == INVALID, (at, bad)
    assert q("vu_surface_metrics", p(st), p(sm), -1, p(per), None, None, s) == INVALID
    assert q("vu_surface_metrics", p(st), p(sm), 1, p(per), p(per), None, s) == INVALID
    assert q("vu_surface_metrics", p(st), p(sm), 1, p(per), None, p(st), s) == INVALID
    assert q("vu_surface_metrics", None, p(sm), 1, p(per), None, None, s) == INVALID
    assert q("vu_surface_metrics", p(st), None, 1, p(per), None, None, s) == INVALID
    assert q("vu_surface_metrics", p(st), p(sm), 1, None, None, None, s) == INVALID
    assert q("vu_surface_metrics", p(st), p(sm), 0, p(per), None, None, s) == 0
    assert q("vu_edt_workspace_bytes", 1, 16385, 8) == -1 and q("vu_edt_workspace_bytes", -1, 8, 8) == -1
    torch.cuda.synchronize()
    assert (out == 7).all() and (b == 7).all() and (st == 7).all() and (sm == 7).all() and (per == 7).all()
    assert (ws == 7).all() and (x == 1).all()


# ----------------------------------------------------------------------------
# surface statistics
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("HW", PAIR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_surface_stats_are_exactly_the_reference(HW):
    H, W = HW
    names, pred, gt = _pairs(H, W)
    want_st, want_sm = _want_stats(H, W, 95, 1.0)
    if HW == (67, 131):   # the scenarios are what their names say
        by = dict(zip(names, want_st[:, 0]))
        assert by["identical"][2:6].tolist() == [0, 0, 0, 0] and by["identical"][6] == by["identical"][0] > 0
        assert by["empty_pred"].tolist()[0] == 0 and by["empty_pred"][1] > 0 and (by["empty_pred"][2:] == -1).all()
        assert by["empty_gt"].tolist()[1] == 0 and by["empty_gt"][0] > 0 and (by["empty_gt"][2:] == -1).all()
        assert by["nested_squares"][2] > by["nested_squares"][4] > 0 and by["shifted_disc"][2] > 0
    for p in (pred, _as_prob(pred, 5 * H + W)):
        st, sm = _stats_raw(p, gt, 95, 1.0)
        bad = [n for k, n in enumerate(names) if not np.array_equal(st[k], want_st[k])]
        assert not bad, (p.dtype, bad, st[:, 0].tolist(), want_st[:, 0].tolist())
        assert _sums_within_bound(sm, want_sm, want_st[..., :2]), (sm, want_sm)
        assert (sm[want_st[..., 2] < 0] == 0).all()


@pytest.mark.parametrize("q,tolerance", [(100, 0.0), (1, 2.5), (50, 3.0), (99, 1.0)])
def test_percentiles_tolerances_and_every_truth_dtype(q, tolerance):
    S = _S()
    H, W = 67, 131
    names, pred, gt = _pairs(H, W)
    want_st, want_sm = _want_stats(H, W, q, tolerance)
    st, sm = _stats_raw(pred, gt, q, tolerance)
    assert np.array_equal(st, want_st), (st[:, 0].tolist(), want_st[:, 0].tolist())
    if q == 100:
        assert np.array_equal(st[..., 4:6], st[..., 2:4])
    dp = torch.from_numpy(np.array(pred)).to(DEV)
    for masks in (gt, gt.astype(np.float32), gt.astype(bool), gt.astype(np.int64)):
        gst, gsm = S.surface_stats(dp, torch.from_numpy(np.array(masks)).to(DEV), percentile=q, tolerance=tolerance)
        assert gst.dtype == torch.int64 and gst.shape == (len(names), 1, 8) and gsm.dtype == torch.float64
        assert np.array_equal(gst.cpu().numpy(), want_st), masks.dtype
        assert np.array_equal(gsm.cpu().numpy(), sm), masks.dtype          # the same sums, bitwise
    # a float32 prediction at another threshold
    prob = _as_prob(pred, 9)
    w2, _ = ER.stats(prob, gt, 0.75, q, tolerance)
    g2, _ = S.surface_stats(torch.from_numpy(prob).to(DEV), torch.from_numpy(np.array(gt)).to(DEV), threshold=0.75,
                            percentile=q, tolerance=tolerance)
    assert np.array_equal(g2.cpu().numpy(), w2)


def test_two_runs_are_bitwise_equal_and_the_metrics_are_within_one_ulp():
    S = _S()
    H, W = 129, 257                                   # 33 blocks per plane in the streaming passes
    names, pred, gt = _pairs(H, W)
    dp, dg = torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV)
    st1, sm1 = S.surface_stats(dp, dg)
    m1 = S.surface_metrics(st1, sm1)
    st2, sm2 = S.surface_stats(dp, dg)
    m2 = S.surface_metrics(st2, sm2)
    assert torch.equal(st1, st2)
    assert torch.equal(sm1.view(torch.int64), sm2.view(torch.int64))
    assert torch.equal(m1.view(torch.int64), m2.view(torch.int64))
    want_st, want_sm = _want_stats(H, W, 95, 1.0)
    assert np.array_equal(st1.cpu().numpy(), want_st)
    assert _sums_within_bound(sm1.cpu().numpy(), want_sm, want_st[..., :2])
    # square roots and quotients of the device's own tables: one ulp
    want = ER.metrics(st1.cpu().numpy(), sm1.cpu().numpy())
    got = m1.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (len(names), 1, 4)
    assert _ulp_close(got, want), (got, want)
    assert np.isnan(got[names.index("empty_pred")]).all() and np.isnan(got[names.index("empty_gt")]).all()
    assert (got[names.index("identical"), 0] == [0.0, 0.0, 0.0, 1.0]).all()
    assert np.isfinite(got[names.index("shifted_disc")]).all()


# ----------------------------------------------------------------------------
# the meter
# ----------------------------------------------------------------------------
def _meter_batches():
    """three (pred float32, gt uint8) batches of different shapes, two classes each; undefined planes among them"""
    out = []
    for i, (H, W) in enumerate(((33, 65), (70, 40), (20, 20))):
        names, pred, gt = _pairs(H, W)
        k = len(names) // 2 * 2
        p, g = pred[:k].reshape(k // 2, 2, H, W), gt[:k].reshape(k // 2, 2, H, W)
        out.append((_as_prob(p, 300 + i), np.ascontiguousarray(g)))
    return out


def _pooled_close(got, per_plane, rel=0.0):
    """got [4] against the mean over the defined planes of per_plane [N, 4], added in plane order on both sides.
    Each of the k terms is within 1 ulp (+ rel, relative) of the reference's, a term is at most the sum, and each
    of the k additions rounds a perturbed value: <= 2 k ulp of the sum; the quotient adds one: 4 k + 2 spacings of the
    result cover it with a factor two to spare."""
    want, k = ER.pooled(per_plane)
    if k == 0:
        return bool(np.isnan(got).all()), want, k
    tol = (4 * k + 2) * np.spacing(np.abs(want)) + rel * np.abs(want)
    return bool((np.abs(got - want) <= tol).all()), want, k


def test_meter_over_three_updates_equals_the_reference_over_all_planes():
    S = _S()
    meter = S.SurfaceMeter(threshold=0.5, percentile=90, tolerance=2.0)
    rows, nmax = [], 0
    for prob, gt in _meter_batches():
        meter.update(torch.from_numpy(prob).to(DEV), torch.from_numpy(np.array(gt)).to(DEV))
        st, sm = ER.stats(prob, gt, 0.5, 90, 2.0)
        rows.append(ER.metrics(st, sm).reshape(-1, 4))
        nmax = max(nmax, int(st[..., :2].max()))
    per_plane = np.concatenate(rows)
    planes = len(per_plane)
    assert meter.n_planes == planes == 18
    got = meter.values()
    assert got.dtype == torch.float64 and got.shape == (4,) and got.device.type == "cuda"
    # the reference's sums are exact (fsum): assd carries the device summation's 2 n 2^-53 on top
    ok, want, k = _pooled_close(got.cpu().numpy(), per_plane, rel=2.0 * nmax * U)
    assert ok, (got, want)
    assert 0 < k < planes and meter.counts().tolist() == [k, planes]
    res = meter.compute()
    assert set(res) == {"hd", "hd_q", "assd", "nsd", "n_defined"} and int(res["n_defined"]) == k
    assert res["hd"].item() == got[0].item() and res["hd"].item() >= res["hd_q"].item() > 0
    # a meter that saw undefined planes only: NaN, zero defined
    m2 = S.SurfaceMeter()
    m2.update(torch.zeros(1, 2, 9, 9, dtype=torch.uint8, device=DEV), torch.ones(1, 2, 9, 9, device=DEV))
    assert torch.isnan(m2.values()).all() and m2.counts().tolist() == [0, 2]
    meter.reset()
    with pytest.raises(RuntimeError):
        meter.values()


def test_meter_update_does_not_synchronise():
    S = _S()
    dev = [(torch.from_numpy(p).to(DEV), torch.from_numpy(np.array(g)).to(DEV)) for p, g in _meter_batches()]
    meter = S.SurfaceMeter()
    meter.update(*dev[2])                        # first use: library load, state and the largest scratch
    meter.update(*dev[1])
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            enforced = False
        except RuntimeError:
            enforced = True
        if enforced:
            for p, g in dev:
                meter.update(p, g)
                S.surface_stats(p, g)
            meter.values()
            meter.compute()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not enforced:
        pytest.skip("this torch build does not enforce torch.cuda.set_sync_debug_mode('error') "
                    "(a .item() did not raise), so the absence of host syncs cannot be asserted")
    assert meter.counts()[1].item() == 12 + 18


# ----------------------------------------------------------------------------
# evaluate
# ----------------------------------------------------------------------------
class _Net(nn.Module):
    """logits = an affine map of the first image channel: both predictions occur, no value near the threshold"""

    def forward(self, x):
        return (torch.round(x[:, :1] * 8) / 8 - 0.4375) * 4


def _host_waits(fn):
    """fn() and the number of host synchronisations torch reports during it"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, sum("synchroniz" in str(w.message).lower() for w in seen)


def test_evaluate_with_surface_against_the_reference_and_evaluate():
    from vaeunet_amd.evaluate import evaluate, evaluate_with_surface
    from vaeunet_amd.lesions import LesionMeter
    from vaeunet_amd.metrics import METRIC_NAMES, seg_counts
    S = _S()
    g = torch.Generator().manual_seed(3)
    batches = []
    for B in (2, 1):
        image = torch.nn.functional.interpolate(torch.rand(B, 3, 12, 12, generator=g), size=(48, 48), mode="nearest")
        mask = torch.nn.functional.interpolate((torch.rand(B, 1, 16, 16, generator=g) < 0.2).float(), size=(48, 48),
                                               mode="nearest")
        batches.append({"image": image.to(DEV), "mask": mask.to(DEV)})
    net = _Net().to(DEV)
    evaluate(net, batches, DEV)                                    # warm: library load, allocations
    evaluate_with_surface(net, batches, DEV, S.SurfaceMeter())
    plain, waits_plain = _host_waits(lambda: evaluate(net, batches, DEV))
    meter = S.SurfaceMeter(percentile=95, tolerance=1.0)
    res, waits = _host_waits(lambda: evaluate_with_surface(net, batches, DEV, meter))
    assert waits == waits_plain, (waits, waits_plain)
    assert waits_plain >= 1, "torch reports no host synchronisation at all: the count is unchecked"
    assert set(plain) == set(METRIC_NAMES) | {f"pooled_{k}" for k in METRIC_NAMES} | {"batches"}
    assert {k: res[k] for k in plain} == plain
    assert set(res) - set(plain) == {"surface_hd", "surface_hd95", "surface_assd", "surface_nsd", "surface_n_defined"}
    rows, nmax = [], 0
    for b in batches:
        hard = torch.empty(b["mask"].shape, dtype=torch.uint8, device=DEV)
        seg_counts(net(b["image"]), b["mask"], hard_mask=hard)
        assert 0 < int(hard.sum()) < hard.numel()
        st, sm = ER.stats(hard.cpu().numpy(), b["mask"].cpu().numpy(), 0.5, 95, 1.0)
        rows.append(ER.metrics(st, sm).reshape(-1, 4))
        nmax = max(nmax, int(st[..., :2].max()))
    got = np.array([res["surface_hd"], res["surface_hd95"], res["surface_assd"], res["surface_nsd"]])
    ok, want, k = _pooled_close(got, np.concatenate(rows), rel=2.0 * nmax * U)
    assert ok and k > 0, (got, want)
    assert res["surface_n_defined"] == k and isinstance(res["surface_n_defined"], int)
    assert isinstance(res["surface_hd"], float) and meter.n_planes == 3
    # with a lesion meter as well: the lesion keys of evaluate_with_lesions join, the percentile names the key
    both = evaluate_with_surface(net, batches, DEV, S.SurfaceMeter(percentile=90), lesion_meter=LesionMeter(min_area=2))
    assert {k: both[k] for k in plain} == plain
    assert set(both) - set(plain) == {"surface_hd", "surface_hd90", "surface_assd", "surface_nsd", "surface_n_defined",
                                      "lesion_sensitivity", "lesion_precision", "lesion_fp_per_image", "lesion_n_gt",
                                      "lesion_n_pred"}
    assert both["surface_hd"] == res["surface_hd"] and both["surface_hd90"] <= res["surface_hd95"]
