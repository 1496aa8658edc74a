"""Calibration / uncertainty metrics on the GPU (csrc/calib.hip,
vaeunet_amd/calibration.py) against a torch CPU restatement of the definitions
in include/vaeunet.h: fp32 for the bin index expressions (one multiply, one
truncation -- the same operation on both sides, so the integer histograms must
be equal, not close), int64 bincount, fp64 for the sums and the metrics."""
import math
import warnings

import pytest
import torch

from vaeunet_amd import calibration as CAL

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 1024
LN2 = math.log(2)


# ---- the restatement --------------------------------------------------------------------
def f32(v):
    return torch.tensor(v, dtype=torch.float64).to(torch.float32)


def bin_index(x, scale, bins):
    """min((int)(x * scale), bins - 1) with the product in fp32"""
    return torch.clamp((x * scale).to(torch.int32), max=bins - 1).long()


def restate(p, mask, u=None, nb=15, u_max=LN2):
    """dict of CPU tensors named as CalibCounts, plus the per-quantity sums of
    |term| that the fp64 error bounds need"""
    p = p.detach().cpu().flatten().float()
    t = mask.detach().cpu().flatten().float() > 0.5
    ok = ~torch.isnan(p)
    pc, tv = torch.clamp(p[ok], 0.0, 1.0), t[ok]
    cb = bin_index(pc, f32(nb), nb)
    rb = bin_index(pc, f32(R), R)
    out = {"conf_hist": torch.bincount(cb * 2 + tv.long(), minlength=2 * nb).view(nb, 2),
           "rank_hist": torch.bincount(rb * 2 + tv.long(), minlength=2 * R).view(R, 2),
           "conf_sum": torch.zeros(nb, dtype=torch.float64).index_add_(0, cb, pc.double())}
    d = pc.double() - tv.double()
    q = pc.double().clamp(1e-7, 1 - 1e-7)
    nll = -torch.where(tv, q.log(), (1 - q).log())
    out["sums"] = torch.stack([(d * d).sum(), nll.sum()])
    out["abs_terms"] = torch.stack([(d * d).sum(), nll.abs().sum()])
    invalid = [int((~ok).sum()), 0]
    out["unc_hist"] = None
    if u is not None:
        uf = u.detach().cpu().flatten().float()[ok]
        uok = ~torch.isnan(uf)
        invalid[1] = int((~uok).sum())
        ub = bin_index(uf[uok].clamp_min(0.0), f32(R / u_max), R)
        err = (pc[uok] > 0.5) != tv[uok]
        out["unc_hist"] = torch.bincount(ub * 2 + err.long(), minlength=2 * R).view(R, 2)
    out["invalid"] = torch.tensor(invalid, dtype=torch.int64)
    return out


def metrics_ref(c):
    """fp64 metrics from a dict / CalibCounts of totals (CPU)"""
    get = (lambda k: c[k]) if isinstance(c, dict) else (lambda k: getattr(c, k))
    ch = get("conf_hist").cpu().double()
    cnt = ch.sum(1)
    N = cnt.sum()
    nz = cnt > 0
    safe = cnt.clamp_min(1.0)
    acc = torch.where(nz, ch[:, 1] / safe, torch.zeros(()).double())
    conf = torch.where(nz, get("conf_sum").cpu().double() / safe, torch.zeros(()).double())
    gap = (acc - conf).abs()
    res = {"reliability": torch.stack([cnt, acc, conf], 1), "n": N}
    res["ece"] = (cnt[nz] / N * gap[nz]).sum()
    res["mce"] = gap[nz].max() if bool(nz.any()) else torch.tensor(float("nan")).double()
    sums = get("sums").cpu().double()
    res["brier"], res["nll"] = sums[0] / N, sums[1] / N
    rh = get("rank_hist").cpu().double()
    neg, pos = rh[:, 0], rh[:, 1]
    P, Q = pos.sum(), neg.sum()
    res["positives"] = P
    nan = torch.tensor(float("nan")).double()
    below = neg.cumsum(0) - neg
    res["auroc"] = ((pos * below).sum() + 0.5 * (pos * neg).sum()) / (P * Q) if P * Q > 0 else nan
    res["auroc_tie_bound"] = (pos * neg).sum() / (2 * P * Q) if P * Q > 0 else nan
    posd, alld = pos.flip(0), (pos + neg).flip(0)
    tp, seen = posd.cumsum(0), alld.cumsum(0)
    m = posd > 0
    res["auprc"] = ((posd[m] / P) * (tp[m] / seen[m])).sum() if P > 0 else nan
    uh = get("unc_hist")
    if uh is None:
        res["ause"] = res["n_uncertainty"] = res["uncertainty_errors"] = nan
        res["sparsification"] = torch.full((R + 1, 3), float("nan"), dtype=torch.float64)
        return res
    uh = uh.cpu().double()
    zero = torch.zeros(1, dtype=torch.float64)
    C = torch.cat([zero, uh.sum(1).flip(0).cumsum(0)])
    Ec = torch.cat([zero, uh[:, 1].flip(0).cumsum(0)])
    Nu, E = C[-1], Ec[-1]
    den = Nu - C
    live = den > 0
    sden = torch.where(live, den, torch.ones(()).double())
    frac = C / Nu
    err = torch.where(live, (E - Ec) / sden, torch.zeros(()).double())
    orc = torch.where(live, (E - C).clamp_min(0.0) / sden, torch.zeros(()).double())
    g = err - orc
    res["sparsification"] = torch.stack([frac, err, orc], 1)
    res["ause"] = ((frac[1:] - frac[:-1]) * (0.5 * (g[1:] + g[:-1]))).sum()
    res["n_uncertainty"], res["uncertainty_errors"] = Nu, E
    return res


def exact_auroc(p, t):
    """Mann-Whitney AUROC from sorted scores, average ranks for ties (fp64, CPU)"""
    vals, inv, cnt = torch.unique(p.cpu().flatten().double(), sorted=True, return_inverse=True, return_counts=True)
    cntd = cnt.double()
    avg_rank = cntd.cumsum(0) - cntd + (cntd + 1) / 2
    t = t.cpu().flatten() > 0.5
    P, Q = t.sum().double(), (~t).sum().double()
    return (avg_rank[inv][t].sum() - P * (P + 1) / 2) / (P * Q)


def assert_ints_equal(got, ref):
    assert torch.equal(got.conf_hist.cpu(), ref["conf_hist"])
    assert torch.equal(got.rank_hist.cpu(), ref["rank_hist"])
    if ref["unc_hist"] is None:
        assert got.unc_hist is None
    else:
        assert torch.equal(got.unc_hist.cpu(), ref["unc_hist"])
    assert torch.equal(got.invalid.cpu(), ref["invalid"])


def assert_sums_close(got, ref, n):
    """|error| <= n 2^-51 sum|term|: the recursive-summation bound n 2^-53 sum|term|, times 4 for the two
    sides and the ulps of the two log implementations"""
    bound = n * 2.0 ** -51
    cs, rs = got.conf_sum.cpu(), ref["conf_sum"]
    print("conf_sum max err", float((cs - rs).abs().max()), "bound(min over bins)", float((bound * rs).min()))
    assert bool(((cs - rs).abs() <= bound * rs).all())
    s = got.sums.cpu()
    print("brier/nll err", (s - ref["sums"]).abs().tolist(), "bound", (bound * ref["abs_terms"]).tolist())
    assert bool(((s - ref["sums"]).abs() <= bound * ref["abs_terms"]).all())


def assert_metrics_close(got, ref, tol=1e-12):
    for k, r in ref.items():
        g = got[k].cpu()
        assert g.shape == r.shape and g.dtype == torch.float64, k
        both_nan = torch.isnan(g) & torch.isnan(r)
        lim = tol * torch.clamp(r.abs(), min=1.0)
        good = both_nan | ((g - r).abs() <= torch.nan_to_num(lim, nan=0.0))
        assert bool(good.all()), (k, g, r)


def rand_case(n, seed, pos_rate=0.3):
    g = torch.Generator().manual_seed(seed)
    # arbitrary fp32 probabilities: not multiples of 2^-24 (scaled by an irrational factor), a few exact 0 / 1
    p = (torch.rand(n, generator=g) * 0.9999).pow(1.7)
    p[torch.rand(n, generator=g) < 0.02] = 1.0
    p[torch.rand(n, generator=g) < 0.02] = 0.0
    m = (torch.rand(n, generator=g) < pos_rate).float()
    u = torch.rand(n, generator=g) * LN2
    return p, m, u


# ---- 1. exact histograms -----------------------------------------------------------------
@pytest.mark.parametrize("nb", [15, 16, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1023, 4099])
def test_histograms_exact(n, nb):
    p, m, u = rand_case(n + 1, 100 + n)
    pd, md, ud = p.to(DEV), m.to(DEV), u.to(DEV)
    for off in (0, 1):                      # off = 1: a view one element past an aligned base
        sl = slice(off, off + n)
        ref = restate(p[sl], m[sl], u[sl], nb)
        assert_ints_equal(CAL.calib_hist(pd[sl], md[sl], ud[sl], n_bins=nb), ref)
        ref["unc_hist"], ref["invalid"][1] = None, 0
        assert_ints_equal(CAL.calib_hist(pd[sl], md[sl], n_bins=nb), ref)


def test_misaligned_uncertainty_only():
    """p aligned, u and the mask on other offsets: the element-wise path"""
    p, m, u = rand_case(1500, 7)
    ud, md = torch.cat([u[:1], u]).to(DEV)[1:], torch.cat([m[:2], m]).to(DEV).to(torch.uint8)[2:]
    assert_ints_equal(CAL.calib_hist(p.to(DEV), md, ud), restate(p, m, u))


# ---- 2. edges --------------------------------------------------------------------------------
@pytest.mark.parametrize("truth", [0, 1])
def test_edges(truth):
    grid = torch.arange(1025, dtype=torch.float64) / 1024
    fifteenths = (torch.arange(16, dtype=torch.float64) / 15).float()
    outside = torch.tensor([-0.25, -1e-30, -0.0, 1.0000001, 3.5, -float("inf"), float("inf")])
    p = torch.cat([grid.float(), fifteenths, outside, torch.tensor([float("nan")] * 3)])
    n = p.numel()
    m = torch.full((n,), float(truth))
    u = torch.linspace(0, LN2, n)
    u[5], u[40], u[41] = float("nan"), LN2 * 1.5, 1e5          # NaN, and two beyond u_max
    u[-1] = float("nan")                                          # with a NaN p: counted once, as invalid p
    u[7] = -0.3                                                   # clamped to bin 0
    for nb in (15, 16):
        ref = restate(p, m, u, nb)
        got = CAL.calib_hist(p.to(DEV), m.to(DEV), u.to(DEV), n_bins=nb)
        assert_ints_equal(got, ref)
        assert ref["invalid"].tolist() == [3, 1]
        assert int(ref["conf_hist"].sum()) == n - 3 and int(ref["unc_hist"].sum()) == n - 4
    # p = 1.0 and everything above it: last bin; p = 0.5: a hard negative (an error iff truth is 1)
    one = CAL.calib_hist(torch.tensor([1.0, 7.0], device=DEV), torch.full((2,), float(truth), device=DEV),
                         torch.tensor([0.0, 5.0], device=DEV))
    assert one.conf_hist.cpu()[14, truth] == 2 and one.rank_hist.cpu()[1023, truth] == 2
    assert one.unc_hist.cpu()[1023].sum() == 1
    half = CAL.calib_hist(torch.tensor([0.5], device=DEV), torch.tensor([float(truth)], device=DEV),
                          torch.tensor([0.0], device=DEV))
    assert half.unc_hist.cpu()[0].tolist() == [1 - truth, truth]
    assert half.rank_hist.cpu()[512, truth] == 1 and half.conf_hist.cpu()[7, truth] == 1


# ---- 3. one-bin skew (the wave-aggregation path) ----------------------------------------------
@pytest.mark.parametrize("value", [0.0, 0.5, 1.0, "mix"])
def test_one_bin_skew(value):
    n = 70001
    g = torch.Generator().manual_seed(3)
    if value == "mix":                       # 99 % below 1/1024 with truth 0, 1 % anywhere with mixed truth
        rare = torch.rand(n, generator=g) < 0.01
        p = torch.where(rare, torch.rand(n, generator=g), torch.rand(n, generator=g) * (0.9 / 1024))
        m = (rare & (torch.rand(n, generator=g) < 0.5)).float()
        u = torch.where(rare, torch.rand(n, generator=g) * LN2, torch.rand(n, generator=g) * 1e-4)
    else:
        p = torch.full((n,), value)
        m = (torch.arange(n) % 3 == 0).float()
        u = torch.full((n,), 0.25)
    ref = restate(p, m, u)
    got = CAL.calib_hist(p.to(DEV), m.to(DEV), u.to(DEV))
    assert_ints_equal(got, ref)
    assert_sums_close(got, ref, n)


# ---- 4. more than one grid sweep ------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_case():
    n = 1_200_003                            # > 768 blocks x 1024 pixels per step, not a multiple of 4
    p, m, u = rand_case(n, 11, 0.2)
    return p, m, u, restate(p, m, u)


def test_grid_stride_sweeps(big_case):
    p, m, u, ref = big_case
    got = CAL.calib_hist(p.to(DEV), m.to(DEV), u.to(DEV))
    assert_ints_equal(got, ref)
    assert_sums_close(got, ref, p.numel())


# ---- 5. mask dtypes ----------------------------------------------------------------------------------
def test_mask_dtypes_agree():
    p, m, u = rand_case(4099 + 1, 21)
    pd, ud = p.to(DEV), u.to(DEV)
    for sl in (slice(0, 4099), slice(1, 4100)):
        ref = restate(p[sl], m[sl], u[sl])
        base = None
        for dt in (torch.float32, torch.uint8, torch.bool, torch.int64):
            got = CAL.calib_hist(pd[sl], m.to(DEV).to(dt)[sl], ud[sl])
            assert_ints_equal(got, ref)
            if base is None:
                base = got
            assert torch.equal(got.conf_sum, base.conf_sum) and torch.equal(got.sums, base.sums)
    # other dtypes are converted: fp64 probabilities, fp16 mask, a non-dense view
    got = CAL.calib_hist(p.double().to(DEV)[:4096].view(64, 64).t(), m.half().to(DEV)[:4096].view(64, 64).t(),
                         u.to(DEV)[:4096].view(64, 64).t())
    assert_ints_equal(got, restate(p[:4096], m[:4096], u[:4096]))


# ---- 6. fp64 sums, reproducibility -------------------------------------------------------------------
@pytest.mark.parametrize("nb", [15, 64])
@pytest.mark.parametrize("n", [1, 257, 40_000])
def test_fp64_sums_and_reproducibility(n, nb):
    p, m, u = rand_case(n, 31 + n)
    pd, md, ud = p.to(DEV), m.to(DEV), u.to(DEV)
    a = CAL.calib_hist(pd, md, ud, n_bins=nb)
    b = CAL.calib_hist(pd, md, ud, n_bins=nb)
    assert_sums_close(a, restate(p, m, u, nb), n)
    for k in ("conf_hist", "conf_sum", "rank_hist", "unc_hist", "sums", "invalid"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k          # bit-identical, fp64 included


def test_reproducible_across_sweeps(big_case):
    p, m, u, _ = big_case
    pd, md, ud = p.to(DEV), m.to(DEV), u.to(DEV)
    a, b = CAL.calib_hist(pd, md, ud), CAL.calib_hist(pd, md, ud)
    assert torch.equal(a.conf_sum, b.conf_sum) and torch.equal(a.sums, b.sums)


# ---- 7. accumulation ---------------------------------------------------------------------------------
def test_accumulation_equals_one_call():
    n = 9001
    p, m, u = rand_case(n, 41)
    pd, md, ud = p.to(DEV), m.to(DEV), u.to(DEV)
    h = 4502                                 # the second half starts on a misaligned element
    acc = CAL.calib_hist(pd[:h], md[:h], ud[:h], n_bins=16)
    ret = CAL.calib_hist(pd[h:], md[h:], ud[h:], out=acc)
    assert ret is acc
    ref = restate(p, m, u, 16)
    assert_ints_equal(acc, ref)
    assert_sums_close(acc, ref, n)
    whole = CAL.calib_hist(pd, md, ud, n_bins=16)
    assert torch.equal(whole.conf_hist, acc.conf_hist) and torch.equal(whole.unc_hist, acc.unc_hist)
    with pytest.raises(ValueError):
        CAL.calib_hist(pd, md, out=acc)      # started with an uncertainty map


# ---- 8. metrics ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,with_u", [(15, True), (64, True), (15, False)])
def test_metrics_match_restatement(nb, with_u):
    g = torch.Generator().manual_seed(51)
    n = 30_000
    t = torch.rand(n, generator=g) < 0.3
    p = torch.sigmoid(torch.randn(n, generator=g) * 1.5 + torch.where(t, 1.0, -1.5))
    u = -(p * p.clamp_min(1e-12).log() + (1 - p) * (1 - p).clamp_min(1e-12).log())
    c = CAL.calib_hist(p.to(DEV), t.to(DEV), u.to(DEV) if with_u else None, n_bins=nb)
    got = CAL.calib_metrics(c)
    assert set(got) == set(CAL.SCALAR_NAMES) | {"reliability", "sparsification"}
    assert_metrics_close(got, metrics_ref(c))
    assert float(got["n"]) == n and float(got["positives"]) == int(t.sum())
    if with_u:
        assert 0 <= float(got["ause"]) < 0.5 and float(got["n_uncertainty"]) == n
    else:
        assert math.isnan(float(got["ause"])) and bool(torch.isnan(got["sparsification"]).all())


def test_metrics_closed_forms():
    n = 4000
    p = torch.full((n,), 0.25, device=DEV)
    t = (torch.arange(n, device=DEV) % 4 == 0)
    r = CAL.calib_metrics(CAL.calib_hist(p, t))
    assert float(r["ece"]) == 0.0 and float(r["mce"]) == 0.0 and float(r["brier"]) == 0.1875
    assert abs(float(r["nll"]) + (0.25 * math.log(0.25) + 0.75 * math.log(0.75))) < 1e-12
    assert float(r["auroc"]) == 0.5 and float(r["auroc_tie_bound"]) == 0.5     # one tie group
    assert float(r["auprc"]) == 0.25
    r = CAL.calib_metrics(CAL.calib_hist(torch.ones(n, device=DEV), torch.zeros(n, device=DEV)))
    assert float(r["ece"]) == 1.0 and float(r["mce"]) == 1.0 and float(r["brier"]) == 1.0
    assert math.isnan(float(r["auroc"])) and math.isnan(float(r["auprc"]))      # P == 0
    assert math.isnan(float(r["auroc_tie_bound"]))
    rel = r["reliability"].cpu()
    assert rel[14].tolist() == [float(n), 0.0, 1.0] and float(rel[:14].abs().sum()) == 0.0


def test_auroc_of_hard_sample_means_is_exact():
    g = torch.Generator().manual_seed(61)
    n = 20_000
    t = torch.rand(n, generator=g) < 0.2
    hits = torch.rand(8, n, generator=g) < torch.where(t, 0.7, 0.2)
    p = hits.float().mean(0)                 # values k / 8: every occupied rank bin holds one score
    r = CAL.calib_metrics(CAL.calib_hist(p.to(DEV), t.to(DEV)))
    exact = float(exact_auroc(p, t))
    assert abs(float(r["auroc"]) - exact) <= 1e-12
    # nine scores, nine occupied rank bins: a bin is exactly one tie group of the exact AUROC
    assert torch.unique(bin_index(p, f32(R), R)).numel() == torch.unique(p).numel() == 9
    # auroc_tie_bound is sum_b pos_b neg_b / (2 P Q) as defined: it cannot tell one repeated score from
    # several scores in a bin, so it is NOT 0 here although the estimate is exact
    ref = metrics_ref(restate(p, t))
    assert abs(float(r["auroc_tie_bound"]) - float(ref["auroc_tie_bound"])) <= 1e-12
    assert abs(float(r["auroc"]) - exact) <= float(r["auroc_tie_bound"])


def test_auroc_tie_bound_holds_on_continuous_scores():
    g = torch.Generator().manual_seed(62)
    n = 50_000
    t = torch.rand(n, generator=g) < 0.3
    p = torch.sigmoid(torch.randn(n, generator=g) + torch.where(t, 1.0, -1.0))
    ref = metrics_ref(restate(p, t))
    exact = float(exact_auroc(p, t))
    assert float(ref["auroc_tie_bound"]) < 0.01                       # a condition on the input
    assert abs(float(ref["auroc"]) - exact) <= float(ref["auroc_tie_bound"])
    r = CAL.calib_metrics(CAL.calib_hist(p.to(DEV), t.to(DEV)))
    assert 0 < float(r["auroc_tie_bound"]) < 0.01
    assert abs(float(r["auroc"]) - exact) <= float(r["auroc_tie_bound"])


def test_sparsification_closed_forms():
    g = torch.Generator().manual_seed(63)
    n = 10_000
    t = torch.rand(n, generator=g) < 0.4
    wrong = torch.rand(n, generator=g) < 0.1
    p = torch.where(t ^ wrong, 0.9, 0.1)     # hard prediction wrong exactly where `wrong`
    # u orders the errors perfectly: every error above every correct pixel
    u = torch.where(wrong, 0.5 + 0.1 * torch.rand(n, generator=g), 0.3 * torch.rand(n, generator=g))
    r = CAL.calib_metrics(CAL.calib_hist(p.to(DEV), t.to(DEV), u.to(DEV)))
    E = int(wrong.sum())
    assert float(r["uncertainty_errors"]) == E and float(r["n_uncertainty"]) == n
    sp = r["sparsification"].cpu()
    widest = float((sp[1:, 0] - sp[:-1, 0]).max())
    assert 0.0 <= float(r["ause"]) <= widest
    assert sp[0].tolist() == [0.0, E / n, E / n] and sp[-1].tolist() == [1.0, 0.0, 0.0]
    # constant u: one occupied bin, the curve has its two end points only
    r = CAL.calib_metrics(CAL.calib_hist(p.to(DEV), t.to(DEV), torch.full((n,), 0.2, device=DEV)))
    sp = r["sparsification"].cpu()
    assert sp[0].tolist() == [0.0, E / n, E / n]
    assert set(sp[:, 0].tolist()) == {0.0, 1.0} and sp[-1].tolist() == [1.0, 0.0, 0.0]
    k = int((sp[:, 0] == 0).sum())           # rows before the occupied bin is removed
    assert bool((sp[:k] == sp[0]).all()) and bool((sp[k:] == sp[-1]).all())


# ---- 9. meter, dispatcher op ------------------------------------------------------------------------------
def _meter_batches():
    out = []
    for i, shape in enumerate([(2, 1, 33, 31), (1, 1, 64, 48), (3, 1, 17, 19)]):
        n = shape[0] * shape[2] * shape[3]
        p, m, u = rand_case(n, 71 + i)
        out.append((p.view(shape), m.view(shape).to(torch.uint8), u.view(shape)))
    return out


def test_meter_equals_one_shot_and_resets():
    batches = _meter_batches()
    meter = CAL.CalibrationMeter(n_bins=16)
    for p, m, u in batches:
        meter.update(p.to(DEV), m.to(DEV), u.to(DEV))
    assert meter.updates == 3
    cat = [torch.cat([b[i].flatten() for b in batches]) for i in range(3)]
    ref = restate(*cat, nb=16)
    assert_ints_equal(meter.counts(), ref)
    assert_sums_close(meter.counts(), ref, cat[0].numel())
    one = CAL.calib_hist(*[c.to(DEV) for c in cat], n_bins=16)
    assert torch.equal(one.rank_hist, meter.counts().rank_hist)
    got = meter.compute()
    assert_metrics_close(got, metrics_ref(meter.counts()))
    assert_metrics_close(got, {k: v.cpu() for k, v in CAL.calib_metrics(one).items()}, tol=1e-12)
    meter.reset()
    with pytest.raises(RuntimeError):
        meter.compute()
    p, m, u = batches[0]
    meter.update(p.to(DEV), m.to(DEV))       # a fresh start, now without an uncertainty map
    ref = restate(p, m, None, 16)
    assert_ints_equal(meter.counts(), ref)


def test_meter_update_does_not_synchronise():
    dev = [tuple(t.to(DEV) for t in b) for b in _meter_batches()]
    meter = CAL.CalibrationMeter()
    meter.update(*dev[0])                    # first use: library load, state allocation
    meter.compute()
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
            for b in dev[1:]:
                meter.update(*b)
            meter.compute()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not enforced:
        pytest.skip("this torch build does not enforce torch.cuda.set_sync_debug_mode('error') "
                    "(a .item() did not raise), so the absence of host syncs cannot be asserted")
    cat = [torch.cat([b[i].flatten() for b in _meter_batches()]) for i in range(3)]
    assert_ints_equal(meter.counts(), restate(*cat))


def test_dispatcher_op():
    p, m, u = rand_case(3 * 37 * 29, 81)
    pd, md, ud = p.view(3, 1, 37, 29).to(DEV), m.view(3, 1, 37, 29).bool().to(DEV), u.view(3, 1, 37, 29).to(DEV)
    op = torch.ops.vaeunet.calib_hist
    names = ("conf_hist", "conf_sum", "rank_hist", "unc_hist", "sums", "invalid")
    for args, kw in (((pd, md, ud), {"n_bins": 16}), ((pd, md), {})):
        out = dict(zip(names, op(*args, **kw)))
        direct = CAL.calib_hist(*args, **kw)
        for k in names:
            d = getattr(direct, k)
            if d is None:
                assert out[k].shape == (0, 2)
            else:
                assert torch.equal(out[k], d), k
        torch.library.opcheck(op.default, args, kw, test_utils=("test_schema", "test_faketensor",
                                                                "test_autograd_registration"))


# ---- 10. end to end --------------------------------------------------------------------------------------
def test_end_to_end_from_sampling_inference():
    from golden_util import INFER_SEED, infer_inputs, pyramid_encoder, seed_bn_stats, seed_vae_tail
    from vaeunet_amd import UNetResNet, inference as I
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = UNetResNet(3, 1, pretrained=False, latent_injection="all")
    seed_vae_tail(model, INFER_SEED)
    seed_bn_stats(model, INFER_SEED + 50)
    model.encoder = pyramid_encoder(INFER_SEED)
    model = model.to(DEV).eval()
    img = torch.from_numpy(infer_inputs()["full_img"]).to(DEV)
    segs, _, _ = I.segmentation_distribution(model, img, num_samples=4)
    unc = I.calculate_uncertainty_metrics(segs)
    g = torch.Generator().manual_seed(91)
    mask = (torch.rand(unc["mean"].shape, generator=g) < 0.3).to(DEV)
    meter = CAL.CalibrationMeter()
    meter.update(unc["mean"], mask, unc["entropy"])
    ref = restate(unc["mean"], mask, unc["entropy"])
    assert_ints_equal(meter.counts(), ref)
    assert_sums_close(meter.counts(), ref, mask.numel())
    ref_metrics = metrics_ref({**ref, "conf_sum": meter.counts().conf_sum, "sums": meter.counts().sums})
    assert_metrics_close(meter.compute(), ref_metrics)
    assert int(ref["invalid"].sum()) == 0 and int(ref["conf_hist"].sum()) == mask.numel()
