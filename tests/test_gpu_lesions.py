"""The lesion-level evaluation (vaeunet_amd/csrc/ccl.hip, vaeunet_amd/lesions.py,
DESIGN.md §4.11) on the GPU against the numpy restatement in
tests/lesions_ref.py.  Every result is an integer or a deterministic function
of integers: labels, areas, masks, counts and histograms are compared
EXACTLY; the fp64 curve within one ulp.

Shapes: 1 x 1, 1 x 70, 70 x 1, 67 x 131, 129 x 257 and 31 x 63, 32 x 64,
33 x 65 (the 32-row, 64-column tile of the labelling kernel, -1 / 0 / +1 in
each dimension).  Planes: lesions_ref.adversarial_planes.  The labelling runs
through the C ABI on guarded buffers: the input comes back unchanged and no
guard element is written."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import lesions_ref as LR
import ref_small as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
INVALID = 1   # hipErrorInvalidValue

SHAPES = [(1, 1), (1, 70), (70, 1), (67, 131), (129, 257), (31, 63), (32, 64), (33, 65)]
KINDS = ["background", "foreground", "checkerboard", "serpentine", "U", "comb", "diagonal", "antidiagonal"] + \
        [f"bernoulli{p}" for p in LR.BERNOULLI_P]
THR = np.float32(0.5)


def _L():
    import vaeunet_amd.lesions as L
    return L


@functools.lru_cache(maxsize=None)
def _planes(H, W):
    out = LR.adversarial_planes(H, W)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(H, W, kind, conn):
    """the reference labels of one plane: computed once, shared, read-only"""
    lab = LR.label_plane(_planes(H, W)[kind] != 0, conn)
    lab.setflags(write=False)
    return lab


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


def _label_raw(x, conn, threshold=0.5, counts=True):
    """vu_ccl_label on guarded buffers -> (labels, ncomp) numpy; the input bitwise unchanged, no guard written"""
    from vaeunet_amd import _lib as L
    B, C, H, W = x.shape
    tdt = torch.float32 if x.dtype == np.float32 else torch.uint8
    dx, gx = R.guarded(x.shape, tdt, DEV)
    dx.copy_(torch.from_numpy(np.array(x)))
    lab, gl = R.guarded(x.shape, torch.int32, DEV)
    nc, gn = R.guarded((B, C), torch.int64, DEV)
    L.call("vu_ccl_label", L.ptr(dx), L.VU_CCL_F32 if tdt == torch.float32 else L.VU_CCL_U8, float(threshold), B * C, H,
           W, conn, L.ptr(lab), L.ptr(nc) if counts else None, L.stream())
    torch.cuda.synchronize()
    for g in (gx, gl, gn):
        g.check("vu_ccl_label")
    back = dx.cpu().numpy()
    assert np.array_equal(back.view(np.uint8), np.ascontiguousarray(x).view(np.uint8))
    return lab.cpu().numpy(), nc.cpu().numpy()


# ----------------------------------------------------------------------------
# labels
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("HW", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_labels_are_bitwise_the_reference(HW, kind, conn):
    H, W = HW
    plane, want = _planes(H, W)[kind], _want(H, W, kind, conn)
    k = len(np.unique(want[want > 0]))
    for x in (plane[None, None], _as_prob(plane, H * 1000 + W)[None, None]):
        got, nc = _label_raw(x, conn)
        assert got.dtype == np.int32 and np.array_equal(got[0, 0], want), (kind, x.dtype)
        assert nc.tolist() == [[k]]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("first", [0, 6])
def test_labels_of_a_batch_of_planes(first, conn):
    """[2, 3, 67, 131]: six different planes per case, every kind over the two cases; planes do not interact"""
    H, W = 67, 131
    kinds = [KINDS[(first + j) % len(KINDS)] for j in range(6)]
    x = np.stack([_planes(H, W)[k] for k in kinds]).reshape(2, 3, H, W)
    want = np.stack([_want(H, W, k, conn) for k in kinds]).reshape(2, 3, H, W)
    for inp in (x, _as_prob(x, first)):
        got, nc = _label_raw(inp, conn)
        assert np.array_equal(got, want)
        assert nc.reshape(-1).tolist() == [len(np.unique(w[w > 0])) for w in want.reshape(6, H, W)]


def test_adjacent_planes_do_not_join_and_the_api_matches_the_c_abi():
    L = _L()
    x = np.zeros((2, 2, 33, 65), np.uint8)
    x[:, :, -1, :] = 1                       # the last row of every plane ...
    x[:, :, 0, :] = 1                        # ... and the first row of the next
    want, n = LR.label(x, 8)
    assert n.tolist() == [[2, 2], [2, 2]]
    d = torch.from_numpy(x).to(DEV)
    for inp in (d, d.bool()):
        lab, nc = L.label_components(inp, return_counts=True)
        assert lab.dtype == torch.int32 and nc.dtype == torch.int64
        assert np.array_equal(lab.cpu().numpy(), want) and np.array_equal(nc.cpu().numpy(), n)
    # a non-contiguous input is densified, not misread
    wide = torch.zeros(2, 2, 33, 130, dtype=torch.uint8, device=DEV)
    wide[..., ::2] = d
    assert torch.equal(L.label_components(wide[..., ::2]), lab)
    assert torch.equal(L.label_components(d, connectivity=4), torch.from_numpy(LR.label(x, 4)[0]).to(DEV))


def test_nan_and_the_threshold_itself_are_background_and_two_runs_are_equal():
    L = _L()
    H, W = 67, 131
    fg = _planes(H, W)["bernoulli0.5"]
    p = _as_prob(fg, 3)
    assert np.isnan(p).sum() > 100 and (p == THR).sum() > 100
    d = torch.from_numpy(p[None, None]).to(DEV)
    a = L.label_components(d, threshold=0.5)
    b = L.label_components(d, threshold=0.5)
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy()[0, 0], _want(H, W, "bernoulli0.5", 8))
    # another threshold is another foreground
    want, _ = LR.label(p[None, None], 8, 0.75)
    assert np.array_equal(L.label_components(d, threshold=0.75).cpu().numpy(), want)
    # the u8 rule ignores the threshold
    u = torch.from_numpy(fg[None, None] * 200).to(DEV)
    assert torch.equal(L.label_components(u, threshold=250.0), a)


def test_labels_past_2_to_the_31_elements():
    """two planes of 46340 x 46340 (H W = 2^31 - 88,048 <= 2^31 - 2): offsets across planes need 64 bits and the labels
    of the last rows are the largest int32 values the kernel forms"""
    L = _L()
    H = W = 46340
    n = H * W
    assert n <= 2 ** 31 - 2 < 2 * n
    x = torch.zeros(1, 2, H, W, dtype=torch.uint8, device=DEV)
    x[0, 1, H - 2:, W - 3:] = 1              # 2 x 3 block in the last corner of the last plane
    x[0, 1, 0, 0] = 1
    x[0, 0, H - 1, W - 1] = 1                # next to plane 1's first pixel in memory: they must not join
    x[0, 0, 31:33, 63:65] = 1                # across a tile corner
    lab, nc = L.label_components(x, return_counts=True)
    assert nc.tolist() == [[2, 2]]
    assert int(lab.count_nonzero()) == 6 + 1 + 1 + 4
    first = (H - 2) * W + W - 3 + 1
    assert lab[0, 1, H - 2:, W - 3:].unique().tolist() == [first] and first > 2 ** 31 - 2 ** 18
    assert int(lab[0, 1, 0, 0]) == 1 and int(lab[0, 0, H - 1, W - 1]) == n
    assert lab[0, 0, 31:33, 63:65].unique().tolist() == [31 * W + 63 + 1]
    del lab, x
    torch.cuda.empty_cache()


def test_c_abi_rejections():
    from vaeunet_amd import _lib as L
    x = torch.zeros(1, 1, 8, 8, dtype=torch.uint8, device=DEV)
    lab = torch.zeros(1, 1, 8, 8, dtype=torch.int32, device=DEV)
    ws = torch.zeros(4 * 64, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(4, dtype=torch.int64, device=DEV)
    q = lambda name, *a: L.query(name, *a)   # noqa: E731
    s = L.stream()
    for args in ((L.ptr(x), 0, 0.5, 1, 8, 8, 6, L.ptr(lab), None, s),
                 (L.ptr(x), 2, 0.5, 1, 8, 8, 8, L.ptr(lab), None, s),
                 (L.ptr(x), 0, 0.5, -1, 8, 8, 8, L.ptr(lab), None, s), (None, 0, 0.5, 1, 8, 8, 8, L.ptr(lab), None, s),
                 (L.ptr(x), 0, 0.5, 1, 8, 8, 8, None, None, s),
                 (L.ptr(x), 0, 0.5, 1, 46341, 46341, 8, L.ptr(lab), None, s)):
        assert q("vu_ccl_label", *args) == INVALID
    assert q("vu_ccl_label", L.ptr(x), 0, 0.5, 0, 8, 8, 8, L.ptr(lab), None, s) == 0
    assert q("vu_ccl_workspace_bytes", 3, 5, 7) == 4 * 4 * 105 and q("vu_ccl_workspace_bytes", 1, 46341, 46341) == -1
    assert q("vu_ccl_remove_small", L.ptr(lab), 1, 8, 8, 0, L.ptr(x), None, L.ptr(ws), s) == INVALID
    assert q("vu_ccl_remove_small", L.ptr(lab), 1, 8, 8, 1, None, None, L.ptr(ws), s) == INVALID
    assert q("vu_lesion_match", L.ptr(lab), L.ptr(lab), None, 0, 1, 8, 8, 0, 10, L.ptr(cnt), None, None, L.ptr(ws), s) \
        == INVALID
    assert q("vu_lesion_match", L.ptr(lab), L.ptr(lab), None, 1, 1, 8, 8, 1, 10, L.ptr(cnt), None, None, L.ptr(ws), s) \
        == INVALID                                  # a float32 prediction without its values
    assert q("vu_lesion_match", L.ptr(lab), L.ptr(lab), None, 0, 1, 8, 8, 1, 0, L.ptr(cnt), L.ptr(cnt), L.ptr(cnt),
             L.ptr(ws), s) == INVALID               # no bins
    torch.cuda.synchronize()
    assert int(lab.abs().sum()) == 0 and int(x.sum()) == 0
    # labels that are no labels of the plane count as background: no table address outside the plane
    Lm = _L()
    wild = torch.zeros(1, 1, 8, 8, dtype=torch.int32, device=DEV)       # n = 64: 65 = n + 1 is no label, 64 is one
    wild[0, 0, :2, :4] = torch.tensor([[2 ** 31 - 1, -5, 65, 64], [1, 1, 0, 9]], dtype=torch.int32, device=DEV)
    assert Lm.component_areas(wild)[0, 0, :2, :4].tolist() == [[0, 0, 0, 1], [2, 2, 0, 1]]


# ----------------------------------------------------------------------------
# areas, small components
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("p", LR.BERNOULLI_P)
def test_areas_and_remove_small_are_bitwise_the_reference(p, conn):
    L = _L()
    H, W = 67, 131
    plane = _planes(H, W)[f"bernoulli{p}"]
    x = np.stack([plane, plane[::-1].copy()])[None]              # [1, 2, H, W]
    lab, _ = LR.label(x, conn)
    area = LR.areas(lab)
    d = torch.from_numpy(x).to(DEV)
    dl = L.label_components(d, connectivity=conn)
    got = L.component_areas(dl)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), area)
    prob = torch.from_numpy(_as_prob(x, 11)).to(DEV)
    for min_area in (1, 2, 5, 10 ** 6):
        want = ((lab > 0) & (area >= min_area)).astype(np.uint8)
        assert np.array_equal(want, LR.remove_small(x, min_area, conn))
        for inp, kw in ((d, {}), (prob, dict(threshold=0.5))):
            m = L.remove_small_components(inp, min_area, connectivity=conn, **kw)
            assert m.dtype == torch.uint8 and np.array_equal(m.cpu().numpy(), want), (min_area, inp.dtype)


# ----------------------------------------------------------------------------
# counts
# ----------------------------------------------------------------------------
def _rect(a, y0, y1, x0, x1):
    a[y0:y1, x0:x1] = 1


@functools.lru_cache(maxsize=None)
def _pairs():
    """(pred uint8, pred float32, gt uint8) [2, 2, 40, 150]: shifted, partially overlapping blobs over tile edges"""
    H, W = 40, 150
    pred, gt = np.zeros((2, 2, H, W), np.uint8), np.zeros((2, 2, H, W), np.uint8)
    p, g = pred[0, 0], gt[0, 0]
    _rect(g, 2, 5, 2, 6); _rect(g, 2, 5, 10, 14); _rect(p, 3, 4, 4, 12)         # a candidate that touches two lesions
    _rect(g, 10, 20, 60, 70); _rect(p, 9, 12, 58, 62); _rect(p, 18, 22, 66, 72)  # a lesion touched by two candidates
    _rect(g, 30, 34, 100, 104); _rect(p, 31, 32, 101, 103)    # a lesion touched only by a candidate of 2 pixels
    _rect(p, 36, 39, 20, 23); p[0, 149] = 1                   # false positives: 9 pixels, 1 pixel
    _rect(g, 25, 27, 140, 143)                                # a missed lesion
    _rect(p, 30, 35, 62, 66); _rect(g, 33, 36, 65, 68)        # one overlap pixel pair across the tile corner (32, 64)
    _rect(pred[0, 1], 5, 9, 5, 9); pred[0, 1, 20, 20] = 1     # an empty ground truth
    _rect(gt[1, 0], 5, 9, 5, 9); gt[1, 0, 39, 149] = 1        # an empty prediction
    rng = np.random.Generator(np.random.PCG64(5))
    pred[1, 1] = rng.random((H, W)) < 0.25
    gt[1, 1] = rng.random((H, W)) < 0.25
    prob = _as_prob(pred, 21)
    for a in (pred, gt, prob):
        a.setflags(write=False)
    return pred, prob, gt


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("min_area", [1, 3])
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_lesion_counts_are_exactly_the_reference(dtype, min_area, conn):
    L = _L()
    pred, prob, gt = _pairs()
    x = pred if dtype == "u8" else prob
    want, _, _ = LR.match(x, gt, 0.5, min_area, conn, 10)
    if conn == 8:   # the scenarios are what their comments say
        assert want[0, 0].tolist() == ([6, 5, 7, 2] if min_area == 1 else [6, 4, 5, 1])
        assert want[0, 1].tolist() == ([0, 0, 2, 2] if min_area == 1 else [0, 0, 1, 1])
        assert want[1, 0].tolist() == [2, 0, 0, 0]
    for masks in (gt, gt.astype(np.float32), gt.astype(bool), gt.astype(np.int64)):
        got = L.lesion_counts(torch.from_numpy(np.array(x)).to(DEV), torch.from_numpy(np.array(masks)).to(DEV),
                              threshold=0.5, min_area=min_area, connectivity=conn)
        assert got.dtype == torch.int64 and got.shape == (2, 2, 4)
        assert np.array_equal(got.cpu().numpy(), want), masks.dtype


# ----------------------------------------------------------------------------
# the meter
# ----------------------------------------------------------------------------
def _meter_batches():
    """three (pred float32, gt uint8) batches of different shapes, two classes; scores of exactly 1.0 and exactly
    the first float above the threshold among the candidates' maxima"""
    out = []
    lo = np.nextafter(THR, np.float32(1))
    for i, (B, H, W) in enumerate(((1, 40, 150), (2, 33, 65), (3, 20, 20))):
        rng = np.random.Generator(np.random.PCG64(100 + i))
        pred = (rng.random((B, 2, H, W)) < 0.006).astype(np.uint8)
        big = pred & (rng.random(pred.shape) < 0.6)                          # most candidates grow to 2 x 2 pixels
        pred[..., :, 1:] |= big[..., :, :-1]
        pred[..., 1:, :] |= big[..., :-1, :]
        pred[..., 1:, 1:] |= big[..., :-1, :-1]
        gt = (rng.random((B, 2, H, W)) < 0.02).astype(np.uint8)
        gt |= (pred & (rng.random(pred.shape) < 0.4)).astype(np.uint8)      # many overlaps
        prob = _as_prob(pred, 200 + i)
        # isolated two-pixel candidates with the edge scores, one on and one off the ground truth each
        gt[:, :, 0:4, 0:9] = 0
        prob[:, :, 0:4, 0:9] = 0.1
        prob[:, :, 1:3, 1] = 1.0; gt[:, :, 1, 1] = 1
        prob[:, :, 1:3, 3] = 1.0
        prob[:, :, 1:3, 5] = lo; gt[:, :, 1, 5] = 1
        prob[:, :, 1:3, 7] = lo
        out.append((prob, gt))
    return out


def _ulp_close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - want) <= np.spacing(np.abs(want))
    return bool((ok | both_nan).all())


@pytest.mark.parametrize("bins", [1000, 7])
@pytest.mark.parametrize("min_area", [1, 2])
def test_meter_accumulates_exactly_and_the_curve_is_within_one_ulp(bins, min_area):
    L = _L()
    meter = L.LesionMeter(threshold=0.5, min_area=min_area, connectivity=8, bins=bins)
    total = np.zeros((2, 4), np.int64)
    hf, hg, planes = np.zeros(bins, np.int64), np.zeros(bins, np.int64), 0
    for prob, gt in _meter_batches():
        meter.update(torch.from_numpy(prob).to(DEV), torch.from_numpy(gt).to(DEV))
        c, f, g = LR.match(prob, gt, 0.5, min_area, 8, bins)
        total += c.sum(0)
        hf += f
        hg += g
        planes += prob.shape[0] * 2
    assert meter.n_planes == planes == 12
    assert np.array_equal(meter.counts().cpu().numpy(), total)
    ghf, ghg = (h.cpu().numpy() for h in meter.histograms())
    assert np.array_equal(ghf, hf) and np.array_equal(ghg, hg)
    assert hf[-1] >= 6 and hg[-1] >= 6 and hf[bins // 2] >= 6 and hg[bins // 2] >= 6      # both edge scores, both sides
    assert int(hf.sum()) == int(total[:, 3].sum()) and int(hg.sum()) == int(total[:, 1].sum())
    sens, fppi, score = LR.froc(hf, hg, int(total[:, 0].sum()), planes)
    gs, gf, gsc = meter.froc()
    assert gs.dtype == gf.dtype == gsc.dtype == torch.float64 and gs.shape == gf.shape == (bins,)
    assert _ulp_close(gs.cpu().numpy(), sens) and _ulp_close(gf.cpu().numpy(), fppi)
    assert 0 < score < 1 and len(np.unique(sens)) > 3 and _ulp_close(gsc.item(), score)
    vals = meter.values().cpu().numpy()
    want = LR.metrics(total, planes)
    assert vals.dtype == np.float32 and (np.abs(vals.astype(np.float64) - want) <= np.spacing(want)).all()
    res = meter.compute()
    assert set(res) == {"sensitivity", "precision", "fp_per_image", "froc"} and res["froc"].item() == gsc.item()
    # lesion_metrics of a per-plane table pools it
    prob, gt = _meter_batches()[1]
    c = L.lesion_counts(torch.from_numpy(prob).to(DEV), torch.from_numpy(gt).to(DEV), min_area=min_area)
    w = LR.metrics(LR.match(prob, gt, 0.5, min_area, 8, 1)[0])
    assert (np.abs(L.lesion_metrics(c).cpu().numpy().astype(np.float64) - w) <= np.spacing(w)).all()
    meter.reset()
    with pytest.raises(RuntimeError):
        meter.counts()


def test_meter_without_ground_truth_gives_nan_sensitivities_and_hard_masks_score_one():
    L = _L()
    meter = L.LesionMeter(bins=10)
    pred = np.zeros((1, 1, 9, 9), np.uint8)
    pred[0, 0, 1:3, 1:3] = 1
    pred[0, 0, 6, 6] = 1
    meter.update(torch.from_numpy(pred).to(DEV).bool(), torch.zeros(1, 1, 9, 9, device=DEV))
    assert meter.counts().tolist() == [[0, 0, 2, 2]]
    hf, hg = meter.histograms()
    assert hf.tolist() == [0] * 9 + [2] and hg.tolist() == [0] * 10
    sens, fppi, score = meter.froc()
    assert torch.isnan(sens).all() and torch.isnan(score) and fppi.tolist() == [2.0] * 10
    with pytest.raises(ValueError):
        meter.update(torch.zeros(1, 2, 9, 9, dtype=torch.uint8, device=DEV), torch.zeros(1, 2, 9, 9, device=DEV))


# ----------------------------------------------------------------------------
# evaluate
# ----------------------------------------------------------------------------
class _Net(nn.Module):
    """logits = an affine map of the first image channel: both predictions occur, no value near the threshold"""

    def forward(self, x):
        return (torch.round(x[:, :1] * 8) / 8 - 0.4375) * 4


def test_evaluate_with_a_lesion_meter_and_without():
    from vaeunet_amd.evaluate import evaluate, evaluate_with_lesions
    from vaeunet_amd.metrics import METRIC_NAMES, seg_counts
    L = _L()
    g = torch.Generator().manual_seed(3)
    batches = []
    for B in (2, 1):
        image = torch.nn.functional.interpolate(torch.rand(B, 3, 12, 12, generator=g), size=(48, 48), mode="nearest")
        mask = torch.nn.functional.interpolate((torch.rand(B, 1, 16, 16, generator=g) < 0.2).float(), size=(48, 48),
                                               mode="nearest")
        batches.append({"image": image, "mask": mask})
    net = _Net().to(DEV)
    plain = evaluate(net, batches, DEV)
    assert set(plain) == set(METRIC_NAMES) | {f"pooled_{k}" for k in METRIC_NAMES} | {"batches"}
    meter = L.LesionMeter(min_area=2)
    res = evaluate_with_lesions(net, batches, DEV, meter)
    assert {k: res[k] for k in plain} == plain
    assert set(res) - set(plain) == {"lesion_sensitivity", "lesion_precision", "lesion_fp_per_image", "lesion_n_gt",
                                     "lesion_n_pred"}
    total = torch.zeros(4, dtype=torch.int64, device=DEV)
    for b in batches:
        image, mask = b["image"].to(DEV), b["mask"].to(DEV)
        hard = torch.empty(mask.shape, dtype=torch.uint8, device=DEV)
        seg_counts(net(image), mask, hard_mask=hard)
        assert 0 < int(hard.sum()) < hard.numel()
        total += L.lesion_counts(hard, mask, min_area=2).sum((0, 1))
    want = L.lesion_metrics(total[None], n_planes=3).cpu().tolist()
    assert [res["lesion_sensitivity"], res["lesion_precision"], res["lesion_fp_per_image"]] == want
    assert (res["lesion_n_gt"], res["lesion_n_pred"]) == (int(total[0]), int(total[2])) and res["lesion_n_gt"] > 0
    assert isinstance(res["lesion_n_gt"], int) and isinstance(res["lesion_sensitivity"], float)
    assert meter.n_planes == 3


# ----------------------------------------------------------------------------
# ops
# ----------------------------------------------------------------------------
def test_ops_equal_the_python_functions():
    import vaeunet_amd.ops  # noqa: F401
    L = _L()
    plane = _planes(67, 131)["bernoulli0.4073"]
    u = torch.from_numpy(np.array(plane[None, None])).to(DEV)
    p = torch.from_numpy(_as_prob(plane, 9)[None, None]).to(DEV)
    for conn in (4, 8):
        assert torch.equal(torch.ops.vaeunet.label_components(u, conn), L.label_components(u, conn))
        assert torch.equal(torch.ops.vaeunet.label_components(p, conn, 0.5), L.label_components(p, conn, 0.5))
        assert torch.equal(torch.ops.vaeunet.remove_small_components(u, 4, conn), L.remove_small_components(u, 4, conn))
        assert torch.equal(torch.ops.vaeunet.remove_small_components(p, 4, conn, 0.5),
                           L.remove_small_components(p, 4, conn, 0.5))
    assert torch.equal(torch.ops.vaeunet.label_components(u), L.label_components(u))
    with pytest.raises(ValueError):
        torch.ops.vaeunet.label_components(p)
