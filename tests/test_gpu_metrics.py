"""Device-side validation metrics (vaeunet_amd.metrics: seg_counts,
seg_metrics, get_all_metrics, SegmentationMeter; csrc/metrics.hip) against a
torch restatement on the CPU: F.interpolate in fp64, ``> 0.5``, integer sums;
the metric formulas are evaluated in numpy.

Counts are integers, so every comparison of counts is exact.  Where the
logits are resized, exactness needs the fp32 interpolation in the kernel and
the fp64 interpolation of the reference to fall on the same side of 0.5: the
tests use inputs where the arithmetic is exact in fp32, or assert first that
no reference value lies within 1e-4 of the threshold (torch's own fp32
interpolation differs from fp64 by at most 3.2e-6 on these inputs)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vaeunet_amd import metrics as M
from vaeunet_amd import ops  # noqa: F401  (registers the ops)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
EPS = 1e-6

SHAPES = [(1, 1, 7, 9), (3, 2, 33, 31), (2, 1, 64, 64)]
MASK_DTYPES = [torch.float32, torch.uint8, torch.bool, torch.int64]


# ---- the reference ------------------------------------------------------------------
def ref_values(logits, size, align_corners=False):
    """the logits at mask resolution, fp64 on the CPU"""
    x = logits.detach().cpu().double()
    if tuple(x.shape[2:]) != tuple(size):
        x = F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=align_corners)
    return x


def ref_counts(values, masks):
    """int64 [B, C, 4] = (TP, FP, FN, TN) per plane"""
    p = values > 0.5
    t = masks.detach().cpu().double() > 0.5
    return torch.stack([(p & t).sum((2, 3)), (p & ~t).sum((2, 3)), (~p & t).sum((2, 3)), (~p & ~t).sum((2, 3))],
                       dim=-1)


def ref_metrics(k, eps=EPS):
    """numpy: one (TP, FP, FN, TN) row -> the six metrics; dice in fp32 (the
    arithmetic of dice_score), the others in fp64 rounded once to fp32"""
    tp, fp, fn, tn = (int(v) for v in k)
    a, b = tp + fp, tp + fn
    f = np.float32
    dice = f(1.0) if a + b == 0 else (f(2.0) * f(tp) + f(eps)) / (f(a) + f(b) + f(eps))
    TP, FP, FN, TN = (np.float64(v) for v in (tp, fp, fn, tn))
    rest = [(TP + eps) / (TP + FP + FN + eps), (TP + eps) / (TP + FP + eps), (TP + eps) / (TP + FN + eps),
            (TN + eps) / (TN + FP + eps), (TP + TN) / (TP + FP + FN + TN)]
    return np.array([dice] + [f(v) for v in rest], dtype=np.float32)


def assert_metrics(got, k, what, dice_exact=True):
    """dice bit-exact, the fp64-formed columns within 1 fp32 ulp (the device's fp64 division)"""
    got = got.detach().cpu().numpy()
    ref = ref_metrics(k)
    if dice_exact:
        assert got[0] == ref[0], (what, got[0], ref[0])
    for i in range(1, 6):
        assert abs(np.float64(got[i]) - np.float64(ref[i])) <= np.spacing(ref[i]), (what, M.METRIC_NAMES[i], got[i],
                                                                                    ref[i])


@functools.lru_cache(maxsize=None)
def case1(shape, bf16):
    g = torch.Generator().manual_seed(1000 + shape[2])
    x = torch.randn(*shape, generator=g) * 3
    if bf16:
        x = x.bfloat16()
    m = (torch.rand(*shape, generator=g) < 0.3).float()
    return x, m, ref_counts(ref_values(x, shape[2:]), m)


def _layout(t, cl):
    return t.to(DEV).contiguous(memory_format=CL) if cl else t.to(DEV).contiguous()


def _counts(x, m, **kw):
    return M.seg_counts(x, m, **kw).cpu()


# ---- 1. no resize: bit-exact counts --------------------------------------------------
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_no_resize_exact(shape, bf16, cl):
    x, m, ref = case1(shape, bf16)
    assert torch.equal(ref.sum(-1), torch.full(ref.shape[:2], shape[2] * shape[3]))
    xd = _layout(x, cl)
    assert xd.dtype == (torch.bfloat16 if bf16 else torch.float32)
    for md in MASK_DTYPES:
        for mcl in (False, True):
            got = _counts(xd, _layout(m.to(md), mcl))
            assert got.dtype == torch.int64 and got.shape == ref.shape
            assert torch.equal(got, ref), (md, mcl, got.tolist(), ref.tolist())
            assert torch.equal(got.sum(-1), torch.full(ref.shape[:2], shape[2] * shape[3]))


def test_counts_strided_views_and_nan():
    """any strides are read in place (a cropped view of a larger tensor); NaN
    logits count as not predicted"""
    g = torch.Generator().manual_seed(7)
    big = torch.randn(2, 3, 20, 24, generator=g) * 3
    bm = (torch.rand(2, 3, 20, 24, generator=g) < 0.3).float()
    m = bm[:, 1:3, 3:16, 5:22]
    xs = big[:, 1:3, 3:16, 5:22].clone()
    xs[0, 0, 2, 3] = float("nan")
    xs[1, 1, 0, 0] = float("nan")
    bigd = big.to(DEV)
    bigd[:, 1:3, 3:16, 5:22] = xs.to(DEV)
    got = _counts(bigd[:, 1:3, 3:16, 5:22], bm.to(DEV)[:, 1:3, 3:16, 5:22])
    assert torch.equal(got, ref_counts(torch.nan_to_num(xs.double(), nan=-1.0), m))


# ---- 2. grid-stride path ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_case():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 1, 1100, 1000, generator=g) * 3
    m = (torch.rand(1, 1, 1100, 1000, generator=g) < 0.3).float()
    return x, m, ref_counts(x.double(), m)


def test_counts_grid_stride():
    """1.1 M pixels in one plane: more 1024-pixel steps than the stage-1 block cap"""
    x, m, ref = big_case()
    assert torch.equal(_counts(x.to(DEV), m.to(DEV)), ref)
    # the same through the scalar (any-stride) kernel: a channels_last view of two classes
    x2 = torch.stack([x[0, 0], -x[0, 0]], 0)[None]
    m2 = torch.stack([m[0, 0], m[0, 0]], 0)[None]
    got = _counts(_layout(x2, True), _layout(m2.to(torch.uint8), True))
    assert torch.equal(got[0, 0], ref[0, 0])
    assert torch.equal(got, ref_counts(x2.double(), m2))


# ---- 3. resize where fp32 is exact ---------------------------------------------------------
@pytest.mark.parametrize("shape,size", [((3, 2, 6, 9), (12, 18)), ((1, 1, 550, 500), (1100, 1000))],
                         ids=["small", "large"])
def test_counts_resize_exact_arithmetic(shape, size):
    """integer logits, 2x upscale, align_corners=False: the weights are 1/4 and
    3/4, every interpolated value is a multiple of 1/16 and exact in fp32 in any
    evaluation order; values exactly 0.5 occur and must classify as false"""
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-4, 5, shape, generator=g).float()
    m = (torch.rand(shape[0], shape[1], *size, generator=g) < 0.3).to(torch.uint8)
    v64 = ref_values(x, size)
    v32 = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    assert torch.equal(v32.double(), v64)
    assert int((v64 == 0.5).sum()) > 0
    ref = ref_counts(v64, m)
    for cl in (False, True):
        assert torch.equal(_counts(_layout(x, cl), m.to(DEV)), ref), cl


# ---- 4. resize in general ----------------------------------------------------------------------
def case4(size, align_corners, bf16=False):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 2, 5, 7, generator=g) * 3
    if bf16:
        x = x.bfloat16()
    m = (torch.rand(3, 2, *size, generator=g) < 0.3).float()
    v = ref_values(x, size, align_corners)
    # margin: at least 30x any fp32 evaluation-order error of the interpolation
    assert float((v - 0.5).abs().min()) > 1e-4
    return x, m, v


@pytest.mark.parametrize("align_corners", [False, True], ids=["ac0", "ac1"])
@pytest.mark.parametrize("size", [(8, 11), (10, 14), (3, 4)], ids=["8x11", "10x14", "3x4"])
def test_counts_resize_general(size, align_corners):
    x, m, v = case4(size, align_corners)
    ref = ref_counts(v, m)
    for cl in (False, True):
        for md in (torch.float32, torch.int64):
            got = _counts(_layout(x, cl), _layout(m.to(md), cl), align_corners=align_corners)
            assert torch.equal(got, ref), (cl, md, got.tolist(), ref.tolist())


def test_counts_resize_bf16_logits():
    x, m, v = case4((10, 14), False, bf16=True)
    assert torch.equal(_counts(x.to(DEV), m.to(DEV)), ref_counts(v, m))


# ---- 5. resize entry point at equal resolution ---------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_resize_identity_equals_streaming(shape):
    x, m, ref = case1(shape, False)
    for ac in (False, True):
        got = _counts(x.to(DEV), m.to(DEV), align_corners=ac, _resize=True)
        assert torch.equal(got, ref), ac


# ---- 6. metrics ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_metrics_vs_dice_score_and_numpy(shape, bf16):
    x, m, ref = case1(shape, bf16)
    xd, md = x.to(DEV), m.to(DEV)
    res = M.get_all_metrics(xd, md)
    assert list(res) == list(M.METRIC_NAMES)
    assert all(v.shape == () and v.dtype == torch.float32 and v.is_cuda for v in res.values())
    # pooled dice: bit-identical to the existing dice_score on the same tensors
    assert res["dice"].item() == M.dice_score(xd.float(), md.float()).item()
    pooled = ref.sum((0, 1))
    assert_metrics(torch.stack([res[k] for k in M.METRIC_NAMES]), pooled, "pooled")
    counts = M.seg_counts(xd, md)
    rows = M.seg_metrics(counts, pooled=False)
    assert rows.shape == (shape[0], shape[1], 6)
    for b in range(shape[0]):
        for c in range(shape[1]):
            assert_metrics(rows[b, c], ref[b, c], (b, c))
    # the single-metric entry points
    assert M.iou_score(xd, md).item() == res["iou"].item()
    p, r = M.precision_recall(xd, md)
    assert (p.item(), r.item()) == (res["precision"].item(), res["recall"].item())
    assert M.specificity(xd, md).item() == res["specificity"].item()
    assert M.accuracy(xd, md).item() == res["accuracy"].item()


@pytest.mark.parametrize("shape", [(2, 2, 9, 11), (1, 1, 16, 16)], ids=["planes", "single_plane"])
def test_metrics_degenerate_tables(shape):
    """empty denominators are eps / eps = 1 exactly ("empty means perfect", as dice_score)"""
    n = shape[2] * shape[3]
    zeros = torch.zeros(shape, device=DEV)
    low = torch.full(shape, 0.5, device=DEV)     # exactly the threshold: not predicted
    res = M.get_all_metrics(low, zeros)
    assert torch.equal(M.seg_counts(low, zeros).cpu(), torch.tensor([0, 0, 0, n]).expand(shape[0], shape[1], 4))
    assert all(v.item() == 1.0 for v in res.values()), res
    assert res["dice"].item() == M.dice_score(low, zeros).item()
    res = M.get_all_metrics(torch.full(shape, 3.0, device=DEV), torch.ones(shape, device=DEV))
    assert all(v.item() == 1.0 for v in res.values()), res
    rows = M.seg_metrics(M.seg_counts(low, zeros), pooled=False)
    assert torch.equal(rows.cpu(), torch.ones(shape[0], shape[1], 6))


# ---- 7. meter -----------------------------------------------------------------------------------------
def _meter_batches():
    g = torch.Generator().manual_seed(11)
    out = []
    for B in (3, 1, 2):
        x = torch.randn(B, 2, 12, 10, generator=g) * 3
        m = (torch.rand(B, 2, 24, 20, generator=g) < 0.3).to(torch.uint8)
        v = ref_values(x, (24, 20))
        assert float((v - 0.5).abs().min()) > 1e-4
        out.append((x, m, ref_counts(v, m)))
    return out


def test_meter_pooled_batch_mean_reset():
    batches = _meter_batches()
    meter = M.SegmentationMeter()
    for x, m, _ in batches:
        meter.update(_layout(x, True), m.to(DEV))
    allc = torch.cat([r for _, _, r in batches], 0)          # the concatenated tensors' counts
    assert torch.equal(meter.counts().cpu(), allc.sum(0))
    pooled = meter.compute("pooled")
    assert_metrics(torch.stack([pooled[k] for k in M.METRIC_NAMES]), allc.sum((0, 1)), "pooled")
    per_class = meter.per_class()
    assert per_class.shape == (2, 6)
    for c in range(2):
        assert_metrics(per_class[c], allc.sum(0)[c], f"class {c}")
    # batch_mean: the fp32 running sum of the three per-batch pooled rows, divided by 3
    rows = []
    for x, m, r in batches:
        row = M.seg_metrics(M.seg_counts(_layout(x, True), m.to(DEV)))
        assert_metrics(row, r.sum((0, 1)), "batch")
        rows.append(row.cpu().numpy().astype(np.float64))
    rows = np.stack(rows)
    mean = rows.mean(0)
    got = meter.compute("batch_mean")
    f = np.float32
    for i, k in enumerate(M.METRIC_NAMES):
        # 1 ulp (of the running sum) per fp32 addition -- 0 + v1 is exact -- and 1 ulp for the division
        tol = (np.spacing(f(rows[0, i] + rows[1, i])) + np.spacing(f(rows[:, i].sum()))) / 3 + np.spacing(f(mean[i]))
        assert abs(np.float64(got[k].item()) - mean[i]) <= tol, (k, got[k].item(), mean[i])
    assert meter.batches == 3
    meter.reset()
    assert meter.batches == 0
    with pytest.raises(RuntimeError):
        meter.compute()
    x, m, r = batches[1]
    meter.update(x.to(DEV), m.to(DEV))
    assert torch.equal(meter.counts().cpu(), r.sum(0))


def test_seg_counts_out_accumulates():
    batches = _meter_batches()
    x, m, r = batches[0]
    acc = M.seg_counts(x.to(DEV), m.to(DEV))
    same = M.seg_counts(x.to(DEV), m.to(DEV), out=acc)
    assert same is acc
    assert torch.equal(acc.cpu(), 2 * r)


def test_meter_update_does_not_synchronise():
    batches = _meter_batches()
    dev = [(x.to(DEV), m.to(DEV)) for x, m, _ in batches]
    meter = M.SegmentationMeter()
    meter.update(*dev[0])                        # first use: library load, state allocation
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
            for x, m in dev[1:]:
                meter.update(x, m)
            meter.compute("pooled")
            meter.compute("batch_mean")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not enforced:
        pytest.skip("this torch build does not enforce torch.cuda.set_sync_debug_mode('error') "
                    "(a .item() did not raise), so the absence of host syncs cannot be asserted")
    assert torch.equal(meter.counts().cpu(), torch.cat([r for _, _, r in batches], 0).sum(0))


# ---- 8. hard-mask output ----------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(10, 14), (5, 7), (8, 8)], ids=["resize", "same_scalar", "same_vector"])
def test_hard_mask_output(size):
    if size == (8, 8):
        g = torch.Generator().manual_seed(0)
        x = torch.randn(3, 2, 8, 8, generator=g) * 3
        m = (torch.rand(3, 2, 8, 8, generator=g) < 0.3).float()
        v = x.double()
    else:
        x, m, v = case4(size, False)
    hard = torch.full((3, 2, *size), 7, dtype=torch.uint8, device=DEV)
    got = M.seg_counts(x.to(DEV), m.to(DEV), hard_mask=hard)
    assert torch.equal(got.cpu(), ref_counts(v, m))
    assert torch.equal(hard.cpu(), (v > 0.5).to(torch.uint8))


# ---- 9. dispatcher op --------------------------------------------------------------------------------------
def test_seg_counts_op():
    x, m, v = case4((10, 14), False)
    xd, md = x.to(DEV), m.to(DEV)
    op = torch.ops.vaeunet.seg_counts
    assert torch.equal(op(xd, md, False).cpu(), ref_counts(v, m))
    torch.library.opcheck(op.default, (xd, md, False), test_utils=("test_schema", "test_faketensor",
                                                                    "test_autograd_registration"))
    x1, m1, ref = case1((3, 2, 33, 31), True)
    torch.library.opcheck(op.default, (x1.to(DEV), m1.to(DEV).bool()),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    assert torch.equal(op(x1.to(DEV), m1.to(DEV).bool()).cpu(), ref)


def test_errors_on_device():
    x = torch.zeros(2, 2, 4, 4, device=DEV)
    with pytest.raises(ValueError):
        M.seg_counts(x, torch.zeros(3, 2, 4, 4, device=DEV))
    with pytest.raises(ValueError):
        M.seg_counts(x, torch.zeros(2, 1, 8, 8, device=DEV))
    with pytest.raises(ValueError):
        M.seg_counts(x, torch.zeros(2, 2, 4, 4, device=DEV), out=torch.zeros(2, 2, 4, device=DEV))
    assert M.seg_counts(x, torch.zeros(2, 2, 8, 8, device=DEV)).shape == (2, 2, 4)
