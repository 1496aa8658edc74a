"""Sample-set metrics on the device (csrc/sampleset.hip): the
pairwise overlap matrix between S thresholded samples and the ground truth, and
the figures that score the samples *as a set*: the generalised energy distance
(GED^2, Kohl et al. 2018), the sample diversity, the spread of the per-sample
Dice and the variability of the segmented area.  These are this project's own
definitions (include/vaeunet.h), unpinned against any reference code.

A *plane* is one (image, class) slice [H, W]; planes never interact.
Foreground follows ``lesions.py``: a uint8 / bool sample element is foreground
when it is nonzero (``threshold`` is not used), a float32 element ``p`` when
``p > threshold``, strictly (NaN is background); a ground-truth element when
nonzero (uint8 / bool) or ``> 0.5`` (float32; other dtypes are converted to
float32 first).

``gram[b, c, i, j]`` counts the pixels of plane (b, c) that are foreground in
column i and in column j; columns 0 .. S - 1 are the samples in order, columns
S .. K - 1 the M ground truths, K = S + M <= 64.  The matrix is full and
symmetric and its diagonal holds each column's area.  Everything in
``sample_set_metrics`` is a deterministic fp64 function of these integers.

Nothing here synchronises the host.
"""
import torch

from ._lib import VU_CCL_F32, VU_CCL_MAX_PLANE, VU_CCL_U8, VU_SAMPLESET_MAX, VU_SAMPLESET_NMETRICS, call, ptr, stream

SAMPLESET_METRIC_NAMES = ("ged2", "cross", "diversity", "truth_diversity", "dice_mean", "dice_min", "dice_max",
                          "area_mean", "area_std")
assert len(SAMPLESET_METRIC_NAMES) == VU_SAMPLESET_NMETRICS
_CODES = {torch.uint8: VU_CCL_U8, torch.bool: VU_CCL_U8, torch.float32: VU_CCL_F32}


# ---- validation: every ValueError is raised before a device is touched --------
def _shape_of(x):
    return tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__


def _check_samples(samples, threshold, what):
    """-> (S, B, C, H, W), the threshold as a float (0.0 when the input has none)"""
    if not isinstance(samples, torch.Tensor) or samples.dim() not in (4, 5):
        raise ValueError(f"{what}: samples must be a [S, B, C, H, W] (or [S, C, H, W]) tensor, got {_shape_of(samples)}")
    shape = tuple(samples.shape) if samples.dim() == 5 else (samples.shape[0], 1) + tuple(samples.shape[1:])
    if samples.numel() == 0:
        raise ValueError(f"{what}: empty samples {tuple(samples.shape)}")
    if samples.dtype not in _CODES:
        raise ValueError(f"{what}: samples must be one of {', '.join(str(d) for d in _CODES)}, got {samples.dtype}")
    if shape[3] * shape[4] > VU_CCL_MAX_PLANE:
        raise ValueError(f"{what}: a plane of {shape[3]} x {shape[4]} pixels exceeds H*W <= {VU_CCL_MAX_PLANE}")
    thr = 0.0
    if samples.dtype == torch.float32:
        if threshold is None:
            raise ValueError(f"{what}: float32 samples need a threshold")
        thr = float(threshold)
        if thr != thr:
            raise ValueError(f"{what}: the threshold is NaN")
    return shape, thr


def _check_truths(truths, shape, what):
    """-> M"""
    if truths is None:
        return 0
    S, B, Cn, H, W = shape
    if not isinstance(truths, torch.Tensor) or truths.dim() not in (4, 5):
        raise ValueError(f"{what}: truths must be a [B, C, H, W] or [M, B, C, H, W] tensor, got {_shape_of(truths)}")
    if truths.numel() == 0:
        raise ValueError(f"{what}: empty truths {tuple(truths.shape)}")
    if tuple(truths.shape[-4:]) != (B, Cn, H, W):
        raise ValueError(f"Shape mismatch in {what}: samples of planes {(B, Cn, H, W)} vs truths {tuple(truths.shape)}")
    return truths.shape[0] if truths.dim() == 5 else 1


def _check_k(S, M, what):
    if S + M > VU_SAMPLESET_MAX:
        raise ValueError(f"{what}: {S} samples + {M} truths exceed K <= {VU_SAMPLESET_MAX} columns")


def _check_out(out, samples, shape, M, what):
    S, B, Cn = shape[:3]
    want = (B, Cn, S + M, S + M)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != want \
            or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous int64 {want} tensor, got "
                         f"{(out.dtype, tuple(out.shape)) if isinstance(out, torch.Tensor) else type(out).__name__}")
    if out.device != samples.device:
        raise ValueError(f"{what}: out is on {out.device}, samples on {samples.device}")


def _check_gram(gram, n_samples, what):
    """-> (S, M)"""
    if not isinstance(gram, torch.Tensor) or gram.dtype != torch.int64 or gram.dim() != 4 \
            or gram.shape[2] != gram.shape[3] or gram.numel() == 0:
        raise ValueError(f"{what}: gram must be a non-empty int64 [B, C, K, K] tensor, got "
                         f"{(gram.dtype, tuple(gram.shape)) if isinstance(gram, torch.Tensor) else type(gram).__name__}")
    K = gram.shape[2]
    if isinstance(n_samples, bool) or not isinstance(n_samples, int) or not 1 <= n_samples <= K:
        raise ValueError(f"{what}: n_samples must be an integer in 1..K = {K}, got {n_samples!r}")
    _check_k(K, 0, what)
    return n_samples, K - n_samples


def _need_device(t, what):
    if t.device.type != "cuda":
        raise RuntimeError(f"vaeunet_amd sample-set metrics run on MI355X (HIP) devices only; {what} got {t.device}")


def _dense(x):
    x = x.detach().contiguous()
    return x.view(torch.uint8) if x.dtype == torch.bool else x


# ---- public functions ----------------------------------------------------------
def sample_gram(samples, truths=None, threshold=0.5, out=None):
    """The pairwise overlap counts of every plane: int64 [B, C, K, K], K = S + M.

    samples [S, B, C, H, W] (``[S, C, H, W]`` means B = 1: what
    ``inference.segmentation_distribution`` returns): float32 probabilities,
    thresholded on the fly (no thresholded copy is written), or uint8 / bool
    hard masks.  truths: None (M = 0), [B, C, H, W] (M = 1) or
    [M, B, C, H, W].  ``out=``: an int64 [B, C, K, K] tensor the counts are
    ADDED to (and which is returned)."""
    what = "sample_gram"
    shape, thr = _check_samples(samples, threshold, what)
    M = _check_truths(truths, shape, what)
    S, B, Cn, H, W = shape
    _check_k(S, M, what)
    if out is not None:
        _check_out(out, samples, shape, M, what)
    _need_device(samples, what)
    samples = _dense(samples)
    tcode = VU_CCL_U8
    if truths is not None:
        truths = truths.to(samples.device)
        if truths.dtype not in _CODES:
            truths = truths.float()
        truths = _dense(truths)
        tcode = _CODES[truths.dtype]
    gram = torch.empty((B, Cn, S + M, S + M), dtype=torch.int64, device=samples.device) if out is None else out
    call("vu_sample_gram", ptr(samples), _CODES[samples.dtype], thr, ptr(truths), tcode, S, M, B * Cn, H, W, ptr(gram),
         0 if out is None else 1, stream())
    return gram


def sample_set_metrics(gram, n_samples):
    """gram int64 [B, C, K, K] (of ``sample_gram``), its first ``n_samples``
    columns the samples -> fp64 [B, C, 9], columns ``SAMPLESET_METRIC_NAMES``.

    With d(a, b) = 1 - |a & b| / |a | b| (0 when both are empty) and
    Dice(a, b) = 2 |a & b| / (|a| + |b|) (1 when both are empty): ``cross`` =
    the mean of d over the S M sample-truth pairs, ``diversity`` = the mean of d
    over all S^2 ordered sample pairs, the diagonal included (Kohl et al.'s
    convention), ``truth_diversity`` the same over the M^2 truth pairs,
    ``ged2`` = 2 cross - diversity - truth_diversity; the mean, minimum and
    maximum of Dice over the S M pairs; the mean and the population standard
    deviation of the samples' areas.  Without a truth (K == n_samples) ged2,
    cross, truth_diversity and the three Dice columns are NaN."""
    what = "sample_set_metrics"
    S, M = _check_gram(gram, n_samples, what)
    _need_device(gram, what)
    g = gram.detach().contiguous()
    B, Cn = g.shape[:2]
    out = torch.empty((B, Cn, VU_SAMPLESET_NMETRICS), dtype=torch.float64, device=g.device)
    call("vu_sampleset_metrics", ptr(g), S, M, B * Cn, ptr(out), stream())
    return out


class SampleSetMeter:
    """Running sample-set scores on the device.

    ``update(samples, truths)``: one batch of S samples per image
    ([S, B, C, H, W] or [S, C, H, W]) and its ground truth ([B, C, H, W] or
    [M, B, C, H, W]).  Each plane's metric row is added to a running fp64 sum
    per class and the planes are counted; it never synchronises the host.
    ``values()`` returns the [C, 9] table of means over the planes seen,
    ``compute()`` a dict of 0-dim device tensors: the means over all planes
    (classes pooled)."""

    def __init__(self, threshold=0.5):
        self.threshold = float(threshold)
        if self.threshold != self.threshold:
            raise ValueError("SampleSetMeter: the threshold is NaN")
        self.reset()

    def reset(self):
        self.n_planes = 0      # planes per class
        self._sum = None       # fp64 [C, 9]

    def update(self, samples, truths):
        what = "SampleSetMeter.update"
        shape, _ = _check_samples(samples, self.threshold, what)
        if truths is None:
            raise ValueError(f"{what}: the meter scores samples against a ground truth; truths is None")
        M = _check_truths(truths, shape, what)
        S, B, Cn = shape[:3]
        _check_k(S, M, what)
        _need_device(samples, what)
        dev = samples.device
        if self._sum is None:
            self._sum = torch.zeros((Cn, VU_SAMPLESET_NMETRICS), dtype=torch.float64, device=dev)
        elif self._sum.shape[0] != Cn or self._sum.device != dev:
            raise ValueError(f"{what}: {Cn} classes on {dev}, earlier batches had {self._sum.shape[0]} on "
                             f"{self._sum.device}")
        rows = sample_set_metrics(sample_gram(samples, truths, self.threshold), S)
        self._sum += rows.sum(0)
        self.n_planes += B

    def _need_state(self):
        if self._sum is None:
            raise RuntimeError("SampleSetMeter: no update() since the last reset()")

    def values(self):
        """fp64 [C, 9] device tensor, columns ``SAMPLESET_METRIC_NAMES``: the mean over the planes of each class"""
        self._need_state()
        return self._sum / self.n_planes

    def compute(self):
        """dict of 0-dim fp64 device tensors: the mean of every metric over all planes; no host sync"""
        self._need_state()
        r = self._sum.sum(0) / (self.n_planes * self._sum.shape[0])
        return {k: r[i] for i, k in enumerate(SAMPLESET_METRIC_NAMES)}
