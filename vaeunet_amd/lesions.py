"""Lesion-level evaluation on the device (csrc/ccl.hip):
connected-component labelling, small-component removal, candidate /
ground-truth matching and the FROC curve.  These are this project's own
definitions (include/vaeunet.h), unpinned against any reference code.

A *plane* is one (image, class) slice [H, W] of a [B, C, H, W] tensor; planes
never interact.  Foreground: a uint8 / bool element is foreground when it is
nonzero (``threshold`` is not used), a float32 element ``p`` when
``p > threshold``, strictly (NaN is background).  A label is 0 on the
background and ``1 + (the smallest row-major index y*W + x of the component)``
elsewhere: canonical, so two runs are bitwise equal and any other labelling
maps onto it exactly.  Ground-truth masks follow the metrics' truth convention:
nonzero for uint8 / bool, ``> 0.5`` for float32 (other dtypes are converted to
float32 first).

Nothing in ``lesion_counts`` or ``LesionMeter.update`` synchronises the host.
"""
import numbers

import torch

from ._lib import (VU_CCL_F32, VU_CCL_MAX_PLANE, VU_CCL_U8, VU_FROC_MAX_BINS, call, ptr, query, stream)

COUNT_NAMES = ("n_gt", "n_gt_detected", "n_pred", "n_pred_fp")
LESION_METRIC_NAMES = ("sensitivity", "precision", "fp_per_image")
_CODES = {torch.uint8: VU_CCL_U8, torch.bool: VU_CCL_U8, torch.float32: VU_CCL_F32}


# ---- validation: every ValueError is raised before a device is touched --------
def _check_connectivity(connectivity, what):
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def _check_min_area(min_area, what):
    if isinstance(min_area, bool) or not isinstance(min_area, numbers.Integral) or not 1 <= min_area <= 2 ** 31 - 1:
        raise ValueError(f"{what}: min_area must be an integer >= 1, got {min_area!r}")
    return int(min_area)


def _check_planes(x, what, name, dtypes):
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"{what}: {name} must be a [B, C, H, W] tensor, got "
                         f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    if x.numel() == 0:
        raise ValueError(f"{what}: empty {name} {tuple(x.shape)}")
    if dtypes is not None and x.dtype not in dtypes:
        raise ValueError(f"{what}: {name} must be one of {', '.join(str(d) for d in dtypes)}, got {x.dtype}")
    if x.shape[2] * x.shape[3] > VU_CCL_MAX_PLANE:
        raise ValueError(f"{what}: a plane of {x.shape[2]} x {x.shape[3]} pixels exceeds the int32 labels "
                         f"(H*W <= {VU_CCL_MAX_PLANE})")


def _check_input(x, threshold, what, name="x"):
    """-> the threshold as a float (0.0 when the input has none)"""
    _check_planes(x, what, name, tuple(_CODES))
    if x.dtype == torch.float32:
        if threshold is None:
            raise ValueError(f"{what}: a float32 {name} needs a threshold")
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError(f"{what}: the threshold is NaN")
        return threshold
    return 0.0


def _need_device(t, what):
    if t.device.type != "cuda":
        raise RuntimeError(f"vaeunet_amd lesion metrics run on MI355X (HIP) devices only; {what} got {t.device}")


def _dense(x):
    x = x.detach().contiguous()
    return x.view(torch.uint8) if x.dtype == torch.bool else x


def _workspace(shape, device):
    B, Cn, H, W = shape
    return torch.empty(query("vu_ccl_workspace_bytes", B * Cn, H, W) // 4, dtype=torch.int32, device=device)


# ---- launches (dense, validated tensors on the device) ------------------------
def _launch_label(x, threshold, connectivity, labels=None, ncomp=None):
    B, Cn, H, W = x.shape
    if labels is None:
        labels = torch.empty((B, Cn, H, W), dtype=torch.int32, device=x.device)
    call("vu_ccl_label", ptr(x), _CODES[x.dtype], threshold, B * Cn, H, W, connectivity, ptr(labels), ptr(ncomp),
         stream())
    return labels


def _launch_remove_small(labels, min_area, mask, areas, ws=None):
    B, Cn, H, W = labels.shape
    ws = _workspace(labels.shape, labels.device) if ws is None else ws
    call("vu_ccl_remove_small", ptr(labels), B * Cn, H, W, min_area, ptr(mask), ptr(areas), ptr(ws), stream())


# ---- public functions ----------------------------------------------------------
def label_components(x, connectivity=8, threshold=None, return_counts=False):
    """Canonical component labels of every plane of ``x`` [B, C, H, W] (uint8,
    bool or float32): int32 [B, C, H, W].  With ``return_counts`` also the
    number of components per plane, int64 [B, C]."""
    what = "label_components"
    connectivity = _check_connectivity(connectivity, what)
    thr = _check_input(x, threshold, what)
    _need_device(x, what)
    x = _dense(x)
    ncomp = torch.empty(x.shape[:2], dtype=torch.int64, device=x.device) if return_counts else None
    labels = _launch_label(x, thr, connectivity, ncomp=ncomp)
    return (labels, ncomp) if return_counts else labels


def component_areas(labels):
    """labels int32 [B, C, H, W] (of ``label_components``) -> int32 image that
    holds the component's area at every foreground pixel, 0 elsewhere."""
    what = "component_areas"
    _check_planes(labels, what, "labels", (torch.int32,))
    _need_device(labels, what)
    labels = labels.detach().contiguous()
    areas = torch.empty_like(labels)
    _launch_remove_small(labels, 1, None, areas)
    return areas


def remove_small_components(x, min_area, connectivity=8, threshold=None):
    """uint8 [B, C, H, W]: 1 on the foreground pixels of ``x`` whose component
    has at least ``min_area`` pixels."""
    what = "remove_small_components"
    connectivity = _check_connectivity(connectivity, what)
    min_area = _check_min_area(min_area, what)
    thr = _check_input(x, threshold, what)
    _need_device(x, what)
    x = _dense(x)
    labels = _launch_label(x, thr, connectivity)
    mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _launch_remove_small(labels, min_area, mask, None)
    return mask


def _check_pair(pred, masks, threshold, what):
    thr = _check_input(pred, threshold, what, "pred")
    _check_planes(masks, what, "masks", None)
    if pred.shape != masks.shape:
        raise ValueError(f"Shape mismatch in {what}: pred {tuple(pred.shape)} vs masks {tuple(masks.shape)}")
    return thr


def _match(pred, masks, thr, min_area, connectivity, nb, counts, hist_fp, hist_gt, buf):
    """labels of both sides and the matching passes; buf: int32 scratch of 6 * numel elements (two label images,
    four tables)"""
    masks = masks.to(pred.device)
    if masks.dtype not in _CODES:
        masks = masks.float()
    pred, masks = _dense(pred), _dense(masks)
    B, Cn, H, W = pred.shape
    n = pred.numel()
    pl, gl = buf[:n].view(pred.shape), buf[n:2 * n].view(pred.shape)
    _launch_label(pred, thr, connectivity, labels=pl)
    _launch_label(masks, 0.5, connectivity, labels=gl)
    call("vu_lesion_match", ptr(pl), ptr(gl), ptr(pred), _CODES[pred.dtype], B * Cn, H, W, min_area, nb, ptr(counts),
         ptr(hist_fp), ptr(hist_gt), ptr(buf[2 * n:]), stream())


def lesion_counts(pred, masks, threshold=0.5, min_area=1, connectivity=8):
    """Lesion-level counts per plane, int64 [B, C, 4] = (n_gt, n_gt_detected,
    n_pred, n_pred_fp), no host sync.

    pred [B, C, H, W]: a float32 probability map (a candidate = a component of
    ``pred > threshold``) or a uint8 / bool hard mask; masks: the ground truth
    at the same shape.  Candidates below ``min_area`` pixels are dropped: they
    are neither true nor false positives and detect nothing.  A kept candidate
    is a false positive when it overlaps no ground-truth pixel; a ground-truth
    component is detected when a kept candidate overlaps it."""
    what = "lesion_counts"
    connectivity = _check_connectivity(connectivity, what)
    min_area = _check_min_area(min_area, what)
    thr = _check_pair(pred, masks, threshold, what)
    _need_device(pred, what)
    counts = torch.empty(tuple(pred.shape[:2]) + (4,), dtype=torch.int64, device=pred.device)
    buf = torch.empty(6 * pred.numel(), dtype=torch.int32, device=pred.device)
    _match(pred, masks, thr, min_area, connectivity, 1, counts, None, None, buf)
    return counts


def lesion_metrics(counts, n_planes=None, epsilon=1e-6):
    """counts int64 [..., 4] -> fp32 [3] on the device, columns
    ``LESION_METRIC_NAMES``, pooled over all rows: sensitivity
    ``(n_gt_detected + eps) / (n_gt + eps)``, precision ``(n_pred - n_pred_fp +
    eps) / (n_pred + eps)`` (the eps convention of ``seg_metrics``) and false
    positives per image ``n_pred_fp / n_planes``; ``n_planes`` defaults to the
    number of rows."""
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or counts.dim() < 1 \
            or counts.shape[-1] != 4 or counts.numel() == 0:
        raise ValueError("lesion_metrics: expected a non-empty int64 [..., 4] counts table")
    rows = counts.numel() // 4
    n_planes = rows if n_planes is None else int(n_planes)
    if n_planes < 1:
        raise ValueError(f"lesion_metrics: n_planes must be >= 1, got {n_planes}")
    _need_device(counts, "lesion_metrics")
    c = counts.contiguous()
    out = torch.empty(3, dtype=torch.float32, device=c.device)
    call("vu_lesion_metrics", ptr(c), rows, n_planes, float(epsilon), ptr(out), stream())
    return out


class LesionMeter:
    """Running lesion-level scores and the FROC histograms on the device.

    ``update(pred, masks)``: pred is a float32 probability map at mask
    resolution (what ``predict_full_image`` / ``predict_with_patches`` return)
    or a uint8 / bool hard mask (what ``seg_counts(hard_mask=...)`` writes).
    It labels both sides, matches them and adds the batch's counts per class
    and its scores to the two histograms; it never synchronises the host, and
    its scratch grows as ``SegmentationMeter``'s does.  ``froc()`` returns
    ``(sens [bins], fppi [bins], score)`` as fp64 device tensors: operating
    point k keeps the scores in bins >= k; with no ground-truth lesion every
    sensitivity, and the score, is NaN."""

    def __init__(self, threshold=0.5, min_area=1, connectivity=8, bins=1000, epsilon=1e-6):
        what = "LesionMeter"
        self.connectivity = _check_connectivity(connectivity, what)
        self.min_area = _check_min_area(min_area, what)
        if isinstance(bins, bool) or not isinstance(bins, int) or not 1 <= bins <= VU_FROC_MAX_BINS:
            raise ValueError(f"{what}: bins must be an integer in 1..{VU_FROC_MAX_BINS}, got {bins!r}")
        self.threshold = float(threshold)
        if self.threshold != self.threshold:
            raise ValueError(f"{what}: the threshold is NaN")
        self.bins = bins
        self.epsilon = float(epsilon)
        self.reset()

    def reset(self):
        self.n_planes = 0
        self._total = None     # int64 [C, 4]
        self._hist = None      # int64 [2, bins]: false-positive candidates, detected ground-truth components
        self._buf = None

    def update(self, pred, masks):
        what = "LesionMeter.update"
        thr = _check_pair(pred, masks, self.threshold, what)
        _need_device(pred, what)
        B, Cn = pred.shape[:2]
        dev = pred.device
        if self._total is None:
            self._total = torch.zeros((Cn, 4), dtype=torch.int64, device=dev)
            self._hist = torch.zeros((2, self.bins), dtype=torch.int64, device=dev)
        elif self._total.shape[0] != Cn or self._total.device != dev:
            raise ValueError(f"{what}: {Cn} classes on {dev}, earlier batches had {self._total.shape[0]} on "
                             f"{self._total.device}")
        need = 6 * pred.numel()
        if self._buf is None or self._buf.numel() < need:
            self._buf = torch.empty(need, dtype=torch.int32, device=dev)
        counts = torch.empty((B, Cn, 4), dtype=torch.int64, device=dev)
        _match(pred, masks, thr, self.min_area, self.connectivity, self.bins, counts, self._hist[0], self._hist[1],
               self._buf)
        self._total += counts.sum(0)
        self.n_planes += B * Cn

    def _need_state(self):
        if self._total is None:
            raise RuntimeError("LesionMeter: no update() since the last reset()")

    def counts(self):
        """total (n_gt, n_gt_detected, n_pred, n_pred_fp) per class: int64 [C, 4]"""
        self._need_state()
        return self._total

    def histograms(self):
        """(hist_fp, hist_gt): int64 [bins] each"""
        self._need_state()
        return self._hist[0], self._hist[1]

    def values(self):
        """fp32 [3] device tensor, columns ``LESION_METRIC_NAMES`` (no host sync)"""
        self._need_state()
        return lesion_metrics(self._total, self.n_planes, self.epsilon)

    def froc(self):
        self._need_state()
        dev = self._total.device
        curve = torch.empty((2, self.bins), dtype=torch.float64, device=dev)
        score = torch.empty((), dtype=torch.float64, device=dev)
        call("vu_froc_metrics", ptr(self._hist[0]), ptr(self._hist[1]), ptr(self._total), self._total.shape[0],
             self.n_planes, self.bins, ptr(curve[0]), ptr(curve[1]), ptr(score), stream())
        return curve[0], curve[1], score

    def compute(self):
        """dict of 0-dim device tensors: the three lesion metrics (fp32) and ``froc`` (fp64); no host sync"""
        r = self.values()
        res = {k: r[i] for i, k in enumerate(LESION_METRIC_NAMES)}
        res["froc"] = self.froc()[2]
        return res
