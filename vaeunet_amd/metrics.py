"""Hard-threshold segmentation metric (drop-in for the reference's
utils/metrics.py:8-47: ``dice_score``, ``multiclass_dice_score``,
``dice_loss``).

``dice_score`` thresholds the RAW tensors at 0.5 (logits, not probabilities:
metrics.py:18-19) and takes global sums; ``reduce_batch_first`` only changes
the view the reference sums over, never the sums, so it does not change the
value.  The counts are exact integers on the device (csrc/loss.hip
``vu_dice_score``) and the reference's ``denominator.item() == 0`` branch is a
device-side select, so no host synchronisation happens.
"""
import ctypes as C

import torch

from ._lib import ptr, call, query, stream
from .loss import _dense_pair


def dice_score(input, target, reduce_batch_first=False, epsilon=1e-6):
    """Dice of (input > 0.5) vs (target > 0.5) (metrics.py:8-35); 0-dim fp32
    tensor on the input's device."""
    if input.shape != target.shape:
        raise ValueError(f'Shape mismatch in dice_score: input {input.shape} vs target {target.shape}')
    x, t = _dense_pair(input, target)
    score = torch.empty((), dtype=torch.float32, device=x.device)
    ws = torch.empty(query("vu_loss_workspace_bytes") // 8 + 1, dtype=torch.float64, device=x.device)
    call("vu_dice_score", ptr(x), ptr(t), x.numel(), float(epsilon), ptr(score), None, ptr(ws),
         stream())
    return score


def multiclass_dice_score(input, target, reduce_batch_first=False, epsilon=1e-6):
    """metrics.py:38-41 (the class flatten does not change the global sums)."""
    return dice_score(input.flatten(0, 1), target.flatten(0, 1), reduce_batch_first, epsilon)


def dice_loss(input, target, multiclass=False):
    """1 - dice (metrics.py:44-47)."""
    fn = multiclass_dice_score if multiclass else dice_score
    return 1 - fn(input, target, reduce_batch_first=True)


# ---- validation: fused counts, the six metrics, the epoch meter --------------
# One pass over a batch (csrc/metrics.hip ``vu_seg_counts``) gives the exact
# integer (TP, FP, FN, TN) of every (image, class) plane, reading bf16 / fp32
# logits and fp32 / uint8 / bool / int64 masks in place (any strides) and
# resizing the logits to the mask on the fly; ``vu_seg_metrics`` turns a counts
# table into the metrics on the device.  Nothing here synchronises the host.
#
# Unpinned vs the reference (its utils/metrics.py beyond dice_score was not
# available): the formulas of iou / precision / recall / specificity /
# accuracy are this project's definition (include/vaeunet.h), eps = 1e-6.
METRIC_NAMES = ("dice", "iou", "precision", "recall", "specificity", "accuracy")

_LOGIT_CODES = {torch.float32: 0, torch.bfloat16: 1}
_MASK_CODES = {torch.float32: 0, torch.uint8: 1, torch.bool: 1, torch.int64: 2}
_I64x4 = C.c_int64 * 4


def _seg_pair(logits, masks, what):
    if logits.dim() != 4 or masks.dim() != 4:
        raise ValueError(f"{what}: expected [B, C, h, w] logits and [B, C, H, W] masks, got "
                         f"{tuple(logits.shape)} and {tuple(masks.shape)}")
    if logits.shape[:2] != masks.shape[:2]:
        raise ValueError(f"Shape mismatch in {what}: input {tuple(logits.shape)} vs target {tuple(masks.shape)}")
    if logits.numel() == 0 or masks.numel() == 0:
        raise ValueError(f"{what}: empty input")
    if logits.device.type != "cuda":
        raise RuntimeError(f"vaeunet_amd metrics run on MI355X (HIP) devices only; {what} got {logits.device}")
    if logits.dtype not in _LOGIT_CODES:
        logits = logits.float()
    masks = masks.to(logits.device)
    if masks.dtype not in _MASK_CODES:
        masks = masks.float()
    return logits.detach(), masks.detach()


def _workspace(planes, device):
    return torch.empty(query("vu_seg_counts_workspace_bytes", planes) // 8, dtype=torch.int64, device=device)


def seg_counts(logits, masks, align_corners=False, out=None, hard_mask=None, workspace=None, _resize=False):
    """Exact (TP, FP, FN, TN) of ``logits > 0.5`` against ``masks > 0.5`` per
    (image, class): int64 [B, C, 4] on the logits' device, no host sync.

    logits [B, C, h, w] (fp32 or bf16, any strides), masks [B, C, H, W] (fp32,
    uint8, bool or int64, any strides).  When (h, w) != (H, W) each mask pixel
    is classified by the bilinear interpolation of the logits
    (``F.interpolate(logits, (H, W), mode='bilinear', align_corners=...)``
    semantics, fp32) computed inside the kernel.  ``out``: an existing int64
    [B, C, 4] tensor to accumulate into (returned).  ``hard_mask``: an
    optional contiguous uint8 [B, C, H, W] tensor that receives the hard
    prediction at mask resolution."""
    x, m = _seg_pair(logits, masks, "seg_counts")
    B, Cn, h, w = x.shape
    H, W = m.shape[2:]
    dev = x.device
    if out is None:
        counts = torch.empty((B, Cn, 4), dtype=torch.int64, device=dev)
    else:
        if out.shape != (B, Cn, 4) or out.dtype != torch.int64 or out.device != dev or not out.is_contiguous():
            raise ValueError(f"seg_counts: out must be a contiguous int64 [{B}, {Cn}, 4] tensor on {dev}")
        counts = out
    if hard_mask is not None and (hard_mask.shape != (B, Cn, H, W) or hard_mask.dtype != torch.uint8
                                  or hard_mask.device != dev or not hard_mask.is_contiguous()):
        raise ValueError(f"seg_counts: hard_mask must be a contiguous uint8 [{B}, {Cn}, {H}, {W}] tensor on {dev}")
    ws = workspace if workspace is not None else _workspace(B * Cn, dev)
    call("vu_seg_counts", ptr(x), _LOGIT_CODES[x.dtype], _I64x4(*x.stride()), h, w, ptr(m), _MASK_CODES[m.dtype],
         _I64x4(*m.stride()), B, Cn, H, W, int(bool(align_corners)), int(bool(_resize)), ptr(counts),
         int(out is not None), ptr(hard_mask), ptr(ws), stream())
    return counts


def seg_metrics(counts, epsilon=1e-6, pooled=True):
    """counts [..., 4] int64 -> fp32 metrics, columns ``METRIC_NAMES``: the
    pooled row [6] (all planes summed first) or, with ``pooled=False``, one
    row per plane [..., 6]."""
    if counts.device.type != "cuda":
        raise RuntimeError(f"vaeunet_amd metrics run on MI355X (HIP) devices only; seg_metrics got {counts.device}")
    if counts.dtype != torch.int64 or counts.dim() < 1 or counts.shape[-1] != 4 or counts.numel() == 0:
        raise ValueError(f"seg_metrics: expected a non-empty int64 [..., 4] counts table, got {tuple(counts.shape)}")
    c = counts.contiguous()
    P = c.numel() // 4
    shape = (6,) if pooled else tuple(counts.shape[:-1]) + (6,)
    res = torch.empty(shape, dtype=torch.float32, device=c.device)
    call("vu_seg_metrics", ptr(c), P, 1, float(epsilon), None if pooled else ptr(res), ptr(res) if pooled else None,
         0, None, stream())
    return res


def _as_planes(input, target, what):
    """(input, target) of the reference's metric signatures as 4-d tensors:
    pooled metrics do not depend on how the elements are cut into planes"""
    if input.dim() == 4 and target.dim() == 4:
        return input, target
    if input.shape != target.shape:
        raise ValueError(f'Shape mismatch in {what}: input {tuple(input.shape)} vs target {tuple(target.shape)}')
    return input.reshape(1, 1, 1, -1), target.reshape(1, 1, 1, -1)


def _pooled(input, target, what, epsilon=1e-6):
    x, t = _as_planes(input, target, what)
    return seg_metrics(seg_counts(x, t), epsilon)


def iou_score(input, target, epsilon=1e-6):
    """(TP + eps) / (TP + FP + FN + eps) of the thresholded tensors; 0-dim fp32."""
    return _pooled(input, target, "iou_score", epsilon)[1]


def precision_recall(input, target, epsilon=1e-6):
    """((TP + eps) / (TP + FP + eps), (TP + eps) / (TP + FN + eps)); 0-dim fp32 each."""
    r = _pooled(input, target, "precision_recall", epsilon)
    return r[2], r[3]


def specificity(input, target, epsilon=1e-6):
    """(TN + eps) / (TN + FP + eps); 0-dim fp32."""
    return _pooled(input, target, "specificity", epsilon)[4]


def accuracy(input, target):
    """(TP + TN) / all pixels; 0-dim fp32."""
    return _pooled(input, target, "accuracy")[5]


def get_all_metrics(input, target, epsilon=1e-6):
    """dict of the six metrics (0-dim fp32 device tensors) from one counts
    pass and one metrics launch; ``dice`` is bit-identical to ``dice_score``."""
    r = _pooled(input, target, "get_all_metrics", epsilon)
    return {k: r[i] for i, k in enumerate(METRIC_NAMES)}


class SegmentationMeter:
    """Running validation metrics on the device.

    ``update(logits, masks)`` launches the counts pass and one metrics launch
    that (a) adds the batch's per-class counts to the epoch totals and (b)
    adds the batch's pooled metric values to a running sum; it never
    synchronises the host and allocates nothing proportional to the image.
    ``compute('pooled')`` = the metrics of the total counts (every pixel of
    the epoch weighs the same); ``compute('batch_mean')`` = the mean over
    update() calls of the per-batch pooled values (the upstream U-Net
    evaluate() convention)."""

    def __init__(self, align_corners=False, epsilon=1e-6):
        self.align_corners = bool(align_corners)
        self.epsilon = float(epsilon)
        self.reset()

    def reset(self):
        self.batches = 0
        self._total = None   # int64 [C, 4]
        self._sum = None     # fp32 [6]: sum over batches of the pooled rows
        self._ws = None

    def update(self, logits, masks, hard_mask=None):
        x, m = _seg_pair(logits, masks, "SegmentationMeter.update")
        B, Cn = x.shape[:2]
        dev = x.device
        if self._total is None:
            self._total = torch.zeros((Cn, 4), dtype=torch.int64, device=dev)
            self._sum = torch.zeros(6, dtype=torch.float32, device=dev)
        elif self._total.shape[0] != Cn or self._total.device != dev:
            raise ValueError(f"SegmentationMeter.update: {Cn} classes on {dev}, earlier batches had "
                             f"{self._total.shape[0]} on {self._total.device}")
        need = query("vu_seg_counts_workspace_bytes", B * Cn) // 8
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.int64, device=dev)
        counts = seg_counts(x, m, self.align_corners, hard_mask=hard_mask, workspace=self._ws)
        call("vu_seg_metrics", ptr(counts), B * Cn, Cn, self.epsilon, None, ptr(self._sum), 1, ptr(self._total),
             stream())
        self.batches += 1

    def _need_state(self):
        if self._total is None:
            raise RuntimeError("SegmentationMeter: no update() since the last reset()")

    def counts(self):
        """total (TP, FP, FN, TN) per class: int64 [C, 4]"""
        self._need_state()
        return self._total

    def values(self, reduction="pooled"):
        """fp32 [6] device tensor, columns ``METRIC_NAMES`` (no host sync)"""
        self._need_state()
        if reduction == "pooled":
            return seg_metrics(self._total, self.epsilon)
        if reduction == "batch_mean":
            return self._sum / self.batches
        raise ValueError(f"SegmentationMeter: reduction must be 'pooled' or 'batch_mean', got {reduction!r}")

    def compute(self, reduction="pooled"):
        """dict of 0-dim fp32 device tensors (no host sync)"""
        r = self.values(reduction)
        return {k: r[i] for i, k in enumerate(METRIC_NAMES)}

    def per_class(self):
        """fp32 [C, 6]: the metrics of each class's total counts"""
        self._need_state()
        return seg_metrics(self._total, self.epsilon, pooled=False)
