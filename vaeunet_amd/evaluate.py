"""Validation loop (drop-in for the reference's evaluate.py, which train.py
calls once per epoch): inference-mode forward, logits resized to the mask,
all segmentation metrics -- with every per-batch result kept on the device.

Per batch this runs the model and ``SegmentationMeter.update`` (one fused
counts pass that resizes the logits on the fly, one small metrics launch);
the host waits for the device once, when the epoch's numbers are read.

Unpinned vs the reference (its evaluate.py was not available when this was
written; both choices are arguments or return keys, so either reading is one
line away):
  * reduction: the plain keys are ``batch_mean`` -- the sum of the per-batch
    pooled scores divided by the number of batches, the upstream U-Net
    evaluate() convention; the scores of all validation pixels pooled are
    returned too, under ``pooled_*``.
  * ``align_corners=False`` for the logits -> mask resize: torch's default for
    a bare ``F.interpolate(..., mode='bilinear')``.
"""
import torch

from .lesions import LESION_METRIC_NAMES
from .metrics import METRIC_NAMES, SegmentationMeter

CL = torch.channels_last


def _split_batch(batch):
    if isinstance(batch, dict):
        return batch['image'], batch['mask']
    image, mask = batch[0], batch[1]
    return image, mask


def evaluate(net, dataloader, device, amp=True, align_corners=False, max_batches=None):
    """Validate ``net`` over ``dataloader``; returns a dict of Python floats:
    ``dice, iou, precision, recall, specificity, accuracy`` (mean over batches
    of the per-batch scores), the same under ``pooled_*`` (all pixels of the
    run pooled) and ``batches``.

    net: returns logits [B, C, h, w] or a tuple whose first item is the logits
    (``(logits, mu, logvar)`` of the VAE U-Net).  Batches: ``{'image', 'mask'}``
    dicts or ``(image, mask)`` pairs; a mask without a channel dimension
    ([B, H, W]) gets one.  The logits are resized to the mask's resolution
    inside the metric kernel when the two differ.  The net's training mode is
    restored on return."""
    return _evaluate(net, dataloader, device, amp, align_corners, max_batches, None)


def evaluate_with_lesions(net, dataloader, device, lesion_meter, amp=True, align_corners=False, max_batches=None):
    """``evaluate`` plus lesion-level scores.  lesion_meter: a
    ``lesions.LesionMeter`` (not reset here).  Each batch's hard prediction at
    mask resolution -- written by the counts pass -- and its mask go to
    ``lesion_meter.update``, and the result gains ``lesion_sensitivity``,
    ``lesion_precision``, ``lesion_fp_per_image`` (floats) and ``lesion_n_gt``,
    ``lesion_n_pred`` (ints) of the meter's totals, read in the same single
    transfer as the pixel scores."""
    if lesion_meter is None:
        raise ValueError("evaluate_with_lesions: lesion_meter is required (evaluate() is the loop without one)")
    return _evaluate(net, dataloader, device, amp, align_corners, max_batches, lesion_meter)


def evaluate_with_surface(net, dataloader, device, surface_meter, lesion_meter=None, amp=True, align_corners=False,
                          max_batches=None):
    """``evaluate`` plus boundary metrics.  surface_meter: a
    ``surface.SurfaceMeter`` (not reset here); lesion_meter: optionally a
    ``lesions.LesionMeter`` as in ``evaluate_with_lesions``.  Each batch's hard
    prediction at mask resolution -- written by the counts pass -- and its mask
    go to the meter(s), and the result gains ``surface_hd``, ``surface_hd<q>``
    (q = the meter's percentile: ``surface_hd95``), ``surface_assd``,
    ``surface_nsd`` (floats: means over the planes where both boundaries exist,
    NaN when there is none) and ``surface_n_defined`` (int), plus the lesion
    keys with a lesion meter, all read in the same single transfer as the pixel
    scores."""
    if surface_meter is None:
        raise ValueError("evaluate_with_surface: surface_meter is required (evaluate() is the loop without one)")
    return _evaluate(net, dataloader, device, amp, align_corners, max_batches, lesion_meter, surface_meter)


@torch.inference_mode()
def _evaluate(net, dataloader, device, amp, align_corners, max_batches, lesion_meter, surface_meter=None):
    """the loop of all three; with no meter the launches, the result keys and the one synchronisation are those of
    evaluate() before the lesion scores existed"""
    device = torch.device(device)
    was_training = net.training
    net.eval()
    meter = SegmentationMeter(align_corners=align_corners)
    try:
        for i, batch in enumerate(dataloader):
            if max_batches is not None and i >= max_batches:
                break
            image, mask = _split_batch(batch)
            image = image.to(device=device, dtype=torch.float32, non_blocking=True)
            if image.dim() == 4:
                image = image.contiguous(memory_format=CL)
            mask = mask.to(device=device, non_blocking=True)
            if mask.dim() == image.dim() - 1:
                mask = mask.unsqueeze(1)
            with torch.autocast(device.type, dtype=torch.bfloat16, enabled=bool(amp)):
                out = net(image)
            logits = out[0] if isinstance(out, (tuple, list)) else out
            if lesion_meter is None and surface_meter is None:
                meter.update(logits, mask)
            else:
                hard = torch.empty(mask.shape, dtype=torch.uint8, device=device)
                meter.update(logits, mask, hard_mask=hard)
                if lesion_meter is not None:
                    lesion_meter.update(hard, mask)
                if surface_meter is not None:
                    surface_meter.update(hard, mask)
    finally:
        net.train(was_training)
    if meter.batches == 0:
        raise ValueError("evaluate: the dataloader produced no batch")
    if lesion_meter is not None or surface_meter is not None:
        return _with_meters(meter, lesion_meter, surface_meter)
    # one transfer (and the only host synchronisation) for all twelve numbers
    both = torch.stack([meter.values("batch_mean"), meter.values("pooled")]).cpu()
    res = {k: both[0, i].item() for i, k in enumerate(METRIC_NAMES)}
    res.update({f"pooled_{k}": both[1, i].item() for i, k in enumerate(METRIC_NAMES)})
    res["batches"] = meter.batches
    return res


def _with_meters(meter, lesion_meter, surface_meter):
    """the result dict with the lesion and / or surface keys: all numbers in one fp64 transfer (fp32 values and counts
    below 2^53 pass through fp64 unchanged)"""
    k = len(METRIC_NAMES)
    parts = [meter.values("batch_mean").double(), meter.values("pooled").double()]
    if lesion_meter is not None:
        parts += [lesion_meter.values().double(), lesion_meter.counts().sum(0).double()]
    if surface_meter is not None:
        parts += [surface_meter.values(), surface_meter.counts().double()]
    flat = torch.cat(parts).cpu()
    res = {name: flat[i].item() for i, name in enumerate(METRIC_NAMES)}
    res.update({f"pooled_{name}": flat[k + i].item() for i, name in enumerate(METRIC_NAMES)})
    res["batches"] = meter.batches
    at = 2 * k
    if lesion_meter is not None:
        for i, name in enumerate(LESION_METRIC_NAMES):
            res[f"lesion_{name}"] = flat[at + i].item()
        res["lesion_n_gt"] = int(flat[at + 3].item())
        res["lesion_n_pred"] = int(flat[at + 5].item())
        at += 7
    if surface_meter is not None:
        names = ("hd", f"hd{surface_meter.percentile}", "assd", "nsd")
        for i, name in enumerate(names):
            res[f"surface_{name}"] = flat[at + i].item()
        res["surface_n_defined"] = int(flat[at + 4].item())
    return res
