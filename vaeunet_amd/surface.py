"""Boundary metrics on the device (csrc/edt.hip): the exact
squared Euclidean distance transform, the boundary of a mask, and the surface
statistics behind the Hausdorff distance, its percentile (HD95), the average
symmetric surface distance (ASSD) and the surface Dice at a tolerance (NSD).
These are this project's own definitions (include/vaeunet.h), unpinned against
any reference code.

Planes and foreground are those of ``vaeunet_amd.lesions``: a plane is one
(image, class) slice [H, W] of a [B, C, H, W] tensor; a uint8 / bool element is
foreground when nonzero, a float32 element ``p`` when ``p > threshold``,
strictly (NaN is background); ground-truth masks are foreground when nonzero
(uint8 / bool) or ``> 0.5`` (float32; other dtypes are converted to float32
first).  A boundary pixel is a foreground pixel with at least one of its four
neighbours background or outside the plane.  Distances are in pixels.

``signed_distance`` (csrc/sdf.hip) is the signed distance map
the boundary loss of ``vaeunet_amd.loss`` multiplies the probabilities with.

Nothing in ``surface_stats``, ``SurfaceMeter.update`` or ``signed_distance``
synchronises the host.
"""
import numbers

import torch

from ._lib import (VU_EDT_INF, VU_EDT_MAX_DIM, VU_EDT_TO_BACKGROUND, VU_EDT_TO_BOUNDARY, VU_EDT_TO_FOREGROUND,
                   VU_SDF_MAX_W, call, ptr, query, stream)
from .lesions import _CODES, _check_input, _check_planes, _dense

MODES = {"foreground": VU_EDT_TO_FOREGROUND, "background": VU_EDT_TO_BACKGROUND, "boundary": VU_EDT_TO_BOUNDARY}
STAT_NAMES = ("n_pred", "n_gt", "max_d2_pred_gt", "max_d2_gt_pred", "pct_d2_pred_gt", "pct_d2_gt_pred",
              "within_pred", "within_gt")
SURFACE_METRIC_NAMES = ("hd", "hd_q", "assd", "nsd")
INF = VU_EDT_INF


# ---- validation: every ValueError is raised before a device is touched --------
def _check_dims(x, what, name):
    if x.shape[2] > VU_EDT_MAX_DIM or x.shape[3] > VU_EDT_MAX_DIM:
        raise ValueError(f"{what}: {name} of {x.shape[2]} x {x.shape[3]} pixels exceeds the distance transform's "
                         f"H, W <= {VU_EDT_MAX_DIM}")


def _check_x(x, threshold, what, name="x"):
    thr = _check_input(x, threshold, what, name)
    _check_dims(x, what, name)
    return thr


def _check_percentile(q, what):
    if isinstance(q, bool) or not isinstance(q, numbers.Integral) or not 1 <= q <= 100:
        raise ValueError(f"{what}: percentile must be an integer in 1..100, got {q!r}")
    return int(q)


def _check_tolerance(tolerance, what):
    """-> tol2 = (int)(tolerance * tolerance), formed in fp64"""
    if isinstance(tolerance, bool) or not isinstance(tolerance, numbers.Real):
        raise ValueError(f"{what}: tolerance must be a number >= 0, got {tolerance!r}")
    t = float(tolerance)
    if not 0.0 <= t or t * t > 2.0 ** 30:      # NaN fails the first test; a real d^2 is below 2^29
        raise ValueError(f"{what}: tolerance must be in [0, 32768], got {tolerance!r}")
    return int(t * t)


def _check_pair(pred, masks, threshold, what):
    thr = _check_x(pred, threshold, what, "pred")
    _check_planes(masks, what, "masks", None)
    if pred.shape != masks.shape:
        raise ValueError(f"Shape mismatch in {what}: pred {tuple(pred.shape)} vs masks {tuple(masks.shape)}")
    return thr


def _need_device(t, what):
    if t.device.type != "cuda":
        raise RuntimeError(f"vaeunet_amd surface metrics run on MI355X (HIP) devices only; {what} got {t.device}")


def workspace_elements(shape):
    """int32 elements of scratch ``surface_stats`` needs for a [B, C, H, W] shape"""
    B, Cn, H, W = shape
    return (query("vu_edt_workspace_bytes", B * Cn, H, W) + 3) // 4


# ---- public functions ----------------------------------------------------------
def distance_transform(x, mode="background", threshold=None, squared=True):
    """The exact Euclidean distance transform of every plane of ``x`` [B, C, H,
    W] (uint8, bool or float32): the distance of each pixel to the nearest
    *site*.  ``mode`` names the sites: ``"background"`` (scipy's
    ``distance_transform_edt`` convention), ``"foreground"`` or ``"boundary"``.
    ``squared=True`` returns the squared distance as int32, ``VU_EDT_INF`` =
    2^31 - 1 on a plane without a site; ``squared=False`` returns float32
    ``(float)sqrt((double)d2)``, ``+inf`` there."""
    what = "distance_transform"
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"{what}: mode must be one of {', '.join(MODES)}, got {mode!r}")
    thr = _check_x(x, threshold, what)
    _need_device(x, what)
    x = _dense(x)
    B, Cn, H, W = x.shape
    out = torch.empty(x.shape, dtype=torch.int32 if squared else torch.float32, device=x.device)
    call("vu_edt", ptr(x), _CODES[x.dtype], thr, MODES[mode], B * Cn, H, W, ptr(out), 0 if squared else 1, stream())
    return out


def boundary(x, threshold=None):
    """uint8 [B, C, H, W]: 1 on the boundary pixels of ``x``."""
    what = "boundary"
    thr = _check_x(x, threshold, what)
    _need_device(x, what)
    x = _dense(x)
    B, Cn, H, W = x.shape
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    call("vu_edt_boundary", ptr(x), _CODES[x.dtype], thr, B * Cn, H, W, ptr(out), stream())
    return out


def _check_clip(clip, what):
    """-> the clip as a float, +inf for None"""
    if clip is None:
        return float("inf")
    if isinstance(clip, bool) or not isinstance(clip, numbers.Real) or not float(clip) > 0.0:   # NaN fails
        raise ValueError(f"{what}: clip must be a number > 0 or None, got {clip!r}")
    return float(clip)


def _check_sdf_input(x, threshold, what, name="x"):
    thr = _check_x(x, threshold, what, name)
    if x.shape[3] > VU_SDF_MAX_W:
        raise ValueError(f"{what}: {name} of width {x.shape[3]} exceeds the signed distance map's W <= {VU_SDF_MAX_W}")
    return thr


def _launch_sdf(x, thr, squared, clip):
    """x dense and validated, on the device; clip a float > 0"""
    B, Cn, H, W = x.shape
    out = torch.empty(x.shape, dtype=torch.int32 if squared else torch.float32, device=x.device)
    call("vu_sdf", ptr(x), _CODES[x.dtype], thr, B * Cn, H, W, ptr(out), 0 if squared else 1, clip, stream())
    return out


def signed_distance(x, threshold=None, squared=False, clip=None):
    """The signed distance map of every plane of ``x`` [B, C, H, W] (uint8, bool
    or float32), DESIGN.md §4.13: ``squared=True`` returns int32 ``s2``, +d^2
    to the nearest foreground pixel at a background pixel, -d^2 to the nearest
    background pixel at a foreground pixel; ``squared=False`` returns float32
    ``phi`` = sqrt(s2) outside, 1 - sqrt(-s2) inside (0 on the foreground
    pixels at the boundary), clamped to [-clip, clip] when ``clip`` is given.
    A plane without foreground or without background is 0 everywhere.  One
    signed transform: two launches, no host synchronisation.  W <= 8192."""
    what = "signed_distance"
    c = _check_clip(clip, what)
    if squared and clip is not None:
        raise ValueError(f"{what}: clip applies to the float32 map, not to squared=True")
    thr = _check_sdf_input(x, threshold, what)
    _need_device(x, what)
    return _launch_sdf(_dense(x), thr, bool(squared), c)


def _stats(pred, masks, thr, q, tol2, stats, sums, buf):
    masks = masks.to(pred.device)
    if masks.dtype not in _CODES:
        masks = masks.float()
    pred, masks = _dense(pred), _dense(masks)
    B, Cn, H, W = pred.shape
    call("vu_surface_stats", ptr(pred), _CODES[pred.dtype], thr, ptr(masks), _CODES[masks.dtype], B * Cn, H, W, q,
         tol2, ptr(stats), ptr(sums), ptr(buf), stream())


def surface_stats(pred, masks, threshold=0.5, percentile=95, tolerance=1.0):
    """Surface statistics per plane between the boundary of the prediction (P)
    and of the ground truth (G), no host sync: ``(stats, sums)`` with stats
    int64 [B, C, 8], columns ``STAT_NAMES`` -- the two boundary sizes, the
    largest squared distance P->G and G->P, its ``percentile``-th percentile
    (nearest rank, an integer) both ways, the number of boundary pixels within
    ``tolerance`` pixels both ways -- and sums fp64 [B, C, 2], the sums of the
    distances P->G and G->P.  A plane with an empty P or G is undefined: its
    columns 2..7 are -1 and its sums 0.

    pred [B, C, H, W]: a float32 probability map (foreground is ``pred >
    threshold``) or a uint8 / bool hard mask; masks: the ground truth at the
    same shape."""
    what = "surface_stats"
    q = _check_percentile(percentile, what)
    tol2 = _check_tolerance(tolerance, what)
    thr = _check_pair(pred, masks, threshold, what)
    _need_device(pred, what)
    dev = pred.device
    stats = torch.empty(tuple(pred.shape[:2]) + (8,), dtype=torch.int64, device=dev)
    sums = torch.empty(tuple(pred.shape[:2]) + (2,), dtype=torch.float64, device=dev)
    buf = torch.empty(workspace_elements(pred.shape), dtype=torch.int32, device=dev)
    _stats(pred, masks, thr, q, tol2, stats, sums, buf)
    return stats, sums


def _check_tables(stats, sums, what):
    if not isinstance(stats, torch.Tensor) or stats.dtype != torch.int64 or stats.dim() < 1 or stats.shape[-1] != 8 \
            or stats.numel() == 0:
        raise ValueError(f"{what}: expected a non-empty int64 [..., 8] stats table")
    if not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64 or sums.dim() < 1 or sums.shape[-1] != 2 \
            or sums.shape[:-1] != stats.shape[:-1]:
        raise ValueError(f"{what}: expected fp64 sums {tuple(stats.shape[:-1]) + (2,)} to go with the stats")


def surface_metrics(stats, sums):
    """(stats [..., 8], sums [..., 2]) of ``surface_stats`` -> fp64 [..., 4] on
    the device, columns ``SURFACE_METRIC_NAMES``: the Hausdorff distance, its
    percentile version (the larger of the two directed percentiles), the
    average symmetric surface distance and the surface Dice at the tolerance
    (the fraction of both boundaries within it); NaN on an undefined plane."""
    what = "surface_metrics"
    _check_tables(stats, sums, what)
    _need_device(stats, what)
    st, sm = stats.contiguous(), sums.contiguous()
    out = torch.empty(tuple(stats.shape[:-1]) + (4,), dtype=torch.float64, device=st.device)
    call("vu_surface_metrics", ptr(st), ptr(sm), st.numel() // 8, ptr(out), None, None, stream())
    return out


class SurfaceMeter:
    """Running boundary metrics on the device.

    ``update(pred, masks)``: pred is a float32 probability map at mask
    resolution or a uint8 / bool hard mask (what ``seg_counts(hard_mask=...)``
    writes).  It computes the batch's surface statistics and adds every defined
    plane's four metrics, in plane order, to fp64 accumulators; it never
    synchronises the host, and its scratch grows as ``LesionMeter``'s does.
    ``values()`` is the mean over the defined planes of (hd, hd_q, assd, nsd),
    fp64 [4] on the device, NaN when no plane was defined."""

    def __init__(self, threshold=0.5, percentile=95, tolerance=1.0):
        what = "SurfaceMeter"
        self.percentile = _check_percentile(percentile, what)
        self.tol2 = _check_tolerance(tolerance, what)
        self.tolerance = float(tolerance)
        self.threshold = float(threshold)
        if self.threshold != self.threshold:
            raise ValueError(f"{what}: the threshold is NaN")
        self.reset()

    def reset(self):
        self.n_planes = 0
        self._acc = None      # fp64 [4]: sums of the metrics over the defined planes
        self._nacc = None     # int64 [2]: defined planes, planes
        self._buf = None

    def update(self, pred, masks):
        what = "SurfaceMeter.update"
        thr = _check_pair(pred, masks, self.threshold, what)
        _need_device(pred, what)
        B, Cn = pred.shape[:2]
        dev = pred.device
        if self._acc is None:
            self._acc = torch.zeros(4, dtype=torch.float64, device=dev)
            self._nacc = torch.zeros(2, dtype=torch.int64, device=dev)
        elif self._acc.device != dev:
            raise ValueError(f"{what}: a batch on {dev}, earlier batches were on {self._acc.device}")
        P = B * Cn
        need = workspace_elements(pred.shape) + 28 * P     # + stats [P, 8], sums [P, 2], metrics [P, 4]: 8-byte words
        if self._buf is None or self._buf.numel() < need:
            self._buf = torch.empty(need, dtype=torch.int32, device=dev)
        tables = self._buf[:28 * P].view(torch.int64)
        stats, sums = tables[:8 * P], tables[8 * P:10 * P].view(torch.float64)
        per_plane = tables[10 * P:].view(torch.float64)
        _stats(pred, masks, thr, self.percentile, self.tol2, stats, sums, self._buf[28 * P:])
        call("vu_surface_metrics", ptr(stats), ptr(sums), B * Cn, ptr(per_plane), ptr(self._acc), ptr(self._nacc),
             stream())
        self.n_planes += B * Cn

    def _need_state(self):
        if self._acc is None:
            raise RuntimeError("SurfaceMeter: no update() since the last reset()")

    def counts(self):
        """int64 [2] device tensor: (defined planes, planes)"""
        self._need_state()
        return self._nacc

    def values(self):
        """fp64 [4] device tensor, columns ``SURFACE_METRIC_NAMES`` (no host sync)"""
        self._need_state()
        return self._acc / self._nacc[0].double()

    def compute(self):
        """dict of 0-dim device tensors: the four metrics (fp64) and ``n_defined`` (int64); no host sync"""
        r = self.values()
        res = {k: r[i] for i, k in enumerate(SURFACE_METRIC_NAMES)}
        res["n_defined"] = self._nacc[0]
        return res
