"""Calibration and uncertainty metrics on the device: the numbers of the
reference's utils/uncertainty_metrics.py (ECE / MCE, Brier, NLL, AUROC / AUPRC,
sparsification / AUSE) for the probability and uncertainty maps that
``inference.segmentation_distribution`` and ``calculate_uncertainty_metrics``
leave on the device.

One fused streaming pass (csrc/calib.hip ``vu_calib_hist``) reads each byte of
the probabilities, the mask and the optional uncertainty map once and leaves
exact integer histograms plus three fp64 sums; ``vu_calib_metrics`` forms every
metric from those totals in one launch.  Nothing here synchronises the host
until the caller reads a number.

Unpinned vs the reference (its utils/uncertainty_metrics.py was not
available): the definitions are this project's, written out in
include/vaeunet.h and DESIGN.md §4.6.
"""
import math
import struct
from dataclasses import dataclass
from typing import Optional

import torch

from ._lib import VU_CALIB_NSCALARS, VU_CALIB_RANK_BINS, call, ptr, query, stream

RANK_BINS = VU_CALIB_RANK_BINS
MAX_CONF_BINS = 64
SCALAR_NAMES = ("ece", "mce", "brier", "nll", "auroc", "auroc_tie_bound", "auprc", "ause",
                "n", "positives", "n_uncertainty", "uncertainty_errors")

_MASK_CODES = {torch.float32: 0, torch.uint8: 1, torch.bool: 1, torch.int64: 2}


@dataclass
class CalibCounts:
    """The totals of one or more ``calib_hist`` passes (device tensors)."""
    conf_hist: torch.Tensor              # int64 [n_bins, 2]: confidence bin x truth
    conf_sum: torch.Tensor               # fp64 [n_bins]: sum of the clamped probability per bin
    rank_hist: torch.Tensor              # int64 [1024, 2]: probability bin x truth
    unc_hist: Optional[torch.Tensor]     # int64 [1024, 2]: uncertainty bin x (hard prediction wrong)
    sums: torch.Tensor                   # fp64 [2]: Brier and NLL numerators
    invalid: torch.Tensor                # int64 [2]: NaN probabilities, NaN uncertainties
    n_bins: int
    u_max: float


def _uscale(u_max):
    """R / u_max rounded once to fp32 (the kernel's multiplier)"""
    return struct.unpack("f", struct.pack("f", RANK_BINS / float(u_max)))[0]


def _check_bins(n_bins, u_max, what):
    if not isinstance(n_bins, int) or not 1 <= n_bins <= MAX_CONF_BINS:
        raise ValueError(f"{what}: n_bins must be an integer in [1, {MAX_CONF_BINS}], got {n_bins!r}")
    if not (isinstance(u_max, (int, float)) and u_max > 0 and math.isfinite(u_max)):
        raise ValueError(f"{what}: u_max must be a positive finite number, got {u_max!r}")


def _calib_args(prob, target, uncertainty, what):
    if prob.shape != target.shape:
        raise ValueError(f"Shape mismatch in {what}: prob {tuple(prob.shape)} vs target {tuple(target.shape)}")
    if uncertainty is not None and uncertainty.shape != prob.shape:
        raise ValueError(f"Shape mismatch in {what}: prob {tuple(prob.shape)} vs uncertainty "
                         f"{tuple(uncertainty.shape)}")
    if prob.numel() == 0:
        raise ValueError(f"{what}: empty input")
    if prob.device.type != "cuda":
        raise RuntimeError(f"vaeunet_amd metrics run on MI355X (HIP) devices only; {what} got {prob.device}")
    if prob.numel() >= 2 ** 31:
        raise ValueError(f"{what}: {prob.numel()} elements in one call; the limit is 2^31 - 1 (accumulate with out=)")
    dev = prob.device
    p = prob.detach()
    p = (p if p.dtype == torch.float32 else p.float()).contiguous()
    m = target.detach().to(dev)
    m = (m if m.dtype in _MASK_CODES else m.float()).contiguous()
    u = None
    if uncertainty is not None:
        u = uncertainty.detach().to(dev)
        u = (u if u.dtype == torch.float32 else u.float()).contiguous()
    return p, m, u


def _new_counts(n_bins, u_max, with_u, dev):
    """uninitialised: the first pass stores (accumulate = 0)"""
    return CalibCounts(conf_hist=torch.empty((n_bins, 2), dtype=torch.int64, device=dev),
                       conf_sum=torch.empty(n_bins, dtype=torch.float64, device=dev),
                       rank_hist=torch.empty((RANK_BINS, 2), dtype=torch.int64, device=dev),
                       unc_hist=torch.empty((RANK_BINS, 2), dtype=torch.int64, device=dev) if with_u else None,
                       sums=torch.empty(2, dtype=torch.float64, device=dev),
                       invalid=torch.empty(2, dtype=torch.int64, device=dev),
                       n_bins=n_bins, u_max=float(u_max))


def _run(p, m, u, counts, accumulate, ws):
    call("vu_calib_hist", ptr(p), ptr(m), _MASK_CODES[m.dtype], ptr(u), p.numel(), counts.n_bins,
         _uscale(counts.u_max), ptr(counts.conf_hist), ptr(counts.conf_sum), ptr(counts.rank_hist),
         ptr(counts.unc_hist), ptr(counts.sums), ptr(counts.invalid), int(accumulate), ptr(ws), stream())


def _workspace(dev):
    return torch.empty(query("vu_calib_workspace_bytes") // 8, dtype=torch.float64, device=dev)


def calib_hist(prob, target, uncertainty=None, *, n_bins=15, u_max=math.log(2), out=None, workspace=None):
    """One pass over ``prob`` (probabilities), ``target`` (truth = target > 0.5;
    fp32, uint8, bool or int64) and optionally ``uncertainty`` (any map of
    ``calculate_uncertainty_metrics``; binned over [0, u_max], larger values in
    the last bin): a ``CalibCounts`` of device tensors, no host sync.  All
    inputs share one shape; fp32 dense tensors are read in place, other dtypes
    are converted and non-dense inputs made contiguous first.  ``out``: an
    earlier ``CalibCounts`` to accumulate into (returned).  At most 2^31 - 1
    elements per call."""
    if out is not None:
        n_bins, u_max = out.n_bins, out.u_max
    _check_bins(n_bins, u_max, "calib_hist")
    p, m, u = _calib_args(prob, target, uncertainty, "calib_hist")
    dev = p.device
    if out is None:
        counts = _new_counts(n_bins, u_max, u is not None, dev)
    else:
        counts = out
        if counts.conf_hist.device != dev:
            raise ValueError(f"calib_hist: out lives on {counts.conf_hist.device}, the inputs on {dev}")
        if (counts.unc_hist is None) != (u is None):
            raise ValueError("calib_hist: out was started " + ("without" if u is not None else "with")
                             + " an uncertainty map; every call of one accumulation must agree")
    _run(p, m, u, counts, out is not None, workspace if workspace is not None else _workspace(dev))
    return counts


def calib_metrics(counts):
    """``CalibCounts`` -> dict of fp64 device tensors (one launch, no sync):
    the 0-dim scalars of ``SCALAR_NAMES`` (ece, mce, brier, nll, auroc,
    auroc_tie_bound, auprc, ause and the pixel totals), ``reliability``
    [n_bins, 3] = (count, accuracy, mean confidence) per confidence bin and
    ``sparsification`` [1025, 3] = (fraction removed, remaining error, the same under an ideal ordering)
    after removing the k highest-uncertainty bins.  The uncertainty entries are
    NaN when the counts hold no uncertainty histogram."""
    if counts.conf_hist.device.type != "cuda":
        raise RuntimeError("vaeunet_amd metrics run on MI355X (HIP) devices only; calib_metrics got "
                           f"{counts.conf_hist.device}")
    dev = counts.conf_hist.device
    scalars = torch.empty(VU_CALIB_NSCALARS, dtype=torch.float64, device=dev)
    rel = torch.empty((counts.n_bins, 3), dtype=torch.float64, device=dev)
    spars = torch.empty((RANK_BINS + 1, 3), dtype=torch.float64, device=dev)
    call("vu_calib_metrics", ptr(counts.conf_hist), ptr(counts.conf_sum), counts.n_bins, ptr(counts.rank_hist),
         ptr(counts.unc_hist), ptr(counts.sums), ptr(scalars), ptr(rel), ptr(spars), stream())
    res = {k: scalars[i] for i, k in enumerate(SCALAR_NAMES)}
    res["reliability"] = rel
    res["sparsification"] = spars
    return res


class CalibrationMeter:
    """Running calibration / uncertainty totals on the device.

    ``update(prob, target, uncertainty=None)`` adds one image or batch to the
    totals (one ``calib_hist`` pass; it never synchronises the host and
    allocates nothing proportional to the image); ``compute()`` is
    ``calib_metrics`` of the totals."""

    def __init__(self, n_bins=15, u_max=math.log(2)):
        _check_bins(n_bins, u_max, "CalibrationMeter")
        self.n_bins = n_bins
        self.u_max = float(u_max)
        self.reset()

    def reset(self):
        self.updates = 0
        self._counts = None
        self._ws = None

    def update(self, prob, target, uncertainty=None):
        p, m, u = _calib_args(prob, target, uncertainty, "CalibrationMeter.update")
        if self._counts is None:
            self._counts = _new_counts(self.n_bins, self.u_max, u is not None, p.device)
            self._ws = _workspace(p.device)
        elif self._counts.conf_hist.device != p.device or (self._counts.unc_hist is None) != (u is None):
            raise ValueError("CalibrationMeter.update: the device and the presence of an uncertainty map must "
                             "match the earlier updates")
        _run(p, m, u, self._counts, self.updates > 0, self._ws)
        self.updates += 1

    def counts(self):
        """the running ``CalibCounts``"""
        if self._counts is None:
            raise RuntimeError("CalibrationMeter: no update() since the last reset()")
        return self._counts

    def compute(self):
        """dict of fp64 device tensors (``calib_metrics``; no host sync)"""
        return calib_metrics(self.counts())
