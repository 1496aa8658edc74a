"""Validation metrics, CPU side: the public names exist, CPU tensors and
mismatched batch / class sizes are refused before any launch, the dispatcher
op propagates shapes on meta tensors, and the C-ABI declarations are in the
header and the binding."""
import inspect
import os
import re

import pytest
import torch

import vaeunet_amd
from vaeunet_amd import _lib, metrics, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vu_seg_counts_workspace_bytes", "vu_seg_counts", "vu_seg_metrics")


def test_names_exported():
    for n in ("seg_counts", "seg_metrics", "iou_score", "precision_recall", "specificity", "accuracy",
              "get_all_metrics", "SegmentationMeter", "dice_score", "evaluate"):
        assert callable(getattr(vaeunet_amd, n)), n
    for n in ("seg_counts", "seg_metrics", "iou_score", "precision_recall", "specificity", "accuracy",
              "get_all_metrics", "SegmentationMeter", "METRIC_NAMES"):
        assert hasattr(metrics, n), n
    assert metrics.METRIC_NAMES == ("dice", "iou", "precision", "recall", "specificity", "accuracy")
    from vaeunet_amd.evaluate import evaluate
    assert list(inspect.signature(evaluate).parameters) == ["net", "dataloader", "device", "amp", "align_corners",
                                                            "max_batches"]
    sig = inspect.signature(evaluate)
    assert sig.parameters["amp"].default is True and sig.parameters["align_corners"].default is False
    assert list(inspect.signature(metrics.seg_counts).parameters)[:4] == ["logits", "masks", "align_corners", "out"]
    for m in ("update", "compute", "per_class", "reset"):
        assert callable(getattr(metrics.SegmentationMeter, m))


def test_cpu_tensors_refused():
    x, t = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4)
    for fn in (metrics.seg_counts, metrics.iou_score, metrics.precision_recall, metrics.specificity,
               metrics.accuracy, metrics.get_all_metrics, metrics.SegmentationMeter().update):
        with pytest.raises(RuntimeError, match=r"run on MI355X \(HIP\) devices only"):
            fn(x, t)
    with pytest.raises(RuntimeError, match=r"run on MI355X \(HIP\) devices only"):
        metrics.seg_metrics(torch.zeros(1, 4, dtype=torch.int64))
    # the same kind of error the losses raise
    from vaeunet_amd.loss import dice_loss
    with pytest.raises(RuntimeError, match=r"run on MI355X \(HIP\) devices only"):
        dice_loss(x, t)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.vaeunet.seg_counts(x, t, False)


def test_shape_mismatch_raises_value_error():
    """B or C differ: ValueError, as dice_score (the shapes are checked before the device)"""
    x = torch.zeros(2, 3, 8, 8)
    for bad in (torch.zeros(1, 3, 8, 8), torch.zeros(2, 1, 8, 8), torch.zeros(2, 3, 8)):
        for fn in (metrics.seg_counts, metrics.get_all_metrics, metrics.SegmentationMeter().update):
            with pytest.raises(ValueError):
                fn(x, bad)
    good = torch.empty(2, 3, 8, 8, device="meta")
    for bad in (torch.empty(1, 3, 8, 8, device="meta"), torch.empty(2, 1, 8, 8, device="meta"),
                torch.empty(2, 3, 8, device="meta")):
        with pytest.raises(ValueError):
            torch.ops.vaeunet.seg_counts(good, bad, False)
    with pytest.raises(ValueError):
        metrics._as_planes(torch.zeros(4, 4), torch.zeros(4, 5), "iou_score")
    # a spatial mismatch alone is the resize case, not an error
    assert torch.ops.vaeunet.seg_counts(good, torch.empty(2, 3, 16, 12, device="meta"), False).shape == (2, 3, 4)


def test_op_registered_with_fake_impl():
    assert "seg_counts" in ops.OPS
    op = torch.ops.vaeunet.seg_counts.default
    assert op._schema.name == "vaeunet::seg_counts"
    x = torch.empty(2, 3, 8, 8, device="meta", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    for md in (torch.float32, torch.uint8, torch.bool, torch.int64):
        out = torch.ops.vaeunet.seg_counts(x, torch.empty(2, 3, 20, 24, device="meta", dtype=md))
        assert out.shape == (2, 3, 4) and out.dtype == torch.int64 and out.device.type == "meta"


def test_header_declares_the_new_entry_points():
    src = open(os.path.join(ROOT, "include", "vaeunet.h")).read()
    declared = set(re.findall(r"\b(vu_[a-z0-9_]+)\s*\(", src))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in _lib.exported_symbols(), s
    # argument counts of the declarations match the binding
    for s in NEW_SYMBOLS:
        m = re.search(r"\b" + s + r"\s*\(([^;]*?)\)\s*;", src, re.S)
        assert m, s
        nargs = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert nargs == len(_lib._SIGS[s][1]), (s, nargs)


def test_library_exports_the_new_entry_points():
    import ctypes
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.vu_seg_counts_workspace_bytes is not None
    h = _lib.lib()
    # 3 unsigned 64-bit partials per stage-1 block; at least the block cap, at least one block per plane
    assert h.vu_seg_counts_workspace_bytes(1) == h.vu_seg_counts_workspace_bytes(8) >= 1024 * 24
    assert h.vu_seg_counts_workspace_bytes(5000) == 5000 * 24
