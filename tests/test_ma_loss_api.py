"""MAFocalLoss / MASegmentationLoss / focal_dice_loss, CPU side: the names and
signatures exist, CPU tensors, mismatched shapes and bad constants are
refused before any launch, the dispatcher op propagates shapes on meta
tensors, and the C-ABI declarations are in the header, the binding and the
built library."""
import inspect
import os
import re

import pytest
import torch

from vaeunet_amd import _lib, loss, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vu_focal_workspace_bytes", "vu_focal_dice_fwd", "vu_focal_dice_bwd")
CPU_MSG = r"run on MI355X \(HIP\) devices only"


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect._empty}


def test_names_and_signatures():
    for n in ("MAFocalLoss", "MASegmentationLoss", "focal_dice_loss"):
        assert callable(getattr(loss, n)), n
    assert _defaults(loss.MAFocalLoss.__init__) == {"alpha": 0.75, "gamma": 2.0, "reduction": "mean"}
    assert _defaults(loss.MASegmentationLoss.__init__) == {"focal_weight": 0.5, "dice_weight": 0.5, "alpha": 0.75,
                                                           "gamma": 2.0, "smooth": 1.0}
    assert list(inspect.signature(loss.focal_dice_loss).parameters)[:2] == ["inputs", "targets"]
    d = _defaults(loss.focal_dice_loss)
    assert d == {"alpha": 0.75, "gamma": 2.0, "smooth": 1.0, "focal_weight": 0.5, "dice_weight": 0.5,
                 "reduction": "mean"}
    assert issubclass(loss.MAFocalLoss, torch.nn.Module) and issubclass(loss.MASegmentationLoss, torch.nn.Module)
    assert loss.MASegmentationLoss().last_parts is None
    # the existing names are still there
    for n in ("CombinedLoss", "DiceLoss", "dice_loss", "KLAnnealer", "kl_with_free_bits"):
        assert hasattr(loss, n), n


def test_cpu_tensors_refused():
    x, t = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4)
    for fn in (loss.MAFocalLoss(), loss.MASegmentationLoss(), loss.focal_dice_loss, loss.MAFocalLoss(reduction="sum")):
        with pytest.raises(RuntimeError, match=CPU_MSG):
            fn(x, t)
    with pytest.raises(RuntimeError, match=CPU_MSG):   # the same message the existing losses raise
        loss.dice_loss(x, t)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.vaeunet.focal_dice_loss(x, t, 0.75, 2.0, 1.0, 0.5, 0.5, False)


def test_shape_mismatch_raises_value_error():
    x = torch.zeros(2, 3, 8, 8)
    for bad in (torch.zeros(1, 3, 8, 8), torch.zeros(2, 1, 8, 8), torch.zeros(2, 3, 8), torch.zeros(2 * 3 * 8 * 8)):
        for fn in (loss.MAFocalLoss(), loss.MASegmentationLoss(), loss.focal_dice_loss):
            with pytest.raises(ValueError, match="shape"):
                fn(x, bad)
    good = torch.empty(2, 3, 8, 8, device="meta")
    with pytest.raises(ValueError, match="shape"):
        torch.ops.vaeunet.focal_dice_loss(good, torch.empty(2, 3, 8, device="meta"), 0.75, 2.0, 1.0, 0.5, 0.5, False)


@pytest.mark.parametrize("kw", [dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(gamma=0.5),
                                dict(gamma=-1.0), dict(gamma=0.999), dict(reduction="none"), dict(reduction=None)])
def test_bad_constants_raise_before_any_device_use(kw):
    """ValueError from the constructor, and from the functional form even on
    CPU tensors (the constants are checked before the device)."""
    x, t = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4)
    with pytest.raises(ValueError):
        loss.MAFocalLoss(**kw)
    with pytest.raises(ValueError):
        loss.focal_dice_loss(x, t, **kw)
    if "reduction" not in kw:
        with pytest.raises(ValueError):
            loss.MASegmentationLoss(**kw)


@pytest.mark.parametrize("smooth", [0.0, -1.0, float("nan")])
def test_bad_smooth_raises(smooth):
    x, t = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4)
    with pytest.raises(ValueError):
        loss.MASegmentationLoss(smooth=smooth)
    with pytest.raises(ValueError):
        loss.focal_dice_loss(x, t, smooth=smooth)
    m = torch.empty(1, 1, 4, 4, device="meta")
    with pytest.raises(ValueError):
        torch.ops.vaeunet.focal_dice_loss(m, m, 0.75, 2.0, smooth, 0.5, 0.5, False)
    with pytest.raises(ValueError):
        torch.ops.vaeunet.focal_dice_loss(m, m, 0.75, 0.5, 1.0, 0.5, 0.5, False)


def test_valid_constants_accepted():
    for g in (0, 0.0, 1, 1.0, 2.0, 2.5, 5):
        loss.MAFocalLoss(gamma=g)
        loss.MASegmentationLoss(gamma=g)
    for a in (0, 0.0, 0.25, 1, 1.0):
        loss.MAFocalLoss(alpha=a, reduction="sum")


def test_op_registered_with_fake_impl():
    assert "focal_dice_loss" in ops.OPS
    assert "focal_dice_loss" in ops.__doc__
    op = torch.ops.vaeunet.focal_dice_loss.default
    assert op._schema.name == "vaeunet::focal_dice_loss"
    assert [a.name for a in op._schema.arguments] == ["logits", "target", "alpha", "gamma", "smooth", "w_focal",
                                                      "w_dice", "sum_reduction"]
    for shape in ((2, 1, 8, 8), (2, 3, 9, 7), (5,), (3, 4, 5, 6, 7)):
        x = torch.empty(shape, device="meta")
        for red in (False, True):
            out, sums = torch.ops.vaeunet.focal_dice_loss(x, torch.empty(shape, device="meta"), 0.75, 2.0, 1.0, 0.5,
                                                          0.5, red)
            assert out.shape == () and out.dtype == torch.float32 and out.device.type == "meta"
            assert sums.shape == (5,) and sums.dtype == torch.float64 and sums.device.type == "meta"


def test_header_declares_the_new_entry_points():
    src = open(os.path.join(ROOT, "include", "vaeunet.h")).read()
    declared = set(re.findall(r"\b(vu_[a-z0-9_]+)\s*\(", src))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in _lib.exported_symbols(), s
        m = re.search(r"\b" + s + r"\s*\(([^;]*?)\)\s*;", src, re.S)
        assert m, s
        nargs = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert nargs == len(_lib._SIGS[s][1]), (s, nargs)
    assert len(_lib._SIGS["vu_focal_dice_fwd"][1]) == 14 and len(_lib._SIGS["vu_focal_dice_bwd"][1]) == 13


def test_library_exports_the_new_entry_points():
    import ctypes
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    h = _lib.lib()
    # five fp64 partials per stage-1 block, for a block cap of at most 2048
    nbytes = h.vu_focal_workspace_bytes()
    assert nbytes % 40 == 0 and 40 <= nbytes <= 2048 * 40
