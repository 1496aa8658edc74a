"""Host side of the signed distance map and the boundary loss
(vaeunet_amd.surface.signed_distance, vaeunet_amd.loss.boundary_loss /
BoundaryLoss / BoundaryAugmentedLoss), no GPU: the names and
signatures, every ValueError raised with CPU tensors before a device is
touched, the RuntimeError for CPU tensors, both dispatcher ops on meta tensors,
and the new symbols and VU_SDF_MAX_W in the header, the binding and the built
library."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"vu_sdf": 10, "vu_boundary_loss_workspace_bytes": 0, "vu_boundary_loss_fwd": 7, "vu_boundary_loss_bwd": 6}
CPU_MSG = r"run on MI355X \(HIP\) devices only"


def _no_device(monkeypatch):
    import vaeunet_amd.loss as L
    import vaeunet_amd.surface as S

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    for mod in (S, L):
        for name in ("call", "query"):
            monkeypatch.setattr(mod, name, no_device)
    monkeypatch.setattr(S, "_launch_sdf", no_device)
    monkeypatch.setattr(torch.Tensor, "to", no_device)
    monkeypatch.setattr(torch.Tensor, "contiguous", no_device)
    return S, L


def _u8(*shape):
    return torch.zeros(shape or (2, 1, 8, 9), dtype=torch.uint8)


def _f32(*shape):
    return torch.zeros(shape or (2, 1, 8, 9), dtype=torch.float32)


def test_names_signatures_and_exports():
    import vaeunet_amd
    from vaeunet_amd import loss, surface
    for n in ("signed_distance", "boundary_loss", "BoundaryLoss", "BoundaryAugmentedLoss"):
        assert callable(getattr(vaeunet_amd, n)), n
    assert vaeunet_amd.signed_distance is surface.signed_distance and vaeunet_amd.boundary_loss is loss.boundary_loss
    sig = inspect.signature(surface.signed_distance)
    assert list(sig.parameters) == ["x", "threshold", "squared", "clip"]
    assert [p.default for p in sig.parameters.values()][1:] == [None, False, None]
    sig = inspect.signature(loss.boundary_loss)
    assert list(sig.parameters) == ["inputs", "targets", "phi", "clip", "threshold"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("phi", "clip", "threshold"))
    assert all(sig.parameters[k].default is None for k in ("targets", "phi", "clip", "threshold"))
    assert list(inspect.signature(loss.BoundaryLoss).parameters) == ["clip"]
    sig = inspect.signature(loss.BoundaryAugmentedLoss)
    assert list(sig.parameters) == ["base", "weight", "clip"]
    assert (sig.parameters["weight"].default, sig.parameters["clip"].default) == (0.01, None)
    assert issubclass(loss.BoundaryLoss, torch.nn.Module) and issubclass(loss.BoundaryAugmentedLoss, torch.nn.Module)
    crit = loss.BoundaryAugmentedLoss(loss.MASegmentationLoss(), weight=0.25, clip=20)
    assert crit.last_parts is None and crit.weight.shape == () and crit.weight.dtype == torch.float32
    assert "weight" in dict(crit.named_buffers()) and float(crit.weight) == 0.25
    crit.set_weight(0.5)
    assert float(crit.weight) == 0.5
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            crit.set_weight(bad)
        with pytest.raises(ValueError):
            loss.BoundaryAugmentedLoss(loss.MASegmentationLoss(), weight=bad)
    with pytest.raises(ValueError):
        loss.BoundaryAugmentedLoss(None)
    # the existing names are still there
    for n in ("CombinedLoss", "MASegmentationLoss", "focal_dice_loss", "KLAnnealer"):
        assert hasattr(loss, n), n
    for n in ("distance_transform", "boundary", "surface_stats", "SurfaceMeter"):
        assert hasattr(surface, n), n


def test_signed_distance_validates_before_touching_a_device(monkeypatch):
    S, _ = _no_device(monkeypatch)
    fn = S.signed_distance
    for bad in (_u8(8, 9), _u8(2, 1, 0, 9), torch.zeros(2, 1, 8, 9, dtype=torch.int32),
                torch.zeros(2, 1, 8, 9, dtype=torch.float64), np.zeros((2, 1, 8, 9), np.uint8), None):
        with pytest.raises(ValueError):
            fn(bad, threshold=0.5)
    with pytest.raises(ValueError, match="needs a threshold"):
        fn(_f32())
    with pytest.raises(ValueError):
        fn(_f32(), threshold=float("nan"))
    for clip in (0, 0.0, -1.0, float("nan"), "2", True):
        with pytest.raises(ValueError, match="clip"):
            fn(_u8(), clip=clip)
    with pytest.raises(ValueError, match="squared"):
        fn(_u8(), squared=True, clip=2.0)
    assert S.VU_SDF_MAX_W == 8192
    for shape, msg in (((1, 1, 2, 8193), "W <= 8192"), ((1, 1, 16385, 2), "exceeds the distance transform")):
        with pytest.raises(ValueError, match=msg):
            fn(torch.empty(shape, dtype=torch.uint8, device="meta"))
    for x, kw in ((_u8(), {}), (_u8().bool(), dict(squared=True)), (_f32(), dict(threshold=0.5, clip=3.0)),
                  (_u8(1, 1, 1, 1), dict(clip=float("inf")))):
        with pytest.raises(RuntimeError, match=CPU_MSG):
            fn(x, **kw)


def test_boundary_loss_validates_before_touching_a_device(monkeypatch):
    _, L = _no_device(monkeypatch)
    x, t, f = _f32(), _u8(), _f32()
    forms = (L.boundary_loss, )
    for fn in forms:
        for args, kw in (((x,), {}), ((x, t), dict(phi=f)),                           # neither, both
                         ((x, _u8(2, 1, 8, 8)), {}), ((x, _u8(8, 9)), {}), ((x, None), dict(phi=_f32(2, 1, 8, 8))),
                         ((x, None), dict(phi=f.double())), ((x, None), dict(phi=t)),
                         ((x, None), dict(phi=f, clip=2.0)), ((x, None), dict(phi=f, threshold=0.5)),
                         ((_f32(2, 1, 0, 9), _u8(2, 1, 0, 9)), {}), ((_f32(9), _u8(9)), {}),
                         ((_f32(1, 2, 1, 8, 9), _u8(1, 2, 1, 8, 9)), {}), ((None, t), {}),
                         ((x, t), dict(clip=0.0)), ((x, t), dict(clip=-2.0)), ((x, t), dict(clip=float("nan"))),
                         ((x, _f32()), dict(threshold=float("nan")))):
            with pytest.raises(ValueError):
                fn(*args, **kw)
    wide_x = torch.empty(1, 1, 2, 8193, device="meta")
    with pytest.raises(ValueError, match="8192"):
        L.boundary_loss(wide_x, torch.empty(1, 1, 2, 8193, dtype=torch.uint8, device="meta"))
    for clip in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            L.BoundaryLoss(clip=clip)
        with pytest.raises(ValueError):
            L.BoundaryAugmentedLoss(L.MASegmentationLoss(), clip=clip)
    with pytest.raises(ValueError, match="shape"):
        L.BoundaryLoss()(x, _u8(2, 1, 8, 8))
    with pytest.raises(ValueError, match="shape"):
        L.BoundaryAugmentedLoss(L.MASegmentationLoss())(x, _u8(2, 1, 8, 8))
    # valid arguments on the CPU: the device is what is missing
    for args, kw in (((x, t), {}), ((x, t.bool()), dict(clip=4.0)), ((x, _f32()), dict(threshold=0.25)),
                     ((x, None), dict(phi=f)), ((_f32(2, 8, 9), _u8(2, 8, 9)), {}), ((x, t.long()), {})):
        with pytest.raises(RuntimeError, match=CPU_MSG):
            L.boundary_loss(*args, **kw)
    with pytest.raises(RuntimeError, match=CPU_MSG):
        L.BoundaryLoss(clip=3)(x, t)


def test_augmented_loss_refuses_cpu_tensors():
    from vaeunet_amd import loss
    with pytest.raises(RuntimeError, match=CPU_MSG):
        loss.BoundaryAugmentedLoss(loss.MASegmentationLoss())(_f32(), _f32())


def test_ops_registered_with_fake_impls_and_refuse_cpu():
    from vaeunet_amd import ops
    v = torch.ops.vaeunet
    for n in ("signed_distance", "boundary_loss"):
        assert n in ops.OPS and n in ops.__doc__
        assert getattr(v, n).default._schema.name == f"vaeunet::{n}"
    assert [a.name for a in v.signed_distance.default._schema.arguments] == ["x", "threshold", "squared", "clip"]
    assert [a.name for a in v.boundary_loss.default._schema.arguments] == ["logits", "phi"]

    def m(*shape, dtype=torch.uint8):
        return torch.empty(shape, device="meta", dtype=dtype)
    for x, kw in ((m(2, 3, 20, 12), {}), (m(2, 3, 20, 12, dtype=torch.bool), dict(clip=5.0)),
                  (m(1, 1, 1, 1, dtype=torch.float32), dict(threshold=0.5)), (m(1, 1, 3, 8192), {})):
        y = v.signed_distance(x, **kw)
        assert y.shape == x.shape and y.dtype == torch.float32 and y.device.type == "meta"
    y = v.signed_distance(m(2, 3, 20, 12), None, True)
    assert y.shape == (2, 3, 20, 12) and y.dtype == torch.int32
    for x, kw in ((m(2, 3, 20, 12, dtype=torch.float32), {}), (m(3, 20, 12), {}), (m(1, 1, 2, 8193), {}),
                  (m(1, 1, 16385, 2), {}), (m(2, 3, 20, 12, dtype=torch.int32), {}), (m(2, 3, 20, 12), dict(clip=0.0)),
                  (m(2, 3, 20, 12), dict(squared=True, clip=1.0))):
        with pytest.raises(ValueError):
            v.signed_distance(x, **kw)
    for shape in ((2, 1, 8, 8), (2, 3, 9, 7), (5,)):
        loss, sums = v.boundary_loss(m(*shape, dtype=torch.float32), m(*shape, dtype=torch.float32))
        assert loss.shape == () and loss.dtype == torch.float32 and loss.device.type == "meta"
        assert sums.shape == (3,) and sums.dtype == torch.float64
    with pytest.raises(ValueError, match="shape"):
        v.boundary_loss(m(2, 3, 8, 8, dtype=torch.float32), m(2, 3, 8, dtype=torch.float32))
    with pytest.raises((NotImplementedError, RuntimeError)):
        v.signed_distance(_u8())
    with pytest.raises((NotImplementedError, RuntimeError)):
        v.boundary_loss(_f32(), _f32())


def test_binding_declares_the_entry_points_and_the_constant():
    from vaeunet_amd import _lib
    src = open(os.path.join(ROOT, "include", "vaeunet.h")).read()
    for name, nargs in SYMBOLS.items():
        m = re.search(r"(int|int64_t) %s\(([^;]*)\);" % name, src)
        assert m and name in _lib.exported_symbols(), name
        res, args = _lib._SIGS[name]
        assert res is (_lib._i if m.group(1) == "int" else _lib._l), name
        decl = [a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
        assert len(decl) == len(args) == nargs, name
        for arg, ct in zip(decl, args):
            assert ("*" in arg) == (ct is _lib._p), (name, arg)
            if "*" not in arg:
                want = {"int": _lib._i, "int64_t": _lib._l, "float": _lib._f}
                assert ct is want[arg.split()[0]], (name, arg)
    assert re.search(r"#define VU_SDF_MAX_W 8192\b", src) and _lib.VU_SDF_MAX_W == 8192
    assert _lib.VU_SDF_MAX_W * 4 <= 32768 and _lib.VU_SDF_MAX_W <= _lib.VU_EDT_MAX_DIM


def test_library_exports_the_entry_points():
    import ctypes
    from vaeunet_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    # three fp64 partials per stage-1 block, for a block cap of at most 2048 (host-only: a size, no device)
    nbytes = _lib.query("vu_boundary_loss_workspace_bytes")
    assert nbytes % 24 == 0 and 24 <= nbytes <= 2048 * 24
