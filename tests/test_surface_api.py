"""Host side of the boundary metrics (vaeunet_amd.surface), no
GPU: every ValueError is raised before a device is touched, CPU tensors get a
RuntimeError, the header prototypes and VU_EDT_* constants against the binding,
the registration and fake implementation of torch.ops.vaeunet.distance_transform,
and the signatures of evaluate / evaluate_with_surface."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"vu_edt_workspace_bytes": 3, "vu_edt": 10, "vu_edt_boundary": 8, "vu_surface_stats": 14,
           "vu_surface_metrics": 7}
CONSTANTS = {"VU_EDT_TO_FOREGROUND": 0, "VU_EDT_TO_BACKGROUND": 1, "VU_EDT_TO_BOUNDARY": 2, "VU_EDT_INF": 2 ** 31 - 1,
             "VU_EDT_MAX_DIM": 16384}


def _no_device(monkeypatch):
    import vaeunet_amd.surface as S

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    for name in ("_stats", "call", "query"):
        monkeypatch.setattr(S, name, no_device)
    monkeypatch.setattr(torch.Tensor, "to", no_device)
    monkeypatch.setattr(torch.Tensor, "contiguous", no_device)
    return S


def _u8(*shape):
    return torch.zeros(shape or (2, 1, 8, 9), dtype=torch.uint8)


def _f32(*shape):
    return torch.zeros(shape or (2, 1, 8, 9), dtype=torch.float32)


def test_transform_and_boundary_validate_before_touching_a_device(monkeypatch):
    S = _no_device(monkeypatch)
    for fn in (S.distance_transform, S.boundary):
        for bad in (_u8(8, 9), _u8(2, 1, 0, 9), torch.zeros(2, 1, 8, 9, dtype=torch.int32),
                    torch.zeros(2, 1, 8, 9, dtype=torch.float64), torch.zeros(2, 1, 8, 9, dtype=torch.bfloat16),
                    np.zeros((2, 1, 8, 9), np.uint8), None):
            with pytest.raises(ValueError):
                fn(bad, threshold=0.5)
        with pytest.raises(ValueError, match="needs a threshold"):
            fn(_f32())
        with pytest.raises(ValueError):
            fn(_f32(), threshold=float("nan"))
        for x, kw in ((_u8(), {}), (_u8().bool(), {}), (_f32(), dict(threshold=0.5)), (_u8(1, 1, 1, 1), {})):
            with pytest.raises(RuntimeError, match=r"run on MI355X \(HIP\) devices only"):
                fn(x, **kw)
    for mode in ("nearest", "", None, 1, "Background"):
        with pytest.raises(ValueError, match="mode must be one of"):
            S.distance_transform(_u8(), mode=mode)
    for mode in S.MODES:
        for squared in (True, False):
            with pytest.raises(RuntimeError):
                S.distance_transform(_u8(), mode=mode, squared=squared)
    assert S.MODES == {"foreground": 0, "background": 1, "boundary": 2}


def test_a_dimension_above_the_cap_is_refused(monkeypatch):
    S = _no_device(monkeypatch)
    assert S.VU_EDT_MAX_DIM == 16384
    for shape in ((1, 1, 16385, 2), (1, 1, 2, 16385)):
        huge = torch.empty(shape, dtype=torch.uint8, device="meta")     # a shape, no storage
        for fn in (S.distance_transform, S.boundary, lambda x: S.surface_stats(x, x),
                   lambda x: S.SurfaceMeter().update(x, x)):
            with pytest.raises(ValueError, match="exceeds the distance transform"):
                fn(huge)


def test_stats_and_meter_validate_before_touching_a_device(monkeypatch):
    S = _no_device(monkeypatch)
    for fn in (S.surface_stats, S.SurfaceMeter().update):
        for pred, masks in ((_u8(), _u8(2, 1, 8, 8)), (_u8(), _u8(8, 9)), (_u8(8, 9), _u8()), (_f32().double(), _u8()),
                            (_u8(2, 1, 0, 9), _u8(2, 1, 0, 9)), (_u8(), None)):
            with pytest.raises(ValueError):
                fn(pred, masks)
        for pred, masks in ((_u8(), _u8()), (_f32(), _f32()), (_u8().bool(), _u8()), (_f32(), _u8().long())):
            with pytest.raises(RuntimeError, match=r"run on MI355X \(HIP\) devices only"):
                fn(pred, masks)
    bad_kw = (dict(percentile=0), dict(percentile=101), dict(percentile=95.0), dict(percentile="95"),
              dict(percentile=True), dict(percentile=None), dict(tolerance=-1.0), dict(tolerance=-1e-9),
              dict(tolerance=float("nan")), dict(tolerance=float("inf")), dict(tolerance=None), dict(tolerance="1"),
              dict(tolerance=True), dict(tolerance=40000.0))
    for kw in bad_kw + (dict(threshold=None), dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            S.surface_stats(_f32(), _u8(), **kw)
    for kw in bad_kw + (dict(threshold=float("nan")),):
        with pytest.raises(ValueError):
            S.SurfaceMeter(**kw)
    m = S.SurfaceMeter()
    assert (m.threshold, m.percentile, m.tolerance, m.tol2) == (0.5, 95, 1.0, 1)
    assert S.SurfaceMeter(tolerance=2.5).tol2 == 6 and S.SurfaceMeter(tolerance=0).tol2 == 0
    assert S.SurfaceMeter(tolerance=1.4142135623730951).tol2 == 2          # (int)(t t) in fp64: 2.0000000000000004
    assert S.SurfaceMeter(tolerance=1.414213562373095).tol2 == 1
    for call in (m.counts, m.values, m.compute):
        with pytest.raises(RuntimeError, match="no update"):
            call()
    ok_st, ok_sm = torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.float64)
    for st, sm in ((torch.zeros(2, 7, dtype=torch.int64), ok_sm), (torch.zeros(2, 8), ok_sm), (ok_st, torch.zeros(2, 2)),
                   (ok_st, torch.zeros(3, 2, dtype=torch.float64)), (ok_st, torch.zeros(2, 3, dtype=torch.float64)),
                   (torch.zeros(0, 8, dtype=torch.int64), torch.zeros(0, 2, dtype=torch.float64)), (None, ok_sm),
                   (ok_st, None)):
        with pytest.raises(ValueError):
            S.surface_metrics(st, sm)
    with pytest.raises(RuntimeError, match=r"run on MI355X \(HIP\) devices only"):
        S.surface_metrics(ok_st, ok_sm)


def test_names_exported():
    import vaeunet_amd
    from vaeunet_amd import surface
    for n in ("distance_transform", "boundary", "surface_stats", "surface_metrics", "SurfaceMeter",
              "evaluate_with_surface"):
        assert callable(getattr(vaeunet_amd, n)), n
    for m in ("update", "values", "counts", "compute", "reset"):
        assert callable(getattr(surface.SurfaceMeter, m))
    sig = inspect.signature(surface.distance_transform)
    assert list(sig.parameters) == ["x", "mode", "threshold", "squared"]
    assert (sig.parameters["mode"].default, sig.parameters["threshold"].default, sig.parameters["squared"].default) \
        == ("background", None, True)
    assert list(inspect.signature(surface.boundary).parameters) == ["x", "threshold"]
    sig = inspect.signature(surface.surface_stats)
    assert list(sig.parameters) == ["pred", "masks", "threshold", "percentile", "tolerance"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [0.5, 95, 1.0]
    assert list(inspect.signature(surface.surface_metrics).parameters) == ["stats", "sums"]
    sig = inspect.signature(surface.SurfaceMeter)
    assert list(sig.parameters) == ["threshold", "percentile", "tolerance"]
    assert [p.default for p in sig.parameters.values()] == [0.5, 95, 1.0]
    assert surface.SURFACE_METRIC_NAMES == ("hd", "hd_q", "assd", "nsd") and len(surface.STAT_NAMES) == 8


def test_evaluate_keeps_its_signature_and_the_surface_loop_has_its_own():
    from vaeunet_amd.evaluate import evaluate, evaluate_with_lesions, evaluate_with_surface
    assert list(inspect.signature(evaluate).parameters) == ["net", "dataloader", "device", "amp", "align_corners",
                                                            "max_batches"]
    assert list(inspect.signature(evaluate_with_lesions).parameters) == ["net", "dataloader", "device", "lesion_meter",
                                                                         "amp", "align_corners", "max_batches"]
    sig = inspect.signature(evaluate_with_surface)
    assert list(sig.parameters) == ["net", "dataloader", "device", "surface_meter", "lesion_meter", "amp",
                                    "align_corners", "max_batches"]
    assert sig.parameters["lesion_meter"].default is None and sig.parameters["amp"].default is True
    assert sig.parameters["align_corners"].default is False and sig.parameters["max_batches"].default is None
    with pytest.raises(ValueError, match="surface_meter is required"):
        evaluate_with_surface(None, [], "cpu", None)


def test_binding_declares_the_entry_points_and_constants():
    from vaeunet_amd import _lib
    src = open(os.path.join(ROOT, "include", "vaeunet.h")).read()
    for name, nargs in SYMBOLS.items():
        m = re.search(r"(int|int64_t) %s\(([^;]*)\);" % name, src)
        assert m and name in _lib.exported_symbols(), name
        res, args = _lib._SIGS[name]
        assert res is (_lib._i if m.group(1) == "int" else _lib._l), name
        decl = m.group(2).split(",")
        assert len(decl) == len(args) == nargs, name
        for arg, ct in zip(decl, args):
            assert ("*" in arg) == (ct is _lib._p), (name, arg)
            if "*" not in arg:
                want = {"int": _lib._i, "int64_t": _lib._l, "float": _lib._f, "double": _lib.C.c_double}
                assert ct is want[arg.split()[0]], (name, arg)
    for k, v in CONSTANTS.items():
        assert re.search(r"#define %s %d\b" % (k, v), src) and getattr(_lib, k) == v, k


def test_library_exports_the_entry_points():
    import ctypes
    from vaeunet_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    q = _lib.query                                    # host-only: sizes, no device
    assert q("vu_edt_workspace_bytes", 1, 16385, 1) == -1 and q("vu_edt_workspace_bytes", 1, 1, 16385) == -1
    assert q("vu_edt_workspace_bytes", -1, 4, 4) == -1 and q("vu_edt_workspace_bytes", 1, -4, 4) == -1
    assert q("vu_edt_workspace_bytes", 0, 4, 4) == 0
    one, two = q("vu_edt_workspace_bytes", 1, 5, 7), q("vu_edt_workspace_bytes", 2, 5, 7)
    assert one >= 2 * 4 * 35 and two == 2 * one and one % 8 == 0
    assert q("vu_edt_workspace_bytes", 6, 16384, 16384) > 6 * 2 * 4 * 2 ** 28       # 64-bit sizes


def test_op_registered_with_a_fake_impl_and_refuses_cpu():
    from vaeunet_amd import ops
    assert "distance_transform" in ops.OPS and "distance_transform" in ops.__doc__
    dt = torch.ops.vaeunet.distance_transform
    assert dt.default._schema.name == "vaeunet::distance_transform"

    def m(*shape, dtype=torch.uint8):
        return torch.empty(shape, device="meta", dtype=dtype)
    for x, kw in ((m(2, 3, 20, 12), {}), (m(2, 3, 20, 12, dtype=torch.bool), dict(mode="boundary")),
                  (m(1, 1, 1, 1, dtype=torch.float32), dict(threshold=0.5, mode="foreground"))):
        y = dt(x, **kw)
        assert y.shape == x.shape and y.dtype == torch.int32 and y.device.type == "meta"
        y = dt(x, squared=False, **kw)
        assert y.shape == x.shape and y.dtype == torch.float32
    for x, kw in ((m(2, 3, 20, 12), dict(mode="nearest")), (m(2, 3, 20, 12, dtype=torch.float32), {}),
                  (m(3, 20, 12), {}), (m(1, 1, 16385, 2), {}), (m(2, 3, 20, 12, dtype=torch.int32), {})):
        with pytest.raises(ValueError):
            dt(x, **kw)
    with pytest.raises((NotImplementedError, RuntimeError)):
        dt(torch.zeros(1, 1, 4, 4, dtype=torch.uint8))
