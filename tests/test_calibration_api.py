"""Calibration / uncertainty metrics, CPU side: the public names exist, the
dispatcher op is registered and propagates shapes on meta tensors, CPU tensors,
too many bins and mismatched shapes are refused before any launch, and the
C-ABI declarations are in the header, the binding and the library."""
import ctypes
import math
import os
import re

import pytest
import torch

import vaeunet_amd
from vaeunet_amd import _lib, calibration, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vu_calib_workspace_bytes", "vu_calib_hist", "vu_calib_metrics")


def test_names_exported():
    for n in ("calib_hist", "calib_metrics", "CalibrationMeter"):
        assert callable(getattr(vaeunet_amd, n)), n
        assert getattr(vaeunet_amd, n) is getattr(calibration, n)
    for m in ("update", "compute", "reset", "counts"):
        assert callable(getattr(calibration.CalibrationMeter, m))
    assert calibration.RANK_BINS == 1024 and calibration.MAX_CONF_BINS == 64
    meter = calibration.CalibrationMeter()
    assert meter.n_bins == 15 and meter.u_max == math.log(2)
    with pytest.raises(RuntimeError, match="no update"):
        meter.counts()


def test_op_registered_with_schema():
    assert "calib_hist" in ops.OPS
    schema = torch.ops.vaeunet.calib_hist.default._schema
    assert schema.name == "vaeunet::calib_hist"
    assert [a.name for a in schema.arguments] == ["prob", "target", "uncertainty", "n_bins", "u_max"]
    assert len(schema.returns) == 1 and str(schema.returns[0].type) == "List[Tensor]"


@pytest.mark.parametrize("nb", [15, 64])
@pytest.mark.parametrize("mdtype", [torch.float32, torch.uint8, torch.bool, torch.int64])
def test_fake_impl_shapes(nb, mdtype):
    p = torch.empty(2, 1, 12, 10, device="meta")
    m = torch.empty(2, 1, 12, 10, device="meta", dtype=mdtype)
    names = ("conf_hist", "conf_sum", "rank_hist", "unc_hist", "sums", "invalid")
    for u, unc_rows in ((torch.empty(2, 1, 12, 10, device="meta"), 1024), (None, 0)):
        out = dict(zip(names, torch.ops.vaeunet.calib_hist(p, m, u, n_bins=nb)))
        assert all(t.device.type == "meta" for t in out.values())
        assert out["conf_hist"].shape == (nb, 2) and out["conf_hist"].dtype == torch.int64
        assert out["conf_sum"].shape == (nb,) and out["conf_sum"].dtype == torch.float64
        assert out["rank_hist"].shape == (1024, 2) and out["rank_hist"].dtype == torch.int64
        assert out["unc_hist"].shape == (unc_rows, 2) and out["unc_hist"].dtype == torch.int64
        assert out["sums"].shape == (2,) and out["sums"].dtype == torch.float64
        assert out["invalid"].shape == (2,) and out["invalid"].dtype == torch.int64


def test_cpu_tensors_refused():
    p, t = torch.rand(1, 1, 4, 4), torch.zeros(1, 1, 4, 4)
    for fn in (calibration.calib_hist, calibration.CalibrationMeter().update):
        with pytest.raises(RuntimeError, match=r"run on MI355X \(HIP\) devices only"):
            fn(p, t)
        with pytest.raises(RuntimeError, match=r"run on MI355X \(HIP\) devices only"):
            fn(p, t, p)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.vaeunet.calib_hist(p, t)


def test_bad_arguments_raise_value_error():
    p, t = torch.rand(2, 8), torch.zeros(2, 8)
    for nb in (65, 0, 1000, 15.0):
        with pytest.raises(ValueError, match="n_bins"):
            calibration.calib_hist(p, t, n_bins=nb)
        with pytest.raises(ValueError, match="n_bins"):
            calibration.CalibrationMeter(n_bins=nb)
    for bad_u_max in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="u_max"):
            calibration.calib_hist(p, t, u_max=bad_u_max)
    for fn in (calibration.calib_hist, calibration.CalibrationMeter().update):
        with pytest.raises(ValueError, match="Shape mismatch"):
            fn(p, torch.zeros(2, 7))
        with pytest.raises(ValueError, match="Shape mismatch"):
            fn(p, t, torch.zeros(8, 2))
    meta = torch.empty(2, 8, device="meta")
    with pytest.raises(ValueError):
        torch.ops.vaeunet.calib_hist(meta, torch.empty(2, 7, device="meta"))
    with pytest.raises(ValueError):
        torch.ops.vaeunet.calib_hist(meta, meta, None, 65)


def test_header_binding_and_library_agree():
    src = open(os.path.join(ROOT, "include", "vaeunet.h")).read()
    assert re.search(r"#define\s+VU_CALIB_RANK_BINS\s+1024\b", src)
    assert re.search(r"#define\s+VU_CALIB_NSCALARS\s+%d\b" % len(calibration.SCALAR_NAMES), src)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        m = re.search(r"\b" + s + r"\s*\(([^;]*?)\)\s*;", src, re.S)
        assert m, s
        nargs = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert s in _lib.exported_symbols() and nargs == len(_lib._SIGS[s][1]), (s, nargs)
        assert hasattr(lib, s), s
    # per-block fp64 partials: 64 confidence bins + Brier + NLL for every stage-1 block
    assert _lib.lib().vu_calib_workspace_bytes() % ((64 + 2) * 8) == 0
