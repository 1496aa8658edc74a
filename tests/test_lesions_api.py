"""Host side of the lesion-level evaluation (vaeunet_amd.lesions, DESIGN.md
§4.11), no GPU: validation before a device is touched, the header prototypes
against the binding, the registration and fake implementations of
torch.ops.vaeunet.label_components / remove_small_components, the signatures
of evaluate / evaluate_with_lesions, and the numpy reference
(tests/lesions_ref.py): against scipy.ndimage.label where scipy is present,
and its own invariants."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import lesions_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"vu_ccl_workspace_bytes": 3, "vu_ccl_label": 10, "vu_ccl_remove_small": 9, "vu_lesion_match": 14,
           "vu_lesion_metrics": 6, "vu_froc_metrics": 10}


# ----------------------------------------------------------------------------
# validation before a device is touched
# ----------------------------------------------------------------------------
def _no_device(monkeypatch):
    import vaeunet_amd.lesions as L

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    for name in ("_launch_label", "_launch_remove_small", "_match", "call", "query"):
        monkeypatch.setattr(L, name, no_device)
    monkeypatch.setattr(torch.Tensor, "to", no_device)
    monkeypatch.setattr(torch.Tensor, "contiguous", no_device)
    return L


def _u8(*shape):
    return torch.zeros(shape or (2, 1, 8, 9), dtype=torch.uint8)


def _f32(*shape):
    return torch.zeros(shape or (2, 1, 8, 9), dtype=torch.float32)


def test_labelling_validates_before_touching_a_device(monkeypatch):
    L = _no_device(monkeypatch)
    for fn in (L.label_components, lambda x, **k: L.remove_small_components(x, 2, **k)):
        for bad in (_u8(8, 9), _u8(2, 1, 0, 9), torch.zeros(2, 1, 8, 9, dtype=torch.int32),
                    torch.zeros(2, 1, 8, 9, dtype=torch.float64), torch.zeros(2, 1, 8, 9, dtype=torch.bfloat16),
                    np.zeros((2, 1, 8, 9), np.uint8), None):
            with pytest.raises(ValueError):
                fn(bad, threshold=0.5)
        for conn in (6, 0, "8", None, True, 4.5):
            with pytest.raises(ValueError):
                fn(_u8(), connectivity=conn)
        with pytest.raises(ValueError, match="needs a threshold"):
            fn(_f32())
        with pytest.raises(ValueError):
            fn(_f32(), threshold=float("nan"))
        # valid arguments on a CPU tensor: a device error, not a ValueError
        for x, kw in ((_u8(), {}), (_u8().bool(), dict(connectivity=4)), (_f32(), dict(threshold=0.5)),
                      (_u8(1, 1, 1, 1), {}), (_u8(), dict(threshold=0.3))):
            with pytest.raises(RuntimeError, match=r"run on MI355X \(HIP\) devices only"):
                fn(x, **kw)
    for min_area in (0, -1, 1.5, "2", None, True, 2 ** 31):
        with pytest.raises(ValueError):
            L.remove_small_components(_u8(), min_area)
    for bad in (_u8(), _f32(), torch.zeros(8, 9, dtype=torch.int32)):
        with pytest.raises(ValueError):
            L.component_areas(bad)
    with pytest.raises(RuntimeError):
        L.component_areas(torch.zeros(1, 1, 8, 9, dtype=torch.int32))


def test_a_plane_too_large_for_int32_labels_is_refused(monkeypatch):
    L = _no_device(monkeypatch)
    assert 46341 * 46341 > L.VU_CCL_MAX_PLANE == 2 ** 31 - 2
    huge = torch.empty(1, 1, 46341, 46341, dtype=torch.uint8, device="meta")     # a shape, no storage
    for fn in (L.label_components, lambda x: L.remove_small_components(x, 2), lambda x: L.lesion_counts(x, x),
               lambda x: L.LesionMeter().update(x, x)):
        with pytest.raises(ValueError, match="exceeds the int32 labels"):
            fn(huge)
    with pytest.raises(ValueError, match="exceeds the int32 labels"):
        L.component_areas(torch.empty(1, 1, 46341, 46341, dtype=torch.int32, device="meta"))


def test_counts_and_meter_validate_before_touching_a_device(monkeypatch):
    L = _no_device(monkeypatch)
    for fn in (L.lesion_counts, L.LesionMeter().update):
        for pred, masks in ((_u8(), _u8(2, 1, 8, 8)), (_u8(), _u8(8, 9)), (_u8(8, 9), _u8()), (_f32().double(), _u8()),
                            (_u8(2, 1, 0, 9), _u8(2, 1, 0, 9)), (_u8(), None)):
            with pytest.raises(ValueError):
                fn(pred, masks)
        for pred, masks in ((_u8(), _u8()), (_f32(), _f32()), (_u8().bool(), _u8()), (_f32(), _u8().long())):
            with pytest.raises(RuntimeError, match=r"run on MI355X \(HIP\) devices only"):
                fn(pred, masks)
    for kw in (dict(min_area=0), dict(connectivity=6), dict(threshold=None), dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            L.lesion_counts(_f32(), _u8(), **kw)
    for kw in (dict(min_area=0), dict(connectivity=5), dict(bins=0), dict(bins=2 ** 20 + 1), dict(bins=10.0),
               dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            L.LesionMeter(**kw)
    m = L.LesionMeter()
    assert (m.threshold, m.min_area, m.connectivity, m.bins) == (0.5, 1, 8, 1000)
    for call in (m.counts, m.froc, m.compute, m.values, m.histograms):
        with pytest.raises(RuntimeError, match="no update"):
            call()
    for bad in (torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 4), torch.zeros(0, 4, dtype=torch.int64), None):
        with pytest.raises(ValueError):
            L.lesion_metrics(bad)
    with pytest.raises(ValueError):
        L.lesion_metrics(torch.zeros(2, 4, dtype=torch.int64), n_planes=0)
    with pytest.raises(RuntimeError):
        L.lesion_metrics(torch.zeros(2, 4, dtype=torch.int64))


def test_names_exported():
    import vaeunet_amd
    from vaeunet_amd import lesions
    for n in ("label_components", "component_areas", "remove_small_components", "lesion_counts", "lesion_metrics",
              "LesionMeter", "evaluate_with_lesions"):
        assert callable(getattr(vaeunet_amd, n)), n
    for m in ("update", "counts", "froc", "compute", "reset"):
        assert callable(getattr(lesions.LesionMeter, m))
    assert list(inspect.signature(lesions.label_components).parameters) == ["x", "connectivity", "threshold",
                                                                            "return_counts"]
    assert list(inspect.signature(lesions.lesion_counts).parameters) == ["pred", "masks", "threshold", "min_area",
                                                                         "connectivity"]
    assert list(inspect.signature(lesions.LesionMeter).parameters)[:4] == ["threshold", "min_area", "connectivity",
                                                                           "bins"]


def test_evaluate_keeps_its_signature_and_the_lesion_loop_has_its_own():
    from vaeunet_amd.evaluate import evaluate, evaluate_with_lesions
    assert list(inspect.signature(evaluate).parameters) == ["net", "dataloader", "device", "amp", "align_corners",
                                                            "max_batches"]
    sig = inspect.signature(evaluate_with_lesions)
    assert list(sig.parameters) == ["net", "dataloader", "device", "lesion_meter", "amp", "align_corners",
                                    "max_batches"]
    assert sig.parameters["amp"].default is True and sig.parameters["align_corners"].default is False
    with pytest.raises(ValueError, match="lesion_meter is required"):
        evaluate_with_lesions(None, [], "cpu", None)


# ----------------------------------------------------------------------------
# binding and ops
# ----------------------------------------------------------------------------
def test_binding_declares_the_entry_points():
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
    for k, v in (("VU_CCL_U8", 0), ("VU_CCL_F32", 1), ("VU_CCL_MAX_PLANE", 2 ** 31 - 2), ("VU_FROC_MAX_BINS", 2 ** 20)):
        assert re.search(r"#define %s %d\b" % (k, v), src) and getattr(_lib, k) == v


def test_ops_registered_with_fake_impls_and_refuse_cpu():
    from vaeunet_amd import ops
    assert "label_components" in ops.OPS and "remove_small_components" in ops.OPS
    assert "label_components" in ops.__doc__ and "remove_small_components" in ops.__doc__
    lc, rs = torch.ops.vaeunet.label_components, torch.ops.vaeunet.remove_small_components
    assert lc.default._schema.name == "vaeunet::label_components"
    assert rs.default._schema.name == "vaeunet::remove_small_components"

    def m(*shape, dtype=torch.uint8):
        return torch.empty(shape, device="meta", dtype=dtype)
    for x, kw in ((m(2, 3, 20, 12), {}), (m(2, 3, 20, 12, dtype=torch.bool), dict(connectivity=4)),
                  (m(1, 1, 1, 1, dtype=torch.float32), dict(threshold=0.5))):
        out = lc(x, **kw)
        assert out.shape == x.shape and out.dtype == torch.int32 and out.is_contiguous()
        out = rs(x, 3, **kw)
        assert out.shape == x.shape and out.dtype == torch.uint8 and out.is_contiguous()
    for x, kw in ((m(3, 20, 12), {}), (m(2, 3, 20, 12, dtype=torch.int32), {}), (m(2, 3, 20, 12), dict(connectivity=6)),
                  (m(2, 3, 20, 12, dtype=torch.float32), {})):
        with pytest.raises(ValueError):
            lc(x, **kw)
        with pytest.raises(ValueError):
            rs(x, 3, **kw)
    with pytest.raises(ValueError):
        rs(m(2, 3, 20, 12), 0)
    with pytest.raises((NotImplementedError, RuntimeError)):
        lc(_u8())
    with pytest.raises((NotImplementedError, RuntimeError)):
        rs(_u8(), 2)


# ----------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 70), (70, 1), (67, 131)]


def _canonical(lab):
    """any labelling -> 1 + the smallest row-major index of each label's pixels"""
    flat = lab.reshape(-1)
    first = np.full(int(flat.max()) + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    out = (first[flat] + 1).astype(np.int32)
    out[flat == 0] = 0
    return out.reshape(lab.shape)


@pytest.mark.parametrize("HW", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_labels_equal_scipy_canonicalised(HW):
    ndi = pytest.importorskip("scipy.ndimage")
    H, W = HW
    for name, plane in LR.adversarial_planes(H, W).items():
        for conn, structure in ((4, ndi.generate_binary_structure(2, 1)), (8, np.ones((3, 3), int))):
            theirs, k = ndi.label(plane, structure=structure)
            ours = LR.label_plane(plane != 0, conn)
            assert np.array_equal(ours, _canonical(theirs)), (name, conn)
            assert len(np.unique(ours[ours > 0])) == k, (name, conn)


@pytest.mark.parametrize("HW", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_invariants(HW):
    H, W = HW
    for name, plane in LR.adversarial_planes(H, W).items():
        for conn in (4, 8):
            lab = LR.label_plane(plane != 0, conn)
            fg = plane != 0
            assert lab.dtype == np.int32 and ((lab > 0) == fg).all(), name
            roots = lab[fg] - 1
            # label - 1 is a foreground pixel of its own component, and the first one
            assert (lab.reshape(-1)[roots] == lab[fg]).all(), name
            assert (roots <= np.flatnonzero(fg.reshape(-1))).all(), name
            area = LR.areas_plane(lab)
            assert area.dtype == np.int32 and (area[~fg] == 0).all()
            per_root = area.reshape(-1)[np.unique(roots)] if roots.size else np.zeros(0, np.int32)
            assert int(per_root.sum()) == int(fg.sum()), name        # the areas sum to the foreground count
    # what the named planes are meant to be
    if H >= 8 and W >= 8:
        P = LR.adversarial_planes(H, W)
        n = lambda p, c: len(np.unique(LR.label_plane(p != 0, c))) - 1   # noqa: E731
        assert n(P["checkerboard"], 8) == 1 and n(P["checkerboard"], 4) == int(P["checkerboard"].sum())
        assert n(P["serpentine"], 4) == 1 and n(P["U"], 4) == 1
        assert n(P["diagonal"], 8) == 1 and n(P["diagonal"], 4) == min(H, W)
        assert n(P["antidiagonal"], 8) == 1 and n(P["comb"], 8) == n(P["comb"], 4) > 4


def test_reference_matching_and_froc_on_a_hand_example():
    f = np.float32
    pred = np.zeros((1, 1, 6, 12), f)
    gt = np.zeros((1, 1, 6, 12), np.uint8)
    gt[0, 0, 0:2, 0:2] = 1                      # lesion A, met by candidate 1 (0.9) and candidate 2 (0.7)
    gt[0, 0, 4:6, 6:8] = 1                      # lesion B, met only by a 1-pixel candidate (0.6)
    gt[0, 0, 0, 11] = 1                         # lesion C, missed
    pred[0, 0, 1, 1:3] = 0.9
    pred[0, 0, 0, 0] = 0.7
    pred[0, 0, 1, 0] = 0.2                      # below the threshold: keeps candidates 1 and 2 apart at connectivity 4
    pred[0, 0, 5, 8] = 0.6
    pred[0, 0, 3, 3:5] = 1.0                    # a false positive of two pixels, score exactly 1.0
    counts, hf, hg = LR.match(pred, gt, threshold=0.5, min_area=1, connectivity=4, nb=10)
    assert counts.tolist() == [[[3, 1, 4, 2]]]  # (5, 8) lies beside B, not on it: a second false positive ...
    gt[0, 0, 5, 8] = 1                          # ... now it is part of B
    counts, hf, hg = LR.match(pred, gt, threshold=0.5, min_area=1, connectivity=4, nb=10)
    assert counts.tolist() == [[[3, 2, 4, 1]]]
    assert hf.tolist() == [0] * 9 + [1] and hg.tolist() == [0, 0, 0, 0, 0, 0, 1, 0, 0, 1]  # 1.0: the last bin; 0.9, 0.6
    counts2, hf2, hg2 = LR.match(pred, gt, threshold=0.5, min_area=2, connectivity=4, nb=10)
    assert counts2.tolist() == [[[3, 1, 2, 1]]] and hg2.tolist() == [0] * 9 + [1]           # the singletons are dropped
    sens, fppi, score = LR.froc(hf, hg, 3, 1)
    assert fppi.tolist() == [1.0] * 10 and np.allclose(sens, [2 / 3] * 7 + [1 / 3] * 3)
    t = np.float64(2) / 3
    assert score == (0 + 0 + 0 + t + t + t + t) / 7
    sens0, _, score0 = LR.froc(hf, hg * 0, 0, 1)
    assert np.isnan(sens0).all() and np.isnan(score0)
    assert LR.score_bin(f(1.0), 1000) == 999 and LR.score_bin(np.nextafter(f(0.5), f(1)), 1000) == 500
    assert LR.score_bin(f(0), 7) == 0 and LR.score_bin(f(np.inf), 7) == 6
