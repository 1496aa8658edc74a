"""Host side of the sample-set metrics (vaeunet_amd.samples),
no GPU: every validation error is raised before a device is touched and names
the function, the header prototypes against the binding, the registration and
the fake implementation of torch.ops.vaeunet.sample_gram, the meter's refusals,
and the numpy reference (tests/samples_ref.py) on hand-computed cases."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import samples_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"vu_sample_gram": 13, "vu_sampleset_metrics": 6}


def _no_device(monkeypatch):
    import vaeunet_amd.samples as S

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(S, "call", no_device)
    monkeypatch.setattr(torch.Tensor, "to", no_device)
    monkeypatch.setattr(torch.Tensor, "contiguous", no_device)
    monkeypatch.setattr(torch.Tensor, "float", no_device)
    return S


def _u8(*shape):
    return torch.zeros(shape or (3, 2, 1, 8, 9), dtype=torch.uint8)


def _f32(*shape):
    return torch.zeros(shape or (3, 2, 1, 8, 9), dtype=torch.float32)


def test_sample_gram_validates_before_touching_a_device(monkeypatch):
    S = _no_device(monkeypatch)
    what = "sample_gram"
    # rank, empty input, dtype
    for bad in (_u8(8, 9), _u8(2, 8, 9), _u8(1, 3, 2, 1, 8, 9), _u8(3, 2, 1, 0, 9), _u8(0, 2, 1, 8, 9),
                torch.zeros(3, 2, 1, 8, 9, dtype=torch.int32), torch.zeros(3, 2, 1, 8, 9, dtype=torch.float64),
                torch.zeros(3, 2, 1, 8, 9, dtype=torch.bfloat16), np.zeros((3, 2, 1, 8, 9), np.uint8), None):
        with pytest.raises(ValueError, match=what):
            S.sample_gram(bad)
    # shape mismatch, rank and emptiness of the truths
    for truths in (_u8(2, 1, 8, 8), _u8(1, 8, 9), _u8(2, 2, 8, 9), _u8(2, 3, 2, 1, 8, 9)[:, :1], _u8(0, 2, 1, 8, 9),
                   np.zeros((2, 1, 8, 9), np.uint8)):
        with pytest.raises(ValueError, match=what):
            S.sample_gram(_u8(), truths)
    # a [S, C, H, W] stack means B = 1: its truth is [1, C, H, W]
    with pytest.raises(ValueError, match=what):
        S.sample_gram(_u8(3, 1, 8, 9), _u8(2, 1, 8, 9))
    # K > 64
    with pytest.raises(ValueError, match=r"sample_gram: 65 samples \+ 0 truths exceed K <= 64"):
        S.sample_gram(_u8(65, 1, 1, 2, 2))
    with pytest.raises(ValueError, match=r"sample_gram: 62 samples \+ 3 truths exceed K <= 64"):
        S.sample_gram(_u8(62, 1, 1, 2, 2), _u8(3, 1, 1, 2, 2))
    # the threshold
    with pytest.raises(ValueError, match="sample_gram: the threshold is NaN"):
        S.sample_gram(_f32(), threshold=float("nan"))
    with pytest.raises(ValueError, match="sample_gram: float32 samples need a threshold"):
        S.sample_gram(_f32(), threshold=None)
    # out=
    for out in (torch.zeros(2, 1, 3, 3), torch.zeros(2, 1, 4, 4, dtype=torch.int64),
                torch.zeros(2, 1, 3, 6, dtype=torch.int64)[..., ::2], "x"):
        with pytest.raises(ValueError, match="sample_gram: out must be"):
            S.sample_gram(_u8(), out=out)
    # a plane too large for the kernel's int32 pixel counts of one block
    huge = torch.empty(1, 1, 1, 46341, 46341, dtype=torch.uint8, device="meta")
    with pytest.raises(ValueError, match="sample_gram: a plane of 46341 x 46341 pixels exceeds"):
        S.sample_gram(huge)
    # valid arguments on a CPU tensor: the project's device error, not a ValueError
    for args, kw in (((_u8(),), {}), ((_u8().bool(), _u8(2, 1, 8, 9)), {}), ((_f32(), _f32(2, 2, 1, 8, 9)), {}),
                     ((_u8(3, 1, 8, 9), _u8(1, 1, 8, 9)), {}), ((_u8(),), dict(threshold=None)),
                     ((_f32(64, 1, 1, 2, 2),), dict(threshold=0.25)),
                     ((_u8(), _u8(2, 1, 8, 9)), dict(out=torch.zeros(2, 1, 4, 4, dtype=torch.int64)))):
        with pytest.raises(RuntimeError, match=r"run on MI355X \(HIP\) devices only; sample_gram got cpu"):
            S.sample_gram(*args, **kw)


def test_metrics_and_meter_validate_before_touching_a_device(monkeypatch):
    S = _no_device(monkeypatch)
    g = torch.zeros(2, 1, 4, 4, dtype=torch.int64)
    for bad, n in ((torch.zeros(2, 1, 4, 4), 3), (g[0], 3), (torch.zeros(2, 1, 4, 5, dtype=torch.int64), 3),
                   (torch.zeros(0, 1, 4, 4, dtype=torch.int64), 3), (None, 3), (g, 0), (g, 5), (g, 3.0), (g, True),
                   (torch.zeros(1, 1, 65, 65, dtype=torch.int64), 60)):
        with pytest.raises(ValueError, match="sample_set_metrics"):
            S.sample_set_metrics(bad, n)
    for n in (1, 3, 4):
        with pytest.raises(RuntimeError, match=r"run on MI355X \(HIP\) devices only; sample_set_metrics got cpu"):
            S.sample_set_metrics(g, n)

    with pytest.raises(ValueError, match="SampleSetMeter: the threshold is NaN"):
        S.SampleSetMeter(float("nan"))
    m = S.SampleSetMeter()
    assert m.threshold == 0.5
    for call in (m.compute, m.values):
        with pytest.raises(RuntimeError, match="SampleSetMeter: no update"):
            call()
    for samples, truths in ((_u8(), None), (_u8(), _u8(2, 1, 8, 8)), (_u8(8, 9), _u8(2, 1, 8, 9)),
                            (torch.zeros(3, 2, 1, 8, 9, dtype=torch.float64), _u8(2, 1, 8, 9)),
                            (_u8(64, 1, 1, 2, 2), _u8(1, 1, 2, 2))):
        with pytest.raises(ValueError, match=r"SampleSetMeter\.update"):
            m.update(samples, truths)
    with pytest.raises(RuntimeError, match=r"devices only; SampleSetMeter\.update got cpu"):
        m.update(_u8(), _u8(2, 1, 8, 9))


def test_the_meter_refuses_inconsistent_updates(monkeypatch):
    """the state is what a first update on some device would have left: a class-count or device change is refused
    before anything is launched, and reset() clears it"""
    S = _no_device(monkeypatch)
    monkeypatch.setattr(S, "_need_device", lambda t, what: None)
    m = S.SampleSetMeter(0.25)
    m._sum = torch.zeros(2, S.VU_SAMPLESET_NMETRICS, dtype=torch.float64)
    m.n_planes = 4
    with pytest.raises(ValueError, match=r"SampleSetMeter\.update: 1 classes on cpu, earlier batches had 2 on cpu"):
        m.update(_u8(), _u8(2, 1, 8, 9))
    m._sum = torch.zeros(1, S.VU_SAMPLESET_NMETRICS, dtype=torch.float64, device="meta")
    with pytest.raises(ValueError, match=r"SampleSetMeter\.update: 1 classes on cpu, earlier batches had 1 on meta"):
        m.update(_u8(), _u8(2, 1, 8, 9))
    m.reset()
    assert m.n_planes == 0
    with pytest.raises(RuntimeError, match="no update"):
        m.values()


def test_names_exported():
    import vaeunet_amd
    from vaeunet_amd import inference, samples
    for n in ("sample_gram", "sample_set_metrics", "SampleSetMeter"):
        assert callable(getattr(vaeunet_amd, n)), n
    assert vaeunet_amd.SAMPLESET_METRIC_NAMES == samples.SAMPLESET_METRIC_NAMES == SR.NAMES
    assert len(SR.NAMES) == samples.VU_SAMPLESET_NMETRICS == 9
    for m in ("update", "compute", "values", "reset"):
        assert callable(getattr(samples.SampleSetMeter, m))
    assert list(inspect.signature(samples.sample_gram).parameters) == ["samples", "truths", "threshold", "out"]
    assert list(inspect.signature(samples.sample_set_metrics).parameters) == ["gram", "n_samples"]
    sig = inspect.signature(inference.sample_set_scores)
    assert list(sig.parameters) == ["model", "img", "mask", "num_samples", "threshold", "kw"]
    assert sig.parameters["num_samples"].default == 32 and sig.parameters["threshold"].default == 0.5
    # the existing entry point keeps its signature
    assert list(inspect.signature(inference.segmentation_distribution).parameters) == [
        "model", "img", "num_samples", "patch_size", "overlap", "temperature", "batch_size", "eps", "sample_batch"]


def test_binding_declares_the_entry_points():
    from vaeunet_amd import _lib
    src = open(os.path.join(ROOT, "include", "vaeunet.h")).read()
    for name, nargs in SYMBOLS.items():
        m = re.search(r"(int|int64_t) %s\(([^;]*)\);" % name, src)
        assert m and name in _lib.exported_symbols(), name
        res, args = _lib._SIGS[name]
        assert res is _lib._i, name
        decl = m.group(2).split(",")
        assert len(decl) == len(args) == nargs, name
        for arg, ct in zip(decl, args):
            assert ("*" in arg) == (ct is _lib._p), (name, arg)
            if "*" not in arg:
                want = {"int": _lib._i, "int64_t": _lib._l, "float": _lib._f, "double": _lib.C.c_double}
                assert ct is want[arg.split()[0]], (name, arg)
    for k, v in (("VU_SAMPLESET_MAX", 64), ("VU_SAMPLESET_NMETRICS", 9)):
        assert re.search(r"#define %s %d\b" % (k, v), src) and getattr(_lib, k) == v
    # the sweep of one grid, named by the kernel's own constants
    assert _lib.VU_SAMPLESET_STEP % _lib.VU_SAMPLESET_VEC == 0 and _lib.VU_SAMPLESET_GRID >= 256


def test_op_registered_with_a_fake_impl_and_refuses_cpu():
    from vaeunet_amd import ops
    assert "sample_gram" in ops.OPS and "sample_gram" in ops.__doc__
    sg = torch.ops.vaeunet.sample_gram
    assert sg.default._schema.name == "vaeunet::sample_gram"

    def m(*shape, dtype=torch.uint8):
        return torch.empty(shape, device="meta", dtype=dtype)
    for args, kw, want in (((m(5, 2, 3, 20, 12),), {}, (2, 3, 5, 5)),
                           ((m(5, 2, 3, 20, 12, dtype=torch.bool), m(2, 3, 20, 12)), {}, (2, 3, 6, 6)),
                           ((m(5, 3, 20, 12, dtype=torch.float32), m(1, 3, 20, 12, dtype=torch.float32)),
                            dict(threshold=0.3), (1, 3, 6, 6)),
                           ((m(61, 1, 1, 1, 1), m(3, 1, 1, 1, 1, dtype=torch.int64)), {}, (1, 1, 64, 64)),
                           ((m(5, 2, 3, 20, 12),), dict(threshold=None), (2, 3, 5, 5))):
        out = sg(*args, **kw)
        assert tuple(out.shape) == want and out.dtype == torch.int64 and out.is_contiguous()
    for args, kw in (((m(3, 20, 12),), {}), ((m(5, 2, 3, 20, 12, dtype=torch.int32),), {}),
                     ((m(5, 2, 3, 20, 12), m(2, 3, 20, 13)), {}), ((m(65, 1, 1, 2, 2),), {}),
                     ((m(62, 1, 1, 2, 2), m(3, 1, 1, 2, 2)), {}), ((m(5, 2, 3, 0, 12),), {}),
                     ((m(5, 2, 3, 20, 12, dtype=torch.float32),), dict(threshold=None)),
                     ((m(5, 2, 3, 20, 12, dtype=torch.float32),), dict(threshold=float("nan")))):
        with pytest.raises(ValueError, match="vaeunet::sample_gram"):
            sg(*args, **kw)
    with pytest.raises((NotImplementedError, RuntimeError)):
        sg(_u8())


# ----------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------
def test_reference_on_hand_cases():
    # two disjoint non-empty samples, an empty truth: d(s, y) = 1, Dice = 0; d(s0, s1) = 1
    s = np.zeros((2, 1, 1, 2, 3), np.uint8)
    s[0, 0, 0, 0, :2] = 1
    s[1, 0, 0, 1, :] = 1
    G = SR.gram(s, np.zeros((1, 1, 1, 2, 3), np.uint8))
    assert G[0, 0].tolist() == [[2, 0, 0], [0, 3, 0], [0, 0, 0]]
    m = SR.metrics(G, 2)[0, 0]
    assert m.tolist() == [2 * 1.0 - 0.5 - 0.0, 1.0, 0.5, 0.0, 0.0, 0.0, 0.0, 2.5, 0.5]
    # identical samples equal to the truth, and everything empty
    for fill in (1, 0):
        s = np.full((3, 1, 1, 2, 3), fill, np.uint8)
        m = SR.metrics(SR.gram(s, s[:1]), 3)[0, 0]
        assert m[:7].tolist() == [0, 0, 0, 0, 1, 1, 1] and m[7] == 6 * fill and m[8] == 0
    # without a truth
    m = SR.metrics(SR.gram(s), 3)[0, 0]
    assert np.isnan(m[list(SR.NAN_WITHOUT_TRUTH)]).all() and not np.isnan(m[[2, 7, 8]]).any()
    # a partial overlap: |a| = 4, |b| = 2, I = 1 -> d = 1 - 1/5, Dice = 2/6
    a = np.array([1, 1, 1, 1, 0, 0], np.uint8).reshape(1, 1, 1, 2, 3)
    b = np.array([0, 0, 0, 1, 1, 0], np.uint8).reshape(1, 1, 1, 2, 3)
    m = SR.metrics(SR.gram(a, b), 1)[0, 0]
    assert m[1] == 1 - np.float64(1) / 5 and m[4] == m[5] == m[6] == np.float64(2) / 6 and m[0] == 2 * m[1]


def test_reference_stacks_and_encodings():
    for kind in SR.KINDS:
        s, t = SR.stack(kind, 4, 2, 3, 9, 7)
        assert s.shape == (4, 3, 9, 7) and t.shape == (2, 3, 9, 7) and s.dtype == t.dtype == np.uint8
        assert set(np.unique(s)) <= {0, 1} and set(np.unique(t)) <= {0, 1}
        G = SR.gram(s[:, :, None], t[:, :, None])
        assert G.shape == (3, 1, 6, 6) and (G == G.transpose(0, 1, 3, 2)).all()
        assert (np.diagonal(G, axis1=2, axis2=3) == np.concatenate([s, t]).reshape(6, 3, -1).sum(-1).T[:, None]).all()
        if kind == "disjoint":
            assert (G[0, 0] == np.diag(np.diag(G[0, 0]))).all() and (np.diag(G[0, 0]) > 0).all()
        if kind == "nested":
            assert (G[0, 0] == np.minimum.outer(np.diag(G[0, 0]), np.diag(G[0, 0]))).all()
        if kind == "truth_empty":
            assert t.sum() == 0 and s.sum() > 0
        if kind == "one_empty":
            assert s[2].sum() == 0 and s[0].sum() > 0
        # the float32 encoding thresholds back to the same bits (asserted inside), at more than one threshold
        for thr in (0.5, 0.3):
            p = SR.as_prob(s, thr, 5)
            assert p.dtype == np.float32 and np.isnan(p).any() == bool((s == 0).any())
            assert np.array_equal(SR.gram(p[:, :, None], t[:, :, None], thr), G)
