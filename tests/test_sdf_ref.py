"""The reference of the signed distance map (tests/sdf_ref.py)
against scipy's distance_transform_edt written as the one_hot2dist of Kervadec
et al., and against a brute force over all site pairs; no GPU."""
import numpy as np
import pytest
import torch

import edt_ref as ER
import sdf_ref as SR

SHAPES = [(1, 1), (1, 70), (70, 1), (9, 7), (33, 65), (17, 40)]
BRUTE_MAX = 4500      # pixels: the brute force is O((H W)^2)


def _planes(H, W):
    d = dict(ER.adversarial_planes(H, W))
    for name, (a, b) in ER.pair_planes(H, W).items():
        if name in ("shifted_disc", "nested_squares"):
            d[name + "_a"], d[name + "_b"] = a, b
    return d


def _one_hot2dist(mask):
    """Kervadec et al.: distance(negmask) * negmask - (distance(posmask) - 1) * posmask, 0 for an empty mask"""
    ndi = pytest.importorskip("scipy.ndimage")
    pos = mask.astype(bool)
    if not pos.any() or pos.all():
        return np.zeros(mask.shape, np.float64)
    neg = ~pos
    return ndi.distance_transform_edt(neg) * neg - (ndi.distance_transform_edt(pos) - 1) * pos


@pytest.mark.parametrize("HW", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_is_the_brute_force_and_never_zero_on_a_mixed_plane(HW):
    H, W = HW
    assert H * W <= BRUTE_MAX
    for name, m in _planes(H, W).items():
        fg = m != 0
        got = SR.s2_plane(fg)
        assert got.dtype == np.int32 and np.array_equal(got, SR.brute_s2_plane(fg)), name
        if fg.any() and not fg.all():
            assert (got != 0).all() and ((got < 0) == fg).all(), name
            assert np.abs(got).min() == 1, name                    # some pixel touches the other class
        else:
            assert (got == 0).all(), name


@pytest.mark.parametrize("HW", SHAPES + [(67, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_phi_is_scipy_written_as_one_hot2dist_bit_for_bit_in_fp32(HW):
    H, W = HW
    for name, m in _planes(H, W).items():
        want = _one_hot2dist(m).astype(np.float32)
        got = SR.phi_of(SR.s2_plane(m != 0))
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), name


def test_phi_values_and_the_clip():
    s2 = np.array([0, 1, 2, 4, 9, -1, -2, -4, -9, 16383 ** 2, -(16383 ** 2)], np.int32)
    phi = SR.phi_of(s2)
    want = [0.0, 1.0, np.float32(np.sqrt(2.0)), 2.0, 3.0, 0.0, np.float32(1.0 - np.sqrt(2.0)), -1.0, -2.0, 16383.0, -16382.0]
    assert phi.dtype == np.float32 and phi.tolist() == [float(v) for v in want]
    for clip in (1.0, 2.5, 1e6):
        c = SR.phi_of(s2, clip)
        assert np.array_equal(c, np.clip(phi, -np.float32(clip), np.float32(clip))) and np.abs(c).max() <= clip
    assert np.array_equal(SR.phi_of(s2, 1e6)[:9], phi[:9]) and SR.phi_of(s2, 2.5).tolist()[3:5] == [2.0, 2.5]
    # a batch: planes do not interact, thresholds as the transform's
    x = np.zeros((2, 2, 5, 6), np.float32)
    x[0, 0, 2, 3], x[1, 1, :, :] = 0.75, 1.0
    x[0, 1, 1, 1] = np.nan
    x[0, 1, 0, 0] = 0.5                                  # not above the threshold
    got = SR.s2(x, 0.5)
    assert got.shape == x.shape and (got[0, 1] == 0).all() and (got[1] == 0).all()
    assert got[0, 0, 2, 3] == -1 and got[0, 0, 0, 0] == 4 + 9


def test_loss_reference_on_a_case_worked_by_hand():
    x = torch.tensor([0.0, 2.0, float("nan"), -1.0, 3.0])
    f = torch.tensor([2.0, -1.0, 5.0, float("inf"), 0.5])
    r = SR.boundary_loss_ref(x, f, gout=3.0)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))   # noqa: E731
    terms = [2.0 * 0.5, -sig(2.0), 0.5 * sig(3.0)]
    assert abs(float(r["sums"][0]) - sum(terms)) < 1e-15 and abs(float(r["sums"][1]) - sum(map(abs, terms))) < 1e-15
    assert float(r["sums"][2]) == 2.0 and abs(float(r["loss"]) - sum(terms) / 5) < 1e-15
    g = r["grad"].tolist()
    assert g[2] == 0.0 and g[3] == 0.0 and abs(g[0] - 3.0 / 5 * 2.0 * 0.25) < 1e-15
    assert abs(g[1] + 3.0 / 5 * sig(2.0) * (1 - sig(2.0))) < 1e-15 and torch.equal(r["sabs"], r["grad"].abs())
    r32 = SR.boundary_loss_ref(x, f, gout=3.0, dtype=torch.float32)
    assert r32["grad"].dtype == torch.float32 and torch.allclose(r32["grad"].double(), r["grad"], rtol=1e-6, atol=0)
