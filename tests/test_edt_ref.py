"""The numpy restatement of the boundary metrics (tests/edt_ref.py) against a
brute force over all site pairs on small planes, and against scipy where it
imports.  CPU only."""
import numpy as np
import pytest

import edt_ref as ER

SMALL = [(1, 1), (1, 9), (9, 1), (7, 13), (33, 65)]


@pytest.mark.parametrize("HW", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_two_passes_equal_the_brute_force(HW):
    H, W = HW
    for name, plane in ER.adversarial_planes(H, W).items():
        for mode in ER.MODES:
            sites = ER.sites_plane(plane != 0, mode)
            got = ER.edt2_sites(sites)
            assert got.dtype == np.int32 and np.array_equal(got, ER.brute_edt2(sites)), (name, mode)
            if not sites.any():
                assert (got == ER.INF).all()


def test_boundary_by_hand():
    a = np.zeros((5, 6), bool)
    a[1:4, 1:5] = True
    want = a.copy()
    want[2, 2:4] = False
    assert np.array_equal(ER.boundary_plane(a), want)
    full = np.ones((4, 4), bool)           # the plane's edge counts as background
    want = full.copy()
    want[1:3, 1:3] = False
    assert np.array_equal(ER.boundary_plane(full), want)
    assert not ER.boundary_plane(np.zeros((3, 3), bool)).any()
    assert ER.boundary_plane(np.ones((1, 1), bool)).all()


def test_rank_and_percentile():
    assert [ER.rank(95, n) for n in (1, 2, 19, 20, 21, 100, 101)] == [1, 2, 19, 19, 20, 95, 96]
    assert ER.rank(100, 7) == 7 and ER.rank(1, 7) == 1 and ER.rank(50, 4) == 2
    v = [5, 1, 9, 3]
    assert [ER.percentile(v, q) for q in (1, 25, 26, 50, 75, 76, 100)] == [1, 1, 3, 3, 5, 9, 9]
    rng = np.random.Generator(np.random.PCG64(1))
    for n in (1, 2, 10, 99, 100, 101):
        v = rng.integers(0, 50, n)
        for q in (1, 50, 95, 100):
            assert ER.percentile(v, q) == sorted(v)[-(-q * n // 100) - 1]      # ceil(q n / 100)


def test_stats_by_hand_and_by_brute_force():
    # P: one pixel at (2, 2); G: one pixel at (2, 5) and one at (6, 2)
    p, g = np.zeros((8, 8), bool), np.zeros((8, 8), bool)
    p[2, 2] = True
    g[2, 5] = g[6, 2] = True
    st, sm = ER.stats_plane(p, g, 95, 9)
    assert st.tolist() == [1, 2, 9, 16, 9, 16, 1, 1] and sm.tolist() == [3.0, 7.0]
    m = ER.metrics(st, sm)
    assert m.tolist() == [4.0, 4.0, 10.0 / 3.0, 2.0 / 3.0]
    st, sm = ER.stats_plane(p, np.zeros((8, 8), bool), 95, 9)
    assert st.tolist() == [1, 0, -1, -1, -1, -1, -1, -1] and sm.tolist() == [0.0, 0.0]
    assert np.isnan(ER.metrics(st, sm)).all()
    pooled, k = ER.pooled(np.array([[1.0, 2, 3, 4], [np.nan] * 4, [3.0, 2, 1, 0]]))
    assert k == 2 and pooled.tolist() == [2.0, 2.0, 2.0, 2.0]
    assert np.isnan(ER.pooled(np.full((2, 4), np.nan))[0]).all()
    for name, (a, b) in ER.pair_planes(33, 65).items():
        st, sm = ER.stats_plane(a != 0, b != 0, 90, 4)
        P, G = ER.boundary_plane(a != 0), ER.boundary_plane(b != 0)
        assert st[0] == P.sum() and st[1] == G.sum()
        if st[0] and st[1]:
            d = ER.brute_edt2(G)[P]
            assert st[2] == d.max() and st[6] == (d <= 4).sum() and st[4] == np.sort(d)[ER.rank(90, len(d)) - 1], name
            assert abs(sm[0] - np.sqrt(d.astype(np.float64)).sum()) <= 1e-9 * max(1.0, sm[0])
        else:
            assert name in ("empty_pred", "empty_gt") and (st[2:] == -1).all()
    a = ER.pair_planes(33, 65)["identical"][0] != 0          # identical masks: every distance is 0
    k = int(ER.boundary_plane(a).sum())
    st, sm = ER.stats_plane(a, a, 95, 0)
    assert k > 0 and st.tolist() == [k, k, 0, 0, 0, 0, k, k] and sm.tolist() == [0.0, 0.0]


def test_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for H, W in ((33, 65), (67, 131)):
        for name, plane in ER.adversarial_planes(H, W).items():
            fg = plane != 0
            cross = ndi.generate_binary_structure(2, 1)
            assert np.array_equal(ER.boundary_plane(fg), fg & ~ndi.binary_erosion(fg, cross, border_value=0)), name
            if (~fg).any():                    # scipy has no "no site" convention
                want = ndi.distance_transform_edt(fg)
                got = ER.edt2_plane(fg, "background")
                assert np.array_equal(got, np.rint(want ** 2).astype(np.int32)), name
            if fg.any():
                want = ndi.distance_transform_edt(~fg)
                assert np.array_equal(ER.edt2_plane(fg, "foreground"), np.rint(want ** 2).astype(np.int32)), name
