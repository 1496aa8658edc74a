"""Host side of the device training augmentation (vaeunet_amd.data, DESIGN.md
§4.8), no GPU: the parameter helpers (affine_matrix, colour_matrix),
TrainAugment.draw, the validation of augment_patches before anything is
uploaded, the registration of torch.ops.vaeunet.augment_patch, and that
PatchCache(augment=True) still draws what it drew before TrainAugment existed."""
import numpy as np
import pytest
import torch

import augment_ref as AR

CL = torch.channels_last


def test_affine_matrix_equals_the_integer_flip_rot_map():
    from vaeunet_amd.data import _flip_rot_map, affine_matrix
    for P in (16, 17):
        for h in (0, 1):
            for v in (0, 1):
                for k in range(4):
                    ay, by, cy, ax, bx, cx = _flip_rot_map(P, h, v, k)
                    a = affine_matrix(P, P, h, v, k)
                    assert a.dtype == np.float32 and a.shape == (6,)
                    assert [int(t) for t in a] == [bx, ax, cx, by, ay, cy] and (a == np.round(a)).all(), (P, h, v, k)


def test_affine_matrix_general():
    """rotation / scale / shift about the centre: the centre maps to centre -
    R shift / scale, and the linear part is R(angle) / scale"""
    from vaeunet_amd.data import affine_matrix
    H, W = 20, 12
    a = affine_matrix(H, W, angle=30.0, scale=1.25, shift=(0.1, -0.05)).astype(np.float64)
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    L = np.array([[c, -s], [s, c]]) / 1.25
    np.testing.assert_allclose([[a[0], a[1]], [a[3], a[4]]], L, atol=1e-7)
    ctr = np.array([(W - 1) / 2, (H - 1) / 2])
    want = ctr - L @ np.array([0.1 * W, -0.05 * H])
    np.testing.assert_allclose([a[0] * ctr[0] + a[1] * ctr[1] + a[2], a[3] * ctr[0] + a[4] * ctr[1] + a[5]], want,
                               atol=1e-5)
    with pytest.raises(ValueError):
        affine_matrix(H, W, scale=0.0)


def test_colour_matrix_identity_is_bitwise():
    from vaeunet_amd.data import colour_matrix
    M, o = colour_matrix(0, 0, 0, 0)
    assert M.dtype == np.float32 and o.dtype == np.float32
    assert M.tobytes() == np.eye(3, dtype=np.float32).tobytes()
    assert o.tobytes() == np.zeros(3, np.float32).tobytes()


def test_colour_matrix_saturation_minus_one_is_grey():
    from vaeunet_amd.data import colour_matrix
    M, o = colour_matrix(saturation=-1.0)
    grey = np.array([0.299, 0.587, 0.114], np.float32)
    assert (M[0] == grey).all() and (M[1] == M[0]).all() and (M[2] == M[0]).all() and (o == 0).all()


def test_colour_matrix_brightness_contrast():
    from vaeunet_amd.data import colour_matrix
    M, o = colour_matrix(brightness=0.1, contrast=0.5)
    np.testing.assert_allclose(M, 1.5 * np.eye(3), atol=1e-7)
    np.testing.assert_allclose(o, np.full(3, 1.5 * 0.1 - 0.25), atol=1e-7)     # 1.5 (v + 0.1 - 0.5) + 0.5


def test_colour_matrix_full_turn_of_hue_is_the_identity():
    """M(hue = 1) - I = (cos t - 1)(I - G) + sin t J at t = 2 pi as held in
    binary: were the angle a float32 its rounding error would be at most
    pi 2^-23 (half an ulp of 2 pi), so |sin t|, |cos t - 1| <= pi 2^-23 and
    every entry moves by at most pi 2^-23 (max|J| + 1), plus half a float32
    ulp of 1 for the final rounding.  (The helper works in float64: far inside.)"""
    from vaeunet_amd.data import _HUE_J, colour_matrix
    bound = np.pi * 2.0 ** -23 * (np.abs(_HUE_J).max() + 1.0) + 2.0 ** -24
    for turns in (1.0, -1.0):
        M, o = colour_matrix(hue=turns)
        assert np.abs(M.astype(np.float64) - np.eye(3)).max() <= bound
        assert (o == 0).all()
    # half a turn is not the identity but keeps grey fixed
    M, _ = colour_matrix(hue=0.5)
    assert np.abs(M - np.eye(3)).max() > 0.5
    np.testing.assert_allclose(M.astype(np.float64) @ np.ones(3), np.ones(3), atol=1e-6)


def test_reference_philox_known_answers():
    """the reference's Philox4x32-10 on the published vectors (Random123 kat_vectors)"""
    full = 0xFFFFFFFF
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
                           ((full,) * 4, (full, full), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
                           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
                            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))):
        got = AR.philox4x32_10(*[[c] for c in ctr], *key)
        assert tuple(int(g[0]) for g in got) == want
    w = AR.pixel_words(4, 5, 2, (7 << 32) | 9, 3)
    assert w.shape == (4, 4, 5)
    one = AR.philox4x32_10([13], [0], [2], [3], 9, 7)              # pixel (2, 3) = index 13
    assert [int(w[k, 2, 3]) for k in range(4)] == [int(o[0]) for o in one]


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def test_draw_is_seeded():
    from vaeunet_amd.data import TrainAugment
    aug = TrainAugment()
    a, b = aug.draw(6, 16, 16, _rng(11)), aug.draw(6, 16, 16, _rng(11))
    for x, y in zip(a, b):
        assert x.dtype == np.float32 and x.tobytes() == y.tobytes()
    assert a[0].shape == (6, 20) and a[1].shape == a[2].shape == (6, aug.grid_steps + 1)
    c = aug.draw(6, 16, 16, _rng(12))
    assert any(x.tobytes() != y.tobytes() for x, y in zip(a, c))


def test_draw_with_all_probabilities_zero_is_the_identity():
    from vaeunet_amd.data import TrainAugment, identity_params
    aug = TrainAugment(p_hflip=0, p_vflip=0, p_rot90=0, p_affine=0, p_grid=0, p_gamma=0, p_colour=0, p_noise=0)
    p, gx, gy = aug.draw(4, 20, 12, _rng(0))
    assert p.tobytes() == identity_params(4).tobytes()
    ident = np.zeros(20, np.float32)
    ident[[0, 4, 6, 7, 11, 15]] = 1
    assert (p == ident).all()
    assert (gx == np.array([0, 11], np.float32)).all() and (gy == np.array([0, 19], np.float32)).all()
    # the identity table is the identity map, bitwise, in the reference too
    assert (AR.knot_map(gx[0], 12) == np.arange(12)).all()


def test_draw_knots_increase_with_pinned_ends():
    from vaeunet_amd.data import TrainAugment
    aug = TrainAugment(p_rot90=0, p_grid=1.0, grid_steps=5, grid_limit=0.3)
    moved = 0
    for seed in range(100):
        _, gx, gy = aug.draw(3, 20, 12, _rng(seed))
        for k, size in ((gx, 12), (gy, 20)):
            assert k.shape == (3, 6) and (k[:, 0] == 0).all() and (k[:, -1] == size - 1).all()
            assert (np.diff(k, axis=1) > 0).all()
            moved += int((k != np.linspace(0, size - 1, 6, dtype=np.float32)).any())
    assert moved == 200                                   # every table is a distortion, not the identity
    with pytest.raises(ValueError):
        TrainAugment(grid_limit=1.0)
    with pytest.raises(ValueError):
        TrainAugment(grid_steps=33)
    with pytest.raises(ValueError):
        TrainAugment(border="wrap")
    with pytest.raises(ValueError):
        TrainAugment().draw(2, 20, 12, _rng(0))      # rot90 on a non-square patch


def _good(B=2, H=16, W=16, Cm=1, S=4):
    from vaeunet_amd.data import identity_knots, identity_params
    img = torch.zeros(B, 3, H, W).contiguous(memory_format=CL)
    msk = torch.zeros(B, Cm, H, W).contiguous(memory_format=CL)
    return img, msk, identity_params(B), identity_knots(B, W, S), identity_knots(B, H, S)


def test_augment_patches_validates_before_touching_a_device(monkeypatch):
    import vaeunet_amd.data as D

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(D, "_launch_augment", no_device)
    monkeypatch.setattr(torch.Tensor, "to", no_device)
    img, msk, p, gx, gy = _good()
    for bad in (np.nan, np.inf, -np.inf):
        for which, idx in ((0, (1, 2)), (0, (0, 19)), (1, (0, 2)), (2, (1, 1))):
            q = [p.copy(), gx.copy(), gy.copy()]
            q[which][idx] = bad
            with pytest.raises(ValueError):
                D.augment_patches(img, msk, *q, seed=0)
    # shapes
    for q in ((p[:1], gx, gy), (p[:, :19], gx, gy), (p, gx[:1], gy), (p, gx, gy[:, :3]), (p, gx[:, :1], gy[:, :1]),
              (p, np.zeros((2, 34), np.float32), np.zeros((2, 34), np.float32))):
        with pytest.raises(ValueError):
            D.augment_patches(img, msk, *q, seed=0)
    with pytest.raises(ValueError):
        D.augment_patches(img[:, :1], msk, p, gx, gy, seed=0)                    # 1-channel image
    with pytest.raises(ValueError):
        D.augment_patches(img, msk[:, :, :8], p, gx, gy, seed=0)                 # mask of another size
    with pytest.raises(ValueError):
        D.augment_patches(img, msk[:, :0], p, gx, gy, seed=0)                    # Cm = 0
    with pytest.raises(ValueError):
        D.augment_patches(img.double(), msk, p, gx, gy, seed=0)
    # knots: equal and decreasing neighbours
    for tbl in (0, 1):
        for val in (gx[0, 1], gx[0, 0] - 1):
            q = [gx.copy(), gy.copy()]
            q[tbl][0, 2] = val
            with pytest.raises(ValueError):
                D.augment_patches(img, msk, p, *q, seed=0)
    # seed / offset / border
    for kw in (dict(seed=-1), dict(seed=2 ** 64), dict(seed=0, offset=2 ** 32), dict(seed=0, offset=-1),
               dict(seed=0, border="wrap")):
        with pytest.raises(ValueError):
            D.augment_patches(img, msk, p, gx, gy, **kw)
    # valid arguments on CPU tensors: refused as a device error, not a ValueError
    with pytest.raises(RuntimeError):
        D.augment_patches(img, msk, p, gx, gy, seed=0)


def test_augment_op_registered_with_fake_impl_and_refuses_cpu():
    from vaeunet_amd import ops
    assert "augment_patch" in ops.OPS
    op = torch.ops.vaeunet.augment_patch
    assert op.default._schema.name == "vaeunet::augment_patch"

    def m(*shape):
        return torch.empty(shape, device="meta", dtype=torch.float32)
    oi, om = op(m(3, 3, 20, 12).contiguous(memory_format=CL), m(3, 2, 20, 12), m(3, 20), m(3, 5), m(3, 5), 7)
    assert oi.shape == (3, 3, 20, 12) and om.shape == (3, 2, 20, 12) and oi.dtype == torch.float32
    assert oi.is_contiguous(memory_format=CL)
    with pytest.raises(ValueError):
        op(m(3, 1, 20, 12), m(3, 2, 20, 12), m(3, 20), m(3, 5), m(3, 5), 7)
    img, msk, p, gx, gy = _good()
    with pytest.raises((NotImplementedError, RuntimeError)):
        op(img, msk, torch.from_numpy(p), torch.from_numpy(gx), torch.from_numpy(gy), 0)


def test_binding_declares_the_entry_point():
    import os
    import re
    from vaeunet_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "vaeunet.h")).read()
    m = re.search(r"int vu_augment_patch\(([^;]*)\);", src)
    assert m and "vu_augment_patch" in _lib.exported_symbols()
    assert len(m.group(1).split(",")) == len(_lib._SIGS["vu_augment_patch"][1]) == 17


# (hflip, vflip, k) of the first batch of 5 drawn by PatchCache(augment=True, seed=3).augment_batch, recorded on
# the commit before TrainAugment was added
PARENT_FLAGS_SEED3 = [(True, True, 0), (False, True, 2), (True, False, 1), (True, False, 2), (False, False, 2)]


def test_patch_cache_flip_flags_unchanged(monkeypatch):
    """augment=True draws hflip, vflip, (coin, k) per sample from the seeded
    generator exactly as before (the launches are stubbed: no device here)"""
    import vaeunet_amd.data as D
    monkeypatch.setattr(D.K, "call", lambda *a: 0)
    monkeypatch.setattr(D.K, "stream", lambda: None)
    pc = D.PatchCache([], batch_size=5, device="cpu", augment=True, seed=3)
    img = torch.zeros(5, 3, 16, 16).contiguous(memory_format=CL)
    msk = torch.zeros(5, 1, 16, 16).contiguous(memory_format=CL)
    _, _, flags = pc.augment_batch(img, msk)
    assert [(bool(h), bool(v), int(k)) for h, v, k in flags] == PARENT_FLAGS_SEED3
    # explicit flags are passed through, nothing is drawn
    state = pc.rng.bit_generator.state
    assert pc.augment_batch(img, msk, [(1, 0, 2)] * 5)[2] == [(1, 0, 2)] * 5
    assert pc.rng.bit_generator.state == state
