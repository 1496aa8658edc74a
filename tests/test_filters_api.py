"""Host side of the device CLAHE and separable blur (vaeunet_amd.data, DESIGN.md
§4.9), no GPU: blur_weights, the validation of clahe / blur / augment_patches
before anything is uploaded, the header prototypes against the binding, the
registration of torch.ops.vaeunet.clahe / blur_separable, that TrainAugment.draw
is what it was with the new arguments at their defaults, draw_filters, and the
invariants of the numpy reference (tests/filters_ref.py)."""
import os
import re

import numpy as np
import pytest
import torch

import filters_ref as FR

CL = torch.channels_last


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ----------------------------------------------------------------------------
# blur_weights
# ----------------------------------------------------------------------------
def test_blur_weights_gaussian_rows():
    from vaeunet_amd.data import NBLUR, RMAX, blur_weights
    assert (RMAX, NBLUR) == (7, 9)
    for sigma in (0.3, 0.5, 1.0, 1.7, 2.3, 2.34, 5.0):
        row = blur_weights(sigma=sigma)
        assert row.dtype == np.float32 and row.shape == (9,)
        r = int(row[0])
        assert r == min(7, int(np.ceil(3 * sigma)))
        w = row[1:].astype(np.float64)
        # normalised in float64, then rounded: at most r + 1 half-ulps of values <= 1 off
        assert abs(w[0] + 2 * w[1:].sum() - 1) <= (2 * r + 1) * 2.0 ** -25
        assert (w[r + 1:] == 0).all() and (w[:r + 1] > 0).all() and (np.diff(w[:r + 1]) < 0).all()
        k = np.arange(1, r + 1)
        np.testing.assert_allclose(w[1:r + 1] / w[0], np.exp(-k * k / (2 * sigma * sigma)), rtol=1e-6)


def test_blur_weights_box_rows():
    from vaeunet_amd.data import blur_weights
    row = blur_weights(box=5)
    assert row.tobytes() == np.array([2, .2, .2, .2, 0, 0, 0, 0, 0], np.float32).tobytes()
    assert blur_weights(box=1).tobytes() == np.array([0, 1, 0, 0, 0, 0, 0, 0, 0], np.float32).tobytes()
    row = blur_weights(box=15)
    assert row[0] == 7 and (row[1:] == np.float32(1 / 15)).all()
    for bad in (0, 2, 17, -3, 2.5):
        with pytest.raises(ValueError):
            blur_weights(box=bad)


def test_blur_weights_small_sigma_is_the_identity_row():
    from vaeunet_amd.data import blur_weights, identity_blur
    ident = np.array([0, 1, 0, 0, 0, 0, 0, 0, 0], np.float32)
    for sigma in (0.0, 1e-6, 1e-3, 0.05):
        assert blur_weights(sigma=sigma).tobytes() == ident.tobytes(), sigma
    assert identity_blur(3).tobytes() == np.tile(ident, (3, 1)).tobytes()
    for kw in (dict(), dict(sigma=1.0, box=3), dict(sigma=-1.0), dict(sigma=np.nan), dict(sigma=np.inf)):
        with pytest.raises(ValueError):
            blur_weights(**kw)


# ----------------------------------------------------------------------------
# validation before a device is touched
# ----------------------------------------------------------------------------
def _no_device(monkeypatch):
    import vaeunet_amd.data as D

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    for name in ("_launch_augment", "_launch_clahe", "_launch_blur"):
        monkeypatch.setattr(D, name, no_device)
    monkeypatch.setattr(torch.Tensor, "to", no_device)
    return D


def _img(B=2, H=16, W=16, C=3):
    return torch.zeros(B, C, H, W).contiguous(memory_format=CL)


def test_clahe_validates_before_touching_a_device(monkeypatch):
    D = _no_device(monkeypatch)
    img = _img()
    for clip in (-1.0, np.nan, np.inf, [1.0, -2.0], [1.0, np.nan], [1.0], [1.0, 2.0, 3.0], np.ones((2, 1))):
        with pytest.raises(ValueError):
            D.clahe(img, clip)
    for tiles in ((0, 8), (8, 0), (17, 8), (8, 17), (2.5, 2), (8,), 8, (8, 8, 8), (-1, 2)):
        with pytest.raises(ValueError):
            D.clahe(img, 2.0, tiles)
    with pytest.raises(ValueError):
        D.clahe(_img(H=12, W=20), 2.0, (13, 8))               # more tiles than rows
    with pytest.raises(ValueError):
        D.clahe(_img(H=20, W=12), 2.0, (8, 13))               # ... than columns
    for bad in (_img(C=1), _img(C=4), _img().double(), torch.zeros(3, 16, 16), torch.zeros(2, 3, 0, 16)):
        with pytest.raises(ValueError):
            D.clahe(bad, 2.0)
    # valid arguments on a CPU tensor: a device error, not a ValueError
    for clip in (2.0, 0.0, [0.0, 3.0], np.array([1.5, 2.5], np.float64)):
        with pytest.raises(RuntimeError):
            D.clahe(img, clip)
    with pytest.raises(RuntimeError):
        D.clahe(_img(H=12, W=12), 2.0, (12, 12))


def test_blur_validates_before_touching_a_device(monkeypatch):
    D = _no_device(monkeypatch)
    img = _img()
    good = np.stack([D.blur_weights(sigma=1.0), D.blur_weights(box=3)])
    for idx, val in (((0, 0), 8), ((0, 0), -1), ((1, 0), 1.5), ((0, 0), np.nan), ((1, 3), np.inf), ((0, 8), np.nan)):
        t = good.copy()
        t[idx] = val
        with pytest.raises(ValueError):
            D.blur(img, t)
    for t in (good[:1], good[:, :8], np.zeros((2, 10), np.float32), good[0]):
        with pytest.raises(ValueError):
            D.blur(img, t)
    for bad in (_img(C=1), _img().double(), torch.zeros(3, 16, 16)):
        with pytest.raises(ValueError):
            D.blur(bad, good)
    with pytest.raises(RuntimeError):
        D.blur(img, good)
    with pytest.raises(RuntimeError):
        D.blur(_img(H=1, W=1), good)                          # a 1 x 1 image is valid


def test_augment_patches_validates_the_filter_tables_first(monkeypatch):
    D = _no_device(monkeypatch)
    img, msk = _img(), torch.zeros(2, 1, 16, 16).contiguous(memory_format=CL)
    p, gx, gy = D.identity_params(2), D.identity_knots(2, 16), D.identity_knots(2, 16)
    good = D.identity_blur(2)
    bad_table = good.copy()
    bad_table[1, 0] = 9
    for kw in (dict(clahe_clip=-1.0), dict(clahe_clip=[1.0, np.nan]), dict(clahe_clip=[1.0]),
               dict(clahe_clip=2.0, clahe_tiles=(17, 2)), dict(clahe_clip=2.0, clahe_tiles=(2, 0)),
               dict(blur=bad_table), dict(blur=good[:1]), dict(clahe_clip=2.0, blur=good[:, :8])):
        with pytest.raises(ValueError):
            D.augment_patches(img, msk, p, gx, gy, seed=0, **kw)
    for kw in (dict(), dict(clahe_clip=2.0), dict(blur=good),
               dict(clahe_clip=[0.0, 1.0], clahe_tiles=(4, 2), blur=good)):
        with pytest.raises(RuntimeError):
            D.augment_patches(img, msk, p, gx, gy, seed=0, **kw)


# ----------------------------------------------------------------------------
# binding and ops
# ----------------------------------------------------------------------------
def test_binding_declares_the_entry_points():
    from vaeunet_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "vaeunet.h")).read()
    for name, nargs in (("vu_clahe_luts", 9), ("vu_clahe_apply", 10), ("vu_blur_sep", 7)):
        m = re.search(r"int %s\(([^;]*)\);" % name, src)
        assert m and name in _lib.exported_symbols()
        assert len(m.group(1).split(",")) == len(_lib._SIGS[name][1]) == nargs
        # pointers in the prototype <-> c_void_p in the binding, position by position
        for arg, ct in zip(m.group(1).split(","), _lib._SIGS[name][1]):
            assert ("*" in arg) == (ct is _lib._p), (name, arg)


def test_ops_registered_with_fake_impls_and_refuse_cpu():
    from vaeunet_amd import ops
    assert "clahe" in ops.OPS and "blur_separable" in ops.OPS
    cl, bl = torch.ops.vaeunet.clahe, torch.ops.vaeunet.blur_separable
    assert cl.default._schema.name == "vaeunet::clahe" and bl.default._schema.name == "vaeunet::blur_separable"

    def m(*shape):
        return torch.empty(shape, device="meta", dtype=torch.float32)
    for out in (cl(m(3, 3, 20, 12), m(3)), cl(m(3, 3, 20, 12), m(3), 3, 2), bl(m(3, 3, 20, 12), m(3, 9))):
        assert out.shape == (3, 3, 20, 12) and out.dtype == torch.float32 and out.is_contiguous(memory_format=CL)
    for args in ((m(3, 1, 20, 12), m(3)), (m(3, 3, 20, 12), m(2)), (m(3, 3, 20, 12), m(3), 17, 2),
                 (m(3, 3, 20, 12), m(3), 8, 13), (m(3, 3, 20, 12), m(3), 0, 2)):
        with pytest.raises(ValueError):
            cl(*args)
    for args in ((m(3, 4, 20, 12), m(3, 9)), (m(3, 3, 20, 12), m(3, 8)), (m(3, 3, 20, 12), m(2, 9))):
        with pytest.raises(ValueError):
            bl(*args)
    with pytest.raises((NotImplementedError, RuntimeError)):
        cl(_img(), torch.ones(2))
    with pytest.raises((NotImplementedError, RuntimeError)):
        bl(_img(), torch.zeros(2, 9))


# ----------------------------------------------------------------------------
# TrainAugment
# ----------------------------------------------------------------------------
# sha256 of the three arrays of TrainAugment().draw(6, 16, 16, PCG64(11)) and the generator's next uniform, recorded
# on the commit before the filter arguments were added
PARENT_DRAW_SEED11 = "1f832ff64c1d2e6bbdb29e1b7d9245f02acb0f704c4e1dd8f1e53b55df03e7c7"
PARENT_NEXT_SEED11 = 0.7810548233983421


def test_draw_is_unchanged_by_the_new_arguments():
    """draw() returns what it returned and consumes the generator exactly as
    before, with the filter arguments at their defaults or set"""
    import hashlib
    from vaeunet_amd.data import TrainAugment
    a, b = TrainAugment(), TrainAugment(p_clahe=0.7, p_blur=0.4, clahe_clip=(2.0, 3.0), blur_sigma=(1.0, 2.0))
    assert (a.p_clahe, a.p_blur, a.clahe_tiles, a.clahe_clip, a.blur_sigma) == (0.0, 0.0, (8, 8), (1.0, 4.0),
                                                                                (0.5, 1.5))
    for aug in (a, b):
        rng = _rng(11)
        arrs = aug.draw(6, 16, 16, rng)
        assert len(arrs) == 3
        assert hashlib.sha256(b"".join(x.tobytes() for x in arrs)).hexdigest() == PARENT_DRAW_SEED11
        assert rng.random() == PARENT_NEXT_SEED11


def test_draw_filters_is_seeded_and_respects_the_coins():
    from vaeunet_amd.data import TrainAugment, identity_blur
    aug = TrainAugment(p_clahe=0.5, p_blur=0.5, clahe_clip=(1.0, 4.0), blur_sigma=(0.5, 2.5))
    c1, t1 = aug.draw_filters(64, _rng(3))
    c2, t2 = aug.draw_filters(64, _rng(3))
    assert c1.dtype == t1.dtype == np.float32 and c1.shape == (64,) and t1.shape == (64, 9)
    assert c1.tobytes() == c2.tobytes() and t1.tobytes() == t2.tobytes()
    c3, t3 = aug.draw_filters(64, _rng(4))
    assert c1.tobytes() != c3.tobytes() and t1.tobytes() != t3.tobytes()
    on = c1 > 0
    assert 10 < on.sum() < 54 and ((c1[on] >= 1) & (c1[on] <= 4)).all() and (c1[~on] == 0).all()
    blurred = t1[:, 0] > 0
    assert 10 < blurred.sum() < 54 and (t1[~blurred] == identity_blur(1)[0]).all()
    assert set(np.unique(t1[blurred, 0])) <= set(range(2, 8))          # ceil(3 sigma), sigma in [0.5, 2.5]
    s = t1[:, 1].astype(np.float64) + 2 * t1[:, 2:].astype(np.float64).sum(1)
    assert np.abs(s - 1).max() <= 15 * 2.0 ** -25
    # both coins off: nothing but the identity, and two uniforms per sample are consumed
    off = TrainAugment()
    rng, ref = _rng(9), _rng(9)
    c, t = off.draw_filters(5, rng)
    assert (c == 0).all() and t.tobytes() == identity_blur(5).tobytes()
    ref.random(10)
    assert rng.bit_generator.state == ref.bit_generator.state
    for kw in (dict(clahe_clip=(0.0, 2.0)), dict(clahe_clip=(3.0, 2.0)), dict(blur_sigma=(-1.0, 1.0)),
               dict(blur_sigma=(2.0, 1.0)), dict(clahe_tiles=(0, 8)), dict(clahe_tiles=(8, 17)),
               dict(clahe_clip=(1.0, np.inf))):
        with pytest.raises(ValueError):
            TrainAugment(**kw)


def test_patch_cache_draws_filters_only_when_asked(monkeypatch):
    """PatchCache's generator is left alone by draw_filters unless p_clahe or
    p_blur is positive (the launches are stubbed: no device here)"""
    import vaeunet_amd.data as D
    calls = []
    monkeypatch.setattr(D.TrainAugment, "draw_filters", lambda self, B, rng: calls.append(B) or
                        (np.zeros(B, np.float32), D.identity_blur(B)))
    seen = []
    monkeypatch.setattr(D, "augment_patches", lambda img, msk, **kw: seen.append(kw) or (img, msk))
    img, msk = torch.zeros(2, 3, 16, 16), torch.zeros(2, 1, 16, 16)

    def one_batch(aug):
        pc = D.PatchCache([], batch_size=2, device="cpu", augment=aug)
        pc.paths = ["a_0", "b_1"]
        monkeypatch.setattr(pc, "_host_batch", lambda idx: (img, msk, ["a", "b"], [(0, 0)] * 2))
        monkeypatch.setattr(pc, "_to_device", lambda host: (*host, _Event()))
        monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: _Stream())
        monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, s: None)
        return next(iter(pc))["aug_params"]
    plain = one_batch(D.TrainAugment())
    assert calls == [] and set(plain) == {"params", "gx", "gy", "seed", "offset", "border"}
    both = one_batch(D.TrainAugment(p_clahe=0.5, p_blur=0.5, clahe_tiles=(4, 2)))
    assert calls == [2] and set(both) == set(plain) | {"clahe_clip", "clahe_tiles", "blur"}
    assert both["clahe_tiles"] == (4, 2)
    for k in ("params", "gx", "gy"):                       # draw() came first and drew what it draws alone
        assert both[k].tobytes() == plain[k].tobytes()
    only_blur = one_batch(D.TrainAugment(p_blur=1.0))
    assert set(only_blur) == set(plain) | {"blur"}
    only_clahe = one_batch(D.TrainAugment(p_clahe=1.0))
    assert set(only_clahe) == set(plain) | {"clahe_clip", "clahe_tiles"}
    assert set(seen[-1]) == set(only_clahe)                # what augment_patches received is what the batch records


class _Event:
    pass


class _Stream:
    def wait_event(self, ev):
        pass


# ----------------------------------------------------------------------------
# the reference's own invariants
# ----------------------------------------------------------------------------
def test_reference_tile_formula():
    """tile_of(y) names the tile [s(t), s(t+1)) that holds y, for every n < 80 and T <= min(16, n)"""
    for n in range(1, 80):
        for T in range(1, min(16, n) + 1):
            s = [FR.tile_start(t, n, T) for t in range(T + 1)]
            assert s[0] == 0 and s[-1] == n and all(b > a for a, b in zip(s, s[1:]))
            for y in range(n):
                t = FR.tile_of(y, n, T)
                assert s[t] <= y < s[t + 1], (n, T, y)


def test_reference_blend_weights():
    for n, T in ((16, 2), (17, 4), (45, 2), (70, 3), (12, 12), (16, 1), (79, 16)):
        t1, t2, w = FR.axis_blend(n, T)
        C = [FR.tile_start(t, n, T) + FR.tile_start(t + 1, n, T) - 1 for t in range(T)]
        assert ((0 <= w) & (w < 1)).all() and ((t2 == t1) | (t2 == t1 + 1)).all() and t2.max() <= T - 1
        assert (w[t1 == t2] == 0).all()
        # the blend reproduces twice the pixel position from the tile centres: it is linear interpolation
        pos = np.array([C[a] + ww * (C[b] - C[a]) for a, b, ww in zip(t1, t2, w)])
        inside = (2 * np.arange(n) >= C[0]) & (2 * np.arange(n) <= C[-1])
        np.testing.assert_allclose(pos[inside], 2 * np.arange(n)[inside], atol=1e-12)
        assert (t1[~inside] == t2[~inside]).all()


def test_reference_clip_keeps_the_total_and_the_lut_is_monotone():
    rng = _rng(0)
    met = set()
    for trial in range(300):
        A = int(rng.integers(1, 3000))
        kind = trial % 3
        if kind == 0:
            y = rng.integers(0, 256, A)
        elif kind == 1:
            y = rng.integers(100, 110, A)
        else:
            y = np.full(A, int(rng.integers(0, 256)))
        h = np.bincount(y, minlength=256)
        lim = FR.clip_limit(rng.choice([0.5, 2.0, 4.0, 40.0, 1e6]), A)
        assert 1 <= lim <= A
        h2, r = FR.clip_hist(h, lim)
        met.add("r0" if r == 0 else ("step>=2" if r <= 128 else "step1"))
        assert int(h2.sum()) == A and h2.min() >= 0
        lut = FR.lut_of(h2, A)
        assert lut.dtype == np.uint8 and lut[255] == 255 and (np.diff(lut.astype(int)) >= 0).all()
    assert met == {"r0", "step>=2", "step1"}
    assert FR.clip_limit(1e6, 64) == 64 and FR.clip_limit(0.5, 64) == 1 and FR.clip_limit(4.0, 64) == 1
    assert FR.clip_limit(2.0, 4096) == 32


def test_reference_quantisation():
    k = np.arange(256)
    assert (FR.quant8((k / 255.0).astype(np.float32)) == k).all()      # cache images lose nothing
    assert FR.quant8(np.float32(np.nan)) == 0 and FR.quant8(np.float32(-3)) == 0 and FR.quant8(np.float32(7)) == 255
    img = np.zeros((1, 1, 2, 3), np.float32)
    img[0, 0, 1] = 1.0
    assert FR.luma8(img).tolist() == [[[0, 255]]]


def test_reference_blur_identity_and_reflection():
    rng = _rng(1)
    img = rng.random((2, 5, 3, 3), dtype=np.float32)
    ident = np.tile(np.array([0, 1, 0, 0, 0, 0, 0, 0, 0], np.float32), (2, 1))
    assert np.array_equal(FR.blur(img, ident), img.astype(np.float64))
    assert FR.fold101(np.arange(-7, 10), 3).tolist() == [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1]
    assert FR.fold101(np.arange(-3, 4), 1).tolist() == [0] * 7
    # a constant image stays constant under any normalised kernel, whatever the fold does
    from vaeunet_amd.data import blur_weights
    const = np.full((1, 5, 3, 3), 0.25, np.float32)
    out = FR.blur(const, blur_weights(sigma=2.3)[None])
    assert np.abs(out - 0.25).max() <= 1e-7
