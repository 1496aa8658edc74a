"""Host side of the device median blur (vaeunet_amd.data), no
GPU: the validation of median_blur / augment_patches(median=) before anything
is uploaded, TrainAugment(p_median=, median_limit=) and draw_median, that
draw() and draw_filters() are what they were on the parent commit, PatchCache's
draw order, the header prototype against the binding, the registration of
torch.ops.vaeunet.median_blur, and the invariants of the numpy reference
(tests/median_ref.py)."""
import hashlib
import os
import re

import numpy as np
import pytest
import torch

import median_ref as MR

CL = torch.channels_last


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ----------------------------------------------------------------------------
# validation before a device is touched
# ----------------------------------------------------------------------------
def _no_device(monkeypatch):
    import vaeunet_amd.data as D

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    for name in ("_launch_augment", "_launch_clahe", "_launch_blur", "_launch_median"):
        monkeypatch.setattr(D, name, no_device)
    monkeypatch.setattr(torch.Tensor, "to", no_device)
    return D


def _img(B=2, H=16, W=16, C=3):
    return torch.zeros(B, C, H, W).contiguous(memory_format=CL)


def test_median_blur_validates_before_touching_a_device(monkeypatch):
    D = _no_device(monkeypatch)
    assert D.MEDIAN_RMAX == 3
    img = _img()
    for radius in (-1, 4, 1.5, np.nan, np.inf, -np.inf, [1, 4], [1, np.nan], [0.5, 1], [1], [1, 2, 3],
                   np.ones((2, 1)), "a", None):
        with pytest.raises(ValueError):
            D.median_blur(img, radius)
    for bad in (_img(C=1), _img(C=4), _img().double(), torch.zeros(3, 16, 16), torch.zeros(2, 3, 0, 16)):
        with pytest.raises(ValueError):
            D.median_blur(bad, 1)
    # valid arguments on a CPU tensor: a device error, not a ValueError
    for radius in (0, 1, 3, 2.0, [0, 3], np.array([1, 2], np.int64), np.array([3.0, 0.0], np.float32)):
        with pytest.raises(RuntimeError):
            D.median_blur(img, radius)
    with pytest.raises(RuntimeError):
        D.median_blur(_img(H=1, W=1), 3)                      # a 1 x 1 image is valid


def test_augment_patches_validates_the_median_first(monkeypatch):
    D = _no_device(monkeypatch)
    img, msk = _img(), torch.zeros(2, 1, 16, 16).contiguous(memory_format=CL)
    p, gx, gy = D.identity_params(2), D.identity_knots(2, 16), D.identity_knots(2, 16)
    for median in (4, -1, 1.5, [1, np.nan], [1], [1, 2, 3]):
        with pytest.raises(ValueError):
            D.augment_patches(img, msk, p, gx, gy, seed=0, median=median)
    for kw in (dict(median=2), dict(median=[0, 3]), dict(clahe_clip=2.0, blur=D.identity_blur(2), median=[1, 0])):
        with pytest.raises(RuntimeError):
            D.augment_patches(img, msk, p, gx, gy, seed=0, **kw)


def test_augment_patches_uploads_the_median_table_last(monkeypatch):
    """one upload; with median=None its bytes are what they were, with it the [B] radii follow them; the
    launches run in the order CLAHE -> blur -> median -> warp, each on its own slice of the upload"""
    import vaeunet_amd.data as D
    B = 2
    img, msk = _img(), torch.zeros(B, 1, 16, 16).contiguous(memory_format=CL)
    p, gx, gy = D.identity_params(B), D.identity_knots(B, 16, 3), D.identity_knots(B, 16, 3)
    clip, table = np.array([2.0, 0.0], np.float32), np.stack([D.blur_weights(box=3), D.blur_weights(sigma=1.0)])
    uploads, order = [], []

    def to(self, *a, **k):
        uploads.append(self.numpy().copy())
        return self
    monkeypatch.setattr(torch.Tensor, "to", to)
    monkeypatch.setattr(D, "_need_device", lambda *a: None)
    monkeypatch.setattr(D, "_launch_clahe", lambda i, d, t: order.append(("clahe", d.numpy().copy())) or i)
    monkeypatch.setattr(D, "_launch_blur", lambda i, d: order.append(("blur", d.numpy().copy())) or i)
    monkeypatch.setattr(D, "_launch_median", lambda i, d: order.append(("median", d.numpy().copy())) or i)
    monkeypatch.setattr(D, "_launch_augment", lambda i, m, dp, dgx, dgy, *a: order.append(
        ("warp", dp.numpy().copy(), dgx.numpy().copy(), dgy.numpy().copy())) or (i, m))
    cuda = type("dev", (), {"type": "cuda"})()
    monkeypatch.setattr(torch.Tensor, "device", property(lambda self: cuda))
    base = np.concatenate([a.reshape(-1) for a in (p, gx, gy)])
    for kw, extra, names in (
            (dict(), [], ["warp"]),
            (dict(clahe_clip=clip, blur=table), [clip, table], ["clahe", "blur", "warp"]),
            (dict(median=[3, 0]), [np.array([3, 0], np.float32)], ["median", "warp"]),
            (dict(clahe_clip=clip, median=1), [clip, np.ones(B, np.float32)], ["clahe", "median", "warp"]),
            (dict(blur=table, median=[0, 2]), [table, np.array([0, 2], np.float32)], ["blur", "median", "warp"]),
            (dict(clahe_clip=clip, blur=table, median=[1, 2]), [clip, table, np.array([1, 2], np.float32)],
             ["clahe", "blur", "median", "warp"])):
        uploads.clear()
        order.clear()
        D.augment_patches(img, msk, p, gx, gy, seed=0, **kw)
        assert len(uploads) == 1
        assert uploads[0].tobytes() == np.concatenate([base] + [e.reshape(-1) for e in extra]).tobytes()
        assert [o[0] for o in order] == names
        for o, e in zip(order[:-1], extra):
            assert o[1].tobytes() == e.tobytes(), o[0]
        assert order[-1][1].tobytes() == p.tobytes() and order[-1][2].tobytes() == gx.tobytes()
        assert order[-1][3].tobytes() == gy.tobytes()


# ----------------------------------------------------------------------------
# binding and op
# ----------------------------------------------------------------------------
def test_binding_declares_the_entry_point():
    from vaeunet_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "vaeunet.h")).read()
    m = re.search(r"int vu_median_blur\(([^;]*)\);", src)
    assert m and "vu_median_blur" in _lib.exported_symbols()
    res, args = _lib._SIGS["vu_median_blur"]
    assert res is _lib._i and len(m.group(1).split(",")) == len(args) == 7
    for arg, ct in zip(m.group(1).split(","), args):
        assert ("*" in arg) == (ct is _lib._p), arg
    assert [ct is _lib._i for ct in args] == [False, True, True, True, False, False, False]
    assert re.search(r"#define VU_MEDIAN_RMAX 3\b", src) and _lib.VU_MEDIAN_RMAX == 3
    from vaeunet_amd import data
    assert data.MEDIAN_RMAX == _lib.VU_MEDIAN_RMAX == MR.RMAX


def test_op_registered_with_a_fake_impl_and_refuses_cpu():
    from vaeunet_amd import ops
    assert "median_blur" in ops.OPS
    mb = torch.ops.vaeunet.median_blur
    assert mb.default._schema.name == "vaeunet::median_blur"

    def m(*shape, dtype=torch.float32):
        return torch.empty(shape, device="meta", dtype=dtype)
    out = mb(m(3, 3, 20, 12), m(3))
    assert out.shape == (3, 3, 20, 12) and out.dtype == torch.float32 and out.is_contiguous(memory_format=CL)
    assert out.stride() == (720, 1, 36, 3)
    for args in ((m(3, 1, 20, 12), m(3)), (m(3, 3, 20, 12), m(2)), (m(3, 3, 20, 12), m(3, 1)), (m(3, 20, 12), m(3)),
                 (m(3, 3, 20, 12), m(3, dtype=torch.int32)), (m(3, 3, 20, 12, dtype=torch.float64), m(3))):
        with pytest.raises(ValueError):
            mb(*args)
    with pytest.raises((NotImplementedError, RuntimeError)):
        mb(_img(), torch.ones(2))


# ----------------------------------------------------------------------------
# TrainAugment
# ----------------------------------------------------------------------------
# sha256 of the arrays of TrainAugment().draw(6, 16, 16, PCG64(11)) and of TrainAugment(p_clahe=0.5,
# p_blur=0.5).draw_filters(16, PCG64(12)), each with the generator's next uniform, recorded on the commit before
# the median arguments were added
PARENT_DRAW_SEED11 = "1f832ff64c1d2e6bbdb29e1b7d9245f02acb0f704c4e1dd8f1e53b55df03e7c7"
PARENT_NEXT_SEED11 = 0.7810548233983421
PARENT_FILTERS_SEED12 = "f72f87e08cb9884f9b50917cf93e35b224eb5c245bcf1324f6985410f7196f4f"
PARENT_NEXT_SEED12 = 0.5360886065111569


def _digest(arrs):
    return hashlib.sha256(b"".join(x.tobytes() for x in arrs)).hexdigest()


def test_draw_and_draw_filters_are_unchanged_by_the_new_arguments():
    from vaeunet_amd.data import TrainAugment
    a = TrainAugment()
    assert (a.p_median, a.median_limit) == (0.0, 7)
    for kw in (dict(), dict(p_median=0.6, median_limit=5)):
        rng = _rng(11)
        arrs = TrainAugment(**kw).draw(6, 16, 16, rng)
        assert len(arrs) == 3 and _digest(arrs) == PARENT_DRAW_SEED11 and rng.random() == PARENT_NEXT_SEED11
        rng = _rng(12)
        arrs = TrainAugment(p_clahe=0.5, p_blur=0.5, **kw).draw_filters(16, rng)
        assert len(arrs) == 2 and _digest(arrs) == PARENT_FILTERS_SEED12 and rng.random() == PARENT_NEXT_SEED12


def test_draw_median_is_seeded_and_respects_the_coin():
    from vaeunet_amd.data import TrainAugment
    for limit, radii in ((3, {1}), (5, {1, 2}), (7, {1, 2, 3})):
        aug = TrainAugment(p_median=0.5, median_limit=limit)
        r1, r2, r3 = aug.draw_median(200, _rng(3)), aug.draw_median(200, _rng(3)), aug.draw_median(200, _rng(4))
        assert r1.dtype == np.float32 and r1.shape == (200,)
        assert r1.tobytes() == r2.tobytes() and r1.tobytes() != r3.tobytes()
        on = r1 > 0
        assert 60 < on.sum() < 140 and set(np.unique(r1[on])) == radii and (r1[~on] == 0).all()
        always = TrainAugment(p_median=1.0, median_limit=limit).draw_median(300, _rng(5))
        assert set(np.unique(always)) == radii
        # uniform over the windows: each radius within 5 sigma of 300 / n
        n = len(radii)
        for r in radii:
            assert abs((always == r).sum() - 300 / n) <= 5 * np.sqrt(300 * (1 / n) * (1 - 1 / n)) + 1e-9
    # the coin fails: radius 0, one uniform per sample consumed and nothing else
    off = TrainAugment()
    rng, ref = _rng(9), _rng(9)
    assert (off.draw_median(5, rng) == 0).all()
    ref.random(5)
    assert rng.bit_generator.state == ref.bit_generator.state


def test_median_limit_is_validated():
    from vaeunet_amd.data import TrainAugment
    for bad in (1, 2, 4, 6, 8, 9, 0, -3, 5.0, 3.5, "7", None, True, np.nan):
        with pytest.raises(ValueError):
            TrainAugment(median_limit=bad)
    for good in (3, 5, 7, np.int64(5)):
        assert TrainAugment(median_limit=good).median_limit == int(good)


class _Event:
    pass


class _Stream:
    def wait_event(self, ev):
        pass


def test_patch_cache_draws_the_median_last_and_only_when_asked(monkeypatch):
    """PatchCache's generator is left alone by draw_median unless p_median is
    positive, and draw() / draw_filters() come first (the launches are stubbed:
    no device here)"""
    import vaeunet_amd.data as D
    calls = []
    real = {n: getattr(D.TrainAugment, n) for n in ("draw", "draw_filters", "draw_median")}
    for n in real:
        monkeypatch.setattr(D.TrainAugment, n, lambda self, *a, _n=n: calls.append(_n) or real[_n](self, *a))
    seen = []
    monkeypatch.setattr(D, "augment_patches", lambda img, msk, **kw: seen.append(kw) or (img, msk))
    img, msk = torch.zeros(2, 3, 16, 16), torch.zeros(2, 1, 16, 16)

    def one_batch(aug):
        calls.clear()
        pc = D.PatchCache([], batch_size=2, device="cpu", augment=aug, seed=5)
        pc.paths = ["a_0", "b_1"]
        monkeypatch.setattr(pc, "_host_batch", lambda idx: (img, msk, ["a", "b"], [(0, 0)] * 2))
        monkeypatch.setattr(pc, "_to_device", lambda host: (*host, _Event()))
        monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: _Stream())
        monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, s: None)
        return next(iter(pc))["aug_params"], pc.rng.bit_generator.state
    plain, plain_state = one_batch(D.TrainAugment())
    assert calls == ["draw"] and set(plain) == {"params", "gx", "gy", "seed", "offset", "border"}
    med, med_state = one_batch(D.TrainAugment(p_median=1.0, median_limit=5))
    assert calls == ["draw", "draw_median"] and set(med) == set(plain) | {"median"}
    assert med["median"].shape == (2,) and set(med["median"]) <= {1.0, 2.0} and med_state != plain_state
    for k in ("params", "gx", "gy"):                       # draw() came first and drew what it draws alone
        assert med[k].tobytes() == plain[k].tobytes()
    assert set(seen[-1]) == set(med)                       # what augment_patches received is what the batch records
    filt, _ = one_batch(D.TrainAugment(p_clahe=0.5, p_blur=0.5))
    every, _ = one_batch(D.TrainAugment(p_clahe=0.5, p_blur=0.5, p_median=0.5))
    assert calls == ["draw", "draw_filters", "draw_median"]
    assert set(every) == set(filt) | {"median"}
    for k in ("params", "gx", "gy", "clahe_clip", "blur"):
        assert every[k].tobytes() == filt[k].tobytes()


# ----------------------------------------------------------------------------
# the reference's own invariants
# ----------------------------------------------------------------------------
SHAPES = [(16, 16), (17, 17), (20, 12), (45, 70), (5, 3), (2, 9), (1, 1), (1, 40)]


def _edge_windows(a, r):
    p = np.pad(a, ((r, r), (r, r), (0, 0)), mode="edge")
    w = np.lib.stride_tricks.sliding_window_view(p, (2 * r + 1, 2 * r + 1), axis=(0, 1))
    return w.reshape(*a.shape, -1)


def test_reference_key_is_an_order_preserving_bijection():
    rng = _rng(0)
    bits = np.concatenate([rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32),
                           np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001,
                                     0xffffffff, 1, 0x80000001, 0x7f7fffff, 0xff7fffff], np.uint32)])
    x = bits.view(np.float32)
    assert np.array_equal(MR.unkey(MR.key(x)).view(np.uint32), bits)
    finite = x[np.isfinite(x)]
    order = np.argsort(MR.key(finite), kind="stable")
    assert (np.diff(finite[order].astype(np.float64)) >= 0).all()
    special = np.array([0xffc00001, 0xff800000, 0xbf800000, 0x80000000, 0, 0x3f800000, 0x7f800000, 0x7fc00001],
                       np.uint32).view(np.float32)     # -nan < -inf < -1 < -0 < +0 < 1 < inf < nan
    assert (np.diff(MR.key(special).astype(np.int64)) > 0).all()


@pytest.mark.parametrize("HW", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_is_np_median_on_finite_data_and_a_member_of_the_window(HW):
    H, W = HW
    rng = _rng(H * 100 + W)
    img = (rng.random((4, H, W, 3), dtype=np.float32) * 4 - 2).astype(np.float32)
    img[1] = np.round(img[1] * 4) / 4                       # ties
    radius = np.array([0, 1, 2, 3])
    out = MR.median(img, radius)
    assert out.dtype == np.float32 and out.shape == img.shape
    assert np.array_equal(out[0].view(np.uint32), img[0].view(np.uint32))          # r = 0 is the identity
    for r in (1, 2, 3):
        full = MR.median(img, np.full(4, r))
        for b in range(4):
            w = _edge_windows(img[b], r)
            assert np.array_equal(full[b], np.median(w, axis=-1))
            assert (w.view(np.uint32) == full[b].view(np.uint32)[..., None]).any(-1).all()
        assert np.array_equal(out[r].view(np.uint32), full[r].view(np.uint32))     # samples are independent


def test_reference_selects_bitwise_among_specials():
    rng = _rng(7)
    H, W = 9, 11
    pool = np.array([0x7fc00001, 0x7fc00002, 0xffc00003, 0xff800004, 0x7f800000, 0xff800000, 0, 0x80000000, 1,
                     0x80000001, 0x007fffff], np.uint32)
    bits = rng.random((2, H, W, 3), dtype=np.float32).view(np.uint32).copy()
    hit = rng.random(bits.shape) < 0.3
    bits[hit] = rng.choice(pool, int(hit.sum()))
    img = bits.view(np.float32)
    for r in (1, 2, 3):
        out = MR.median(img, np.full(2, r)).view(np.uint32)
        for b in range(2):
            w = _edge_windows(bits[b], r)
            assert (w == out[b][..., None]).any(-1).all()
            # exactly rank (n - 1) / 2: as many keys at or below it as the rank needs, fewer strictly below
            k, ko = MR.key(w.view(np.float32)), MR.key(out[b].view(np.float32))[..., None]
            m = (2 * r + 1) ** 2 // 2
            assert ((k < ko).sum(-1) <= m).all() and ((k <= ko).sum(-1) > m).all()


def test_reference_kernel_radius():
    assert [MR.kernel_radius(t) for t in (3.9, 7, -1, np.nan, 0, 1, 2.5, np.inf, -np.inf)] == [3, 3, 0, 0, 0, 1, 2, 3, 0]
