"""vu_median_blur (vaeunet_amd/csrc/median.hip) on the GPU
against the numpy definition in tests/median_ref.py, through the C ABI on
guarded buffers (inputs come back unchanged, no guard element is written),
B = 4.

The median is a selection: every output value is one of its window's inputs,
so every comparison here is BITWISE (through an int32 view), NaN payloads and
the sign of zero included; there is no tolerance.

Shapes: 16 x 16, 17 x 17, 20 x 12 (inside one 32 x 32 tile, ragged), 45 x 70
(2 x 3 tiles, ragged on both axes), 5 x 3, 2 x 9, 1 x 1 (smaller than the
window on one or both axes: the clamp folds most of the window onto the edge).
Images: random floats in [-2, 2), k/255 (ties), constant, the narrow band
100..109 / 255, and "specials" (about 10 % of the elements NaNs of both signs
with distinct payloads, +-inf, +-0, denormals).  Radii: the mixed batch
[0, 1, 2, 3] and the uniform batches 1, 2, 3, so every instantiation meets
every shape and kind."""
import functools

import numpy as np
import pytest
import torch

import median_ref as MR
import ref_small as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
INVALID = 1   # hipErrorInvalidValue
B = 4

SHAPES = [(16, 16), (17, 17), (20, 12), (45, 70), (5, 3), (2, 9), (1, 1)]
KINDS = ["floats", "k255", "constant", "narrow", "specials"]
RADII = [(0, 1, 2, 3), (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3)]
CASES = [(s, k, r) for s in SHAPES for k in KINDS for r in RADII]


def _id(case):
    (H, W), kind, radii = case
    return f"{H}x{W}-{kind}-r{''.join(map(str, radii))}"


def _D():
    import vaeunet_amd.data as D
    return D


def _i32(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _bits(a, b):
    return np.array_equal(_i32(a), _i32(b))


SPECIALS = np.array([0x7fc00000, 0x7fc00001, 0x7fa5a5a5, 0x7fffffff, 0xffc00000, 0xffc00002, 0xff812345, 0xffffffff,
                     0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff],
                    np.uint32)


@functools.lru_cache(maxsize=None)
def _image(H, W, kind):
    """NHWC float32 [4, H, W, 3], read-only"""
    rng = np.random.Generator(np.random.PCG64(H * 1000 + W))
    if kind == "floats":
        img = (rng.random((B, H, W, 3), dtype=np.float32) * 4 - 2).astype(np.float32)
    elif kind == "k255":
        img = rng.integers(0, 256, (B, H, W, 3)).astype(np.float32) / np.float32(255)
    elif kind == "constant":
        img = np.broadcast_to((rng.integers(0, 256, (B, 1, 1, 3)).astype(np.float32) / np.float32(255)),
                              (B, H, W, 3)).copy()
    elif kind == "narrow":
        img = rng.integers(100, 110, (B, H, W, 3)).astype(np.float32) / np.float32(255)
    else:
        bits = (rng.random((B, H, W, 3), dtype=np.float32) * 2 - 1).astype(np.float32).view(np.uint32).copy()
        hit = rng.random(bits.shape) < 0.1
        bits[hit] = rng.choice(SPECIALS, int(hit.sum()))
        if bits.size >= 64:
            bits.reshape(-1)[:len(SPECIALS)] = SPECIALS            # every special at least once
        img = bits.view(np.float32)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _ref(H, W, kind):
    """{r: the reference of all four samples at radius r}: computed once, shared, read-only"""
    img = _image(H, W, kind)
    out = {r: MR.median(img, np.full(B, r)) for r in range(MR.RMAX + 1)}
    for v in out.values():
        v.setflags(write=False)
    return out


def _want(H, W, kind, radii):
    ref = _ref(H, W, kind)
    return np.stack([ref[r][b] for b, r in enumerate(radii)])


def _median_raw(img, radius):
    """vu_median_blur on guarded buffers -> out numpy; inputs bitwise unchanged, no guard element written"""
    from vaeunet_amd import _lib as L
    n, H, W, _ = img.shape
    radius = np.ascontiguousarray(radius, np.float32)
    dimg, gi = R.guarded(img.shape, torch.float32, DEV)
    drad, gr = R.guarded(radius.shape, torch.float32, DEV)
    dimg.copy_(torch.from_numpy(np.array(img)))
    drad.copy_(torch.from_numpy(radius.copy()))
    out, go = R.guarded(img.shape, torch.float32, DEV)
    L.call("vu_median_blur", L.ptr(dimg), n, H, W, L.ptr(drad), L.ptr(out), L.stream())
    torch.cuda.synchronize()
    for g in (gi, gr, go):
        g.check("median")
    assert _bits(dimg.cpu().numpy(), img) and _bits(drad.cpu().numpy(), radius)
    return out.cpu().numpy()


# ----------------------------------------------------------------------------
# 1. the definition, bitwise
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_median_is_bitwise_the_reference(case):
    (H, W), kind, radii = case
    img = _image(H, W, kind)
    got = _median_raw(img, radii)
    want = _want(H, W, kind, radii)
    bad = np.argwhere(_i32(got) != _i32(want))
    assert len(bad) == 0, (len(bad), bad[:4])
    for b, r in enumerate(radii):
        if r == 0:
            assert _bits(got[b], img[b])                        # off: the input, bitwise


def test_cases_meet_every_instantiation_on_every_shape_and_kind():
    for s in SHAPES:
        for k in KINDS:
            met = {r for (s2, k2, radii) in CASES if (s2, k2) == (s, k) for r in radii}
            assert met == {0, 1, 2, 3}, (s, k, met)
    # the specials are all there and the filter does move values on the images that are not constant
    img = _image(45, 70, "specials")
    assert set(SPECIALS.tolist()) <= set(img.view(np.uint32).reshape(-1).tolist())
    assert np.isnan(img).mean() > 0.02
    for kind in ("floats", "k255", "narrow", "specials"):
        for r in (1, 2, 3):
            assert not _bits(_ref(45, 70, kind)[r], _image(45, 70, kind))
    assert _bits(_ref(45, 70, "constant")[3], _image(45, 70, "constant"))


@pytest.mark.parametrize("HW", [(17, 17), (45, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sample_alone_equals_sample_in_batch(HW):
    H, W = HW
    img = _image(H, W, "specials")
    for radii in ((0, 1, 2, 3), (3, 2, 1, 0)):
        full = _median_raw(img, radii)
        for b in range(B):
            assert _bits(_median_raw(img[b:b + 1], radii[b:b + 1]), full[b:b + 1]), (radii, b)


def test_kernel_clamps_the_radius():
    """outside the host's validation: 3.9 and 7 run as 3, -1 and NaN as 0 (off)"""
    for H, W in ((17, 17), (45, 70)):
        img = _image(H, W, "floats")
        table = np.array([3.9, 7.0, -1.0, np.nan], np.float32)
        assert [MR.kernel_radius(t) for t in table] == [3, 3, 0, 0]
        got = _median_raw(img, table)
        assert _bits(got, _want(H, W, "floats", (3, 3, 0, 0)))
        assert _bits(got[2:], img[2:])
        got = _median_raw(img, np.array([1.75, np.inf, -np.inf, 2.0], np.float32))
        assert _bits(got, _want(H, W, "floats", (1, 3, 0, 2)))


# ----------------------------------------------------------------------------
# 2. C-ABI rejections
# ----------------------------------------------------------------------------
def test_abi_rejections_leave_the_output_alone():
    from vaeunet_amd import _lib as L
    H, W = 16, 12
    f32 = dict(dtype=torch.float32, device=DEV)
    img, rad = torch.rand(B, H, W, 3, **f32), torch.full((B,), 2.0, **f32)
    out, go = R.guarded((B, H, W, 3), torch.float32, DEV)
    out0, img0 = out.clone(), img.clone()

    def rm(B=B, H=H, W=W, src=img, r=rad, o=out):
        return L.query("vu_median_blur", L.ptr(src), B, H, W, L.ptr(r), L.ptr(o), L.stream())
    assert rm(src=None) == INVALID and rm(r=None) == INVALID and rm(o=None) == INVALID
    assert rm(o=img) == INVALID                                                    # in place
    assert rm(B=65536) == INVALID and rm(H=32769) == INVALID and rm(W=32769) == INVALID
    assert rm(B=-1) == INVALID and rm(H=-1) == INVALID and rm(W=-1) == INVALID
    assert rm(B=0) == 0 and rm(H=0) == 0 and rm(W=0) == 0 and rm(B=0, src=None, r=None, o=None) == 0
    assert rm(H=0, o=img) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, out0) and torch.equal(img, img0)
    go.check("rejected output")


# ----------------------------------------------------------------------------
# 3. the Python functions, PatchCache, the op
# ----------------------------------------------------------------------------
def _nchw(a):
    return torch.from_numpy(np.array(a)).permute(0, 3, 1, 2).to(DEV)          # channels_last [B, 3, H, W]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).cpu().numpy()


def _clahe_abi(img, clip, TY, TX):
    from vaeunet_amd import _lib as L
    n, H, W, _ = img.shape
    dimg, dclip = torch.from_numpy(np.array(img)).to(DEV), torch.from_numpy(np.asarray(clip, np.float32)).to(DEV)
    luts, out = torch.empty((n, TY, TX, 256), dtype=torch.uint8, device=DEV), torch.empty_like(dimg)
    L.call("vu_clahe_luts", L.ptr(dimg), n, H, W, L.ptr(dclip), TY, TX, L.ptr(luts), L.stream())
    L.call("vu_clahe_apply", L.ptr(dimg), n, H, W, L.ptr(dclip), TY, TX, L.ptr(luts), L.ptr(out), L.stream())
    return out.cpu().numpy()


def _blur_abi(img, table):
    from vaeunet_amd import _lib as L
    n, H, W, _ = img.shape
    dimg, dtab = torch.from_numpy(np.array(img)).to(DEV), torch.from_numpy(np.asarray(table, np.float32)).to(DEV)
    out = torch.empty_like(dimg)
    L.call("vu_blur_sep", L.ptr(dimg), n, H, W, L.ptr(dtab), L.ptr(out), L.stream())
    return out.cpu().numpy()


def test_python_functions_equal_the_chained_abi_stages():
    D = _D()
    H, W = 20, 12
    img = _image(H, W, "k255")
    rng = np.random.Generator(np.random.PCG64(3))
    msk = (rng.random((B, H, W, 1)) < 0.3).astype(np.float32)
    radii = np.array([2, 0, 3, 1], np.float32)
    timg, tmsk = _nchw(img), _nchw(msk)
    got = D.median_blur(timg, radii)
    assert got.is_contiguous(memory_format=torch.channels_last) and got.shape == timg.shape
    assert _bits(_nhwc(got), _median_raw(img, radii))
    assert _bits(_nhwc(D.median_blur(timg, [2, 0, 3, 1])), _median_raw(img, radii))             # integers
    assert _bits(_nhwc(D.median_blur(timg, 2)), _ref(H, W, "k255")[2])                          # a scalar radius
    sp = _image(H, W, "specials")
    assert _bits(_nhwc(D.median_blur(_nchw(sp), radii)), _want(H, W, "specials", (2, 0, 3, 1)))
    nchw = timg.contiguous()                                                                    # any input layout
    assert torch.equal(D.median_blur(nchw, radii), got)
    # the pipeline: CLAHE -> blur -> median -> vu_augment_patch
    clip = np.array([2.0, 0.0, 3.5, 1.0], np.float32)
    table = np.stack([D.blur_weights(sigma=1.0), D.blur_weights(box=5), D.identity_blur(1)[0], D.blur_weights(box=3)])
    aug = D.TrainAugment(p_rot90=0, p_affine=1.0, p_gamma=1.0, p_colour=1.0, p_noise=1.0)
    params, gx, gy = aug.draw(B, H, W, rng)
    kw = dict(seed=5, offset=2)
    c_abi = _clahe_abi(img, clip, 3, 2)
    cb_abi = _blur_abi(c_abi, table)
    want_i, want_m = D.augment_patches(_nchw(_median_raw(cb_abi, radii)), tmsk, params, gx, gy, **kw)
    got_i, got_m = D.augment_patches(timg, tmsk, params, gx, gy, clahe_clip=clip, clahe_tiles=(3, 2), blur=table,
                                     median=radii, **kw)
    assert torch.equal(got_i, want_i) and torch.equal(got_m, want_m)
    bare_i, bare_m = D.augment_patches(timg, tmsk, params, gx, gy, **kw)
    for extra, staged in ((dict(), img), (dict(clahe_clip=clip, clahe_tiles=(3, 2)), c_abi),
                          (dict(blur=table), _blur_abi(img, table))):
        gi, gm = D.augment_patches(timg, tmsk, params, gx, gy, median=radii, **extra, **kw)
        wi, _ = D.augment_patches(_nchw(_median_raw(staged, radii)), tmsk, params, gx, gy, **kw)
        assert torch.equal(gi, wi) and torch.equal(gm, bare_m)                                  # masks are not touched
        assert not torch.equal(gi, bare_i)
    # radius 0 everywhere is the path without the median
    zi, zm = D.augment_patches(timg, tmsk, params, gx, gy, median=0, **kw)
    assert torch.equal(zi, bare_i) and torch.equal(zm, bare_m)


def _write_cache(tmp_path, n=7, P=16):
    g = torch.Generator().manual_seed(4)
    for i in range(n):
        img = torch.randint(0, 256, (3, P, P), generator=g).float() / 255
        msk = (torch.rand(1, P, P, generator=g) < 0.1).float()
        torch.save({"image": img.contiguous(), "mask": msk.contiguous(), "coords": (i, 2 * i),
                    "has_lesion": torch.any(msk > 0.5)}, tmp_path / f"IDRiD_{i:02d}_{i}")


def test_patch_cache_with_the_median(tmp_path):
    D = _D()
    _write_cache(tmp_path)
    aug = D.TrainAugment(p_median=1.0, median_limit=5, p_blur=0.5)

    def epoch(augment, seed=9):
        return list(D.PatchCache(str(tmp_path), batch_size=3, device="cuda", augment=augment, seed=seed))
    e1, e2, plain = epoch(aug), epoch(aug), epoch(False)
    assert [b["image"].shape[0] for b in e1] == [3, 3, 1]
    for k, (a, b, p) in enumerate(zip(e1, e2, plain)):
        assert torch.equal(a["image"], b["image"]) and torch.equal(a["mask"], b["mask"])   # one seed, one epoch
        assert a["image"].is_contiguous(memory_format=torch.channels_last)
        ap = a["aug_params"]
        n = a["image"].shape[0]
        assert set(ap) == {"params", "gx", "gy", "seed", "offset", "border", "blur", "median"}
        assert ap["median"].shape == (n,) and ap["median"].dtype == np.float32 and ap["offset"] == k
        assert set(ap["median"].tolist()) <= {1.0, 2.0}
        ri, rm = D.augment_patches(p["image"], p["mask"], **ap)                             # replay
        assert torch.equal(ri, a["image"]) and torch.equal(rm, a["mask"])
        # the median did something: without it the same draw gives another image, the same mask
        bare = {key: v for key, v in ap.items() if key != "median"}
        ni, nm = D.augment_patches(p["image"], p["mask"], **bare)
        assert not torch.equal(ni, a["image"]) and torch.equal(nm, a["mask"])
    assert not torch.equal(epoch(aug, seed=10)[0]["image"], e1[0]["image"])


def test_patch_cache_without_the_median_is_what_it_was(tmp_path):
    """p_median = 0: the batches and aug_params are those of the existing path,
    drawn in the existing order from the cache's generator (draw, then
    draw_filters when a filter is on), with the launches the C ABI gives"""
    from vaeunet_amd import _lib as L
    D = _D()
    _write_cache(tmp_path)
    plain = list(D.PatchCache(str(tmp_path), batch_size=3, device="cuda", augment=False, seed=9))
    aug = D.TrainAugment(p_hflip=1.0, p_affine=0.8, p_grid=0.6, p_gamma=0.6, p_colour=0.8, p_noise=0.6)
    got = list(D.PatchCache(str(tmp_path), batch_size=3, device="cuda", augment=aug, seed=9))
    rng = np.random.Generator(np.random.PCG64(9))
    for k, (a, p) in enumerate(zip(got, plain)):
        assert set(a["aug_params"]) == {"params", "gx", "gy", "seed", "offset", "border"}
        n, _, H, W = p["image"].shape
        params, gx, gy = aug.draw(n, H, W, rng)
        assert a["aug_params"]["params"].tobytes() == params.tobytes()
        dp, dgx, dgy = (torch.from_numpy(t).to(DEV) for t in (params, gx, gy))
        oi, om = torch.empty_like(p["image"]), torch.empty_like(p["mask"])
        L.call("vu_augment_patch", L.ptr(p["image"]), L.ptr(p["mask"]), n, H, W, 3, 1, L.ptr(dp), L.ptr(dgx),
               L.ptr(dgy), gx.shape[1] - 1, 1, 9, k, L.ptr(oi), L.ptr(om), L.stream())
        assert torch.equal(oi, a["image"]) and torch.equal(om, a["mask"])
    # with the filters on: draw, then draw_filters, nothing after them
    aug = D.TrainAugment(p_clahe=0.5, p_blur=0.5, clahe_tiles=(2, 2))
    got = list(D.PatchCache(str(tmp_path), batch_size=3, device="cuda", augment=aug, seed=9))
    rng = np.random.Generator(np.random.PCG64(9))
    for k, (a, p) in enumerate(zip(got, plain)):
        ap = a["aug_params"]
        assert set(ap) == {"params", "gx", "gy", "seed", "offset", "border", "clahe_clip", "clahe_tiles", "blur"}
        n, _, H, W = p["image"].shape
        params, gx, gy = aug.draw(n, H, W, rng)
        clip, table = aug.draw_filters(n, rng)
        assert ap["params"].tobytes() == params.tobytes() and ap["clahe_clip"].tobytes() == clip.tobytes()
        assert ap["blur"].tobytes() == table.tobytes()
        staged = _nchw(_blur_abi(_clahe_abi(_nhwc(p["image"]), clip, 2, 2), table))
        wi, wm = D.augment_patches(staged, p["mask"], params, gx, gy, seed=9, offset=k)
        assert torch.equal(wi, a["image"]) and torch.equal(wm, a["mask"])


def test_dispatcher_op():
    D = _D()
    H, W = 20, 12
    timg = _nchw(_image(H, W, "specials"))
    radii = np.array([2, 0, 3, 1], np.float32)
    drad = torch.from_numpy(radii).to(DEV)
    mb = torch.ops.vaeunet.median_blur
    got = mb(timg, drad)
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert _bits(_nhwc(got), _nhwc(D.median_blur(timg, radii)))
    assert _bits(_nhwc(got), _want(H, W, "specials", (2, 0, 3, 1)))
    finite = _nchw(_image(H, W, "floats"))
    assert torch.equal(mb(finite, drad), D.median_blur(finite, radii))
    torch.library.opcheck(mb, (finite, drad))
    with pytest.raises((NotImplementedError, RuntimeError)):
        mb(finite.cpu(), drad.cpu())
