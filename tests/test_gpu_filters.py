"""vu_clahe_luts, vu_clahe_apply and vu_blur_sep (vaeunet_amd/csrc/filters.hip,
DESIGN.md §4.9) on the GPU against the numpy definition in tests/filters_ref.py,
through the C ABI on guarded buffers (inputs come back unchanged, no guard
element is written), B = 3.

Bounds (derived, not fitted):

  CLAHE tables          integer arithmetic on an fp32 quantisation done with two
      separately rounded operations: bitwise.
  CLAHE output, Gaussian blur   4 x the error of the same formulas evaluated by
      numpy in float32 against float64 on the same inputs, plus one float32 ulp
      of 1.0 (2^-23): the rule and the margin of §4.8's photometry tests (the
      device contracts a + t (b - a) to an fma and numpy does not).
  blur, dyadic          images on multiples of 2^-8 and weights that are powers
      of two: every product and partial sum is exact in float32 (at most 17
      significant bits), so the result is bitwise the float64 one.
  identity, off samples, B-independence   bitwise.

Measured on the MI355X (each test prints its figures, run with -s): CLAHE
output device error 9.3e-10-8.4e-8 = 0.50-1.01 x numpy float32's, at most 0.19
of the bound; Gaussian blur 6.1e-8-1.4e-7 = 0.77-1.20 x numpy float32's, at most
0.24 of the bound; the 96 CLAHE cases meet lim = 1 in 7932 tiles, r = 0 in 7416,
step >= 2 in 1005, step 1 in 75."""
import functools

import numpy as np
import pytest
import torch

import filters_ref as FR
import ref_small as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
INVALID = 1   # hipErrorInvalidValue
ULP1 = 2.0 ** -23
B = 3

CLAHE_SHAPES = [(16, 16, 2, 2), (17, 17, 4, 4), (20, 12, 3, 2), (45, 70, 2, 3), (16, 16, 1, 1), (12, 12, 12, 12)]
CLIPS = [0.5, 2.0, 4.0, 1e6]
KINDS = ["k255", "floats", "constant", "narrow"]
CLAHE_CASES = [(s, k, c) for s in CLAHE_SHAPES for k in KINDS for c in CLIPS]


def _id(case):
    (H, W, TY, TX), kind, clip = case
    return f"{H}x{W}-{TY}x{TX}-{kind}-clip{clip:g}"


def _D():
    import vaeunet_amd.data as D
    return D


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32),
                          np.ascontiguousarray(b, np.float32).view(np.int32))


@functools.lru_cache(maxsize=None)
def _image(H, W, kind):
    """NHWC float32 [3, H, W, 3]"""
    rng = np.random.Generator(np.random.PCG64(H * 1000 + W))
    if kind == "k255":
        img = rng.integers(0, 256, (B, H, W, 3)).astype(np.float32) / np.float32(255)
    elif kind == "floats":
        img = rng.random((B, H, W, 3), dtype=np.float32)
    elif kind == "constant":
        img = np.broadcast_to((rng.integers(0, 256, (B, 1, 1, 3)).astype(np.float32) / np.float32(255)),
                              (B, H, W, 3)).copy()
    else:
        img = rng.integers(100, 110, (B, H, W, 3)).astype(np.float32) / np.float32(255)
    img.setflags(write=False)
    return img


def _upload(arrays, dtype=torch.float32):
    bufs, guards = [], []
    for a in arrays:
        t, g = R.guarded(a.shape, dtype, DEV)
        t.copy_(torch.from_numpy(np.array(a)))            # a copy: the shared inputs are read-only
        bufs.append(t)
        guards.append(g)
    return bufs, guards


def _clahe_raw(img, clip, TY, TX):
    """vu_clahe_luts then vu_clahe_apply on guarded buffers -> (luts uint8, out) numpy"""
    from vaeunet_amd import _lib as L
    n, H, W, _ = img.shape
    clip = np.asarray(clip, np.float32)
    (dimg, dclip), guards = _upload((img, clip))
    luts, gl = R.guarded((n, TY, TX, 256), torch.uint8, DEV)
    out, go = R.guarded(img.shape, torch.float32, DEV)
    L.call("vu_clahe_luts", L.ptr(dimg), n, H, W, L.ptr(dclip), TY, TX, L.ptr(luts), L.stream())
    L.call("vu_clahe_apply", L.ptr(dimg), n, H, W, L.ptr(dclip), TY, TX, L.ptr(luts), L.ptr(out), L.stream())
    torch.cuda.synchronize()
    for g in guards + [gl, go]:
        g.check("clahe")
    assert np.array_equal(dimg.cpu().numpy(), img) and np.array_equal(dclip.cpu().numpy(), clip, equal_nan=True)
    return luts.cpu().numpy(), out.cpu().numpy()


def _blur_raw(img, table):
    from vaeunet_amd import _lib as L
    n, H, W, _ = img.shape
    table = np.ascontiguousarray(table, np.float32)
    (dimg, dtab), guards = _upload((img, table))
    out, go = R.guarded(img.shape, torch.float32, DEV)
    L.call("vu_blur_sep", L.ptr(dimg), n, H, W, L.ptr(dtab), L.ptr(out), L.stream())
    torch.cuda.synchronize()
    for g in guards + [go]:
        g.check("blur")
    assert np.array_equal(dimg.cpu().numpy(), img) and np.array_equal(dtab.cpu().numpy(), table, equal_nan=True)
    return out.cpu().numpy()


# ----------------------------------------------------------------------------
# 1. CLAHE
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clahe_ref(case):
    """(image, clip, reference tables, branch statistics): computed once, shared, read-only"""
    (H, W, TY, TX), kind, c = case
    img = _image(H, W, kind)
    clip = np.full(B, c, np.float32)
    stats = {}
    luts = FR.clahe_luts(img, clip, TY, TX, stats)
    luts.setflags(write=False)
    return img, clip, luts, stats


@functools.lru_cache(maxsize=None)
def _clahe_gpu(case):
    img, clip, _, _ = _clahe_ref(case)
    return _clahe_raw(img, clip, case[0][2], case[0][3])


@pytest.mark.parametrize("case", CLAHE_CASES, ids=_id)
def test_clahe_luts_are_bitwise(case):
    _, _, want, _ = _clahe_ref(case)
    got, _ = _clahe_gpu(case)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert (got[..., 255] == 255).all() and (np.diff(got.astype(np.int32), axis=-1) >= 0).all()


def test_clahe_cases_reach_every_branch():
    """from the reference alone: lim = 1, r = 0, 0 < r <= 128 (step >= 2), r > 128 (step 1)"""
    total = {}
    for case in CLAHE_CASES:
        for k, v in _clahe_ref(case)[3].items():
            total[k] = total.get(k, 0) + v
    print(f"CLAHE branches over {len(CLAHE_CASES)} cases: {total}")
    for key in ("lim1", "r0", "step>=2", "step1"):
        assert total.get(key, 0) > 0, (key, total)


@pytest.mark.parametrize("case", CLAHE_CASES, ids=_id)
def test_clahe_output_against_float64(case):
    (H, W, TY, TX), _, _ = case
    img, clip, luts, _ = _clahe_ref(case)
    _, got = _clahe_gpu(case)
    r64 = FR.clahe_apply(img, clip, TY, TX, luts)
    r32 = FR.clahe_apply(img, clip, TY, TX, luts, dtype=np.float32)
    cpu = float(np.abs(r32.astype(np.float64) - r64).max())
    gpu = float(np.abs(got.astype(np.float64) - r64).max())
    print(f"CLAHE output {_id(case)}: float32 numpy error {cpu:.3e}, device {gpu:.3e}, bound {4 * cpu + ULP1:.3e}")
    assert gpu <= 4 * cpu + ULP1, (gpu, cpu)
    assert got.min() >= 0 and got.max() <= 1


def test_clahe_off_sample_among_active_ones_is_bitwise():
    H, W, TY, TX = 20, 12, 3, 2
    img = _image(H, W, "floats")
    luts_on, out_on = _clahe_raw(img, np.array([2.0, 2.0, 4.0], np.float32), TY, TX)
    # the kernel takes 0, a negative value and a NaN as off (the host functions reject the last two)
    for clip in ([2.0, 0.0, 4.0], [0.0, 0.0, 0.0], [-1.0, 2.0, np.nan]):
        clip = np.asarray(clip, np.float32)
        luts, out = _clahe_raw(img, clip, TY, TX)
        for b in range(B):
            if clip[b] > 0:
                assert not _bits(out[b], img[b])
                assert _bits(out[b], out_on[b]) and np.array_equal(luts[b], luts_on[b])    # whatever its neighbours
            else:
                assert _bits(out[b], img[b]), b
                assert (luts[b] == np.arange(256, dtype=np.uint8)).all()


def test_clahe_moves_the_luma_to_the_table_value():
    """one tile, k/255 pixels: where no channel is clamped, v + (lut[Y] - Y) / 255 is again on the 8-bit grid and
    the luma of the output is lut[Y] exactly ((77 + 150 + 29) d = 256 d); a narrow band is spread out"""
    H, W = 16, 16
    img = _image(H, W, "narrow")
    luts, out = _clahe_raw(img, np.full(B, 1e6, np.float32), 1, 1)
    y0, y1 = FR.luma8(img), FR.luma8(out)
    free = ((out > 0) & (out < 1)).all(-1)
    assert free.mean() > 0.5
    for b in range(B):
        assert (y1[b][free[b]] == luts[b, 0, 0][y0[b]][free[b]]).all()
    assert y1.max() - y1.min() > 4 * (y0.max() - y0.min())


# ----------------------------------------------------------------------------
# 2. blur
# ----------------------------------------------------------------------------
def _row(r, w):
    row = np.zeros(9, np.float32)
    row[0], row[1:1 + len(w)] = r, w
    return row


IDENT = _row(0, [1.0])
DYADIC = {0: IDENT, 1: _row(1, [1 / 2, 1 / 4]), 2: _row(2, [1 / 4, 1 / 4, 1 / 8]), 7: _row(7, [1 / 8] + [1 / 16] * 7)}
BLUR_SHAPES = [(16, 16), (17, 17), (20, 12), (45, 70), (5, 3), (2, 9)]


def _dyadic_image(H, W):
    rng = np.random.Generator(np.random.PCG64(H * 100 + W))
    return (rng.integers(0, 257, (B, H, W, 3)) / 256.0).astype(np.float32)


@pytest.mark.parametrize("radii", [(0, 1, 7), (7, 2, 1), (7, 7, 7)], ids=lambda r: "r" + "".join(map(str, r)))
@pytest.mark.parametrize("HW", BLUR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_blur_dyadic_is_bitwise(HW, radii):
    H, W = HW
    img = _dyadic_image(H, W)
    table = np.stack([DYADIC[r] for r in radii])
    assert all(abs(float(t[1]) + 2 * float(t[2:].sum()) - 1) == 0 for t in table)
    out = _blur_raw(img, table)
    want = FR.blur(img, table)
    assert np.array_equal(want, want.astype(np.float32).astype(np.float64))        # exact in float32
    assert _bits(out, want.astype(np.float32)), np.argwhere(out != want)[:4]
    for b, r in enumerate(radii):
        if r == 0:
            assert _bits(out[b], img[b])
        elif H > 1 or W > 1:
            assert not _bits(out[b], img[b])


@pytest.mark.parametrize("HW", BLUR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_blur_identity_row_is_bitwise(HW):
    H, W = HW
    rng = np.random.Generator(np.random.PCG64(7))
    img = (rng.random((B, H, W, 3), dtype=np.float32) * 4 - 2).astype(np.float32)   # any floats, not only [0, 1]
    img[0, 0, 0, 0] = -0.0
    assert _bits(_blur_raw(img, np.stack([IDENT] * B)), img)


@pytest.mark.parametrize("HW", BLUR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_blur_gaussian_against_float64(HW):
    D = _D()
    H, W = HW
    sigmas = (0.5, 1.0, 2.3)
    rng = np.random.Generator(np.random.PCG64(H + W))
    img = rng.random((B, H, W, 3), dtype=np.float32)
    table = np.stack([D.blur_weights(sigma=s) for s in sigmas])
    assert [int(t[0]) for t in table] == [2, 3, 7]
    out = _blur_raw(img, table)
    r64, r32 = FR.blur(img, table), FR.blur(img, table, dtype=np.float32)
    for b, s in enumerate(sigmas):
        cpu = float(np.abs(r32[b].astype(np.float64) - r64[b]).max())
        gpu = float(np.abs(out[b].astype(np.float64) - r64[b]).max())
        print(f"blur {H}x{W} sigma {s}: float32 numpy error {cpu:.3e}, device {gpu:.3e}, bound {4 * cpu + ULP1:.3e}")
        assert gpu <= 4 * cpu + ULP1, (b, gpu, cpu)


def test_blur_kernel_clamps_the_radius():
    """outside the host's validation: r = 9 runs as 7, r = -3 and NaN as 0, a fraction is truncated"""
    H, W = 17, 17
    img = _dyadic_image(H, W)
    w7 = DYADIC[7][1:]
    for r_in, r_eff in ((9.0, 7), (-3.0, 0), (np.nan, 0), (1.75, 1)):
        table = np.stack([_row(0, w7)] * B)
        table[:, 0] = r_in
        want = np.stack([_row(r_eff, w7)] * B)
        assert _bits(_blur_raw(img, table), FR.blur(img, want).astype(np.float32)), r_in


# ----------------------------------------------------------------------------
# 3. independence of B
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("HW", [(17, 17), (45, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sample_alone_equals_sample_in_batch(HW):
    D = _D()
    H, W = HW
    img = _image(H, W, "floats")
    clip = np.array([2.0, 4.0, 0.5], np.float32)
    luts3, out3 = _clahe_raw(img, clip, 2, 3)
    luts1, out1 = _clahe_raw(img[1:2], clip[1:2], 2, 3)
    assert np.array_equal(luts3[1:2], luts1) and _bits(out3[1:2], out1)
    table = np.stack([D.blur_weights(sigma=s) for s in (0.5, 2.3, 1.0)])
    assert _bits(_blur_raw(img, table)[1:2], _blur_raw(img[1:2], table[1:2]))


# ----------------------------------------------------------------------------
# 4. C-ABI rejections
# ----------------------------------------------------------------------------
def test_abi_rejections_leave_the_outputs_alone():
    from vaeunet_amd import _lib as L
    H, W = 16, 12
    f32 = dict(dtype=torch.float32, device=DEV)
    img, clip, table = torch.rand(B, H, W, 3, **f32), torch.full((B,), 2.0, **f32), torch.zeros(B, 9, **f32)
    table[:, 1] = 1
    luts, gl = R.guarded((B, 2, 2, 256), torch.uint8, DEV)
    out, go = R.guarded((B, H, W, 3), torch.float32, DEV)
    luts0, out0 = luts.clone(), out.clone()

    def rl(B=B, H=H, W=W, TY=2, TX=2, src=img, c=clip, l=luts):
        return L.query("vu_clahe_luts", L.ptr(src), B, H, W, L.ptr(c), TY, TX, L.ptr(l), L.stream())

    def ra(B=B, H=H, W=W, TY=2, TX=2, src=img, c=clip, l=luts, o=out):
        return L.query("vu_clahe_apply", L.ptr(src), B, H, W, L.ptr(c), TY, TX, L.ptr(l), L.ptr(o), L.stream())

    def rb(B=B, H=H, W=W, src=img, t=table, o=out):
        return L.query("vu_blur_sep", L.ptr(src), B, H, W, L.ptr(t), L.ptr(o), L.stream())
    for rc in (rl, ra):
        assert rc(src=None) == INVALID and rc(c=None) == INVALID and rc(l=None) == INVALID
        assert rc(B=65536) == INVALID and rc(H=32769) == INVALID and rc(W=32769) == INVALID
        assert rc(B=-1) == INVALID and rc(H=-1) == INVALID and rc(W=-1) == INVALID
        assert rc(TY=0) == INVALID and rc(TX=0) == INVALID and rc(TY=17) == INVALID and rc(TX=17) == INVALID
        assert rc(TX=13) == INVALID and rc(H=3, TY=4) == INVALID and rc(H=0) == INVALID   # more tiles than pixels
        assert rc(B=0) == 0 and rc(B=0, src=None, c=None, l=None) == 0
        assert rc(B=0, TY=0) == INVALID and rc(B=0, TX=17) == INVALID
    assert ra(o=None) == INVALID
    assert rb(src=None) == INVALID and rb(t=None) == INVALID and rb(o=None) == INVALID
    assert rb(B=65536) == INVALID and rb(H=32769) == INVALID and rb(W=32769) == INVALID
    assert rb(B=-1) == INVALID and rb(H=-1) == INVALID and rb(W=-1) == INVALID
    assert rb(B=0) == 0 and rb(H=0) == 0 and rb(W=0) == 0 and rb(B=0, src=None, t=None, o=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, out0) and torch.equal(luts, luts0)
    gl.check("rejected luts")
    go.check("rejected output")


# ----------------------------------------------------------------------------
# 5. the Python functions, PatchCache, the ops
# ----------------------------------------------------------------------------
def _nchw(a):
    return torch.from_numpy(np.array(a)).permute(0, 3, 1, 2).to(DEV)          # channels_last [B, 3, H, W]


def test_python_functions_equal_the_chained_abi_stages():
    D = _D()
    H, W = 20, 12
    img = _image(H, W, "floats")
    rng = np.random.Generator(np.random.PCG64(3))
    msk = (rng.random((B, H, W, 1)) < 0.3).astype(np.float32)
    clip = np.array([2.0, 0.0, 3.5], np.float32)
    table = np.stack([D.blur_weights(sigma=1.0), D.blur_weights(box=5), D.identity_blur(1)[0]])
    timg, tmsk = _nchw(img), _nchw(msk)
    _, c_abi = _clahe_raw(img, clip, 3, 2)
    got = D.clahe(timg, clip, (3, 2))
    assert got.is_contiguous(memory_format=torch.channels_last) and got.shape == timg.shape
    assert _bits(got.permute(0, 2, 3, 1).cpu().numpy(), c_abi)
    assert _bits(D.clahe(timg, 2.0, (3, 2)).permute(0, 2, 3, 1).cpu().numpy(),
                 _clahe_raw(img, np.full(B, 2.0, np.float32), 3, 2)[1])                    # a scalar clip limit
    b_abi = _blur_raw(img, table)
    got = D.blur(timg, table)
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert _bits(got.permute(0, 2, 3, 1).cpu().numpy(), b_abi)
    # the pipeline: CLAHE -> blur -> vu_augment_patch
    aug = D.TrainAugment(p_rot90=0, p_affine=1.0, p_gamma=1.0, p_colour=1.0, p_noise=1.0)
    params, gx, gy = aug.draw(B, H, W, rng)
    staged = _nchw(_blur_raw(c_abi, table))
    want_i, want_m = D.augment_patches(staged, tmsk, params, gx, gy, seed=5, offset=2)
    got_i, got_m = D.augment_patches(timg, tmsk, params, gx, gy, seed=5, offset=2, clahe_clip=clip,
                                     clahe_tiles=(3, 2), blur=table)
    assert torch.equal(got_i, want_i) and torch.equal(got_m, want_m)
    only_c = D.augment_patches(timg, tmsk, params, gx, gy, seed=5, offset=2, clahe_clip=clip, clahe_tiles=(3, 2))
    assert torch.equal(only_c[0], D.augment_patches(_nchw(c_abi), tmsk, params, gx, gy, seed=5, offset=2)[0])
    only_b = D.augment_patches(timg, tmsk, params, gx, gy, seed=5, offset=2, blur=table)
    assert torch.equal(only_b[0], D.augment_patches(_nchw(b_abi), tmsk, params, gx, gy, seed=5, offset=2)[0])
    assert torch.equal(only_b[1], want_m) and torch.equal(only_c[1], want_m)              # masks are not touched


def _write_cache(tmp_path, n=7, P=16):
    g = torch.Generator().manual_seed(4)
    for i in range(n):
        img = torch.randint(0, 256, (3, P, P), generator=g).float() / 255
        msk = (torch.rand(1, P, P, generator=g) < 0.1).float()
        torch.save({"image": img.contiguous(), "mask": msk.contiguous(), "coords": (i, 2 * i),
                    "has_lesion": torch.any(msk > 0.5)}, tmp_path / f"IDRiD_{i:02d}_{i}")


def test_patch_cache_with_filters(tmp_path):
    D = _D()
    _write_cache(tmp_path)
    aug = D.TrainAugment(p_clahe=1.0, p_blur=1.0, clahe_tiles=(2, 2))

    def epoch(augment, seed=9):
        return list(D.PatchCache(str(tmp_path), batch_size=3, device="cuda", augment=augment, seed=seed))
    e1, e2, plain = epoch(aug), epoch(aug), epoch(False)
    assert [b["image"].shape[0] for b in e1] == [3, 3, 1]
    for k, (a, b, p) in enumerate(zip(e1, e2, plain)):
        assert torch.equal(a["image"], b["image"]) and torch.equal(a["mask"], b["mask"])   # one seed, one epoch
        assert a["image"].is_contiguous(memory_format=torch.channels_last)
        ap = a["aug_params"]
        n = a["image"].shape[0]
        assert ap["clahe_clip"].shape == (n,) and (ap["clahe_clip"] >= 1).all() and ap["clahe_tiles"] == (2, 2)
        assert ap["blur"].shape == (n, 9) and (ap["blur"][:, 0] >= 2).all() and ap["offset"] == k
        ri, rm = D.augment_patches(p["image"], p["mask"], **ap)                             # replay
        assert torch.equal(ri, a["image"]) and torch.equal(rm, a["mask"])
        # the filters did something: without them the same draw gives another image, the same mask
        bare = {key: v for key, v in ap.items() if key not in ("clahe_clip", "clahe_tiles", "blur")}
        ni, nm = D.augment_patches(p["image"], p["mask"], **bare)
        assert not torch.equal(ni, a["image"]) and torch.equal(nm, a["mask"])
    assert not torch.equal(epoch(aug, seed=10)[0]["image"], e1[0]["image"])


def test_patch_cache_without_filters_is_what_it_was(tmp_path):
    """p_clahe = p_blur = 0: the batches are the one vu_augment_patch launch on
    the arrays draw() gives from the cache's generator, as before the filters
    existed; aug_params holds no new key"""
    from vaeunet_amd import _lib as L
    D = _D()
    _write_cache(tmp_path)
    aug = D.TrainAugment(p_hflip=1.0, p_affine=0.8, p_grid=0.6, p_gamma=0.6, p_colour=0.8, p_noise=0.6)
    got = list(D.PatchCache(str(tmp_path), batch_size=3, device="cuda", augment=aug, seed=9))
    plain = list(D.PatchCache(str(tmp_path), batch_size=3, device="cuda", augment=False, seed=9))
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


def test_dispatcher_ops():
    D = _D()
    H, W = 20, 12
    timg = _nchw(_image(H, W, "floats"))
    clip = np.array([2.0, 0.0, 3.5], np.float32)
    table = np.stack([D.blur_weights(sigma=1.0), D.blur_weights(box=5), D.identity_blur(1)[0]])
    dclip, dtable = torch.from_numpy(clip).to(DEV), torch.from_numpy(table).to(DEV)
    cl, bl = torch.ops.vaeunet.clahe, torch.ops.vaeunet.blur_separable
    assert torch.equal(cl(timg, dclip, 3, 2), D.clahe(timg, clip, (3, 2)))
    assert torch.equal(cl(timg, dclip), D.clahe(timg, clip))
    assert torch.equal(bl(timg, dtable), D.blur(timg, table))
    torch.library.opcheck(cl, (timg, dclip), {"tiles_y": 3, "tiles_x": 2})
    torch.library.opcheck(bl, (timg, dtable))
    with pytest.raises((NotImplementedError, RuntimeError)):
        cl(timg.cpu(), dclip.cpu())
    with pytest.raises((NotImplementedError, RuntimeError)):
        bl(timg.cpu(), dtable.cpu())
