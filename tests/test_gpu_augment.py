"""vu_augment_patch (vaeunet_amd/csrc/augment.hip) on the GPU
against the float64 definition in tests/augment_ref.py, which works on the
same float32 parameter values.

Bounds (derived, not fitted):

  geometry, exact cases   identity, flips / rot90, integer shifts: bitwise.
  geometry, general       eps = 2^-24 bounds the relative error of one float32
      rounding.  u = k[c] + r d[c] with d = (k[c+1] - k[c]) / (W - 1): the knot
      difference, the division, the product and the sum each round a quantity
      of magnitude <= W, so |du| <= 4 eps W (dv likewise with H).  sx = a0 u +
      a1 v + a2 propagates |a0| du + |a1| dv and adds at most three roundings of
      terms of magnitude <= T = |a0| W + |a1| H + |a2|: delta = 3 eps T +
      4 eps (|a0| W + |a1| H) <= 7 eps T, taken per sample over both rows.  The
      bilinear surface (zero-padded or reflected) is continuous with slope <=
      max|v| per axis, so the image differs by at most 4 delta max|v| (twice the
      two axes) plus 4 float32 ulps of max|v| for the three lerps.  The mask is
      exact wherever the float64 coordinate + 0.5 is farther than delta from an
      integer on both axes; the other pixels are left out and must be <= 2 %.
  photometry / noise      4 x the error of the same formulas evaluated by numpy
      in float32 against float64 on the same inputs (the margin covers the
      device's powf / logf / sinf / cosf against numpy's).

Measured on the MI355X (each test prints its figures, run with -s): general
affine image error 0.018-0.036 of its bound with no mask pixel left out;
photometry device error 8.8e-8-1.7e-7 = 0.69-0.92 x numpy float32's; noise
9.9e-7-1.4e-6 = 1.00-1.09 x numpy float32's; moments of 12288 normals: mean
-0.0034, variance 1.0069."""
import numpy as np
import pytest
import torch

import augment_ref as AR
import ref_small as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
INVALID = 1   # hipErrorInvalidValue
EPS = 2.0 ** -24
SHAPES = [(16, 16), (17, 17), (20, 12)]
BORDER_NAMES = {AR.CONSTANT: "constant", AR.REFLECT101: "reflect101"}


def _D():
    import vaeunet_amd.data as D
    return D


def _inputs(B, H, W, Cm, seed):
    """NHWC numpy image in [0, 1] and 0/1 mask"""
    rng = np.random.Generator(np.random.PCG64(seed))
    img = rng.random((B, H, W, 3), dtype=np.float32)
    msk = (rng.random((B, H, W, Cm)) < 0.3).astype(np.float32)
    return img, msk


def _raw(img, msk, params, gx, gy, seed=0, offset=0, border=AR.REFLECT101):
    """One vu_augment_patch launch through the C ABI on guarded buffers; NHWC
    numpy in and out.  The inputs must come back unchanged and no guard
    element may be written."""
    from vaeunet_amd import _lib as L
    B, H, W, C = img.shape
    Cm, S = msk.shape[3], gx.shape[1] - 1
    bufs, guards = [], []
    for a in (img, msk, params, gx, gy):
        t, g = R.guarded(a.shape, torch.float32, DEV)
        t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        bufs.append(t)
        guards.append(g)
    oi, goi = R.guarded(img.shape, torch.float32, DEV)
    om, gom = R.guarded(msk.shape, torch.float32, DEV)
    L.call("vu_augment_patch", L.ptr(bufs[0]), L.ptr(bufs[1]), B, H, W, C, Cm, L.ptr(bufs[2]), L.ptr(bufs[3]),
           L.ptr(bufs[4]), S, border, seed, offset, L.ptr(oi), L.ptr(om), L.stream())
    torch.cuda.synchronize()
    for g in guards + [goi, gom]:
        g.check("augment")
    for t, a in zip(bufs, (img, msk, params, gx, gy)):
        assert np.array_equal(t.cpu().numpy(), a)
    return oi.cpu().numpy(), om.cpu().numpy()


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32),
                          np.ascontiguousarray(b, np.float32).view(np.int32))


def _ident(B, H, W, S=1):
    D = _D()
    return D.identity_params(B), D.identity_knots(B, W, S), D.identity_knots(B, H, S)


# ----------------------------------------------------------------------------
# 1. identity
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("border", [AR.CONSTANT, AR.REFLECT101], ids=["constant", "reflect101"])
@pytest.mark.parametrize("Cm", [1, 2])
@pytest.mark.parametrize("HW", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity_is_bitwise(HW, Cm, border):
    H, W = HW
    img, msk = _inputs(3, H, W, Cm, 1)
    oi, om = _raw(img, msk, *_ident(3, H, W), border=border)
    assert _bits(oi, img) and _bits(om, msk)


# ----------------------------------------------------------------------------
# 2. flips and rot90
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("border", [AR.CONSTANT, AR.REFLECT101], ids=["constant", "reflect101"])
def test_flips_and_rot90_match_torch_and_the_integer_gather(border):
    D = _D()
    P = 16
    flags = [(h, v, k) for h in (0, 1) for v in (0, 1) for k in range(4)]
    img, msk = _inputs(16, P, P, 2, 2)
    params, gx, gy = _ident(16, P, P)
    for b, f in enumerate(flags):
        params[b, :6] = D.affine_matrix(P, P, *f)
    timg = torch.from_numpy(img).permute(0, 3, 1, 2).to(DEV)          # channels_last [B, 3, P, P]
    tmsk = torch.from_numpy(msk).permute(0, 3, 1, 2).to(DEV)
    oi, om = D.augment_patches(timg, tmsk, params, gx, gy, seed=0, border=BORDER_NAMES[border])
    assert oi.is_contiguous(memory_format=torch.channels_last) and om.shape == tmsk.shape
    pc = D.PatchCache([], batch_size=16, device="cuda")
    gi, gm, _ = pc.augment_batch(timg, tmsk, flags)
    assert torch.equal(oi, gi) and torch.equal(om, gm)
    for b, (h, v, k) in enumerate(flags):
        for src, got in ((timg[b], oi[b]), (tmsk[b], om[b])):
            ref = src
            if h:
                ref = torch.flip(ref, (2,))
            if v:
                ref = torch.flip(ref, (1,))
            assert torch.equal(got, torch.rot90(ref, k, (1, 2))), (h, v, k)


# ----------------------------------------------------------------------------
# 3. integer shifts
# ----------------------------------------------------------------------------
def _shifted(x, dy, dx, border):
    """x [H, W, C]: out[i, j] = x[i + dy, j + dx] under the border mode"""
    H, W, _ = x.shape
    py, px = abs(dy), abs(dx)
    mode = dict(mode="reflect") if border == AR.REFLECT101 else dict(mode="constant", constant_values=0)
    big = np.pad(x, ((py, py), (px, px), (0, 0)), **mode)
    return big[py + dy:py + dy + H, px + dx:px + dx + W]


@pytest.mark.parametrize("border", [AR.CONSTANT, AR.REFLECT101], ids=["constant", "reflect101"])
@pytest.mark.parametrize("HW", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_integer_shifts_are_exact(HW, border):
    H, W = HW
    shifts = [(3, 5), (-3, 5), (3, -5), (-3, -5), (37, -41)]      # (dx, dy); the last is larger than the patch
    B = len(shifts)
    img, msk = _inputs(B, H, W, 2, 3)
    params, gx, gy = _ident(B, H, W)
    for b, (dx, dy) in enumerate(shifts):
        params[b, 2], params[b, 5] = dx, dy
    oi, om = _raw(img, msk, params, gx, gy, border=border)
    for b, (dx, dy) in enumerate(shifts):
        assert _bits(oi[b], _shifted(img[b], dy, dx, border)), (dx, dy)
        assert _bits(om[b], _shifted(msk[b], dy, dx, border)), (dx, dy)


# ----------------------------------------------------------------------------
# 4. general affine, with and without grid distortion
# ----------------------------------------------------------------------------
def _general(H, W, B, S, seed):
    """random rotation in +-45 deg, scale in [0.8, 1.25], shift in +-10 %; knots at limit 0.3 when S > 1"""
    D = _D()
    rng = np.random.Generator(np.random.PCG64(seed))
    params, gx, gy = _ident(B, H, W, S)
    aug = D.TrainAugment(grid_steps=S, grid_limit=0.3)
    for b in range(B):
        params[b, :6] = D.affine_matrix(H, W, angle=rng.uniform(-45, 45), scale=rng.uniform(0.8, 1.25),
                                        shift=(rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)))
        if S > 1:
            gx[b], gy[b] = aug._knots(W, S, rng), aug._knots(H, S, rng)
    return params, gx, gy


def _delta(p, H, W):
    p = np.abs(np.asarray(p, np.float64))
    T = max(p[0] * W + p[1] * H + p[2], p[3] * W + p[4] * H + p[5])
    return 7 * EPS * T


@pytest.mark.parametrize("border", [AR.CONSTANT, AR.REFLECT101], ids=["constant", "reflect101"])
@pytest.mark.parametrize("S", [1, 4, 5])
@pytest.mark.parametrize("Cm", [1, 2])
@pytest.mark.parametrize("HW", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_general_affine_against_float64(HW, Cm, S, border):
    _check_general(HW[0], HW[1], 3, Cm, S, border)


@pytest.mark.parametrize("border", [AR.CONSTANT, AR.REFLECT101], ids=["constant", "reflect101"])
def test_general_affine_over_several_tiles(border):
    """45 x 70: three 32-wide and six 8-tall tiles per sample, ragged on both axes"""
    H, W = 45, 70
    img, msk = _inputs(2, H, W, 1, 1)
    oi, om = _raw(img, msk, *_ident(2, H, W), border=border)
    assert _bits(oi, img) and _bits(om, msk)
    _check_general(H, W, 2, 1, 5, border)


def _check_general(H, W, B, Cm, S, border):
    img, msk = _inputs(B, H, W, Cm, 4)
    params, gx, gy = _general(H, W, B, S, 100 + S)
    oi, om = _raw(img, msk, params, gx, gy, border=border)
    ri, rm = AR.augment(img, msk, params, gx, gy, 0, 0, border)
    vmax = float(img.max())
    worst, left_out = 0.0, 0
    for b in range(B):
        delta = _delta(params[b], H, W)
        assert delta < 1e-4
        bound = 4 * delta * vmax + 4 * 2.0 ** -23 * vmax
        err = float(np.abs(oi[b] - ri[b]).max())
        worst = max(worst, err / bound)
        assert err <= bound, (b, err, bound)
        sx, sy = AR.source_coords(params[b], gx[b], gy[b], H, W)
        near = (np.abs(sx + 0.5 - np.round(sx + 0.5)) <= delta) | (np.abs(sy + 0.5 - np.round(sy + 0.5)) <= delta)
        left_out += int(near.sum())
        assert np.array_equal(om[b][~near], rm[b][~near]), b
    # the seed check: the reference alone decides how many pixels sit on a rounding boundary
    assert left_out <= 0.02 * B * H * W, left_out
    print(f"general affine {H}x{W} S={S} {BORDER_NAMES[border]}: image error / bound {worst:.3f}, "
          f"{left_out} mask pixels left out")


# ----------------------------------------------------------------------------
# 5. photometry
# ----------------------------------------------------------------------------
def _photo_params(B):
    D = _D()
    params = D.identity_params(B)
    cols = [D.colour_matrix(0.1, 0.2, -0.3, 0.05), D.colour_matrix(-0.15, -0.2, 0.4, -0.1),
            D.colour_matrix(0.05, 0.3, 0.2, 0.25)]
    for b in range(B):
        params[b, 6] = (0.8, 1.25, 0.8)[b % 3]
        M, o = cols[b % 3]
        params[b, 7:16], params[b, 16:19] = M.reshape(9), o
    return params


@pytest.mark.parametrize("HW", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_photometry_against_float64(HW):
    H, W = HW
    B = 3
    img, msk = _inputs(B, H, W, 1, 5)
    img[0, 0, 0] = 0.0                                   # pow(0, g)
    params = _photo_params(B)
    _, gx, gy = _ident(B, H, W)
    oi, om = _raw(img, msk, params, gx, gy)
    assert _bits(om, msk)
    for b in range(B):
        r64 = AR.photometry(img[b], params[b])
        r32 = AR.photometry(img[b], params[b], dtype=np.float32)
        cpu = float(np.abs(r32.astype(np.float64) - r64).max())
        gpu = float(np.abs(oi[b].astype(np.float64) - r64).max())
        print(f"photometry {H}x{W} sample {b} (gamma {params[b, 6]}): float32 numpy error {cpu:.3e}, device {gpu:.3e}, "
              f"ratio {gpu / cpu:.2f}")
        assert cpu > 0 and gpu <= 4 * cpu, (b, gpu, cpu)


def test_photometry_clip_is_exact():
    """v <- 3 v - 1 overshoots on both sides: exactly 0 below 1/3, exactly 1 above 2/3"""
    H, W = 17, 17
    img, msk = _inputs(3, H, W, 1, 6)
    params, gx, gy = _ident(3, H, W)
    params[:, 7], params[:, 11], params[:, 15] = 3.0, 3.0, 3.0
    params[:, 16:19] = -1.0
    oi, _ = _raw(img, msk, params, gx, gy)
    lin = 3.0 * img.astype(np.float64) - 1.0
    assert (oi[lin < -1e-6] == 0).all() and (oi[lin > 1 + 1e-6] == 1).all()
    assert (lin < 0).sum() > 100 and (lin > 1).sum() > 100 and oi.min() == 0 and oi.max() == 1
    mid = (lin > 1e-6) & (lin < 1 - 1e-6)
    assert np.abs(oi[mid] - lin[mid]).max() <= 4 * 2.0 ** -23


# ----------------------------------------------------------------------------
# 6. noise
# ----------------------------------------------------------------------------
SIGMA = np.float32(0.05)


def _noise_run(B, H, W, seed, offset=0):
    img = np.full((B, H, W, 3), 0.5, np.float32)
    msk = np.zeros((B, H, W, 1), np.float32)
    params, gx, gy = _ident(B, H, W)
    params[:, 19] = SIGMA
    return _raw(img, msk, params, gx, gy, seed=seed, offset=offset)[0]


@pytest.mark.parametrize("HW", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_noise_equals_the_reference_normals(HW):
    """(out - 0.5) / sigma against the float64 normals.  The float32 yardstick
    is the kernel's whole formula in numpy float32: Box-Muller on the same
    words, 0.5 + sigma n, then the same (out - 0.5) / sigma in float64."""
    H, W = HW
    seed, offset = 0x1234_5678_9ABC_DEF0, 7
    out = _noise_run(3, H, W, seed, offset)
    s64 = float(SIGMA)
    for b in range(3):
        words = AR.pixel_words(H, W, b, seed, offset)
        n64 = AR.normals(words)
        n32 = AR.normals(words, np.float32)
        assert np.abs(n64).max() <= 6.7
        out32 = np.float32(0.5) + SIGMA * n32
        cpu = float(np.abs((out32.astype(np.float64) - 0.5) / s64 - n64).max())
        gpu = float(np.abs((out[b].astype(np.float64) - 0.5) / s64 - n64).max())
        print(f"noise {H}x{W} sample {b}: float32 numpy error {cpu:.3e}, device {gpu:.3e}, ratio {gpu / cpu:.2f}")
        assert cpu > 0 and gpu <= 4 * cpu, (b, gpu, cpu)


def test_noise_is_a_function_of_seed_offset_sample_pixel():
    H, W = 17, 17
    a = _noise_run(3, H, W, 11, 0)
    assert _bits(a, _noise_run(3, H, W, 11, 0))                       # reproducible
    assert not _bits(a, _noise_run(3, H, W, 12, 0))                   # seed
    assert not _bits(a, _noise_run(3, H, W, 11 + 2 ** 32, 0))         # high word of the seed
    assert not _bits(a, _noise_run(3, H, W, 11, 1))                   # offset
    assert not _bits(a[0], a[1]) and not _bits(a[1], a[2])            # sample
    assert _bits(a[:1], _noise_run(1, H, W, 11, 0))                   # independent of B


def test_noise_moments():
    H = W = 64
    n = (_noise_run(1, H, W, 5).astype(np.float64) - 0.5) / float(SIGMA)
    N = n.size
    assert abs(n.mean()) <= 5 / np.sqrt(N)
    assert abs(n.var() - 1) <= 5 * np.sqrt(2 / N)
    # the three channels are different normals
    assert abs(np.corrcoef(n[0, ..., 0].ravel(), n[0, ..., 1].ravel())[0, 1]) <= 5 / np.sqrt(H * W)
    print(f"noise moments over {N}: mean {n.mean():.4f}, var {n.var():.4f}")


# ----------------------------------------------------------------------------
# 7. C-ABI rejections
# ----------------------------------------------------------------------------
def test_abi_rejections_leave_the_outputs_alone():
    from vaeunet_amd import _lib as L
    B, H, W = 3, 16, 16
    f32 = dict(dtype=torch.float32, device=DEV)
    img, msk = torch.rand(B, H, W, 4, **f32), torch.rand(B, H, W, 2, **f32)
    params = torch.from_numpy(_D().identity_params(B)).to(DEV)
    knots = torch.from_numpy(_D().identity_knots(B, W, 33)).to(DEV)
    oi, goi = R.guarded((B, H, W, 4), torch.float32, DEV)
    om, gom = R.guarded((B, H, W, 2), torch.float32, DEV)
    oi0, om0 = oi.clone(), om.clone()

    def rc(B=B, C=3, Cm=1, S=1, border=1, out=oi, mout=om, src=img):
        return L.query("vu_augment_patch", L.ptr(src), L.ptr(msk), B, H, W, C, Cm, L.ptr(params), L.ptr(knots),
                       L.ptr(knots), S, border, 0, 0, L.ptr(out), L.ptr(mout), L.stream())
    assert rc(C=1) == INVALID and rc(C=4) == INVALID
    assert rc(Cm=0) == INVALID
    assert rc(S=0) == INVALID and rc(S=33) == INVALID
    assert rc(border=7) == INVALID and rc(border=-1) == INVALID
    assert rc(out=None) == INVALID and rc(mout=None) == INVALID and rc(src=None) == INVALID
    assert rc(B=-1) == INVALID
    assert rc(B=0) == 0 and rc(B=0, out=None, mout=None, src=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(oi, oi0) and torch.equal(om, om0)
    goi.check("rejected image")
    gom.check("rejected mask")


# ----------------------------------------------------------------------------
# 8. PatchCache(augment=TrainAugment(...))
# ----------------------------------------------------------------------------
def _write_cache(tmp_path, n=7, P=16):
    g = torch.Generator().manual_seed(4)
    recs = []
    for i in range(n):
        img = torch.rand(3, P, P, generator=g)
        msk = (torch.rand(1, P, P, generator=g) < 0.1).float()
        rec = {"image": img.contiguous(), "mask": msk.contiguous(), "coords": (i, 2 * i),
               "has_lesion": torch.any(msk > 0.5)}
        torch.save(rec, tmp_path / f"IDRiD_{i:02d}_{i}")
        recs.append(rec)
    return recs


def test_patch_cache_with_train_augment(tmp_path):
    D = _D()
    _write_cache(tmp_path)
    # every sample is flipped (so every batch changes); the other coins are raised to meet every transform in 7 draws
    aug = D.TrainAugment(p_hflip=1.0, p_affine=0.8, p_grid=0.6, p_gamma=0.6, p_colour=0.8, p_noise=0.6)

    def epoch(augment, seed=9):
        return list(D.PatchCache(str(tmp_path), batch_size=3, device="cuda", augment=augment, seed=seed))
    e1, e2, plain = epoch(aug), epoch(aug), epoch(False)
    assert [b["image"].shape[0] for b in e1] == [3, 3, 1]
    changed = 0
    for k, (a, b, p) in enumerate(zip(e1, e2, plain)):
        for key in ("image", "mask"):
            t = a[key]
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(memory_format=torch.channels_last)
            assert t.shape == p[key].shape
            assert torch.equal(t, b[key])                                   # same seed: the same epoch, bitwise
        assert float(a["image"].min()) >= 0 and float(a["image"].max()) <= 1
        assert bool(((a["mask"] == 0) | (a["mask"] == 1)).all())
        assert a["img_id"] == p["img_id"] and a["coords"] == p["coords"]
        ap = a["aug_params"]
        assert ap["offset"] == k and ap["seed"] == 9 and ap["border"] == "reflect101"
        ri, rm = D.augment_patches(p["image"], p["mask"], **ap)             # replay on the un-augmented batch
        assert torch.equal(ri, a["image"]) and torch.equal(rm, a["mask"])
        changed += int(not torch.equal(a["image"], p["image"]))
    assert changed == 3
    assert "aug_params" not in plain[0]
    e3 = epoch(aug, seed=10)
    assert not torch.equal(e3[0]["image"], e1[0]["image"])


def test_patch_cache_flip_path_unchanged(tmp_path):
    """augment=True: still the flip / rot90 gather on flags drawn from the
    seeded generator (test_gpu_data.py's assertion on drawn flags)"""
    D = _D()
    _write_cache(tmp_path, n=16)
    pc = D.PatchCache(str(tmp_path), batch_size=16, device="cuda", augment=True, seed=3)
    plain = next(iter(D.PatchCache(str(tmp_path), batch_size=16, device="cuda")))
    rng = np.random.Generator(np.random.PCG64(3))
    flags = []
    for _ in range(16):
        h, v = rng.random() < 0.5, rng.random() < 0.5
        flags.append((h, v, int(rng.integers(0, 4)) if rng.random() < 0.5 else 0))
    b = next(iter(pc))
    assert "aug_params" not in b
    for i, (h, v, k) in enumerate(flags):
        for src, got in ((plain["image"][i], b["image"][i]), (plain["mask"][i], b["mask"][i])):
            ref = src
            if h:
                ref = torch.flip(ref, (2,))
            if v:
                ref = torch.flip(ref, (1,))
            assert torch.equal(got, torch.rot90(ref, k, (1, 2))), (i, h, v, k)


# ----------------------------------------------------------------------------
# 9. dispatcher op
# ----------------------------------------------------------------------------
def test_dispatcher_op():
    D = _D()
    H, W, B = 20, 12, 3
    img, msk = _inputs(B, H, W, 2, 8)
    params, gx, gy = _general(H, W, B, 4, 77)
    params[:, 6], params[:, 19] = 0.8, 0.02
    timg = torch.from_numpy(img).permute(0, 3, 1, 2).to(DEV)
    tmsk = torch.from_numpy(msk).permute(0, 3, 1, 2).to(DEV)
    dp, dgx, dgy = (torch.from_numpy(a).to(DEV) for a in (params, gx, gy))
    op = torch.ops.vaeunet.augment_patch
    for reflect in (True, False):
        oi, om = op(timg, tmsk, dp, dgx, dgy, 5, 2, reflect)
        ri, rm = D.augment_patches(timg, tmsk, params, gx, gy, seed=5, offset=2,
                                   border="reflect101" if reflect else "constant")
        assert torch.equal(oi, ri) and torch.equal(om, rm)
    torch.library.opcheck(op, (timg, tmsk, dp, dgx, dgy, 5), {"offset": 2, "reflect": False})
    with pytest.raises((NotImplementedError, RuntimeError)):
        op(timg.cpu(), tmsk.cpu(), dp.cpu(), dgx.cpu(), dgy.cpu(), 5)
