"""numpy reference of the device-side training augmentation (DESIGN.md §4.8,
vu_augment_patch): the whole definition in float64 on the SAME float32
parameter values the kernel receives, plus the same formulas in float32 (the
yardstick the GPU tests take their bounds from).  Philox4x32-10 and
Box-Muller work on the same 32-bit words as the kernel.

Layouts here are NHWC numpy arrays: image [B, H, W, 3], mask [B, H, W, Cm]."""
import numpy as np

CONSTANT, REFLECT101 = 0, 1
COORD_MAX = float(2 ** 20)
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words -> four such arrays"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = c0 * np.uint64(_M0), c2 * np.uint64(_M1)     # < 2^64: exact
        h0, l0 = p0 >> np.uint64(32), p0 & np.uint64(_MASK)
        h1, l1 = p1 >> np.uint64(32), p1 & np.uint64(_MASK)
        c0, c1, c2, c3 = h1 ^ c1 ^ np.uint64(k0), l1, h0 ^ c3 ^ np.uint64(k1), l0
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def pixel_words(H, W, sample, seed, offset):
    """the four Philox words of every pixel of one sample: uint64 [4, H, W]"""
    pix = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    full = np.full((H, W), 0, dtype=np.uint64)
    return np.stack(philox4x32_10(pix & np.uint64(_MASK), pix >> np.uint64(32), full + np.uint64(sample),
                                  full + np.uint64(offset), seed & _MASK, (seed >> 32) & _MASK))


def normals(words, dtype=np.float64):
    """Box-Muller: three normals [H, W, 3] from the four words, evaluated in
    ``dtype`` (float64: the reference; float32: the kernel's formula)"""
    f = dtype
    w = [words[k].astype(f) for k in range(4)]          # float32: rounds like the device's conversion
    two32 = f(2.0 ** -32)
    r0 = np.sqrt(f(-2.0) * np.log((w[0] + f(1.0)) * two32))
    r1 = np.sqrt(f(-2.0) * np.log((w[2] + f(1.0)) * two32))
    a0 = f(6.283185307179586) * (w[1] * two32)
    a1 = f(6.283185307179586) * (w[3] * two32)
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1)], axis=-1).astype(f)


def knot_map(knots, size):
    """g(0..size-1) in float64: piecewise-linear through the S + 1 knots over S
    equal cells of [0, size - 1]"""
    k = np.asarray(knots, dtype=np.float64)
    S = len(k) - 1
    d = max(size - 1, 1)
    j = np.arange(size)
    c = np.minimum((j * S) // d, S - 1)
    r = j * S - c * d
    return k[c] + r * ((k[c + 1] - k[c]) / d)


def source_coords(p, gx, gy, H, W):
    """(sx, sy) float64 [H, W] of one sample from its fp32 parameters"""
    p = np.asarray(p, dtype=np.float64)
    u, v = knot_map(gx, W)[None, :], knot_map(gy, H)[:, None]
    sx = p[0] * u + p[1] * v + p[2]
    sy = p[3] * u + p[4] * v + p[5]
    return np.clip(sx, -COORD_MAX, COORD_MAX), np.clip(sy, -COORD_MAX, COORD_MAX)


def _fold(i, size, border):
    """(index, valid) of integer taps under the border mode"""
    if border == REFLECT101:
        if size == 1:
            return np.zeros_like(i), np.ones(i.shape, bool)
        per = 2 * (size - 1)
        m = np.mod(i, per)
        return np.where(m < size, m, per - m), np.ones(i.shape, bool)
    ok = (i >= 0) & (i < size)
    return np.where(ok, i, 0), ok


def warp_image(img, sx, sy, border):
    """bilinear taps of img [H, W, C] (float64) at (sx, sy)"""
    H, W, _ = img.shape
    fx, fy = np.floor(sx), np.floor(sy)
    tx, ty = (sx - fx)[..., None], (sy - fy)[..., None]
    x0, kx0 = _fold(fx.astype(np.int64), W, border)
    x1, kx1 = _fold(fx.astype(np.int64) + 1, W, border)
    y0, ky0 = _fold(fy.astype(np.int64), H, border)
    y1, ky1 = _fold(fy.astype(np.int64) + 1, H, border)

    def at(y, x, ok):
        return img[y, x] * ok[..., None]
    top = at(y0, x0, ky0 & kx0) + tx * (at(y0, x1, ky0 & kx1) - at(y0, x0, ky0 & kx0))
    bot = at(y1, x0, ky1 & kx0) + tx * (at(y1, x1, ky1 & kx1) - at(y1, x0, ky1 & kx0))
    return top + ty * (bot - top)


def warp_mask(msk, sx, sy, border):
    H, W, _ = msk.shape
    x, kx = _fold(np.floor(sx + 0.5).astype(np.int64), W, border)
    y, ky = _fold(np.floor(sy + 0.5).astype(np.int64), H, border)
    return msk[y, x] * (kx & ky)[..., None]


def photometry(v, p, noise=None, dtype=np.float64):
    """gamma -> colour matrix -> noise -> clip on v [H, W, 3], evaluated in
    ``dtype``; noise: the normals [H, W, 3] (or None)"""
    f = dtype
    p = np.asarray(p, dtype=np.float32).astype(f)
    v = v.astype(f)
    if p[6] != 1:
        v = np.power(np.maximum(v, f(0)), p[6])
    M, o = p[7:16].reshape(3, 3), p[16:19]
    v = np.stack([o[c] + M[c, 0] * v[..., 0] + M[c, 1] * v[..., 1] + M[c, 2] * v[..., 2] for c in range(3)], axis=-1)
    if p[19] != 0 and noise is not None:
        v = v + p[19] * noise.astype(f)
    return np.clip(v, f(0), f(1)).astype(f)


def augment(img, msk, params, gx, gy, seed, offset=0, border=REFLECT101):
    """The whole definition in float64: img [B, H, W, 3], msk [B, H, W, Cm]
    (any float dtype) -> (image, mask) float64."""
    B, H, W, _ = img.shape
    oi, om = np.empty(img.shape, np.float64), np.empty(msk.shape, np.float64)
    for b in range(B):
        sx, sy = source_coords(params[b], gx[b], gy[b], H, W)
        n = normals(pixel_words(H, W, b, seed, offset)) if params[b][19] != 0 else None
        oi[b] = photometry(warp_image(img[b].astype(np.float64), sx, sy, border), params[b], n)
        om[b] = warp_mask(msk[b].astype(np.float64), sx, sy, border)
    return oi, om
