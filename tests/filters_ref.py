"""numpy reference of the device-side CLAHE and separable blur (DESIGN.md §4.9,
include/vaeunet.h: vu_clahe_luts, vu_clahe_apply, vu_blur_sep).

CLAHE is integer up to the lookup tables (the fp32 quantisation and the one
fp32 product of the clip limit are done in np.float32, as the kernel does
them), so the tables are compared bitwise.  The per-pixel blend and the blur
are evaluated in ``dtype``: float64 is the reference, float32 the yardstick
the GPU tests take their bounds from; both work on the same fp32 weights.

Layouts are NHWC numpy arrays: image [B, H, W, 3]."""
import numpy as np

RMAX = 7
F32 = np.float32


# ----------------------------------------------------------------------------
# CLAHE
# ----------------------------------------------------------------------------
def quant8(v):
    """(int)(clamp(v, 0, 1) * 255 + 0.5): product and sum rounded to fp32 one by one; NaN -> 0"""
    v = np.asarray(v, F32)
    v = np.clip(np.where(np.isnan(v), F32(0), v), F32(0), F32(1)).astype(F32)
    return ((v * F32(255.0)).astype(F32) + F32(0.5)).astype(F32).astype(np.int64)


def luma8(img):
    q = quant8(img)
    return (77 * q[..., 0] + 150 * q[..., 1] + 29 * q[..., 2] + 128) >> 8


def tile_start(t, n, T):
    return (t * n) // T


def tile_of(y, n, T):
    return ((y + 1) * T - 1) // n


def clip_limit(clip, A):
    t = F32(F32(clip) * F32(A)) * F32(1.0 / 256.0)
    return int(A) if t >= F32(A) else max(1, int(t))


def clip_hist(h, lim):
    """(redistributed histogram, remainder r) in OpenCV's order"""
    h = np.asarray(h, np.int64)
    E = int(np.maximum(h - lim, 0).sum())
    h = np.minimum(h, lim) + E // 256
    r = E % 256
    if r > 0:
        step = max(256 // r, 1)
        i = np.arange(256)
        h = h + ((i % step == 0) & (i // step < r))
    return h, r


def lut_of(h, A):
    cdf = np.cumsum(np.asarray(h, np.int64))
    return ((cdf * 255 + A // 2) // A).astype(np.uint8)


def clahe_luts(img, clip, TY, TX, stats=None):
    """uint8 [B, TY, TX, 256]; an off sample (clip not > 0) holds the identity
    table.  ``stats``: a dict that collects which branches were met."""
    B, H, W, _ = img.shape
    Y = luma8(img)
    luts = np.empty((B, TY, TX, 256), np.uint8)
    for b in range(B):
        if not clip[b] > 0:
            luts[b] = np.arange(256, dtype=np.uint8)
            continue
        for ty in range(TY):
            y0, y1 = tile_start(ty, H, TY), tile_start(ty + 1, H, TY)
            for tx in range(TX):
                x0, x1 = tile_start(tx, W, TX), tile_start(tx + 1, W, TX)
                A = (y1 - y0) * (x1 - x0)
                h = np.bincount(Y[b, y0:y1, x0:x1].ravel(), minlength=256)
                lim = clip_limit(clip[b], A)
                h2, r = clip_hist(h, lim)
                assert int(h2.sum()) == A
                luts[b, ty, tx] = lut_of(h2, A)
                if stats is not None:
                    for key, hit in (("lim1", lim == 1), ("r0", r == 0), ("step>=2", 0 < r <= 128),
                                     ("step1", r > 128)):
                        stats[key] = stats.get(key, 0) + int(hit)
    return luts


def axis_blend(n, T, dtype=np.float64):
    """(t1, t2, weight of t2) of every pixel of an axis, by a plain search"""
    C = [tile_start(t, n, T) + tile_start(t + 1, n, T) - 1 for t in range(T)]
    t1, t2, w = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, dtype)
    for y in range(n):
        P = 2 * y
        below = [t for t in range(T) if C[t] <= P]
        if not below:
            continue                                   # before the first centre: tile 0, weight 0
        a = below[-1]
        t1[y] = t2[y] = a
        if a < T - 1:
            t2[y] = a + 1
            w[y] = dtype(dtype(P - C[a]) / dtype(C[a + 1] - C[a]))
    return t1, t2, w


def clahe_apply(img, clip, TY, TX, luts, dtype=np.float64):
    """the blend and the output in ``dtype`` on the integer tables; off samples
    come back as they are (the output keeps the dtype of ``dtype`` otherwise)"""
    f = dtype
    B, H, W, _ = img.shape
    Y = luma8(img)
    out = np.empty(img.shape, f)
    y1, y2, wy = axis_blend(H, TY, f)
    x1, x2, wx = axis_blend(W, TX, f)
    wy, wx = wy[:, None], wx[None, :]
    for b in range(B):
        if not clip[b] > 0:
            out[b] = img[b]
            continue
        L = luts[b].astype(f)
        Yb = Y[b]
        l11, l12 = L[y1[:, None], x1[None, :], Yb], L[y1[:, None], x2[None, :], Yb]
        l21, l22 = L[y2[:, None], x1[None, :], Yb], L[y2[:, None], x2[None, :], Yb]
        top = l11 + wx * (l12 - l11)
        bot = l21 + wx * (l22 - l21)
        d = ((top + wy * (bot - top)) - Yb.astype(f)) * f(F32(1.0 / 255.0))
        v = img[b].astype(f) + d[..., None]
        out[b] = np.clip(np.where(np.isnan(v), f(0), v), f(0), f(1))
    return out


def clahe(img, clip, TY, TX, dtype=np.float64):
    clip = np.asarray(clip, F32)
    return clahe_apply(img, clip, TY, TX, clahe_luts(img, clip, TY, TX), dtype)


# ----------------------------------------------------------------------------
# blur
# ----------------------------------------------------------------------------
def fold101(i, size):
    i = np.asarray(i, np.int64)
    if size == 1:
        return np.zeros_like(i)
    per = 2 * (size - 1)
    m = np.mod(i, per)
    return np.where(m < size, m, per - m)


def _pass(x, w, r, axis, dtype):
    n = x.shape[axis]
    idx = np.arange(n)
    acc = w[0] * x
    for k in range(1, r + 1):
        acc = w[k] * (np.take(x, fold101(idx - k, n), axis=axis) + np.take(x, fold101(idx + k, n), axis=axis)) + acc
    return acc.astype(dtype)


def blur(img, table, dtype=np.float64):
    """horizontal then vertical pass per sample in ``dtype``; table [B, 9] fp32 = r, w_0..w_7"""
    out = np.empty(img.shape, dtype)
    for b in range(img.shape[0]):
        t = np.asarray(table[b], F32)
        r = int(min(max(t[0], 0), RMAX)) if not np.isnan(t[0]) else 0
        w = t[1:].astype(dtype)
        x = img[b].astype(dtype)
        out[b] = _pass(_pass(x, w, r, 1, dtype), w, r, 0, dtype)
    return out
