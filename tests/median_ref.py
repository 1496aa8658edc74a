"""numpy reference of the device-side median blur (DESIGN.md §4.10,
include/vaeunet.h: vu_median_blur): per channel, the element of rank
((2r + 1)^2 - 1) / 2 of the (2r + 1) x (2r + 1) window at clamped (replicated)
coordinates, in ascending order of the key of its bits.  The key is a total
order of all float32 bit patterns (the ordinary one on finite values, -0 below
+0, NaNs at the two ends by sign), so the result is one of the window's inputs
bit for bit and the GPU tests compare bitwise.

Layouts are NHWC numpy arrays: image [B, H, W, 3]; radius [B] integers 0..3."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

RMAX = 3


def key(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    return np.where(k >> 31 != 0, k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def median(img, radius):                      # img [B,H,W,3] f32, radius [B] ints 0..3
    out = np.empty_like(img)
    for b in range(img.shape[0]):
        r = int(radius[b])
        if r == 0:
            out[b] = img[b]
            continue
        k = np.pad(key(img[b]), ((r, r), (r, r), (0, 0)), mode="edge")
        w = sliding_window_view(k, (2 * r + 1, 2 * r + 1), axis=(0, 1)).reshape(*img.shape[1:], -1)
        out[b] = unkey(np.sort(w, axis=-1)[..., (2 * r + 1) ** 2 // 2])
    return out


def kernel_radius(t):
    """what the kernel makes of a table value: (int)fminf(fmaxf(t, 0), 3), a NaN gives 0"""
    t = np.float32(t)
    return 0 if np.isnan(t) else int(min(max(t, np.float32(0)), np.float32(RMAX)))
