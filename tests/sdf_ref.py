"""numpy / torch restatement of the signed distance map and the boundary loss
(include/vaeunet.h): s2 from edt_ref's squared transforms, phi
in fp64 rounded once to fp32, the clip; the loss, its gradient and the gradient
with every factor replaced by its absolute value, in a chosen dtype.  Test
infrastructure only."""
import numpy as np
import torch

import edt_ref as ER
from lesions_ref import foreground


def s2_plane(fg):
    """[H, W] bool -> int32: + d^2 to the nearest foreground pixel outside, - d^2 to the nearest background pixel
    inside, 0 everywhere on a plane with one class only"""
    fg = np.asarray(fg, bool)
    if fg.all() or not fg.any():
        return np.zeros(fg.shape, np.int32)
    to_fg = ER.edt2_plane(fg, "foreground").astype(np.int64)
    to_bg = ER.edt2_plane(fg, "background").astype(np.int64)
    return np.where(fg, -to_bg, to_fg).astype(np.int32)


def brute_s2_plane(fg):
    """the same from all site pairs, for small planes"""
    fg = np.asarray(fg, bool)
    if fg.all() or not fg.any():
        return np.zeros(fg.shape, np.int32)
    to_fg = ER.brute_edt2(fg).astype(np.int64)
    to_bg = ER.brute_edt2(~fg).astype(np.int64)
    return np.where(fg, -to_bg, to_fg).astype(np.int32)


def s2(x, threshold=None):
    """[B, C, H, W] -> int32 [B, C, H, W]"""
    fg = foreground(x, threshold)
    return np.stack([np.stack([s2_plane(p) for p in img]) for img in fg])


def phi_of(s2v, clip=None):
    """int32 s2 -> float32 phi: the fp64 value rounded once, then clamped to [-clip, clip] in fp32"""
    s = np.asarray(s2v).astype(np.float64)
    v = np.where(s > 0, np.sqrt(np.abs(s)), np.where(s < 0, 1.0 - np.sqrt(np.abs(s)), 0.0))
    phi = v.astype(np.float32)
    if clip is not None:
        c = np.float32(clip)
        phi = np.minimum(np.maximum(phi, -c), c)
    return phi


def phi(x, threshold=None, clip=None):
    return phi_of(s2(x, threshold), clip)


def boundary_loss_ref(x, f, gout=1.0, dtype=torch.float64):
    """logits x and map f, any shape, taken in memory order of the flattened
    tensors -> dict(loss, sums [3], grad, sabs).  An element with a NaN logit or
    a non-finite f adds nothing, gets gradient 0 and still counts in n.  sabs:
    the gradient with |f| for f (it is a product, so sabs = |grad|)."""
    x, f = x.detach().cpu().to(dtype).flatten(), f.detach().cpu().to(dtype).flatten()
    skip = torch.isnan(x) | ~torch.isfinite(f)
    zero = torch.zeros((), dtype=dtype)
    xs, fs = torch.where(skip, zero, x), torch.where(skip, zero, f)
    e = torch.exp(-xs.abs())
    hi, lo = 1 / (1 + e), e / (1 + e)
    p = torch.where(xs >= 0, hi, lo)
    dp = lo * hi
    n = x.numel()
    term = fs * p
    S, A = term.sum(), term.abs().sum()
    k = torch.tensor(gout, dtype=torch.float64).div(n).to(dtype)
    grad = k * fs * dp
    sabs = k.abs() * fs.abs() * dp
    return dict(loss=S / n, sums=torch.stack([S, A, skip.sum().to(dtype)]), grad=grad, sabs=sabs)
