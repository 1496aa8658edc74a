"""numpy restatement of the boundary metrics (DESIGN.md §4.12,
include/vaeunet.h): the exact squared Euclidean distance transform as a column
pass and a per-row minimum over ALL x' (no pruning), the boundary, the surface
statistics with the nearest-rank percentile, and the metrics in fp64.  Test
infrastructure only."""
import math

import numpy as np

from lesions_ref import foreground

INF = 2 ** 31 - 1
MODES = ("foreground", "background", "boundary")
BERNOULLI_P = (0.5, 0.0085)


def boundary_plane(fg):
    """[H, W] bool -> bool: foreground with a 4-neighbour that is background or outside the plane"""
    p = np.pad(fg, 1)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return fg & ~inner


def sites_plane(fg, mode):
    return {"foreground": fg, "background": ~fg, "boundary": boundary_plane(fg)}[mode]


def edt2_sites(sites):
    """[H, W] bool sites -> int32 squared distance to the nearest site, INF everywhere without one"""
    H, W = sites.shape
    if not sites.any():
        return np.full((H, W), INF, np.int32)
    big = 1 << 40
    ys = np.arange(H, dtype=np.int64)
    g2 = np.full((H, W), big, np.int64)
    for x in range(W):                                   # column pass: the nearest site row of every column
        rows = np.flatnonzero(sites[:, x])
        if len(rows):
            g2[:, x] = ((ys[:, None] - rows[None, :]) ** 2).min(1)
    xs = np.arange(W, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2               # [x, x']
    out = np.empty((H, W), np.int64)
    for y in range(H):                                   # row pass: all x'
        out[y] = (g2[y][None, :] + dx2).min(1)
    assert out.max() < 2 ** 29
    return out.astype(np.int32)


def edt2_plane(fg, mode):
    return edt2_sites(sites_plane(fg, mode))


def edt2(x, mode="background", threshold=None):
    """[B, C, H, W] -> int32 [B, C, H, W]"""
    fg = foreground(x, threshold)
    return np.stack([np.stack([edt2_plane(p, mode) for p in img]) for img in fg])


def boundary(x, threshold=None):
    fg = foreground(x, threshold)
    return np.stack([np.stack([boundary_plane(p) for p in img]) for img in fg]).astype(np.uint8)


def brute_edt2(sites):
    """all site pairs: O((HW)^2), for small planes"""
    H, W = sites.shape
    if not sites.any():
        return np.full((H, W), INF, np.int32)
    sy, sx = np.nonzero(sites)
    yy, xx = np.mgrid[:H, :W]
    d = (yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2
    return d.min(-1).astype(np.int32)


def rank(q, n):
    return (q * n + 99) // 100


def percentile(values, q):
    """nearest rank in integers: the value of rank (q n + 99) // 100, 1-based, ascending"""
    v = np.sort(np.asarray(values))
    return int(v[rank(q, len(v)) - 1])


def stats_plane(pf, gf, q, tol2):
    """two [H, W] bool foregrounds -> (int64 [8], float64 [2])"""
    P, G = boundary_plane(pf), boundary_plane(gf)
    st = np.full(8, -1, np.int64)
    st[0], st[1] = P.sum(), G.sum()
    sm = np.zeros(2, np.float64)
    if st[0] == 0 or st[1] == 0:
        return st, sm
    for s, (a, b) in enumerate(((P, G), (G, P))):
        d2 = edt2_sites(b)[a].astype(np.int64)           # row-major order of the set
        st[2 + s] = d2.max()
        st[4 + s] = percentile(d2, q)
        st[6 + s] = (d2 <= tol2).sum()
        sm[s] = math.fsum(np.sqrt(d2.astype(np.float64)).tolist())     # the correctly rounded sum of the fp64 roots
    return st, sm


def tol2_of(tolerance):
    return int(float(tolerance) * float(tolerance))


def stats(pred, gt, threshold=0.5, q=95, tolerance=1.0):
    """[B, C, H, W] pair -> (int64 [B, C, 8], float64 [B, C, 2])"""
    pf = foreground(pred, threshold)
    g = np.asarray(gt)
    gf = foreground(g if g.dtype in (np.uint8, np.bool_, np.float32) else g.astype(np.float32), 0.5)
    B, C = pf.shape[:2]
    st, sm = np.zeros((B, C, 8), np.int64), np.zeros((B, C, 2), np.float64)
    for b in range(B):
        for c in range(C):
            st[b, c], sm[b, c] = stats_plane(pf[b, c], gf[b, c], q, tol2_of(tolerance))
    return st, sm


def metrics(st, sm):
    """[..., 8], [..., 2] -> float64 [..., 4] = hd, hd_q, assd, nsd; NaN on an undefined plane"""
    st, sm = np.asarray(st, np.int64), np.asarray(sm, np.float64)
    out = np.full(st.shape[:-1] + (4,), np.nan)
    ok = (st[..., 0] > 0) & (st[..., 1] > 0)
    s = st[ok].astype(np.float64)
    n = s[:, 0] + s[:, 1]
    out[ok] = np.stack([np.sqrt(np.maximum(s[:, 2], s[:, 3])), np.maximum(np.sqrt(s[:, 4]), np.sqrt(s[:, 5])),
                        (sm[ok][:, 0] + sm[ok][:, 1]) / n, (s[:, 6] + s[:, 7]) / n], -1)
    return out


def pooled(per_plane):
    """[N, 4] in plane order -> (float64 [4] mean over the defined planes, their number); NaN when there is none"""
    acc, k = np.zeros(4), 0
    for row in np.asarray(per_plane, np.float64).reshape(-1, 4):
        if not np.isnan(row[0]):
            acc = acc + row
            k += 1
    with np.errstate(invalid="ignore"):
        return acc / np.float64(k), k


def adversarial_planes(H, W, seed=0):
    """name -> uint8 [H, W]"""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * H + W))
    z = lambda: np.zeros((H, W), np.uint8)   # noqa: E731
    out = {"none": z(), "all": np.ones((H, W), np.uint8)}
    for name, (y, x) in (("corner00", (0, 0)), ("corner01", (0, W - 1)), ("corner10", (H - 1, 0)),
                         ("corner11", (H - 1, W - 1))):
        out[name] = z()
        out[name][y, x] = 1
    out["last_column"] = z()
    out["last_column"][:, W - 1] = 1
    out["last_row"] = z()
    out["last_row"][H - 1, :] = 1
    out["full_row"] = z()
    out["full_row"][H // 2, :] = 1
    out["full_column"] = z()
    out["full_column"][:, W // 2] = 1
    yy, xx = np.mgrid[:H, :W]
    out["checkerboard"] = ((yy + xx) & 1).astype(np.uint8)
    out["equidistant"] = z()                 # two sites at equal distance from the pixels between them
    out["equidistant"][H // 2, W // 4] = 1
    out["equidistant"][H // 2, W // 4 + 2 * ((W - 1 - W // 4) // 2)] = 1
    for p in BERNOULLI_P:
        out[f"bernoulli{p}"] = (rng.random((H, W)) < p).astype(np.uint8)
    return out


def disc(H, W, cy, cx, r):
    yy, xx = np.mgrid[:H, :W]
    return (((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r).astype(np.uint8)


def pair_planes(H, W):
    """name -> (pred uint8 [H, W], gt uint8 [H, W]) for the pair statistics"""
    out = {}
    r = max(1, min(H, W) // 4)
    out["shifted_disc"] = (disc(H, W, H // 2, W // 2, r), disc(H, W, H // 2 + max(1, r // 3), W // 2 + max(1, r // 2), r))
    a, b = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    a[H // 8:H - H // 8, W // 8:W - W // 8] = 1
    b[H // 3:H - H // 3, W // 3:W - W // 3] = 1
    out["nested_squares"] = (a, b)
    out["identical"] = (out["shifted_disc"][0], out["shifted_disc"][0].copy())
    out["empty_pred"] = (np.zeros((H, W), np.uint8), a)
    out["empty_gt"] = (a, np.zeros((H, W), np.uint8))
    e, f = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    e[:H // 2 + 1, :W // 2 + 1] = 1          # foreground that touches the plane's edge
    f[H // 3:, W // 3:] = 1
    out["touching_edge"] = (e, f)
    rng = np.random.Generator(np.random.PCG64(7 * H + W))
    out["bernoulli"] = ((rng.random((H, W)) < 0.3).astype(np.uint8), (rng.random((H, W)) < 0.02).astype(np.uint8))
    return out
