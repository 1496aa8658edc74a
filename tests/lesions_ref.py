"""numpy restatement of the lesion-level evaluation (DESIGN.md §4.11,
include/vaeunet.h): canonical connected-component labels by a plain stack-based
flood fill, areas, scores, any-overlap matching, counts, FROC histograms and the
curve.  fp32 for the bin index, fp64 for the curve.  Test infrastructure only."""
import numpy as np

FROC_TARGETS = (0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0)


def foreground(x, threshold=None):
    """bool array: nonzero for integer / bool input, x > threshold (strict; NaN is background) for float32"""
    x = np.asarray(x)
    if x.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            return x > np.float32(threshold)
    return x != 0


def label_plane(fg, connectivity=8):
    """[H, W] bool -> int32 labels: 0 background, else 1 + the smallest row-major index of the component"""
    H, W = fg.shape
    lab = np.zeros((H, W), np.int32)
    flat = fg.reshape(-1)
    out = lab.reshape(-1)
    if connectivity == 8:
        nbrs = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
    else:
        nbrs = [(-1, 0), (0, -1), (0, 1), (1, 0)]
    for s in np.flatnonzero(flat):          # raster order: an unlabelled s is its component's smallest index
        if out[s]:
            continue
        out[s] = s + 1
        stack = [int(s)]
        while stack:
            i = stack.pop()
            y, x = divmod(i, W)
            for dy, dx in nbrs:
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W:
                    j = yy * W + xx
                    if flat[j] and not out[j]:
                        out[j] = s + 1
                        stack.append(j)
    return lab


def label(x, connectivity=8, threshold=None):
    """[B, C, H, W] -> (int32 labels [B, C, H, W], int64 component counts [B, C])"""
    fg = foreground(x, threshold)
    B, C = fg.shape[:2]
    lab = np.zeros(fg.shape, np.int32)
    n = np.zeros((B, C), np.int64)
    for b in range(B):
        for c in range(C):
            lab[b, c] = label_plane(fg[b, c], connectivity)
            n[b, c] = len(np.unique(lab[b, c][lab[b, c] > 0]))
    return lab, n


def areas_plane(lab):
    """int32 image: the component's pixel count at every foreground pixel"""
    cnt = np.bincount(lab.reshape(-1), minlength=lab.size + 1)
    out = cnt[lab].astype(np.int32)
    out[lab == 0] = 0
    return out


def areas(lab):
    return np.stack([np.stack([areas_plane(p) for p in img]) for img in lab])


def remove_small(x, min_area, connectivity=8, threshold=None):
    lab, _ = label(x, connectivity, threshold)
    return ((lab > 0) & (areas(lab) >= min_area)).astype(np.uint8)


def score_bin(score, nb):
    t = np.float32(score) * np.float32(nb)                  # fp32 product
    return nb - 1 if t >= np.float32(nb) else int(t)


def match_plane(pred, gt_fg, threshold, min_area, connectivity, nb):
    """one plane -> ((n_gt, n_gt_detected, n_pred kept, n_pred_fp), hist_fp [nb], hist_gt [nb])"""
    pl = label_plane(foreground(pred, threshold), connectivity)
    gl = label_plane(gt_fg, connectivity)
    hist_fp, hist_gt = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    scores, n_pred, n_fp = {}, 0, 0
    for r in np.unique(pl[pl > 0]):
        comp = pl == r
        if comp.sum() < min_area:
            continue
        if pred.dtype == np.float32:
            s = np.float32(max(np.float32(0), pred[comp].max()))
        else:
            s = np.float32(1)
        scores[int(r)] = s
        n_pred += 1
        if not gt_fg[comp].any():
            n_fp += 1
            hist_fp[score_bin(s, nb)] += 1
    n_gt, n_det = 0, 0
    for r in np.unique(gl[gl > 0]):
        n_gt += 1
        over = [scores[int(q)] for q in np.unique(pl[(gl == r) & (pl > 0)]) if int(q) in scores]
        if over:
            n_det += 1
            hist_gt[score_bin(max(over), nb)] += 1
    return (n_gt, n_det, n_pred, n_fp), hist_fp, hist_gt


def gt_foreground(masks):
    """ground truth: nonzero for integer / bool masks, > 0.5 for float32 masks"""
    return foreground(masks, 0.5)


def match(pred, masks, threshold=0.5, min_area=1, connectivity=8, nb=1000):
    """[B, C, H, W] pair -> (int64 counts [B, C, 4], hist_fp [nb], hist_gt [nb])"""
    pred = np.asarray(pred)
    if pred.dtype == np.bool_:
        pred = pred.astype(np.uint8)
    g = gt_foreground(masks)
    B, C = pred.shape[:2]
    counts = np.zeros((B, C, 4), np.int64)
    hist_fp, hist_gt = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    for b in range(B):
        for c in range(C):
            k, hf, hg = match_plane(pred[b, c], g[b, c], threshold, min_area, connectivity, nb)
            counts[b, c] = k
            hist_fp += hf
            hist_gt += hg
    return counts, hist_fp, hist_gt


def froc(hist_fp, hist_gt, n_gt, n_planes):
    """-> (sens [nb] fp64, fppi [nb] fp64, score fp64); NaN sensitivities when n_gt == 0"""
    cf = np.cumsum(hist_fp[::-1])[::-1].astype(np.float64)
    cg = np.cumsum(hist_gt[::-1])[::-1].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        sens = cg / np.float64(n_gt)
    fppi = cf / np.float64(n_planes)
    total = np.float64(0)
    for t in FROC_TARGETS:
        ok = np.flatnonzero(fppi <= t)
        if len(ok) == 0:
            term = np.float64(0)
        elif n_gt == 0:
            term = np.float64(np.nan)
        else:
            term = sens[ok].max()                           # the largest sensitivity within the target
        total = total + term
    return sens, fppi, total / np.float64(7)


# ---- the test planes -------------------------------------------------------------
BERNOULLI_P = (0.5927, 0.4073, 0.5, 0.0085)   # site percolation at connectivity 4 / 8 (two), the measured lesion rate


def bernoulli_planes(H, W):
    """{p: uint8 [H, W]} from numpy.random.PCG64(7), drawn in the order of BERNOULLI_P"""
    rng = np.random.Generator(np.random.PCG64(7))
    return {p: (rng.random((H, W)) < p).astype(np.uint8) for p in BERNOULLI_P}


def adversarial_planes(H, W):
    """{name: uint8 [H, W]}: the planes on which a tiled union-find can go wrong"""
    z = lambda: np.zeros((H, W), np.uint8)   # noqa: E731
    out = {"background": z(), "foreground": np.ones((H, W), np.uint8)}
    yy, xx = np.mgrid[:H, :W]
    out["checkerboard"] = ((yy + xx) & 1).astype(np.uint8)
    s = z()                                   # width-1 serpentine: one component, maximal chain depth
    s[::2] = 1
    for y in range(1, H, 2):
        s[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    out["serpentine"] = s
    u = z()                                   # the arms join only in the last row
    u[:, 0] = u[:, W - 1] = u[H - 1] = 1
    out["U"] = u
    c, k = z(), 0                             # nested U's, two columns / rows apart: separate at either connectivity
    while 4 * k + 2 < W and 2 * k < H:
        l, r, b = 2 * k, W - 1 - 2 * k, H - 1 - 2 * k
        c[:b + 1, l] = c[:b + 1, r] = 1
        c[b, l:r + 1] = 1
        k += 1
    out["comb"] = c
    d, a = z(), z()                           # through tile corners: connected only by the corner neighbour
    i = np.arange(min(H, W))
    d[i, i] = 1
    a[i, W - 1 - i] = 1
    out["diagonal"], out["antidiagonal"] = d, a
    for p, v in bernoulli_planes(H, W).items():
        out[f"bernoulli{p}"] = v
    return out


def metrics(counts, n_planes=None, eps=1e-6):
    """pooled (sensitivity, precision, false positives per plane) as float32"""
    t = np.asarray(counts).reshape(-1, 4).sum(0).astype(np.float64)
    n_planes = np.asarray(counts).reshape(-1, 4).shape[0] if n_planes is None else n_planes
    return np.array([(t[1] + eps) / (t[0] + eps), (t[2] - t[3] + eps) / (t[2] + eps), t[3] / n_planes], np.float32)
