"""numpy restatement of the sample-set metrics (DESIGN.md §4.14,
include/vaeunet.h): the foreground rules, the Gram matrix as an int64 B^T B and
the nine metrics with every sum in fp64 in row-major order (i outer, j inner).
Also the adversarial sample stacks of the tests and their float32 encodings.
Test infrastructure only."""
import numpy as np

NAMES = ("ged2", "cross", "diversity", "truth_diversity", "dice_mean", "dice_min", "dice_max", "area_mean", "area_std")
NAN_WITHOUT_TRUTH = (0, 1, 3, 4, 5, 6)
KINDS = ("background", "foreground", "identical", "disjoint", "nested", "one_empty", "truth_empty", "all_empty",
         "bernoulli0.5", "bernoulli0.0015")


def foreground(x, threshold=None):
    """bool array: nonzero for integer / bool input, x > threshold (strict; NaN is background) for float32"""
    x = np.asarray(x)
    if x.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            return x > np.float32(threshold)
    return x != 0


def gram(samples, truths=None, threshold=0.5):
    """samples [S, B, C, H, W], truths None or [M, B, C, H, W] -> int64 [B, C, K, K] = B^T B of the 0 / 1 columns"""
    cols = foreground(samples, threshold)
    if truths is not None and truths.shape[0]:
        cols = np.concatenate([cols, foreground(truths, 0.5)])
    K, B, C = cols.shape[:3]
    bits = cols.reshape(K, B, C, -1).astype(np.int64)
    out = np.empty((B, C, K, K), np.int64)
    for b in range(B):
        for c in range(C):
            out[b, c] = bits[:, b, c] @ bits[:, b, c].T
    return out


def dist(I, na, nb):
    U = int(na) + int(nb) - int(I)
    return np.float64(0.0) if U == 0 else np.float64(1.0) - np.float64(int(I)) / np.float64(U)


def dice(I, na, nb):
    s = int(na) + int(nb)
    return np.float64(1.0) if s == 0 else np.float64(2 * int(I)) / np.float64(s)


def _sum(terms):
    """the fp64 sum of an array in row-major order, one term after another from 0.0 (np.add.accumulate is the
    plain sequential loop; np.sum would add pairwise)"""
    t = np.asarray(terms, np.float64).reshape(-1)
    return np.float64(0.0) if t.size == 0 else np.add.accumulate(np.concatenate([[0.0], t]))[-1]


def metrics_plane(G, S):
    """G int64 [K, K] -> fp64 [9]; the terms are formed elementwise (each one IEEE operation on the same integers
    as dist / dice above), the sums by _sum"""
    K = G.shape[0]
    M = K - S
    G = G.astype(np.int64)
    area = np.diagonal(G)
    tot = area[:, None] + area[None, :]
    U = tot - G
    with np.errstate(invalid="ignore", divide="ignore"):
        D = np.where(U == 0, np.float64(0.0), np.float64(1.0) - G.astype(np.float64) / U.astype(np.float64))
        Dc = np.where(tot == 0, np.float64(1.0), (2 * G).astype(np.float64) / tot.astype(np.float64))
    out = np.full(9, np.nan, np.float64)
    out[2] = _sum(D[:S, :S]) / (np.float64(S) * np.float64(S))
    mean = _sum(area[:S]) / np.float64(S)
    out[7] = mean
    out[8] = np.sqrt(_sum((area[:S].astype(np.float64) - mean) ** 2) / np.float64(S))
    if M == 0:
        return out
    sm = np.float64(S) * np.float64(M)
    out[1] = _sum(D[:S, S:]) / sm
    out[3] = _sum(D[S:, S:]) / (np.float64(M) * np.float64(M))
    out[0] = np.float64(2.0) * out[1] - out[2] - out[3]
    out[4] = _sum(Dc[:S, S:]) / sm
    out[5], out[6] = Dc[:S, S:].min(), Dc[:S, S:].max()
    return out


def metrics(G, S):
    """int64 [B, C, K, K] -> fp64 [B, C, 9]"""
    return np.stack([np.stack([metrics_plane(g, S) for g in img]) for img in G])


# ----------------------------------------------------------------------------
# adversarial stacks
# ----------------------------------------------------------------------------
def stack(kind, S, M, planes, H, W, seed=0):
    """-> (samples uint8 [S, planes, H, W], truths uint8 [M, planes, H, W]) of 0 / 1"""
    n = H * W
    rng = np.random.Generator(np.random.PCG64([KINDS.index(kind), S, M, planes, H, W, seed]))
    s = np.zeros((S, planes, n), np.uint8)
    t = np.zeros((M, planes, n), np.uint8)
    base = (rng.random((planes, n)) < 0.3).astype(np.uint8)
    if kind == "background" or kind == "all_empty":
        pass
    elif kind == "foreground":
        s[:], t[:] = 1, 1
    elif kind == "identical":
        s[:], t[:] = base, base
    elif kind == "disjoint":          # pixel e belongs to column e % (K + 1); the last class is nobody's
        owner = np.arange(n) % (S + M + 1)
        for k in range(S):
            s[k, :, owner == k] = 1
        for m in range(M):
            t[m, :, owner == S + m] = 1
    elif kind == "nested":            # column k holds the first ceil(n (k + 1) / K) pixels
        K = S + M
        for k in range(K):
            (s[k] if k < S else t[k - S])[:, :-(-n * (k + 1) // K)] = 1
    elif kind == "one_empty":
        s[:], t[:] = base, base
        s[S // 2] = 0
    elif kind == "truth_empty":
        s[:] = base
        s[0, :, 0] = 1                 # never empty, also at 1 x 1
    else:
        p = float(kind[len("bernoulli"):])
        s = (rng.random(s.shape) < p).astype(np.uint8)
        t = (rng.random(t.shape) < p).astype(np.uint8)
    return s.reshape(S, planes, H, W), t.reshape(M, planes, H, W)


def as_prob(fg, threshold, seed):
    """a float32 map whose foreground at ``threshold`` (in (0, 1)) is fg: foreground in (threshold, 1] with
    nextafter(threshold) and 1.0 among it, background in [0, threshold] with the exact threshold and NaN among it"""
    thr = np.float32(threshold)
    rng = np.random.Generator(np.random.PCG64(seed))
    u = rng.random(fg.shape, dtype=np.float32)
    lo = np.nextafter(thr, np.float32(1))
    p = np.where(fg != 0, lo + u * (np.float32(1) - lo), u * thr).astype(np.float32)
    pick = rng.random(fg.shape)
    p[(fg == 0) & (pick < 0.1)] = thr
    p[(fg == 0) & (pick > 0.9)] = np.nan
    p[(fg != 0) & (pick < 0.05)] = lo
    p[(fg != 0) & (pick > 0.95)] = 1.0
    assert np.array_equal(foreground(p, thr), fg != 0)
    return p
