"""fp64 reference, inputs, checks and case lists of the weight-gradient GEMM
family: vu_gemm_wgrad (gemm_wgrad.hip v1, gemm_wgrad2.hip v2, gemm_wgrad3.hip
v3) and vu_slab_reduce.  Shared by tests/test_gpu_wgrad_kernels.py (the
kernels) and tests/test_wgrad_ref.py (CPU self-checks of everything here).

The contraction is evaluated from the two VuGather descriptors exactly as
include/vaeunet.h defines them (gemm_audit._Im2col), on whatever device the
descriptors' tensors live:

    ref[i][j]  = sum_m P[m][i] Q[m][j]        sabs[i][j] = sum_m |P[m][i]| |Q[m][j]|

The bound for random operands.  A bf16 x bf16 product is exact in fp32, so a
kernel's only error is fp32 accumulation, in whatever order and with whatever
split: M - 1 additions, |dW - ref| <= (M - 1) 2^-24 sabs.  With accumulate
one more term and one more rounding: M 2^-24 (sabs + |old|).  fp32 operands
may round each product once on its own: (2M - 1) 2^-24 sabs (2M with
accumulate).  No fitted constant.

Impulse operands.  With P[m_i][i] = +-2^k for one pixel per channel i (or one
(pixel, channel) of the gathered source non-zero per channel) and random
storage-dtype values on the other side, every sum has at most one non-zero,
exactly representable term: the fp64 reference is a float32, and any correct
kernel must return it bit for bit in any summation order and with any split.
"""
import functools
from dataclasses import dataclass

import torch
import torch.nn.functional as F

import ref_small as R
from gemm_audit import _Im2col, _bits

U32 = 2.0 ** -24
F32, BF16 = 0, 1
TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16}

# kernel size, stride, padding of the conv kinds; convT: the 2x2 / stride-2
# sub-pixel gather of the output gradient canvas (K.gather_convT)
_KSP = {"3x3": (3, 1, 1), "1x1": (1, 1, 0), "1x1s2": (1, 2, 0), "3x3s2": (3, 2, 1), "stem": (7, 2, 3),
        "convT": (2, 2, 0)}


# ----------------------------------------------------------------------------
# geometry
# ----------------------------------------------------------------------------
@dataclass(frozen=True)
class Geo:
    """One weight-gradient problem.  (N, H, W) is the row grid (the pixels m
    of the reduction: the conv's output, or the ConvT's input); ``cins`` the
    channel sources of Q, ``ni`` the channels of P.
      stride-2 kinds: the source image is (2H - odd[0], 2W - odd[1]);
      stem: 8 packed channels of which 3 are valid (cvalid);
      convT: the canvas is (2H + extra[0], 2W + extra[1]), read at pyx."""
    kind: str
    N: int
    H: int
    W: int
    cins: tuple
    ni: int
    odd: tuple = (0, 0)
    pyx: tuple = (0, 0)
    extra: tuple = (0, 0)

    @property
    def M(self):
        return self.N * self.H * self.W

    @property
    def C(self):
        return sum(self.cins)

    @property
    def ksp(self):
        return _KSP[self.kind]

    @property
    def taps(self):
        return self.ksp[0] ** 2

    @property
    def nj(self):
        return self.taps * self.C

    @property
    def cvalid(self):
        return 3 if self.kind == "stem" else self.C

    @property
    def src_hw(self):
        k, s, p = self.ksp
        if self.kind == "convT":
            return 2 * self.H + self.extra[0], 2 * self.W + self.extra[1]
        if s == 1:
            return self.H, self.W
        hs, ws = 2 * self.H - self.odd[0], 2 * self.W - self.odd[1]
        assert (hs + 2 * p - k) // s + 1 == self.H and (ws + 2 * p - k) // s + 1 == self.W
        return hs, ws

    @property
    def qkw(self):
        """K.gather keywords of Q"""
        k, s, p = self.ksp
        if self.kind == "convT":
            return dict(R=2, S=2, sy=2, sx=2, oy=self.pyx[0], ox=self.pyx[1])
        return dict(R=k, S=k, sy=s, sx=s, oy=-p, ox=-p)

    @property
    def grad_shape(self):
        """[Cout, Cin, k, k], or the ConvT's [Cin, Cout, 2, 2]"""
        k = self.ksp[0]
        return (self.ni, self.cvalid, k, k)

    def __str__(self):
        s = f"{self.kind} {self.N}x{self.H}x{self.W} src {'x'.join(map(str, self.src_hw))} C{list(self.cins)} ni{self.ni}"
        return s + (f" pyx{self.pyx}" if self.kind == "convT" else "")


def _storage(t, dtype):
    return t.to(TORCH_DTYPE[dtype]).float()


@functools.lru_cache(maxsize=None)
def operands(geo, dtype, seed=0):
    """Random CPU operands rounded to the storage dtype (held as float32):
    P [N, ni, H, W] and the sources of Q, [N, c, Hs, Ws] each.  The stem's
    channels >= cvalid hold non-zero values (cvalid must drop them)."""
    g = torch.Generator().manual_seed(7919 * seed + 131 * geo.M + 17 * geo.ni + geo.C + len(geo.kind))
    hs, ws = geo.src_hw
    P = _storage(torch.randn(geo.N, geo.ni, geo.H, geo.W, generator=g), dtype)
    Q = tuple(_storage(torch.randn(geo.N, c, hs, ws, generator=g), dtype) for c in geo.cins)
    return P, Q


def autograd_grad(geo, P, Q):
    """The gradient torch derives for the layer, fp64, in ``geo.grad_shape``
    (channels >= cvalid left out): conv2d_weight, or autograd through
    F.conv_transpose2d placed at pyx in the canvas."""
    k, s, p = geo.ksp
    x = torch.cat([q.double() for q in Q], 1)
    if geo.kind == "convT":
        w = torch.zeros(geo.ni, geo.C, 2, 2, dtype=torch.float64, requires_grad=True)
        up = F.conv_transpose2d(P.double(), w, stride=2)
        py, px = geo.pyx
        (up * x[:, :, py:py + 2 * geo.H, px:px + 2 * geo.W]).sum().backward()
        return w.grad
    gw = torch.nn.grad.conv2d_weight(x, (geo.ni, geo.C, k, k), P.double(), stride=s, padding=p)
    return gw[:, :geo.cvalid]


def to_itc(grad4):
    """a gradient [i, c, r, s] -> [i, tap, c], the (i, j = tap * C + c) order"""
    return grad4.permute(0, 2, 3, 1).reshape(grad4.shape[0], grad4.shape[2] * grad4.shape[3], grad4.shape[1])


def descriptors(geo, p_t, q_ts):
    """(gp, gq): the VuGather descriptors of P (1x1 over p_t) and Q"""
    from vaeunet_amd import kernels as K
    gp = K.gather([p_t], geo.N, geo.H, geo.W)
    gq = K.gather(list(q_ts), geo.N, geo.H, geo.W, **geo.qkw)
    assert (gq.Hs, gq.Ws) == geo.src_hw and gq.C == geo.C
    return gp, gq


def place(x, dtype, device, strided):
    """CPU [N, C, H, W] -> NHWC storage-dtype tensor inside a guarded buffer,
    dense or (strided) the upper channel slice of a tensor twice as wide whose
    other half holds the (non-zero) sentinel.  -> (tensor, Guard)"""
    N, C, H, W = x.shape
    t, g = R.guarded_act(N, C, H, W, TORCH_DTYPE[dtype], device, wide=2 * C if strided else None,
                         c0=C if strided else 0)
    t.copy_(x.to(TORCH_DTYPE[dtype]))
    return t, g


# ----------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------
def gathered(gp, gq, ni, nj):
    """P [M, ni] and Q [M, nj] in fp64, as the descriptors define them"""
    P = torch.cat([A for _, A in _Im2col(gp).taps(0, gp.N)], 1)[:, :ni]
    Q = torch.cat([A for _, A in _Im2col(gq).taps(0, gq.N)], 1)[:, :nj]
    return P, Q


def wgrad_ref(gp, gq, ni, nj):
    """(ref, sabs) [ni, nj] fp64: ref = sum_m P[m][i] Q[m][j], sabs the same
    over |P| |Q|."""
    P, Q = gathered(gp, gq, ni, nj)
    return P.t() @ Q, P.abs().t() @ Q.abs()


def grad_view(t, ni, taps, cvalid, layout):
    """the written (i, tap, c < cvalid) elements of gradient tensor ``t``
    (any shape; its first element is the base) as a strided view"""
    return torch.as_strided(t, (ni, taps, cvalid), tuple(layout), t.storage_offset())


def same_view(store, t):
    """``t``'s view (shape, strides, offset) over another flat buffer, e.g. a
    clone of the guarded buffer that holds ``t``, taken before the launch"""
    return torch.as_strided(store, t.shape, t.stride(), t.storage_offset())


def slab_ref(slab, layout, C, cvalid, old):
    """The fp64 result of vu_slab_reduce and its sabs, [ni, taps, cvalid]:
    sum_s slab[s][i][tap * C + c] (+ old at i s_i + tap s_tap + c s_c); ``old``:
    the gradient tensor before the launch when accumulating, else None."""
    S, ni, nj = slab.shape
    taps = nj // C
    s = slab.double().view(S, ni, taps, C)[..., :cvalid]
    val, sabs = s.sum(0), s.abs().sum(0)
    if old is not None:
        o = grad_view(old, ni, taps, cvalid, layout).double()
        val, sabs = val + o, sabs + o.abs()
    return val, sabs


def bound_random(M, sabs, dtype, old=None):
    """the order-independent fp32 summation bound of the module docstring"""
    n = M if dtype == BF16 else 2 * M
    if old is None:
        return (n - 1) * U32 * sabs
    return n * U32 * (sabs + old.double().abs())


class Worst(float):
    """a worst err/bound, with the index ``at`` and the case ``what`` it was met at"""
    at, what = None, ""

    def __str__(self):
        return f"worst err/bound {float(self):.3e} at {self.at} of {self.what}"


def check_bound(got, ref, bound, what):
    """every element within its bound -> the worst err/bound (a Worst)"""
    got, ref, bound = got.double(), ref.double(), bound.double()
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (bound + 1e-300))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    worst = float(ratio.max())
    at = tuple(int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape))
    assert worst <= 1.0, (f"{what}: bound exceeded {worst:.4g}x at {at}: got {float(got[at]):.9g}, ref "
                          f"{float(ref[at]):.9g}; {int((ratio > 1).sum())} of {ratio.numel()} elements off")
    worst = Worst(worst)
    worst.at, worst.what = at, what
    return worst


def check_exact(got, ref, what):
    """impulse operands: the fp64 reference is a float32 and ``got`` is it
    -> the number of non-zero elements"""
    assert bool((ref.float().double() == ref).all()), f"{what}: reference is not exactly a float32"
    want = ref.float()
    same = got.float() == want      # (-0 equals +0)
    n = int((~same).sum())
    if n:
        at = tuple(int(v) for v in (~same).nonzero()[0])
        raise AssertionError(f"{what}: {n} of {same.numel()} elements differ from the exact result, first at {at}: "
                             f"got {float(got[at]):.9g}, want {float(want[at]):.9g}")
    return int((want != 0).sum())


def check_slab_written(slab, what):
    n = int((slab == R.SENTINEL).sum())
    assert n == 0, f"{what}: {n} slab elements were not written"


def written_mask(store, grad, ni, taps, cvalid, layout):
    """bool mask over the flat storage ``store`` (which holds ``grad``) of the
    elements the reduce may write"""
    idx = torch.arange(store.numel(), device=store.device)
    off = grad.storage_offset() - store.storage_offset()
    m = torch.zeros(store.numel(), dtype=torch.bool, device=store.device)
    m[torch.as_strided(idx, (ni, taps, cvalid), tuple(layout), off).reshape(-1)] = True
    assert int(m.sum()) == ni * taps * cvalid, "layout maps two gradient elements onto one address"
    return m


def check_untouched(store, before, written, what):
    """everything outside the written set is bit-unchanged"""
    bad = (_bits(store) != _bits(before)) & ~written
    n = int(bad.sum())
    assert n == 0, f"{what}: {n} elements outside the written set changed, first at flat offset {int(bad.nonzero()[0])}"


def grad_sink(shape, layout_kind, device, old=None, wide=0):
    """A gradient of ``shape`` = [i, c, r, s] inside a guarded buffer.
    layout_kind: "contig" ([i, c, r, s] contiguous), "cl" (channels_last),
    "sub" (channels [wide, wide + c) of a contiguous gradient ``2 wide + c``
    channels wide: s_i larger than the written row).  Pre-filled with ``old``
    (CPU [i, c, r, s]) or left at the sentinel.
    -> (grad view [i, c, r, s], Guard, (s_i, s_tap, s_c))"""
    i, c, r, s = shape
    if layout_kind == "cl":
        t, g = R.guarded((i, r, s, c), torch.float32, device)
        grad = t.permute(0, 3, 1, 2)
    elif layout_kind == "sub":
        t, g = R.guarded((i, c + 2 * wide, r, s), torch.float32, device)
        grad = t[:, wide:wide + c]
    else:
        assert layout_kind == "contig"
        grad, g = R.guarded((i, c, r, s), torch.float32, device)
    if old is not None:
        grad.copy_(old)
    st = grad.stride()
    assert r == 1 or st[2] == s * st[3]       # engine.conv_layout / convT_layout accept it
    return grad, g, (st[0], st[3], st[1])


# ----------------------------------------------------------------------------
# split geometry
# ----------------------------------------------------------------------------
def tile_walk(N, H, W, TW, TH):
    """the halo kernel's tile order: image, tile column, tile row -> [(n, y0, x0)]"""
    return [(n, ty * TH, tx * TW) for n in range(N) for tx in range(W // TW) for ty in range(H // TH)]


def _tile_pixels(N, H, W, TW, TH, t):
    n, y0, x0 = t
    yy = torch.arange(y0, y0 + TH).view(-1, 1)
    xx = torch.arange(x0, x0 + TW).view(1, -1)
    return ((n * H + yy) * W + xx).reshape(-1)


def split_rows(geo, m_per_split, splits, tile=None):
    """The pixels m of every split, a list of ``splits`` index tensors.
    tile None: split s is the range [s mps, (s + 1) mps) of m (v1, v2).
    tile (TW, TH): split s is mps / 128 consecutive tiles of the halo kernel's
    walk (v3)."""
    M = geo.M
    if tile is None:
        return [torch.arange(min(M, s * m_per_split), min(M, (s + 1) * m_per_split)) for s in range(splits)]
    TW, TH = tile
    assert m_per_split % 128 == 0 and TW * TH == 128
    tps = m_per_split // 128
    walk = tile_walk(geo.N, geo.H, geo.W, TW, TH)
    out = []
    for s in range(splits):
        ts = walk[s * tps:(s + 1) * tps]
        out.append(torch.cat([_tile_pixels(geo.N, geo.H, geo.W, TW, TH, t) for t in ts]) if ts
                   else torch.zeros(0, dtype=torch.long))
    return out


def seam_pixels(geo, tile, m_per_split):
    """The pixels m worth an impulse: the four corners and four edge midpoints
    of every image; both sides of every tile seam in x and y (tile = (TW, TH)
    for v3; an int = the pixels per step of v1 / v2, whose seams are in m);
    the last pixel of image n and the first of image n + 1; both sides of
    every split seam; pixel M - 1.  Sorted, unique."""
    N, H, W, M = geo.N, geo.H, geo.W, geo.M
    px = set()
    lin = lambda n, y, x: (n * H + y) * W + x  # noqa: E731
    for n in range(N):
        for y in (0, H // 2, H - 1):
            for x in (0, W // 2, W - 1):
                if (y, x) != (H // 2, W // 2):
                    px.add(lin(n, y, x))
        px.add(lin(n, H - 1, W - 1))
        if n + 1 < N:
            px.add(lin(n + 1, 0, 0))
    if isinstance(tile, tuple):
        TW, TH = tile
        xs = sorted({0, W - 1} | {x for k in range(1, W // TW) for x in (k * TW - 1, k * TW)})
        ys = sorted({0, H - 1} | {y for k in range(1, H // TH) for y in (k * TH - 1, k * TH)})
        for n in range(N):
            px.update(lin(n, y, x) for y in ys for x in xs)
        walk = tile_walk(N, H, W, TW, TH)
        tps = m_per_split // 128
        for t in range(tps, len(walk), tps):           # split seams: last / first tile of a split
            for (n, y0, x0) in (walk[t - 1], walk[t]):
                px.update(lin(n, y, x) for y in (y0, y0 + TH - 1) for x in (x0, x0 + TW - 1))
    else:
        for unit in ([tile] if tile else []) + [m_per_split]:      # step seams, split seams
            for m in range(unit, M, unit):
                px.update((m - 1, m))
    px.add(M - 1)
    return sorted(px)


def _imp_value(i):
    return (-1.0) ** i * 2.0 ** ((i % 7) - 3)


def impulse_P(M, ni, pixels):
    """[M, ni]: P[pixels[i % len]][i] = +-2^k, zero elsewhere (one impulse
    per channel)"""
    assert 0 < len(pixels) <= ni
    P = torch.zeros(M, ni)
    for i in range(ni):
        P[pixels[i % len(pixels)], i] = _imp_value(i)
    return P


def impulse_Q(N, C, Hs, Ws, pixels):
    """[N, C, Hs, Ws]: channel c is +-2^k at source pixel pixels[c % len] (a
    linear index over (n, y, x)), zero elsewhere: every column group
    {tap * C + c} of the gathered Q then has at most one non-zero per column"""
    assert 0 < len(pixels) <= C
    q = torch.zeros(N, Hs, Ws, C)
    for c in range(C):
        q.view(-1, C)[pixels[c % len(pixels)], c] = _imp_value(c)
    return q.permute(0, 3, 1, 2)


def source_pixels(geo, pixels):
    """row-grid pixels -> the source pixels their centre tap reads (clipped
    into the image), plus the source image's corners; sorted, unique"""
    k, s, p = geo.ksp
    hs, ws = geo.src_hw
    kw = geo.qkw
    out = set()
    for m in pixels:
        n, rem = divmod(m, geo.H * geo.W)
        h, w = divmod(rem, geo.W)
        y = min(max(h * kw["sy"] + (kw["R"] // 2) + kw["oy"], 0), hs - 1)
        x = min(max(w * kw["sx"] + (kw["S"] // 2) + kw["ox"], 0), ws - 1)
        out.add((n * hs + y) * ws + x)
    for n in range(geo.N):
        out.update((n * hs + y) * ws + x for y in (0, hs - 1) for x in (0, ws - 1))
    return sorted(out)


def chunks(seq, n):
    return [seq[i:i + n] for i in range(0, len(seq), n)]


V2_STEP = {(32, 64): 128, (64, 128): 128, (64, 256): 64, (128, 256): 64, (256, 256): 32}   # gemm_wgrad2.hip


def run_step(run):
    """the seam unit of a Run: the halo tile (v3), else the pixels per step"""
    if run.tile:
        return run.tile
    return V2_STEP[run.expect[1:]] if run.expect[0] == 2 else 64


def impulse_sets(run, m_per_split):
    """(side, pixels) of every launch of an impulse case: impulse_P over all
    seam pixels, one per channel, in as many launches as that takes; then
    impulse_Q over the source pixels they read"""
    geo = run.geo
    seams = seam_pixels(geo, run_step(run), m_per_split)
    return ([("P", c) for c in chunks(seams, geo.ni)]
            + [("Q", c) for c in chunks(source_pixels(geo, seams), geo.C)])


def impulse_operands(geo, dtype, side, pixels):
    """(P [N, ni, H, W], Q sources) with the impulse on ``side`` ("P" | "Q":
    ``pixels`` are row-grid / source pixels) and the random operand of
    ``operands(geo, dtype)`` on the other"""
    P, Q = operands(geo, dtype)
    if side == "P":
        P = impulse_P(geo.M, geo.ni, pixels).view(geo.N, geo.H, geo.W, geo.ni).permute(0, 3, 1, 2)
    else:
        hs, ws = geo.src_hw
        Q = tuple(impulse_Q(geo.N, geo.C, hs, ws, pixels).split(list(geo.cins), 1))
    return P, Q


# ----------------------------------------------------------------------------
# float32 emulation of the kernels (CPU): per-split matmuls, then the slab
# reduce in the kernel's lane order
# ----------------------------------------------------------------------------
def emulate_slabs(P, Q, rows):
    """slab[s] = P[rows[s]]^T Q[rows[s]] in float32 (zeros for an empty split)"""
    P32, Q32 = P.float(), Q.float()
    return torch.stack([P32[r].t() @ Q32[r] for r in rows])


def slab_lanes(splits, vectorised):
    """split lanes of vu_slab_reduce (gemm_wgrad.hip)"""
    if not vectorised:
        return 4
    return 16 if splits >= 64 else 8 if splits >= 32 else 4 if splits >= 16 else 2 if splits >= 8 else 1


def slab_sum_emul(slab, vectorised=True):
    """float32 sum over the splits in the order of slab_reduce4_kernel<SL>
    (vectorised) or slab_reduce_kernel: lane q adds splits q, q + SL, ... into
    four accumulators (the 4 SL unroll), folds them pairwise, and the lanes
    are added in order (pairwise for the scalar kernel's 4 lanes)."""
    S = slab.shape[0]
    SL = slab_lanes(S, vectorised)
    slab = slab.float()
    lanes = []
    for q in range(SL):
        a = [torch.zeros_like(slab[0]) for _ in range(4)]
        k = q
        while k + 3 * SL < S:
            for u in range(4):
                a[u] = a[u] + slab[k + u * SL]
            k += 4 * SL
        while k < S:
            a[0] = a[0] + slab[k]
            k += SL
        lanes.append((a[0] + a[1]) + (a[2] + a[3]))
    if not vectorised:
        return (lanes[0] + lanes[1]) + (lanes[2] + lanes[3])
    s = lanes[0]
    for w in range(1, SL):
        s = s + lanes[w]
    return s


def slab_reduce_emul(slab, C, cvalid, layout, grad, accumulate, vectorised=True):
    """vu_slab_reduce in float32 on the CPU, writing the (i, tap, c < cvalid)
    elements of ``grad``"""
    S, ni, nj = slab.shape
    taps = nj // C
    s = slab_sum_emul(slab, vectorised).view(ni, taps, C)[..., :cvalid]
    view = grad_view(grad, ni, taps, cvalid, layout)
    view.copy_(view + s if accumulate else s)


def emulate(geo, P, Q, m_per_split, splits, tile, grad, layout, accumulate, vectorised=True):
    """the whole path on gathered fp64 operands P [M, ni], Q [M, nj] -> slab"""
    slab = emulate_slabs(P, Q, split_rows(geo, m_per_split, splits, tile))
    slab_reduce_emul(slab, geo.C, geo.cvalid, layout, grad, accumulate, vectorised)
    return slab


# ----------------------------------------------------------------------------
# case lists of tests/test_gpu_wgrad_kernels.py (every input set is also run
# through the float32 emulation on the CPU, tests/test_wgrad_ref.py)
# ----------------------------------------------------------------------------
GEN, SLAB4, W3_SMALL, W2_BIG = "VU_TUNE_GEN", "VU_TUNE_SLAB4", "VU_TUNE_W3_SMALL", "VU_TUNE_W2_BIG"
TUNE_DEFAULTS = {GEN: 4, SLAB4: 1, W3_SMALL: 1, W2_BIG: 0}        # csrc/tuning.hip


@dataclass(frozen=True)
class Run:
    """One launch sequence: the problem, its storage dtype, the tuning it runs
    under, the (generation, bi, bj) vu_gemm_wgrad_tile must answer, the halo
    tile (TW, TH) when the launch runs v3, and the (m_per_split, splits) list."""
    geo: Geo
    dtype: int
    tune: tuple
    expect: tuple
    plans: tuple
    tile: tuple = None
    sp: bool = False          # P as the upper channel slice of a wider tensor
    sq: bool = False          # the sources of Q likewise

    @property
    def id(self):
        t = ",".join(f"{k[8:]}={v}" for k, v in self.tune) or "default"
        return (f"{self.geo}-{'bf16' if self.dtype else 'fp32'}-{t}" + ("-sp" if self.sp else "")
                + ("-sq" if self.sq else "")).replace(" ", "_")


def _ceil(a, b):
    return -(-a // b)


def plans_linear(M, step):
    """v1 / v2: one split; m_per_split = ``step`` with ceil(M / step) splits;
    the same with one (empty) split more"""
    return ((M, 1), (step, _ceil(M, step)), (step, _ceil(M, step) + 1))


def v1_tile(ni):
    return (1, 64 if ni <= 64 else 128, 128)


# ---- B. v1: M on both sides of the 64-pixel step (35, 64, 65, 126, ...)
V1_GEOS = [
    Geo("3x3", 1, 5, 7, (8,), 8),
    Geo("3x3", 1, 8, 8, (32, 32), 64),
    Geo("3x3", 1, 5, 13, (24, 8, 16), 72),
    Geo("3x3", 2, 9, 7, (8,), 136),
    Geo("1x1", 2, 9, 7, (40,), 72),
    Geo("1x1", 1, 5, 13, (136,), 8),
    Geo("1x1s2", 1, 8, 8, (16,), 64),
    Geo("1x1s2", 1, 5, 7, (16,), 8, odd=(1, 1)),
    Geo("3x3s2", 2, 9, 7, (16,), 136),
    Geo("3x3s2", 1, 5, 13, (8,), 72, odd=(1, 1)),
    Geo("stem", 2, 7, 7, (8,), 64, odd=(1, 1)),          # 13 x 13 image
    Geo("stem", 1, 8, 10, (8,), 72),                     # 16 x 20 image
    Geo("convT", 1, 8, 8, (16,), 64, pyx=(0, 0), extra=(1, 1)),
    Geo("convT", 2, 9, 7, (8,), 136, pyx=(1, 0), extra=(2, 2)),
]
V1_RUNS = []
for _g in V1_GEOS:
    for _st in (False, True):
        V1_RUNS.append(Run(_g, BF16, ((GEN, 1),), v1_tile(_g.ni), plans_linear(_g.M, 64), sp=_st, sq=_st))
        V1_RUNS.append(Run(_g, F32, (), v1_tile(_g.ni), plans_linear(_g.M, 64), sp=_st, sq=_st))
_g = Geo("3x3", 1, 5, 7, (4,), 4)                                    # fp32 only: 4-channel chunks
V1_RUNS += [Run(_g, F32, (), (1, 64, 128), plans_linear(_g.M, 64), sp=_st, sq=_st) for _st in (False, True)]
# the dispatcher itself picks v1: bf16, default tuning, M < 512 (v2 refuses), 8 input channels (v3 refuses)
V1_RUNS.append(Run(Geo("3x3", 2, 9, 7, (8,), 72), BF16, (), (1, 128, 128), plans_linear(126, 64)))
V1_RUNS.append(Run(Geo("1x1", 1, 8, 8, (64,), 64), BF16, (), (1, 64, 128), plans_linear(64, 64)))


# ---- C. v2 (bf16, VU_TUNE_GEN = 2, M >= 512): (geo, tile, pixels per step)
def plans_v2(M, bmr):
    """one split; m_per_split = 1.5 steps, so that odd splits start off a step
    boundary (linear and decoding blocks in one launch), plus one empty split"""
    mps = 3 * bmr // 2
    return ((M, 1), (mps, _ceil(M, mps) + 1))


V2_GEOS = [
    # 32 x 64 tiles (128 pixels per step)
    (Geo("1x1", 2, 32, 8, (64,), 32), (32, 64), 128),                    # M = 512, W = 8: whole rows per step
    (Geo("1x1", 1, 13, 40, (24, 16), 24), (32, 64), 128),                # 24 x 40, M = 520: ragged, decoded walk
    (Geo("convT", 1, 8, 64, (16,), 32), (32, 64), 128),                  # ConvT (0, 0), canvas 2h x 2w: linear
    (Geo("1x1", 2, 4, 64, (24, 8, 16), 32), (32, 64), 128),              # three sources, cend 24 / 32 / 48
    # 64 x 128 tiles (128 pixels per step)
    (Geo("1x1", 1, 2, 256, (128,), 64), (64, 128), 128),                 # W = 256: steps inside a row, row wraps
    (Geo("1x1", 1, 13, 40, (72,), 40), (64, 128), 128),                  # 40 x 72
    (Geo("convT", 1, 8, 64, (32,), 64, pyx=(1, 1), extra=(2, 2)), (64, 128), 128),   # larger canvas: decoded
    (Geo("1x1s2", 2, 4, 64, (40, 32), 40), (64, 128), 128),              # source 2H x 2W: linear, sy = 2
    (Geo("1x1s2", 2, 4, 64, (40, 32), 40, odd=(1, 0)), (64, 128), 128),  # source height 2H - 1: decoded
    (Geo("1x1s2", 2, 32, 8, (72,), 64, odd=(0, 1)), (64, 128), 128),     # even height, odd width: linear
    (Geo("1x1s2", 2, 5, 64, (40, 32), 40), (64, 128), 128),              # M = 640: a step spans the image seam
    # 64 x 256 tiles (64 pixels per step)
    (Geo("stem", 2, 18, 17, (8,), 64, odd=(1, 1)), (64, 256), 64),       # 35 x 33 image, M = 612, nj = 392
    (Geo("3x3s2", 1, 8, 64, (16,), 64), (64, 256), 64),
    (Geo("3x3s2", 1, 13, 40, (16,), 40, odd=(1, 1)), (64, 256), 64),
    (Geo("1x1", 2, 32, 8, (136,), 64), (64, 256), 64),
    # 128 x 256 tiles (64 pixels per step)
    (Geo("1x1", 1, 8, 64, (128, 136), 136), (128, 256), 64),             # 136 x 264
    (Geo("3x3", 1, 22, 24, (64,), 72), (128, 256), 64),                  # W = 24: v3 refuses, decoded walk
    (Geo("1x1", 1, 2, 256, (264,), 136), (128, 256), 64),
    (Geo("convT", 2, 4, 64, (72,), 72), (128, 256), 64),                 # nj = 288
]
V2_RUNS = []
for _g, _tile, _bmr in V2_GEOS:
    for _st in (False, True):
        V2_RUNS.append(Run(_g, BF16, ((GEN, 2),), (2,) + _tile, plans_v2(_g.M, _bmr), sp=_st, sq=_st))
# 256 x 256 tiles (VU_TUNE_W2_BIG = 1; 32 pixels per step, 4-slot ring)
for _g in (Geo("1x1", 2, 32, 8, (264,), 264), Geo("1x1", 1, 13, 40, (128, 136), 264),
           Geo("1x1s2", 1, 8, 64, (264,), 264)):
    for _st in (False, True):
        V2_RUNS.append(Run(_g, BF16, ((GEN, 2), (W2_BIG, 1)), (2, 256, 256), plans_v2(_g.M, 32), sp=_st, sq=_st))


# ---- D. v3 (bf16, default generation)
def plans_v3(T, tps_list):
    return tuple((128 * tps, _ceil(T, tps)) for tps in tps_list if tps <= T) + ((128 * T, 2),)   # + an empty split


def _v3(kind_geo, tune, bi, tile, tps, sp=False, sq=False):
    T = kind_geo.M // 128
    return Run(kind_geo, BF16, tune, (3, bi, 576), plans_v3(T, tps), tile=tile, sp=sp, sq=sq)


_T32, _T16 = (32, 4), (16, 8)
V3_RUNS = [
    # <64, 32>: the default tuning
    _v3(Geo("3x3", 1, 4, 32, (64,), 8), (), 64, _T32, (1,)),                       # one tile, every border
    _v3(Geo("3x3", 1, 4, 32, (64,), 64), (), 64, _T32, (1,), sp=True, sq=True),
    _v3(Geo("3x3", 1, 12, 96, (64, 128), 72), (), 64, _T32, (1, 2, 3, 4, 9)),      # 3 x 3 tiles, one interior
    _v3(Geo("3x3", 1, 12, 96, (64,), 192), (), 64, _T32, (2, 9), sp=True),
    _v3(Geo("3x3", 1, 12, 96, (64,), 24), (), 64, _T32, (4,), sq=True),
    _v3(Geo("3x3", 2, 8, 64, (64, 64, 64), 136), (), 64, _T32, (1, 2, 3, 4, 8)),   # tps = 3: mid-column, image seam
    _v3(Geo("3x3", 2, 8, 64, (64,), 128), (), 64, _T32, (3,), sp=True, sq=True),
    # <64, 16>: W = 16 or 48
    _v3(Geo("3x3", 1, 8, 16, (64,), 8), (), 64, _T16, (1,)),
    _v3(Geo("3x3", 1, 24, 48, (64, 128), 72), (), 64, _T16, (1, 2, 3, 4, 9)),
    _v3(Geo("3x3", 1, 24, 48, (64,), 136), (), 64, _T16, (2, 9), sp=True, sq=True),
    _v3(Geo("3x3", 2, 16, 16, (64, 64, 64), 192), (), 64, _T16, (1, 2, 3, 4)),     # tps = 3 crosses the image seam
    _v3(Geo("3x3", 2, 16, 16, (64,), 24), (), 64, _T16, (3,), sp=True),
    # <128, 32>: VU_TUNE_W3_SMALL = 0, W % 32 == 0, ni > 64
    _v3(Geo("3x3", 1, 12, 96, (64,), 72), ((W3_SMALL, 0),), 128, _T32, (1, 2, 3, 4, 9)),
    _v3(Geo("3x3", 2, 8, 64, (64, 128), 136), ((W3_SMALL, 0),), 128, _T32, (1, 3, 8), sp=True, sq=True),
    _v3(Geo("3x3", 1, 4, 32, (64, 64, 64), 192), ((W3_SMALL, 0),), 128, _T32, (1,)),
    _v3(Geo("3x3", 2, 8, 64, (64,), 192), ((W3_SMALL, 0),), 128, _T32, (3,), sq=True),
    # (VU_TUNE_W3_SMALL = 0, ni <= 64 stays on <64, 32>)
    _v3(Geo("3x3", 2, 8, 64, (64,), 64), ((W3_SMALL, 0),), 64, _T32, (3,)),
]
# refusals: the round-2 rules do not take 16-pixel-wide tiles, the problem goes to v2
V3_REFUSED_RUNS = [
    Run(Geo("3x3", 2, 16, 16, (64,), 72), BF16, ((W3_SMALL, 0),), (2, 128, 256), ((512, 1), (384, 3))),
    Run(Geo("3x3", 1, 24, 48, (64,), 64), BF16, ((W3_SMALL, 0),), (2, 64, 256), ((1152, 1), (384, 4))),
]
# m_per_split % 128 != 0 on a v3-eligible problem: the tile query answers v3, the launch runs v2
V3_OFF_GRANULE_RUN = Run(Geo("3x3", 2, 8, 64, (64,), 64), BF16, (), (3, 64, 576), ((192, 6), (192, 7)))

# cross-generation: the same operands under VU_TUNE_GEN 1, 2, 3, each held to the fp64 reference
XGEN_RUNS = []
for _g, _tile in ((Geo("3x3", 1, 12, 96, (64, 128), 72), _T32), (Geo("3x3", 2, 8, 64, (64,), 64), _T32),
                  (Geo("3x3", 2, 16, 16, (64, 64, 64), 136), _T16)):
    _pl = ((128 * (_g.M // 128), 1), (384, _ceil(_g.M, 384)))
    XGEN_RUNS.append(Run(_g, BF16, ((GEN, 1),), v1_tile(_g.ni), _pl))
    XGEN_RUNS.append(Run(_g, BF16, ((GEN, 2),), (2, 64 if _g.ni <= 64 else 128, 256), _pl))
    XGEN_RUNS.append(Run(_g, BF16, ((GEN, 3),), (3, 64, 576), _pl, tile=_tile))

# ---- E. impulse cases: one N = 2 geometry per instantiation; plans: one
# split, the finest the generation runs, and seams inside a tile row (v1 / v2:
# a split that is no multiple of the step or of the image width; v3: 3 tiles
# per split, which starts splits mid-column)
IMPULSE_RUNS = [
    Run(Geo("3x3", 2, 9, 7, (8,), 64), BF16, ((GEN, 1),), (1, 64, 128), ((126, 1), (64, 2), (25, 6))),
    Run(Geo("3x3", 2, 9, 7, (8,), 136), BF16, ((GEN, 1),), (1, 128, 128), ((126, 1), (64, 2), (25, 6))),
    Run(Geo("3x3", 2, 9, 7, (8,), 64), F32, (), (1, 64, 128), ((126, 1), (64, 2), (25, 6))),
    Run(Geo("3x3s2", 2, 9, 7, (16,), 136, odd=(1, 1)), F32, (), (1, 128, 128), ((126, 1), (64, 2), (25, 6))),
    Run(Geo("1x1", 2, 32, 8, (64,), 32), BF16, ((GEN, 2),), (2, 32, 64), ((512, 1), (64, 8), (100, 6))),
    Run(Geo("convT", 2, 4, 64, (32,), 64, pyx=(1, 1), extra=(2, 2)), BF16, ((GEN, 2),), (2, 64, 128),
        ((512, 1), (64, 8), (100, 6))),
    Run(Geo("stem", 2, 18, 17, (8,), 64, odd=(1, 1)), BF16, ((GEN, 2),), (2, 64, 256), ((612, 1), (64, 10), (100, 7))),
    Run(Geo("3x3", 2, 11, 24, (64,), 136), BF16, ((GEN, 2),), (2, 128, 256), ((528, 1), (64, 9), (100, 6))),
    Run(Geo("1x1", 2, 32, 8, (264,), 264), BF16, ((GEN, 2), (W2_BIG, 1)), (2, 256, 256),
        ((512, 1), (64, 8), (100, 6))),
    # (3 x 3 tiles per image: the interior tile takes the halo kernel's precomputed-offset path)
    Run(Geo("3x3", 2, 12, 96, (64,), 72), BF16, (), (3, 64, 576), ((2304, 1), (128, 18), (640, 4)), tile=_T32),
    Run(Geo("3x3", 2, 24, 48, (64,), 72), BF16, (), (3, 64, 576), ((2304, 1), (128, 18), (640, 4)), tile=_T16),
    Run(Geo("3x3", 2, 8, 64, (64,), 136), BF16, ((W3_SMALL, 0),), (3, 128, 576), ((1024, 1), (128, 8), (384, 3)),
        tile=_T32),
]

# ---- F. through kernels.gemm_wgrad (the production plan): default tuning
PLAN_GEOS = [
    (Geo("3x3", 2, 8, 64, (64,), 72), (3, 64, 576)),
    (Geo("1x1", 2, 32, 8, (64, 72), 40), (2, 64, 256)),
    (Geo("convT", 2, 4, 64, (32,), 64, pyx=(1, 0), extra=(1, 0)), (2, 64, 128)),
    (Geo("stem", 2, 18, 17, (8,), 64, odd=(1, 1)), (2, 64, 256)),
]

# ---- A. vu_slab_reduce alone
SLAB_SPLITS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]
SLAB_SHAPES = [(8, 72, 8, 8), (8, 72, 8, 3), (64, 392, 8, 3), (4, 27, 3, 3), (5, 27, 3, 3), (24, 256, 64, 64)]


def slab_input(splits, ni, nj, seed=0):
    """random slabs whose magnitudes spread over 2^-8 .. 2^8 (order matters)"""
    g = torch.Generator().manual_seed(1000 * splits + ni + nj + seed)
    e = torch.randint(-8, 9, (splits, ni, nj), generator=g).float()
    return torch.randn(splits, ni, nj, generator=g) * torch.exp2(e)


def slab_grad_shape(ni, nj, C, cvalid):
    k = int(round((nj // C) ** 0.5))
    assert k * k * C == nj
    return (ni, cvalid, k, k)


ALL_RUNS = V1_RUNS + V2_RUNS + V3_RUNS + V3_REFUSED_RUNS + [V3_OFF_GRANULE_RUN] + XGEN_RUNS
