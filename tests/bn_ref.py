"""Plain fp64 CPU references of the BatchNorm kernels of bn.hip (formulas as
include/vaeunet.h and the comments of bn.hip state them), the per-element
bounds their tests share, float32 restatements of the kernels' own operation
order (the yardstick of tests/test_bn_attention_ref.py: a bound may not be
tighter than float32 arithmetic allows), and the seeded inputs of
tests/test_gpu_bn_kernels.py.

Conventions of ref_small.py: CPU tensors in, float64 out, ``sabs`` is the same
expression on |operands|; activations are pixel-major [P, C].  A reference is
NOT rounded to the storage dtype unless its name says so: the bound's
``u_store max(|ref|, |got|)`` term is that one rounding.
"""
import torch

from ref_small import (C_SUM, U32, bn_bwd_finish_ref, bn_coef_inputs, bn_near_zero, bnb_partials_ref,
                       condition_bn_input)
from vaeunet_amd import _lib

F32, BF16 = torch.float32, torch.bfloat16
U_STORE = {F32: 2.0 ** -24, BF16: 2.0 ** -8}
KEY_BN_NT_MB, KEY_BN_MINBLK = _lib.VU_TUNE_BN_NT_MB, _lib.VU_TUNE_BN_MINBLK
UNR = 4                                  # rows in flight per thread (bn.hip)
MOM, EPS = 0.1, 1e-5


# ----------------------------------------------------------------------------
# bounds
# ----------------------------------------------------------------------------
def el_ratio(got, ref, sabs, n, dtype):
    """|got - ref| / (u_store max(|ref|, |got|) + n U32 sabs) per element: one
    rounding to the storage dtype plus n float32 operations, each within U32 of
    the expression on |operands|.  0 where both agree exactly."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    bound = U_STORE[dtype] * torch.maximum(r.abs(), g.abs()) + n * U32 * sabs.detach().double().cpu()
    diff = (g - r).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)
    return torch.where(torch.isfinite(g) & torch.isfinite(r), ratio, torch.full_like(ratio, float("inf")))


def assert_el(got, ref, sabs, n, dtype, what):
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    ratio = el_ratio(got, ref, sabs, n, dtype)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        i = int(ratio.flatten().argmax())
        raise AssertionError(f"{what}: per-element bound exceeded {worst:.3g}x at flat index {i} (got "
                             f"{float(got.flatten()[i]):.9g}, ref {float(ref.flatten()[i]):.9g}); "
                             f"{int((ratio > 1).sum())} of {ratio.numel()} elements off")
    return worst


def assert_fin(got, ref, sabs, what):
    """A quantity finished in fp64 and rounded once, from operands that are
    themselves one or two float32 roundings off: 4 U32 relative to sabs."""
    g, r, s = got.detach().double().cpu(), ref.detach().double().cpu(), sabs.detach().double().cpu()
    assert tuple(g.shape) == tuple(r.shape), f"{what}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
    diff = (g - r).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / (4 * U32 * s))
    ratio = torch.where(torch.isfinite(g) & torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    assert worst <= 1.0, (f"{what}: 4 U32 sabs exceeded {worst:.3g}x at flat index {int(ratio.flatten().argmax())}; "
                          f"{int((ratio > 1).sum())} of {ratio.numel()} off")
    return worst


# ----------------------------------------------------------------------------
# statistics: per-tile (sum, M2) -> coefficients and running statistics
# ----------------------------------------------------------------------------
def tile_counts(tiles, tile_rows, rows):
    n = torch.full((tiles,), float(tile_rows), dtype=torch.float64)
    n[-1] = rows - (tiles - 1) * tile_rows
    return n


def bn_stats_ref(psum, pm2, tile_rows, rows, gamma, beta, rm, rv, momentum, eps):
    """psum, pm2 [tiles, C] -> dict(mean, var (biased), invstd, scale, shift
    and, with running statistics and momentum != 0, rm / rv (unbiased
    variance); *_abs: the operands of each bound).  momentum and eps are the
    float32 values the kernel is handed."""
    tiles, C = psum.shape
    n = tile_counts(tiles, tile_rows, rows)[:, None]
    s, q = psum.double(), pm2.double()
    mom = float(torch.tensor(momentum, dtype=F32))
    eps = float(torch.tensor(eps, dtype=F32))
    mean = s.sum(0) / rows
    M2 = (q + n * (s / n - mean) ** 2).sum(0)
    var = M2 / rows
    invstd = 1 / torch.sqrt(var + eps)
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    b = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    scale = g * invstd
    out = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=b - mean * scale,
               mean_abs=s.abs().sum(0) / rows, invstd_abs=invstd, scale_abs=scale.abs(),
               shift_abs=b.abs() + (mean * scale).abs())
    if rm is not None and mom != 0:
        unb = M2 / (rows - 1) if rows > 1 else var
        out.update(rm=(1 - mom) * rm.double() + mom * mean, rv=(1 - mom) * rv.double() + mom * unb,
                   rm_abs=(1 - mom) * rm.double().abs() + mom * mean.abs(),
                   rv_abs=(1 - mom) * rv.double().abs() + mom * unb.abs())
    return out


def bn_stats_f32(psum, pm2, tile_rows, rows, gamma, beta, rm, rv, momentum, eps):
    """bn_stats_stage2's tail: the fp64 combine rounded once, then float32."""
    r = bn_stats_ref(psum, pm2, tile_rows, rows, None, None, None, None, momentum, eps)
    C = psum.shape[1]
    mom = torch.tensor(momentum, dtype=F32)
    invstd, mean = r["invstd"].float(), r["mean"].float()
    g = torch.ones(C) if gamma is None else gamma.float()
    b = torch.zeros(C) if beta is None else beta.float()
    out = dict(mean=mean, invstd=invstd, scale=g * invstd, shift=b - mean * g * invstd)
    if rm is not None and momentum != 0:
        unb = (r["var"] * rows / (rows - 1) if rows > 1 else r["var"]).float()
        out.update(rm=(1 - mom) * rm.float() + mom * mean, rv=(1 - mom) * rv.float() + mom * unb)
    return out


def bn_eval_ref(gamma, beta, rm, rv, eps):
    """Eval coefficients: invstd = 1 / sqrt(rv + eps), scale = gamma invstd,
    shift = beta - rm scale, mean = rm."""
    C = rm.shape[0]
    eps = float(torch.tensor(eps, dtype=F32))
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    b = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    invstd = 1 / torch.sqrt(rv.double() + eps)
    scale = g * invstd
    return dict(mean=rm.double(), invstd=invstd, scale=scale, shift=b - rm.double() * scale,
                mean_abs=rm.double().abs(), invstd_abs=invstd, scale_abs=scale.abs(),
                shift_abs=b.abs() + (rm.double() * scale).abs())


# float32 operations of bn_eval_kernel behind each output: rv + eps, sqrt (which
# halves what is in front of it), 1 / x -> 3; times gamma -> 4; rm * gamma, times
# invstd, the subtraction -> 3 + 3
EVAL_N = dict(mean=0, invstd=3, scale=4, shift=6)


def bn_eval_f32(gamma, beta, rm, rv, eps):
    C = rm.shape[0]
    g = torch.ones(C) if gamma is None else gamma.float()
    b = torch.zeros(C) if beta is None else beta.float()
    invstd = 1 / torch.sqrt(rv.float() + torch.tensor(eps, dtype=F32))
    return dict(mean=rm.float(), invstd=invstd, scale=g * invstd, shift=b - rm.float() * g * invstd)


# ----------------------------------------------------------------------------
# apply, backward sums, finish, backward apply
# ----------------------------------------------------------------------------
APPLY_N = 2      # multiply, add (or one fma)
FUSED_N = 5      # ... the residual's multiply and add, the sum
BWD_APPLY_N = 4  # x - mean, k2 (.), the fma, + k3


def bn_apply_ref(x, scale, shift, relu, res=None, rscale=None, rshift=None):
    """[relu](x scale + shift [+ res rscale + rshift | + res]) -> (z, sabs)"""
    x, sc, sh = x.double(), scale.double(), shift.double()
    z, s = x * sc + sh, (x * sc).abs() + sh.abs()
    if res is not None:
        r = res.double()
        if rscale is not None:
            z, s = z + r * rscale.double() + rshift.double(), s + (r * rscale.double()).abs() + rshift.double().abs()
        else:
            z, s = z + r, s + r.abs()
    return (z.clamp_min(0) if relu else z), s


def bn_apply_f32(x, scale, shift, relu, dtype, res=None, rscale=None, rshift=None):
    z = x.float() * scale.float() + shift.float()
    if res is not None:
        r = res.float()
        if rscale is not None:
            r = r * rscale.float() + rshift.float()
        z = z + r
    return (z.clamp_min(0) if relu else z).to(dtype)


def bn_bwd_sums_ref(dy, x, scale, shift, mean, invstd, relu, nblk=1):
    """S0 = sum dz, S1 = sum dz xhat, dz = dy masked by x scale + shift > 0
    (relu), per block as bnb_partials_ref owns the pixels (nblk = 1: dense).
    -> (part [nblk, 2, C], sabs)"""
    if not relu:   # every element kept: a mask operand that is positive everywhere
        scale, shift = torch.zeros_like(scale), torch.ones_like(shift)
    return bnb_partials_ref(dy, x, scale, shift, mean, invstd, nblk)


def bn_bwd_sums_f32(dy, x, scale, shift, mean, invstd, relu, fused_mask=True):
    """chan_partial_kernel's element formulas in float32, summed in fp64 (the
    kernel's fp32 per-thread sums are what C_SUM is for).  -> [2, C]"""
    dz, xv = dy.float(), x.float()
    if relu:
        pre = (xv.double() * scale.double() + shift.double()).float() if fused_mask else xv * scale.float() + shift.float()
        dz = torch.where(pre > 0, dz, torch.zeros_like(dz))
    t = dz * ((xv - mean.float()) * invstd.float())
    return torch.stack([dz.double().sum(0), t.double().sum(0)])


def bn_finish_ref(part, part_abs, gamma, invstd, P, train):
    """dgamma = S1, dbeta = S0, k1 = gamma invstd, k2 = -k1 invstd S1 / P,
    k3 = -k1 S0 / P (train = 0: k2 = k3 = 0).  part_abs: sum |partials| (the
    sabs of the sums).  -> dict(dgamma, dbeta, coef [3, C], and *_abs)"""
    C = part.shape[2]
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    s0, s1 = part[:, 0].sum(0, dtype=torch.float64), part[:, 1].sum(0, dtype=torch.float64)
    dgamma, dbeta, coef = bn_bwd_finish_ref(torch.stack([s0, s1])[None], g, invstd, P)
    a0, a1 = part_abs[:, 0].sum(0, dtype=torch.float64), part_abs[:, 1].sum(0, dtype=torch.float64)
    k1, is_ = coef[0], invstd.double()
    coef_abs = torch.stack([k1.abs(), (k1 * is_).abs() * a1 / P, k1.abs() * a0 / P])
    if not train:
        coef = torch.stack([k1, torch.zeros_like(k1), torch.zeros_like(k1)])
    return dict(dgamma=dgamma, dbeta=dbeta, coef=coef, dgamma_abs=a1, dbeta_abs=a0, coef_abs=coef_abs)


def bn_finish_f32(part, gamma, invstd, P, train):
    """bn_bwd_final: fp64 column sums, k1 in float32, k2 / k3 in fp64 from the
    float32 k1 and rounded once."""
    C = part.shape[2]
    s0, s1 = part[:, 0].sum(0, dtype=torch.float64), part[:, 1].sum(0, dtype=torch.float64)
    g = torch.ones(C) if gamma is None else gamma.float()
    k1 = g * invstd.float()
    k2 = (-(k1.double()) * invstd.double() * s1 / P).float()
    k3 = (-(k1.double()) * s0 / P).float()
    zero = torch.zeros(C)
    return dict(dgamma=s1.float(), dbeta=s0.float(), coef=torch.stack([k1, k2 if train else zero, k3 if train else zero]))


def bn_bwd_apply_ref(dy, x, scale, shift, mean, coef, relu):
    """dx = k1 dz + k2 (x - mean) + k3, dz masked by x scale + shift > 0 (relu)
    -> (dx, sabs)"""
    dz, xv = dy.double(), x.double()
    if relu:
        dz = dz * ((xv * scale.double() + shift.double()) > 0)
    k1, k2, k3 = coef.double()
    t = k2 * (xv - mean.double())
    return k1 * dz + t + k3, (k1 * dz).abs() + t.abs() + k3.abs()


def bn_bwd_apply_f32(dy, x, scale, shift, mean, coef, relu, dtype):
    """bn_bwd_elem: fmaf(k1, dz, k2 * (x - mean)) + k3 with the mask by
    fmaf(x, scale, shift) > 0 (the fmas formed in fp64 and rounded once)."""
    dz, xv = dy.float(), x.float()
    if relu:
        pre = (xv.double() * scale.double() + shift.double()).float()
        dz = torch.where(pre > 0, dz, torch.zeros_like(dz))
    k1, k2, k3 = coef.float()
    t = k2 * (xv - mean.float())
    return ((k1.double() * dz.double() + t.double()).float() + k3).to(dtype)


def pool2_ref(a):
    """a [N, H, W, C] (stored values) -> the 2x2 / stride 2 maximum"""
    N, H, W, C = a.shape
    return a.reshape(N, H // 2, 2, W // 2, 2, C).amax((2, 4))


def chan_sum_ref(x, y0, x0, Hr, Wr):
    """x [N, H, W, C] -> (sum over the (Hr, Wr) window at (y0, x0) of every
    image, sum |x|), [C]"""
    w = x[:, y0:y0 + Hr, x0:x0 + Wr].double()
    return w.sum((0, 1, 2)), w.abs().sum((0, 1, 2))


# ----------------------------------------------------------------------------
# shapes and seeded inputs of tests/test_gpu_bn_kernels.py
# ----------------------------------------------------------------------------
# (C, input row stride, output row stride, first channel): None = dense.
# 8 .. 2048: the vector path (V = 1 and V = 256 are the ends of ChanMap); 24 and
# 3: the scalar path; 64 at stride 68: a vector-shaped C forced onto it.
DENSE = [(8, None, None, 0), (64, None, None, 0), (256, None, None, 0), (2048, None, None, 0)]
SCALAR = [(24, None, None, 0), (3, None, None, 0), (64, 68, 68, 4)]
SLICES = [(C, wi, wo, c0) for C in (8, 64) for (wi, wo, c0) in ((2 * C, C + 8, 8), (C + 8, 2 * C, 0))]
LAYOUTS = DENSE + SCALAR + SLICES
VECTOR = DENSE + SLICES


def layout_id(l):
    C, wi, wo, c0 = l
    return f"C{C}" + ("" if wi is None else f"-in{wi}-out{wo}-c{c0}")


def is_vector(l):
    C, wi, wo, _ = l
    V = C // 8
    return C % 8 == 0 and V & (V - 1) == 0 and V <= 256 and (wi or C) % 8 == 0 and (wo or C) % 8 == 0


def pixel_counts(C):
    """P in {1, R - 1, R UNR, R UNR + 1, 3 R 16 + 5}, R = 256 / (C / 8) the
    pixel rows a block covers per pass (scalar path: 256 / C, at least 1)."""
    R = 256 // (C // 8) if C % 8 == 0 else max(1, 256 // C)
    return sorted({1, max(1, R - 1), R * UNR, R * UNR + 1, 3 * R * 16 + 5})


def bn_inputs(P, C, dtype, seed=51):
    """x [P, C] conditioned against (scale, shift) and dy, both rounded to the
    storage dtype; scale (both signs, every fourth channel dead), shift, mean,
    invstd, gamma; k [3, C]; a residual and its affine."""
    g = torch.Generator().manual_seed(seed + 13 * C + P)
    scale, shift, mean, invstd, gamma = bn_coef_inputs(C, seed=seed + C)
    x = condition_bn_input(torch.randn(P, C, generator=g), scale, shift, dtype)
    dy = torch.randn(P, C, generator=g).to(dtype).float()
    k = torch.randn(3, C, generator=g)
    res = torch.randn(P, C, generator=g).to(dtype).float()
    rscale, rshift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    return dict(x=x, dy=dy, scale=scale, shift=shift, mean=mean, invstd=invstd, gamma=gamma, k=k, res=res,
                rscale=rscale, rshift=rshift)


def near_zero_count(x, scale, shift):
    return int(bn_near_zero(x, scale, shift).sum())


def stats_of(y, tile_rows, dtype=F32):
    """per-tile (sum, centered M2) of y [P, C] in fp64, rounded to float32 (what
    a GEMM epilogue hands vu_bn_finalize) -> psum, pm2 [tiles, C]"""
    P, C = y.shape
    tiles = (P + tile_rows - 1) // tile_rows
    ps, pm = torch.zeros(tiles, C, dtype=torch.float64), torch.zeros(tiles, C, dtype=torch.float64)
    for t in range(tiles):
        blk = y[t * tile_rows:(t + 1) * tile_rows].double()
        ps[t] = blk.sum(0)
        pm[t] = ((blk - blk.mean(0)) ** 2).sum(0)
    return ps.to(dtype), pm.to(dtype)


# (tiles, tile_rows, C): test_bn_finalize_partials' shapes, then C in {1, 3, 33}
# and tiles in {1, 31, 32, 33} (one stage-1 block's 32 tiles and either side)
FINALIZE_CASES = [(40000, 7, 64), (300, 128, 192), (5, 64, 8), (16385, 4, 16), (64, 128, 1024)] + \
                 [(t, 9, C) for t in (1, 31, 32, 33) for C in (1, 3, 33)]
# (momentum, running statistics, gamma / beta)
FINALIZE_MODES = [(0.1, True, True), (0.0, True, True), (0.1, False, True), (0.1, True, False)]


def finalize_inputs(tiles, tile_rows, C, seed=41):
    """synthetic partials with a ragged last tile (3 rows short, at least 1)"""
    g = torch.Generator().manual_seed(seed + tiles + C)
    rows = max(tiles * tile_rows - 3, (tiles - 1) * tile_rows + 1)
    n = tile_counts(tiles, tile_rows, rows)[:, None]
    mu_t = torch.randn(tiles, C, generator=g, dtype=torch.float64) * 0.5 + 2.0
    m2_t = torch.rand(tiles, C, generator=g, dtype=torch.float64) * n
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    beta = torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5
    return dict(psum=(mu_t * n).float(), pm2=m2_t.float(), rows=rows, gamma=gamma, beta=beta, rm=rm, rv=rv)


# vu_bn_bwd_finish on synthetic partials: 1024 is the last direct nblk, 1025
# the first folded one, 4097 and 16385 + 3 leave ragged fold rows
FINISH_NBLK = [1, 2, 1024, 1025, 4097, 16385 + 3]
FINISH_C = [1, 24, 64, 2048]


def finish_inputs(nblk, C, seed=61):
    g = torch.Generator().manual_seed(seed + nblk + C)
    part = torch.randn(nblk, 2, C, generator=g)
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    invstd = torch.rand(C, generator=g) + 0.5
    pre = torch.randn(2, C, generator=g)
    return dict(part=part, gamma=gamma, invstd=invstd, pre=pre, P=nblk * 64 - 7 if nblk > 1 else 57)


def planted_mask_inputs(P, C, dtype, seed=71):
    """The ReLU-mask agreement inputs: in a quarter of the pixels of each
    channel an x0 with shift = -fl32(x0 scale), so that the fused
    pre-activation fma(x0, scale, shift) is the rounding residual of the
    product (either sign, or zero) and the unfused one is exactly 0.  One x0
    per channel (the shift is per channel); the other pixels are conditioned
    away from the edge.  -> x [P, C] (rounded to dtype), scale, shift"""
    g = torch.Generator().manual_seed(seed + C + P)
    scale = torch.randn(C, generator=g)
    scale = torch.where(scale.abs() < 0.05, torch.full_like(scale, 0.05), scale)
    x0 = (torch.randn(C, generator=g) + 2.0).to(dtype).float()
    shift = -(x0 * scale)                                   # fl32 of the product
    x = torch.randn(P, C, generator=g).to(dtype).float()
    planted = torch.rand(P, C, generator=g) < 0.25
    x = torch.where(planted, x0.expand(P, C), x)
    bad = bn_near_zero(x, scale, shift) & ~planted
    x = torch.where(bad, ((x + 1.0) * 1.25).to(dtype).float(), x)
    return x, scale, shift, planted
