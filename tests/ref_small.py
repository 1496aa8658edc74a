"""Plain fp64 CPU references of the small hand-written kernels (VAE glue,
OutConv family, capturable AdamW, the latent path of latent.hip, the objective
of loss.hip, the inference kernels of infer.hip), the per-element bounds their
tests share, and guarded device buffers for those tests.

Every reference takes CPU tensors, computes in float64 and returns the value
and, where a bound needs it, the same op on |operands| (``sabs``, the
convention of ``_close`` in test_gpu_kernels.py).  Activations are pixel-major
matrices [P, C] (NHWC with the pixels flattened) unless a shape says otherwise.
"""
import torch
import torch.nn.functional as F

SENTINEL = 12345.0
TILE = 256      # pixels per block of the OutConv backward kernels
BF16_TINY = 2.0 ** -133   # smallest positive (subnormal) bfloat16


# ----------------------------------------------------------------------------
# guarded buffers
# ----------------------------------------------------------------------------
class Guard:
    """A flat buffer pre-filled with the sentinel and a mask of the elements
    no kernel may write; ``check()`` asserts that those still hold it."""

    def __init__(self, buf, keep):
        self.buf = buf
        self.keep = keep   # bool mask over buf: True where the sentinel must survive

    def check(self, what=""):
        want = torch.full((), _sentinel(self.buf.dtype), dtype=self.buf.dtype, device=self.buf.device)
        bad = (self.buf != want) & self.keep
        n = int(bad.sum())
        assert n == 0, (f"{what}: {n} guard elements overwritten, first at flat offset "
                        f"{int(bad.flatten().nonzero()[0])} of {self.buf.numel()}")


def _sentinel(dtype):
    return SENTINEL if dtype.is_floating_point else 0xA5   # (uint8 argmax codes)


def guarded(shape, dtype, device="cuda", pad=64, offset=0):
    """A contiguous tensor of ``shape`` that starts ``pad + offset`` elements
    into a sentinel-filled buffer with ``pad`` more elements behind it (offset
    = 1 misaligns a float tensor to 16 bytes).  The inner part holds the
    sentinel too, so an element the kernel skipped shows as a wrong value.
    Returns (tensor, Guard)."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * pad + offset,), _sentinel(dtype), dtype=dtype, device=device)
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=device)
    keep[pad + offset:pad + offset + n] = False
    return buf[pad + offset:pad + offset + n].view(shape), Guard(buf, keep)


def guarded_act(N, C, H, W, dtype, device="cuda", wide=None, c0=0, pad=64):
    """An NHWC activation [N, C, H, W] (channels_last strides) inside a guarded
    buffer; with ``wide`` the view is channels [c0, c0 + C) of a ``wide``-channel
    tensor, whose other channels are part of the guard."""
    Cw = wide or C
    full, g = guarded((N, H, W, Cw), dtype, device, pad)
    inner = torch.zeros((N, H, W, Cw), dtype=torch.bool, device=device)
    inner[..., c0:c0 + C] = True
    g.keep[pad:pad + inner.numel()] = ~inner.flatten()
    return full.permute(0, 3, 1, 2)[:, c0:c0 + C], g


def guarded_rows(P, C, dtype, device="cuda", wide=None, c0=0, pad=64):
    """The same for a pixel-major matrix [P, C] at row stride ``wide``."""
    t, g = guarded_act(1, C, P, 1, dtype, device, wide, c0, pad)
    return t[0, :, :, 0].t(), g


# ----------------------------------------------------------------------------
# max pool 3x3 / stride 2 / pad 1
# ----------------------------------------------------------------------------
def pool3_ref(x):
    """x [N, C, H, W] -> (y, code uint8): torch's max_pool2d and its flat
    argmax turned into the window code a*3 + b, a = h - (2i - 1), b = w - (2j - 1)."""
    N, C, H, W = x.shape
    y, flat = F.max_pool2d(x.double(), 3, 2, 1, return_indices=True)
    Ho, Wo = y.shape[2], y.shape[3]
    h, w = flat // W, flat % W
    i = torch.arange(Ho).view(1, 1, Ho, 1)
    j = torch.arange(Wo).view(1, 1, 1, Wo)
    a, b = h - (2 * i - 1), w - (2 * j - 1)
    assert int(a.min()) >= 0 and int(a.max()) <= 2 and int(b.min()) >= 0 and int(b.max()) <= 2
    return y, (a * 3 + b).to(torch.uint8)


def pool3_bwd_ref(dy, code, H, W):
    """Scatter dy [N, C, Ho, Wo] to the input pixel its window code names."""
    N, C, Ho, Wo = dy.shape
    dx = torch.zeros(N, C, H, W, dtype=torch.float64)
    code = code.long()
    a, b = code // 3, code % 3
    i = torch.arange(Ho).view(1, 1, Ho, 1)
    j = torch.arange(Wo).view(1, 1, 1, Wo)
    flat = ((2 * i - 1 + a) * W + (2 * j - 1 + b)).reshape(N, C, -1)
    dx.view(N, C, -1).scatter_add_(2, flat, dy.double().reshape(N, C, -1))
    return dx


# ----------------------------------------------------------------------------
# per-sample sums, tiny linear, reparameterisation
# ----------------------------------------------------------------------------
def sample_sum_ref(x, scale):
    """x [N, HW, C] -> (scale * sum over pixels, |scale| * sum |x|), [N, C]."""
    x = x.double()
    return scale * x.sum(1), abs(scale) * x.abs().sum(1)


def linear_fwd_ref(x, w, bias):
    """y[b, j] = bias[j] + sum_k x[b, k] w[j, k]; sabs = |bias| + sum |x||w|."""
    x, w = x.double(), w.double()
    y, s = x @ w.t(), x.abs() @ w.abs().t()
    if bias is not None:
        y, s = y + bias.double(), s + bias.double().abs()
    return y, s


def linear_bwd_ref(x, w, dy):
    """-> (dx, dw, db), (sabs of each)."""
    x, w, dy = x.double(), w.double(), dy.double()
    return (dy @ w, dy.t() @ x, dy.sum(0)), (dy.abs() @ w.abs(), dy.abs().t() @ x.abs(), dy.abs().sum(0))


def reparam_fwd_ref(mu, lv, eps):
    """z = mu + eps * exp(lv / 2); mag = |mu| + |eps| exp(lv / 2)."""
    mu, lv = mu.double(), lv.double()
    if eps is None:
        return mu, mu.abs()
    t = eps.double() * torch.exp(0.5 * lv)
    return mu + t, mu.abs() + t.abs()


def reparam_bwd_ref(lv, eps, dz):
    """-> dmu, dlv (dlv = dz * eps * exp(lv / 2) / 2, zero without eps)."""
    dz = dz.double()
    if eps is None:
        return dz, torch.zeros_like(dz)
    return dz, dz * eps.double() * 0.5 * torch.exp(0.5 * lv.double())


# ----------------------------------------------------------------------------
# 1x1 conv with a tiny output (OutConv), pixel-major
# ----------------------------------------------------------------------------
def pointwise_fwd_ref(x, w, b):
    """x [P, C], w [J, C], b [J] | None -> (y [P, J], mag = sum |x||w| + |b|)."""
    return linear_fwd_ref(x, w, b)


def pointwise_bwd_ref(x, w, dy):
    """-> (dx [P, C], dw [J, C], db [J]), (sabs of each)."""
    return linear_bwd_ref(x, w, dy)


def bn_near_zero(x, scale, shift):
    """Elements whose BatchNorm output x * scale + shift cancels to within
    1e-3 of its terms: there the sign (the ReLU mask) could depend on whether
    the multiply-add is contracted."""
    x, sc, sh = x.double(), scale.double(), shift.double()
    return (x * sc + sh).abs() < 1e-3 * ((x * sc).abs() + sh.abs())


def condition_bn_input(x, scale, shift, dtype):
    """Push every such element away from the cancellation (x grown by 1/32,
    several ulps of either storage dtype, and rounded back to it)."""
    x = x.to(dtype).float()
    bad = bn_near_zero(x, scale, shift)
    x = torch.where(bad, (x * 1.03125).to(dtype).float(), x)
    return x


def bn_act_ref(x, scale, shift, dtype):
    """relu(x * scale + shift) rounded to the storage dtype (fp64 multiply-add;
    compare with the device's bytes only where that is stated)."""
    return (x.double() * scale.double() + shift.double()).clamp_min(0).to(dtype).double()


def bnb_partials_ref(dx_stored, x, scale, shift, mean, invstd, nblk):
    """Block b's sums over the pixels {p : (p // TILE) % nblk == b} of
    dz = dx_stored masked by x * scale + shift > 0 and of dz * xhat.
    -> (part [nblk, 2, C], sabs [nblk, 2, C])."""
    P, C = x.shape
    x = x.double()
    keep = (x * scale.double() + shift.double()) > 0
    dz = dx_stored.double() * keep
    t = dz * ((x - mean.double()) * invstd.double())
    owner = (torch.arange(P) // TILE) % nblk
    part = torch.zeros(nblk, 2, C, dtype=torch.float64)
    sabs = torch.zeros(nblk, 2, C, dtype=torch.float64)
    part[:, 0].index_add_(0, owner, dz)
    part[:, 1].index_add_(0, owner, t)
    sabs[:, 0].index_add_(0, owner, dz.abs())
    sabs[:, 1].index_add_(0, owner, t.abs())
    return part, sabs


def bn_bwd_finish_ref(part, gamma, invstd, P):
    """vu_bn_bwd_reduce's finish (train = 1): dgamma = S1, dbeta = S0,
    k1 = gamma * invstd, k2 = -k1 * invstd * S1 / P, k3 = -k1 * S0 / P."""
    s0, s1 = part[:, 0].sum(0), part[:, 1].sum(0)
    k1 = gamma.double() * invstd.double()
    return s1, s0, torch.stack([k1, -k1 * invstd.double() * s1 / P, -k1 * s0 / P])


# ----------------------------------------------------------------------------
# shapes and seeded inputs shared by the GPU tests and their CPU self-checks
# ----------------------------------------------------------------------------
POOL_SHAPES = [(2, 8, 7, 9), (1, 16, 8, 6), (2, 8, 1, 1), (1, 8, 2, 5), (1, 24, 5, 4), (1, 64, 33, 17)]
LINEAR_FWD_CASES = [(1, 8, 1), (3, 512, 32), (64, 2048, 64), (5, 24, 7)]
LINEAR_BWD_CASES = [(2, 8, 32), (64, 512, 8), (3, 40, 5), (1, 8, 1)]
REPARAM_N = [1, 255, 256, 257, 64 * 64]
# (P, C, J) of the OutConv backward kernels; the last one exceeds the grid cap
# of 1024 blocks, so blocks 0 and 1 walk a second tile and block 1 a ragged one
PW_BWD_CASES = [(1, 8, 1), (255, 16, 2), (256, 64, 2), (257, 64, 3), (3 * 256 + 17, 256, 4),
                (1024 * 256 + 300, 8, 2)]
PW_BN_FWD_CASES = [(P, C, J) for P in (1, 255, 1029) for C in (8, 64, 256, 512) for J in (1, 2, 3, 4)]


def pool_input(shape, seed=3, negative=False):
    """Small integers (plenty of ties); ``negative``: all below zero."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 3, shape, generator=g).float()
    return x - 4 if negative else x


def pw_inputs(P, C, J, dtype, seed=21):
    """x [P, C] (rounded to dtype), w [J, C], b [J], dy [P, J] (fp32)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, C, generator=g).to(dtype).float()
    w = torch.randn(J, C, generator=g) / C ** 0.5
    b = torch.randn(J, generator=g)
    dy = torch.randn(P, J, generator=g)
    return x, w, b, dy


def bn_coef_inputs(C, seed=22):
    """scale (both signs), shift, mean, invstd, gamma [C]; every fourth channel
    is fully negative before the ReLU (all-zero operand)."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.randn(C, generator=g)
    scale = torch.where(scale.abs() < 0.05, torch.full_like(scale, 0.05), scale)
    shift = torch.randn(C, generator=g) * 0.5
    dead = torch.arange(C) % 4 == 3
    scale = torch.where(dead, torch.full_like(scale, 1e-3), scale)
    shift = torch.where(dead, torch.full_like(shift, -10.0), shift)
    mean = torch.randn(C, generator=g) * 0.1
    invstd = torch.rand(C, generator=g) + 0.5
    gamma = torch.rand(C, generator=g) + 0.5
    return scale, shift, mean, invstd, gamma


def pw_bn_inputs(P, C, J, dtype, seed=21):
    """pw_inputs with x conditioned against the BatchNorm's coefficients."""
    x, w, b, dy = pw_inputs(P, C, J, dtype, seed)
    coef = bn_coef_inputs(C)
    x = condition_bn_input(x, coef[0], coef[1], dtype)
    return x, w, b, dy, coef


# ----------------------------------------------------------------------------
# AdamW (torch.optim.AdamW, decoupled weight decay), fp64
# ----------------------------------------------------------------------------
def adamw_ref(p, m, v, g, step, lr, wd, beta1, beta2, eps):
    p, m, v, g = p.double(), m.double(), v.double(), g.double()
    p = p * (1 - lr * wd)
    m = m + (1 - beta1) * (g - m)
    v = v * beta2 + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
    return p, m, v


# ============================================================================
# Bounds shared by the kernel-level tests of latent.hip, loss.hip, infer.hip
# ============================================================================
U32 = 2.0 ** -24
C_SUM = 1e-5          # fp32 summation-order noise (test_gpu_kernels.py)
TINY = 2.0 ** -126
F32_MAX = 3.4028234663852886e38


def lin_ratio(got, ref, sabs, acc=None, u=U32):
    """Per element |got - ref| / (u max(|ref|, |got|) + C_SUM sabs [+ u |acc|])
    (the ``_close(..., sabs=...)`` bound of test_gpu_kernels.py without its
    global floor); 0 where both sides agree exactly, inf for a non-finite side."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    bound = u * torch.maximum(r.abs(), g.abs()) + C_SUM * sabs.detach().double().cpu()
    if acc is not None:
        bound = bound + u * acc.detach().double().cpu().abs()
    diff = (g - r).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)
    return torch.where(torch.isfinite(g) & torch.isfinite(r), ratio, torch.full_like(ratio, float("inf")))


def assert_lin(got, ref, sabs, what, acc=None, u=U32):
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    ratio = lin_ratio(got, ref, sabs, acc, u)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        i = int(ratio.flatten().argmax())
        raise AssertionError(f"{what}: per-element bound exceeded {worst:.3g}x at flat index {i} (got "
                             f"{float(got.flatten()[i]):.9g}, ref {float(ref.flatten()[i]):.9g}); "
                             f"{int((ratio > 1).sum())} of {ratio.numel()} elements off")
    return worst


def trans_ratio(got, ref, sabs):
    """The smallest r with |got - ref| <= r u sabs + 2^-126 for every element
    (the convention of test_gpu_ma_loss.py).  NaNs must sit in the same
    places on both sides (else inf) and are left out."""
    g, r, s = got.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten(), \
        sabs.detach().double().cpu().flatten()
    if not torch.equal(torch.isnan(g), torch.isnan(r)):
        return float("inf")
    ok = ~torch.isnan(r)
    g, r, s = g[ok], r[ok], s[ok]
    if g.numel() == 0:
        return 0.0
    same = g == r                                     # (equal infinities included)
    excess = torch.where(same, torch.zeros_like(g), ((g - r).abs() - TINY).clamp_min(0))
    ratio = torch.where(excess > 0, excess / (U32 * s), torch.zeros_like(excess))   # sabs = 0 and an excess: inf
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return float(ratio.max())


def assert_trans(got, ref64, ref32, sabs, what, log=None, split=None):
    """|got - ref64| <= 4 max(r_cpu, 1) u sabs + 2^-126, r_cpu measured from
    ``ref32`` (the same formulas in float32 on the CPU).  -> (r_hip, r_cpu)
    ``split`` (a bool mask): the planted, ill-conditioned elements and the
    rest are each held to their own r_cpu, so that the former's large figure
    does not loosen the bound of the latter."""
    if split is not None:
        m = split.flatten()
        if 0 < int(m.sum()) < m.numel():
            pick = lambda t, k: t.detach().cpu().flatten()[k]
            a = assert_trans(*(pick(t, m) for t in (got, ref64, ref32, sabs)), what + " (planted)", log)
            b = assert_trans(*(pick(t, ~m) for t in (got, ref64, ref32, sabs)), what + " (rest)", log)
            return max(a[0], b[0]), max(a[1], b[1])
    r_cpu, r_hip = trans_ratio(ref32, ref64, sabs), trans_ratio(got, ref64, sabs)
    msg = f"{what}: ratio {r_hip:.3g} (CPU float32 {r_cpu:.3g})"
    if log is not None:
        log.append(msg)
    print(msg)
    assert r_hip <= 4 * max(r_cpu, 1.0), msg
    return r_hip, r_cpu


# ============================================================================
# latent.hip: heads, consumers (1x1 conv + BatchNorm + ReLU of a per-sample
# constant map), split sums, backward -- plain fp64 formulas
# ============================================================================
LAT_SPLITS = 32
LAT_PCH = 1024
LAT_CG = 64
GATE_MARGIN = 1e-3


def pooled_ref(f):
    """f [N, HW, C] (stored values) -> (mean over pixels, mean |f|), [N, C]."""
    f = f.double()
    return f.mean(1), f.abs().mean(1)


def latent_bn_ref(y, gamma, beta, rm, rv, momentum, eps, train, HW):
    """BatchNorm of the per-sample constant maps y [N, co] (every vector
    counted HW times).  -> dict(scale, shift, mean, invstd, and in train mode
    with running statistics rm, rv (their updates), plus the *_abs operands of
    the shift and the updates).  momentum and eps are the float32 values the
    kernel is handed."""
    y, gamma, beta = y.double(), gamma.double(), beta.double()
    N = y.shape[0]
    M = N * HW
    mom = float(torch.tensor(momentum, dtype=torch.float32))
    eps = float(torch.tensor(eps, dtype=torch.float32))
    out = {}
    if train:
        mean = y.mean(0)
        var = ((y - mean) ** 2).mean(0)
        invstd = 1 / torch.sqrt(var + eps)
        if rm is not None:
            unb = var * (M / (M - 1) if M > 1 else 1.0)
            out["rm"] = (1 - mom) * rm.double() + mom * mean
            out["rv"] = (1 - mom) * rv.double() + mom * unb
            out["rm_abs"] = (1 - mom) * rm.double().abs() + mom * mean.abs()
            out["rv_abs"] = out["rv"].abs()
    else:
        mean = rm.double()
        invstd = 1 / torch.sqrt(rv.double() + eps)
    scale = gamma * invstd
    out.update(scale=scale, shift=beta - mean * scale, shift_abs=beta.abs() + (mean * scale).abs(), mean=mean,
               invstd=invstd)
    return out


def latent_act_ref(y, scale, shift):
    """relu(y * scale + shift) in fp64 and |y scale| + |shift|."""
    y, scale, shift = y.double(), scale.double(), shift.double()
    return (y * scale + shift).clamp_min(0), (y * scale).abs() + shift.abs()


def gate_near_zero(y, scale, shift):
    """(n, c) whose ReLU gate y * scale + shift > 0 could depend on the
    float32 rounding of the multiply-add (bn_near_zero's margin)."""
    return bn_near_zero(y, scale, shift)


def latent_sums_ref(dmap):
    """dmap [N, HW, C] -> part [N, LAT_SPLITS, C]: split s sums the pixels
    [s per, min(HW, (s + 1) per)), per = ceil(HW / LAT_SPLITS) (empty: 0)."""
    N, HW, C = dmap.shape
    per = (HW + LAT_SPLITS - 1) // LAT_SPLITS
    part = torch.zeros(N, LAT_SPLITS, C, dtype=torch.float64)
    for s in range(LAT_SPLITS):
        p0, p1 = s * per, min(HW, (s + 1) * per)
        if p1 > p0:
            part[:, s] = dmap[:, p0:p1].double().sum(1)
    return part


def latent_bwd_consumer_ref(part, y, coef, z, w, gamma, train):
    """The BatchNorm (+ReLU) and 1x1 conv backward of one consumer on the N
    vectors.  part [N, LAT_SPLITS, co] (per-sample pixel sums of the map's
    gradient, split), y [N, co], coef [4, co] = scale, shift, mean, invstd,
    z [N, L], w [co, L].  -> (dict(dgamma, dbeta, dbias, dw, dz), dict of the
    same formulas on |operands|)."""
    part, y, coef, z, w, gamma = (t.double() for t in (part, y, coef, z, w, gamma))
    N = y.shape[0]
    scale, shift, mean, invstd = coef
    S, S_abs = part.sum(1), part.abs().sum(1)
    keep = (y * scale + shift) > 0
    G, G_abs = S * keep, S_abs * keep
    xhat, xhat_abs = (y - mean) * invstd, (y.abs() + mean.abs()) * invstd
    dbeta, dbeta_abs = G.sum(0), G_abs.sum(0)
    dgamma, dgamma_abs = (G * xhat).sum(0), (G_abs * xhat_abs).sum(0)
    gi = gamma * invstd
    if train:
        v = gi * (G - (dbeta + xhat * dgamma) / N)
        v_abs = gi.abs() * (G_abs + (dbeta_abs + xhat_abs * dgamma_abs) / N)
    else:
        v, v_abs = gi * G, gi.abs() * G_abs
    val = dict(dgamma=dgamma, dbeta=dbeta, dbias=v.sum(0), dw=v.t() @ z, dz=v @ w, v=v)
    mag = dict(dgamma=dgamma_abs, dbeta=dbeta_abs, dbias=v_abs.sum(0), dw=v_abs.t() @ z.abs(), dz=v_abs @ w.abs(),
               v=v_abs)
    return val, mag


def latent_bwd_heads_ref(dz, dz_abs, dmu_in, dlv_in, eps, logvar, pooled, w_mu, w_lv):
    """dz [N, L] (incoming + the consumers'), reparameterize backward, both
    heads' backward.  None inputs count as zero (eps None: z = mu).
    -> (dict(dw_mu, dw_lv, db_mu, db_lv, dpooled), the same on |operands|)."""
    dz, dz_abs, pooled, w_mu, w_lv = (t.double() for t in (dz, dz_abs, pooled, w_mu, w_lv))
    zero = torch.zeros_like(dz)
    gm = zero if dmu_in is None else dmu_in.double()
    gl = zero if dlv_in is None else dlv_in.double()
    dmu, dmu_abs = gm + dz, gm.abs() + dz_abs
    if eps is None:
        dlv, dlv_abs = gl, gl.abs()
    else:
        k = eps.double() * 0.5 * torch.exp(0.5 * logvar.double())
        dlv, dlv_abs = gl + dz * k, gl.abs() + dz_abs * k.abs()
    val = dict(dw_mu=dmu.t() @ pooled, dw_lv=dlv.t() @ pooled, db_mu=dmu.sum(0), db_lv=dlv.sum(0),
               dpooled=dmu @ w_mu + dlv @ w_lv)
    mag = dict(dw_mu=dmu_abs.t() @ pooled.abs(), dw_lv=dlv_abs.t() @ pooled.abs(), db_mu=dmu_abs.sum(0),
               db_lv=dlv_abs.sum(0), dpooled=dmu_abs @ w_mu.abs() + dlv_abs @ w_lv.abs())
    return val, mag


# case lists of tests/test_gpu_latent_kernels.py (asserted free of gate edges
# on the CPU in test_ref_small.py)
HEADS_CASES = [(1, 1, 8, 1), (3, 3, 64, 12), (2, 33, 512, 32), (2, 37, 512, 64), (2, 9, 2048, 8), (64, 4, 16, 5)]
# (N, L, co, cpad, HW): every geometry, N in {1, 3, 64}, L in {1, 5, 32, 64};
# N = 3, HW = 600: a 1024-pixel store chunk straddles samples
LAT_FWD_CASES = [(1, 1, 8, 8, 1), (3, 5, 32, 64, 600), (64, 32, 8, 136, 70), (3, 64, 128, 128, 1024),
                 (1, 5, 2048, 2048, 1), (3, 32, 32, 32, 1025), (64, 64, 32, 64, 600), (3, 1, 8, 136, 70)]
# tables of 3 and 8 jobs with mixed geometry: (N, L, [(co, cpad, HW)])
LAT_FWD_TABLES = [(3, 5, [(32, 64, 600), (8, 136, 70), (8, 8, 1)]),
                  (3, 32, [(8, 8, 1), (32, 64, 600), (8, 136, 70), (128, 128, 1024), (2048, 2048, 1), (32, 32, 1025),
                           (64, 64, 33), (16, 24, 7)])]
LAT_SUMS_CASES = [(N, co, HW) for N in (1, 3) for co in (8, 32, 2048) for HW in (1, 31, 32, 33, 600)]
# (N, L, [co], heads C)
LAT_BWD_CASES = [(1, 1, [8], 8), (3, 5, [32], 24), (9, 64, [64], 512), (64, 5, [512], 24), (3, 64, [8, 32, 512], 512),
                 (9, 5, [64, 8, 32], 8), (64, 64, [32], 8), (1, 5, [8, 64, 512], 24)]


def heads_inputs(N, HW, C, L, dtype, seed=31):
    g = torch.Generator().manual_seed(seed + N + HW + C + L)
    f = torch.randn(N, HW, C, generator=g).to(dtype).float()
    w_mu = torch.randn(L, C, generator=g) / C ** 0.5
    w_lv = torch.randn(L, C, generator=g) / C ** 0.5
    b_mu, b_lv = torch.randn(L, generator=g) * 0.3, torch.randn(L, generator=g) * 0.3
    eps = torch.randn(N, L, generator=g)
    return f, w_mu, b_mu, w_lv, b_lv, eps


def consumer_params(L, co, train, bias=True, seed=32):
    """w [co, L], bias, gamma (both signs), beta, running mean / var, fp32."""
    g = torch.Generator().manual_seed(seed + 7 * L + co + (1 if train else 0))
    w = torch.randn(co, L, generator=g) / L ** 0.5
    b = torch.randn(co, generator=g) * 0.3 if bias else None
    gamma = (torch.rand(co, generator=g) + 0.5) * torch.where(torch.rand(co, generator=g) < 0.25, -1.0, 1.0)
    beta = torch.randn(co, generator=g) * 0.3
    rm = torch.randn(co, generator=g) * 0.2
    rv = torch.rand(co, generator=g) + 0.5
    return w, b, gamma, beta, rm, rv


def latent_z(N, L, seed=33):
    g = torch.Generator().manual_seed(seed + 3 * N + L)
    return torch.randn(N, L, generator=g)


def condition_beta(y, gamma, beta, rm, rv, momentum, eps, train, HW):
    """Move beta (fp32, by quarters) until no (n, c) of the gate y * scale +
    shift sits within the margin of zero: the BatchNorm's shift is what a test
    can place when y is the kernel's own (or, at N = 1, equals the mean).  -> beta"""
    beta = beta.clone()
    for _ in range(200):
        bn = latent_bn_ref(y, gamma, beta, rm, rv, momentum, eps, train, HW)
        bad = gate_near_zero(y, bn["scale"], bn["shift"]).any(0)
        if not bool(bad.any()):
            return beta
        beta = torch.where(bad, beta + 0.25, beta)
    raise AssertionError("condition_beta: gate edges left")


def condition_consumer(z, w, b, gamma, beta, rm, rv, momentum, eps, train, HW):
    """condition_beta on y = conv(z) in fp64 (the kernel's y is within a few
    float32 ulps of it, the margin is 1e-3)."""
    y, _ = linear_fwd_ref(z, w, b)
    return condition_beta(y, gamma, beta, rm, rv, momentum, eps, train, HW)


LAT_MOM, LAT_EPS = 0.1, 1e-5


def fwd_job_inputs(N, L, co, HW, train, bias=True, idx=0):
    """z [N, L] and one consumer's parameters (w, bias | None, gamma, beta,
    running mean, running var), beta conditioned against the gate's edge."""
    z = latent_z(N, L)
    w, b, gamma, beta, rm, rv = consumer_params(L, co, train, bias, seed=32 + 101 * idx)
    beta = condition_consumer(z, w, b, gamma, beta, rm, rv, LAT_MOM, LAT_EPS, train, HW)
    return z, (w, b, gamma, beta, rm, rv)


def bwd_consumer_inputs(N, L, co, train, integer=False, seed=34):
    """part [N, 32, co], y [N, co] (conditioned against coef), coef [4, co],
    gamma [co], w [co, L] given directly to vu_latent_bwd."""
    g = torch.Generator().manual_seed(seed + N + 5 * L + co + (1 if train else 0))
    if integer:
        part = torch.randint(-4, 5, (N, LAT_SPLITS, co), generator=g).float()
    else:
        part = torch.randn(N, LAT_SPLITS, co, generator=g)
    y = torch.randn(N, co, generator=g)
    w = torch.randn(co, L, generator=g) / L ** 0.5
    gamma = (torch.rand(co, generator=g) + 0.5) * torch.where(torch.rand(co, generator=g) < 0.25, -1.0, 1.0)
    beta = torch.randn(co, generator=g) * 0.3
    rm = None if train else torch.randn(co, generator=g) * 0.2
    rv = None if train else torch.rand(co, generator=g) + 0.5
    beta = condition_beta(y, gamma, beta, rm, rv, LAT_MOM, LAT_EPS, train, 1)
    bn = latent_bn_ref(y, gamma, beta, rm, rv, LAT_MOM, LAT_EPS, train, 1)
    coef = torch.stack([bn["scale"], bn["shift"], bn["mean"], bn["invstd"]]).float()
    assert int(gate_near_zero(y, coef[0], coef[1]).sum()) == 0    # (after the rounding to fp32 too)
    return part, y, coef, gamma, w


def heads_bwd_inputs(N, L, C, seed=35):
    g = torch.Generator().manual_seed(seed + N + 3 * L + C)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(dz_in=r(N, L), dmu_in=r(N, L), dlv_in=r(N, L), eps=r(N, L), logvar=r(N, L) * 0.5, pooled=r(N, C),
                w_mu=r(L, C) / C ** 0.5, w_lv=r(L, C) / C ** 0.5)


# ============================================================================
# loss.hip
# ============================================================================
def _sigmoid_plain(x):
    return 1 / (1 + torch.exp(-x))


def bce_dice_fwd_ref(x, t, dtype=torch.float64):
    """The four sums of vu_bce_dice_fwd2 -> (sums [4] fp64, sabs [4]): BCE with
    logits, sum p t, sum p, sum t with p = sigmoid(x), NaN -> 0 in the Dice
    sums.  float64: utils/loss.py's formulas (oracle/cpu_ref.py).  float32: the
    kernel's documented element formulas -- ATen's BCE form (1 - t) x + m +
    log(exp(-m) + exp(-x - m)), m = max(-x, 0), p = 1 / (1 + exp(-x)) --
    evaluated by torch in float32 and summed in float64 as the kernel does."""
    x, t = x.to(dtype).flatten(), t.to(dtype).flatten()
    if dtype == torch.float64:
        b = x.clamp_min(0) - x * t + torch.log1p(torch.exp(-x.abs()))
        b = torch.where(torch.isnan(x), x, b)
        p = torch.sigmoid(x)
    else:
        m = (-x).clamp_min(0)
        b = (1 - t) * x + m + torch.log(torch.exp(-m) + torch.exp(-x - m))
        p = _sigmoid_plain(x)
    p = torch.where(torch.isnan(p), torch.zeros_like(p), p)
    b, p, t = b.double(), p.double(), t.double()
    sums = torch.stack([b.sum(), (p * t).sum(), p.sum(), t.sum()])
    sabs = torch.stack([b.abs().sum(), (p * t).abs().sum(), p.abs().sum(), t.abs().sum()])
    return sums, sabs


def dice_loss_from_sums(sums, smooth, dtype=torch.float64):
    """1 - (2 I + smooth) / (max(sum p, smooth / 2) + max(sum t, smooth / 2) +
    smooth) from the kernel's own sums, cast to float32 first as the kernel
    does; -> (dice loss, 1 + dice)"""
    s = sums.double().float().to(dtype)
    sm = torch.tensor(smooth, dtype=torch.float32).to(dtype)
    half = sm * 0.5
    dice = (2 * s[1] + sm) / (torch.maximum(s[2], half) + torch.maximum(s[3], half) + sm)
    return 1 - dice, 1 + dice.abs().double()


def bce_dice_bwd_ref(x, t, sums, smooth, w_bce, w_dice, gscale, dtype=torch.float64):
    """d loss / d x from the kernel's own four sums (loss.hip's header):
    g (w_bce (p - t) / n - w_dice dp (2 t U - num mp) / U^2), dp = p (1 - p)
    (0 for a NaN logit), mp = [sum p >= smooth / 2].  -> (grad, sabs)"""
    x, t = x.to(dtype).flatten(), t.to(dtype).flatten()
    n = x.numel()
    f = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)
    sm, wb, wd, g = f(smooth), f(w_bce), f(w_dice), f(gscale)
    s = sums.double().float().to(dtype)
    half = sm * 0.5
    Uu = torch.maximum(s[2], half) + torch.maximum(s[3], half) + sm
    mp = (s[2] >= half).to(dtype)
    num = 2 * s[1] + sm
    if dtype == torch.float64:
        p, q = torch.sigmoid(x), torch.sigmoid(-x)
    else:
        p = _sigmoid_plain(x)
        q = 1 - p
    dp = torch.where(torch.isnan(p), torch.zeros_like(p), p * q)
    inv_n = (1 / f(float(n))) if dtype != torch.float64 else 1.0 / n
    grad = g * (wb * (p - t) * inv_n - wd * (dp * (2 * t * Uu - num * mp) / (Uu * Uu)))
    sabs = g.abs() * (wb.abs() * (p.abs() + t.abs()) * inv_n + wd.abs() * (dp * (2 * t.abs() * Uu + num * mp) / (Uu * Uu)))
    return grad, sabs.double()


def _nan0(v):
    return torch.nan_to_num(v, nan=0.0, posinf=F32_MAX, neginf=-F32_MAX)


def kl_ref(mu, lv, fb, gscale=1.0, dtype=torch.float64):
    """kl_with_free_bits (utils/loss.py:148-170) and its gradients as loss.hip
    documents them.  The free-bits comparison (>, ==, <) and the clamp mask are
    decided on the float32 value of kl in both dtypes (a tie exists only
    there).  -> dict(value, gmu, glv, gmu_abs, glv_abs, kl32)"""
    B = mu.shape[0]
    m32, v32 = _nan0(mu.float()), _nan0(lv.float())
    kl32 = 0.5 * (m32 * m32 + torch.exp(v32) - v32 - 1)
    m, v = _nan0(mu.float()).to(dtype), _nan0(lv.float()).to(dtype)
    kl = 0.5 * (m * m + torch.exp(v) - v - 1)
    cmask = ((kl32 >= -100) & (kl32 <= 100)).to(dtype)
    klc = kl.clamp(-100, 100)
    mmask = torch.ones_like(klc)
    fb32 = torch.tensor(fb, dtype=torch.float32)
    if fb > 0:
        klc32 = kl32.clamp(-100, 100)
        mmask = torch.where(klc32 > fb32, 1.0, torch.where(klc32 == fb32, 0.5, 0.0)).to(dtype)
        klc = torch.maximum(klc, fb32.to(dtype))
    value = klc.double().sum() / B
    g = torch.tensor(gscale, dtype=torch.float32).to(dtype)
    s = g * cmask * mmask / B
    e = torch.exp(v)
    gmu = torch.where(torch.isfinite(mu), s * m, torch.zeros_like(m))
    glv = torch.where(torch.isfinite(lv), s * 0.5 * (e - 1), torch.zeros_like(m))
    return dict(value=value, gmu=gmu, glv=glv, gmu_abs=(s * m).abs().double(),
                glv_abs=(s.abs() * 0.5 * (e + 1)).double(), kl32=kl32)


def dice_score_ref(x, t, epsilon):
    """-> (score fp32, counts [3] fp64): a = x > 0.5, b = t > 0.5, the fp32
    formula (2 I + eps) / (sum a + sum b + eps), 1 when both are empty."""
    a, b = x.flatten() > 0.5, t.flatten() > 0.5
    na, nb, nab = int(a.sum()), int(b.sum()), int((a & b).sum())
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)
    score = f(1.0) if na + nb == 0 else (f(2.0) * f(nab) + f(epsilon)) / ((f(na) + f(nb)) + f(epsilon))
    return score, torch.tensor([na, nb, nab], dtype=torch.float64)


# ============================================================================
# infer.hip
# ============================================================================
def mean_groups_ref(x):
    """x [groups, n] fp32 -> the left-to-right fp32 sum over k divided by groups."""
    s = torch.zeros(x.shape[1], dtype=torch.float32)
    for k in range(x.shape[0]):
        s = s + x[k]
    return s / torch.tensor(float(x.shape[0]), dtype=torch.float32)


def sigmoid_ref(x, dtype=torch.float64):
    """1 / (1 + exp(-x)) -> (value, |value|)"""
    y = _sigmoid_plain(x.to(dtype))
    return y, y.abs().double()


def blend_weight_ref(ph, pw, ov, ramp, top, bottom, left, right):
    """visualize_vae.py:364-378: ones, times the ramp on the leading ``ov``
    entries and (1 - ramp) on the trailing ones of an axis, only when that
    axis is longer than 2 ov.  fp32 [ph, pw]"""
    w = torch.ones(ph, pw, dtype=torch.float32)
    if ov > 0 and ph > 2 * ov:
        if top:
            w[:ov, :] *= ramp[:ov, None]
        if bottom:
            w[ph - ov:, :] *= (1 - ramp[:ov])[:, None]
    if ov > 0 and pw > 2 * ov:
        if left:
            w[:, :ov] *= ramp[None, :ov]
        if right:
            w[:, pw - ov:] *= (1 - ramp[:ov])[None, :]
    return w


def patch_blend_ref(out, wsum, pred, w, sh, sw):
    """out [B, H, W], wsum [B, H, W] (fp32, updated in place), pred [B, ph, pw]
    -> |p w| + |new out| of the touched window (the slack of the fp32 bound)"""
    ph, pw = w.shape
    pwt = pred * w
    out[:, sh:sh + ph, sw:sw + pw] += pwt
    wsum[:, sh:sh + ph, sw:sw + pw] += w
    slack = torch.zeros_like(out, dtype=torch.float64)
    slack[:, sh:sh + ph, sw:sw + pw] = pwt.abs().double() + out[:, sh:sh + ph, sw:sw + pw].abs().double()
    return slack


def uncertainty_ref(seg, dtype=torch.float64):
    """seg [S, n] -> dict(mean, std, entropy, mi, cv) and dict of sabs
    (visualize_vae.py:90-117; eps = float32(1e-7); std unbiased, NaN at S = 1;
    sums over the samples run left to right)."""
    S = seg.shape[0]
    v = seg.to(dtype)
    eps = torch.tensor(1e-7, dtype=torch.float32).to(dtype)

    def ent(a):
        l1, l2 = torch.log(a + eps), torch.log(1 - a + eps)
        return -(a * l1 + (1 - a) * l2), (a.abs() * l1.abs() + (1 - a).abs() * l2.abs()).double()

    s = torch.zeros_like(v[0])
    e = torch.zeros_like(v[0])
    e_abs = torch.zeros(v.shape[1], dtype=torch.float64)
    for k in range(S):
        s = s + v[k]
        ek, ek_abs = ent(v[k])
        e = e + ek
        e_abs = e_abs + ek_abs
    Sf = torch.tensor(float(S), dtype=torch.float32).to(dtype)
    m = s / Sf
    q = torch.zeros_like(m)
    q_abs = torch.zeros(v.shape[1], dtype=torch.float64)
    for k in range(S):
        d = v[k] - m
        q = q + d * d
        q_abs = q_abs + (v[k].abs().double() + m.abs().double()) ** 2
    nan = torch.full_like(m, float("nan"))
    sd = torch.sqrt(q / (Sf - 1)) if S > 1 else nan
    sd_abs = torch.sqrt(q_abs / (S - 1)) if S > 1 else nan.double()
    h, h_abs = ent(m)
    val = dict(mean=m, std=sd, entropy=h, mi=h - e / Sf, cv=sd / (m + eps))
    mag = dict(mean=v.abs().double().sum(0) / S, std=sd_abs, entropy=h_abs, mi=h_abs + e_abs / S,
               cv=sd_abs / (m.double() + float(eps)).abs())
    return val, mag


def flip_rot_map(H, W, hflip, vflip, k):
    """data._flip_rot_map for an H x W patch: the source pixel (y, x) = (ay i +
    by j + cy, ax i + bx j + cx) of output (i, j) after HorizontalFlip ->
    VerticalFlip -> rot90(k) (counter-clockwise).  -> (map, Ho, Wo)"""
    ay, by, cy, ax, bx, cx = 1, 0, 0, 0, 1, 0
    h, w = H, W
    for _ in range(k % 4):
        # out[i][j] = prev[j][w - 1 - i], prev h x w -> out w x h
        ay, by, cy, ax, bx, cx = -by, ay, cy + by * (w - 1), -bx, ax, cx + bx * (w - 1)
        h, w = w, h
    if vflip:
        ay, by, cy = -ay, -by, (H - 1) - cy
    if hflip:
        ax, bx, cx = -ax, -bx, (W - 1) - cx
    return [ay, by, cy, ax, bx, cx], h, w


def flip_rot_ref(x, hflip, vflip, k):
    """x [C, H, W] -> torch.flip / torch.rot90 in the augmentation's order."""
    if hflip:
        x = torch.flip(x, [2])
    if vflip:
        x = torch.flip(x, [1])
    return torch.rot90(x, k % 4, [1, 2])


FLIP_ROT = [(hf, vf, k) for k in range(4) for vf in (False, True) for hf in (False, True)]
