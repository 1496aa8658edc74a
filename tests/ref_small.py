"""Plain fp64 CPU references of the small hand-written kernels (VAE glue,
OutConv family, capturable AdamW) and guarded device buffers for their tests.

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
