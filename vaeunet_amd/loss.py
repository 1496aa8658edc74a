"""Training objective (drop-in for the reference's utils/loss.py).

CombinedLoss / dice_loss / DiceLoss / kl_with_free_bits / KLAnnealer with the
reference's signatures and semantics (loss.py:6-63, 114-170), computed by the
fused HIP reduction kernels of csrc/loss.hip: one pass produces the four
global sums (BCE, sum p*t, sum p, sum t) in fp64, the loss is formed on the
device and the backward is one elementwise kernel — no host synchronisation
(the reference's ``isnan().any()`` check at loss.py:12 becomes a per-element
NaN->0 inside the kernel, which is what its nan_to_num achieves).

MAFocalLoss / MASegmentationLoss (loss.py:66-111, the ``--lesion-type MA``
objective) run on the fused focal + Dice kernels of csrc/focal.hip; their
definitions are written out in DESIGN.md §4.7 and are unpinned against the
reference, so every constant is a constructor argument.

boundary_loss / BoundaryLoss / BoundaryAugmentedLoss: the
boundary loss of Kervadec et al., mean(phi * sigmoid(x)) with phi the signed
distance map of the ground truth, computed on the device by csrc/sdf.hip and
reduced by csrc/boundary_loss.hip; not part of the reference.

Deviation, documented: the reference's ``.view(-1)`` (loss.py:17-18) raises on
channels_last logits with more than one class; here the sums are taken in
memory order, which equals the reference's result whenever it runs.
"""
import torch
import torch.nn as nn

from . import _lib
from . import surface as _surface
from ._lib import ptr, call, query, stream

CL = torch.channels_last


def _dense_pair(inputs, targets):
    if inputs.device.type != "cuda":
        raise RuntimeError("vaeunet_amd losses run on MI355X (HIP) devices only")
    x = inputs.float() if inputs.dtype != torch.float32 else inputs
    fmt = CL if (x.dim() == 4 and not x.is_contiguous() and x.is_contiguous(memory_format=CL)) \
        else torch.contiguous_format
    x = x.contiguous(memory_format=fmt)
    t = targets.to(device=x.device, dtype=torch.float32)
    if t.shape != x.shape:
        raise ValueError(f"target shape {tuple(t.shape)} != input shape {tuple(x.shape)}")
    t = t.contiguous(memory_format=fmt)
    return x, t


class _BceDice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, smooth, w_bce, w_dice):
        n = x.numel()
        sums = torch.empty(4, dtype=torch.float64, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        parts = torch.empty(2, dtype=torch.float32, device=x.device)
        ws = torch.empty(query("vu_loss_workspace_bytes") // 8 + 1, dtype=torch.float64,
                         device=x.device)
        call("vu_bce_dice_fwd2", ptr(x), ptr(t), n, ptr(sums), smooth, w_bce, w_dice, ptr(loss),
             ptr(parts), ptr(ws), stream())
        ctx.save_for_backward(x, t, sums)
        ctx.cfg = (smooth, w_bce, w_dice)
        ctx.mark_non_differentiable(parts)
        # no zero gradient materialised for `parts` (one fill launch less per step)
        ctx.set_materialize_grads(False)
        return loss, parts

    @staticmethod
    def backward(ctx, gout, _gparts):
        x, t, sums = ctx.saved_tensors
        smooth, w_bce, w_dice = ctx.cfg
        if gout is None:
            return None, None, None, None, None
        g = gout.float().contiguous()
        grad = torch.empty_like(x)
        call("vu_bce_dice_bwd", ptr(x), ptr(t), x.numel(), ptr(sums), smooth, w_bce, w_dice,
             ptr(g), ptr(grad), stream())
        return grad, None, None, None, None


def _combined(inputs, targets, smooth, w_bce, w_dice):
    x, t = _dense_pair(inputs, targets)
    loss, parts = _BceDice.apply(x, t, float(smooth), float(w_bce), float(w_dice))
    return loss, parts


def dice_loss(inputs, targets, smooth=1.0):
    """1 - soft Dice over the whole batch (loss.py:6-28)."""
    return _combined(inputs, targets, smooth, 0.0, 1.0)[0]


class DiceLoss(nn.Module):
    def __init__(self, smooth=1.0):
        super().__init__()
        self.smooth = smooth

    def forward(self, inputs, targets):
        return dice_loss(inputs, targets, self.smooth)


class CombinedLoss(nn.Module):
    """bce_weight * BCEWithLogits(mean) + dice_weight * dice_loss (loss.py:44-63).

    After a call, ``self.last_parts`` holds the device tensor [total, bce,
    dice_loss] (for logging without an extra pass)."""

    def __init__(self, bce_weight=0.5, dice_weight=0.5):
        super().__init__()
        self.bce_weight = bce_weight
        self.dice_weight = dice_weight
        self.last_parts = None

    def forward(self, inputs, targets):
        loss, parts = _combined(inputs, targets, 1.0, self.bce_weight, self.dice_weight)
        self.last_parts = parts
        return loss


# ---- focal + Dice (MAFocalLoss / MASegmentationLoss) --------------------------
def _check_focal_cfg(alpha, gamma, smooth, reduction):
    """Host-side validation, before any tensor is looked at."""
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"alpha must be in [0, 1], got {alpha}")
    g = float(gamma)
    if not (g == 0.0 or g >= 1.0):
        raise ValueError(f"gamma must be 0 or >= 1 (between them the gradient is unbounded at b -> 0), got {gamma}")
    if not float(smooth) > 0.0:
        raise ValueError(f"smooth must be > 0, got {smooth}")
    if reduction not in ("mean", "sum"):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")


def _focal_pair(inputs, targets):
    """_dense_pair with the shapes compared first (a mismatch is a ValueError
    on any device) and empty tensors refused."""
    if tuple(targets.shape) != tuple(inputs.shape):
        raise ValueError(f"target shape {tuple(targets.shape)} != input shape {tuple(inputs.shape)}")
    x, t = _dense_pair(inputs, targets)
    if x.numel() == 0:
        raise ValueError("focal_dice_loss: empty input")
    return x, t


def _focal_fwd(x, t, cfg):
    """The two forward launches: (loss, parts [focal, dice_loss], sums fp64 [5])."""
    alpha, gamma, smooth, w_focal, w_dice, sum_reduction = cfg
    sums = torch.empty(5, dtype=torch.float64, device=x.device)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    parts = torch.empty(2, dtype=torch.float32, device=x.device)
    ws = torch.empty(query("vu_focal_workspace_bytes") // 8, dtype=torch.float64, device=x.device)
    call("vu_focal_dice_fwd", ptr(x), ptr(t), x.numel(), alpha, gamma, smooth, w_focal, w_dice, sum_reduction,
         ptr(sums), ptr(loss), ptr(parts), ptr(ws), stream())
    return loss, parts, sums


def _focal_bwd(x, t, sums, gout, cfg):
    alpha, gamma, smooth, w_focal, w_dice, sum_reduction = cfg
    g = gout.float().contiguous()
    grad = torch.empty_like(x)
    call("vu_focal_dice_bwd", ptr(x), ptr(t), x.numel(), alpha, gamma, smooth, w_focal, w_dice, sum_reduction,
         ptr(sums), ptr(g), ptr(grad), stream())
    return grad


class _FocalDice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, cfg):
        loss, parts, sums = _focal_fwd(x, t, cfg)
        ctx.save_for_backward(x, t, sums)
        ctx.cfg = cfg
        ctx.mark_non_differentiable(parts)
        ctx.set_materialize_grads(False)
        return loss, parts

    @staticmethod
    def backward(ctx, gout, _gparts):
        if gout is None:
            return None, None, None
        x, t, sums = ctx.saved_tensors
        return _focal_bwd(x, t, sums, gout, ctx.cfg), None, None


def _focal_dice(inputs, targets, alpha, gamma, smooth, w_focal, w_dice, reduction):
    _check_focal_cfg(alpha, gamma, smooth, reduction)
    x, t = _focal_pair(inputs, targets)
    cfg = (float(alpha), float(gamma), float(smooth), float(w_focal), float(w_dice), int(reduction == "sum"))
    return _FocalDice.apply(x, t, cfg)


def focal_dice_loss(inputs, targets, alpha=0.75, gamma=2.0, smooth=1.0, focal_weight=0.5, dice_weight=0.5,
                    reduction="mean"):
    """focal_weight * focal + dice_weight * dice_loss in one fused pass:
    focal = mean | sum of a_t * (1 - exp(-b))**gamma * b, b = BCEWithLogits(x, t),
    a_t = alpha * t + (1 - alpha) * (1 - t); dice_loss as ``dice_loss``.  Any
    shape, soft targets allowed; a NaN logit adds nothing and gets gradient 0."""
    return _focal_dice(inputs, targets, alpha, gamma, smooth, focal_weight, dice_weight, reduction)[0]


class MAFocalLoss(nn.Module):
    """The focal term alone (loss.py:66-92)."""

    def __init__(self, alpha=0.75, gamma=2.0, reduction="mean"):
        super().__init__()
        _check_focal_cfg(alpha, gamma, 1.0, reduction)
        self.alpha = alpha
        self.gamma = gamma
        self.reduction = reduction

    def forward(self, inputs, targets):
        return _focal_dice(inputs, targets, self.alpha, self.gamma, 1.0, 1.0, 0.0, self.reduction)[0]


class MASegmentationLoss(nn.Module):
    """focal_weight * MAFocalLoss(mean) + dice_weight * dice_loss (loss.py:95-111).

    After a call, ``self.last_parts`` holds the device tensor [focal,
    dice_loss] (for logging without an extra pass)."""

    def __init__(self, focal_weight=0.5, dice_weight=0.5, alpha=0.75, gamma=2.0, smooth=1.0):
        super().__init__()
        _check_focal_cfg(alpha, gamma, smooth, "mean")
        self.focal_weight = focal_weight
        self.dice_weight = dice_weight
        self.alpha = alpha
        self.gamma = gamma
        self.smooth = smooth
        self.last_parts = None

    def forward(self, inputs, targets):
        loss, parts = _focal_dice(inputs, targets, self.alpha, self.gamma, self.smooth, self.focal_weight,
                                  self.dice_weight, "mean")
        self.last_parts = parts
        return loss


# ---- boundary loss --------------------------------------------
def _boundary_inputs(inputs, what):
    if not isinstance(inputs, torch.Tensor) or inputs.dim() not in (3, 4):
        raise ValueError(f"{what}: inputs must be a [B, C, H, W] or [B, H, W] tensor, got "
                         f"{tuple(inputs.shape) if isinstance(inputs, torch.Tensor) else type(inputs).__name__}")
    if inputs.numel() == 0:
        raise ValueError(f"{what}: empty input {tuple(inputs.shape)}")
    return tuple(inputs.shape) if inputs.dim() == 4 else (inputs.shape[0], 1) + tuple(inputs.shape[1:])


def _boundary_check(inputs, targets, phi, clip, threshold, what="boundary_loss"):
    """Every ValueError, before a device is touched -> (shape [B, C, H, W], clip as a float, threshold)"""
    shape = _boundary_inputs(inputs, what)
    if (targets is None) == (phi is None):
        raise ValueError(f"{what}: exactly one of targets and phi must be given")
    c = _surface._check_clip(clip, what)
    if phi is not None:
        if clip is not None or threshold is not None:
            raise ValueError(f"{what}: clip and threshold describe how phi is computed from targets; with phi= "
                             "they must be None")
        if not isinstance(phi, torch.Tensor) or phi.dtype != torch.float32 or tuple(phi.shape) != tuple(inputs.shape):
            raise ValueError(f"{what}: phi must be a float32 tensor of the inputs' shape {tuple(inputs.shape)}")
        return shape, c, None
    if not isinstance(targets, torch.Tensor) or tuple(targets.shape) != tuple(inputs.shape):
        raise ValueError(f"{what}: target shape {tuple(targets.shape) if isinstance(targets, torch.Tensor) else None} "
                         f"!= input shape {tuple(inputs.shape)}")
    if targets.dtype in (torch.uint8, torch.bool):
        thr = 0.0
    else:
        thr = 0.5 if threshold is None else float(threshold)
        if thr != thr:
            raise ValueError(f"{what}: the threshold is NaN")
    if shape[2] > _surface.VU_EDT_MAX_DIM or shape[3] > _surface.VU_SDF_MAX_W:
        raise ValueError(f"{what}: planes of {shape[2]} x {shape[3]} pixels exceed the signed distance map's "
                         f"H <= {_surface.VU_EDT_MAX_DIM}, W <= {_surface.VU_SDF_MAX_W}")
    return shape, c, thr


def _boundary_pair(inputs, phi):
    """_dense_pair for (logits, phi): the shapes compared first, empty tensors refused"""
    if tuple(phi.shape) != tuple(inputs.shape):
        raise ValueError(f"phi shape {tuple(phi.shape)} != input shape {tuple(inputs.shape)}")
    if inputs.numel() == 0:
        raise ValueError("boundary_loss: empty input")
    return _dense_pair(inputs, phi)


def _boundary_fwd(x, phi):
    """The two forward launches: (loss, sums fp64 [3] = sum phi p, sum |phi| p, skipped elements)."""
    sums = torch.empty(3, dtype=torch.float64, device=x.device)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    ws = torch.empty(query("vu_boundary_loss_workspace_bytes") // 8, dtype=torch.float64, device=x.device)
    call("vu_boundary_loss_fwd", ptr(x), ptr(phi), x.numel(), ptr(sums), ptr(loss), ptr(ws), stream())
    return loss, sums


def _boundary_bwd(x, phi, gout):
    g = gout.float().contiguous()
    grad = torch.empty_like(x)
    call("vu_boundary_loss_bwd", ptr(x), ptr(phi), x.numel(), ptr(g), ptr(grad), stream())
    return grad


class _Boundary(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, phi):
        loss, sums = _boundary_fwd(x, phi)
        ctx.save_for_backward(x, phi)
        ctx.mark_non_differentiable(sums)
        ctx.set_materialize_grads(False)
        return loss, sums

    @staticmethod
    def backward(ctx, gout, _gsums):
        if gout is None:
            return None, None
        x, phi = ctx.saved_tensors
        return _boundary_bwd(x, phi, gout), None


def _boundary(inputs, targets, phi, clip, threshold):
    shape, c, thr = _boundary_check(inputs, targets, phi, clip, threshold)
    if inputs.device.type != "cuda":
        raise RuntimeError("vaeunet_amd losses run on MI355X (HIP) devices only")
    as4 = (lambda a: a) if inputs.dim() == 4 else (lambda a: a.unsqueeze(1))
    x4 = as4(inputs)
    if phi is None:
        with torch.no_grad():
            t = as4(targets.to(x4.device))
            if t.dtype not in (torch.uint8, torch.bool, torch.float32):
                t = t.float()
            phi4 = _surface._launch_sdf(_surface._dense(t), thr, False, c)
    else:
        phi4 = as4(phi.detach())
    x, f = _dense_pair(x4, phi4)
    return _Boundary.apply(x, f)


def boundary_loss(inputs, targets=None, *, phi=None, clip=None, threshold=None):
    """The boundary loss of Kervadec et al.: the mean over all
    elements of phi * sigmoid(inputs), phi the signed distance map of the
    ground truth (``surface.signed_distance``: positive outside the mask,
    <= 0 inside).  inputs [B, C, H, W], or [B, H, W] viewed as C = 1, any memory
    format.  Exactly one of ``targets`` (a mask of the inputs' shape: uint8 /
    bool nonzero, anything else ``> threshold``, 0.5 by default; phi is
    computed from it on the device, under ``no_grad``, clamped to [-clip, clip]
    when ``clip`` is given) and ``phi`` (a precomputed float32 map) is given.
    The gradient goes to ``inputs`` only.  An element with a NaN logit or a
    non-finite phi adds nothing and gets gradient 0.  No host synchronisation."""
    return _boundary(inputs, targets, phi, clip, threshold)[0]


class BoundaryLoss(nn.Module):
    """``boundary_loss(inputs, targets, clip=clip)`` as a module."""

    def __init__(self, clip=None):
        super().__init__()
        _surface._check_clip(clip, "BoundaryLoss")
        self.clip = clip

    def forward(self, inputs, targets):
        return boundary_loss(inputs, targets, clip=self.clip)


class BoundaryAugmentedLoss(nn.Module):
    """``base(inputs, targets) + weight * boundary_loss(inputs, targets, clip=clip)``.

    ``weight`` is a scalar buffer that lives on the device of the first batch;
    ``set_weight(v)`` fills it in place, so a schedule that raises the weight
    from epoch to epoch works under graph replay without recapture.  After a
    call, ``self.last_parts`` holds the device tensor [base, boundary]."""

    def __init__(self, base, weight=0.01, clip=None):
        super().__init__()
        if not callable(base):
            raise ValueError(f"BoundaryAugmentedLoss: base must be a loss module or function, got {type(base).__name__}")
        _surface._check_clip(clip, "BoundaryAugmentedLoss")
        self.base = base
        self.clip = clip
        self.register_buffer("weight", torch.tensor(self._check_weight(weight), dtype=torch.float32))
        self.last_parts = None

    @staticmethod
    def _check_weight(v):
        v = float(v)
        if v != v or v in (float("inf"), float("-inf")):
            raise ValueError(f"BoundaryAugmentedLoss: weight must be finite, got {v}")
        return v

    def set_weight(self, v):
        self.weight.fill_(self._check_weight(v))

    def forward(self, inputs, targets):
        _boundary_check(inputs, targets, None, self.clip, None, "BoundaryAugmentedLoss")
        if self.weight.device != inputs.device:
            self.weight = self.weight.to(inputs.device)
        base = self.base(inputs, targets)
        bnd = boundary_loss(inputs, targets, clip=self.clip)
        self.last_parts = torch.stack([base.detach().float(), bnd.detach()])
        return base + self.weight * bnd


class KLAnnealer:
    """KL weight schedule (loss.py:114-145); host arithmetic."""

    def __init__(self, kl_start=0.0, kl_end=1.0, warmup_epochs=10, strategy='linear'):
        self.kl_start = kl_start
        self.kl_end = kl_end
        self.warmup_epochs = warmup_epochs
        self.strategy = strategy

    def get_weight(self, epoch, batch=None, num_batches=None):
        if self.strategy == 'constant':
            return self.kl_end
        if batch is not None and num_batches is not None:
            progress = (epoch + batch / num_batches) / self.warmup_epochs
        else:
            progress = epoch / self.warmup_epochs
        progress = min(progress, 1.0)
        span = self.kl_end - self.kl_start
        if self.strategy == 'linear':
            return self.kl_start + progress * span
        if self.strategy == 'cyclical':
            return self.kl_start + (progress % 1.0) * span
        return self.kl_end


class _KL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, logvar, free_bits):
        B, L = mu.shape
        val = torch.empty((), dtype=torch.float32, device=mu.device)
        call("vu_kl_free_bits2", ptr(mu), ptr(logvar), B, L, free_bits, None, ptr(val), None, None,
             stream())
        ctx.save_for_backward(mu, logvar)
        ctx.fb = free_bits
        return val

    @staticmethod
    def backward(ctx, g):
        mu, logvar = ctx.saved_tensors
        B, L = mu.shape
        gmu = torch.empty_like(mu)
        glv = torch.empty_like(logvar)
        gs = g.float().contiguous()
        call("vu_kl_free_bits2", ptr(mu), ptr(logvar), B, L, ctx.fb, ptr(gs), None, ptr(gmu),
             ptr(glv), stream())
        return gmu, glv, None


def kl_with_free_bits(mu, logvar, free_bits=1e-4):
    """KL(q||N(0,I)) per latent dim, clamp +-100, free-bits floor, sum(1).mean() (loss.py:148-170)."""
    if mu.device.type != "cuda":
        raise RuntimeError("vaeunet_amd losses run on MI355X (HIP) devices only")
    m = mu.float().contiguous()
    v = logvar.float().contiguous()
    if m.dim() != 2:
        m, v = m.reshape(m.shape[0], -1), v.reshape(v.shape[0], -1)
    return _KL.apply(m, v, float(free_bits))
