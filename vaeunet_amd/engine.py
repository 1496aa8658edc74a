"""Fused forward / backward sequences of the reference's building blocks.

Each function here restates, as a sequence of HIP kernel launches, one block
of the reference (file:line cited per function).  The nn.Module classes in
unet_parts.py / unet_model.py / unet_resnet.py own the parameters (same
attribute tree and state_dict keys as the reference) and call these through
torch.autograd.Function wrappers, so ``model(x)``, ``loss.backward()`` and
``optimizer.step()`` stay drop-in.

Parameter gradients are written straight into ``param.grad`` by the weight-
gradient kernels (allocated on first use, accumulated afterwards — the
gradient-accumulation semantics of train.py:401-411); the autograd Functions
return None for parameters.  A ``grad_ready`` hook on the run mode lets the
data-parallel reducer start all-reducing a block's gradients while the
backward of the blocks below it is still running.
"""
import warnings

import torch

from . import kernels as K
from ._lib import BF16, F32


# Weight gradients on a side HIP stream: in every backward the weight-gradient
# GEMM of a layer (and its slab reduce / bias sums) depends only on that
# layer's output gradient and input activation, not on the input-gradient chain
# (dgrad -> BatchNorm backward -> next dgrad) the main stream walks, so it is
# forked onto a second stream and joined once at the end of the block's
# backward.  The GPU then fills CUs left idle by small grids and kernel tails,
# and co-schedules memory-bound BatchNorm passes with MFMA-bound GEMMs where
# registers and LDS allow (a captured HIP graph keeps the fork/join as
# parallel branches).  Measured SLOWER on MI355X (same-box A/B,
# profiles/r3_ab_wgrad_overlap.log: UNet 500.4 -> 491.5, VAE 722.2 -> 687.3
# img/s): the 3x3 GEMMs hold 230-256 VGPRs x 8 waves, so nothing co-resides
# with them and the extra graph edges cost more than the tails they fill.
# Off by default; module-level switch for A/B runs (bench.py --overlap).
OVERLAP_WGRAD = False

# The first stage of a BatchNorm backward reduction (sum dz, sum dz * xhat)
# emitted by the epilogue of the input-gradient GEMM that produces dz's
# source (DoubleConv conv2 -> BN1; the ping-pong kernel and its split-K
# finish), instead of a separate pass over dy and x.  Round 3 measured it
# neutral (profiles/r3_ab_bn_bwd_fusion.log: UNet +0.35 %, VAE -0.4 %): the
# epilogue variant ran the two-halves step loop, not the one-read-segment
# FULL loop of the plain input gradient (+56 us/step of the 172 the fused
# reduction saves, profiles/r6l_*).  Round 6: the epilogue variant on the
# FULL loop (243-246 VGPRs, no spill): UNet +0.38 / +0.40 %, VAE +0.04 /
# -0.02 % in a same-box A/B (profiles/r6m_ab_bn_bwd_fusion.txt).  On by
# default; module-level switch for A/B runs.
FUSE_BN_BWD_REDUCE = True


class SideStream:
    """One side stream per device; ``run`` forks it from the current stream,
    enqueues ``fn`` on it and keeps the tensors the side work reads alive
    until ``join`` (the caching allocator would otherwise hand their blocks
    to the main stream while the side stream still reads them)."""

    _per_device = {}

    def __init__(self, device):
        self.stream = torch.cuda.Stream(device=device)
        self.keep = []
        self.pending = False

    @classmethod
    def get(cls, device):
        key = torch.device(device).index
        if key not in cls._per_device:
            cls._per_device[key] = cls(device)
        return cls._per_device[key]

    def run(self, fn, keep):
        self.stream.wait_stream(torch.cuda.current_stream(self.stream.device))
        with torch.cuda.stream(self.stream):
            r = fn()
        self.keep.extend(keep)
        self.pending = True
        return r

    def join(self):
        if self.pending:
            torch.cuda.current_stream(self.stream.device).wait_stream(self.stream)
            self.keep = []
            self.pending = False


def join_side():
    """Join every device's side stream into its current stream (end of a backward)."""
    for side in SideStream._per_device.values():
        side.join()


class Mode:
    """Per-call execution mode: storage dtype and training flag."""

    def __init__(self, dtype_code, device, grad_ready=None):
        self.d = dtype_code
        self.tdtype = torch.bfloat16 if dtype_code == BF16 else torch.float32
        self.device = device
        self.grad_ready = grad_ready
        self.ov = SideStream.get(device) if OVERLAP_WGRAD else None
        # no backward can follow a forward run with autograd off: eval-mode
        # BatchNorms may then fold into their convolutions (fold_bn_eval)
        self.infer = not torch.is_grad_enabled()

    def side(self, fn, *keep):
        """Run ``fn`` (weight-gradient launches) on the side stream, reading
        the tensors ``keep``; inline when overlap is off."""
        if self.ov is None:
            return fn()
        return self.ov.run(fn, keep)

    def join(self):
        if self.ov is not None:
            self.ov.join()

    def act(self, N, Cc, H, W):
        return K.empty_act(N, Cc, H, W, self.tdtype, self.device)

    def zeros(self, N, Cc, H, W):
        return K.zeros_act(N, Cc, H, W, self.tdtype, self.device)

    def notify(self, params):
        """Tell the DP reducer these gradients are final.  Its collectives wait
        on the stream current at the call, so with overlap on the call is made
        on the side stream, behind the weight-gradient launches."""
        if self.grad_ready is None:
            return
        ready = lambda: self.grad_ready([p for p in params if p is not None and p.grad is not None])  # noqa: E731
        if self.ov is None or torch.cuda.current_stream(self.ov.stream.device) == self.ov.stream:
            ready()
        else:
            self.ov.run(ready, ())


_FP16_WARNED = False


def current_mode(device, grad_ready=None):
    """bf16 under torch.autocast (train.py:385), fp32 otherwise (parity).

    The reference's ``torch.autocast('cuda')`` defaults to float16 (with a
    GradScaler).  The kernels have no fp16 storage path: an fp16 autocast
    region runs in bf16 (same 16-bit storage, 8-bit exponent, no overflow
    risk) and says so once.  GradScaler keeps working: it only scales the
    loss and unscales fp32 gradients."""
    global _FP16_WARNED
    if device.type != "cuda":
        raise RuntimeError("vaeunet_amd runs on MI355X (HIP) devices only; got "
                           f"a tensor on {device}")
    ac = torch.is_autocast_enabled("cuda")
    if ac and torch.get_autocast_dtype("cuda") == torch.float16 and not _FP16_WARNED:
        _FP16_WARNED = True
        warnings.warn("vaeunet_amd: float16 autocast requested; the HIP kernels compute this "
                      "region with bf16 storage (fp32 accumulation) instead")
    return Mode(BF16 if ac else F32, device, grad_ready)


# ----------------------------------------------------------------------------
# weight preparation (derived, version-keyed caches; the fp32 parameter stays
# the single source of truth so state_dict / optimizer semantics are intact)
# ----------------------------------------------------------------------------
def _cached(p, key, build):
    cache = p.__dict__.setdefault("_vu_cache", {})
    p.__dict__.setdefault("_vu_build", {})[key] = build
    ent = cache.get(key)
    ver = (p._version, p.data_ptr())
    if ent is None or ent[0] != ver:
        ent = (ver, build())
        cache[key] = ent
    return ent[1]


class StaticRefresh:
    """Every derived weight image of ``params`` rebuilt IN PLACE by one
    prebuilt vu_permute4_batch2 call (no allocation, no host upload): what a
    captured HIP graph of the training step replays at its start.  Built
    after a warm-up step, when every image the step uses exists."""

    def __init__(self, params):
        self.entries = []
        with K.record_permutes() as rec:
            for p in params:
                builders = p.__dict__.get("_vu_build")
                if not builders:
                    continue
                cache = p.__dict__["_vu_cache"]
                for key, build in builders.items():
                    n0 = len(rec.jobs)
                    build()
                    if len(rec.jobs) != n0 + 1:
                        raise RuntimeError("StaticRefresh: an image build must be one permute")
                    src, base, strides, dims, d3v, out, dtype = rec.jobs[n0]
                    img = cache[key][1]
                    if img.numel() < out.numel() or not img.is_contiguous():
                        raise RuntimeError("StaticRefresh: cached image layout changed")
                    rec.jobs[n0] = (src, base, strides, dims, d3v, img.view(-1)[:out.numel()], dtype)
                    self.entries.append((p, cache, key))
        self.jobs = rec.jobs
        self.table, self.ntap, self.ctap, self.crest = K.job_table(self.jobs) if self.jobs else (None, 0, 0, 0)

    def launch(self):
        if self.jobs:
            K.permute_launch(self.table, len(self.jobs), self.ntap, self.ctap, self.crest)
        for p, cache, key in self.entries:
            cache[key] = ((p._version, p.data_ptr()), cache[key][1])


_STATIC_REFRESH = None  # a StaticRefresh while a graph of the step is captured


def refresh_weights(params):
    """Rebuild every stale derived weight image of ``params`` (those built in
    earlier steps, i.e. after an optimizer step bumped the version) in ONE
    batched launch, instead of one permute launch per image mid-step."""
    if _STATIC_REFRESH is not None:
        _STATIC_REFRESH.launch()
        return
    stale = []
    for p in params:
        builders = p.__dict__.get("_vu_build")
        if not builders:
            continue
        cache = p.__dict__["_vu_cache"]
        ver = (p._version, p.data_ptr())
        for key, build in builders.items():
            ent = cache.get(key)
            if ent is None or ent[0] != ver:
                stale.append((cache, key, build, ver))
    if stale:
        with K.permute_batch():
            for cache, key, build, ver in stale:
                cache[key] = (ver, build())


def w3x3_fwd(w, d, cin_pad=None, cin_use=None):
    """[Cout, Cin, R, S] -> B[Cout][(r*S+s)*Cp + c] (Cp >= Cin zero padded).
    cin_use < Cin: only the first cin_use input channels (Cp = cin_use) -- a
    DecoderBlock conv1 whose z_proj source rides the latent shortcut."""
    co, ci, R, S = w.shape
    nv = cin_use or ci
    cp = cin_use or cin_pad or ci

    def build():
        s = w.stride()
        return K.permute4(w.detach(), 0, (s[0], s[2], s[3], s[1]), (co, R, S, cp), nv, d).view(co, -1)
    return _cached(w, ("w3f", d, cp, nv), build)


def w3x3_dgrad(w, d, rows_pad=None, rows_use=None):
    """Input-gradient weights: B[ci][(r'*S+s')*Cout + co] = W[co][ci][R-1-r'][S-1-s'].
    rows_pad > Cin: zero rows for the padded input channels of a 64-aligned
    concat (a persistent zero-initialised image whose first Cin rows are
    rebuilt each step).  rows_use < Cin: the first rows_use input channels
    only (the latent shortcut, as w3x3_fwd's cin_use)."""
    co, ci, R, S = w.shape
    if rows_use is not None and rows_use < ci:
        def build_sub():
            s = w.stride()
            base = (R - 1) * s[2] + (S - 1) * s[3]
            return K.permute4(w.detach(), base, (s[1], -s[2], -s[3], s[0]), (rows_use, R, S, co), co,
                              d).view(rows_use, -1)
        return _cached(w, ("w3d", d, "use", rows_use), build_sub)
    rp = rows_pad or ci

    def build():
        s = w.stride()
        base = (R - 1) * s[2] + (S - 1) * s[3]
        out = None
        if rp > ci:
            bufs = w.__dict__.setdefault("_vu_pad", {})
            key = ("w3d", d, rp)
            if key not in bufs:
                bufs[key] = torch.zeros((rp, R * S * co), device=w.device,
                                        dtype=torch.bfloat16 if d == BF16 else torch.float32)
            out = bufs[key]
            K.permute4(w.detach(), base, (s[1], -s[2], -s[3], s[0]), (ci, R, S, co), co, d,
                       out=out[:ci].view(ci, R, S, co))
            return out
        return K.permute4(w.detach(), base, (s[1], -s[2], -s[3], s[0]), (ci, R, S, co), co, d).view(ci, -1)
    return _cached(w, ("w3d", d, rp), build)


def w1x1_fwd(w, d):
    co, ci = w.shape[0], w.shape[1]

    def build():
        s = w.stride()
        return K.permute4(w.detach(), 0, (s[0], s[1], 0, 0), (co, ci, 1, 1), 1, d).view(co, ci)
    return _cached(w, ("w1f", d), build)


def w1x1_dgrad(w, d):
    co, ci = w.shape[0], w.shape[1]

    def build():
        s = w.stride()
        return K.permute4(w.detach(), 0, (s[1], s[0], 0, 0), (ci, co, 1, 1), 1, d).view(ci, co)
    return _cached(w, ("w1d", d), build)


def wT_fwd(w, d):
    """ConvTranspose2d weight [Cin, Cout, 2, 2] -> B[(a*2+b)*Cout + co][ci]."""
    ci, co = w.shape[0], w.shape[1]

    def build():
        s = w.stride()
        return K.permute4(w.detach(), 0, (s[2], s[3], s[1], s[0]), (2, 2, co, ci), ci, d).view(4 * co, ci)
    return _cached(w, ("wTf", d), build)


def wT_dgrad(w, d):
    """-> B[ci][(a*2+b)*Cout + co] (gather of the 2x2 output sub-pixels)."""
    ci, co = w.shape[0], w.shape[1]

    def build():
        s = w.stride()
        return K.permute4(w.detach(), 0, (s[0], s[2], s[3], s[1]), (ci, 2, 2, co), co, d).view(ci, 4 * co)
    return _cached(w, ("wTd", d), build)


# ----------------------------------------------------------------------------
# gradient sinks
# ----------------------------------------------------------------------------
def grad_sink(p):
    """(tensor, accumulate) for writing d(loss)/dp, or (None, False) if frozen."""
    if p is None or not p.requires_grad:
        return None, False
    if p.grad is None:
        p.grad = torch.empty_like(p)
        return p.grad, False
    return p.grad, True


def conv_layout(g):
    """wgrad output layout (s_i, s_tap, s_c) of a [Cout, Cin, R, S] gradient."""
    s = g.stride()
    if g.shape[2] > 1 and s[2] != g.shape[3] * s[3]:
        raise ValueError("unsupported weight-gradient strides")
    return (s[0], s[3], s[1])


def convT_layout(g):
    s = g.stride()
    if s[2] != 2 * s[3]:
        raise ValueError("unsupported ConvTranspose weight-gradient strides")
    return (s[0], s[3], s[1])


def wgrad3x3(dy, srcs, w, M, cvalid=None, sink=None):
    """sink: a (grad, accumulate) taken by the caller -- when another kernel
    writes other input channels of the same gradient (the latent shortcut)."""
    g, acc = sink if sink is not None else grad_sink(w)
    if g is None:
        return
    co = dy.shape[1]
    cin = sum(s.shape[1] for s in srcs)
    K.gemm_wgrad(K.gather1x1([dy]), K.gather3x3(srcs), co, 9 * cin, g, conv_layout(g), M.d, acc,
                 cvalid=cvalid)


def wgrad1x1(dy, srcs, w, M):
    g, acc = grad_sink(w)
    if g is None:
        return
    cin = sum(s.shape[1] for s in srcs)
    K.gemm_wgrad(K.gather1x1([dy]), K.gather1x1(srcs), dy.shape[1], cin, g, conv_layout(g), M.d, acc)


def bias_grad(dy, b, M, window=None, bn=None):
    """d(loss)/d(conv bias) = per-channel sum of dy.  When the conv feeds a
    TRAIN-mode BatchNorm (``bn``), BN(x + b) does not depend on b (the batch
    mean absorbs it), so the gradient is exactly zero: it is written as zeros
    instead of summing a zero-mean map (autograd's sum leaves only rounding
    noise there).  Eval-mode BN and plain consumers get the real sum."""
    g, acc = grad_sink(b)
    if g is None:
        return
    if bn is not None and bn.training:
        if not acc:
            K.call("vu_zero", K.ptr(g), 0, 1, g.numel(), K.dcode(g.dtype), K.stream())
        return
    K.chan_sum(dy, g, acc, M.d, window)


# ----------------------------------------------------------------------------
# BatchNorm2d: stats from the GEMM epilogue -> (scale, shift, mean, invstd)
# ----------------------------------------------------------------------------
def bn_running_args(bn):
    """(running_mean, running_var, num_batches_tracked, momentum) of a
    train-mode BatchNorm for the finalize kernels: None / 0.0 when it tracks no
    running statistics."""
    if not (bn.track_running_stats and bn.running_mean is not None):
        return None, None, None, 0.0
    return bn.running_mean, bn.running_var, bn.num_batches_tracked, 0.1 if bn.momentum is None else bn.momentum


def bn_coef(bn, st, C_):
    if bn.training:
        if st is None:
            raise RuntimeError("train-mode BatchNorm needs GEMM statistics")
        return K.bn_finalize(st, C_, bn.weight, bn.bias, *bn_running_args(bn), bn.eps)
    return K.bn_eval(C_, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)


FUSED_BN_FWD = True  # small train-mode BatchNorms as one finalize + apply launch (A/B switch)
FUSED_BN_BWD = True  # small BatchNorm backwards: finish folded into the apply pass (A/B switch)
# bf16 input gradients of 3x3 / stride-2 convs as one stride-1 conv over the
# zero-inserted output gradient (vu_zero_insert2) instead of four parity-class
# GEMMs (A/B switch; vae_engine.conv_dgrad)
S2_ZERO_INSERT_DGRAD = True


def bn_fwd_apply(bn, st, y, a, relu, M, res=None, rcoef=None):
    """Train/eval BatchNorm of y into a: a = relu?(BN(y) [+ BN_r(res) | + res]);
    returns coef.  Small train-mode tensors take the single-launch fused path
    (kernels.bn_forward_fused); otherwise finalize (bn_coef) + the apply."""
    C_ = y.shape[1]
    if FUSED_BN_FWD and bn.training and st is not None:
        coef = K.bn_forward_fused(st, C_, bn.weight, bn.bias, *bn_running_args(bn), bn.eps,
                                  y, a, relu, M.d, res=res, rcoef=rcoef)
        if coef is not None:
            return coef
    coef = bn_coef(bn, st, C_)
    if res is None:
        K.bn_apply(y, a, coef, relu, M.d)
    else:
        if not relu:
            raise ValueError("bn_fwd_apply: the residual form always applies ReLU (vu_bn_add_relu)")
        N, _, H, W = y.shape
        K.call("vu_bn_add_relu", K.ptr(y), K.pstride(y), K.ptr(coef[0]), K.ptr(coef[1]), K.ptr(res),
               K.pstride(res), K.ptr(rcoef[0]) if rcoef is not None else None,
               K.ptr(rcoef[1]) if rcoef is not None else None, N * H * W, C_, K.ptr(a), K.pstride(a),
               M.d, K.stream())
    return coef


def bn_grad_sinks(bn):
    gw, accw = grad_sink(bn.weight)
    gb, accb = grad_sink(bn.bias)
    if gw is not None and gb is not None and accw != accb:
        raise RuntimeError("inconsistent BatchNorm grad state")
    return gw, gb, accw or accb


def bn_bwd_finish(x, coef, bn, part):
    """The fp64 finish of a BatchNorm backward whose first reduction stage
    (part, a BnbPart) a producing kernel emitted: dgamma / dbeta into the grad
    sinks; returns the apply coefficients k."""
    gw, gb, acc = bn_grad_sinks(bn)
    return K.bn_backward_finish(part, x, coef, bn.weight, gw, gb, acc, train=bn.training)


def bn_bwd(dy, x, coef, bn, relu, M, dx=None, part=None, zrs=None):
    """BatchNorm2d(+ReLU) backward.  Train mode differentiates through the
    batch statistics; eval mode (running statistics, constants) gives
    dx = gamma*invstd*dz and the same dgamma/dbeta sums.  part: the first
    reduction stage, already emitted by the GEMM that produced dy.  zrs: a
    latent shortcut's K.ZbiasRegions, filled by the apply pass when it serves."""
    if dx is None:
        dx = torch.empty_like(x)
    if part is not None and part.x is x:
        k = bn_bwd_finish(x, coef, bn, part)
        K.bn_backward_apply(dy, x, coef, k, relu, dx, K.dcode(x.dtype), zrs)
    else:
        gw, gb, acc = bn_grad_sinks(bn)
        K.bn_backward(dy, x, coef, bn.weight, relu, gw, gb, acc, dx, K.dcode(x.dtype),
                      train=bn.training, fused=FUSED_BN_BWD, zrs=zrs)
    return dx


def bn_bwd_pair(dy, a, b, M):
    """Backward of two BatchNorms (no ReLU) fed by the same dy, each
    a / b = (x, coef, bn, BnbPart): both fp64 finishes, then one apply pass
    that reads dy once (vu_bn_bwd_apply2; the attention gate's W_g / W_x
    BatchNorms, round 6).  Returns (dx_a, dx_b)."""
    ka, kb = bn_bwd_finish(*a), bn_bwd_finish(*b)
    (xa, ca, _, _), (xb, cb, _, _) = a, b
    dxa, dxb = torch.empty_like(xa), torch.empty_like(xb)
    if not K.bn_backward_apply2(dy, xa, ca, ka, dxa, xb, cb, kb, dxb, K.dcode(xa.dtype)):
        K.bn_backward_apply(dy, xa, ca, ka, False, dxa, K.dcode(xa.dtype))
        K.bn_backward_apply(dy, xb, cb, kb, False, dxb, K.dcode(xb.dtype))
    return dxa, dxb


# ----------------------------------------------------------------------------
# DoubleConv  (unet_parts.py:32-49; DecoderBlock conv1/conv2 unet_resnet.py:59-69)
#   conv3x3(no bias) -> BN -> ReLU -> conv3x3(no bias) -> BN -> ReLU
# ----------------------------------------------------------------------------
# Inference (autograd off) with an eval-mode BatchNorm after a convolution:
# the BN's affine map folds into the convolution (weight rows scaled, bias
# shifted) and the ReLU runs in the GEMM epilogue, so conv + BN + ReLU is one
# pass instead of two (visualize_vae.py:61-87,578-652 run the model this way
# for every latent sample).  A/B switch.
FOLD_BN_EVAL = True


def can_fold(M, bn):
    return FOLD_BN_EVAL and M.infer and not bn.training and bn.track_running_stats \
        and bn.running_mean is not None


def fold_bn_eval(M, conv, bn, cin_pad=None, cin_use=None):
    """(weight image, bias) of ``conv`` followed by the eval-mode ``bn``:
    rows of the fp32 image scaled by gamma / sqrt(running_var + eps), bias
    (conv bias) * scale + beta - running_mean * scale; storage dtype image.
    Rebuilt per call (the running statistics are written in place by the
    train-mode kernels, so no version counter would tell a cache)."""
    co = conv.out_channels
    coef = bn_coef(bn, None, co)                    # eval rows: scale, shift
    img = w3x3_fwd(conv.weight, F32, cin_pad, cin_use)  # [co][R*S*Cp] fp32, cached
    w = img * coef[0][:, None]
    if M.d != F32:
        w = w.to(torch.bfloat16)
    b = coef[1] if conv.bias is None else conv.bias.float() * coef[0] + coef[1]
    return w, b.contiguous()


def conv_bn_relu_fwd(M, srcs, conv, bn, cin_pad=None, defer=False, zbias=None, cin_use=None):
    """defer: leave BN + ReLU unapplied (returns a = None) when the consumer
    is a MaxPool2d that applies it in the same pass (down_fwd); defer="any":
    for any consumer that applies it itself (the OutConv kernel, outconv_fwd).
    zbias / cin_use: the latent shortcut of a DecoderBlock conv1 (the conv
    contracts over the first cin_use input channels; VuGemmFwd.zbias adds the
    rest)."""
    N, _, H, W = srcs[0].shape
    co = conv.out_channels
    if can_fold(M, bn) and not defer:
        wf, bf = fold_bn_eval(M, conv, bn, cin_pad, cin_use)
        a = M.act(N, co, H, W)
        K.gemm_fwd(K.gather3x3(srcs), wf, co, a, M.d, bias=bf, relu=True, zbias=zbias)
        return a, None
    y = M.act(N, co, H, W)
    st = K.gemm_fwd(K.gather3x3(srcs), w3x3_fwd(conv.weight, M.d, cin_pad, cin_use), co, y, M.d,
                    stats=bn.training, zbias=zbias)
    if defer == "any" or (defer and K.pool_fusable(y)):
        return None, (y, bn_coef(bn, st, co))
    a = M.act(N, co, H, W)
    coef = bn_fwd_apply(bn, st, y, a, True, M)
    return a, (y, coef)


# The first convolution of the network (inc.double_conv[0]) needs no input
# gradient, so its weight gradient is the only reader of dy = the BN1 backward
# apply's output: the apply then runs in that weight gradient's operand path
# (vu_conv_image_wgrad_bn) and dy is never stored.  dgamma, dbeta and the
# apply coefficients come from the same reduce / finish launches as before.
# Where dy is stored anyway (the caller wants the image's gradient, or a small
# tensor takes vu_bn_bwd_fused) the same kernel runs over it without the
# transform.  Module-level switch for A/B runs (bench.py --engine-flag): off,
# the image weight gradient is vu_gemm_wgrad's as before.
FUSE_IMAGE_WGRAD_BN = True


def _image_wgrad_kernel_serves(M, srcs, conv, shortcut, da, y):
    """conv_image_wgrad.hip runs this weight gradient (da, y: the BatchNorm's
    output gradient and input, or the stored dy twice)."""
    if not FUSE_IMAGE_WGRAD_BN or shortcut is not None or M.d != BF16 or K.AUDIT is not None:
        return False
    if len(srcs) != 1 or not conv.weight.requires_grad:
        return False
    return K.image_wgrad_bn_ok(da, y, srcs[0], M.d)


def _image_wgrad_bn_serves(M, srcs, conv, bn, y, da, need_dsrc, da_part, shortcut):
    if need_dsrc or (da_part is not None and da_part.x is not y):
        return False
    N, Cc, H, W = y.shape
    # small tensors without epilogue partials take vu_bn_bwd_fused, which keeps
    # its own reduction: they stay on it (dgamma / dbeta exactly as before)
    if da_part is None and FUSED_BN_BWD and K.query("vu_bn_bwd_fused_supported", N * H * W, Cc, K.pstride(da),
                                                    K.pstride(y), Cc):
        return False
    return _image_wgrad_kernel_serves(M, srcs, conv, shortcut, da, y)


def _image_wgrad_bn(M, srcs, conv, bn, y, coef, da, cvalid, da_part):
    if da_part is not None:
        k = bn_bwd_finish(y, coef, bn, da_part)
    else:
        gw, gb, acc = bn_grad_sinks(bn)
        k = K.bn_backward_reduce(da, y, coef, bn.weight, True, gw, gb, acc, M.d, train=bn.training)

    def wg():
        g, gacc = grad_sink(conv.weight)
        K.image_wgrad_bn(da, y, coef, k, True, srcs[0], g, conv_layout(g), gacc, cvalid=cvalid)
        M.notify([bn.weight, bn.bias, conv.weight])
    M.side(wg, da, y, k, *srcs)


def conv_bn_relu_bwd(M, srcs, conv, bn, saved, da, need_dsrc, cvalid=None, dsrc=None, dsrc_acc=False,
                     cin_pad=None, da_part=None, feeds=None, shortcut=None):
    """cin_pad: compute the input gradient for cin_pad channels (zero weight
    rows past conv.in_channels) so that its column count stays a tile
    multiple; the caller reads the real channels only.
    shortcut: the latent shortcut of a DecoderBlock conv1 (vae_engine.ZShortcut):
    srcs are its first shortcut.lead input channels; their weight gradient is
    written through shortcut.sink; dy (the pre-BN gradient) is kept for the
    shortcut's backward, which writes the z columns and then reports the
    weight to the DP reducer.
    da_part: BatchNorm-backward partials of ``da`` from the GEMM that made it.
    feeds=(saved, bn) of the BN(+ReLU) the input gradient feeds (the previous
    conv's): its first backward reduction stage then rides this input-gradient
    GEMM's epilogue, returned as (dsrc, part) -- part None when the kernel
    cannot."""
    y, coef = saved
    if _image_wgrad_bn_serves(M, srcs, conv, bn, y, da, need_dsrc, da_part, shortcut):
        _image_wgrad_bn(M, srcs, conv, bn, y, coef, da, cvalid, da_part)
        return None
    zrs = shortcut.regions(y) if shortcut is not None else None
    dy = bn_bwd(da, y, coef, bn, True, M, part=da_part, zrs=zrs)
    if shortcut is not None:
        shortcut.dy = dy

    def wg():
        if _image_wgrad_kernel_serves(M, srcs, conv, shortcut, dy, dy):
            g, gacc = grad_sink(conv.weight)
            K.image_wgrad_bn(dy, None, None, None, False, srcs[0], g, conv_layout(g), gacc, cvalid=cvalid)
        else:
            wgrad3x3(dy, srcs, conv.weight, M, cvalid, sink=shortcut.sink if shortcut is not None else None)
        M.notify([bn.weight, bn.bias] + ([conv.weight] if shortcut is None else []))
    M.side(wg, dy, *srcs)
    if not need_dsrc:
        return None
    N, _, H, W = y.shape
    # a channel-padded input (the 3-channel image) gets a gradient for its
    # real channels only: the dgrad weights have conv.in_channels rows
    cin = shortcut.lead if shortcut is not None else (cin_pad or conv.in_channels)
    if dsrc is None:
        dsrc = M.act(N, cin, H, W)
    bnb = None
    if feeds is not None and FUSE_BN_BWD_REDUCE:
        (fy, fcoef), fbn = feeds
        bnb = (fy, fcoef, True)
    wd = w3x3_dgrad(conv.weight, M.d, rows_use=cin) if shortcut is not None else w3x3_dgrad(conv.weight, M.d, cin)
    part = K.gemm_fwd(K.gather3x3([dy]), wd, cin, dsrc, M.d, accumulate=dsrc_acc, kind="dgrad", bnb=bnb)
    if feeds is not None:
        return dsrc, part
    return dsrc


def double_conv_fwd(M, seq, srcs, cin_pad=None, defer=False):
    """defer: the output feeds a Down (down_fwd applies BN2 + ReLU fused with
    its max-pool); a2 is then None and saved[3] = (y2, coef2)."""
    conv1, bn1, _, conv2, bn2, _ = seq
    a1, s1 = conv_bn_relu_fwd(M, srcs, conv1, bn1, cin_pad)
    a2, s2 = conv_bn_relu_fwd(M, [a1], conv2, bn2, defer=defer)
    return a2, (srcs, a1, s1, s2)


def double_conv_bwd(M, seq, saved, da2, need_dsrc, cvalid=None, da2_part=None):
    """da2_part: BN2's first backward reduction stage, emitted by the kernel
    that produced da2 (outconv_bwd with a deferred BN2)."""
    conv1, bn1, _, conv2, bn2, _ = seq
    srcs, a1, s1, s2 = saved
    # conv2's input gradient also emits BN1's first backward reduction stage
    da1, part = conv_bn_relu_bwd(M, [a1], conv2, bn2, s2, da2, True, feeds=(s1, bn1), da_part=da2_part)
    return conv_bn_relu_bwd(M, srcs, conv1, bn1, s1, da1, need_dsrc, cvalid, da_part=part)


# ----------------------------------------------------------------------------
# Down (unet_parts.py:51-63): MaxPool2d(2) -> DoubleConv
# ----------------------------------------------------------------------------
def down_fwd(M, mod, x, pend=None, defer=False):
    """x: the input activation, or None with pend = (y, coef) of the producing
    DoubleConv's unapplied BN2 -- then BN + ReLU and the 2x2 max-pool run as
    one pass (vu_bn_apply_maxpool2) that also materialises x (the skip
    connection).  defer: this Down's own output feeds another Down.
    Returns (x, out, saved)."""
    seq = mod.maxpool_conv[1].double_conv
    if x is None:
        y, coef = pend
        N, C_, H, W = y.shape
        x = M.act(N, C_, H, W)
        xp = M.act(N, C_, H // 2, W // 2)
        K.bn_apply_maxpool(y, x, xp, coef, True, M.d)
    else:
        xp = K.maxpool_fwd(x, M.d)
    out, sdc = double_conv_fwd(M, seq, [xp], defer=defer)
    return x, out, (x, sdc)


def down_bwd(M, mod, saved, dout, add=None):
    """d(loss)/d(this Down's input): the max-pool backward of the pooled
    gradient plus add, the skip gradient.  (A max-pool backward carrying the
    producing BN's backward reduction, and that BN's backward read through the
    pool, both measured slower than these separate passes: DESIGN.md §4.2.)"""
    x, sdc = saved
    seq = mod.maxpool_conv[1].double_conv
    dxp = double_conv_bwd(M, seq, sdc, dout, True)
    dx = torch.empty_like(x)
    K.maxpool_bwd(x, dxp, dx, add, M.d)
    return dx


# ----------------------------------------------------------------------------
# AttentionGate (unet_parts.py:7-30): x * sigmoid(BN(psi(relu(BN(W_g g) + BN(W_x x)))))
# ----------------------------------------------------------------------------
# Round 6: the attention psi backward emits the first backward-reduction
# stage of the W_g and W_x BatchNorms (vu_attn_psi_bwd_bnb).  A/B switch.
FUSE_ATTN_BN_REDUCE = True
# Everything after the psi backward's reductions -- ds, both BatchNorm applies,
# both 1x1 input gradients, the dout * psi term of dx -- as one stream over the
# pixels (vu_attn_tail_bwd): ds and the first dx are never written, dug / dux
# are written once and not read back by the input-gradient GEMMs.  A/B switch.
FUSE_ATTN_TAIL = True
# the fused tail is a persistent stream kernel: it serves a gate with at least
# this many wave tiles per compute unit (the floor of the stream 1x1 GEMMs it
# replaces; smaller gates keep the separate kernels)
ATTN_TAIL_MIN_TILES_PER_CU = 8


def _attn_tail_ok(M, P, F, g, x, dout, dg_out, wdg, wdx, dx):
    if not FUSE_ATTN_TAIL or M.d != BF16 or dg_out is None or g.shape[1] != x.shape[1]:
        return False
    C_ = x.shape[1]
    dst, coff = dg_out
    if not K.query("vu_attn_tail_bwd_ok", P, F, C_, wdg.shape[-1], wdx.shape[-1], K.pstride(dout),
                   K.pstride(dst), coff, K.pstride(dx), M.d):
        return False
    cus = torch.cuda.get_device_properties(x.device).multi_processor_count
    return P // K.query("vu_attn_tail_bwd_tile", F, C_) >= ATTN_TAIL_MIN_TILES_PER_CU * cus


def attention_fwd(M, att, g, x):
    N, _, H, W = x.shape
    P = N * H * W
    wg, bng = att.W_g[0], att.W_g[1]
    wx, bnx = att.W_x[0], att.W_x[1]
    wp, bnp = att.psi[0], att.psi[1]
    F = wg.out_channels
    ug = M.act(N, F, H, W)
    stg = K.gemm_fwd(K.gather1x1([g]), w1x1_fwd(wg.weight, M.d), F, ug, M.d, bias=wg.bias,
                     stats=bng.training)
    ux = M.act(N, F, H, W)
    stx = K.gemm_fwd(K.gather1x1([x]), w1x1_fwd(wx.weight, M.d), F, ux, M.d, bias=wx.bias,
                     stats=bnx.training)
    cg = bn_coef(bng, stg, F)
    cx = bn_coef(bnx, stx, F)
    tile = K.query("vu_attn_tile_rows")
    tiles = (P + tile - 1) // tile
    q = torch.empty((N, 1, H, W), dtype=torch.float32, device=x.device)
    psum = torch.empty(tiles, dtype=torch.float32, device=x.device)
    pm2 = torch.empty_like(psum)
    K.call("vu_attn_psi_fwd", K.ptr(ug), K.ptr(ux), P, F, K.ptr(cg[0]), K.ptr(cg[1]), K.ptr(cx[0]),
           K.ptr(cx[1]), K.ptr(wp.weight), K.ptr(wp.bias), K.ptr(q), K.ptr(psum), K.ptr(pm2), tile,
           M.d, K.stream())
    cq = bn_coef(bnp, K.Stats(psum.view(tiles, 1), pm2.view(tiles, 1), tiles, tile, P), 1)
    pmap = torch.empty((N, 1, H, W), dtype=torch.float32, device=x.device)
    out = M.act(N, x.shape[1], H, W)
    K.call("vu_attn_gate_fwd", K.ptr(q), K.ptr(cq), K.ptr(x), K.pstride(x), P, x.shape[1],
           K.ptr(pmap), K.ptr(out), K.pstride(out), M.d, K.stream())
    _fire_psi_hooks(att.psi, pmap)
    return out, (g, x, ug, ux, cg, cx, q, cq, pmap)


def _fire_psi_hooks(psi, pmap):
    """analyze_model.py:733-736 hooks AttentionGate.psi; keep them firing."""
    if psi._forward_hooks:
        for hook in list(psi._forward_hooks.values()):
            hook(psi, (None,), pmap)


def attention_bwd(M, att, saved, dout, dg_out, dg_acc):
    """Returns dx (skip gradient); adds the gate-input gradient into dg_out."""
    g, x, ug, ux, cg, cx, q, cq, pmap = saved
    N, _, H, W = x.shape
    P = N * H * W
    wg, bng = att.W_g[0], att.W_g[1]
    wx, bnx = att.W_x[0], att.W_x[1]
    wp, bnp = att.psi[0], att.psi[1]
    F = wg.out_channels
    dx = torch.empty_like(x)
    dbnq = torch.empty((N, 1, H, W), dtype=torch.float32, device=x.device)
    bnb = FUSE_ATTN_BN_REDUCE and K.query("vu_attn_psi_bwd_bnb_ok", F)
    tail = bool(bnb) and _attn_tail_ok(M, P, F, g, x, dout, dg_out, w1x1_dgrad(wg.weight, M.d),
                                       w1x1_dgrad(wx.weight, M.d), dx)
    # (fused tail: dx = dout * psi is formed there, not stored here)
    K.call("vu_attn_gate_bwd", K.ptr(dout), K.pstride(dout), K.ptr(x), K.pstride(x), K.ptr(pmap),
           P, x.shape[1], None if tail else K.ptr(dx), K.pstride(dx), K.ptr(dbnq), M.d, K.stream())
    # BatchNorm2d(1) backward (fp32 single channel)
    gw, accw = grad_sink(bnp.weight)
    gb, _ = grad_sink(bnp.bias)
    dq = torch.empty_like(q)
    K.bn_backward(dbnq, q, cq, bnp.weight, False, gw, gb, accw, dq, F32, train=bnp.training)
    # psi conv + ReLU backward -> ds (grad of g1 + x1)
    ds = None if tail else M.act(N, F, H, W)
    gwp, accp = grad_sink(wp.weight)
    gbp, _ = grad_sink(wp.bias)
    ws = K.workspace_f32(K.query("vu_attn_psi_bwd_workspace_bytes", P, F), x.device)
    pg = px = None
    if bnb:
        # the psi backward also emits both BatchNorms' first reduction stage
        # (round 6): no separate reduction passes over (ds, ug) and (ds, ux)
        nb = K.query("vu_attn_psi_bwd_blocks", P)
        bg = torch.empty((nb, 2, F), dtype=torch.float32, device=x.device)
        bx = torch.empty_like(bg)
        K.call("vu_attn_psi_bwd_bnb", K.ptr(ug), K.ptr(ux), P, F, K.ptr(cg[0]), K.ptr(cg[1]),
               K.ptr(cx[0]), K.ptr(cx[1]), K.ptr(wp.weight), K.ptr(dq), None if tail else K.ptr(ds),
               K.ptr(gwp), K.ptr(gbp), 1 if accp else 0, K.ptr(ws), K.ptr(cg[2]), K.ptr(cg[3]), K.ptr(cx[2]),
               K.ptr(cx[3]), K.ptr(bg), K.ptr(bx), M.d, K.stream())
        pg, px = K.BnbPart(bg, nb, ug), K.BnbPart(bx, nb, ux)
    else:
        K.call("vu_attn_psi_bwd", K.ptr(ug), K.ptr(ux), P, F, K.ptr(cg[0]), K.ptr(cg[1]),
               K.ptr(cx[0]), K.ptr(cx[1]), K.ptr(wp.weight), K.ptr(dq), K.ptr(ds), K.ptr(gwp),
               K.ptr(gbp), 1 if accp else 0, K.ptr(ws), M.d, K.stream())
    if tail:
        # both fp64 finishes (bn_bwd_pair's), then the one pass
        ks = [bn_bwd_finish(ug, cg, bng, pg), bn_bwd_finish(ux, cx, bnx, px)]
        dug, dux = torch.empty_like(ug), torch.empty_like(ux)
        wdg, wdx = w1x1_dgrad(wg.weight, M.d), w1x1_dgrad(wx.weight, M.d)
        dst, coff = dg_out

        def run_tail():
            K.call("vu_attn_tail_bwd", K.ptr(ug), K.ptr(ux), K.ptr(dq), P, F, x.shape[1], K.ptr(cg[0]),
                   K.ptr(cg[1]), K.ptr(cx[0]), K.ptr(cx[1]), K.ptr(wp.weight), K.ptr(cg[2]), K.ptr(ks[0]),
                   K.ptr(cx[2]), K.ptr(ks[1]), K.ptr(wdg), wdg.shape[-1], K.ptr(wdx), wdx.shape[-1],
                   K.ptr(dout), K.pstride(dout), K.ptr(pmap), K.ptr(dst), K.pstride(dst), coff,
                   1 if dg_acc else 0, K.ptr(dx), K.pstride(dx), K.ptr(dug), K.ptr(dux), M.d, K.stream())
        if K.AUDIT is None:
            run_tail()
        else:
            # a GEMM audit sees the two input-gradient GEMMs inside the one
            # launch: dg (+)= dug W_g, and dx = (dout * psi) + dux W_x with the
            # accumulate operand -- what the gate backward would have stored
            # -- put into dx beforehand
            dx.copy_(dout.float() * pmap)
            K.audited_gemm(K.gather1x1([dug]), wdg, g.shape[1], dst, M.d, coff, dg_acc,
                           lambda: K.audited_gemm(K.gather1x1([dux]), wdx, x.shape[1], dx, M.d, 0, True, run_tail))
    elif pg is not None:
        dug, dux = bn_bwd_pair(ds, (ug, cg, bng, pg), (ux, cx, bnx, px), M)
    else:
        dug = bn_bwd(ds, ug, cg, bng, False, M)
        dux = bn_bwd(ds, ux, cx, bnx, False, M)

    def wgs():
        wgrad1x1(dug, [g], wg.weight, M)
        bias_grad(dug, wg.bias, M, bn=bng)
        wgrad1x1(dux, [x], wx.weight, M)
        bias_grad(dux, wx.bias, M, bn=bnx)
        M.notify([wg.weight, wg.bias, wx.weight, wx.bias, wp.weight, wp.bias, bng.weight, bng.bias,
                  bnx.weight, bnx.bias, bnp.weight, bnp.bias])
    M.side(wgs, dug, dux, g, x)
    if tail:
        return dx
    # input gradients of the two 1x1 convs
    if dg_out is not None:
        dst, coff = dg_out
        K.gemm_fwd(K.gather1x1([dug]), w1x1_dgrad(wg.weight, M.d), g.shape[1], dst, M.d,
                   out_coff=coff, accumulate=dg_acc)
    K.gemm_fwd(K.gather1x1([dux]), w1x1_dgrad(wx.weight, M.d), x.shape[1], dx, M.d, accumulate=True)
    return dx


# ----------------------------------------------------------------------------
# Up (unet_parts.py:65-95): up(x1) -> F.pad -> attention(x1, x2) -> cat([x2, x1]) -> DoubleConv
# ----------------------------------------------------------------------------
def up_fwd(M, mod, x1, x2, defer_out=False):
    """defer_out: leave the DoubleConv's BN2 + ReLU unapplied (out None; its
    (y2, coef2) is saved[5][3]) for a consumer that applies it itself."""
    N, _, H, W = x2.shape
    h, w = x1.shape[2], x1.shape[3]
    bilinear = isinstance(mod.up, torch.nn.Upsample)
    uh, uw = 2 * h, 2 * w
    dy_, dx_ = H - uh, W - uw
    # F.pad(x1, [dx//2, dx - dx//2, dy//2, dy - dy//2]): the upsampled map sits
    # at (dy//2, dx//2) of the skip-sized canvas; a negative offset crops
    py, px = dy_ // 2, dx_ // 2
    crop = dy_ < 0 or dx_ < 0
    if bilinear:
        cu = x1.shape[1]
        u = M.act(N, cu, H, W)
        K.upsample_fwd(x1, u, uh, uw, py, px, M.d)
    else:
        cu = mod.up.out_channels
        if crop:
            # full ConvT map, then an exact shifted copy into the canvas (the
            # align_corners resampler at scale 1 with the pad offsets)
            uf = M.act(N, cu, uh, uw)
            K.gemm_fwd(K.gather1x1([x1]), wT_fwd(mod.up.weight, M.d), 4 * cu, uf, M.d,
                       bias=mod.up.bias, convT=(uh, uw, 0, 0, cu))
            u = M.act(N, cu, H, W)
            K.upsample_fwd(uf, u, uh, uw, py, px, M.d)
        else:
            u = M.zeros(N, cu, H, W) if (dy_ or dx_) else M.act(N, cu, H, W)
            K.gemm_fwd(K.gather1x1([x1]), wT_fwd(mod.up.weight, M.d), 4 * cu, u, M.d,
                       bias=mod.up.bias, convT=(H, W, py, px, cu))
    x2a, satt = attention_fwd(M, mod.attention, u, x2)
    out, sdc = double_conv_fwd(M, mod.conv.double_conv, [x2a, u], defer="any" if defer_out else False)
    return out, (x1, x2, u, (py, px, uh, uw), satt, sdc)


def up_bwd(M, mod, saved, dout, dout_part=None):
    x1, x2, u, (py, px, uh, uw), satt, sdc = saved
    N, cs, H, W = x2.shape
    cu = u.shape[1]
    dcat = double_conv_bwd(M, mod.conv.double_conv, sdc, dout, True, da2_part=dout_part)
    dx2a = dcat[:, :cs]
    du = dcat[:, cs:]
    dx2 = attention_bwd(M, mod.attention, satt, dx2a, (dcat, cs), True)
    h, w = x1.shape[2], x1.shape[3]
    if isinstance(mod.up, torch.nn.Upsample):
        dx1 = torch.empty_like(x1)
        K.upsample_bwd(du, dx1, uh, uw, py, px, False, M.d)
    else:
        if py < 0 or px < 0:
            # gradient of the crop: scatter du back onto the full ConvT map
            duf = M.act(N, cu, uh, uw)
            K.upsample_bwd(du, duf, uh, uw, py, px, False, M.d)
            du, py, px = duf, 0, 0
            H, W = uh, uw
        def wgt(du=du, H=H, W=W, py=py, px=px):
            g, acc = grad_sink(mod.up.weight)
            if g is not None:
                K.gemm_wgrad(K.gather1x1([x1]), K.gather_convT(du, N, h, w, py, px), x1.shape[1], 4 * cu,
                             g, convT_layout(g), M.d, acc)
            bias_grad(du, mod.up.bias, M, window=(py, px, uh, uw))
            M.notify([mod.up.weight, mod.up.bias])
        M.side(wgt, du, x1, dcat)
        dx1 = torch.empty_like(x1)
        K.gemm_fwd(K.gather_convT(du, N, h, w, py, px), wT_dgrad(mod.up.weight, M.d), x1.shape[1],
                   dx1, M.d)
    return dx1, dx2


# ----------------------------------------------------------------------------
# OutConv (unet_parts.py:97-103): 1x1 conv + bias, fp32 logits
# ----------------------------------------------------------------------------
# OutConv over the UNet's last BatchNorm + ReLU applied in its operand path
# (round 6): up4's DoubleConv leaves BN2 unapplied (defer "any"), the 1x1
# kernel forms a = relu(y2 * scale + shift) in registers (bit-identical to the
# applied bytes), and its backward re-forms a for the weight gradient and
# emits BN2's first backward reduction stage over the gradient it writes --
# the BN2 apply pass and the BN2 reduction pass are not run.  A/B switch.
FUSE_OUTCONV_BN = True


def outconv_fusable(x_channels, n_classes):
    return FUSE_OUTCONV_BN and x_channels % 8 == 0 and x_channels <= 256 and \
        (x_channels // 8) & (x_channels // 8 - 1) == 0 and 1 <= n_classes <= 4


def outconv_fwd(M, conv, x, pend=None):
    """pend = (y, coef): x is None and the operand is relu(BN(y)) (the
    producing DoubleConv's deferred BN2)."""
    src = x if pend is None else pend[0]
    N, Cc, H, W = src.shape
    J = conv.out_channels
    y = torch.empty((N, J, H, W), dtype=torch.float32, device=src.device, memory_format=K.CL)
    if pend is None:
        K.call("vu_pointwise_fwd", K.ptr(x), K.pstride(x), N * H * W, Cc, J, K.ptr(conv.weight),
               K.ptr(conv.bias), K.ptr(y), J, M.d, K.stream())
        return y, (x,)
    yb, coef = pend
    K.call("vu_pointwise_bn_fwd", K.ptr(yb), K.pstride(yb), N * H * W, Cc, J, K.ptr(coef[0]), K.ptr(coef[1]),
           K.ptr(conv.weight), K.ptr(conv.bias), K.ptr(y), J, M.d, K.stream())
    return y, (yb, coef)


def outconv_bwd(M, conv, saved, dy):
    """Returns the gradient of OutConv's input, or (da2, BnbPart) for a
    deferred BN2 (saved = (y2, coef2)): da2 is the gradient w.r.t. the
    never-stored relu(BN2(y2)) and the part BN2's first reduction stage."""
    x = saved[0]
    N, Cc, H, W = x.shape
    J = conv.out_channels
    dy = dy.float().contiguous(memory_format=K.CL)
    gw, acc = grad_sink(conv.weight)
    gb, _ = grad_sink(conv.bias)
    dx = torch.empty_like(x)
    ws = K.workspace_f32(K.query("vu_pointwise_bwd_workspace_bytes", N * H * W, Cc, J), x.device)
    if len(saved) == 1:
        K.call("vu_pointwise_bwd", K.ptr(x), K.pstride(x), K.ptr(dy), J, N * H * W, Cc, J,
               K.ptr(conv.weight), K.ptr(dx), K.pstride(dx), K.ptr(gw), K.ptr(gb), 1 if acc else 0,
               K.ptr(ws), M.d, K.stream())
        M.notify([conv.weight, conv.bias])
        return dx
    coef = saved[1]
    nblk = K.query("vu_pointwise_bn_bwd_blocks", N * H * W)
    bnb = torch.empty((nblk, 2, Cc), dtype=torch.float32, device=x.device)
    K.call("vu_pointwise_bn_bwd", K.ptr(x), K.pstride(x), K.ptr(coef), coef.stride(0), K.ptr(dy), J, N * H * W,
           Cc, J, K.ptr(conv.weight), K.ptr(dx), K.pstride(dx), K.ptr(gw), K.ptr(gb), 1 if acc else 0,
           K.ptr(ws), K.ptr(bnb), M.d, K.stream())
    M.notify([conv.weight, conv.bias])
    return dx, K.BnbPart(bnb, nblk, x)


# ----------------------------------------------------------------------------
# external tensors -> NHWC storage
# ----------------------------------------------------------------------------
def to_act(M, x, cpad=None):
    """Bring a caller tensor into NHWC storage of the mode's dtype (padding the
    channel count to a multiple of 8 for the 3-channel image input)."""
    N, Cc, H, W = x.shape
    cp = cpad or Cc
    if cp == Cc and x.dtype == M.tdtype and x.is_contiguous(memory_format=K.CL):
        return x
    return K.input_pack(x, cp, M.d)


def from_act(dx, like):
    """Gradient for a caller tensor of shape/dtype ``like``."""
    if dx.shape[1] != like.shape[1]:
        dx = dx[:, :like.shape[1]]
    return dx.to(dtype=like.dtype)
