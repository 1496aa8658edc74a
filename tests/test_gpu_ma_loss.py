"""The fused focal + Dice kernels (csrc/focal.hip) and MAFocalLoss /
MASegmentationLoss / torch.ops.vaeunet.focal_dice_loss over them, against the
definitions of DESIGN.md §4.7 evaluated in float64 on the CPU.

Bounds (u = 2^-24; ``sabs`` = the closed-form gradient with every subtraction
replaced by an addition, the convention of ref_small.py):

  gradient, per element   |g_hip - g_64| <= 4 * r_cpu * u * sabs + 2^-126
  focal                   relative error <= 4 * max(r_cpu, 1) * u
  dice_loss               absolute error <= 4 * max(r_cpu, 1) * u
  the five sums           relative error <= 4 * max(r_cpu, 1) * u (the NaN count exactly)

r_cpu is measured here, on the same inputs: the error of the same formulas
evaluated by torch in float32 on the CPU, in the same units (for the gradient
the smallest r with |g_32 - g_64| <= r * u * sabs + 2^-126 everywhere).  The
factor 4 covers the device libm's expf / log1pf / expm1f differing from
glibc's by a few ulp.  Every element is compared.

Worst ratios measured on the MI355X over the cases of test_kernel_parity
(gradient: the r above; losses: error / u), with the CPU's float32 figure on
the same case in brackets:
  gradient   gamma 0: 5.1 (4.7)   1: 6.9 (5.8)   2: 9.4 (7.8)   2.5: 12.7 (9.2)
  focal      0.84 (0.85) for n >= 7; at n = 1 and 2 the focal value is a float32
             subnormal or 0 and both evaluations are off by the same 8.05 u or by all of it
  dice_loss  0.50 (0.50)
The tightest case is n = 7, soft targets, gamma 0: 2.13 against 4 * 0.621.
"""
import functools

import pytest
import torch

from ref_small import guarded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CL = torch.channels_last
U = 2.0 ** -24
TINY = 2.0 ** -126
SPECIAL = [-90.0, -30.0, -1e-3, 0.0, 1e-3, 30.0, 90.0, 17.0, -17.0]
BIG = 3 * 2 ** 20 + 5   # > 2048 blocks * 256 threads * 4 elements: the grid-stride path


# ----------------------------------------------------------------------------
# reference: DESIGN.md §4.7 written with torch, in the dtype asked for
# ----------------------------------------------------------------------------
def focal_dice_ref(x, t, alpha, gamma, smooth, wf, wd, sum_red, gout=1.0, dtype=torch.float64):
    """-> dict(loss, focal, dice, sums [5], grad, sabs); a NaN logit: p = 0,
    no focal term, gradient 0, still counted in n."""
    x, t = x.detach().cpu().to(dtype).flatten(), t.detach().cpu().to(dtype).flatten()
    nan = torch.isnan(x)
    zero = torch.zeros((), dtype=dtype)
    xs = torch.where(nan, zero, x)

    def sp(z):
        return z.clamp_min(0) + torch.log1p(torch.exp(-z.abs()))

    b = t * sp(-xs) + (1 - t) * sp(xs)
    q, omq = torch.exp(-b), -torch.expm1(-b)
    at = alpha * t + (1 - alpha) * (1 - t)
    if gamma == 0:
        pw = torch.ones_like(b)
        w = torch.ones_like(b)
    else:
        pw = omq ** gamma
        w = pw + gamma * omq ** (gamma - 1) * q * b
    f = torch.where(nan, zero, at * pw * b)
    p = torch.where(nan, zero, torch.sigmoid(xs))
    dp = torch.where(nan, zero, torch.sigmoid(xs) * torch.sigmoid(-xs))
    n = x.numel()
    Sf, I, Sp, St = f.sum(), (p * t).sum(), p.sum(), t.sum()
    div = 1.0 if sum_red else float(n)
    focal = Sf / div
    Uu = Sp.clamp_min(smooth / 2) + St.clamp_min(smooth / 2) + smooth
    num = 2 * I + smooth
    mp = (Sp >= smooth / 2).to(dtype)
    dice = 1 - num / Uu
    keep = (~nan).to(dtype)
    gf, gf_abs = at * w * (p - t) / div, at * w * (p + t) / div
    gd, gd_abs = dp * (2 * t * Uu - num * mp) / Uu ** 2, dp * (2 * t * Uu + num * mp) / Uu ** 2
    grad = gout * (wf * gf - wd * gd) * keep
    sabs = abs(gout) * (wf * gf_abs + wd * gd_abs) * keep
    sums = torch.stack([Sf, I, Sp, St, nan.sum().to(dtype)])
    return dict(loss=wf * focal + wd * dice, focal=focal, dice=dice, sums=sums, grad=grad, sabs=sabs)


def grad_ratio(g, ref):
    """the smallest r with |g - g_64| <= r * u * sabs + 2^-126 for every element"""
    excess = ((g.double().cpu().flatten() - ref["grad"]).abs() - TINY).clamp_min(0)
    sabs = ref["sabs"]
    r = torch.where(excess > 0, excess / (U * sabs), torch.zeros_like(excess))   # sabs = 0 and an excess: inf
    return float(r.max())


def rel_u(got, ref):
    ref = float(ref)
    return abs(float(got) - ref) / (U * abs(ref)) if ref != 0 else (0.0 if float(got) == 0 else float("inf"))


@functools.lru_cache(maxsize=None)
def make_inputs(n, soft, nan_at=-1):
    g = torch.Generator().manual_seed(1000 + n + (7 if soft else 0))
    x = torch.randn(n, generator=g) * 4.0            # N(0, 16)
    k = min(n, len(SPECIAL))
    x[:k] = torch.tensor(SPECIAL[:k])
    t = torch.rand(n, generator=g) if soft else (torch.rand(n, generator=g) < 0.03).float()
    if nan_at >= 0:
        x[nan_at] = float("nan")
    return x, t


@functools.lru_cache(maxsize=None)
def references(n, soft, gamma, sum_red, wf, wd, nan_at=-1, gout=1.0):
    """(fp64 reference, the same in fp32 on the CPU), computed once per case"""
    x, t = make_inputs(n, soft, nan_at)
    args = (x, t, 0.75, gamma, 1.0, wf, wd, sum_red, gout)
    return focal_dice_ref(*args), focal_dice_ref(*args, dtype=torch.float32)


def run_kernels(x, t, offs, gamma, sum_red, wf, wd, gout=1.0, alpha=0.75, smooth=1.0):
    """Both C-ABI entry points on guarded buffers -> (loss, parts, sums, grad, guards)"""
    from vaeunet_amd._lib import call, ptr, query, stream
    n = x.numel()
    xd, gx = guarded(n, torch.float32, offset=offs[0])
    td, gt = guarded(n, torch.float32, offset=offs[1])
    gd, gg = guarded(n, torch.float32, offset=offs[2])
    xd.copy_(x)
    td.copy_(t)
    sums, gs = guarded(5, torch.float64)
    loss, gl = guarded(1, torch.float32)
    parts, gp = guarded(2, torch.float32)
    nws = query("vu_focal_workspace_bytes") // 8
    ws, gw = guarded(nws, torch.float64)
    gscale = torch.tensor([gout], dtype=torch.float32, device=DEV)
    call("vu_focal_dice_fwd", ptr(xd), ptr(td), n, alpha, gamma, smooth, wf, wd, int(sum_red), ptr(sums), ptr(loss),
         ptr(parts), ptr(ws), stream())
    call("vu_focal_dice_bwd", ptr(xd), ptr(td), n, alpha, gamma, smooth, wf, wd, int(sum_red), ptr(sums),
         ptr(gscale), ptr(gd), stream())
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu().nan_to_num(nan=7.0), x.nan_to_num(nan=7.0)) and torch.equal(td.cpu(), t), "inputs written"
    return loss, parts, sums, gd, (gx, gt, gg, gs, gl, gp, gw)


def check_against(ref64, ref32, loss, parts, sums, grad, what):
    """the bounds of the module docstring; returns the measured ratios"""
    r_cpu_g = grad_ratio(ref32["grad"], ref64)
    r_hip_g = grad_ratio(grad, ref64)
    r_cpu_f, r_hip_f = rel_u(ref32["focal"], ref64["focal"]), rel_u(parts[0], ref64["focal"])
    r_cpu_d = abs(float(ref32["dice"]) - float(ref64["dice"])) / U
    r_hip_d = abs(float(parts[1]) - float(ref64["dice"])) / U
    r_cpu_s = max(max(rel_u(ref32["sums"][k], ref64["sums"][k]) for k in range(4)), r_cpu_f, 1.0)
    r_hip_s = max(rel_u(sums[k], ref64["sums"][k]) for k in range(4))
    msg = (f"{what}: worst HIP ratio (CPU fp32 ratio): grad {r_hip_g:.3g} ({r_cpu_g:.3g}), focal {r_hip_f:.3g} "
           f"({r_cpu_f:.3g}), dice_loss {r_hip_d:.3g} ({r_cpu_d:.3g}), sums {r_hip_s:.3g} ({r_cpu_s:.3g})")
    print(msg)
    assert torch.isfinite(grad).all(), msg
    assert r_hip_g <= 4 * r_cpu_g, msg
    assert r_hip_f <= 4 * max(r_cpu_f, 1.0), msg
    assert r_hip_d <= 4 * max(r_cpu_d, 1.0), msg
    assert r_hip_s <= 4 * r_cpu_s, msg
    assert float(sums[4]) == float(ref64["sums"][4]), msg
    return r_hip_g, r_hip_f, r_hip_d


def check_parts_from_sums(loss, parts, sums, n, sum_red, wf, wd, smooth=1.0):
    """parts and loss are what the five sums give (fp64 arithmetic rounded once
    to fp32; the loss one fp32 multiply-add more)"""
    s = sums.cpu().double()
    focal = s[0] if sum_red else s[0] / n
    Uu = max(float(s[2]), smooth / 2) + max(float(s[3]), smooth / 2) + smooth
    dice = 1 - (2 * float(s[1]) + smooth) / Uu
    assert float(parts[0]) == float(focal.float())
    assert float(parts[1]) == float(torch.tensor(dice, dtype=torch.float64).float())
    want = wf * float(parts[0]) + wd * float(parts[1])
    assert abs(float(loss) - want) <= 2 * U * (abs(wf * float(parts[0])) + abs(wd * float(parts[1])))


# n, (offset of logits, target, grad) in floats from a 16-byte boundary
LAYOUTS = [(1, (0, 0, 0)), (7, (0, 0, 0)), (4099, (0, 0, 0)), (2053, (1, 1, 1)), (BIG, (0, 0, 0)),
           # the head cut short by n; pointers with no common alignment (the one-element-per-load form)
           (2, (1, 1, 1)), (2053, (1, 0, 1)), (2053, (0, 0, 1))]


# every combination; the large size with one pair of weights (its references take the longest)
PARITY_CASES = [(n, offs, gamma, sum_red, soft, w)
                for n, offs in LAYOUTS for gamma in (0.0, 1.0, 2.0, 2.5) for sum_red in (False, True)
                for soft in (False, True) for w in ((0.5, 0.5), (1.0, 0.0)) if n != BIG or w == (0.5, 0.5)]


@pytest.mark.parametrize("n,offs,gamma,sum_red,soft,weights", PARITY_CASES)
def test_kernel_parity(n, offs, gamma, sum_red, soft, weights):
    wf, wd = weights
    x, t = make_inputs(n, soft)
    ref64, ref32 = references(n, soft, gamma, sum_red, wf, wd)
    loss, parts, sums, grad, guards = run_kernels(x, t, offs, gamma, sum_red, wf, wd)
    what = f"n={n} offs={offs} gamma={gamma} sum={sum_red} soft={soft} w={weights}"
    for gd in guards:
        gd.check(what)
    check_against(ref64, ref32, loss, parts, sums, grad, what)
    check_parts_from_sums(loss, parts, sums, n, sum_red, wf, wd)
    # bitwise repeatable
    loss2, parts2, sums2, grad2, _ = run_kernels(x, t, offs, gamma, sum_red, wf, wd)
    assert torch.equal(grad, grad2) and torch.equal(sums, sums2) and torch.equal(loss, loss2) \
        and torch.equal(parts, parts2), what


@pytest.mark.parametrize("soft", [False, True])
def test_sums_and_parts(soft):
    """the five sums vs fp64, other constants than the defaults, no loss / parts output"""
    from vaeunet_amd._lib import call, ptr, query, stream
    n = 4099
    x, t = make_inputs(n, soft)
    alpha, gamma, smooth, wf, wd = 0.25, 2.0, 3.0, 0.3, 0.7
    ref64 = focal_dice_ref(x, t, alpha, gamma, smooth, wf, wd, False)
    ref32 = focal_dice_ref(x, t, alpha, gamma, smooth, wf, wd, False, dtype=torch.float32)
    loss, parts, sums, grad, guards = run_kernels(x, t, (0, 0, 0), gamma, False, wf, wd, alpha=alpha, smooth=smooth)
    for gd in guards:
        gd.check("sums")
    check_against(ref64, ref32, loss, parts, sums, grad, f"sums soft={soft}")
    check_parts_from_sums(loss, parts, sums, n, False, wf, wd, smooth)
    assert abs(float(loss) - float(ref64["loss"])) <= 16 * U * (wf * abs(float(ref64["focal"])) + wd)
    # loss = parts = NULL: the sums alone, the same bits
    sums2 = torch.empty(5, dtype=torch.float64, device=DEV)
    ws = torch.empty(query("vu_focal_workspace_bytes") // 8, dtype=torch.float64, device=DEV)
    xd, td = x.to(DEV), t.to(DEV)
    call("vu_focal_dice_fwd", ptr(xd), ptr(td), n, alpha, gamma, smooth, wf, wd, 0, ptr(sums2), None, None, ptr(ws),
         stream())
    assert torch.equal(sums2, sums)


def test_dice_clamp_branch():
    """sum p < smooth / 2: the clamp is active and no Dice gradient flows through sum p"""
    n = 7
    x = torch.full((n,), -12.0)
    t = torch.zeros(n)
    t[3] = 1.0
    ref64 = focal_dice_ref(x, t, 0.75, 2.0, 1.0, 0.5, 0.5, False)
    ref32 = focal_dice_ref(x, t, 0.75, 2.0, 1.0, 0.5, 0.5, False, dtype=torch.float32)
    assert float(ref64["sums"][2]) < 0.5
    loss, parts, sums, grad, guards = run_kernels(x, t, (0, 0, 0), 2.0, False, 0.5, 0.5)
    check_against(ref64, ref32, loss, parts, sums, grad, "clamp")


def test_invalid_constants_are_an_error_code():
    """the C entry points refuse what the Python layer refuses (no launch)"""
    x, t = make_inputs(7, False)
    for kw in (dict(gamma=0.5), dict(alpha=1.5), dict(smooth=0.0)):
        args = dict(gamma=2.0, alpha=0.75, smooth=1.0)
        args.update(kw)
        with pytest.raises(RuntimeError, match="vu_focal_dice_fwd failed"):
            run_kernels(x, t, (0, 0, 0), args["gamma"], False, 0.5, 0.5, alpha=args["alpha"], smooth=args["smooth"])


@pytest.mark.parametrize("gamma", [0.0, 2.0, 2.5])
@pytest.mark.parametrize("sum_red", [False, True])
def test_nan_logit(gamma, sum_red):
    n, at = 4099, 1234
    x, t = make_inputs(n, False, at)
    assert torch.isnan(x[at]) and int(torch.isnan(x).sum()) == 1
    ref64, ref32 = references(n, False, gamma, sum_red, 0.5, 0.5, at)
    # the reference = that element's focal term dropped and p = 0, n unchanged
    clean, _ = references(n, False, gamma, sum_red, 0.5, 0.5)
    xc, tc = make_inputs(n, False)
    one = focal_dice_ref(xc[at:at + 1], tc[at:at + 1], 0.75, gamma, 1.0, 0.5, 0.5, True)
    assert abs(float(ref64["sums"][0]) - (float(clean["sums"][0]) - float(one["sums"][0]))) <= 1e-12 * float(
        clean["sums"][0])
    assert abs(float(ref64["sums"][2]) - (float(clean["sums"][2]) - float(one["sums"][2]))) <= 1e-12 * float(
        clean["sums"][2])
    loss, parts, sums, grad, guards = run_kernels(x, t, (0, 0, 0), gamma, sum_red, 0.5, 0.5)
    for gd in guards:
        gd.check("nan")
    assert torch.isfinite(loss).all() and torch.isfinite(parts).all() and torch.isfinite(sums).all()
    assert float(sums[4]) == 1.0
    assert float(grad[at]) == 0.0
    check_against(ref64, ref32, loss, parts, sums, grad, f"nan gamma={gamma} sum={sum_red}")
    check_parts_from_sums(loss, parts, sums, n, sum_red, 0.5, 0.5)


# ----------------------------------------------------------------------------
# modules, autograd, dispatcher op
# ----------------------------------------------------------------------------
def _module_inputs(shape, cl, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 3.0
    t = (torch.rand(shape, generator=g) < 0.1).float()
    if cl:
        x, t = x.contiguous(memory_format=CL), t.contiguous(memory_format=CL)
    return x, t


def _memory_order(a):
    """a's elements in the order of its memory (what the kernels and the reference walk)"""
    a = a.detach().cpu()
    return a.permute(0, 2, 3, 1).flatten() if a.dim() == 4 and not a.is_contiguous() else a.flatten()


def _check_grad(got, x, t, cfg, gout, what):
    """cfg = (alpha, gamma, smooth, wf, wd, sum_red)"""
    xm, tm = _memory_order(x), _memory_order(t)
    ref64 = focal_dice_ref(xm, tm, *cfg, gout=gout)
    ref32 = focal_dice_ref(xm, tm, *cfg, gout=gout, dtype=torch.float32)
    r_cpu, r_hip = grad_ratio(ref32["grad"], ref64), grad_ratio(_memory_order(got), ref64)
    assert r_hip <= 4 * r_cpu, f"{what}: gradient ratio {r_hip:.3g} vs CPU fp32 {r_cpu:.3g}"
    return ref64, ref32


@pytest.mark.parametrize("shape,cl", [((2, 1, 32, 32), False), ((2, 2, 33, 31), True)])
def test_module_and_autograd(shape, cl):
    from vaeunet_amd.loss import MAFocalLoss, MASegmentationLoss, focal_dice_loss
    x, t = _module_inputs(shape, cl)
    cfg = (0.75, 2.0, 1.0, 0.5, 0.5, False)
    xd = x.to(DEV).requires_grad_(True)
    td = t.to(DEV)
    crit = MASegmentationLoss()
    loss = crit(xd, td)
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    assert xd.grad.shape == x.shape and xd.grad.stride() == xd.stride()
    ref64, ref32 = _check_grad(xd.grad, x, t, cfg, 1.0, "MASegmentationLoss")
    # last_parts = [focal, dice_loss]
    assert crit.last_parts is not None and crit.last_parts.shape == (2,) and crit.last_parts.device.type == "cuda"
    assert not crit.last_parts.requires_grad
    assert rel_u(crit.last_parts[0], ref64["focal"]) <= 4 * max(rel_u(ref32["focal"], ref64["focal"]), 1.0)
    assert abs(float(crit.last_parts[1]) - float(ref64["dice"])) <= 4 * U * max(
        abs(float(ref32["dice"]) - float(ref64["dice"])) / U, 1.0)
    assert abs(float(loss.detach()) - float(ref64["loss"])) <= 16 * U * float(ref64["loss"])
    # (3 * loss).backward(): the factor reaches the kernel as a device scalar
    x3 = x.to(DEV).requires_grad_(True)
    (3 * MASegmentationLoss()(x3, td)).backward()
    _check_grad(x3.grad, x, t, cfg, 3.0, "3 * loss")
    # the functional form is the same computation
    xf = x.to(DEV).requires_grad_(True)
    lf = focal_dice_loss(xf, td)
    lf.backward()
    assert torch.equal(lf.detach(), loss.detach()) and torch.equal(xf.grad, xd.grad)
    # MAFocalLoss = the w_dice = 0 case with weight 1, both reductions
    for red in ("mean", "sum"):
        x1 = x.to(DEV).requires_grad_(True)
        l1 = MAFocalLoss(reduction=red)(x1, td)
        l1.backward()
        c1 = (0.75, 2.0, 1.0, 1.0, 0.0, red == "sum")
        r64, r32 = _check_grad(x1.grad, x, t, c1, 1.0, f"MAFocalLoss {red}")
        assert rel_u(l1.detach(), r64["focal"]) <= 4 * max(rel_u(r32["focal"], r64["focal"]), 1.0)
        x2 = x.to(DEV).requires_grad_(True)
        l2 = focal_dice_loss(x2, td, focal_weight=1.0, dice_weight=0.0, reduction=red)
        l2.backward()
        assert torch.equal(l1.detach(), l2.detach()) and torch.equal(x1.grad, x2.grad)
    # bf16 logits and a bool mask are normalised as the other losses do
    xb = x.to(DEV).bfloat16().requires_grad_(True)
    lb = MASegmentationLoss()(xb, td.bool())
    lb.backward()
    assert xb.grad.dtype == torch.bfloat16 and torch.isfinite(lb)


def test_op_parity_and_opcheck():
    from vaeunet_amd import ops  # noqa: F401  (registers the ops)
    v = torch.ops.vaeunet
    for shape, cl in (((2, 1, 32, 32), False), ((2, 2, 33, 31), True)):
        x, t = _module_inputs(shape, cl, seed=6)
        td = t.to(DEV)
        for gamma, red in ((2.0, False), (2.5, True)):
            cfg = (0.75, gamma, 1.0, 0.5, 0.5, red)
            xd = x.to(DEV).requires_grad_(True)
            loss, sums = v.focal_dice_loss(xd, td, *cfg)
            assert sums.shape == (5,) and sums.dtype == torch.float64
            (3 * loss).backward()
            ref64, ref32 = _check_grad(xd.grad, x, t, cfg, 3.0, f"op {shape} gamma={gamma}")
            assert abs(float(loss.detach()) - float(ref64["loss"])) <= 16 * U * float(ref64["loss"])
    x, t = _module_inputs((2, 1, 8, 8), False, seed=7)
    xr = x.to(DEV).requires_grad_(True)
    for args in ((xr, t.to(DEV), 0.75, 2.0, 1.0, 0.5, 0.5, False), (xr, t.to(DEV), 0.25, 2.5, 2.0, 1.0, 0.0, True)):
        torch.library.opcheck(v.focal_dice_loss.default, args,
                              test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))


# ----------------------------------------------------------------------------
# the captured training step (the fixture of test_gpu_graph.py, MA objective)
# ----------------------------------------------------------------------------
def _graph_setup():
    from vaeunet_amd import UNet
    from vaeunet_amd.init import seeded_init_
    from vaeunet_amd.loss import MASegmentationLoss
    from vaeunet_amd.optim import FusedAdamW
    torch.manual_seed(0)
    model = seeded_init_(UNet(3, 2), 0).to(DEV).to(memory_format=CL).train()
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-2)
    crit = MASegmentationLoss()
    g = torch.Generator().manual_seed(3)
    S = 64
    x = torch.rand(2, 3, S, S, generator=g).to(DEV).contiguous(memory_format=CL)
    lab = torch.randint(0, 2, (2, S, S), generator=g)
    t = torch.nn.functional.one_hot(lab, 2).permute(0, 3, 1, 2).float().to(DEV)

    def fwd_bwd():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = crit(model(x), t)
        loss.backward()
        return loss
    return model, opt, fwd_bwd


def test_graph_replay_matches_eager():
    from vaeunet_amd.graph import GraphedTrainStep
    from vaeunet_amd.optim import clip_grad_norm_
    m1, o1, fb1 = _graph_setup()
    losses1 = []
    for i in range(5):
        loss = fb1()
        clip_grad_norm_(m1.parameters(), 1.0)
        o1.step()
        o1.zero_grad(set_to_none=True)
        if i >= 2:
            losses1.append(float(loss.detach()))
    m2, o2, fb2 = _graph_setup()
    gs = GraphedTrainStep(fb2, o2, max_norm=1.0, warmup=2)
    losses2 = [float(gs.step().detach()) for _ in range(3)]
    torch.cuda.synchronize()
    for a, b in zip(losses1, losses2):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (losses1, losses2)
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        torch.testing.assert_close(p2, p1, rtol=1e-6, atol=1e-7, msg=f"param {n}")
    gs.sync_optimizer_state()
    assert float(o2.state[next(m2.parameters())]["step"]) == 5.0
