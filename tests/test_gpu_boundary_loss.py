"""The boundary loss kernels (csrc/boundary_loss.hip) and boundary_loss /
BoundaryLoss / BoundaryAugmentedLoss / torch.ops.vaeunet.boundary_loss over
them, against the definitions of DESIGN.md §4.13 evaluated in float64 on the
CPU (tests/sdf_ref.py).

Bounds, the convention of test_gpu_ma_loss.py (u = 2^-24; A = sum |phi| p, the
sum with every term replaced by its absolute value; sabs = |gradient|, the
gradient being a product):

  gradient, per element   |g_hip - g_64| <= 4 * r_cpu * u * sabs + 2^-126
  loss                    |l_hip - l_64| <= 4 * max(r_cpu, 1) * u * A / n
  sum phi p               the same in units of u * A;  sum |phi| p relative;  the skipped count exactly

r_cpu is measured here, on the same inputs: the error of the same formulas
evaluated by torch in float32 on the CPU, in the same units.  The factor 4
covers the device libm's expf differing from glibc's by a few ulp.  Every
element is compared and the worst ratios are printed.

Inputs: N(0, 16) logits with the special values of test_gpu_ma_loss.py among
the first elements (17 first: at n = 1 the loss of a logit of -90 is a float32
subnormal, where a bound in units of u says nothing); phi of 67 x 131 planes
with negative interiors (a disc, nested squares), so that A differs from the
sum, and of sparse planes (Bernoulli 0.0085, a single corner pixel).

Worst ratios measured on the MI355X over the cases of test_kernel_parity, with
the CPU's float32 figure on the same case in brackets: gradient 6.59 (6.37) at
n = 3145733; the tightest case is n = 2053 with interiors, 6.17 against 4 *
4.70; loss 0.85 (0.58) at n = 7, below 1 everywhere; the fp64 sums 0.70 at
n = 1 (the sigmoid is a float32), below 0.03 from n = 2053 on."""
import functools

import numpy as np
import pytest
import torch

import edt_ref as ER
import sdf_ref as SR
from ref_small import guarded
from test_gpu_ma_loss import focal_dice_ref
from test_gpu_ma_loss import grad_ratio as focal_grad_ratio

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CL = torch.channels_last
U = 2.0 ** -24
TINY = 2.0 ** -126
SPECIAL = [17.0, -1e-3, -90.0, -30.0, 0.0, 1e-3, 30.0, 90.0, -17.0]
BIG = 3 * 2 ** 20 + 5   # > 2048 blocks * 256 threads * 4 elements: the grid-stride path


@functools.lru_cache(maxsize=None)
def phi_pool(kind):
    """float32 phi of four 67 x 131 planes, flattened: 'dense' has interiors, 'sparse' almost none"""
    H, W = 67, 131
    pairs, adv = ER.pair_planes(H, W), ER.adversarial_planes(H, W)
    if kind == "dense":
        planes = [pairs["shifted_disc"][0], pairs["nested_squares"][0], pairs["nested_squares"][1], pairs["touching_edge"][0]]
    else:
        planes = [adv["bernoulli0.0085"], adv["corner00"], adv["equidistant"], adv["none"]]
    phi = np.concatenate([SR.phi_of(SR.s2_plane(p != 0)).reshape(-1) for p in planes])
    if kind == "dense":
        assert (phi < -1).sum() > 1000 and (phi > 1).sum() > 1000
    start = int(np.flatnonzero(phi < -1)[0]) if kind == "dense" else 0     # n = 1 takes an interior value
    return torch.from_numpy(np.roll(phi, -start).copy())


@functools.lru_cache(maxsize=None)
def make_inputs(n, kind, bad=False):
    g = torch.Generator().manual_seed(2000 + n + (7 if kind == "dense" else 0))
    x = torch.randn(n, generator=g) * 4.0            # N(0, 16)
    k = min(n, len(SPECIAL))
    x[:k] = torch.tensor(SPECIAL[:k])
    pool = phi_pool(kind)
    f = pool.repeat((n + pool.numel() - 1) // pool.numel())[:n].clone()
    if bad:
        x[1234] = float("nan")
        f[77], f[78], f[79] = float("inf"), float("-inf"), float("nan")
        x[79] = float("nan")                         # both at once: one skipped element
    return x, f


@functools.lru_cache(maxsize=None)
def references(n, kind, bad=False, gout=1.0):
    """(fp64 reference, the same in fp32 on the CPU), computed once per case"""
    x, f = make_inputs(n, kind, bad)
    return SR.boundary_loss_ref(x, f, gout), SR.boundary_loss_ref(x, f, gout, dtype=torch.float32)


def grad_ratio(g, ref):
    """the smallest r with |g - g_64| <= r * u * sabs + 2^-126 for every element"""
    excess = ((g.double().cpu().flatten() - ref["grad"]).abs() - TINY).clamp_min(0)
    r = torch.where(excess > 0, excess / (U * ref["sabs"]), torch.zeros_like(excess))   # sabs = 0 and an excess: inf
    return float(r.max())


def in_units(got, want, unit):
    d = abs(float(got) - float(want))
    return d / unit if unit > 0 else (0.0 if d == 0 else float("inf"))


def run_kernels(x, f, offs, gout=1.0):
    """Both C-ABI entry points on guarded buffers -> (loss, sums, grad, guards)"""
    from vaeunet_amd._lib import call, ptr, query, stream
    n = x.numel()
    xd, gx = guarded(n, torch.float32, offset=offs[0])
    fd, gf = guarded(n, torch.float32, offset=offs[1])
    gd, gg = guarded(n, torch.float32, offset=offs[2])
    xd.copy_(x)
    fd.copy_(f)
    sums, gs = guarded(3, torch.float64)
    loss, gl = guarded(1, torch.float32)
    ws, gw = guarded(query("vu_boundary_loss_workspace_bytes") // 8, torch.float64)
    gscale = torch.tensor([gout], dtype=torch.float32, device=DEV)
    call("vu_boundary_loss_fwd", ptr(xd), ptr(fd), n, ptr(sums), ptr(loss), ptr(ws), stream())
    call("vu_boundary_loss_bwd", ptr(xd), ptr(fd), n, ptr(gscale), ptr(gd), stream())
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(a.cpu().view(torch.int32), b.view(torch.int32))   # noqa: E731
    assert same(xd, x) and same(fd, f), "inputs written"
    return loss, sums, gd, (gx, gf, gg, gs, gl, gw)


def check_against(ref64, ref32, loss, sums, grad, n, what):
    """the bounds of the module docstring; returns the measured ratios"""
    s64, s32 = ref64["sums"], ref32["sums"]
    A = float(s64[1])
    r_cpu_g, r_hip_g = grad_ratio(ref32["grad"], ref64), grad_ratio(grad, ref64)
    r_cpu_l, r_hip_l = in_units(ref32["loss"], ref64["loss"], U * A / n), in_units(loss, ref64["loss"], U * A / n)
    r_cpu_s = max(in_units(s32[0], s64[0], U * A), in_units(s32[1], s64[1], U * A), 1.0)
    r_hip_s = max(in_units(sums[0], s64[0], U * A), in_units(sums[1], s64[1], U * A))
    msg = (f"{what}: worst HIP ratio (CPU fp32 ratio): grad {r_hip_g:.3g} ({r_cpu_g:.3g}), loss {r_hip_l:.3g} "
           f"({r_cpu_l:.3g}), sums {r_hip_s:.3g} ({r_cpu_s:.3g}); sum {float(s64[0]):.6g}, absolute sum {A:.6g}")
    print(msg)
    assert torch.isfinite(grad).all() and torch.isfinite(loss).all() and torch.isfinite(sums).all(), msg
    assert r_hip_g <= 4 * r_cpu_g, msg
    assert r_hip_l <= 4 * max(r_cpu_l, 1.0), msg
    assert r_hip_s <= 4 * r_cpu_s, msg
    assert float(sums[2]) == float(s64[2]), msg
    return r_hip_g, r_hip_l


def check_loss_from_sums(loss, sums, n):
    """the loss is what the sums give: the fp64 quotient rounded once to fp32"""
    sums = sums.detach()
    assert float(loss) == float((sums.cpu()[0] / n).float())
    assert float(sums[1]) >= abs(float(sums[0]))


# n, (offset of logits, phi, grad) in floats from a 16-byte boundary
LAYOUTS = [(1, (0, 0, 0)), (7, (0, 0, 0)), (4099, (0, 0, 0)), (2053, (1, 1, 1)), (BIG, (0, 0, 0)),
           # the head cut short by n; pointers with no common alignment (the one-element-per-load form)
           (2, (1, 1, 1)), (2053, (1, 0, 1)), (2053, (0, 0, 1))]


@pytest.mark.parametrize("kind", ["dense", "sparse"])
@pytest.mark.parametrize("n,offs", LAYOUTS)
def test_kernel_parity(n, offs, kind):
    x, f = make_inputs(n, kind)
    ref64, ref32 = references(n, kind)
    if kind == "dense" and n >= 4099:
        assert float(ref64["sums"][1]) > 1.02 * abs(float(ref64["sums"][0]))      # the absolute sum is another number
    loss, sums, grad, guards = run_kernels(x, f, offs)
    what = f"n={n} offs={offs} {kind}"
    for gd in guards:
        gd.check(what)
    check_against(ref64, ref32, loss, sums, grad, n, what)
    check_loss_from_sums(loss, sums, n)
    # bitwise repeatable
    loss2, sums2, grad2, _ = run_kernels(x, f, offs)
    assert torch.equal(grad, grad2) and torch.equal(sums, sums2) and torch.equal(loss, loss2), what


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_nan_logits_and_non_finite_phi_are_counted_and_get_no_gradient(kind):
    n = 4099
    x, f = make_inputs(n, kind, True)
    ref64, ref32 = references(n, kind, True, 2.0)
    assert float(ref64["sums"][2]) == 4.0
    loss, sums, grad, guards = run_kernels(x, f, (0, 0, 0), gout=2.0)
    for gd in guards:
        gd.check("skipped")
    assert float(sums[2]) == 4.0
    for at in (77, 78, 79, 1234):
        assert float(grad[at]) == 0.0 and not bool(torch.signbit(grad[at]))
    check_against(ref64, ref32, loss, sums, grad, n, f"skipped {kind}")
    check_loss_from_sums(loss, sums, n)
    # the reference = the clean one without those elements' terms, n unchanged
    xc, fc = make_inputs(n, kind)
    clean, _ = references(n, kind)
    idx = torch.tensor([77, 78, 79, 1234])
    dropped = SR.boundary_loss_ref(xc[idx], fc[idx])["sums"][0]
    assert abs(float(ref64["sums"][0]) - (float(clean["sums"][0]) - float(dropped))) <= 1e-12 * float(clean["sums"][1])


def test_c_abi_rejections_write_nothing_and_the_loss_is_optional():
    from vaeunet_amd._lib import ptr, query, stream
    n = 7
    x, f = make_inputs(n, "dense")
    xd, fd = x.to(DEV), f.to(DEV)
    sums, gs = guarded(3, torch.float64)
    loss, gl = guarded(1, torch.float32)
    grad, gg = guarded(n, torch.float32)
    ws, gw = guarded(query("vu_boundary_loss_workspace_bytes") // 8, torch.float64)
    before = [g.buf.clone() for g in (gs, gl, gg, gw)]
    s, INVALID = stream(), 1
    ok = [ptr(xd), ptr(fd), n, ptr(sums), ptr(loss), ptr(ws), s]
    for at, bad in ((0, None), (1, None), (2, 0), (2, -1), (3, None), (5, None)):
        args = list(ok)
        args[at] = bad
        assert query("vu_boundary_loss_fwd", *args) == INVALID, (at, bad)
    ok = [ptr(xd), ptr(fd), n, None, ptr(grad), s]
    for at, bad in ((0, None), (1, None), (2, 0), (2, -5), (4, None)):
        args = list(ok)
        args[at] = bad
        assert query("vu_boundary_loss_bwd", *args) == INVALID, (at, bad)
    torch.cuda.synchronize()
    for g, b in zip((gs, gl, gg, gw), before):
        assert torch.equal(g.buf, b)
    # loss = NULL: the sums alone, the same bits; gscale = NULL is 1
    l1, s1, g1, _ = run_kernels(x, f, (0, 0, 0))
    assert query("vu_boundary_loss_fwd", ptr(xd), ptr(fd), n, ptr(sums), None, ptr(ws), s) == 0
    assert query("vu_boundary_loss_bwd", ptr(xd), ptr(fd), n, None, ptr(grad), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(sums, s1) and torch.equal(grad, g1)
    gl.check("loss not written")
    assert torch.equal(gl.buf, before[1])


# ----------------------------------------------------------------------------
# modules, autograd, dispatcher op: 2 x 2 x 33 x 31
# ----------------------------------------------------------------------------
SHAPE = (2, 2, 33, 31)


@functools.lru_cache(maxsize=None)
def _module_inputs(cl):
    """(logits, mask uint8, reference phi per clip): a disc, nested squares, an empty plane and a sparse one"""
    B, C, H, W = SHAPE
    g = torch.Generator().manual_seed(11)
    x = torch.randn(SHAPE, generator=g) * 3.0
    pairs, adv = ER.pair_planes(H, W), ER.adversarial_planes(H, W)
    m = np.stack([pairs["shifted_disc"][0], pairs["nested_squares"][0], adv["none"], adv["bernoulli0.0085"]])
    m = np.ascontiguousarray(m.reshape(SHAPE))
    assert m[0, 0].any() and m[1, 1].any() and not m[1, 0].any()
    t = torch.from_numpy(m)
    if cl:
        x, t = x.contiguous(memory_format=CL), t.contiguous(memory_format=CL)
    return x, t, {clip: torch.from_numpy(SR.phi(m, clip=clip)) for clip in (None, 2.5)}


def _memory_order(a, like):
    """a's elements in the order of like's memory (what the kernels and the reference walk)"""
    a = a.detach().cpu()
    return a.permute(0, 2, 3, 1).flatten() if like.dim() == 4 and not like.is_contiguous() else a.flatten()


def _refs(x, phi, gout=1.0):
    xm, fm = _memory_order(x, x), _memory_order(phi, x)
    return SR.boundary_loss_ref(xm, fm, gout), SR.boundary_loss_ref(xm, fm, gout, dtype=torch.float32)


def _check_module(loss, grad, x, phi, gout, what):
    ref64, ref32 = _refs(x, phi, gout)
    n, A = x.numel(), float(ref64["sums"][1])
    r_cpu, r_hip = grad_ratio(ref32["grad"], ref64), grad_ratio(_memory_order(grad, x), ref64)
    r_cpu_l = in_units(ref32["loss"], ref64["loss"], U * A / n)
    r_hip_l = in_units(loss, ref64["loss"], U * A / n)
    print(f"{what}: gradient ratio {r_hip:.3g} (CPU fp32 {r_cpu:.3g}), loss {r_hip_l:.3g} ({r_cpu_l:.3g})")
    assert r_hip <= 4 * r_cpu, f"{what}: gradient ratio {r_hip:.3g} vs CPU fp32 {r_cpu:.3g}"
    assert r_hip_l <= 4 * max(r_cpu_l, 1.0), f"{what}: loss ratio {r_hip_l:.3g} vs CPU fp32 {r_cpu_l:.3g}"
    return ref64, ref32


@pytest.mark.parametrize("cl", [False, True])
def test_module_function_and_autograd(cl):
    from vaeunet_amd.loss import BoundaryLoss, boundary_loss
    x, t, phis = _module_inputs(cl)
    td = t.to(DEV)
    for clip in (None, 2.5):
        phi = phis[clip]
        xd = x.to(DEV).requires_grad_(True)
        loss = BoundaryLoss(clip=clip)(xd, td)
        assert loss.shape == () and loss.dtype == torch.float32
        loss.backward()
        assert xd.grad.shape == x.shape and xd.grad.stride() == xd.stride()
        _check_module(loss.detach(), xd.grad, x, phi, 1.0, f"BoundaryLoss clip={clip} cl={cl}")
        # the functional form, targets= and phi=: the same bits; every target dtype
        for kw in (dict(targets=td, clip=clip), dict(phi=phi.to(DEV)), dict(targets=td.bool(), clip=clip),
                   dict(targets=td.float(), clip=clip), dict(targets=td.float() * 0.75, clip=clip, threshold=0.5),
                   dict(targets=td.long(), clip=clip)):
            xf = x.to(DEV).requires_grad_(True)
            lf = boundary_loss(xf, **kw)
            lf.backward()
            assert torch.equal(lf.detach(), loss.detach()) and torch.equal(xf.grad, xd.grad), sorted(kw)
        # (3 * loss).backward(): the factor reaches the kernel as a device scalar
        x3 = x.to(DEV).requires_grad_(True)
        (3 * BoundaryLoss(clip=clip)(x3, td)).backward()
        _check_module(loss.detach(), x3.grad, x, phi, 3.0, f"3 * loss clip={clip} cl={cl}")
    # phi is what signed_distance gives, and no gradient reaches the targets
    from vaeunet_amd.surface import signed_distance
    assert torch.equal(signed_distance(td.contiguous(), clip=2.5).cpu(), phis[2.5].contiguous())
    tf = td.float().requires_grad_(True)
    xg = x.to(DEV).requires_grad_(True)
    boundary_loss(xg, tf).backward()
    assert tf.grad is None and xg.grad is not None
    # [B, H, W] is C = 1; bf16 logits are normalised as the other losses do
    x3d, t3d = x[:, 0].contiguous().to(DEV).requires_grad_(True), td[:, 0].contiguous()
    x4d = x[:, :1].contiguous().to(DEV).requires_grad_(True)
    l3, l4 = boundary_loss(x3d, t3d), boundary_loss(x4d, t3d[:, None])
    l3.backward()
    l4.backward()
    assert torch.equal(l3.detach(), l4.detach()) and torch.equal(x3d.grad, x4d.grad[:, 0])
    xb = x.to(DEV).bfloat16().requires_grad_(True)
    lb = BoundaryLoss()(xb, td)
    lb.backward()
    assert xb.grad.dtype == torch.bfloat16 and torch.isfinite(lb)


def test_augmented_loss_is_the_sum_of_the_two_references():
    from vaeunet_amd.loss import BoundaryAugmentedLoss, MASegmentationLoss, boundary_loss
    x, t, phis = _module_inputs(False)
    td = t.to(DEV)
    crit = BoundaryAugmentedLoss(MASegmentationLoss(), weight=0.05, clip=2.5).to(DEV)
    w = float(np.float32(0.05))                      # the buffer is float32
    xd = x.to(DEV).requires_grad_(True)
    total = crit(xd, td)
    total.backward()
    assert float(crit.weight) == w and crit.weight.device.type == "cuda"
    xm, tm = x.flatten(), t.flatten().float()
    cfg = (0.75, 2.0, 1.0, 0.5, 0.5, False)
    f64, f32 = focal_dice_ref(xm, tm, *cfg), focal_dice_ref(xm, tm, *cfg, dtype=torch.float32)
    b64, b32 = _refs(x, phis[2.5], gout=w)
    # last_parts = [base, boundary]: each what its own module gives, bitwise
    parts = crit.last_parts
    assert parts.shape == (2,) and parts.device.type == "cuda" and not parts.requires_grad
    x1 = x.to(DEV)
    assert float(parts[0]) == float(MASegmentationLoss()(x1, td))
    assert float(parts[1]) == float(boundary_loss(x1, td, clip=2.5))
    # the total: base + w * boundary in fp32, two roundings on top of the parts
    want = float(parts[0]) + w * float(parts[1])
    assert abs(float(total.detach()) - want) <= 2 * U * (abs(float(parts[0])) + abs(w * float(parts[1])))
    n = x.numel()
    unit = U * float(b64["sums"][1]) / n
    assert in_units(parts[1], b64["loss"], unit) <= 4 * max(in_units(b32["loss"], b64["loss"], unit), 1.0)
    assert abs(float(parts[0]) - float(f64["loss"])) <= 16 * U * float(f64["loss"])
    # gradients: within the sum of the two bounds, plus the one fp32 addition autograd makes (u * the sum of the
    # magnitudes of the two terms covers its rounding)
    r_f, r_b = focal_grad_ratio(f32["grad"], f64), grad_ratio(b32["grad"], b64)
    got = xd.grad.detach().cpu().double().flatten()
    bound = 4 * r_f * U * f64["sabs"] + 4 * r_b * U * b64["sabs"] + 2 * TINY + U * (f64["grad"].abs() + b64["grad"].abs())
    err = (got - (f64["grad"] + b64["grad"])).abs()
    print(f"augmented: worst error / bound {float((err / bound).max()):.3g} (CPU ratios: focal {r_f:.3g}, boundary {r_b:.3g})")
    assert (err <= bound).all()
    # set_weight: another weight, the same parts
    crit.set_weight(0.5)
    x2 = x.to(DEV).requires_grad_(True)
    total2 = crit(x2, td)
    assert torch.equal(crit.last_parts, parts)
    assert abs(float(total2.detach()) - (float(parts[0]) + 0.5 * float(parts[1]))) <= 2 * U * (
        abs(float(parts[0])) + abs(0.5 * float(parts[1])))


def _capture(crit, x, t):
    """the forward and backward of crit(x, t) as one graph -> (graph, static loss, static gradient)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(crit(x, t), x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = crit(x, t)
        (grad,) = torch.autograd.grad(loss, x)
    return graph, loss, grad


def test_graph_replay_equals_eager_and_set_weight_needs_no_recapture():
    from vaeunet_amd.loss import BoundaryAugmentedLoss, MASegmentationLoss
    x, t, _ = _module_inputs(False)
    xd, td = x.to(DEV).requires_grad_(True), t.to(DEV)
    crit = BoundaryAugmentedLoss(MASegmentationLoss(), weight=0.01, clip=2.5)
    graph, loss, grad = _capture(crit, xd, td)
    seen = []
    for w in (0.01, 0.3, 0.0):
        crit.set_weight(w)
        graph.replay()
        torch.cuda.synchronize()
        gl, gg = loss.detach().clone(), grad.clone()
        el = crit(xd, td)
        (eg,) = torch.autograd.grad(el, xd)
        assert torch.equal(gl, el.detach()) and torch.equal(gg, eg), w                 # replay = eager, bitwise
        seen.append((float(gl), gg))
    assert seen[0][0] != seen[1][0] and not torch.equal(seen[0][1], seen[1][1])
    base, bnd = (float(v) for v in crit.last_parts)
    assert seen[2][0] == base and bnd != 0.0
    assert abs(seen[1][0] - (base + float(np.float32(0.3)) * bnd)) <= 2 * U * (abs(base) + abs(0.3 * bnd))
    # two runs are bitwise equal
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, torch.tensor(seen[2][0], device=DEV)) and torch.equal(grad, seen[2][1])


def test_forward_and_backward_do_not_synchronise():
    from vaeunet_amd.loss import BoundaryAugmentedLoss, BoundaryLoss, MASegmentationLoss, boundary_loss
    x, t, phis = _module_inputs(True)
    xd, td, pd = x.to(DEV).requires_grad_(True), t.to(DEV), phis[None].to(DEV).contiguous(memory_format=CL)
    crit, plain = BoundaryAugmentedLoss(MASegmentationLoss(), clip=4.0), BoundaryLoss()

    def step():
        crit(xd, td).backward()
        (3 * plain(xd, td)).backward()
        boundary_loss(xd, phi=pd).backward()
        crit.set_weight(0.2)
    step()                                        # first use: library load, the weight moves to the device
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            enforced = False
        except RuntimeError:
            enforced = True
        if enforced:
            step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not enforced:
        pytest.skip("this torch build does not enforce torch.cuda.set_sync_debug_mode('error') "
                    "(a .item() did not raise), so the absence of host syncs cannot be asserted")
    assert torch.isfinite(xd.grad).all()


def test_op_parity_and_opcheck():
    from vaeunet_amd import ops  # noqa: F401  (registers the ops)
    from vaeunet_amd.loss import boundary_loss
    v = torch.ops.vaeunet
    for cl in (False, True):
        x, t, phis = _module_inputs(cl)
        phi = phis[None]
        pd = phi.to(DEV).contiguous(memory_format=CL) if cl else phi.to(DEV)
        xd = x.to(DEV).requires_grad_(True)
        loss, sums = v.boundary_loss(xd, pd)
        assert loss.shape == () and sums.shape == (3,) and sums.dtype == torch.float64
        (3 * loss).backward()
        _check_module(loss.detach(), xd.grad, x, phi, 3.0, f"op cl={cl}")
        check_loss_from_sums(loss.detach(), sums, x.numel())
        xf = x.to(DEV).requires_grad_(True)
        lf = boundary_loss(xf, phi=pd)
        (3 * lf).backward()
        assert torch.equal(lf.detach(), loss.detach()) and torch.equal(xf.grad, xd.grad)
    g = torch.Generator().manual_seed(7)
    xr = (torch.randn(2, 1, 8, 8, generator=g) * 3).to(DEV).requires_grad_(True)
    pr = (torch.randn(2, 1, 8, 8, generator=g) * 5).to(DEV)
    torch.library.opcheck(v.boundary_loss.default, (xr, pr),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
