"""The training objective's kernels of csrc/loss.hip -- BCE + Dice (forward
sums, on-device loss, backward), KL with free bits, the hard Dice score and
the double-precision sum of squares -- each called through the C ABI on
guarded buffers and compared with fp64 CPU references (tests/ref_small.py).

Bounds (u = 2^-24; r_cpu = the error of the same formulas evaluated by torch
in float32 on the CPU on the same inputs, in the same units -- the convention
of test_gpu_ma_loss.py; sabs = the formula on |operands|):

  the four sums, KL value   relative error <= 4 max(r_cpu, 1) u  (a zero sum exactly)
  BCE / Dice gradient       |g - g_64| <= 4 max(r_cpu, 1) u sabs + 2^-126, per element,
                            g_64 built from the kernel's own sums
  parts[0] (BCE mean)       bitwise float(sums[0] / n)
  parts[1] (Dice loss)      4 max(r_cpu, 1) u (1 + dice) from the kernel's sums
  loss                      2 u (|w_bce bce| + |w_dice dl|) from the kernel's parts
  KL gradients              4 max(r_cpu, 1) u sabs + 2^-126 per element; exactly 0 above
                            the +-100 clamp and below free_bits, exactly half at a tie;
                            at non-finite inputs NaN / 0 where torch's float32 autograd of
                            oracle.cpu_ref.kl_with_free_bits has them
  vu_dice_score             counts exactly, the score bitwise (fp32 formula)
  vu_sumsq                  relative error <= 1e-12

The float32 BCE formula is the kernel's documented one (ATen's (1 - t) x + m +
log(exp(-m) + exp(-x - m))), which cancels for a confidently right logit; the
float64 reference is utils/loss.py's log1p form.

Worst ratios measured on the MI355X (the CPU's float32 figure in brackets):
  sums         BCE 0.07 (0.11) on mixed logits; 3.5e5 (3.5e5) when every logit <= -12 and
               1.7e7 (1.7e7) at n = 1, 2 (x = -90, -30: ATen's form returns 0 for 8e-40 and 9e-14);
               sum p t 0.33 (0.33), sum p 0.083 (0.076) for n >= 7, sum t exact
  gradient     random elements 5.3 (5.3), planted ones 2.3 (2.3) with a BCE term; with w_bce = 0
               1.9e6 (1.9e6) and 1.7e7 (1.7e7): p (1 - p) loses its bits for a large logit (it is
               0 at x = 17) on either machine and nothing else is in sabs.  The planted logits
               and the random remainder are each held to their own r_cpu.
  Dice loss    0.68 (0.68)
  KL           value 0.71 (0.71), gmu 1.33 (1.33), glv 1.59 (1.29)
The tightest case is glv at (64, 64) with non-finite inputs planted: 1.59 against 4 * 1.29.
"""
import ctypes
import functools

import pytest
import torch

import ref_small as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32, F64 = torch.float32, torch.float64
NAN, INF = float("nan"), float("inf")
BIG = 2 ** 20 + 5                      # > 1024 blocks * 256 threads * 4: the capped grid strides
N_LIST = [1, 2, 7, 255, 256, 257, 4099, BIG]
SPECIAL = [-90.0, -30.0, -1e-3, 0.0, 1e-3, 30.0, 90.0, 17.0, -17.0]


def _lib():
    from vaeunet_amd import _lib as L
    return L


def _call(name, *args):
    L = _lib()
    L.call(name, *args, L.stream())
    torch.cuda.synchronize()


def _raw(name, argtypes):
    """an exported wrapper that _lib's signature table does not list"""
    fn = getattr(_lib().lib(), name)
    fn.restype, fn.argtypes = ctypes.c_int, argtypes
    return fn


def _ptr(t):
    return _lib().ptr(t)


def _put(x, offset=0):
    t, g = R.guarded(tuple(x.shape), x.dtype, DEV, offset=offset)
    t.copy_(x)
    return t, g


def _f32(v):
    return float(torch.tensor(v, dtype=F32))


def _rel_u(got, ref):
    got, ref = float(got), float(ref)
    if got == ref:
        return 0.0
    return abs(got - ref) / (R.U32 * abs(ref)) if ref != 0 else INF


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    it = torch.int32 if a.dtype == F32 else torch.int64
    return a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def _ws():
    return R.guarded(_lib().query("vu_loss_workspace_bytes") // 8, F64, DEV)


# ----------------------------------------------------------------------------
# BCE + Dice
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bd_inputs(n, soft, kind="plain"):
    g = torch.Generator().manual_seed(2000 + n + (7 if soft else 0))
    if kind == "cold":                     # every logit <= -12, no positive target
        return -12.0 - 8.0 * torch.rand(n, generator=g), torch.zeros(n)
    x = torch.randn(n, generator=g) * 4.0
    k = min(n, len(SPECIAL))
    x[:k] = torch.tensor(SPECIAL[:k])
    t = torch.rand(n, generator=g) if soft else (torch.rand(n, generator=g) < 0.03).float()
    if kind == "faint":                    # soft targets whose sum stays below smooth / 2
        t = t * (0.2 / max(float(t.sum()), 1e-30))
    if kind == "nan":
        x[min(n - 1, 1234)] = NAN
    return x, t


def run_bce_dice(x, t, smooth, wb, wd, gscale=None, offs=(0, 0, 0), parts=True, loss=True):
    """vu_bce_dice_fwd2 + vu_bce_dice_bwd on guarded buffers
    -> dict(sums, loss, parts, grad), guards (checked)"""
    n = x.numel()
    xd, gx = _put(x, offs[0])
    td, gt = _put(t, offs[1])
    grad, gg = R.guarded(n, F32, DEV, offset=offs[2])
    sums, gs = R.guarded(4, F64, DEV)
    lo, gl = R.guarded(1, F32, DEV)
    pa, gp = R.guarded(2, F32, DEV)
    ws, gw = _ws()
    gsc = None if gscale is None else torch.tensor([gscale], dtype=F32, device=DEV)
    _call("vu_bce_dice_fwd2", _ptr(xd), _ptr(td), n, _ptr(sums), smooth, wb, wd, _ptr(lo) if loss else None,
          _ptr(pa) if parts and loss else None, _ptr(ws))
    _call("vu_bce_dice_bwd", _ptr(xd), _ptr(td), n, _ptr(sums), smooth, wb, wd, _ptr(gsc), _ptr(grad))
    for gd, what in ((gx, "x"), (gt, "t"), (gg, "grad"), (gs, "sums"), (gl, "loss"), (gp, "parts"), (gw, "workspace")):
        gd.check(f"bce_dice {what}")
    same = lambda a, b: torch.equal(a.cpu().nan_to_num(nan=7.0), b.nan_to_num(nan=7.0))
    assert same(xd, x) and same(td, t), "inputs written"
    if not loss:
        assert float(lo) == R.SENTINEL and bool((pa == R.SENTINEL).all())
    elif not parts:
        assert bool((pa == R.SENTINEL).all())
    return dict(sums=sums.cpu(), loss=lo.cpu(), parts=pa.cpu(), grad=grad.cpu())


def check_bce_dice(x, t, got, smooth, wb, wd, gscale, what, log=None, parts=True):
    """every bound of the module docstring"""
    n = x.numel()
    gs = 1.0 if gscale is None else gscale
    s64, _ = R.bce_dice_fwd_ref(x, t)
    s32, _ = R.bce_dice_fwd_ref(x, t, F32)
    ratios = {}
    for k, name in enumerate(("bce", "sum_pt", "sum_p", "sum_t")):
        if torch.isnan(s64[k]):
            assert torch.isnan(got["sums"][k]) and torch.isnan(s32[k]), f"{what}: {name} must be NaN"
            continue
        r_cpu, r_hip = _rel_u(s32[k], s64[k]), _rel_u(got["sums"][k], s64[k])
        ratios[name] = (r_hip, r_cpu)
        assert r_hip <= 4 * max(r_cpu, 1.0), f"{what}: {name} {r_hip:.3g} (CPU float32 {r_cpu:.3g})"
    # loss and parts from the kernel's own sums
    ks = got["sums"]
    bce = (ks[0] / n).float()
    dl64, dsabs = R.dice_loss_from_sums(ks, smooth)
    dl32, _ = R.dice_loss_from_sums(ks, smooth, F32)
    if parts:
        if torch.isnan(bce):
            assert bool(torch.isnan(got["parts"][0])), f"{what}: parts[0] must be NaN"
        else:
            assert _same_bits(got["parts"][0:1], bce.reshape(1)), f"{what}: parts[0]"
        r = R.assert_trans(got["parts"][1], dl64, dl32, dsabs, f"{what} dice loss", log)
        ratios["dice_loss"] = r
        want = _f32(wb) * float(got["parts"][0]) + _f32(wd) * float(got["parts"][1])
        tol = 2 * R.U32 * (abs(_f32(wb) * float(got["parts"][0])) + abs(_f32(wd) * float(got["parts"][1])))
        if torch.isnan(bce):
            assert torch.isnan(got["loss"]).all(), f"{what}: loss must be NaN"
        else:
            assert abs(float(got["loss"]) - want) <= tol, f"{what}: loss {float(got['loss'])} vs {want}"
    g64, sabs = R.bce_dice_bwd_ref(x, t, ks, smooth, wb, wd, gs)
    g32, _ = R.bce_dice_bwd_ref(x, t, ks, smooth, wb, wd, gs, F32)
    planted = torch.arange(n) < len(SPECIAL)
    ratios["grad"] = R.assert_trans(got["grad"], g64, g32, sabs, f"{what} gradient", log, split=planted)
    print(f"{what}: sums " + ", ".join(f"{k} {v[0]:.3g} ({v[1]:.3g})" for k, v in ratios.items()
                                      if k.startswith(("bce", "sum"))))
    return ratios


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("n", N_LIST)
def test_bce_dice_sizes(n, soft):
    x, t = bd_inputs(n, soft)
    got = run_bce_dice(x, t, 1.0, 0.5, 0.5, gscale=None)
    check_bce_dice(x, t, got, 1.0, 0.5, 0.5, None, f"n={n} soft={soft}")
    again = run_bce_dice(x, t, 1.0, 0.5, 0.5, gscale=None)
    for k in got:
        assert _same_bits(got[k], again[k]), f"{k} differs between two launches"


@pytest.mark.parametrize("weights", [(0.5, 0.5), (1.0, 0.0), (0.0, 1.0), (0.3, 0.7)])
@pytest.mark.parametrize("smooth", [0.25, 1.0, 4.0])
def test_bce_dice_constants(smooth, weights):
    wb, wd = weights
    for n, soft in ((7, True), (4099, False)):
        x, t = bd_inputs(n, soft)
        got = run_bce_dice(x, t, smooth, wb, wd, gscale=-2.5)
        check_bce_dice(x, t, got, smooth, wb, wd, -2.5, f"n={n} smooth={smooth} w={weights}")
    if wd == 0.0:
        # no Dice term: the gradient is g w_bce (p - t) / n whatever the sums
        assert float(got["grad"][3]) == pytest.approx(-2.5 * wb * (0.5 - float(t[3])) / n, rel=1e-6)


def test_bce_dice_clamp_branch():
    """every logit <= -12, t = 0: sum p < smooth / 2 and sum t < smooth / 2, so
    both clamps hold and no Dice gradient flows through sum p (mp = 0)"""
    x, t = bd_inputs(7, False, "cold")
    assert float(x.max()) <= -12.0 and float(t.sum()) == 0.0
    for smooth in (0.25, 1.0):
        assert float(torch.sigmoid(x.double()).sum()) < smooth / 2
        got = run_bce_dice(x, t, smooth, 0.5, 0.5)
        check_bce_dice(x, t, got, smooth, 0.5, 0.5, None, f"cold smooth={smooth}")
        # Dice loss = 1 - smooth / (2 smooth) = 1/2 up to the 2 I term (I = 0 here)
        assert float(got["parts"][1]) == 0.5
        # mp = 0, t = 0: the gradient is the BCE's alone
        p = torch.sigmoid(x.double())
        assert torch.allclose(got["grad"].double(), 0.5 * p / 7, rtol=1e-5, atol=0)


def test_bce_dice_faint_targets():
    """soft targets with sum t < smooth / 2 <= sum p: the target clamp alone"""
    x, t = bd_inputs(255, True, "faint")
    assert float(t.double().sum()) < 0.5 < float(torch.sigmoid(x.double()).sum())
    got = run_bce_dice(x, t, 1.0, 0.5, 0.5)
    check_bce_dice(x, t, got, 1.0, 0.5, 0.5, None, "faint")


@pytest.mark.parametrize("n", [7, 4099])
def test_bce_dice_nan_logit(n):
    """one NaN logit: p -> 0 in the Dice sums; the BCE sum, the loss and that
    element's gradient are NaN, exactly where torch's float32 autograd of
    oracle.cpu_ref.combined_loss has them"""
    from oracle import cpu_ref
    x, t = bd_inputs(n, False, "nan")
    at = min(n - 1, 1234)
    assert int(torch.isnan(x).sum()) == 1 and bool(torch.isnan(x[at]))
    xr = x.clone().requires_grad_(True)
    lt = cpu_ref.combined_loss(xr, t)
    lt.backward()
    got = run_bce_dice(x, t, 1.0, 0.5, 0.5)
    assert torch.equal(torch.isnan(got["grad"]), torch.isnan(xr.grad))
    assert bool(torch.isnan(got["grad"][at])) and int(torch.isnan(got["grad"]).sum()) == 1
    assert bool(torch.isnan(lt)) and bool(torch.isnan(got["loss"]).all()) and bool(torch.isnan(got["sums"][0]))
    assert bool(torch.isnan(got["parts"][0])) and bool(torch.isfinite(got["parts"][1]))
    assert bool(torch.isfinite(got["sums"][1:]).all())
    check_bce_dice(x, t, got, 1.0, 0.5, 0.5, None, f"nan n={n}")
    # the Dice sums are those of the input without that element
    keep = torch.arange(n) != at
    s_clean, _ = R.bce_dice_fwd_ref(x[keep], t[keep])
    s_nan, _ = R.bce_dice_fwd_ref(x, t)
    assert torch.allclose(s_nan[1:3], s_clean[1:3], rtol=1e-14, atol=0)


def test_bce_dice_output_forms():
    """loss == NULL (and the vu_bce_dice_fwd wrapper), parts == NULL,
    gscale == NULL: the same sums and gradient bits, nothing else written"""
    L = _lib()
    n = 4099
    x, t = bd_inputs(n, True)
    full = run_bce_dice(x, t, 1.0, 0.5, 0.5, gscale=1.0)
    nog = run_bce_dice(x, t, 1.0, 0.5, 0.5, gscale=None)
    assert _same_bits(full["grad"], nog["grad"])
    nol = run_bce_dice(x, t, 1.0, 0.5, 0.5, loss=False)
    nop = run_bce_dice(x, t, 1.0, 0.5, 0.5, parts=False)
    assert _same_bits(nol["sums"], full["sums"]) and _same_bits(nop["sums"], full["sums"])
    assert _same_bits(nop["loss"], full["loss"]) and _same_bits(nol["grad"], full["grad"])
    fwd = _raw("vu_bce_dice_fwd", [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p])
    xd, gx = _put(x)
    td, gt = _put(t)
    sums, gs = R.guarded(4, F64, DEV)
    ws, gw = _ws()
    assert fwd(_ptr(xd), _ptr(td), n, _ptr(sums), _ptr(ws), L.stream()) == 0
    torch.cuda.synchronize()
    for gd in (gx, gt, gs, gw):
        gd.check("vu_bce_dice_fwd")
    assert _same_bits(sums, full["sums"])


@pytest.mark.parametrize("offs", [(1, 1, 1), (1, 0, 1), (0, 1, 0)])
def test_bce_dice_misaligned(offs):
    """pointers one float off a 16-byte boundary"""
    n = 4099
    x, t = bd_inputs(n, True)
    base = run_bce_dice(x, t, 1.0, 0.5, 0.5)
    got = run_bce_dice(x, t, 1.0, 0.5, 0.5, offs=offs)
    for k in got:
        assert _same_bits(got[k], base[k]), k
    check_bce_dice(x, t, got, 1.0, 0.5, 0.5, None, f"offs={offs}")


# ----------------------------------------------------------------------------
# KL with free bits
# ----------------------------------------------------------------------------
def _find_tie(fb):
    """a finite pair (mu, lv) whose float32 kl equals fb exactly; lv = 0 first
    (exp(0) = 1 in every libm, so the tie does not hang on the last bit of expf)"""
    mus = torch.arange(0, 65, dtype=F32) / 16
    lvs = torch.tensor([0.0] + [j / 4 for j in range(-8, 9) if j != 0], dtype=F32)
    for lv in lvs:
        kl = 0.5 * (mus * mus + torch.exp(lv) - lv - 1)
        hit = (kl == torch.tensor(fb, dtype=F32)).nonzero()
        if hit.numel():
            return float(mus[hit[0, 0]]), float(lv)
    return None


@functools.lru_cache(maxsize=None)
def kl_inputs(B, L, nonfinite):
    """-> mu, lv [B, L], dict name -> flat index of the planted elements"""
    g = torch.Generator().manual_seed(3000 + B + L)
    mu = torch.randn(B, L, generator=g)
    lv = torch.randn(B, L, generator=g)
    tie = _find_tie(0.5)
    assert tie is not None, "no float32 pair with kl == 0.5"
    plant = [("mu_high", 15.0, 0.0), ("lv_neg_high", 0.0, -250.0), ("lv_neg_in", 0.0, -150.0), ("zero", 0.0, 0.0),
             ("tie", tie[0], tie[1]), ("lv_overflow", 0.3, 89.0)]
    if nonfinite:
        plant += [("mu_nan", NAN, 0.2), ("mu_pinf", INF, 0.2), ("mu_ninf", -INF, 0.2), ("lv_nan", 0.3, NAN),
                  ("lv_pinf", 0.3, INF), ("lv_ninf", 0.3, -INF)]
    n = B * L
    where = {}
    for i, (name, m, v) in enumerate(plant[:n]):
        at = (i * 37) % n if n >= 2 * len(plant) else i
        assert at not in where.values()
        mu.view(-1)[at], lv.view(-1)[at] = m, v
        where[name] = at
    return mu, lv, where


def run_kl(mu, lv, fb, gscale=None, value=True, grads=True, wrapper=False):
    L = _lib()
    B, Ld = mu.shape
    md, gm = _put(mu)
    ld, gl = _put(lv)
    val, gv = R.guarded(1, F32, DEV)
    gmu, ggm = R.guarded((B, Ld), F32, DEV)
    glv, ggl = R.guarded((B, Ld), F32, DEV)
    gsc = None if gscale is None else torch.tensor([gscale], dtype=F32, device=DEV)
    pv, pm, pl = _ptr(val) if value else None, _ptr(gmu) if grads else None, _ptr(glv) if grads else None
    if wrapper:
        fn = _raw("vu_kl_free_bits", [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
        assert fn(_ptr(md), _ptr(ld), B, Ld, fb, pv, pm, pl, L.stream()) == 0
        torch.cuda.synchronize()
    else:
        _call("vu_kl_free_bits2", _ptr(md), _ptr(ld), B, Ld, fb, _ptr(gsc), pv, pm, pl)
    for gd in (gm, gl, gv, ggm, ggl):
        gd.check("kl")
    if not value:
        assert float(val) == R.SENTINEL
    if not grads:
        assert bool((gmu == R.SENTINEL).all()) and bool((glv == R.SENTINEL).all())
    return val.cpu(), gmu.cpu(), glv.cpu()


def check_kl(mu, lv, where, fb, gscale, got, what):
    val, gmu, glv = got
    gs = 1.0 if gscale is None else gscale
    B = mu.shape[0]
    r64, r32 = R.kl_ref(mu, lv, fb, gs), R.kl_ref(mu, lv, fb, gs, F32)
    # no element but the planted ones decides its free-bits comparison within rounding
    if fb > 0:
        near = ((r64["kl32"].double() - _f32(fb)).abs() <= 1e-5 * _f32(fb)).flatten().nonzero().flatten().tolist()
        assert set(near) <= {where.get("tie", -1)}, f"{what}: unplanted near-ties at {near}"
    r_cpu, r_hip = _rel_u(r32["value"].float(), r64["value"]), _rel_u(val, r64["value"])
    print(f"{what}: value {r_hip:.3g} (CPU float32 {r_cpu:.3g})")
    assert r_hip <= 4 * max(r_cpu, 1.0), f"{what}: value {r_hip:.3g} (CPU float32 {r_cpu:.3g})"
    # non-finite inputs and the overflowing exp: the class torch's float32 autograd gives
    from oracle import cpu_ref
    mt, lt = mu.clone().requires_grad_(True), lv.clone().requires_grad_(True)
    (gs * cpu_ref.kl_with_free_bits(mt, lt, fb)).backward()
    odd = (~torch.isfinite(mu) | ~torch.isfinite(lv)).flatten()
    if "lv_overflow" in where:
        odd[where["lv_overflow"]] = True
    for name, g_hip, g_t in (("gmu", gmu, mt.grad), ("glv", glv, lt.grad)):
        a, b = g_hip.flatten()[odd], g_t.flatten()[odd]
        assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what}: {name} NaN pattern {a} vs torch {b}"
        assert torch.equal(a == 0, b == 0), f"{what}: {name} zero pattern {a} vs torch {b}"
    fin = ~odd
    for name, g_hip in (("gmu", gmu), ("glv", glv)):
        pick = lambda v: v.flatten()[fin]
        R.assert_trans(pick(g_hip), pick(r64[name]), pick(r32[name]), pick(r64[name + "_abs"]), f"{what} {name}")
    flat = lambda v: v.flatten()
    at = where.get
    if "mu_high" in where:
        assert float(flat(gmu)[at("mu_high")]) == 0.0 and float(flat(glv)[at("mu_high")]) == 0.0
    if "lv_neg_high" in where:
        assert float(flat(glv)[at("lv_neg_high")]) == 0.0
    if "lv_neg_in" in where and fb < 70:
        i = at("lv_neg_in")   # exp(-150) = 0 in float32: glv = -g / (2 B)
        assert float(flat(glv)[i]) == pytest.approx(-0.5 * gs / B, rel=1e-6)
    if "zero" in where:
        assert float(flat(gmu)[at("zero")]) == 0.0 and float(flat(glv)[at("zero")]) == 0.0
    if "tie" in where:
        i = at("tie")
        m, v = float(flat(mu)[i]), float(flat(lv)[i])
        assert float(r64["kl32"].flatten()[i]) == 0.5
        share = {0.5: 0.5}.get(fb, 1.0 if fb < 0.5 else 0.0)   # fb == kl: torch.max splits the gradient
        want_mu = torch.tensor(gs, dtype=F32) * share / torch.tensor(float(B), dtype=F32) * torch.tensor(m, dtype=F32)
        if v == 0.0:
            assert float(flat(gmu)[i]) == float(want_mu), f"{what}: tie share"
            assert float(flat(glv)[i]) == 0.0
    return r_hip, r_cpu


KL_SHAPES = [(1, 1), (8, 32), (3, 100), (64, 64)]


@pytest.mark.parametrize("fb", [0.0, 1e-3, 0.5])
@pytest.mark.parametrize("shape", KL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kl_finite(shape, fb):
    mu, lv, where = kl_inputs(*shape, False)
    got = run_kl(mu, lv, fb)
    check_kl(mu, lv, where, fb, None, got, f"kl {shape} fb={fb}")
    again = run_kl(mu, lv, fb)
    for a, b in zip(got, again):
        assert _same_bits(a, b)


@pytest.mark.parametrize("fb", [0.0, 1e-3, 0.5])
@pytest.mark.parametrize("shape", KL_SHAPES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_kl_nonfinite(shape, fb):
    mu, lv, where = kl_inputs(*shape, True)
    assert len(where) == 12
    got = run_kl(mu, lv, fb, gscale=0.75)
    check_kl(mu, lv, where, fb, 0.75, got, f"kl non-finite {shape} fb={fb}")


def test_kl_output_forms():
    mu, lv, where = kl_inputs(3, 100, False)
    base = run_kl(mu, lv, 1e-3)
    one = run_kl(mu, lv, 1e-3, gscale=1.0)
    wrap = run_kl(mu, lv, 1e-3, wrapper=True)
    for a, b, c in zip(base, one, wrap):
        assert _same_bits(a, b) and _same_bits(a, c)
    v_only = run_kl(mu, lv, 1e-3, grads=False)
    g_only = run_kl(mu, lv, 1e-3, value=False)
    assert _same_bits(v_only[0], base[0]) and _same_bits(g_only[1], base[1]) and _same_bits(g_only[2], base[2])
    scaled = run_kl(mu, lv, 1e-3, gscale=-2.0)
    assert _same_bits(scaled[0], base[0])                       # the value ignores gscale
    assert torch.equal(scaled[1], -2.0 * base[1]) and torch.equal(scaled[2].nan_to_num(nan=5.0),
                                                                  (-2.0 * base[2]).nan_to_num(nan=5.0))


# ----------------------------------------------------------------------------
# hard Dice score
# ----------------------------------------------------------------------------
def run_dice_score(x, t, epsilon, counts=True):
    n = x.numel()
    xd, gx = _put(x)
    td, gt = _put(t)
    score, gs = R.guarded(1, F32, DEV)
    cnt, gc = R.guarded(3, F64, DEV)
    ws, gw = _ws()
    _call("vu_dice_score", _ptr(xd), _ptr(td), n, epsilon, _ptr(score), _ptr(cnt) if counts else None, _ptr(ws))
    for gd in (gx, gt, gs, gc, gw):
        gd.check("dice_score")
    if not counts:
        assert bool((cnt == R.SENTINEL).all())
    return score.cpu(), cnt.cpu()


@pytest.mark.parametrize("epsilon", [1e-6, 1.0])
@pytest.mark.parametrize("n", N_LIST)
def test_dice_score(n, epsilon):
    g = torch.Generator().manual_seed(4000 + n)
    x = torch.rand(n, generator=g)
    t = (torch.rand(n, generator=g) < 0.4).float()
    # exactly 0.5 (not counted, either side), its neighbours, NaN (not counted)
    above, below = float(torch.nextafter(torch.tensor(0.5), torch.tensor(1.0))), float(
        torch.nextafter(torch.tensor(0.5), torch.tensor(0.0)))
    for i, (a, b) in enumerate([(0.5, 1.0), (1.0, 0.5), (0.5, 0.5), (above, 1.0), (below, 1.0), (NAN, 1.0), (1.0, NAN)]):
        if n >= 255:
            x[i * 3], t[i * 3] = a, b
    if n == 1:
        x[0], t[0] = 0.5, 0.5
    if n == 2:
        x[:], t[:] = torch.tensor([0.5, above]), torch.tensor([1.0, 1.0])
    score, cnt = run_dice_score(x, t, epsilon)
    ref_s, ref_c = R.dice_score_ref(x, t, epsilon)
    assert torch.equal(cnt, ref_c), (cnt, ref_c)
    assert _same_bits(score, ref_s.reshape(1)), (float(score), float(ref_s))
    if n == 1:
        assert float(score) == 1.0 and not cnt.any()        # 0.5 on both sides: all empty
    if n == 2:
        assert cnt.tolist() == [1.0, 2.0, 1.0]
    s2, _ = run_dice_score(x, t, epsilon, counts=False)
    assert _same_bits(s2, score)


def test_dice_score_all_empty():
    x = torch.full((4099,), 0.5)
    t = torch.zeros(4099)
    x[5] = NAN
    for epsilon in (1e-6, 1.0):
        score, cnt = run_dice_score(x, t, epsilon)
        assert float(score) == 1.0 and not cnt.any()


# ----------------------------------------------------------------------------
# sum of squares
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", N_LIST)
def test_sumsq(n):
    """accumulated in double: 1e-30 and 1e30 both count (a float square would
    underflow to 0 / overflow to inf)"""
    g = torch.Generator().manual_seed(5000 + n)
    cases = [torch.randn(n, generator=g), torch.full((n,), 1e-30), torch.randn(n, generator=g) * 1e-30]
    big = torch.randn(n, generator=g)
    big[0] = 1e30
    cases.append(big)
    for x in cases:
        xd, gx = _put(x)
        out, go = R.guarded(1, F64, DEV)
        ws, gw = _ws()
        _call("vu_sumsq", _ptr(xd), n, _ptr(out), _ptr(ws))
        for gd in (gx, go, gw):
            gd.check("sumsq")
        ref = float((x.double() ** 2).sum())
        assert ref > 0 and abs(float(out) - ref) <= 1e-12 * ref, (float(out), ref)
