"""CPU checks of tests/bn_ref.py and tests/attention_ref.py themselves, and of
the case lists of tests/test_gpu_bn_kernels.py and
tests/test_gpu_attention_ref.py:

  * every reference equals torch autograd in fp64 (1e-12 relative): BatchNorm
    as a batch_norm(training = True / False) + ReLU module, the gate as
    oracle.cpu_ref.attention_gate's formulas from s onward;
  * every seeded input set is free of ReLU pre-activations near zero
    (bn_near_zero's 1e-3 cancellation criterion, its analogue over the four
    terms of s): the count is 0, so no GPU comparison leaves elements out;
  * for every bound of the GPU tests, a float32 restatement of the kernel's
    formula (its operation order, torch float32 ops) passes that bound on that
    case's inputs: no bound is tighter than float32 arithmetic allows.
"""
import pytest
import torch
import torch.nn.functional as Fn

import attention_ref as A
import bn_ref as B
from bn_ref import BF16, F32
from ref_small import assert_lin, assert_trans

DTYPES = [F32, BF16]
DT_ID = {F32: "f32", BF16: "bf16"}.get


def close(got, want, scale=None):
    """1e-12 relative to the magnitude of the operands (``scale``; |want| without it)"""
    s = want.abs() if scale is None else scale
    assert bool(((got - want).abs() <= 1e-12 * s + 1e-300).all()), float(((got - want).abs() / (s + 1e-300)).max())


# ----------------------------------------------------------------------------
# BatchNorm references vs autograd
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("P,C,tile_rows", [(1029, 8, 128), (53, 24, 7), (300, 3, 300), (2, 64, 1)])
def test_bn_refs_match_autograd(P, C, tile_rows, train, relu):
    inp = B.bn_inputs(P, C, F32)
    fin = B.finalize_inputs(4, 8, C)
    g = torch.Generator().manual_seed(3)
    y = (torch.randn(P, C, generator=g, dtype=torch.float64) * 2 + 0.5)
    dy = inp["dy"].double()
    gamma, beta = fin["gamma"].double(), fin["beta"].double()
    rm, rv = fin["rm"].double(), fin["rv"].double()
    # torch: NCHW with the pixels as a batch of 1 x 1 images
    yr = y.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm_t, rv_t = rm.clone(), rv.clone()
    # (momentum and eps as the float32 values the kernels are handed)
    mom32, eps32 = float(torch.tensor(B.MOM, dtype=F32)), float(torch.tensor(B.EPS, dtype=F32))
    z = Fn.batch_norm(yr[:, :, None, None], rm_t, rv_t, gr, br, training=train, momentum=mom32, eps=eps32)[:, :, 0, 0]
    out = torch.relu(z) if relu else z
    out.backward(dy)
    if train:
        psum, pm2 = B.stats_of(y, tile_rows, torch.float64)
        st = B.bn_stats_ref(psum, pm2, tile_rows, P, gamma, beta, rm, rv, B.MOM, B.EPS)
        close(st["mean"], y.mean(0), y.abs().mean(0))
        close(st["var"], y.var(0, unbiased=False))
        close(st["invstd"], 1 / torch.sqrt(y.var(0, unbiased=False) + eps32))
        close(st["rm"], rm_t, st["rm_abs"])
        close(st["rv"], rv_t, st["rv_abs"])
    else:
        st = B.bn_eval_ref(gamma, beta, rm, rv, B.EPS)
    f, fabs = B.bn_apply_ref(y, st["scale"], st["shift"], relu)
    close(f, out.detach(), fabs)
    assert bool((fabs >= f.abs() * (1 - 1e-12)).all())
    # backward: sums, finish, apply
    part, pabs = B.bn_bwd_sums_ref(dy, y, st["scale"], st["shift"], st["mean"], st["invstd"], relu)
    fi = B.bn_finish_ref(part, pabs, gamma, st["invstd"], P, int(train))
    close(fi["dgamma"], gr.grad, fi["dgamma_abs"])
    close(fi["dbeta"], br.grad, fi["dbeta_abs"])
    dx, dxabs = B.bn_bwd_apply_ref(dy, y, st["scale"], st["shift"], st["mean"], fi["coef"], relu)
    close(dx, yr.grad, dxabs)
    assert bool((dxabs >= dx.abs() * (1 - 1e-12)).all())
    # the per-block form sums to the dense one
    p4, a4 = B.bn_bwd_sums_ref(dy, y, st["scale"], st["shift"], st["mean"], st["invstd"], relu, nblk=3)
    close(p4.sum(0), part[0], pabs[0])
    close(a4.sum(0), pabs[0])


def test_bn_fused_residual_pool_window_refs():
    g = torch.Generator().manual_seed(9)
    N, H, W, C = 2, 6, 10, 8
    y = torch.randn(N * H * W, C, generator=g, dtype=torch.float64)
    res = torch.randn(N * H * W, C, generator=g, dtype=torch.float64)
    sc, sh, rsc, rsh = (torch.randn(C, generator=g, dtype=torch.float64) for _ in range(4))
    f, fabs = B.bn_apply_ref(y, sc, sh, True, res, rsc, rsh)
    close(f, torch.relu(y * sc + sh + (res * rsc + rsh)), fabs)
    f, fabs = B.bn_apply_ref(y, sc, sh, False, res)
    close(f, y * sc + sh + res, fabs)
    a = f.reshape(N, H, W, C)
    assert torch.equal(B.pool2_ref(a), Fn.max_pool2d(a.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
    s, sabs = B.chan_sum_ref(a, 2, 3, 3, 4)
    close(s, a[:, 2:5, 3:7].sum((0, 1, 2)), sabs)


# ----------------------------------------------------------------------------
# BatchNorm: input conditions
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("layout", B.LAYOUTS, ids=B.layout_id)
def test_bn_inputs_have_no_mask_edges(layout, dt):
    C = layout[0]
    for P in B.pixel_counts(C):
        for seed in (51, 52):
            inp = B.bn_inputs(P, C, dt, seed)
            assert torch.equal(inp["x"].to(dt).float(), inp["x"]) and torch.equal(inp["dy"].to(dt).float(), inp["dy"])
            assert B.near_zero_count(inp["x"], inp["scale"], inp["shift"]) == 0
    for P, C2 in ((128 * 16 * 16, 128), (1, 128), (1029, 64), (777, 32), (4, C), (120, C), (1836, C)):
        inp = B.bn_inputs(P, C2, dt)
        assert B.near_zero_count(inp["x"], inp["scale"], inp["shift"]) == 0


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("C", [8, 64, 24, 3])
def test_planted_mask_inputs(C, dt):
    """the planted elements cancel exactly when unfused, have a fused residual
    of either sign in some channel, and nothing else is near the edge"""
    x, scale, shift, planted = B.planted_mask_inputs(1024, C, dt)
    assert torch.equal(x.to(dt).float(), x)
    unfused = x * scale + shift
    assert not bool(unfused[planted].any())
    fused = (x.double() * scale.double() + shift.double())[planted]      # exact: 24 + 24 bits
    assert bool((fused > 0).any()) and bool((fused < 0).any())
    assert int((B.bn_near_zero(x, scale, shift) & ~planted).sum()) == 0
    assert int(planted.sum(0).min()) > 0


# ----------------------------------------------------------------------------
# BatchNorm: float32 restatements pass every bound
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("layout", B.DENSE + B.SCALAR[:2], ids=B.layout_id)
def test_bn_f32_restatements_pass_bounds(layout, dt):
    C = layout[0]
    for P in B.pixel_counts(C):
        inp = B.bn_inputs(P, C, dt)
        x, dy, sc, sh, mu, is_, gm, k = (inp[n] for n in ("x", "dy", "scale", "shift", "mean", "invstd", "gamma", "k"))
        for relu in (1, 0):
            ref, sabs = B.bn_apply_ref(x, sc, sh, relu)
            B.assert_el(B.bn_apply_f32(x, sc, sh, relu, dt), ref, sabs, B.APPLY_N, dt, "apply")
            ref, sabs = B.bn_apply_ref(x, sc, sh, relu, inp["res"], inp["rscale"], inp["rshift"])
            B.assert_el(B.bn_apply_f32(x, sc, sh, relu, dt, inp["res"], inp["rscale"], inp["rshift"]), ref, sabs,
                        B.FUSED_N, dt, "fused apply")
            ref, sabs = B.bn_bwd_apply_ref(dy, x, sc, sh, mu, k, relu)
            B.assert_el(B.bn_bwd_apply_f32(dy, x, sc, sh, mu, k, relu, dt), ref, sabs, B.BWD_APPLY_N, dt, "bwd apply")
            part, pabs = B.bn_bwd_sums_ref(dy, x, sc, sh, mu, is_, relu)
            for fused_mask in (True, False):     # chan_partial_kernel's fmaf, chan_partial_scalar's expression
                s32 = B.bn_bwd_sums_f32(dy, x, sc, sh, mu, is_, relu, fused_mask)
                assert_lin(s32, part[0], pabs[0], "sums")
            for train in (1, 0):
                fi = B.bn_finish_ref(part, pabs, gm, is_, P, train)
                f32 = B.bn_finish_f32(s32[None].float(), gm, is_, P, train)
                B.assert_fin(f32["coef"][0], fi["coef"][0], fi["coef_abs"][0], "k1")
                assert_lin(f32["coef"][1:], fi["coef"][1:], fi["coef_abs"][1:], "k2 k3")
                # from the stored sums, as the GPU test forms them
                k1 = fi["coef"][0]
                k2, k3 = -k1 * is_.double() * f32["dgamma"].double() / P, -k1 * f32["dbeta"].double() / P
                if train:
                    B.assert_fin(f32["coef"][1], k2, k2.abs(), "k2 from dgamma")
                    B.assert_fin(f32["coef"][2], k3, k3.abs(), "k3 from dbeta")
                    kk = torch.stack([k1, k2, k3])
                    ref, sabs = B.bn_bwd_apply_ref(dy, x, sc, sh, mu, kk, relu)
                    B.assert_el(B.bn_bwd_apply_f32(dy, x, sc, sh, mu, f32["coef"], relu, dt), ref, sabs,
                                B.BWD_APPLY_N + 2, dt, "fused bwd apply")


@pytest.mark.parametrize("mode", B.FINALIZE_MODES, ids=lambda m: f"mom{m[0]}-run{int(m[1])}-aff{int(m[2])}")
@pytest.mark.parametrize("case", B.FINALIZE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bn_stats_f32_passes_bounds(case, mode):
    tiles, tile_rows, C = case
    mom, running, affine = mode
    inp = B.finalize_inputs(tiles, tile_rows, C)
    a = (inp["psum"], inp["pm2"], tile_rows, inp["rows"], inp["gamma"] if affine else None, inp["beta"] if affine else None,
         inp["rm"] if running else None, inp["rv"] if running else None, mom, B.EPS)
    ref, f32 = B.bn_stats_ref(*a), B.bn_stats_f32(*a)
    for k in f32:
        B.assert_fin(f32[k], ref[k], ref[k + "_abs"], k)
    assert ("rm" in ref) == (running and mom != 0)


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("C", [1, 3, 33, 64, 65, 2048])
def test_bn_eval_f32_passes_bounds(C, affine):
    inp = B.finalize_inputs(4, 8, C)
    a = (inp["gamma"] if affine else None, inp["beta"] if affine else None, inp["rm"], inp["rv"], B.EPS)
    ref, f32 = B.bn_eval_ref(*a), B.bn_eval_f32(*a)
    for k in f32:
        B.assert_el(f32[k], ref[k], ref[k + "_abs"], B.EVAL_N[k], F32, k)


@pytest.mark.parametrize("C", B.FINISH_C)
@pytest.mark.parametrize("nblk", B.FINISH_NBLK[:-1])
def test_bn_finish_f32_passes_bounds(nblk, C):
    inp = B.finish_inputs(nblk, C)
    pabs = inp["part"].abs()
    for train in (1, 0):
        ref = B.bn_finish_ref(inp["part"], pabs, inp["gamma"], inp["invstd"], inp["P"], train)
        f32 = B.bn_finish_f32(inp["part"], inp["gamma"], inp["invstd"], inp["P"], train)
        B.assert_fin(f32["dgamma"], ref["dgamma"], ref["dgamma_abs"], "dgamma")
        B.assert_fin(f32["dbeta"], ref["dbeta"], ref["dbeta_abs"], "dbeta")
        B.assert_fin(f32["coef"], ref["coef"], ref["coef_abs"], "coef")


# ----------------------------------------------------------------------------
# attention gate: references vs autograd
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("P,F,C", [(257, 8, 8), (63, 32, 24), (300, 64, 520)])
def test_attention_refs_match_autograd(P, F, C):
    """oracle.cpu_ref.attention_gate from s onward: s = relu(g1 + x1), q = conv(s),
    z = bn(q) (an affine map st here), psi = sigmoid(z), out = x psi"""
    inp, gi = A.psi_inputs(P, F, F32), A.gate_inputs(P, C, F32)
    d = lambda t: t.double()
    ug, ux = d(inp["ug"]).requires_grad_(True), d(inp["ux"]).requires_grad_(True)
    w, b = d(inp["wpsi"]).requires_grad_(True), d(inp["bpsi"]).requires_grad_(True)
    x = d(gi["x"]).requires_grad_(True)
    g1, x1 = ug * d(inp["sg"]) + d(inp["tg"]), ux * d(inp["sx"]) + d(inp["tx"])
    s = torch.relu(g1 + x1)
    q = s @ w + b
    q.retain_grad()
    z = q * float(gi["st"][0]) + float(gi["st"][1])
    z.retain_grad()
    psi = torch.sigmoid(z)
    out = x * psi[:, None]
    out.backward(d(gi["dout"]))
    qr, qabs = A.psi_fwd_ref(*(inp[k] for k in ("ug", "ux", "sg", "tg", "sx", "tx", "wpsi", "bpsi")))
    close(qr, q.detach(), qabs)
    assert bool((qabs >= qr.abs() * (1 - 1e-12)).all())
    p, pabs, zr = A.gate_p_ref(qr, gi["st"])
    close(p, psi.detach())
    o, oabs = A.gate_out_ref(gi["x"], p)
    close(o, out.detach(), oabs)
    dxr, _ = A.gate_out_ref(gi["dout"], p)
    close(dxr, x.grad, dxr.abs())
    dqpre, dabs = A.gate_bwd_ref(gi["dout"], gi["x"], p)
    close(dqpre, z.grad, dabs)
    # the psi backward from the gradient of q
    r = A.psi_bwd_ref(*(inp[k] for k in ("ug", "ux", "sg", "tg", "sx", "tx", "wpsi")), q.grad)
    close(r["ds"] * d(inp["sg"]), ug.grad, r["ds_abs"] * d(inp["sg"]).abs())
    close(r["ds"] * d(inp["sx"]), ux.grad, r["ds_abs"] * d(inp["sx"]).abs())
    close(r["dw"], w.grad, r["dw_abs"])
    close(r["db"], b.grad, r["db_abs"])
    # exact zeros planted: the gradient is exactly 0 there, as torch's ReLU gradient at 0 is
    s0 = (g1 + x1).detach() == 0
    assert bool(s0.any()) and not bool(r["ds"][s0].any()) and not bool(ug.grad[s0].any())
    # tile statistics against a plain loop
    ts = A.tile_stats_ref(qr)
    close(ts[0].sum(), qr.sum(), qr.abs().sum())
    # the BatchNorm partials: their sum over blocks is the dense sum
    nb = A.psi_blocks(P)
    part, sabs = A.psi_bnb_ref(r["ds"], inp["ug"], inp["mg"], inp["ig"], nb)
    xhat = (d(inp["ug"]) - d(inp["mg"])) * d(inp["ig"])
    close(part[:, 0].sum(0), r["ds"].sum(0), sabs[:, 0].sum(0))
    close(part[:, 1].sum(0), (r["ds"] * xhat).sum(0), sabs[:, 1].sum(0))


# ----------------------------------------------------------------------------
# attention gate: input conditions and float32 restatements
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("F", A.PSI_F)
def test_psi_inputs_and_f32_restatements(F, dt):
    for P in A.PSI_P:
        inp = A.psi_inputs(P, F, dt)
        a = [inp[k] for k in ("ug", "ux", "sg", "tg", "sx", "tx")]
        assert torch.equal(inp["ug"].to(dt).float(), inp["ug"]) and torch.equal(inp["ux"].to(dt).float(), inp["ux"])
        assert int(A.pre_near_zero(*a).sum()) == 0
        s64, _ = A.pre_ref(*a)
        if P >= 63:
            assert bool((s64 == 0).any())          # the planted exact zeros
        f32 = A.psi_bwd_f32(*a, inp["wpsi"], inp["dq"], dt)
        assert torch.equal(f32["s"] > 0, s64 > 0)   # the float32 mask is the fp64 one
        A.check_psi_bwd(f32, inp, dt, "psi bwd f32")
        acc = dict(f32, dw=(f32["dw"].float() + inp["pre"][:-1]), db=(f32["db"].float() + inp["pre"][-1:]))
        A.check_psi_bwd(acc, inp, dt, "psi bwd f32 acc", acc=True)
        q32 = A.psi_fwd_f32(*a, inp["wpsi"], inp["bpsi"])
        A.check_q(q32, inp, F, "psi fwd f32")
        A.check_tile_stats(*A.tile_stats_f32(q32), q32, "tile stats f32")
        # the BatchNorm partials over the stored ds, float32 element formulas
        nb = A.psi_blocks(P)
        ref, sabs = A.psi_bnb_ref(f32["ds"].float(), inp["ug"], inp["mg"], inp["ig"], nb)
        t32 = f32["ds"].float() * ((inp["ug"] - inp["mg"]) * inp["ig"])
        p32, _ = A.psi_bnb_ref(t32, inp["ug"], torch.zeros(F), torch.ones(F), nb)
        assert_lin(p32[:, 0], ref[:, 1], sabs[:, 1], "bnb partials f32")


def test_psi_inputs_big_case_has_no_mask_edges():
    inp = A.psi_inputs(A.PSI_P_BIG, 8, BF16)
    assert int(A.pre_near_zero(*(inp[k] for k in ("ug", "ux", "sg", "tg", "sx", "tx"))).sum()) == 0
    assert A.psi_blocks(A.PSI_P_BIG) == A.MAXB and A.psi_blocks(A.PSI_P_BIG - 258) == A.MAXB - 1 + 1


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("C", sorted(set(A.GATE_FWD_C + A.GATE_BWD_C)))
def test_gate_inputs_and_f32_restatements(C, dt):
    for P in A.GATE_P:
        gi = A.gate_inputs(P, C, dt)
        p64, sabs, z = A.gate_p_ref(gi["q"], gi["st"])
        if P > 3:
            assert bool((z == 0).any()) and float(z.max()) == 30 and float(z.min()) == -30
            assert bool((gi["pmap"] == 0).any()) and bool((gi["pmap"] == 1).any())
        p32 = A.gate_p_f32(gi["q"], gi["st"])
        r, r_cpu = assert_trans(p32, p64, p32, sabs, "pmap f32")
        assert r_cpu <= 8, r_cpu      # sabs is the right sensitivity: a handful of roundings, saturated ends included
        ref, oabs = A.gate_out_ref(gi["x"], p32)
        B.assert_el((gi["x"] * p32[:, None]).to(dt), ref, oabs, 1, dt, "out f32")
        ref, oabs = A.gate_out_ref(gi["dout"], gi["pmap"])
        B.assert_el((gi["dout"] * gi["pmap"][:, None]).to(dt), ref, oabs, 1, dt, "dx f32")
        ref, dabs = A.gate_bwd_ref(gi["dout"], gi["x"], gi["pmap"])
        d32 = (gi["dout"] * gi["x"]).sum(1) * gi["pmap"] * (1 - gi["pmap"])
        B.assert_el(d32, ref, dabs, A.gate_bwd_n(C), F32, "dqpre f32")
