"""Plain fp64 CPU references of the attention gate's memory-bound kernels
(attention.hip: vu_attn_psi_fwd, vu_attn_gate_fwd, vu_attn_gate_bwd,
vu_attn_psi_bwd, vu_attn_psi_bwd_bnb; AttentionGate, unet_parts.py:7-30), the
bounds of tests/test_gpu_attention_ref.py with their derivations, float32
restatements of the kernels' operation order (the yardstick of
tests/test_bn_attention_ref.py), and the seeded inputs of both.

Conventions of ref_small.py: CPU tensors in, float64 out, ``sabs`` the same
expression on |operands|, activations pixel-major [P, C].
"""
import math

import torch

from ref_small import C_SUM, TILE, U32, bnb_partials_ref
from vaeunet_amd import _lib

F32, BF16 = torch.float32, torch.bfloat16
KEY_ATTN = _lib.VU_TUNE_ATTN   # 1 batched kernels (default), 0 one-row kernels
MAXB = 1024              # grid cap of the psi backward (vu_attn_psi_bwd_blocks)
EDGE = 1e-3              # bn_near_zero's cancellation criterion

PSI_F = [8, 16, 32, 64, 128, 256, 512]            # every group_sum width
PSI_P = [1, 63, 255, 256, 257, 3 * 256 + 77]
PSI_P_BIG = MAXB * 256 + 257                      # the grid-stride loop and the MAXB cap (F = 8)
GATE_FWD_C = [8, 24, 40, 64, 512, 520, 1024]      # 24, 40, 520: C / 8 no power of two (gate_fwd_kernel)
GATE_BWD_C = [8, 64, 256, 512, 520, 768, 1024]    # > 512: gate_bwd_kernel under both VU_TUNE_ATTN values
GATE_P = [1, 63, 257, 3 * 256 + 77]


# ----------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------
def pre_ref(ug, ux, sg, tg, sx, tx):
    """s = ug sg + tg + ux sx + tx -> (s, sabs), [P, F]"""
    a, b = ug.double() * sg.double(), ux.double() * sx.double()
    return a + tg.double() + b + tx.double(), a.abs() + tg.double().abs() + b.abs() + tx.double().abs()


def pre_near_zero(ug, ux, sg, tg, sx, tx):
    """Elements of s that cancel to within EDGE of their four terms without
    being exactly zero in every arithmetic (the planted ug = ux = 0, tg = -tx,
    where each partial sum is exact): there the mask s > 0 could depend on the
    rounding of the float32 sums."""
    s, sabs = pre_ref(ug, ux, sg, tg, sx, tx)
    exact = (ug == 0) & (ux == 0) & (tg + tx == 0).expand_as(ug)
    return (s.abs() < EDGE * sabs) & ~exact


def psi_fwd_ref(ug, ux, sg, tg, sx, tx, wpsi, bpsi):
    """q = bpsi + sum_c wpsi relu(s) -> (q [P], sabs = |bpsi| + sum |wpsi| sabs_s)"""
    s, sabs = pre_ref(ug, ux, sg, tg, sx, tx)
    w = wpsi.double()
    return s.clamp_min(0) @ w + bpsi.double(), sabs @ w.abs() + bpsi.double().abs()


def psi_fwd_n(F):
    """float32 operations behind one q: the four of s (a rounding error of s
    passes the ReLU at most unchanged), the multiply by wpsi, the lane's 8
    additions, log2(F / 8) shuffle steps, + bpsi"""
    return 4 + 1 + 8 + int(math.log2(F // 8)) + 1


def tile_stats_ref(q, tile=TILE):
    """per-tile (sum, centered M2) of q [P] in fp64 and the bounds' operands:
    sum |q| and sum (q - mean)^2 + sum |q| |mean|  -> 4 x [tiles]"""
    q = q.double()
    P = q.shape[0]
    tiles = (P + tile - 1) // tile
    out = torch.zeros(4, tiles, dtype=torch.float64)
    for t in range(tiles):
        b = q[t * tile:(t + 1) * tile]
        m = b.mean()
        out[0, t], out[1, t] = b.sum(), ((b - m) ** 2).sum()
        out[2, t], out[3, t] = b.abs().sum(), ((b - m) ** 2).sum() + b.abs().sum() * m.abs()
    return out


def gate_p_ref(q, st):
    """p = sigmoid(q st0 + st1) -> (p, sabs, z).  sabs = p (1 - p) (1 + |z|) + p:
    the sensitivity of p to an error of U32 (|q st0| + |st1| + ...) in z and in
    exp's argument, plus p itself for the rounding of the stored float32 (the
    first term vanishes where p saturates, the float32 p does not)."""
    z = q.double() * float(st[0]) + float(st[1])
    p = torch.sigmoid(z)
    return p, p * (1 - p) * (1 + z.abs()) + p, z


def gate_p_f32(q, st):
    z = q.float() * st[0].float() + st[1].float()
    return 1 / (1 + torch.exp(-z))


def gate_out_ref(x, p):
    """out = x p (also dx = dout p) -> (out, sabs)"""
    o = x.double() * p.double()[:, None]
    return o, o.abs()


def gate_bwd_ref(dout, x, p):
    """dqpre = (sum_c dout x) p (1 - p) -> (dqpre [P], sabs)"""
    t = dout.double() * x.double()
    k = p.double() * (1 - p.double())
    return t.sum(1) * k, t.abs().sum(1) * k.abs()


def gate_bwd_n(C):
    """the multiply, the lane's additions (8 per 512 channels), log2(lanes)
    shuffle steps, 1 - p and the two multiplies"""
    lpp = min(64, C // 8)
    return 1 + 8 * ((C // 8 + lpp - 1) // lpp) + int(math.log2(lpp)) + 3


def psi_bwd_ref(ug, ux, sg, tg, sx, tx, wpsi, dq):
    """ds = dq wpsi [s > 0], dwpsi = sum_p dq relu(s), dbpsi = sum_p dq
    -> dict(ds, dw, db and *_abs)"""
    s, sabs = pre_ref(ug, ux, sg, tg, sx, tx)
    on = s > 0
    g = dq.double()[:, None]
    ds = g * wpsi.double() * on
    return dict(ds=ds, ds_abs=ds.abs(), dw=(g * s * on).sum(0), dw_abs=(g.abs() * sabs * on).sum(0),
                db=dq.double().sum().reshape(1), db_abs=dq.double().abs().sum().reshape(1))


def psi_bwd_f32(ug, ux, sg, tg, sx, tx, wpsi, dq, dtype):
    """attn_pre's order ((ug sg + tg) + ux sx) + tx without contraction; the
    sums over pixels in fp64 (C_SUM covers the kernel's float32 ones)"""
    s = ug.float() * sg.float() + tg.float() + ux.float() * sx.float() + tx.float()
    on = s > 0
    g = dq.float()[:, None]
    zero = torch.zeros_like(s)
    return dict(ds=torch.where(on, g * wpsi.float(), zero).to(dtype), dw=torch.where(on, g * s, zero).double().sum(0),
                db=dq.double().sum().reshape(1), s=s)


def psi_fwd_f32(ug, ux, sg, tg, sx, tx, wpsi, bpsi):
    s = (ug.float() * sg.float() + tg.float() + ux.float() * sx.float() + tx.float()).clamp_min(0)
    return (s * wpsi.float()).sum(1) + bpsi.float()


def psi_blocks(P):
    return min(MAXB, (P + TILE - 1) // TILE)


def psi_bnb_ref(ds_stored, u, mean, invstd, nblk):
    """One BatchNorm's per-block (sum ds, sum ds xhat) over the stored ds, no
    ReLU between (bnb_partials_ref with a mask that keeps every element)."""
    F = u.shape[1]
    return bnb_partials_ref(ds_stored, u, torch.zeros(F), torch.ones(F), mean, invstd, nblk)


# ----------------------------------------------------------------------------
# seeded inputs
# ----------------------------------------------------------------------------
def psi_inputs(P, F, dtype, seed=81, plant=True):
    """ug, ux [P, F] (rounded to dtype, conditioned away from the mask's edge),
    sg / sx (both signs), tg, tx, wpsi [F], bpsi [1], dq [P], the two
    BatchNorms' mean / invstd.  ``plant``: in every eighth channel tg = -tx and
    a third of the pixels hold ug = ux = 0, so s is exactly 0 there."""
    g = torch.Generator().manual_seed(seed + 7 * F + P)
    r = lambda *s: torch.randn(*s, generator=g)
    ug, ux = r(P, F).to(dtype).float(), r(P, F).to(dtype).float()
    sign = lambda: torch.where(torch.rand(F, generator=g) < 0.25, -1.0, 1.0)
    sg, sx = (torch.rand(F, generator=g) + 0.5) * sign(), (torch.rand(F, generator=g) + 0.5) * sign()
    tg, tx = r(F) * 0.3, r(F) * 0.3
    wpsi, bpsi, dq = r(F) / F ** 0.5, r(1), r(P)
    if plant:
        ch = torch.arange(F) % 8 == 5
        tg = torch.where(ch, -tx, tg)
        px = (torch.rand(P, generator=g) < 1 / 3)[:, None] & ch[None, :]
        ug, ux = torch.where(px, torch.zeros_like(ug), ug), torch.where(px, torch.zeros_like(ux), ux)
    for _ in range(20):
        bad = pre_near_zero(ug, ux, sg, tg, sx, tx)
        if not bool(bad.any()):
            break
        ug = torch.where(bad, (ug * 1.03125 + 0.125).to(dtype).float(), ug)
    mg, ig, mx, ix = r(F) * 0.2, torch.rand(F, generator=g) + 0.5, r(F) * 0.2, torch.rand(F, generator=g) + 0.5
    pre = r(F + 1)
    return dict(ug=ug, ux=ux, sg=sg, tg=tg, sx=sx, tx=tx, wpsi=wpsi, bpsi=bpsi, dq=dq, mg=mg, ig=ig, mx=mx, ix=ix,
                pre=pre)


def gate_inputs(P, C, dtype, seed=91):
    """q [P] and st with q st0 + st1 spread over [-30, 30] (p saturates at both
    ends) and exactly 0 at the pixels p % 7 == 3 (st1 = 0 and q = 0 there);
    x, dout [P, C] rounded to dtype; pmap in (0, 1) with exact 0 and 1."""
    g = torch.Generator().manual_seed(seed + 3 * C + P)
    st = torch.tensor([1.5, 0.0])
    q = (torch.rand(P, generator=g) * 40 - 20)
    q = torch.where(torch.arange(P) % 7 == 3, torch.zeros_like(q), q)
    if P > 2:
        q[0], q[1] = 20.0, -20.0
    x = torch.randn(P, C, generator=g).to(dtype).float()
    dout = torch.randn(P, C, generator=g).to(dtype).float()
    pmap = torch.rand(P, generator=g)
    pmap = torch.where(torch.arange(P) % 5 == 1, torch.zeros_like(pmap), pmap)
    pmap = torch.where(torch.arange(P) % 5 == 3, torch.ones_like(pmap), pmap)
    return dict(q=q, st=st, x=x, dout=dout, pmap=pmap)


# ----------------------------------------------------------------------------
# checks shared by the GPU tests (device outputs) and the CPU self-checks (the
# float32 restatements): the same bound on the same inputs
# ----------------------------------------------------------------------------
def check_q(q, inp, F, what):
    from bn_ref import assert_el
    ref, sabs = psi_fwd_ref(inp["ug"], inp["ux"], inp["sg"], inp["tg"], inp["sx"], inp["tx"], inp["wpsi"], inp["bpsi"])
    return assert_el(q, ref, sabs, psi_fwd_n(F), F32, what + " q")


def check_tile_stats(psum, pm2, q_dev, what):
    """against the fp64 sums of the device's own q: C_SUM sum |q| for psum,
    C_SUM (sum (q - mean)^2 + sum |q| |mean|) for pm2"""
    ref = tile_stats_ref(q_dev)
    worst = 0.0
    for name, got, r, s in (("psum", psum, ref[0], ref[2]), ("pm2", pm2, ref[1], ref[3])):
        diff = (got.double().cpu() - r).abs()
        bound = C_SUM * s
        ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)
        w = float(ratio.max())
        assert w <= 1.0, f"{what} {name}: bound exceeded {w:.3g}x at tile {int(ratio.argmax())}"
        worst = max(worst, w)
    return worst


def tile_stats_f32(q, tile=TILE):
    q = q.float()
    tiles = (q.shape[0] + tile - 1) // tile
    ps, pm = torch.zeros(tiles), torch.zeros(tiles)
    for t in range(tiles):
        b = q[t * tile:(t + 1) * tile]
        ps[t] = b.sum()
        pm[t] = ((b - ps[t] / b.shape[0]) ** 2).sum()
    return ps, pm


def check_psi_bwd(got, inp, dtype, what, acc=False):
    """got: dict(ds (stored), dw, db).  ds per element (one multiply, the
    storage rounding), and exactly 0 where s is exactly 0; the sums by assert_lin."""
    from bn_ref import assert_el
    from ref_small import assert_lin
    ref = psi_bwd_ref(inp["ug"], inp["ux"], inp["sg"], inp["tg"], inp["sx"], inp["tx"], inp["wpsi"], inp["dq"])
    w = [0.0]
    if got.get("ds") is not None:
        w.append(assert_el(got["ds"], ref["ds"], ref["ds_abs"], 1, dtype, what + " ds"))
        s, _ = pre_ref(inp["ug"], inp["ux"], inp["sg"], inp["tg"], inp["sx"], inp["tx"])
        assert not bool(got["ds"].double().cpu()[s <= 0].any()), what + ": ds not exactly 0 where s <= 0"
    pw = inp["pre"][:-1] if acc else None
    pb = inp["pre"][-1:] if acc else None
    w.append(assert_lin(got["dw"], ref["dw"] + (pw.double() if acc else 0), ref["dw_abs"], what + " dwpsi", acc=pw))
    w.append(assert_lin(got["db"], ref["db"] + (pb.double() if acc else 0), ref["db_abs"], what + " dbpsi", acc=pb))
    return max(w)


def sigmoid_ratio(got, ref, sabs):
    """max |got - ref| / (U32 sabs)"""
    diff = (got.double().cpu() - ref).abs()
    return float(torch.where(diff == 0, torch.zeros_like(diff), diff / (U32 * sabs)).max())
