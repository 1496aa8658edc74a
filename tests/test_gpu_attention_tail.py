"""The fused attention-gate backward tail (attention_tail.hip,
vu_attn_tail_bwd) against the chain of kernels it replaces -- vu_attn_gate_bwd
(dx = dout * psi), vu_attn_psi_bwd_bnb (ds), vu_bn_bwd_apply2 (dug, dux) and
two accumulating vu_gemm_fwd input-gradient calls -- bit for bit, its refusals,
and engine.attention_bwd with FUSE_ATTN_TAIL on against off."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
INVALID = 1   # hipErrorInvalidValue


def _k():
    from vaeunet_amd import kernels as K
    return K


def _nhwc(t2d):
    """[P][C] memory as an NHWC activation of logical shape [1, C, 1, P]."""
    P, C = t2d.shape
    return t2d.view(1, 1, P, C).permute(0, 3, 1, 2)


def _inputs(P, F, C, cancel=False):
    """Seeded as test_gpu_attention_kernels._run draws them (same order), then
    what the tail needs on top.  cancel: ux = -ug with the same scale and the
    opposite shift, so every pre-activation is zero in exact arithmetic and
    its computed sign is rounding residue -- the ReLU masks of two kernels
    then agree only if they round the expression identically."""
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(P + F)
    ug = torch.randn(P, F, generator=g).to(dt)
    ux = torch.randn(P, F, generator=g).to(dt)
    co = [torch.rand(F, generator=g) + 0.5, torch.randn(F, generator=g) * 0.3,
          torch.rand(F, generator=g) + 0.5, torch.randn(F, generator=g) * 0.3]
    if cancel:
        ux, co[2], co[3] = -ug, co[0].clone(), -co[1]
    wpsi = torch.randn(F, generator=g) / F ** 0.5
    torch.randn(1, generator=g)                      # bpsi
    x = torch.randn(P, C, generator=g).to(dt)
    dout = torch.randn(P, C, generator=g).to(dt)
    dq = torch.randn(P, generator=g)
    # BatchNorm statistics (the psi backward's partials only) and random
    # BN-backward coefficient vectors (mean, coef[3][F]) for both BatchNorms
    mg, ig = torch.randn(F, generator=g) * 0.2, torch.rand(F, generator=g) + 0.5
    mx, ix = torch.randn(F, generator=g) * 0.2, torch.rand(F, generator=g) + 0.5
    kg, kx = torch.randn(3, F, generator=g), torch.randn(3, F, generator=g)
    wdg = (torch.randn(C, F, generator=g) / F ** 0.5).to(dt)
    wdx = (torch.randn(C, F, generator=g) / F ** 0.5).to(dt)
    pmap = torch.rand(P, generator=g)
    # dout and the dg destination: the channel halves of one [P][2C] tensor
    # (engine.up_bwd's dcat); the dg half holds an earlier gradient
    cat = torch.cat([dout, torch.randn(P, C, generator=g).to(dt)], dim=1).contiguous()
    # pixels whose ReLU mask a different fma contraction may flip
    s = ug.double() * co[0].double() + co[1].double() + ux.double() * co[2].double() + co[3].double()
    keep = ~(s.abs() < 1e-5).any(dim=1)
    dev = lambda t: t.to(DEV)  # noqa: E731
    return dict(ug=dev(ug), ux=dev(ux), co=[dev(c) for c in co], wpsi=dev(wpsi), x=dev(x), dq=dev(dq),
                mg=dev(mg), ig=dev(ig), mx=dev(mx), ix=dev(ix), kg=dev(kg), kx=dev(kx), wdg=dev(wdg),
                wdx=dev(wdx), pmap=dev(pmap), cat=dev(cat), keep=dev(keep))


def _tail_args(K, i, P, F, C, cat, dx, dug, dux, d, acc=1):
    co = i["co"]
    return [K.ptr(i["ug"]), K.ptr(i["ux"]), K.ptr(i["dq"]), P, F, C, K.ptr(co[0]), K.ptr(co[1]), K.ptr(co[2]),
            K.ptr(co[3]), K.ptr(i["wpsi"]), K.ptr(i["mg"]), K.ptr(i["kg"]), K.ptr(i["mx"]), K.ptr(i["kx"]),
            K.ptr(i["wdg"]), F, K.ptr(i["wdx"]), F, K.ptr(cat), 2 * C, K.ptr(i["pmap"]), K.ptr(cat), 2 * C, C, acc,
            K.ptr(dx), C, K.ptr(dug), K.ptr(dux), d, K.stream()]


def _present_chain(K, i, P, F, C, d):
    co = i["co"]
    cat = i["cat"].clone()
    dx = torch.empty(P, C, dtype=torch.bfloat16, device=DEV)
    dbnq = torch.empty(P, device=DEV)
    K.call("vu_attn_gate_bwd", K.ptr(cat), 2 * C, K.ptr(i["x"]), C, K.ptr(i["pmap"]), P, C, K.ptr(dx), C,
           K.ptr(dbnq), d, K.stream())
    ds = torch.empty_like(i["ug"])
    dw, db = torch.zeros(F, device=DEV), torch.zeros(1, device=DEV)
    ws = K.workspace_f32(K.query("vu_attn_psi_bwd_workspace_bytes", P, F), DEV)
    nb = K.query("vu_attn_psi_bwd_blocks", P)
    bg, bx = torch.empty(nb, 2, F, device=DEV), torch.empty(nb, 2, F, device=DEV)
    K.call("vu_attn_psi_bwd_bnb", K.ptr(i["ug"]), K.ptr(i["ux"]), P, F, K.ptr(co[0]), K.ptr(co[1]), K.ptr(co[2]),
           K.ptr(co[3]), K.ptr(i["wpsi"]), K.ptr(i["dq"]), K.ptr(ds), K.ptr(dw), K.ptr(db), 0, K.ptr(ws),
           K.ptr(i["mg"]), K.ptr(i["ig"]), K.ptr(i["mx"]), K.ptr(i["ix"]), K.ptr(bg), K.ptr(bx), d, K.stream())
    dug, dux = torch.empty_like(i["ug"]), torch.empty_like(i["ux"])
    K.call("vu_bn_bwd_apply2", K.ptr(ds), F, K.ptr(i["ug"]), F, K.ptr(i["ux"]), F, P, F, K.ptr(i["mg"]),
           K.ptr(i["kg"]), K.ptr(i["mx"]), K.ptr(i["kx"]), K.ptr(dug), F, K.ptr(dux), F, d, K.stream())
    K.gemm_fwd(K.gather1x1([_nhwc(dug)]), i["wdg"], C, _nhwc(cat), d, out_coff=C, accumulate=True)
    K.gemm_fwd(K.gather1x1([_nhwc(dux)]), i["wdx"], C, _nhwc(dx), d, accumulate=True)
    torch.cuda.synchronize()
    return dict(dug=dug, dux=dux, cat=cat, dx=dx, dbnq=dbnq, dw=dw, db=db, bg=bg, bx=bx)


CASES = [
    # (P, F_int, C)
    (1024, 32, 64),
    (2368, 32, 64),      # 37 wave tiles: odd, not a multiple of a block's 4 waves (grid-stride tail)
    (2368, 64, 128),
    (1040, 128, 256),    # 16-pixel tiles
]
# the same shapes with every pre-activation an exact-arithmetic zero
CANCEL = [(1024, 32, 64), (2368, 64, 128), (1040, 128, 256)]


@pytest.mark.parametrize("case", [c + (False,) for c in CASES] + [c + (True,) for c in CANCEL])
def test_tail_matches_present_chain_bit_for_bit(case):
    """Every pixel is compared: attn_pre.h fixes the rounding of the
    pre-activation, so the pixels with |s| < 1e-5 need no exemption (their
    count is printed; the cancelling cases consist of them)."""
    K = _k()
    from vaeunet_amd import _lib
    P, F, C, cancel = case
    d = _lib.BF16
    i = _inputs(P, F, C, cancel)
    ref = _present_chain(K, i, P, F, C, d)
    assert K.query("vu_attn_tail_bwd_ok", P, F, C, F, F, 2 * C, 2 * C, C, C, d)
    assert P % K.query("vu_attn_tail_bwd_tile", F, C) == 0
    cat = i["cat"].clone()
    dx = torch.full((P, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    dug, dux = torch.full_like(i["ug"], float("nan")), torch.full_like(i["ux"], float("nan"))
    K.call("vu_attn_tail_bwd", *_tail_args(K, i, P, F, C, cat, dx, dug, dux, d))
    torch.cuda.synchronize()
    near = P - int(i["keep"].sum())
    print(f"P={P} F={F} C={C} cancel={cancel}: {near} pixels with a |s| < 1e-5, "
          f"{int((ref['dug'] != dug).any(1).sum())} pixels differ")
    assert near == P if cancel else near < 0.01 * P
    assert torch.equal(dug, ref["dug"])
    assert torch.equal(dux, ref["dux"])
    assert torch.equal(cat[:, C:], ref["cat"][:, C:])
    assert torch.equal(dx, ref["dx"])
    # the dout half is read, never written; every pixel was written
    assert torch.equal(cat[:, :C], i["cat"][:, :C])
    assert not bool(torch.isnan(dx.float()).any() | torch.isnan(dug.float()).any() | torch.isnan(dux.float()).any())


def test_gate_and_psi_backward_without_their_streams():
    """vu_attn_gate_bwd with a null dx still writes dbnq; vu_attn_psi_bwd_bnb
    with a null ds writes the same psi gradients and BatchNorm partials."""
    K = _k()
    from vaeunet_amd import _lib
    P, F, C = 2368, 64, 128
    d = _lib.BF16
    i = _inputs(P, F, C)
    co = i["co"]
    ref = _present_chain(K, i, P, F, C, d)
    dbnq = torch.full((P,), float("nan"), device=DEV)
    K.call("vu_attn_gate_bwd", K.ptr(i["cat"]), 2 * C, K.ptr(i["x"]), C, K.ptr(i["pmap"]), P, C, None, C,
           K.ptr(dbnq), d, K.stream())
    dw, db = torch.zeros(F, device=DEV), torch.zeros(1, device=DEV)
    ws = K.workspace_f32(K.query("vu_attn_psi_bwd_workspace_bytes", P, F), DEV)
    nb = K.query("vu_attn_psi_bwd_blocks", P)
    bg, bx = torch.full((nb, 2, F), float("nan"), device=DEV), torch.full((nb, 2, F), float("nan"), device=DEV)
    K.call("vu_attn_psi_bwd_bnb", K.ptr(i["ug"]), K.ptr(i["ux"]), P, F, K.ptr(co[0]), K.ptr(co[1]), K.ptr(co[2]),
           K.ptr(co[3]), K.ptr(i["wpsi"]), K.ptr(i["dq"]), None, K.ptr(dw), K.ptr(db), 0, K.ptr(ws),
           K.ptr(i["mg"]), K.ptr(i["ig"]), K.ptr(i["mx"]), K.ptr(i["ix"]), K.ptr(bg), K.ptr(bx), d, K.stream())
    torch.cuda.synchronize()
    # same lanes and summation order; the two instantiations may contract
    # their per-lane sums differently (fp32 rounding)
    # dbnq: a C-term fp32 dot product times psi (1 - psi) <= 1/4; each add
    # rounds by at most 2^-24 of a partial sum, itself at most sum |dout x|
    bound = float((i["cat"][:, :C].float() * i["x"].float()).abs().sum(1).max()) * C * 2.0 ** -24 / 4
    torch.testing.assert_close(dbnq, ref["dbnq"], rtol=0, atol=bound)
    for a, b in ((dw, ref["dw"]), (db, ref["db"]), (bg, ref["bg"]), (bx, ref["bx"])):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6 * float(b.abs().max()))


def test_tail_refusals():
    K = _k()
    from vaeunet_amd import _lib
    P, F, C = 1024, 32, 64
    i = _inputs(P, F, C)
    cat = i["cat"].clone()
    dx = torch.zeros(P, C, dtype=torch.bfloat16, device=DEV)
    dug, dux = torch.zeros_like(i["ug"]), torch.zeros_like(i["ux"])
    ok = lambda P_, F_, C_, d_: K.query("vu_attn_tail_bwd_ok", P_, F_, C_, F_, F_, 2 * C_, 2 * C_, C_, C_, d_)  # noqa: E731
    assert ok(P, F, C, _lib.BF16)
    bad = [(P, F, C, _lib.F32),          # fp32
           (P, 256, 512, _lib.BF16),     # F = 256
           (P, 256, 256, _lib.BF16),
           (P - 24, F, C, _lib.BF16)]    # ragged P
    for P_, F_, C_, d_ in bad:
        assert not ok(P_, F_, C_, d_)
        # (refused before anything is launched: the buffers are not touched)
        rc = K.query("vu_attn_tail_bwd", *_tail_args(K, i, P_, F_, C_, cat, dx, dug, dux, d_))
        assert rc == INVALID
    torch.cuda.synchronize()
    assert torch.equal(cat, i["cat"]) and not bool(dx.any())


@pytest.mark.parametrize("C", [64, 128])
def test_engine_tail_on_matches_off(C, monkeypatch):
    """engine.attention_bwd at N = 1, 32 x 32: dx, the dg slice and every
    parameter gradient of the gate bit-equal with the fused tail on and off."""
    from vaeunet_amd import _lib, engine as E
    from vaeunet_amd.unet_parts import AttentionGate
    K = _k()
    monkeypatch.setattr(E, "ATTN_TAIL_MIN_TILES_PER_CU", 0)
    N, H, W = 1, 32, 32
    torch.manual_seed(C)
    att = AttentionGate(C, C, C // 2).to(DEV).train()
    with torch.no_grad():
        for m in (att.W_g[1], att.W_x[1], att.psi[1]):
            m.weight.uniform_(0.5, 1.5)
            m.bias.normal_(0, 0.3)
    gen = torch.Generator().manual_seed(7 + C)
    act = lambda c: torch.randn(N, c, H, W, generator=gen).to(torch.bfloat16).to(DEV).contiguous(  # noqa: E731
        memory_format=torch.channels_last)
    g, x, cat0 = act(C), act(C), act(2 * C)
    M = E.Mode(_lib.BF16, DEV)
    calls = []
    real_call = K.call

    def spy(name, *a):
        calls.append(name)
        return real_call(name, *a)
    monkeypatch.setattr(K, "call", spy)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(E, "FUSE_ATTN_TAIL", on)
        for p in att.parameters():
            p.grad = None
        with torch.no_grad():
            _, saved = E.attention_fwd(M, att, g, x)
        cat = cat0.clone()
        calls.clear()
        dx = E.attention_bwd(M, att, saved, cat[:, :C], (cat, C), True)
        M.join()
        torch.cuda.synchronize()
        assert ("vu_attn_tail_bwd" in calls) == on
        res[on] = (dx.clone(), cat.clone(), {n: p.grad.clone() for n, p in att.named_parameters()})
    assert torch.equal(res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1])
    assert torch.equal(res[True][1][:, :C], cat0[:, :C])
    for n, gr in res[False][2].items():
        assert torch.equal(res[True][2][n], gr), n


def test_engine_tail_under_gemm_audit(monkeypatch):
    """With a GEMM audit installed (tests/gemm_audit.py) the fused launch
    reports its two input-gradient GEMMs, they pass the per-element check, and
    the results are the bits of the unaudited run."""
    from gemm_audit import GemmAudit
    from vaeunet_amd import _lib, engine as E
    from vaeunet_amd.unet_parts import AttentionGate
    K = _k()
    monkeypatch.setattr(E, "ATTN_TAIL_MIN_TILES_PER_CU", 0)
    C, N, H, W = 64, 1, 32, 32
    torch.manual_seed(C)
    att = AttentionGate(C, C, C // 2).to(DEV).train()
    gen = torch.Generator().manual_seed(11)
    act = lambda c: torch.randn(N, c, H, W, generator=gen).to(torch.bfloat16).to(DEV).contiguous(  # noqa: E731
        memory_format=torch.channels_last)
    g, x, cat0 = act(C), act(C), act(2 * C)
    M = E.Mode(_lib.BF16, DEV)
    res = {}
    for audited in (False, True):
        for p in att.parameters():
            p.grad = None
        with torch.no_grad():
            _, saved = E.attention_fwd(M, att, g, x)
        cat = cat0.clone()
        audit = GemmAudit(strict=True)
        monkeypatch.setattr(K, "AUDIT", audit if audited else None)
        dx = E.attention_bwd(M, att, saved, cat[:, :C], (cat, C), True)
        monkeypatch.setattr(K, "AUDIT", None)
        M.join()
        torch.cuda.synchronize()
        res[audited] = (dx.clone(), cat.clone())
        if audited:
            fwd = [r for r in audit.records if r["op"] == "fwd"]
            assert len(fwd) == 2 and all(r["acc"] and not r["off"] and r["untouched"] for r in fwd), fwd
            assert len([r for r in audit.records if r["op"] == "wgrad"]) == 2
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
