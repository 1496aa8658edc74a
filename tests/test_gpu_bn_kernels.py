"""Every export of bn.hip against the plain fp64 references of tests/bn_ref.py,
element by element, in guarded and strided buffers.

Bounds (bn_ref.py / ref_small.py; none is fitted to an observed error):
  elementwise outputs   u_store max(|ref|, |got|) + n U32 sabs, n the float32
                        operations of the kernel's expression (APPLY_N = 2:
                        multiply, add; FUSED_N = 5: + the residual's affine and
                        the sum; BWD_APPLY_N = 4: x - mean, k2 (.), the fma, + k3)
  sums over pixels      assert_lin: u max + C_SUM sabs (+ u |prefill|)
  finished in fp64      assert_fin: 4 U32 sabs (mean, invstd, scale, shift,
                        k1..k3, running statistics: at most two roundings of
                        the operands, one of the result)
Where one kernel's output feeds the next (reduce -> coefficients, the fused
kernels' own coefficients -> their apply) the reference takes the device's
stored intermediate, so each stage is judged alone.  Inputs are conditioned so
that no ReLU pre-activation sits near zero (asserted on the CPU in
test_bn_attention_ref.py): no element is left out of a comparison.
"""
import pytest
import torch

import bn_ref as B
from bn_ref import BF16, F32
from ref_small import assert_lin, guarded, guarded_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [F32, BF16]
DT_ID = {F32: "f32", BF16: "bf16"}.get
TUNE_DEFAULTS = {B.KEY_BN_NT_MB: 32, B.KEY_BN_MINBLK: 256}


def _L():
    from vaeunet_amd import _lib
    return _lib


def _code(dt):
    return _L().BF16 if dt == BF16 else _L().F32


class tuned:
    """Set tuning keys for a block; every key goes back to its default."""

    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            _L().call("vu_gemm_set_tuning", k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            _L().call("vu_gemm_set_tuning", k, TUNE_DEFAULTS[k])


def put(t, dt, wide=None, c0=0):
    """CPU [P, C] -> the same values as channels [c0, c0 + C) of a guarded
    device buffer of row stride ``wide`` (dense without it)"""
    v, g = guarded_rows(t.shape[0], t.shape[1], dt, DEV, wide=wide, c0=c0)
    v.copy_(t.to(dt))
    return v, g


def out_rows(P, C, dt, wide=None, c0=0):
    return guarded_rows(P, C, dt, DEV, wide=wide, c0=c0)


def vec(t):
    """CPU float tensor -> guarded contiguous float32 device copy"""
    v, g = guarded(tuple(t.shape), F32, DEV)
    v.copy_(t)
    return v, g


def empty_vec(*shape, dtype=F32):
    return guarded(shape, dtype, DEV)


def ptr(t):
    return _L().ptr(t)


def st():
    return _L().stream()


def cpu(t):
    return t.detach().float().cpu()


def variants(layout, dt, last):
    """(name, tuning) runs of one case: the default, the 16-rows-per-thread
    grid for the largest P, the non-temporal instantiations for bf16 on the
    vector path"""
    v = [("default", {})]
    if last:
        v.append(("minblk0", {B.KEY_BN_MINBLK: 0}))
    if dt == BF16 and B.is_vector(layout):
        v.append(("nt", {B.KEY_BN_NT_MB: 0}))
    return v


def workspace(P, C):
    n = max(1, _L().query("vu_reduce_workspace_bytes", P, C) // 4)
    return guarded(n, F32, DEV)


WORST = {}


def note(family, w):
    WORST[family] = max(WORST.get(family, 0.0), w)
    print(f"worst err/bound {family}: {WORST[family]:.3f}")


# ----------------------------------------------------------------------------
# vu_bn_finalize, vu_bn_eval_coeffs
# ----------------------------------------------------------------------------
def _finalize(inp, tiles, tile_rows, C, mom, running, affine):
    L = _L()
    psum, pm2 = inp["psum"].to(DEV), inp["pm2"].to(DEV)
    gamma, beta = (vec(inp["gamma"])[0], vec(inp["beta"])[0]) if affine else (None, None)
    rm, grm = vec(inp["rm"])
    rv, grv = vec(inp["rv"])
    nbt, gn = empty_vec(1, dtype=torch.int64)
    nbt.fill_(5)
    outs = [empty_vec(C) for _ in range(4)]
    ws, gw = guarded(max(1, L.query("vu_bn_finalize_workspace_bytes", tiles, C) // 4), F32, DEV)
    L.call("vu_bn_finalize", ptr(psum), ptr(pm2), tiles, tile_rows, inp["rows"], C, ptr(gamma), ptr(beta),
           ptr(rm) if running else None, ptr(rv) if running else None, mom, B.EPS, *(ptr(o[0]) for o in outs),
           ptr(nbt) if running else None, ptr(ws), st())
    torch.cuda.synchronize()
    for g in [grm, grv, gn, gw] + [o[1] for o in outs]:
        g.check("vu_bn_finalize")
    names = ("scale", "shift", "mean", "invstd")
    return dict(zip(names, (cpu(o[0]) for o in outs)), rm=cpu(rm), rv=cpu(rv), nbt=int(nbt[0]))


@pytest.mark.parametrize("mode", B.FINALIZE_MODES, ids=lambda m: f"mom{m[0]}-run{int(m[1])}-aff{int(m[2])}")
@pytest.mark.parametrize("case", B.FINALIZE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bn_finalize(case, mode):
    tiles, tile_rows, C = case
    mom, running, affine = mode
    inp = B.finalize_inputs(tiles, tile_rows, C)
    got = _finalize(inp, tiles, tile_rows, C, mom, running, affine)
    ref = B.bn_stats_ref(inp["psum"], inp["pm2"], tile_rows, inp["rows"], inp["gamma"] if affine else None,
                         inp["beta"] if affine else None, inp["rm"] if running else None,
                         inp["rv"] if running else None, mom, B.EPS)
    w = max(B.assert_fin(got[k], ref[k], ref[k + "_abs"], f"finalize {k}") for k in ("mean", "invstd", "scale", "shift"))
    if running and mom != 0:
        w = max(w, B.assert_fin(got["rm"], ref["rm"], ref["rm_abs"], "finalize running_mean"),
                B.assert_fin(got["rv"], ref["rv"], ref["rv_abs"], "finalize running_var"))
    else:   # momentum 0 or no running statistics: left as they were
        assert torch.equal(got["rm"], inp["rm"]) and torch.equal(got["rv"], inp["rv"])
    assert got["nbt"] == (6 if running else 5)
    again = _finalize(inp, tiles, tile_rows, C, mom, running, affine)
    assert all(torch.equal(again[k], got[k]) for k in ("scale", "shift", "mean", "invstd", "rm", "rv"))
    note("finalize", w)


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("C", [1, 3, 33, 64, 65, 2048])
def test_bn_eval_coeffs(C, affine):
    L = _L()
    inp = B.finalize_inputs(4, 8, C)
    gamma, beta = (vec(inp["gamma"])[0], vec(inp["beta"])[0]) if affine else (None, None)
    rm, rv = vec(inp["rm"])[0], vec(inp["rv"])[0]
    ref = B.bn_eval_ref(inp["gamma"] if affine else None, inp["beta"] if affine else None, inp["rm"], inp["rv"], B.EPS)
    for save in (True, False):
        outs = [empty_vec(C) for _ in range(4)]
        L.call("vu_bn_eval_coeffs", ptr(gamma), ptr(beta), ptr(rm), ptr(rv), B.EPS, C, ptr(outs[0][0]),
               ptr(outs[1][0]), ptr(outs[2][0]) if save else None, ptr(outs[3][0]) if save else None, st())
        torch.cuda.synchronize()
        for o in outs:
            o[1].check("vu_bn_eval_coeffs")
        for k, o in list(zip(("scale", "shift", "mean", "invstd"), outs))[:4 if save else 2]:
            note("eval", B.assert_el(cpu(o[0]), ref[k], ref[k + "_abs"], B.EVAL_N[k], F32, f"eval {k}"))
        if not save:   # untouched (still the sentinel)
            assert bool((outs[2][0] == 12345.0).all()) and bool((outs[3][0] == 12345.0).all())


# ----------------------------------------------------------------------------
# vu_bn_apply
# ----------------------------------------------------------------------------
def _apply(inp, layout, dt, relu, scale=None, shift=None):
    C, wi, wo, c0 = layout
    P = inp["x"].shape[0]
    x, _ = put(inp["x"], dt, wi, c0)
    y, gy = out_rows(P, C, dt, wo, c0)
    sc, sh = vec(inp["scale"] if scale is None else scale)[0], vec(inp["shift"] if shift is None else shift)[0]
    _L().call("vu_bn_apply", ptr(x), wi or C, ptr(y), wo or C, P, C, ptr(sc), ptr(sh), relu, _code(dt), st())
    torch.cuda.synchronize()
    gy.check("vu_bn_apply")
    return y


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("layout", B.LAYOUTS, ids=B.layout_id)
def test_bn_apply(layout, dt):
    C = layout[0]
    Ps = B.pixel_counts(C)
    for P in Ps:
        inp = B.bn_inputs(P, C, dt)
        for relu in (1, 0):
            ref, sabs = B.bn_apply_ref(inp["x"], inp["scale"], inp["shift"], relu)
            base = None
            for name, kv in variants(layout, dt, P == Ps[-1]):
                with tuned(kv):
                    y = _apply(inp, layout, dt, relu)
                note("apply", B.assert_el(cpu(y), ref, sabs, B.APPLY_N, dt, f"apply P={P} relu={relu} {name}"))
                base = y if base is None else base
                assert torch.equal(y, base), f"apply P={P} {name}: bits differ from the default run"


# ----------------------------------------------------------------------------
# vu_bn_bwd_reduce
# ----------------------------------------------------------------------------
def _reduce(inp, layout, dt, relu, train, acc, null):
    C, wi, wo, c0 = layout
    P = inp["x"].shape[0]
    dy, _ = put(inp["dy"], dt, wi, c0)
    x, _ = put(inp["x"], dt, wo, c0)
    co = [vec(inp[k])[0] for k in ("scale", "shift", "mean", "invstd", "gamma")]
    pre = inp["k"][:2]
    dg, gdg = vec(pre[0])
    db, gdb = vec(pre[1])
    coef, gco = empty_vec(3, C)
    ws, gws = workspace(P, C)
    _L().call("vu_bn_bwd_reduce", ptr(dy), wi or C, ptr(x), wo or C, P, C, *(ptr(c) for c in co[:4]), ptr(co[4]), relu,
              train, None if null else ptr(dg), None if null else ptr(db), acc, ptr(coef), ptr(ws), _code(dt), st())
    torch.cuda.synchronize()
    for g in (gdg, gdb, gco, gws):
        g.check("vu_bn_bwd_reduce")
    return cpu(dg), cpu(db), cpu(coef)


def _check_reduce(got, inp, P, relu, train, acc, null, what):
    dg, db, coef = got
    part, pabs = B.bn_bwd_sums_ref(inp["dy"], inp["x"], inp["scale"], inp["shift"], inp["mean"], inp["invstd"], relu)
    ref = B.bn_finish_ref(part, pabs, inp["gamma"], inp["invstd"], P, train)
    pre = inp["k"][:2]
    w = 0.0
    if null:
        assert torch.equal(dg, pre[0]) and torch.equal(db, pre[1]), what + ": null dgamma / dbeta written"
    else:
        w = max(assert_lin(dg, ref["dgamma"] + (pre[0].double() if acc else 0), ref["dgamma_abs"], what + " dgamma",
                           acc=pre[0] if acc else None),
                assert_lin(db, ref["dbeta"] + (pre[1].double() if acc else 0), ref["dbeta_abs"], what + " dbeta",
                           acc=pre[1] if acc else None))
    # k1 is finished alone; k2, k3 are linear in the sums: their summation noise, scaled
    w = max(w, B.assert_fin(coef[0], ref["coef"][0], ref["coef_abs"][0], what + " k1"),
            assert_lin(coef[1:], ref["coef"][1:], ref["coef_abs"][1:], what + " k2 k3"))
    if train and not acc and not null:
        # and against the device's own stored sums: k2 = -k1 invstd dgamma / P, k3 = -k1 dbeta / P
        k1, is_ = ref["coef"][0], inp["invstd"].double()
        k2, k3 = -k1 * is_ * dg.double() / P, -k1 * db.double() / P
        w = max(w, B.assert_fin(coef[1], k2, k2.abs(), what + " k2 from dgamma"),
                B.assert_fin(coef[2], k3, k3.abs(), what + " k3 from dbeta"))
    if not train:
        assert not bool(coef[1:].any()), what + ": eval mode k2 / k3 not zero"
    return w


REDUCE_COMBOS = [(relu, train, acc, False) for relu in (1, 0) for train in (1, 0) for acc in (0, 1)] + [(1, 1, 0, True)]


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("layout", B.LAYOUTS, ids=B.layout_id)
def test_bn_bwd_reduce(layout, dt):
    C = layout[0]
    Ps = B.pixel_counts(C)
    for P in Ps:
        inp = B.bn_inputs(P, C, dt)
        for relu, train, acc, null in REDUCE_COMBOS:
            base = None
            for name, kv in variants(layout, dt, P == Ps[-1]):
                with tuned(kv):
                    got = _reduce(inp, layout, dt, relu, train, acc, null)
                what = f"reduce P={P} relu={relu} train={train} acc={acc} null={null} {name}"
                note("reduce", _check_reduce(got, inp, P, relu, train, acc, null, what))
                if name == "nt":   # the same grid as the default run: the same bits
                    assert all(torch.equal(a, b) for a, b in zip(got, base)), what + ": bits differ from the default"
                base = got if base is None else base


# ----------------------------------------------------------------------------
# vu_bn_bwd_finish on synthetic partials
# ----------------------------------------------------------------------------
def _finish(inp, nblk, C, train, acc, gamma=True):
    L = _L()
    part = inp["part_dev"] if "part_dev" in inp else inp.setdefault("part_dev", inp["part"].to(DEV))
    g, is_ = vec(inp["gamma"])[0], vec(inp["invstd"])[0]
    dg, gdg = vec(inp["pre"][0])
    db, gdb = vec(inp["pre"][1])
    coef, gco = empty_vec(3, C)
    nbytes = L.query("vu_bn_bwd_finish_workspace_bytes", nblk, C)
    assert (nbytes == 0) == (nblk <= 1024)
    ws, gws = guarded(max(1, nbytes // 4), F32, DEV)
    L.call("vu_bn_bwd_finish", ptr(part), nblk, inp["P"], C, ptr(g) if gamma else None, ptr(is_), train, ptr(dg),
           ptr(db), acc, ptr(coef), ptr(ws), st())
    torch.cuda.synchronize()
    for gd in (gdg, gdb, gco, gws):
        gd.check("vu_bn_bwd_finish")
    return cpu(dg), cpu(db), cpu(coef)


@pytest.mark.parametrize("C", B.FINISH_C)
@pytest.mark.parametrize("nblk", B.FINISH_NBLK)
def test_bn_bwd_finish(nblk, C):
    inp = B.finish_inputs(nblk, C)
    pabs = inp["part"].abs()
    for train, acc, gamma in ((1, 0, True), (0, 1, True), (1, 1, False)):
        ref = B.bn_finish_ref(inp["part"], pabs, inp["gamma"] if gamma else None, inp["invstd"], inp["P"], train)
        dg, db, coef = got = _finish(inp, nblk, C, train, acc, gamma)
        pre = inp["pre"].double() if acc else torch.zeros(2, C, dtype=torch.float64)
        what = f"finish nblk={nblk} C={C} train={train} acc={acc}"
        w = max(B.assert_fin(dg, ref["dgamma"] + pre[0], ref["dgamma_abs"] + pre[0].abs(), what + " dgamma"),
                B.assert_fin(db, ref["dbeta"] + pre[1], ref["dbeta_abs"] + pre[1].abs(), what + " dbeta"),
                B.assert_fin(coef, ref["coef"], ref["coef_abs"], what + " coef"))
        if not train:
            assert not bool(coef[1:].any())
        again = _finish(inp, nblk, C, train, acc, gamma)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), what + ": two launches differ"
        note("finish", w)


# ----------------------------------------------------------------------------
# vu_bn_bwd_apply, vu_bn_bwd_apply2
# ----------------------------------------------------------------------------
def _bwd_apply(inp, layout, dt, relu, x=None, mean=None, k=None, scale=None, shift=None, dy=None):
    C, wi, wo, c0 = layout
    xx = inp["x"] if x is None else x
    P = xx.shape[0]
    dyd, _ = put(inp["dy"] if dy is None else dy, dt, wi, c0)
    xd, _ = put(xx, dt, wo, c0)
    dx, gdx = out_rows(P, C, dt, wi, c0)
    sc, sh = vec(inp["scale"] if scale is None else scale)[0], vec(inp["shift"] if shift is None else shift)[0]
    mu, kk = vec(inp["mean"] if mean is None else mean)[0], vec(inp["k"] if k is None else k)[0]
    _L().call("vu_bn_bwd_apply", ptr(dyd), wi or C, ptr(xd), wo or C, P, C, ptr(sc), ptr(sh), ptr(mu), ptr(kk), relu,
              ptr(dx), wi or C, _code(dt), st())
    torch.cuda.synchronize()
    gdx.check("vu_bn_bwd_apply")
    return dx


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("layout", B.LAYOUTS, ids=B.layout_id)
def test_bn_bwd_apply(layout, dt):
    C = layout[0]
    Ps = B.pixel_counts(C)
    for P in Ps:
        inp = B.bn_inputs(P, C, dt)
        for relu in (1, 0):
            ref, sabs = B.bn_bwd_apply_ref(inp["dy"], inp["x"], inp["scale"], inp["shift"], inp["mean"], inp["k"], relu)
            base = None
            for name, kv in variants(layout, dt, P == Ps[-1]):
                with tuned(kv):
                    dx = _bwd_apply(inp, layout, dt, relu)
                note("bwd_apply", B.assert_el(cpu(dx), ref, sabs, B.BWD_APPLY_N, dt, f"bwd apply P={P} relu={relu} {name}"))
                base = dx if base is None else base
                assert torch.equal(dx, base), f"bwd apply P={P} {name}: bits differ from the default run"


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("layout", B.LAYOUTS, ids=B.layout_id)
def test_bn_bwd_apply2(layout, dt):
    """the paired apply: the bits of two single applies (no ReLU), each within
    the reference bound; refused off the vector path"""
    L = _L()
    C, wi, wo, c0 = layout
    s_in, s_out = wi or C, wo or C
    ok = L.query("vu_bn_bwd_apply2_ok", C, s_in, s_out, s_in, s_out, s_in)
    assert bool(ok) == B.is_vector(layout)
    if not ok:
        z = torch.zeros(8, device=DEV)
        rc = L.query("vu_bn_bwd_apply2", ptr(z), s_in, ptr(z), s_out, ptr(z), s_in, 1, C, ptr(z), ptr(z), ptr(z),
                     ptr(z), ptr(z), s_out, ptr(z), s_in, _code(dt), st())
        assert rc != 0
        return
    Ps = B.pixel_counts(C)
    for P in Ps:
        a, b = B.bn_inputs(P, C, dt), B.bn_inputs(P, C, dt, seed=52)
        refs = [B.bn_bwd_apply_ref(a["dy"], i["x"], i["scale"], i["shift"], i["mean"], i["k"], 0) for i in (a, b)]
        base = None
        for name, kv in variants(layout, dt, P == Ps[-1]):
            with tuned(kv):
                singles = [_bwd_apply(i, layout, dt, 0, dy=a["dy"]) for i in (a, b)]
                dy, _ = put(a["dy"], dt, wi, c0)
                x1, _ = put(a["x"], dt, wo, c0)
                x2, _ = put(b["x"], dt, wi, c0)
                d1, g1 = out_rows(P, C, dt, wo, c0)
                d2, g2 = out_rows(P, C, dt, wi, 0)
                co = [vec(t)[0] for t in (a["mean"], a["k"], b["mean"], b["k"])]
                L.call("vu_bn_bwd_apply2", ptr(dy), s_in, ptr(x1), s_out, ptr(x2), s_in, P, C, *(ptr(c) for c in co),
                       ptr(d1), s_out, ptr(d2), s_in, _code(dt), st())
                torch.cuda.synchronize()
                g1.check("vu_bn_bwd_apply2 dx1")
                g2.check("vu_bn_bwd_apply2 dx2")
            assert torch.equal(d1, singles[0]) and torch.equal(d2, singles[1]), f"apply2 P={P} {name}: not the bits of two applies"
            for d, (ref, sabs) in zip((d1, d2), refs):
                note("bwd_apply2", B.assert_el(cpu(d), ref, sabs, B.BWD_APPLY_N, dt, f"apply2 P={P} {name}"))
            base = (d1, d2) if base is None else base
            assert torch.equal(d1, base[0]) and torch.equal(d2, base[1])


# ----------------------------------------------------------------------------
# vu_bn_fwd_fused
# ----------------------------------------------------------------------------
def _fwd_fused(y, psum, pm2, tile_rows, P, C, gamma, beta, rm, rv, res, rsc, rsh, relu, dt, wi, wo, c0):
    L = _L()
    tiles = psum.shape[0]
    yd, _ = put(y, dt, wi, c0)
    rd = put(res, dt, wo, c0)[0] if res is not None else None
    out, go = out_rows(P, C, dt, wo, 0)
    g, b = vec(gamma)[0], vec(beta)[0]
    rmd, grm = vec(rm)
    rvd, grv = vec(rv)
    nbt, gn = empty_vec(1, dtype=torch.int64)
    nbt.fill_(2)
    coef, gc = empty_vec(4, C)
    rs_, rh_ = (vec(rsc)[0], vec(rsh)[0]) if rsc is not None else (None, None)
    assert L.query("vu_bn_fwd_fused_supported", tiles, C, wi or C, wo or C, wo or C)
    ps, pm = psum.to(DEV), pm2.to(DEV)
    L.call("vu_bn_fwd_fused", ptr(ps), ptr(pm), tiles, tile_rows, P, C, ptr(g), ptr(b), ptr(rmd),
           ptr(rvd), ptr(nbt), B.MOM, B.EPS, ptr(coef), ptr(yd), wi or C, ptr(rd), wo or C, ptr(rs_), ptr(rh_), ptr(out),
           wo or C, relu, _code(dt), st())
    torch.cuda.synchronize()
    for gd in (go, grm, grv, gn, gc):
        gd.check("vu_bn_fwd_fused")
    return out, cpu(coef), cpu(rmd), cpu(rvd), int(nbt[0])


FUSED_LAYOUTS = [(64, None, None, 0), (256, None, None, 0), (64, 128, 72, 8), (64, 72, 128, 0)]


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("resk", [None, "plain", "bn"])
@pytest.mark.parametrize("tiles", [1, 255, 256])
@pytest.mark.parametrize("layout", FUSED_LAYOUTS, ids=B.layout_id)
def test_bn_fwd_fused(layout, tiles, resk, dt):
    C, wi, wo, c0 = layout
    tile_rows = 8
    P = tiles * tile_rows - 3            # a ragged last tile
    inp = B.bn_inputs(P, C, dt)
    fin = B.finalize_inputs(4, 8, C)
    y = inp["x"] * 2 + 0.5
    y = y.to(dt).float()
    psum, pm2 = B.stats_of(y, tile_rows)
    res = inp["res"] if resk else None
    rsc, rsh = (inp["rscale"], inp["rshift"]) if resk == "bn" else (None, None)
    for relu in (1, 0):
        out, coef, rm, rv, nbt = _fwd_fused(y, psum, pm2, tile_rows, P, C, fin["gamma"], fin["beta"], fin["rm"], fin["rv"],
                                            res, rsc, rsh, relu, dt, wi, wo, c0)
        ref = B.bn_stats_ref(psum, pm2, tile_rows, P, fin["gamma"], fin["beta"], fin["rm"], fin["rv"], B.MOM, B.EPS)
        w = max(B.assert_fin(coef[i], ref[k], ref[k + "_abs"], f"fused {k}")
                for i, k in enumerate(("scale", "shift", "mean", "invstd")))
        w = max(w, B.assert_fin(rm, ref["rm"], ref["rm_abs"], "fused running_mean"),
                B.assert_fin(rv, ref["rv"], ref["rv_abs"], "fused running_var"))
        assert nbt == 3
        note("fwd_fused coef", w)
        # the apply stage from the device's own coefficients
        r, sabs = B.bn_apply_ref(y, coef[0], coef[1], relu, res, rsc, rsh)
        note("fwd_fused out", B.assert_el(cpu(out), r, sabs, B.FUSED_N, dt, f"fused out relu={relu}"))


def test_bn_fwd_fused_refuses():
    L = _L()
    assert L.query("vu_bn_fwd_fused_supported", 256, 64, 64, 64, 64) == 1
    assert L.query("vu_bn_fwd_fused_supported", 257, 64, 64, 64, 64) == 0
    assert L.query("vu_bn_fwd_fused_supported", 8, 48, 48, 48, 48) == 0
    assert L.query("vu_bn_fwd_fused_supported", 8, 64, 68, 64, 64) == 0
    z = torch.zeros(64, device=DEV)
    for tiles, C in ((257, 64), (8, 48)):   # rejected before any launch
        rc = L.query("vu_bn_fwd_fused", ptr(z), ptr(z), tiles, 8, 8, C, None, None, None, None, None, B.MOM, B.EPS, ptr(z),
                     ptr(z), C, None, C, None, None, ptr(z), C, 1, _L().F32, st())
        assert rc != 0


# ----------------------------------------------------------------------------
# vu_bn_bwd_fused
# ----------------------------------------------------------------------------
def _bwd_fused(inp, P, C, dt, relu, train, acc, wi, wo, c0):
    L = _L()
    dy, _ = put(inp["dy"], dt, wi, c0)
    x, _ = put(inp["x"], dt, wo, c0)
    dx, gdx = out_rows(P, C, dt, wo, 0)
    co = [vec(inp[k])[0] for k in ("scale", "shift", "mean", "invstd", "gamma")]
    dg, gdg = vec(inp["k"][0])
    db, gdb = vec(inp["k"][1])
    ws, gws = workspace(P, C)
    L.call("vu_bn_bwd_fused", ptr(dy), wi or C, ptr(x), wo or C, P, C, *(ptr(c) for c in co), relu, train, ptr(dg),
           ptr(db), acc, ptr(dx), wo or C, ptr(ws), _code(dt), st())
    torch.cuda.synchronize()
    for g in (gdx, gdg, gdb, gws):
        g.check("vu_bn_bwd_fused")
    return dx, cpu(dg), cpu(db)


# C = 128: a block covers 16 pixel rows per pass, the 16-row grid reaches the
# fused path's 128 blocks at P = 128 * 16 * 16
BWD_FUSED_PMAX = 128 * 16 * 16


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("case", [(BWD_FUSED_PMAX, 128, None, None, 0), (1, 128, None, None, 0), (1029, 64, 128, 72, 8),
                                  (777, 32, None, None, 0)], ids=lambda c: f"P{c[0]}-C{c[1]}-in{c[2]}")
def test_bn_bwd_fused(case, dt):
    L = _L()
    P, C, wi, wo, c0 = case
    assert L.query("vu_bn_bwd_fused_supported", P, C, wi or C, wo or C, wo or C) == 1
    inp = B.bn_inputs(P, C, dt)
    pre = inp["k"][:2]
    for relu, train in ((1, 1), (0, 1), (1, 0)):
        dx, dg, db = _bwd_fused(inp, P, C, dt, relu, train, 0, wi, wo, c0)
        part, pabs = B.bn_bwd_sums_ref(inp["dy"], inp["x"], inp["scale"], inp["shift"], inp["mean"], inp["invstd"], relu)
        ref = B.bn_finish_ref(part, pabs, inp["gamma"], inp["invstd"], P, train)
        what = f"bwd fused P={P} relu={relu} train={train}"
        note("bwd_fused sums", max(assert_lin(dg, ref["dgamma"], ref["dgamma_abs"], what + " dgamma"),
                                   assert_lin(db, ref["dbeta"], ref["dbeta_abs"], what + " dbeta")))
        # the apply stage from the device's own sums: two more roundings (k1 in
        # float32, the coefficient) than vu_bn_bwd_apply's four operations
        k1 = ref["coef"][0]
        k = torch.stack([k1, -k1 * inp["invstd"].double() * dg.double() / P, -k1 * db.double() / P])
        if not train:
            k[1:] = 0
        r, sabs = B.bn_bwd_apply_ref(inp["dy"], inp["x"], inp["scale"], inp["shift"], inp["mean"], k, relu)
        note("bwd_fused dx", B.assert_el(cpu(dx), r, sabs, B.BWD_APPLY_N + 2, dt, what + " dx"))
        # accumulating changes the gradients by the pre-fill and nothing else
        dx2, dg2, db2 = _bwd_fused(inp, P, C, dt, relu, train, 1, wi, wo, c0)
        assert torch.equal(dx2, dx)
        assert_lin(dg2, ref["dgamma"] + pre[0].double(), ref["dgamma_abs"], what + " dgamma acc", acc=pre[0])
        assert_lin(db2, ref["dbeta"] + pre[1].double(), ref["dbeta_abs"], what + " dbeta acc", acc=pre[1])


def test_bn_bwd_fused_refuses():
    L = _L()
    assert L.query("vu_bn_bwd_fused_supported", BWD_FUSED_PMAX, 128, 128, 128, 128) == 1
    assert L.query("vu_bn_bwd_fused_supported", BWD_FUSED_PMAX + 1, 128, 128, 128, 128) == 0
    assert L.query("vu_bn_bwd_fused_supported", 64, 48, 48, 48, 48) == 0
    z = torch.zeros(256, device=DEV)
    rc = L.query("vu_bn_bwd_fused", ptr(z), 128, ptr(z), 128, BWD_FUSED_PMAX + 1, 128, ptr(z), ptr(z), ptr(z), ptr(z),
                 ptr(z), 1, 1, ptr(z), ptr(z), 0, ptr(z), 128, ptr(z), L.F32, st())
    assert rc != 0


# ----------------------------------------------------------------------------
# vu_bn_apply_maxpool2
# ----------------------------------------------------------------------------
def _maxpool(y4, scale, shift, relu, dt, wi, wo, c0):
    """y4 CPU [N, H, W, C] -> (a [P, C], pool [Q, C]) device views"""
    N, H, W, C = y4.shape
    P, Q = N * H * W, N * (H // 2) * (W // 2)
    y, _ = put(y4.reshape(P, C), dt, wi, c0)
    a, ga = out_rows(P, C, dt, wo, c0)
    pool, gp = out_rows(Q, C, dt, wi, 0)
    sc, sh = vec(scale)[0], vec(shift)[0]
    _L().call("vu_bn_apply_maxpool2", ptr(y), wi or C, ptr(a), wo or C, ptr(pool), wi or C, N, H, W, C, ptr(sc), ptr(sh),
              relu, _code(dt), st())
    torch.cuda.synchronize()
    ga.check("vu_bn_apply_maxpool2 a")
    gp.check("vu_bn_apply_maxpool2 pool")
    return a, pool


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("layout", B.VECTOR, ids=B.layout_id)
@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 6, 10), (3, 34, 18)], ids=lambda s: "x".join(map(str, s)))
def test_bn_apply_maxpool2(shape, layout, dt):
    """a as vu_bn_apply stores it; the pool is the maximum of the STORED
    (rounded) values, exactly.  Small-integer inputs: ties between rounded
    values in most windows; relu off over all-negative windows."""
    C, wi, wo, c0 = layout
    N, H, W = shape
    g = torch.Generator().manual_seed(7 + C + H)
    inp = B.bn_inputs(N * H * W, C, dt)
    ints = torch.randint(-3, 4, (N, H, W, C), generator=g).float()
    for name, y4, scale, shift, relu in (
            ("random", inp["x"].reshape(N, H, W, C), inp["scale"], inp["shift"], 1),
            ("ties", ints, torch.full((C,), 1.0078125), torch.zeros(C), 1),
            ("negative", ints - 4, torch.full((C,), 1.0078125), torch.zeros(C), 0)):
        a, pool = _maxpool(y4, scale, shift, relu, dt, wi, wo, c0)
        ref, sabs = B.bn_apply_ref(y4.reshape(-1, C), scale, shift, relu)
        note("maxpool a", B.assert_el(cpu(a), ref, sabs, B.APPLY_N, dt, f"maxpool {name} a"))
        want = B.pool2_ref(cpu(a).reshape(N, H, W, C)).reshape(-1, C)
        assert torch.equal(cpu(pool), want), f"maxpool {name}: pool is not the maximum of the stored values"
        if name == "negative":
            assert float(cpu(pool).max()) < 0


def test_bn_apply_maxpool2_refuses():
    L = _L()
    z = torch.zeros(4096, device=DEV)
    for H, W, C, s in ((3, 4, 8, 8), (4, 3, 8, 8), (4, 4, 24, 24), (4, 4, 8, 12)):   # rejected before any launch
        rc = L.query("vu_bn_apply_maxpool2", ptr(z), s, ptr(z), s, ptr(z), s, 1, H, W, C, ptr(z), ptr(z), 1, L.F32, st())
        assert rc != 0, (H, W, C, s)


# ----------------------------------------------------------------------------
# vu_chan_sum
# ----------------------------------------------------------------------------
# (y0, x0, Hr, Wr) in a 7 x 9 image: dense, interior, each border, 1 x 1
WINDOWS = [(0, 0, 7, 9), (2, 3, 3, 4), (0, 1, 2, 5), (5, 2, 2, 3), (1, 0, 4, 2), (3, 6, 2, 3), (6, 8, 1, 1)]


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("C,wide,c0", [(2, None, 0), (8, None, 0), (40, None, 0), (64, None, 0), (8, 16, 8), (64, 72, 0),
                                      (64, 68, 4)])
def test_chan_sum(C, wide, c0, dt):
    L = _L()
    N, H, W = 3, 7, 9
    g = torch.Generator().manual_seed(17 + C)
    x4 = torch.randn(N, H, W, C, generator=g).to(dt).float()
    x, _ = put(x4.reshape(-1, C), dt, wide, c0)
    pre = torch.randn(C, generator=g)
    for (y0, x0, Hr, Wr) in WINDOWS:
        for acc in (0, 1):
            out, go = vec(pre)
            ws, gws = workspace(N * Hr * Wr, C)
            L.call("vu_chan_sum", ptr(x), wide or C, N, H, W, y0, x0, Hr, Wr, C, ptr(out), acc, ptr(ws), _code(dt), st())
            torch.cuda.synchronize()
            go.check("vu_chan_sum out")
            gws.check("vu_chan_sum workspace")
            ref, sabs = B.chan_sum_ref(x4, y0, x0, Hr, Wr)
            note("chan_sum", assert_lin(cpu(out), ref + (pre.double() if acc else 0), sabs,
                                        f"chan_sum window {(y0, x0, Hr, Wr)} acc={acc}", acc=pre if acc else None))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("C", [8, 64, 24])
def test_chan_sum_many_blocks(C, dt):
    """more than one block and the grid-stride loop: 3 R 16 + 5 pixels, dense"""
    L = _L()
    P = B.pixel_counts(C)[-1]
    g = torch.Generator().manual_seed(19 + C)
    xc = torch.randn(P, C, generator=g).to(dt).float()
    x, _ = put(xc, dt)
    for kv in ({}, {B.KEY_BN_MINBLK: 0}):
        with tuned(kv):
            out, go = empty_vec(C)
            ws, gws = workspace(P, C)
            L.call("vu_chan_sum", ptr(x), C, 1, P, 1, 0, 0, P, 1, C, ptr(out), 0, ptr(ws), _code(dt), st())
            torch.cuda.synchronize()
            go.check("vu_chan_sum out")
            gws.check("vu_chan_sum workspace")
        note("chan_sum", assert_lin(cpu(out), xc.double().sum(0), xc.double().abs().sum(0), f"chan_sum P={P}"))


# ----------------------------------------------------------------------------
# ReLU-mask agreement of the forward and the backward: exact
# ----------------------------------------------------------------------------
MASK_LAYOUTS = [(8, None, None, 0), (64, None, None, 0), (24, None, None, 0), (3, None, None, 0), (64, 68, 68, 4)]


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("layout", MASK_LAYOUTS, ids=B.layout_id)
def test_relu_mask_agreement(layout, dt):
    """A quarter of the pixels of each channel hold an x0 with shift =
    -fl32(x0 scale): the fused pre-activation is the product's rounding
    residual (either sign, or zero), the unfused one exactly 0.  The forward
    kernels leave the multiply-add to the compiler, the backward kernels mask
    by fmaf(x, scale, shift) > 0 (chan_partial_scalar by a contractable
    expression): (forward output > 0) == (dx != 0) for every element, and
    dbeta[c] is the count of positive forward outputs of channel c (dy = 1;
    exact in float32 for P < 2^24)."""
    L = _L()
    C, wi, wo, c0 = layout
    N, H, W = 1, 32, 32
    P = N * H * W
    x, scale, shift, planted = B.planted_mask_inputs(P, C, dt)
    inp = dict(x=x, dy=torch.ones(P, C), scale=scale, shift=shift, mean=torch.zeros(C), invstd=torch.ones(C),
               gamma=torch.ones(C), k=torch.stack([torch.ones(C), torch.zeros(C), torch.zeros(C)]))
    dx = cpu(_bwd_apply(inp, layout, dt, 1))
    assert bool(((dx == 0) | (dx == 1)).all())
    on = dx != 0
    # the planted elements exercise both sides of the mask
    assert bool(on[planted].any()) and bool((~on[planted]).any())
    _, db, _ = _reduce(inp, layout, dt, 1, 1, 0, False)
    fwd = {"vu_bn_apply": cpu(_apply(inp, layout, dt, 1))}
    if B.is_vector(layout):
        a, _ = _maxpool(x.reshape(N, H, W, C), scale, shift, 1, dt, wi, wo, c0)
        fwd["vu_bn_apply_maxpool2"] = cpu(a)
    if C % 32 == 0 and B.is_vector(layout):
        # the fused forward forms its own coefficients: all-zero sums give mean = 0 and shift = beta exactly; its
        # scale = gamma invstd is read back from a first launch and beta planted against it
        tiles, tr = 128, 8
        psum, pm2 = torch.zeros(tiles, C), torch.full((tiles, C), 6.0)
        args = (x, psum, pm2, tr, P, C, scale, shift, torch.zeros(C), torch.ones(C), None, None, None, 1, dt, wi, wo, c0)
        _, coef, _, _, _ = _fwd_fused(*args)
        x0 = x[planted.float().argmax(0), torch.arange(C)]
        beta = -(x0 * coef[0])
        xf = torch.where(planted, x0.expand(P, C), x)
        args = (xf, psum, pm2, tr, P, C, scale, beta) + args[8:]
        out, coef2, _, _, _ = _fwd_fused(*args)
        assert torch.equal(coef2[0], coef[0]) and torch.equal(coef2[1], beta)
        inp_f = dict(inp, x=xf, scale=coef2[0], shift=coef2[1])
        dxf = cpu(_bwd_apply(inp_f, layout, dt, 1))
        assert torch.equal(cpu(out) > 0, dxf != 0), "vu_bn_fwd_fused: forward and backward ReLU masks differ"
    for name, y in fwd.items():
        bad = (y > 0) != on
        assert not bool(bad.any()), (f"{name}: forward and backward ReLU masks differ at {int(bad.sum())} elements "
                                     f"({int((bad & planted).sum())} of them planted)")
        assert torch.equal(db, (y > 0).sum(0).float()), f"{name}: dbeta is not the count of positive outputs"
