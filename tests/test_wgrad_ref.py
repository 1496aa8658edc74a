"""CPU self-checks of tests/wgrad_ref.py (no GPU, the library is not loaded):
the reference against torch's own weight gradients, a float32 emulation of the
kernels inside the random-operand bound on every input set the GPU file uses,
the impulse references exactly float32, and planted defects caught by the
check aimed at them."""
import pytest
import torch

import ref_small as R
import wgrad_ref as G
from wgrad_ref import BF16, Geo


def _problem(geo, dtype, ops=None, strided=False):
    """CPU descriptors over guarded NHWC tensors -> (gp, gq, p_t, q_ts)"""
    P, Q = ops if ops is not None else G.operands(geo, dtype)
    p_t, _ = G.place(P, dtype, "cpu", strided)
    q_ts = [G.place(q, dtype, "cpu", strided)[0] for q in Q]
    gp, gq = G.descriptors(geo, p_t, q_ts)
    return gp, gq, p_t, q_ts


def _all_geos():
    seen = {}
    for r in G.ALL_RUNS + G.IMPULSE_RUNS:
        seen.setdefault((r.geo, r.dtype), None)
    for g, _ in G.PLAN_GEOS:
        seen.setdefault((g, BF16), None)
    return list(seen)


GEOS = _all_geos()


def test_every_kind_and_edge_is_in_the_lists():
    kinds = {g.kind for g, _ in GEOS}
    assert kinds == {"3x3", "1x1", "1x1s2", "3x3s2", "stem", "convT"}
    assert any(g.odd != (0, 0) for g, _ in GEOS) and any(len(g.cins) == 3 for g, _ in GEOS)
    assert any(g.kind == "convT" and g.pyx != (0, 0) for g, _ in GEOS)


@pytest.mark.parametrize("geo,dtype", GEOS, ids=[f"{g}-{d}".replace(" ", "_") for g, d in GEOS])
def test_reference_equals_torch_weight_gradient(geo, dtype):
    """wgrad_ref from the descriptors (dense and channel-slice operands) =
    conv2d_weight / autograd through conv_transpose2d, fp64 to 1e-12"""
    P, Q = G.operands(geo, dtype)
    want = G.to_itc(G.autograd_grad(geo, P, Q))
    for strided in (False, True):
        gp, gq, _, _ = _problem(geo, dtype, strided=strided)
        ref, sabs = G.wgrad_ref(gp, gq, geo.ni, geo.nj)
        assert ref.dtype == torch.float64 and ref.shape == (geo.ni, geo.nj)
        got = ref.view(geo.ni, geo.taps, geo.C)[..., :geo.cvalid]
        s = sabs.view(geo.ni, geo.taps, geo.C)[..., :geo.cvalid]
        assert got.shape == want.shape
        assert bool(((got - want).abs() <= 1e-12 * (1 + s)).all()), float((got - want).abs().max())
        assert bool((sabs >= ref.abs() * (1 - 1e-12)).all())


def _emul_runs():
    seen = {}
    for r in G.ALL_RUNS:
        seen.setdefault((r.geo, r.dtype, r.plans, r.tile), r)
    return list(seen.values())


@pytest.mark.parametrize("run", _emul_runs(), ids=lambda r: r.id)
def test_float32_emulation_meets_the_bound(run):
    """per-split float32 matmuls + the float32 slab sum in the kernel's lane
    order stay inside the random-operand bound on every GPU input set: the
    reference-side computation alone does not eat the bound"""
    geo = run.geo
    gp, gq, _, _ = _problem(geo, run.dtype)
    P, Q = G.gathered(gp, gq, geo.ni, geo.nj)
    ref, sabs = P.t() @ Q, P.abs().t() @ Q.abs()
    pick = lambda t: t.view(geo.ni, geo.taps, geo.C)[..., :geo.cvalid]  # noqa: E731
    for mps, splits in run.plans:
        rows = G.split_rows(geo, mps, splits, run.tile)
        assert sorted(torch.cat(rows).tolist()) == list(range(geo.M)), "the plan covers every pixel once"
        for vec in (True, False):
            grad, _, layout = G.grad_sink(geo.grad_shape, "contig", "cpu")
            G.emulate(geo, P, Q, mps, splits, run.tile, grad, layout, False, vec)
            worst = G.check_bound(G.to_itc(grad), pick(ref), G.bound_random(geo.M, pick(sabs), run.dtype),
                                  f"emulation {geo} mps {mps} x {splits}")
            assert worst < 0.25     # (the reference side leaves the kernels at least 3/4 of the bound)


@pytest.mark.parametrize("geo,_t", G.PLAN_GEOS, ids=[str(g).replace(" ", "_") for g, _ in G.PLAN_GEOS])
@pytest.mark.parametrize("kind", ["contig", "cl"])
def test_float32_emulation_meets_the_accumulate_bound(geo, _t, kind):
    gp, gq, _, _ = _problem(geo, BF16)
    P, Q = G.gathered(gp, gq, geo.ni, geo.nj)
    old = torch.randn(geo.grad_shape, generator=torch.Generator().manual_seed(5))
    grad, guard, layout = G.grad_sink(geo.grad_shape, kind, "cpu", old=old)
    slab = G.emulate(geo, P, Q, 128, -(-geo.M // 128), None, grad, layout, True)
    assert slab.shape == (-(-geo.M // 128), geo.ni, geo.nj)
    ref, sabs = G.wgrad_ref(gp, gq, geo.ni, geo.nj)
    pick = lambda t: t.view(geo.ni, geo.taps, geo.C)[..., :geo.cvalid]  # noqa: E731
    o = G.to_itc(old)
    G.check_bound(G.to_itc(grad), pick(ref) + o.double(), G.bound_random(geo.M, pick(sabs), BF16, old=o),
                  f"accumulating emulation {geo} {kind}")
    guard.check("gradient")


@pytest.mark.parametrize("shape", G.SLAB_SHAPES)
def test_slab_reduce_emulation_meets_its_bound(shape):
    """(splits - 1 + accumulate) 2^-24 sabs holds for the float32 lane-order
    sum on the slab inputs of the GPU file, in every layout"""
    ni, nj, C, cv = shape
    gshape = G.slab_grad_shape(ni, nj, C, cv)
    for splits in G.SLAB_SPLITS:
        slab = G.slab_input(splits, ni, nj)
        for kind in ("contig", "cl", "sub"):
            for acc in (0, 1):
                old = torch.randn(gshape, generator=torch.Generator().manual_seed(splits)) if acc else None
                grad, guard, layout = G.grad_sink(gshape, kind, "cpu", old=old, wide=2)
                before = guard.buf.clone()
                ref, sabs = G.slab_ref(slab, layout, C, cv, G.same_view(before, grad) if acc else None)
                G.slab_reduce_emul(slab, C, cv, layout, grad, acc, vectorised=(ni * nj) % 4 == 0)
                taps = nj // C
                got = G.grad_view(grad, ni, taps, cv, layout)
                w = G.check_bound(got, ref, (splits - 1 + acc) * G.U32 * sabs, f"slab emulation {shape} x {splits}")
                assert w <= 1.0
                guard.check("gradient")
                G.check_untouched(guard.buf, before, G.written_mask(guard.buf, grad, ni, taps, cv, layout), "grad")


def test_slab_lane_selection_covers_every_instantiation():
    lanes = {G.slab_lanes(s, True) for s in G.SLAB_SPLITS}
    assert lanes == {1, 2, 4, 8, 16}
    for sl, lo in ((2, 8), (4, 16), (8, 32), (16, 64)):       # both sides of every selection threshold
        assert lo - 1 in G.SLAB_SPLITS and lo in G.SLAB_SPLITS and lo + 1 in G.SLAB_SPLITS
        assert G.slab_lanes(lo - 1, True) == sl // 2 and G.slab_lanes(lo, True) == sl
    # and of the 4 SL unroll (k + 3 SL < splits): a whole number of unrolled passes with no tail
    # (4 SL), one more split (lane 0 alone has a tail), one short of the next pass (every lane's
    # tail at its longest; 16 lanes: two passes and a tail); one lane: no unrolled pass (1, 2, 3)
    # and one pass plus a tail (7)
    for sl in (2, 4, 8, 16):
        for s in (4 * sl, 4 * sl + 1, 8 * sl - 1 if sl < 16 else 130):
            assert s in G.SLAB_SPLITS and G.slab_lanes(s, True) == sl
    assert {1, 2, 3, 7} <= set(G.SLAB_SPLITS) and G.slab_lanes(7, True) == 1
    assert G.slab_lanes(130, True) == 16 and 130 > 2 * 64


# ----------------------------------------------------------------------------
# impulse inputs
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("run", G.IMPULSE_RUNS, ids=lambda r: r.id)
def test_impulse_reference_is_exactly_float32(run):
    geo = run.geo
    pick = lambda t: t.view(geo.ni, geo.taps, geo.C)[..., :geo.cvalid]  # noqa: E731
    for mps, splits in run.plans:
        sets = G.impulse_sets(run, mps)
        assert {s for s, _ in sets} == {"P", "Q"}
        covered = set()
        for side, px in sets:
            gp, gq, _, _ = _problem(geo, run.dtype, G.impulse_operands(geo, run.dtype, side, px))
            P, Q = G.gathered(gp, gq, geo.ni, geo.nj)
            terms = (P != 0).double().t() @ (Q != 0).double()
            assert int(terms.max()) <= 1, "at most one non-zero term per sum"
            ref = P.t() @ Q
            assert bool((ref.float().double() == ref).all())
            assert int((ref != 0).sum()) > 0
            grad, _, layout = G.grad_sink(geo.grad_shape, "contig", "cpu")
            slab = G.emulate(geo, P, Q, mps, splits, run.tile, grad, layout, False)
            G.check_exact(G.to_itc(grad), pick(ref), f"emulated {geo} impulse {side}")
            G.check_exact(slab.double().sum(0), ref, "raw slabs")
            if side == "P":
                covered.update(px)
        assert covered == set(G.seam_pixels(geo, G.run_step(run), mps))


def test_seam_pixels_name_what_they_should():
    geo = Geo("3x3", 2, 8, 64, (64,), 72)
    s = set(G.seam_pixels(geo, (32, 4), 384))
    lin = lambda n, y, x: (n * 8 + y) * 64 + x  # noqa: E731
    for n in (0, 1):
        for y, x in ((0, 0), (0, 63), (7, 0), (7, 63), (0, 32), (4, 0), (7, 32), (4, 63)):   # corners, midpoints
            assert lin(n, y, x) in s
        for y, x in ((0, 31), (0, 32), (3, 0), (4, 0), (3, 31), (4, 32), (3, 32), (4, 31)):   # tile seams
            assert lin(n, y, x) in s
    assert lin(0, 7, 63) in s and lin(1, 0, 0) in s and geo.M - 1 in s                           # image seam, M - 1
    # split seams of 3 tiles per split: tiles 2 | 3 (image 0, column 1) and 5 | 6 (image 1, columns 0 | 1)
    walk = G.tile_walk(2, 8, 64, 32, 4)
    assert walk[2] == (0, 0, 32) and walk[3] == (0, 4, 32) and walk[5] == (1, 4, 0) and walk[6] == (1, 0, 32)
    for (n, y0, x0) in (walk[2], walk[3], walk[5], walk[6]):
        assert lin(n, y0, x0) in s and lin(n, y0 + 3, x0 + 31) in s
    s = set(G.seam_pixels(Geo("3x3", 2, 9, 7, (8,), 64), 64, 25))
    assert {24, 25, 49, 50, 63, 64, 62, 63, 125, 0, 6} <= s


# ----------------------------------------------------------------------------
# planted defects: each on an otherwise correct emulation, caught by its check
# ----------------------------------------------------------------------------
LIN = (Geo("3x3", 2, 9, 7, (8,), 72), None, 25, 6)
HALO = (Geo("3x3", 2, 8, 64, (64,), 72), (32, 4), 384, 3)
STEM = (Geo("stem", 2, 7, 7, (8,), 64, odd=(1, 1)), None, 64, 2)


def _emul_check(case, P, Q, ref, sabs, rows=None, exact=False, accumulate=False, assume_old=None):
    """emulate (with ``rows`` in place of the plan's) and run the GPU file's
    result check"""
    geo, tile, mps, splits = case
    old = assume_old
    grad, _, layout = G.grad_sink(geo.grad_shape, "contig", "cpu", old=old)
    rows = rows if rows is not None else G.split_rows(geo, mps, splits, tile)
    slab = G.emulate_slabs(P, Q, rows)
    G.slab_reduce_emul(slab, geo.C, geo.cvalid, layout, grad, accumulate)
    pick = lambda t: t.view(geo.ni, geo.taps, geo.C)[..., :geo.cvalid]  # noqa: E731
    if exact:
        G.check_exact(G.to_itc(grad), pick(ref), "planted")
        return
    o = None if old is None else G.to_itc(old)
    want = pick(ref) if o is None else pick(ref) + o.double()
    G.check_bound(G.to_itc(grad), want, G.bound_random(geo.M, pick(sabs), BF16, old=o), "planted")


def _gathered(geo, ops=None, strided=False):
    gp, gq, p_t, q_ts = _problem(geo, BF16, ops, strided)
    P, Q = G.gathered(gp, gq, geo.ni, geo.nj)
    return P, Q, P.t() @ Q, P.abs().t() @ Q.abs()


@pytest.mark.parametrize("case", [LIN, HALO], ids=["linear", "halo"])
@pytest.mark.parametrize("defect", ["dropped", "twice"])
def test_planted_split_seam_defects(case, defect):
    """a pixel dropped at a split seam / counted in two splits: the random
    bound and the impulse_P comparison both catch it"""
    geo, tile, mps, splits = case
    rows = G.split_rows(geo, mps, splits, tile)
    bad = list(rows)
    if defect == "dropped":
        bad[1] = rows[1][1:]
    else:
        bad[0] = torch.cat([rows[0], rows[1][:1]])
    seam = int(rows[1][0])
    seams = G.seam_pixels(geo, tile if tile else 64, mps)
    assert seam in seams
    chunk = next(c for c in G.chunks(seams, geo.ni) if seam in c)
    for ops, exact in ((None, False), (G.impulse_operands(geo, BF16, "P", chunk), True)):
        P, Q, ref, sabs = _gathered(geo, ops)
        _emul_check(case, P, Q, ref, sabs, exact=exact)
        with pytest.raises(AssertionError):
            _emul_check(case, P, Q, ref, sabs, rows=bad, exact=exact)


@pytest.mark.parametrize("case", [LIN, HALO], ids=["linear", "halo"])
def test_planted_tap_shifted_by_a_column(case):
    from vaeunet_amd import kernels as K
    geo = case[0]
    seams = G.source_pixels(geo, G.seam_pixels(geo, case[1] if case[1] else 64, case[2]))
    for ops, exact in ((None, False), (G.impulse_operands(geo, BF16, "Q", seams[:geo.C]), True)):
        gp, gq, p_t, q_ts = _problem(geo, BF16, ops)
        P, Q = G.gathered(gp, gq, geo.ni, geo.nj)
        ref, sabs = P.t() @ Q, P.abs().t() @ Q.abs()
        kw = dict(geo.qkw, ox=geo.qkw["ox"] + 1)
        _, Q2 = G.gathered(gp, K.gather(q_ts, geo.N, geo.H, geo.W, **kw), geo.ni, geo.nj)
        bad = Q.clone()
        bad[:, 5 * geo.C:6 * geo.C] = Q2[:, 5 * geo.C:6 * geo.C]
        _emul_check(case, P, Q, ref, sabs, exact=exact)
        with pytest.raises(AssertionError):
            _emul_check(case, P, bad, ref, sabs, exact=exact)


@pytest.mark.parametrize("case", [LIN, HALO], ids=["linear", "halo"])
def test_planted_left_halo_column_from_the_previous_row(case):
    """taps with s = 0 at w = 0 read the pixel before the row (the previous
    row's last one) instead of the zero padding"""
    geo, tile, mps, splits = case
    H, W, C = geo.H, geo.W, geo.C
    left = [m for m in G.seam_pixels(geo, tile if tile else 64, mps) if m % W == 0]
    assert left
    for ops, exact in ((None, False), (G.impulse_operands(geo, BF16, "P", left[:geo.ni]), True)):
        gp, gq, p_t, q_ts = _problem(geo, BF16, ops)
        P, Q = G.gathered(gp, gq, geo.ni, geo.nj)
        ref, sabs = P.t() @ Q, P.abs().t() @ Q.abs()
        flat = torch.cat([t.double() for t in q_ts], 1).permute(0, 2, 3, 1).reshape(-1, C)
        bad = Q.clone()
        for m in range(geo.M):
            n, rem = divmod(m, H * W)
            h, w = divmod(rem, W)
            if w != 0:
                continue
            for r in range(3):
                y = h + r - 1
                src = (n * H + y) * W - 1
                if 0 <= y < H and src >= 0:
                    assert float(Q[m, (r * 3) * C:(r * 3 + 1) * C].abs().max()) == 0.0
                    bad[m, (r * 3) * C:(r * 3 + 1) * C] = flat[src]
        _emul_check(case, P, Q, ref, sabs, exact=exact)
        with pytest.raises(AssertionError):
            _emul_check(case, P, bad, ref, sabs, exact=exact)


def test_planted_unwritten_slab():
    geo, tile, mps, splits = LIN
    P, Q, _, _ = _gathered(geo)
    slab = G.emulate_slabs(P, Q, G.split_rows(geo, mps, splits, tile))
    G.check_slab_written(slab, "slab")
    slab[4] = R.SENTINEL
    with pytest.raises(AssertionError, match="not written"):
        G.check_slab_written(slab, "slab")
    slab = G.emulate_slabs(P, Q, G.split_rows(geo, mps, splits, tile))
    slab[2, geo.ni - 1, geo.nj - 8:] = R.SENTINEL          # a skipped partial edge tile
    with pytest.raises(AssertionError, match="not written"):
        G.check_slab_written(slab, "slab")


def test_planted_channels_past_cvalid_written():
    geo, tile, mps, splits = STEM
    P, Q, _, _ = _gathered(geo)
    slab = G.emulate_slabs(P, Q, G.split_rows(geo, mps, splits, tile))
    for cv, ok in ((geo.cvalid, True), (geo.C, False)):
        grad, guard, layout = G.grad_sink(geo.grad_shape, "sub", "cpu", wide=5)
        before = guard.buf.clone()
        G.slab_reduce_emul(slab, geo.C, cv, layout, grad, False)
        written = G.written_mask(guard.buf, grad, geo.ni, geo.taps, geo.cvalid, layout)
        guard.check("gradient")
        if ok:
            G.check_untouched(guard.buf, before, written, "gradient")
        else:
            with pytest.raises(AssertionError, match="outside the written set"):
                G.check_untouched(guard.buf, before, written, "gradient")


def test_planted_neighbour_channels_of_the_slice():
    """the operand read from the other half of the wide tensor (a pixel stride
    / channel offset mistake)"""
    geo = LIN[0]
    gp, gq, p_t, q_ts = _problem(geo, BF16, strided=True)
    P, Q = G.gathered(gp, gq, geo.ni, geo.nj)
    ref, sabs = P.t() @ Q, P.abs().t() @ Q.abs()
    _emul_check(LIN, P, Q, ref, sabs)
    wrong = torch.as_strided(p_t, p_t.shape, p_t.stride(), p_t.storage_offset() - geo.ni)
    gp2, _ = G.descriptors(geo, wrong, q_ts)
    P2, _ = G.gathered(gp2, gq, geo.ni, geo.nj)
    assert float(P2.abs().min()) > 0                   # the other half holds non-zero values
    with pytest.raises(AssertionError):
        _emul_check(LIN, P2, Q, ref, sabs)


def test_planted_accumulate_ignores_the_old_value():
    geo = LIN[0]
    P, Q, ref, sabs = _gathered(geo)
    old = torch.randn(geo.grad_shape, generator=torch.Generator().manual_seed(5))
    _emul_check(LIN, P, Q, ref, sabs, accumulate=True, assume_old=old)
    with pytest.raises(AssertionError):
        _emul_check(LIN, P, Q, ref, sabs, accumulate=False, assume_old=old)


def test_checks_reject_what_they_should():
    ref = torch.tensor([[1.0, 2.0]], dtype=torch.float64)
    with pytest.raises(AssertionError):
        G.check_bound(ref + 1e-3, ref, torch.full_like(ref, 1e-6), "x")
    with pytest.raises(AssertionError):
        G.check_bound(torch.tensor([[float("nan"), 2.0]], dtype=torch.float64), ref, torch.full_like(ref, 1.0), "x")
    with pytest.raises(AssertionError, match="not exactly a float32"):
        G.check_exact(ref.float(), ref + 1e-12, "x")
    with pytest.raises(AssertionError, match="differ"):
        G.check_exact(torch.tensor([[1.0, 2.0000002]]), ref, "x")
    G.check_exact(torch.tensor([[1.0, 2.0]]), ref, "x")
    G.check_exact(torch.tensor([[-0.0]]), torch.zeros(1, 1, dtype=torch.float64), "signed zero")
