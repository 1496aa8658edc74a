"""Kernel-level tests of the weight-gradient path: vu_gemm_wgrad in its three
generations (gemm_wgrad.hip v1, gemm_wgrad2.hip v2, gemm_wgrad3.hip v3) and
vu_slab_reduce, against the fp64 evaluation of the contraction their
descriptors define (tests/wgrad_ref.py, where the bound, the impulse inputs
and the case lists are; tests/test_wgrad_ref.py checks those on the CPU).

Every case calls the C-ABI directly with an explicit (m_per_split, splits),
sets its tuning keys with vu_gemm_set_tuning (restored in ``finally``), first
asserts the (generation, bi, bj) vu_gemm_wgrad_tile answers, and keeps the
operands, the slab and the gradient in guarded buffers:

  * every guard intact, no sentinel left in slab[splits][ni][nj], every
    element of the gradient's storage outside the written (i, tap, c < cvalid)
    set bit-unchanged;
  * random operands: |dW - ref| <= (M - 1) 2^-24 sabs per element (fp32:
    2M - 1; accumulating: M and |old| joins), for the reduced gradient and for
    the fp64 sum of the raw slabs; the worst err/bound and its index printed;
  * impulse operands: the reduced gradient and the sum of the raw slabs equal
    the fp64 reference bit for bit.

MI355X figures (profiles/wgrad_kernel_tests.log; reported, not caps): worst
err/bound v1 bf16 0.031, v1 fp32 0.033 (both at M = 35), v2 0.0036, v3 0.012;
vu_slab_reduce 0.9997 (one addition: the bound is then half an ulp of the
result)."""
import ctypes as C

import pytest
import torch

import ref_small as R
import wgrad_ref as G
from test_gpu_kernels import DEV

pytestmark = pytest.mark.gpu


def _k():
    from vaeunet_amd import kernels as K
    return K


class _tuning:
    """set the run's keys; back to the defaults of csrc/tuning.hip on exit"""

    def __init__(self, tune):
        self.tune = tune

    @staticmethod
    def _set(key, value):
        from vaeunet_amd import _lib
        _lib.call("vu_gemm_set_tuning", getattr(_lib, key), value)

    def __enter__(self):
        for k, v in list(G.TUNE_DEFAULTS.items()) + list(self.tune):   # (whatever an earlier test left)
            self._set(k, v)

    def __exit__(self, *exc):
        for k, v in G.TUNE_DEFAULTS.items():
            self._set(k, v)


@pytest.fixture(autouse=True)
def _default_tuning():
    """every test starts from, and leaves, the default dispatch"""
    with _tuning(()):
        yield


def _problem(run, ops):
    """operands in guarded device buffers -> (VuGemmWgrad without a plan, gp, gq, guards)"""
    from vaeunet_amd import _lib
    geo = run.geo
    P, Q = ops
    p_t, pg = G.place(P, run.dtype, DEV, run.sp)
    qs = [G.place(q, run.dtype, DEV, run.sq) for q in Q]
    gp, gq = G.descriptors(geo, p_t, [t for t, _ in qs])
    w = _lib.VuGemmWgrad()
    w.p, w.q, w.ni, w.nj = gp, gq, geo.ni, geo.nj
    return w, gp, gq, [pg] + [g for _, g in qs]


def _assert_tile(w, run):
    K = _k()
    bi, bj = C.c_int(0), C.c_int(0)
    gen = K.query("vu_gemm_wgrad_tile", C.byref(w), run.dtype, C.byref(bi), C.byref(bj))
    assert (gen, bi.value, bj.value) == run.expect, f"{run.id}: dispatched to {(gen, bi.value, bj.value)}"
    return gen


def _tag(run, mps):
    """the kernel that runs: a v3 answer with a split off the 128-pixel
    granule is launched on v2"""
    gen = run.expect[0]
    if gen == 3 and mps % 128:
        gen = 2
    return f"[v{gen} {'bf16' if run.dtype else 'fp32'}]"


def _head(run, mps=0):
    """what a log line says of a run: the kernel that runs, the problem, the asserted dispatch"""
    tune = ", ".join(f"{k[8:]}={v}" for k, v in run.tune) or "default tuning"
    return (f"{_tag(run, mps)} {run.geo}{' sp' if run.sp else ''}{' sq' if run.sq else ''}, {tune}: "
            f"gen {run.expect[0]} tile {run.expect[1]}x{run.expect[2]}")


def _launch(run, ops, mps, splits, kind="contig", exact=False):
    """vu_gemm_wgrad + vu_slab_reduce of one plan, every check.  The caller
    has set the tuning.  -> the worst err/bound (random operands)"""
    K = _k()
    geo = run.geo
    ni, nj, taps, cv = geo.ni, geo.nj, geo.taps, geo.cvalid
    w, gp, gq, guards = _problem(run, ops)
    w.splits, w.m_per_split = splits, mps
    _assert_tile(w, run)
    slab, gslab = R.guarded((splits, ni, nj), torch.float32, DEV)
    w.out = slab.data_ptr()
    grad, ggrad, layout = G.grad_sink(geo.grad_shape, kind, DEV, wide=3)
    before = ggrad.buf.clone()
    what = f"mps {mps} x {splits} {kind}"
    K.call("vu_gemm_wgrad", C.byref(w), run.dtype, K.stream())
    K.call("vu_slab_reduce", K.ptr(slab), splits, ni, nj, geo.C, cv, *layout, K.ptr(grad), 0, K.stream())
    torch.cuda.synchronize()
    for g in guards:
        g.check("operand")
    gslab.check("slabs")
    ggrad.check("gradient")
    G.check_slab_written(slab, what)
    G.check_untouched(ggrad.buf, before, G.written_mask(ggrad.buf, grad, ni, taps, cv, layout), what)
    ref, sabs = G.wgrad_ref(gp, gq, ni, nj)
    pick = lambda t: t.view(ni, taps, geo.C)[..., :cv]  # noqa: E731
    got = G.grad_view(grad, ni, taps, cv, layout)
    if exact:
        G.check_exact(got, pick(ref), what)
        G.check_exact(slab.double().sum(0), ref, what + " (raw slabs)")
        return None
    return max(G.check_bound(got, pick(ref), G.bound_random(geo.M, pick(sabs), run.dtype), what),
               G.check_bound(slab.double().sum(0), ref, G.bound_random(geo.M, sabs, run.dtype), what + " (raw slabs)"))


def _run_random(run):
    ops = G.operands(run.geo, run.dtype)
    with _tuning(run.tune):
        worst = [_launch(run, ops, mps, splits, kind=("contig", "cl", "sub")[k % 3])
                 for k, (mps, splits) in enumerate(run.plans)]
    print(f"{_head(run, run.plans[-1][0])}, plans {list(run.plans)}: {max(worst)}")


# ----------------------------------------------------------------------------
# A. vu_slab_reduce alone
# ----------------------------------------------------------------------------
def _reduce_once(slab, shape, kind, acc, old, what):
    from vaeunet_amd import engine as E
    K = _k()
    ni, nj, Cc, cv = shape
    splits, taps = slab.shape[0], nj // Cc
    gshape = G.slab_grad_shape(ni, nj, Cc, cv)
    grad, guard, layout = G.grad_sink(gshape, kind, DEV, old=old, wide=2)
    assert layout == (E.convT_layout(grad) if taps == 4 else E.conv_layout(grad))
    before = guard.buf.clone()
    K.call("vu_slab_reduce", K.ptr(slab), splits, ni, nj, Cc, cv, *layout, K.ptr(grad), acc, K.stream())
    torch.cuda.synchronize()
    guard.check("gradient")
    G.check_untouched(guard.buf, before, G.written_mask(guard.buf, grad, ni, taps, cv, layout), what)
    ref, sabs = G.slab_ref(slab, layout, Cc, cv, G.same_view(before, grad) if acc else None)
    got = G.grad_view(grad, ni, taps, cv, layout)
    return got.clone(), G.check_bound(got, ref, (splits - 1 + acc) * G.U32 * sabs, what)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("shape", G.SLAB_SHAPES)
def test_slab_reduce(shape, acc):
    """every slab_reduce4_kernel<SL> (1, 2, 4, 8, 16 split lanes, both sides of
    each selection threshold and of the 4 SL unroll) and the scalar kernel
    (tot % 4 != 0, a slab pointer off 16 bytes, VU_TUNE_SLAB4 = 0), into the
    contiguous, channels_last and sub-range layouts (taps = 4: the ConvT
    [Ci, Co, 2, 2] ones).  Two runs bit-equal."""
    ni, nj, Cc, cv = shape
    gshape = G.slab_grad_shape(ni, nj, Cc, cv)
    old = torch.randn(gshape, generator=torch.Generator().manual_seed(11)) if acc else None
    worst = {}          # per kernel: split lanes of the vectorised one, or "scalar"
    for splits in G.SLAB_SPLITS:
        src = G.slab_input(splits, ni, nj)
        for off, slab4 in ((0, 1), (1, 1), (0, 0)):
            slab, gslab = R.guarded((splits, ni, nj), torch.float32, DEV, offset=off)
            assert (slab.data_ptr() % 16 == 0) == (off == 0)
            slab.copy_(src)
            with _tuning(((G.SLAB4, slab4),)):
                for kind in (("contig", "cl", "sub") if (off, slab4) == (0, 1) else ("contig",)):
                    vec = slab4 == 1 and off == 0 and ni * nj % 4 == 0
                    kern = f"SL{G.slab_lanes(splits, True)}" if vec else "scalar"
                    what = f"splits {splits} offset {off} SLAB4={slab4} {kind}"
                    a, w = _reduce_once(slab, shape, kind, acc, old, what)
                    b, _ = _reduce_once(slab, shape, kind, acc, old, what + " (again)")
                    assert torch.equal(a, b), what
                    worst[kern] = max(worst.get(kern, w), w)
            gslab.check("slabs")
            assert torch.equal(slab.cpu(), src), "the reduce changed its input"
    assert set(worst) == ({"SL1", "SL2", "SL4", "SL8", "SL16", "scalar"} if ni * nj % 4 == 0 else {"scalar"})
    print(f"[slab] {shape} acc {acc}: " + ", ".join(f"{k} {float(v):.3f}" for k, v in worst.items())
          + f": {max(worst.values())}")


# ----------------------------------------------------------------------------
# B, C, D. the three generations on random operands
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("run", G.V1_RUNS, ids=lambda r: r.id)
def test_v1(run):
    """register-staged kernel, 64 x 128 and 128 x 128 tiles, fp32 (always v1)
    and bf16 (VU_TUNE_GEN = 1, or M < 512 under the default tuning): one
    split, 64-pixel splits, and one empty split more"""
    _run_random(run)


@pytest.mark.parametrize("run", G.V2_RUNS, ids=lambda r: r.id)
def test_v2(run):
    """LDS-DMA kernel, every tile instantiation with partial edge tiles, the
    linear and the decoding operand walk (splits of 1.5 steps run both in one
    launch), an empty split"""
    _run_random(run)


@pytest.mark.parametrize("run", G.V3_RUNS, ids=lambda r: r.id)
def test_v3(run):
    """halo kernel <64, 32>, <64, 16>, <128, 32>: 1, 2, 3, 4 and all tiles per
    split, an empty split; splits that start mid-column and cross the image
    seam"""
    _run_random(run)


@pytest.mark.parametrize("run", G.V3_REFUSED_RUNS, ids=lambda r: r.id)
def test_v3_refuses_16_wide_tiles_under_the_old_rules(run):
    """VU_TUNE_W3_SMALL = 0 with W = 16 or 48: vu_gemm_wgrad_tile answers
    generation 2, whose result meets the same bound"""
    _run_random(run)


def test_v3_split_off_the_tile_granule_runs_v2():
    """m_per_split % 128 != 0 on a v3-eligible problem: the tile query answers
    v3, the launch goes to v2 (the halo kernel would refuse the launch)"""
    _run_random(G.V3_OFF_GRANULE_RUN)


@pytest.mark.parametrize("run", G.XGEN_RUNS, ids=lambda r: r.id)
def test_same_problem_on_every_generation(run):
    """the same operands under VU_TUNE_GEN 1, 2, 3, each against the fp64 reference"""
    _run_random(run)


def test_launch_refuses_malformed_descriptors():
    """vu_gemm_wgrad's own argument checks: row grids that differ, a pixel
    stride or channel end off the 16-byte chunk, no source.  Nothing is
    launched: the slab keeps its sentinel."""
    K = _k()
    run = G.V1_RUNS[0]
    geo = run.geo
    slab, gslab = R.guarded((1, geo.ni, geo.nj), torch.float32, DEV)

    def rc(edit, dtype=G.BF16):
        w, gp, gq, _ = _problem(run, G.operands(geo, run.dtype))
        w.splits, w.m_per_split, w.out = 1, geo.M, slab.data_ptr()
        edit(w)
        return K.query("vu_gemm_wgrad", C.byref(w), dtype, K.stream())

    def grid(w):
        w.p.N += 1

    def stride(w):
        w.q.stride[0] += 4

    def cend(w):
        w.q.cend[0] -= 4

    def nsrc(w):
        w.q.nsrc = 0

    for edit in (grid, stride, cend, nsrc):
        assert rc(edit) != 0, edit.__name__
    torch.cuda.synchronize()
    assert bool((slab == R.SENTINEL).all())
    gslab.check("slabs")


# ----------------------------------------------------------------------------
# E. impulse operands: exact
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("run", G.IMPULSE_RUNS, ids=lambda r: r.id)
def test_impulses_are_returned_exactly(run):
    """impulse_P on every seam pixel (random Q), then impulse_Q (random P);
    one split, the finest split, and seams inside a tile row / mid-column"""
    n = {"P": 0, "Q": 0}
    with _tuning(run.tune):
        for mps, splits in run.plans:
            for side, px in G.impulse_sets(run, mps):
                _launch(run, G.impulse_operands(run.geo, run.dtype, side, px), mps, splits, exact=True)
                n[side] += 1
    print(f"{_head(run, 128)}, plans {list(run.plans)}: {n['P']} impulse_P + {n['Q']} impulse_Q launches, "
          "gradient and raw slabs exact")


# ----------------------------------------------------------------------------
# F. through kernels.gemm_wgrad: the production plan
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["contig", "cl"])
@pytest.mark.parametrize("geo,expect", G.PLAN_GEOS, ids=[str(g).replace(" ", "_") for g, _ in G.PLAN_GEOS])
def test_production_plan_accumulates(geo, expect, kind, monkeypatch):
    """accumulate = True on a pre-filled gradient in both parameter layouts;
    two identical calls bit-equal (fixed reduction order); the plan has
    ceil(M / m_per_split) splits of whole granules, none empty"""
    from vaeunet_amd import engine as E
    K = _k()
    run = G.Run(geo, G.BF16, (), expect, ())
    ni, nj, taps, cv, M = geo.ni, geo.nj, geo.taps, geo.cvalid, geo.M
    w, gp, gq, guards = _problem(run, G.operands(geo, G.BF16))
    gen = _assert_tile(w, run)
    old = torch.randn(geo.grad_shape, generator=torch.Generator().manual_seed(5))
    plans = []
    real = K.call

    def spy(name, *a):
        if name == "vu_gemm_wgrad":
            plans.append((a[0]._obj.splits, a[0]._obj.m_per_split))
        return real(name, *a)
    monkeypatch.setattr(K, "call", spy)
    res = []
    for rep in range(2):
        grad, guard, layout = G.grad_sink(geo.grad_shape, kind, DEV, old=old)
        assert layout == (E.convT_layout(grad) if geo.kind == "convT" else E.conv_layout(grad))
        before = guard.buf.clone()
        slab = K.gemm_wgrad(gp, gq, ni, nj, grad, layout, G.BF16, True, cvalid=cv)
        torch.cuda.synchronize()
        what = f"{kind} accumulate, {slab.shape[0]} splits of {plans[-1][1]}"
        for g in guards + [guard]:
            g.check(what)
        G.check_untouched(guard.buf, before, G.written_mask(guard.buf, grad, ni, taps, cv, layout), what)
        splits, mps = plans[-1]
        gran = 128 if gen == 3 else 64
        assert tuple(slab.shape) == (splits, ni, nj)
        assert mps % gran == 0 and splits == -(-M // mps) and (splits - 1) * mps < M, (splits, mps)
        ref, sabs = G.wgrad_ref(gp, gq, ni, nj)
        pick = lambda t: t.view(ni, taps, geo.C)[..., :cv]  # noqa: E731
        o = G.grad_view(G.same_view(before, grad), ni, taps, cv, layout)
        got = G.grad_view(grad, ni, taps, cv, layout)
        worst = G.check_bound(got, pick(ref) + o.double(), G.bound_random(M, pick(sabs), G.BF16, old=o), what)
        res.append(got.clone())
    assert torch.equal(res[0], res[1]), "two identical calls differ: the reduction order is not fixed"
    print(f"[plan] {_head(run)}: {worst}; two calls bit-equal")
