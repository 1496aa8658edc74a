"""The VAE bottleneck kernels of csrc/latent.hip -- vu_vae_heads_fwd,
vu_latent_fwd, vu_latent_bwd_sums, vu_latent_bwd and their queries -- each
called through the C ABI on guarded buffers and compared with the plain fp64
formulas of tests/ref_small.py.  Every stage's reference starts from the bytes
the kernel stored for the stage before (pooled, mu / logvar, y, coef, part, the
dz partials), so each stage is held to its own rounding.

Bounds (u = 2^-24, C_SUM = 1e-5, sabs = the reference on |operands|):

  pooled, mu, logvar, y, every gradient   u max(|ref|, |got|) + C_SUM sabs (+ u |old| when
                                          accumulating), per element
  z = mu + eps exp(lv / 2)                4 max(r_cpu, 1) u sabs + 2^-126 (r_cpu: the same formula
                                          in float32 on the CPU); eps == NULL: z is mu, bitwise
  coef, running statistics (train)        u max(|ref|, |got|) + 1e-10 sabs: the kernel works in double
  coef (eval)                             mean bitwise; invstd as above; scale one rounding from the
                                          kernel's invstd; shift u (|shift| + |mean scale|) from its scale
  activated vector                        one storage ulp + u (|y scale| + |shift|) (contracted or not)
  map                                     every pixel of a sample bitwise that vector; padding exactly 0
  part (integer gradients), counts,
  zero gradients, refusals                exact

The ReLU gate y scale + shift > 0 is decided in float32 by the kernel: inputs are
conditioned (ref_small.condition_consumer / condition_bn_input) so that no
(n, c) sits within 1e-3 of the edge, asserted here on the kernel's own y and coef.

Worst ratios measured on the MI355X (bound = 1; for z the CPU's float32 figure in brackets):
  heads     pooled 0.012, mu 0.0079, logvar 0.0078, z 1.58 (2.18) against 4 * 2.18
  forward   y 0.022; coef, running statistics and activations inside their bounds in every case
  backward  dw 0.127, dgamma 0.0084, dbeta 0.0086, dbias 0.0087, dz partials 0.0045,
            dw_mu 0.094, dw_lv 0.027, db_mu 0.014, db_lv 0.012, dpooled 0.011
  (C_SUM is an allowance for any summation order; these kernels' orders sit two decades inside it)
"""
import ctypes

import pytest
import torch

import ref_small as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32 = torch.float32
MODES = ["f32", "bf16"]
INVALID = 1            # hipErrorInvalidValue
MOM, EPS = R.LAT_MOM, R.LAT_EPS


def _lib():
    from vaeunet_amd import _lib as L
    return L


def _dt(mode):
    return torch.bfloat16 if mode == "bf16" else torch.float32


def _code(mode):
    return _lib().BF16 if mode == "bf16" else _lib().F32


def _ulp(mode):
    return 2.0 ** -8 if mode == "bf16" else 2.0 ** -23     # one ulp, relative


def _put(x, dtype=None):
    """CPU tensor -> guarded contiguous device tensor holding it"""
    t, g = R.guarded(tuple(x.shape), dtype or x.dtype, DEV)
    t.copy_(x)
    return t, g


def _dev(x):
    return None if x is None else x.to(DEV)


def _p(t):
    return None if t is None else t.data_ptr()


def _check(guards, what):
    for g in guards:
        g.check(what)


def _tight(got, ref, sabs, what):
    """a value the kernel forms in double and rounds once"""
    g, r = got.double().cpu(), ref.double()
    bound = R.U32 * torch.maximum(g.abs(), r.abs()) + 1e-10 * sabs.double()
    assert bool(((g - r).abs() <= bound).all()), f"{what}: worst {float(((g - r).abs() / (bound + 1e-300)).max()):.3g}"


def _rows(x, mode, strided):
    """[P, C] CPU values -> device rows in the storage dtype, dense or as
    channels [C, 2C) of rows twice as wide.  -> tensor, guard, row stride"""
    P, C = x.shape
    t, g = R.guarded_rows(P, C, _dt(mode), DEV, wide=2 * C if strided else None, c0=C if strided else 0)
    t.copy_(x.to(_dt(mode)))
    return t, g, (2 * C if strided else C)


# ----------------------------------------------------------------------------
# vu_vae_heads_fwd
# ----------------------------------------------------------------------------
def _heads_call(fd, fs, N, HW, C, w_mu, b_mu, w_lv, b_lv, L, eps, outs, mode):
    Lb = _lib()
    rc = Lb.query("vu_vae_heads_fwd", Lb.ptr(fd), fs, N, HW, C, Lb.ptr(w_mu), Lb.ptr(b_mu), Lb.ptr(w_lv), Lb.ptr(b_lv),
                  L, Lb.ptr(eps), *[Lb.ptr(o) for o in outs], _code(mode), Lb.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("case", R.HEADS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_heads_fwd(case, strided, mode):
    N, HW, C, L = case
    f, w_mu, b_mu, w_lv, b_lv, eps = R.heads_inputs(N, HW, C, L, _dt(mode))
    fd, gf, fs = _rows(f.reshape(N * HW, C), mode, strided)
    dw_mu, dw_lv = _dev(w_mu), _dev(w_lv)
    worst = {}
    for with_eps, with_bias in ((True, True), (False, True), (True, False)):
        what = f"heads {case} eps={with_eps} bias={with_bias}"
        bm, bl = (b_mu, b_lv) if with_bias else (None, None)
        e = eps if with_eps else None
        pooled, gp = R.guarded((N, C), F32, DEV)
        mu, gm = R.guarded((N, L), F32, DEV)
        lv, gl = R.guarded((N, L), F32, DEV)
        z, gz = R.guarded((N, L), F32, DEV)
        assert _heads_call(fd, fs, N, HW, C, dw_mu, _dev(bm), dw_lv, _dev(bl), L, _dev(e), (pooled, mu, lv, z), mode) == 0
        _check((gf, gp, gm, gl, gz), what)
        assert torch.equal(fd.float().cpu(), f.reshape(N * HW, C))
        ref, sabs = R.pooled_ref(f)
        worst["pooled"] = max(worst.get("pooled", 0), R.assert_lin(pooled, ref, sabs, what + " pooled"))
        pk = pooled.cpu()
        for name, got, w, b in (("mu", mu, w_mu, bm), ("logvar", lv, w_lv, bl)):
            ref, sabs = R.linear_fwd_ref(pk, w, b)
            worst[name] = max(worst.get(name, 0), R.assert_lin(got, ref, sabs, f"{what} {name}"))
        mk, lk = mu.cpu(), lv.cpu()
        if e is None:
            assert torch.equal(z.cpu().view(torch.int32), mk.view(torch.int32)), what + ": z must be mu"
        else:
            ref64, mag = R.reparam_fwd_ref(mk, lk, e)
            ref32 = mk + e * torch.exp(0.5 * lk)
            R.assert_trans(z.cpu(), ref64, ref32, mag, what + " z")
    print(f"heads {case} {mode}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("bad", ["C=24", "C=4096", "fs=C+4", "L=0", "N=0"])
def test_heads_fwd_refusals(bad):
    N, HW, C, L = 2, 3, 64, 4
    fs = None
    if bad == "C=24":
        C = 24
    elif bad == "C=4096":
        C = 4096
    elif bad == "fs=C+4":
        fs = C + 4
    f = torch.ones(N * HW, (fs or C))
    fd, gf = _put(f)
    w = _dev(torch.ones(max(L, 1), C))
    eps = _dev(torch.ones(N, max(L, 1)))
    outs = [R.guarded((N, C), F32, DEV)] + [R.guarded((N, 4), F32, DEV) for _ in range(3)]
    rc = _heads_call(fd, fs or C, 0 if bad == "N=0" else N, HW, C, w, None, w, None, 0 if bad == "L=0" else L, eps,
                     [o for o, _ in outs], "f32")
    assert rc == (0 if bad == "N=0" else INVALID)
    _check([g for _, g in outs] + [gf], bad)
    for o, _ in outs:
        assert bool((o == R.SENTINEL).all()), bad


# ----------------------------------------------------------------------------
# vu_latent_fwd
# ----------------------------------------------------------------------------
class FwdJob:
    """one consumer's device state for vu_latent_fwd, its CPU inputs beside it"""

    def __init__(self, N, L, geo, mode, train, strided, bias, track, form, idx=0):
        co, cpad, HW = geo
        self.N, self.L, self.co, self.cpad, self.HW, self.mode, self.train = N, L, co, cpad, HW, mode, train
        self.form, self.track = form, track
        self.z, (self.w, self.b, self.gamma, self.beta, self.rm, self.rv) = R.fwd_job_inputs(N, L, co, HW, train, bias, idx)
        self.keep = [_dev(t) for t in (self.w, self.b, self.gamma, self.beta)]
        self.guards = []
        dt = _dt(mode)

        def out(shape, dtype, fill=None):
            t, g = R.guarded(shape, dtype, DEV)
            if fill is not None:
                t.copy_(fill)
            self.guards.append(g)
            return t
        self.y, self.coef = out((N, co), F32), out((4, co), F32)
        self.drm = out(co, F32, self.rm) if track else None
        self.drv = out(co, F32, self.rv) if track else None
        self.nbt = out(1, torch.int64, torch.tensor([7])) if track else None
        self.act = out((N, co), F32) if form in ("act", "both") else None     # float* whatever the storage dtype
        self.map, self.stride = None, 0
        if form in ("map", "both"):
            wide = cpad + 16 if strided else None
            m, g = R.guarded_rows(N * HW, cpad, dt, DEV, wide=wide, c0=8 if strided else 0)
            self.guards.append(g)
            self.map, self.stride = m, (wide or cpad)

    def job(self):
        j = _lib().VuLatentJob()
        w, b, gamma, beta = self.keep
        j.w, j.bias, j.gamma, j.beta = _p(w), _p(b), _p(gamma), _p(beta)
        j.running_mean, j.running_var, j.num_batches_tracked = _p(self.drm), _p(self.drv), _p(self.nbt)
        j.momentum, j.eps, j.train = MOM, EPS, int(self.train)
        j.co, j.cpad, j.HW = self.co, self.cpad, self.HW
        j.out, j.out_stride = _p(self.map), self.stride
        j.act, j.y, j.coef = _p(self.act), _p(self.y), _p(self.coef)
        return j

    def check(self, what, launches=1, worst=None):
        N, co, cpad, HW = self.N, self.co, self.cpad, self.HW
        _check(self.guards, what)
        worst = {} if worst is None else worst
        yk, ck = self.y.cpu(), self.coef.cpu()
        ref, sabs = R.linear_fwd_ref(self.z, self.w, self.b)
        worst["y"] = max(worst.get("y", 0), R.assert_lin(yk, ref, sabs, what + " y"))
        bn = R.latent_bn_ref(yk, self.gamma, self.beta, self.rm, self.rv, MOM, EPS, self.train, HW)
        scale, shift, mean, invstd = ck
        if self.train:
            _tight(scale, bn["scale"], bn["scale"].abs(), what + " scale")
            _tight(shift, bn["shift"], bn["shift_abs"], what + " shift")
            _tight(mean, bn["mean"], yk.double().abs().mean(0), what + " mean")
            _tight(invstd, bn["invstd"], bn["invstd"], what + " invstd")
        else:
            assert torch.equal(mean, self.rm), what + " mean"
            _tight(invstd, bn["invstd"], bn["invstd"], what + " invstd")
            _tight(scale, self.gamma.double() * invstd.double(), torch.zeros(co), what + " scale")
            sref = self.beta.double() - mean.double() * scale.double()
            assert bool(((shift.double() - sref).abs() <= R.U32 * (sref.abs() + (mean.double() * scale.double()).abs())
                         ).all()), what + " shift"
        assert int(R.gate_near_zero(yk, scale, shift).sum()) == 0, what + ": a gate within the margin of its edge"
        if self.track:
            if self.train and launches == 1:
                _tight(self.drm, bn["rm"], bn["rm_abs"], what + " running_mean")
                _tight(self.drv, bn["rv"], bn["rv_abs"], what + " running_var")
            if not self.train:
                assert torch.equal(self.drm.cpu(), self.rm) and torch.equal(self.drv.cpu(), self.rv), what
            assert int(self.nbt) == 7 + (launches if self.train else 0), what + " num_batches_tracked"
        a64, amag = R.latent_act_ref(yk, scale, shift)
        vec = None
        if self.map is not None:
            m = self.map.cpu().float().reshape(N, HW, cpad)
            assert torch.equal(m, m[:, :1].expand(N, HW, cpad)), what + ": pixels of a sample differ"
            assert not m[:, :, co:].any(), what + ": channel padding"
            assert (torch.signbit(m[:, :, co:]) == 0).all(), what + ": channel padding"
            vec = m[:, 0, :co]
        if self.act is not None:
            ak = self.act.cpu()
            assert torch.equal(ak.to(_dt(self.mode)).float(), ak), what + ": act not rounded to the storage dtype"
            if vec is not None:
                assert torch.equal(vec, ak), what + ": map vs act"
            vec = ak
        bound = _ulp(self.mode) * torch.maximum(a64.abs(), vec.double().abs()) + R.U32 * amag
        err = (vec.double() - a64).abs()
        assert bool((err <= bound).all()), what + f": activation, worst {float((err / (bound + 1e-300)).max()):.3g}"
        assert bool((vec >= 0).all())
        return worst


def _fwd_launch(jobs, N, L, mode, z):
    Lb = _lib()
    arr = (Lb.VuLatentJob * len(jobs))(*[j.job() if isinstance(j, FwdJob) else j for j in jobs])
    zd = _dev(z)
    rc = Lb.query("vu_latent_fwd", arr, len(jobs), Lb.ptr(zd), N, L, _code(mode), Lb.stream())
    torch.cuda.synchronize()
    return rc


# form, strided map, bias, running statistics, train
FWD_VARIANTS = [("map", False, True, True, True), ("both", True, False, True, True), ("map", True, True, False, True),
                ("act", False, True, True, True), ("both", False, True, True, False), ("map", True, False, True, False)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", FWD_VARIANTS, ids=lambda v: f"{v[0]}-{'slice' if v[1] else 'dense'}-"
                         f"{'bias' if v[2] else 'nobias'}-{'track' if v[3] else 'notrack'}-{'train' if v[4] else 'eval'}")
@pytest.mark.parametrize("case", R.LAT_FWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_latent_fwd(case, variant, mode):
    N, L, co, cpad, HW = case
    form, strided, bias, track, train = variant
    if form == "act" and cpad != co:
        form = "both"          # the shortcut form has no padding: run both outputs instead
    J = FwdJob(N, L, (co, cpad, HW), mode, train, strided, bias, track, form)
    assert _fwd_launch([J], N, L, mode, J.z) == 0
    w = J.check(f"fwd {case} {variant} {mode}")
    print(f"fwd {case} {variant} {mode}: y {w['y']:.3g}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("table", R.LAT_FWD_TABLES, ids=lambda t: f"{len(t[2])}jobs")
def test_latent_fwd_tables(table, train, mode):
    """3 and 8 consumers of mixed geometry in one launch (the by-value table);
    a second train launch counts a second batch"""
    N, L, geos = table
    forms = ["map", "both", "act"]
    jobs = []
    for i, geo in enumerate(geos):
        form = forms[i % 3] if geo[0] == geo[1] else forms[i % 2]
        jobs.append(FwdJob(N, L, geo, mode, train, strided=bool(i % 2), bias=bool((i + 1) % 3), track=True, form=form,
                           idx=i))
    assert _fwd_launch(jobs, N, L, mode, jobs[0].z) == 0
    for i, J in enumerate(jobs):
        J.check(f"table job {i} {geos[i]} {mode}")
    assert _fwd_launch(jobs, N, L, mode, jobs[0].z) == 0
    for i, J in enumerate(jobs):
        J.check(f"table job {i} second launch", launches=2)


def test_latent_fwd_refusals_and_queries():
    Lb = _lib()
    N, L = 2, 4

    def fresh(form="both", geo=(8, 16, 3)):
        return FwdJob(N, L, geo, "f32", True, False, True, True, form)

    def refused(J, j, n=N, l=L, njobs=1):
        arr = (Lb.VuLatentJob * max(njobs, 1))(*([j] * max(njobs, 1)))
        rc = Lb.query("vu_latent_fwd", arr, njobs, Lb.ptr(_dev(J.z)), n, l, Lb.F32, Lb.stream())
        torch.cuda.synchronize()
        assert rc == INVALID
        _check(J.guards, "refusal")
        for t in (J.y, J.coef, J.act, J.map):
            assert t is None or bool((t == R.SENTINEL).all())
        assert torch.equal(J.drm.cpu(), J.rm) and int(J.nbt) == 7

    for n, l in ((0, L), (65, L), (N, 65), (N, 0)):
        J = fresh()
        refused(J, J.job(), n, l)
    for field, value in (("co", 24), ("co", 0), ("cpad", 4), ("cpad", 12), ("out_stride", 20), ("HW", 0)):
        J = fresh(geo=(8, 16, 3) if field != "cpad" or value != 4 else (8, 8, 3))
        j = J.job()
        setattr(j, field, value)
        refused(J, j)
    J = fresh("map", (8, 8, 3))      # out == NULL without act
    j = J.job()
    j.out = None
    refused(J, j)
    J = fresh("both", (8, 16, 3))    # out == NULL with cpad != co
    j = J.job()
    j.out = None
    refused(J, j)
    J = fresh()
    refused(J, J.job(), njobs=9)
    refused(J, J.job(), njobs=0)
    # the documented formulas
    pow2 = lambda v: v & (v - 1) == 0
    for co in (0, 8, 16, 24, 64, 2048, 4096):
        for cpad in (8, 12, 64, 2048, 4096):
            for stride in (cpad, cpad + 4, cpad + 8):
                ok = co >= 1 and cpad >= co and cpad % 8 == 0 and stride % 8 == 0 and co % 8 == 0 and pow2(co // 8) \
                    and co // 8 <= 256
                assert Lb.query("vu_latent_check_job", co, cpad, stride, Lb.F32) == (0 if ok else INVALID), (co, cpad)
    for n, hw, cpad in ((1, 1, 8), (3, 600, 64), (64, 70, 136), (3, 1024, 128), (3, 1025, 32), (1, 1, 2048)):
        want = -(-cpad // R.LAT_CG) * -(-(n * hw) // R.LAT_PCH)
        assert Lb.query("vu_latent_fwd_blocks", n, hw, cpad) == want
    assert Lb.query("vu_latent_part_floats", 3, 32) == 3 * R.LAT_SPLITS * 32


# ----------------------------------------------------------------------------
# vu_latent_bwd_sums
# ----------------------------------------------------------------------------
def _sums_job(N, co, HW, mode, strided, seed):
    g = torch.Generator().manual_seed(seed)
    dmap = torch.randint(-4, 5, (N, HW, co), generator=g).float()
    dd, gd, stride = _rows(dmap.reshape(N * HW, co), mode, strided)
    part, gp = R.guarded((N, R.LAT_SPLITS, co), F32, DEV)
    j = _lib().VuLatentJob()
    j.co, j.cpad, j.HW, j.out, j.out_stride = co, co, HW, _p(dd), stride
    j.dmap, j.dmap_stride, j.part = _p(dd), stride, _p(part)
    return j, dmap, dd, part, (gd, gp)


def _sums_launch(jobs, N, mode):
    Lb = _lib()
    arr = (Lb.VuLatentJob * len(jobs))(*jobs)
    rc = Lb.query("vu_latent_bwd_sums", arr, len(jobs), N, _code(mode), Lb.stream())
    torch.cuda.synchronize()
    return rc


def _sums_check(dmap, part, guards, what):
    _check(guards, what)
    N, HW, co = dmap.shape
    ref = R.latent_sums_ref(dmap)
    assert torch.equal(part.cpu().double(), ref), what
    per = -(-HW // R.LAT_SPLITS)
    first_empty = -(-HW // per)
    assert not part[:, first_empty:].any(), what + ": splits past the end"
    assert torch.equal(part.cpu().double().sum(1), dmap.double().sum(1)), what


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("case", R.LAT_SUMS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_latent_bwd_sums(case, strided, mode):
    """integer gradients in [-4, 4]: every partial sum is exact in both dtypes"""
    N, co, HW = case
    j, dmap, dd, part, guards = _sums_job(N, co, HW, mode, strided, 51 + co + HW)
    assert _sums_launch([j], N, mode) == 0
    _sums_check(dmap, part, guards, f"sums {case}")
    assert torch.equal(dd.float().cpu(), dmap.reshape(N * HW, co))


@pytest.mark.parametrize("mode", MODES)
def test_latent_bwd_sums_two_jobs_and_refusals(mode):
    N = 3
    a = _sums_job(N, 32, 33, mode, True, 61)
    b = _sums_job(N, 8, 600, mode, False, 62)
    assert _sums_launch([a[0], b[0]], N, mode) == 0
    _sums_check(a[1], a[3], a[4], "two jobs, first")
    _sums_check(b[1], b[3], b[4], "two jobs, second")
    for field, value in (("dmap", None), ("part", None), ("dmap_stride", 36)):
        c = _sums_job(N, 32, 33, mode, False, 63)
        setattr(c[0], field, value)
        assert _sums_launch([c[0]], N, mode) == INVALID
        _check(c[4], "sums refusal")
        assert bool((c[3] == R.SENTINEL).all())
    c = _sums_job(N, 32, 33, mode, False, 63)
    assert _sums_launch([c[0]], 0, mode) == INVALID and _sums_launch([c[0]], 65, mode) == INVALID
    assert bool((c[3] == R.SENTINEL).all())


# ----------------------------------------------------------------------------
# vu_latent_bwd
# ----------------------------------------------------------------------------
J_OUT = ("dw", "dbias", "dgamma", "dbeta")
H_OUT = ("dw_mu", "dw_lv", "db_mu", "db_lv")


def _blocks(co):
    return -(-co // 32)


class Bwd:
    """inputs of one vu_latent_bwd launch given directly (part, y, coef, z) and
    its guarded outputs, pre-filled (gradients are accumulated into)"""

    def __init__(self, N, L, cos, C, train, acc, integer=False, null=(), heads_null=(), seed=0):
        self.N, self.L, self.cos, self.C, self.train, self.acc = N, L, cos, C, train, acc
        self.null = set(null)
        g = torch.Generator().manual_seed(70 + seed)
        self.z = R.latent_z(N, L)
        self.cons = [R.bwd_consumer_inputs(N, L, co, train, integer, seed=34 + 13 * i) for i, co in enumerate(cos)]
        self.h = R.heads_bwd_inputs(N, L, C)
        if integer:
            for k in ("dz_in", "dmu_in", "dlv_in"):
                self.h[k] = torch.randint(-4, 5, (N, L), generator=g).float()
        for k in heads_null:
            self.h[k] = None
        if self.h["eps"] is None:
            self.h["logvar"] = None
        self.guards, self.pre, self.out = [], {}, {}

        def out(name, shape):
            pre = torch.randint(-3, 4, shape, generator=g).float() if integer else torch.randn(shape, generator=g)
            t, gd = R.guarded(shape, F32, DEV)
            t.copy_(pre)
            self.guards.append(gd)
            self.pre[name], self.out[name] = pre, t
            return t
        self.dev = []     # device inputs kept alive
        self.jobs = []
        Lb = _lib()
        for i, (co, (part, y, coef, gamma, w)) in enumerate(zip(cos, self.cons)):
            d = [_dev(t) for t in (part, y, coef, gamma, w)]
            self.dev.append(d)
            j = Lb.VuLatentJob()
            j.part, j.y, j.coef, j.gamma, j.w = (_p(t) for t in d)
            j.act = _p(d[1])     # the table check wants a forward output; the backward never reads it
            j.co, j.cpad, j.HW, j.out_stride, j.train, j.grad_acc = co, co, 1, co, int(train), acc
            for name, shape in (("dw", (co, L)), ("dbias", (co,)), ("dgamma", (co,)), ("dbeta", (co,))):
                t = out(f"{name}{i}", shape)
                setattr(j, name, None if name in self.null else _p(t))
            self.jobs.append(j)
        hb = Lb.VuLatentHeads()
        self.hdev = {k: _dev(v) for k, v in self.h.items()}
        self.zd = _dev(self.z)
        hb.z = _p(self.zd)
        for k in ("eps", "logvar", "dmu_in", "dlv_in", "dz_in", "pooled", "w_mu", "w_lv"):
            setattr(hb, k, _p(self.hdev[k]))
        for name, shape in (("dw_mu", (L, C)), ("dw_lv", (L, C)), ("db_mu", (L,)), ("db_lv", (L,)), ("dpooled", (N, C))):
            t = out(name, shape)
            setattr(hb, name, None if name in self.null else _p(t))
        hb.C, hb.grad_acc = C, acc
        self.hb = hb
        self.nbp = sum(_blocks(co) for co in cos)
        nws = Lb.query("vu_latent_bwd_workspace_bytes", N, L, sum(cos)) // 4
        assert nws >= self.nbp * N * L
        self.ws, gw = R.guarded(max(nws, 1), F32, DEV)
        self.guards.append(gw)

    def launch(self, njobs=None, ws=True, hb=None):
        Lb = _lib()
        n = len(self.jobs) if njobs is None else njobs
        arr = (Lb.VuLatentJob * max(len(self.jobs), 1))(*self.jobs) if self.jobs else None
        rc = Lb.query("vu_latent_bwd", arr, n, ctypes.byref(hb or self.hb), self.N, self.L,
                      Lb.ptr(self.ws) if ws else None, Lb.stream())
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return all(torch.equal(self.out[k].cpu(), self.pre[k]) for k in self.out) and bool((self.ws == R.SENTINEL).all())

    def check(self, what, worst=None):
        """every output against the references; -> worst ratio per quantity"""
        N, L, acc = self.N, self.L, self.acc
        worst = {} if worst is None else worst
        _check(self.guards, what)

        def cmp(name, ref, sabs, key):
            if name.rstrip("0123456789") in self.null:
                assert torch.equal(self.out[name].cpu(), self.pre[name]), f"{what}: {name} is NULL"
                return
            pre = self.pre[name] if acc and name != "dpooled" else None
            r = R.assert_lin(self.out[name], ref + (pre.double() if pre is not None else 0), sabs, f"{what} {name}", acc=pre)
            worst[key] = max(worst.get(key, 0.0), r)

        wsk = self.ws.cpu()[:self.nbp * N * L].reshape(self.nbp, N, L) if self.nbp else torch.zeros(0, N, L)
        b0 = 0
        for i, (co, (part, y, coef, gamma, w)) in enumerate(zip(self.cos, self.cons)):
            assert int(R.gate_near_zero(y, coef[0], coef[1]).sum()) == 0
            val, mag = R.latent_bwd_consumer_ref(part, y, coef, self.z, w, gamma, self.train)
            for name in ("dw", "dgamma", "dbeta"):
                cmp(f"{name}{i}", val[name], mag[name], name)
            if self.train:      # exactly old + 0
                if "dbias" not in self.null:
                    want = self.pre[f"dbias{i}"] if acc else torch.zeros(co)
                    assert torch.equal(self.out[f"dbias{i}"].cpu(), want), f"{what}: dbias{i} must be old + 0"
            else:
                cmp(f"dbias{i}", val["dbias"], mag["dbias"], "dbias")
            for b in range(_blocks(co)):
                c0, c1 = 32 * b, min(co, 32 * b + 32)
                ref, sabs = val["v"][:, c0:c1] @ w[c0:c1].double(), mag["v"][:, c0:c1] @ w[c0:c1].double().abs()
                r = R.assert_lin(wsk[b0 + b], ref, sabs, f"{what}: dz partial of job {i} block {b}")
                worst["dz"] = max(worst.get("dz", 0.0), r)
            b0 += _blocks(co)
            if self.train and N == 1:
                assert torch.equal(y, coef[2].reshape(1, co))       # one sample: y is the batch mean
                for name in ("dw", "dgamma"):
                    if name not in self.null:
                        want = self.pre[f"{name}{i}"] if acc else torch.zeros_like(self.pre[f"{name}{i}"])
                        assert torch.equal(self.out[f"{name}{i}"].cpu(), want), f"{what}: {name}{i} at N = 1"
        if self.train and N == 1:
            assert not wsk.any(), what + ": dz partials at N = 1"
        # the heads from the kernel's own partials
        h = self.h
        dz = (h["dz_in"].double() if h["dz_in"] is not None else torch.zeros(N, L, dtype=torch.float64)) + wsk.double().sum(0)
        dz_abs = (h["dz_in"].double().abs() if h["dz_in"] is not None else 0) + wsk.double().abs().sum(0)
        val, mag = R.latent_bwd_heads_ref(dz, dz_abs, h["dmu_in"], h["dlv_in"], h["eps"], h["logvar"], h["pooled"],
                                          h["w_mu"], h["w_lv"])
        for name in H_OUT + ("dpooled",):
            cmp(name, val[name], mag[name], name)
        return worst


@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", R.LAT_BWD_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{'-'.join(map(str, c[2]))}x{c[3]}")
def test_latent_bwd(case, train, acc):
    N, L, cos, C = case
    B = Bwd(N, L, cos, C, train, acc)
    assert _lib().query("vu_latent_bwd_supported", N, L, sum(cos), C) == 1
    assert B.launch() == 0
    w = B.check(f"bwd {case} train={train} acc={acc}")
    print(f"bwd {case} train={train} acc={acc}: " + ", ".join(f"{k} {v:.3g}" for k, v in w.items()))


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_latent_bwd_integer_sums(train):
    """integer split sums and incoming gradients: the beta, bias and head-bias
    gradients are exact sums (eval: gamma invstd is made a power of two)"""
    N, L, co, C = 9, 5, 32, 8
    for acc in (0, 1):
        B = Bwd(N, L, [co], C, train, acc, integer=True, heads_null=("eps",))
        part, y, coef, gamma, w = B.cons[0]
        if not train:
            gamma = torch.where(gamma < 0, -2.0, 2.0)
            coef[3] = 1.0
            coef[0] = gamma
            y = R.condition_bn_input(y, coef[0], coef[1], F32)
            B.cons[0] = (part, y, coef, gamma, w)
            for t, src in zip(B.dev[0], B.cons[0]):
                t.copy_(src)
        assert B.launch() == 0
        B.check(f"integer train={train} acc={acc}")
        keep = (y.double() * coef[0].double() + coef[1].double()) > 0
        G = part.double().sum(1) * keep
        old = lambda k: B.pre[k].double() if acc else 0
        assert torch.equal(B.out["dbeta0"].cpu().double(), G.sum(0) + old("dbeta0"))
        if not train:
            assert torch.equal(B.out["dbias0"].cpu().double(), (gamma.double() * G).sum(0) + old("dbias0"))
        # eps == NULL: dlv = dlv_in; the workspace partials are whatever they are, dmu = dmu_in + dz
        assert torch.equal(B.out["db_lv"].cpu().double(), B.h["dlv_in"].double().sum(0) + old("db_lv"))
    # the heads alone (njobs = 0): db_mu = sum (dmu_in + dz_in), exact
    for acc in (0, 1):
        B = Bwd(N, L, [], C, train, acc, integer=True, heads_null=("eps",))
        assert B.launch(njobs=0) == 0
        B.check(f"heads only acc={acc}")
        old = B.pre["db_mu"].double() if acc else 0
        assert torch.equal(B.out["db_mu"].cpu().double(), (B.h["dmu_in"] + B.h["dz_in"]).double().sum(0) + old)
        assert bool((B.ws == R.SENTINEL).all())


@pytest.mark.parametrize("name", J_OUT + H_OUT)
def test_latent_bwd_null_outputs(name):
    """each gradient output NULL in turn: the others keep their bits"""
    N, L, cos, C = 3, 5, [32, 8], 24
    for train in (True, False):
        full = Bwd(N, L, cos, C, train, 1)
        assert full.launch() == 0
        B = Bwd(N, L, cos, C, train, 1, null=(name,))
        assert B.launch() == 0
        B.check(f"NULL {name} train={train}")
        for k in B.out:
            if k.rstrip("0123456789") != name:
                assert torch.equal(B.out[k].cpu(), full.out[k].cpu()), f"{k} changed when {name} is NULL"


@pytest.mark.parametrize("nulls", [("eps",), ("dmu_in",), ("dlv_in",), ("dz_in",), ("dmu_in", "dlv_in", "dz_in"),
                                   ("eps", "dz_in")], ids=lambda n: "+".join(n))
def test_latent_bwd_null_inputs(nulls):
    for acc in (0, 1):
        B = Bwd(9, 5, [64, 8], 24, True, acc, heads_null=nulls)
        assert B.launch() == 0
        B.check(f"NULL inputs {nulls} acc={acc}")
        if "eps" in nulls and "dlv_in" not in nulls:
            # z = mu: nothing flows into logvar but its own incoming gradient
            Bz = Bwd(9, 5, [64, 8], 24, True, acc, heads_null=tuple(nulls) + ("dz_in",))
            assert Bz.launch() == 0
            assert torch.equal(B.out["db_lv"].cpu(), Bz.out["db_lv"].cpu())


def test_latent_bwd_refusals_and_queries():
    Lb = _lib()
    N, L, cos, C = 3, 5, [32, 8], 24
    B = Bwd(N, L, cos, C, True, 0)
    assert B.launch(ws=False) == INVALID and B.untouched()
    assert B.launch(njobs=-1) == INVALID and B.untouched()
    assert B.launch(njobs=9) == INVALID and B.untouched()
    for bad_c in (4, 12, 0):
        hb = Lb.VuLatentHeads.from_buffer_copy(B.hb)
        hb.C = bad_c
        assert B.launch(hb=hb) == INVALID and B.untouched()
    Lb2 = Lb.query
    for n, l, sco, c, ok in ((1, 1, 0, 8, 1), (64, 64, 4096, 2048, 1), (0, 5, 8, 8, 0), (65, 5, 8, 8, 0), (3, 0, 8, 8, 0),
                             (3, 65, 8, 8, 0), (3, 5, -1, 8, 0), (3, 5, 8, 4, 0), (3, 5, 8, 12, 0), (3, 5, 8, 24, 1)):
        assert Lb2("vu_latent_bwd_supported", n, l, sco, c) == ok, (n, l, sco, c)
    for cos_ in ([8], [8] * 8, [32, 64, 8], [2048], [512, 8, 8, 16]):
        nbp = sum(_blocks(co) for co in cos_)
        for n, l in ((1, 1), (3, 5), (64, 64)):
            assert Lb2("vu_latent_bwd_workspace_bytes", n, l, sum(cos_)) >= nbp * n * l * 4


# ----------------------------------------------------------------------------
# the chain, and repeatability
# ----------------------------------------------------------------------------
def _chain(mode, seed=0):
    """heads -> consumers -> split sums -> backward, each launch on the
    previous one's device buffers.  -> everything needed to check it"""
    Lb = _lib()
    N, HW4, C, L = 3, 9, 64, 5
    geos = [(32, 64, 70), (8, 8, 33)]
    f, w_mu, b_mu, w_lv, b_lv, eps = R.heads_inputs(N, HW4, C, L, _dt(mode), seed=91)
    fd, gf, fs = _rows(f.reshape(N * HW4, C), mode, False)
    dw_mu, db_mu, dw_lv, db_lv, deps = (_dev(t) for t in (w_mu, b_mu, w_lv, b_lv, eps))
    pooled, gp = R.guarded((N, C), F32, DEV)
    mu, gm = R.guarded((N, L), F32, DEV)
    lv, gl = R.guarded((N, L), F32, DEV)
    z, gz = R.guarded((N, L), F32, DEV)
    assert _heads_call(fd, fs, N, HW4, C, dw_mu, db_mu, dw_lv, db_lv, L, deps, (pooled, mu, lv, z), mode) == 0
    zk = z.cpu()
    # consumers: parameters conditioned against the z the device produced
    jobs = []
    for i, geo in enumerate(geos):
        J = FwdJob(N, L, geo, mode, True, bool(i), True, True, "both", idx=20 + i)
        J.z = zk
        J.beta = R.condition_consumer(zk, J.w, J.b, J.gamma, J.beta, J.rm, J.rv, MOM, EPS, True, geo[2])
        J.keep[3] = _dev(J.beta)
        jobs.append(J)
    arr = (Lb.VuLatentJob * len(jobs))(*[J.job() for J in jobs])
    assert Lb.query("vu_latent_fwd", arr, len(jobs), Lb.ptr(z), N, L, _code(mode), Lb.stream()) == 0
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(92)
    outs, keep, dmaps = {}, [], []
    guards = [gf, gp, gm, gl, gz]
    for i, (J, (co, cpad, HW)) in enumerate(zip(jobs, geos)):
        dmap = (torch.randn(N, HW, co, generator=g) / HW).to(_dt(mode)).float()
        dd, gd, stride = _rows(dmap.reshape(N * HW, co), mode, bool(i))
        part, gpt = R.guarded((N, R.LAT_SPLITS, co), F32, DEV)
        arr[i].dmap, arr[i].dmap_stride, arr[i].part, arr[i].grad_acc = _p(dd), stride, _p(part), 0
        for name, shape in (("dw", (co, L)), ("dbias", (co,)), ("dgamma", (co,)), ("dbeta", (co,))):
            t, gg = R.guarded(shape, F32, DEV)
            setattr(arr[i], name, _p(t))
            outs[f"{name}{i}"] = t
            guards.append(gg)
        keep += [dd, part]
        dmaps.append(dmap)
        guards += [gd, gpt] + J.guards
        outs[f"part{i}"] = part
    assert Lb.query("vu_latent_bwd_sums", arr, len(jobs), N, _code(mode), Lb.stream()) == 0
    hin = R.heads_bwd_inputs(N, L, C, seed=93)
    hdev = {k: _dev(hin[k]) for k in ("dmu_in", "dlv_in", "dz_in")}
    hb = Lb.VuLatentHeads()
    hb.z, hb.eps, hb.logvar, hb.pooled, hb.w_mu, hb.w_lv = _p(z), _p(deps), _p(lv), _p(pooled), _p(dw_mu), _p(dw_lv)
    hb.dmu_in, hb.dlv_in, hb.dz_in = _p(hdev["dmu_in"]), _p(hdev["dlv_in"]), _p(hdev["dz_in"])
    for name, shape in (("dw_mu", (L, C)), ("dw_lv", (L, C)), ("db_mu", (L,)), ("db_lv", (L,)), ("dpooled", (N, C))):
        t, gg = R.guarded(shape, F32, DEV)
        setattr(hb, name, _p(t))
        outs[name] = t
        guards.append(gg)
    hb.C, hb.grad_acc = C, 0
    ws, gw = R.guarded(Lb.query("vu_latent_bwd_workspace_bytes", N, L, sum(g_[0] for g_ in geos)) // 4, F32, DEV)
    guards.append(gw)
    assert Lb.query("vu_latent_bwd", arr, len(jobs), ctypes.byref(hb), N, L, Lb.ptr(ws), Lb.stream()) == 0
    torch.cuda.synchronize()
    _check(guards, "chain")
    outs.update(pooled=pooled, mu=mu, logvar=lv, z=z, ws=ws)
    for i, J in enumerate(jobs):
        outs.update({f"y{i}": J.y, f"coef{i}": J.coef, f"map{i}": J.map, f"act{i}": J.act, f"rm{i}": J.drm,
                     f"rv{i}": J.drv})
    inputs = dict(f=f, w_mu=w_mu, b_mu=b_mu, w_lv=w_lv, b_lv=b_lv, eps=eps, jobs=jobs, dmaps=dmaps, hin=hin, geos=geos,
                  dims=(N, HW4, C, L))
    return inputs, {k: v.cpu().contiguous().clone() for k, v in outs.items()}, keep


@pytest.mark.parametrize("mode", MODES)
def test_chain(mode):
    """End to end against fp64 autograd-free formulas from the ORIGINAL inputs:
    every gradient within u max + 4 C_SUM sabs, the sum of the four stage
    bounds (heads, consumers, split sums, backward: each perturbs a gradient
    term by at most C_SUM of that term's |operand| form), with sabs evaluated
    on the fp64 intermediates; the split sums, which here add storage-dtype
    values in float32, are held to their own stage bound."""
    inp, out, _ = _chain(mode)
    N, HW4, C, L = inp["dims"]
    pooled, _ = R.pooled_ref(inp["f"])
    mu, _ = R.linear_fwd_ref(pooled, inp["w_mu"], inp["b_mu"])
    lv, _ = R.linear_fwd_ref(pooled, inp["w_lv"], inp["b_lv"])
    z, _ = R.reparam_fwd_ref(mu, lv, inp["eps"])
    dz = inp["hin"]["dz_in"].double()
    dz_abs = dz.abs()
    K = 4.0
    for i, (J, dmap) in enumerate(zip(inp["jobs"], inp["dmaps"])):
        co, cpad, HW = inp["geos"][i]
        part = R.latent_sums_ref(dmap)
        sabs = R.latent_sums_ref(dmap.abs())
        R.assert_lin(out[f"part{i}"], part, sabs, f"chain part{i}")
        y, _ = R.linear_fwd_ref(z, J.w, J.b)
        bn = R.latent_bn_ref(y, J.gamma, J.beta, J.rm, J.rv, MOM, EPS, True, HW)
        coef = torch.stack([bn["scale"], bn["shift"], bn["mean"], bn["invstd"]])
        # the device decided the same gates as fp64 does from the original inputs
        assert torch.equal((y * coef[0] + coef[1]) > 0, out[f"act{i}"].float() > 0)
        val, mag = R.latent_bwd_consumer_ref(part, y, coef, z, J.w, J.gamma, True)
        for name in ("dw", "dgamma", "dbeta"):
            R.assert_lin(out[f"{name}{i}"], val[name], K * mag[name], f"chain {name}{i}")
        assert not out[f"dbias{i}"].any()
        dz, dz_abs = dz + val["dz"], dz_abs + mag["dz"]
    hin = inp["hin"]
    val, mag = R.latent_bwd_heads_ref(dz, dz_abs, hin["dmu_in"], hin["dlv_in"], inp["eps"], lv, pooled, inp["w_mu"],
                                      inp["w_lv"])
    for name in H_OUT + ("dpooled",):
        R.assert_lin(out[name], val[name], K * mag[name], f"chain {name}")


@pytest.mark.parametrize("mode", MODES)
def test_repeatable(mode):
    """two identical chains of launches: identical bits everywhere"""
    _, a, _ = _chain(mode)
    _, b, _ = _chain(mode)
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is not None:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
