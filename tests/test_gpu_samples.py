"""The sample-set metrics (vaeunet_amd/csrc/sampleset.hip, vaeunet_amd/samples.py,
DESIGN.md §4.14) on the GPU against the numpy restatement in
tests/samples_ref.py.

The Gram matrix is integers: compared EXACTLY.  Plane shapes 1 x 1, 1 x 63,
1 x 64, 1 x 65, 67 x 131, 129 x 257 (odd H W with several planes: rows that are
not 16-byte aligned) and 68 x 132 (several block steps of the 16-byte path);
(S, M) from (1, 0) to (63, 1) and (61, 3); 1, 3 and 2 x 2 planes; float32 and
uint8 samples against float32 and uint8 truths; one shape per load path that
is larger than one sweep of the capped grid, named from VU_SAMPLESET_GRID,
VU_SAMPLESET_STEP and VU_SAMPLESET_VEC.  Every run goes through the C ABI on
guarded buffers: the inputs come back bitwise unchanged and no guard element is
written.

The metrics are fp64 functions of the integers, summed in the reference's
order: columns 0-6 within 1e-12 absolute (each is a sum of at most 64^2 terms
in [0, 1]: 4096 * 2^-53 = 4.5e-13, plus the final operations), the area columns
within the same bound relative to the value."""
import functools
import warnings

import numpy as np
import pytest
import torch

import ref_small as R
import samples_ref as SR
from golden_util import INFER_SEED, infer_inputs, pyramid_encoder, seed_bn_stats, seed_vae_tail

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
INVALID = 1   # hipErrorInvalidValue

SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (67, 131), (129, 257), (68, 132)]
SM = [(1, 0), (1, 1), (2, 1), (31, 1), (32, 1), (33, 3), (63, 1), (61, 3)]
PLANES = [(1, 1), (1, 3), (2, 2)]
DTYPES = [(np.float32, np.float32), (np.float32, np.uint8), (np.uint8, np.float32), (np.uint8, np.uint8)]
CASES = [(hw, sm) for hw in SHAPES for sm in SM]
TOL = 1e-12


def _L():
    from vaeunet_amd import _lib
    return _lib


def _S():
    import vaeunet_amd.samples as S
    return S


@functools.lru_cache(maxsize=None)
def _stack(kind, S, M, B, C, H, W):
    """(samples [S, B, C, H, W], truths [M, B, C, H, W]) uint8 and their reference Gram: computed once, read-only"""
    s, t = SR.stack(kind, S, M, B * C, H, W)
    s, t = s.reshape(S, B, C, H, W), t.reshape(M, B, C, H, W)
    G = SR.gram(s, t)
    for a in (s, t, G):
        a.setflags(write=False)
    return s, t, G


def _encode(bits, dtype, thr, seed):
    """the bits as a uint8 mask with arbitrary nonzero values, or as float32 probabilities around ``thr``"""
    if dtype == np.uint8:
        rng = np.random.Generator(np.random.PCG64(seed))
        return (bits * rng.integers(1, 256, bits.shape)).astype(np.uint8)
    return SR.as_prob(bits, thr, seed)


def _code(a):
    L = _L()
    return L.VU_CCL_F32 if a.dtype == np.float32 else L.VU_CCL_U8


def _gram_raw(samples, truths, thr=0.5, accumulate=0, runs=1, offset=0, fill=None):
    """vu_sample_gram on guarded buffers -> int64 [B, C, K, K] numpy; the inputs bitwise unchanged, no guard written.
    ``fill``: what the output holds before the first run (default: the guard's sentinel)"""
    L = _L()
    S, B, C, H, W = samples.shape
    M = 0 if truths is None else truths.shape[0]
    K = S + M
    bufs = []
    for a in (samples, truths):
        if a is None or a.shape[0] == 0:
            bufs.append((None, None, None))
            continue
        d, g = R.guarded(a.shape, torch.float32 if a.dtype == np.float32 else torch.uint8, DEV, offset=offset)
        d.copy_(torch.from_numpy(np.array(a)))
        bufs.append((d, g, a))
    gram, gg = R.guarded((B, C, K, K), torch.int64, DEV)
    if fill is not None:
        gram.fill_(fill)
    (ds, _, _), (dt, _, _) = bufs
    for _ in range(runs):
        L.call("vu_sample_gram", L.ptr(ds), _code(samples), float(thr), L.ptr(dt), _code(truths) if M else 0, S, M, B * C,
               H, W, L.ptr(gram), accumulate, L.stream())
    torch.cuda.synchronize()
    gg.check("vu_sample_gram gram")
    for d, g, a in bufs:
        if d is not None:
            g.check("vu_sample_gram input")
            assert np.array_equal(d.cpu().numpy().view(np.uint8), np.ascontiguousarray(a).view(np.uint8))
    return gram.cpu().numpy()


# ----------------------------------------------------------------------------
# the Gram matrix
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(CASES)), ids=lambda i: "%dx%d-S%dM%d" % (CASES[i][0] + CASES[i][1]))
def test_gram_is_exactly_the_reference(idx):
    """every shape with every (S, M); the planes, the kind of stack and the threshold rotate with the case, and each
    case runs all four dtype pairs against one reference"""
    (H, W), (S, M) = CASES[idx]
    B, C = PLANES[idx % len(PLANES)]
    kind = SR.KINDS[idx % len(SR.KINDS)]
    thr = (0.5, 0.3, 0.75)[idx % 3]
    s, t, want = _stack(kind, S, M, B, C, H, W)
    for n, (sdt, tdt) in enumerate(DTYPES):
        if M == 0 and tdt == np.uint8:
            continue          # no truths: one run per sample dtype
        got = _gram_raw(_encode(s, sdt, thr, idx * 8 + n), _encode(t, tdt, 0.5, idx * 8 + 4 + n) if M else None, thr)
        assert got.dtype == np.int64 and np.array_equal(got, want), (kind, sdt.__name__, tdt.__name__)


@pytest.mark.parametrize("kind", SR.KINDS)
def test_gram_of_every_adversarial_stack(kind):
    """every kind at an odd and at a 16-byte plane, 2 x 2 planes, S + M = 5 + 2; the API agrees with the C ABI"""
    Sm = _S()
    for H, W in ((67, 131), (68, 132)):
        s, t, want = _stack(kind, 5, 2, 2, 2, H, W)
        p = _encode(s, np.float32, 0.5, 11)
        assert np.array_equal(_gram_raw(p, t), want), (H, W)
        assert np.array_equal(_gram_raw(s, _encode(t, np.float32, 0.5, 12)), want), (H, W)
        got = Sm.sample_gram(torch.from_numpy(p).to(DEV), torch.from_numpy(np.array(t)).to(DEV))
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)


def test_gram_past_one_sweep_of_the_grid():
    """one plane with more steps than VU_SAMPLESET_GRID blocks take at VU_SAMPLESET_MIN_STEPS each, on each load
    path: the grid is at its cap and blocks walk a further, ragged step"""
    L = _L()
    sweep = L.VU_SAMPLESET_GRID * L.VU_SAMPLESET_MIN_STEPS * L.VU_SAMPLESET_STEP
    vec = L.VU_SAMPLESET_VEC
    for (H, W), px, sdt in (((2900, 2900), sweep, np.uint8), ((1449, 1449), sweep // vec, np.float32)):
        assert (H * W) % vec == (0 if px == sweep else 1) and px < H * W < px + px // 64
        rng = np.random.Generator(np.random.PCG64(H))
        s = (rng.random((1, 1, 1, H, W)) < 0.4).astype(np.uint8)
        t = (rng.random((1, 1, 1, H, W)) < 0.4).astype(np.uint8)
        s[0, 0, 0, -1, -3:] = 1                  # the last pixels of the ragged step count
        t[0, 0, 0, -1, -2:] = 1
        want = SR.gram(s, t)
        assert np.array_equal(_gram_raw(_encode(s, sdt, 0.5, 1), t), want)
    # several planes share the cap
    s, t, want = _stack("bernoulli0.5", 2, 1, 2, 2, 129, 257)
    assert np.array_equal(_gram_raw(s, t), want)


def test_a_misaligned_base_takes_the_scalar_path_and_equals_the_aligned_run():
    """68 x 132 is a multiple of 4 pixels, but a base one element past a 16-byte boundary has no aligned row"""
    s, t, want = _stack("bernoulli0.5", 3, 1, 1, 3, 68, 132)
    p, q = _encode(s, np.float32, 0.5, 3), _encode(t, np.float32, 0.5, 4)
    for off in (0, 1, 2, 3):
        assert np.array_equal(_gram_raw(p, q, offset=off), want), off
        assert np.array_equal(_gram_raw(s, t, offset=off), want), off


def test_accumulate_adds_overwrite_overwrites_and_two_runs_are_bitwise_equal():
    s, t, want = _stack("bernoulli0.5", 33, 3, 1, 3, 67, 131)
    p = _encode(s, np.float32, 0.5, 7)
    a = _gram_raw(p, t)
    b = _gram_raw(p, t)
    assert a.tobytes() == b.tobytes() and np.array_equal(a, want)
    assert np.array_equal(_gram_raw(p, t, accumulate=1, runs=2, fill=0), 2 * want)
    assert np.array_equal(_gram_raw(p, t, accumulate=1, runs=1, fill=5), want + 5)
    assert np.array_equal(_gram_raw(p, t, accumulate=0, runs=2, fill=5), want)
    # out= of the API accumulates
    Sm = _S()
    dp, dt = torch.from_numpy(p).to(DEV), torch.from_numpy(np.array(t)).to(DEV)
    out = Sm.sample_gram(dp, dt)
    assert Sm.sample_gram(dp, dt, out=out) is out
    assert np.array_equal(out.cpu().numpy(), 2 * want)


def test_nan_the_threshold_itself_bool_and_other_truth_dtypes():
    Sm = _S()
    s, t, want = _stack("bernoulli0.5", 4, 1, 2, 1, 33, 65)
    p = SR.as_prob(s, 0.5, 9)
    assert np.isnan(p).sum() > 100 and (p == np.float32(0.5)).sum() > 100
    dp, ds, dt = torch.from_numpy(p).to(DEV), torch.from_numpy(np.array(s)).to(DEV), torch.from_numpy(np.array(t)).to(DEV)
    for samples, truths in ((dp, dt), (ds.bool(), dt.bool()), (ds * 200, dt.long()), (dp, dt.double() * 0.75),
                            (dp, dt[0]), (ds, dt.cpu())):
        assert np.array_equal(Sm.sample_gram(samples, truths).cpu().numpy(), want)
    # another threshold is another foreground; the uint8 rule ignores it
    assert np.array_equal(Sm.sample_gram(dp, dt, threshold=0.75).cpu().numpy(), SR.gram(p, t, 0.75))
    assert np.array_equal(Sm.sample_gram(ds, dt, threshold=250.0).cpu().numpy(), want)
    # [S, C, H, W] means B = 1; a non-contiguous stack is densified, not misread
    assert np.array_equal(Sm.sample_gram(dp[:, 0], dt[:, 0]).cpu().numpy(), want[:1])
    wide = torch.zeros(4, 2, 1, 33, 130, device=DEV)
    wide[..., ::2] = dp
    assert np.array_equal(Sm.sample_gram(wide[..., ::2], dt).cpu().numpy(), want)
    # no truths
    assert np.array_equal(Sm.sample_gram(dp).cpu().numpy(), want[:, :, :4, :4])


def test_c_abi_rejections_leave_the_output_untouched():
    L = _L()
    x = torch.zeros(65, 1, 8, 8, dtype=torch.uint8, device=DEV)
    y = torch.zeros(3, 1, 8, 8, dtype=torch.float32, device=DEV)
    gram, gg = R.guarded((1, 65, 65), torch.int64, DEV)
    out, go = R.guarded((1, 9), torch.float64, DEV)
    s, px, py, pg = L.stream(), L.ptr(x), L.ptr(y), L.ptr(gram)
    q = lambda *a: L.query("vu_sample_gram", *a)   # noqa: E731
    for args in ((px, 0, 0.5, None, 0, 65, 0, 1, 8, 8, pg, 0, s),            # K = 65
                 (px, 0, 0.5, py, 1, 62, 3, 1, 8, 8, pg, 0, s),              # K = 65 with truths
                 (px, 0, 0.5, None, 0, 0, 0, 1, 8, 8, pg, 0, s),             # S = 0
                 (px, 0, 0.5, py, 1, 0, 3, 1, 8, 8, pg, 0, s),
                 (px, 0, 0.5, None, 0, 4, -1, 1, 8, 8, pg, 0, s),            # M < 0
                 (px, 2, 0.5, None, 0, 4, 0, 1, 8, 8, pg, 0, s),             # a bad dtype
                 (px, -1, 0.5, None, 0, 4, 0, 1, 8, 8, pg, 0, s),
                 (px, 0, 0.5, py, 2, 4, 3, 1, 8, 8, pg, 0, s),               # a bad truth dtype
                 (None, 0, 0.5, None, 0, 4, 0, 1, 8, 8, pg, 0, s),           # null pointers
                 (px, 0, 0.5, None, 1, 4, 3, 1, 8, 8, pg, 0, s),             # truths null with M > 0
                 (px, 0, 0.5, None, 0, 4, 0, 1, 8, 8, None, 0, s),
                 (px, 0, 0.5, None, 0, 4, 0, -1, 8, 8, pg, 0, s),            # negative sizes
                 (px, 0, 0.5, None, 0, 4, 0, 1, -8, 8, pg, 0, s),
                 (px, 0, 0.5, None, 0, 4, 0, 1, 8, -8, pg, 0, s),
                 (px, 0, 0.5, None, 0, 4, 0, 1, 46341, 46341, pg, 0, s),     # H W above the lesions limit
                 (px, 0, 0.5, None, 0, 4, 0, 1, 8, 8, pg, 2, s)):            # accumulate neither 0 nor 1
        assert q(*args) == INVALID, args[1:10]
    # a size of zero returns 0 and launches nothing, null pointers included; the truth dtype is not read at M = 0
    for args in ((px, 0, 0.5, None, 0, 4, 0, 0, 8, 8, pg, 0, s), (px, 0, 0.5, None, 0, 4, 0, 1, 0, 8, pg, 0, s),
                 (None, 0, 0.5, None, 0, 4, 0, 1, 8, 0, None, 0, s)):
        assert q(*args) == 0
    m = lambda *a: L.query("vu_sampleset_metrics", *a)   # noqa: E731
    po = L.ptr(out)
    for args in ((pg, 65, 0, 1, po, s), (pg, 62, 3, 1, po, s), (pg, 0, 3, 1, po, s), (pg, 4, -1, 1, po, s),
                 (pg, 4, 1, -1, po, s), (None, 4, 1, 1, po, s), (pg, 4, 1, 1, None, s)):
        assert m(*args) == INVALID, args[1:4]
    assert m(None, 4, 1, 0, None, s) == 0
    torch.cuda.synchronize()
    gg.keep[:] = True          # nothing at all was written, the inner part included
    go.keep[:] = True
    gg.check("rejected vu_sample_gram")
    go.check("rejected vu_sampleset_metrics")


# ----------------------------------------------------------------------------
# the metrics
# ----------------------------------------------------------------------------
def _metrics_raw(G, S):
    """vu_sampleset_metrics on guarded buffers -> fp64 [B, C, 9] numpy; gram unchanged"""
    L = _L()
    B, C, K, _ = G.shape
    g, gg = R.guarded(G.shape, torch.int64, DEV)
    g.copy_(torch.from_numpy(np.array(G)))
    out, go = R.guarded((B, C, 9), torch.float64, DEV)
    L.call("vu_sampleset_metrics", L.ptr(g), S, K - S, B * C, L.ptr(out), L.stream())
    torch.cuda.synchronize()
    gg.check("vu_sampleset_metrics gram")
    go.check("vu_sampleset_metrics out")
    assert np.array_equal(g.cpu().numpy(), G)
    return out.cpu().numpy()


def _assert_metrics(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    err = np.abs(got - want)
    err[..., 7:] /= np.maximum(np.abs(want[..., 7:]), 1.0)
    worst = np.nanmax(err) if err.size else 0.0
    print(f"{what}: worst error {worst:.3g}")
    assert worst <= TOL, (what, worst)


@pytest.mark.parametrize("SM_", [(1, 0), (1, 1), (2, 1), (5, 0), (32, 1), (33, 3), (63, 1), (61, 3), (32, 32), (1, 63)],
                         ids=lambda c: "S%dM%d" % c)
def test_metrics_match_the_reference(SM_):
    """every kind of stack as the planes of one call (2 x 5 planes), 9 x 13 pixels: the Gram matrix is the
    reference's, so this compares the metrics kernel alone"""
    S, M = SM_
    G = np.stack([_stack(k, S, M, 1, 1, 9, 13)[2][0, 0] for k in SR.KINDS]).reshape(2, 5, S + M, S + M)
    want = SR.metrics(G, S)
    got = _metrics_raw(G, S)
    _assert_metrics(got, want, f"S {S} M {M}")
    if M == 0:
        assert np.isnan(got[..., list(SR.NAN_WITHOUT_TRUTH)]).all() and not np.isnan(got[..., [2, 7, 8]]).any()
    else:
        assert not np.isnan(got).any()
    # the API agrees bitwise with the C ABI
    api = _S().sample_set_metrics(torch.from_numpy(G).to(DEV), S)
    assert api.dtype == torch.float64 and api.cpu().numpy().tobytes() == got.tobytes()


def test_metrics_of_areas_near_2_to_the_31():
    """nested columns of up to 2^31 - 2 pixels: |a| + |b| and 2 I pass 2^31, the variance squares 2^30"""
    big = 2 ** 31 - 2
    area = np.array([big, big - 1, big // 2, 3, 0, big // 3], np.int64)
    G = np.minimum.outer(area, area)[None, None]          # nested sets: I = min(|a|, |b|)
    for S in (6, 4, 1):
        _assert_metrics(_metrics_raw(G, S), SR.metrics(G, S), f"large areas S {S}")


def test_hand_cases():
    Sm = _S()
    d = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    # identical samples equal to the truth; everything empty
    base = (np.arange(35).reshape(1, 1, 1, 5, 7) % 3 == 0).astype(np.uint8)
    for fill in (base, base * 0):
        s = np.repeat(fill, 4, axis=0)
        m = Sm.sample_set_metrics(Sm.sample_gram(d(s), d(fill)), 4).cpu().numpy()[0, 0]
        assert m[:7].tolist() == [0, 0, 0, 0, 1, 1, 1] and m[7] == fill.sum() and m[8] == 0
    # two disjoint non-empty samples (2 and 3 pixels), an empty truth:
    #   d(s_i, y) = 1 - 0 / |s_i| = 1 -> cross 1, Dice 0; d(s0, s1) = 1 - 0 / 5 = 1, d(s_i, s_i) = 0 -> diversity 2 / 4
    #   ged2 = 2 - 0.5 - 0; areas 2, 3 -> mean 2.5, population sd 0.5
    s = np.zeros((2, 1, 1, 2, 3), np.uint8)
    s[0, 0, 0, 0, :2] = 1
    s[1, 0, 0, 1, :] = 1
    G = Sm.sample_gram(d(s), d(np.zeros((1, 1, 2, 3), np.uint8)))
    assert G.cpu().numpy()[0, 0].tolist() == [[2, 0, 0], [0, 3, 0], [0, 0, 0]]
    assert Sm.sample_set_metrics(G, 2).cpu().numpy()[0, 0].tolist() == [1.5, 1.0, 0.5, 0.0, 0.0, 0.0, 0.0, 2.5, 0.5]


# ----------------------------------------------------------------------------
# meter, op, inference
# ----------------------------------------------------------------------------
def test_meter_over_three_batches_is_the_mean_of_the_reference_rows():
    Sm = _S()
    meter = Sm.SampleSetMeter(0.3)
    rows = []
    for n, (kind, B) in enumerate((("bernoulli0.5", 2), ("nested", 1), ("one_empty", 3))):
        s, t, G = _stack(kind, 6, 2, B, 2, 33, 65)
        rows.append(SR.metrics(G, 6))
        samples = torch.from_numpy(SR.as_prob(s, 0.3, n)).to(DEV)
        meter.update(samples, torch.from_numpy(np.array(t)).to(DEV))
    rows = np.concatenate(rows)                                     # [6, 2, 9]
    assert meter.n_planes == 6
    vals = meter.values()
    assert vals.dtype == torch.float64 and vals.shape == (2, 9) and vals.device.type == "cuda"
    _assert_metrics(vals.cpu().numpy(), rows.mean(0), "meter values")
    res = meter.compute()
    assert list(res) == list(SR.NAMES) and all(v.dim() == 0 and v.device.type == "cuda" for v in res.values())
    _assert_metrics(np.array([float(v) for v in res.values()]), rows.reshape(-1, 9).mean(0), "meter compute")
    with pytest.raises(ValueError, match="3 classes"):
        meter.update(torch.zeros(6, 1, 3, 33, 65, device=DEV), torch.zeros(1, 3, 33, 65, device=DEV))
    meter.reset()
    with pytest.raises(RuntimeError, match="no update"):
        meter.compute()


def test_the_op_agrees_with_the_function_and_passes_opcheck():
    Sm = _S()
    s, t, want = _stack("bernoulli0.5", 4, 1, 2, 1, 33, 65)
    dp = torch.from_numpy(SR.as_prob(s, 0.5, 9)).to(DEV)
    dt = torch.from_numpy(np.array(t)).to(DEV)
    op = torch.ops.vaeunet.sample_gram
    for args in ((dp, dt, 0.5), (dp, None, 0.5), (dp > 0.5, dt[0], None)):
        got = op(*args)
        assert torch.equal(got, Sm.sample_gram(*args))
        torch.library.opcheck(op.default, args, test_utils=("test_schema", "test_faketensor"))
    assert np.array_equal(op(dp, dt).cpu().numpy(), want)


def test_sample_set_scores_equals_the_reference_on_the_distributions_own_output():
    from vaeunet_amd import UNetResNet
    from vaeunet_amd import inference as I
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = UNetResNet(3, 1, pretrained=False, latent_injection="all")
    seed_vae_tail(model, INFER_SEED)
    seed_bn_stats(model, INFER_SEED + 50)
    model.encoder = pyramid_encoder(INFER_SEED)
    model = model.to(DEV).eval()
    img = torch.from_numpy(np.ascontiguousarray(infer_inputs()["full_img"][:, :, :64])).to(DEV)
    assert tuple(img.shape) == (1, 3, 64, 64)
    eps = torch.randn(6, 1, 32, generator=torch.Generator().manual_seed(5)).to(DEV)
    segs, mu, lv = I.segmentation_distribution(model, img, num_samples=6, eps=eps, sample_batch=4)
    # a threshold at the samples' median, a mask from one of them: neither side is trivially empty
    thr = float(segs.median())
    mask = (segs[0:1] > thr).to(torch.uint8)
    scores, mu2, lv2 = I.sample_set_scores(model, img, mask, num_samples=6, threshold=thr, eps=eps, sample_batch=4)
    assert torch.equal(mu, mu2) and torch.equal(lv, lv2)
    assert scores.shape == (1, 1, 9) and scores.dtype == torch.float64 and scores.device.type == "cuda"
    assert tuple(segs.shape) == (6, 1, 64, 64)
    G = SR.gram(segs.cpu().numpy()[:, None], mask.cpu().numpy()[:, None], np.float32(thr))
    assert 0 < G[0, 0, 6, 6] < 64 * 64
    _assert_metrics(scores.cpu().numpy(), SR.metrics(G, 6), "sample_set_scores")
    assert scores[0, 0, 5] <= scores[0, 0, 4] <= scores[0, 0, 6] == 1.0        # sample 0 is the mask itself
