"""CPU checks of tests/ref_small.py itself: the hand-written backward
references agree with torch autograd in fp64 on the shapes the GPU tests use,
the BatchNorm input conditioning leaves no element near the ReLU's edge on the
seeds used, and the guarded buffers notice a stray write.  The references of
latent.hip are compared with autograd of the real composition (pool + heads,
reparameterize, expand, 1x1 conv + BatchNorm + ReLU), every latent case list is
asserted free of ReLU-gate edges, and the loss / inference references are
compared with oracle/cpu_ref.py and plain torch."""
import pytest
import torch
import torch.nn.functional as F

import ref_small as R

BF16 = torch.bfloat16


@pytest.mark.parametrize("shape", R.POOL_SHAPES)
@pytest.mark.parametrize("negative", [False, True])
def test_pool3_refs_match_autograd(shape, negative):
    N, C, H, W = shape
    x = R.pool_input(shape, negative=negative).double().requires_grad_(True)
    y, code = R.pool3_ref(x.detach())
    yt = F.max_pool2d(x, 3, 2, 1)
    assert torch.equal(y, yt.detach())
    if negative:
        assert float(y.max()) < 0   # padding never wins
    # the code names an element of the window that holds the maximum, and no
    # earlier element of the window (row-major) does: first maximum wins
    xp = F.pad(x.detach(), [1, 1, 1, 1], value=float("-inf"))
    win = xp.unfold(2, 3, 2).unfold(3, 3, 2).reshape(N, C, y.shape[2], y.shape[3], 9)
    first = (win == y[..., None]).to(torch.uint8).argmax(-1)
    assert torch.equal(first.to(torch.uint8), code)
    g = torch.Generator().manual_seed(5)
    dy = torch.randint(-4, 5, y.shape, generator=g).double()
    yt.backward(dy)
    assert torch.equal(R.pool3_bwd_ref(dy, code, H, W), x.grad)


@pytest.mark.parametrize("case", R.LINEAR_BWD_CASES + R.LINEAR_FWD_CASES)
def test_linear_refs_match_autograd(case):
    B, K, J = case
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, K, generator=g).double().requires_grad_(True)
    w = torch.randn(J, K, generator=g).double().requires_grad_(True)
    b = torch.randn(J, generator=g).double().requires_grad_(True)
    dy = torch.randn(B, J, generator=g).double()
    y = F.linear(x, w, b)
    yr, mag = R.linear_fwd_ref(x.detach(), w.detach(), b.detach())
    torch.testing.assert_close(yr, y.detach(), rtol=1e-13, atol=1e-13)
    assert (mag >= yr.abs() * (1 - 1e-12)).all()
    y.backward(dy)
    (dx, dw, db), (ax, aw, ab) = R.linear_bwd_ref(x.detach(), w.detach(), dy)
    for got, want, sab in ((dx, x.grad, ax), (dw, w.grad, aw), (db, b.grad, ab)):
        torch.testing.assert_close(got, want, rtol=1e-13, atol=1e-13)
        assert (sab >= got.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("n", R.REPARAM_N)
def test_reparam_refs_match_autograd(n):
    g = torch.Generator().manual_seed(7)
    mu = torch.randn(n, generator=g).double().requires_grad_(True)
    lv = (torch.rand(n, generator=g).double() * 12 - 6).requires_grad_(True)
    eps = torch.randn(n, generator=g).double()
    dz = torch.randn(n, generator=g).double()
    z = mu + eps * torch.exp(0.5 * lv)
    z.backward(dz)
    zr, mag = R.reparam_fwd_ref(mu.detach(), lv.detach(), eps)
    torch.testing.assert_close(zr, z.detach(), rtol=1e-14, atol=0)
    assert (mag >= zr.abs() * (1 - 1e-12)).all()
    dmu, dlv = R.reparam_bwd_ref(lv.detach(), eps, dz)
    torch.testing.assert_close(dmu, mu.grad, rtol=0, atol=0)
    torch.testing.assert_close(dlv, lv.grad, rtol=1e-14, atol=0)
    dmu, dlv = R.reparam_bwd_ref(lv.detach(), None, dz)
    assert torch.equal(dmu, dz) and not dlv.any()


@pytest.mark.parametrize("case", R.PW_BWD_CASES[:-1])
def test_pointwise_refs_match_conv1x1_autograd(case):
    P, C, J = case
    x, w, b, dy = R.pw_inputs(P, C, J, torch.float32)
    xi = x.double().t().reshape(1, C, P, 1).requires_grad_(True)
    wi = w.double().reshape(J, C, 1, 1).requires_grad_(True)
    bi = b.double().requires_grad_(True)
    y = F.conv2d(xi, wi, bi)
    yr, _ = R.pointwise_fwd_ref(x, w, b)
    torch.testing.assert_close(yr, y.detach()[0, :, :, 0].t(), rtol=1e-13, atol=1e-13)
    y.backward(dy.double().t().reshape(1, J, P, 1))
    (dx, dw, db), _ = R.pointwise_bwd_ref(x, w, dy)
    torch.testing.assert_close(dx, xi.grad[0, :, :, 0].t(), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(dw, wi.grad.reshape(J, C), rtol=1e-13, atol=1e-12)
    torch.testing.assert_close(db, bi.grad, rtol=1e-13, atol=1e-12)


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("case", sorted(set(R.PW_BWD_CASES + R.PW_BN_FWD_CASES)))
def test_bn_conditioning_leaves_no_element_near_zero(case, dtype):
    P, C, J = case
    x, _, _, _, coef = R.pw_bn_inputs(P, C, J, dtype)
    assert torch.equal(x.to(dtype).float(), x)   # still representable in the storage dtype
    assert int(R.bn_near_zero(x, coef[0], coef[1]).sum()) == 0
    # both signs of scale, and channels the ReLU removes entirely
    if C >= 8:
        assert (coef[0] > 0).any() and (coef[0] < 0).any()
        a = R.bn_act_ref(x, coef[0], coef[1], dtype)
        assert (a[:, 3::4] == 0).all() and (a > 0).any()


def test_bnb_partials_ref_ownership_and_finish():
    """The interleaved block ownership sums to the plain per-channel sums, and
    the finish formulas reproduce autograd's BatchNorm(+ReLU) backward."""
    P, C, nblk = 3 * R.TILE + 17, 8, 3
    g = torch.Generator().manual_seed(8)
    x = torch.randn(P, C, generator=g).double()
    dy = torch.randn(P, C, generator=g).double()
    gamma = (torch.rand(C, generator=g) + 0.5).double().requires_grad_(True)
    beta = (torch.randn(C, generator=g) * 0.3).double().requires_grad_(True)
    eps = 1e-5
    mean, var = x.mean(0), x.var(0, unbiased=False)
    invstd = 1 / torch.sqrt(var + eps)
    scale, shift = gamma.detach() * invstd, beta.detach() - mean * gamma.detach() * invstd
    xi = x.clone().requires_grad_(True)
    out = torch.relu(F.batch_norm(xi, None, None, gamma, beta, True, 0.0, eps))
    out.backward(dy)
    part, sabs = R.bnb_partials_ref(dy, x, scale, shift, mean, invstd, nblk)
    keep = (x * scale + shift) > 0
    torch.testing.assert_close(part[:, 0].sum(0), (dy * keep).sum(0), rtol=1e-12, atol=1e-12)
    own1 = ((torch.arange(P) // R.TILE) % nblk) == 1
    torch.testing.assert_close(part[1, 0], (dy * keep)[own1].sum(0), rtol=1e-12, atol=1e-12)
    assert (sabs >= part.abs() * (1 - 1e-12)).all()
    dgamma, dbeta, k = R.bn_bwd_finish_ref(part, gamma.detach(), invstd, P)
    torch.testing.assert_close(dgamma, gamma.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(dbeta, beta.grad, rtol=1e-10, atol=1e-10)
    dx = k[0] * (dy * keep) + k[1] * (x - mean) + k[2]
    torch.testing.assert_close(dx, xi.grad, rtol=1e-9, atol=1e-9)


def test_adamw_ref_matches_torch_adamw_fp64():
    g = torch.Generator().manual_seed(9)
    p0 = torch.randn(37, generator=g).double()
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([p], lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8)
    pr, m, v = p0.clone(), torch.zeros(37).double(), torch.zeros(37).double()
    for step in (1, 2, 3):
        gr = torch.randn(37, generator=g).double()
        p.grad = gr.clone()
        opt.step()
        pr, m, v = R.adamw_ref(pr, m, v, gr, step, 1e-3, 1e-2, 0.9, 0.999, 1e-8)
    torch.testing.assert_close(pr, p.detach(), rtol=1e-12, atol=1e-14)
    st = opt.state[p]
    torch.testing.assert_close(m, st["exp_avg"], rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("dtype", [torch.float32, BF16, torch.uint8])
def test_guarded_buffers_notice_stray_writes(dtype):
    t, g = R.guarded((3, 5), dtype, device="cpu", offset=1)
    t.zero_()
    g.check("inner write")
    g.buf[R.guarded.__defaults__[1] + 1 + 15] = 0   # one past the end
    with pytest.raises(AssertionError):
        g.check("tail")
    if dtype == torch.uint8:
        return
    a, g = R.guarded_act(2, 8, 3, 4, dtype, device="cpu", wide=16, c0=8)
    assert a.shape == (2, 8, 3, 4) and a.stride(1) == 1 and a.stride(3) == 16
    a.zero_()
    g.check("slice write")
    a2, g2 = R.guarded_act(2, 8, 3, 4, dtype, device="cpu", wide=16, c0=0)
    a2.zero_()
    g2.buf[64 + 8] = 1.0   # the neighbouring channel of pixel 0
    with pytest.raises(AssertionError):
        g2.check("neighbour")
    r, g3 = R.guarded_rows(5, 8, dtype, device="cpu", wide=24, c0=8)
    assert r.shape == (5, 8) and r.stride() == (24, 1)
    r.fill_(1.0)
    g3.check("rows")


# ----------------------------------------------------------------------------
# latent.hip references
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_latent_refs_match_autograd(train):
    """pool + 1x1 heads, reparameterize, expand, Conv2d(L, co, 1) + BatchNorm2d
    + ReLU under a random upstream gradient (and incoming gradients on mu and
    logvar): outputs, running statistics and every gradient."""
    N, C, H4, W4, L, co, H, W = 3, 16, 3, 2, 5, 8, 4, 3
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g).double()
    f = rnd(N, C, H4, W4).requires_grad_(True)
    w_mu, w_lv = (rnd(L, C) / 4).requires_grad_(True), (rnd(L, C) / 4).requires_grad_(True)
    b_mu, b_lv = rnd(L).requires_grad_(True), rnd(L).requires_grad_(True)
    eps, dmap, a_mu, a_lv = rnd(N, L), rnd(N, co, H, W), rnd(N, L), rnd(N, L)
    mom, bn_eps = float(torch.tensor(R.LAT_MOM)), float(torch.tensor(R.LAT_EPS))
    conv = torch.nn.Conv2d(L, co, 1).double()
    bn = torch.nn.BatchNorm2d(co, momentum=mom, eps=bn_eps).double()
    with torch.no_grad():
        bn.weight.copy_(rnd(co) + 0.2)
        bn.bias.copy_(rnd(co) * 0.3)
        bn.running_mean.copy_(rnd(co) * 0.2)
        bn.running_var.copy_(torch.rand(co, generator=g).double() + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    bn.train(train)
    pooled = F.adaptive_avg_pool2d(f, 1)
    mu = F.conv2d(pooled, w_mu[:, :, None, None], b_mu).flatten(1)
    lv = F.conv2d(pooled, w_lv[:, :, None, None], b_lv).flatten(1)
    z = mu + eps * torch.exp(lv / 2)
    y_map = conv(z[:, :, None, None].expand(N, L, H, W))
    out = torch.relu(bn(y_map))
    ((out * dmap).sum() + (mu * a_mu).sum() + (lv * a_lv).sum()).backward()
    close = lambda got, want, what: torch.testing.assert_close(got, want.detach(), rtol=1e-9, atol=1e-10, msg=what)
    # forward
    rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1])
    pr, pabs = R.pooled_ref(rows(f))
    close(pr, pooled.flatten(1), "pooled")
    assert (pabs >= pr.abs() * (1 - 1e-12)).all()
    mr, _ = R.linear_fwd_ref(pr, w_mu.detach(), b_mu.detach())
    lr, _ = R.linear_fwd_ref(pr, w_lv.detach(), b_lv.detach())
    zr, _ = R.reparam_fwd_ref(mr, lr, eps)
    close(mr, mu, "mu"), close(lr, lv, "logvar"), close(zr, z, "z")
    wc, bc = conv.weight.detach().reshape(co, L), conv.bias.detach()
    yr, _ = R.linear_fwd_ref(zr, wc, bc)
    close(yr, y_map[:, :, 0, 0], "y")
    bnr = R.latent_bn_ref(yr, bn.weight.detach(), bn.bias.detach(), rm0, rv0, mom, bn_eps, train, H * W)
    act, amag = R.latent_act_ref(yr, bnr["scale"], bnr["shift"])
    close(act[:, :, None, None].expand(N, co, H, W), out, "map")
    assert (amag >= act * (1 - 1e-12)).all()
    if train:
        close(bnr["rm"], bn.running_mean, "running_mean"), close(bnr["rv"], bn.running_var, "running_var")
        assert int(bn.num_batches_tracked) == 1
    else:
        assert "rm" not in bnr and torch.equal(bn.running_mean, rm0) and torch.equal(bn.running_var, rv0)
    # backward
    part = R.latent_sums_ref(rows(dmap))
    close(part.sum(1), dmap.sum((2, 3)), "split sums")
    coef = torch.stack([bnr["scale"], bnr["shift"], bnr["mean"], bnr["invstd"]])
    val, mag = R.latent_bwd_consumer_ref(part, yr, coef, zr, wc, bn.weight.detach(), train)
    close(val["dw"], conv.weight.grad.reshape(co, L), "dw"), close(val["dbias"], conv.bias.grad, "dbias")
    close(val["dgamma"], bn.weight.grad, "dgamma"), close(val["dbeta"], bn.bias.grad, "dbeta")
    if train:
        assert float(conv.bias.grad.abs().max()) < 1e-12      # the batch mean absorbs the conv bias
    hv, hm = R.latent_bwd_heads_ref(val["dz"], mag["dz"], a_mu, a_lv, eps, lr, pr, w_mu.detach(), w_lv.detach())
    close(hv["dw_mu"], w_mu.grad, "dw_mu"), close(hv["dw_lv"], w_lv.grad, "dw_lv")
    close(hv["db_mu"], b_mu.grad, "db_mu"), close(hv["db_lv"], b_lv.grad, "db_lv")
    close((hv["dpooled"] / (H4 * W4))[:, :, None, None].expand(N, C, H4, W4), f.grad, "d f4")
    for k in val:
        assert (mag[k] >= val[k].abs() * (1 - 1e-12)).all(), k
    for k in hv:
        assert (hm[k] >= hv[k].abs() * (1 - 1e-12)).all(), k
    # eps None: z = mu, no gradient into logvar but the incoming one
    hv0, _ = R.latent_bwd_heads_ref(val["dz"], mag["dz"], a_mu, None, None, None, pr, w_mu.detach(), w_lv.detach())
    assert not hv0["dw_lv"].any() and not hv0["db_lv"].any()


def _no_gate_edge(z, params, train, HW):
    w, b, gamma, beta, rm, rv = params
    y, _ = R.linear_fwd_ref(z, w, b)
    bn = R.latent_bn_ref(y, gamma, beta, rm, rv, R.LAT_MOM, R.LAT_EPS, train, HW)
    assert int(R.gate_near_zero(y, bn["scale"], bn["shift"]).sum()) == 0
    # the margin is there, not just absent edges: the gate is at least 1e-3 of its terms
    a, amag = R.latent_act_ref(y, bn["scale"], bn["shift"])
    assert bool(((y * bn["scale"] + bn["shift"]).abs() >= R.GATE_MARGIN * amag).all())


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("case", R.LAT_FWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_latent_fwd_cases_have_no_gate_edge(case, bias, train):
    N, L, co, cpad, HW = case
    z, params = R.fwd_job_inputs(N, L, co, HW, train, bias)
    _no_gate_edge(z, params, train, HW)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("table", R.LAT_FWD_TABLES, ids=lambda t: f"{len(t[2])}jobs")
def test_latent_fwd_tables_have_no_gate_edge(table, train):
    N, L, geos = table
    for i, (co, cpad, HW) in enumerate(geos):
        z, params = R.fwd_job_inputs(N, L, co, HW, train, bool((i + 1) % 3), i)
        _no_gate_edge(z, params, train, HW)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", R.LAT_BWD_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{'-'.join(map(str, c[2]))}x{c[3]}")
def test_latent_bwd_cases_have_no_gate_edge(case, train):
    N, L, cos, C = case
    for integer in (False, True):
        for i, co in enumerate(cos):
            part, y, coef, gamma, w = R.bwd_consumer_inputs(N, L, co, train, integer, seed=34 + 13 * i)
            assert int(R.gate_near_zero(y, coef[0], coef[1]).sum()) == 0
            assert (coef[0] > 0).any() and ((coef[0] < 0).any() or co <= 8)
            if train and N == 1:
                assert torch.equal(y, coef[2].reshape(1, co))


def test_latent_case_lists_cover_the_axes():
    assert {c[0] for c in R.LAT_FWD_CASES} == {1, 3, 64} and {c[1] for c in R.LAT_FWD_CASES} == {1, 5, 32, 64}
    assert {c[2:] for c in R.LAT_FWD_CASES} == {(8, 8, 1), (32, 64, 600), (8, 136, 70), (128, 128, 1024),
                                                  (2048, 2048, 1), (32, 32, 1025)}
    assert (3, 5, 32, 64, 600) in R.LAT_FWD_CASES and [len(t[2]) for t in R.LAT_FWD_TABLES] == [3, 8]
    assert {c[0] for c in R.LAT_BWD_CASES} == {1, 3, 9, 64} and {c[1] for c in R.LAT_BWD_CASES} == {1, 5, 64}
    assert {co for c in R.LAT_BWD_CASES for co in c[2]} == {8, 32, 64, 512}
    assert {c[3] for c in R.LAT_BWD_CASES} == {8, 24, 512} and {len(c[2]) for c in R.LAT_BWD_CASES} == {1, 3}


def test_latent_sums_ref_splits():
    g = torch.Generator().manual_seed(12)
    for HW in (1, 31, 32, 33, 600):
        d = torch.randint(-4, 5, (2, HW, 8), generator=g).float()
        part = R.latent_sums_ref(d)
        per = -(-HW // R.LAT_SPLITS)
        assert torch.equal(part.sum(1), d.double().sum(1))
        assert torch.equal(part[:, 0], d[:, :per].double().sum(1))
        assert not part[:, -(-HW // per):].any()


# ----------------------------------------------------------------------------
# loss.hip references
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("smooth,weights", [(1.0, (0.5, 0.5)), (0.25, (0.3, 0.7)), (4.0, (0.0, 1.0))])
@pytest.mark.parametrize("cold", [False, True])
def test_bce_dice_refs_match_autograd(smooth, weights, cold):
    from oracle import cpu_ref
    wb, wd = weights
    g = torch.Generator().manual_seed(13)
    n = 37
    x = (torch.randn(n, generator=g) * 3).double()
    t = torch.rand(n, generator=g).double()
    if cold:
        x, t = -12 - x.abs(), t * 0.001
    xr = x.clone().requires_grad_(True)
    loss = wb * cpu_ref.bce_with_logits_mean(xr, t) + wd * cpu_ref.dice_loss(xr, t, smooth)
    (-2.5 * loss).backward()
    sums, sabs = R.bce_dice_fwd_ref(x, t)
    dl, _ = R.dice_loss_from_sums(sums, smooth)
    # (the sums pass through float32 on their way into the loss, as in the kernel)
    torch.testing.assert_close(wb * sums[0] / n + wd * dl, loss.detach(), rtol=1e-6, atol=1e-7)
    grad, gabs = R.bce_dice_bwd_ref(x, t, sums, smooth, wb, wd, -2.5)
    torch.testing.assert_close(grad, xr.grad, rtol=2e-6, atol=1e-9)
    assert (gabs >= grad.abs() * (1 - 1e-12)).all() and (sabs >= sums.abs() * (1 - 1e-12)).all()
    if cold:
        assert float(sums[2]) < smooth / 2 and float(sums[3]) < smooth / 2
    # the float32 form (ATen's BCE) is the same function
    s32, _ = R.bce_dice_fwd_ref(x.float(), t.float(), torch.float32)
    torch.testing.assert_close(s32, sums, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("fb", [0.0, 1e-3, 0.5])
def test_kl_ref_matches_autograd(fb):
    from oracle import cpu_ref
    g = torch.Generator().manual_seed(14)
    mu, lv = torch.randn(6, 9, generator=g), torch.randn(6, 9, generator=g)
    mu[0, :3], lv[0, :3] = torch.tensor([15.0, 0.0, 0.0]), torch.tensor([0.0, -250.0, -150.0])
    mu[1, 0], lv[1, 0] = 1.0, 0.0          # kl = 0.5 exactly
    m, v = mu.double().requires_grad_(True), lv.double().requires_grad_(True)
    val = cpu_ref.kl_with_free_bits(m, v, fb)
    (0.75 * val).backward()
    r = R.kl_ref(mu, lv, fb, 0.75)
    assert float(r["kl32"][1, 0]) == 0.5
    torch.testing.assert_close(r["value"], val.detach(), rtol=1e-12, atol=0)
    torch.testing.assert_close(r["gmu"], m.grad, rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(r["glv"], v.grad, rtol=1e-12, atol=1e-15)
    assert float(r["gmu"][0, 0]) == 0.0 and float(r["glv"][0, 1]) == 0.0 and float(r["glv"][0, 2]) != 0.0
    if fb == 0.5:
        assert float(r["gmu"][1, 0]) == 0.5 * 0.75 / 6


def test_dice_score_ref_matches_oracle():
    from oracle import cpu_ref
    g = torch.Generator().manual_seed(15)
    x, t = torch.rand(300, generator=g), (torch.rand(300, generator=g) < 0.4).float()
    x[:3] = torch.tensor([0.5, float("nan"), 1.0])
    s, c = R.dice_score_ref(x, t, 1e-6)
    assert float(s) == float(cpu_ref.dice_score(x, t, 1e-6))
    assert c.tolist() == [float((x > 0.5).sum()), float((t > 0.5).sum()), float(((x > 0.5) & (t > 0.5)).sum())]
    assert float(R.dice_score_ref(torch.full((5,), 0.5), torch.zeros(5), 1.0)[0]) == 1.0


# ----------------------------------------------------------------------------
# infer.hip references
# ----------------------------------------------------------------------------
def test_uncertainty_ref_matches_torch():
    g = torch.Generator().manual_seed(16)
    seg = torch.rand(8, 50, generator=g)
    val, mag = R.uncertainty_ref(seg)
    s = seg.double()
    eps = float(torch.tensor(1e-7))
    ent = lambda a: -(a * torch.log(a + eps) + (1 - a) * torch.log(1 - a + eps))
    torch.testing.assert_close(val["mean"], s.mean(0), rtol=1e-13, atol=0)
    torch.testing.assert_close(val["std"], s.std(0), rtol=1e-12, atol=0)            # unbiased
    torch.testing.assert_close(val["entropy"], ent(s.mean(0)), rtol=1e-12, atol=0)
    torch.testing.assert_close(val["mi"], ent(s.mean(0)) - ent(s).mean(0), rtol=1e-9, atol=1e-14)
    torch.testing.assert_close(val["cv"], s.std(0) / (s.mean(0) + eps), rtol=1e-12, atol=0)
    for k in val:
        assert (mag[k] >= val[k].abs() * (1 - 1e-12)).all(), k
    one, _ = R.uncertainty_ref(seg[:1])
    assert torch.isnan(one["std"]).all() and torch.isnan(one["cv"]).all() and torch.isfinite(one["mi"]).all()


def test_blend_weight_ref():
    ramp = torch.linspace(0, 1, 3)
    w = R.blend_weight_ref(12, 10, 3, ramp, 1, 1, 1, 1)
    assert torch.equal(w[:, 5], torch.tensor([0, .5, 1, 1, 1, 1, 1, 1, 1, 1, .5, 0]))
    assert torch.equal(w[5], torch.tensor([0, .5, 1, 1, 1, 1, 1, 1, .5, 0]))
    assert float(w[1, 1]) == 0.25
    assert bool((R.blend_weight_ref(12, 10, 3, ramp, 0, 0, 0, 0) == 1).all())
    assert torch.equal(R.blend_weight_ref(6, 10, 3, ramp, 1, 1, 1, 1), w[5:6].expand(6, 10))   # 6 = 2 ov: no feathering
    assert bool((R.blend_weight_ref(5, 4, 0, torch.zeros(1), 1, 1, 1, 1) == 1).all())


@pytest.mark.parametrize("HW", [(16, 16), (5, 9)])
def test_flip_rot_map_matches_flip_and_rot90(HW):
    H, W = HW
    x = torch.arange(2 * H * W).float().view(2, H, W)
    for f in R.FLIP_ROT:
        m, Ho, Wo = R.flip_rot_map(H, W, *f)
        want = R.flip_rot_ref(x, *f)
        assert want.shape == (2, Ho, Wo)
        i, j = torch.arange(Ho).view(-1, 1), torch.arange(Wo).view(1, -1)
        sy, sx = m[0] * i + m[1] * j + m[2], m[3] * i + m[4] * j + m[5]
        assert int(sy.min()) >= 0 and int(sy.max()) < H and int(sx.min()) >= 0 and int(sx.max()) < W
        assert torch.equal(x[:, sy, sx], want), f
    assert len({tuple(R.flip_rot_map(16, 16, *f)[0]) for f in R.FLIP_ROT}) == 8     # the 8 symmetries of the square


def test_mean_groups_and_sigmoid_refs():
    x = torch.tensor([[1.0, 2.0], [3.0, 5.0], [5.0, 2.0]])
    assert torch.equal(R.mean_groups_ref(x), torch.tensor([3.0, 3.0]))
    y, _ = R.sigmoid_ref(torch.tensor([0.0, float("inf"), float("-inf"), float("nan")]))
    assert y[:3].tolist() == [0.5, 1.0, 0.0] and torch.isnan(y[3])
    assert R.trans_ratio(torch.tensor([1.0, float("nan")]), torch.tensor([1.0, float("nan")]), torch.ones(2)) == 0.0
    assert R.trans_ratio(torch.tensor([1.0, 2.0]), torch.tensor([1.0, float("nan")]), torch.ones(2)) == float("inf")
    assert abs(R.trans_ratio(torch.tensor([1.0 + 2.0 ** -20]), torch.tensor([1.0]), torch.ones(1)) - 16.0) < 1e-6
    assert float(R.lin_ratio(torch.tensor([1.0 + 2.0 ** -23]), torch.tensor([1.0]), torch.zeros(1))) > 1.0
