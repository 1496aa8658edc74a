"""CPU checks of tests/ref_small.py itself: the hand-written backward
references agree with torch autograd in fp64 on the shapes the GPU tests use,
the BatchNorm input conditioning leaves no element near the ReLU's edge on the
seeds used, and the guarded buffers notice a stray write."""
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
