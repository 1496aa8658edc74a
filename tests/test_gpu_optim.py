"""Optimizer tail (train.py:406-411): vaeunet_amd.optim.clip_grad_norm_ and
FusedAdamW against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW (the
reference's own calls) on the same parameters and gradients."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(64, 3, 3, 3), (64,), (128, 64, 3, 3), (32, 64, 1, 1), (1,), (2, 64, 1, 1), (9000,)]
    ps = []
    for i, s in enumerate(shapes):
        t = torch.randn(s, generator=g)
        if len(s) == 4 and i % 2 == 0:
            t = t.contiguous(memory_format=torch.channels_last)
        ps.append(t)
    return ps


def _grads(ps, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(p.shape, generator=g) * scale for p in ps]


@pytest.mark.parametrize("max_norm,scale", [(1.0, 1.0), (1.0, 1e-4), (0.5, 3.0)])
def test_clip_grad_norm_matches_torch(max_norm, scale):
    from vaeunet_amd.optim import clip_grad_norm_
    ps = _params(0)
    gs = _grads(ps, 1, scale)
    a = [torch.nn.Parameter(p.to(DEV)) for p in ps]
    b = [torch.nn.Parameter(p.to(DEV)) for p in ps]
    for pa, pb, g in zip(a, b, gs):
        pa.grad = g.to(DEV).contiguous(memory_format=torch.preserve_format)
        pb.grad = g.to(DEV)
    n_ref = torch.nn.utils.clip_grad_norm_(a, max_norm, foreach=True)
    n_got = clip_grad_norm_(b, max_norm)
    assert n_got.device.type == "cuda"
    torch.testing.assert_close(n_got.cpu(), n_ref.cpu(), rtol=1e-6, atol=0)
    for pa, pb in zip(a, b):
        torch.testing.assert_close(pb.grad.cpu(), pa.grad.cpu(), rtol=2e-6, atol=1e-12)


def test_fused_adamw_matches_torch_adamw():
    """Three steps (bias corrections change), lr 1e-4 / wd 1e-5 as in train.py,
    clip before each step; state_dict moves between the two optimizers."""
    from vaeunet_amd.optim import FusedAdamW, clip_grad_norm_
    ps = _params(3)
    a = [torch.nn.Parameter(p.to(DEV)) for p in ps]
    b = [torch.nn.Parameter(p.to(DEV)) for p in ps]
    oa = torch.optim.AdamW(a, lr=1e-4, weight_decay=1e-5, foreach=True)
    ob = FusedAdamW(b, lr=1e-4, weight_decay=1e-5)
    for it in range(3):
        gs = _grads(ps, 10 + it, 0.3)
        for pa, pb, g in zip(a, b, gs):
            pa.grad = g.to(DEV)
            pb.grad = g.to(DEV)
        torch.nn.utils.clip_grad_norm_(a, 1.0, foreach=True)
        clip_grad_norm_(b, 1.0)
        oa.step()
        ob.step()
        for pa, pb in zip(a, b):
            # one fp32 rounding of difference per op at most (fma contraction)
            torch.testing.assert_close(pb.detach().cpu(), pa.detach().cpu(), rtol=1e-6, atol=1e-9)
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["param_groups"][0]["lr"] == sb["param_groups"][0]["lr"]
    for k in sa["state"]:
        assert float(sa["state"][k]["step"]) == float(sb["state"][k]["step"]) == 3.0
        for name in ("exp_avg", "exp_avg_sq"):
            want, got = sa["state"][k][name].cpu(), sb["state"][k][name].cpu()
            # moments that nearly cancel carry the ulp-level differences of
            # their inputs (clip coefficient, fma contraction) at a few 1e-5
            # relative: bound the error by the tensor's scale
            torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6 * float(want.abs().max()))
    # torch AdamW state loads into FusedAdamW and continues identically
    oc = FusedAdamW([torch.nn.Parameter(p.detach().clone()) for p in a], lr=1e-4, weight_decay=1e-5)
    oc.load_state_dict(sa)
    assert float(oc.state_dict()["state"][0]["step"]) == 3.0


def test_fused_optimizer_training_loop_matches_torch():
    """End to end: UNet train steps with FusedAdamW + fused clip give the same
    losses as with torch's AdamW + clip, i.e. the in-place HIP update is seen
    by the next forward (derived bf16/fp32 weight layouts are invalidated)."""
    from vaeunet_amd import UNet
    from vaeunet_amd.init import seeded_init_
    from vaeunet_amd.loss import CombinedLoss
    from vaeunet_amd.optim import FusedAdamW, clip_grad_norm_
    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, 3, 64, 64, generator=g).to(DEV)
    t = (torch.rand(2, 1, 64, 64, generator=g) < 0.1).float().to(DEV)
    losses = {}
    for kind in ("torch", "fused"):
        model = seeded_init_(UNet(3, 1), 0).to(DEV).train()
        if kind == "torch":
            opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-5, foreach=True)
            clip = lambda ps: torch.nn.utils.clip_grad_norm_(ps, 1.0, foreach=True)  # noqa: E731
        else:
            opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=1e-5)
            clip = lambda ps: clip_grad_norm_(ps, 1.0)  # noqa: E731
        crit = CombinedLoss()
        out = []
        for _ in range(4):
            loss = crit(model(x), t)
            loss.backward()
            clip(model.parameters())
            opt.step()
            opt.zero_grad(set_to_none=True)
            out.append(float(loss))
        losses[kind] = out
    # step 0 is bitwise the same forward; afterwards ulp-level differences
    # (fp64 vs fp32 clip norm, fma contraction) pass through Adam's
    # sign-like first updates: a stale-weight bug would repeat loss 0 instead
    assert losses["torch"][0] == losses["fused"][0]
    for a, b in zip(losses["torch"][1:], losses["fused"][1:]):
        assert abs(a - b) < 2e-4 * max(1.0, abs(a)), losses
    assert losses["fused"][3] != losses["fused"][0]


# ----------------------------------------------------------------------------
# capturable AdamW (vu_mt_adamw_dev / vu_mt_adamw_dev_scaled), kernel level
# ----------------------------------------------------------------------------
LR, WD, B1, B2, EPS = 1e-3, 1e-2, 0.9, 0.999, 1e-8   # (1 - LR * WD != 1 in fp32: the decay is exercised)
# (numel, param/moment offset, grad offset) in floats past a 16-byte boundary:
# around the 8192-element chunk (tail, exact, one over, several chunks); an
# offset of 1 misaligns the views, which selects the kernel's scalar path
MT_TENSORS = [(1, 0, 0), (3, 0, 0), (8191, 0, 0), (8192, 0, 0), (8193, 0, 0), (9001, 0, 0), (2 * 8192 + 5, 0, 0),
              (3, 1, 1), (8193, 1, 1), (9001, 1, 1), (2 * 8192 + 5, 0, 1)]


def _mt_values(seed=31):
    g = torch.Generator().manual_seed(seed)
    return [dict(p=torch.randn(n, generator=g), m=torch.randn(n, generator=g) * 0.1,
                 v=torch.rand(n, generator=g) * 0.01 + 1e-3) for n, _, _ in MT_TENSORS]


def _mt_grads(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * 0.3 for n, _, _ in MT_TENSORS]


class _MtSet:
    """One replica of the tensor set on the device, every tensor in a guarded
    buffer at its (mis)alignment."""

    def __init__(self, values):
        import ref_small as R
        self.t, self.guards = [], []
        for val, (n, off, goff) in zip(values, MT_TENSORS):
            row = {}
            for key, o in (("p", off), ("g", goff), ("m", off), ("v", off)):
                row[key], gd = R.guarded(n, torch.float32, DEV, offset=o)
                assert row[key].data_ptr() % 16 == (4 * o) % 16
                if key != "g":
                    row[key].copy_(val[key])
                self.guards.append(gd)
            self.t.append(row)
        self.step, gs = R.guarded(1, torch.float32, DEV)
        self.step.zero_()
        self.guards.append(gs)

    def set_grads(self, grads):
        for row, g in zip(self.t, grads):
            row["g"].copy_(g)

    def table(self, step_size=0.0, bc2s=1.0):
        from vaeunet_amd.optim import _Table
        return _Table([(r["p"], r["g"], r["m"], r["v"], step_size, bc2s) for r in self.t], DEV)

    def check(self, what):
        torch.cuda.synchronize()
        for gd in self.guards:
            gd.check(what)

    def same_bits(self, other, what, keys=("p", "m", "v")):
        for i, (a, b) in enumerate(zip(self.t, other.t)):
            for k in keys:
                assert torch.equal(a[k], b[k]), (
                    f"{what}: tensor {i} {MT_TENSORS[i]} '{k}' differs in "
                    f"{int((a[k] != b[k]).sum())} elements, max {float((a[k] - b[k]).abs().max()):.3e}")


def _dev_step(s, zero_grad, scale=None, scaled_entry=False):
    from vaeunet_amd import _lib
    tab = s.table()
    if scaled_entry:
        _lib.call("vu_mt_adamw_dev_scaled", tab.ptr(), tab.n, tab.nchunks, LR, WD, B1, B2, EPS, _lib.ptr(s.step),
                  zero_grad, _lib.ptr(scale), _lib.stream())
    else:
        _lib.call("vu_mt_adamw_dev", tab.ptr(), tab.n, tab.nchunks, LR, WD, B1, B2, EPS, _lib.ptr(s.step),
                  zero_grad, _lib.stream())
    torch.cuda.synchronize()


def test_capturable_adamw_same_bits_as_host_path():
    """Three steps of vu_mt_adamw_dev (device step counter, zero_grad = 0) give
    p / m / v bit-identical to three vu_mt_adamw launches with step_size and
    bc2_sqrt computed on the host as FusedAdamW.step does -- "the same values
    as the host path" -- on the 16-byte and the scalar path and across chunk
    tails; and both are within the eager test's tolerances of an fp64 AdamW on
    the CPU (the independent reference: the identity alone would not catch a
    shared mistake)."""
    import ref_small as R
    from vaeunet_amd import _lib
    vals = _mt_values()
    host, dev = _MtSet(vals), _MtSet(vals)
    ref = [(v["p"].double(), v["m"].double(), v["v"].double()) for v in vals]
    for step in (1, 2, 3):
        grads = _mt_grads(40 + step)
        host.set_grads(grads)
        dev.set_grads(grads)
        bc1, bc2 = 1 - B1 ** float(step), 1 - B2 ** float(step)
        tab = host.table(LR / bc1, bc2 ** 0.5)
        _lib.call("vu_mt_adamw", tab.ptr(), tab.n, tab.nchunks, 1.0 - LR * WD, 1.0 - B1, float(B2), 1.0 - B2,
                  float(EPS), None, _lib.stream())
        _dev_step(dev, 0)
        host.check(f"host step {step}")
        dev.check(f"dev step {step}")
        assert float(dev.step) == float(step)
        dev.same_bits(host, f"step {step}")
        for row, g in zip(dev.t, grads):
            assert torch.equal(row["g"].cpu(), g), "zero_grad = 0 changed a gradient"
        ref = [R.adamw_ref(p, m, v, g, step, LR, WD, B1, B2, EPS) for (p, m, v), g in zip(ref, grads)]
    for row, (p, m, v) in zip(dev.t, ref):
        torch.testing.assert_close(row["p"].double().cpu(), p, rtol=1e-6, atol=1e-9)
        torch.testing.assert_close(row["m"].double().cpu(), m, rtol=1e-6, atol=1e-6 * float(m.abs().max()))
        torch.testing.assert_close(row["v"].double().cpu(), v, rtol=1e-6, atol=1e-6 * float(v.abs().max()))


@pytest.mark.parametrize("coef", [0.37, 1.0, None], ids=["clip", "one", "null"])
def test_capturable_adamw_fused_clip_scale_same_bits(coef):
    """vu_mt_scale_grads(c) then vu_mt_adamw_dev(zero_grad = 1) equals
    vu_mt_adamw_dev_scaled(zero_grad = 1, grad_scale = c) bit for bit (c a
    clip coefficient below 1, c = 1, and grad_scale = NULL against the
    unscaled step); gradients are exactly zero afterwards, the step counter
    has advanced by one, guard regions are untouched."""
    from vaeunet_amd import _lib
    vals = _mt_values()
    two, one = _MtSet(vals), _MtSet(vals)
    grads = _mt_grads(50)
    two.set_grads(grads)
    one.set_grads(grads)
    c = None if coef is None else torch.tensor([coef], dtype=torch.float32, device=DEV)
    if c is not None:
        tab = two.table()
        _lib.call("vu_mt_scale_grads", tab.ptr(), tab.n, tab.nchunks, _lib.ptr(c), _lib.stream())
        torch.cuda.synchronize()
        for row, g in zip(two.t, grads):
            assert torch.equal(row["g"].cpu(), g * torch.tensor(coef, dtype=torch.float32))
    _dev_step(two, 1)
    _dev_step(one, 1, scale=c, scaled_entry=True)
    two.check("scale + step")
    one.check("fused scale step")
    one.same_bits(two, f"grad_scale {coef}")
    for s in (one, two):
        assert float(s.step) == 1.0
        for row in s.t:
            assert not row["g"].any(), "gradient not cleared"
    # and the step moved the parameters at all
    assert all(not torch.equal(r["p"].cpu(), v["p"]) for r, v in zip(one.t, vals))


def test_capturable_adamw_scaled_refuses_keeping_grads():
    """grad_scale with zero_grad = 0 is refused (the scaled gradient is never
    stored), and nothing is touched."""
    vals = _mt_values()
    s = _MtSet(vals)
    grads = _mt_grads(60)
    s.set_grads(grads)
    c = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError):
        _dev_step(s, 0, scale=c, scaled_entry=True)
    s.check("refused")
    assert float(s.step) == 0.0
    for row, v, g in zip(s.t, vals, grads):
        assert torch.equal(row["p"].cpu(), v["p"]) and torch.equal(row["g"].cpu(), g)
