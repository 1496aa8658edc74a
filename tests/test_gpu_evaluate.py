"""vaeunet_amd.evaluate.evaluate(): the validation loop against the same
numbers computed the long way -- the same model forward (inference mode, bf16
autocast), the logits moved to the CPU, F.interpolate in fp64, ``> 0.5``,
integer sums, and the metric formulas in numpy.

The logits are the same tensor on both sides, so the only arithmetic that can
differ is the interpolation (fp32 in the kernel, fp64 here): the tests assert
that no fp64-interpolated logit lies within 1e-4 of the threshold, >30x the
fp32 evaluation-order error, and then demand exact counts -- which makes dice
and pooled_dice bit-exact and the fp64-formed metrics exact to 1 ulp."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from vaeunet_amd.evaluate import evaluate
from vaeunet_amd.metrics import METRIC_NAMES

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
EPS = 1e-6
DATA_SEED = 0


def ref_row(k, eps=EPS):
    tp, fp, fn, tn = (int(v) for v in k)
    a, b = tp + fp, tp + fn
    f = np.float32
    dice = f(1.0) if a + b == 0 else (f(2.0) * f(tp) + f(eps)) / (f(a) + f(b) + f(eps))
    TP, FP, FN, TN = (np.float64(v) for v in (tp, fp, fn, tn))
    rest = [(TP + eps) / (TP + FP + FN + eps), (TP + eps) / (TP + FP + eps), (TP + eps) / (TP + FN + eps),
            (TN + eps) / (TN + FP + eps), (TP + TN) / (TP + FP + FN + TN)]
    return np.array([dice] + [f(v) for v in rest], dtype=np.float32)


def counts_cpu(logits, mask, align_corners=False):
    """pooled (TP, FP, FN, TN) of one batch + the distance of the closest resized logit to the threshold"""
    v = logits.detach().float().cpu().double()
    if v.shape[2:] != mask.shape[2:]:
        v = F.interpolate(v, size=tuple(mask.shape[2:]), mode="bilinear", align_corners=align_corners)
    p, t = v > 0.5, mask.double() > 0.5
    k = torch.stack([(p & t).sum(), (p & ~t).sum(), (~p & t).sum(), (~p & ~t).sum()])
    return k, float((v - 0.5).abs().min())


@functools.lru_cache(maxsize=None)
def tiny_unet(sharp=False):
    """UNet(3, 1), seeded init.  Its logits on uniform-noise images all lie in [-0.034, -0.005] (nothing is
    predicted); ``sharp`` rescales the last 1x1 conv so that logits' = 1000 * (logits + 0.0125) + 0.5: both
    predictions occur and |logits'| stays below ~25, where one fp32 rounding is < 2e-6"""
    from vaeunet_amd import UNet
    from vaeunet_amd.init import seeded_init_
    net = seeded_init_(UNet(3, 1), 0)
    if sharp:
        with torch.no_grad():
            net.outc.conv.weight.mul_(1000.0)
            net.outc.conv.bias.mul_(1000.0).add_(13.0)
    return net.to(DEV).to(memory_format=CL).eval()


def make_batches(mask_hw, squeeze=False, seed=DATA_SEED):
    """two batches of 2 images at 64x64 (the size of the tiny goldens); Bernoulli(0.3) masks at mask_hw"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        image = torch.rand(2, 3, 64, 64, generator=g)
        mask = (torch.rand(2, 1, *mask_hw, generator=g) < 0.3).float()
        out.append((image, mask[:, 0] if squeeze else mask))
    return out


def long_way(net, batches, align_corners=False, amp=True):
    net.eval()
    rows, total, margin = [], torch.zeros(4, dtype=torch.int64), float("inf")
    for image, mask in batches:
        with torch.inference_mode(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            out = net(image.to(DEV).contiguous(memory_format=CL))
        logits = out[0] if isinstance(out, tuple) else out
        if mask.dim() == 3:
            mask = mask.unsqueeze(1)
        k, d = counts_cpu(logits, mask, align_corners)
        margin = min(margin, d)
        rows.append(ref_row(k))
        total += k
    f = np.float32
    mean = rows[0].copy()
    for r in rows[1:]:
        mean = (mean + r).astype(f)          # the meter's fp32 running sum
    mean = (mean / f(len(rows))).astype(f)
    return mean, ref_row(total), total, margin


def check(res, mean, pooled, nbatches):
    assert set(res) == set(METRIC_NAMES) | {f"pooled_{k}" for k in METRIC_NAMES} | {"batches"}
    assert res["batches"] == nbatches
    assert all(isinstance(res[k], float) for k in METRIC_NAMES)
    assert res["dice"] == float(mean[0]), (res["dice"], mean[0])
    assert res["pooled_dice"] == float(pooled[0]), (res["pooled_dice"], pooled[0])
    for i, k in enumerate(METRIC_NAMES[1:], 1):
        # formed from exact integers in fp64 and rounded once; the mean is the same fp32 sum on both sides
        assert abs(res[f"pooled_{k}"] - np.float64(pooled[i])) <= np.spacing(pooled[i]), (k, res[f"pooled_{k}"])
        assert abs(res[k] - np.float64(mean[i])) <= np.spacing(mean[i]), (k, res[k], mean[i])


@pytest.mark.parametrize("sharp", [False, True], ids=["seeded", "sharp"])
@pytest.mark.parametrize("mask_hw", [(64, 64), (96, 96)], ids=["same", "resize"])
def test_evaluate_matches_the_long_way(mask_hw, sharp):
    net = tiny_unet(sharp)
    # the data seed is chosen so that the no-near-tie precondition holds: a property of the fp64 reference
    # values alone (about half of the seeds qualify for the sharp net: ~37k resized logits, density ~0.1 per
    # unit at the threshold)
    for seed in range(DATA_SEED, DATA_SEED + 24):
        batches = make_batches(mask_hw, seed=seed)
        mean, pooled, total, margin = long_way(net, batches)
        if mask_hw == (64, 64) or margin > 1e-4:
            break
    if mask_hw != (64, 64):
        assert margin > 1e-4, margin           # no near tie: the counts must then be exact
    if sharp:
        assert int(total[0] + total[1]) > 0 and int(total[2] + total[3]) > 0, total   # both predictions occur
    loader = [{"image": im, "mask": m} for im, m in batches]
    res = evaluate(net, loader, torch.device(DEV))
    check(res, mean, pooled, 2)
    # (image, mask) pairs, masks without a channel dimension, max_batches
    res2 = evaluate(net, make_batches(mask_hw, squeeze=True, seed=seed), DEV)
    assert res2 == res
    res1 = evaluate(net, loader, DEV, max_batches=1)
    mean1, pooled1, _, _ = long_way(net, batches[:1])
    check(res1, mean1, pooled1, 1)


def test_evaluate_restores_the_training_mode():
    net = tiny_unet()
    batches = make_batches((64, 64))[:1]
    try:
        net.train()
        evaluate(net, batches, DEV)
        assert net.training and all(m.training for m in net.modules())
        net.eval()
        evaluate(net, batches, DEV)
        assert not net.training and not any(m.training for m in net.modules())

        class Boom(Exception):
            pass

        def loader():
            yield batches[0]
            raise Boom

        net.train()
        with pytest.raises(Boom):
            evaluate(net, loader(), DEV)
        assert net.training
    finally:
        net.eval()


class _VaeStub(nn.Module):
    """returns (logits, mu, logvar) like the VAE U-Net; logits at half resolution, two classes"""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.tensor([[9.0, -12.0, 4.0], [-5.0, 7.0, 6.0]]))

    def forward(self, x):
        z = x.float()[:, :, ::2, ::2]
        logits = torch.einsum("kc,bchw->bkhw", self.w, z) - 0.5
        mu = z.mean((2, 3))
        return logits, mu, torch.zeros_like(mu)


def test_evaluate_accepts_a_vae_net():
    net = _VaeStub().to(DEV)
    g = torch.Generator().manual_seed(8)   # closest resized logit 1.8e-3 (4.1e-3 aligned) from the threshold
    batches = [(torch.rand(2, 3, 16, 16, generator=g), (torch.rand(2, 2, 16, 16, generator=g) < 0.4).to(torch.uint8))
               for _ in range(3)]
    for ac in (False, True):
        mean, pooled, total, margin = long_way(net, batches, align_corners=ac, amp=False)
        assert margin > 1e-4, margin
        assert int(total[0] + total[1]) > 0 and int(total[2] + total[3]) > 0, total
        check_res = evaluate(net, batches, DEV, amp=False, align_corners=ac)
        assert check_res["batches"] == 3
        assert check_res["pooled_dice"] == float(pooled[0])
        for i, k in enumerate(METRIC_NAMES[1:], 1):
            assert abs(check_res[f"pooled_{k}"] - np.float64(pooled[i])) <= np.spacing(pooled[i]), k
