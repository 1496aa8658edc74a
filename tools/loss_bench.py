"""Forward + backward time of the segmentation objectives on fp32 logits and a
0/1 fp32 target (3 % positives, the logits N(-4, 4): mostly easy pixels) at
8x1x512x512 and 8x2x512x512:
  (a) MASegmentationLoss        the fused focal + Dice kernels (csrc/focal.hip): 2 + 1 launches
  (b) the same loss in torch ops   softplus / expm1 / sigmoid / sums and autograd, no .item()
  (c) CombinedLoss              BCE + Dice (csrc/loss.hip) on the same tensors
  (a0/a1/a25) MASegmentationLoss with gamma = 0, 1 and 2.5 (the general-exponent path)
Two figures per variant, both stream time per forward + backward between hip
events around `iters` back-to-back runs, `rounds` times with the variants
alternating: `eager` (Python, autograd and the launches included: at these
sizes the host is the limit) and `graph` (one forward + backward captured
with torch.cuda.graph and replayed: the device's share, what a
GraphedTrainStep pays).  GB/s = (logits + target read twice, gradient
written: 20 B per element) / graph time.
usage: python tools/loss_bench.py [--iters 50] [--rounds 5]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaeunet_amd.loss import CombinedLoss, MASegmentationLoss  # noqa: E402

SHAPES = [(8, 1, 512, 512), (8, 2, 512, 512)]


def torch_focal_dice(x, t, alpha=0.75, gamma=2.0, smooth=1.0, wf=0.5, wd=0.5):
    """DESIGN.md §4.7 composed from torch ops (NaN -> 0 as a select: no host sync)."""
    ax = x.abs()
    lg = torch.log1p(torch.exp(-ax))
    b = t * (torch.relu(-x) + lg) + (1 - t) * (torch.relu(x) + lg)
    omq = -torch.expm1(-b)
    at = alpha * t + (1 - alpha) * (1 - t)
    f = at * omq ** gamma * b
    focal = torch.where(torch.isnan(f), 0.0, f).mean()
    p = torch.sigmoid(x)
    p = torch.where(torch.isnan(p), 0.0, p)
    inter, sp, st = (p * t).sum(), p.sum(), t.sum()
    dice = (2 * inter + smooth) / (sp.clamp_min(smooth / 2) + st.clamp_min(smooth / 2) + smooth)
    return wf * focal + wd * (1 - dice)


def stream_us(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def captured(fn):
    """fn captured into a graph after a warm-up on a side stream -> replay()"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    for shape in SHAPES:
        g = torch.Generator().manual_seed(0)
        x = (torch.randn(*shape, generator=g) * 2.0 - 4.0).to(dev).requires_grad_(True)
        t = (torch.rand(*shape, generator=g) < 0.03).float().to(dev)

        def fwd_bwd(crit):
            def run():
                x.grad = None
                crit(x, t).backward()
            return run
        variants = [("a   MASegmentationLoss (fused)     ", fwd_bwd(MASegmentationLoss())),
                    ("b   the same loss in torch ops     ", fwd_bwd(torch_focal_dice)),
                    ("c   CombinedLoss (BCE + Dice)      ", fwd_bwd(CombinedLoss())),
                    ("a0  MASegmentationLoss, gamma = 0  ", fwd_bwd(MASegmentationLoss(gamma=0.0))),
                    ("a1  MASegmentationLoss, gamma = 1  ", fwd_bwd(MASegmentationLoss(gamma=1.0))),
                    ("a25 MASegmentationLoss, gamma = 2.5", fwd_bwd(MASegmentationLoss(gamma=2.5)))]
        # the fused and the composed loss are the same number
        with torch.no_grad():
            la, lb = float(MASegmentationLoss()(x, t)), float(torch_focal_dice(x, t))
        assert abs(la - lb) <= 1e-5 * abs(lb), (la, lb)
        for _, fn in variants:                      # warm-up: code objects, allocator
            for _ in range(3):
                fn()
        replays = [(name, captured(fn)) for name, fn in variants]
        times = {name: [] for name, _ in variants}
        gtimes = {name: [] for name, _ in variants}
        for _ in range(a.rounds):
            for (name, fn), (_, rep) in zip(variants, replays):
                times[name].append(stream_us(fn, a.iters))
                gtimes[name].append(stream_us(rep, a.iters))
        nbytes = 20 * x.numel()
        print(f"shape {'x'.join(map(str, shape))}  ({a.iters} forward + backward per figure, {a.rounds} rounds, "
              f"{nbytes / 1e6:.1f} MB per call)", flush=True)
        for name, _ in variants:
            v, w = sorted(times[name]), sorted(gtimes[name])
            med = w[len(w) // 2]
            print(f"  {name}: eager median {v[len(v) // 2]:8.1f} us (min {v[0]:8.1f})   graph median {med:8.1f} us "
                  f"(min {w[0]:8.1f}, max {w[-1]:8.1f})  {nbytes / med / 1e3:7.1f} GB/s", flush=True)


if __name__ == "__main__":
    main()
