"""Per-call time of one validation batch's metrics at the flagship shapes
(8x1x512^2 and 8x2x512^2, fp32 channels_last logits, fp32 masks):
  (a) SegmentationMeter.update      one counts pass + stage 2 + one metrics launch
  (b) metrics.dice_score            one metric from the same bytes
  (c) the six metrics in torch ops  threshold, products, sums, divisions (no .item())
Each figure is stream time per call (hip events around `iters` back-to-back
calls, so it includes the launch gaps a validation loop pays), `rounds` times
with the three variants alternating; GB/s = (logit + mask bytes) / time.
usage: python tools/metrics_bench.py [--iters 100] [--rounds 5]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaeunet_amd import metrics as M  # noqa: E402

CL = torch.channels_last
SHAPES = [(8, 1, 512, 512), (8, 2, 512, 512)]


def torch_metrics(x, t, eps=1e-6):
    p = x > 0.5
    g = t > 0.5
    tp = (p & g).sum().double()
    fp = (p & ~g).sum().double()
    fn = (~p & g).sum().double()
    tn = (~p & ~g).sum().double()
    return ((2 * tp + eps) / (2 * tp + fp + fn + eps), (tp + eps) / (tp + fp + fn + eps),
            (tp + eps) / (tp + fp + eps), (tp + eps) / (tp + fn + eps), (tn + eps) / (tn + fp + eps),
            (tp + tn) / (tp + fp + fn + tn))


def stream_us(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    for shape in SHAPES:
        x = (torch.randn(*shape, generator=g) * 3).to(dev).contiguous(memory_format=CL)
        t = (torch.rand(*shape, generator=g) < 0.3).float().to(dev).contiguous(memory_format=CL)
        t8 = t.to(torch.uint8)
        xb = x.bfloat16()
        meter = M.SegmentationMeter()
        variants = [
            ("a  meter.update fp32 logits, fp32 mask", lambda: meter.update(x, t), x.nbytes + t.nbytes),
            ("b  dice_score   fp32 logits, fp32 mask", lambda: M.dice_score(x, t), x.nbytes + t.nbytes),
            ("c  six metrics in torch ops           ", lambda: torch_metrics(x, t), x.nbytes + t.nbytes),
            ("a' meter.update bf16 logits, u8 mask  ", lambda: meter.update(xb, t8), xb.nbytes + t8.nbytes),
        ]
        for _, fn, _ in variants:                      # warm-up: code objects, allocator
            for _ in range(10):
                fn()
        times = {name: [] for name, _, _ in variants}
        for _ in range(a.rounds):
            for name, fn, _ in variants:
                times[name].append(stream_us(fn, a.iters))
        print(f"shape {'x'.join(map(str, shape))}  ({a.iters} calls per figure, {a.rounds} rounds)", flush=True)
        for name, _, nbytes in variants:
            v = sorted(times[name])
            med = v[len(v) // 2]
            print(f"  {name}: median {med:8.1f} us  min {v[0]:8.1f}  max {v[-1]:8.1f}   "
                  f"{nbytes / med / 1e3:8.1f} GB/s", flush=True)


if __name__ == "__main__":
    main()
