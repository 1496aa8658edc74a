"""Time of the device-side CLAHE and separable blur of one batch,
image 8x3x512x512 fp32 channels_last (mask 8x1x512x512 for the vu_augment_patch rows):
  (c)  CLAHE, 8 x 8 tiles, clip 2: vu_clahe_luts + vu_clahe_apply (c1 / c2: each launch alone)
  (b0) vu_blur_sep at r = 0 (the copy), (b1) (b3) (b7) at r = 1, 3, 7 (box rows)
  (t1) (t3) (t7) the same blur composed from torch ops: reflect pad + depthwise conv2d, per axis
  (p)  the three stages: CLAHE -> blur r = 3 -> vu_augment_patch with identity parameters
  (a0) vu_augment_patch with identity parameters alone: the streaming yardstick of §4.8
  (m1) (m2) (m3) vu_median_blur at r = 1, 2, 3; (b0) copies the same bytes
  (tm) the r = 3 median composed from torch ops: replicate pad + unfold + median over the 49 taps, on ONE sample
       (1x3x512x512: the unfolded batch would be 1.2 GB), 1 / 50 of the iterations; compare 8 x its time
  (pm) the four stages: CLAHE -> blur r = 3 -> median r = 3 -> vu_augment_patch with identity parameters
Two figures per variant, both stream time per batch between hip events around
`iters` back-to-back runs, `rounds` times with the variants alternating:
`eager` (Python and the launches included) and `graph` (captured with
torch.cuda.graph and replayed: the device's share).  Every table is on the
device before the timed window.  GB/s = useful bytes / graph time, with useful
bytes = the image read twice and written once for CLAHE (75.5 MB), read and
written once for the blur (50.3 MB), image and mask read and written once for
(a0) (67.1 MB), and the sum of its stages for (p).
usage: python tools/filters_bench.py [--iters 500] [--rounds 5]"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vaeunet_amd.data as D  # noqa: E402
from vaeunet_amd import kernels as K  # noqa: E402

B, H, W = 8, 512, 512
TILES = (8, 8)


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


def torch_blur(img, kh, kv, r):
    """reflect pad + depthwise conv2d along W, then along H; kh [3, 1, 1, 2r+1], kv [3, 1, 2r+1, 1]"""
    v = F.conv2d(F.pad(img, (r, r, 0, 0), mode="reflect"), kh, groups=3)
    return F.conv2d(F.pad(v, (0, 0, r, r), mode="reflect"), kv, groups=3)


def torch_median(img, r):
    """replicate pad + unfold of the (2r + 1)^2 taps + median over them (odd count: the middle element)"""
    k = 2 * r + 1
    n, c, h, w = img.shape
    taps = F.unfold(F.pad(img, (r, r, r, r), mode="replicate"), k).view(n, c, k * k, h, w)
    return taps.median(dim=2).values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    img = (torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255).to(dev).contiguous(
        memory_format=torch.channels_last)
    msk = (torch.rand(B, 1, H, W, generator=g) < 0.03).float().to(dev).contiguous(memory_format=torch.channels_last)
    clip = torch.full((B,), 2.0, device=dev)
    luts = torch.empty((B, *TILES, 256), dtype=torch.uint8, device=dev)
    out = torch.empty_like(img)
    rows = {r: D.blur_weights(box=2 * r + 1) for r in (0, 1, 3, 7)}
    tabs = {r: torch.from_numpy(np.tile(row, (B, 1))).to(dev) for r, row in rows.items()}
    kern = {}
    for r in (1, 3, 7):
        # w_r..w_1 w_0 w_1..w_r
        full = torch.from_numpy(np.concatenate([rows[r][1 + r:1:-1], rows[r][1:2 + r]])).to(dev)
        kern[r] = (full.view(1, 1, 1, -1).repeat(3, 1, 1, 1).contiguous(),
                   full.view(1, 1, -1, 1).repeat(3, 1, 1, 1).contiguous())
    ip, ikx, iky = (torch.from_numpy(t).to(dev) for t in (D.identity_params(B), D.identity_knots(B, W),
                                                          D.identity_knots(B, H)))

    def luts_only():
        K.call("vu_clahe_luts", K.ptr(img), B, H, W, K.ptr(clip), *TILES, K.ptr(luts), K.stream())

    def apply_only():
        K.call("vu_clahe_apply", K.ptr(img), B, H, W, K.ptr(clip), *TILES, K.ptr(luts), K.ptr(out), K.stream())

    mrad = {r: torch.full((B,), float(r), device=dev) for r in (1, 2, 3)}
    one = img[:1].contiguous()          # NCHW: what unfold wants

    def pipeline_median():
        v = D._launch_median(D._launch_blur(D._launch_clahe(img, clip, TILES), tabs[3]), mrad[3])
        return D._launch_augment(v, msk, ip, ikx, iky, 1, 0, 1)

    def pipeline():
        v = D._launch_blur(D._launch_clahe(img, clip, TILES), tabs[3])
        return D._launch_augment(v, msk, ip, ikx, iky, 1, 0, 1)

    nimg = 12 * B * H * W
    variants = [("c  CLAHE: luts + apply                  ", lambda: D._launch_clahe(img, clip, TILES), 3 * nimg),
                ("c1 vu_clahe_luts alone                  ", luts_only, nimg),
                ("c2 vu_clahe_apply alone                 ", apply_only, 2 * nimg),
                ("b0 vu_blur_sep r = 0 (copy)             ", lambda: D._launch_blur(img, tabs[0]), 2 * nimg),
                ("b1 vu_blur_sep r = 1                    ", lambda: D._launch_blur(img, tabs[1]), 2 * nimg),
                ("b3 vu_blur_sep r = 3                    ", lambda: D._launch_blur(img, tabs[3]), 2 * nimg),
                ("b7 vu_blur_sep r = 7                    ", lambda: D._launch_blur(img, tabs[7]), 2 * nimg),
                ("t1 torch pad + depthwise conv2d, r = 1  ", lambda: torch_blur(img, *kern[1], 1), 2 * nimg),
                ("t3 torch pad + depthwise conv2d, r = 3  ", lambda: torch_blur(img, *kern[3], 3), 2 * nimg),
                ("t7 torch pad + depthwise conv2d, r = 7  ", lambda: torch_blur(img, *kern[7], 7), 2 * nimg),
                ("p  CLAHE -> blur r = 3 -> augment (ident)", pipeline, 5 * nimg + 32 * B * H * W),
                ("a0 vu_augment_patch, identity params    ", lambda: D._launch_augment(img, msk, ip, ikx, iky, 1, 0, 1),
                 32 * B * H * W),
                ("m1 vu_median_blur r = 1                 ", lambda: D._launch_median(img, mrad[1]), 2 * nimg),
                ("m2 vu_median_blur r = 2                 ", lambda: D._launch_median(img, mrad[2]), 2 * nimg),
                ("m3 vu_median_blur r = 3                 ", lambda: D._launch_median(img, mrad[3]), 2 * nimg),
                ("tm torch pad + unfold + median, r = 3, 1 sample", lambda: torch_median(one, 3), 2 * nimg // B),
                ("pm CLAHE -> blur 3 -> median 3 -> augment", pipeline_median, 7 * nimg + 32 * B * H * W)]
    slow = {"tm torch pad + unfold + median, r = 3, 1 sample": 50}     # name -> divisor of --iters
    same = torch.equal(D._launch_median(img[:1], mrad[3][:1]), torch_median(one, 3).contiguous(
        memory_format=torch.channels_last))
    print(f"vu_median_blur vs the torch composition at r = 3 (one sample): {'bitwise equal' if same else 'DIFFERENT'}",
          flush=True)
    # the two blurs are the same filter: compare them once
    for r in (1, 3, 7):
        d = float((D._launch_blur(img, tabs[r]) - torch_blur(img, *kern[r], r)).abs().max())
        print(f"vu_blur_sep vs the torch composition at r = {r}: max |difference| {d:.2e}", flush=True)
    ce = D._launch_clahe(img, clip, TILES)
    print(f"CLAHE: mean |change| {float((ce - img).abs().mean()):.4f}, output range [{float(ce.min()):.3f}, "
          f"{float(ce.max()):.3f}]", flush=True)
    for _, fn, _ in variants:                   # warm-up: code objects, allocator, conv algorithms
        for _ in range(3):
            fn()
    replays = [captured(fn) for _, fn, _ in variants]
    times = {name: [] for name, _, _ in variants}
    gtimes = {name: [] for name, _, _ in variants}
    for _ in range(a.rounds):
        for (name, fn, _), rep in zip(variants, replays):
            n = max(1, a.iters // slow.get(name, 1))
            times[name].append(stream_us(fn, n))
            gtimes[name].append(stream_us(rep, n))
    print(f"image {B}x3x{H}x{W} ({nimg / 1e6:.1f} MB)  ({a.iters} batches per figure, {a.rounds} rounds)", flush=True)
    for name, _, nbytes in variants:
        v, w = sorted(times[name]), sorted(gtimes[name])
        med = w[len(w) // 2]
        print(f"  {name}: eager median {v[len(v) // 2]:8.1f} us (min {v[0]:8.1f})   graph median {med:8.1f} us "
              f"(min {w[0]:8.1f}, max {w[-1]:8.1f})  {nbytes / 1e6:6.1f} MB {nbytes / med / 1e3:7.1f} GB/s", flush=True)


if __name__ == "__main__":
    main()
