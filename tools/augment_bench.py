"""Time of the device-side training augmentation of one batch, image 8x3x512x512
and mask 8x1x512x512 (fp32, channels_last):
  (a) vu_augment_patch, every transform on: flips / rot90 / +-15 deg affine, a 5-step grid
      distortion at limit 0.3, gamma, a colour matrix, Gaussian noise, reflect101 border: ONE launch
      (a1: without the noise; a2: geometry only; a0: identity parameters, i.e. the gamma and noise branches
      skipped and every tap on its own pixel: what each part of the launch costs)
  (b) today's flip / rot90 path: two vu_gather_affine launches (image, mask)
  (c) the pipeline of (a) without the grid distortion composed from torch ops: affine_grid, grid_sample
      (bilinear image, nearest mask, reflection padding), pow, a 1x1 matmul, randn, clamp
Two figures per variant, both stream time per batch between hip events around
`iters` back-to-back runs, `rounds` times with the variants alternating:
`eager` (Python and the launches included) and `graph` (captured with
torch.cuda.graph and replayed: the device's share).  The parameter tables are
on the device before the timed window ((a) through PatchCache adds one small
host-to-device copy per batch).  GB/s = (image and mask read once and written
once: 32 B per pixel) / graph time.
usage: python tools/augment_bench.py [--iters 500] [--rounds 5]"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vaeunet_amd.data as D  # noqa: E402
from vaeunet_amd import kernels as K  # noqa: E402
from vaeunet_amd._lib import F32  # noqa: E402

B, H, W = 8, 512, 512


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


def torch_pipeline(img, msk, theta, gamma, M, o, sigma):
    """(c): theta [B, 2, 3] normalised output -> source maps, M [B, 3, 3], o / gamma / sigma [B, ...]"""
    grid = F.affine_grid(theta, list(img.shape), align_corners=True)
    v = F.grid_sample(img, grid, mode="bilinear", padding_mode="reflection", align_corners=True)
    m = F.grid_sample(msk, grid, mode="nearest", padding_mode="reflection", align_corners=True)
    v = v.clamp_min(0).pow(gamma)
    v = torch.einsum("bij,bjhw->bihw", M, v) + o
    v = v + sigma * torch.randn_like(v)
    return v.clamp(0, 1), m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    img = torch.rand(B, 3, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    msk = (torch.rand(B, 1, H, W, generator=g) < 0.03).float().to(dev).contiguous(memory_format=torch.channels_last)
    aug = D.TrainAugment(p_hflip=0.5, p_vflip=0.5, p_rot90=0.5, p_affine=1.0, p_grid=1.0, p_gamma=1.0, p_colour=1.0,
                         p_noise=1.0)
    rng = np.random.Generator(np.random.PCG64(0))
    params, gx, gy = aug.draw(B, H, W, rng)
    dp, dgx, dgy = (torch.from_numpy(t).to(dev) for t in (params, gx, gy))
    ip, ikx, iky = (torch.from_numpy(t).to(dev) for t in (D.identity_params(B), D.identity_knots(B, W),
                                                          D.identity_knots(B, H)))
    flags = [(b & 1, (b >> 1) & 1, b % 4) for b in range(B)]
    fmap = torch.tensor([D._flip_rot_map(H, *f) for f in flags], dtype=torch.int32).to(dev)
    # (c): pixel-space a0..a5 -> affine_grid's normalised [-1, 1] coordinates (align_corners=True)
    A = params[:, :6].astype(np.float64).reshape(B, 2, 3)
    sx, sy = (W - 1) / 2.0, (H - 1) / 2.0
    theta = np.empty((B, 2, 3))
    theta[:, 0, 0], theta[:, 0, 1] = A[:, 0, 0], A[:, 0, 1] * sy / sx
    theta[:, 1, 0], theta[:, 1, 1] = A[:, 1, 0] * sx / sy, A[:, 1, 1]
    theta[:, 0, 2] = (A[:, 0, 0] * sx + A[:, 0, 1] * sy + A[:, 0, 2]) / sx - 1
    theta[:, 1, 2] = (A[:, 1, 0] * sx + A[:, 1, 1] * sy + A[:, 1, 2]) / sy - 1
    theta = torch.from_numpy(theta).float().to(dev)
    gam = dp[:, 6].view(B, 1, 1, 1).contiguous()
    M, o = dp[:, 7:16].reshape(B, 3, 3).contiguous(), dp[:, 16:19].reshape(B, 3, 1, 1).contiguous()
    sig = dp[:, 19].view(B, 1, 1, 1).contiguous()

    def gather2():
        for t in (img, msk):
            out = K.empty_act(B, t.shape[1], H, W, torch.float32, dev)
            K.call("vu_gather_affine", K.ptr(t), B, H, W, t.shape[1], K.ptr(fmap), K.ptr(out), H, W, F32, K.stream())

    # (a1), (a2): the parameters of (a) with the noise, then also gamma and colour, switched off
    p1, p2 = params.copy(), params.copy()
    p1[:, 19] = 0
    p2[:, 6:] = D.identity_params(B)[:, 6:]
    dp1, dp2 = torch.from_numpy(p1).to(dev), torch.from_numpy(p2).to(dev)
    variants = [("a  vu_augment_patch, every transform   ", lambda: D._launch_augment(img, msk, dp, dgx, dgy, 1, 0, 1)),
                ("a1 the same without noise              ", lambda: D._launch_augment(img, msk, dp1, dgx, dgy, 1, 0, 1)),
                ("a2 the same, geometry only             ", lambda: D._launch_augment(img, msk, dp2, dgx, dgy, 1, 0, 1)),
                ("a0 vu_augment_patch, identity params   ", lambda: D._launch_augment(img, msk, ip, ikx, iky, 1, 0, 1)),
                ("b  2 x vu_gather_affine (flip / rot90)  ", gather2),
                ("c  torch ops (no grid distortion)      ", lambda: torch_pipeline(img, msk, theta, gam, M, o, sig))]
    # (a) and (c) are the same warp where no grid distortion is set: compare them once on the geometry alone
    geo = D.identity_params(B)
    geo[:, :6] = params[:, :6]
    ai, am = D.augment_patches(img, msk, geo, D.identity_knots(B, W), D.identity_knots(B, H), seed=0)
    one = torch.ones(B, 1, 1, 1, device=dev)
    ci, cm = torch_pipeline(img, msk, theta, one, torch.eye(3, device=dev).expand(B, 3, 3).contiguous(),
                            torch.zeros(B, 3, 1, 1, device=dev), 0 * one)
    print(f"geometry of (a) vs (c): max |image difference| {float((ai - ci).abs().max()):.2e}, "
          f"mask pixels that differ {int((am != cm).sum())} of {am.numel()}", flush=True)
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
    nbytes = 32 * B * H * W
    print(f"image {B}x3x{H}x{W} + mask {B}x1x{H}x{W}  ({a.iters} batches per figure, {a.rounds} rounds, "
          f"{nbytes / 1e6:.1f} MB per batch)", flush=True)
    for name, _ in variants:
        v, w = sorted(times[name]), sorted(gtimes[name])
        med = w[len(w) // 2]
        print(f"  {name}: eager median {v[len(v) // 2]:8.1f} us (min {v[0]:8.1f})   graph median {med:8.1f} us "
              f"(min {w[0]:8.1f}, max {w[-1]:8.1f})  {nbytes / med / 1e3:7.1f} GB/s", flush=True)


if __name__ == "__main__":
    main()
