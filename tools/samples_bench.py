"""Time of the sample-set metrics: S = 32 float32 samples
against M = 1 uint8 ground truth, about 0.15 % foreground, the samples being
perturbations of one mask (the probabilities of the pixels near its boundary
cross the threshold in some samples and not in others).
  workloads   one 2848 x 4288 plane (the samples are 1.56 GB), and one
              8 x 1 x 512 x 512 batch
  (g)  sample_gram: the zeroing memset and the one streaming launch
  (u)  SampleSetMeter.update: (g), vu_sampleset_metrics and the running sum
  (a)  what a user writes today, the pair loop: threshold once, then
       (a & b).sum() for the K (K + 1) / 2 pairs, stacked on the device
  (b)  the other way: threshold, .float(), B @ B.T -- a second stack, and
       counts in fp32, exact only while every count stays below 2^24
  (c)  a device copy of the sample stack (dst.copy_(src)): the rate this
       device reaches on a plain stream, the yardstick of (g)'s share
Device figures: stream time per call between hip events around `iters`
back-to-back calls (`base-iters` for the baselines), `rounds` times with the
variants alternating, after a warm-up; median, min and max over the rounds.
Bytes: (g) and (u) have to read every sample and truth element once, S n 4 + M n
bytes; (a) and (b) are charged the same bytes (what the task needs, not what
they move); (c) reads and writes the stack.  The device Gram matrix is compared
with both baselines once, where they are exact.  The lines are printed and
written to --out.
usage: python tools/samples_bench.py [--iters 50] [--base-iters 3] [--rounds 5] [--out profiles/samples_bench.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vaeunet_amd import samples as SM  # noqa: E402

S, M, THR = 32, 1, 0.5
HBM_PEAK = 8.0e12    # HBM3E datasheet peak of the MI355X, bytes / s


def base_map(B, H, W, seed=0):
    """float32 [B, 1, H, W]: discs of radius 2..6 covering about 0.15 % of the plane with probabilities 0.45..1,
    background below 0.3"""
    rng = np.random.Generator(np.random.PCG64(seed))
    prob = (rng.random((B, 1, H, W), dtype=np.float32) * np.float32(0.3)).astype(np.float32)
    discs = max(1, int(0.0015 * H * W / 55))          # mean disc area: about 55 pixels
    for b in range(B):
        for _ in range(discs):
            cy, cx, r = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(2, 7))
            y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
            yy, xx = np.mgrid[y0:y1, x0:x1]
            m = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
            prob[b, 0, y0:y1, x0:x1][m] = np.float32(0.45 + 0.55 * rng.random())
    return prob


def workload(B, H, W, dev):
    """samples float32 [S, B, 1, H, W]: the base map plus uniform noise in (-0.12, 0.12) per sample; truth uint8
    [B, 1, H, W]: the base map above 0.55"""
    base = torch.from_numpy(base_map(B, H, W)).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    samples = torch.empty((S, B, 1, H, W), dtype=torch.float32, device=dev)
    for k in range(S):
        samples[k] = base + (torch.rand(base.shape, generator=g, device=dev) - 0.5) * 0.24
    return samples, (base > 0.55).to(torch.uint8)


def pair_loop(samples, truth):
    """(a) -> int64 [B, 1, K, K]"""
    cols = list(samples > THR) + [truth != 0]
    K = len(cols)
    rows = []
    for i in range(K):
        row = []
        for j in range(K):
            row.append((cols[i] & cols[j]).sum(dim=(-2, -1)) if j >= i else rows[j][i])
        rows.append(row)
    return torch.stack([torch.stack(r, -1) for r in rows], -2)


def float_matmul(samples, truth):
    """(b) -> fp32 [B, 1, K, K]"""
    Bn = samples.shape[1]
    cols = torch.cat([(samples > THR).float(), (truth != 0).float()[None]])      # [K, B, 1, H, W]: the second stack
    m = cols.reshape(cols.shape[0], Bn, -1).permute(1, 0, 2)                      # [B, K, n]
    return (m @ m.transpose(1, 2))[:, None]


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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--base-iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "samples_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say("python tools/samples_bench.py    (one MI355X; DESIGN.md 4.14)")
    say(f"S = {S} float32 samples, M = {M} uint8 truth, threshold {THR}; {a.iters} calls per figure, {a.base_iters} per "
        f"baseline figure, {a.rounds} rounds")
    for B, H, W in ((1, 2848, 4288), (8, 512, 512)):
        samples, truth = workload(B, H, W, dev)
        n = B * H * W
        nbytes = S * n * 4 + M * n
        gram = SM.sample_gram(samples, truth, THR)
        area = gram[..., torch.arange(S), torch.arange(S)].double()
        say(f"--- {B} x 1 x {H} x {W}: stack {S * n * 4 / 1e6:.1f} MB; foreground of the samples "
            f"{float(area.mean()) / (H * W):.4%} (min {float(area.min()) / (H * W):.4%}, max "
            f"{float(area.max()) / (H * W):.4%}), of the truth {float(gram[..., S, S].double().mean()) / (H * W):.4%}")
        row = SM.sample_set_metrics(gram, S).mean((0, 1)).tolist()
        say("    " + ", ".join(f"{k} {v:.6g}" for k, v in zip(SM.SAMPLESET_METRIC_NAMES, row)))
        ga, gb = pair_loop(samples, truth), float_matmul(samples, truth)
        exact_b = int(gram.max()) < 2 ** 24
        say(f"    device Gram vs (a) pair loop: {'equal' if torch.equal(gram, ga) else 'DIFFERENT'}; vs (b) fp32 matmul "
            f"({'exact here: every count < 2^24' if exact_b else 'NOT exact here: counts reach 2^24'}): "
            f"{'equal' if torch.equal(gram, gb.long()) else 'DIFFERENT'}")
        del ga, gb
        meter = SM.SampleSetMeter(THR)
        dst = torch.empty_like(samples)
        fast = [("g  sample_gram                  ", lambda: SM.sample_gram(samples, truth, THR), nbytes),
                ("u  SampleSetMeter.update        ", lambda: meter.update(samples, truth), nbytes),
                ("c  copy of the sample stack     ", lambda: dst.copy_(samples), 2 * S * n * 4)]
        slow = [("a  pair loop of (a & b).sum()   ", lambda: pair_loop(samples, truth), nbytes),
                ("b  threshold, .float(), B @ B.T ", lambda: float_matmul(samples, truth), nbytes)]
        for _, fn, _ in fast + slow:                 # warm-up: code objects, the allocator, the GEMM's choice
            for _ in range(2):
                fn()
        times = {name: [] for name, *_ in fast + slow}
        for _ in range(a.rounds):
            for name, fn, _ in fast:
                times[name].append(stream_us(fn, a.iters))
            for name, fn, _ in slow:
                times[name].append(stream_us(fn, a.base_iters))
        med = {}
        for name, _, nb in fast + slow:
            v = sorted(times[name])
            med[name[0]] = v[len(v) // 2]
            say(f"  {name}: median {med[name[0]]:10.1f} us (min {v[0]:10.1f}, max {v[-1]:10.1f})  {nb / 1e6:7.1f} MB "
                f"{nb / med[name[0]] / 1e3:7.1f} GB/s")
        rate = nbytes / med["g"] * 1e6
        copy_rate = 2 * S * n * 4 / med["c"] * 1e6
        say(f"  sample_gram reads at {rate / HBM_PEAK:.1%} of the 8.0 TB/s HBM peak and at {rate / copy_rate:.1%} of the "
            f"copy's {copy_rate / 1e12:.2f} TB/s; it takes {med['g'] / med['a']:.4f} x the time of (a) "
            f"({med['a'] / med['g']:.1f} x faster) and {med['g'] / med['b']:.4f} x the time of (b) "
            f"({'%.1f x faster' % (med['b'] / med['g']) if med['g'] < med['b'] else 'NOT faster than (b)'})")
        del samples, truth, dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
