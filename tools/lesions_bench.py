"""Time of the lesion-level evaluation of one full IDRiD frame:
a 1x1x2848x4288 fp32 probability map with sparse blobs against a uint8 ground
truth of the same size.
  (u)  LesionMeter.update: both labellings, the matching, the counts and the
       FROC histograms, nothing leaves the device
  (lp) vu_ccl_label of the probability map alone (fp32, threshold 0.5)
  (lg) vu_ccl_label of the ground truth alone (uint8)
  (m)  vu_lesion_match alone on the two label images (tables cleared, three passes)
  (h)  the path a user has without it: both tensors copied to the host,
       scipy.ndimage.label twice, and the same matching in numpy (areas,
       maximum score, any-overlap, min_area, the two histograms); (h0) is the
       copy alone
Device figures: stream time per call between hip events around `iters`
back-to-back calls, `rounds` times with the variants alternating, after a
warm-up; median, min and max over the rounds.  Host figures: wall clock around
`host_iters` calls that end on the host, per round.  GB/s = the bytes the
phase has to move / median time: (lp) reads 4 B and writes 4 B per pixel in
the tile pass and reads 4 B in the flatten pass (12 B per pixel; the border
pass and the stores of changed labels touch foreground only), (lg) 1 + 4 + 4 =
9 B, (m) clears four tables (16 B), reads one label image in the area pass
(4 B) and both in the overlap and root passes (16 B): 36 B per pixel, and (u)
is their sum.  The counts of the two paths are compared once.
usage: python tools/lesions_bench.py [--iters 200] [--rounds 5] [--host-iters 1]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaeunet_amd import _lib as K  # noqa: E402
from vaeunet_amd import lesions as L  # noqa: E402

H, W = 2848, 4288
THR, MIN_AREA, BINS = 0.5, 2, 1000


def frame(seed=0):
    """(prob float32 [H, W], gt uint8 [H, W]): 300 ground-truth discs of radius 2..6; 70 % of them predicted, shifted
    by up to 3 pixels; 200 false discs and 300 single false pixels; probabilities 0.55..1 inside, below 0.45 outside"""
    rng = np.random.Generator(np.random.PCG64(seed))
    gt = np.zeros((H, W), np.uint8)
    prob = (rng.random((H, W), dtype=np.float32) * np.float32(0.45)).astype(np.float32)

    def disc(a, cy, cx, r, v):
        y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        m = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        a[y0:y1, x0:x1][m] = v
    for _ in range(300):
        cy, cx, r = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(2, 7))
        disc(gt, cy, cx, r, 1)
        if rng.random() < 0.7:
            dy, dx = (int(v) for v in rng.integers(-3, 4, 2))
            disc(prob, cy + dy, cx + dx, r, np.float32(0.55 + 0.45 * rng.random()))
    for _ in range(200):
        disc(prob, int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, 5)),
             np.float32(0.55 + 0.45 * rng.random()))
    prob[rng.integers(0, H, 300), rng.integers(0, W, 300)] = np.float32(0.9)
    return prob, gt


def host_path(dprob, dgt, ndi):
    """copy, label twice, match in numpy -> (counts [4], hist_fp, hist_gt)"""
    prob, gt = dprob.cpu().numpy()[0, 0], dgt.cpu().numpy()[0, 0]
    eight = np.ones((3, 3), int)
    pl, kp = ndi.label(prob > np.float32(THR), structure=eight)
    gl, kg = ndi.label(gt != 0, structure=eight)
    area = np.bincount(pl.reshape(-1), minlength=kp + 1)
    score = np.zeros(kp + 1, np.float32)
    fg = pl > 0
    np.maximum.at(score, pl[fg], np.maximum(prob[fg], np.float32(0)))
    kept = area >= MIN_AREA
    kept[0] = False
    both = fg & (gl > 0)
    pairs = np.unique(np.stack([pl[both], gl[both]]), axis=1)
    hit = np.zeros(kp + 1, bool)
    hit[pairs[0]] = True
    pk = pairs[:, kept[pairs[0]]]
    det = np.full(kg + 1, -1, np.float32)
    np.maximum.at(det, pk[1], score[pk[0]])

    def bins(s):
        t = s.astype(np.float32) * np.float32(BINS)
        return np.where(t >= BINS, BINS - 1, t.astype(np.int64))
    fp = kept & ~hit
    hist_fp = np.bincount(bins(score[fp]), minlength=BINS)
    hist_gt = np.bincount(bins(det[det >= 0]), minlength=BINS)
    return np.array([kg, int((det >= 0).sum()), int(kept.sum()), int(fp.sum())]), hist_fp, hist_gt


def stream_us(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def wall_us(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda")
    prob, gt = frame()
    dprob, dgt = torch.from_numpy(prob)[None, None].to(dev), torch.from_numpy(gt)[None, None].to(dev)
    n = H * W
    pl = torch.empty((1, 1, H, W), dtype=torch.int32, device=dev)
    gl = torch.empty_like(pl)
    ws = torch.empty(K.query("vu_ccl_workspace_bytes", 1, H, W) // 4, dtype=torch.int32, device=dev)
    counts = torch.empty((1, 1, 4), dtype=torch.int64, device=dev)
    hist = torch.zeros((2, BINS), dtype=torch.int64, device=dev)
    meter = L.LesionMeter(THR, MIN_AREA, 8, BINS)

    def label_pred():
        K.call("vu_ccl_label", K.ptr(dprob), K.VU_CCL_F32, THR, 1, H, W, 8, K.ptr(pl), None, K.stream())

    def label_gt():
        K.call("vu_ccl_label", K.ptr(dgt), K.VU_CCL_U8, 0.0, 1, H, W, 8, K.ptr(gl), None, K.stream())

    def match():
        K.call("vu_lesion_match", K.ptr(pl), K.ptr(gl), K.ptr(dprob), K.VU_CCL_F32, 1, H, W, MIN_AREA, BINS,
               K.ptr(counts), K.ptr(hist[0]), K.ptr(hist[1]), K.ptr(ws), K.stream())

    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    meter.update(dprob, dgt)
    dc = meter.counts().cpu().numpy()[0]
    print(f"frame 1x1x{H}x{W} ({n / 1e6:.1f} Mpixel), foreground {float((prob > THR).mean()):.4%} of the prediction, "
          f"{float(gt.mean()):.4%} of the ground truth; min_area {MIN_AREA}, {BINS} bins", flush=True)
    print(f"device counts (n_gt, n_gt_detected, n_pred, n_pred_fp): {dc.tolist()}", flush=True)
    if ndi is not None:
        hc, hf, hg = host_path(dprob, dgt, ndi)
        mf, mg = (h.cpu().numpy() for h in meter.histograms())
        same = np.array_equal(hc, dc) and np.array_equal(hf, mf) and np.array_equal(hg, mg)
        print(f"host path counts {hc.tolist()}: counts and both histograms {'equal' if same else 'DIFFERENT'}",
              flush=True)
    device = [("u  LesionMeter.update                 ", lambda: meter.update(dprob, dgt), 57 * n),
              ("lp vu_ccl_label, fp32 prediction      ", label_pred, 12 * n),
              ("lg vu_ccl_label, uint8 ground truth   ", label_gt, 9 * n),
              ("m  vu_lesion_match                    ", match, 36 * n)]
    host = [("h0 copy of both tensors to the host   ", lambda: (dprob.cpu(), dgt.cpu()))]
    if ndi is not None:
        host.append(("h  copy + scipy label x 2 + numpy match", lambda: host_path(dprob, dgt, ndi)))
    for _, fn, _ in device:                      # warm-up: code objects, the allocator
        for _ in range(3):
            fn()
    for _, fn in host:
        fn()
    times = {name: [] for name, *_ in device + host}
    for _ in range(a.rounds):
        for name, fn, _ in device:
            times[name].append(stream_us(fn, a.iters))
        for name, fn in host:
            times[name].append(wall_us(fn, a.host_iters))
    print(f"({a.iters} calls per device figure, {a.host_iters} per host figure, {a.rounds} rounds)", flush=True)
    for name, _, nbytes in device:
        v = sorted(times[name])
        med = v[len(v) // 2]
        print(f"  {name}: median {med:9.1f} us (min {v[0]:9.1f}, max {v[-1]:9.1f})  {nbytes / 1e6:6.1f} MB "
              f"{nbytes / med / 1e3:7.1f} GB/s", flush=True)
    for name, _ in host:
        v = sorted(times[name])
        print(f"  {name}: median {v[len(v) // 2]:9.1f} us (min {v[0]:9.1f}, max {v[-1]:9.1f})", flush=True)
    if ndi is None:
        print("  h  not measured: scipy is not installed", flush=True)


if __name__ == "__main__":
    main()
