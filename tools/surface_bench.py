"""Time of the boundary metrics of one full IDRiD frame: a
1x1x2848x4288 uint8 hard prediction against a uint8 ground truth of the same
size, on two inputs:
  frame   one disc of radius 300 (the optic disc; the prediction's is shifted by
          (7, -5) pixels) and sparse blobs (300 ground-truth discs of radius
          2..6, 70 % of them predicted with a shift of up to 3 pixels, 200 false
          discs)
  single  the worst case of the row search: a single site in the corner (0, 0),
          so a pixel in column x walks x steps along its row before it meets a
          finite g; the ground truth of the pair statistics is a single pixel
          in the opposite corner
Timed, per input:
  (ef / eb / ed) vu_edt of the prediction, mode foreground / background / boundary
  (s)  vu_surface_stats: both boundary transforms, the reduction, the select
  (u)  SurfaceMeter.update: (s) and the metrics launch, nothing leaves the device
  (h)  the path a user has without it: both tensors copied to the host, the
       boundaries by binary_erosion, scipy.ndimage.distance_transform_edt twice,
       the same statistics in numpy; (h0) is the copy alone
Device figures: stream time per call between hip events around `iters`
back-to-back calls (chosen per variant from one timed call so that a figure
takes about `budget` seconds, at most --iters), `rounds` times with the
variants alternating, after a warm-up; median, min and max over the rounds.
Host figures: wall clock around `host_iters` calls that end on the host, per
round.  MB = the bytes the phase has to move per call: a transform reads its
input (1 B per pixel) and writes the down scan (4 B), reads and writes it in
the up scan (8 B) and in the row pass (8 B): 21 B per pixel; the statistics are
two transforms (42 B), the reduction over both (8 B) and four digit passes of
the select over both (32 B): 82 B per pixel.  The searched width of the row
pass is LDS traffic and is not in these bytes: the time of a transform follows
the data.  The statistics of the two paths are compared once per input.
The report is printed and written to profiles/surface_bench.txt (--out).
usage: python tools/surface_bench.py [--iters 200] [--rounds 5] [--host-iters 1] [--budget 1.0] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaeunet_amd import _lib as K  # noqa: E402
from vaeunet_amd import surface as S  # noqa: E402

H, W = 2848, 4288
Q, TOL = 95, 2.0
MODES = (("ef", "foreground", K.VU_EDT_TO_FOREGROUND), ("eb", "background", K.VU_EDT_TO_BACKGROUND),
         ("ed", "boundary  ", K.VU_EDT_TO_BOUNDARY))


def _disc(a, cy, cx, r):
    y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
    yy, xx = np.mgrid[y0:y1, x0:x1]
    a[y0:y1, x0:x1][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1


def frame(seed=0):
    """(pred uint8 [H, W], gt uint8 [H, W])"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pred, gt = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    _disc(gt, 1400, 3000, 300)
    _disc(pred, 1407, 2995, 300)
    for _ in range(300):
        cy, cx, r = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(2, 7))
        _disc(gt, cy, cx, r)
        if rng.random() < 0.7:
            dy, dx = (int(v) for v in rng.integers(-3, 4, 2))
            _disc(pred, cy + dy, cx + dx, r)
    for _ in range(200):
        _disc(pred, int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, 5)))
    return pred, gt


def single():
    pred, gt = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    pred[0, 0] = 1
    gt[H - 1, W - 1] = 1
    return pred, gt


def host_path(dpred, dgt, ndi):
    """copy, erode, transform twice, statistics in numpy -> (stats int64 [8], sums float64 [2])"""
    p, g = dpred.cpu().numpy()[0, 0] != 0, dgt.cpu().numpy()[0, 0] != 0
    cross = ndi.generate_binary_structure(2, 1)
    P, G = p & ~ndi.binary_erosion(p, cross, border_value=0), g & ~ndi.binary_erosion(g, cross, border_value=0)
    st, sm = np.full(8, -1, np.int64), np.zeros(2)
    st[0], st[1] = P.sum(), G.sum()
    if st[0] == 0 or st[1] == 0:
        return st, sm
    tol2 = int(TOL * TOL)
    for s, (a, b) in enumerate(((P, G), (G, P))):
        d2 = np.rint(ndi.distance_transform_edt(~b)[a] ** 2).astype(np.int64)
        srt = np.sort(d2)
        st[2 + s], st[4 + s], st[6 + s] = srt[-1], srt[(Q * len(srt) + 99) // 100 - 1], (d2 <= tol2).sum()
        sm[s] = np.sqrt(d2.astype(np.float64)).sum()
    return st, sm


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
    ap.add_argument("--budget", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "surface_bench.txt"))
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    dev = torch.device("cuda")
    n = H * W
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    say(f"python tools/surface_bench.py {' '.join(sys.argv[1:])}".rstrip() + "    (one MI355X; DESIGN.md 4.12)")
    say(f"frame 1x1x{H}x{W} ({n / 1e6:.1f} Mpixel), percentile {Q}, tolerance {TOL}; at most {a.iters} calls per device "
        f"figure (about {a.budget} s), {a.host_iters} per host figure, {a.rounds} rounds")
    for label, (pred, gt) in (("frame", frame()), ("single", single())):
        dpred, dgt = torch.from_numpy(pred)[None, None].to(dev), torch.from_numpy(gt)[None, None].to(dev)
        out = torch.empty((1, 1, H, W), dtype=torch.int32, device=dev)
        ws = torch.empty(S.workspace_elements(dpred.shape), dtype=torch.int32, device=dev)
        stats = torch.empty((1, 1, 8), dtype=torch.int64, device=dev)
        sums = torch.empty((1, 1, 2), dtype=torch.float64, device=dev)
        meter = S.SurfaceMeter(0.5, Q, TOL)

        def edt(mode):
            return lambda: K.call("vu_edt", K.ptr(dpred), K.VU_CCL_U8, 0.0, mode, 1, H, W, K.ptr(out), 0, K.stream())

        def stats_call():
            K.call("vu_surface_stats", K.ptr(dpred), K.VU_CCL_U8, 0.0, K.ptr(dgt), K.VU_CCL_U8, 1, H, W, Q,
                   int(TOL * TOL), K.ptr(stats), K.ptr(sums), K.ptr(ws), K.stream())

        stats_call()
        dst, dsm = stats.cpu().numpy()[0, 0], sums.cpu().numpy()[0, 0]
        say(f"[{label}] foreground {float(pred.mean()):.4%} of the prediction, {float(gt.mean()):.4%} of the ground "
            f"truth")
        say(f"[{label}] device stats {dst.tolist()} sums {dsm.tolist()}")
        if ndi is not None:
            hst, hsm = host_path(dpred, dgt, ndi)
            same = np.array_equal(hst, dst)
            rel = float(np.max(np.abs(hsm - dsm) / np.maximum(np.abs(hsm), 1e-300))) if same and hst[2] >= 0 else 0.0
            say(f"[{label}] host path stats {hst.tolist()}: {'equal' if same else 'DIFFERENT'}; sums differ by "
                f"{rel:.1e} relative")
        device = [(f"{k} vu_edt to the {name}           ", edt(code), 21 * n) for k, name, code in MODES]
        device += [("s  vu_surface_stats                    ", stats_call, 82 * n),
                   ("u  SurfaceMeter.update                 ", lambda: meter.update(dpred, dgt), 82 * n)]
        host = [("h0 copy of both tensors to the host    ", lambda: (dpred.cpu(), dgt.cpu()))]
        if ndi is not None:
            host.append(("h  copy + erosion + scipy edt x 2 + numpy", lambda: host_path(dpred, dgt, ndi)))
        iters = {}
        for name, fn, _ in device:                   # warm-up, and one timed call to size the figure
            fn()
            one = stream_us(fn, 1)
            iters[name] = int(max(1, min(a.iters, a.budget * 1e6 / max(one, 1.0))))
        for _, fn in host:
            fn()
        times = {name: [] for name, *_ in device + host}
        for _ in range(a.rounds):
            for name, fn, _ in device:
                times[name].append(stream_us(fn, iters[name]))
            for name, fn in host:
                times[name].append(wall_us(fn, a.host_iters))
        for name, _, nbytes in device:
            v = sorted(times[name])
            med = v[len(v) // 2]
            say(f"  [{label}] {name}: median {med:10.1f} us (min {v[0]:10.1f}, max {v[-1]:10.1f}; {iters[name]:3d} calls)  "
                f"{nbytes / 1e6:6.1f} MB {nbytes / med / 1e3:7.1f} GB/s")
        for name, _ in host:
            v = sorted(times[name])
            say(f"  [{label}] {name}: median {v[len(v) // 2]:10.1f} us (min {v[0]:10.1f}, max {v[-1]:10.1f})")
        if ndi is None:
            say(f"  [{label}] h  not measured: scipy is not installed")


if __name__ == "__main__":
    main()
