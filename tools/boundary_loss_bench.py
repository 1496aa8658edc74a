"""Time of the signed distance map and the boundary loss on
three inputs:
  (a) blobs   8x1x512x512 uint8, twelve discs of radius 5..12 per plane, about
              2 % foreground: a training batch of lesion masks
  (b) single  the same shape, a single foreground pixel in the corner (0, 0) of
              every plane: the worst case of the row search, a pixel in column
              x walks x steps along its row before it meets a finite distance
  (c) frame   1x1x2848x4288, the prediction of tools/surface_bench.py's frame
Timed, per input:
  (s)  vu_sdf: one signed transform, float32 phi, two launches
  (c)  the same map composed from the public API the package had before it:
       distance_transform(x, "foreground", squared=False), distance_transform(x,
       "background", squared=False), and torch ops that sign, offset and zero
       the planes with one class only
  (l)  boundary_loss(logits, phi=phi) forward + backward
  (t)  boundary_loss(logits, targets) forward + backward: (s) + (l) and the
       autograd glue, what a training step adds
  (h)  the path a user has without it: the mask copied to the host,
       scipy.ndimage.distance_transform_edt twice per plane (Kervadec et al.'s
       one_hot2dist), the map copied back
Device figures: stream time per call between hip events around `iters`
back-to-back calls (chosen per variant from one timed call so that a figure
takes about `budget` seconds, at most --iters), `rounds` times with the
variants alternating, after a warm-up; median, min and max over the rounds.
Host figures: wall clock around `host_iters` calls that end on the host, per
round.  MB = the bytes the phase has to move per call, by counting: the signed
transform reads its input (1 B per pixel), writes the packed down scan (4 B),
reads and writes it in the up scan (8 B) and in the row pass (8 B): 21 B per
pixel; the composition is two transforms (42 B), a comparison of the input
(1 B read; its 1 B mask stays in cache) and three elementwise passes over
float32 maps (12 B): 55 B per pixel; the loss reads logits and phi twice and
writes the gradient: 20 B per element.  The searched width of the row pass is
LDS traffic and is not in these bytes.  The two maps are compared once per input.

Every input is measured in a child process of its own under a time limit
(--limit seconds); the parent never opens the device, and stops at the first
child that fails.  The report is printed and written to
profiles/boundary_loss_bench.txt (--out).
usage: python tools/boundary_loss_bench.py [--iters 200] [--rounds 5] [--host-iters 1] [--budget 0.5]
                                           [--limit 240] [--out FILE]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INPUTS = ("blobs", "single", "frame")


def _disc(a, cy, cx, r):
    H, W = a.shape
    y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
    yy, xx = np.mgrid[y0:y1, x0:x1]
    a[y0:y1, x0:x1][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1


def make_input(name):
    """uint8 [B, 1, H, W]"""
    if name == "frame":
        from surface_bench import frame
        return frame()[0][None, None]
    x = np.zeros((8, 1, 512, 512), np.uint8)
    if name == "single":
        x[:, :, 0, 0] = 1
        return x
    rng = np.random.Generator(np.random.PCG64(0))
    for b in range(8):
        for _ in range(12):
            _disc(x[b, 0], int(rng.integers(0, 512)), int(rng.integers(0, 512)), int(rng.integers(5, 13)))
    return x


def measure(name):
    """one input, in this process: prints the report lines"""
    import torch
    from vaeunet_amd import _lib as K
    from vaeunet_amd import surface as S
    from vaeunet_amd.loss import boundary_loss

    def say(text):
        print(text, flush=True)

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

    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    dev = torch.device("cuda")
    x = make_input(name)
    B, Cn, H, W = x.shape
    n = x.size
    dx = torch.from_numpy(x).to(dev)
    out = torch.empty(x.shape, dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(x.shape, generator=g) * 3).to(dev).requires_grad_(True)
    inf = float("inf")

    def sdf():
        K.call("vu_sdf", K.ptr(dx), K.VU_CCL_U8, 0.0, B * Cn, H, W, K.ptr(out), 1, inf, K.stream())

    def composed(squared=False):
        to_fg = S.distance_transform(dx, "foreground", squared=squared)
        to_bg = S.distance_transform(dx, "background", squared=squared)
        none = K.VU_EDT_INF if squared else inf
        mixed = (to_fg[:, :, :1, :1] != none) & (to_bg[:, :, :1, :1] != none)        # one pixel tells for its plane
        signed = torch.where(dx != 0, -to_bg if squared else 1.0 - to_bg, to_fg)
        return torch.where(mixed, signed, torch.zeros((), dtype=signed.dtype, device=dev))

    def host_path():
        m = dx.cpu().numpy() != 0
        phi = np.zeros(m.shape, np.float32)
        for b in range(B):
            for c in range(Cn):
                pos = m[b, c]
                if pos.any() and not pos.all():
                    neg = ~pos
                    phi[b, c] = ndi.distance_transform_edt(neg) * neg - (ndi.distance_transform_edt(pos) - 1) * pos
        return torch.from_numpy(phi).to(dev)

    sdf()
    phi = out.clone()
    s2 = S.signed_distance(dx, squared=True)
    say(f"[{name}] {B}x{Cn}x{H}x{W} uint8 ({n / 1e6:.2f} Mpixel), foreground {float(x.mean()):.4%}; phi in "
        f"[{float(phi.min()):.1f}, {float(phi.max()):.1f}]")
    same2 = bool(torch.equal(composed(True), s2))
    dphi = float((composed() - phi).abs().max())
    say(f"[{name}] composition: s2 {'equal' if same2 else 'DIFFERENT'}; float32 phi differs by at most {dphi:.1e} (it "
        f"rounds the root before the offset)")
    if ndi is not None:
        same = bool(torch.equal(host_path().view(torch.int32), phi.view(torch.int32)))
        say(f"[{name}] host path phi: {'bitwise equal' if same else 'DIFFERENT'}")

    def loss_only():
        logits.grad = None
        boundary_loss(logits, phi=phi).backward()

    def loss_targets():
        logits.grad = None
        boundary_loss(logits, dx).backward()

    device = [("s  vu_sdf (phi, float32)                ", sdf, 21 * n),
              ("c  composed from two distance transforms", composed, 55 * n),
              ("l  boundary_loss(phi=) fwd + bwd        ", loss_only, 20 * n),
              ("t  boundary_loss(targets) fwd + bwd     ", loss_targets, 41 * n)]
    host = [("h0 copy of the mask to the host         ", lambda: dx.cpu())]
    if ndi is not None:
        host.append(("h  copy + scipy edt x 2 per plane + copy ", host_path))
    iters = {}
    for label, fn, _ in device:                   # warm-up, and one timed call to size the figure
        fn()
        one = stream_us(fn, 1)
        iters[label] = int(max(1, min(ARGS.iters, ARGS.budget * 1e6 / max(one, 1.0))))
    for _, fn in host:
        fn()
    times = {label: [] for label, *_ in device + host}
    for _ in range(ARGS.rounds):
        for label, fn, _ in device:
            times[label].append(stream_us(fn, iters[label]))
        for label, fn in host:
            times[label].append(wall_us(fn, ARGS.host_iters))
    med = {}
    for label, _, nbytes in device:
        v = sorted(times[label])
        med[label[0]] = m = v[len(v) // 2]
        say(f"  [{name}] {label}: median {m:10.1f} us (min {v[0]:10.1f}, max {v[-1]:10.1f}; {iters[label]:3d} calls)  "
            f"{nbytes / 1e6:6.1f} MB {nbytes / m / 1e3:7.1f} GB/s")
    for label, _ in host:
        v = sorted(times[label])
        say(f"  [{name}] {label}: median {v[len(v) // 2]:10.1f} us (min {v[0]:10.1f}, max {v[-1]:10.1f})")
    if ndi is None:
        say(f"  [{name}] h  not measured: scipy is not installed")
    say(f"  [{name}] composed / vu_sdf = {med['c'] / med['s']:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--budget", type=float, default=0.5)
    ap.add_argument("--limit", type=float, default=240.0)
    ap.add_argument("--input", choices=INPUTS, help="measure this input in this process (what the parent starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_loss_bench.txt"))
    global ARGS
    ARGS = ap.parse_args()
    if ARGS.input:
        measure(ARGS.input)
        return 0
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if ARGS.out:
            with open(ARGS.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    shown, skip = [], False                          # the command as typed, without where the report goes
    for a in sys.argv[1:]:
        if not skip and not a.startswith("--out"):
            shown.append(a)
        skip = a == "--out" and not skip
    say(f"python tools/boundary_loss_bench.py {' '.join(shown)}".rstrip() + "    (one MI355X; DESIGN.md 4.13)")
    say(f"at most {ARGS.iters} calls per device figure (about {ARGS.budget} s), {ARGS.host_iters} per host figure, "
        f"{ARGS.rounds} rounds; every input in its own process, {ARGS.limit:.0f} s at most")
    passed = [f"--{k}={getattr(ARGS, k.replace('-', '_'))}" for k in ("iters", "rounds", "host-iters", "budget")]
    for name in INPUTS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--input", name] + passed,
                               capture_output=True, text=True, timeout=ARGS.limit)
        except subprocess.TimeoutExpired:
            say(f"[{name}] no result within {ARGS.limit:.0f} s; stopping")
            return 1
        for line in r.stdout.splitlines():
            say(line)
        if r.returncode != 0:
            say(f"[{name}] failed with exit status {r.returncode}; stopping\n{r.stderr[-2000:]}")
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
