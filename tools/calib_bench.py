"""Per-call time of the calibration / uncertainty pass (fp32 probabilities,
fp32 uncertainty, uint8 mask: 9 B per pixel) at 8x1x512^2 (a validation batch)
and 1x1x2848x4288 (one IDRiD image):
  (a) CalibrationMeter.update        one fused pass + the fp64 stage 2
  (b) the same totals in torch ops   clamp / multiply / bincount / masked sums, no .item(); timed over
      iters / 10 calls per figure.  The per-bin confidence sums are one masked fp64 sum per bin:
      index_add_ into 15 fp64 words measured 0.62 s per call at 8x1x512^2 (atomic contention)
  (c) SegmentationMeter.update       the streaming reference: seg_counts_vec on p and the mask (5 B per pixel)
  (a:NAME) vu_calib_hist of another build of the same sources (--ab NAME=PATH; e.g. a library
      built with -DVU_CALIB_PEEL=0, the LDS histogram without wave aggregation, or =2, two peels)
for two inputs each: `uniform` (p uniform in [0, 1), 30 % positives, u uniform
in [0, ln 2)) and `skewed` (99 % of the pixels with p < 1/1024 and truth 0, the
rest uniform with mixed truth; u = the binary entropy of p), the shape of a
lesion probability map.
Each figure is stream time per call (hip events around `iters` back-to-back
calls), `rounds` times with the variants alternating; GB/s = (p + u + mask
bytes) / time.
usage: python tools/calib_bench.py [--iters 100] [--rounds 5] [--ab peel0=ab/libvaeunet_hip_peel0.so ...]"""
import argparse
import ctypes
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaeunet_amd import _lib  # noqa: E402
from vaeunet_amd import calibration as CAL  # noqa: E402
from vaeunet_amd import metrics as M  # noqa: E402

SHAPES = [(8, 1, 512, 512), (1, 1, 2848, 4288)]
R = CAL.RANK_BINS


def torch_calib(p, t, u, nb, uscale):
    tb = t > 0
    ok = ~torch.isnan(p)
    pc = p.clamp(0.0, 1.0)
    cb = (pc * float(nb)).to(torch.int32).clamp_max(nb - 1).long()
    rb = (pc * float(R)).to(torch.int32).clamp_max(R - 1).long()
    ub = (u.clamp_min(0.0) * uscale).to(torch.int32).clamp_max(R - 1).long()
    conf_hist = torch.bincount((cb * 2 + tb).flatten(), minlength=2 * nb)
    rank_hist = torch.bincount((rb * 2 + tb).flatten(), minlength=2 * R)
    unc_hist = torch.bincount((ub * 2 + ((pc > 0.5) != tb)).flatten(), minlength=2 * R)
    pd = pc.double()
    conf_sum = torch.stack([torch.where(cb == b, pd, 0.0).sum() for b in range(nb)])
    d = pd - tb.double()
    q = pd.clamp(1e-7, 1 - 1e-7)
    return (conf_hist, rank_hist, unc_hist, conf_sum, (d * d).sum(), -torch.where(tb, q.log(), (1 - q).log()).sum(),
            (~ok).sum())


def make_inputs(shape, kind, dev):
    g = torch.Generator().manual_seed(0)
    if kind == "uniform":
        p = torch.rand(*shape, generator=g)
        t = (torch.rand(*shape, generator=g) < 0.3).to(torch.uint8)
        u = torch.rand(*shape, generator=g) * math.log(2)
    else:
        rare = torch.rand(*shape, generator=g) < 0.01
        p = torch.where(rare, torch.rand(*shape, generator=g), torch.rand(*shape, generator=g) * (0.999 / 1024))
        t = (rare & (torch.rand(*shape, generator=g) < 0.5)).to(torch.uint8)
        q = p.double().clamp(1e-12, 1 - 1e-12)
        u = (-(q * q.log() + (1 - q) * (1 - q).log())).float()
    return p.to(dev), t.to(dev), u.to(dev)


def other_build(path):
    """vu_calib_hist of another library file as fn(p, t, u, counts, ws)"""
    h = ctypes.CDLL(os.path.abspath(path))
    fn = h.vu_calib_hist
    fn.restype, fn.argtypes = _lib._SIGS["vu_calib_hist"]

    def run(p, t, u, c, ws):
        rc = fn(_lib.ptr(p), _lib.ptr(t), 1, _lib.ptr(u), p.numel(), c.n_bins, CAL._uscale(c.u_max),
                _lib.ptr(c.conf_hist), _lib.ptr(c.conf_sum), _lib.ptr(c.rank_hist), _lib.ptr(c.unc_hist),
                _lib.ptr(c.sums), _lib.ptr(c.invalid), 1, _lib.ptr(ws), _lib.stream())
        assert rc == 0, rc
    return run


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
    ap.add_argument("--ab", action="append", default=[], metavar="NAME=PATH")
    a = ap.parse_args()
    dev = torch.device("cuda")
    others = [(s.split("=", 1)[0], other_build(s.split("=", 1)[1])) for s in a.ab]
    for shape in SHAPES:
        for kind in ("uniform", "skewed"):
            p, t, u = make_inputs(shape, kind, dev)
            nbytes = p.nbytes + t.nbytes + u.nbytes
            meter = CAL.CalibrationMeter()
            meter.update(p, t, u)
            uscale = CAL._uscale(meter.u_max)
            seg = M.SegmentationMeter()
            variants = [("a  CalibrationMeter.update          ", lambda: meter.update(p, t, u), nbytes),
                        ("b  the totals in torch ops          ", lambda: torch_calib(p, t, u, 15, uscale), nbytes),
                        ("c  SegmentationMeter.update (p, mask)", lambda: seg.update(p, t), p.nbytes + t.nbytes)]
            for name, run in others:
                c, ws = meter.counts(), meter._ws
                variants.append((f"a:{name:<8} vu_calib_hist, other build", lambda run=run: run(p, t, u, c, ws),
                                 nbytes))
            # the other builds must produce the same integers
            ref = CAL.calib_hist(p, t, u)
            for name, run in others:
                c = CAL.calib_hist(p, t, u)
                run(p, t, u, c, meter._ws)
                assert torch.equal(c.rank_hist, 2 * ref.rank_hist) and torch.equal(c.unc_hist, 2 * ref.unc_hist), name
            for name, fn, _ in variants:                # warm-up: code objects, allocator
                for _ in range(2 if name[0] == "b" else 5):
                    fn()
            times = {name: [] for name, _, _ in variants}
            for _ in range(a.rounds):
                for name, fn, _ in variants:
                    times[name].append(stream_us(fn, max(1, a.iters // 10) if name[0] == "b" else a.iters))
            print(f"shape {'x'.join(map(str, shape))}  input {kind}  ({a.iters} calls per figure, b: {max(1, a.iters // 10)}; {a.rounds} rounds, "
                  f"{nbytes / 1e6:.1f} MB per call)", flush=True)
            for name, _, nb in variants:
                v = sorted(times[name])
                med = v[len(v) // 2]
                print(f"  {name}: median {med:9.1f} us  min {v[0]:9.1f}  max {v[-1]:9.1f}   "
                      f"{nb / med / 1e3:8.1f} GB/s", flush=True)


if __name__ == "__main__":
    main()
