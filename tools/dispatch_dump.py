#!/usr/bin/env python
"""Dump every host-side dispatch decision of the library for a fixed sweep.

No GPU is needed and nothing is launched: the tool only asks the query entry
points (which kernel, row tile, workspace bytes, ...) and the return codes of
vu_gemm_set_tuning.  Two builds decide alike exactly when their dumps are
byte-identical:

    VU_LIB_PATH=/path/to/a/libvaeunet_hip.so python tools/dispatch_dump.py --full a.txt
    VU_LIB_PATH=/path/to/b/libvaeunet_hip.so python tools/dispatch_dump.py --full b.txt
    diff a.txt b.txt

Prints the per-kernel-id counts of the forward sweep and the SHA-256 of all
lines; fails if a kernel id of vu_gemm_fwd_kernel is never reached (a broken
sweep would otherwise hide a route).
"""
import argparse
import collections
import ctypes as C
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from vaeunet_amd._lib import BF16, F32, VuConvFp8, VuGemmFwd, VuGemmWgrad, lib  # noqa: E402
# tuning keys: the header's numbers (the binding reads them from include/vaeunet.h)
from vaeunet_amd._lib import (  # noqa: E402
    VU_TUNE_ATTN as ATTN, VU_TUNE_BN_MINBLK as BN_MINBLK, VU_TUNE_BN_NT_MB as BN_NT_MB, VU_TUNE_FP8_C64 as FP8_C64,
    VU_TUNE_FP8_GRID as FP8_GRID, VU_TUNE_FP8_PP as FP8_PP, VU_TUNE_FP8_SPLIT as FP8_SPLIT, VU_TUNE_FP8_XM as FP8_XM,
    VU_TUNE_GEN as GEN, VU_TUNE_PP_FULL as PP_FULL, VU_TUNE_SLAB4 as SLAB4, VU_TUNE_STREAM as STREAM,
    VU_TUNE_UNSAFE as UNSAFE, VU_TUNE_V2_SMALL as V2_SMALL, VU_TUNE_V4_MIN_BLOCKS as V4_MIN_BLOCKS,
    VU_TUNE_V4_SPLIT_CHUNKS as V4_SPLIT_CHUNKS, VU_TUNE_V4_SPLITK as V4_SPLITK, VU_TUNE_V5 as V5, VU_TUNE_V6 as V6,
    VU_TUNE_V6_STAG as V6_STAG, VU_TUNE_V6_XM as V6_XM, VU_TUNE_V7 as V7, VU_TUNE_V7_NBW as V7_NBW,
    VU_TUNE_V7_XM as V7_XM, VU_TUNE_W2_BIG as W2_BIG, VU_TUNE_W3_SMALL as W3_SMALL)

# the defaults (the header has none: csrc/tuning.hip holds them)
DEFAULTS = {V4_MIN_BLOCKS: 256, FP8_GRID: 0, STREAM: 1, V4_SPLITK: 1, V4_SPLIT_CHUNKS: 2, V2_SMALL: 1, V5: 1, V6: 1,
            GEN: 4, SLAB4: 1, BN_NT_MB: 32, V7: 1, V7_NBW: 3, V7_XM: 0, W3_SMALL: 1, FP8_XM: 0, FP8_PP: 1, ATTN: 1,
            FP8_C64: 2, FP8_SPLIT: 1, BN_MINBLK: 256, PP_FULL: 1, W2_BIG: 0, V6_XM: 0,
            V6_STAG: 1, UNSAFE: 0}
FWD_IDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13)

GRIDS = [(1, 8, 32), (2, 16, 16), (2, 16, 64), (8, 32, 32), (8, 64, 64), (8, 128, 128), (8, 512, 512), (2, 9, 7)]
SOURCES = [[8], [64], [128], [96, 64], [32, 32, 64], [256], [512], [1024], [64, 128]]
NCOLS = [16, 32, 64, 128, 192, 256, 512, 832]
# epilogue options, each alone and a few together (zbias: 3x3 only)
FLAGS = [(), ("zbias",), ("stat_sum",), ("accumulate",), ("bias",), ("bnb_part",), ("stat_sum", "bias"),
         ("accumulate", "bias"), ("zbias", "stat_sum"), ("zbias", "bnb_part"), ("stat_sum", "bnb_part", "bias")]
# generations 1..4 at default tuning, then single keys at generation 4
FWD_SETTINGS = [(GEN, 1), (GEN, 2), (GEN, 3), (GEN, 4), (V4_MIN_BLOCKS, 0), (V4_SPLITK, 0), (V4_SPLITK, 3), (V7, 0),
                (V7, 2), (V6, 0), (V6, 2), (V6, -1), (V5, 0), (V5, 2), (V5, -1), (V2_SMALL, 0), (STREAM, 0),
                (V4_SPLIT_CHUNKS, 1)]
WGRAD_SETTINGS = [(GEN, 1), (GEN, 2), (GEN, 3), (GEN, 4), (W3_SMALL, 0), (W2_BIG, 1)]
FP8_SETTINGS = [(GEN, 4), (FP8_GRID, 2), (FP8_PP, 0), (FP8_C64, 0), (FP8_C64, 1), (FP8_C64, -1), (FP8_SPLIT, 0)]
TUNE_VALUES = [-1, 0, 1, 2, 3, 4, 5, 6, 256]

DUMMY = 0x1000  # a non-null pointer: the queries never dereference it


def restore_defaults(L):
    L.vu_gemm_set_tuning(UNSAFE, 1)
    for k, v in DEFAULTS.items():
        if k != UNSAFE and L.vu_gemm_set_tuning(k, v) != 0:
            raise SystemExit(f"default of key {k} refused")
    L.vu_gemm_set_tuning(UNSAFE, 0)
    if L.vu_gemm_experiment_modes() != 0:
        raise SystemExit("experiment modes left on")


def fill_gather(g, grid, srcs, R=1, S=1, sy=1, sx=1, oy=0, ox=0, Hs=None, Ws=None):
    N, H, W = grid
    cend = 0
    for i in range(3):
        if i < len(srcs):
            cend += srcs[i]
            g.src[i], g.stride[i] = DUMMY, srcs[i]
        else:
            g.src[i], g.stride[i] = None, 0
        g.cend[i] = cend
    g.nsrc, g.C, g.N, g.H, g.W = len(srcs), cend, N, H, W
    g.Hs, g.Ws = (H if Hs is None else Hs), (W if Ws is None else Ws)
    g.R, g.S, g.sy, g.sx, g.dy, g.dx, g.oy, g.ox = R, S, sy, sx, 1, 1, oy, ox


def fwd_problem(grid, srcs, ncol, ksz, flags=(), mode=0):
    """mode 0: plain conv (ksz 1 or 3); 1: ConvTranspose forward (1x1 gather, pixel-shuffle store);
    2: ConvTranspose input gradient (2x2 stride-2 gather); 7: the 7x7 stride-2 stem."""
    a = VuGemmFwd()
    N, H, W = grid
    if mode == 2:
        fill_gather(a.a, grid, srcs, R=2, S=2, sy=2, sx=2, Hs=2 * H, Ws=2 * W)
    elif mode == 7:
        fill_gather(a.a, grid, srcs, R=7, S=7, sy=2, sx=2, oy=-3, ox=-3, Hs=2 * H, Ws=2 * W)
    elif ksz == 3:
        fill_gather(a.a, grid, srcs, R=3, S=3, oy=-1, ox=-1)
    else:
        fill_gather(a.a, grid, srcs)
    a.b, a.ldb, a.ncol, a.out, a.out_stride = DUMMY, a.a.R * a.a.S * a.a.C, ncol, DUMMY, ncol
    if mode == 1:
        a.out_mode, a.cout, a.oH, a.oW, a.out_stride = 1, ncol // 4, 2 * H, 2 * W, ncol // 4
    for f in flags:
        if f == "accumulate":
            a.accumulate = 1
        else:
            setattr(a, f, DUMMY)
    if "stat_sum" in flags:
        a.stat_m2 = DUMMY
    if "bnb_part" in flags:
        a.bnb_x, a.bnb_xstride, a.bnb_scale, a.bnb_shift, a.bnb_mean, a.bnb_invstd = DUMMY, ncol, DUMMY, DUMMY, DUMMY, DUMMY
    return a


def fwd_problems():
    for grid, srcs, ncol, ksz in itertools.product(GRIDS, SOURCES, NCOLS, (1, 3)):
        for flags in FLAGS:
            if "zbias" in flags and ksz != 3:
                continue
            tag = f"conv{ksz} {grid} {srcs} n{ncol} {'+'.join(flags) or '-'}"
            yield tag, fwd_problem(grid, srcs, ncol, ksz, flags)
    for grid, srcs, ncol in itertools.product(GRIDS, SOURCES, NCOLS):
        for flags in ((), ("bias",), ("stat_sum",), ("accumulate",)):
            yield f"convT {grid} {srcs} n{ncol} {'+'.join(flags) or '-'}", fwd_problem(grid, srcs, ncol, 1, flags, 1)
            yield f"convT_dgrad {grid} {srcs} n{ncol} {'+'.join(flags) or '-'}", fwd_problem(grid, srcs, ncol, 1, flags, 2)
    for grid, ncol in itertools.product(GRIDS, (64, 128)):
        for flags in ((), ("stat_sum",), ("accumulate",)):
            yield f"stem {grid} n{ncol} {'+'.join(flags) or '-'}", fwd_problem(grid, [8], ncol, 7, flags, 7)


def dump_fwd(L, out, counts):
    probs = list(fwd_problems())
    for key, value in FWD_SETTINGS:
        restore_defaults(L)
        if L.vu_gemm_set_tuning(key, value) != 0:
            raise SystemExit(f"tuning {key}={value} refused")
        for tag, a in probs:
            for dt in (BF16, F32):
                k = L.vu_gemm_fwd_kernel(C.byref(a), dt)
                counts[k] += 1
                out.append(f"fwd t{key}={value} {tag} dt{dt}: k{k} bm{L.vu_gemm_fwd_row_tile(C.byref(a), dt)} "
                           f"ws{L.vu_gemm_fwd_workspace_bytes(C.byref(a), dt)} bnb{L.vu_gemm_fwd_bnb_tile(C.byref(a), dt)}")
    return len(probs)


def dump_wgrad(L, out):
    probs = []
    for grid, srcs, ni, ksz in itertools.product(GRIDS, SOURCES, (16, 32, 64, 128, 256, 512), (1, 3)):
        N, H, W = grid
        M = N * H * W
        for mps in sorted({M, 128, 256, 100}):
            a = VuGemmWgrad()
            fill_gather(a.p, grid, [ni])
            if ksz == 3:
                fill_gather(a.q, grid, srcs, R=3, S=3, oy=-1, ox=-1)
            else:
                fill_gather(a.q, grid, srcs)
            a.ni, a.nj, a.m_per_split, a.out = ni, ksz * ksz * a.q.C, mps, DUMMY
            a.splits = (M + mps - 1) // mps
            probs.append((f"wgrad{ksz} {grid} {srcs} ni{ni} mps{mps}", a))
    bi, bj = C.c_int(0), C.c_int(0)
    for key, value in WGRAD_SETTINGS:
        restore_defaults(L)
        if L.vu_gemm_set_tuning(key, value) != 0:
            raise SystemExit(f"tuning {key}={value} refused")
        for tag, a in probs:
            for dt in (BF16, F32):
                bi.value = bj.value = -1
                g = L.vu_gemm_wgrad_tile(C.byref(a), dt, C.byref(bi), C.byref(bj))
                out.append(f"wgrad t{key}={value} {tag} dt{dt}: gen{g} bi{bi.value} bj{bj.value}")
    return len(probs)


def dump_fp8(L, out):
    probs = []
    for grid, srcs, ncol in itertools.product(GRIDS, SOURCES, NCOLS):
        for flags in ((), ("stat_sum",), ("stat_min",), ("stat_sum", "stat_min"), ("bias",)):
            a = VuConvFp8()
            fill_gather(a.a, grid, srcs, R=3, S=3, oy=-1, ox=-1)
            a.w, a.ldw, a.ncol, a.out, a.out_stride = DUMMY, 9 * a.a.C, ncol, DUMMY, ncol
            a.x_scale = a.w_scale = DUMMY
            for f in flags:
                setattr(a, f, DUMMY)
            if "stat_sum" in flags:
                a.stat_m2 = DUMMY
            if "stat_min" in flags:
                a.stat_max = DUMMY
            probs.append((f"fp8 {grid} {srcs} n{ncol} {'+'.join(flags) or '-'}", a))
    for key, value in FP8_SETTINGS:
        restore_defaults(L)
        if L.vu_gemm_set_tuning(key, value) != 0:
            raise SystemExit(f"tuning {key}={value} refused")
        for tag, a in probs:
            out.append(f"fp8 t{key}={value} {tag}: bm{L.vu_conv3x3_fp8_row_tile(C.byref(a))} "
                       f"ws{L.vu_conv3x3_fp8_workspace_bytes(C.byref(a))} mm{L.vu_conv3x3_fp8_minmax_ok(C.byref(a))}")
    return len(probs)


def dump_tuning(L, out):
    for unsafe in (0, 1):
        restore_defaults(L)
        for key in list(range(0, 41)) + [-1]:
            L.vu_gemm_set_tuning(UNSAFE, unsafe)
            for value in TUNE_VALUES:
                rc = L.vu_gemm_set_tuning(key, value)
                out.append(f"tune unsafe{unsafe} k{key} v{value}: rc{rc} xm{L.vu_gemm_experiment_modes()}")
            if key in DEFAULTS:
                L.vu_gemm_set_tuning(UNSAFE, 1)
                L.vu_gemm_set_tuning(key, DEFAULTS[key])
    restore_defaults(L)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--full", metavar="FILE", help="write every line to FILE (for diff)")
    args = ap.parse_args()
    L = lib()
    out, counts = [], collections.Counter()
    nf = dump_fwd(L, out, counts)
    nw = dump_wgrad(L, out)
    n8 = dump_fp8(L, out)
    dump_tuning(L, out)
    restore_defaults(L)
    text = "\n".join(out) + "\n"
    if args.full:
        with open(args.full, "w") as f:
            f.write(text)
    print(f"problems: forward {nf} x {len(FWD_SETTINGS)} settings x 2 dtypes, wgrad {nw} x {len(WGRAD_SETTINGS)} x 2, "
          f"fp8 {n8} x {len(FP8_SETTINGS)}; {len(out)} lines")
    print("forward kernel ids:", " ".join(f"{k}:{counts[k]}" for k in sorted(counts)))
    print("sha256", hashlib.sha256(text.encode()).hexdigest())
    missing = [k for k in FWD_IDS if counts[k] == 0]
    if missing or set(counts) - set(FWD_IDS):
        raise SystemExit(f"kernel ids never reached: {missing}; unknown ids: {sorted(set(counts) - set(FWD_IDS))}")


if __name__ == "__main__":
    main()
