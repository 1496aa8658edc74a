// Host-side declarations shared by the .hip files: the tuning accessor, the
// small launch helpers, and every host function one file calls in another.
// (Device state is per code object, each .hip being its own: the LDS-DMA zero
// page is declared once, in wave.h, as a static array, so every file that
// uses it gets its own storage.)
#pragma once
#include "common.h"
#include "../../include/vaeunet.h"

// ---- tuning (tuning.hip holds the table: keys, defaults, validation) --------
constexpr int VU_TUNE_NKEYS = 35;  // key numbers are 0 .. VU_TUNE_NKEYS - 1
struct VuTuneValues {
  int v[VU_TUNE_NKEYS];
};
extern VuTuneValues vu_tune_values;
// current value of a live VU_TUNE_* key, as normalised by vu_gemm_set_tuning
inline int tune(int key) { return vu_tune_values.v[key]; }

// ---- launch helpers ---------------------------------------------------------
// compute units of the current device (persistent grids, one-block-per-CU rules)
inline int cu_count() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  }
  return n;
}

// grid of a 256-thread grid-stride elementwise kernel
inline unsigned ew_grid(int64_t work) {
  int64_t g = (work + 255) / 256;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  return (unsigned)g;
}

inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// 3x3 stride-1 dilation-1 pad-1 gather over sources of the grid's own size
inline bool same3x3(const VuGather& g) {
  return g.R == 3 && g.S == 3 && g.sy == 1 && g.sx == 1 && g.dy == 1 && g.dx == 1 && g.oy == -1 && g.ox == -1 &&
         g.Hs == g.H && g.Ws == g.W;
}

// ---- forward GEMM kernels (routes of gemm_fwd.hip) --------------------------
// *_bm: row tile when the kernel serves the problem, else 0
int conv_image_bm(const VuGemmFwd& p, int dtype);  // conv_image.hip (3-channel image conv)
int conv_image_launch(const VuGemmFwd& p, hipStream_t st);
int conv_stem_bm(const VuGemmFwd& p, int dtype);  // conv_stem.hip (ResNet34 7x7/s2 stem)
int conv_stem_launch(const VuGemmFwd& p, hipStream_t st);
int gemm_stream_bm(const VuGemmFwd& p, int dtype);  // gemm_stream.hip (short-K 1x1 streams)
int gemm_stream_launch(const VuGemmFwd& p, hipStream_t st);
int gemm_fwd_v2_bm(const VuGemmFwd& p, int dtype);  // gemm_fwd2.hip (large-tile LDS-DMA)
int gemm_fwd_v2_launch(const VuGemmFwd& p, hipStream_t st);
int gemm_fwd_v2_small(const VuGemmFwd& p, int dtype);  // (the split count, not a tile; rows: 128)
int gemm_fwd_v2_small_launch(const VuGemmFwd& p, hipStream_t st);
int64_t gemm_fwd_v2_small_workspace(const VuGemmFwd& p, int dtype);
int gemm_fwd_v2_tail(const VuGemmFwd& p, int dtype);
int gemm_fwd_v2_tail_launch(const VuGemmFwd& p, hipStream_t st);
int gemm_fwd_v3_bm(const VuGemmFwd& p, int dtype);  // gemm_fwd3.hip (halo)
int gemm_fwd_v3_launch(const VuGemmFwd& p, hipStream_t st);
int gemm_fwd_v4_bm(const VuGemmFwd& p, int dtype);  // gemm_fwd4.hip (ping-pong)
int gemm_fwd_v4_launch(const VuGemmFwd& p, hipStream_t st);
int64_t gemm_fwd_v4_workspace(const VuGemmFwd& p, int dtype);
int gemm_fwd_v4_bnb_tile(const VuGemmFwd& p, int dtype);
int splitk_finish_launch(const VuGemmFwd& p, hipStream_t st);
int gemm_fwd_v5_bm(const VuGemmFwd& p, int dtype);  // gemm_fwd5.hip (persistent short-K GEMM)
int gemm_fwd_v5_launch(const VuGemmFwd& p, hipStream_t st);
int gemm_fwd_v6_bm(const VuGemmFwd& p, int dtype);  // gemm_fwd6.hip (64 -> 64 3x3, resident weights)
int gemm_fwd_v6_launch(const VuGemmFwd& p, hipStream_t st);
int gemm_fwd_v7_bm(const VuGemmFwd& p, int dtype);  // gemm_fwd7.hip (small-grid 3x3, two K groups)
int gemm_fwd_v7_launch(const VuGemmFwd& p, hipStream_t st);
int64_t gemm_fwd_v7_workspace(const VuGemmFwd& p, int dtype);

// ---- weight-gradient kernels (picked by gemm_wgrad.hip) ---------------------
int gemm_wgrad_v2_tile(const VuGemmWgrad& p, int dtype, int* bi, int* bj);  // gemm_wgrad2.hip
int gemm_wgrad_v2_launch(const VuGemmWgrad& p, hipStream_t st);
int gemm_wgrad_v3_tile(const VuGemmWgrad& p, int dtype, int* bi, int* bj);  // gemm_wgrad3.hip
int gemm_wgrad_v3_launch(const VuGemmWgrad& p, hipStream_t st);
