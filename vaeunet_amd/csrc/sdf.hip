// Signed distance map of a mask: the exact signed squared
// Euclidean distance s2 of every pixel of the planes [H][W] of a contiguous
// [planes][H][W] tensor to the nearest pixel of the other class, or the map phi
// the boundary loss multiplies the probabilities with.  Definitions:
// include/vaeunet.h; the per-pixel steps: edt_core.h and sdf_core.h.
//
//   vu_sdf   two launches, in place in the output, no workspace:
//            1. the column pass of edt.hip's edt_col_kernel (64 columns x 16
//               chunks of rows, the chunks' carries through LDS) run for both
//               site sets at once, the foreground and the background; the two
//               vertical distances share the output word, 16 bits each.
//            2. one block per row: the packed row goes to two 16-bit rows in LDS
//               (W * 4 B <= 32 KB), whole, before any of it is written; each
//               thread runs edt_row_search over the row of the class its pixel
//               does not belong to and stores s2, or phi with the clip.  A row
//               without a finite distance in either half means a plane without
//               that class: written as 0, not searched.
//
// Offsets are 64-bit across planes, int32 within one (H W <= 2^27).
#include "common.h"
#include "sdf_core.h"
#include "../../include/vaeunet.h"

namespace {

constexpr int SC_COLS = 64, SC_SEG = 16;   // column pass: columns per block, chunks per column
constexpr int SR_BLK = 256;                // row pass: threads per row
constexpr unsigned SPLANES = 65535;        // grid.y; further planes are looped over

static_assert(VU_EDT_MAX_DIM <= EDT_NONE && EDT_NONE <= 65535, "a vertical distance, and EDT_NONE, fit 16 bits");
static_assert((size_t)VU_SDF_MAX_W * 2 * sizeof(uint16_t) <= 32768, "both rows of the row pass fit 32 KB of LDS");

VU_DEV bool is_fg(float v, float thr) { return v > thr; }       // NaN: background
VU_DEV bool is_fg(uint8_t v, float) { return v != 0; }

// ---- column pass ---------------------------------------------------------------
// edt_col_kernel's three steps (edt.hip) with two carried distances: df to the
// nearest foreground row, db to the nearest background row.  Set 0 of the LDS
// tables is the foreground's, set 1 the background's.
template <typename T>
__global__ void __launch_bounds__(SC_COLS * SC_SEG)
sdf_col_kernel(const T* __restrict__ x, float thr, int64_t planes, int H, int W, int32_t* __restrict__ g) {
  __shared__ int32_t first[2][SC_SEG][SC_COLS], last[2][SC_SEG][SC_COLS];   // absolute rows, -1: none in the chunk
  const int lane = threadIdx.x % SC_COLS, seg = threadIdx.x / SC_COLS;
  const int col = (int)blockIdx.x * SC_COLS + lane;
  const int rows = (H + SC_SEG - 1) / SC_SEG;
  const int y0 = min(seg * rows, H), y1 = min(y0 + rows, H);          // [y0, y1), empty past the plane
  const bool in = col < W;
  const int64_t n = (int64_t)H * W;
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    const T* src = x + plane * n;
    int32_t* dst = g + plane * n;
    int32_t df = EDT_NONE, db = EDT_NONE, ff = -1, lf = -1, fb = -1, lb = -1;
    if (in) {
#pragma unroll 4
      for (int y = y0; y < y1; ++y) {
        const bool fg = is_fg(src[y * W + col], thr);
        df = edt_col_step(df, fg);
        db = edt_col_step(db, !fg);
        dst[y * W + col] = sdf_pack(df, db);
        if (fg) {
          ff = ff < 0 ? y : ff;
          lf = y;
        } else {
          fb = fb < 0 ? y : fb;
          lb = y;
        }
      }
    }
    first[0][seg][lane] = ff;
    last[0][seg][lane] = lf;
    first[1][seg][lane] = fb;
    last[1][seg][lane] = lb;
    __syncthreads();
    if (in && y0 < y1) {
      const int32_t above_f = edt_chunk_above(&last[0][0][lane], SC_COLS, seg, y0);        // of the row y0 - 1
      const int32_t above_b = edt_chunk_above(&last[1][0][lane], SC_COLS, seg, y0);
      df = edt_chunk_below(&first[0][0][lane], SC_COLS, seg, SC_SEG, y1);                  // of the row y1
      db = edt_chunk_below(&first[1][0][lane], SC_COLS, seg, SC_SEG, y1);
#pragma unroll 4
      for (int y = y1 - 1; y >= y0; --y) {
        const int o = y * W + col;
        const int32_t w = dst[o];
        const int32_t down_f = edt_chunk_down(sdf_gf(w), above_f, y - y0);
        const int32_t down_b = edt_chunk_down(sdf_gb(w), above_b, y - y0);
        df = edt_col_step(df, down_f == 0);
        db = edt_col_step(db, down_b == 0);
        dst[o] = sdf_pack(edt_col_min(down_f, df), edt_col_min(down_b, db));
      }
    }
    __syncthreads();
  }
}

VU_DEV void store_sdf(int32_t* p, int32_t s2, float) { *p = s2; }
VU_DEV void store_sdf(float* p, int32_t s2, float clip) { *p = sdf_phi(s2, clip); }

// ---- row pass ------------------------------------------------------------------
// in place: the row is read into LDS whole before any of it is written
template <typename OUT>
__global__ void __launch_bounds__(SR_BLK)
sdf_row_kernel(int32_t* g, int64_t planes, int H, int W, float clip) {
  extern __shared__ uint16_t rows[];     // to_fg [W], to_bg [W]
  uint16_t* to_fg = rows;
  uint16_t* to_bg = rows + W;
  const int64_t n = (int64_t)H * W;
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
      int32_t* src = g + plane * n + (int64_t)y * W;
      int anyf = 0, anyb = 0;
      for (int xx = threadIdx.x; xx < W; xx += SR_BLK) {
        const int32_t v = src[xx];
        const uint16_t gf = sdf_gf(v), gb = sdf_gb(v);
        to_fg[xx] = gf;
        to_bg[xx] = gb;
        anyf |= gf != EDT_NONE;
        anyb |= gb != EDT_NONE;
      }
      anyf = __syncthreads_or(anyf);
      anyb = __syncthreads_or(anyb);
      const bool mixed = anyf && anyb;      // block-uniform: the plane has both classes
      OUT* dst = reinterpret_cast<OUT*>(src);
      for (int xx = threadIdx.x; xx < W; xx += SR_BLK) {
        int32_t s2 = 0;
        if (mixed) {
          const bool fg = sdf_is_fg(to_fg[xx]);
          s2 = sdf_signed(edt_row_search(sdf_opposite(to_fg, to_bg, fg), W, xx), fg);
        }
        store_sdf(dst + xx, s2, clip);
      }
      __syncthreads();
    }
  }
}

unsigned plane_grid(int64_t planes) { return (unsigned)(planes < SPLANES ? planes : SPLANES); }

}  // namespace

extern "C" int vu_sdf(const void* x, int dtype, float threshold, int64_t planes, int H, int W, void* out, int out_f32,
                      float clip, void* stream) {
  if (planes < 0 || H < 0 || W < 0 || H > VU_EDT_MAX_DIM || W > VU_SDF_MAX_W || (dtype != VU_CCL_U8 && dtype != VU_CCL_F32) ||
      (out_f32 != 0 && out_f32 != 1) || !(clip > 0.f))
    return (int)hipErrorInvalidValue;
  if (planes == 0 || H == 0 || W == 0) return 0;
  if (!x || !out) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const dim3 cgrid((unsigned)((W + SC_COLS - 1) / SC_COLS), plane_grid(planes));
  int32_t* g = static_cast<int32_t*>(out);
  if (dtype == VU_CCL_U8)
    hipLaunchKernelGGL(sdf_col_kernel<uint8_t>, cgrid, dim3(SC_COLS * SC_SEG), 0, st, static_cast<const uint8_t*>(x), threshold,
                       planes, H, W, g);
  else
    hipLaunchKernelGGL(sdf_col_kernel<float>, cgrid, dim3(SC_COLS * SC_SEG), 0, st, static_cast<const float*>(x), threshold,
                       planes, H, W, g);
  const dim3 rgrid((unsigned)H, plane_grid(planes));
  const size_t lds = (size_t)W * 2 * sizeof(uint16_t);
  if (out_f32) hipLaunchKernelGGL(sdf_row_kernel<float>, rgrid, dim3(SR_BLK), lds, st, g, planes, H, W, clip);
  else hipLaunchKernelGGL(sdf_row_kernel<int32_t>, rgrid, dim3(SR_BLK), lds, st, g, planes, H, W, clip);
  return (int)hipGetLastError();
}
