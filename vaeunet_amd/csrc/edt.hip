// Boundary metrics: the exact squared Euclidean distance
// transform of the planes [H][W] of a contiguous [planes][H][W] tensor, the
// boundary of a mask, and the surface statistics between two boundary sets.
// Definitions: include/vaeunet.h; the per-pixel steps: edt_core.h.
//
//   vu_edt              separable, two launches, in place in the output:
//                       1. a down scan leaves the vertical distance to the nearest
//                          site above, an up scan the distance g to the nearest
//                          site of the column (EDT_NONE for a column without
//                          one).  Lanes are neighbouring columns: coalesced.  A
//                          column is cut into 16 chunks of rows, one thread each,
//                          that exchange the rows of their first and last site
//                          in LDS.
//                       2. one block per row: g of the row goes to LDS, 16 bits
//                          each (W * 2 B <= 32 KB); each thread searches outwards
//                          from its x over g^2 + dx^2 and stops once dx^2 >= best
//                          (edt_row_search), so the searched width follows the
//                          data.  A row without a finite g means a plane without
//                          a site: written as EDT_INF, not searched.
//   vu_edt_boundary     foreground pixels with a 4-neighbour that is background
//                       or outside the plane.
//   vu_surface_stats    two VU_EDT_TO_BOUNDARY transforms into the workspace (a
//                       boundary pixel is where its own transform is 0, so the
//                       later passes read the two transforms only); block
//                       partials of n, max, within-tolerance count (integers) and
//                       of the fp64 sum of square roots, reduced per plane in a
//                       fixed order; the percentile by a radix select over the
//                       32-bit keys, four 8-bit digits, digit histograms in LDS,
//                       prefix and remaining rank kept in device memory.
//   vu_surface_metrics  one small fp64 launch.
//
// No floating-point atomics: a thread adds its pixels in index order, a wave in
// a shuffle butterfly, a block over its waves in order, the plane over its
// blocks' partials in the same way; the grid depends on H W only.  Two runs are
// bitwise equal.  Offsets are 64-bit across planes, int32 within one
// (H W <= 2^28).
#include "common.h"
#include "edt_core.h"
#include "lds_hist.h"
#include "../../include/vaeunet.h"

namespace {

constexpr int EC_COLS = 64, EC_SEG = 16;   // column pass: columns per block, chunks per column
constexpr int ER_BLK = 256;            // row pass: threads per row
constexpr int SBLK = 256;              // streaming passes
constexpr int SNB = 1024;              // their blocks per plane, at most
constexpr unsigned EPLANES = 65535;    // grid.y; further planes are looped over

static_assert(VU_EDT_INF == EDT_INF, "edt_core.h restates the sentinel");
static_assert(VU_EDT_MAX_DIM <= EDT_NONE && EDT_NONE <= 65535, "a vertical distance, and EDT_NONE, fit 16 bits");

typedef unsigned long long ull;

VU_DEV bool is_fg(float v, float thr) { return v > thr; }       // NaN: background
VU_DEV bool is_fg(uint8_t v, float) { return v != 0; }

// is (y, x) of plane src a site?  y, x inside the plane
template <typename T>
VU_DEV bool boundary_at(const T* __restrict__ src, int H, int W, int y, int x, float thr) {
  if (!is_fg(src[y * W + x], thr)) return false;
  const bool up = y > 0 && is_fg(src[(y - 1) * W + x], thr);
  const bool dn = y + 1 < H && is_fg(src[(y + 1) * W + x], thr);
  const bool lf = x > 0 && is_fg(src[y * W + x - 1], thr);
  const bool rt = x + 1 < W && is_fg(src[y * W + x + 1], thr);
  return !(up && dn && lf && rt);
}

// ---- column pass ---------------------------------------------------------------
// A block takes EC_COLS neighbouring columns (one wave: coalesced rows of 64) and
// cuts each into EC_SEG chunks of rows, one thread per (chunk, column).
//   1. the chunk's own down scan from EDT_NONE goes to the output; the rows of its
//      first and last site go to LDS
//   2. the carries: the distance the row above the chunk has to the nearest site
//      of the chunks above it, and the row below the chunk to the nearest site of
//      the chunks below, from the LDS table
//   3. the up scan: a row the chunk's own scan left at EDT_NONE takes the carry
//      from above, the up scan starts from the carry from below
// Both scans advance by edt_col_step; only the start values differ from a scan of
// the whole column.
template <typename T>
VU_DEV bool site_at(const T* __restrict__ src, int H, int W, int y, int col, int mode, float thr) {
  if (mode == VU_EDT_TO_BOUNDARY) return boundary_at(src, H, W, y, col, thr);
  return is_fg(src[y * W + col], thr) == (mode == VU_EDT_TO_FOREGROUND);
}

template <typename T>
__global__ void __launch_bounds__(EC_COLS * EC_SEG)
edt_col_kernel(const T* __restrict__ x, float thr, int mode, int64_t planes, int H, int W, int32_t* __restrict__ g) {
  __shared__ int32_t first[EC_SEG][EC_COLS], last[EC_SEG][EC_COLS];   // absolute rows, -1: the chunk has no site
  const int lane = threadIdx.x % EC_COLS, seg = threadIdx.x / EC_COLS;
  const int col = (int)blockIdx.x * EC_COLS + lane;
  const int rows = (H + EC_SEG - 1) / EC_SEG;
  const int y0 = min(seg * rows, H), y1 = min(y0 + rows, H);          // [y0, y1), empty past the plane
  const bool in = col < W;
  const int64_t n = (int64_t)H * W;
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    const T* src = x + plane * n;
    int32_t* dst = g + plane * n;
    int32_t d = EDT_NONE, f = -1, l = -1;
    if (in) {
#pragma unroll 4
      for (int y = y0; y < y1; ++y) {
        const bool site = site_at(src, H, W, y, col, mode, thr);
        d = edt_col_step(d, site);
        dst[y * W + col] = d;
        if (site) {
          f = f < 0 ? y : f;
          l = y;
        }
      }
    }
    first[seg][lane] = f;
    last[seg][lane] = l;
    __syncthreads();
    if (in && y0 < y1) {
      const int32_t above = edt_chunk_above(&last[0][lane], EC_COLS, seg, y0);             // of the row y0 - 1
      d = edt_chunk_below(&first[0][lane], EC_COLS, seg, EC_SEG, y1);                      // of the row y1
#pragma unroll 4
      for (int y = y1 - 1; y >= y0; --y) {
        const int o = y * W + col;
        const int32_t down = edt_chunk_down(dst[o], above, y - y0);
        d = edt_col_step(d, down == 0);
        dst[o] = edt_col_min(down, d);
      }
    }
    __syncthreads();
  }
}

VU_DEV void store_dist(int32_t* p, int32_t d2) { *p = d2; }
VU_DEV void store_dist(float* p, int32_t d2) {
  *p = d2 == EDT_INF ? __uint_as_float(0x7f800000u) : (float)sqrt((double)d2);
}

// ---- row pass ------------------------------------------------------------------
// in place: the row is read into LDS whole before any of it is written
template <typename OUT>
__global__ void __launch_bounds__(ER_BLK)
edt_row_kernel(int32_t* g, int64_t planes, int H, int W) {
  extern __shared__ uint16_t row[];
  const int64_t n = (int64_t)H * W;
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
      int32_t* src = g + plane * n + (int64_t)y * W;
      int any = 0;
      for (int xx = threadIdx.x; xx < W; xx += ER_BLK) {
        const int32_t v = src[xx];
        row[xx] = (uint16_t)v;
        any |= v != EDT_NONE;
      }
      any = __syncthreads_or(any);
      OUT* dst = reinterpret_cast<OUT*>(src);
      for (int xx = threadIdx.x; xx < W; xx += ER_BLK)
        store_dist(dst + xx, any ? edt_row_search(row, W, xx) : EDT_INF);
      __syncthreads();
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(SBLK)
boundary_kernel(const T* __restrict__ x, float thr, int64_t planes, int H, int W, uint8_t* __restrict__ out) {
  const int64_t n = (int64_t)H * W;
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y)
    for (int64_t i = (int64_t)blockIdx.x * SBLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SBLK)
      out[plane * n + i] = boundary_at(x + plane * n, H, W, (int)(i / W), (int)(i % W), thr) ? 1 : 0;
}

// ---- surface statistics --------------------------------------------------------
// per set s (0: P -> G, 1: G -> P): n, max d^2, number within tolerance, sum of sqrt(d^2)
struct Acc {
  ull n[2], mx[2], c[2];
  double s[2];
};

VU_DEV void acc_zero(Acc& a) {
#pragma unroll
  for (int s = 0; s < 2; ++s) { a.n[s] = 0; a.mx[s] = 0; a.c[s] = 0; a.s[s] = 0.0; }
}

VU_DEV void acc_merge(Acc& a, const Acc& b) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    a.n[s] += b.n[s];
    a.mx[s] = a.mx[s] > b.mx[s] ? a.mx[s] : b.mx[s];
    a.c[s] += b.c[s];
    a.s[s] += b.s[s];
  }
}

// the block's total on thread 0: a shuffle butterfly per wave, then the waves in order.  sh: [8][SBLK / 64] words
VU_DEV void acc_block(Acc& a, ull* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Acc b;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      b.n[s] = __shfl_xor(a.n[s], o, 64);
      b.mx[s] = __shfl_xor(a.mx[s], o, 64);
      b.c[s] = __shfl_xor(a.c[s], o, 64);
      b.s[s] = __shfl_xor(a.s[s], o, 64);
    }
    acc_merge(a, b);
  }
  constexpr int NW = SBLK / 64;
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      sh[(0 + s) * NW + wv] = a.n[s];
      sh[(2 + s) * NW + wv] = a.mx[s];
      sh[(4 + s) * NW + wv] = a.c[s];
      sh[(6 + s) * NW + wv] = (ull)__double_as_longlong(a.s[s]);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    acc_zero(a);
    for (int w = 0; w < NW; ++w) {
      Acc b;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        b.n[s] = sh[(0 + s) * NW + w];
        b.mx[s] = sh[(2 + s) * NW + w];
        b.c[s] = sh[(4 + s) * NW + w];
        b.s[s] = __longlong_as_double((long long)sh[(6 + s) * NW + w]);
      }
      acc_merge(a, b);
    }
  }
  __syncthreads();
}

// one pixel of set s: its key is the other side's transform.  EDT_INF (the other set is empty) enters nothing
VU_DEV void acc_pixel(Acc& a, int s, int32_t key, int tol2) {
  a.n[s] += 1;
  if (key == EDT_INF) return;
  a.mx[s] = a.mx[s] > (ull)key ? a.mx[s] : (ull)key;
  a.c[s] += key <= tol2;
  a.s[s] += sqrt((double)key);
}

// bp[plane][block][8] = n0, n1, max0, max1, within0, within1, sum0 bits, sum1 bits
__global__ void __launch_bounds__(SBLK)
surf_reduce_kernel(const int32_t* __restrict__ dP, const int32_t* __restrict__ dG, int64_t planes, int64_t n,
                   int tol2, ull* __restrict__ bp) {
  __shared__ ull sh[8 * (SBLK / 64)];
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    const int32_t *a = dP + plane * n, *b = dG + plane * n;
    Acc acc;
    acc_zero(acc);
    for (int64_t i = (int64_t)blockIdx.x * SBLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SBLK) {
      const int32_t p = a[i], g = b[i];
      if (p == 0) acc_pixel(acc, 0, g, tol2);
      if (g == 0) acc_pixel(acc, 1, p, tol2);
    }
    acc_block(acc, sh);
    if (threadIdx.x == 0) {
      ull* o = bp + (plane * gridDim.x + blockIdx.x) * 8;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        o[0 + s] = acc.n[s];
        o[2 + s] = acc.mx[s];
        o[4 + s] = acc.c[s];
        o[6 + s] = (ull)__double_as_longlong(acc.s[s]);
      }
    }
  }
}

// one block per plane: the blocks' partials in a fixed order -> stats, sums, and the select's start: prefix 0, the
// percentile's rank (0 on an undefined plane: the select passes skip it), zeroed digit histograms
__global__ void __launch_bounds__(SBLK)
surf_finalize_kernel(const ull* __restrict__ bp, int nb, int64_t planes, int q, long long* __restrict__ stats,
                     double* __restrict__ sums, uint32_t* __restrict__ state, uint32_t* __restrict__ hist) {
  __shared__ ull sh[8 * (SBLK / 64)];
  for (int64_t plane = blockIdx.x; plane < planes; plane += gridDim.x) {
    Acc acc;
    acc_zero(acc);
    for (int k = threadIdx.x; k < nb; k += SBLK) {
      const ull* o = bp + (plane * nb + k) * 8;
      Acc b;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        b.n[s] = o[0 + s];
        b.mx[s] = o[2 + s];
        b.c[s] = o[4 + s];
        b.s[s] = __longlong_as_double((long long)o[6 + s]);
      }
      acc_merge(acc, b);
    }
    acc_block(acc, sh);
    for (int k = threadIdx.x; k < 512; k += SBLK) hist[plane * 512 + k] = 0;
    if (threadIdx.x == 0) {
      const bool defined = acc.n[0] > 0 && acc.n[1] > 0;
      long long* st = stats + plane * 8;
      st[0] = (long long)acc.n[0];
      st[1] = (long long)acc.n[1];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        st[2 + s] = defined ? (long long)acc.mx[s] : -1;
        st[4 + s] = -1;   // the select's last pass writes it on a defined plane
        st[6 + s] = defined ? (long long)acc.c[s] : -1;
        sums[plane * 2 + s] = defined ? acc.s[s] : 0.0;
        state[plane * 4 + s] = 0;
        state[plane * 4 + 2 + s] = defined ? (uint32_t)edt_rank(q, (int64_t)acc.n[s]) : 0u;
      }
    }
  }
}

// pass p of the select: the digit histograms of the keys still in play, both sets
__global__ void __launch_bounds__(SBLK)
surf_hist_kernel(const int32_t* __restrict__ dP, const int32_t* __restrict__ dG, int64_t planes, int64_t n, int p,
                 const uint32_t* __restrict__ state, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[512];
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    const uint32_t pre0 = state[plane * 4], pre1 = state[plane * 4 + 1];
    if (state[plane * 4 + 2] == 0) continue;   // undefined plane (both ranks are 0): block-uniform
    for (int k = threadIdx.x; k < 512; k += SBLK) h[k] = 0;
    __syncthreads();
    const int32_t *a = dP + plane * n, *b = dG + plane * n;
    // whole waves stay in the loop: the aggregation needs them converged
    for (int64_t base = (int64_t)blockIdx.x * SBLK; base < n; base += (int64_t)gridDim.x * SBLK) {
      const int64_t i = base + threadIdx.x;
      const bool in = i < n;
      const uint32_t kp = in ? (uint32_t)a[i] : 1u, kg = in ? (uint32_t)b[i] : 1u;
      hist_add<2>(h, edt_sel_digit(kg, p), in && kp == 0 && edt_sel_match(kg, pre0, p));
      hist_add<2>(h + 256, edt_sel_digit(kp, p), in && kg == 0 && edt_sel_match(kp, pre1, p));
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 512; k += SBLK)
      if (h[k]) atomicAdd(&hist[plane * 512 + k], h[k]);
    __syncthreads();
  }
}

// one block per plane: thread s settles set s's digit, then the histograms are zeroed for the next pass
__global__ void __launch_bounds__(64)
surf_select_kernel(int64_t planes, int p, uint32_t* __restrict__ state, uint32_t* __restrict__ hist,
                   long long* __restrict__ stats) {
  for (int64_t plane = blockIdx.x; plane < planes; plane += gridDim.x) {
    if (threadIdx.x < 2) {
      const int s = threadIdx.x;
      uint32_t rank = state[plane * 4 + 2 + s];
      if (rank) {
        const int d = edt_sel_step(hist + plane * 512 + s * 256, &rank);
        const uint32_t prefix = (state[plane * 4 + s] << 8) | (uint32_t)d;
        state[plane * 4 + s] = prefix;
        state[plane * 4 + 2 + s] = rank;
        if (p == 3) stats[plane * 8 + 4 + s] = (long long)prefix;
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 512; k += 64) hist[plane * 512 + k] = 0;
    __syncthreads();
  }
}

constexpr int MBLK = 256;

__global__ void __launch_bounds__(MBLK)
surf_metrics_kernel(const long long* __restrict__ stats, const double* __restrict__ sums, int64_t planes,
                    double* out, double* __restrict__ acc, long long* __restrict__ nacc) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int64_t r = threadIdx.x; r < planes; r += MBLK) {
    const long long* st = stats + r * 8;
    double* o = out + r * 4;
    if (st[0] > 0 && st[1] > 0) {
      const double np = (double)(st[0] + st[1]);
      const double a = sqrt((double)st[4]), b = sqrt((double)st[5]);
      o[0] = sqrt((double)(st[2] > st[3] ? st[2] : st[3]));
      o[1] = a > b ? a : b;
      o[2] = (sums[r * 2] + sums[r * 2 + 1]) / np;
      o[3] = (double)(st[6] + st[7]) / np;
    } else {
      o[0] = o[1] = o[2] = o[3] = nan;
    }
  }
  __syncthreads();   // the block's own global writes are visible to it after the barrier
  if (threadIdx.x == 0 && acc) {
    double t[4] = {acc[0], acc[1], acc[2], acc[3]};
    long long defined = 0;
    for (int64_t r = 0; r < planes; ++r) {   // plane order
      if (!(stats[r * 8] > 0 && stats[r * 8 + 1] > 0)) continue;
      ++defined;
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] += out[r * 4 + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = t[k];
    nacc[0] += defined;
    nacc[1] += planes;
  }
}

bool dims_ok(int64_t planes, int H, int W) {
  return planes >= 0 && H >= 0 && W >= 0 && H <= VU_EDT_MAX_DIM && W <= VU_EDT_MAX_DIM;
}
bool dtype_ok(int d) { return d == VU_CCL_U8 || d == VU_CCL_F32; }

unsigned plane_grid(int64_t planes) { return (unsigned)(planes < EPLANES ? planes : EPLANES); }

int stream_blocks(int64_t n) {
  int64_t nb = (n + SBLK * 4 - 1) / (SBLK * 4);
  return (int)(nb > SNB ? SNB : (nb < 1 ? 1 : nb));
}

// the transform of every plane into out (int32 g, then OUT in place)
void launch_edt(const void* x, int dtype, float thr, int mode, int64_t planes, int H, int W, void* out, bool out_f32,
                hipStream_t st) {
  const dim3 cgrid((unsigned)((W + EC_COLS - 1) / EC_COLS), plane_grid(planes));
  int32_t* g = static_cast<int32_t*>(out);
  if (dtype == VU_CCL_U8)
    hipLaunchKernelGGL(edt_col_kernel<uint8_t>, cgrid, dim3(EC_COLS * EC_SEG), 0, st, static_cast<const uint8_t*>(x), thr, mode,
                       planes, H, W, g);
  else
    hipLaunchKernelGGL(edt_col_kernel<float>, cgrid, dim3(EC_COLS * EC_SEG), 0, st, static_cast<const float*>(x), thr, mode,
                       planes, H, W, g);
  const dim3 rgrid((unsigned)H, plane_grid(planes));
  const size_t lds = (size_t)W * sizeof(uint16_t);
  if (out_f32) hipLaunchKernelGGL(edt_row_kernel<float>, rgrid, dim3(ER_BLK), lds, st, g, planes, H, W);
  else hipLaunchKernelGGL(edt_row_kernel<int32_t>, rgrid, dim3(ER_BLK), lds, st, g, planes, H, W);
}

// workspace of vu_surface_stats: dP, dG int32 [planes][H W]; bp [planes][SNB][8] 8-byte words; hist uint32
// [planes][512]; state uint32 [planes][4]
int64_t ws_bytes(int64_t planes, int64_t n) { return planes * (2 * n * 4 + (int64_t)SNB * 64 + 512 * 4 + 4 * 4); }

}  // namespace

extern "C" int64_t vu_edt_workspace_bytes(int64_t planes, int H, int W) {
  if (!dims_ok(planes, H, W)) return -1;
  return ws_bytes(planes, (int64_t)H * W);
}

extern "C" int vu_edt(const void* x, int dtype, float threshold, int mode, int64_t planes, int H, int W, void* out,
                      int out_f32, void* stream) {
  if (!dims_ok(planes, H, W) || !dtype_ok(dtype) || (out_f32 != 0 && out_f32 != 1) ||
      (mode != VU_EDT_TO_FOREGROUND && mode != VU_EDT_TO_BACKGROUND && mode != VU_EDT_TO_BOUNDARY))
    return (int)hipErrorInvalidValue;
  if (planes == 0 || H == 0 || W == 0) return 0;
  if (!x || !out) return (int)hipErrorInvalidValue;
  launch_edt(x, dtype, threshold, mode, planes, H, W, out, out_f32 != 0, (hipStream_t)stream);
  return (int)hipGetLastError();
}

extern "C" int vu_edt_boundary(const void* x, int dtype, float threshold, int64_t planes, int H, int W, uint8_t* out,
                               void* stream) {
  if (!dims_ok(planes, H, W) || !dtype_ok(dtype)) return (int)hipErrorInvalidValue;
  if (planes == 0 || H == 0 || W == 0) return 0;
  if (!x || !out) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)stream_blocks((int64_t)H * W), plane_grid(planes));
  if (dtype == VU_CCL_U8)
    hipLaunchKernelGGL(boundary_kernel<uint8_t>, grid, dim3(SBLK), 0, (hipStream_t)stream,
                       static_cast<const uint8_t*>(x), threshold, planes, H, W, out);
  else
    hipLaunchKernelGGL(boundary_kernel<float>, grid, dim3(SBLK), 0, (hipStream_t)stream,
                       static_cast<const float*>(x), threshold, planes, H, W, out);
  return (int)hipGetLastError();
}

extern "C" int vu_surface_stats(const void* pred, int dtype, float threshold, const void* gt, int gt_dtype,
                                int64_t planes, int H, int W, int q, int tol2, int64_t* stats, double* sums,
                                void* workspace, void* stream) {
  if (!dims_ok(planes, H, W) || !dtype_ok(dtype) || !dtype_ok(gt_dtype) || q < 1 || q > 100 || tol2 < 0)
    return (int)hipErrorInvalidValue;
  if (planes == 0 || H == 0 || W == 0) return 0;
  if (!pred || !gt || !stats || !sums || !workspace) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)H * W;
  int32_t* dP = static_cast<int32_t*>(workspace);
  int32_t* dG = dP + planes * n;
  ull* bp = reinterpret_cast<ull*>(dG + planes * n);
  uint32_t* hist = reinterpret_cast<uint32_t*>(bp + planes * SNB * 8);
  uint32_t* state = hist + planes * 512;
  launch_edt(pred, dtype, threshold, VU_EDT_TO_BOUNDARY, planes, H, W, dP, false, st);
  launch_edt(gt, gt_dtype, 0.5f, VU_EDT_TO_BOUNDARY, planes, H, W, dG, false, st);
  const int nb = stream_blocks(n);
  const dim3 grid((unsigned)nb, plane_grid(planes));
  long long* sp = reinterpret_cast<long long*>(stats);
  hipLaunchKernelGGL(surf_reduce_kernel, grid, dim3(SBLK), 0, st, dP, dG, planes, n, tol2, bp);
  hipLaunchKernelGGL(surf_finalize_kernel, dim3(plane_grid(planes)), dim3(SBLK), 0, st, bp, nb, planes, q, sp, sums,
                     state, hist);
  for (int p = 0; p < 4; ++p) {
    hipLaunchKernelGGL(surf_hist_kernel, grid, dim3(SBLK), 0, st, dP, dG, planes, n, p, state, hist);
    hipLaunchKernelGGL(surf_select_kernel, dim3(plane_grid(planes)), dim3(64), 0, st, planes, p, state, hist, sp);
  }
  return (int)hipGetLastError();
}

extern "C" int vu_surface_metrics(const int64_t* stats, const double* sums, int64_t planes, double* out, double* acc,
                                  int64_t* nacc, void* stream) {
  if (planes < 0 || (acc != nullptr) != (nacc != nullptr)) return (int)hipErrorInvalidValue;
  if (planes == 0) return 0;
  if (!stats || !sums || !out) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(surf_metrics_kernel, dim3(1), dim3(MBLK), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(stats), sums, planes, out, acc,
                     reinterpret_cast<long long*>(nacc));
  return (int)hipGetLastError();
}
