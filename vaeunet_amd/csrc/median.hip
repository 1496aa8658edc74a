// Median blur of the patch loader on image batches
// [B][H][W][3] fp32 (NHWC), per channel, window 2r + 1 with a per-sample radius
// r in 0..3, replicated border.  Definition: include/vaeunet.h.
//
//   vu_median_blur  one block per 32 x 32 output tile, the structure of
//                   vu_blur_sep (filters.hip): the tile plus a halo of the
//                   sample's radius (replicate: the source row / column of
//                   every tile row / column clamped once per block into two
//                   index maps) goes to LDS as rows of 3 (32 + 2r) values,
//                   channels interleaved, so the lanes read at unit stride.
//                   LDS holds the KEYS of the values, an order-preserving map
//                   of the float bits to uint32, converted once per loaded
//                   element; the selection network (median_select.h) runs on
//                   integer min / max and the selected key is converted back
//                   at the store.  No value passes through floating-point
//                   arithmetic: the output is bitwise one of the inputs, NaN
//                   payloads included.  The radius is block-uniform; each
//                   radius is a template instantiation (constant window and
//                   row lengths, the window in registers), r = 0 is a
//                   streaming copy.
//
// Every source index is clamped into [0, size): no table value can form an
// address outside the sample.
#include "common.h"
#include "median_select.h"
#include "../../include/vaeunet.h"

namespace {

constexpr int MD_T = 32, MD_BLK = 512;               // output tile edge, threads per block
constexpr int MD_SPAN = MD_T + 2 * VU_MEDIAN_RMAX;   // tile + halo at the largest radius

// total order of the float bit patterns as uint32: negatives reversed below the positives, -0 < +0, NaNs at the ends
VU_DEV uint32_t to_key(uint32_t u) { return (u >> 31) ? ~u : (u | 0x80000000u); }
VU_DEV uint32_t from_key(uint32_t k) { return (k >> 31) ? (k & 0x7fffffffu) : ~k; }

// One 32 x 32 output tile at radius R >= 1.  keys: (32 + 2R) rows of 3 (32 + 2R) keys; mx / my: the source column /
// row of every tile column / row, clamped.
template <int R>
VU_DEV void median_tile(const uint32_t* __restrict__ src, int H, int W, uint32_t* __restrict__ dst, int x0, int y0,
                        uint32_t* keys, int* mx, int* my) {
  constexpr int SP = MD_T + 2 * R, ROW = 3 * SP, OROW = 3 * MD_T, K = 2 * R + 1;
  const int t = threadIdx.x;
  if (t < SP) mx[t] = min(max(x0 - R + t, 0), W - 1);
  else if (t >= 64 && t < 64 + SP) my[t - 64] = min(max(y0 - R + (t - 64), 0), H - 1);
  __syncthreads();
  for (int i = t; i < SP * ROW; i += MD_BLK) {
    const int row = i / ROW, e = i - row * ROW, px = e / 3, c = e - 3 * px;
    keys[i] = to_key(src[((int64_t)my[row] * W + mx[px]) * 3 + c]);
  }
  __syncthreads();
  for (int i = t; i < MD_T * OROW; i += MD_BLK) {
    const int y = i / OROW, j = i - y * OROW;
    const uint32_t* p = keys + y * ROW + j;
    uint32_t v[K * K];
#pragma unroll
    for (int dy = 0; dy < K; ++dy)
#pragma unroll
      for (int dx = 0; dx < K; ++dx) v[dy * K + dx] = p[dy * ROW + 3 * dx];
    const uint32_t m = median_select<K * K>(v);   // MedianOrder<uint32_t>: v_min_u32 / v_max_u32
    if (y0 + y < H && x0 + j / 3 < W) dst[((int64_t)(y0 + y) * W + x0) * 3 + j] = from_key(m);
  }
}

__global__ void __launch_bounds__(MD_BLK)
median_blur_kernel(const uint32_t* __restrict__ img, int H, int W, const float* __restrict__ radius,
                   uint32_t* __restrict__ out) {
  __shared__ uint32_t keys[MD_SPAN * MD_SPAN * 3];
  __shared__ int mx[MD_SPAN], my[MD_SPAN];
  const int b = blockIdx.z, x0 = blockIdx.x * MD_T, y0 = blockIdx.y * MD_T;
  const int r = (int)fminf(fmaxf(radius[b], 0.f), (float)VU_MEDIAN_RMAX);   // block-uniform: a scalar load; NaN -> 0
  const uint32_t* src = img + (int64_t)b * H * W * 3;
  uint32_t* dst = out + (int64_t)b * H * W * 3;
  switch (r) {
    case 0:   // off: the bits, copied
      for (int i = threadIdx.x; i < MD_T * MD_T * 3; i += MD_BLK) {
        const int y = i / (3 * MD_T), j = i - y * (3 * MD_T);
        if (y0 + y < H && x0 + j / 3 < W) {
          const int64_t e = ((int64_t)(y0 + y) * W + x0) * 3 + j;
          dst[e] = src[e];
        }
      }
      break;
    case 1: median_tile<1>(src, H, W, dst, x0, y0, keys, mx, my); break;
    case 2: median_tile<2>(src, H, W, dst, x0, y0, keys, mx, my); break;
    default: median_tile<3>(src, H, W, dst, x0, y0, keys, mx, my); break;
  }
}

}  // namespace

extern "C" int vu_median_blur(const float* img, int B, int H, int W, const float* radius, float* out, void* stream) {
  if (B < 0 || H < 0 || W < 0) return (int)hipErrorInvalidValue;
  if (B == 0 || H == 0 || W == 0) return 0;
  // the halo reads make in-place wrong; grid.y / grid.z limits
  if (!img || !radius || !out || out == img || B > 65535 || H > 32768 || W > 32768) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((W + MD_T - 1) / MD_T), (unsigned)((H + MD_T - 1) / MD_T), (unsigned)B);
  hipLaunchKernelGGL(median_blur_kernel, grid, dim3(MD_BLK), 0, (hipStream_t)stream, (const uint32_t*)img, H, W,
                     radius, (uint32_t*)out);
  return (int)hipGetLastError();
}
