// The two neighbourhood transforms of the patch loader: CLAHE
// on an integer luma and a separable symmetric blur, both on image batches
// [B][H][W][3] fp32 (NHWC) and both ahead of vu_augment_patch (§4.8), so they
// see the un-warped patch.  Definitions: include/vaeunet.h.
//
//   vu_clahe_luts   one block per (tile, sample): LDS histogram of the 8-bit
//                   luma of the tile (integer atomics, equal bins of a wave
//                   aggregated first: a constant tile is one bin), clip and
//                   redistribute, a 256-wide inclusive scan, 256 LUT bytes.
//                   Everything is integer: the result does not depend on order.
//   vu_clahe_apply  one thread per pixel in the 32 x 8 tile of §4.8; the tile
//                   pair and weight of the block's 32 columns and 8 rows are
//                   formed once per block in LDS (no per-pixel division); the
//                   four LUT bytes of a pixel are gathered through L1 / L2
//                   (B TY TX 256 bytes: 128 KiB at 8 x 8 x 8).
//   vu_blur_sep     one block per 32 x 32 output tile: the tile plus a halo of
//                   the sample's radius (reflect101, folded once per block into
//                   two index maps) goes to LDS, the horizontal pass is written
//                   to LDS, the vertical pass is stored: the intermediate never
//                   reaches HBM.  The radius is block-uniform; each radius is a
//                   template instantiation (constant trip counts and row
//                   lengths), r = 0 is a streaming copy.
//
// Every tile index is clamped and every tap index folded into [0, size): no
// table value can form an address outside the sample.
#include "common.h"
#include "lds_hist.h"
#include "reflect.h"
#include "../../include/vaeunet.h"

namespace {

constexpr int FT_TW = 32, FT_TH = 8;            // pixel tile of the per-pixel kernel (as augment.hip)
constexpr int CL_BINS = 256, CL_MAX_TILES = 16, CL_BLK = 256;
constexpr int BL_RMAX = 7, BL_NTAB = 2 + BL_RMAX;
constexpr int BL_T = 32, BL_BLK = 512;          // output tile edge, threads per block
constexpr int BL_SPAN = BL_T + 2 * BL_RMAX;     // tile + halo at the largest radius

// 8-bit value of a channel: two separately rounded fp32 operations (no fma); NaN -> 0
VU_DEV int quant8(float v) { return (int)__fadd_rn(__fmul_rn(fminf(fmaxf(v, 0.f), 1.f), 255.0f), 0.5f); }

VU_DEV int luma8(float r, float g, float b) { return (77 * quant8(r) + 150 * quant8(g) + 29 * quant8(b) + 128) >> 8; }

// first pixel of tile t of an axis of n pixels in T tiles (t n <= 16 * 32768)
VU_DEV int tile_start(int t, int n, int T) { return t * n / T; }
// twice the centre of tile t
VU_DEV int tile_centre2(int t, int n, int T) { return tile_start(t, n, T) + tile_start(t + 1, n, T) - 1; }

__global__ void __launch_bounds__(CL_BLK)
clahe_luts_kernel(const float* __restrict__ img, int H, int W, const float* __restrict__ clip, int TY, int TX,
                  uint8_t* __restrict__ luts) {
  __shared__ uint32_t h[CL_BINS], part[2][CL_BLK / 64];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint8_t* lut = luts + ((int64_t)b * (TY * TX) + tile) * CL_BINS;
  const float c = clip[b];
  if (!(c > 0.f)) {   // off (0, negative, NaN): block-uniform; the apply kernel does not read it
    lut[tid] = (uint8_t)tid;
    return;
  }
  const int ty = tile / TX, tx = tile - ty * TX;
  const int y0 = tile_start(ty, H, TY), x0 = tile_start(tx, W, TX);
  const int tw = tile_start(tx + 1, W, TX) - x0, A = tw * (tile_start(ty + 1, H, TY) - y0);
  h[tid] = 0;
  __syncthreads();
  const FastDiv dw((uint32_t)tw);
  const float* base = img + ((int64_t)b * H + y0) * W * 3;
  for (int p0 = 0; p0 < A; p0 += CL_BLK) {   // whole waves iterate together
    const bool valid = p0 + tid < A;
    const int p = valid ? p0 + tid : 0;
    const int row = (int)dw.div((uint32_t)p), col = p - row * tw;
    const float* px = base + ((int64_t)row * W + x0 + col) * 3;
    hist_add<1>(h, luma8(px[0], px[1], px[2]), valid);   // one peel: a constant tile is one atomic per wave
  }
  __syncthreads();

  // clip limit: t = clip A / 256 in fp32; t >= A means no clipping
  const float t = __fmul_rn(__fmul_rn(c, (float)A), 0.00390625f);
  const uint32_t lim = t >= (float)A ? (uint32_t)A : (uint32_t)max(1, (int)t);
  uint32_t v = h[tid];
  uint32_t ex = v > lim ? v - lim : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ex += __shfl_xor(ex, o, 64);
  if (lane == 0) part[0][wv] = ex;
  __syncthreads();
  const uint32_t E = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
  // OpenCV's order: clip, an equal share to every bin, the remainder one each to every step-th bin
  v = min(v, lim) + E / CL_BINS;
  const int r = (int)(E % CL_BINS);
  if (r > 0) {
    const int step = max(CL_BINS / r, 1);
    if (tid % step == 0 && tid / step < r) ++v;
  }
  // inclusive scan over the 256 bins
  uint32_t s = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t n = __shfl_up(s, o, 64);
    if (lane >= o) s += n;
  }
  if (lane == 63) part[1][wv] = s;
  __syncthreads();
  for (int q = 0; q < wv; ++q) s += part[1][q];
  lut[tid] = (uint8_t)(((uint64_t)s * 255u + (uint64_t)(A / 2)) / (uint64_t)A);
}

__global__ void __launch_bounds__(FT_TW * FT_TH)
clahe_apply_kernel(const float* __restrict__ img, int H, int W, const float* __restrict__ clip, int TY, int TX,
                   const uint8_t* __restrict__ luts, float* __restrict__ out) {
  // lower / upper tile and the weight of the upper one: the block's 32 columns, then its 8 rows
  __shared__ int lo[FT_TW + FT_TH], hi[FT_TW + FT_TH];
  __shared__ float wt[FT_TW + FT_TH];
  const int b = blockIdx.z, t = threadIdx.x;
  const bool on = clip[b] > 0.f;   // block-uniform
  if (on && t < FT_TW + FT_TH) {
    const bool col = t < FT_TW;
    const int n = col ? W : H, T = col ? TX : TY;
    const int p = min(col ? blockIdx.x * FT_TW + t : blockIdx.y * FT_TH + (t - FT_TW), n - 1);
    // the last tile whose centre is <= p is the pixel's own tile k or the one before it
    const int k = ((p + 1) * T - 1) / n;
    const int a = 2 * p >= tile_centre2(k, n, T) ? k : k - 1;
    int l = min(max(a, 0), T - 1), u = l;
    float w = 0.f;
    if (a >= 0 && a < T - 1) {
      const int ca = tile_centre2(a, n, T), cb = tile_centre2(a + 1, n, T);
      u = a + 1;
      w = (float)(2 * p - ca) / (float)(cb - ca);
    }
    lo[t] = l; hi[t] = u; wt[t] = w;
  }
  __syncthreads();
  const int lx = t & (FT_TW - 1), ly = t / FT_TW;
  const int j = blockIdx.x * FT_TW + lx, i = blockIdx.y * FT_TH + ly;
  if (i >= H || j >= W) return;
  const int64_t pix = ((int64_t)b * H + i) * W + j;
  const float* src = img + pix * 3;
  float* dst = out + pix * 3;
  const float v0 = src[0], v1 = src[1], v2 = src[2];
  if (!on) {
    dst[0] = v0; dst[1] = v1; dst[2] = v2;
    return;
  }
  const int Y = luma8(v0, v1, v2);
  const uint8_t* L = luts + (int64_t)b * (TY * TX) * CL_BINS + Y;
  const int x1 = lo[lx], x2 = hi[lx], y1 = lo[FT_TW + ly], y2 = hi[FT_TW + ly];
  const float wx = wt[lx], wy = wt[FT_TW + ly];
  const float l11 = (float)L[(y1 * TX + x1) * CL_BINS], l12 = (float)L[(y1 * TX + x2) * CL_BINS];
  const float l21 = (float)L[(y2 * TX + x1) * CL_BINS], l22 = (float)L[(y2 * TX + x2) * CL_BINS];
  const float top = l11 + wx * (l12 - l11), bot = l21 + wx * (l22 - l21);
  const float d = ((top + wy * (bot - top)) - (float)Y) * 0.00392156862745098f;
  dst[0] = fminf(fmaxf(v0 + d, 0.f), 1.f);   // NaN -> 0
  dst[1] = fminf(fmaxf(v1 + d, 0.f), 1.f);
  dst[2] = fminf(fmaxf(v2 + d, 0.f), 1.f);
}

// One 32 x 32 output tile at radius R >= 1.  in: (32 + 2R) rows of 3 (32 + 2R) floats; hr: the horizontal pass of
// those rows, 96 floats each; mx / my: the source column / row of every tile column / row, folded.
template <int R>
VU_DEV void blur_tile(const float* __restrict__ src, int H, int W, const float* __restrict__ w,
                      float* __restrict__ dst, int x0, int y0, float* in, float* hr, int* mx, int* my) {
  constexpr int SP = BL_T + 2 * R, ROW = 3 * SP, HROW = 3 * BL_T;
  const int t = threadIdx.x;
  if (t < SP) mx[t] = reflect101(x0 - R + t, W);
  else if (t >= 64 && t < 64 + SP) my[t - 64] = reflect101(y0 - R + (t - 64), H);
  float wk[R + 1];
#pragma unroll
  for (int k = 0; k <= R; ++k) wk[k] = w[k];   // block-uniform: scalar loads
  __syncthreads();
  for (int i = t; i < SP * ROW; i += BL_BLK) {
    const int row = i / ROW, e = i - row * ROW, px = e / 3, c = e - 3 * px;
    in[i] = src[((int64_t)my[row] * W + mx[px]) * 3 + c];
  }
  __syncthreads();
  for (int i = t; i < SP * HROW; i += BL_BLK) {
    const int row = i / HROW, j = i - row * HROW;
    const float* p = in + row * ROW + 3 * R + j;
    float acc = wk[0] * p[0];
#pragma unroll
    for (int k = 1; k <= R; ++k) acc = fmaf(wk[k], p[-3 * k] + p[3 * k], acc);
    hr[i] = acc;
  }
  __syncthreads();
  for (int i = t; i < BL_T * HROW; i += BL_BLK) {
    const int y = i / HROW, j = i - y * HROW;
    const float* p = hr + (y + R) * HROW + j;
    float acc = wk[0] * p[0];
#pragma unroll
    for (int k = 1; k <= R; ++k) acc = fmaf(wk[k], p[-k * HROW] + p[k * HROW], acc);
    if (y0 + y < H && x0 + j / 3 < W) dst[((int64_t)(y0 + y) * W + x0) * 3 + j] = acc;
  }
}

__global__ void __launch_bounds__(BL_BLK)
blur_sep_kernel(const float* __restrict__ img, int H, int W, const float* __restrict__ table,
                float* __restrict__ out) {
  __shared__ float in[BL_SPAN * BL_SPAN * 3], hr[BL_SPAN * BL_T * 3];
  __shared__ int mx[BL_SPAN], my[BL_SPAN];
  const int b = blockIdx.z, x0 = blockIdx.x * BL_T, y0 = blockIdx.y * BL_T;
  const float* tab = table + (int64_t)b * BL_NTAB;                  // block-uniform: scalar loads
  const int r = (int)fminf(fmaxf(tab[0], 0.f), (float)BL_RMAX);     // NaN -> 0
  const float* w = tab + 1;
  const float* src = img + (int64_t)b * H * W * 3;
  float* dst = out + (int64_t)b * H * W * 3;
  switch (r) {
    case 0: {   // both passes are one product: a copy where w_0 = 1
      const float w0 = w[0];
      for (int i = threadIdx.x; i < BL_T * BL_T * 3; i += BL_BLK) {
        const int y = i / (3 * BL_T), j = i - y * (3 * BL_T);
        if (y0 + y < H && x0 + j / 3 < W) {
          const int64_t e = ((int64_t)(y0 + y) * W + x0) * 3 + j;
          dst[e] = __fmul_rn(w0, __fmul_rn(w0, src[e]));
        }
      }
      break;
    }
    case 1: blur_tile<1>(src, H, W, w, dst, x0, y0, in, hr, mx, my); break;
    case 2: blur_tile<2>(src, H, W, w, dst, x0, y0, in, hr, mx, my); break;
    case 3: blur_tile<3>(src, H, W, w, dst, x0, y0, in, hr, mx, my); break;
    case 4: blur_tile<4>(src, H, W, w, dst, x0, y0, in, hr, mx, my); break;
    case 5: blur_tile<5>(src, H, W, w, dst, x0, y0, in, hr, mx, my); break;
    case 6: blur_tile<6>(src, H, W, w, dst, x0, y0, in, hr, mx, my); break;
    default: blur_tile<7>(src, H, W, w, dst, x0, y0, in, hr, mx, my); break;
  }
}

// the arguments both CLAHE entry points share; an empty batch passes whatever its pointers are
int check_clahe(int B, int H, int W, int TY, int TX, bool pointers) {
  if (B < 0 || H < 0 || W < 0 || TY < 1 || TY > CL_MAX_TILES || TX < 1 || TX > CL_MAX_TILES)
    return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  // grid.y / grid.z limits; (p + 1) T and t n stay far below 2^31
  if (!pointers || B > 65535 || H > 32768 || W > 32768 || TY > H || TX > W) return (int)hipErrorInvalidValue;
  return 0;
}

}  // namespace

extern "C" int vu_clahe_luts(const float* img, int B, int H, int W, const float* clip, int TY, int TX,
                             uint8_t* luts, void* stream) {
  const int rc = check_clahe(B, H, W, TY, TX, img && clip && luts);
  if (rc || B == 0) return rc;
  hipLaunchKernelGGL(clahe_luts_kernel, dim3((unsigned)(TY * TX), (unsigned)B), dim3(CL_BLK), 0, (hipStream_t)stream,
                     img, H, W, clip, TY, TX, luts);
  return (int)hipGetLastError();
}

extern "C" int vu_clahe_apply(const float* img, int B, int H, int W, const float* clip, int TY, int TX,
                              const uint8_t* luts, float* out, void* stream) {
  const int rc = check_clahe(B, H, W, TY, TX, img && clip && luts && out);
  if (rc || B == 0) return rc;
  const dim3 grid((unsigned)((W + FT_TW - 1) / FT_TW), (unsigned)((H + FT_TH - 1) / FT_TH), (unsigned)B);
  hipLaunchKernelGGL(clahe_apply_kernel, grid, dim3(FT_TW * FT_TH), 0, (hipStream_t)stream, img, H, W, clip, TY, TX,
                     luts, out);
  return (int)hipGetLastError();
}

extern "C" int vu_blur_sep(const float* img, int B, int H, int W, const float* table, float* out, void* stream) {
  if (B < 0 || H < 0 || W < 0) return (int)hipErrorInvalidValue;
  if (B == 0 || H == 0 || W == 0) return 0;
  if (!img || !table || !out || B > 65535 || H > 32768 || W > 32768) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((W + BL_T - 1) / BL_T), (unsigned)((H + BL_T - 1) / BL_T), (unsigned)B);
  hipLaunchKernelGGL(blur_sep_kernel, grid, dim3(BL_BLK), 0, (hipStream_t)stream, img, H, W, table, out);
  return (int)hipGetLastError();
}
