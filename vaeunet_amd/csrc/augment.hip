// Device-side training augmentation of a patch batch: one
// launch warps image AND mask with the same per-sample geometry (separable
// grid distortion, then an affine map) and applies the photometric chain
// (gamma, colour matrix, Gaussian noise, clip) to the image.
//
// Layout: image [B][H][W][3] fp32, mask [B][H][W][Cm] fp32 (NHWC, the
// channels_last tensors PatchCache holds); outputs of the same shape.
// Per sample: params[20] = a0..a5 (output -> source affine), g (gamma),
// M[9] (row-major colour matrix), o[3], sigma; knot tables gx[S+1], gy[S+1].
//
// One thread per output pixel (all image and mask channels).  A block is a
// 32 x 8 output tile of one sample: a wave covers two 32-pixel row segments,
// so its stores are two contiguous runs (384 B of image each) and a rotated
// source footprint stays a compact patch of L2 lines.  The sample's 20
// parameters are read through a block-uniform address (scalar loads); the
// knots are staged once per block in LDS, and since the distortion is
// separable its value for the tile's 32 columns and 8 rows is formed there
// once per block too.
//
// Every float source coordinate is clamped to +-2^20 before the integer
// conversion and every tap index is either folded into [0, size) (reflect101)
// or tested against it (constant): no parameter value can form an address
// outside the sample.  The noise of a pixel is a pure function of (seed,
// offset, sample, pixel): Philox4x32-10, counter = (pixel lo, pixel hi,
// sample, offset), key = seed; it does not depend on B or the tile shape.
#include "common.h"
#include "reflect.h"
#include "../../include/vaeunet.h"

namespace {

constexpr int AUG_TW = 32, AUG_TH = 8, AUG_MAX_STEPS = 32;
constexpr int AUG_NPARAM = 20;
constexpr float AUG_COORD_MAX = 1048576.f;   // 2^20

enum { AUG_BORDER_CONSTANT = 0, AUG_BORDER_REFLECT101 = 1 };

// tap index and validity under the launch's border mode
template <int BORDER>
VU_DEV int tap(int i, int size, bool& ok) {
  if (BORDER == AUG_BORDER_REFLECT101) {
    ok = true;
    return reflect101(i, size);
  }
  ok = (unsigned)i < (unsigned)size;
  return ok ? i : 0;
}

VU_DEV float clamp_coord(float s) { return fminf(fmaxf(s, -AUG_COORD_MAX), AUG_COORD_MAX); }   // NaN -> -2^20

VU_DEV void mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
  lo = a * b;
  hi = __umulhi(a, b);
}

// Philox4x32-10 (Salmon et al., SC'11)
VU_DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                          uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t h0, l0, h1, l1;
    mulhilo(0xD2511F53u, c0, h0, l0);
    mulhilo(0xCD9E8D57u, c2, h1, l1);
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Box-Muller on two 32-bit words: radius from (a + 1) 2^-32 in (0, 1], angle 2 pi b 2^-32
VU_DEV void box_muller(uint32_t a, uint32_t b, float& rad, float& ang) {
  const float u1 = ((float)a + 1.0f) * 2.3283064365386963e-10f;
  const float u2 = (float)b * 2.3283064365386963e-10f;
  rad = sqrtf(-2.0f * logf(u1));
  ang = 6.283185307179586f * u2;
}

template <int BORDER>
__global__ void __launch_bounds__(AUG_TW * AUG_TH)
augment_patch_kernel(const float* __restrict__ img, const float* __restrict__ msk, int H, int W, int Cm,
                     const float* __restrict__ params, const float* __restrict__ gx, const float* __restrict__ gy,
                     int S, uint32_t seed_lo, uint32_t seed_hi, uint32_t offset, float* __restrict__ oimg,
                     float* __restrict__ omsk) {
  // the sample's knots, then the distorted coordinate of each of the tile's 32 columns and 8 rows: the map is
  // separable, so 40 threads evaluate it once per block and the integer division leaves the per-pixel path
  __shared__ float kx[AUG_MAX_STEPS + 1], ky[AUG_MAX_STEPS + 1], su[AUG_TW], sv[AUG_TH];
  const int b = blockIdx.z;
  const int t = threadIdx.x;
  if (t <= S) {
    kx[t] = gx[(int64_t)b * (S + 1) + t];
    ky[t] = gy[(int64_t)b * (S + 1) + t];
  }
  __syncthreads();
  // cell c of S equal cells, r = j S - c (W - 1) in [0, W - 1], u = k[c] + r ((k[c+1] - k[c]) / (W - 1))
  // (S = 1, knots {0, W - 1}: the slope is 1 and u = j exactly)
  if (t < AUG_TW + AUG_TH) {
    const bool col = t < AUG_TW;
    const int size = col ? W : H, d = max(size - 1, 1);
    const int n = min(col ? blockIdx.x * AUG_TW + t : blockIdx.y * AUG_TH + (t - AUG_TW), size - 1);
    const float* k = col ? kx : ky;
    const int c = min(n * S / d, S - 1);
    const float g = k[c] + (float)(n * S - c * d) * ((k[c + 1] - k[c]) / (float)d);
    if (col) su[t] = g; else sv[t - AUG_TW] = g;
  }
  __syncthreads();

  const float* __restrict__ p = params + (int64_t)b * AUG_NPARAM;   // block-uniform: scalar loads
  const int lx = t & (AUG_TW - 1), ly = t / AUG_TW;
  const int j = blockIdx.x * AUG_TW + lx;
  const int i = blockIdx.y * AUG_TH + ly;
  if (i >= H || j >= W) return;
  const float u = su[lx], v = sv[ly];

  // affine, output -> source
  const float sx = clamp_coord(fmaf(p[0], u, fmaf(p[1], v, p[2])));
  const float sy = clamp_coord(fmaf(p[3], u, fmaf(p[4], v, p[5])));

  const int64_t plane = (int64_t)H * W;
  const int64_t opix = (int64_t)b * plane + (int64_t)i * W + j;

  // mask: nearest neighbour at floor(s + 0.5)
  {
    bool okx, oky;
    const int mx = tap<BORDER>((int)floorf(sx + 0.5f), W, okx);
    const int my = tap<BORDER>((int)floorf(sy + 0.5f), H, oky);
    const float* src = msk + ((int64_t)b * plane + (int64_t)my * W + mx) * Cm;
    float* dst = omsk + opix * Cm;
    const bool ok = okx && oky;
    for (int c = 0; c < Cm; ++c) {
      const float m = src[c];   // a rejected tap has index 0: a valid address
      dst[c] = ok ? m : 0.f;
    }
  }

  // image: bilinear, a + t (b - a) so that t = 0 returns a bitwise
  const float fx = floorf(sx), fy = floorf(sy);
  const float tx = sx - fx, ty = sy - fy;
  bool okx0, okx1, oky0, oky1;
  const int x0 = tap<BORDER>((int)fx, W, okx0), x1 = tap<BORDER>((int)fx + 1, W, okx1);
  const int y0 = tap<BORDER>((int)fy, H, oky0), y1 = tap<BORDER>((int)fy + 1, H, oky1);
  const float* base = img + (int64_t)b * plane * 3;
  const float* p00 = base + ((int64_t)y0 * W + x0) * 3;
  const float* p01 = base + ((int64_t)y0 * W + x1) * 3;
  const float* p10 = base + ((int64_t)y1 * W + x0) * 3;
  const float* p11 = base + ((int64_t)y1 * W + x1) * 3;
  const bool k00 = oky0 && okx0, k01 = oky0 && okx1, k10 = oky1 && okx0, k11 = oky1 && okx1;
  float px[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    // a rejected tap has index 0: the address is valid, so the loads are unconditional (and merge per tap)
    const float v00 = p00[c], v01 = p01[c], v10 = p10[c], v11 = p11[c];
    const float a = k00 ? v00 : 0.f, bb = k01 ? v01 : 0.f;
    const float cc = k10 ? v10 : 0.f, d = k11 ? v11 : 0.f;
    const float top = a + tx * (bb - a);
    const float bot = cc + tx * (d - cc);
    px[c] = top + ty * (bot - top);
  }

  // photometry: gamma, colour matrix, noise, clip
  const float g = p[6];
  if (g != 1.0f) {   // uniform per block
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = powf(fmaxf(px[c], 0.f), g);
  }
  float q[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    q[c] = fmaf(p[7 + 3 * c + 2], px[2], fmaf(p[7 + 3 * c + 1], px[1], fmaf(p[7 + 3 * c], px[0], p[16 + c])));
  const float sigma = p[19];
  if (sigma != 0.0f) {   // uniform per block
    const uint64_t pix = (uint64_t)i * (uint64_t)W + (uint64_t)j;
    uint32_t r[4];
    philox4x32_10((uint32_t)pix, (uint32_t)(pix >> 32), (uint32_t)b, offset, seed_lo, seed_hi, r);
    float r0, a0, r1, a1;
    box_muller(r[0], r[1], r0, a0);
    box_muller(r[2], r[3], r1, a1);
    q[0] = fmaf(sigma, r0 * cosf(a0), q[0]);
    q[1] = fmaf(sigma, r0 * sinf(a0), q[1]);
    q[2] = fmaf(sigma, r1 * cosf(a1), q[2]);
  }
  float* dst = oimg + opix * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[c] = fminf(fmaxf(q[c], 0.f), 1.f);   // NaN -> 0
}

}  // namespace

extern "C" int vu_augment_patch(const float* img, const float* msk, int B, int H, int W, int C, int Cm,
                                const float* params, const float* gx, const float* gy, int S, int border,
                                uint64_t seed, uint32_t offset, float* out_img, float* out_msk, void* stream) {
  if (C != 3 || Cm < 1 || S < 1 || S > AUG_MAX_STEPS) return (int)hipErrorInvalidValue;
  if (border != AUG_BORDER_CONSTANT && border != AUG_BORDER_REFLECT101) return (int)hipErrorInvalidValue;
  if (B < 0 || H < 0 || W < 0) return (int)hipErrorInvalidValue;
  if (B == 0 || H == 0 || W == 0) return 0;
  if (!img || !msk || !params || !gx || !gy || !out_img || !out_msk) return (int)hipErrorInvalidValue;
  // grid.z and grid.y limits; j S and i S stay far below 2^31
  if (B > 65535 || H > 32768 || W > 32768) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((W + AUG_TW - 1) / AUG_TW), (unsigned)((H + AUG_TH - 1) / AUG_TH), (unsigned)B);
  const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
  if (border == AUG_BORDER_CONSTANT)
    hipLaunchKernelGGL(augment_patch_kernel<AUG_BORDER_CONSTANT>, grid, dim3(AUG_TW * AUG_TH), 0,
                       (hipStream_t)stream, img, msk, H, W, Cm, params, gx, gy, S, lo, hi, offset, out_img, out_msk);
  else
    hipLaunchKernelGGL(augment_patch_kernel<AUG_BORDER_REFLECT101>, grid, dim3(AUG_TW * AUG_TH), 0,
                       (hipStream_t)stream, img, msk, H, W, Cm, params, gx, gy, S, lo, hi, offset, out_img, out_msk);
  return (int)hipGetLastError();
}
