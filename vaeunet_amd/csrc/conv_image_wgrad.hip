// Weight gradient of the 3-channel image convolution (inc.0, the first conv of
// DoubleConv(n_channels, 64): unet_parts.py:40 via unet_model.py:21), bf16,
// with the BatchNorm(+ReLU) backward apply of its output gradient formed in
// the operand path:
//
//   slab[s][co][tap*8 + ci] = sum_{pixels p of block s} dy[p][co] * img[p + tap][ci]
//   dy[p][co] = bf16(bn_bwd_elem(y[p][co], da[p][co], ...))   -- vu_bn_bwd_apply's bytes
//
// The image needs no gradient, so this weight gradient is dy's only reader:
// forming dy here saves its 268 MB store and re-read at 8 x 512^2.  K = 72 is
// a memory stream with a little MFMA work attached (as conv_image.hip in the
// forward), so unlike the LDS-DMA weight-gradient kernels the pixel operand
// passes through registers, 8 channels of one pixel per lane -- the layout the
// BN apply works in:
//
//   * persistent grid, 4 waves per block; a wave owns 32-pixel tiles (one
//     16x16x32 k-step) of the linear pixel range, the next tile's y, da and
//     image taps in flight behind the current tile's work (one tile ahead in
//     registers is what fits beside 80 accumulator and 48 coefficient
//     registers at two waves per SIMD);
//   * per tile the wave writes dy [32][64] and the patch rows [32][9 taps x 8
//     (+ 8 zero columns)] to a wave-private LDS image and reads both back with
//     the transposed ds_read_b64_tr_b16 (pixels are the reduction dimension);
//     taps outside the image, and pixels past the end, are zero;
//   * 4 x 5 accumulator fragments (64 x 80) stay in registers over all of the
//     wave's tiles; the block's waves are then summed through LDS in a fixed
//     order and the block writes one fp32 slab [64][72] (vu_slab_reduce sums the
//     slabs in a fixed order: deterministic).
//
// BN = false: the same body with dy given (no transform).
#include "host.h"
#include "wave.h"
#include "bn_bwd_elem.h"

namespace {

constexpr int NT = 256, NW = NT / 64;
constexpr int TP = 32;            // pixels per wave tile
constexpr int CO = 64;            // output channels (dy columns)
constexpr int NJ = 72, NJP = 80;  // patch columns, padded to whole 16-column fragments
constexpr int DYS = CO * 2 + 16;  // dy row pitch, bytes
constexpr int PTS = NJP * 2;      // patch row pitch, bytes
constexpr int WAVE_LDS = TP * (DYS + PTS);
constexpr int NA = CO / 16, NB = NJP / 16;
constexpr int RED = NA * NB * 4 * 64;  // floats of one wave's accumulators
constexpr int SMEM = (NW - 1) * RED * 4 > NW * WAVE_LDS ? (NW - 1) * RED * 4 : NW * WAVE_LDS;

struct WgArgs {
  const bf16_t* da;   // output gradient of the BN (BN) or dy itself (!BN)
  int64_t das;
  const bf16_t* y;    // the BN input
  int64_t ys;
  const float *scale, *shift, *mean, *k;
  int relu;
  const bf16_t* img;  // packed image, 8 channels
  int64_t imgs;
  int N, H, W;
  float* slab;
};

struct Tile {
  u32x4 d[4], y[4];
};

VU_DEV u32x4 tr_frag(const char* lo, const char* hi) {
  const s16x4 l = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)lo);
  const s16x4 h = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)hi);
  const u32x2 l2 = __builtin_bit_cast(u32x2, l), h2 = __builtin_bit_cast(u32x2, h);
  return u32x4{l2[0], l2[1], h2[0], h2[1]};
}

template <bool BN>
__global__ __launch_bounds__(NT, 2) void conv_image_wgrad_kernel(WgArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[SMEM];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  char* dyb = smem + wid * WAVE_LDS;
  char* ptb = dyb + TP * DYS;
  const int H = a.H, W = a.W, HW = a.H * a.W;
  const int P = a.N * HW;
  const int ntiles = (P + TP - 1) / TP;
  // y / da: lane = (pixel r8 of each group of 8, channels 8*c8 .. 8*c8 + 7)
  const int c8 = lane & 7, r8 = lane >> 3;
  const int c = c8 * 8;
  // image taps: lane = (pixel tp, taps 5*th .. 5*th + 4; tap 9 = the zero pad columns)
  const int tp = lane & 31, th = lane >> 5;
  const FastDiv div_hw((uint32_t)HW), div_w((uint32_t)W);

  float sc[8], sf[8], mu[8], k1[8], k2[8], k3[8];
  if constexpr (BN) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sc[e] = a.scale[c + e]; sf[e] = a.shift[c + e]; mu[e] = a.mean[c + e];
      k1[e] = a.k[c + e]; k2[e] = a.k[CO + c + e]; k3[e] = a.k[2 * CO + c + e];
    }
  }

  auto load_tile = [&](int t, Tile& q) {
    const int p0 = t * TP;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = min(p0 + i * 8 + r8, P - 1);  // (rows past the end are zeroed in process)
      q.d[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.da + (int64_t)p * a.das + c));
      if constexpr (BN)
        q.y[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.y + (int64_t)p * a.ys + c));
    }
  };
  auto load_taps = [&](int t, u32x4* tv) {
    const int p0 = t * TP;
    const bool ok = p0 + tp < P;
    const int p = ok ? p0 + tp : P - 1;
    const int n = (int)div_hw.div((uint32_t)p);
    const int rem = p - n * HW;
    const int h = (int)div_w.div((uint32_t)rem), w = rem - h * W;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int tap = th * 5 + j;
      const int ty = tap / 3;
      const int yy = h + ty - 1, xx = w + (tap - ty * 3) - 1;
      tv[j] = u32x4{0, 0, 0, 0};
      if (ok && tap < 9 && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
        tv[j] = *reinterpret_cast<const u32x4*>(a.img + ((int64_t)(n * H + yy) * W + xx) * a.imgs);
    }
  };

  f32x4 acc[NA][NB];
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

  const int g4 = lane >> 4, li = lane & 15, qd = li >> 2, pp = li & 3;
  // transposed-read addresses: lane 4*qd + pp of a 16-lane group names row qd,
  // columns 4*pp .. 4*pp + 3 of the group's 4 x 16 block (rows 8*g4 .. + 3, then + 4)
  const char* rdA = dyb + (8 * g4 + qd) * DYS + 8 * pp;
  const char* rdB = ptb + (8 * g4 + qd) * PTS + 8 * pp;

  auto store_taps = [&](const u32x4* tv) {
#pragma unroll
    for (int j = 0; j < 5; ++j) *reinterpret_cast<u32x4*>(ptb + tp * PTS + (th * 5 + j) * 16) = tv[j];
  };

  // One tile: dy of the loaded (y, da) into the LDS image, both operands'
  // fragments read back, then the NEXT tile's taps (tn, loaded one tile ahead)
  // stored over the patch rows -- behind the reads in program order, and the
  // LDS serves one wave's operations in order -- and the MFMAs.
  auto process = [&](int t, const Tile& q, const u32x4* tn, bool more) {
    const int p0 = t * TP;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      Vec8<bf16_t> vo;
      if constexpr (BN) {
        Vec8<bf16_t> vx, vd;
        vx.v = q.y[i];
        vd.v = q.d[i];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          vo.set(e, bn_bwd_elem(vx.get(e), vd.get(e), a.relu, sc[e], sf[e], mu[e], k1[e], k2[e], k3[e]));
      } else {
        vo.v = q.d[i];
      }
      if (p0 + i * 8 + r8 >= P) vo.zero();
      *reinterpret_cast<u32x4*>(dyb + (i * 8 + r8) * DYS + c8 * 16) = vo.v;
    }
    // (the LDS serves one wave's operations in order: no wait between the
    // stores and the reads of the same wave; the compiler must keep the order)
    asm volatile("" ::: "memory");
    u32x4 af[NA], bf[NB];
#pragma unroll
    for (int i = 0; i < NA; ++i) af[i] = tr_frag(rdA + i * 32, rdA + 4 * DYS + i * 32);
#pragma unroll
    for (int j = 0; j < NB; ++j) bf[j] = tr_frag(rdB + j * 32, rdB + 4 * PTS + j * 32);
    asm volatile("" ::: "memory");
    if (more) store_taps(tn);
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[i]),
                                                            __builtin_bit_cast(bf16x8, bf[j]), acc[i][j], 0, 0, 0);
  };

  // wave-uniform trip count (the transposed reads need every lane active)
  const int tstep = gridDim.x * NW;
  int t = blockIdx.x * NW + wid;
  if (t < ntiles) {
    Tile cur;
    u32x4 tn[5];
    load_tile(t, cur);
    load_taps(t, tn);
    store_taps(tn);
    for (; t < ntiles; t += tstep) {
      Tile nxt;
      const bool more = t + tstep < ntiles;
      if (more) {
        load_tile(t + tstep, nxt);
        load_taps(t + tstep, tn);
      }
      process(t, cur, tn, more);
      if (more) cur = nxt;
    }
  }

  // ---- block sum in a fixed order: ((wave 0 + wave 1) + wave 2) + wave 3
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);
  if (wid > 0) {
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wid - 1) * RED + ((i * NB + j) * 4 + r) * 64 + lane] = acc[i][j][r];
  }
  __syncthreads();
  if (wid != 0) return;
#pragma unroll 1
  for (int w = 0; w < NW - 1; ++w)
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] += red[w * RED + ((i * NB + j) * 4 + r) * 64 + lane];
  // lane holds rows 16*i + 4*g4 + r, column 16*j + li of the 64 x 80 tile
  float* out = a.slab + (int64_t)blockIdx.x * CO * NJ;
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int col = 16 * j + li;
      if (col < NJ)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(16 * i + 4 * g4 + r) * NJ + col] = acc[i][j][r];
    }
}

}  // namespace

extern "C" int vu_conv_image_wgrad_bn_ok(int C, int Cp, int64_t das, int64_t ys, int64_t imgs, int N, int H, int W,
                                         int dtype) {
  if (dtype != VU_BF16 || C != CO || Cp != 8) return 0;
  if (das % 8 != 0 || ys % 8 != 0 || imgs % 8 != 0 || das < CO || ys < CO || imgs < 8) return 0;
  if (N < 1 || H < 1 || W < 1) return 0;
  if ((int64_t)N * H * W >= (int64_t)1 << 31) return 0;
  return 1;
}

// slab count the launch is sized for by default: two blocks per CU, at most
// one wave per tile
extern "C" int vu_conv_image_wgrad_bn_slabs(int N, int H, int W) {
  const int64_t tiles = ((int64_t)N * H * W + TP - 1) / TP;
  int64_t nblk = (tiles + NW - 1) / NW;
  const int64_t cap = 2 * (int64_t)cu_count();
  if (nblk > cap) nblk = cap;
  return nblk < 1 ? 1 : (int)nblk;
}

extern "C" int vu_conv_image_wgrad_bn(const void* da, int64_t das, const void* y, int64_t ys, const float* scale,
                                      const float* shift, const float* mean, const float* k, int relu,
                                      const void* img, int64_t imgs, int N, int H, int W, float* slab, int nslab,
                                      void* stream) {
  if (!vu_conv_image_wgrad_bn_ok(CO, 8, das, y ? ys : das, imgs, N, H, W, VU_BF16)) return (int)hipErrorInvalidValue;
  if (!da || !img || !slab || nslab < 1) return (int)hipErrorInvalidValue;
  if (y && (!scale || !shift || !mean || !k)) return (int)hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(da) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(img)) % 16 != 0)
    return (int)hipErrorInvalidValue;
  WgArgs a{(const bf16_t*)da, das, (const bf16_t*)y, ys, scale, shift, mean, k, relu, (const bf16_t*)img, imgs,
           N, H, W, slab};
  hipStream_t st = (hipStream_t)stream;
  if (y)
    hipLaunchKernelGGL(conv_image_wgrad_kernel<true>, dim3((unsigned)nslab), dim3(NT), 0, st, a);
  else
    hipLaunchKernelGGL(conv_image_wgrad_kernel<false>, dim3((unsigned)nslab), dim3(NT), 0, st, a);
  return (int)hipGetLastError();
}
