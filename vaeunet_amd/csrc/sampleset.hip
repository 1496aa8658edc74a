// Sample-set metrics: the pairwise overlap counts between S
// thresholded samples and M ground truths of every plane, and the generalised
// energy distance, sample diversity, Dice spread and area variability that are
// functions of those counts.  Definitions: include/vaeunet.h; the per-pair
// formulas, the summation order and the pair index: sampleset_core.h.
//
//   vu_sample_gram        one streaming launch (after a zeroing memset unless
//                         accumulate = 1).  A block step covers SG_WAVES wave
//                         steps; a wave step covers 64 VEC pixels of one plane, VEC
//                         consecutive pixels per lane.  For each of the K columns
//                         the lane loads its VEC elements once (16-byte
//                         non-temporal loads for fp32 at VEC = 4), and each of the
//                         VEC comparisons becomes a 64-bit lane mask by a ballot;
//                         lane k keeps column k's masks and stores them to LDS.
//                         The K (K + 1) / 2 pairs i <= j are dealt over the threads
//                         of the block: a thread adds popcount(m_i & m_j) over
//                         the SG_WAVES VEC masks of the step into its own entries
//                         of the block's uint32 table in LDS (no LDS atomics).
//                         After its last step of a plane the block adds every
//                         non-zero count into gram, both triangles, with one
//                         64-bit integer atomic each.
//                         Nothing else is written: no thresholded copy exists.
//   vu_sampleset_metrics  one launch, a block per plane: the K K distances and
//                         the S M Dice terms in parallel into LDS, then four
//                         threads form the four sums in sampleset_core.h's order.
//
// VEC = 4 needs every row 16-byte (fp32) or 4-byte (uint8) aligned: H W a
// multiple of 4 and aligned base pointers; every other input takes VEC = 1.
// Counts are integers and integer addition commutes: the result depends neither
// on the grid nor on the order of the atomics.  A block's LDS count of a pair is
// at most the pixels the block has seen of ONE plane, <= H W <= 2^31 - 2 < 2^32:
// it is flushed, and cleared, before the block moves to another plane.
#include "common.h"
#include "sampleset_core.h"
#include "../../include/vaeunet.h"

namespace {

constexpr int SG_WAVES = 4, SG_BLK = 64 * SG_WAVES;
constexpr int SG_UNROLL = 4;                 // columns whose loads are issued before the first ballot
constexpr int SG_MIN_STEPS = VU_SAMPLESET_MIN_STEPS;   // steps of a plane per block before the plane gets another block
constexpr unsigned SG_PLANES = 65535;        // grid.y; further planes are looped over
constexpr int SG_MAXPAIRS = SS_MAX * (SS_MAX + 1) / 2;
constexpr int SM_BLK = 256;

static_assert(SS_MAX == VU_SAMPLESET_MAX && SS_NMETRICS == VU_SAMPLESET_NMETRICS, "sampleset_core.h and vaeunet.h agree");
static_assert(VU_SAMPLESET_VEC * SG_BLK == VU_SAMPLESET_STEP, "pixels of one block step at VEC = 4");
static_assert(SS_MAX <= 64, "one lane per column, one bit per lane");

// VEC consecutive pixels of one column
template <typename T, int VEC> struct Pix;
template <> struct Pix<float, 4> {
  f32x4 v;
  VU_DEV void load(const float* p) { v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }
  VU_DEV void zero() { v = f32x4{0.f, 0.f, 0.f, 0.f}; }
  VU_DEV bool fg(int j, float thr) const { return v[j] > thr; }     // NaN: background
};
template <> struct Pix<float, 1> {
  float v;
  VU_DEV void load(const float* p) { v = __builtin_nontemporal_load(p); }
  VU_DEV void zero() { v = 0.f; }
  VU_DEV bool fg(int, float thr) const { return v > thr; }
};
template <> struct Pix<uint8_t, 4> {
  uint32_t v;
  VU_DEV void load(const uint8_t* p) { v = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p)); }
  VU_DEV void zero() { v = 0u; }
  VU_DEV bool fg(int j, float) const { return ((v >> (8 * j)) & 0xffu) != 0u; }
};
template <> struct Pix<uint8_t, 1> {
  uint8_t v;
  VU_DEV void load(const uint8_t* p) { v = __builtin_nontemporal_load(p); }
  VU_DEV void zero() { v = 0; }
  VU_DEV bool fg(int, float) const { return v != 0; }
};

// The ncols columns of one tensor [ncols][planes][HW] at element offset off (plane HW + e) of each: lane kbase + k
// keeps the VEC lane masks of column k.  Every lane of the wave calls it (ballots); a lane with in = false loads
// nothing and contributes zero bits.
template <typename T, int VEC>
VU_DEV void gather(const T* __restrict__ x, int ncols, int64_t colstride, int64_t off, bool in, float thr, int kbase, int lane,
                   uint64_t (&mine)[VEC]) {
  for (int k0 = 0; k0 < ncols; k0 += SG_UNROLL) {
    Pix<T, VEC> v[SG_UNROLL];
#pragma unroll
    for (int u = 0; u < SG_UNROLL; ++u) {
      const int k = min(k0 + u, ncols - 1);       // past the last column: the last one again, not used
      if (in) v[u].load(x + (int64_t)k * colstride + off);
      else v[u].zero();
    }
#pragma unroll
    for (int u = 0; u < SG_UNROLL; ++u) {
      if (k0 + u < ncols) {                        // wave-uniform
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const uint64_t b = __ballot(in && v[u].fg(j, thr));
          if (lane == kbase + k0 + u) mine[j] = b;
        }
      }
    }
  }
}

template <typename TS, typename TT, int VEC>
__global__ void __launch_bounds__(SG_BLK)
sample_gram_kernel(const TS* __restrict__ samples, const TT* __restrict__ truths, float thr, int S, int M, int64_t planes,
                   int64_t HW, unsigned long long* __restrict__ gram) {
  __shared__ uint64_t msk[SG_WAVES][VEC][SS_MAX];    // [wave][pixel of the lane][column]: a lane mask
  __shared__ uint32_t acc[SG_MAXPAIRS];              // the block's counts of the current plane, by pair index
  __shared__ uint16_t tab[SG_MAXPAIRS];              // pair index -> i | j << 8
  const int K = S + M, np = ss_npairs(K);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int p = threadIdx.x; p < np; p += SG_BLK) {
    int i, j;
    ss_pair_ij(p, K, &i, &j);
    tab[p] = (uint16_t)(i | (j << 8));
    acc[p] = 0u;
  }
  __syncthreads();
  const int64_t step_px = (int64_t)SG_BLK * VEC;
  const int64_t nsteps = (HW + step_px - 1) / step_px;
  const int64_t colstride = planes * HW;
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    for (int64_t step = blockIdx.x; step < nsteps; step += gridDim.x) {      // block-uniform
      const int64_t e = step * step_px + (int64_t)(wave * 64 + lane) * VEC;
      const bool in = e < HW;                      // VEC = 4: H W is a multiple of 4, all four pixels or none
      const int64_t off = plane * HW + e;
      uint64_t mine[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) mine[j] = 0;
      gather<TS, VEC>(samples, S, colstride, off, in, thr, 0, lane, mine);
      if (M > 0) gather<TT, VEC>(truths, M, colstride, off, in, 0.5f, S, lane, mine);
      if (lane < K) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) msk[wave][j][lane] = mine[j];
      }
      __syncthreads();
      for (int p = threadIdx.x; p < np; p += SG_BLK) {       // acc[p] belongs to this thread alone: no atomic
        const uint32_t ij = tab[p];
        const int i = ij & 0xff, jj = ij >> 8;
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < SG_WAVES; ++w)
#pragma unroll
          for (int j = 0; j < VEC; ++j) c += (uint32_t)__popcll(msk[w][j][i] & msk[w][j][jj]);
        acc[p] += c;
      }
      __syncthreads();
    }
    unsigned long long* g = gram + plane * (int64_t)(K * K);
    for (int p = threadIdx.x; p < np; p += SG_BLK) {
      const uint32_t c = acc[p];
      if (c) {
        const uint32_t ij = tab[p];
        const int i = ij & 0xff, jj = ij >> 8;
        atomicAdd(g + i * K + jj, (unsigned long long)c);
        if (i != jj) atomicAdd(g + jj * K + i, (unsigned long long)c);
        acc[p] = 0u;
      }
    }
    __syncthreads();
  }
}

template <typename TS, typename TT, int VEC>
void launch_gram(const void* samples, const void* truths, float thr, int S, int M, int64_t planes, int64_t HW, int64_t* gram,
                 hipStream_t st) {
  const int64_t step_px = (int64_t)SG_BLK * VEC;
  const int64_t nsteps = (HW + step_px - 1) / step_px;
  const int64_t gy = planes < (int64_t)SG_PLANES ? planes : (int64_t)SG_PLANES;
  int64_t cap = VU_SAMPLESET_GRID / gy;
  cap = cap < 1 ? 1 : cap;
  int64_t gx = (nsteps + SG_MIN_STEPS - 1) / SG_MIN_STEPS;
  gx = gx > cap ? cap : gx;
  hipLaunchKernelGGL((sample_gram_kernel<TS, TT, VEC>), dim3((unsigned)gx, (unsigned)gy), dim3(SG_BLK), 0, st,
                     static_cast<const TS*>(samples), static_cast<const TT*>(truths), thr, S, M, planes, HW,
                     reinterpret_cast<unsigned long long*>(gram));
}

template <typename TS, typename TT>
void launch_gram_vec(bool vec, const void* samples, const void* truths, float thr, int S, int M, int64_t planes, int64_t HW,
                     int64_t* gram, hipStream_t st) {
  if (vec) launch_gram<TS, TT, VU_SAMPLESET_VEC>(samples, truths, thr, S, M, planes, HW, gram, st);
  else launch_gram<TS, TT, 1>(samples, truths, thr, S, M, planes, HW, gram, st);
}

bool aligned(const void* p, int dtype) { return ((uintptr_t)p % (dtype == VU_CCL_F32 ? 16 : 4)) == 0; }

// ---- metrics ---------------------------------------------------------------------
__global__ void __launch_bounds__(SM_BLK)
sampleset_metrics_kernel(const int64_t* __restrict__ gram, int S, int M, int64_t planes, double* __restrict__ out) {
  __shared__ double dist[SS_MAX * SS_MAX];           // [a][b], leading dimension K
  __shared__ double dice[SS_MAX * SS_MAX / 4];       // [i][m], leading dimension M; S M <= 32 32
  __shared__ double part[8];                         // sum cross, div, tdiv, dice; dice min, max; area mean, sd
  const int K = S + M;
  for (int64_t plane = blockIdx.x; plane < planes; plane += gridDim.x) {
    const int64_t* G = gram + plane * (int64_t)(K * K);
    for (int t = threadIdx.x; t < K * K; t += SM_BLK) {
      const int a = t / K, b = t - a * K;
      const int64_t I = G[t], na = G[a * K + a], nb = G[b * K + b];
      dist[t] = ss_dist(I, na, nb);
      if (a < S && b >= S) dice[a * M + (b - S)] = ss_dice(I, na, nb);
    }
    __syncthreads();
    // one thread of each wave: the four chains run side by side
    if (threadIdx.x == 0) part[1] = ss_sum_block(dist, K, 0, S, 0, S);
    if (threadIdx.x == 64) {
      part[0] = ss_sum_block(dist, K, 0, S, S, M);
      part[2] = ss_sum_block(dist, K, S, M, S, M);
    }
    if (threadIdx.x == 128) {
      part[3] = ss_sum_block(dice, M, 0, S, 0, M);
      part[4] = part[5] = 0.0;
      if (M > 0) ss_minmax_block(dice, M, 0, S, 0, M, &part[4], &part[5]);
    }
    if (threadIdx.x == 192) ss_area_stats(G, K, S, &part[6], &part[7]);
    __syncthreads();
    if (threadIdx.x == 0)
      ss_finish(S, M, part[0], part[1], part[2], part[3], part[4], part[5], part[6], part[7], out + plane * SS_NMETRICS);
    __syncthreads();
  }
}

bool bad_dtype(int d) { return d != VU_CCL_U8 && d != VU_CCL_F32; }

}  // namespace

extern "C" int vu_sample_gram(const void* samples, int dtype, float threshold, const void* truths, int truth_dtype, int S, int M,
                              int64_t planes, int H, int W, int64_t* gram, int accumulate, void* stream) {
  const int64_t HW = (int64_t)H * W;
  if (planes < 0 || H < 0 || W < 0 || S < 1 || M < 0 || (int64_t)S + M > VU_SAMPLESET_MAX || bad_dtype(dtype) ||
      (M > 0 && bad_dtype(truth_dtype)) || HW > VU_CCL_MAX_PLANE || (accumulate != 0 && accumulate != 1))
    return (int)hipErrorInvalidValue;
  if (planes == 0 || HW == 0) return 0;
  if (!samples || !gram || (M > 0 && !truths)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int K = S + M;
  if (!accumulate) {
    hipError_t rc = hipMemsetAsync(gram, 0, (size_t)planes * K * K * sizeof(int64_t), st);
    if (rc != hipSuccess) return (int)rc;
  }
  const int tdt = M > 0 ? truth_dtype : VU_CCL_U8;
  const bool vec = HW % VU_SAMPLESET_VEC == 0 && aligned(samples, dtype) && (M == 0 || aligned(truths, tdt));
  if (dtype == VU_CCL_F32) {
    if (tdt == VU_CCL_F32) launch_gram_vec<float, float>(vec, samples, truths, threshold, S, M, planes, HW, gram, st);
    else launch_gram_vec<float, uint8_t>(vec, samples, truths, threshold, S, M, planes, HW, gram, st);
  } else {
    if (tdt == VU_CCL_F32) launch_gram_vec<uint8_t, float>(vec, samples, truths, threshold, S, M, planes, HW, gram, st);
    else launch_gram_vec<uint8_t, uint8_t>(vec, samples, truths, threshold, S, M, planes, HW, gram, st);
  }
  return (int)hipGetLastError();
}

extern "C" int vu_sampleset_metrics(const int64_t* gram, int S, int M, int64_t planes, double* out, void* stream) {
  if (planes < 0 || S < 1 || M < 0 || (int64_t)S + M > VU_SAMPLESET_MAX) return (int)hipErrorInvalidValue;
  if (planes == 0) return 0;
  if (!gram || !out) return (int)hipErrorInvalidValue;
  const unsigned grid = (unsigned)(planes < 4096 ? planes : 4096);
  hipLaunchKernelGGL(sampleset_metrics_kernel, dim3(grid), dim3(SM_BLK), 0, (hipStream_t)stream, gram, S, M, planes, out);
  return (int)hipGetLastError();
}
