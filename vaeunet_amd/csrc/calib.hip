// Calibration and uncertainty metrics (the numbers of the reference's
// utils/uncertainty_metrics.py: ECE / MCE, Brier, NLL, AUROC / AUPRC,
// sparsification) from ONE streaming pass over a probability map, its mask and
// an optional uncertainty map.  Definitions: include/vaeunet.h (unpinned vs
// the reference).
//
//   vu_calib_hist     stage 1: per-block LDS histograms (32-bit counters, one
//                     increment per pixel and histogram at bin * 2 + column)
//                     flushed with 64-bit global atomics (integers: the result
//                     does not depend on the grid or the order); the fp64
//                     quantities never meet an atomic: Brier / NLL are per-lane
//                     registers, the per-bin confidence sums live in one LDS
//                     column per lane, both are folded in a fixed order into
//                     per-block partials.  stage 2: one wave per quantity sums
//                     the partials in a fixed order.
//   vu_calib_metrics  the totals -> every metric, fp64, one 1024-thread block
//                     (one rank / uncertainty bin per thread, integer suffix
//                     scans in LDS).
//
// Skew: a lesion probability map puts > 99 % of the pixels of a wave on one
// histogram word.  Before the LDS atomic the wave peels the index of its first
// pending lane VU_CALIB_PEEL times (readfirstlane + ballot; one lane adds the
// popcount); the remaining lanes use plain LDS atomics.  One peel is what
// tools/calib_bench.py measured fastest on a skewed map (DESIGN.md 4.6;
// -DVU_CALIB_PEEL=0 / 2 build the other forms of that A/B).
#include "common.h"
#include "lds_hist.h"
#include "../../include/vaeunet.h"

#ifndef VU_CALIB_PEEL
#define VU_CALIB_PEEL 1
#endif

namespace {

constexpr int CBLK = 256;
constexpr int CNB = 768;  // max stage-1 blocks (3 per CU at nb <= 16)
constexpr int R = VU_CALIB_RANK_BINS;
constexpr int NBMAX = 64;
constexpr int WSROW = NBMAX + 2;  // per-block fp64 partials: conf_sum[NBMAX], brier, nll

enum { M_F32 = 0, M_U8 = 1, M_I64 = 2 };

typedef unsigned long long u64;

struct CalibArgs {
  const float* p;
  const void* m;
  const float* u;
  int64_t n, head, n4;  // elements; scalar head; 4-element vectors of the aligned body
  int nb;
  float uscale;
  u64 *conf_hist, *rank_hist, *unc_hist, *invalid;
  double* ws;
};

template <typename T> VU_DEV bool truth1(const T* p) { return (float)(*p) > 0.5f; }

VU_DEV void truth4(const float* p, bool (&t)[4]) {
  const f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
#pragma unroll
  for (int j = 0; j < 4; ++j) t[j] = q[j] > 0.5f;
}
VU_DEV void truth4(const uint8_t* p, bool (&t)[4]) {
  const uint32_t q = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
#pragma unroll
  for (int j = 0; j < 4; ++j) t[j] = (float)((q >> (8 * j)) & 0xffu) > 0.5f;
}
VU_DEV void truth4(const int64_t* p, bool (&t)[4]) {
  const u32x4 q0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  const u32x4 q1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + 2));
  const int64_t e[4] = {(int64_t)(((uint64_t)q0[1] << 32) | q0[0]), (int64_t)(((uint64_t)q0[3] << 32) | q0[2]),
                        (int64_t)(((uint64_t)q1[1] << 32) | q1[0]), (int64_t)(((uint64_t)q1[3] << 32) | q1[2])};
#pragma unroll
  for (int j = 0; j < 4; ++j) t[j] = (float)e[j] > 0.5f;
}

// min((int)v, bins - 1) for v >= 0; the clamp ahead of the conversion keeps it
// defined for huge v and does not change the result for the others
VU_DEV int bin_of(float v, int bins) { return min((int)fminf(v, (float)bins), bins - 1); }

struct Acc {
  double brier, nll;
  uint32_t inv_p, inv_u;
};

template <bool HAS_U>
VU_DEV void pixel(bool valid, float p, bool t, float u, int nb, float uscale, uint32_t* hc, uint32_t* hr,
                  uint32_t* hu, double* col, Acc& a) {
  const bool ok = valid && !(p != p);
  a.inv_p += valid && !ok;
  const float pc = ok ? fminf(fmaxf(p, 0.f), 1.f) : 0.f;
  const int cb = bin_of(pc * (float)nb, nb);
  const int rb = bin_of(pc * (float)R, R);
  hist_add<VU_CALIB_PEEL>(hc, cb * 2 + (int)t, ok);
  hist_add<VU_CALIB_PEEL>(hr, rb * 2 + (int)t, ok);
  if (HAS_U) {
    const bool uok = ok && !(u != u);
    a.inv_u += ok && !uok;
    const int ub = bin_of(fmaxf(uok ? u : 0.f, 0.f) * uscale, R);
    hist_add<VU_CALIB_PEEL>(hu, ub * 2 + (int)((pc > 0.5f) != t), uok);
  }
  if (ok) {
    const double q = (double)pc, d = q - (t ? 1.0 : 0.0);
    a.brier += d * d;
    const double qc = fmin(fmax(q, 1e-7), 1.0 - 1e-7);
    a.nll -= log(t ? qc : 1.0 - qc);
    col[cb * CBLK] += q;
  }
}

// NBC: confidence-bin columns of the per-lane fp64 table (nb <= NBC)
template <typename MT, bool HAS_U, int NBC>
__global__ void __launch_bounds__(CBLK) calib_hist_kernel(CalibArgs A) {
  __shared__ uint32_t hc[NBMAX * 2], hr[R * 2], hu[HAS_U ? R * 2 : 2], hinv[2];
  __shared__ double cs[NBC * CBLK];
  __shared__ double red[2][CBLK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < NBMAX * 2; i += CBLK) hc[i] = 0;
  for (int i = tid; i < R * 2; i += CBLK) hr[i] = 0;
  if (HAS_U)
    for (int i = tid; i < R * 2; i += CBLK) hu[i] = 0;
  if (tid < 2) hinv[tid] = 0;
  for (int b = 0; b < A.nb; ++b) cs[b * CBLK + tid] = 0.0;
  __syncthreads();

  const MT* m = static_cast<const MT*>(A.m);
  double* col = cs + tid;
  Acc a = {0.0, 0.0, 0u, 0u};
  const int64_t step = (int64_t)gridDim.x * CBLK;
  // aligned body: 4 pixels per lane and step, whole waves iterate together
  for (int64_t base = (int64_t)blockIdx.x * CBLK; base < A.n4; base += step) {
    const int64_t i = base + tid;
    const bool valid = i < A.n4;
    const int64_t e = A.head + 4 * (valid ? i : 0);
    f32x4 pv = {0.f, 0.f, 0.f, 0.f}, uv = {0.f, 0.f, 0.f, 0.f};
    bool t[4] = {false, false, false, false};
    if (valid) {
      pv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(A.p + e));
      if (HAS_U) uv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(A.u + e));
      truth4(m + e, t);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) pixel<HAS_U>(valid, pv[j], t[j], uv[j], A.nb, A.uscale, hc, hr, hu, col, a);
  }
  // scalar head [0, head) and tail [head + 4 n4, n)
  const int64_t ns = A.n - 4 * A.n4;
  for (int64_t base = (int64_t)blockIdx.x * CBLK; base < ns; base += step) {
    const int64_t j = base + tid;
    const bool valid = j < ns;
    const int64_t e = !valid ? 0 : (j < A.head ? j : j + 4 * A.n4);
    float pv = 0.f, uv = 0.f;
    bool t = false;
    if (valid) {
      pv = A.p[e];
      if (HAS_U) uv = A.u[e];
      t = truth1<MT>(m + e);
    }
    pixel<HAS_U>(valid, pv, t, uv, A.nb, A.uscale, hc, hr, hu, col, a);
  }
  if (a.inv_p) atomicAdd(&hinv[0], a.inv_p);
  if (a.inv_u) atomicAdd(&hinv[1], a.inv_u);
  __syncthreads();

  // integers: 64-bit global atomics on the non-zero words
  for (int i = tid; i < A.nb * 2; i += CBLK)
    if (hc[i]) atomicAdd(&A.conf_hist[i], (u64)hc[i]);
  for (int i = tid; i < R * 2; i += CBLK)
    if (hr[i]) atomicAdd(&A.rank_hist[i], (u64)hr[i]);
  if (HAS_U)
    for (int i = tid; i < R * 2; i += CBLK)
      if (hu[i]) atomicAdd(&A.unc_hist[i], (u64)hu[i]);
  if (tid < 2 && hinv[tid]) atomicAdd(&A.invalid[tid], (u64)hinv[tid]);

  // fp64: fixed-order fold of the lane columns, one wave per bin
  double* ws = A.ws + (int64_t)blockIdx.x * WSROW;
  for (int b = wv; b < A.nb; b += CBLK / 64) {
    const double* c = cs + b * CBLK + lane;
    const double s = warp_sum_d(((c[0] + c[64]) + c[128]) + c[192]);
    if (lane == 0) ws[b] = s;
  }
  const double sb = warp_sum_d(a.brier), sn = warp_sum_d(a.nll);
  if (lane == 0) { red[0][wv] = sb; red[1][wv] = sn; }
  __syncthreads();
  if (tid < 2) ws[NBMAX + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

__global__ void calib_zero(u64* conf_hist, int nb, u64* rank_hist, u64* unc_hist, u64* invalid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb * 2) conf_hist[i] = 0;
  if (i < R * 2) {
    rank_hist[i] = 0;
    if (unc_hist) unc_hist[i] = 0;
  }
  if (i < 2) invalid[i] = 0;
}

// one wave per quantity (nb confidence sums, Brier, NLL): the partials of the
// nblk stage-1 blocks in a fixed order
__global__ void calib_stage2(const double* ws, int nblk, int nb, double* conf_sum, double* sums, int accumulate) {
  const int q = blockIdx.x;
  const double* p = ws + (q < nb ? q : NBMAX + (q - nb));
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) s += p[(int64_t)i * WSROW];
  s = warp_sum_d(s);
  if (threadIdx.x != 0) return;
  double* o = q < nb ? conf_sum + q : sums + (q - nb);
  *o = accumulate ? *o + s : s;
}

// ---- finalize -------------------------------------------------------------
constexpr int FBLK = R;  // one rank / uncertainty bin per thread

VU_DEV double block_sum_d(double v, double* sh) {
  v = warp_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < FBLK / 64; ++i) s += sh[i];
  return s;
}

__global__ void __launch_bounds__(FBLK) calib_metrics_kernel(const long long* conf_hist, const double* conf_sum,
                                                             int nb, const long long* rank_hist,
                                                             const long long* unc_hist, const double* sums,
                                                             double* scalars, double* rel, double* spars) {
  // suffix sums over the bins >= k: rank negatives, rank positives, uncertainty counts, uncertainty errors
  __shared__ long long suf[4][R + 1];
  __shared__ double gap[R + 1], frac[R + 1];
  __shared__ double shred[FBLK / 64];
  __shared__ double rgap[NBMAX], rcnt[NBMAX];
  const int k = threadIdx.x;
  const double nan = __builtin_nan("");
  const long long neg = rank_hist[k * 2], pos = rank_hist[k * 2 + 1];
  const long long ucnt = unc_hist ? unc_hist[k * 2] + unc_hist[k * 2 + 1] : 0, uerr = unc_hist ? unc_hist[k * 2 + 1] : 0;
  suf[0][k] = neg; suf[1][k] = pos; suf[2][k] = ucnt; suf[3][k] = uerr;
  if (k < 4) suf[k][R] = 0;
  __syncthreads();
  for (int o = 1; o < R; o <<= 1) {
    long long t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] = k + o < R ? suf[q][k + o] : 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) suf[q][k] += t[q];
    __syncthreads();
  }
  const double Q = (double)suf[0][0], P = (double)suf[1][0];

  // ranking: bin k is one tie group
  const double dpos = (double)pos, dneg = (double)neg;
  const double below = (double)(suf[0][0] - suf[0][k]);  // negatives in bins < k
  const double num = block_sum_d(dpos * below + 0.5 * (dpos * dneg), shred);
  const double tie = block_sum_d(dpos * dneg, shred);
  const double cum_pos = (double)suf[1][k], cum_all = (double)(suf[1][k] + suf[0][k]);  // score >= bin k
  const double ap = block_sum_d(pos > 0 ? (dpos / P) * (cum_pos / cum_all) : 0.0, shred);

  // sparsification: row k removes the k highest-uncertainty bins
  const double Nu = (double)suf[2][0], E = (double)suf[3][0];
  for (int r = k; r <= R; r += FBLK) {
    const double C = (double)suf[2][R - r], Ec = (double)suf[3][R - r], den = Nu - C;
    const double f = C / Nu, err = den > 0.0 ? (E - Ec) / den : 0.0, orc = den > 0.0 ? fmax(E - C, 0.0) / den : 0.0;
    frac[r] = f;
    gap[r] = err - orc;
    spars[r * 3] = unc_hist ? f : nan;
    spars[r * 3 + 1] = unc_hist ? err : nan;
    spars[r * 3 + 2] = unc_hist ? orc : nan;
  }
  __syncthreads();
  const double ause = block_sum_d((frac[k + 1] - frac[k]) * (0.5 * (gap[k + 1] + gap[k])), shred);

  // reliability table
  if (k < nb) {
    const double c0 = (double)conf_hist[k * 2], c1 = (double)conf_hist[k * 2 + 1], cnt = c0 + c1;
    const double acc = cnt > 0.0 ? c1 / cnt : 0.0, conf = cnt > 0.0 ? conf_sum[k] / cnt : 0.0;
    rel[k * 3] = cnt; rel[k * 3 + 1] = acc; rel[k * 3 + 2] = conf;
    rcnt[k] = cnt;
    rgap[k] = fabs(acc - conf);
  }
  __syncthreads();
  if (k != 0) return;
  double N = 0.0;
  for (int b = 0; b < nb; ++b) N += rcnt[b];
  double ece = 0.0, mce = 0.0;
  for (int b = 0; b < nb; ++b)
    if (rcnt[b] > 0.0) {
      ece += rcnt[b] / N * rgap[b];
      mce = fmax(mce, rgap[b]);
    }
  const double PQ = P * Q;
  scalars[0] = N > 0.0 ? ece : nan;
  scalars[1] = N > 0.0 ? mce : nan;
  scalars[2] = sums[0] / N;
  scalars[3] = sums[1] / N;
  scalars[4] = PQ > 0.0 ? num / PQ : nan;
  scalars[5] = PQ > 0.0 ? tie / (2.0 * PQ) : nan;
  scalars[6] = P > 0.0 ? ap : nan;
  scalars[7] = unc_hist ? ause : nan;
  scalars[8] = N;
  scalars[9] = P;
  scalars[10] = unc_hist ? Nu : nan;
  scalars[11] = unc_hist ? E : nan;
}

template <typename MT, bool HAS_U>
void launch_nbc(int nb, int grid, hipStream_t st, const CalibArgs& A) {
  if (nb <= 16) hipLaunchKernelGGL((calib_hist_kernel<MT, HAS_U, 16>), dim3(grid), dim3(CBLK), 0, st, A);
  else hipLaunchKernelGGL((calib_hist_kernel<MT, HAS_U, NBMAX>), dim3(grid), dim3(CBLK), 0, st, A);
}

template <typename MT>
void launch_u(int nb, int grid, hipStream_t st, const CalibArgs& A) {
  if (A.u) launch_nbc<MT, true>(nb, grid, st, A);
  else launch_nbc<MT, false>(nb, grid, st, A);
}

}  // namespace

extern "C" int64_t vu_calib_workspace_bytes() { return (int64_t)CNB * WSROW * (int64_t)sizeof(double); }

extern "C" int vu_calib_hist(const float* p, const void* mask, int mdtype, const float* u, int64_t n, int nb,
                             float uscale, int64_t* conf_hist, double* conf_sum, int64_t* rank_hist,
                             int64_t* unc_hist, double* sums, int64_t* invalid, int accumulate, void* workspace,
                             void* stream) {
  if (n < 1 || n >= ((int64_t)1 << 31) || nb < 1 || nb > NBMAX || mdtype < M_F32 || mdtype > M_I64)
    return (int)hipErrorInvalidValue;
  if (!p || !mask || !conf_hist || !conf_sum || !rank_hist || !sums || !invalid || !workspace || (u == nullptr) != (unc_hist == nullptr))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  CalibArgs A;
  A.p = p; A.m = mask; A.u = u; A.n = n; A.nb = nb; A.uscale = uscale;
  A.conf_hist = reinterpret_cast<u64*>(conf_hist);
  A.rank_hist = reinterpret_cast<u64*>(rank_hist);
  A.unc_hist = reinterpret_cast<u64*>(unc_hist);
  A.invalid = reinterpret_cast<u64*>(invalid);
  A.ws = static_cast<double*>(workspace);
  // elements ahead of the first 16-B boundary of p; the vector body needs u and
  // the mask aligned at the same element, otherwise every element goes the
  // scalar way
  const int msize = mdtype == M_F32 ? 4 : (mdtype == M_U8 ? 1 : 8), malign = mdtype == M_U8 ? 4 : 16;
  int64_t head = (int64_t)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
  if (head > n) head = n;
  const bool vec = ((uintptr_t)p & 3) == 0 && (!u || (((uintptr_t)(u + head)) & 15) == 0) &&
                   (((uintptr_t)mask + (uintptr_t)(head * msize)) % malign) == 0;
  if (!vec) head = n;
  A.head = head;
  A.n4 = (n - head) >> 2;
  const int64_t work = A.n4 > 0 ? A.n4 : 1, ns = n - 4 * A.n4;
  int64_t grid = ((work > ns ? work : ns) + CBLK - 1) / CBLK;
  if (grid > CNB) grid = CNB;
  if (!accumulate)
    hipLaunchKernelGGL(calib_zero, dim3(R * 2 / 256), dim3(256), 0, st, A.conf_hist, nb, A.rank_hist, A.unc_hist,
                       A.invalid);
  if (mdtype == M_F32) launch_u<float>(nb, (int)grid, st, A);
  else if (mdtype == M_U8) launch_u<uint8_t>(nb, (int)grid, st, A);
  else launch_u<int64_t>(nb, (int)grid, st, A);
  hipLaunchKernelGGL(calib_stage2, dim3(nb + 2), dim3(64), 0, st, A.ws, (int)grid, nb, conf_sum, sums, accumulate);
  return (int)hipGetLastError();
}

extern "C" int vu_calib_metrics(const int64_t* conf_hist, const double* conf_sum, int nb, const int64_t* rank_hist,
                                const int64_t* unc_hist, const double* sums, double* scalars, double* reliability,
                                double* sparsification, void* stream) {
  if (nb < 1 || nb > NBMAX || !conf_hist || !conf_sum || !rank_hist || !sums || !scalars || !reliability ||
      !sparsification)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(calib_metrics_kernel, dim3(1), dim3(FBLK), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(conf_hist), conf_sum, nb,
                     reinterpret_cast<const long long*>(rank_hist), reinterpret_cast<const long long*>(unc_hist),
                     sums, scalars, reliability, sparsification);
  return (int)hipGetLastError();
}
