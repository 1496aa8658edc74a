// Fused focal + soft-Dice objective (MAFocalLoss / MASegmentationLoss,
// utils/loss.py:66-111; DESIGN.md §4.7, unpinned vs the reference).
//
//   sp(z)  = max(z, 0) + log1p(exp(-|z|))
//   b      = t * sp(-x) + (1 - t) * sp(x)             BCE-with-logits, a sum of non-negatives
//   q      = exp(-b),  omq = -expm1(-b)               1 - q without cancellation
//   a_t    = alpha * t + (1 - alpha) * (1 - t)
//   f      = a_t * omq^gamma * b
//   p      = sigmoid(x) (NaN -> 0),  I = sum p t,  Sp = sum p,  St = sum t
//   loss   = w_focal * (mean | sum)(f) + w_dice * (1 - (2 I + s) / (max(Sp, s/2) + max(St, s/2) + s))
//
// Stage 1 streams logits and targets once and leaves five fp64 partials per
// block; stage 2 (one block) adds them in a fixed order and forms the loss on
// the device.  The backward is one elementwise kernel that reads the sums and
// a device scalar.  No float atomics, no host synchronisation, results are
// bitwise repeatable (the grid is a function of n and the alignment only).
//
// Every exp / log1p of an element derives from e = exp(-|x|) in (0, 1]:
//   sp(x) = max(x, 0) + log1p(e),  sigmoid(|x|) = 1 / (1 + e),  sigmoid(-|x|) = e / (1 + e),
//   dp/dx = sigmoid(x) sigmoid(-x) = e / (1 + e)^2
// so nothing is formed as 1 - (something near 1).
#include "common.h"
#include "../../include/vaeunet.h"

namespace {

constexpr int FBLK = 256;
constexpr int FNB = 2048;  // stage-1 / backward block cap (256 CUs x 8 blocks): grid-stride above it
constexpr int FNQ = 5;     // sum f, sum p t, sum p, sum t, NaN logits

enum { GM_ZERO = 0, GM_ONE = 1, GM_TWO = 2, GM_GENERAL = 3 };

// a[k] <- the block's sum of a[k], in every thread: the FNQ quantities share one barrier
VU_DEV void block_sums(double (&a)[FNQ], double (*sh)[FBLK / 64]) {
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < FNQ; ++k) {
    a[k] = warp_sum_d(a[k]);
    if ((threadIdx.x & 63) == 0) sh[k][w] = a[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < FNQ; ++k) a[k] = sh[k][0] + sh[k][1] + sh[k][2] + sh[k][3];
}

// pw = omq^gamma and w = d(omq^gamma * b)/db = omq^gamma + gamma * omq^(gamma-1) * q * b.
// gm is uniform over the launch (a scalar branch).  The general case goes
// through fp64 exp2 / log2: the fp32 pair loses |gamma * log2 omq| (up to
// ~100) ulps on the easy pixels, which is all of a focal-only gradient there.
VU_DEV void focal_pow(int gm, float gamma, float omq, float q, float b, float& pw, float& w) {
  if (gm == GM_TWO) {
    pw = omq * omq;
    w = pw + 2.f * omq * (q * b);
  } else if (gm == GM_ONE) {
    pw = omq;
    w = omq + q * b;
  } else if (gm == GM_ZERO) {
    pw = 1.f;
    w = 1.f;
  } else {
    const float pw1 = omq > 0.f ? (float)exp2((double)(gamma - 1.f) * log2((double)omq)) : 0.f;
    pw = pw1 * omq;
    w = pw + gamma * pw1 * (q * b);
  }
}

struct FocalElem {
  float f, p, dp, wpt;  // focal term, sigmoid, sigmoid(x) sigmoid(-x), a_t * w * (p - t)
};

// A NaN logit: p = 0 for the Dice sums, no focal term, no gradient.
template <bool BWD>
VU_DEV FocalElem focal_elem(float x, float t, float alpha, float gamma, int gm) {
  FocalElem r;
  if (isnan(x)) {
    r.f = r.p = r.dp = r.wpt = 0.f;
    return r;
  }
  const float e = expf(-fabsf(x));
  const float l = log1pf(e);
  const float inv = 1.f / (1.f + e);
  const float hi = inv, lo = e * inv;  // sigmoid(|x|), sigmoid(-|x|)
  r.p = x >= 0.f ? hi : lo;
  r.dp = lo * hi;
  const float b = t * (fmaxf(-x, 0.f) + l) + (1.f - t) * (fmaxf(x, 0.f) + l);
  const float q = expf(-b), omq = -expm1f(-b);
  const float at = alpha * t + (1.f - alpha) * (1.f - t);
  float pw, w;
  focal_pow(gm, gamma, omq, q, b, pw, w);
  r.f = at * pw * b;
  r.wpt = BWD ? at * w * (r.p - t) : 0.f;
  return r;
}

// Elements [0, head) and [head + V * nvec, n) are scalar (thread k < head + ntail
// of block 0 takes one); the body is nvec vectors of V floats: V = 4 at 16-byte
// aligned addresses, or V = 1 (no head, no tail) when there is no common alignment.
struct Split {
  int head;
  int64_t nvec;
  int ntail;
};

template <int V> struct FVec;
template <> struct FVec<4> { typedef f32x4 T; };
template <> struct FVec<1> { typedef float T; };
VU_DEV float lane(const f32x4& v, int k) { return v[k]; }
VU_DEV float lane(float v, int) { return v; }
VU_DEV void set_lane(f32x4& v, int k, float f) { v[k] = f; }
VU_DEV void set_lane(float& v, int, float f) { v = f; }

template <int V>
VU_DEV int64_t edge_index(const Split& s, int k) { return k < s.head ? k : s.head + V * s.nvec + (k - s.head); }

template <int V>
__global__ __launch_bounds__(FBLK) void focal_stage1(const float* __restrict__ x, const float* __restrict__ t,
                                                      Split s, float alpha, float gamma, int gm, double* ws) {
  __shared__ double sh[FNQ][FBLK / 64];
  double a[FNQ] = {0, 0, 0, 0, 0};
  auto acc = [&](float xv, float tv) {
    const FocalElem r = focal_elem<false>(xv, tv, alpha, gamma, gm);
    a[0] += r.f;
    a[1] += (double)r.p * tv;
    a[2] += r.p;
    a[3] += tv;
    a[4] += isnan(xv) ? 1.0 : 0.0;
  };
  if (blockIdx.x == 0 && (int)threadIdx.x < s.head + s.ntail) {
    const int64_t i = edge_index<V>(s, threadIdx.x);
    acc(x[i], t[i]);
  }
  typedef typename FVec<V>::T vec_t;
  const vec_t* xv = reinterpret_cast<const vec_t*>(x + s.head);
  const vec_t* tv = reinterpret_cast<const vec_t*>(t + s.head);
  for (int64_t i = (int64_t)blockIdx.x * FBLK + threadIdx.x; i < s.nvec; i += (int64_t)gridDim.x * FBLK) {
    const vec_t xx = __builtin_nontemporal_load(xv + i), tt = __builtin_nontemporal_load(tv + i);
#pragma unroll
    for (int k = 0; k < V; ++k) acc(lane(xx, k), lane(tt, k));
  }
  block_sums(a, sh);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < FNQ; ++k) ws[(int64_t)k * FNB + blockIdx.x] = a[k];
}

struct DiceTerms {
  double U, num, mp, dl;
};

VU_DEV DiceTerms dice_terms(const double* sums, float smooth) {
  DiceTerms d;
  const double half = 0.5 * (double)smooth;
  d.U = fmax(sums[2], half) + fmax(sums[3], half) + (double)smooth;
  d.num = 2.0 * sums[1] + (double)smooth;
  d.mp = sums[2] >= half ? 1.0 : 0.0;
  d.dl = 1.0 - d.num / d.U;
  return d;
}

__global__ __launch_bounds__(FBLK) void focal_stage2(const double* ws, int nblk, int64_t n, float smooth,
                                                      float w_focal, float w_dice, int sum_reduction, double* sums,
                                                      float* loss, float* parts) {
  __shared__ double sh[FNQ][FBLK / 64];
  double s[FNQ] = {0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < nblk; b += FBLK)
#pragma unroll
    for (int k = 0; k < FNQ; ++k) s[k] += ws[(int64_t)k * FNB + b];
  block_sums(s, sh);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < FNQ; ++k) sums[k] = s[k];
  const float focal = (float)(sum_reduction ? s[0] : s[0] / (double)n);
  const float dl = (float)dice_terms(s, smooth).dl;
  if (loss) loss[0] = w_focal * focal + w_dice * dl;
  if (parts) { parts[0] = focal; parts[1] = dl; }
}

template <int V>
__global__ __launch_bounds__(FBLK) void focal_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                          Split s, int64_t n, float alpha, float gamma, int gm,
                                                          float smooth, float w_focal, float w_dice,
                                                          int sum_reduction, const double* sums, const float* gscale,
                                                          float* __restrict__ grad) {
  const double g = gscale ? (double)gscale[0] : 1.0;
  const DiceTerms d = dice_terms(sums, smooth);
  // grad = kf * a_t w (p - t) - dp * (t * c1 - c0):  the launch-uniform factors in fp64, rounded once
  const float kf = (float)(g * (double)w_focal / (sum_reduction ? 1.0 : (double)n));
  const float c1 = (float)(g * (double)w_dice * 2.0 / d.U);
  const float c0 = (float)(g * (double)w_dice * d.num * d.mp / (d.U * d.U));
  auto one = [&](float xv, float tv) {
    const FocalElem r = focal_elem<true>(xv, tv, alpha, gamma, gm);
    return kf * r.wpt - r.dp * (tv * c1 - c0);
  };
  if (blockIdx.x == 0 && (int)threadIdx.x < s.head + s.ntail) {
    const int64_t i = edge_index<V>(s, threadIdx.x);
    grad[i] = one(x[i], t[i]);
  }
  typedef typename FVec<V>::T vec_t;
  const vec_t* xv = reinterpret_cast<const vec_t*>(x + s.head);
  const vec_t* tv = reinterpret_cast<const vec_t*>(t + s.head);
  vec_t* gv = reinterpret_cast<vec_t*>(grad + s.head);
  for (int64_t i = (int64_t)blockIdx.x * FBLK + threadIdx.x; i < s.nvec; i += (int64_t)gridDim.x * FBLK) {
    const vec_t xx = __builtin_nontemporal_load(xv + i), tt = __builtin_nontemporal_load(tv + i);
    vec_t o;
#pragma unroll
    for (int k = 0; k < V; ++k) set_lane(o, k, one(lane(xx, k), lane(tt, k)));
    gv[i] = o;
  }
}

// The 16-byte body needs every pointer at the same offset from a 16-byte
// boundary (a contiguous view with a storage offset: a scalar head of up to 3
// elements).  Pointers that disagree have no common body: vec = false, and
// the V = 1 instantiations take the whole range as one-element "vectors".
Split split(int64_t n, const void* a, const void* b, const void* c, bool& vec) {
  const uintptr_t ma = (uintptr_t)a & 15, mb = (uintptr_t)b & 15, mc = c ? ((uintptr_t)c & 15) : ma;
  Split s;
  vec = ma == mb && ma == mc;
  if (!vec) {
    s.head = 0;
    s.nvec = n;
    s.ntail = 0;
    return s;
  }
  int64_t head = ((16 - (int64_t)ma) & 15) / 4;
  if (head > n) head = n;
  s.head = (int)head;
  s.nvec = (n - head) / 4;
  s.ntail = (int)(n - head - 4 * s.nvec);
  return s;
}

int gamma_mode(float gamma) {
  return gamma == 0.f ? GM_ZERO : gamma == 1.f ? GM_ONE : gamma == 2.f ? GM_TWO : GM_GENERAL;
}

int fblocks(int64_t work) {
  int64_t b = (work + FBLK - 1) / FBLK;
  if (b > FNB) b = FNB;
  if (b < 1) b = 1;
  return (int)b;
}

bool bad_args(int64_t n, float alpha, float gamma, float smooth) {
  return n < 1 || !(alpha >= 0.f && alpha <= 1.f) || !(gamma == 0.f || gamma >= 1.f) || !(smooth > 0.f);
}

}  // namespace

extern "C" int64_t vu_focal_workspace_bytes() { return (int64_t)FNB * FNQ * sizeof(double); }

extern "C" int vu_focal_dice_fwd(const float* logits, const float* target, int64_t n, float alpha, float gamma,
                                 float smooth, float w_focal, float w_dice, int sum_reduction, double* sums,
                                 float* loss, float* parts, double* workspace, void* stream) {
  if (bad_args(n, alpha, gamma, smooth) || !logits || !target || !sums || !workspace) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int gm = gamma_mode(gamma);
  bool vec;
  const Split s = split(n, logits, target, nullptr, vec);
  // four elements per thread and grid-stride trip in either form
  const int nb = fblocks(vec ? s.nvec : (n + 3) / 4);
  if (vec)
    hipLaunchKernelGGL(focal_stage1<4>, dim3(nb), dim3(FBLK), 0, st, logits, target, s, alpha, gamma, gm, workspace);
  else
    hipLaunchKernelGGL(focal_stage1<1>, dim3(nb), dim3(FBLK), 0, st, logits, target, s, alpha, gamma, gm, workspace);
  hipLaunchKernelGGL(focal_stage2, dim3(1), dim3(FBLK), 0, st, workspace, nb, n, smooth, w_focal, w_dice,
                     sum_reduction, sums, loss, parts);
  return (int)hipGetLastError();
}

extern "C" int vu_focal_dice_bwd(const float* logits, const float* target, int64_t n, float alpha, float gamma,
                                 float smooth, float w_focal, float w_dice, int sum_reduction, const double* sums,
                                 const float* gscale, float* grad, void* stream) {
  if (bad_args(n, alpha, gamma, smooth) || !logits || !target || !sums || !grad) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int gm = gamma_mode(gamma);
  bool vec;
  const Split s = split(n, logits, target, grad, vec);
  const int nb = fblocks(vec ? s.nvec : (n + 3) / 4);
  if (vec)
    hipLaunchKernelGGL(focal_bwd_kernel<4>, dim3(nb), dim3(FBLK), 0, st, logits, target, s, n, alpha, gamma, gm,
                       smooth, w_focal, w_dice, sum_reduction, sums, gscale, grad);
  else
    hipLaunchKernelGGL(focal_bwd_kernel<1>, dim3(nb), dim3(FBLK), 0, st, logits, target, s, n, alpha, gamma, gm,
                       smooth, w_focal, w_dice, sum_reduction, sums, gscale, grad);
  return (int)hipGetLastError();
}
