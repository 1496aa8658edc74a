// Boundary loss: the mean over all elements of phi * sigmoid(x),
// phi the signed distance map of the ground truth (sdf.hip).
//
//   p      = sigmoid(x)
//   loss   = (1 / n) sum phi p
//   grad   = g * phi * p (1 - p) / n
//   an element with a NaN logit or a non-finite phi adds nothing and gets gradient
//   0; it still counts in n
//
// Stage 1 streams logits and phi once and leaves three fp64 partials per block;
// stage 2 (one block) adds them in a fixed order and forms the loss on the
// device.  The backward is one elementwise kernel that reads a device scalar.
// No float atomics, no host synchronisation, results are bitwise repeatable (the
// grid is a function of n and the alignment only).
//
// The sigmoid derives from e = exp(-|x|) in (0, 1], as focal.hip's:
//   sigmoid(|x|) = 1 / (1 + e),  sigmoid(-|x|) = e / (1 + e),  p (1 - p) = e / (1 + e)^2
// so nothing is formed as 1 - (something near 1).
#include "common.h"
#include "../../include/vaeunet.h"

namespace {

constexpr int BBLK = 256;
constexpr int BNB = 2048;  // stage-1 / backward block cap (256 CUs x 8 blocks): grid-stride above it
constexpr int BNQ = 3;     // sum phi p, sum |phi| p, skipped elements

// a[k] <- the block's sum of a[k], in every thread: the BNQ quantities share one barrier
VU_DEV void block_sums(double (&a)[BNQ], double (*sh)[BBLK / 64]) {
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < BNQ; ++k) {
    a[k] = warp_sum_d(a[k]);
    if ((threadIdx.x & 63) == 0) sh[k][w] = a[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < BNQ; ++k) a[k] = sh[k][0] + sh[k][1] + sh[k][2] + sh[k][3];
}

VU_DEV bool bl_skip(float x, float phi) { return isnan(x) || !isfinite(phi); }

struct BlElem {
  float p, dp;  // sigmoid(x), sigmoid(x) sigmoid(-x)
};

VU_DEV BlElem bl_elem(float x) {
  const float e = expf(-fabsf(x));
  const float inv = 1.f / (1.f + e);
  const float hi = inv, lo = e * inv;  // sigmoid(|x|), sigmoid(-|x|)
  BlElem r;
  r.p = x >= 0.f ? hi : lo;
  r.dp = lo * hi;
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

template <int V> struct BVec;
template <> struct BVec<4> { typedef f32x4 T; };
template <> struct BVec<1> { typedef float T; };
VU_DEV float lane(const f32x4& v, int k) { return v[k]; }
VU_DEV float lane(float v, int) { return v; }
VU_DEV void set_lane(f32x4& v, int k, float f) { v[k] = f; }
VU_DEV void set_lane(float& v, int, float f) { v = f; }

template <int V>
VU_DEV int64_t edge_index(const Split& s, int k) { return k < s.head ? k : s.head + V * s.nvec + (k - s.head); }

template <int V>
__global__ __launch_bounds__(BBLK) void bl_stage1(const float* __restrict__ x, const float* __restrict__ phi, Split s,
                                                  double* ws) {
  __shared__ double sh[BNQ][BBLK / 64];
  double a[BNQ] = {0, 0, 0};
  auto acc = [&](float xv, float fv) {
    if (bl_skip(xv, fv)) {
      a[2] += 1.0;
      return;
    }
    const double t = (double)fv * (double)bl_elem(xv).p;   // exact: two fp32 factors
    a[0] += t;
    a[1] += fabs(t);
  };
  if (blockIdx.x == 0 && (int)threadIdx.x < s.head + s.ntail) {
    const int64_t i = edge_index<V>(s, threadIdx.x);
    acc(x[i], phi[i]);
  }
  typedef typename BVec<V>::T vec_t;
  const vec_t* xv = reinterpret_cast<const vec_t*>(x + s.head);
  const vec_t* fv = reinterpret_cast<const vec_t*>(phi + s.head);
  for (int64_t i = (int64_t)blockIdx.x * BBLK + threadIdx.x; i < s.nvec; i += (int64_t)gridDim.x * BBLK) {
    const vec_t xx = __builtin_nontemporal_load(xv + i), ff = __builtin_nontemporal_load(fv + i);
#pragma unroll
    for (int k = 0; k < V; ++k) acc(lane(xx, k), lane(ff, k));
  }
  block_sums(a, sh);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < BNQ; ++k) ws[(int64_t)k * BNB + blockIdx.x] = a[k];
}

__global__ __launch_bounds__(BBLK) void bl_stage2(const double* ws, int nblk, int64_t n, double* sums, float* loss) {
  __shared__ double sh[BNQ][BBLK / 64];
  double s[BNQ] = {0, 0, 0};
  for (int b = threadIdx.x; b < nblk; b += BBLK)
#pragma unroll
    for (int k = 0; k < BNQ; ++k) s[k] += ws[(int64_t)k * BNB + b];
  block_sums(s, sh);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < BNQ; ++k) sums[k] = s[k];
  if (loss) loss[0] = (float)(s[0] / (double)n);
}

template <int V>
__global__ __launch_bounds__(BBLK) void bl_bwd_kernel(const float* __restrict__ x, const float* __restrict__ phi, Split s,
                                                      int64_t n, const float* gscale, float* __restrict__ grad) {
  // grad = kf * phi * dp: the launch-uniform factor in fp64, rounded once
  const float kf = (float)((gscale ? (double)gscale[0] : 1.0) / (double)n);
  auto one = [&](float xv, float fv) { return bl_skip(xv, fv) ? 0.f : kf * fv * bl_elem(xv).dp; };
  if (blockIdx.x == 0 && (int)threadIdx.x < s.head + s.ntail) {
    const int64_t i = edge_index<V>(s, threadIdx.x);
    grad[i] = one(x[i], phi[i]);
  }
  typedef typename BVec<V>::T vec_t;
  const vec_t* xv = reinterpret_cast<const vec_t*>(x + s.head);
  const vec_t* fv = reinterpret_cast<const vec_t*>(phi + s.head);
  vec_t* gv = reinterpret_cast<vec_t*>(grad + s.head);
  for (int64_t i = (int64_t)blockIdx.x * BBLK + threadIdx.x; i < s.nvec; i += (int64_t)gridDim.x * BBLK) {
    const vec_t xx = __builtin_nontemporal_load(xv + i), ff = __builtin_nontemporal_load(fv + i);
    vec_t o;
#pragma unroll
    for (int k = 0; k < V; ++k) set_lane(o, k, one(lane(xx, k), lane(ff, k)));
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

int bblocks(int64_t work) {
  int64_t b = (work + BBLK - 1) / BBLK;
  if (b > BNB) b = BNB;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

extern "C" int64_t vu_boundary_loss_workspace_bytes() { return (int64_t)BNB * BNQ * sizeof(double); }

extern "C" int vu_boundary_loss_fwd(const float* logits, const float* phi, int64_t n, double* sums, float* loss,
                                    double* workspace, void* stream) {
  if (n < 1 || !logits || !phi || !sums || !workspace) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  bool vec;
  const Split s = split(n, logits, phi, nullptr, vec);
  // four elements per thread and grid-stride trip in either form
  const int nb = bblocks(vec ? s.nvec : (n + 3) / 4);
  if (vec) hipLaunchKernelGGL(bl_stage1<4>, dim3(nb), dim3(BBLK), 0, st, logits, phi, s, workspace);
  else hipLaunchKernelGGL(bl_stage1<1>, dim3(nb), dim3(BBLK), 0, st, logits, phi, s, workspace);
  hipLaunchKernelGGL(bl_stage2, dim3(1), dim3(BBLK), 0, st, workspace, nb, n, sums, loss);
  return (int)hipGetLastError();
}

extern "C" int vu_boundary_loss_bwd(const float* logits, const float* phi, int64_t n, const float* gscale, float* grad,
                                    void* stream) {
  if (n < 1 || !logits || !phi || !grad) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  bool vec;
  const Split s = split(n, logits, phi, grad, vec);
  const int nb = bblocks(vec ? s.nvec : (n + 3) / 4);
  if (vec) hipLaunchKernelGGL(bl_bwd_kernel<4>, dim3(nb), dim3(BBLK), 0, st, logits, phi, s, n, gscale, grad);
  else hipLaunchKernelGGL(bl_bwd_kernel<1>, dim3(nb), dim3(BBLK), 0, st, logits, phi, s, n, gscale, grad);
  return (int)hipGetLastError();
}
