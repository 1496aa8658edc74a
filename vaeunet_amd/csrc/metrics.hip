// Validation metrics (utils/metrics.py: dice_score, iou_score,
// precision_recall, specificity, accuracy, get_all_metrics) from ONE pass over
// a batch of logits and masks.
//
//   vu_seg_counts   per (image, class) plane: exact 64-bit counts (TP, FP, FN,
//                   TN) of pred = logit > 0.5 (raw logit, NaN -> false) against
//                   truth = (float)mask > 0.5.  Logits (fp32 / bf16) and masks
//                   (fp32 / uint8 / int64) are read in place through element
//                   strides; when the logits' resolution differs from the
//                   mask's, the logit at a mask pixel is the bilinear
//                   interpolation (F.interpolate's source-index rules, fp32)
//                   formed in registers -- the resized tensor never exists.
//   vu_seg_metrics  a counts table -> dice / iou / precision / recall /
//                   specificity / accuracy per plane and pooled, plus the
//                   running state of a validation meter, in one small launch.
//
// Two-stage reduction as csrc/loss.hip: per-block integer partials in a
// workspace, a second launch sums them per plane.  Integer sums: the result
// does not depend on the order or on the grid.
#include "common.h"
#include "../../include/vaeunet.h"

namespace {

constexpr int MBLK = 256;
constexpr int MNB = 1024;  // max stage-1 blocks per launch (when planes <= MNB)

enum { M_F32 = 0, M_U8 = 1, M_I64 = 2 };

template <typename T> VU_DEV bool truth1(const T* p) { return (float)(*p) > 0.5f; }

struct Plane {
  int64_t sb, sc, sh, sw;  // element strides of [B, C, H, W]
};

struct SegArgs {
  const void* x;
  const void* m;
  Plane xs, ms;
  int C, h, w, H, W;
  int nbx;             // stage-1 blocks per plane
  float sy, sx;        // source-index scale (rows, columns)
  int align;
  unsigned long long* ws;
  uint8_t* hard;       // optional [B, C, H, W] contiguous
};

// three per-thread counts -> ws[(plane * nbx + block) * 3 + {pred, truth, both}]
VU_DEV void block_store(uint32_t a32, uint32_t b32, uint32_t ab32, unsigned long long* ws) {
  __shared__ unsigned long long sh[3][MBLK / 64];
  unsigned long long a = a32, b = b32, ab = ab32;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
    ab += __shfl_xor(ab, o, 64);
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[0][wv] = a; sh[1][wv] = b; sh[2][wv] = ab; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    ws[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + k] = sh[k][0] + sh[k][1] + sh[k][2] + sh[k][3];
  }
}

// four consecutive elements of a dense plane as fp32 / as truth bits
VU_DEV void ld4(const float* p, float (&v)[4]) {
  const f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
  v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
}
VU_DEV void ld4(const bf16_t* p, float (&v)[4]) {
  const u32x2 q = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
  v[0] = __uint_as_float(q[0] << 16); v[1] = __uint_as_float(q[0] & 0xffff0000u);
  v[2] = __uint_as_float(q[1] << 16); v[3] = __uint_as_float(q[1] & 0xffff0000u);
}
VU_DEV void truth4(const float* p, bool (&t)[4]) {
  float v[4];
  ld4(p, v);
#pragma unroll
  for (int j = 0; j < 4; ++j) t[j] = v[j] > 0.5f;
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

// Dense planes (w-stride 1, h-stride W, H*W % 4 == 0, 4-element aligned) at
// equal resolution: 4 elements per lane per load (16 B of fp32 logits).
template <typename LT, typename MT>
__global__ void __launch_bounds__(MBLK) seg_counts_vec(SegArgs A) {
  const int plane = blockIdx.y, b = plane / A.C, c = plane - b * A.C;
  const LT* x = static_cast<const LT*>(A.x) + b * A.xs.sb + c * A.xs.sc;
  const MT* m = static_cast<const MT*>(A.m) + b * A.ms.sb + c * A.ms.sc;
  const int64_t n4 = ((int64_t)A.H * A.W) >> 2;
  uint8_t* hard = A.hard ? A.hard + (int64_t)plane * A.H * A.W : nullptr;
  uint32_t na = 0, nb = 0, nab = 0;
  for (int64_t i = (int64_t)blockIdx.x * MBLK + threadIdx.x; i < n4; i += (int64_t)gridDim.x * MBLK) {
    float v[4];
    bool t[4];
    ld4(x + 4 * i, v);
    truth4(m + 4 * i, t);
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool p = v[j] > 0.5f;
      na += p;
      nb += t[j];
      nab += p && t[j];
      bits |= (uint32_t)p << (8 * j);
    }
    if (hard) *reinterpret_cast<uint32_t*>(hard + 4 * i) = bits;
  }
  block_store(na, nb, nab, A.ws);
}

// F.interpolate(mode='bilinear') source index of destination index d
VU_DEV float src_index(float scale, int d, int align) {
  if (align) return scale * (float)d;
  const float s = scale * ((float)d + 0.5f) - 0.5f;
  return s < 0.f ? 0.f : s;
}

// Any strides; one mask pixel per lane per step.  RESIZE: the logit is the
// bilinear interpolation of the [h, w] logits at the pixel (ATen's fp32
// formula: h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11)).
template <typename LT, typename MT, bool RESIZE>
__global__ void __launch_bounds__(MBLK) seg_counts_any(SegArgs A) {
  const int plane = blockIdx.y, b = plane / A.C, c = plane - b * A.C;
  const LT* x = static_cast<const LT*>(A.x) + b * A.xs.sb + c * A.xs.sc;
  const MT* m = static_cast<const MT*>(A.m) + b * A.ms.sb + c * A.ms.sc;
  const int64_t n = (int64_t)A.H * A.W;  // < 2^31 (host check)
  uint8_t* hard = A.hard ? A.hard + (int64_t)plane * n : nullptr;
  const FastDiv dw((uint32_t)A.W);
  uint32_t na = 0, nb = 0, nab = 0;
  for (int64_t i = (int64_t)blockIdx.x * MBLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MBLK) {
    const int yy = (int)dw.div((uint32_t)i), xx = (int)((uint32_t)i - (uint32_t)yy * (uint32_t)A.W);
    float v;
    if (RESIZE) {
      const float fy = src_index(A.sy, yy, A.align), fx = src_index(A.sx, xx, A.align);
      const int y0 = min((int)fy, A.h - 1), x0 = min((int)fx, A.w - 1);
      const int y1 = y0 + (y0 < A.h - 1 ? 1 : 0), x1 = x0 + (x0 < A.w - 1 ? 1 : 0);
      const float ly = fy - (float)y0, lx = fx - (float)x0;
      const float hy = 1.f - ly, hx = 1.f - lx;
      const LT* r0 = x + y0 * A.xs.sh;
      const LT* r1 = x + y1 * A.xs.sh;
      const float v00 = ld1<LT>(r0 + x0 * A.xs.sw), v01 = ld1<LT>(r0 + x1 * A.xs.sw);
      const float v10 = ld1<LT>(r1 + x0 * A.xs.sw), v11 = ld1<LT>(r1 + x1 * A.xs.sw);
      v = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
    } else {
      v = ld1<LT>(x + yy * A.xs.sh + xx * A.xs.sw);
    }
    const bool p = v > 0.5f;
    const bool t = truth1<MT>(m + yy * A.ms.sh + xx * A.ms.sw);
    na += p;
    nb += t;
    nab += p && t;
    if (hard) hard[i] = p ? 1 : 0;
  }
  block_store(na, nb, nab, A.ws);
}

// one wave per plane: (pred, truth, both) partials -> (TP, FP, FN, TN)
__global__ void seg_counts_stage2(const unsigned long long* ws, int nbx, long long n, long long* counts,
                                  int accumulate) {
  const unsigned long long* p = ws + (int64_t)blockIdx.x * nbx * 3;
  unsigned long long a = 0, b = 0, ab = 0;
  for (int i = threadIdx.x; i < nbx; i += 64) { a += p[i * 3]; b += p[i * 3 + 1]; ab += p[i * 3 + 2]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
    ab += __shfl_xor(ab, o, 64);
  }
  if (threadIdx.x != 0) return;
  long long* o = counts + (int64_t)blockIdx.x * 4;
  const long long r[4] = {(long long)ab, (long long)(a - ab), (long long)(b - ab), n - (long long)(a + b - ab)};
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = accumulate ? o[k] + r[k] : r[k];
}

// The six metrics of one (TP, FP, FN, TN) row.  dice: the fp32 arithmetic of
// dice_score_stage2 (csrc/loss.hip) on a = TP + FP, b = TP + FN; the others in
// fp64 from the integers, rounded once.
VU_DEV void metrics_row(const long long* k, double eps, float* o) {
  const long long tp = k[0], fp = k[1], fn = k[2], tn = k[3];
  const unsigned long long a = (unsigned long long)(tp + fp), b = (unsigned long long)(tp + fn);
  const float epsilon = (float)eps;
  const float I = (float)(unsigned long long)tp, den = (float)a + (float)b;
  o[0] = (a + b == 0) ? 1.f : (2.f * I + epsilon) / (den + epsilon);
  const double TP = (double)tp, FP = (double)fp, FN = (double)fn, TN = (double)tn;
  o[1] = (float)((TP + eps) / (TP + FP + FN + eps));
  o[2] = (float)((TP + eps) / (TP + FP + eps));
  o[3] = (float)((TP + eps) / (TP + FN + eps));
  o[4] = (float)((TN + eps) / (TN + FP + eps));
  const long long tot = tp + fp + fn + tn;
  o[5] = tot == 0 ? 1.f : (float)((double)(tp + tn) / (double)tot);
}

// One block: per-plane rows, the pooled row (all planes summed first; stored,
// or added to pooled[] when pooled_accumulate), and class_total[c][4] += the
// counts of class c over the images (planes are [image][class]).
__global__ void __launch_bounds__(MBLK) seg_metrics_kernel(const long long* counts, int P, int C, double eps,
                                                           float* out, float* pooled, int pooled_accumulate,
                                                           long long* class_total) {
  __shared__ long long sh[4][MBLK / 64];
  if (out)
    for (int p = threadIdx.x; p < P; p += MBLK) metrics_row(counts + (int64_t)p * 4, eps, out + (int64_t)p * 6);
  if (class_total)
    for (int j = threadIdx.x; j < C * 4; j += MBLK) {
      long long s = 0;
      for (int p = j >> 2; p < P; p += C) s += counts[(int64_t)p * 4 + (j & 3)];
      class_total[j] += s;
    }
  if (!pooled) return;
  long long s[4] = {0, 0, 0, 0};
  for (int p = threadIdx.x; p < P; p += MBLK)
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += counts[(int64_t)p * 4 + k];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o, 64);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = s[k];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  long long t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) t[k] = sh[k][0] + sh[k][1] + sh[k][2] + sh[k][3];
  float r[6];
  metrics_row(t, eps, r);
#pragma unroll
  for (int k = 0; k < 6; ++k) pooled[k] = pooled_accumulate ? pooled[k] + r[k] : r[k];
}

// 1024 pixels per block and step: one 4-element vector per lane on the dense
// path, four scalar steps otherwise; beyond the cap the grid-stride loops run
int blocks_per_plane(int64_t planes, int64_t n) {
  int64_t nb = (n + MBLK * 4 - 1) / (MBLK * 4);
  const int64_t cap = planes >= MNB ? 1 : MNB / planes;
  if (nb > cap) nb = cap;
  if (nb < 1) nb = 1;
  return (int)nb;
}

bool aligned4(const void* p, int64_t sb, int64_t sc, int B, int C, int esize) {
  return ((uintptr_t)p % (4 * esize)) == 0 && (B == 1 || sb % 4 == 0) && (C == 1 || sc % 4 == 0);
}

float src_scale(int in, int out, int align) {
  if (align) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  return (float)in / (float)out;
}

template <typename LT, typename MT>
void launch(int kind, dim3 grid, hipStream_t st, const SegArgs& A) {
  if (kind == 0) hipLaunchKernelGGL((seg_counts_vec<LT, MT>), grid, dim3(MBLK), 0, st, A);
  else if (kind == 1) hipLaunchKernelGGL((seg_counts_any<LT, MT, false>), grid, dim3(MBLK), 0, st, A);
  else hipLaunchKernelGGL((seg_counts_any<LT, MT, true>), grid, dim3(MBLK), 0, st, A);
}

template <typename LT>
void launch_m(int mdtype, int kind, dim3 grid, hipStream_t st, const SegArgs& A) {
  if (mdtype == M_F32) launch<LT, float>(kind, grid, st, A);
  else if (mdtype == M_U8) launch<LT, uint8_t>(kind, grid, st, A);
  else launch<LT, int64_t>(kind, grid, st, A);
}

}  // namespace

extern "C" int64_t vu_seg_counts_workspace_bytes(int64_t planes) {
  return (planes > MNB ? planes : (int64_t)MNB) * 3 * (int64_t)sizeof(unsigned long long);
}

extern "C" int vu_seg_counts(const void* logits, int ldtype, const int64_t* lstride, int h, int w, const void* mask,
                             int mdtype, const int64_t* mstride, int B, int C, int H, int W, int align_corners,
                             int resize, int64_t* counts, int accumulate, uint8_t* hard, void* workspace,
                             void* stream) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || h < 1 || w < 1) return (int)hipErrorInvalidValue;
  if ((ldtype != VU_F32 && ldtype != VU_BF16) || mdtype < M_F32 || mdtype > M_I64) return (int)hipErrorInvalidValue;
  const int64_t n = (int64_t)H * W, planes = (int64_t)B * C;
  if (n >= ((int64_t)1 << 31) || (int64_t)h * w >= ((int64_t)1 << 31) || planes > 65535)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  SegArgs A;
  A.x = logits; A.m = mask;
  A.xs = Plane{lstride[0], lstride[1], lstride[2], lstride[3]};
  A.ms = Plane{mstride[0], mstride[1], mstride[2], mstride[3]};
  A.C = C; A.h = h; A.w = w; A.H = H; A.W = W;
  A.sy = src_scale(h, H, align_corners); A.sx = src_scale(w, W, align_corners);
  A.align = align_corners;
  A.ws = static_cast<unsigned long long*>(workspace);
  A.hard = hard;
  const bool rs = resize || h != H || w != W;
  int kind = rs ? 2 : 1;
  const int lsize = ldtype == VU_F32 ? 4 : 2, msize = mdtype == M_F32 ? 4 : (mdtype == M_U8 ? 1 : 8);
  if (!rs && (n & 3) == 0 && (H == 1 || A.xs.sh == W) && (H == 1 || A.ms.sh == W) && A.xs.sw == 1 &&
      A.ms.sw == 1 && aligned4(logits, A.xs.sb, A.xs.sc, B, C, lsize) &&
      aligned4(mask, A.ms.sb, A.ms.sc, B, C, msize) && (!hard || ((uintptr_t)hard & 3) == 0))
    kind = 0;
  A.nbx = blocks_per_plane(planes, n);
  const dim3 grid(A.nbx, (unsigned)planes);
  if (ldtype == VU_F32) launch_m<float>(mdtype, kind, grid, st, A);
  else launch_m<bf16_t>(mdtype, kind, grid, st, A);
  hipLaunchKernelGGL(seg_counts_stage2, dim3((unsigned)planes), dim3(64), 0, st, A.ws, A.nbx, (long long)n,
                     reinterpret_cast<long long*>(counts), accumulate);
  return (int)hipGetLastError();
}

extern "C" int vu_seg_metrics(const int64_t* counts, int P, int C, double eps, float* out, float* pooled,
                              int pooled_accumulate, int64_t* class_total, void* stream) {
  if (P < 1 || C < 1 || P % C) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(seg_metrics_kernel, dim3(1), dim3(MBLK), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(counts), P, C, eps, out, pooled, pooled_accumulate,
                     reinterpret_cast<long long*>(class_total));
  return (int)hipGetLastError();
}
