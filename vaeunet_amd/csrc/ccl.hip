// Lesion-level evaluation: connected-component labelling of
// the planes [H][W] of a contiguous [planes][H][W] tensor, per-component tables,
// candidate / ground-truth matching and the FROC curve.  Definitions:
// include/vaeunet.h.
//
//   vu_ccl_label        a tiled union-find in three launches (ccl_uf.h holds the
//                       union-find and the per-pixel steps):
//                       1. one block per 64 x 32 tile: a wave takes a tile row,
//                          its ballot is the row's foreground mask, every pixel
//                          starts under the first pixel of its row run and the
//                          runs of adjacent rows are united in LDS (one union
//                          per pair of touching runs); the tile's labels leave
//                          as plane-wide root indices + 1
//                       2. one thread per pixel on a tile's first row / first
//                          column: unions across the edge (diagonals and tile
//                          corners included at connectivity 8) by atomic
//                          minimum on the label image, larger root under smaller
//                       3. every label is replaced by its root + 1; roots are
//                          counted for ncomp
//                       The smaller index always wins, so a component's root is
//                       its first raster pixel: the label is canonical.  No
//                       block waits for another one; the only ordering is the
//                       kernel boundary, and every loop walks strictly
//                       decreasing indices.
//   vu_lesion_match     root-indexed uint32 tables (area, score bits, hit,
//                       detected-score) filled by integer atomics in three
//                       ordered passes: areas and scores; overlaps (a candidate
//                       must know its area to be kept); one pass over the root
//                       pixels for the counts and the two histograms.
//   vu_ccl_remove_small the same area pass, then a gather.
//   vu_lesion_metrics / vu_froc_metrics   small single-block launches, fp64.
//
// Offsets are 64-bit across planes and int32 within one (H W <= 2^31 - 2).  No
// neighbour outside the tile (phase 1) or outside the plane (phase 2) is read;
// ragged tiles are predicated, never padded.
#include "common.h"
#include "ccl_uf.h"
#include "lds_hist.h"
#include "../../include/vaeunet.h"

namespace {

constexpr int CT_W = 64, CT_H = 32, CT_BLK = 256;   // tile (one wave = one tile row), threads per block
constexpr int CBLK = 256;                            // the streaming passes
constexpr int CNB = 2048;                            // their blocks per plane, at most
constexpr unsigned CPLANES = 65535;                  // grid.y; further planes are looped over

static_assert(CT_W == 64, "a tile row is one wave: its ballot is the row mask");

VU_DEV bool is_fg(float v, float thr) { return v > thr; }       // NaN: background
VU_DEV bool is_fg(uint8_t v, float) { return v != 0; }

typedef unsigned long long ull;

// ---- phase 1 ----------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(CT_BLK)
ccl_tile_kernel(const T* __restrict__ x, float thr, int64_t planes, int H, int W, int ntx, int connectivity,
                int32_t* __restrict__ labels, ull* __restrict__ ncomp) {
  __shared__ int32_t lab[CT_H * CT_W];
  __shared__ uint64_t rows[CT_H];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ty = (int)blockIdx.x / ntx, tx = (int)blockIdx.x - ty * ntx;
  const int x0 = tx * CT_W, y0 = ty * CT_H, xx = x0 + lane;
  const int64_t n = (int64_t)H * W;
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    const T* src = x + plane * n;
    int32_t* dst = labels + plane * n;
    if (ncomp && blockIdx.x == 0 && threadIdx.x == 0) ncomp[plane] = 0;   // counted in phase 3
    for (int r = wv; r < CT_H; r += CT_BLK / 64) {
      const int yy = y0 + r;
      const bool in = yy < H && xx < W;
      const bool fg = in && is_fg(src[yy * W + xx], thr);
      const uint64_t m = __ballot(fg);
      if (lane == 0) rows[r] = m;
      lab[r * CT_W + lane] = fg ? r * CT_W + ccl_run_start(m, lane) + 1 : 0;
    }
    __syncthreads();
    for (int r = wv; r < CT_H; r += CT_BLK / 64) {
      if (r == 0) continue;
      const uint64_t c = rows[r];
      if ((c >> lane) & 1) ccl_row_unite(lab, r * CT_W, (r - 1) * CT_W, lane, c, rows[r - 1], connectivity);
    }
    __syncthreads();
    for (int r = wv; r < CT_H; r += CT_BLK / 64) {
      const int yy = y0 + r;
      if (yy < H && xx < W) {
        int32_t out = 0;
        if (lab[r * CT_W + lane]) {
          const int32_t root = ccl_find(lab, r * CT_W + lane);   // the tile's order is the plane's order
          out = (y0 + root / CT_W) * W + x0 + root % CT_W + 1;
        }
        dst[yy * W + xx] = out;
      }
    }
    __syncthreads();
  }
}

// ---- phase 2 ----------------------------------------------------------------
// ids [0, nh): the pixels of the first rows of the tile rows 1 .., then the
// pixels of the first columns of the tile columns 1 ..
__global__ void __launch_bounds__(CBLK)
ccl_border_kernel(int32_t* labels, int64_t planes, int H, int W, int connectivity) {
  const int64_t n = (int64_t)H * W;
  const int64_t nh = (int64_t)((H - 1) / CT_H) * W, nv = (int64_t)((W - 1) / CT_W) * H;
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    int32_t* L = labels + plane * n;
    for (int64_t id = (int64_t)blockIdx.x * CBLK + threadIdx.x; id < nh + nv; id += (int64_t)gridDim.x * CBLK) {
      int y, xx;
      if (id < nh) {
        y = ((int)(id / W) + 1) * CT_H;
        xx = (int)(id % W);
      } else {
        const int64_t j = id - nh;
        xx = ((int)(j / H) + 1) * CT_W;
        y = (int)(j % H);
      }
      if (L[y * W + xx])
        ccl_border_unite(L, H, W, y, xx, y > 0 && y % CT_H == 0, xx > 0 && xx % CT_W == 0, connectivity);
    }
  }
}

// ---- phase 3 ----------------------------------------------------------------
__global__ void __launch_bounds__(CBLK)
ccl_flatten_kernel(int32_t* labels, int64_t planes, int64_t n, ull* __restrict__ ncomp) {
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    int32_t* L = labels + plane * n;
    uint32_t roots = 0;
    for (int64_t i = (int64_t)blockIdx.x * CBLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CBLK)
      if (L[i]) roots += ccl_flatten(L, (int32_t)i) == (int32_t)i;
    if (ncomp) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) roots += __shfl_xor(roots, o, 64);
      if ((threadIdx.x & 63) == 0 && roots) atomicAdd(&ncomp[plane], (ull)roots);
    }
  }
}

// ---- component tables -------------------------------------------------------
// a label read from a caller's image: anything that is not 1 + an index of the plane counts as background, so no
// label value can form an address outside the plane's tables
VU_DEV int32_t label_at(const int32_t* L, int64_t i, int64_t n) {
  if (i >= n) return 0;
  const int32_t l = L[i];
  return (l > 0 && l <= n) ? l : 0;
}

// SCORE 0: areas only; 1: the score of every component is 1.0; 2: the maximum of the fp32 input, negatives as 0
template <int SCORE>
__global__ void __launch_bounds__(CBLK)
ccl_area_kernel(const int32_t* __restrict__ labels, const float* __restrict__ p, int64_t planes, int64_t n,
                uint32_t* __restrict__ area, uint32_t* __restrict__ score) {
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    const int32_t* L = labels + plane * n;
    // whole waves stay in the loop: the aggregation needs them converged
    for (int64_t base = (int64_t)blockIdx.x * CBLK; base < n; base += (int64_t)gridDim.x * CBLK) {
      const int64_t i = base + threadIdx.x;
      const int32_t l = label_at(L, i, n);
      const bool pend = l > 0;
      hist_add<2>(area + plane * n, l - 1, pend);
      if (SCORE) {
        uint32_t bits = 0x3f800000u;
        if (SCORE == 2 && pend) {
          const float v = p[plane * n + i];
          bits = __float_as_uint(v > 0.f ? v : 0.f);
        }
        hist_max<2>(score + plane * n, l - 1, bits, pend);
      }
    }
  }
}

// pass 2: a candidate that meets ground truth is hit; a kept one hands its score (+ 1: 0 = undetected) to the lesion
__global__ void __launch_bounds__(CBLK)
lesion_overlap_kernel(const int32_t* __restrict__ pl, const int32_t* __restrict__ gl, int64_t planes, int64_t n,
                      int min_area, const uint32_t* __restrict__ area, const uint32_t* __restrict__ score,
                      uint32_t* __restrict__ hit, uint32_t* __restrict__ det) {
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    const int64_t o = plane * n;
    for (int64_t base = (int64_t)blockIdx.x * CBLK; base < n; base += (int64_t)gridDim.x * CBLK) {
      const int64_t i = base + threadIdx.x;
      const int32_t lp = label_at(pl + o, i, n), lg = label_at(gl + o, i, n);
      const bool both = lp > 0 && lg > 0;
      bool kept = false;
      uint32_t s = 0;
      if (both) {
        const int64_t rp = o + lp - 1;
        if (VU_UF_LOAD(hit + rp) == 0) atomicOr(hit + rp, 1u);   // a stale 0 costs one more atomic
        kept = (int64_t)area[rp] >= min_area;
        s = score[rp] + 1u;
      }
      hist_max<2>(det + o, lg - 1, s, kept);
    }
  }
}

VU_DEV int froc_bin(uint32_t bits, int nb) {
  const float t = __uint_as_float(bits) * (float)nb;
  return t >= (float)nb ? nb - 1 : (int)t;
}

// pass 3: the root pixels; counts[plane] += (n_gt, n_gt_detected, n_pred kept, n_pred_fp)
__global__ void __launch_bounds__(CBLK)
lesion_roots_kernel(const int32_t* __restrict__ pl, const int32_t* __restrict__ gl, int64_t planes, int64_t n,
                    int min_area, int nb, const uint32_t* __restrict__ area, const uint32_t* __restrict__ score,
                    const uint32_t* __restrict__ hit, const uint32_t* __restrict__ det, ull* __restrict__ counts,
                    ull* __restrict__ hist_fp, ull* __restrict__ hist_gt) {
  __shared__ uint32_t sh[4][CBLK / 64];
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    const int64_t o = plane * n;
    uint32_t c[4] = {0, 0, 0, 0};
    for (int64_t base = (int64_t)blockIdx.x * CBLK; base < n; base += (int64_t)gridDim.x * CBLK) {
      const int64_t i = base + threadIdx.x;
      const int32_t lp = label_at(pl + o, i, n), lg = label_at(gl + o, i, n);
      bool fp = false, dt = false;
      int bfp = 0, bgt = 0;
      if (lp > 0 && lp - 1 == i && (int64_t)area[o + i] >= min_area) {
        fp = hit[o + i] == 0;
        c[2] += 1;
        c[3] += fp;
        bfp = froc_bin(score[o + i], nb);
      }
      if (lg > 0 && lg - 1 == i) {
        const uint32_t d = det[o + i];
        dt = d != 0;
        c[0] += 1;
        c[1] += dt;
        bgt = dt ? froc_bin(d - 1u, nb) : 0;
      }
      if (hist_fp) {
        hist_add<2>(hist_fp, bfp, fp);
        hist_add<2>(hist_gt, bgt, dt);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) c[k] += __shfl_xor(c[k], s, 64);
      if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = c[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
      ull t = 0;
#pragma unroll
      for (int w = 0; w < CBLK / 64; ++w) t += sh[threadIdx.x][w];
      if (t) atomicAdd(&counts[plane * 4 + threadIdx.x], t);
    }
    __syncthreads();
  }
}

// mask = the component's area >= min_area; areas = the area, at every foreground pixel
__global__ void __launch_bounds__(CBLK)
ccl_gather_kernel(const int32_t* __restrict__ labels, int64_t planes, int64_t n, int min_area,
                  const uint32_t* __restrict__ area, uint8_t* __restrict__ mask, int32_t* __restrict__ areas) {
  for (int64_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    const int64_t o = plane * n;
    for (int64_t i = (int64_t)blockIdx.x * CBLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CBLK) {
      const int32_t l = label_at(labels + o, i, n);
      const uint32_t a = l > 0 ? area[o + l - 1] : 0u;
      if (mask) mask[o + i] = (l > 0 && (int64_t)a >= min_area) ? 1 : 0;
      if (areas) areas[o + i] = (int32_t)a;
    }
  }
}

// ---- the small launches -----------------------------------------------------
// pooled over the rows of a counts table: sensitivity, precision (fp64 from the integers, eps as vu_seg_metrics,
// rounded once) and false positives per plane
__global__ void lesion_metrics_kernel(const long long* counts, int64_t rows, int64_t n_planes, double eps, float* out) {
  long long t[4] = {0, 0, 0, 0};
  for (int64_t r = threadIdx.x; r < rows; r += 64)
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] += counts[r * 4 + k];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t[k] += __shfl_xor(t[k], o, 64);
  if (threadIdx.x != 0) return;
  const double tp = (double)(t[2] - t[3]);
  out[0] = (float)(((double)t[1] + eps) / ((double)t[0] + eps));
  out[1] = (float)((tp + eps) / ((double)t[2] + eps));
  out[2] = (float)((double)t[3] / (double)n_planes);
}

constexpr int FBLK = 256;
constexpr int FROC_TARGETS = 7;

// one block; thread t owns the bins [t chunk, (t + 1) chunk)
__global__ void __launch_bounds__(FBLK)
froc_kernel(const long long* __restrict__ hist_fp, const long long* __restrict__ hist_gt,
            const long long* __restrict__ counts, int64_t rows, int64_t n_planes, int nb, double* __restrict__ sens,
            double* __restrict__ fppi, double* __restrict__ score) {
  __shared__ long long sfp[FBLK], sgt[FBLK], ngt_s;
  __shared__ double term[FROC_TARGETS];
  const int t = threadIdx.x, chunk = (nb + FBLK - 1) / FBLK;
  const int lo = min(t * chunk, nb), hi = min(lo + chunk, nb);
  long long a = 0, b = 0;
  for (int k = lo; k < hi; ++k) { a += hist_fp[k]; b += hist_gt[k]; }
  sfp[t] = a;
  sgt[t] = b;
  if (t < FROC_TARGETS) term[t] = 0.0;
  __syncthreads();
  if (t == 0) {   // suffix sums of the chunk totals, exclusive: what lies above each chunk
    long long ca = 0, cb = 0, g = 0;
    for (int j = FBLK - 1; j >= 0; --j) {
      const long long ta = sfp[j], tb = sgt[j];
      sfp[j] = ca;
      sgt[j] = cb;
      ca += ta;
      cb += tb;
    }
    for (int64_t r = 0; r < rows; ++r) g += counts[r * 4];
    ngt_s = g;
  }
  __syncthreads();
  const double ngt = (double)ngt_s, np = (double)n_planes;
  long long cf = sfp[t], cg = sgt[t];
  for (int k = hi - 1; k >= lo; --k) {
    cf += hist_fp[k];
    cg += hist_gt[k];
    const double s = (double)cg / ngt, f = (double)cf / np;   // 0 / 0: NaN when there is no ground truth
    sens[k] = s;
    fppi[k] = f;
    // fppi and sens both fall with k: the largest sens within a target is at the first bin within it
    const double fprev = k > 0 ? (double)(cf + hist_fp[k - 1]) / np : 0.0;
#pragma unroll
    for (int j = 0; j < FROC_TARGETS; ++j) {
      const double target = 0.125 * (double)(1 << j);
      if (f <= target && (k == 0 || fprev > target)) term[j] = s;
    }
  }
  __syncthreads();
  if (t == 0) {
    double sum = 0.0;
    for (int j = 0; j < FROC_TARGETS; ++j) sum += term[j];
    *score = sum / (double)FROC_TARGETS;
  }
}

bool plane_ok(int64_t planes, int H, int W) {
  return planes >= 0 && H >= 0 && W >= 0 && (int64_t)H * W <= VU_CCL_MAX_PLANE;
}

dim3 stream_grid(int64_t planes, int64_t n) {
  int64_t nbx = (n + CBLK * 4 - 1) / (CBLK * 4);
  if (nbx > CNB) nbx = CNB;
  if (nbx < 1) nbx = 1;
  return dim3((unsigned)nbx, (unsigned)(planes < CPLANES ? planes : CPLANES));
}

void launch_area(int score, const int32_t* labels, const void* p, int64_t planes, int64_t n, uint32_t* area,
                 uint32_t* sc, hipStream_t st) {
  const dim3 grid = stream_grid(planes, n);
  const float* pf = static_cast<const float*>(p);
  if (score == 0) hipLaunchKernelGGL(ccl_area_kernel<0>, grid, dim3(CBLK), 0, st, labels, pf, planes, n, area, sc);
  else if (score == 1) hipLaunchKernelGGL(ccl_area_kernel<1>, grid, dim3(CBLK), 0, st, labels, pf, planes, n, area, sc);
  else hipLaunchKernelGGL(ccl_area_kernel<2>, grid, dim3(CBLK), 0, st, labels, pf, planes, n, area, sc);
}

}  // namespace

extern "C" int64_t vu_ccl_workspace_bytes(int64_t planes, int H, int W) {
  if (!plane_ok(planes, H, W)) return -1;
  return 4 * planes * H * W * (int64_t)sizeof(uint32_t);
}

extern "C" int vu_ccl_label(const void* x, int dtype, float threshold, int64_t planes, int H, int W, int connectivity,
                            int32_t* labels, int64_t* ncomp, void* stream) {
  if (!plane_ok(planes, H, W) || (dtype != VU_CCL_U8 && dtype != VU_CCL_F32) ||
      (connectivity != 4 && connectivity != 8))
    return (int)hipErrorInvalidValue;
  if (planes == 0 || H == 0 || W == 0) return 0;
  if (!x || !labels) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)H * W;
  const int ntx = (W + CT_W - 1) / CT_W, nty = (H + CT_H - 1) / CT_H;
  const unsigned gy = (unsigned)(planes < CPLANES ? planes : CPLANES);
  ull* nc = reinterpret_cast<ull*>(ncomp);
  const dim3 tiles((unsigned)((int64_t)ntx * nty), gy);
  if (dtype == VU_CCL_U8)
    hipLaunchKernelGGL(ccl_tile_kernel<uint8_t>, tiles, dim3(CT_BLK), 0, st, static_cast<const uint8_t*>(x), threshold,
                       planes, H, W, ntx, connectivity, labels, nc);
  else
    hipLaunchKernelGGL(ccl_tile_kernel<float>, tiles, dim3(CT_BLK), 0, st, static_cast<const float*>(x), threshold,
                       planes, H, W, ntx, connectivity, labels, nc);
  const int64_t edge = (int64_t)(nty - 1) * W + (int64_t)(ntx - 1) * H;
  if (edge > 0) {
    int64_t nbx = (edge + CBLK - 1) / CBLK;
    if (nbx > CNB) nbx = CNB;
    hipLaunchKernelGGL(ccl_border_kernel, dim3((unsigned)nbx, gy), dim3(CBLK), 0, st, labels, planes, H, W,
                       connectivity);
  }
  hipLaunchKernelGGL(ccl_flatten_kernel, stream_grid(planes, n), dim3(CBLK), 0, st, labels, planes, n, nc);
  return (int)hipGetLastError();
}

extern "C" int vu_ccl_remove_small(const int32_t* labels, int64_t planes, int H, int W, int min_area, uint8_t* mask,
                                   int32_t* areas, void* workspace, void* stream) {
  if (!plane_ok(planes, H, W) || min_area < 1) return (int)hipErrorInvalidValue;
  if (planes == 0 || H == 0 || W == 0) return 0;
  if (!labels || !workspace || (!mask && !areas)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)H * W, total = planes * n;
  uint32_t* area = static_cast<uint32_t*>(workspace);
  hipError_t e = hipMemsetAsync(area, 0, total * sizeof(uint32_t), st);
  if (e != hipSuccess) return (int)e;
  launch_area(0, labels, nullptr, planes, n, area, nullptr, st);
  hipLaunchKernelGGL(ccl_gather_kernel, stream_grid(planes, n), dim3(CBLK), 0, st, labels, planes, n, min_area, area,
                     mask, areas);
  return (int)hipGetLastError();
}

extern "C" int vu_lesion_match(const int32_t* pred_labels, const int32_t* gt_labels, const void* pred, int dtype,
                               int64_t planes, int H, int W, int min_area, int nb, int64_t* counts, int64_t* hist_fp,
                               int64_t* hist_gt, void* workspace, void* stream) {
  if (!plane_ok(planes, H, W) || min_area < 1 || (dtype != VU_CCL_U8 && dtype != VU_CCL_F32) ||
      (hist_fp != nullptr) != (hist_gt != nullptr) || (hist_fp && (nb < 1 || nb > VU_FROC_MAX_BINS)))
    return (int)hipErrorInvalidValue;
  if (planes == 0) return 0;
  if (!counts) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, planes * 4 * sizeof(int64_t), st);
  if (e != hipSuccess) return (int)e;
  if (H == 0 || W == 0) return 0;
  if (!pred_labels || !gt_labels || !workspace || (dtype == VU_CCL_F32 && !pred)) return (int)hipErrorInvalidValue;
  const int64_t n = (int64_t)H * W, total = planes * n;
  uint32_t* area = static_cast<uint32_t*>(workspace);
  uint32_t *score = area + total, *hit = score + total, *det = hit + total;
  e = hipMemsetAsync(area, 0, 4 * total * sizeof(uint32_t), st);
  if (e != hipSuccess) return (int)e;
  launch_area(dtype == VU_CCL_F32 ? 2 : 1, pred_labels, pred, planes, n, area, score, st);
  const dim3 grid = stream_grid(planes, n);
  hipLaunchKernelGGL(lesion_overlap_kernel, grid, dim3(CBLK), 0, st, pred_labels, gt_labels, planes, n, min_area, area,
                     score, hit, det);
  hipLaunchKernelGGL(lesion_roots_kernel, grid, dim3(CBLK), 0, st, pred_labels, gt_labels, planes, n, min_area, nb,
                     area, score, hit, det, reinterpret_cast<ull*>(counts), reinterpret_cast<ull*>(hist_fp),
                     reinterpret_cast<ull*>(hist_gt));
  return (int)hipGetLastError();
}

extern "C" int vu_lesion_metrics(const int64_t* counts, int64_t rows, int64_t n_planes, double eps, float* out,
                                 void* stream) {
  if (!counts || !out || rows < 1 || n_planes < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(lesion_metrics_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(counts), rows, n_planes, eps, out);
  return (int)hipGetLastError();
}

extern "C" int vu_froc_metrics(const int64_t* hist_fp, const int64_t* hist_gt, const int64_t* counts, int64_t rows,
                               int64_t n_planes, int nb, double* sens, double* fppi, double* score, void* stream) {
  if (!hist_fp || !hist_gt || !counts || !sens || !fppi || !score || rows < 1 || n_planes < 1 || nb < 1 ||
      nb > VU_FROC_MAX_BINS)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(froc_kernel, dim3(1), dim3(FBLK), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(hist_fp), reinterpret_cast<const long long*>(hist_gt),
                     reinterpret_cast<const long long*>(counts), rows, n_planes, nb, sens, fppi, score);
  return (int)hipGetLastError();
}
