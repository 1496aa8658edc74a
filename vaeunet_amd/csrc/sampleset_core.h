// Per-pair formulas and the reduction of the sample-set metrics (sampleset.hip,
// DESIGN.md §4.14; definitions: include/vaeunet.h), and the mapping between a
// pair index and its (i, j) that the Gram kernel deals its lanes by.
//
//   ss_npairs / ss_pair_index / ss_pair_ij   the K (K + 1) / 2 unordered pairs i <= j of K columns in
//                                            row-major order of the upper triangle: (0,0) (0,1) .. (0,K-1)
//                                            (1,1) .. (K-1,K-1)
//   ss_dist / ss_dice                        d(a, b) = 1 - I / U and Dice(a, b) = 2 I / (|a| + |b|) in fp64
//                                            from the integers; 0 and 1 when both columns are empty
//   ss_sum_block                             the fp64 sum of a sub-block of a row-major table, i outer, j
//                                            inner, from 0.0: THE summation order of every mean below
//   ss_minmax_block                          its minimum and maximum
//   ss_area_stats                            mean and population standard deviation of the diagonal
//   ss_finish                                the nine output columns from the four sums
//   ss_metrics_plane                         all of it serially from one plane's Gram matrix: what the
//                                            kernel computes with its terms formed in parallel
//
// No HIP dependency, as edt_core.h: a host program can include this file
// (tests/test_sampleset_core.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VU_SS_HD __host__ __device__ __forceinline__
#else
#define VU_SS_HD inline
#endif

#define SS_MAX 64        // = VU_SAMPLESET_MAX
#define SS_NMETRICS 9    // = VU_SAMPLESET_NMETRICS
enum { SS_GED2 = 0, SS_CROSS, SS_DIVERSITY, SS_TRUTH_DIVERSITY, SS_DICE_MEAN, SS_DICE_MIN, SS_DICE_MAX, SS_AREA_MEAN,
       SS_AREA_STD };

// ---- pairs -----------------------------------------------------------------------
VU_SS_HD int ss_npairs(int K) { return K * (K + 1) / 2; }

// 0 <= i <= j < K
VU_SS_HD int ss_pair_index(int i, int j, int K) { return i * K - i * (i - 1) / 2 + (j - i); }

// 0 <= p < ss_npairs(K); K <= SS_MAX, so every term is exact in fp32; the two loops
// correct whatever the rounding of the root leaves
VU_SS_HD void ss_pair_ij(int p, int K, int* i, int* j) {
  const int b = 2 * K + 1;
  int r = (int)(((float)b - sqrtf((float)(b * b - 8 * p))) * 0.5f);
  r = r < 0 ? 0 : (r > K - 1 ? K - 1 : r);
  while (r > 0 && ss_pair_index(r, r, K) > p) --r;
  while (r + 1 < K && ss_pair_index(r + 1, r + 1, K) <= p) ++r;
  *i = r;
  *j = r + (p - ss_pair_index(r, r, K));
}

// ---- one pair: I = |a & b|, na = |a|, nb = |b| ------------------------------------
VU_SS_HD double ss_dist(int64_t I, int64_t na, int64_t nb) {
  const int64_t U = na + nb - I;
  return U == 0 ? 0.0 : 1.0 - (double)I / (double)U;
}

VU_SS_HD double ss_dice(int64_t I, int64_t na, int64_t nb) {
  const int64_t s = na + nb;
  return s == 0 ? 1.0 : (double)(2 * I) / (double)s;
}

// ---- sums over a table t[r * ld + c], rows [r0, r0 + nr), columns [c0, c0 + nc) ----
// The terms are read eight at a time and added one by one: the order is the plain loop's.
VU_SS_HD double ss_sum_block(const double* t, int ld, int r0, int nr, int c0, int nc) {
  double s = 0.0;
  for (int r = r0; r < r0 + nr; ++r) {
    const double* row = t + r * ld + c0;
    int c = 0;
    for (; c + 8 <= nc; c += 8) {
      double v[8];
      for (int u = 0; u < 8; ++u) v[u] = row[c + u];
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; c < nc; ++c) s += row[c];
  }
  return s;
}

// nr nc >= 1
VU_SS_HD void ss_minmax_block(const double* t, int ld, int r0, int nr, int c0, int nc, double* lo, double* hi) {
  double a = t[r0 * ld + c0], b = a;
  for (int r = r0; r < r0 + nr; ++r)
    for (int c = c0; c < c0 + nc; ++c) {
      const double v = t[r * ld + c];
      a = v < a ? v : a;
      b = v > b ? v : b;
    }
  *lo = a;
  *hi = b;
}

// G: one plane's [K][K] matrix; the areas of columns 0 .. S - 1 in that order, two passes
VU_SS_HD void ss_area_stats(const int64_t* G, int K, int S, double* mean, double* sd) {
  double s = 0.0;
  for (int i = 0; i < S; ++i) s += (double)G[i * K + i];
  const double m = s / (double)S;
  double q = 0.0;
  for (int i = 0; i < S; ++i) {
    const double d = (double)G[i * K + i] - m;
    q += d * d;
  }
  *mean = m;
  *sd = sqrt(q / (double)S);
}

// sums of d over the S M sample-truth pairs, the S S sample pairs, the M M truth pairs; of Dice over the S M pairs
VU_SS_HD void ss_finish(int S, int M, double sum_cross, double sum_div, double sum_tdiv, double sum_dice, double dice_lo,
                        double dice_hi, double area_mean, double area_sd, double* out) {
  const double nan = (double)NAN;
  const double div = sum_div / ((double)S * (double)S);
  out[SS_DIVERSITY] = div;
  out[SS_AREA_MEAN] = area_mean;
  out[SS_AREA_STD] = area_sd;
  if (M == 0) {
    out[SS_GED2] = out[SS_CROSS] = out[SS_TRUTH_DIVERSITY] = nan;
    out[SS_DICE_MEAN] = out[SS_DICE_MIN] = out[SS_DICE_MAX] = nan;
    return;
  }
  const double sm = (double)S * (double)M;
  const double cross = sum_cross / sm, tdiv = sum_tdiv / ((double)M * (double)M);
  out[SS_GED2] = 2.0 * cross - div - tdiv;
  out[SS_CROSS] = cross;
  out[SS_TRUTH_DIVERSITY] = tdiv;
  out[SS_DICE_MEAN] = sum_dice / sm;
  out[SS_DICE_MIN] = dice_lo;
  out[SS_DICE_MAX] = dice_hi;
}

// dist: K K doubles, dice: S M doubles, filled here: dist[a][b] for every pair of columns, dice[i][m] for the
// sample-truth pairs
VU_SS_HD void ss_metrics_plane(const int64_t* G, int S, int M, double* dist, double* dice, double* out) {
  const int K = S + M;
  for (int a = 0; a < K; ++a)
    for (int b = 0; b < K; ++b) dist[a * K + b] = ss_dist(G[a * K + b], G[a * K + a], G[b * K + b]);
  for (int i = 0; i < S; ++i)
    for (int m = 0; m < M; ++m) dice[i * M + m] = ss_dice(G[i * K + S + m], G[i * K + i], G[(S + m) * K + S + m]);
  double lo = 0.0, hi = 0.0, mean, sd;
  if (M > 0) ss_minmax_block(dice, M, 0, S, 0, M, &lo, &hi);
  ss_area_stats(G, K, S, &mean, &sd);
  ss_finish(S, M, ss_sum_block(dist, K, 0, S, S, M), ss_sum_block(dist, K, 0, S, 0, S), ss_sum_block(dist, K, S, M, S, M),
            ss_sum_block(dice, M, 0, S, 0, M), lo, hi, mean, sd, out);
}
