"""The per-pair formulas, the reduction and the pair index of the sample-set
metrics (vaeunet_amd/csrc/sampleset_core.h) on the host, no
GPU: a small program with its own main includes the header, is built with the
host C++ compiler and run.

The program builds Gram matrices from explicit bit columns (all background, all
foreground, identical, pairwise disjoint, nested, one sample empty, truth empty,
everything empty, Bernoulli at 0.5 and at 0.0015; (S, M) from (1, 0) to (63, 1)
and (61, 3)) by a plain loop over pixels, and compares

* ss_dist / ss_dice with long-double quotients of the same integers,
* ss_metrics_plane (the serial composition the kernel's phases reproduce) with
  the nine columns computed independently in the program: plain nested loops
  that add in row-major order, exactly (the same fp64 operations in the same
  order), and with a long-double evaluation within 1e-12,
* ss_sum_block with the plain loop on sub-blocks of every offset and width
  (its eight-wide reads must not change the order nor read outside the block),
* ss_pair_ij / ss_pair_index round trip for every K in 1..64: the index
  enumerates the upper triangle in row-major order without a gap.

Where the compiler's sanitizer runtime is present the program is also built with
-fsanitize=address,undefined: a plain executable, nothing preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sampleset_core.h"

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }

static long cases = 0, bad = 0;
static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0 || (std::isnan(a) && std::isnan(b)); }

// columns: K vectors of n bits -> G by a loop over the pixels
static std::vector<int64_t> gram_of(const std::vector<std::vector<uint8_t>>& col) {
  const int K = (int)col.size();
  std::vector<int64_t> G((size_t)K * K, 0);
  for (int a = 0; a < K; ++a)
    for (int b = 0; b < K; ++b)
      for (size_t e = 0; e < col[a].size(); ++e) G[(size_t)a * K + b] += col[a][e] && col[b][e];
  return G;
}

static long double dl(const std::vector<int64_t>& G, int K, int a, int b) {
  const int64_t I = G[(size_t)a * K + b], U = G[(size_t)a * K + a] + G[(size_t)b * K + b] - I;
  return U == 0 ? 0.0L : 1.0L - (long double)I / (long double)U;
}
static long double cl(const std::vector<int64_t>& G, int K, int a, int b) {
  const int64_t I = G[(size_t)a * K + b], s = G[(size_t)a * K + a] + G[(size_t)b * K + b];
  return s == 0 ? 1.0L : 2.0L * (long double)I / (long double)s;
}

static void check(const std::vector<std::vector<uint8_t>>& col, int S, int M, const char* name) {
  const int K = S + M;
  const std::vector<int64_t> G = gram_of(col);
  std::vector<double> dist((size_t)K * K), dice((size_t)S * M + 1);
  double got[SS_NMETRICS];
  ss_metrics_plane(G.data(), S, M, dist.data(), dice.data(), got);

  // the same values, independently: fp64 in row-major order, and long double
  double want[SS_NMETRICS];
  long double wide[SS_NMETRICS];
  auto d = [&](int a, int b) {
    const int64_t I = G[(size_t)a * K + b], U = G[(size_t)a * K + a] + G[(size_t)b * K + b] - I;
    return U == 0 ? 0.0 : 1.0 - (double)I / (double)U;
  };
  auto c = [&](int a, int b) {
    const int64_t I = G[(size_t)a * K + b], s = G[(size_t)a * K + a] + G[(size_t)b * K + b];
    return s == 0 ? 1.0 : (double)(2 * I) / (double)s;
  };
  double div = 0, cross = 0, tdiv = 0, dsum = 0, lo = 2, hi = -1, asum = 0, q = 0;
  long double Ldiv = 0, Lcross = 0, Ltdiv = 0, Ldsum = 0, Lasum = 0, Lq = 0;
  for (int i = 0; i < S; ++i) for (int j = 0; j < S; ++j) { div += d(i, j); Ldiv += dl(G, K, i, j); }
  for (int i = 0; i < S; ++i) for (int m = S; m < K; ++m) {
    cross += d(i, m); Lcross += dl(G, K, i, m);
    dsum += c(i, m); Ldsum += cl(G, K, i, m);
    lo = std::min(lo, c(i, m)); hi = std::max(hi, c(i, m));
  }
  for (int a = S; a < K; ++a) for (int b = S; b < K; ++b) { tdiv += d(a, b); Ltdiv += dl(G, K, a, b); }
  for (int i = 0; i < S; ++i) { asum += (double)G[(size_t)i * K + i]; Lasum += (long double)G[(size_t)i * K + i]; }
  const double mean = asum / (double)S;
  const long double Lmean = Lasum / S;
  for (int i = 0; i < S; ++i) {
    const double t = (double)G[(size_t)i * K + i] - mean; q += t * t;
    const long double Lt = (long double)G[(size_t)i * K + i] - Lmean; Lq += Lt * Lt;
  }
  const double nan = std::nan("");
  want[SS_DIVERSITY] = div / ((double)S * (double)S);
  want[SS_AREA_MEAN] = mean;
  want[SS_AREA_STD] = std::sqrt(q / (double)S);
  wide[SS_DIVERSITY] = Ldiv / ((long double)S * S);
  wide[SS_AREA_MEAN] = Lmean;
  wide[SS_AREA_STD] = std::sqrt(Lq / S);
  if (M == 0) {
    for (int k : {SS_GED2, SS_CROSS, SS_TRUTH_DIVERSITY, SS_DICE_MEAN, SS_DICE_MIN, SS_DICE_MAX}) want[k] = wide[k] = nan;
  } else {
    const double sm = (double)S * (double)M;
    want[SS_CROSS] = cross / sm;
    want[SS_TRUTH_DIVERSITY] = tdiv / ((double)M * (double)M);
    want[SS_GED2] = 2.0 * want[SS_CROSS] - want[SS_DIVERSITY] - want[SS_TRUTH_DIVERSITY];
    want[SS_DICE_MEAN] = dsum / sm;
    want[SS_DICE_MIN] = lo;
    want[SS_DICE_MAX] = hi;
    wide[SS_CROSS] = Lcross / ((long double)S * M);
    wide[SS_TRUTH_DIVERSITY] = Ltdiv / ((long double)M * M);
    wide[SS_GED2] = 2 * wide[SS_CROSS] - wide[SS_DIVERSITY] - wide[SS_TRUTH_DIVERSITY];
    wide[SS_DICE_MEAN] = Ldsum / ((long double)S * M);
    wide[SS_DICE_MIN] = lo;
    wide[SS_DICE_MAX] = hi;
  }
  ++cases;
  for (int k = 0; k < SS_NMETRICS; ++k) {
    const bool area = k == SS_AREA_MEAN || k == SS_AREA_STD;
    const long double scale = area ? std::max(1.0L, std::fabs(wide[k])) : 1.0L;
    const bool close = std::isnan(want[k]) ? std::isnan(got[k]) : std::fabs((long double)got[k] - wide[k]) <= 1e-12L * scale;
    if (!same(got[k], want[k]) || !close) {
      std::printf("MISMATCH %s S %d M %d column %d: %.17g want %.17g wide %.17Lg\n", name, S, M, k, got[k], want[k], wide[k]);
      ++bad;
    }
  }
  // the per-pair functions against the long-double quotients: each is one division and at most one subtraction
  ++cases;
  for (int a = 0; a < K; ++a)
    for (int b = 0; b < K; ++b) {
      const int64_t I = G[(size_t)a * K + b], na = G[(size_t)a * K + a], nb = G[(size_t)b * K + b];
      const double x = ss_dist(I, na, nb), y = ss_dice(I, na, nb);
      if (std::fabs((long double)x - dl(G, K, a, b)) > 3e-16L || std::fabs((long double)y - cl(G, K, a, b)) > 3e-16L ||
          x < 0 || x > 1 || y < 0 || y > 1 || !same(x, ss_dist(I, nb, na)) || !same(y, ss_dice(I, nb, na))) {
        std::printf("MISMATCH pair %s %d %d\n", name, a, b);
        ++bad;
      }
    }
}

static void stacks(int S, int M, int n) {
  const int K = S + M;
  typedef std::vector<std::vector<uint8_t>> Cols;
  Cols z(K, std::vector<uint8_t>(n, 0));
  check(z, S, M, "all_empty");
  Cols f(K, std::vector<uint8_t>(n, 1));
  check(f, S, M, "foreground");
  std::vector<uint8_t> base(n);
  for (auto& v : base) v = uni() < 0.3;
  base[0] = 1;
  Cols same_(K, base);
  check(same_, S, M, "identical");
  Cols dis(z);
  for (int e = 0; e < n; ++e) if (e % (K + 1) < K) dis[e % (K + 1)][e] = 1;
  check(dis, S, M, "disjoint");
  Cols nest(z);
  for (int k = 0; k < K; ++k) for (int e = 0; e < (int)(((int64_t)n * (k + 1) + K - 1) / K); ++e) nest[k][e] = 1;
  check(nest, S, M, "nested");
  Cols one(same_);
  std::fill(one[S / 2].begin(), one[S / 2].end(), 0);
  check(one, S, M, "one_empty");
  Cols te(same_);
  for (int m = S; m < K; ++m) std::fill(te[m].begin(), te[m].end(), 0);
  check(te, S, M, "truth_empty");
  for (double p : {0.5, 0.0015}) {
    Cols b(z);
    for (auto& col : b) for (auto& v : col) v = uni() < p;
    check(b, S, M, "bernoulli");
  }
}

int main() {
  static const int sm[][2] = {{1, 0}, {1, 1}, {2, 1}, {5, 0}, {31, 1}, {32, 1}, {33, 3}, {63, 1}, {61, 3}, {32, 32}, {1, 63}};
  for (const auto& c : sm)
    for (int n : {1, 67, 1000}) stacks(c[0], c[1], n);

  // areas near 2^31: the integer sums |a| + |b| and 2 I need 64 bits, the variance squares 2^31
  {
    ++cases;
    const int64_t big = 2147483646;
    const int64_t G[9] = {big, big - 1, big, big - 1, big - 1, big - 1, big, big - 1, big};
    double dist[9], dice[3], out[SS_NMETRICS];
    ss_metrics_plane(G, 2, 1, dist, dice, out);
    const long double d01 = 1.0L - (long double)(big - 1) / (long double)big;
    const long double div = 2 * d01 / 4, cross = d01 / 2;
    if (std::fabs((long double)out[SS_GED2] - (2 * cross - div)) > 1e-12L || out[SS_AREA_MEAN] != (double)big - 0.5 ||
        out[SS_AREA_STD] != 0.5 || std::fabs((long double)out[SS_DICE_MIN] - 2.0L * (big - 1) / (2 * big - 1)) > 3e-16L ||
        out[SS_DICE_MAX] != 1.0) {
      std::printf("MISMATCH large areas\n");
      ++bad;
    }
  }

  // ss_sum_block: every offset and width of a 13 x 29 table inside a guarded buffer
  {
    ++cases;
    const int R = 13, Ccols = 29;
    std::vector<double> t((size_t)R * Ccols);
    for (auto& v : t) v = uni() * std::ldexp(1.0, (int)(rnd() % 40) - 20);
    for (int r0 = 0; r0 < R; r0 += 3)
      for (int nr = 0; r0 + nr <= R; nr += 2)
        for (int c0 = 0; c0 < Ccols; c0 += 5)
          for (int nc = 0; c0 + nc <= Ccols; ++nc) {
            double s = 0.0;
            for (int r = r0; r < r0 + nr; ++r) for (int c = c0; c < c0 + nc; ++c) s += t[(size_t)r * Ccols + c];
            if (!same(s, ss_sum_block(t.data(), Ccols, r0, nr, c0, nc))) { std::printf("MISMATCH sum %d %d %d %d\n", r0, nr, c0, nc); ++bad; }
            if (nr > 0 && nc > 0) {
              double lo, hi, a = t[(size_t)r0 * Ccols + c0], b = a;
              for (int r = r0; r < r0 + nr; ++r) for (int c = c0; c < c0 + nc; ++c) { a = std::min(a, t[(size_t)r * Ccols + c]); b = std::max(b, t[(size_t)r * Ccols + c]); }
              ss_minmax_block(t.data(), Ccols, r0, nr, c0, nc, &lo, &hi);
              if (lo != a || hi != b) { std::printf("MISMATCH minmax\n"); ++bad; }
            }
          }
  }

  // the pair index: row-major upper triangle, no gap, for every K
  for (int K = 1; K <= SS_MAX; ++K) {
    ++cases;
    int p = 0;
    bool ok = true;
    for (int i = 0; i < K; ++i)
      for (int j = i; j < K; ++j, ++p) {
        int a = -1, b = -1;
        ss_pair_ij(p, K, &a, &b);
        ok = ok && ss_pair_index(i, j, K) == p && a == i && b == j;
      }
    if (!ok || p != ss_npairs(K)) { std::printf("MISMATCH pairs K %d\n", K); ++bad; }
  }
  std::printf("cases %ld bad %ld\n", cases, bad);
  return bad != 0;
}
"""

# 11 (S, M) x 3 sizes x 9 stacks x (metrics + pairs) + large areas + sum_block + 64 values of K
EXPECT = f"cases {11 * 3 * 9 * 2 + 1 + 1 + 64} bad 0".split()


def _build_and_run(tmp_path, name, flags):
    src, exe = tmp_path / "sampleset_core_check.cpp", tmp_path / name
    src.write_text(PROGRAM)
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I",
           os.path.join(ROOT, "vaeunet_amd", "csrc"), str(src), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0:
        return built, None
    return built, subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("c++") is None, reason="no host C++ compiler")
def test_formulas_reduction_and_pair_index_on_the_host(tmp_path):
    built, run = _build_and_run(tmp_path, "sampleset_core_check", [])
    assert built.returncode == 0, built.stderr
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.split()[-4:] == EXPECT, (run.stdout[-2000:], run.stderr[-2000:])


@pytest.mark.skipif(shutil.which("c++") is None, reason="no host C++ compiler")
def test_formulas_reduction_and_pair_index_under_asan_and_ubsan(tmp_path):
    built, run = _build_and_run(tmp_path, "sampleset_core_check_san",
                                ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert built.returncode == 0, built.stderr
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.split()[-4:] == EXPECT, (run.stdout[-2000:], run.stderr[-2000:])
