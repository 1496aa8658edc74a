"""The per-pixel steps of the device distance transform and of the percentile
select (vaeunet_amd/csrc/edt_core.h) on the host, no GPU: a
small program with its own main includes the header, is built with the host C++
compiler and run.

The program runs the column pass (edt_col_step down, then up with edt_col_min;
whole columns, and columns cut into 16 and into 3 chunks joined by
edt_chunk_above / edt_chunk_below / edt_chunk_down as the kernel's blocks do),
the row pass (edt_row_search over the row's 16-bit vertical distances) and the
four digit passes of the radix select (edt_sel_match / edt_sel_digit /
edt_sel_step, rank from edt_rank) serially, and compares every squared distance
with a brute force over all sites and every percentile with a sorted copy.
Planes: no site, all sites, a single site in each corner, sites only in the
last column / the last row, one full row, one full column, a checkerboard, two
equidistant sites, Bernoulli planes at p = 0.5 and 0.0085; each as the site
set itself and as a foreground whose boundary is the site set.  One 1 x 16384
and one 16384 x 1 plane with the single site at one end reach d^2 = 16383^2.

Where the compiler's sanitizer runtime is present the program is also built with
-fsanitize=address,undefined: a plain executable, nothing preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "edt_core.h"

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

typedef std::vector<uint8_t> Plane;

static Plane boundary(const Plane& f, int H, int W) {
  Plane b((size_t)H * W, 0);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      if (!f[(size_t)y * W + x]) continue;
      const bool up = y > 0 && f[(size_t)(y - 1) * W + x], dn = y + 1 < H && f[(size_t)(y + 1) * W + x];
      const bool lf = x > 0 && f[(size_t)y * W + x - 1], rt = x + 1 < W && f[(size_t)y * W + x + 1];
      b[(size_t)y * W + x] = !(up && dn && lf && rt);
    }
  return b;
}

// the two passes as edt.hip runs them, one "thread" after another
static std::vector<int32_t> transform(const Plane& s, int H, int W) {
  std::vector<int32_t> g((size_t)H * W);
  for (int x = 0; x < W; ++x) {
    int32_t d = EDT_NONE;
    for (int y = 0; y < H; ++y) { d = edt_col_step(d, s[(size_t)y * W + x] != 0); g[(size_t)y * W + x] = d; }
    d = EDT_NONE;
    for (int y = H - 1; y >= 0; --y) {
      const int32_t down = g[(size_t)y * W + x];
      d = edt_col_step(d, down == 0);
      g[(size_t)y * W + x] = edt_col_min(down, d);
    }
  }
  std::vector<uint16_t> row(W);   // exactly W: a read outside [0, W) is out of bounds
  for (int y = 0; y < H; ++y) {
    for (int x = 0; x < W; ++x) row[x] = (uint16_t)g[(size_t)y * W + x];
    for (int x = 0; x < W; ++x) g[(size_t)y * W + x] = edt_row_search(row.data(), W, x);
  }
  return g;
}

// the column pass cut into SEG chunks per column, as edt.hip's blocks run it
template <int SEG>
static std::vector<int32_t> transform_chunked(const Plane& s, int H, int W) {
  std::vector<int32_t> g((size_t)H * W);
  const int rows = (H + SEG - 1) / SEG;
  for (int x = 0; x < W; ++x) {
    int32_t first[SEG], last[SEG];
    for (int k = 0; k < SEG; ++k) {
      const int y0 = std::min(k * rows, H), y1 = std::min(y0 + rows, H);
      int32_t d = EDT_NONE;
      first[k] = last[k] = -1;
      for (int y = y0; y < y1; ++y) {
        const bool site = s[(size_t)y * W + x] != 0;
        d = edt_col_step(d, site);
        g[(size_t)y * W + x] = d;
        if (site) { if (first[k] < 0) first[k] = y; last[k] = y; }
      }
    }
    for (int k = 0; k < SEG; ++k) {
      const int y0 = std::min(k * rows, H), y1 = std::min(y0 + rows, H);
      if (y0 >= y1) continue;
      const int32_t above = edt_chunk_above(last, 1, k, y0);
      int32_t d = edt_chunk_below(first, 1, k, SEG, y1);
      for (int y = y1 - 1; y >= y0; --y) {
        const int32_t down = edt_chunk_down(g[(size_t)y * W + x], above, y - y0);
        d = edt_col_step(d, down == 0);
        g[(size_t)y * W + x] = edt_col_min(down, d);
      }
    }
  }
  std::vector<uint16_t> row(W);
  for (int y = 0; y < H; ++y) {
    for (int x = 0; x < W; ++x) row[x] = (uint16_t)g[(size_t)y * W + x];
    for (int x = 0; x < W; ++x) g[(size_t)y * W + x] = edt_row_search(row.data(), W, x);
  }
  return g;
}

static std::vector<int32_t> brute(const Plane& s, int H, int W) {
  std::vector<int> sy, sx;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x)
      if (s[(size_t)y * W + x]) { sy.push_back(y); sx.push_back(x); }
  std::vector<int32_t> out((size_t)H * W, EDT_INF);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      int64_t best = EDT_INF;
      for (size_t k = 0; k < sy.size(); ++k) {
        const int64_t d = (int64_t)(y - sy[k]) * (y - sy[k]) + (int64_t)(x - sx[k]) * (x - sx[k]);
        best = std::min(best, d);
      }
      out[(size_t)y * W + x] = (int32_t)best;
    }
  return out;
}

// the q-th percentile of keys by the four digit passes
static uint32_t select_q(const std::vector<uint32_t>& keys, int q) {
  uint32_t prefix = 0, rank = (uint32_t)edt_rank(q, (int64_t)keys.size());
  for (int p = 0; p < 4; ++p) {
    uint32_t hist[256] = {0};
    for (uint32_t k : keys)
      if (edt_sel_match(k, prefix, p)) ++hist[edt_sel_digit(k, p)];
    prefix = (prefix << 8) | (uint32_t)edt_sel_step(hist, &rank);
  }
  return prefix;
}

static long cases = 0, bad = 0;

static void check(const Plane& s, int H, int W, const char* name) {
  const std::vector<int32_t> got = transform(s, H, W);
  ++cases;
  if (got != brute(s, H, W) || transform_chunked<16>(s, H, W) != got || transform_chunked<3>(s, H, W) != got) {
    std::printf("MISMATCH edt %s %dx%d\n", name, H, W);
    ++bad;
  }
  // the select on this plane's distances (the sentinel included when there is no site)
  std::vector<uint32_t> keys(got.begin(), got.end()), sorted(keys);
  std::sort(sorted.begin(), sorted.end());
  static const int qs[] = {1, 50, 95, 100};
  for (int q : qs) {
    ++cases;
    const uint32_t want = sorted[(size_t)(((int64_t)q * (int64_t)keys.size() + 99) / 100) - 1];
    if (select_q(keys, q) != want) { std::printf("MISMATCH select %s %dx%d q %d\n", name, H, W, q); ++bad; }
  }
}

static void both(const Plane& f, int H, int W, const char* name) {
  check(f, H, W, name);
  check(boundary(f, H, W), H, W, name);
}

int main() {
  static const int shapes[][2] = {{1, 1}, {1, 70}, {70, 1}, {33, 65}, {9, 7}, {2, 2}, {17, 40}};
  static const double ps[] = {0.5, 0.0085};
  for (const auto& sh : shapes) {
    const int H = sh[0], W = sh[1];
    Plane f((size_t)H * W);
    auto at = [&](int y, int x) -> uint8_t& { return f[(size_t)y * W + x]; };
    auto clear = [&]() { for (auto& v : f) v = 0; };
    clear();
    both(f, H, W, "none");
    for (auto& v : f) v = 1;
    both(f, H, W, "all");
    const int cy[4] = {0, 0, H - 1, H - 1}, cx[4] = {0, W - 1, 0, W - 1};
    for (int k = 0; k < 4; ++k) { clear(); at(cy[k], cx[k]) = 1; both(f, H, W, "corner"); }
    clear();
    for (int y = 0; y < H; ++y) at(y, W - 1) = 1;
    both(f, H, W, "last_column");
    clear();
    for (int x = 0; x < W; ++x) at(H - 1, x) = 1;
    both(f, H, W, "last_row");
    clear();
    for (int x = 0; x < W; ++x) at(H / 2, x) = 1;
    both(f, H, W, "full_row");
    clear();
    for (int y = 0; y < H; ++y) at(y, W / 2) = 1;
    both(f, H, W, "full_column");
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) at(y, x) = (y + x) & 1;
    both(f, H, W, "checkerboard");
    clear();
    at(H / 2, W / 4) = 1;
    at(H / 2, W / 4 + 2 * ((W - 1 - W / 4) / 2)) = 1;
    both(f, H, W, "equidistant");
    for (double p : ps) {
      for (auto& v : f) v = (double)(rnd() >> 11) * (1.0 / 9007199254740992.0) < p;
      both(f, H, W, "bernoulli");
    }
  }
  // the largest distances: the single site at one end of the longest row / column
  for (int t = 0; t < 2; ++t) {
    const int H = t ? 16384 : 1, W = t ? 1 : 16384;
    for (int end = 0; end < 2; ++end) {
      Plane f((size_t)H * W, 0);
      f[end ? (size_t)H * W - 1 : 0] = 1;
      const std::vector<int32_t> got = transform(f, H, W);
      ++cases;
      long wrong = transform_chunked<16>(f, H, W) != got;
      for (int i = 0; i < H * W; ++i) {
        const int64_t d = end ? H * W - 1 - i : i;
        wrong += got[i] != (int32_t)(d * d);
      }
      if (wrong || *std::max_element(got.begin(), got.end()) != 16383 * 16383) { std::printf("MISMATCH long %d %d\n", t, end); ++bad; }
    }
  }
  // ranks, and a select over keys that use all four digits
  ++cases;
  if (edt_rank(95, 1) != 1 || edt_rank(95, 20) != 19 || edt_rank(95, 21) != 20 || edt_rank(100, 7) != 7 ||
      edt_rank(1, 7) != 1 || edt_rank(100, 268435456) != 268435456 || edt_rank(95, 268435456) != 255013684) {
    std::printf("MISMATCH rank\n");
    ++bad;
  }
  std::vector<uint32_t> keys(5000);
  for (auto& k : keys) k = (uint32_t)rnd() >> (rnd() % 24);
  keys[0] = 0xffffffffu; keys[1] = 0; keys[2] = EDT_INF;
  std::vector<uint32_t> sorted(keys);
  std::sort(sorted.begin(), sorted.end());
  for (int q = 1; q <= 100; ++q) {
    ++cases;
    if (select_q(keys, q) != sorted[(size_t)((q * 5000 + 99) / 100) - 1]) { std::printf("MISMATCH wide select %d\n", q); ++bad; }
  }
  std::printf("cases %ld bad %ld\n", cases, bad);
  return bad != 0;
}
"""

# 7 shapes x 14 planes x {sites, boundary} x (1 transform + 4 selects) + 4 long + 1 rank + 100 wide selects
EXPECT = f"cases {7 * 14 * 2 * 5 + 4 + 1 + 100} bad 0".split()


def _build_and_run(tmp_path, name, flags):
    src, exe = tmp_path / "edt_core_check.cpp", tmp_path / name
    src.write_text(PROGRAM)
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I",
           os.path.join(ROOT, "vaeunet_amd", "csrc"), str(src), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0:
        return built, None
    return built, subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("c++") is None, reason="no host C++ compiler")
def test_both_passes_and_the_select_on_the_host_match_a_brute_force(tmp_path):
    built, run = _build_and_run(tmp_path, "edt_core_check", [])
    assert built.returncode == 0, built.stderr
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.split()[-4:] == EXPECT, (run.stdout[-2000:], run.stderr[-2000:])


@pytest.mark.skipif(shutil.which("c++") is None, reason="no host C++ compiler")
def test_both_passes_and_the_select_on_the_host_under_asan_and_ubsan(tmp_path):
    built, run = _build_and_run(tmp_path, "edt_core_check_san",
                                ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert built.returncode == 0, built.stderr
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.split()[-4:] == EXPECT, (run.stdout[-2000:], run.stderr[-2000:])
