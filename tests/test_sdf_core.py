"""The per-pixel steps of the device signed distance map
(vaeunet_amd/csrc/sdf_core.h with edt_core.h) on the host, no
GPU: a small program with its own main includes both headers, is built with the
host C++ compiler and run.

The program runs the column pass for both site sets at once (edt_col_step down,
then up with edt_col_min, the two distances packed by sdf_pack; whole columns,
and columns cut into 16 and into 3 chunks joined by edt_chunk_above /
edt_chunk_below / edt_chunk_down as the kernel's blocks do) and the row pass
(the packed row staged into two 16-bit rows of exactly W entries, then
edt_row_search over sdf_opposite's row, the sign by sdf_signed, 0 on a plane
with one class) serially, and compares every s2 with a brute force over all
pixel pairs and every phi (sdf_phi, with and without a clip) with the fp64
formula.  Planes: none, all, a single pixel in each corner, the last column /
the last row, one full row, one full column, a checkerboard, two equidistant
pixels, Bernoulli planes at p = 0.5 and 0.0085, each as the mask and as its
complement.  One 1 x 8192 and one 16384 x 1 plane with a single pixel at one
end reach the longest search and the largest distance.

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
#include <limits>
#include <vector>

#include "sdf_core.h"

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

typedef std::vector<uint8_t> Plane;

// the row pass as sdf.hip runs it: the row staged whole, then one "thread" after another
static void row_pass(std::vector<int32_t>& g, int H, int W) {
  std::vector<uint16_t> to_fg(W), to_bg(W);   // exactly W each: a read outside [0, W) is out of bounds
  for (int y = 0; y < H; ++y) {
    bool anyf = false, anyb = false;
    for (int x = 0; x < W; ++x) {
      const int32_t v = g[(size_t)y * W + x];
      to_fg[x] = sdf_gf(v);
      to_bg[x] = sdf_gb(v);
      anyf |= to_fg[x] != EDT_NONE;
      anyb |= to_bg[x] != EDT_NONE;
    }
    for (int x = 0; x < W; ++x) {
      int32_t s2 = 0;
      if (anyf && anyb) {
        const bool fg = sdf_is_fg(to_fg[x]);
        s2 = sdf_signed(edt_row_search(sdf_opposite(to_fg.data(), to_bg.data(), fg), W, x), fg);
      }
      g[(size_t)y * W + x] = s2;
    }
  }
}

// whole columns
static std::vector<int32_t> transform(const Plane& s, int H, int W) {
  std::vector<int32_t> g((size_t)H * W);
  for (int x = 0; x < W; ++x) {
    int32_t df = EDT_NONE, db = EDT_NONE;
    for (int y = 0; y < H; ++y) {
      const bool fg = s[(size_t)y * W + x] != 0;
      df = edt_col_step(df, fg);
      db = edt_col_step(db, !fg);
      g[(size_t)y * W + x] = sdf_pack(df, db);
    }
    df = db = EDT_NONE;
    for (int y = H - 1; y >= 0; --y) {
      const int32_t w = g[(size_t)y * W + x];
      const int32_t down_f = sdf_gf(w), down_b = sdf_gb(w);
      df = edt_col_step(df, down_f == 0);
      db = edt_col_step(db, down_b == 0);
      g[(size_t)y * W + x] = sdf_pack(edt_col_min(down_f, df), edt_col_min(down_b, db));
    }
  }
  row_pass(g, H, W);
  return g;
}

// the column pass cut into SEG chunks per column, as sdf.hip's blocks run it
template <int SEG>
static std::vector<int32_t> transform_chunked(const Plane& s, int H, int W) {
  std::vector<int32_t> g((size_t)H * W);
  const int rows = (H + SEG - 1) / SEG;
  for (int x = 0; x < W; ++x) {
    int32_t first[2][SEG], last[2][SEG];
    for (int k = 0; k < SEG; ++k) {
      const int y0 = std::min(k * rows, H), y1 = std::min(y0 + rows, H);
      int32_t df = EDT_NONE, db = EDT_NONE;
      first[0][k] = last[0][k] = first[1][k] = last[1][k] = -1;
      for (int y = y0; y < y1; ++y) {
        const bool fg = s[(size_t)y * W + x] != 0;
        df = edt_col_step(df, fg);
        db = edt_col_step(db, !fg);
        g[(size_t)y * W + x] = sdf_pack(df, db);
        const int c = fg ? 0 : 1;
        if (first[c][k] < 0) first[c][k] = y;
        last[c][k] = y;
      }
    }
    for (int k = 0; k < SEG; ++k) {
      const int y0 = std::min(k * rows, H), y1 = std::min(y0 + rows, H);
      if (y0 >= y1) continue;
      const int32_t above_f = edt_chunk_above(last[0], 1, k, y0), above_b = edt_chunk_above(last[1], 1, k, y0);
      int32_t df = edt_chunk_below(first[0], 1, k, SEG, y1), db = edt_chunk_below(first[1], 1, k, SEG, y1);
      for (int y = y1 - 1; y >= y0; --y) {
        const int32_t w = g[(size_t)y * W + x];
        const int32_t down_f = edt_chunk_down(sdf_gf(w), above_f, y - y0);
        const int32_t down_b = edt_chunk_down(sdf_gb(w), above_b, y - y0);
        df = edt_col_step(df, down_f == 0);
        db = edt_col_step(db, down_b == 0);
        g[(size_t)y * W + x] = sdf_pack(edt_col_min(down_f, df), edt_col_min(down_b, db));
      }
    }
  }
  row_pass(g, H, W);
  return g;
}

static std::vector<int32_t> brute(const Plane& s, int H, int W) {
  std::vector<int> py[2], px[2];   // 0: background pixels, 1: foreground pixels
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) { const int c = s[(size_t)y * W + x] != 0; py[c].push_back(y); px[c].push_back(x); }
  std::vector<int32_t> out((size_t)H * W, 0);
  if (py[0].empty() || py[1].empty()) return out;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int c = s[(size_t)y * W + x] != 0, o = 1 - c;
      int64_t best = std::numeric_limits<int64_t>::max();
      for (size_t k = 0; k < py[o].size(); ++k) {
        const int64_t d = (int64_t)(y - py[o][k]) * (y - py[o][k]) + (int64_t)(x - px[o][k]) * (x - px[o][k]);
        best = std::min(best, d);
      }
      out[(size_t)y * W + x] = (int32_t)(c ? -best : best);
    }
  return out;
}

static float phi_ref(int32_t s2, double clip) {
  double v = 0.0;
  if (s2 > 0) v = std::sqrt((double)s2);
  if (s2 < 0) v = 1.0 - std::sqrt(-(double)s2);
  float f = (float)v;
  const float c = (float)clip;
  return std::min(std::max(f, -c), c);
}

static long cases = 0, bad = 0;

static void check(const Plane& s, int H, int W, const char* name) {
  const std::vector<int32_t> got = transform(s, H, W), want = brute(s, H, W);
  ++cases;
  if (got != want || transform_chunked<16>(s, H, W) != got || transform_chunked<3>(s, H, W) != got) {
    std::printf("MISMATCH sdf %s %dx%d\n", name, H, W);
    ++bad;
  }
  static const double clips[] = {std::numeric_limits<double>::infinity(), 1.0, 2.5, 1e6};
  ++cases;
  long wrong = 0;
  for (double clip : clips)
    for (int32_t v : got) {
      const float a = sdf_phi(v, (float)clip), b = phi_ref(v, clip);
      wrong += std::memcmp(&a, &b, sizeof a) != 0;
    }
  if (wrong) { std::printf("MISMATCH phi %s %dx%d: %ld\n", name, H, W, wrong); ++bad; }
}

static void both(const Plane& f, int H, int W, const char* name) {
  check(f, H, W, name);
  Plane c(f);
  for (auto& v : c) v = !v;
  check(c, H, W, name);
}

int main() {
  // the packing: both halves over their whole range
  ++cases;
  for (int32_t a : {0, 1, 255, 256, 16383, 32767, EDT_NONE})
    for (int32_t b : {0, 1, 255, 256, 16383, 32767, EDT_NONE}) {
      const int32_t w = sdf_pack(a, b);
      if (sdf_gf(w) != a || sdf_gb(w) != b || sdf_is_fg(sdf_gf(w)) != (a == 0)) { std::printf("MISMATCH pack %d %d\n", a, b); ++bad; }
    }
  static const int shapes[][2] = {{1, 1}, {1, 70}, {70, 1}, {33, 65}, {9, 7}, {2, 2}, {17, 40}};
  static const double ps[] = {0.5, 0.0085};
  for (const auto& sh : shapes) {
    const int H = sh[0], W = sh[1];
    Plane f((size_t)H * W);
    auto at = [&](int y, int x) -> uint8_t& { return f[(size_t)y * W + x]; };
    auto clear = [&]() { for (auto& v : f) v = 0; };
    clear();
    both(f, H, W, "none");          // its complement is "all"
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
  // the longest row the row pass takes and the longest column, the single pixel at one end
  for (int t = 0; t < 2; ++t) {
    const int H = t ? 16384 : 1, W = t ? 1 : 8192;
    for (int end = 0; end < 2; ++end)
      for (int inv = 0; inv < 2; ++inv) {
        Plane f((size_t)H * W, (uint8_t)inv);
        const int site = end ? H * W - 1 : 0;
        f[site] = (uint8_t)!inv;
        const std::vector<int32_t> got = transform(f, H, W);
        ++cases;
        long wrong = transform_chunked<16>(f, H, W) != got;
        for (int i = 0; i < H * W; ++i) {
          const int64_t d = i > site ? i - site : site - i;
          // the single pixel sees its neighbour of the other class at distance 1
          const int64_t want = i == site ? -1 : d * d;
          wrong += got[i] != (int32_t)(inv ? -want : want);
        }
        if (wrong) { std::printf("MISMATCH long %d %d %d: %ld\n", t, end, inv, wrong); ++bad; }
      }
  }
  std::printf("cases %ld bad %ld\n", cases, bad);
  return bad != 0;
}
"""

# 1 packing + 7 shapes x 13 planes x {mask, complement} x (s2 + phi) + 2 x 2 x 2 long
EXPECT = f"cases {1 + 7 * 13 * 2 * 2 + 8} bad 0".split()


def _build_and_run(tmp_path, name, flags):
    src, exe = tmp_path / "sdf_core_check.cpp", tmp_path / name
    src.write_text(PROGRAM)
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I",
           os.path.join(ROOT, "vaeunet_amd", "csrc"), str(src), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0:
        return built, None
    return built, subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("c++") is None, reason="no host C++ compiler")
def test_both_passes_on_the_host_match_a_brute_force(tmp_path):
    built, run = _build_and_run(tmp_path, "sdf_core_check", [])
    assert built.returncode == 0, built.stderr
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.split()[-4:] == EXPECT, (run.stdout[-2000:], run.stderr[-2000:])


@pytest.mark.skipif(shutil.which("c++") is None, reason="no host C++ compiler")
def test_both_passes_on_the_host_under_asan_and_ubsan(tmp_path):
    built, run = _build_and_run(tmp_path, "sdf_core_check_san",
                                ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert built.returncode == 0, built.stderr
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.split()[-4:] == EXPECT, (run.stdout[-2000:], run.stderr[-2000:])
