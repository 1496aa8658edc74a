"""The union-find core of the device labelling (vaeunet_amd/csrc/ccl_uf.h,
DESIGN.md §4.11) on the host, no GPU: a small program with its own main
includes the header, is built with the host C++ compiler and run.

The program runs the three phases of vu_ccl_label serially with the header's own
per-pixel steps -- the tile phase (row masks, run starts, ccl_row_unite on a
tile-local label array, roots written as plane-wide indices), the border phase
(ccl_border_unite on every pixel of a tile's first row / column) and the
flatten phase -- and compares every label with a stack-based flood fill's
canonical labels (1 + the component's smallest row-major index).  The tile edge
is a compile-time parameter, 4 and 8, so that a small plane has many borders
and corners.  Planes: all background, all foreground, checkerboard, a width-1
serpentine, a U joined in the last row, a comb of nested U's, diagonal lines of
both orientations (connected through tile corners only), Bernoulli planes at
p = 0.5927, 0.4073, 0.5 and 0.0085; connectivity 4 and 8.

Each case also runs with STALE reads: the program supplies VU_UF_LOAD itself and
serves, one read in four during the tile and border phases, the value the cell
held when the phase began (an older parent, which is what a stale cache line
gives).  ccl_find then stops at nodes that are no longer roots; the result must
still be exact, because ccl_unite trusts only what VU_UF_MIN returns.

Where the compiler's sanitizer runtime is present the program is also built with
-fsanitize=address,undefined: a plain executable, nothing preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <vector>

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// stale reads: while `stale_cur` is set, one load in four of a cell of that array returns what the cell held when
// the phase began
static const int32_t* stale_cur = nullptr;
static const int32_t* stale_old = nullptr;
static long stale_n = 0, stale_served = 0;
static int32_t load(const int32_t* p) {
  if (stale_cur && p >= stale_cur && p < stale_cur + stale_n && (rnd() & 3) == 0) {
    ++stale_served;
    return stale_old[p - stale_cur];
  }
  return *p;
}
static int32_t fetch_min(int32_t* p, int32_t v) {
  const int32_t old = *p;
  if (v < old) *p = v;
  return old;
}
#define VU_UF_LOAD(p) load(p)
#define VU_UF_MIN(p, v) fetch_min((p), (v))
#define VU_UF_STORE(p, v) (*(p) = (v))
#include "ccl_uf.h"

typedef std::vector<uint8_t> Plane;

static std::vector<int32_t> flood(const Plane& f, int H, int W, int conn) {
  std::vector<int32_t> lab((size_t)H * W, 0);
  std::vector<int32_t> stack;
  for (int32_t s = 0; s < H * W; ++s) {
    if (!f[s] || lab[s]) continue;
    lab[s] = s + 1;   // raster order: s is the smallest index of its component
    stack.push_back(s);
    while (!stack.empty()) {
      const int32_t i = stack.back();
      stack.pop_back();
      const int y = i / W, x = i % W;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if ((!dy && !dx) || (conn == 4 && dy && dx)) continue;
          const int yy = y + dy, xx = x + dx;
          if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
          const int32_t j = yy * W + xx;
          if (f[j] && !lab[j]) { lab[j] = s + 1; stack.push_back(j); }
        }
    }
  }
  return lab;
}

template <int T>
static std::vector<int32_t> label(const Plane& f, int H, int W, int conn, bool stale) {
  std::vector<int32_t> L((size_t)H * W, 0);
  // phase 1
  for (int y0 = 0; y0 < H; y0 += T)
    for (int x0 = 0; x0 < W; x0 += T) {
      int32_t lab[T * T], init[T * T];
      uint64_t rows[T];
      for (int r = 0; r < T; ++r) {
        uint64_t m = 0;
        for (int c = 0; c < T; ++c)
          if (y0 + r < H && x0 + c < W && f[(y0 + r) * W + x0 + c]) m |= 1ull << c;
        rows[r] = m;
        for (int c = 0; c < T; ++c) lab[r * T + c] = ((m >> c) & 1) ? r * T + ccl_run_start(m, c) + 1 : 0;
      }
      for (int i = 0; i < T * T; ++i) init[i] = lab[i];
      if (stale) { stale_cur = lab; stale_old = init; stale_n = T * T; }
      for (int r = 1; r < T; ++r)
        for (int c = 0; c < T; ++c)
          if ((rows[r] >> c) & 1) ccl_row_unite(lab, r * T, (r - 1) * T, c, rows[r], rows[r - 1], conn);
      stale_cur = nullptr;
      for (int r = 0; r < T; ++r)
        for (int c = 0; c < T; ++c)
          if (y0 + r < H && x0 + c < W && lab[r * T + c]) {
            const int32_t root = ccl_find(lab, r * T + c);
            L[(y0 + r) * W + x0 + c] = (y0 + root / T) * W + x0 + root % T + 1;
          }
    }
  // phase 2
  std::vector<int32_t> before(L);
  if (stale) { stale_cur = L.data(); stale_old = before.data(); stale_n = (long)L.size(); }
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const bool top = y > 0 && y % T == 0, left = x > 0 && x % T == 0;
      if ((top || left) && L[y * W + x]) ccl_border_unite(L.data(), H, W, y, x, top, left, conn);
    }
  stale_cur = nullptr;
  // phase 3
  for (int32_t i = 0; i < H * W; ++i)
    if (L[i]) ccl_flatten(L.data(), i);
  return L;
}

static long cases = 0;

static long check(const Plane& f, int H, int W, const char* name) {
  long bad = 0;
  for (int conn = 4; conn <= 8; conn += 4) {
    const std::vector<int32_t> want = flood(f, H, W, conn);
    for (int st = 0; st < 2; ++st) {
      const bool ok = label<4>(f, H, W, conn, st) == want && label<8>(f, H, W, conn, st) == want;
      ++cases;
      if (!ok) { std::printf("MISMATCH %s %dx%d conn %d stale %d\n", name, H, W, conn, st); ++bad; }
    }
  }
  return bad;
}

int main() {
  static const int shapes[][2] = {{1, 1}, {1, 70}, {70, 1}, {67, 131}, {33, 17}, {8, 8}, {9, 7}, {16, 24}, {5, 64}};
  static const double ps[] = {0.5927, 0.4073, 0.5, 0.0085};
  long bad = 0;
  for (const auto& s : shapes) {
    const int H = s[0], W = s[1];
    Plane f((size_t)H * W);
    auto at = [&](int y, int x) -> uint8_t& { return f[(size_t)y * W + x]; };
    auto clear = [&]() { for (auto& v : f) v = 0; };
    clear();
    bad += check(f, H, W, "background");
    for (auto& v : f) v = 1;
    bad += check(f, H, W, "foreground");
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) at(y, x) = (y + x) & 1;
    bad += check(f, H, W, "checkerboard");
    clear();   // serpentine: every other row full, joined alternately at the right and the left end
    for (int y = 0; y < H; ++y) {
      if (y % 2 == 0) for (int x = 0; x < W; ++x) at(y, x) = 1;
      else at(y, (y / 2) % 2 == 0 ? W - 1 : 0) = 1;
    }
    bad += check(f, H, W, "serpentine");
    clear();   // U: the two outer columns and the last row
    for (int y = 0; y < H; ++y) { at(y, 0) = 1; at(y, W - 1) = 1; }
    for (int x = 0; x < W; ++x) at(H - 1, x) = 1;
    bad += check(f, H, W, "U");
    clear();   // comb of nested U's: U k occupies columns 2k and W - 1 - 2k down to row H - 1 - 2k
    for (int k = 0; 4 * k + 2 < W && 2 * k < H; ++k) {
      const int l = 2 * k, r = W - 1 - 2 * k, b = H - 1 - 2 * k;
      for (int y = 0; y <= b; ++y) { at(y, l) = 1; at(y, r) = 1; }
      for (int x = l; x <= r; ++x) at(b, x) = 1;
    }
    bad += check(f, H, W, "comb");
    clear();
    for (int i = 0; i < H && i < W; ++i) at(i, i) = 1;
    bad += check(f, H, W, "diagonal");
    clear();
    for (int i = 0; i < H && i < W; ++i) at(i, W - 1 - i) = 1;
    bad += check(f, H, W, "antidiagonal");
    for (double p : ps) {
      for (auto& v : f) v = (double)(rnd() >> 11) * (1.0 / 9007199254740992.0) < p;
      bad += check(f, H, W, "bernoulli");
    }
  }
  std::printf("cases %ld bad %ld stale_reads %s\n", cases, bad, stale_served > 1000 ? "many" : "few");
  return bad != 0;
}
"""

EXPECT = "cases 432 bad 0 stale_reads many".split()   # 9 shapes x 12 planes x 2 connectivities x {fresh, stale}


def _build_and_run(tmp_path, name, flags):
    src, exe = tmp_path / "ccl_uf_check.cpp", tmp_path / name
    src.write_text(PROGRAM)
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I",
           os.path.join(ROOT, "vaeunet_amd", "csrc"), str(src), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0:
        return built, None
    return built, subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("c++") is None, reason="no host C++ compiler")
def test_three_phases_on_the_host_match_a_flood_fill(tmp_path):
    built, run = _build_and_run(tmp_path, "ccl_uf_check", [])
    assert built.returncode == 0, built.stderr
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.split()[-6:] == EXPECT, (run.stdout[-2000:], run.stderr[-2000:])


@pytest.mark.skipif(shutil.which("c++") is None, reason="no host C++ compiler")
def test_three_phases_on_the_host_under_asan_and_ubsan(tmp_path):
    built, run = _build_and_run(tmp_path, "ccl_uf_check_san",
                                ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert built.returncode == 0, built.stderr
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.split()[-6:] == EXPECT, (run.stdout[-2000:], run.stderr[-2000:])
