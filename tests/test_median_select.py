"""The selection network of the device median blur (vaeunet_amd/csrc/median_select.h,
DESIGN.md §4.10) on the host, no GPU: a small program with its own main includes
the header, is built with the host C++ compiler and run.

The network is data-oblivious (min / max only), so the 0-1 principle holds: it
selects the median of every input iff it does so for every input of zeros and
ones.  The program runs it bit-sliced, 64 cases per uint64_t word (lo = a & b,
hi = a | b), against a bit-sliced population count:
  n = 9   all 2^9 inputs
  n = 25  all 2^25 inputs
  n = 49  2^26 random 0/1 inputs (fixed seed), and every input that differs
          from all-0 or all-1 in at most two places
and, with the device's order (uint32 min / max), 10^5 random vectors per n
against std::sort, half of them drawn from 8 values (duplicates)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include "median_select.h"

struct Sliced {
  static uint64_t lo(uint64_t a, uint64_t b) { return a & b; }
  static uint64_t hi(uint64_t a, uint64_t b) { return a | b; }
};

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// per case (bit): 1 where at least (N + 1) / 2 of the N inputs are 1
template <int N>
static uint64_t majority(const uint64_t (&v)[N]) {
  uint64_t c[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < N; ++i) {
    uint64_t carry = v[i];
    for (int p = 0; p < 6; ++p) {
      const uint64_t t = c[p] & carry;
      c[p] ^= carry;
      carry = t;
    }
  }
  const int m = (N + 1) / 2;
  uint64_t gt = 0, eq = ~0ull;
  for (int p = 5; p >= 0; --p) {
    const uint64_t mb = ((m >> p) & 1) ? ~0ull : 0ull;
    gt |= eq & c[p] & ~mb;
    eq &= ~(c[p] ^ mb);
  }
  return gt | eq;
}

template <int N>
static long check(const uint64_t (&v)[N]) {
  return median_select<N, uint64_t, Sliced>(v) == majority(v) ? 0 : 1;
}

// all 2^N inputs: case x = 64 word + bit, input i of case x is bit i of x
template <int N>
static long exhaustive() {
  static const uint64_t low[6] = {0xaaaaaaaaaaaaaaaaull, 0xccccccccccccccccull, 0xf0f0f0f0f0f0f0f0ull,
                                  0xff00ff00ff00ff00ull, 0xffff0000ffff0000ull, 0xffffffff00000000ull};
  long bad = 0;
  for (uint64_t word = 0; word < (1ull << (N - 6)); ++word) {
    uint64_t v[N];
    for (int i = 0; i < N; ++i) v[i] = i < 6 ? low[i] : (((word >> (i - 6)) & 1) ? ~0ull : 0ull);
    bad += check(v);
  }
  return bad;
}

template <int N>
static long random01(long words) {
  long bad = 0;
  for (long w = 0; w < words; ++w) {
    uint64_t v[N];
    for (int i = 0; i < N; ++i) v[i] = rnd();
    bad += check(v);
  }
  return bad;
}

// every input at most two places away from all-0 or all-1; one case per word
template <int N>
static long near_constant(long* cases) {
  long bad = 0;
  for (int base = 0; base < 2; ++base)
    for (int i = -1; i < N; ++i)
      for (int j = i; j < N; ++j) {
        if (i < 0 && j >= 0) continue;   // (-1, -1): no flip; (i, i): one; (i, j): two
        uint64_t v[N];
        for (int k = 0; k < N; ++k) v[k] = ((k == i || k == j) != (base == 1)) ? ~0ull : 0ull;
        bad += check(v);
        ++*cases;
      }
  return bad;
}

template <int N>
static long against_sort(int vectors) {
  long bad = 0;
  for (int t = 0; t < vectors; ++t) {
    uint32_t v[N], s[N];
    for (int i = 0; i < N; ++i) s[i] = v[i] = (t & 1) ? (uint32_t)(rnd() & 7u) * 0x20000001u : (uint32_t)rnd();
    std::sort(s, s + N);
    bad += median_select<N>(v) != s[(N - 1) / 2];
  }
  return bad;
}

int main() {
  long near = 0;
  const long e9 = exhaustive<9>(), e25 = exhaustive<25>(), r49 = random01<49>(1l << 20), n49 = near_constant<49>(&near);
  const long s9 = against_sort<9>(100000), s25 = against_sort<25>(100000), s49 = against_sort<49>(100000);
  std::printf("exhaustive9 %ld exhaustive25 %ld random49 %ld near49 %ld of %ld sort %ld %ld %ld\n", e9, e25, r49, n49,
              near, s9, s25, s49);
  return (e9 | e25 | r49 | n49 | s9 | s25 | s49) != 0;
}
"""


@pytest.mark.skipif(shutil.which("c++") is None, reason="no host C++ compiler")
def test_selection_network_on_the_host(tmp_path):
    src, exe = tmp_path / "median_select_check.cpp", tmp_path / "median_select_check"
    src.write_text(PROGRAM)
    subprocess.run(["c++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "vaeunet_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    # 2 (1 + 49 + 49 * 48 / 2) near-constant inputs
    assert run.returncode == 0 and run.stdout.split() == (
        "exhaustive9 0 exhaustive25 0 random49 0 near49 0 of 2452 sort 0 0 0".split()), (run.stdout, run.stderr)
