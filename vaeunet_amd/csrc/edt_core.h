// Per-pixel steps of the exact squared Euclidean distance transform and of the
// surface statistics (edt.hip; definitions: include/vaeunet.h).
//
//   edt_col_step     the column scan: the vertical distance g to the nearest
//                    site seen so far, carried from one row to the next
//   edt_col_min      the smaller of the down and the up scan's distance
//   edt_chunk_*      the start values of a scan that covers a chunk of a column
//   edt_row_search   the bounded row search over a row of g (16 bits each)
//   edt_rank         the nearest-rank percentile's rank
//   edt_sel_*        one 8-bit digit step of the radix select over 32-bit keys
//
// Number ranges.  H, W <= 16384, so a vertical distance is <= 16383 and a real
// d^2 is <= 2 * 16383^2 < 2^29.  A column without a site has g = EDT_NONE =
// 32768: g^2 = 2^30 exceeds every real d^2, and 2^30 + dx^2 <= 2^30 + 2^28 fits
// uint32, so the row search adds in uint32 and never tests for "no site"; a
// result >= 2^30 means the row holds no finite g, i.e. the plane has no site.
//
// No HIP dependency: VU_EDT_HD is empty on the host, so a host program can
// include this file and run both passes and the select serially
// (tests/test_edt_core.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VU_EDT_HD __host__ __device__ __forceinline__
#else
#define VU_EDT_HD inline
#endif

#define EDT_INF 2147483647          // VU_EDT_INF
#define EDT_NONE 32768              // a vertical distance that no column reaches: no site seen yet

// the carried vertical distance after one more row: 0 on a site, one more below / above one, EDT_NONE before any
VU_EDT_HD int32_t edt_col_step(int32_t d, bool site) { return site ? 0 : (d >= EDT_NONE ? EDT_NONE : d + 1); }

VU_EDT_HD int32_t edt_col_min(int32_t down, int32_t up) { return down < up ? down : up; }

// A column cut into chunks of rows [y0, y1), each scanned on its own from
// EDT_NONE.  first / last: the rows of the first and the last site of every
// chunk, -1 for a chunk without one.  edt_chunk_above: the distance the row
// y0 - 1 has to the nearest site of the chunks before chunk k; edt_chunk_below:
// the distance the row y1 has to the nearest site of the chunks after it; both
// EDT_NONE when there is none.  stride: the distance between two chunks' entries.
VU_EDT_HD int32_t edt_chunk_above(const int32_t* last, int stride, int k, int y0) {
  for (int j = k - 1; j >= 0; --j)
    if (last[j * stride] >= 0) return y0 - 1 - last[j * stride];
  return EDT_NONE;
}
VU_EDT_HD int32_t edt_chunk_below(const int32_t* first, int stride, int k, int nchunks, int y1) {
  for (int j = k + 1; j < nchunks; ++j)
    if (first[j * stride] >= 0) return first[j * stride] - y1;
  return EDT_NONE;
}
// the down distance of row y0 + i of a chunk whose own scan gave `local`
VU_EDT_HD int32_t edt_chunk_down(int32_t local, int32_t above, int i) {
  return local >= EDT_NONE && above < EDT_NONE ? above + i + 1 : local;
}

VU_EDT_HD uint32_t edt_sq(uint16_t g) { return (uint32_t)g * (uint32_t)g; }

// min over x' of g[x']^2 + (x - x')^2, EDT_INF when the row has no finite g.
// Outwards from x in both directions; the search ends once dx^2 >= best: every
// candidate that is skipped costs at least dx^2.  Reads g[0, W) only.
VU_EDT_HD int32_t edt_row_search(const uint16_t* g, int W, int x) {
  uint32_t best = edt_sq(g[x]);
  const int far = x > W - 1 - x ? x : W - 1 - x;
  for (int dx = 1; dx <= far; ++dx) {
    const uint32_t dd = (uint32_t)dx * (uint32_t)dx;
    if (dd >= best) break;
    if (x - dx >= 0) {
      const uint32_t c = edt_sq(g[x - dx]) + dd;
      best = c < best ? c : best;
    }
    if (x + dx < W) {
      const uint32_t c = edt_sq(g[x + dx]) + dd;
      best = c < best ? c : best;
    }
  }
  return best >= (uint32_t)EDT_NONE * EDT_NONE ? EDT_INF : (int32_t)best;
}

// nearest rank, 1-based, of the q-th percentile of n values (q in 1..100, n >= 1): ceil(q n / 100)
VU_EDT_HD int64_t edt_rank(int q, int64_t n) { return ((int64_t)q * n + 99) / 100; }

// ---- radix select: pass p = 0..3 settles bits [31 - 8p, 24 - 8p] --------------
// the keys still in play at pass p: those whose top 8p bits equal the prefix
VU_EDT_HD bool edt_sel_match(uint32_t key, uint32_t prefix, int p) {
  return p == 0 || (key >> (32 - 8 * p)) == prefix;
}
VU_EDT_HD int edt_sel_digit(uint32_t key, int p) { return (int)((key >> (24 - 8 * p)) & 255u); }

// hist[256]: the digit counts of the keys in play; rank: 1-based among them.
// Returns the digit that holds the rank and makes rank relative to that digit's
// keys.  A rank outside 1..sum(hist) (an undefined plane) returns 255 or 0 and
// a rank that is not used.
VU_EDT_HD int edt_sel_step(const uint32_t* hist, uint32_t* rank) {
  uint32_t before = 0;
  for (int d = 0; d < 255; ++d) {
    if (before + hist[d] >= *rank) {
      *rank -= before;
      return d;
    }
    before += hist[d];
  }
  *rank -= before;
  return 255;
}
