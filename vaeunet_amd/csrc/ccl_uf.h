// Union-find core of the connected-component labelling (ccl.hip, DESIGN.md
// §4.11).  The label image is its own forest: a background pixel holds 0, a
// foreground pixel i holds parent(i) + 1 with parent(i) <= i, and a root holds
// i + 1.  Links always go from the larger index to the smaller, so the root of
// a finished component is its first pixel in raster order and 1 + root is the
// canonical label.
//
// Concurrency: the only write that links is VU_UF_MIN (an atomic minimum that
// returns the value it replaced), so a cell only ever decreases and every
// value it held is an ancestor-or-self of the pixel.  ccl_find follows strictly
// decreasing indices: it ends after at most i steps whatever it reads, and a
// stale read (an older, larger value) only makes it stop at a node that is no
// longer a root.  ccl_unite does not trust it: the value VU_UF_MIN returns says
// whether the node still was a root when the link landed; when it was not, the
// parent it had is united with the other side instead, and the larger of the
// two indices has strictly decreased, so that loop is bounded too.  No code
// here waits for another thread.
//
// No HIP dependency: on the host VU_UF_HD is empty and the two accesses are
// plain serial code, so a host program can include this file and run the tile,
// border and flatten steps one after another (tests/test_ccl_uf.py; it may
// define VU_UF_LOAD / VU_UF_MIN itself, e.g. to serve stale values).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VU_UF_HD __host__ __device__ __forceinline__
#else
#define VU_UF_HD inline
#endif

#if !defined(VU_UF_LOAD)
#if defined(__HIPCC__)
// relaxed, agent scope: served by L2, never by a CU's L1 (which other CUs' writes do not refresh)
#define VU_UF_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define VU_UF_MIN(p, v) __hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define VU_UF_STORE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#else
#define VU_UF_LOAD(p) (*(p))
static inline int32_t vu_uf_min_serial(int32_t* p, int32_t v) {
  const int32_t old = *p;
  if (v < old) *p = v;
  return old;
}
#define VU_UF_MIN(p, v) vu_uf_min_serial((p), (v))
#define VU_UF_STORE(p, v) (*(p) = (v))
#endif
#endif

// index of the root above foreground pixel i (as far as the reads show it)
VU_UF_HD int32_t ccl_find(const int32_t* L, int32_t i) {
  int32_t p = VU_UF_LOAD(L + i) - 1;
  while (p < i && p >= 0) {   // strictly decreasing; p < 0 (a background cell) cannot be followed
    i = p;
    p = VU_UF_LOAD(L + i) - 1;
  }
  return i;
}

// join the components of foreground pixels a and b
VU_UF_HD void ccl_unite(int32_t* L, int32_t a, int32_t b) {
  for (;;) {
    a = ccl_find(L, a);
    b = ccl_find(L, b);
    if (a == b) return;
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    const int32_t old = VU_UF_MIN(L + a, b + 1) - 1;   // a's parent before the link: the truth
    if (old == a || old == b) return;                  // a was a root (now below b), or hung under b already
    a = old;   // a hung under old < a: cell a keeps min(old, b), the other one is joined to it here
  }
}

// column at which the run of set bits containing bit x starts (bit x of m set)
VU_UF_HD int ccl_run_start(uint64_t m, int x) {
  const uint64_t z = ~m & ((1ull << x) - 1ull);
  return z ? 64 - __builtin_clzll(z) : 0;
}

// Phase 1, one foreground pixel at column x of a tile row: unions with the row
// above.  cur / up: index in L of column 0 of the row / of the row above;
// C / U: foreground bits of the two rows (bit = column, zero outside the tile).
// One union per pair of touching runs, made at the first column of the lower
// run that touches the upper one, so a pixel makes at most two.
VU_UF_HD void ccl_row_unite(int32_t* L, int32_t cur, int32_t up, int x, uint64_t C, uint64_t U, int connectivity) {
  const bool cl = x > 0 && ((C >> (x - 1)) & 1), ul = x > 0 && ((U >> (x - 1)) & 1);
  const bool uc = (U >> x) & 1, ur = x < 63 && ((U >> (x + 1)) & 1);
  if (connectivity == 4) {
    if (uc && !(ul && cl)) ccl_unite(L, cur + x, up + x);   // the upper run starts here, or the lower one does
    return;
  }
  if (!cl) {   // the run starts here: the upper run over x - 1 (it covers x too when set), else the one over x
    if (ul) ccl_unite(L, cur + x, up + x - 1);
    else if (uc) ccl_unite(L, cur + x, up + x);
  }
  if (ur && !uc) ccl_unite(L, cur + x, up + x + 1);   // an upper run starts at x + 1: first touched from x
}

// Phase 2, one foreground pixel (y, x) of an H x W plane on a tile edge: unions
// with the neighbours in the tile above (top: y is a tile's first row, y > 0)
// and in the tile to the left (left: x is a tile's first column, x > 0),
// diagonals included at connectivity 8.  Every neighbour is inside the plane.
VU_UF_HD void ccl_border_unite(int32_t* L, int H, int W, int y, int x, bool top, bool left, int connectivity) {
  const int32_t i = y * W + x;
  const bool diag = connectivity == 8;
  if (top) {
    const int32_t u = i - W;
    if (L[u]) ccl_unite(L, i, u);
    if (diag && x > 0 && L[u - 1]) ccl_unite(L, i, u - 1);
    if (diag && x + 1 < W && L[u + 1]) ccl_unite(L, i, u + 1);
  }
  if (left) {
    if (L[i - 1]) ccl_unite(L, i, i - 1);
    if (diag && !top && y > 0 && L[i - W - 1]) ccl_unite(L, i, i - W - 1);
    if (diag && y + 1 < H && L[i + W - 1]) ccl_unite(L, i, i + W - 1);
  }
}

// Phase 3: a foreground pixel's cell becomes 1 + root.  Concurrent flattening
// only writes ancestors, so the walk still ends at the root.
VU_UF_HD int32_t ccl_flatten(int32_t* L, int32_t i) {
  const int32_t r = ccl_find(L, i);
  VU_UF_STORE(L + i, r + 1);
  return r;
}
