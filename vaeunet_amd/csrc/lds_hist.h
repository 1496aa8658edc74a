// Table increment / maximum with per-wave aggregation of equal indices
// (calib.hip, filters.hip: LDS histograms; ccl.hip: the
// per-component tables in global memory).
#pragma once
#include "common.h"

// One peel round, called inside a branch on "this lane is pending": the lanes
// that share the index of the first pending lane.  Returns true on them;
// first = that index, mask = their ballot.
VU_DEV bool peel_same(int idx, int& first, unsigned long long& mask) {
  first = __builtin_amdgcn_readfirstlane(idx);
  const bool same = idx == first;
  mask = __ballot(same);
  return same;
}
// the one lane of mask that acts for all of them
VU_DEV bool peel_leader(unsigned long long mask) { return (int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1; }

// h[idx] += 1 for every lane with pend set.  Called by whole waves (pend is
// false on lanes without a pixel).  Skewed data put most lanes of a wave on one
// word: PEEL times, the lanes that share the index of the wave's first pending
// lane leave together (readfirstlane + ballot; one lane adds the popcount);
// the remaining lanes use plain atomics.  T: uint32_t, or unsigned long long
// for counts that outgrow 32 bits.
template <int PEEL, typename T>
VU_DEV void hist_add(T* h, int idx, bool pend) {
#pragma unroll
  for (int r = 0; r < PEEL; ++r) {
    if (pend) {
      int first;
      unsigned long long mask;
      if (peel_same(idx, first, mask)) {
        if (peel_leader(mask)) atomicAdd(&h[first], (T)__popcll(mask));
        pend = false;
      }
    }
  }
  if (pend) atomicAdd(&h[idx], (T)1);
}

// h[idx] = max(h[idx], v) for every lane with pend set, the same way: the
// lanes of a peel round reduce their values over the wave first (lanes outside
// the round contribute 0) and one lane issues the atomic.  Called by whole,
// converged waves: the reduction shuffles across all 64 lanes.
template <int PEEL>
VU_DEV void hist_max(uint32_t* h, int idx, uint32_t v, bool pend) {
#pragma unroll
  for (int r = 0; r < PEEL; ++r) {
    const unsigned long long any = __ballot(pend);
    if (any == 0) return;   // wave-uniform
    const int lead = __ffsll((long long)any) - 1;
    const int first = __shfl(idx, lead, 64);
    const bool same = pend && idx == first;
    uint32_t m = same ? v : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    if ((int)(threadIdx.x & 63) == lead) atomicMax(&h[first], m);
    pend = pend && !same;
  }
  if (pend) atomicMax(&h[idx], v);
}
