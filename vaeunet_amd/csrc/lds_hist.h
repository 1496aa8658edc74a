// LDS histogram increment with per-wave aggregation of equal bins (calib.hip,
// filters.hip).
#pragma once
#include "common.h"

// h[idx] += 1 for every lane with pend set.  Called by whole waves (pend is
// false on lanes without a pixel).  Skewed data put most lanes of a wave on one
// word: PEEL times, the lanes that share the index of the wave's first pending
// lane leave together (readfirstlane + ballot; one lane adds the popcount);
// the remaining lanes use plain LDS atomics.
template <int PEEL>
VU_DEV void hist_add(uint32_t* h, int idx, bool pend) {
#pragma unroll
  for (int r = 0; r < PEEL; ++r) {
    if (pend) {
      const int first = __builtin_amdgcn_readfirstlane(idx);
      const bool same = idx == first;
      const unsigned long long mask = __ballot(same);
      if (same) {
        if ((int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(&h[first], (uint32_t)__popcll(mask));
        pend = false;
      }
    }
  }
  if (pend) atomicAdd(&h[idx], 1u);
}
