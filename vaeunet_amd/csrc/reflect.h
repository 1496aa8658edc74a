// The reflect101 border rule shared by the patch-loader kernels (augment.hip,
// filters.hip).
#pragma once
#include "common.h"

// index folded with period 2 (size - 1): ... 2 1 | 0 1 2 ... n-1 | n-2 ...
VU_DEV int reflect101(int i, int size) {
  if ((unsigned)i < (unsigned)size) return i;
  if (size == 1) return 0;
  const int p = 2 * (size - 1);
  int m = i % p;
  if (m < 0) m += p;
  return m < size ? m : p - m;
}
