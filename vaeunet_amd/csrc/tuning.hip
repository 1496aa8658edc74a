// The dispatcher tuning keys (vu_gemm_set_tuning; tests and A/B runs only --
// the library reads no environment variables): one row per live key with its
// default and the rule a set value passes through.  Host code only; readers
// call tune(VU_TUNE_...) (host.h).  include/vaeunet.h documents the meanings.
#include "host.h"

namespace {

enum Rule {
  RAW,     // any value, stored as given
  FLAG,    // any value, stored as value != 0
  NONNEG,  // any value, negative ones stored as 0
  RANGE,   // lo <= value <= hi, else refused
};

struct Key {
  int key, def;
  Rule rule;
  int lo, hi;  // RANGE only
  int xm_bit;  // experiment mode: bit of vu_gemm_experiment_modes(), non-zero values need VU_TUNE_UNSAFE
};

constexpr Key kKeys[] = {
    {VU_TUNE_V4_MIN_BLOCKS, 256, RAW},
    {VU_TUNE_FP8_GRID, 0, RAW},
    {VU_TUNE_STREAM, 1, FLAG},
    {VU_TUNE_V4_SPLITK, 1, RAW},
    {VU_TUNE_V4_SPLIT_CHUNKS, 2, RAW},
    {VU_TUNE_V2_SMALL, 1, FLAG},
    {VU_TUNE_V5, 1, NONNEG},
    {VU_TUNE_V6, 1, NONNEG},
    {VU_TUNE_GEN, 4, RANGE, 1, 4},
    {VU_TUNE_SLAB4, 1, RAW},
    {VU_TUNE_BN_NT_MB, 32, RAW},
    {VU_TUNE_V7, 1, RANGE, 0, 2},
    {VU_TUNE_V7_NBW, 3, RANGE, 3, 4},
    {VU_TUNE_V7_XM, 0, RAW, 0, 0, 2},
    {VU_TUNE_W3_SMALL, 1, FLAG},
    {VU_TUNE_FP8_XM, 0, RAW, 0, 0, 4},
    {VU_TUNE_FP8_PP, 1, FLAG},
    {VU_TUNE_ATTN, 1, RANGE, 0, 1},
    {VU_TUNE_FP8_C64, 2, NONNEG},
    {VU_TUNE_FP8_SPLIT, 1, FLAG},
    {VU_TUNE_BN_MINBLK, 256, NONNEG},
    {VU_TUNE_PP_FULL, 1, RAW},
    {VU_TUNE_W2_BIG, 0, RAW},
    {VU_TUNE_V6_XM, 0, RANGE, 0, 5, 1},
    {VU_TUNE_UNSAFE, 0, FLAG},
    {VU_TUNE_V6_STAG, 1, FLAG},
};

int g_xm_modes = 0;  // vu_gemm_experiment_modes()

constexpr VuTuneValues defaults() {
  VuTuneValues r{};
  for (const Key& k : kKeys) r.v[k.key] = k.def;
  return r;
}

}  // namespace

VuTuneValues vu_tune_values = defaults();

// Experiment modes (timing decompositions, several with wrong results by
// design) are refused unless VU_TUNE_UNSAFE was set first, and
// tracked so that a benchmark can refuse to report while one is active.
// Retired and unknown keys have no row and are refused.
extern "C" int vu_gemm_set_tuning(int key, int value) {
  for (const Key& k : kKeys) {
    if (k.key != key) continue;
    if (k.xm_bit && value != 0 && !tune(VU_TUNE_UNSAFE)) return (int)hipErrorInvalidValue;
    if (k.rule == RANGE && (value < k.lo || value > k.hi)) return (int)hipErrorInvalidValue;
    vu_tune_values.v[key] = k.rule == FLAG ? value != 0 : (k.rule == NONNEG && value < 0 ? 0 : value);
    if (k.xm_bit) g_xm_modes = value != 0 ? (g_xm_modes | k.xm_bit) : (g_xm_modes & ~k.xm_bit);
    return 0;
  }
  return (int)hipErrorInvalidValue;
}

extern "C" int vu_gemm_experiment_modes(void) { return g_xm_modes; }
