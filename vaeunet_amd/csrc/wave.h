// Wave- and LDS-level primitives of the MFMA kernels (gfx950 / CDNA4 only):
// DPP lane moves and row sums, bf16 packing, the LDS address-space types,
// counted waits and the scheduling-fenced barrier, the LDS-DMA call with its
// zero page, the LDS swizzles and the ping-pong tile-shape table.  Every
// helper is a single definition: a kernel file includes this header next to
// host.h and takes its primitives from here instead of declaring its own.
#pragma once
#include "common.h"

// ---- DPP helpers -------------------------------------------------------------
// sum over the 16 lanes of a DPP row (every lane receives the total)
template <int R>
VU_DEV float ror_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + R, 0xf, 0xf, false));
}
VU_DEV float row16_sum(float v) { return ror_add<1>(ror_add<2>(ror_add<4>(ror_add<8>(v)))); }

// (sum, M2 about the tile mean) of one column over a tile of 16 * NF rows: the
// lane's NF values acc[f][j][r] and the 16 lanes of its DPP row (every lane
// receives both); the BatchNorm partial statistics of the register epilogues
template <int NF, int NJ>
VU_DEV void tile_sum_m2(const f32x4 (&acc)[NF][NJ], int j, int r, float& sum, float& m2) {
  float sv = 0.f;
#pragma unroll
  for (int f = 0; f < NF; ++f) sv += acc[f][j][r];
  sv = row16_sum(sv);
  const float mean = sv * (1.f / (16 * NF));
  float v = 0.f;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const float d = acc[f][j][r] - mean;
    v += d * d;
  }
  sum = sv;
  m2 = row16_sum(v);
}

// lane-xor moves inside a DPP row (all VALU: no LDS crossbar)
template <int CTRL>
VU_DEV float dmov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
VU_DEV float lx1(float v) { return dmov<0xB1>(v); }               // lane ^ 1
VU_DEV float lx2(float v) { return dmov<0x4E>(v); }               // lane ^ 2
VU_DEV float lx4(float v) { return dmov<0x1B>(dmov<0x141>(v)); }  // lane ^ 4
VU_DEV float lx8(float v) { return dmov<0x128>(v); }              // lane ^ 8 (row_ror:8)

// ---- bf16 packing ------------------------------------------------------------
// two floats -> packed bf16 pair (a in the low half)
VU_DEV uint32_t pack2(float a, float b) { return (uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16); }

// the two bf16 halves of a packed pair as floats
VU_DEV float lo_f(uint32_t w) { return __uint_as_float(w << 16); }
VU_DEV float hi_f(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// ---- LDS address-space types -------------------------------------------------
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
// 32-bit LDS byte address of a pointer into __shared__ memory (inline-asm reads)
VU_DEV uint32_t lds_addr(const char* p) { return (uint32_t)(uintptr_t)(const lds_void*)p; }

// ---- counters and fences -----------------------------------------------------
// at most N vector-memory operations of this wave outstanding (loads AND
// stores: CDNA counts both in vmcnt, in issue order)
template <int N>
VU_DEV void wait_vm() {
  static_assert(N >= 0 && N <= 63, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// wait until at most N LDS reads are outstanding (the counter holds 0..15);
// the fragments read are tied to the wait with tie() so their consumers
// cannot be scheduled above it
template <int N> VU_DEV void lgkm_wait() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N > 15 ? 15 : N) : "memory");
}
VU_DEV void tie(u32x4& v) { asm volatile("" : "+v"(v)); }

// a workgroup barrier that neither drains the memory counters nor lets the
// compiler move LDS reads, DMA issues or MFMAs across it
VU_DEV void raw_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// ---- LDS-DMA -----------------------------------------------------------------
// 16 B of zeros (and slack): padding lanes of an LDS-DMA load from here.  The
// declaration is shared, the storage is not: each .hip is its own code object
// and device code cannot reference another object's variable, so the array is
// static and every file that uses it gets its own copy.
static __device__ __attribute__((aligned(16), unused)) uint32_t vu_zero_page[16];

// 16 bytes per lane, global -> LDS (global_load_lds_dwordx4): lane l of the
// wave lands at lds + 16 * l, lds being wave-uniform
VU_DEV void dma16(const void* g, char* lds) { __builtin_amdgcn_global_load_lds(g, (lds_void*)lds, 16, 0, 0); }

// ---- LDS swizzles ------------------------------------------------------------
// 128-byte K rows of 16-byte chunks, XOR-swizzled by the row's low three bits
// (conflict-free ds_read_b128 fragment reads)
VU_DEV int swz(int row, int chunk) {
  constexpr int KB = 128;  // bytes of K per LDS row per k-step
  return row * KB + ((chunk ^ (row & 7)) << 4);
}

// 32-byte block swizzle of the [m][col] images read with ds_read_b64_tr_b16: a
// 32-lane half of a transposed read touches 8 rows (4 consecutive + 4 rows 8
// apart), one 32-byte block each; f(m) spreads them over the 8 bank blocks of
// the 256-byte bank window.  Rows >= 256 B: all three row bits; 128-B rows (4
// blocks): pairs by parity; 64-B rows (2 blocks): the two row quads.
template <int RB> VU_DEV int fsw(int m) {
  return RB >= 256 ? ((m & 3) | ((m >> 1) & 4))
                   : RB == 128 ? (((m >> 1) & 1) | ((m >> 2) & 2)) : ((m >> 3) & 1);
}
// byte offset of bf16 column col of row m (rows of RB bytes)
template <int RB> VU_DEV int tr_off(int m, int col) {
  return m * RB + (((col >> 4) ^ fsw<RB>(m)) << 5) + ((col & 15) << 1);
}
// logical column of the 16-byte physical chunk pc of row m (source-side swizzle)
template <int RB> VU_DEV int swz_col(int m, int pc) {
  return ((((pc >> 1) ^ fsw<RB>(m)) << 1) | (pc & 1)) * 8;
}

// ---- tile shapes of the ping-pong 3x3 kernels --------------------------------
// BN output channels: waves WM x WN (128 pixels x 64 channels each), pixel
// tile TH x TW
template <int BN> struct PP;
template <> struct PP<256> { static constexpr int WM = 2, WN = 4, TH = 8, TW = 32; };
template <> struct PP<128> { static constexpr int WM = 4, WN = 2, TH = 16, TW = 32; };
template <> struct PP<64> { static constexpr int WM = 8, WN = 1, TH = 32, TW = 32; };
