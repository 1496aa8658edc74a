// AttentionGate backward tail (unet_parts.py:7-30), bf16: everything after the
// psi backward's reductions in ONE stream over the pixels --
//
//   ds  = (s > 0) ? dq * wpsi : 0               (psi_bwd_u_kernel's stored ds)
//   dug = BN_g backward apply(ds, ug)            (bn_bwd_apply2_kernel)
//   dux = BN_x backward apply(ds, ux)
//   dg (=|+=) dug W_g                            (gemm_stream_kernel, dgrad)
//   dx  = bf16(dout * psi) + dux W_x             (gate_bwd_u_kernel + dgrad)
//
// -- bit for bit what those four kernels store.  It is gemm_stream_kernel's
// body (persistent blocks, both permuted weight images resident in LDS, a
// wave streams its own 16*NF-pixel tiles with the next tile's loads in
// flight, permlane-regrouped 64-byte stores) whose A operands are formed in
// registers: a lane of the MFMA B fragment holds 8 channels of one pixel,
// which is the layout the BatchNorm apply works in.  ds and the first dx are
// never in memory, dug / dux are written once (the weight-gradient GEMMs read
// them) and not read back.  The 13 per-channel coefficient vectors live in
// LDS next to the weights (13 F floats do not fit the register file at
// F >= 64); the two GEMMs of a tile run one after the other, so one
// accumulator set is live.
#include <type_traits>

#include "host.h"
#include "wave.h"
#include "attn_pre.h"

namespace {

enum { Q_SG, Q_TG, Q_SX, Q_TX, Q_WP, Q_MG, Q_AG, Q_BG, Q_EG, Q_MX, Q_AX, Q_BX, Q_EX, NQ };

struct AttnTail {
  const bf16_t *ug, *ux;   // [P][F]
  const float *dq, *pmap;  // [P]
  const float* coef[NQ];   // [F] each
  const bf16_t *wg, *wx;   // dgrad images [C][ld]
  int64_t ldg, ldx;
  const bf16_t* dout;      // [P][dos]
  int64_t dos;
  bf16_t* dg;              // channel offset applied
  int64_t dgs;
  int dg_acc;
  bf16_t* dx;
  int64_t dxs;
  bf16_t *dug, *dux;       // [P][F]
  int64_t P;
};

// KS: k-steps of 32 (F = 32*KS); NJ: 16-column fragments (C = 16*NJ, a
// multiple of 64); NF: 16-pixel fragments per wave tile; NW: waves per block
template <int KS, int NJ, int NF, int NW>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void attn_tail_kernel(AttnTail p) {
  constexpr int K = 32 * KS, N = 16 * NJ, PX = 16 * NF, NT = 64 * NW;
  constexpr int GS = 4;
  static_assert(NJ % GS == 0, "whole 64-column groups");
  __shared__ __attribute__((aligned(16))) char wsm[2][N * K * 2];
  __shared__ __attribute__((aligned(16))) float csm[NQ][K];

  const int ntiles = (int)(p.P / PX);
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gq = lane >> 4, r16 = lane & 15;

  // both weight images -> LDS in gemm_stream_kernel's fragment order
  auto wrow = [&](int j, int r) { return (j / GS) * 16 * GS + 4 * GS * (r >> 2) + 4 * (j % GS) + (r & 3); };
  {
    constexpr int PIECES = NJ * KS * 64;
#pragma unroll
    for (int img = 0; img < 2; ++img) {
      const bf16_t* bmat = img ? p.wx : p.wg;
      const int64_t ld = img ? p.ldx : p.ldg;
      for (int e = threadIdx.x; e < PIECES; e += NT) {
        const int l = e & 63, jk = e >> 6, j = jk / KS, ks = jk - j * KS;
        *reinterpret_cast<u32x4*>(wsm[img] + e * 16) =
            *reinterpret_cast<const u32x4*>(bmat + (int64_t)wrow(j, l & 15) * ld + 32 * ks + 8 * (l >> 4));
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      for (int c = threadIdx.x; c < K; c += NT) csm[q][c] = p.coef[q][c];
    __syncthreads();
  }

  const int tstride = gridDim.x * NW;
  // Addresses are (uniform 64-bit tile base) + (32-bit lane offset) + constant.
  // The tile number is opaque to the optimiser: the seven streams' accesses
  // otherwise become loop-carried 64-bit lane pointers (12-14 VGPRs more per
  // instantiation, and a spill at F = 128, C = 256).
  auto tile_px = [&](int t) {
    asm volatile("" : "+s"(t));
    return (int64_t)t * PX;
  };
  // (the lane offsets too: base + lane offset is otherwise hoisted as one
  // 64-bit lane pointer per stream)
  auto opq = [](uint32_t v) {
    asm volatile("" : "+v"(v));
    return v;
  };
  const uint32_t lk0 = (uint32_t)(r16 * K + 8 * gq);   // lane's element of a [P][K] tile
  auto load = [&](int t, u32x4 (&a)[NF][KS], u32x4 (&b)[NF][KS], float (&g)[NF], float (&pv)[NF]) {
    const int64_t pb = tile_px(t);
    const uint32_t lk = opq(lk0), lr = opq((uint32_t)r16);
    const bf16_t *ugb = p.ug + pb * K + lk, *uxb = p.ux + pb * K + lk;
    const float *dqb = p.dq + pb + lr, *pmb = p.pmap + pb + lr;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      g[f] = dqb[16 * f];
      pv[f] = pmb[16 * f];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        a[f][ks] = *reinterpret_cast<const u32x4*>(ugb + 16 * f * K + 32 * ks);
        b[f][ks] = *reinterpret_cast<const u32x4*>(uxb + 16 * f * K + 32 * ks);
      }
    }
  };
  u32x4 na[NF][KS], nb[NF][KS];
  float ng[NF], npv[NF];
  int tile = blockIdx.x * NW + wid;
  if (tile < ntiles) load(tile, na, nb, ng, npv);
  for (; tile < ntiles; tile += tstride) {
    const int64_t pb = tile_px(tile);
    // opaque LDS offset: weight fragments and coefficients are re-read per
    // tile instead of being hoisted out of the tile loop (gemm_stream_kernel)
    int lo = 0;
    asm volatile("" : "+v"(lo));
    auto coef8 = [&](int q, int ks, float (&d)[8]) {
      const char* s = reinterpret_cast<const char*>(&csm[q][32 * ks + 8 * gq]) + lo;
      const f32x4 u = *reinterpret_cast<const f32x4*>(s), v = *reinterpret_cast<const f32x4*>(s + 16);
#pragma unroll
      for (int k = 0; k < 4; ++k) { d[k] = u[k]; d[4 + k] = v[k]; }
    };
    // ---- ds, dug, dux in the A-operand layout ------------------------------
    u32x4 ag[NF][KS], ax[NF][KS];
    float pv[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) pv[f] = npv[f];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      Vec8<bf16_t> va[NF], vb[NF];
      float dsv[NF][8];   // the stored (bf16-rounded) ds values
      {
        float wsg[8], wtg[8], wsx[8], wtx[8], wp[8];
        coef8(Q_SG, ks, wsg); coef8(Q_TG, ks, wtg); coef8(Q_SX, ks, wsx); coef8(Q_TX, ks, wtx); coef8(Q_WP, ks, wp);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          va[f].v = na[f][ks];
          vb[f].v = nb[f][ks];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            float s = attn_pre(va[f].get(k), wsg[k], wtg[k], vb[f].get(k), wsx[k], wtx[k]);
            bool on = s > 0.f;
            // the product is rounded before the select (tied: a select, not a
            // divergent branch around the conversion, which split the tile
            // body into 8 * NF scheduling regions per k-step)
            float gw = rnd<bf16_t>(ng[f] * wp[k]);
            asm volatile("" : "+v"(gw));
            dsv[f][k] = on ? gw : 0.f;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        float mu[8], a[8], b[8], e[8];
        coef8(side ? Q_MX : Q_MG, ks, mu); coef8(side ? Q_AX : Q_AG, ks, a);
        coef8(side ? Q_BX : Q_BG, ks, b); coef8(side ? Q_EX : Q_EG, ks, e);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const Vec8<bf16_t>& vx = side ? vb[f] : va[f];
          Vec8<bf16_t> o;
          o.zero();
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float dz = dsv[f][k];
            o.set(k, fmaf(a[k], dz, b[k] * (vx.get(k) - mu[k])) + e[k]);
          }
          // (tied: the arithmetic is done here, not sunk to the MFMAs)
          asm volatile("" : "+v"(o.v));
          (side ? ax : ag)[f][ks] = o.v;
        }
        // one coefficient set live at a time: otherwise every k-step's LDS
        // reads are issued first and the arithmetic sinks to its use
        // (13 * 8 * KS registers of coefficients live at once, spills)
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // the next tile's loads are in flight over this tile's MFMAs and stores
    if (tile + tstride < ntiles) load(tile + tstride, na, nb, ng, npv);
    {
      const uint32_t lk = opq(lk0);
      bf16_t *dugb = p.dug + pb * K + lk, *duxb = p.dux + pb * K + lk;
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          *reinterpret_cast<u32x4*>(dugb + 16 * f * K + 32 * ks) = ag[f][ks];
          *reinterpret_cast<u32x4*>(duxb + 16 * f * K + 32 * ks) = ax[f][ks];
        }
    }

    auto add_old = [&](u32x4& v, const u32x4 o) {
#pragma unroll
      for (int w = 0; w < 4; ++w)
        v[w] = pack2(lo_f(o[w]) + lo_f(v[w]), hi_f(o[w]) + hi_f(v[w]));
    };
    // one dgrad GEMM and its epilogue: gemm_stream_kernel's MFMA order and
    // GS = 4 store pass.  OLD 0: plain store; 1: the destination's old value
    // is added (accumulate); 2: bf16(dout * psi), formed here, is added
    auto gemm = [&](const char* wimg, const u32x4 (&pf)[NF][KS], bf16_t* out, int64_t os, auto old_tag) {
      constexpr int OLD = decltype(old_tag)::value;
      f32x4 acc[NF][NJ];
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[f][j] = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const u32x4 wf = *reinterpret_cast<const u32x4*>(wimg + lo + ((j * KS + ks) * 64 + lane) * 16);
#pragma unroll
          for (int f = 0; f < NF; ++f)
            acc[f][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf),
                                                                __builtin_bit_cast(bf16x8, pf[f][ks]), acc[f][j], 0, 0, 0);
          // F = 128, C = 256: at most 8 weight fragments read ahead (16 of
          // them put two operand sets of the other GEMM in scratch)
          if constexpr (KS * NJ >= 64)
            if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
      // acc[f][j][r]: pixel pb + 16f + r16, column (j/GS)*64 + 16*gq + 4*(j%GS) + r
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        // row 16f + r16 of the tile, columns 8gq .. +7 (strides < 2^20: _ok)
        const uint32_t row = (uint32_t)(16 * f + r16);
        bf16_t* outp = out + pb * os + opq(row * (uint32_t)os + 8 * gq);
        const bf16_t* dop = p.dout + pb * p.dos + opq(row * (uint32_t)p.dos + 8 * gq);
        // (two 64-column groups at a time: the packed results and the old
        // values of all four groups of C = 256 did not fit next to the
        // accumulators and the prefetched tile)
        constexpr int GC = NJ / GS < 2 ? NJ / GS : 2;
#pragma unroll
        for (int g0 = 0; g0 < NJ / GS; g0 += GC) {
          u32x4 c[GC][2];
#pragma unroll
          for (int gi = 0; gi < GC; ++gi) {
            const int grp = g0 + gi;
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
              // (+ 0.f: the stream kernel's bias add with no bias)
              const f32x4 a = acc[f][grp * 4 + 2 * h2] + 0.f, b = acc[f][grp * 4 + 2 * h2 + 1] + 0.f;
              c[gi][h2] = u32x4{pack2(a[0], a[1]), pack2(a[2], a[3]), pack2(b[0], b[1]), pack2(b[2], b[3])};
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const auto r1 = __builtin_amdgcn_permlane16_swap(c[gi][0][w], c[gi][1][w], false, false);
              const auto r2 = __builtin_amdgcn_permlane32_swap(r1[0], r1[1], false, false);
              c[gi][0][w] = r2[0];
              c[gi][1][w] = r2[1];
            }
          }
          // lane row gq now holds columns grp*64 + 32h + 8gq .. +7 of its pixel
          if constexpr (OLD != 0) {
            u32x4 o[GC][2];
#pragma unroll
            for (int gi = 0; gi < GC; ++gi)
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                const int col = (g0 + gi) * 64 + 32 * h;
                if constexpr (OLD == 1) o[gi][h] = *reinterpret_cast<const u32x4*>(outp + col);
                else o[gi][h] = *reinterpret_cast<const u32x4*>(dop + col);
              }
#pragma unroll
            for (int gi = 0; gi < GC; ++gi)
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                if constexpr (OLD == 2) {
                  // gate_bwd_u_kernel's dx = dout * psi, rounded to bf16
#pragma unroll
                  for (int w = 0; w < 4; ++w)
                    o[gi][h][w] = pack2(lo_f(o[gi][h][w]) * pv[f], hi_f(o[gi][h][w]) * pv[f]);
                }
                add_old(c[gi][h], o[gi][h]);
              }
          }
#pragma unroll
          for (int gi = 0; gi < GC; ++gi)
#pragma unroll
            for (int h = 0; h < 2; ++h)
              *reinterpret_cast<u32x4*>(outp + (g0 + gi) * 64 + 32 * h) = c[gi][h];
        }
      }
    };
    if (p.dg_acc) gemm(wsm[0], ag, p.dg, p.dgs, std::integral_constant<int, 1>{});
    else gemm(wsm[0], ag, p.dg, p.dgs, std::integral_constant<int, 0>{});
    gemm(wsm[1], ax, p.dx, p.dxs, std::integral_constant<int, 2>{});
  }
}

// pixel fragments per wave tile: NF*NJ <= 16 accumulator fragments as in
// gemm_stream.hip, but NF*KS <= 4: there are four operand register sets per
// fragment here (ug, ux of the next tile, dug, dux of this one), not two
constexpr int nf_of(int ks, int nj) {
  return (16 / nj < 4 ? 16 / nj : 4) < (4 / ks) ? (16 / nj < 4 ? 16 / nj : 4) : 4 / ks;
}
// both weight images above half the LDS: one 8-wave block per CU instead of
// two 4-wave blocks
constexpr int nw_of(int ks, int nj) { return 2 * (16 * nj) * (32 * ks) * 2 > 72 * 1024 ? 8 : 4; }

template <int KS, int NJ>
int launch_nj(const AttnTail& p, hipStream_t st) {
  constexpr int NF = nf_of(KS, NJ), NW = nw_of(KS, NJ);
  const int64_t tiles = p.P / (16 * NF);
  int64_t nblk = (tiles + NW - 1) / NW;
  const int64_t cap = (NW == 4 ? 2 : 1) * (int64_t)cu_count();
  if (nblk > cap) nblk = cap;
  if (nblk == 0) return 0;
  hipLaunchKernelGGL((attn_tail_kernel<KS, NJ, NF, NW>), dim3((unsigned)nblk), dim3(64 * NW), 0, st, p);
  return (int)hipGetLastError();
}

template <int KS>
int launch_ks(const AttnTail& p, int C, hipStream_t st) {
  switch (C / 16) {
    case 4: return launch_nj<KS, 4>(p, st);
    case 8: return launch_nj<KS, 8>(p, st);
    case 16: return launch_nj<KS, 16>(p, st);
    default: return (int)hipErrorInvalidValue;
  }
}

}  // namespace

extern "C" int64_t vu_attn_tail_bwd_tile(int F, int C) {
  if ((F != 32 && F != 64 && F != 128) || (C != 64 && C != 128 && C != 256)) return 0;
  return 16 * nf_of(F / 32, C / 16);
}

extern "C" int vu_attn_tail_bwd_ok(int64_t P, int F, int C, int64_t ldg, int64_t ldx, int64_t dos, int64_t dgs,
                                   int64_t dg_coff, int64_t dxs, int dtype) {
  if (dtype != VU_BF16) return 0;
  const int64_t px = vu_attn_tail_bwd_tile(F, C);
  if (px == 0) return 0;
  if (ldg % 8 != 0 || ldg < F || ldx % 8 != 0 || ldx < F) return 0;
  if (dos % 8 != 0 || dos < C || dgs % 8 != 0 || dg_coff % 8 != 0 || dg_coff < 0 || dgs < dg_coff + C || dxs % 8 != 0 ||
      dxs < C)
    return 0;
  if (dos >= (1 << 20) || dgs >= (1 << 20) || dxs >= (1 << 20)) return 0;   // 32-bit in-tile offsets
  if (P <= 0 || P % px != 0 || P >= ((int64_t)1 << 31)) return 0;
  return 1;
}

extern "C" int vu_attn_tail_bwd(const void* ug, const void* ux, const float* dq, int64_t P, int F, int C,
                                const float* sg, const float* tg, const float* sx, const float* tx,
                                const float* wpsi, const float* mean_g, const float* coef_g, const float* mean_x,
                                const float* coef_x, const void* wdg, int64_t ldg, const void* wdx, int64_t ldx,
                                const void* dout, int64_t dos, const float* pmap, void* dg, int64_t dgs,
                                int64_t dg_coff, int dg_acc, void* dx, int64_t dxs, void* dug, void* dux, int dtype,
                                void* stream) {
  if (!vu_attn_tail_bwd_ok(P, F, C, ldg, ldx, dos, dgs, dg_coff, dxs, dtype)) return (int)hipErrorInvalidValue;
  if (!ug || !ux || !dq || !sg || !tg || !sx || !tx || !wpsi || !mean_g || !coef_g || !mean_x || !coef_x || !wdg ||
      !wdx || !dout || !pmap || !dg || !dx || !dug || !dux)
    return (int)hipErrorInvalidValue;
  AttnTail p;
  p.ug = (const bf16_t*)ug; p.ux = (const bf16_t*)ux; p.dq = dq; p.pmap = pmap;
  p.coef[Q_SG] = sg; p.coef[Q_TG] = tg; p.coef[Q_SX] = sx; p.coef[Q_TX] = tx; p.coef[Q_WP] = wpsi;
  p.coef[Q_MG] = mean_g; p.coef[Q_AG] = coef_g; p.coef[Q_BG] = coef_g + F; p.coef[Q_EG] = coef_g + 2 * F;
  p.coef[Q_MX] = mean_x; p.coef[Q_AX] = coef_x; p.coef[Q_BX] = coef_x + F; p.coef[Q_EX] = coef_x + 2 * F;
  p.wg = (const bf16_t*)wdg; p.wx = (const bf16_t*)wdx; p.ldg = ldg; p.ldx = ldx;
  p.dout = (const bf16_t*)dout; p.dos = dos;
  p.dg = (bf16_t*)dg + dg_coff; p.dgs = dgs; p.dg_acc = dg_acc;
  p.dx = (bf16_t*)dx; p.dxs = dxs;
  p.dug = (bf16_t*)dug; p.dux = (bf16_t*)dux;
  p.P = P;
  hipStream_t st = (hipStream_t)stream;
  switch (F) {
    case 32: return launch_ks<1>(p, C, st);
    case 64: return launch_ks<2>(p, C, st);
    case 128: return launch_ks<4>(p, C, st);
    default: return (int)hipErrorInvalidValue;
  }
}
