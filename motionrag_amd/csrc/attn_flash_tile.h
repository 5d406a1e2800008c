// attn_flash_tile.h -- the tile functions of the 32x32x16 flash family (attn_flash.hip: fixed-length launches; attn_varlen.hip: packed variable-length
// launches): the K . Q^T product, the online-softmax bookkeeping and the V^T . P^T product of one 64-key tile over the LDS ring both kernels stage by LDS-DMA.
// The design notes are at the head of attn_flash.hip.  Unnamed namespace: each unit gets its own copy, nothing here is a symbol of the library.
#pragma once
#include <type_traits>
#include "attn_common.h"

namespace {

constexpr float kThr = 5.0f;          // deferred-rescale threshold in log2 units (P <= 32)
constexpr int NS = 4;  // LDS ring stages per operand (DMA runs D = NS-1 tiles ahead); 2 x 64 KB fit two workgroups per CU
constexpr int V_BASE = NS * TILE_BYTES;  // LDS: K stages 0..NS-1, then V stages 0..NS-1

__device__ __forceinline__ bf16x8 scale_frag(u32x4 raw, float s) {
  u32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float lo = __uint_as_float(raw[i] << 16) * s;
    const float hi = __uint_as_float(raw[i] & 0xffff0000u) * s;
    r[i] = pack_bf2(lo, hi);
  }
  return __builtin_bit_cast(bf16x8, r);
}

__device__ __forceinline__ float half_swap_max(float v) {
  const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return max3_asm(__uint_as_float(sw[0]), __uint_as_float(sw[1]), __uint_as_float(sw[1]));
}

struct Lane {
  int hh, k_row_off, k_swz, v_lane_off, v_half0, v_half1, head;
  unsigned kb[4], vc0, vc1;   // loop-invariant LDS addresses of this lane's K fragment chunks / V^T reads in ring stage 0 (the stage itself is an instruction immediate: qk_tile_imm8 / pv_tile_imm)
};

struct NoHook {
  __device__ __forceinline__ void operator()() const {}
};

// S'^T = K . Q^T + C for the two 32-key blocks of one tile (8 MFMAs); C = -running max.
// All 8 K fragments are requested in one asm statement (hipcc otherwise serialises read -> wait -> MFMA pairs and
// exposes the LDS latency four times per tile); `between()` runs while they are in flight (the DMA issue of a later
// tile), then one wait statement that names every destination releases them to the MFMAs.
template <typename Between = NoHook>
__device__ __forceinline__ void qk_tile(const char* kst, const Lane& ln, const bf16x8 (&qf)[4], const f32x16& negm, f32x16& s0, f32x16& s1,
                                        Between between = Between()) {
  // register-lean form (4 waves per SIMD hide the LDS latency): one 32-key block at a time
  const unsigned base = (unsigned)(size_t)(kst + ln.k_row_off);
  const unsigned b0 = base + ((0 + ln.hh) ^ ln.k_swz) * 16, b1 = base + ((2 + ln.hh) ^ ln.k_swz) * 16;
  const unsigned b2 = base + ((4 + ln.hh) ^ ln.k_swz) * 16, b3 = base + ((6 + ln.hh) ^ ln.k_swz) * 16;
  u32x4 kf[4];
  asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %6\n\tds_read_b128 %3, %7"
               : "=&v"(kf[0]), "=&v"(kf[1]), "=&v"(kf[2]), "=&v"(kf[3]) : "v"(b0), "v"(b1), "v"(b2), "v"(b3) : "memory");
  between();
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(kf[0]), "+v"(kf[1]), "+v"(kf[2]), "+v"(kf[3]) :: "memory");
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // inline-constant C
  // The running max is subtracted BY THE MATRIX PIPE: one more k-step whose key fragment is the constant (-1, 0, ..., 0) and whose
  // query fragment is (m, 0, ..., 0) adds -m to every score of the lane's query.  The vector pipe is the saturated one here
  // (per tile 32 v_exp + 32 row-sum adds + 17 v_max3 + 16 cvt_pk against 16 MFMAs); this trades 32 v_add (128 issue cycles)
  // for 2 MFMAs (64 matrix cycles, 16 issue cycles).  m is kept bf16-representable so the product is exact (softmax_tile).
  const u32x4 kneg = {ln.hh == 0 ? 0x0000bf80u : 0u, 0u, 0u, 0u};
  const u32x4 qm = {__float_as_uint(negm[1]), 0u, 0u, 0u};
  s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf[0]), qf[0], zero, 0, 0, 0);
#pragma unroll
  for (int ks = 1; ks < 4; ++ks) s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf[ks]), qf[ks], s0, 0, 0, 0);
  asm volatile("ds_read_b128 %0, %4 offset:4096\n\tds_read_b128 %1, %5 offset:4096\n\tds_read_b128 %2, %6 offset:4096\n\tds_read_b128 %3, %7 offset:4096\n\t"
               "s_waitcnt lgkmcnt(0)"
               : "=&v"(kf[0]), "=&v"(kf[1]), "=&v"(kf[2]), "=&v"(kf[3]) : "v"(b0), "v"(b1), "v"(b2), "v"(b3) : "memory");
  s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf[0]), qf[0], zero, 0, 0, 0);
#pragma unroll
  for (int ks = 1; ks < 4; ++ks) s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf[ks]), qf[ks], s1, 0, 0, 0);
  s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kneg), __builtin_bit_cast(bf16x8, qm), s0, 0, 0, 0);
  s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kneg), __builtin_bit_cast(bf16x8, qm), s1, 0, 0, 0);
}

// O^T += V^T . P^T (8 MFMAs).  The 16 transposed reads go through ONE asm statement: hipcc cannot see that the
// ds_read_tr16 builtin does not alias the in-flight LDS-DMA of later tiles and would drain it (s_waitcnt vmcnt(0))
// in the middle of the tile.  EXEC is all ones here (wave-uniform control flow only).
__device__ __forceinline__ void pv_tile(const char* vst, const Lane& ln, const bf16x8 (&pb)[4], f32x16& o0, f32x16& o1) {
  {
    const unsigned c0 = (unsigned)(size_t)(vst + ln.v_lane_off + ln.v_half0), c1 = (unsigned)(size_t)(vst + ln.v_lane_off + ln.v_half1);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      u32x2 u0[4], u1[4];
      const unsigned d0 = c0 + half * 4096, d1 = c1 + half * 4096;
      asm volatile("ds_read_b64_tr_b16 %0, %8 offset:0\n\tds_read_b64_tr_b16 %1, %8 offset:1024\n\t"
                   "ds_read_b64_tr_b16 %4, %9 offset:0\n\tds_read_b64_tr_b16 %5, %9 offset:1024\n\t"
                   "ds_read_b64_tr_b16 %2, %8 offset:2048\n\tds_read_b64_tr_b16 %3, %8 offset:3072\n\t"
                   "ds_read_b64_tr_b16 %6, %9 offset:2048\n\tds_read_b64_tr_b16 %7, %9 offset:3072\n\t"
                   "s_waitcnt lgkmcnt(0)"
                   : "=&v"(u0[0]), "=&v"(u0[1]), "=&v"(u0[2]), "=&v"(u0[3]), "=&v"(u1[0]), "=&v"(u1[1]), "=&v"(u1[2]), "=&v"(u1[3])
                   : "v"(d0), "v"(d1) : "memory");
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        const u32x4 w0 = {u0[2 * k2][0], u0[2 * k2][1], u0[2 * k2 + 1][0], u0[2 * k2 + 1][1]};
        const u32x4 w1 = {u1[2 * k2][0], u1[2 * k2][1], u1[2 * k2 + 1][0], u1[2 * k2 + 1][1]};
        o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w0), pb[2 * half + k2], o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w1), pb[2 * half + k2], o1, 0, 0, 0);
      }
    }
  }
}

// The ring stage as an INSTRUCTION IMMEDIATE (ds_read offset field) instead of per-tile address arithmetic: the main loop is unrolled by
// NS, so `t % NS` is a compile-time constant, the lane's base addresses are loop-invariant registers, and ~11 integer vector instructions
// per tile (of ~144) disappear from a loop whose vector pipe is ~77 % busy.
template <int STG>
__device__ __forceinline__ void pv_tile_imm(const Lane& ln, const bf16x8 (&pb)[4], f32x16& o0, f32x16& o1) {
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    u32x2 u0[4], u1[4];
    if (half == 0) {
      asm volatile("ds_read_b64_tr_b16 %0, %8 offset:%10\n\tds_read_b64_tr_b16 %1, %8 offset:%11\n\t"
                   "ds_read_b64_tr_b16 %4, %9 offset:%10\n\tds_read_b64_tr_b16 %5, %9 offset:%11\n\t"
                   "ds_read_b64_tr_b16 %2, %8 offset:%12\n\tds_read_b64_tr_b16 %3, %8 offset:%13\n\t"
                   "ds_read_b64_tr_b16 %6, %9 offset:%12\n\tds_read_b64_tr_b16 %7, %9 offset:%13\n\t"
                   "s_waitcnt lgkmcnt(0)"
                   : "=&v"(u0[0]), "=&v"(u0[1]), "=&v"(u0[2]), "=&v"(u0[3]), "=&v"(u1[0]), "=&v"(u1[1]), "=&v"(u1[2]), "=&v"(u1[3])
                   : "v"(ln.vc0), "v"(ln.vc1), "n"(STG * TILE_BYTES), "n"(STG * TILE_BYTES + 1024), "n"(STG * TILE_BYTES + 2048), "n"(STG * TILE_BYTES + 3072) : "memory");
    } else {
      asm volatile("ds_read_b64_tr_b16 %0, %8 offset:%10\n\tds_read_b64_tr_b16 %1, %8 offset:%11\n\t"
                   "ds_read_b64_tr_b16 %4, %9 offset:%10\n\tds_read_b64_tr_b16 %5, %9 offset:%11\n\t"
                   "ds_read_b64_tr_b16 %2, %8 offset:%12\n\tds_read_b64_tr_b16 %3, %8 offset:%13\n\t"
                   "ds_read_b64_tr_b16 %6, %9 offset:%12\n\tds_read_b64_tr_b16 %7, %9 offset:%13\n\t"
                   "s_waitcnt lgkmcnt(0)"
                   : "=&v"(u0[0]), "=&v"(u0[1]), "=&v"(u0[2]), "=&v"(u0[3]), "=&v"(u1[0]), "=&v"(u1[1]), "=&v"(u1[2]), "=&v"(u1[3])
                   : "v"(ln.vc0), "v"(ln.vc1), "n"(STG * TILE_BYTES + 4096), "n"(STG * TILE_BYTES + 5120), "n"(STG * TILE_BYTES + 6144), "n"(STG * TILE_BYTES + 7168) : "memory");
    }
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      const u32x4 w0 = {u0[2 * k2][0], u0[2 * k2][1], u0[2 * k2 + 1][0], u0[2 * k2 + 1][1]};
      const u32x4 w1 = {u1[2 * k2][0], u1[2 * k2][1], u1[2 * k2 + 1][0], u1[2 * k2 + 1][1]};
      o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w0), pb[2 * half + k2], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w1), pb[2 * half + k2], o1, 0, 0, 0);
    }
  }
}

// Both 32-key blocks' K fragments requested UP FRONT (8 reads in flight, released to the MFMAs by counted lgkmcnt waits --
// LDS reads return in order): the second block's LDS latency hides under the first block's MFMAs instead of being paid behind them.  The LDS
// pipe is only ~25 % busy in this loop (256 B/clk per CU, tools/exp/lds_rate.hip; SQ_LDS_IDX_ACTIVE), so what the reads cost is their latency.
template <int STG, typename Between = NoHook>
__device__ __forceinline__ void qk_tile_imm8(const Lane& ln, const bf16x8 (&qf)[4], const f32x16& negm, f32x16& s0, f32x16& s1, Between between = Between()) {
  u32x4 k0[4], k1[4];
  asm volatile("ds_read_b128 %0, %8 offset:%12\n\tds_read_b128 %1, %9 offset:%12\n\tds_read_b128 %2, %10 offset:%12\n\tds_read_b128 %3, %11 offset:%12\n\t"
               "ds_read_b128 %4, %8 offset:%13\n\tds_read_b128 %5, %9 offset:%13\n\tds_read_b128 %6, %10 offset:%13\n\tds_read_b128 %7, %11 offset:%13"
               : "=&v"(k0[0]), "=&v"(k0[1]), "=&v"(k0[2]), "=&v"(k0[3]), "=&v"(k1[0]), "=&v"(k1[1]), "=&v"(k1[2]), "=&v"(k1[3])
               : "v"(ln.kb[0]), "v"(ln.kb[1]), "v"(ln.kb[2]), "v"(ln.kb[3]), "n"(STG * TILE_BYTES), "n"(STG * TILE_BYTES + 4096) : "memory");
  between();
  asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(k0[0]), "+v"(k0[1]), "+v"(k0[2]), "+v"(k0[3]) :: "memory");
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const u32x4 kneg = {ln.hh == 0 ? 0x0000bf80u : 0u, 0u, 0u, 0u};
  const u32x4 qm = {__float_as_uint(negm[1]), 0u, 0u, 0u};
  s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, k0[0]), qf[0], zero, 0, 0, 0);
#pragma unroll
  for (int ks = 1; ks < 4; ++ks) s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, k0[ks]), qf[ks], s0, 0, 0, 0);
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(k1[0]), "+v"(k1[1]), "+v"(k1[2]), "+v"(k1[3]) :: "memory");
  s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, k1[0]), qf[0], zero, 0, 0, 0);
#pragma unroll
  for (int ks = 1; ks < 4; ++ks) s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, k1[ks]), qf[ks], s1, 0, 0, 0);
  s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kneg), __builtin_bit_cast(bf16x8, qm), s0, 0, 0, 0);
  s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kneg), __builtin_bit_cast(bf16x8, qm), s1, 0, 0, 0);
}

struct Run {
  f32x16 o0, o1, negm;
  f32x16 lacc;   // row sum: element 0 holds the lane's half of l of its query, accumulated by v_dot2c over the bf16 P pairs (softmax_tile)
  float m;
};

// softmax bookkeeping of one tile: masks, tile max, deferred rescale, P = exp2(S'), row sum, bf16 B fragments.
// register i of block kb holds key t*64 + kb*32 + (i&3) + 8*(i>>2) + 4*hh for query (lane & 31).
template <bool HAS_MASK>
__device__ __forceinline__ void softmax_tile(const AttnP& p, const int skv, const Lane& ln, int t, int nt, int qrow_c, f32x16& s0, f32x16& s1,
                                             Run& r, bf16x8 (&pb)[4]) {
  // skv = keys this workgroup scans (p.Skv, or its chunk of them in the key-split tail; the mask path is never split)
  // key held by register i of block kb: tile_start + kb*32 + (i&3) + 8*(i>>2) + 4*hh; the last tile of a long sequence starts at
  // Skv-64 (slid back), keys before t*64 were already consumed by the previous tile
  const int tile_start = skv >= KVB ? (t * KVB < skv - KVB ? t * KVB : skv - KVB) : 0;
  const int kbase_idx = tile_start + 4 * ln.hh;
  if (t == nt - 1 && (skv & (KVB - 1))) {
    const int lo = t * KVB;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = kbase_idx + (i & 3) + 8 * (i >> 2);
      if (key < lo || key >= skv) s0[i] = -INFINITY;
      if (key + 32 < lo || key + 32 >= skv) s1[i] = -INFINITY;
    }
  }
  if constexpr (HAS_MASK) {   // the instantiation for a byte mask and / or an additive score bias
    if (p.mask) {
      const uint8_t* mrow = p.mask + (long long)qrow_c * p.Skv;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int key = kbase_idx + (i & 3) + 8 * (i >> 2);
        if (key < p.Skv && mrow[key]) s0[i] = -INFINITY;
        if (key + 32 < p.Skv && mrow[key + 32]) s1[i] = -INFINITY;
      }
    }
    if (p.bias) {   // softmax(scale q k^T + bias): the scores are in log2 units here (Q carries scale * log2 e), so the bias is too
      const float* brow = p.bias + (long long)ln.head * p.bias_sh + (long long)qrow_c * p.Skv;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int key = kbase_idx + (i & 3) + 8 * (i >> 2);
        if (key < p.Skv) s0[i] = fmaf(brow[key], kLog2e, s0[i]);
        if (key + 32 < p.Skv) s1[i] = fmaf(brow[key + 32], kLog2e, s1[i]);
      }
    }
  }
  // The v_max3 chains below are inline asm: hipcc pads the MFMA -> VALU read hazard only for instructions it can see, and on the paths without a
  // DMA hook between the score MFMAs and this point nothing else separates them (a stale read only mis-places the running max -- harmless to the
  // result, P is formed from the real scores by compiler-visible code -- but the fp8 kernel showed what a stale NaN pattern does).  19 wait
  // states cover the 16-pass MFMA (< 1 % of a tile).
  asm volatile("s_nop 15\n\ts_nop 2" ::: "memory");
  // tile max: four independent v_max3 chains, then across the two half-waves
  float ma = max3_asm(s0[0], s0[1], s0[2]), mb = max3_asm(s1[0], s1[1], s1[2]);
  float mc = max3_asm(s0[3], s0[4], s0[5]), md = max3_asm(s1[3], s1[4], s1[5]);
#pragma unroll
  for (int i = 6; i < 16; i += 4) {
    ma = max3_asm(ma, s0[i], s0[i + 1]);
    mb = max3_asm(mb, s1[i], s1[i + 1]);
    if (i + 3 < 16) {
      mc = max3_asm(mc, s0[i + 2], s0[i + 3]);
      md = max3_asm(md, s1[i + 2], s1[i + 3]);
    }
  }
  float tm = half_swap_max(max3_asm(max3_asm(ma, mb, mc), md, md));
  // deferred rescale: move the running max only on the first tile or when a row grew past THR
  const bool first = (t == 0);
  if (first || __any(tm > kThr)) {
    // First-tile floor.  A row whose first tile is fully blocked has tm = -inf and must start somewhere finite.  Masked / biased launches start it at
    // -2^14: exact in bf16, and the scores of the next tiles come out of the MFMA chain as S + 16384 with S kept to 2^-9 log2 units (0.07 % in P, below
    // P's own bf16 rounding); the row's first open tile then re-centres it through the tm > kThr branch (alpha = exp2(-delta) = 0 times an O and l that
    // are still zero).  From -1e30 the sum S + 1e30 lost S altogether and the row came out as uniform attention over that tile.
    constexpr float kFloor = HAS_MASK ? -16384.f : -1e30f;
    float delta = first ? fmaxf(tm, kFloor) : fmaxf(tm, 0.f);
    // the shift lives in a bf16 MFMA operand: round the new running max to bf16 and move by the EXACT difference (both ends are
    // bf16 values, their fp32 difference is exact), so O / l / P all see the same shift.  Rows that do not move keep delta == 0.
    const float m_new = bf_round(r.m + delta);
    delta = m_new - r.m;
    if (!first) {
      const float alpha = __builtin_amdgcn_exp2f(-delta);
#pragma unroll
      for (int i = 0; i < 16; ++i) { r.o0[i] *= alpha; r.o1[i] *= alpha; }
      r.lacc[0] *= alpha;
    }
    r.m += delta;
    r.negm[0] = -r.m;
    r.negm[1] = __uint_as_float(ln.hh == 0 ? (unsigned)f2bf(r.m) : 0u);   // query-side fragment (m, 0, ..., 0) of the max-subtracting k-step
#pragma unroll
    for (int i = 0; i < 16; ++i) { s0[i] -= delta; s1[i] -= delta; }
  }
  float la = 0.f, lb = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    s0[i] = __builtin_amdgcn_exp2f(s0[i]);
    s1[i] = __builtin_amdgcn_exp2f(s1[i]);
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    u32x4 w0, w1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w0[j] = pack_bf2(s0[8 * s + 2 * j], s0[8 * s + 2 * j + 1]);
      w1[j] = pack_bf2(s1[8 * s + 2 * j], s1[8 * s + 2 * j + 1]);
      // row sum of the bf16 pairs the PV MFMAs consume: one v_dot2c_f32_bf16 (pair . (1, 1) + acc, fp32) per packed register instead of
      // two v_add_f32 per pair -- 16 instead of 32 vector instructions per tile, and l sums exactly the P values that multiply V
      // (the packed registers pass through an empty asm: hipcc 7.2 otherwise selects sub-register 0 of the u32x4 for all four dot2c)
      unsigned p0 = w0[j], p1 = w1[j];
      asm volatile("" : "+v"(p0), "+v"(p1));
      w0[j] = p0; w1[j] = p1;
      la = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16v2, p0), __builtin_bit_cast(bf16v2, 0x3f803f80u), la, false);
      lb = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16v2, p1), __builtin_bit_cast(bf16v2, 0x3f803f80u), lb, false);
    }
    pb[s] = __builtin_bit_cast(bf16x8, w0);
    pb[2 + s] = __builtin_bit_cast(bf16x8, w1);
  }
  r.lacc[0] += la + lb;   // lane-local half of the row sum; the two half-waves are combined in the epilogue
}
}  // namespace
