// gemm_w4.hip -- the persistent four-wave GEMM: gemm_w4_kernel, its epilogues and its launcher (tests/test_gemm_w4_isa_cpu.py checks this unit's ISA).
#include "gemm_common.h"

namespace {

// the lane id, re-derived where it is needed from the (full: every branch around a caller is wave-uniform) exec mask.  volatile asm: hipcc neither hoists it
// out of the tile loop nor keeps a copy of the kernel's own lane id live across the K loop for it (such a copy is spilled around the loop)
__device__ __forceinline__ int lane_id_here() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}
// a masked (so provably non-negative) lane-derived index on its way into 64-bit pointer arithmetic: hipcc zero-extends it into a register pair whose high half, a
// constant 0, it defines once in front of the tile loop -- the pair is then live across the K loop and spilled around it.  Behind this the sign is unknown and the
// high half is made where the low half is (one shift per tile)
__device__ __forceinline__ int opaque_sign(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

// ---- the four-wave kernel's epilogue: 128x128 per wave.
// Fast path (the wave's 128 x 128 outputs all inside the matrix, 16-byte aligned rows, one gate vector for the whole wave tile -- every tile of the DiT but
// the last row of tiles): sixteen rows at a time go from the accumulator layout (lane: row (lane & 15), columns (lane >> 4) * 4 + {0..3} of every 16x16
// tile) through two PRIVATE 4-KB LDS buffers of the wave (the 32 KB the operand stages leave free -- those hold the NEXT tile's first two K-tiles by now;
// 16 rows x 256 B, 16-byte chunk c of row r at ((c ^ r) * 16): the 8-byte writes and the 16-byte reads both spread over every bank) into the row layout
// (lane: row (lane >> 4) of four, chunk (lane & 15)) and leave as whole 256-byte row segments -- 32 sixteen-byte stores per lane instead of 64 eight-byte
// pieces of sixteen rows each (direct form: 20 k cycles per tile; every CU of a round stores at the same time and the L2s take a 32-byte partial-line write
// as a transaction of its own).  No predication, no 64-bit multiplies (pointers step by scalar multiples of the leading dimension), no barrier (the
// buffers are the wave's own; row group i is written while i - 1 is read back).  vmcnt is one in-order counter: the residual vectors of row group i + 1 are
// requested BEFORE the stores of i - 1, so waiting for them never waits for a store.  Bias, activation, gate, the bf16 rounding and the residual add happen
// in the accumulator layout: the rounding points of the other epilogues (bit-equal results).
// General path (edge tiles, a sample or text / video boundary inside the wave's rows, unaligned C): 8-byte predicated stores from the accumulator layout.
template <int EPI>
__device__ __forceinline__ void epilogue_w4(const GemmP& p, char* smem, f32x4 (&acc)[8][8], const long long bm0, const long long bn0, const int wave, const int wrow0,
                                            const int wcol0, const long long Mend) {   // Mend: rows [.., Mend) exist (p.M, or the end of the tile's sample)
  constexpr bool HAS_R = (EPI == MRAG_EPI_GATE_RESID || EPI == MRAG_EPI_RESID), HAS_G = (EPI == MRAG_EPI_GATE_RESID), QK = (EPI == MRAG_EPI_QKNORM_ROPE);
  // the lane id comes from a volatile asm: everything below that depends on the lane only (LDS addresses, column offsets, row pointers) would
  // otherwise be hoisted out of the tile loop and kept in registers ACROSS the K loop, whose 128 fragment registers leave no room -- hipcc then spills
  // around the loop and parks the reload's `s_waitcnt vmcnt(0)` in the loop header, which drains the DMA ring once per K-tile (measured: +33 % K-loop time)
  const int lane = lane_id_here();
  const int frag_row = opaque_sign(lane & 15), frag_q = lane >> 4;
  const long long n0 = bn0 + wcol0 + frag_q * 4;                       // + 16 j
  const long long m0 = bm0 + wrow0;                                    // the wave's first row (wave-uniform)
  // sample / position of the wave's first row (GATE_RESID)
  long long g_b = 0, g_pos = 0;
  if constexpr (HAS_G || QK) {
    g_b = m0 / p.rows_per_batch;
    g_pos = m0 - g_b * p.rows_per_batch;
  }
  if (m0 >= Mend || bn0 + wcol0 >= p.N) return;                         // (a wave tile outside the matrix: nothing to store)
  const int mrows = (int)(Mend - m0 < 128 ? Mend - m0 : 128);            // the wave's valid rows (wave-uniform): < 128 in the last row of tiles only
  bool fast = p.staged && bn0 + wcol0 + 128 <= p.N;
  if constexpr (HAS_G) fast = fast && g_pos + mrows - 1 < p.rows_per_batch && ((g_pos < p.split) == (g_pos + mrows - 1 < p.split));
  auto add_resid = [&](u32x2 out, const u32x2 r2) __attribute__((always_inline)) -> u32x2 {
    out[0] = pack_bf2(__uint_as_float(out[0] << 16) + __uint_as_float(r2[0] << 16), __uint_as_float(out[0] & 0xffff0000u) + __uint_as_float(r2[0] & 0xffff0000u));
    out[1] = pack_bf2(__uint_as_float(out[1] << 16) + __uint_as_float(r2[1] << 16), __uint_as_float(out[1] & 0xffff0000u) + __uint_as_float(r2[1] & 0xffff0000u));
    return out;
  };
  auto acc_math = [&](const int i, const int j, const u32x2 b2, const u32x2 g2) __attribute__((always_inline)) -> u32x2 {   // bias, activation, gate, scale; packed (ONE rounding)
    float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
    v[0] += __uint_as_float(b2[0] << 16); v[1] += __uint_as_float(b2[0] & 0xffff0000u);
    v[2] += __uint_as_float(b2[1] << 16); v[3] += __uint_as_float(b2[1] & 0xffff0000u);
    if constexpr (EPI == MRAG_EPI_GELU_TANH) {                          // packed form: same bits, 4.5 instead of 7 issue slots per value
      const f32x2 lo = gelu_tanh_f2(f32x2{v[0], v[1]}), hi = gelu_tanh_f2(f32x2{v[2], v[3]});
      v[0] = lo[0]; v[1] = lo[1]; v[2] = hi[0]; v[3] = hi[1];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = epi_act<EPI>(v[e]);
    }
    if constexpr (HAS_G) {
      v[0] *= __uint_as_float(g2[0] << 16); v[1] *= __uint_as_float(g2[0] & 0xffff0000u);
      v[2] *= __uint_as_float(g2[1] << 16); v[3] *= __uint_as_float(g2[1] & 0xffff0000u);
    }
    if constexpr (EPI == MRAG_EPI_RESID) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= p.acc_scale;
    }
    return u32x2{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
  };
  if (fast) {
    u32x2 bias[8], gate[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bias[j] = p.bias ? *(const u32x2*)(p.bias + n0 + 16 * j) : u32x2{0u, 0u};
      if constexpr (HAS_G) gate[j] = *(const u32x2*)((g_pos < p.split ? p.gate0 : p.gate1) + g_b * p.gate_stride + n0 + 16 * j);
      else gate[j] = u32x2{0u, 0u};
    }
    const int r4 = lane >> 4, chunk = opaque_sign(lane & 15);           // row layout
    const bf16_t* rbase = HAS_R ? p.resid + m0 * p.ldr + n0 : nullptr;  // + row * ldr
    bf16_t* cbase = p.C + (m0 + r4) * p.ldc + (bn0 + wcol0 + chunk * 8);
    char* wput = smem + 131072 + wave * 8192 + frag_row * 256 + (frag_q & 1) * 8;
    const char* wget = smem + 131072 + wave * 8192 + r4 * 256;
    const int xput = frag_q >> 1;
    // QKNORM_ROPE (the fused QKV projection): the wave's 128 columns are two heads of ONE third (q_dmodel % 128 == 0), in the row layout the 8 lanes
    // (r4, chunk >> 3) hold a row of a head: qk_row_math on every 16-byte vector between the LDS read and the store.  The fp32 cos / sin rows (64 B per
    // lane and row) come through a ring of three (row-of-four) steps, each slot refilled as it is consumed
    int qk_which = 2;
    bool has_rope = false;
    const bf16_t *gm = nullptr, *bt = nullptr;
    float gam[8], bet[8];
    f32x4 qk_tab[QK ? 3 : 1][4];
    unsigned qk_video = 0;                                              // bit s: this lane's row of step s lies past the text rows
    auto qk_fetch = [&](const int st) __attribute__((always_inline)) {   // step st = rows 4 st .. 4 st + 3 of the wave tile
      if constexpr (QK) {
        const int row = 4 * st + r4;
        long long pos = g_pos + (row < mrows ? row : mrows - 1);
        while (pos >= p.rows_per_batch) pos -= p.rows_per_batch;
        const int rp = (int)pos - p.rope_text_len;
        if (rp >= 0) qk_video |= 1u << st;
        const long long ro = (long long)opaque_sign(rp > 0 ? rp : 0) * 64 + opaque_sign(chunk & 7) * 8;
        f32x4(&dst)[4] = qk_tab[st % 3];
        dst[0] = *(const f32x4*)(p.rcos + ro); dst[1] = *(const f32x4*)(p.rcos + ro + 4);
        dst[2] = *(const f32x4*)(p.rsin + ro); dst[3] = *(const f32x4*)(p.rsin + ro + 4);
      }
    };
    if constexpr (QK) {
      qk_which = p.qk_first + (int)((bn0 + wcol0) / p.qk_D);
      has_rope = p.rcos != nullptr && qk_which < 2;
#pragma unroll
      for (int e = 0; e < 8; ++e) { gam[e] = 1.f; bet[e] = 0.f; }
      if (qk_which < 2) {
        gm = qk_which ? p.kg : p.qg;
        bt = qk_which ? p.kb : p.qb;
        const int d0 = (chunk & 7) * 8;
        if (gm) {
          const u32x4 graw = *(const u32x4*)(gm + d0);
#pragma unroll
          for (int e = 0; e < 4; ++e) { gam[2 * e] = __uint_as_float(graw[e] << 16); gam[2 * e + 1] = __uint_as_float(graw[e] & 0xffff0000u); }
          if (bt) {
            const u32x4 braw = *(const u32x4*)(bt + d0);
#pragma unroll
            for (int e = 0; e < 4; ++e) { bet[2 * e] = __uint_as_float(braw[e] << 16); bet[2 * e + 1] = __uint_as_float(braw[e] & 0xffff0000u); }
          }
        }
      }
      if (has_rope) { qk_fetch(0); qk_fetch(1); qk_fetch(2); }
    }
    constexpr int RD = 2;   // residual row groups in flight (requested RD - 1 groups ahead of their use; deeper rings measured no faster and cost registers)
    u32x2 rr[RD][8];
    auto fetch = [&](const int i, const int slot) __attribute__((always_inline)) {
      if constexpr (HAS_R) {
        const int row = 16 * i + frag_row;
        const bf16_t* rrow = rbase + (long long)(row < mrows ? row : mrows - 1) * p.ldr;   // rows below the matrix re-read the last valid one
#pragma unroll
        for (int j = 0; j < 8; ++j) rr[slot][j] = *(const u32x2*)(rrow + 16 * j);
      }
    };
    auto put = [&](const int i) __attribute__((always_inline)) {        // row group i -> LDS buffer i & 1 (accumulator layout)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        u32x2 out = acc_math(i, j, bias[j], gate[j]);
        if constexpr (HAS_R) out = add_resid(out, rr[i % RD][j]);
        *(u32x2*)(wput + (i & 1) * 4096 + (((2 * j + xput) ^ frag_row) * 16)) = out;
      }
    };
    auto get_store = [&](const int i) __attribute__((always_inline)) {  // LDS buffer i & 1 -> global (row layout)
      u32x4 val[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) val[q] = *(const u32x4*)(wget + (i & 1) * 4096 + q * 1024 + ((chunk ^ (q * 4 + r4)) * 16));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if constexpr (QK) {
          const int st = 4 * i + q;
          if (qk_which < 2) {
            val[q] = qk_row_math(val[q], gm != nullptr, bt != nullptr, gam, bet, p.qk_eps, has_rope, (qk_video >> st) & 1u, qk_tab[st % 3], qk_which == 0 && p.q_premul != 1.0f, p.q_premul);
            if (has_rope && st + 3 < 32) qk_fetch(st + 3);             // refill the slot just consumed
          }
        }
        if (16 * i + 4 * q + r4 < mrows) *(u32x4*)(cbase + (long long)(16 * i + 4 * q) * p.ldc) = val[q];
      }
    };
#pragma unroll
    for (int i = 0; i < RD - 1; ++i) fetch(i, i);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      __builtin_amdgcn_sched_barrier(0);   // one row group at a time (keeps the live ranges of a group's 32 accumulator reads short)
      // (row groups below the matrix are computed like the others -- their loads re-read the last valid row, only their stores are masked: every load is
      // issued and consumed unconditionally, so hipcc's vmcnt bookkeeping is exact and carries nothing pending into the K loop)
      if (i + RD - 1 < 8) fetch(i + RD - 1, (i + RD - 1) % RD);
      put(i);
      if (i > 0) get_store(i - 1);     // (one wave, in-order LDS: these reads see the writes of iteration i - 1; the writes of i + 1 come after them)
    }
    __builtin_amdgcn_sched_barrier(0);
    get_store(7);
    // (every load of this path was consumed above, so hipcc's vmcnt bookkeeping carries nothing pending into the K loop: an explicit wait here would only
    // expose the latency of the stores just issued -- tests/test_gemm_w4_isa_cpu.py checks the compiled loop)
    return;
  }
  // ---- general path
  if constexpr (QK) return;             // (never dispatched without the fast path's conditions: launch_w4)
  auto ncol = [&](const int j) __attribute__((always_inline)) { const long long n = n0 + 16 * j; return n < p.N ? n : p.N - 4; };   // (N % 4 == 0)
#pragma unroll
  for (int i = 0; i < 8; ++i) {                                         // (fully unrolled: the accumulators are registers, never indexed at run time)
    __builtin_amdgcn_sched_barrier(0);
    const long long m = m0 + i * 16 + frag_row;
    const bool mok = m < Mend;
    const long long mc = mok ? m : Mend - 1;
    const bf16_t* gate = nullptr;
    if constexpr (HAS_G) {
      long long b = g_b, pos = g_pos + (mc - m0);
      while (pos >= p.rows_per_batch) { pos -= p.rows_per_batch; ++b; }
      gate = (pos < p.split ? p.gate0 : p.gate1) + b * p.gate_stride;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long n = ncol(j);
      const u32x2 b2 = p.bias ? *(const u32x2*)(p.bias + n) : u32x2{0u, 0u};
      u32x2 g2 = u32x2{0u, 0u};
      if constexpr (HAS_G) g2 = *(const u32x2*)(gate + n);
      u32x2 out = acc_math(i, j, b2, g2);
      if constexpr (HAS_R) out = add_resid(out, *(const u32x2*)(p.resid + mc * p.ldr + n));
      if (mok && n0 + 16 * j < p.N) *(u32x2*)(p.C + mc * p.ldc + n) = out;
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0070);     // vmcnt(0) lgkmcnt(0): see the fast path (this path runs on edge tiles only)
}

// ---- the four-wave kernel's GEGLU epilogue (W rows interleaved in 16-row [value | gate] groups: the even 16-column MFMA tile of a pair holds the values, the
// odd one the gates of the same 16 outputs, in the same lanes; C is [M, N / 2]): the wave's 128 x 64 outputs, sixteen rows at a time through two private
// 2-KB LDS buffers (128-byte rows, 16-byte chunk c of row r at ((c ^ (r & 7)) * 16)) into whole 128-byte row segments.  The arithmetic of the 8-wave GEGLU
// epilogues: both halves rounded to bf16 before the product (nn.Linear's output dtype).  Launched only with whole 128-column wave tiles and 16-byte aligned rows.
template <int EPI>
__device__ __forceinline__ void epilogue_w4_geglu(const GemmP& p, char* smem, f32x4 (&acc)[8][8], const long long bm0, const long long bn0, const int wave, const int wrow0,
                                                  const int wcol0) {
  const int lane = lane_id_here();                                     // see epilogue_w4
  const int frag_row = lane & 15, frag_q = lane >> 4;
  const long long m0 = bm0 + wrow0;
  if (m0 >= p.M || bn0 + wcol0 >= p.N) return;                         // a wave tile outside the matrix (N % 128 == 0: a wave's columns are all in or all out)
  const int mrows = (int)(p.M - m0 < 128 ? p.M - m0 : 128);
  const long long n0 = bn0 + wcol0 + frag_q * 4;                       // value columns of pair jj at n0 + 32 jj, gates 16 further
  u32x2 bv[4], bg[4];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    bv[jj] = p.bias ? *(const u32x2*)(p.bias + n0 + 32 * jj) : u32x2{0u, 0u};
    bg[jj] = p.bias ? *(const u32x2*)(p.bias + n0 + 32 * jj + 16) : u32x2{0u, 0u};
  }
  const int r8 = lane >> 3, chunk = opaque_sign(lane & 7);             // row layout: 8 rows x 8 chunks per instruction
  bf16_t* cbase = p.C + (m0 + r8) * p.ldc + ((bn0 + wcol0) >> 1) + chunk * 8;
  char* wput = smem + 131072 + wave * 8192 + frag_row * 128 + (frag_q & 1) * 8;
  const char* wget = smem + 131072 + wave * 8192 + r8 * 128 + ((chunk ^ r8) * 16);   // rows r8 and r8 + 8 share (row & 7)
  const int xput = frag_q >> 1, sw = frag_row & 7;
  auto put = [&](const int i) __attribute__((always_inline)) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      float v[4] = {acc[i][2 * jj][0], acc[i][2 * jj][1], acc[i][2 * jj][2], acc[i][2 * jj][3]};
      float g[4] = {acc[i][2 * jj + 1][0], acc[i][2 * jj + 1][1], acc[i][2 * jj + 1][2], acc[i][2 * jj + 1][3]};
      v[0] += __uint_as_float(bv[jj][0] << 16); v[1] += __uint_as_float(bv[jj][0] & 0xffff0000u);
      v[2] += __uint_as_float(bv[jj][1] << 16); v[3] += __uint_as_float(bv[jj][1] & 0xffff0000u);
      g[0] += __uint_as_float(bg[jj][0] << 16); g[1] += __uint_as_float(bg[jj][0] & 0xffff0000u);
      g[2] += __uint_as_float(bg[jj][1] << 16); g[3] += __uint_as_float(bg[jj][1] & 0xffff0000u);
      geglu4<EPI == EPI_GEGLU_TANH>(v, g);
      *(u32x2*)(wput + (i & 1) * 2048 + (((2 * jj + xput) ^ sw) * 16)) = u32x2{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
    }
  };
  auto get_store = [&](const int i) __attribute__((always_inline)) {
    u32x4 val[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) val[q] = *(const u32x4*)(wget + (i & 1) * 2048 + q * 1024);
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (16 * i + 8 * q + r8 < mrows) *(u32x4*)(cbase + (long long)(16 * i + 8 * q) * p.ldc) = val[q];
  };
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    __builtin_amdgcn_sched_barrier(0);
    put(i);                                                            // (rows below the matrix: computed, not stored)
    if (i > 0) get_store(i - 1);
  }
  __builtin_amdgcn_sched_barrier(0);
  get_store(7);
}

// compile-time loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>)
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (N > 0) {
    static_for<N - 1>(f);
    f(std::integral_constant<int, N - 1>{});
  }
}

// logical tile L -> (tile_m, tile_n): groups of group_m m-tiles walked n-major (see gemm_tile)
__device__ __forceinline__ void tile_coords(const GemmP& p, const int L, int& tile_m, int& tile_n) {
  const int gw = p.group_m * p.tiles_n;
  const int first_m = (L / gw) * p.group_m;
  const int gsz = min(p.tiles_m - first_m, p.group_m);
  tile_m = first_m + (L % gw) % gsz;
  tile_n = (L % gw) / gsz;
}

// ---- 256x256 tiles on FOUR waves (one per SIMD, 128x128 per wave, the 256 accumulator registers pinned in AGPRs), PERSISTENT workgroups (one per CU)
// whose K-tile stream runs across tile boundaries, and an instruction-level hand schedule.
// * Per 64-deep K-tile and wave the matrix pipe sees 128 MFMAs with one memory instruction behind every second one: 32 fragment reads (2/3 of the 8-wave
//   tile's LDS bytes per FLOP) and 16 LDS-DMA pieces (scalar base + loop-invariant 32-bit lane offset: no vector address arithmetic in the loop), two
//   barriers, two counted waits.  Every statement of the K loop is volatile inline asm: hipcc only allocates registers.  (Round-3 attempts with 8-MFMA
//   blocks and bursts of reads / pieces lost 3-15 % to the 8-wave loop: one wave per SIMD has no partner to hide a burst behind.)
// * The DMA cursor runs two K-tiles ahead of the MFMAs and simply walks into the workgroup's NEXT tile: when a tile's last MFMA retires, the first two
//   K-tiles of the next one are in LDS (its first fragments are read again behind the epilogue: one LDS latency, and 64 registers the epilogue does not have to
//   spill around), so the matrix pipe idles only for the epilogue's own instructions -- not for
//   a workgroup launch, an address set-up and a cold first fetch per tile (measured on the non-persistent form of this loop: 17 us per tile, 18 % of a
//   K = 3072 tile).  vmcnt is ONE in-order counter for loads and stores: the epilogue first waits for the (old) DMA pieces, then stores, and the first K-tile
//   behind it runs the variant without a counted wait, so no wait in the loop ever stands behind a store that has just been issued.
// LDS: two 64-KB stages [A rows 0..255 | W rows 0..255], 128-byte rows, 16-byte chunk c of row r at ((c ^ (r & 7)) * 16).
// K-tile g of the stream (stage s = g & 1):  k-step 0 MFMAs | reads of (g, k-step 1) .. lgkmcnt(0), BARRIER (stage s is free) .. DMA of K-tile g + 2 -> stage s
//                                            k-step 1 MFMAs | vmcnt (K-tile g + 1 landed), BARRIER .. reads of (g + 1, k-step 0) .. rest of the DMA
// WB (per-sample weights; EPI_NONE): sample b's rows [b rows_per_batch, (b + 1) rows_per_batch) multiply W + b w_bstride -- the motion branch's folded score GEMM, whose
// weights are built from each CFG sample's own motion tokens (attn_processor.py:250-256).  The row-tile grid restarts at every sample (no tile straddles
// two weight matrices; a sample's last tile is clamped / masked at the sample's end), so both samples ride ONE persistent launch: 700 tiles = 2.73 -> 3
// rounds where two launches of 350 paid 2 + 2.
template <int EPI, bool WB = false>
__global__ __launch_bounds__(256) void gemm_w4_kernel(const GemmP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr unsigned STAGE = 65536, WOFF = 32768;
  const int lane = threadIdx.x & 63;
  const int wave_s = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), wm = wave_s >> 1, wn = wave_s & 1;   // scalars: the epilogue's row / column origins and branches stay off the VGPRs
  const int tiles = p.tile_limit, nk = (int)(p.K / 64), G = (int)gridDim.x;
  // origin of logical tile (tm, tn): first row, one past the last row that exists for it, element offset of its weight matrix
  auto tile_origin = [&](const int tm, long long& bm0, long long& m_end, long long& w_off) __attribute__((always_inline)) {
    if constexpr (WB) {
      const int b = tm / p.wb_tiles_m;
      bm0 = (long long)b * p.rows_per_batch + (long long)(tm - b * p.wb_tiles_m) * 256;
      m_end = (long long)(b + 1) * p.rows_per_batch;
      w_off = (long long)b * p.w_bstride;
    } else {
      bm0 = (long long)tm * 256; m_end = p.M; w_off = 0;
    }
  };
  const int slot = xcd_remap((int)blockIdx.x, G);   // this workgroup's tiles: slot, slot + G, ... (round r of the grid = what a one-tile-per-workgroup launch dispatches)
  // ---- DMA cursor: (tile d_r of this workgroup, K-tile d_kt).  Piece q = wave + 4 i, i = 0..15 (i < 8: A rows 8 q .. 8 q + 7, else W rows 8 (q - 32) ..);
  // lane -> row (lane >> 3) of the piece, source chunk (lane & 7) ^ row
  unsigned voff[16];
  const bf16_t *baseA = p.A, *baseW = p.W;
  int d_r = 0, d_kt = 0;
  bool d_valid = false;
  auto cursor_set = [&](const int r) __attribute__((always_inline)) {
    const int L = r * G + slot;
    d_valid = L < tiles;
    if (!d_valid) return;                 // the stream has ended: the cursor stays where it is (see `advance`)
    int tm, tn;
    tile_coords(p, L, tm, tn);
    long long bm0, m_end, w_off;
    tile_origin(tm, bm0, m_end, w_off);
    const long long bn0 = (long long)tn * 256;
    const int lane_c = lane_id_here();      // (see epilogue_w4: nothing lane-derived of this block may stay live across the K loop)
    const int prow = lane_c >> 3, pchk = (lane_c & 7) ^ prow;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int q = wave_s + 4 * i;
      long long r8 = (i < 8) ? 8 * q + prow : 8 * (q - 32) + prow;
      const long long lim = (i < 8) ? m_end - bm0 : p.N - bn0;        // clamp: tail rows re-read the tile's last valid row, stores are masked
      r8 = r8 < lim ? r8 : lim - 1;
      voff[i] = (unsigned)((r8 * ((i < 8) ? p.lda : p.ldw) + pchk * 8) * 2);
    }
    baseA = p.A + bm0 * p.lda;
    baseW = p.W + w_off + bn0 * p.ldw;
  };
  // past the end of the stream the cursor stays on its last K-tile: the loop below has ONE instruction stream (one register allocation for the 256 pinned
  // accumulators -- with one body per stream state hipcc spilled accumulators at the joins), so the last two K-tiles of a workgroup re-request a K-tile
  // into a stage nobody reads again (two redundant L2 reads per workgroup) instead of branching around their DMA
  auto advance = [&]() __attribute__((always_inline)) {
    if (!d_valid) return;
    if (d_kt + 1 < nk) { ++d_kt; return; }
    cursor_set(d_r + 1);
    if (d_valid) { ++d_r; d_kt = 0; }
  };
  const unsigned smem_u = (unsigned)(size_t)smem;
  // fragment reads: lane (row r = lane & 15, k-quarter q = lane >> 4) reads chunk (q [+ 4]) ^ (r & 7) of its row
  const unsigned fr = lane & 15, fq = lane >> 4, swz = lane & 7;
  const unsigned c0 = ((fq + 0) ^ swz) * 16, c1 = ((fq + 4) ^ swz) * 16;
  const unsigned rowA = smem_u + (wm * 128 + fr) * 128, rowW = smem_u + WOFF + (wn * 128 + fr) * 128;
  f32x4 acc[8][8];
  u32x4 a0[8], w0[8], a1[8], w1[8];
#define MRAG_W4_MF(I, J, W, A) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[I][J]) : "v"(W[J]), "v"(A[I]))
#define MRAG_W4_RD(D, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(D) : "v"(ADDR), "n"(OFF) : "memory")
#define MRAG_W4_LGKM0(W, A)                                                                                          \
      asm volatile("s_waitcnt lgkmcnt(0)"                                                                             \
                   : "+v"(W[0]), "+v"(W[1]), "+v"(W[2]), "+v"(W[3]), "+v"(W[4]), "+v"(W[5]), "+v"(W[6]), "+v"(W[7]),   \
                     "+v"(A[0]), "+v"(A[1]), "+v"(A[2]), "+v"(A[3]), "+v"(A[4]), "+v"(A[5]), "+v"(A[6]), "+v"(A[7])    \
                   :: "memory")
  unsigned aw1, aa1, aw0, aa0, stage_u;   // function scope: clang rejects asm operands that name an enclosing LAMBDA's locals from a nested lambda
  auto dma = [&](auto I) __attribute__((always_inline)) {                // piece wave + 4 i of the cursor's K-tile into the stage at LDS address stage_u
    constexpr int i = decltype(I)::value;
    (void)&voff;                          // (clang does not capture a variable that a generic lambda names only in asm operands)
    const bf16_t* sb = (i < 8 ? baseA : baseW) + (long long)d_kt * 64;
    const unsigned lds = stage_u + (unsigned)(wave_s + 4 * i) * 1024u;
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voff[i]), "s"(sb), "s"(lds) : "memory", "m0");
  };
  // one K-tile of the stream.  `counted`: the wait in front of the second barrier (false for the K-tile right behind an epilogue, which waited for every piece)
  auto kstep = [&](const unsigned g, const bool counted) __attribute__((always_inline)) {
    const unsigned so = (g & 1) ? STAGE : 0u, sn = STAGE - so;        // this K-tile's stage offset, the other stage's
    aw1 = rowW + so + c1; aa1 = rowA + so + c1;                       // (g, k-step 1)
    aw0 = rowW + sn + c0; aa0 = rowA + sn + c0;                       // (g + 1, k-step 0)
    stage_u = smem_u + so;
    MRAG_W4_LGKM0(w0, a0);
    // ---- k-step 0: 64 MFMAs on (w0, a0)
    static_for<32>([&](auto S) __attribute__((always_inline)) {
      constexpr int sl = decltype(S)::value, i = (2 * sl) / 8, j = (2 * sl) % 8;
      (void)&acc; (void)&w0; (void)&a0; (void)&w1; (void)&a1; (void)&aw1; (void)&aa1;
      MRAG_W4_MF(i, j, w0, a0);
      if constexpr (sl < 8) MRAG_W4_RD(w1[sl], aw1, sl * 2048);
      else if constexpr (sl < 16) MRAG_W4_RD(a1[sl - 8], aa1, (sl - 8) * 2048);
      else if constexpr (sl == 22) { MRAG_W4_LGKM0(w1, a1); asm volatile("s_barrier" ::: "memory"); }
      else if constexpr (sl >= 23 && (sl & 1)) dma(std::integral_constant<int, (sl - 23) / 2>{});   // pieces 0..4
      MRAG_W4_MF(i, j + 1, w0, a0);
    });
    // ---- k-step 1: 64 MFMAs on (w1, a1)
    if (counted) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");      // K-tile g + 1 has landed (5 pieces of g + 2 in flight)
    asm volatile("s_barrier" ::: "memory");                            // ... for every wave
    static_for<32>([&](auto S) __attribute__((always_inline)) {
      constexpr int sl = decltype(S)::value, i = (2 * sl) / 8, j = (2 * sl) % 8;
      (void)&acc; (void)&w0; (void)&a0; (void)&w1; (void)&a1; (void)&aw0; (void)&aa0;
      MRAG_W4_MF(i, j, w1, a1);
      if constexpr (sl < 8) MRAG_W4_RD(w0[sl], aw0, sl * 2048);
      else if constexpr (sl < 16) MRAG_W4_RD(a0[sl - 8], aa0, (sl - 8) * 2048);
      else if constexpr (sl >= 16 && sl < 27) dma(std::integral_constant<int, sl - 11>{});          // pieces 5..15
      MRAG_W4_MF(i, j + 1, w1, a1);
    });
  };
  // ---- prologue: the stream's first two K-tiles, the first fragments
  cursor_set(0);
  if (!d_valid) return;
  stage_u = smem_u;
  static_for<16>([&](auto I) __attribute__((always_inline)) { dma(I); });
  advance();
  stage_u = smem_u + STAGE;
  static_for<16>([&](auto I) __attribute__((always_inline)) { dma(I); });
  advance();
  asm volatile("s_waitcnt vmcnt(16)\n\ts_barrier" ::: "memory");
  unsigned g = 0;
  for (int r = 0;; ++r) {
    const int L = r * G + slot;
    if (L >= tiles) break;
    // the tile's first fragments (K-tile g, k-step 0), read HERE for every tile and not carried over from the previous tile's last K-tile: that K-tile
    // issues the same reads (one loop body), but their 64 registers are dead across the epilogue, which would otherwise spill accumulator copies around them
    // (the reloads stood behind the tile's own stores in the in-order vmcnt).  The stage was published by the barrier in front of that K-tile's k-step 1 (by
    // the one above for the stream's first tile) and the DMA in flight goes to the other stage; kstep begins with lgkmcnt(0).
    aw0 = rowW + ((g & 1) ? STAGE : 0u) + c0; aa0 = rowA + ((g & 1) ? STAGE : 0u) + c0;
    static_for<8>([&](auto J) __attribute__((always_inline)) { constexpr int j = decltype(J)::value; (void)&w0; (void)&aw0; MRAG_W4_RD(w0[j], aw0, j * 2048); });
    static_for<8>([&](auto J) __attribute__((always_inline)) { constexpr int j = decltype(J)::value; (void)&a0; (void)&aa0; MRAG_W4_RD(a0[j], aa0, j * 2048); });
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    asm volatile("s_nop 4" ::: "memory");   // accumulator writes -> first MFMA (the asm MFMAs are invisible to hipcc's hazard pass)
    for (int t = 0; t < nk; ++t, ++g) {
      kstep(g, !(t == 0 && r > 0));
      advance();
    }
    // the MFMAs above are invisible to hipcc's hazard pass: the accumulators are read (v_accvgpr_read) only after the matrix pipe has drained; every DMA piece
    // in flight (issued BEFORE the stores below) is waited for here, so the next counted wait in the loop comes two K-tiles after the stores
    // (lgkmcnt(0): the last K-tile's k-step-1 reads have landed before hipcc reuses their -- now dead -- registers in the epilogue)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15\n\ts_nop 7" ::: "memory");
    int tm, tn;
    tile_coords(p, L, tm, tn);
    long long e_bm0, e_mend, e_woff;
    tile_origin(tm, e_bm0, e_mend, e_woff);
    if constexpr (is_geglu<EPI>) epilogue_w4_geglu<EPI>(p, smem, acc, e_bm0, (long long)tn * 256, wave_s, wm * 128, wn * 128);
    else epilogue_w4<EPI>(p, smem, acc, e_bm0, (long long)tn * 256, wave_s, wm * 128, wn * 128, e_mend);
  }
#undef MRAG_W4_MF
#undef MRAG_W4_RD
#undef MRAG_W4_LGKM0
}

// The partial last round of the persistent grid as a RECTANGLE of small tiles.  One workgroup per CU: a launch costs ceil(tiles / 256) rounds however
// full the last one is -- the DiT's FF1 (139 x 48 = 6 672 tiles = 26.06 rounds) pays a 27th round of 79 us for 16 tiles.  Stream-K over those tiles
// measured slower (EXPERIMENTS.md section 3: the runs lose the lock-step that lets an XCD's L2 serve an operand panel once).  When the remainder is SMALL
// the tail was EXPECTED to be cheaper as its own launch of 128x128 tiles (two workgroups per CU, 72 workgroups for FF1's 3 x 6 tiles) -- and MEASURED equal:
// FF1 + GELU 2.236-2.246 ms against 2.245-2.257 ms, the denoise step 550.41 against 550.40 ms (profiles/r6_microbench_items.txt, r6_step_ab_toggles.txt): sixteen
// tiles on sixteen CUs of an otherwise idle chip run well above the loaded rate, so the 27th round costs far less than a round.  OPT-IN
// (MRAG_GEMM_TUNE_TAIL_RECT), kept with its test like the stream-K tail.  The logical tile order walks
// the last group of row tiles column by column, so the last `rem` tiles lie inside the rectangle [last row group] x [last ceil(rem / gsz) tile
// columns]; the persistent launch stops in front of it (GemmP::tile_limit) and the rectangle runs as a plain sub-problem (pointers advanced).  Same K
// order and rounding points: bit-equal to the one-launch form (test_gemm_w4_tail_rectangle).
struct TailRect { bool use = false; int limit = 0; long long r0 = 0, c0 = 0; };
inline TailRect plan_tail_rect(const GemmP& p, int epi) {
  TailRect t;
  const long long tiles = (long long)p.tiles_m * p.tiles_n;
  if (p.wb_tiles_m || !tail_rect_wanted(tiles, epi, p.tuning)) return t;
  const int rem = (int)(tiles % SK_CUS);
  const int first_m = ((p.tiles_m - 1) / p.group_m) * p.group_m, gsz = p.tiles_m - first_m;
  const int ncols = (rem + gsz - 1) / gsz;
  if (ncols > p.tiles_n) return t;
  t.use = true;
  t.limit = (int)(tiles - (long long)gsz * ncols);
  t.r0 = (long long)first_m * 256; t.c0 = (long long)(p.tiles_n - ncols) * 256;
  return t;
}

}  // namespace

// the persistent four-wave launch: one workgroup per CU, 128 KB of LDS
extern "C" int launch_w4(hipStream_t s, const GemmP& p0, int epi) {
  // the K-tile stream walks A and W with 32-bit byte offsets inside a 256-row panel: (row * ld + chunk) * 2 with row <= 255 must stay below 4 GiB
  // (a view with a huge leading dimension goes to the 8-wave kernel, whose row pointers are 64-bit)
  if (256LL * (p0.lda > p0.ldw ? p0.lda : p0.ldw) * 2 >= (1LL << 32)) return MRAG_ENOTSUP;
  GemmP p = p0;
  const bool wb = p.w_bstride != 0;
  if (wb) {                                     // per-sample weights: the row-tile grid restarts at every sample
    if (epi != MRAG_EPI_NONE || p.rows_per_batch <= 0 || p.M % p.rows_per_batch != 0) return MRAG_ENOTSUP;
    p.wb_tiles_m = (int)((p.rows_per_batch + 255) / 256);
    p.tiles_m = (int)(p.M / p.rows_per_batch) * p.wb_tiles_m;
  } else {
    p.wb_tiles_m = 0;
    p.tiles_m = (int)((p.M + 255) / 256);
  }
  p.tiles_n = (int)((p.N + 255) / 256);
  p.group_m = group_m_of(p.tuning);
  const long long tiles = (long long)p.tiles_m * p.tiles_n;
  // the LDS-staged epilogue needs 16-byte aligned rows of C (and of the residual); otherwise the direct 8-byte store path runs
  p.staged = rows_16B_aligned(p.C, p.ldc, p.resid, p.ldr);
  if (p.tuning & MRAG_GEMM_TUNE_NO_STAGED) p.staged = 0;
  const TailRect tail = plan_tail_rect(p, epi);
  p.tile_limit = tail.use ? tail.limit : (int)tiles;
  const dim3 grid((unsigned)(p.tile_limit < SK_CUS ? p.tile_limit : SK_CUS)), block(256);
  const size_t lds = 131072 + 32768;   // two operand stages + 8 KB of epilogue staging per wave: all 160 KB of a CU
  int rc;
  switch (epi) {
    case MRAG_EPI_NONE:
      rc = wb ? launch_dyn_lds(gemm_w4_kernel<MRAG_EPI_NONE, true>, grid, block, lds, s, p) : launch_dyn_lds(gemm_w4_kernel<MRAG_EPI_NONE>, grid, block, lds, s, p);
      break;
    case MRAG_EPI_GELU_TANH: rc = launch_dyn_lds(gemm_w4_kernel<MRAG_EPI_GELU_TANH>, grid, block, lds, s, p); break;
    case MRAG_EPI_RESID: rc = launch_dyn_lds(gemm_w4_kernel<MRAG_EPI_RESID>, grid, block, lds, s, p); break;
    case MRAG_EPI_GATE_RESID: rc = launch_dyn_lds(gemm_w4_kernel<MRAG_EPI_GATE_RESID>, grid, block, lds, s, p); break;
    case MRAG_EPI_GEGLU:
    case EPI_GEGLU_TANH:                  // whole 128-column wave tiles, aligned rows of C [M, N / 2]
      if (!p.staged || p.N % 128 != 0) return MRAG_ENOTSUP;
      rc = epi == MRAG_EPI_GEGLU ? launch_dyn_lds(gemm_w4_kernel<MRAG_EPI_GEGLU>, grid, block, lds, s, p) : launch_dyn_lds(gemm_w4_kernel<EPI_GEGLU_TANH>, grid, block, lds, s, p);
      break;
    case MRAG_EPI_QKNORM_ROPE:            // fast epilogue path only: whole 128-column wave tiles inside one third, aligned rows
      if (!p.staged || p.N % 128 != 0 || p.qk_D % 128 != 0) return MRAG_ENOTSUP;
      rc = launch_dyn_lds(gemm_w4_kernel<MRAG_EPI_QKNORM_ROPE>, grid, block, lds, s, p);
      break;
    default: return MRAG_ENOTSUP;
  }
  if (rc != MRAG_OK) return rc;
  MRAG_COUNT(epi == MRAG_EPI_QKNORM_ROPE ? MRAG_K_GEMM_W4_QKNORM_ROPE : (epi == MRAG_EPI_GEGLU || epi == EPI_GEGLU_TANH) ? MRAG_K_GEMM_W4_GEGLU : wb ? MRAG_K_GEMM_W4_BATCHED_W : MRAG_K_GEMM_W4);
  if (tail.use) {                               // the rectangle behind the whole rounds: rows [r0, M) x columns [c0, N) on 128x128 tiles
    GemmP t = p0;
    t.A = p0.A + tail.r0 * p0.lda; t.W = p0.W + tail.c0 * p0.ldw; t.C = p0.C + tail.r0 * p0.ldc + tail.c0;
    if (p0.bias) t.bias = p0.bias + tail.c0;
    if (p0.resid) t.resid = p0.resid + tail.r0 * p0.ldr + tail.c0;
    t.M = p0.M - tail.r0; t.N = p0.N - tail.c0;
    rc = launch_tiled(s, t, epi, TILE_128x128, nullptr);
    if (rc != MRAG_OK) return rc;
    MRAG_COUNT(MRAG_K_GEMM_W4_TAIL_RECT);
  }
  return MRAG_OK;
}
