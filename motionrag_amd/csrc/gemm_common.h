// gemm_common.h -- what the GEMM units share.  One kernel family per unit, so that a family can be read, edited and rebuilt alone:
//   gemm_bf16.hip    dispatch only: mrag_gemm_bf16 picks a family per problem
//   gemm_tile.h      the tiled kernel (gemm_bf16_kernel) and its launcher template; instantiated by
//   gemm_tiled.hip     ... the linears' tile shapes and the stream-K tail (launch_tiled)
//   gemm_conv.hip      ... the implicit-GEMM convolutions (mrag_conv_bf16)
//   gemm_w4.hip      the persistent four-wave kernel (launch_w4)
//   gemm_k320.hip    K = 320, weight in registers (launch_k320)
//   gemm_skinny.hip  few rows, K split over the waves (launch_skinny)
// Here: the kernel parameter block, the epilogue arithmetic that more than one family uses, the tile-choice predicates of the GEMM and the convolution
// dispatch and the family launchers' declarations (the launch helper, launch_dyn_lds, is common.h's).
#pragma once
#include <type_traits>
#include "common.h"
#include "../../include/mrag_hip.h"

namespace {

struct GemmP {
  const bf16_t* A; const bf16_t* W; const bf16_t* bias; bf16_t* C; const bf16_t* resid;
  const bf16_t* gate0; const bf16_t* gate1;
  long long M, N, K, lda, ldw, ldc, ldr, rows_per_batch, split, gate_stride;
  int tiles_m, tiles_n, group_m, staged, tuning;
  // MRAG_EPI_QKNORM_ROPE
  const bf16_t* qg; const bf16_t* qb; const bf16_t* kg; const bf16_t* kb; const float* rcos; const float* rsin;
  long long qk_D; int rope_text_len, qk_first; float qk_eps, q_premul;
  // implicit-GEMM convolution (CONV != 0): A is the channels-last activation, rows are gathered per K-tile
  int cv_H, cv_W, cv_Hi, cv_Wi, cv_Ho, cv_Wo, cv_stride, cv_up, cv_ctiles, cv_T, cv_pad;   // cv_pad: zero rows / columns in FRONT of the image (1, or 0 for the bottom/right-only padding)
  long long cv_C, cv_HW;
  // stream-K tail (SK instantiation): logical tiles [0, sk_main) run one per workgroup; the sk_rem tiles behind them are cut into sk_units equal
  // runs of K-tiles, one per workgroup; partial accumulators meet in sk_part, the last arriver of a tile (sk_ticket) sums them in K order
  float acc_scale;    // MRAG_EPI_RESID: C = resid + acc_scale * (acc + bias) (1 unless the caller blends: AlphaBlender folded into a residual branch)
  float* sk_part; unsigned* sk_ticket;
  int sk_main, sk_rem, sk_units, sk_maxparts;
  const bf16_t* lna_g; const bf16_t* lna_b; float lna_eps; int lna;   // gemm_skinny_kernel<.., LNA>: A := LayerNorm_K(A) * lna_g + lna_b in front of the product (either may be null)
  int tile_limit;     // gemm_w4_kernel: tiles [0, tile_limit) of the logical order (all of them, or the whole rounds in front of a tail launch: launch_w4)
  int wb_tiles_m;     // gemm_w4_kernel<EPI, true> (per-sample weights): 256-row tiles per sample -- the row-tile grid restarts at every sample; 0 otherwise
  long long w_bstride;   // elements between the samples' weight matrices
  int cv_lds;         // CONV != 0: byte offset of the parked per-lane tap state in LDS (behind the operand stages / staged-epilogue region)
  int cv_tf;          // CONV == 1 with three temporal taps (causal 3x3x3): output frames per sample (input holds cv_tf + 2 frames per sample); 0 = 2-D
  long long cv_fs;    // elements between consecutive input frames
};

// stream-K and the persistent kernels: one workgroup per CU
constexpr int SK_CUS = 256, SK_TICKET_BYTES = 1024;
constexpr int SK_FLAG_OFF = 8 * 128 * 144;   // one LDS word behind the staged epilogue's region (stream-K: "this workgroup finishes the tile")
constexpr int SKM_ROWS = 32;                 // rows of a few-row tile (gemm_skinny_kernel; skinny_applies)

// sum over the 8 lanes that hold one row (lanes 8g..8g+7) on the vector pipe: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror
// (lane i <-> 7 - i of its half row).  __shfl_xor compiles to ds_bpermute_b32 -- an LDS round trip each, six dependent ones per row group.
__device__ __forceinline__ float sum8_dpp(float x) {
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, true));
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xF, 0xF, true));
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x141, 0xF, 0xF, true));
  return x;
}

// one row's 8 features of a head in the row layout (the 8 lanes 8g .. 8g + 7 hold the head's 64 features): per-head LayerNorm across those lanes, RoPE on the
// lane's four (even, odd) pairs, Q pre-multiplied -- the arithmetic of qknorm_rope_kernel (norm.hip).  Shared by the 8-wave and the four-wave kernels (same bits).
__device__ __forceinline__ u32x4 qk_row_math(u32x4 val, const bool has_gamma, const bool has_beta, const float (&gam)[8], const float (&bet)[8], const float eps,
                                             const bool has_rope, const bool vid, const f32x4 (&t4)[4], const bool premul_on, const float premul) {
  float v[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[2 * e] = __uint_as_float(val[e] << 16); v[2 * e + 1] = __uint_as_float(val[e] & 0xffff0000u); }
  if (has_gamma) {
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) sum += v[e];
    sum = sum8_dpp(sum);
    const float mean = sum * (1.0f / 64.0f);
    float sq = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { v[e] -= mean; sq += v[e] * v[e]; }
    sq = sum8_dpp(sq);
    const float rstd = rsqrtf(sq * (1.0f / 64.0f) + eps);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = v[e] * rstd * gam[e];
    if (has_beta) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += bet[e];
    }
  }
  if (has_rope) {
    const float cc[8] = {t4[0][0], t4[0][1], t4[0][2], t4[0][3], t4[1][0], t4[1][1], t4[1][2], t4[1][3]};
    const float ss[8] = {t4[2][0], t4[2][1], t4[2][2], t4[2][3], t4[3][0], t4[3][1], t4[3][2], t4[3][3]};
#pragma unroll
    for (int i2 = 0; i2 < 4; ++i2) {
      const float a = v[2 * i2], b2 = v[2 * i2 + 1];
      const float oa = a * cc[2 * i2] - b2 * ss[2 * i2];
      const float ob = b2 * cc[2 * i2 + 1] + a * ss[2 * i2 + 1];
      v[2 * i2] = vid ? oa : a;
      v[2 * i2 + 1] = vid ? ob : b2;
    }
  }
  if (premul_on) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= premul;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) val[e] = pack_bf2(v[2 * e], v[2 * e + 1]);
  return val;
}

// internal epilogue id: MRAG_EPI_GEGLU with the tanh gate (mrag_gemm_args.geglu_act = 1, T5's gated-gelu): its own instantiation, so the erf kernels of the
// UNets (epilogue-bound at K = 320) carry neither a branch nor the second activation's registers
constexpr int EPI_GEGLU_TANH = 8;
template <int EPI>
constexpr bool is_geglu = (EPI == MRAG_EPI_GEGLU || EPI == EPI_GEGLU_TANH);

template <int EPI>
__device__ __forceinline__ float epi_act(float v) {
  if constexpr (EPI == MRAG_EPI_GELU_TANH) return gelu_tanh_f(v);
  else if constexpr (EPI == MRAG_EPI_GELU_ERF) return gelu_erf_f(v);
  else if constexpr (EPI == MRAG_EPI_SILU) return silu_f(v);
  else return v;
}

// ---- host side

// the LDS-staged epilogues write (and read the residual in) whole 16-byte pieces of a row
inline bool rows_16B_aligned(const void* C, long long ldc, const void* resid, long long ldr) {
  return ldc % 8 == 0 && ((uintptr_t)C & 15) == 0 && (!resid || (ldr % 8 == 0 && ((uintptr_t)resid & 15) == 0));
}

// m-tiles per group of the logical tile order (gemm_tile, tile_coords): bits 8..15 of the tuning word, 4 unless set
inline int group_m_of(int tuning) { return ((tuning >> 8) & 0xff) ? ((tuning >> 8) & 0xff) : 4; }

// UNet widths are multiples of 320: N = 320 / 640 / 960 wastes 38 / 17 / 6 % of a 256-wide tile grid, nothing of a 320-wide one
inline bool wide_n_pays(long long N, int tuning = 0) {
  if (tuning & MRAG_GEMM_TUNE_NO_WIDE) return false;
  const long long w256 = (N + 255) / 256 * 256, w320 = (N + 319) / 320 * 320;
  return w320 * 100 < w256 * 90;                   // at least 10 % fewer padded columns
}

// Round quantisation (round 5, tools/unet_op_table.py): one workgroup per CU means a launch costs ceil(tiles / 256) ROUNDS of one tile's time, however full the
// last round is.  The UNets' level-2 problems (M = 16 128 rows, N = 1 280) are 63 x 5 = 315 tiles of 256x256 -- two rounds, the second 23 % full -- but
// 63 x 4 = 252 tiles of 256x320: ONE round of tiles 1.25x as long, 1.6x less time (the 3x3 convolutions at K = 11 520 .. 23 040 and the K = 5 120 FF2 ran at
// 0.30 of the MFMA peak there).  `rounds x tile width` prices a launch; the 320-wide tile is taken when it is at least 15 % cheaper (same bits: same K order).
inline long long round_cost(long long M, long long N, int BN) {
  const long long tiles = ((M + 255) / 256) * ((N + BN - 1) / BN);
  return ((tiles + 255) / 256) * BN;
}
// (tail_rect: the caller will run a small partial last round of the 256x256 grid as its own launch of 128x128 tiles -- plan_tail_rect -- which costs about half
// a round instead of a whole one)
inline bool wide_rounds_pay(long long M, long long N, int tuning = 0, bool tail_rect = false) {
  if (tuning & MRAG_GEMM_TUNE_NO_WIDE) return false;
  long long c256 = round_cost(M, N, 256);
  if (tail_rect) c256 = (((M + 255) / 256) * ((N + 255) / 256) / 256) * 256 + 128;
  return round_cost(M, N, 320) * 100 < c256 * 85;
}
// DynamiCrafter's level 2 (M = 18 432 rows, N = 1 280) is 72 x 5 = 360 tiles of 256x256 -- two rounds, the second 41 % full -- and 288 of 256x320 (two rounds
// of larger tiles: worse).  A 192-row tile (8 waves of 96 x 64; the generic K loop and the direct epilogue, ~8 % behind the pipelined 256x256 loop per FLOP)
// makes it 96 x 5 = 480 tiles: two nearly full rounds of tiles 3/4 the size.  Taken by the convolutions only (K = 3 840 .. 23 040: 626 -> 537 us at K = 11 520,
// 1 291 -> 1 000 us at K = 23 040, the (3,1,1) one 227 -> 178 us); a K = 5 120 LINEAR measured slower on it (259 vs 248 us on the persistent kernel: the
// direct epilogue's 8-byte stores), so linears keep their kernels.
inline bool short_rows_pay(long long M, long long N, int tuning = 0) {
  if (tuning & MRAG_GEMM_TUNE_NO_WIDE) return false;
  const long long t192 = ((M + 191) / 192) * ((N + 255) / 256), t256 = ((M + 255) / 256) * ((N + 255) / 256);
  const long long c192 = ((t192 + 255) / 256) * 192 * 108, c256 = ((t256 + 255) / 256) * 256 * 100;     // rounds x rows per tile x per-FLOP cost
  return c192 * 100 < c256 * 90 && round_cost(M, N, 320) * 100 >= round_cost(M, N, 256) * 85;
}

// the VAEs' finest levels are 128 channels wide: a 256-wide tile grid computes as many masked columns as real ones there
inline bool narrow_n_pays(long long N) {
  const long long r = N % 256;
  return r != 0 && r <= 128;
}

// Stream-K for the partial last round of the 256x256 tile grid (one workgroup per CU, 256 CUs).  The DiT's to_out / FF2 GEMMs are 1 668 tiles =
// 6.52 rounds: the seventh round runs 132 workgroups on 256 CUs for a whole tile's time.  Here the K-tiles of those `rem` tiles are dealt evenly to
// `units` workgroups (all co-resident: <= 256), so the round ends after rem / units of a tile's time plus the partial-sum exchange.
struct SkPlan {
  bool use = false;
  int n_main = 0, rem = 0, units = 0, maxparts = 0;
  size_t bytes = 0;
};
inline SkPlan plan_streamk(long long M, long long N, long long K) {
  SkPlan pl;
  const long long tiles = ((M + 255) / 256) * ((N + 255) / 256);
  const int nk = (int)(K / 64);
  if (tiles < SK_CUS || tiles > (1 << 24) || nk < 16 || nk > 4096) return pl;
  const int rem = (int)(tiles % SK_CUS);
  if (rem == 0 || rem > 208) return pl;           // a nearly full last round has nothing to win (the exchange costs ~15 us)
  pl.rem = rem; pl.n_main = (int)(tiles - rem);
  pl.units = rem * 4 < SK_CUS ? rem * 4 : SK_CUS;  // at most ~4 contributors per tile (+1 where a run straddles)
  const long long I = (long long)rem * nk;
  for (int t = 0, u = 0; t < rem; ++t) {           // contributors per tile: units meeting [t nk, (t + 1) nk)
    while ((long long)(u + 1) * I / pl.units <= (long long)t * nk) ++u;
    int v = u;
    while ((long long)(v + 1) * I / pl.units < (long long)(t + 1) * nk) ++v;
    pl.maxparts = pl.maxparts > v - u + 1 ? pl.maxparts : v - u + 1;
  }
  pl.bytes = SK_TICKET_BYTES + (size_t)rem * pl.maxparts * 256 * 256 * sizeof(float);
  pl.use = true;
  return pl;
}

// The persistent four-wave launch may run a SMALL partial last round as a rectangle of 128x128 tiles (plan_tail_rect, gemm_w4.hip), which changes what the
// 256x256 grid costs (wide_rounds_pay): the conditions that the dispatch and the plan share, on the count of 256x256 tiles
constexpr int W4_TAIL_MAX = 32;
inline bool tail_rect_wanted(long long tiles, int epi, int tuning) {
  const int rem = (int)(tiles % SK_CUS);
  return (tuning & MRAG_GEMM_TUNE_TAIL_RECT) && tiles >= 2 * SK_CUS && rem != 0 && rem <= W4_TAIL_MAX &&
         (epi == MRAG_EPI_NONE || epi == MRAG_EPI_GELU_TANH || epi == MRAG_EPI_RESID);   // (epilogues whose arithmetic does not depend on a row's absolute index)
}

// the tile shapes of launch_tiled
enum { TILE_256x256_W16, TILE_128x128, TILE_256x320, TILE_256x256 };

}  // namespace

// The family launchers, one per unit (MRAG_FAMILY_LAUNCHER, common.h: GemmP is part of their signatures).
MRAG_FAMILY_LAUNCHER launch_tiled(hipStream_t s, const GemmP& p, int epi, int tile, const SkPlan* sk);   // gemm_tiled.hip; sk: a stream-K plan (TILE_256x256 only) or null
MRAG_FAMILY_LAUNCHER launch_w4(hipStream_t s, const GemmP& p, int epi);                                  // gemm_w4.hip
MRAG_FAMILY_LAUNCHER launch_k320(hipStream_t s, const GemmP& p, int epi);                                // gemm_k320.hip
MRAG_FAMILY_LAUNCHER launch_skinny(hipStream_t s, const GemmP& p, int epi);                              // gemm_skinny.hip
