// attn_common.h -- what the attention units share: the launch parameters of the head_dim-64 kernels, the one check and fill of a mrag_attn_args block, the
// key-split plan of long launches and the launchers that cross units.  One unit per kernel family:
//   attn_bf16.hip       mrag_attn_fwd_bf16 (dispatch only), the key-split planner and the merge kernel of its partial results
//   attn16.hip          16x16x32 family: long unmasked sequences (the joint attention)
//   attn_flash.hip      32x32x16 family: short / masked / biased / cross-attention launches (its tile functions: attn_flash_tile.h)
//   attn_varlen.hip     the same tile functions over packed variable-length sequences (mrag_attn_varlen_fwd_bf16; its own parameter block)
//   attn_tiny.hip       one wavefront per (batch, head) for <= 16 x 16 (temporal attention of the UNets)
//   attn_fp8.hip        e4m3 operands (mrag_attn_fwd_fp8, mrag_attn_joint_fwd_fp8)
//   attn_small.hip      other head dims, short sequences, fp32 FMAs (mrag_attn_small_bf16; its own parameter block)
//   attn_hd.hip         other head dims at any length on the 32x32x16 MFMA (mrag_attn_hd_fwd_bf16; its own parameter block)
//   attn_ip_folded.hip  the folded motion-adapter branch (mrag_ip_attn_folded_bf16; scalar arguments, nothing from here but common.h)
#pragma once
#include "common.h"
#include "../../include/mrag_hip.h"

struct AttnP {
  const bf16_t* Q; const bf16_t* K; const bf16_t* V; bf16_t* O; const bf16_t* resid; const uint8_t* mask;
  long long q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss, v_sh, o_sb, o_ss;
  int B, H, Sq, Skv, kv_div, n_qtiles;
  float qscale, out_scale;
  // key-split tail (KVSPLIT instantiation): workgroups >= n_main own (b, h, chunk) of the ragged last query tile
  int n_main, kv_splits, chunk_keys, rem_rows, tile_rows;
  const float* bias; long long bias_sh;   // additive score bias [H, Sq, Skv] fp32 (head stride bias_sh) or null: the 32x32x16 kernel's mask path only
  float* part_o;    // [B*H*kv_splits, rem_rows, 64] unnormalised partial outputs
  float2* part_ml;  // [B*H*kv_splits, rem_rows] (running max in log2 units, row sum)
};

constexpr int KVB = 64;               // keys per K / V tile of the bf16 families (ring depths are per kernel)
constexpr int TILE_BYTES = KVB * 128; // one K (or V) tile
constexpr float kLog2e = 1.4426950408889634f;

// ---- the argument block every entry point takes (include/mrag_hip.h: mrag_attn_args).  An entry point calls the two checks around its own refusals, in the
// order that decides between MRAG_EINVAL and MRAG_ENOTSUP for it, then the fill.
static inline bool attn_args_present(const mrag_attn_args* a) {
  return a && a->Q && a->K && a->V && a->O && a->B > 0 && a->H > 0 && a->Sq > 0 && a->Skv > 0;
}
// 16-byte fragment / DMA loads of Q, K, V; O (and resid) by the width of the kernel's store: 8 bytes -> strides in multiples of 4, 16 -> of 8
static inline bool attn_args_aligned(const mrag_attn_args* a, int store_bytes) {
  if (((uintptr_t)a->Q | (uintptr_t)a->K | (uintptr_t)a->V) & 15) return false;
  if ((a->q_sb | a->q_ss | a->q_sh | a->k_sb | a->k_ss | a->k_sh | a->v_sb | a->v_ss | a->v_sh) % 8 != 0) return false;
  if (((uintptr_t)a->O & (store_bytes - 1)) || (a->o_sb | a->o_ss) % (store_bytes / 2) != 0) return false;
  return !(a->resid && ((uintptr_t)a->resid & (store_bytes - 1)));
}
// pointers, strides and sizes: the fields AttnP and attn_small.hip's SmallP share by name
template <class P>
static inline void attn_fill_views(P& p, const mrag_attn_args* a) {
  p.Q = (const bf16_t*)a->Q; p.K = (const bf16_t*)a->K; p.V = (const bf16_t*)a->V; p.O = (bf16_t*)a->O;
  p.q_sb = a->q_sb; p.q_ss = a->q_ss; p.q_sh = a->q_sh;
  p.k_sb = a->k_sb; p.k_ss = a->k_ss; p.k_sh = a->k_sh;
  p.v_sb = a->v_sb; p.v_ss = a->v_ss; p.v_sh = a->v_sh;
  p.o_sb = a->o_sb; p.o_ss = a->o_ss;
  p.B = a->B; p.H = a->H; p.Sq = a->Sq; p.Skv = a->Skv;
}
static inline void attn_fill(AttnP& p, const mrag_attn_args* a) {
  attn_fill_views(p, a);
  p.resid = (const bf16_t*)a->resid;
  p.kv_div = a->kv_batch_div;
  p.qscale = a->q_prescaled ? 1.0f : a->scale * kLog2e;   // q_prescaled: Q already carries scale * log2 e (the QKV GEMM's q_premul)
  p.out_scale = a->out_scale;
}

// ---- key-split tail of long launches (attn_bf16.hip: the plan and the merge kernel; both bf16 kernel families use them)
struct SplitPlan {
  int splits = 1, chunk_keys = 0, rem_rows = 0, n_full = 0;
  size_t bytes = 0;
};
__attribute__((visibility("hidden"))) SplitPlan mrag_plan_kv_split(int B, int H, int Sq, int Skv, int tile_rows, int slots);
MRAG_FAMILY_LAUNCHER mrag_launch_attn_combine(hipStream_t s, const AttnP& p);
// the split fields of a launch: full query tiles first, then (b, h, chunk) units of the ragged tile; partial outputs, then (max, sum) pairs in the workspace
static inline void attn_fill_split(AttnP& p, const SplitPlan& pl, void* workspace, int tile_rows) {
  const int nbh = p.B * p.H;
  p.n_qtiles = pl.n_full;
  p.n_main = pl.n_full * nbh;
  p.kv_splits = pl.splits; p.chunk_keys = pl.chunk_keys; p.rem_rows = pl.rem_rows; p.tile_rows = tile_rows;
  p.part_o = (float*)workspace;
  p.part_ml = (float2*)((char*)workspace + (size_t)nbh * pl.splits * pl.rem_rows * 64 * sizeof(float));
}

// attn16 workgroup shape: query blocks of 16 rows per wave (4 waves per workgroup).  3 -> 192-row workgroups, three per CU (168 VGPRs): shipped;
// 4 -> 256-row workgroups, two per CU (214 VGPRs): fewer K / V fragment bytes and barriers per FLOP.  With the optimistic sweep, QB = 4 is 2.6 % AHEAD
// at S = 17 776 in a cold interleaved microbenchmark (6.05 vs 6.22 ms, profiles/r4_attn_qb4_ab.txt) and 1.5 % BEHIND inside the denoise step, where the
// chip sits in its sustained power state (6.38 vs 6.28 ms per launch, 562 vs 560 ms per step on one box: profiles/r4_attn_step_ab.txt) -- the step is
// what ships, so 3 everywhere.
inline int mrag_attn16_qb(int /*Sq*/) { return 3; }
inline int mrag_attn16_rows(int qb) { return 64 * qb; }
inline int mrag_attn16_slots(int qb) { return (qb == 3 ? 3 : (qb == 2 ? 4 : 2)) * 256; }

// ---- the family launchers mrag_attn_fwd_bf16 dispatches to (MRAG_FAMILY_LAUNCHER, common.h: hidden, not part of the ABI)
// attn16.hip: long unmasked sequences (Sq > 128, Skv >= 256) on v_mfma_f32_16x16x32_bf16; returns MRAG_ENOTSUP for shapes it does not take
MRAG_FAMILY_LAUNCHER mrag_launch_attn16(hipStream_t s, AttnP p, const SplitPlan* pl, void* workspace, int qb);
// attn_flash.hip: nw = 1 / 2 / 8 waves of 32 query rows; short_kv: the one-tile instantiation (nw = 8 only); pl: a key-split plan for 256-row tiles (nw = 8,
// unmasked, with its workspace) or null
MRAG_FAMILY_LAUNCHER mrag_launch_attn_flash(hipStream_t s, const AttnP& p, int nw, bool short_kv, const SplitPlan* pl, void* workspace);
// attn_tiny.hip: Sq, Skv <= 16, no mask / bias / resid
MRAG_FAMILY_LAUNCHER mrag_launch_attn_tiny(hipStream_t s, const AttnP& p);

// ---- device helpers
// v_max3_f32 through asm: plain fmaxf() on MFMA outputs makes hipcc emit a canonicalising v_max per operand
__device__ __forceinline__ float max3_asm(float a, float b, float c) {
  float d;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
