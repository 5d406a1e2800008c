// attn_bf16.hip -- O[b, q, h, :] = resid + out_scale * softmax(Q K^T * scale  [masked, + bias])  V at head dim 64, bf16: the entry point behind every
// F.scaled_dot_product_attention call site of the MotionRAG hot path (see include/mrag_hip.h).  Dispatch only: which kernel family takes a call (attn_common.h
// lists them, one per unit) -- and what the two long-sequence families share, the key-split plan of a launch's ragged last query tile and the kernel that
// merges its partial results.
#include "attn_common.h"

// ---------------------------------------------------------------------------------------------- key-split tail
// Long-sequence launches are many rounds of 512 resident workgroups (2 per CU) and the LAST round is what the ragged query tile of each
// (b, h) pair leaves: B*H workgroups that each scan ALL keys for Sq % 256 rows.  At the BASELINE shape (B*H = 96, Sq = 17 776 =
// 69 x 256 + 112) those 96 workgroups are 1.4 % of the launch's work and 4 % of its time (tools/tail_probe.py: 7.33 ms for the 6624
// full tiles, 7.63 ms with the ragged ones).  Splitting THEIR keys into `kv_splits` chunks turns the 96 long stragglers into ~512 short
// workgroups that drain into the slots the last full round frees; each leaves (unnormalised O, running max, row sum) in a caller-provided
// workspace and attn_combine_kernel merges the chunks, applies out_scale / resid and writes bf16 -- the same online-softmax algebra as
// between two key tiles, carried through HBM instead of registers.
SplitPlan mrag_plan_kv_split(int B, int H, int Sq, int Skv, int tile_rows, int slots) {
  // tile_rows: query rows per workgroup (256: attn_flash.hip; 192: attn16.hip); slots: workgroups resident on the chip (2 or 3 per CU)
  SplitPlan pl;
  const int rem = Sq % tile_rows, n_full = Sq / tile_rows, nt = (Skv + KVB - 1) / KVB;
  const long long nbh = (long long)B * H;
  int want = (int)(slots / nbh);
  if (want > 8) want = 8;
  if (rem == 0 || nbh * n_full < 1024 || want < 2 || nt < 8 * want) return pl;
  const int tpc = (nt + want - 1) / want;
  const int chunk = tpc * KVB, splits = (Skv + chunk - 1) / chunk;
  if (splits < 2 || Skv - (splits - 1) * chunk < KVB) return pl;       // every chunk must hold one whole (slid-back) tile
  pl.splits = splits; pl.chunk_keys = chunk; pl.rem_rows = rem; pl.n_full = n_full;
  pl.bytes = (size_t)nbh * splits * rem * (64 * sizeof(float) + sizeof(float2));
  return pl;
}

namespace {

__global__ __launch_bounds__(256) void attn_combine_kernel(const AttnP p) {
  const long long idx = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);   // (b*H + h, row of the ragged tile); 16 lanes x 4 columns per row
  if (idx >= (long long)p.B * p.H * p.rem_rows) return;
  const int bh = (int)(idx / p.rem_rows), row = (int)(idx % p.rem_rows), d = (threadIdx.x & 15) * 4;
  const long long u0 = (long long)bh * p.kv_splits;
  float M = -INFINITY;
  for (int c = 0; c < p.kv_splits; ++c) M = fmaxf(M, p.part_ml[(u0 + c) * p.rem_rows + row].x);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float l = 0.f;
  for (int c = 0; c < p.kv_splits; ++c) {
    const long long pr = (u0 + c) * p.rem_rows + row;
    const float2 ml = p.part_ml[pr];
    const float w = __builtin_amdgcn_exp2f(ml.x - M);
    l += w * ml.y;
    acc += *(const f32x4*)(p.part_o + pr * 64 + d) * w;
  }
  const float inv = p.out_scale / l;
  const int b = bh / p.H, h = bh % p.H;
  const long long off = (long long)b * p.o_sb + (long long)(p.n_qtiles * p.tile_rows + row) * p.o_ss + h * 64 + d;
  float v[4] = {acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv};
  if (p.resid) {
    const u32x2 rr = *(const u32x2*)(p.resid + off);
    v[0] += __uint_as_float(rr[0] << 16); v[1] += __uint_as_float(rr[0] & 0xffff0000u);
    v[2] += __uint_as_float(rr[1] << 16); v[3] += __uint_as_float(rr[1] & 0xffff0000u);
  }
  u32x2 out;
  out[0] = pack_bf2(v[0], v[1]);
  out[1] = pack_bf2(v[2], v[3]);
  *(u32x2*)(p.O + off) = out;
}

}  // namespace

MRAG_FAMILY_LAUNCHER mrag_launch_attn_combine(hipStream_t s, const AttnP& p) {
  MRAG_LAUNCH(attn_combine_kernel, dim3((unsigned)(((long long)p.B * p.H * p.rem_rows + 15) / 16)), dim3(256), 0, s, p);
  MRAG_LAUNCH_CHECK();
  MRAG_COUNT(MRAG_K_ATTN_COMBINE);
  return MRAG_OK;
}

extern "C" int64_t mrag_attn_workspace_bytes(int32_t B, int32_t H, int32_t Sq, int32_t Skv) {
  if (B <= 0 || H <= 0 || Sq <= 0 || Skv <= 0) return 0;
  const size_t a = mrag_plan_kv_split(B, H, Sq, Skv, 256, 512).bytes, b = mrag_plan_kv_split(B, H, Sq, Skv, mrag_attn16_rows(mrag_attn16_qb(Sq)), mrag_attn16_slots(mrag_attn16_qb(Sq))).bytes;
  return (int64_t)(a > b ? a : b);      // either kernel family's tail plan fits
}

extern "C" int mrag_attn_fwd_bf16(void* stream, const mrag_attn_args* a) {
  if (!attn_args_present(a) || a->kv_batch_div <= 0 || a->B % a->kv_batch_div != 0) return MRAG_EINVAL;
  if (!attn_args_aligned(a, 8)) return MRAG_EINVAL;
  // the scalar-base LDS-DMA path folds a tile's per-lane K / V offsets (up to 63 rows) into 32-bit unsigned byte offsets
  if (a->k_ss < 0 || a->v_ss < 0 || a->k_ss > 0x1ffffff || a->v_ss > 0x1ffffff) return MRAG_ENOTSUP;
  if (a->bias && (((uintptr_t)a->bias & 3) || a->bias_sh < 0)) return MRAG_EINVAL;
  AttnP p{};
  attn_fill(p, a);
  p.mask = a->mask; p.bias = a->bias; p.bias_sh = a->bias_sh;
  const bool masked = a->mask || a->bias;   // either one takes the 32x32x16 kernel's per-score path
  hipStream_t s = (hipStream_t)stream;
  if (a->Sq <= 16 && a->Skv <= 16 && !masked && !a->resid && !(a->tuning & MRAG_ATTN_TUNE_NO_TINY)) return mrag_launch_attn_tiny(s, p);   // temporal attention of the UNets
  if (a->Sq > 128 && a->Skv <= KVB) return mrag_launch_attn_flash(s, p, 8, true, nullptr, nullptr);
  const bool legacy = (a->tuning & MRAG_ATTN_TUNE_LEGACY) != 0;
  const bool may_split = a->Sq > 128 && !masked && a->workspace;   // key-split tail for the ragged last query tile (mrag_plan_kv_split)
  if (may_split && ((uintptr_t)a->workspace & 15) != 0) return MRAG_EINVAL;
  if (a->Sq > 128 && !masked && !legacy) {        // long unmasked sequences: the 16x16x32 family (attn16.hip), 192-row workgroups
    SplitPlan pl;
    bool split = false;
    if (may_split) {
      pl = mrag_plan_kv_split(a->B, a->H, a->Sq, a->Skv, mrag_attn16_rows(mrag_attn16_qb(a->Sq)), mrag_attn16_slots(mrag_attn16_qb(a->Sq)));
      split = pl.splits > 1 && a->workspace_bytes >= (int64_t)pl.bytes;
    }
    const int rc = mrag_launch_attn16(s, p, split ? &pl : nullptr, a->workspace, mrag_attn16_qb(a->Sq));
    if (rc != MRAG_ENOTSUP) return rc;
  }
  if (may_split) {
    const SplitPlan pl = mrag_plan_kv_split(a->B, a->H, a->Sq, a->Skv, 256, 512);
    if (pl.splits > 1 && a->workspace_bytes >= (int64_t)pl.bytes) return mrag_launch_attn_flash(s, p, 8, false, &pl, a->workspace);
  }
  return mrag_launch_attn_flash(s, p, a->Sq > 128 ? 8 : (a->Sq > 32 ? 2 : 1), false, nullptr, nullptr);
}
