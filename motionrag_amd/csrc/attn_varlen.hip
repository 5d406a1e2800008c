// attn_varlen.hip -- packed variable-length attention at head dim 64, bf16 (mrag_attn_varlen_fwd_bf16, include/mrag_hip.h): sequence i owns rows
// [cu_seqlens[i], cu_seqlens[i + 1]) of packed Q / K / V / O row matrices and attends to itself only,
//
//   O[s_i:e_i] = softmax(scale . Q[s_i:e_i] K[s_i:e_i]^T) V[s_i:e_i]      per head.
//
// The text side of the retrieval row (text_embedder.py) embeds captions of 5 to 100 and more tokens: with this entry one forward pass takes a whole chunk of them
// as one [T, hidden] row matrix instead of one pass per distinct token count.
//
// The kernel is attn_fwd_kernel (attn_flash.hip) with (Sq, Skv, row base) read from cu_seqlens[seq] instead of the launch arguments: the same tile functions
// (attn_flash_tile.h: qk_tile, softmax_tile<false>, pv_tile), the same LDS ring fed by 16-byte LDS-DMA, the same counted vmcnt + raw barrier.  What it does not
// carry: mask / bias, residual, key-split units, the XCD-aware block order (a caption's K / V are a few KB) and the NS-unrolled immediate-stage loop (that one is
// for eight-wave workgroups over long key sets).
//   * grid = (ceil(max_seqlen / 64), H, B): workgroup (qt, h, seq) owns query rows [64 qt, 64 qt + 64) of sequence seq, 32 per wave (NW = 2).  Captions are
//     short: 64-row workgroups cover most sequences in one workgroup whose two waves share one K / V stream; 32-row workgroups (NW = 1) would read K / V
//     twice for every sequence of 33 to 64 tokens and leave each DMA tile to a single wave (8 pieces per operand instead of 4).
//   * early exit: a workgroup whose first query row is at or beyond its sequence's length (a zero-length sequence included) returns before its first DMA
//     and its first barrier.  The condition depends on (blockIdx, cu_seqlens) only, so it is workgroup-uniform: no wave waits at a barrier others never reach.
//   * key range: every K / V read stays inside [s_i, e_i).  len < 64: the per-lane clamped DMA (rows past the end re-read row len - 1, their scores are
//     masked); len >= 64 with len % 64 != 0: the last tile is slid back to [len - 64, len) and the keys it repeats are masked; len = 1: every lane reads row 0
//     of the sequence.  Prefetches past the last tile re-read the last tile.  Q rows past the end of the sequence clamp to its last row and are not stored.
//   * the row base s_i and the length are scalar (one s_load per workgroup); the 64-bit products s_i * stride are scalar arithmetic.
#include "attn_flash_tile.h"

namespace {

unsigned long long g_attn_varlen_launches[1];

struct VarlenP {
  const bf16_t* Q; const bf16_t* K; const bf16_t* V; bf16_t* O; const int* cu;
  long long q_ss, q_sh, k_ss, k_sh, v_ss, v_sh, o_ss;
  int B, H, total_rows;
  float qscale;
};

template <int NW>
__global__ __launch_bounds__(NW * 64, 1) void attn_varlen_kernel(const VarlenP p) {
  constexpr int PPW = 8 / NW;  // 1 KiB DMA pieces per wave per K (or V) tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int seq = blockIdx.z, h = blockIdx.y, qt = blockIdx.x;
  // ---- this workgroup's sequence: rows [row0, row0 + len) of the packed buffers.  A cu_seqlens that is not what the header asks for (decreasing, negative,
  // past total_rows) makes the workgroup return: no row outside [0, total_rows) is ever addressed.
  const int row0 = __builtin_amdgcn_readfirstlane(p.cu[seq]);
  const int len = __builtin_amdgcn_readfirstlane(p.cu[seq + 1]) - row0;
  if (row0 < 0 || len <= 0 || len > p.total_rows - row0 || qt * (NW * 32) >= len) return;   // workgroup-uniform, before the first DMA and barrier

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform: scalar branches, SGPR LDS bases
  const int r32 = lane & 31;
  Lane ln;
  ln.hh = lane >> 5;
  ln.head = h;
  const int skv = len;

  const int q0 = qt * (NW * 32) + wave * 32;
  const bool wave_active = q0 < len;
  const int qrow = q0 + r32;
  const int qrow_c = qrow < len ? qrow : len - 1;

  // ---- Q fragments: B operand of S^T = K.Q^T : lane holds Q[q = lane&31][d = 16 ks + 8 hh + j]
  bf16x8 qf[4];
  {
    const bf16_t* qp = p.Q + (long long)row0 * p.q_ss + (long long)qrow_c * p.q_ss + (long long)h * p.q_sh + ln.hh * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const u32x4 raw = *(const u32x4*)(qp + ks * 16);
      qf[ks] = p.qscale == 1.0f ? __builtin_bit_cast(bf16x8, raw) : scale_frag(raw, p.qscale);
    }
  }

  // ---- LDS-DMA staging: piece = 8 keys x 128 B; lane i -> key (i >> 3), 16-byte position (i & 7)
  const bf16_t* kbase = p.K + (long long)row0 * p.k_ss + (long long)h * p.k_sh;
  const bf16_t* vbase = p.V + (long long)row0 * p.v_ss + (long long)h * p.v_sh;
  const int prow = lane >> 3, ppos = lane & 7;
  unsigned k_loff[PPW], v_loff[PPW];   // loop-invariant per-lane byte offsets inside a tile (source-side swizzles folded in)
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int kit = ((wave + i * NW) & 7) * 8 + prow;
    k_loff[i] = (unsigned)(kit * p.k_ss + (ppos ^ ((kit >> 1) & 7)) * 8) * 2u;
    v_loff[i] = (unsigned)(kit * p.v_ss + (ppos ^ (((kit >> 1) & 1) << 2)) * 8) * 2u;
  }
  // the two DMA forms of attn_fwd_kernel: whole in-range tiles (the last one slid back) for len >= 64, per-lane clamped rows below
  const int last_start = skv - KVB;
  const unsigned lds0 = (unsigned)(size_t)smem;
  auto issue_k = [&](int stage, int t) {
    if (last_start >= 0) {
      const int start = t * KVB < last_start ? t * KVB : last_start;
      const char* tile = (const char*)kbase + (long long)start * p.k_ss * 2;
#pragma unroll
      for (int i = 0; i < PPW; ++i) glds16_sbase(tile, k_loff[i], lds0 + stage * TILE_BYTES + ((wave + i * NW) & 7) * 1024);
    } else {
#pragma unroll
      for (int i = 0; i < PPW; ++i) {
        const int piece = (wave + i * NW) & 7;
        const int kit = piece * 8 + prow;
        const int key = kit < skv ? kit : skv - 1;  // rows past the end re-read a valid row; their scores are masked
        glds16(kbase + (long long)key * p.k_ss + (ppos ^ ((kit >> 1) & 7)) * 8, smem + stage * TILE_BYTES + piece * 1024);
      }
    }
  };
  auto issue_v = [&](int stage, int t) {
    if (last_start >= 0) {
      const int start = t * KVB < last_start ? t * KVB : last_start;
      const char* tile = (const char*)vbase + (long long)start * p.v_ss * 2;
#pragma unroll
      for (int i = 0; i < PPW; ++i) glds16_sbase(tile, v_loff[i], lds0 + V_BASE + stage * TILE_BYTES + ((wave + i * NW) & 7) * 1024);
    } else {
#pragma unroll
      for (int i = 0; i < PPW; ++i) {
        const int piece = (wave + i * NW) & 7;
        const int kit = piece * 8 + prow;
        const int key = kit < skv ? kit : skv - 1;
        glds16(vbase + (long long)key * p.v_ss + (ppos ^ (((kit >> 1) & 1) << 2)) * 8, smem + V_BASE + stage * TILE_BYTES + piece * 1024);
      }
    }
  };

  // ---- fragment read addresses (bytes, relative to the tile base): attn_fwd_kernel's
  ln.k_row_off = r32 * 128;
  ln.k_swz = (r32 >> 1) & 7;
  const int g16 = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
  ln.v_lane_off = (4 * ln.hh + q4) * 128 + (g16 & 1) * 32 + p4 * 8;
  ln.v_half0 = (q4 >> 1) * 64;
  ln.v_half1 = (1 - (q4 >> 1)) * 64;
#pragma unroll
  for (int c = 0; c < 4; ++c) ln.kb[c] = 0;   // (the immediate-stage tile forms are not used here)
  ln.vc0 = ln.vc1 = 0;

  Run r;
#pragma unroll
  for (int i = 0; i < 16; ++i) { r.o0[i] = 0.f; r.o1[i] = 0.f; r.negm[i] = 0.f; r.lacc[i] = 0.f; }
  r.m = 0.f;

  // ---- main loop: attn_fwd_kernel's ring (DMA D = NS - 1 tiles ahead, retired by a counted vmcnt + a raw s_barrier); every wave of the workgroup
  // runs the same nt iterations, so every barrier is reached by all of them
  const int nt = (skv + KVB - 1) / KVB;
  constexpr int D = NS - 1;
  const AttnP none{};   // softmax_tile<false> reads nothing of it
#pragma unroll
  for (int i = 0; i < D; ++i) { issue_k(i, i); issue_v(i, i); }
  for (int t = 0; t < nt; ++t) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PPW * (D - 1)) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    auto early_issue = [&]() { issue_k((t + D) % NS, t + D); issue_v((t + D) % NS, t + D); };
    if (!wave_active) { early_issue(); continue; }
    f32x16 s0, s1;
    bf16x8 pb[4];
    qk_tile(smem + (t % NS) * TILE_BYTES, ln, qf, r.negm, s0, s1, early_issue);
    softmax_tile<false>(none, skv, ln, t, nt, qrow_c, s0, s1, r, pb);
    pv_tile(smem + V_BASE + (t % NS) * TILE_BYTES, ln, pb, r.o0, r.o1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // retire the clamped tail DMAs before the LDS is released

  if (!wave_active || qrow >= len) return;
  // ---- epilogue: the two half-waves' row sums (each over its own keys) are added, then normalise
  {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(r.lacc[0]), __float_as_uint(r.lacc[0]), false, false);
    r.lacc[0] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
  }
  const float inv = 1.0f / r.lacc[0];
  bf16_t* orow = p.O + (long long)row0 * p.o_ss + (long long)qrow * p.o_ss + h * 64 + 4 * ln.hh;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (dt ? r.o1[4 * g + e] : r.o0[4 * g + e]) * inv;
      u32x2 out;
      out[0] = pack_bf2(v[0], v[1]);
      out[1] = pack_bf2(v[2], v[3]);
      *(u32x2*)(orow + dt * 32 + 8 * g) = out;
    }
  }
}

// ---- the argument block (include/mrag_hip.h: mrag_attn_varlen_args), checked in the form of attn_common.h's attn_args_present / attn_args_aligned
inline bool varlen_args_present(const mrag_attn_varlen_args* a) {
  return a && a->Q && a->K && a->V && a->O && a->cu_seqlens && a->B > 0 && a->H > 0 && a->max_seqlen > 0;
}
// 16-byte fragment / DMA loads of Q, K, V; 8-byte stores of O; 4-byte reads of cu_seqlens
inline bool varlen_args_aligned(const mrag_attn_varlen_args* a) {
  if (((uintptr_t)a->Q | (uintptr_t)a->K | (uintptr_t)a->V) & 15) return false;
  if ((a->q_ss | a->q_sh | a->k_ss | a->k_sh | a->v_ss | a->v_sh) % 8 != 0) return false;
  if (((uintptr_t)a->O & 7) || a->o_ss % 4 != 0) return false;
  return ((uintptr_t)a->cu_seqlens & 3) == 0;
}

}  // namespace

extern "C" int mrag_attn_varlen_launch_counts(uint64_t* out_host, int32_t n) {
  for (int i = 0; out_host && i < n && i < 1; ++i) out_host[i] = __atomic_load_n(&g_attn_varlen_launches[i], __ATOMIC_RELAXED);
  return 1;
}

extern "C" int mrag_attn_varlen_fwd_bf16(void* stream, const mrag_attn_varlen_args* a) {
  constexpr int NW = 2;
  if (!varlen_args_present(a) || a->max_seqlen > a->total_rows) return MRAG_EINVAL;
  if (!varlen_args_aligned(a)) return MRAG_EINVAL;
  // the scalar-base LDS-DMA path folds a tile's per-lane K / V offsets (up to 63 rows) into 32-bit unsigned byte offsets (as mrag_attn_fwd_bf16)
  if (a->k_ss < 0 || a->v_ss < 0 || a->k_ss > 0x1ffffff || a->v_ss > 0x1ffffff) return MRAG_ENOTSUP;
  if (a->H > 65535 || a->B > 65535) return MRAG_ENOTSUP;   // grid dimensions y and z
  VarlenP p{};
  p.Q = (const bf16_t*)a->Q; p.K = (const bf16_t*)a->K; p.V = (const bf16_t*)a->V; p.O = (bf16_t*)a->O; p.cu = a->cu_seqlens;
  p.q_ss = a->q_ss; p.q_sh = a->q_sh; p.k_ss = a->k_ss; p.k_sh = a->k_sh; p.v_ss = a->v_ss; p.v_sh = a->v_sh; p.o_ss = a->o_ss;
  p.B = a->B; p.H = a->H; p.total_rows = a->total_rows;
  p.qscale = a->scale * kLog2e;
  const dim3 grid((unsigned)((a->max_seqlen + NW * 32 - 1) / (NW * 32)), (unsigned)a->H, (unsigned)a->B), block(NW * 64);
  const int rc = launch_dyn_lds(attn_varlen_kernel<NW>, grid, block, (size_t)2 * NS * TILE_BYTES, (hipStream_t)stream, p);
  if (rc != MRAG_OK) return rc;
  (void)__atomic_fetch_add(&g_attn_varlen_launches[0], 1ull, __ATOMIC_RELAXED);
  return MRAG_OK;
}
