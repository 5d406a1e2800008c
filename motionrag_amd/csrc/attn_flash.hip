// attn_flash.hip -- head_dim-64 bf16 attention forward on v_mfma_f32_32x32x16_bf16 (flash-style, online softmax): attn_fwd_kernel and its launcher.
//
//   O[b, q, h, :] = resid + out_scale * softmax(Q K^T * scale  [masked, + bias])  V
//
// mrag_attn_fwd_bf16 (attn_bf16.hip) sends here what the other families do not take: short and cross-attention launches (the 25-key motion ("ip")
// cross-attention with its fused `hidden + scale * ip` update, the Perceiver resampler's 25 queries x 1 593 keys), everything with a byte mask or a score
// bias (the block-causal CAMA encoder, T5), and long unmasked sequences when the 16x16x32 family (attn16.hip) is switched off or refuses.
//
// CDNA4 design:
//   * v_mfma_f32_32x32x16_bf16 with SWAPPED products: S^T = K . Q^T and O^T = V^T . P^T, so a lane
//     owns one query row -- row max / row sum are lane-local plus one v_permlane32_swap, and the S
//     accumulator registers are already the B operand of the PV product (no LDS round trip for P);
//   * each wave owns 32 query rows (Q fragments live in registers, pre-multiplied by
//     scale*log2 e so the softmax is a bare v_exp_f32); a workgroup is NW waves;
//   * K/V tiles of 64 keys are staged by 16-byte LDS-DMA (global_load_lds) into two K stages and two
//     V stages; K is XOR-swizzled on the source side for conflict-free ds_read_b128, V keeps
//     row-major [key][d] with its 64-byte halves swapped on odd key pairs and is consumed through
//     ds_read_b64_tr_b16 (hardware transpose) as the A operand of O^T = V^T . P^T;
//   * variants retired by measurement (round 3 pruned their code; numbers in DESIGN.md section 3): the intra-wave software-pipelined tile
//     (9.9 vs 8.7 ms at S = 17 776), 4-wave workgroups for long sequences, packed fp32 adds, per-32-key-block softmax + PV, static priorities
//     for the younger half, a half-tile stagger of the two halves, vector-pipe max subtraction, f32-add row sums;
//   * the running max is carried as the MFMA's C operand (S' = K.Q^T - m comes out of the chain,
//     no per-score subtract) and only moved when a tile raises it by more than THR (deferred
//     rescale): the rare path rescales O, l, the pending S' and the prefetched S' together;
//   * grid = q-tiles x (b, h) with an XCD-aware order: all q-tiles of one (b, h) run on one XCD,
//     so its K/V (4.5 MB at S = 17 776) streams from that XCD's L2.
#include "attn_flash_tile.h"   // qk_tile, softmax_tile, pv_tile and the ring constants: shared with attn_varlen.hip

namespace {

// SHORTKV: key sets of at most one tile (motion tokens, text, temporal frames) -- same code, no barrier stagger; a separate
// instantiation so that profiles list the HBM-bound small-KV launches apart from the MFMA-bound long-sequence ones.
// KVSPLIT: the launch's last workgroups (blockIdx >= n_main) each scan ONE CHUNK of the keys for the ragged last query tile of a
// (b, h) pair and leave (unnormalised O, running max, row sum) in the workspace for attn_combine_kernel (attn_bf16.hip) -- see launch_attn_split.
template <int NW, bool HAS_MASK, bool SHORTKV = false, bool KVSPLIT = false>
__global__ __launch_bounds__(NW * 64, (NW == 8 && !HAS_MASK) ? 4 : 1) void attn_fwd_kernel(const AttnP p) {
  constexpr int PPW = NW >= 8 ? 1 : 8 / NW;  // 1 KiB DMA pieces per wave per K (or V) tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform: scalar branches, SGPR LDS bases
  const int r32 = lane & 31;
  Lane ln;
  ln.hh = lane >> 5;

  // ---- XCD-aware block -> (q-tile, b, h)
  const int nbh = p.B * p.H;
  int bh, qt;
  int skv = p.Skv, key0 = 0;          // keys this workgroup scans: [key0, key0 + skv)
  bool split_unit = false;
  if (KVSPLIT && (int)blockIdx.x >= p.n_main) {
    const int u = blockIdx.x - p.n_main;
    bh = u / p.kv_splits;
    qt = p.n_qtiles;                  // the ragged tile after the n_qtiles full ones
    key0 = (u % p.kv_splits) * p.chunk_keys;
    skv = p.Skv - key0 < p.chunk_keys ? p.Skv - key0 : p.chunk_keys;
    split_unit = true;
  } else if ((nbh & 7) == 0) {
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
    bh = (j / p.n_qtiles) * 8 + x;
    qt = j % p.n_qtiles;
  } else {
    bh = blockIdx.x / p.n_qtiles;
    qt = blockIdx.x % p.n_qtiles;
  }
  const int b = bh / p.H, h = bh % p.H;
  const int bkv = b / p.kv_div;
  ln.head = h;

  const int q0 = qt * (NW * 32) + wave * 32;
  const bool wave_active = q0 < p.Sq;
  const int qrow = q0 + r32;
  const int qrow_c = qrow < p.Sq ? qrow : p.Sq - 1;

  // ---- Q fragments: B operand of S^T = K.Q^T : lane holds Q[q = lane&31][d = 16 ks + 8 hh + j]
  bf16x8 qf[4];
  {
    const bf16_t* qp = p.Q + (long long)b * p.q_sb + (long long)qrow_c * p.q_ss + (long long)h * p.q_sh + ln.hh * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const u32x4 raw = *(const u32x4*)(qp + ks * 16);
      qf[ks] = p.qscale == 1.0f ? __builtin_bit_cast(bf16x8, raw) : scale_frag(raw, p.qscale);
    }
  }

  // ---- LDS-DMA staging: piece = 8 keys x 128 B; lane i -> key (i >> 3), 16-byte position (i & 7)
  const bf16_t* kbase = p.K + (long long)bkv * p.k_sb + (long long)h * p.k_sh + (long long)key0 * p.k_ss;
  const bf16_t* vbase = p.V + (long long)bkv * p.v_sb + (long long)h * p.v_sh + (long long)key0 * p.v_ss;
  const int prow = lane >> 3, ppos = lane & 7;
  unsigned k_loff[PPW], v_loff[PPW];   // loop-invariant per-lane byte offsets inside a tile (source-side swizzles folded in)
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int kit = ((wave + i * NW) & 7) * 8 + prow;
    k_loff[i] = (unsigned)(kit * p.k_ss + (ppos ^ ((kit >> 1) & 7)) * 8) * 2u;
    v_loff[i] = (unsigned)(kit * p.v_ss + (ppos ^ (((kit >> 1) & 1) << 2)) * 8) * 2u;
  }
  // A partial last tile is SLID BACK to keys [Skv-64, Skv) (its already-seen keys are masked in softmax_tile), and prefetches past
  // the end re-read that tile: every DMA of a >= 64-key sequence is a full in-range tile -> scalar tile base + loop-invariant
  // per-lane offset, no per-lane clamping (no 64-bit lane arithmetic, nothing to spill).  Shorter key sets clamp rows instead.
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

  // ---- fragment read addresses (bytes, relative to the tile base)
  // K (A operand of K.Q^T): lane reads row key = kb*32 + r32, 16-byte chunk (2 ks + hh) ^ ((key>>1)&7)
  ln.k_row_off = r32 * 128;
  ln.k_swz = (r32 >> 1) & 7;
  // V^T (A operand of V^T.P^T) through ds_read_b64_tr_b16: lane 4q+p of a 16-lane group supplies the address of
  // key row (k0 + q), columns 4p..4p+3 of the block; it receives column (lane & 15).
  const int g16 = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
  ln.v_lane_off = (4 * ln.hh + q4) * 128 + (g16 & 1) * 32 + p4 * 8;
  ln.v_half0 = (q4 >> 1) * 64;        // d-tile 0: 64-byte half index 0 ^ ((key >> 1) & 1)
  ln.v_half1 = (1 - (q4 >> 1)) * 64;  // d-tile 1
  {
    const unsigned kbase = (unsigned)(size_t)(smem + ln.k_row_off);
#pragma unroll
    for (int c = 0; c < 4; ++c) ln.kb[c] = kbase + ((2 * c + ln.hh) ^ ln.k_swz) * 16;
    ln.vc0 = (unsigned)(size_t)(smem + NS * TILE_BYTES + ln.v_lane_off + ln.v_half0);
    ln.vc1 = (unsigned)(size_t)(smem + NS * TILE_BYTES + ln.v_lane_off + ln.v_half1);
  }

  Run r;
#pragma unroll
  for (int i = 0; i < 16; ++i) { r.o0[i] = 0.f; r.o1[i] = 0.f; r.negm[i] = 0.f; r.lacc[i] = 0.f; }
  r.m = 0.f;

  // ---- main loop.  K and V each own a ring of NS stages; the DMA runs D = NS-1 tiles ahead of the compute and is
  // retired by a COUNTED vmcnt (every wave issues exactly 2*PPW DMA instructions per tile pair, tiles past the end
  // re-read clamped rows so the count never changes) + a raw s_barrier: __syncthreads() would drain the queue.
  const int nt = (skv + KVB - 1) / KVB;
  constexpr int D = NS - 1;   // without the half-tile stagger the stage refilled after barrier #t is the one read in iteration t-1
  auto wait_pair = [&]() {   // all but the (D-1) youngest tile pairs of this wave have landed; then rendezvous
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PPW * (D - 1)) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  {
    // iteration t reads K(t), V(t) from stage t % NS.  Barrier #t guarantees tile t has landed for every wave; after it each
    // wave issues tile t + D into the stage of tile t - 1, which every wave has finished reading (ring of NS = D + 1).  All waves of
    // the workgroup run in step.
#pragma unroll
    for (int i = 0; i < D; ++i) { issue_k(i, i); issue_v(i, i); }
    auto iter = [&](int t, auto stage_c) {
      constexpr int STG = decltype(stage_c)::value;   // ring stage as a compile-time constant, or -1
      wait_pair();   // barrier #t
      auto early_issue = [&]() { issue_k((t + D) % NS, t + D); issue_v((t + D) % NS, t + D); };
      if (!wave_active) { early_issue(); return; }
      f32x16 s0, s1;
      bf16x8 pb[4];
      if constexpr (STG >= 0) qk_tile_imm8<STG>(ln, qf, r.negm, s0, s1, early_issue);
      else qk_tile(smem + (t % NS) * TILE_BYTES, ln, qf, r.negm, s0, s1, early_issue);
      softmax_tile<HAS_MASK>(p, skv, ln, t, nt, qrow_c, s0, s1, r, pb);
      if constexpr (STG >= 0) pv_tile_imm<STG>(ln, pb, r.o0, r.o1);
      else pv_tile(smem + V_BASE + (t % NS) * TILE_BYTES, ln, pb, r.o0, r.o1);
    };
    using RT = std::integral_constant<int, -1>;
    int t = 0;
    if constexpr (NS == 4 && NW == 8 && !HAS_MASK && !SHORTKV) {
      // unrolled by the ring depth: stage = t % NS is an immediate (t starts at 0 and advances by NS)
      for (; t + NS <= nt; t += NS) {
        iter(t, std::integral_constant<int, 0>{});
        iter(t + 1, std::integral_constant<int, 1>{});
        iter(t + 2, std::integral_constant<int, 2>{});
        iter(t + 3, std::integral_constant<int, 3>{});
      }
    }
    for (; t < nt; ++t) iter(t, RT{});   // the tiles left over, and every other instantiation: the stage from t % NS
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // retire the clamped tail DMAs before the LDS is released

  if (!wave_active) return;
  // ---- epilogue: the two half-waves' row sums (each over its own keys) are added, then normalise; fused residual
  if (qrow >= p.Sq) return;
  {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(r.lacc[0]), __float_as_uint(r.lacc[0]), false, false);
    r.lacc[0] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
  }
  if (KVSPLIT && split_unit) {   // partial result of this key chunk; attn_combine_kernel merges the chunks
    const long long prow_i = (long long)(blockIdx.x - p.n_main) * p.rem_rows + wave * 32 + r32;
    float* po = p.part_o + prow_i * 64 + 4 * ln.hh;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 v = dt ? f32x4{r.o1[4 * g], r.o1[4 * g + 1], r.o1[4 * g + 2], r.o1[4 * g + 3]}
                           : f32x4{r.o0[4 * g], r.o0[4 * g + 1], r.o0[4 * g + 2], r.o0[4 * g + 3]};
        *(f32x4*)(po + dt * 32 + 8 * g) = v;
      }
    }
    if (ln.hh == 0) p.part_ml[prow_i] = make_float2(r.m, r.lacc[0]);
    return;
  }
  const float inv = p.out_scale / r.lacc[0];
  const long long obase = (long long)b * p.o_sb + (long long)qrow * p.o_ss + h * 64 + 4 * ln.hh;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (dt ? r.o1[4 * g + e] : r.o0[4 * g + e]) * inv;
      const long long off = obase + dt * 32 + 8 * g;
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
  }
}

template <int NW, bool SHORTKV = false>
int launch_attn(hipStream_t s, AttnP p) {
  p.n_qtiles = (p.Sq + NW * 32 - 1) / (NW * 32);
  const dim3 grid(p.n_qtiles * p.B * p.H), block(NW * 64);
  const size_t lds = 2 * NS * TILE_BYTES;
  const int rc = launch_dyn_lds((p.mask || p.bias) ? attn_fwd_kernel<NW, true, SHORTKV> : attn_fwd_kernel<NW, false, SHORTKV>, grid, block, lds, s, p);
  if (rc != MRAG_OK) return rc;
  MRAG_COUNT(MRAG_K_ATTN_FLASH);
  return MRAG_OK;
}

// Key-split tail (attn_bf16.hip: mrag_plan_kv_split): the launch's last workgroups each scan one chunk of the keys for the ragged last query tile of a
// (b, h) pair; the merge kernel finishes those rows.
int launch_attn_split(hipStream_t s, AttnP p, const SplitPlan& pl, void* workspace) {
  attn_fill_split(p, pl, workspace, 256);
  const size_t lds = 2 * NS * TILE_BYTES;
  const int rc = launch_dyn_lds(attn_fwd_kernel<8, false, false, true>, dim3(p.n_main + p.B * p.H * pl.splits), dim3(512), lds, s, p);
  if (rc != MRAG_OK) return rc;
  MRAG_COUNT(MRAG_K_ATTN_FLASH_KSPLIT);
  return mrag_launch_attn_combine(s, p);
}

}  // namespace

MRAG_FAMILY_LAUNCHER mrag_launch_attn_flash(hipStream_t s, const AttnP& p, int nw, bool short_kv, const SplitPlan* pl, void* workspace) {
  if (pl) return launch_attn_split(s, p, *pl, workspace);
  if (short_kv) return launch_attn<8, true>(s, p);
  return nw == 8 ? launch_attn<8>(s, p) : (nw == 2 ? launch_attn<2>(s, p) : launch_attn<1>(s, p));
}
