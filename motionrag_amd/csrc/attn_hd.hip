// attn_hd.hip -- softmax(scale * Q K^T) V in bf16 on the matrix pipe at the head dims the head_dim-64 families do not take (32, 80, 96, 128), any Sq and Skv
// (mrag_attn_hd_fwd_bf16, include/mrag_hip.h).  attn_small.hip covers the same head dims with fp32 FMAs, one workgroup per (batch, head) and K / V of the head
// resident in LDS; here K and V stream through LDS in 64-key tiles and a workgroup owns 64 query rows of one (batch, head), so nothing bounds the lengths.
// First user: the CLIP-ViT-H/14 tower (16 heads of 80; 257 tokens at 224 px, 577 at 336 px).
//   * grid = B * H * ceil(Sq / 64) workgroups of two waves; a wave owns 32 query rows.  The ragged last tile (one row at Sq = 257) costs one workgroup whose
//     second wave only helps staging.
//   * S^T = K . Q^T on v_mfma_f32_32x32x16_bf16 (D / 16 k-steps: 80 needs no padding here): K rows from LDS as the A operand, Q (read once, in registers)
//     as the B operand.  A lane then holds 32 of the 64 scores of ITS query (the other half-wave holds the rest): the softmax is lane-local but for one
//     cross-half exchange of the tile maximum, and the bf16 P^T registers are the B operand of the second product with no lane movement
//     (register i of a 32-key block is key (i & 3) + 8 (i >> 2) + 4 (lane >> 5)).
//   * O^T = V^T . P^T in 32-row tiles of d: ceil(D / 32) accumulator tiles (80 runs as 96: the 16 extra columns are zeros in LDS, they are never read from
//     or written to global memory).  V is staged row-major and read transposed (ds_read_b64_tr_b16) in the key order of P^T's registers.
//   * staging: 16-byte global loads into registers one tile ahead, written to LDS after the tile in flight is consumed (two barriers per tile, one buffer:
//     <= 38 KB at D = 128, 23.5 KB at D = 80).  Keys past Skv re-read row Skv - 1 and are masked to -inf in front of the row maximum; query rows past Sq re-read
//     row Sq - 1 and are not stored.
//   * rounding points: fp32 scores (scale * log2 e applied to the fp32 score), fp32 statistics, P rounded to bf16 for the second product with the row sum
//     taken over the rounded values, fp32 accumulation, one bf16 rounding of the output.
#include "attn_common.h"

namespace {

unsigned long long g_attn_hd_launches[1];

struct HdP {
  const bf16_t* Q; const bf16_t* K; const bf16_t* V; bf16_t* O;
  long long q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss, v_sh, o_sb, o_ss;
  int B, H, Sq, Skv, n_qtiles;
  float qscale;   // scale * log2 e
};

constexpr int HD_KT = 64;     // keys per tile
constexpr int HD_ROWS = 64;   // query rows per workgroup (32 per wave)
constexpr int HD_THREADS = 128;

template <int D>
struct HdCfg {
  static constexpr int DV = D / 8;                 // 16-byte chunks of a row
  static constexpr int KS = D / 16;                // k-steps of the score product
  static constexpr int DT = (D + 31) / 32;         // 32-row tiles of O^T
  static constexpr int PK = D * 2 + 16;            // K row pitch (bytes): 16 lanes' ds_read_b128 fall on 16 different 16-byte bank slots
  static constexpr int PV = (DT * 64) % 128 == 64 ? DT * 64 : DT * 64 + 64;   // V row pitch: 64 mod 128, four rows x 64 bytes of a transposed read cover all banks
  static constexpr int NCH = HD_KT * DV / HD_THREADS;   // chunks per thread per operand per tile
  static constexpr int PADCH = (DT * 32 - D) / 8;  // zero chunks behind a V row (2 at D = 80)
  static constexpr int V_OFF = HD_KT * PK;
  static constexpr int LDS = HD_KT * (PK + PV);
  static_assert(D % 16 == 0 && (HD_KT * DV) % HD_THREADS == 0 && PK % 16 == 0 && PV % 16 == 0 && LDS <= 64 * 1024, "tile geometry");
};

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

template <int D>
__global__ __launch_bounds__(HD_THREADS) void attn_hd_kernel(const HdP p) {
  using C = HdCfg<D>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const ks = smem;
  char* const vs = smem + C::V_OFF;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hh = lane >> 5;
  int blk = blockIdx.x;
  const int qt = blk % p.n_qtiles;
  blk /= p.n_qtiles;
  const int h = blk % p.H, b = blk / p.H;
  const bf16_t* kg = p.K + (long long)b * p.k_sb + (long long)h * p.k_sh;
  const bf16_t* vg = p.V + (long long)b * p.v_sb + (long long)h * p.v_sh;

  // ---- staging: chunk c = tid + 128 i of a tile is (key c / DV, 16-byte column c % DV)
  u32x4 kr[C::NCH], vr[C::NCH];
  auto fetch = [&](int t) {
#pragma unroll
    for (int i = 0; i < C::NCH; ++i) {
      const int c = tid + HD_THREADS * i, row = c / C::DV, col = c - row * C::DV;
      int key = t * HD_KT + row;
      key = key < p.Skv ? key : p.Skv - 1;          // rows past the end re-read a valid row; their scores are masked
      kr[i] = *(const u32x4*)(kg + (long long)key * p.k_ss + col * 8);
      vr[i] = *(const u32x4*)(vg + (long long)key * p.v_ss + col * 8);
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < C::NCH; ++i) {
      const int c = tid + HD_THREADS * i, row = c / C::DV, col = c - row * C::DV;
      *(u32x4*)(ks + row * C::PK + col * 16) = kr[i];
      *(u32x4*)(vs + row * C::PV + col * 16) = vr[i];
    }
  };
  if constexpr (C::PADCH > 0) {   // columns D .. 32 DT - 1 of the V image: rows of O^T that are never stored; zeros, written once
    for (int c = tid; c < HD_KT * C::PADCH; c += HD_THREADS) {
      const int row = c / C::PADCH, col = c - row * C::PADCH;
      *(u32x4*)(vs + row * C::PV + D * 2 + col * 16) = u32x4{0u, 0u, 0u, 0u};
    }
  }
  fetch(0);

  // ---- this wave's 32 query rows; Q fragments: B operand of S^T = K . Q^T, lane holds Q[q = lane & 31][d = 16 ks + 8 hh + j]
  const int q0 = qt * HD_ROWS + wave * 32;
  const bool wave_active = q0 < p.Sq;               // wave-uniform
  const int qrow = q0 + r32;
  const int qrow_c = qrow < p.Sq ? qrow : p.Sq - 1;
  bf16x8 qf[C::KS];
  {
    const bf16_t* qp = p.Q + (long long)b * p.q_sb + (long long)qrow_c * p.q_ss + (long long)h * p.q_sh + hh * 8;
#pragma unroll
    for (int s = 0; s < C::KS; ++s) qf[s] = __builtin_bit_cast(bf16x8, *(const u32x4*)(qp + s * 16));
  }

  // ---- fragment read addresses
  const char* kfrag = ks + r32 * C::PK + hh * 16;   // + (32 kb) * PK + 32 s: K[key 32 kb + r32][d = 16 s + 8 hh ..]
  // transposed V read: group g = lane >> 4 of 16 lanes takes the block (4 keys x 16 columns) at keys r0 .. r0 + 3, columns 32 dt + 16 (g & 1); lane
  // 4 q + p of the group supplies the address of key r0 + q, columns 4 p .. 4 p + 3, and receives column (lane & 15) of the four keys.  With
  // r0 = 32 kb + 16 s + 8 half + 4 hh the two reads (half = 0, 1) of a fragment are V^T[d = 32 dt + r32][key 32 kb + 16 s + 8 (j >> 2) + 4 hh + (j & 3)]:
  // the key order of P^T's registers.
  const char* vfrag = vs + (4 * hh + ((lane >> 2) & 3)) * C::PV + ((lane >> 4) & 1) * 32 + (lane & 3) * 8;

  f32x16 o[C::DT];
#pragma unroll
  for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
  float m = -INFINITY, l = 0.f;                     // running maximum (log2 units) and this half-wave's part of the row sum

  const int nt = (p.Skv + HD_KT - 1) / HD_KT;
  for (int t = 0; t < nt; ++t) {
    stage();
    __syncthreads();
    if (t + 1 < nt) fetch(t + 1);
    if (wave_active) {
      f32x16 s[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) s[kb][i] = 0.f;
#pragma unroll
        for (int st = 0; st < C::KS; ++st) {
          const u32x4 kf = *(const u32x4*)(kfrag + (32 * kb) * C::PK + 32 * st);
          s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf), qf[st], s[kb], 0, 0, 0);
        }
      }
      // scores in log2 units; register i of block kb is key t * 64 + 32 kb + (i & 3) + 8 (i >> 2) + 4 hh
      const bool ragged = (t == nt - 1) && (p.Skv & (HD_KT - 1));
      float tm = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float x = s[kb][i] * p.qscale;
          if (ragged && t * HD_KT + 32 * kb + (i & 3) + 8 * (i >> 2) + 4 * hh >= p.Skv) x = -INFINITY;
          s[kb][i] = x;
          tm = fmaxf(tm, x);
        }
      tm = fmaxf(tm, __shfl_xor(tm, 32));           // key t * 64 of every tile is in range: tm is finite
      const float m_new = fmaxf(m, tm);
      const float alpha = __builtin_amdgcn_exp2f(m - m_new);   // first tile: exp2(-inf) = 0 times an O and l that are zero
      m = m_new;
      l *= alpha;
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
      bf16x8 pb[2][2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          u32x4 w;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            w[j] = pack_bf2(__builtin_amdgcn_exp2f(s[kb][8 * st + 2 * j] - m), __builtin_amdgcn_exp2f(s[kb][8 * st + 2 * j + 1] - m));
            l += __uint_as_float(w[j] << 16) + __uint_as_float(w[j] & 0xffff0000u);   // the row sum adds the P values that multiply V
          }
          pb[kb][st] = __builtin_bit_cast(bf16x8, w);
        }
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int st = 0; st < 2; ++st) {
            const char* vp = vfrag + (32 * kb + 16 * st) * C::PV + dt * 64;
            const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)vp);
            const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(vp + 8 * C::PV));
            const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pb[kb][st], o[dt], 0, 0, 0);
          }
    }
    __syncthreads();                                // the tile is consumed: the next stage() may overwrite it
  }

  // ---- epilogue: the two half-waves' row sums are added; register i of tile dt is O[q][d = 32 dt + (i & 3) + 8 (i >> 2) + 4 hh]
  l += __shfl_xor(l, 32);
  if (!wave_active || qrow >= p.Sq) return;
  const float inv = 1.0f / l;
  bf16_t* orow = p.O + (long long)b * p.o_sb + (long long)qrow * p.o_ss + h * D + 4 * hh;
#pragma unroll
  for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (32 * dt + 8 * g < D) {                    // compile-time: the columns past D of the last tile are not stored
        u32x2 out;
        out[0] = pack_bf2(o[dt][4 * g] * inv, o[dt][4 * g + 1] * inv);
        out[1] = pack_bf2(o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv);
        *(u32x2*)(orow + 32 * dt + 8 * g) = out;
      }
}

template <int D>
int launch_hd(hipStream_t s, HdP& p) {
  p.n_qtiles = (p.Sq + HD_ROWS - 1) / HD_ROWS;
  const long long blocks = (long long)p.B * p.H * p.n_qtiles;
  if (blocks > 0x7fffffffLL) return MRAG_ENOTSUP;   // one grid dimension
  const int rc = launch_dyn_lds(attn_hd_kernel<D>, dim3((unsigned)blocks), dim3(HD_THREADS), (size_t)HdCfg<D>::LDS, s, p);
  if (rc != MRAG_OK) return rc;
  (void)__atomic_fetch_add(&g_attn_hd_launches[0], 1ull, __ATOMIC_RELAXED);
  return MRAG_OK;
}

}  // namespace

extern "C" int mrag_attn_hd_launch_counts(uint64_t* out_host, int32_t n) {
  for (int i = 0; out_host && i < n && i < 1; ++i) out_host[i] = __atomic_load_n(&g_attn_hd_launches[i], __ATOMIC_RELAXED);
  return 1;
}

extern "C" int mrag_attn_hd_fwd_bf16(void* stream, const mrag_attn_args* a, int32_t head_dim) {
  if (!attn_args_present(a)) return MRAG_EINVAL;
  if (a->mask || a->bias || a->resid || a->kv_batch_div != 1 || a->q_prescaled) return MRAG_ENOTSUP;
  if (head_dim != 32 && head_dim != 80 && head_dim != 96 && head_dim != 128) return MRAG_ENOTSUP;
  if (!attn_args_aligned(a, 16)) return MRAG_EINVAL;   // 16-byte loads of Q / K / V; O as mrag_attn_small_bf16 asks (the stores here are 8 bytes wide)
  HdP p;
  attn_fill_views(p, a);
  p.qscale = a->scale * kLog2e;
  hipStream_t s = (hipStream_t)stream;
  switch (head_dim) {
    case 32: return launch_hd<32>(s, p);
    case 80: return launch_hd<80>(s, p);
    case 96: return launch_hd<96>(s, p);
    default: return launch_hd<128>(s, p);
  }
}
