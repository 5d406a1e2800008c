// gemm_skinny.hip -- the few-row GEMM (M <= 256): gemm_skinny_kernel and its launcher.
#include "gemm_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Few-row GEMM (M <= 256: CAMA's Perceiver latents and encoder tokens, 25-251 rows; the retrieval query's text embedder, 16 rows).  On the tiled kernels such a
// problem is 8-96 workgroups, each walking the whole K through an LDS ring with a barrier per K-tile: 15-45 us per launch whatever the size.
// Here a workgroup owns a 32 x 64 output tile and its EIGHT waves split K between them (wave w takes the 32-deep K-steps w, w + 8, ...): every wave streams its
// fragments straight from L2 / HBM into MFMA operands -- no LDS staging, no barrier in the loop, dozens of independent 16-byte loads in flight per lane -- and the
// eight partial tiles meet once in LDS, where they are added in wave order (a fixed order: bit-reproducible; NOT the summation order of the tiled kernels, so
// the last bits differ from theirs).  Grid = ceil(M / 32) x ceil(N / 64) workgroups: 128-512 for CAMA's shapes.  Epilogue and rounding points: epilogue_direct's.
// Long K (>= 2 048: the feed-forward's second projection) takes SIXTEEN waves over a 32 x 32 tile instead: half the K-steps per wave, twice the workgroups.
// LNA (round 6): the LayerNorm in FRONT of the projection rides in the A load -- CAMA's Perceiver layers run `to_q(norm2(latents))` and `ff1(ln(latents))` over 250
// rows, where the LayerNorm was a 6 us launch of its own in a chain of dependent launches.  A workgroup reads all of K for its 32 rows anyway: its waves first
// compute the rows' statistics (4 or 2 rows per wave, the arithmetic of layernorm_kernel in norm.hip lane for lane: per-lane sums over idx = (c 64 + lane) 8,
// the wave butterfly, mean, then the squared deviations -- so the normalised bf16 values are the SAME BITS the separate kernel writes), park them in LDS, and every
// A fragment is normalised, scaled, shifted and rounded to bf16 in registers before its MFMAs.  Results are bit-identical to LayerNorm kernel + GEMM.
template <int EPI, int NWV, int COLS, bool LNA = false>
__global__ __launch_bounds__(64 * NWV) void gemm_skinny_kernel(const GemmP p) {
  constexpr int TJ = COLS / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* part = (float*)smem;                                   // [NWV][SKM_ROWS][COLS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.y * SKM_ROWS, n0 = (long long)blockIdx.x * COLS;
  const int r = lane & 15, kc = (lane >> 4) * 8;
  const bf16_t* ap[2];
  const bf16_t* wp[TJ];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    long long m = m0 + i * 16 + r;
    m = m < p.M ? m : p.M - 1;                                  // (rows / columns past the problem are computed on a clamped copy and never stored)
    ap[i] = p.A + m * p.lda + kc;
  }
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    long long n = n0 + j * 16 + r;
    n = n < p.N ? n : p.N - 1;
    wp[j] = p.W + n * p.ldw + kc;
  }
  f32x4 acc[2][TJ];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nks = (int)(p.K / 32);
  float ln_mean[2] = {0.f, 0.f}, ln_rstd[2] = {1.f, 1.f};
  if constexpr (LNA) {
    constexpr int RPWV = SKM_ROWS / NWV;                          // rows whose statistics this wave computes
    const int D = (int)p.K;
#pragma unroll
    for (int rr = 0; rr < RPWV; ++rr) {
      const int row_l = wave * RPWV + rr;
      long long m = m0 + row_l;
      m = m < p.M ? m : p.M - 1;
      const bf16_t* x = p.A + m * p.lda;
      float sum = 0.f;
      for (int c = 0; c * 512 < D; ++c) {
        const int idx = (c * 64 + lane) * 8;
        if (idx < D) {
          const u32x4 raw = *(const u32x4*)(x + idx);
#pragma unroll
          for (int e = 0; e < 4; ++e) { sum += __uint_as_float(raw[e] << 16); sum += __uint_as_float(raw[e] & 0xffff0000u); }
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      const float mean = sum / (float)D;
      float sq = 0.f;
      for (int c = 0; c * 512 < D; ++c) {
        const int idx = (c * 64 + lane) * 8;
        if (idx < D) {
          const u32x4 raw = *(const u32x4*)(x + idx);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float d0 = __fsub_rn(__uint_as_float(raw[e] << 16), mean), d1 = __fsub_rn(__uint_as_float(raw[e] & 0xffff0000u), mean);
            sq = __builtin_fmaf(d0, d0, sq); sq = __builtin_fmaf(d1, d1, sq);
          }
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
      if (lane == 0) { part[2 * row_l] = mean; part[2 * row_l + 1] = rsqrtf(sq / (float)D + p.lna_eps); }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) { ln_mean[i] = part[2 * (i * 16 + r)]; ln_rstd[i] = part[2 * (i * 16 + r) + 1]; }
    __syncthreads();                                              // (the partial tiles reuse this LDS behind the K loop)
  }
  auto steps = [&](auto U, const int ks0) __attribute__((always_inline)) {       // U K-steps of this wave from ks0: all loads first ((2 + TJ) U independent 16-byte loads in flight)
    constexpr int u_n = decltype(U)::value;
    bf16x8 a[u_n][2], w[u_n][TJ];
    u32x4 lg[LNA ? u_n : 1], lb[LNA ? u_n : 1];
#pragma unroll
    for (int u = 0; u < u_n; ++u) {
      const int k = (ks0 + u * NWV) * 32;
#pragma unroll
      for (int i = 0; i < 2; ++i) a[u][i] = *(const bf16x8*)(ap[i] + k);
#pragma unroll
      for (int j = 0; j < TJ; ++j) w[u][j] = *(const bf16x8*)(wp[j] + k);
      if constexpr (LNA) {
        lg[u] = p.lna_g ? *(const u32x4*)(p.lna_g + k + kc) : u32x4{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
        lb[u] = p.lna_b ? *(const u32x4*)(p.lna_b + k + kc) : u32x4{0u, 0u, 0u, 0u};
      }
    }
    if constexpr (LNA) {                                           // o = (v - mean) * rstd [* gamma] [+ beta], ONE rounding to bf16: layernorm_kernel's arithmetic
#pragma unroll
      for (int u = 0; u < u_n; ++u)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const u32x4 raw = __builtin_bit_cast(u32x4, a[u][i]);
          u32x4 o4;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float o0 = __fmul_rn(__fsub_rn(__uint_as_float(raw[e] << 16), ln_mean[i]), ln_rstd[i]), o1 = __fmul_rn(__fsub_rn(__uint_as_float(raw[e] & 0xffff0000u), ln_mean[i]), ln_rstd[i]);
            if (p.lna_g) { o0 = __fmul_rn(o0, __uint_as_float(lg[u][e] << 16)); o1 = __fmul_rn(o1, __uint_as_float(lg[u][e] & 0xffff0000u)); }
            if (p.lna_b) { o0 = __fadd_rn(o0, __uint_as_float(lb[u][e] << 16)); o1 = __fadd_rn(o1, __uint_as_float(lb[u][e] & 0xffff0000u)); }
            o4[e] = pack_bf2(o0, o1);
          }
          a[u][i] = __builtin_bit_cast(bf16x8, o4);
        }
    }
#pragma unroll
    for (int u = 0; u < u_n; ++u)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[u][j], a[u][i], acc[i][j], 0, 0, 0);
  };
  int ks = wave;
  constexpr int UB = (LNA && NWV == 16) ? 2 : 4;   // K-steps whose loads are in flight together (sixteen waves leave 128 registers per lane: four steps + the LayerNorm's operands spilled)
  for (; ks + (UB - 1) * NWV < nks; ks += UB * NWV) steps(std::integral_constant<int, UB>{}, ks);
  for (; ks < nks; ks += NWV) steps(std::integral_constant<int, 1>{}, ks);
  // accumulator layout: lane owns row i * 16 + (lane & 15), columns j * 16 + (lane >> 4) * 4 + {0..3}
  float* mine = part + wave * (SKM_ROWS * COLS);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) *(f32x4*)(mine + (i * 16 + r) * COLS + j * 16 + (lane >> 4) * 4) = acc[i][j];
  __syncthreads();
  // one thread per 4 consecutive columns of the 32 x COLS tile
  if (tid >= SKM_ROWS * COLS / 4) return;
  const int row = tid / (COLS / 4), col = (tid % (COLS / 4)) * 4;
  const long long m = m0 + row, n = n0 + col;
  if (m >= p.M || n >= p.N) return;
  f32x4 t = *(const f32x4*)(part + row * COLS + col);
#pragma unroll
  for (int w8 = 1; w8 < NWV; ++w8) {
    const f32x4 u = *(const f32x4*)(part + w8 * (SKM_ROWS * COLS) + row * COLS + col);
    t[0] += u[0]; t[1] += u[1]; t[2] += u[2]; t[3] += u[3];
  }
  float v[4] = {t[0], t[1], t[2], t[3]};
  if (p.bias) {
    const u32x2 bb = *(const u32x2*)(p.bias + n);
    v[0] += __uint_as_float(bb[0] << 16); v[1] += __uint_as_float(bb[0] & 0xffff0000u);
    v[2] += __uint_as_float(bb[1] << 16); v[3] += __uint_as_float(bb[1] & 0xffff0000u);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = epi_act<EPI>(v[e]);
  if constexpr (EPI == MRAG_EPI_RESID) {
    const u32x2 rr = *(const u32x2*)(p.resid + m * p.ldr + n);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] *= p.acc_scale;
    v[0] = bf_round(v[0]) + __uint_as_float(rr[0] << 16); v[1] = bf_round(v[1]) + __uint_as_float(rr[0] & 0xffff0000u);
    v[2] = bf_round(v[2]) + __uint_as_float(rr[1] << 16); v[3] = bf_round(v[3]) + __uint_as_float(rr[1] & 0xffff0000u);
  }
  u32x2 out;
  out[0] = pack_bf2(v[0], v[1]);
  out[1] = pack_bf2(v[2], v[3]);
  *(u32x2*)(p.C + m * p.ldc + n) = out;
}

}  // namespace

extern "C" int launch_skinny(hipStream_t s, const GemmP& p, int epi) {
  // 16 waves x 32 columns where K is long and the 8-wave grid would leave most CUs idle ([250 x 1024 x 4096] 25.5 -> 20.1 us, [64 x 4096 x 4096] 26.1 -> 20.7;
  // a grid that already fills the chip loses: [128 x 4096 x 4096] 26.6 -> 34.6; profiles/r5_gemm_skinny_sweep.txt).  MRAG_GEMM_TUNE_SKINNY_8: the 8-wave form always (A/B runs)
  const long long wg8 = ((p.M + SKM_ROWS - 1) / SKM_ROWS) * ((p.N + 63) / 64);
  const bool sixteen = p.K >= 2048 && p.N >= 1024 && wg8 < 256 && !(p.tuning & MRAG_GEMM_TUNE_SKINNY_8);
  const int cols = sixteen ? 32 : 64, nw = sixteen ? 16 : 8;
  const dim3 grid((unsigned)((p.N + cols - 1) / cols), (unsigned)((p.M + SKM_ROWS - 1) / SKM_ROWS)), block(64 * nw);
  const size_t lds = (size_t)nw * SKM_ROWS * cols * sizeof(float);
  int rc;
#define MRAG_SKINNY_CASE(E, LNA) \
  case E: rc = sixteen ? launch_dyn_lds(gemm_skinny_kernel<E, 16, 32, LNA>, grid, block, lds, s, p) : launch_dyn_lds(gemm_skinny_kernel<E, 8, 64, LNA>, grid, block, lds, s, p); break;
  if (p.lna) {
    switch (epi) {                            // the two forms CAMA runs: to_q(norm2(.)), gelu(ff1(ln(.)))
      MRAG_SKINNY_CASE(MRAG_EPI_NONE, true)
      MRAG_SKINNY_CASE(MRAG_EPI_GELU_ERF, true)
      default: return MRAG_ENOTSUP;
    }
  } else {
    switch (epi) {
      MRAG_SKINNY_CASE(MRAG_EPI_NONE, false)
      MRAG_SKINNY_CASE(MRAG_EPI_GELU_TANH, false)
      MRAG_SKINNY_CASE(MRAG_EPI_GELU_ERF, false)
      MRAG_SKINNY_CASE(MRAG_EPI_SILU, false)
      MRAG_SKINNY_CASE(MRAG_EPI_RESID, false)
      default: return MRAG_ENOTSUP;
    }
  }
#undef MRAG_SKINNY_CASE
  if (rc != MRAG_OK) return rc;
  MRAG_COUNT(p.lna ? MRAG_K_GEMM_SKINNY_LNA : MRAG_K_GEMM_SKINNY);
  return MRAG_OK;
}
