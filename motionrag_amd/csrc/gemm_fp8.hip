// gemm_fp8.hip -- the opt-in e4m3 path of the DiT's four large linears (attn_processor.py:209-211,276 and diffusers CogVideoXBlock FF):
//
//   mrag_quant_rows_e4m3   x [M, K] bf16 -> x8 [M, K] OCP e4m3fn bytes + exp [M] int32: per row e = pow2_fit(amax_row) (common.h: the function
//                          attn_fp8.hip scales with), x8 = rne_e4m3(x * 2^e).  One pass: a row is read once (kept in registers), its maximum reduced in the wave /
//                          workgroup, written once.  Activations every call, weights ([N, K]: per output channel) once.
//   mrag_gemm_fp8          C[m, n] = epilogue(2^-(ea[m] + ew[n]) * sum_k A8[m, k] W8[n, k] + bias[n]) on v_mfma_scale_f32_32x32x64_f8f6f4 (twice the bf16
//                          MFMA rate, half the LDS / DMA bytes).  The row exponents ride the instruction's E8M0 scale operands (127 - e per lane: a lane's
//                          scale byte applies to its own row's 32 k's), which undoes both power-of-two scales for free, as attn8_kernel does with scale_q.
//
//   mrag_gemm_fp8_k64      the same kernel for the UNets' feed-forward linears (layers.set_ff_precision): K % 64 == 0 -- at K % 128 == 64 the last
//                          K-tile is ONE 64-deep MFMA step, its DMA lanes of the absent half re-read the present half (inside the row: nothing behind
//                          the last row of A8 or W8 is touched) into LDS bytes no fragment read visits -- and MRAG_EPI_GEGLU: W rows in ops.geglu_interleave's
//                          32-row groups (16 value | 16 gate) put a lane's values in register quads 0, 1 and their gates in quads 2, 3 of one accumulator.
//
// Kernel shape, operand maps and the staged epilogue: gemm_fp8_tile.h (the tile conv_fp8.hip shares), here on plain rows of A8 and W8; C may alias resid.
#include "gemm_fp8_tile.h"

// host-side relaxed launch counters (mrag_fp8_launch_counts): slot 0 the GEMM, slot 1 the row quantiser
static unsigned long long g_fp8_launches[2];
// mrag_gemm_fp8_k64_launch_counts: slot 0 mrag_gemm_fp8_k64, slot 1 mrag_layernorm_e4m3 (norm.hip counts into it)
unsigned long long g_fp8_k64_launches[2];

namespace {

// ------------------------------------------------------------------------------------------------ row quantiser
__device__ __forceinline__ u32x4 quant16(const u32x4 a, const u32x4 b, const float mul) {
  float f[16];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = __uint_as_float(a[j] << 16) * mul;
    f[2 * j + 1] = __uint_as_float(a[j] & 0xffff0000u) * mul;
    f[8 + 2 * j] = __uint_as_float(b[j] << 16) * mul;
    f[8 + 2 * j + 1] = __uint_as_float(b[j] & 0xffff0000u) * mul;
  }
  return u32x4{pack4_fp8(f[0], f[1], f[2], f[3]), pack4_fp8(f[4], f[5], f[6], f[7]), pack4_fp8(f[8], f[9], f[10], f[11]), pack4_fp8(f[12], f[13], f[14], f[15])};
}

// TPR threads per row (64: a wave per row, four rows per workgroup; 256: the workgroup per row).  A thread owns the 16-element units t, t + TPR, ...
// (32 bytes in, 16 bytes out); its first QCACHE units stay in registers between the two phases, units behind them (K > 16 QCACHE TPR) are read again.
constexpr int QCACHE = 4;
template <int TPR>
__global__ __launch_bounds__(256) void quant_rows_kernel(const bf16_t* __restrict__ x, uint8_t* __restrict__ x8, int* __restrict__ exps, const long long M,
                                                          const int units, const long long ldx, const long long ld8) {
  __shared__ unsigned red[4];
  const int t = threadIdx.x % TPR;
  const long long row = (long long)blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
  if (TPR == 64 && row >= M) return;       // (whole waves: no barrier below in this form)
  const bf16_t* src = x + row * ldx;
  u32x4 va[QCACHE], vb[QCACHE];
  unsigned m = 0;
#pragma unroll
  for (int i = 0; i < QCACHE; ++i) {
    const int u = t + i * TPR;
    va[i] = vb[i] = u32x4{0u, 0u, 0u, 0u};
    if (u < units) {
      va[i] = *(const u32x4*)(src + u * 16);
      vb[i] = *(const u32x4*)(src + u * 16 + 8);
    }
    m = absmax8(absmax8(m, va[i]), vb[i]);
  }
  for (int u = t + QCACHE * TPR; u < units; u += TPR) m = absmax8(absmax8(m, *(const u32x4*)(src + u * 16)), *(const u32x4*)(src + u * 16 + 8));
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const unsigned s = __shfl_xor(m, o); m = s > m ? s : m; }
  if (TPR == 256) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    const unsigned a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
    m = a > b ? a : b;
  }
  const int e = pow2_fit(__uint_as_float(m));
  const float mul = ldexpf(1.0f, e);
  if (t == 0) exps[row] = e;
  uint8_t* dst = x8 + row * ld8;
#pragma unroll
  for (int i = 0; i < QCACHE; ++i) {
    const int u = t + i * TPR;
    if (u < units) *(u32x4*)(dst + u * 16) = quant16(va[i], vb[i], mul);
  }
  for (int u = t + QCACHE * TPR; u < units; u += TPR)
    *(u32x4*)(dst + u * 16) = quant16(*(const u32x4*)(src + u * 16), *(const u32x4*)(src + u * 16 + 8), mul);
}

// ------------------------------------------------------------------------------------------------ GEMM
struct Gemm8P {
  const uint8_t* A; const uint8_t* W; const int* ea; const int* ew;
  const bf16_t* bias; bf16_t* C; const bf16_t* resid; const bf16_t* gate0; const bf16_t* gate1;
  long long M, N, K, lda, ldw, ldc, ldr, rows_per_batch, split, gate_stride;
  int tiles_m, tiles_n, group_m;
};

// K64 (mrag_gemm_fp8_k64): p.K % 64 == 0, a last half K-tile is one MFMA step; EPI may be MRAG_EPI_GEGLU (C [M, N / 2])
template <int EPI, bool K64 = false>
__global__ __launch_bounds__(512) void gemm_fp8_kernel(const Gemm8P p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NW = 8, PPW = (F8_BM + F8_BN) / 8 / NW;     // 64 pieces of 1 KiB per stage, 8 per wave: the first 4 are A rows, the others W rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int r32 = lane & 31, hh = lane >> 5;

  long long bm0, bn0;
  fp8_tile_origin(p.tiles_m, p.tiles_n, p.group_m, bm0, bn0);

  const uint8_t* gsrc[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int piece = wave + i * NW;
    const int r = piece * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ (lane >> 3);             // source-side swizzle: row & 7 == lane >> 3
    if (piece < F8_BM / 8) {
      long long row = bm0 + r;
      row = row < p.M ? row : p.M - 1;                      // clamp: tail rows re-read a valid row, stores are masked
      gsrc[i] = p.A + row * p.lda + chunk * 16;
    } else {
      long long row = bn0 + (r - F8_BM);
      row = row < p.N ? row : p.N - 1;
      gsrc[i] = p.W + row * p.ldw + chunk * 16;
    }
  }
  // K64, last half K-tile: the row has 64 bytes left, so the lanes of chunks 4 .. 7 fetch chunks 0 .. 3 again (a lane's chunk is the same in all its pieces)
  const bool half = K64 && (p.K % F8_BK) != 0;
  const int half_back = (((lane & 7) ^ (lane >> 3)) >= 4) ? -64 : 0;
  auto issue = [&](int stage, int kt, bool clamp = false) {
    char* base = smem + stage * F8_STAGE;
    const long long off = (long long)kt * F8_BK + (clamp ? half_back : 0);
#pragma unroll
    for (int i = 0; i < PPW; ++i) glds16(gsrc[i] + off, base + (wave + i * NW) * 1024);
  };

  // E8M0 scale operands: the lane's W row (A operand) and activation row (B operand) of every 32-row block
  int sw[2], sa[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) sw[j] = fp8_row_scale(p.ew, bn0 + wn * 64 + j * 32 + r32, p.N);
#pragma unroll
  for (int i = 0; i < 4; ++i) sa[i] = fp8_row_scale(p.ea, bm0 + wm * 128 + i * 32 + r32, p.M);

  f32x16 acc[4][2] = {};
  // fragment read addresses: the lane's first activation / W row in stage 0, and its chunks' offsets inside a row
  const unsigned smem_u = (unsigned)(size_t)smem;
  const unsigned rowA = smem_u + (wm * 128 + r32) * 128, rowW = smem_u + F8_BM * 128 + (wn * 64 + r32) * 128;
  unsigned ca[2][2];                                         // [k-step][half]
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int c = 0; c < 2; ++c) ca[ks][c] = fp8_frag_chunk(ks, hh, c, r32);

  const int nk = (int)((p.K + (K64 ? F8_BK - 1 : 0)) / F8_BK);
  issue(0, 0, half && nk == 1);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");   // tile kt landed for every wave; every wave finished reading the other stage
    const unsigned so = (unsigned)((kt & 1) * F8_STAGE);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (K64 && ks == 1 && half && kt == nk - 1) break;             // (workgroup-uniform) the half tile has no second step
      Fp8Frag f;
      fp8_tile_read<false>(f, rowW + so + ca[ks][0], rowW + so + ca[ks][1], rowA + so + ca[ks][0], rowA + so + ca[ks][1]);
      if (ks == 0 && kt + 1 < nk) issue((kt + 1) & 1, kt + 1, half && kt + 2 == nk);    // the next tile's eight DMA requests go out under the first fragments' LDS latency
      fp8_tile_mfma<false>(acc, f, sw, sa);
    }
  }

  // ---- epilogue, LDS-staged as in gemm_tile.h: the wave's 128 x 64 bf16 tile goes through LDS (row pitch 144 B) and leaves as whole 128-byte row
  // segments with 16-byte lanes; bias / activation / gate in the accumulator layout, the residual add in the row layout
  long long wg_b = 0, wg_pos = 0;
  if constexpr (EPI == MRAG_EPI_GATE_RESID) {
    wg_b = bm0 / p.rows_per_batch;
    wg_pos = bm0 - wg_b * p.rows_per_batch;
  }
  auto row_bp = [&](long long m, long long& b, long long& pos) {
    b = wg_b; pos = wg_pos + (m - bm0);
    while (pos >= p.rows_per_batch) { pos -= p.rows_per_batch; ++b; }
  };
  char* wbase = smem + wave * (128 * F8_ROWB);
  __syncthreads();   // every wave is done with the operand stages that these per-wave regions overlay (no DMA is in flight: the last tile issued none)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lrow = i * 32 + r32;
    const bf16_t* gate = nullptr;
    if constexpr (EPI == MRAG_EPI_GATE_RESID) {
      const long long m = bm0 + wm * 128 + lrow;
      long long b, pos;
      row_bp(m < p.M ? m : p.M - 1, b, pos);
      gate = (pos < p.split ? p.gate0 : p.gate1) + b * p.gate_stride;
    }
    if constexpr (EPI == MRAG_EPI_GEGLU) {
      // accumulator j is one 32-row group of W: quads 0, 1 hold the values of output columns 8 g + 4 hh .. + 3 of the group's 16, quads 2, 3 their gates
#pragma unroll
      for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          long long n = bn0 + wn * 64 + j * 32 + 8 * g + 4 * hh;
          n = n < p.N ? n : p.N - 32 + 8 * g + 4 * hh;   // (N % 32 == 0: the gate column n + 16 exists with the value column) clamped columns are never stored
          float v[4] = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
          float gt[4] = {acc[i][j][4 * g + 8], acc[i][j][4 * g + 9], acc[i][j][4 * g + 10], acc[i][j][4 * g + 11]};
          if (p.bias) {
            fp8_add_bf4(p.bias + n, v);
            fp8_add_bf4(p.bias + n + 16, gt);
          }
          geglu4<false>(v, gt);
          fp8_stage_quad(wbase, lrow, j * 16 + 8 * g + 4 * hh, v);
        }
      }
      continue;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int lcol = j * 32 + 8 * g + 4 * hh;
        long long n = bn0 + wn * 64 + lcol;
        n = n < p.N ? n : p.N - 4;   // clamped columns are never stored
        float v[4] = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
        if (p.bias) fp8_add_bf4(p.bias + n, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = epi_act<EPI>(v[e]);
        if constexpr (EPI == MRAG_EPI_GATE_RESID) {
          float gg[4];
          fp8_unpack_bf4(*(const u32x2*)(gate + n), gg);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] *= gg[e];
        }
        fp8_stage_quad(wbase, lrow, lcol, v);
      }
    }
  }
  if constexpr (EPI == MRAG_EPI_GEGLU) {
    // the wave's 128 x 32 outputs: lane -> row (lane >> 2) of a 16-row group, 16-byte chunk (lane & 3); one instruction = 16 x 64 contiguous bytes
    const int rsub = lane >> 2, chunk = lane & 3;
    const long long n = (bn0 + wn * 64) / 2 + chunk * 8;
    const bool n_ok = n + 8 <= p.N / 2;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const int row = g * 16 + rsub;
      const long long m = bm0 + wm * 128 + row;
      const u32x4 val = *(const u32x4*)(wbase + row * F8_ROWB + chunk * 16);
      if (m < p.M && n_ok) *(u32x4*)(p.C + m * p.ldc + n) = val;
    }
    return;
  }
  // row layout: lane -> row (lane >> 3) of an 8-row group, 16-byte chunk (lane & 7); one instruction = 8 x 128 contiguous bytes
  const int rsub = lane >> 3, chunk = lane & 7;
  const long long n = bn0 + wn * 64 + chunk * 8;
  const bool n_ok = n + 8 <= p.N;
  u32x4 rpre[16];
  if constexpr (EPI == MRAG_EPI_GATE_RESID || EPI == MRAG_EPI_RESID) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {   // all 16 residual vectors up front: one memory latency for the tail of the workgroup
      const long long m = bm0 + wm * 128 + g * 8 + rsub;
      rpre[g] = (m < p.M && n_ok) ? *(const u32x4*)(p.resid + m * p.ldr + n) : u32x4{0u, 0u, 0u, 0u};
    }
  }
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int row = g * 8 + rsub;
    const long long m = bm0 + wm * 128 + row;
    u32x4 val = *(const u32x4*)(wbase + row * F8_ROWB + chunk * 16);
    if (m < p.M && n_ok) {
      if constexpr (EPI == MRAG_EPI_GATE_RESID || EPI == MRAG_EPI_RESID) val = fp8_add_bf8(val, rpre[g]);
      *(u32x4*)(p.C + m * p.ldc + n) = val;
    }
  }
}

}  // namespace

extern "C" int mrag_fp8_launch_counts(uint64_t* out_host, int32_t n) {
  for (int i = 0; out_host && i < n && i < 2; ++i) out_host[i] = __atomic_load_n(&g_fp8_launches[i], __ATOMIC_RELAXED);
  return 2;
}

extern "C" int mrag_quant_rows_e4m3(void* stream, const void* x, void* x8, int32_t* exp, int64_t M, int64_t K, int64_t ldx, int64_t ld8) {
  if (!x || !x8 || !exp || M < 1 || K < 1 || M > 0x7fffffffll) return MRAG_EINVAL;
  if (K % 16 != 0 || K > (1ll << 30) || ldx % 8 != 0 || ld8 % 16 != 0 || ldx < K || ld8 < K) return MRAG_ENOTSUP;
  if (((uintptr_t)x | (uintptr_t)x8) & 15 || ((uintptr_t)exp & 3)) return MRAG_ENOTSUP;
  hipStream_t s = (hipStream_t)stream;
  const int units = (int)(K / 16);
  if (units <= QCACHE * 64) {
    MRAG_LAUNCH(quant_rows_kernel<64>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, (const bf16_t*)x, (uint8_t*)x8, (int*)exp, (long long)M, units, (long long)ldx, (long long)ld8);
  } else {
    MRAG_LAUNCH(quant_rows_kernel<256>, dim3((unsigned)M), dim3(256), 0, s, (const bf16_t*)x, (uint8_t*)x8, (int*)exp, (long long)M, units, (long long)ldx, (long long)ld8);
  }
  MRAG_LAUNCH_CHECK();
  (void)__atomic_fetch_add(&g_fp8_launches[1], 1ull, __ATOMIC_RELAXED);
  return MRAG_OK;
}

extern "C" int mrag_gemm_fp8_k64_launch_counts(uint64_t* out_host, int32_t n) {
  for (int i = 0; out_host && i < n && i < 2; ++i) out_host[i] = __atomic_load_n(&g_fp8_k64_launches[i], __ATOMIC_RELAXED);
  return 2;
}

// the one launch path of both entry points.  k64 (mrag_gemm_fp8_k64): K % 64 == 0 and EPI_GEGLU (C [M, N / 2]) in place of EPI_GELU_TANH / EPI_GATE_RESID
static int gemm_fp8_launch(void* stream, const mrag_gemm_fp8_args* a, const bool k64) {
  if (!a || !a->A8 || !a->W8 || !a->a_exp || !a->w_exp || !a->C) return MRAG_EINVAL;
  if (a->M < 1 || a->N < 1 || a->K < 1) return MRAG_EINVAL;
  const int epi = a->epilogue;
  const bool glu = k64 && epi == MRAG_EPI_GEGLU, gated = !k64 && epi == MRAG_EPI_GATE_RESID;
  if (epi != MRAG_EPI_NONE && epi != MRAG_EPI_RESID && !(k64 ? glu : gated || epi == MRAG_EPI_GELU_TANH)) return MRAG_ENOTSUP;
  if (a->K % (k64 ? 64 : F8_BK) != 0 || a->N % (glu ? 32 : 16) != 0) return MRAG_ENOTSUP;
  const long long ncols = glu ? a->N / 2 : a->N;             // columns of C
  if (a->lda < a->K || a->ldw < a->K || a->ldc < ncols) return MRAG_EINVAL;
  // 16-byte aligned rows of both operands (the DMA moves 16-byte chunks) and of C / resid (the staged epilogue's row segments); 8-byte bias / gate reads
  if ((((uintptr_t)a->A8 | (uintptr_t)a->W8) & 15) || a->lda % 16 != 0 || a->ldw % 16 != 0) return MRAG_EINVAL;
  if ((((uintptr_t)a->a_exp | (uintptr_t)a->w_exp) & 3) || (a->bias && ((uintptr_t)a->bias & 7))) return MRAG_EINVAL;
  const bool res = epi == MRAG_EPI_RESID || gated;
  if (res && (!a->resid || a->ldr < a->N)) return MRAG_EINVAL;
  if (!rows_16B_aligned(a->C, a->ldc, res ? a->resid : nullptr, a->ldr)) return MRAG_EINVAL;
  if (gated) {
    if (!a->gate0 || !a->gate1 || a->rows_per_batch < 1) return MRAG_EINVAL;
    if ((((uintptr_t)a->gate0 | (uintptr_t)a->gate1) & 7) || a->gate_stride % 4 != 0) return MRAG_EINVAL;
  }
  const long long tiles_m = (a->M + F8_BM - 1) / F8_BM, tiles_n = (a->N + F8_BN - 1) / F8_BN;
  if (tiles_m * tiles_n > 0x7fffffffll) return MRAG_ENOTSUP;
  Gemm8P p{};
  p.A = (const uint8_t*)a->A8; p.W = (const uint8_t*)a->W8; p.ea = a->a_exp; p.ew = a->w_exp;
  p.bias = (const bf16_t*)a->bias; p.C = (bf16_t*)a->C; p.resid = res ? (const bf16_t*)a->resid : nullptr;
  p.M = a->M; p.N = a->N; p.K = a->K; p.lda = a->lda; p.ldw = a->ldw; p.ldc = a->ldc; p.ldr = a->ldr;
  if (!k64) {
    p.gate0 = (const bf16_t*)a->gate0; p.gate1 = (const bf16_t*)a->gate1;
    p.rows_per_batch = a->rows_per_batch; p.split = a->split; p.gate_stride = a->gate_stride;
  }
  p.tiles_m = (int)tiles_m; p.tiles_n = (int)tiles_n; p.group_m = 4;
  void (*kernel)(Gemm8P);
  switch (epi) {
    case MRAG_EPI_NONE: kernel = k64 ? gemm_fp8_kernel<MRAG_EPI_NONE, true> : gemm_fp8_kernel<MRAG_EPI_NONE>; break;
    case MRAG_EPI_RESID: kernel = k64 ? gemm_fp8_kernel<MRAG_EPI_RESID, true> : gemm_fp8_kernel<MRAG_EPI_RESID>; break;
    case MRAG_EPI_GEGLU: kernel = gemm_fp8_kernel<MRAG_EPI_GEGLU, true>; break;
    case MRAG_EPI_GELU_TANH: kernel = gemm_fp8_kernel<MRAG_EPI_GELU_TANH>; break;
    default: kernel = gemm_fp8_kernel<MRAG_EPI_GATE_RESID>; break;
  }
  const int rc = launch_dyn_lds(kernel, dim3((unsigned)(tiles_m * tiles_n)), dim3(512), F8_EPI_LDS, (hipStream_t)stream, p);
  if (rc != MRAG_OK) return rc;
  (void)__atomic_fetch_add(k64 ? &g_fp8_k64_launches[0] : &g_fp8_launches[0], 1ull, __ATOMIC_RELAXED);
  return MRAG_OK;
}

extern "C" int mrag_gemm_fp8_k64(void* stream, const mrag_gemm_fp8_args* a) { return gemm_fp8_launch(stream, a, true); }

extern "C" int mrag_gemm_fp8(void* stream, const mrag_gemm_fp8_args* a) { return gemm_fp8_launch(stream, a, false); }
