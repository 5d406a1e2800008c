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
// Kernel shape: a 256x256 tile on 8 waves (2 x 4, 128 rows x 64 columns each: 4 x 2 accumulators of 32x32), K-tiles of 128 bytes, two LDS stages of
// 64 KiB filled by 16-byte global_load_lds in 1-KiB pieces (8 rows x 128 B) with the XOR swizzle on the SOURCE address (chunk ^= row & 7) and on the
// ds_read_b128 -- the LDS image and idiom of gemm_tile.h with bytes for bf16 pairs.  The DMA of K-tile t + 1 is issued behind the barrier that opens
// tile t and retired by the vmcnt(0) in front of the next barrier.  The fragment reads are hand-written (a compiler-made LDS load would be ordered
// behind the DMA in flight: vmcnt(0)) and released to the MFMAs by counted lgkmcnt.
// Operand maps as measured (tools/exp/fp8_layout_probe.hip): lane l holds A[row l & 31][k = 32 (l >> 5) + byte], B likewise.  W is the A operand
// and the activations the B operand, so a lane owns 4 consecutive output columns of one row per register quad (C/D: column = lane & 31 -> m,
// row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) -> n).  Epilogue: the LDS-staged form of gemm_tile.h (same rounding points: bias / activation / gate
// in the accumulator layout, rounded to bf16, the residual added in the row layout), so C may alias resid.
#include "gemm_common.h"

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

constexpr int G8_BM = 256, G8_BN = 256, G8_BK = 128;        // BK in bytes == e4m3 elements
constexpr int G8_STAGE = (G8_BM + G8_BN) * G8_BK;          // 64 KiB
constexpr int G8_ROWB = 144;                               // staged epilogue: row pitch of a wave's 128 x 64 bf16 tile
constexpr int G8_LDS = 8 * 128 * G8_ROWB;                  // 144 KiB: the epilogue's per-wave regions overlay the two operand stages (128 KiB)
static_assert(G8_LDS >= 2 * G8_STAGE, "the operand stages fit the allocation");

// K64 (mrag_gemm_fp8_k64): p.K % 64 == 0, a last half K-tile is one MFMA step; EPI may be MRAG_EPI_GEGLU (C [M, N / 2])
template <int EPI, bool K64 = false>
__global__ __launch_bounds__(512) void gemm_fp8_kernel(const Gemm8P p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NW = 8, PPW = (G8_BM + G8_BN) / 8 / NW;     // 64 pieces of 1 KiB per stage, 8 per wave: the first 4 are A rows, the others W rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int r32 = lane & 31, hh = lane >> 5;

  // logical tile order of gemm_tile.h: groups of group_m m-tiles walked n-major behind the XCD remap
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int gw = p.group_m * p.tiles_n;
  const int first_m = (wg / gw) * p.group_m;
  const int gsz = min(p.tiles_m - first_m, p.group_m);
  const int tile_m = first_m + (wg % gw) % gsz, tile_n = (wg % gw) / gsz;
  const long long bm0 = (long long)tile_m * G8_BM, bn0 = (long long)tile_n * G8_BN;

  const uint8_t* gsrc[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int piece = wave + i * NW;
    const int r = piece * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ (lane >> 3);             // source-side swizzle: row & 7 == lane >> 3
    if (piece < G8_BM / 8) {
      long long row = bm0 + r;
      row = row < p.M ? row : p.M - 1;                      // clamp: tail rows re-read a valid row, stores are masked
      gsrc[i] = p.A + row * p.lda + chunk * 16;
    } else {
      long long row = bn0 + (r - G8_BM);
      row = row < p.N ? row : p.N - 1;
      gsrc[i] = p.W + row * p.ldw + chunk * 16;
    }
  }
  // K64, last half K-tile: the row has 64 bytes left, so the lanes of chunks 4 .. 7 fetch chunks 0 .. 3 again (a lane's chunk is the same in all its pieces)
  const bool half = K64 && (p.K % G8_BK) != 0;
  const int half_back = (((lane & 7) ^ (lane >> 3)) >= 4) ? -64 : 0;
  auto issue = [&](int stage, int kt, bool clamp = false) {
    char* base = smem + stage * G8_STAGE;
    const long long off = (long long)kt * G8_BK + (clamp ? half_back : 0);
#pragma unroll
    for (int i = 0; i < PPW; ++i) glds16(gsrc[i] + off, base + (wave + i * NW) * 1024);
  };

  // E8M0 scale operands: the lane's W row (A operand) and activation row (B operand) of every 32-row block
  int sw[2], sa[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    long long n = bn0 + wn * 64 + j * 32 + r32;
    n = n < p.N ? n : p.N - 1;
    sw[j] = ((127 - p.ew[n]) & 0xff) * 0x01010101;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    long long m = bm0 + wm * 128 + i * 32 + r32;
    m = m < p.M ? m : p.M - 1;
    sa[i] = ((127 - p.ea[m]) & 0xff) * 0x01010101;
  }

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment read addresses: row r32 of a 32-row block (pitch 4096), bytes 32 hh .. + 31 of the 64-byte k-step as two 16-byte chunks, un-swizzled by row & 7
  const unsigned smem_u = (unsigned)(size_t)smem;
  const int swz = r32 & 7;
  const unsigned rowA = smem_u + (wm * 128 + r32) * 128, rowW = smem_u + G8_BM * 128 + (wn * 64 + r32) * 128;
  unsigned ca[2][2];                                         // [k-step][half]: byte offset of the chunk inside the row
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int c = 0; c < 2; ++c) ca[ks][c] = (unsigned)(((4 * ks + 2 * hh + c) ^ swz) << 4);

  // twelve reads of one k-step in one statement (W blocks first), released by counted lgkmcnt (LDS reads return in order)
#define MRAG8_READ12(W, A, AW0, AW1, AA0, AA1)                                                                      \
  asm volatile(                                                                                                     \
      "ds_read_b128 %0, %12\n\tds_read_b128 %1, %13\n\tds_read_b128 %2, %12 offset:4096\n\tds_read_b128 %3, %13 offset:4096\n\t" \
      "ds_read_b128 %4, %14\n\tds_read_b128 %5, %15\n\tds_read_b128 %6, %14 offset:4096\n\tds_read_b128 %7, %15 offset:4096\n\t" \
      "ds_read_b128 %8, %14 offset:8192\n\tds_read_b128 %9, %15 offset:8192\n\tds_read_b128 %10, %14 offset:12288\n\tds_read_b128 %11, %15 offset:12288" \
      : "=&v"(W[0]), "=&v"(W[1]), "=&v"(W[2]), "=&v"(W[3]), "=&v"(A[0]), "=&v"(A[1]), "=&v"(A[2]), "=&v"(A[3]),      \
        "=&v"(A[4]), "=&v"(A[5]), "=&v"(A[6]), "=&v"(A[7])                                                         \
      : "v"(AW0), "v"(AW1), "v"(AA0), "v"(AA1)                                                                      \
      : "memory")
  // the wait names the registers it releases ("+v"): the MFMAs that read them cannot be scheduled in front of it
#define MRAG8_WAIT_WA(N, W, A0, A1)                                                                                  \
  asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(W[0]), "+v"(W[1]), "+v"(W[2]), "+v"(W[3]), "+v"(A0), "+v"(A1) :: "memory")
#define MRAG8_WAIT_A(N, A0, A1) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(A0), "+v"(A1) :: "memory")
#define MRAG8_FRAG(X, Y) (i32x8{(int)X[0], (int)X[1], (int)X[2], (int)X[3], (int)Y[0], (int)Y[1], (int)Y[2], (int)Y[3]})
#define MRAG8_ROW(I, W, A0, A1)                                                                                      \
  do {                                                                                                              \
    const i32x8 af = MRAG8_FRAG(A0, A1);                                                                            \
    acc[I][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(MRAG8_FRAG(W[0], W[1]), af, acc[I][0], 0, 0, 0, sw[0], 0, sa[I]); \
    acc[I][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(MRAG8_FRAG(W[2], W[3]), af, acc[I][1], 0, 0, 0, sw[1], 0, sa[I]); \
  } while (0)

  const int nk = (int)((p.K + (K64 ? G8_BK - 1 : 0)) / G8_BK);
  issue(0, 0, half && nk == 1);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");   // tile kt landed for every wave; every wave finished reading the other stage
    const unsigned so = (unsigned)((kt & 1) * G8_STAGE);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (K64 && ks == 1 && half && kt == nk - 1) break;             // (workgroup-uniform) the half tile has no second step
      u32x4 w[4], a[8];
      MRAG8_READ12(w, a, rowW + so + ca[ks][0], rowW + so + ca[ks][1], rowA + so + ca[ks][0], rowA + so + ca[ks][1]);
      if (ks == 0 && kt + 1 < nk) issue((kt + 1) & 1, kt + 1, half && kt + 2 == nk);    // the next tile's eight DMA requests go out under the first fragments' LDS latency
      // the order below is the schedule (hipcc would gather the four waits in front of the first MFMA): each pair of MFMAs starts when ITS rows are here
      __builtin_amdgcn_sched_barrier(0);
      MRAG8_WAIT_WA(6, w, a[0], a[1]);
      MRAG8_ROW(0, w, a[0], a[1]);
      __builtin_amdgcn_sched_barrier(0);
      MRAG8_WAIT_A(4, a[2], a[3]);
      MRAG8_ROW(1, w, a[2], a[3]);
      __builtin_amdgcn_sched_barrier(0);
      MRAG8_WAIT_A(2, a[4], a[5]);
      MRAG8_ROW(2, w, a[4], a[5]);
      __builtin_amdgcn_sched_barrier(0);
      MRAG8_WAIT_A(0, a[6], a[7]);
      MRAG8_ROW(3, w, a[6], a[7]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#undef MRAG8_READ12
#undef MRAG8_WAIT_WA
#undef MRAG8_WAIT_A
#undef MRAG8_FRAG
#undef MRAG8_ROW

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
  char* wbase = smem + wave * (128 * G8_ROWB);
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
            const u32x2 bv = *(const u32x2*)(p.bias + n), bg = *(const u32x2*)(p.bias + n + 16);
            v[0] += __uint_as_float(bv[0] << 16); v[1] += __uint_as_float(bv[0] & 0xffff0000u);
            v[2] += __uint_as_float(bv[1] << 16); v[3] += __uint_as_float(bv[1] & 0xffff0000u);
            gt[0] += __uint_as_float(bg[0] << 16); gt[1] += __uint_as_float(bg[0] & 0xffff0000u);
            gt[2] += __uint_as_float(bg[1] << 16); gt[3] += __uint_as_float(bg[1] & 0xffff0000u);
          }
          geglu4<false>(v, gt);
          u32x2 out;
          out[0] = pack_bf2(v[0], v[1]);
          out[1] = pack_bf2(v[2], v[3]);
          *(u32x2*)(wbase + lrow * G8_ROWB + (j * 16 + 8 * g + 4 * hh) * 2) = out;
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
        if (p.bias) {
          const u32x2 bb = *(const u32x2*)(p.bias + n);
          v[0] += __uint_as_float(bb[0] << 16); v[1] += __uint_as_float(bb[0] & 0xffff0000u);
          v[2] += __uint_as_float(bb[1] << 16); v[3] += __uint_as_float(bb[1] & 0xffff0000u);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = epi_act<EPI>(v[e]);
        if constexpr (EPI == MRAG_EPI_GATE_RESID) {
          const u32x2 gg = *(const u32x2*)(gate + n);
          v[0] *= __uint_as_float(gg[0] << 16); v[1] *= __uint_as_float(gg[0] & 0xffff0000u);
          v[2] *= __uint_as_float(gg[1] << 16); v[3] *= __uint_as_float(gg[1] & 0xffff0000u);
        }
        u32x2 out;
        out[0] = pack_bf2(v[0], v[1]);
        out[1] = pack_bf2(v[2], v[3]);
        *(u32x2*)(wbase + lrow * G8_ROWB + lcol * 2) = out;
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
      const u32x4 val = *(const u32x4*)(wbase + row * G8_ROWB + chunk * 16);
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
    u32x4 val = *(const u32x4*)(wbase + row * G8_ROWB + chunk * 16);
    if (m < p.M && n_ok) {
      if constexpr (EPI == MRAG_EPI_GATE_RESID || EPI == MRAG_EPI_RESID) {
        const u32x4 rr = rpre[g];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = __uint_as_float(val[e] << 16) + __uint_as_float(rr[e] << 16);
          const float hi = __uint_as_float(val[e] & 0xffff0000u) + __uint_as_float(rr[e] & 0xffff0000u);
          val[e] = pack_bf2(lo, hi);
        }
      }
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

extern "C" int mrag_gemm_fp8_k64(void* stream, const mrag_gemm_fp8_args* a) {
  if (!a || !a->A8 || !a->W8 || !a->a_exp || !a->w_exp || !a->C) return MRAG_EINVAL;
  if (a->M < 1 || a->N < 1 || a->K < 1) return MRAG_EINVAL;
  const int epi = a->epilogue;
  if (epi != MRAG_EPI_NONE && epi != MRAG_EPI_RESID && epi != MRAG_EPI_GEGLU) return MRAG_ENOTSUP;
  const bool glu = epi == MRAG_EPI_GEGLU, res = epi == MRAG_EPI_RESID;
  if (a->K % 64 != 0 || a->N % (glu ? 32 : 16) != 0) return MRAG_ENOTSUP;
  const long long ncols = glu ? a->N / 2 : a->N;             // columns of C
  if (a->lda < a->K || a->ldw < a->K || a->ldc < ncols) return MRAG_EINVAL;
  // the pointer and alignment checks of mrag_gemm_fp8
  if ((((uintptr_t)a->A8 | (uintptr_t)a->W8) & 15) || a->lda % 16 != 0 || a->ldw % 16 != 0) return MRAG_EINVAL;
  if ((((uintptr_t)a->a_exp | (uintptr_t)a->w_exp) & 3) || (a->bias && ((uintptr_t)a->bias & 7))) return MRAG_EINVAL;
  if (res && (!a->resid || a->ldr < a->N)) return MRAG_EINVAL;
  if (!rows_16B_aligned(a->C, a->ldc, res ? a->resid : nullptr, a->ldr)) return MRAG_EINVAL;
  const long long tiles_m = (a->M + G8_BM - 1) / G8_BM, tiles_n = (a->N + G8_BN - 1) / G8_BN;
  if (tiles_m * tiles_n > 0x7fffffffll) return MRAG_ENOTSUP;
  Gemm8P p{};
  p.A = (const uint8_t*)a->A8; p.W = (const uint8_t*)a->W8; p.ea = a->a_exp; p.ew = a->w_exp;
  p.bias = (const bf16_t*)a->bias; p.C = (bf16_t*)a->C; p.resid = res ? (const bf16_t*)a->resid : nullptr;
  p.M = a->M; p.N = a->N; p.K = a->K; p.lda = a->lda; p.ldw = a->ldw; p.ldc = a->ldc; p.ldr = a->ldr;
  p.tiles_m = (int)tiles_m; p.tiles_n = (int)tiles_n; p.group_m = 4;
  const dim3 grid((unsigned)(tiles_m * tiles_n)), block(512);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  switch (epi) {
    case MRAG_EPI_NONE: rc = launch_dyn_lds(gemm_fp8_kernel<MRAG_EPI_NONE, true>, grid, block, G8_LDS, s, p); break;
    case MRAG_EPI_RESID: rc = launch_dyn_lds(gemm_fp8_kernel<MRAG_EPI_RESID, true>, grid, block, G8_LDS, s, p); break;
    default: rc = launch_dyn_lds(gemm_fp8_kernel<MRAG_EPI_GEGLU, true>, grid, block, G8_LDS, s, p); break;
  }
  if (rc != MRAG_OK) return rc;
  (void)__atomic_fetch_add(&g_fp8_k64_launches[0], 1ull, __ATOMIC_RELAXED);
  return MRAG_OK;
}

extern "C" int mrag_gemm_fp8(void* stream, const mrag_gemm_fp8_args* a) {
  if (!a || !a->A8 || !a->W8 || !a->a_exp || !a->w_exp || !a->C) return MRAG_EINVAL;
  if (a->M < 1 || a->N < 1 || a->K < 1) return MRAG_EINVAL;
  const int epi = a->epilogue;
  if (epi != MRAG_EPI_NONE && epi != MRAG_EPI_GELU_TANH && epi != MRAG_EPI_RESID && epi != MRAG_EPI_GATE_RESID) return MRAG_ENOTSUP;
  if (a->K % G8_BK != 0 || a->N % 16 != 0) return MRAG_ENOTSUP;
  if (a->lda < a->K || a->ldw < a->K || a->ldc < a->N) return MRAG_EINVAL;
  // 16-byte aligned rows of both operands (the DMA moves 16-byte chunks) and of C / resid (the staged epilogue's row segments); 8-byte bias / gate reads
  if ((((uintptr_t)a->A8 | (uintptr_t)a->W8) & 15) || a->lda % 16 != 0 || a->ldw % 16 != 0) return MRAG_EINVAL;
  if ((((uintptr_t)a->a_exp | (uintptr_t)a->w_exp) & 3) || (a->bias && ((uintptr_t)a->bias & 7))) return MRAG_EINVAL;
  const bool res = epi == MRAG_EPI_RESID || epi == MRAG_EPI_GATE_RESID;
  if (res && (!a->resid || a->ldr < a->N)) return MRAG_EINVAL;
  if (!rows_16B_aligned(a->C, a->ldc, res ? a->resid : nullptr, a->ldr)) return MRAG_EINVAL;
  if (epi == MRAG_EPI_GATE_RESID) {
    if (!a->gate0 || !a->gate1 || a->rows_per_batch < 1) return MRAG_EINVAL;
    if ((((uintptr_t)a->gate0 | (uintptr_t)a->gate1) & 7) || a->gate_stride % 4 != 0) return MRAG_EINVAL;
  }
  const long long tiles_m = (a->M + G8_BM - 1) / G8_BM, tiles_n = (a->N + G8_BN - 1) / G8_BN;
  if (tiles_m * tiles_n > 0x7fffffffll) return MRAG_ENOTSUP;
  Gemm8P p{};
  p.A = (const uint8_t*)a->A8; p.W = (const uint8_t*)a->W8; p.ea = a->a_exp; p.ew = a->w_exp;
  p.bias = (const bf16_t*)a->bias; p.C = (bf16_t*)a->C; p.resid = res ? (const bf16_t*)a->resid : nullptr;
  p.gate0 = (const bf16_t*)a->gate0; p.gate1 = (const bf16_t*)a->gate1;
  p.M = a->M; p.N = a->N; p.K = a->K; p.lda = a->lda; p.ldw = a->ldw; p.ldc = a->ldc; p.ldr = a->ldr;
  p.rows_per_batch = a->rows_per_batch; p.split = a->split; p.gate_stride = a->gate_stride;
  p.tiles_m = (int)tiles_m; p.tiles_n = (int)tiles_n; p.group_m = 4;
  const dim3 grid((unsigned)(tiles_m * tiles_n)), block(512);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  switch (epi) {
    case MRAG_EPI_NONE: rc = launch_dyn_lds(gemm_fp8_kernel<MRAG_EPI_NONE>, grid, block, G8_LDS, s, p); break;
    case MRAG_EPI_GELU_TANH: rc = launch_dyn_lds(gemm_fp8_kernel<MRAG_EPI_GELU_TANH>, grid, block, G8_LDS, s, p); break;
    case MRAG_EPI_RESID: rc = launch_dyn_lds(gemm_fp8_kernel<MRAG_EPI_RESID>, grid, block, G8_LDS, s, p); break;
    default: rc = launch_dyn_lds(gemm_fp8_kernel<MRAG_EPI_GATE_RESID>, grid, block, G8_LDS, s, p); break;
  }
  if (rc != MRAG_OK) return rc;
  (void)__atomic_fetch_add(&g_fp8_launches[0], 1ull, __ATOMIC_RELAXED);
  return MRAG_OK;
}
