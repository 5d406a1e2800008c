// gemm_k320.hip -- K = 320, N a multiple of 320: the weight slice in registers, the activations streamed (gemm_k320_kernel) and its launcher.
#include "gemm_common.h"

namespace {

// ---- K = 320, N a multiple of 320: the UNets' level-0 linears (to_q / to_out / proj_in / proj_out: N = 320; the fused QKV: N = 960; the GEGLU projection:
// N = 2 560 -- 75-95 launches per CFG step over 258 048 / 294 912 pixel rows).  0.05-0.5 TFLOP against 0.4-0.9 GB each: memory-bound -- but a 256x320 or
// 256x256 tile re-stages 160-200 KB of weights per tile and runs load, five short K-tiles and store strictly one after the other with one workgroup per
// CU: 2.4-2.5 TB/s on the plain shapes, 1.4 TB/s with GEGLU (tools/unet_op_table.py).  Here the weight never moves.  A workgroup owns ONE 320-column slice of
// W: its ten waves hold it as MFMA operands in REGISTERS (wave w: slice columns 32 w .. 32 w + 31 = 2 column tiles x 10 k-steps = 80 VGPRs) for its
// lifetime, and streams 64-row activation tiles through a two-stage LDS-DMA ring (40 KB per stage, the K-tile-major swizzled image of the other kernels);
// the outputs leave through an LDS staging tile as whole rows of the slice, the residual added in the row layout.  N / 320 slices x G persistent
// workgroups; block id = slice * G + g with G a multiple of 8, so the workgroups that read the SAME activation tiles (equal g) share an XCD's L2 and the
// activations come from HBM once.  GEGLU: a wave's two column tiles are the value and the gate tile of the same 16 outputs (the 16-row [value | gate]
// interleave of the other GEGLU epilogues).  Same K order and rounding points as the other tiles: bit-equal results.
constexpr int SK320_ROWS = 64, SK320_STAGE = SK320_ROWS * 640, SK320_CPITCH = 656;   // C staging: 64 rows x <= 640 B, pitch 656 B (8-byte writes of 16 rows spread over the banks)

template <int EPI>
__global__ __launch_bounds__(640) void gemm_k320_kernel(const GemmP p) {
  constexpr bool GEGLU = is_geglu<EPI>;
  constexpr int CW = GEGLU ? 160 : 320, CH = CW / 8;        // columns / 16-byte chunks of a staged output row
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* cst = smem + 2 * SK320_STAGE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4, swz = lane & 7;
  const int slices = (int)(p.N / 320), G = (int)gridDim.x / slices;
  const int slice = (int)blockIdx.x / G, g = (int)blockIdx.x - slice * G;
  const int n0 = slice * 320 + wave * 32;                   // the wave's first column of W / bias
  // the wave's weight fragments: W[n0 + 16 j + fr][32 ks + 8 fq .. + 7]
  bf16x8 wf[2][10];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int ks = 0; ks < 10; ++ks) wf[j][ks] = *(const bf16x8*)(p.W + (long long)(n0 + 16 * j + fr) * p.ldw + 32 * ks + 8 * fq);
  u32x2 bias[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) bias[j] = p.bias ? *(const u32x2*)(p.bias + n0 + 16 * j + 4 * fq) : u32x2{0u, 0u};
  const long long c0 = GEGLU ? slice * 160 : slice * 320;   // the slice's first output column
  const int tiles = (int)((p.M + SK320_ROWS - 1) / SK320_ROWS);
  // DMA: piece q = wave + 10 i (i < 4) of a tile: K-tile q / 8, rows 8 (q % 8) .. + 7; lane -> row (lane >> 3), source chunk (lane & 7) ^ row
  auto issue = [&](const int tile, const int stage) {
    const long long m0 = (long long)tile * SK320_ROWS;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = wave + 10 * i, kt = q >> 3;
      long long row = m0 + 8 * (q & 7) + (lane >> 3);
      row = row < p.M ? row : p.M - 1;                      // tail rows re-read the last valid row; their stores are masked
      glds16(p.A + row * p.lda + kt * 64 + (((lane & 7) ^ (lane >> 3)) * 8), smem + stage * SK320_STAGE + q * 1024);
    }
  };
  int tile = g;
  if (tile < tiles) issue(tile, 0);
  for (int it = 0; tile < tiles; ++it, tile += G) {
    const int stage = it & 1;
    const bool more = tile + G < tiles;
    if (more) {
      issue(tile + G, stage ^ 1);                           // (the other stage was released by the barrier that closed the previous iteration)
      // INVARIANT of the counted wait (as in topk.hip): no vector-memory op may be issued between a stage's DMA pieces and their counted wait.  vmcnt retires in
      // order and counts every vector-memory op of the wave; the previous tile's residual loads and C stores all precede `issue`, so "4 outstanding" means exactly
      // the next tile's four pieces.  -DMRAG_DIAG_VMCNT0 turns the wait into vmcnt(0): the results must not change.
#ifdef MRAG_DIAG_VMCNT0
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");      // this tile's four pieces have landed, the next tile's four are in flight
#endif
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    const char* st = smem + stage * SK320_STAGE;
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 10; ++ks) {
      const int off = (ks >> 1) * 8192 + (((fq + 4 * (ks & 1)) ^ swz) * 16);
#pragma unroll
      for (int i = 0; i < 4; i += 2) {                      // two row tiles at a time: 8 fragment registers live (158 VGPRs at three waves per SIMD)
        const bf16x8 a0 = *(const bf16x8*)(st + off + (i * 16 + fr) * 128), a1 = *(const bf16x8*)(st + off + ((i + 1) * 16 + fr) * 128);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][ks], a0, acc[i][j], 0, 0, 0);
          acc[i + 1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][ks], a1, acc[i + 1][j], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);                    // (keeps hipcc from hoisting the next k-steps' fragment reads: they would spill)
    }
    // ---- epilogue: bias (+ scale | GEGLU), ONE rounding to bf16 in the accumulator layout, staged to rows
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v[2][4];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        v[j][0] = acc[i][j][0] + __uint_as_float(bias[j][0] << 16); v[j][1] = acc[i][j][1] + __uint_as_float(bias[j][0] & 0xffff0000u);
        v[j][2] = acc[i][j][2] + __uint_as_float(bias[j][1] << 16); v[j][3] = acc[i][j][3] + __uint_as_float(bias[j][1] & 0xffff0000u);
      }
      if constexpr (GEGLU) {                                // column tile 0: values, tile 1: the gates of the same 16 outputs
        geglu4<EPI == EPI_GEGLU_TANH>(v[0], v[1]);
        *(u32x2*)(cst + (i * 16 + fr) * SK320_CPITCH + (wave * 16 + 4 * fq) * 2) = u32x2{pack_bf2(v[0][0], v[0][1]), pack_bf2(v[0][2], v[0][3])};
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if constexpr (EPI == MRAG_EPI_RESID) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[j][e] *= p.acc_scale;
          }
          *(u32x2*)(cst + (i * 16 + fr) * SK320_CPITCH + (wave * 32 + 16 * j + 4 * fq) * 2) = u32x2{pack_bf2(v[j][0], v[j][1]), pack_bf2(v[j][2], v[j][3])};
        }
      }
    }
    __syncthreads();
    const long long m0 = (long long)tile * SK320_ROWS;
#pragma unroll 2
    for (int idx = tid; idx < SK320_ROWS * CH; idx += 640) {  // whole rows of the slice: CH sixteen-byte chunks per row (two at a time: the 80 weight registers stay live)
      const int row = idx / CH, ch = idx - row * CH;
      const long long m = m0 + row;
      u32x4 val = *(const u32x4*)(cst + row * SK320_CPITCH + ch * 16);
      if (m < p.M) {
        if constexpr (EPI == MRAG_EPI_RESID) {
          const u32x4 rr = *(const u32x4*)(p.resid + m * p.ldr + c0 + ch * 8);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = __uint_as_float(val[e] << 16) + __uint_as_float(rr[e] << 16);
            const float hi = __uint_as_float(val[e] & 0xffff0000u) + __uint_as_float(rr[e] & 0xffff0000u);
            val[e] = pack_bf2(lo, hi);
          }
        }
        *(u32x4*)(p.C + m * p.ldc + c0 + ch * 8) = val;
      }
    }
    __syncthreads();                                        // the staging tile and this stage are free again
  }
}

}  // namespace

extern "C" int launch_k320(hipStream_t s, const GemmP& p, int epi) {
  const int tiles = (int)((p.M + SK320_ROWS - 1) / SK320_ROWS), slices = (int)(p.N / 320);
  int G = (SK_CUS / slices) & ~7;                           // persistent workgroups per slice: a multiple of 8 (block id % 8 = XCD: equal g -> one XCD)
  if (G > tiles) G = tiles >= 8 ? (tiles & ~7) : tiles;
  const dim3 grid((unsigned)(slices * G)), block(640);
  const size_t lds = 2 * SK320_STAGE + SK320_ROWS * SK320_CPITCH;
  int rc;
  switch (epi) {
    case MRAG_EPI_NONE: rc = launch_dyn_lds(gemm_k320_kernel<MRAG_EPI_NONE>, grid, block, lds, s, p); break;
    case MRAG_EPI_RESID: rc = launch_dyn_lds(gemm_k320_kernel<MRAG_EPI_RESID>, grid, block, lds, s, p); break;
    default: return MRAG_ENOTSUP;                           // (the GEGLU form of the template was measured and is not instantiated: k320_applies)
  }
  if (rc != MRAG_OK) return rc;
  MRAG_COUNT(MRAG_K_GEMM_N320K320);
  return MRAG_OK;
}
