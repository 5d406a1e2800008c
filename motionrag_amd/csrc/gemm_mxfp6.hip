// gemm_mxfp6.hip -- the opt-in MXFP6 path of the DiT's four large linears (cogvideox.set_linear_precision(model, "mxfp6")): both operands OCP e2m3
// in blocks of 32 along K with one E8M0 scale byte per block, on v_mfma_scale_f32_32x32x64_f8f6f4 cbsz:2 blgp:2 (six operand registers per side).
//
//   mrag_quant_rows_mxfp6    x [M, K] bf16 -> packed e2m3 + scale bytes [M, K / 32] (include/mrag_hip.h states the format).  One pass: a lane reads the
//                            64 bytes of one (row, block), takes their maximum, and writes the block's 24 bytes and its scale byte.
//   mrag_dequant_rows_mxfp6  the packed operand and its scales back to bf16 (exact): the one reader of the layout outside the kernels.
//   mrag_gemm_mxfp6          C = epilogue(sum_k A[m, k] W[n, k] + bias): the 256 x 256 / 8-wave tile of gemm_fp8_tile.h (its tile order, its staged
//                            epilogue and rounding points) with 6-bit operands; the block scales ride the instruction's scale operands.
//
// Operand map as measured (tools/exp/mxfp6_layout_probe.hip, profiles/mxfp6_layout_probe.txt): lane l holds row l & 31, k = 32 (l >> 5) + j for
// j = 0 .. 31 -- element j in bits 6 j .. 6 j + 5 of the lane's 192 operand bits (register 0 lowest), a code being sign | exponent (2, bias 1) |
// mantissa (3).  Byte 0 of the lane's scale register applies to exactly these 32 k's: one MX block.  C / D as for e4m3 (gemm_fp8_tile.h).
//
// Packed layout (fragment-major, written by the quantiser): tiles of 32 rows x 64 k, 1536 bytes each, tile (r, c) = rows 32 r .. + 31, k 64 c .. + 63 at
// byte 1536 (r K / 64 + c).  A tile is the MFMA operand of its 64 lanes: bytes 0 .. 15 of lane l's 24 at 16 l, bytes 16 .. 23 at 1024 + 8 l.  Rows
// behind M in the last row block are zeros.  Why: a K-tile of a row block is 3072 contiguous bytes, so the DMA is three plain 1-KiB pieces with no
// swizzle (row-major 24-byte groups would make 96-byte row pitches that a 16-byte-per-lane global_load_lds cannot tile into whole rows), and the
// fragment reads are one ds_read_b128 and one ds_read_b64 per lane at consecutive addresses: no bank conflict.
//
// LDS: two operand stages of 48 KiB (row blocks 0 .. 7 of the activations, then 8 of W; each 2 k-steps x 1536), behind them two stages of 2 KiB with
// the K-tile's four scale bytes of each of the 512 rows (a 4-byte global_load_lds per row: scale rows are [rows, K / 32] bytes, so a K-tile is one
// aligned word).  The DMA goes out in the scalar-base form (glds16_sbase), which the compiler's wait bookkeeping does not see, so the fragment reads
// are plain LDS loads that it orders and counts itself (a load behind a visible LDS DMA would wait for vmcnt(0)); the kernel retires the DMA by the
// vmcnt(0) in front of the barrier that opens the tile.
#include "gemm_fp8_tile.h"

// host-side relaxed launch counters (mrag_mxfp6_launch_counts): slot 0 the GEMM, slot 1 the quantiser, slot 2 the dequantiser
static unsigned long long g_mx6_launches[3];

namespace {

constexpr int MX6_TILE = 1536, MX6_LO = 1024;   // a 32 x 64 tile; its 16-byte plane
constexpr int MX6_RB = 2 * MX6_TILE;            // a row block's K-tile of 128: two k-steps
constexpr int MX6_STAGE = 16 * MX6_RB;          // 48 KiB: 8 activation row blocks, 8 of W
constexpr int MX6_SC = 2 * MX6_STAGE;           // the scale words: 2 stages of (256 + 256) rows x 4 bytes
static_assert(MX6_SC + 2 * 2048 <= F8_EPI_LDS, "the stages fit the epilogue's allocation");

// ------------------------------------------------------------------------------------------------ quantiser / dequantiser
// round-to-nearest-even of v (|v| <= 7.5 under the block's scale; clamped there) onto the e2m3 grid: the grid is uniform with step 1/8 below 2,
// 1/4 below 4 and 1/2 above, and the code's parity is that of the rounded multiple, so rintf's ties-to-even are ties to the even mantissa code
__device__ __forceinline__ unsigned e2m3_code(const float v) {
  const float a = fminf(fabsf(v), 7.5f);
  const float mul = a < 2.0f ? 8.0f : (a < 4.0f ? 4.0f : 2.0f);
  const unsigned add = a < 2.0f ? 0u : (a < 4.0f ? 8u : 16u);
  const unsigned mag = (unsigned)(int)rintf(a * mul) + add;
  return mag ? (mag | ((__float_as_uint(v) >> 26) & 32u)) : 0u;
}

// a wave per tile: lane l <-> row 32 r + (l & 31), block 2 c + (l >> 5), which is the lane that holds the block in the MFMA
__global__ __launch_bounds__(256) void quant_mxfp6_kernel(const bf16_t* __restrict__ x, uint8_t* __restrict__ xq, uint8_t* __restrict__ sc, const long long M,
                                                           const int kt64, const long long ldx, const long long ntiles) {
  const int lane = threadIdx.x & 63;
  const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= ntiles) return;
  const long long rb = t / kt64;
  const int blk = 2 * (int)(t - rb * kt64) + (lane >> 5);
  const long long row = rb * 32 + (lane & 31);
  u32x4 v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = u32x4{0u, 0u, 0u, 0u};
  if (row < M) {
    const bf16_t* src = x + row * ldx + blk * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = *(const u32x4*)(src + 8 * i);
  }
  unsigned m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) m = absmax8(m, v[i]);
  // smallest s with amax 2^-s <= 7.5 = 1.875 * 2^2: from amax = 1.f * 2^e (bf16: 7 mantissa bits, 1.875 = mantissa 0x70), s = e - 2, one more above 1.875
  const unsigned b = m >> 16;
  int s = 0;
  if (b) {
    s = (int)(b >> 7) - 129 + ((b & 0x7f) > 0x70 ? 1 : 0);
    s = s < -60 ? -60 : (s > 60 ? 60 : s);
  }
  const float mul = ldexpf(1.0f, -s);
  unsigned long long w[3] = {0ull, 0ull, 0ull};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const unsigned pair = v[j >> 2][j & 3];
    const unsigned c[2] = {e2m3_code(__uint_as_float(pair << 16) * mul), e2m3_code(__uint_as_float(pair & 0xffff0000u) * mul)};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int bit = 6 * (2 * j + h), q = bit >> 6, sh = bit & 63;
      w[q] |= (unsigned long long)c[h] << sh;
      if (sh > 58) w[q + 1] |= (unsigned long long)c[h] >> (64 - sh);
    }
  }
  uint8_t* dst = xq + t * MX6_TILE;
  *(u32x4*)(dst + lane * 16) = u32x4{(unsigned)w[0], (unsigned)(w[0] >> 32), (unsigned)w[1], (unsigned)(w[1] >> 32)};
  *(u32x2*)(dst + MX6_LO + lane * 8) = u32x2{(unsigned)w[2], (unsigned)(w[2] >> 32)};
  if (row < M) sc[row * (2 * kt64) + blk] = (uint8_t)(127 + s);
}

__global__ __launch_bounds__(256) void dequant_mxfp6_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ sc, bf16_t* __restrict__ y, const long long M,
                                                             const int kt64, const long long ldy, const long long ntiles) {
  const int lane = threadIdx.x & 63;
  const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= ntiles) return;
  const long long rb = t / kt64;
  const int blk = 2 * (int)(t - rb * kt64) + (lane >> 5);
  const long long row = rb * 32 + (lane & 31);
  if (row >= M) return;
  const uint8_t* src = xq + t * MX6_TILE;
  const u32x4 lo = *(const u32x4*)(src + lane * 16);
  const u32x2 hi = *(const u32x2*)(src + MX6_LO + lane * 8);
  const unsigned long long w[3] = {lo[0] | ((unsigned long long)lo[1] << 32), lo[2] | ((unsigned long long)lo[3] << 32), hi[0] | ((unsigned long long)hi[1] << 32)};
  const float unit = ldexpf(1.0f, (int)sc[row * (2 * kt64) + blk] - 127 - 3);   // a code's integer mantissa counts eighths
  unsigned out[16];
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int bit = 6 * j, q = bit >> 6, sh = bit & 63;
    unsigned c = (unsigned)(w[q] >> sh);
    if (sh > 58) c |= (unsigned)(w[q + 1] << (64 - sh));
    const unsigned e = (c >> 3) & 3u, mant = c & 7u;
    const float val = (float)(e ? (8u + mant) << (e - 1) : mant) * unit;        // <= 4 significant bits times a power of two: exact in bf16
    const unsigned bits = (__float_as_uint(val) >> 16) | ((c & 32u) << 10);
    if (j & 1) out[j >> 1] |= bits << 16;
    else out[j >> 1] = bits;
  }
  bf16_t* dst = y + row * ldy + blk * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) *(u32x4*)(dst + 8 * i) = u32x4{out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]};
}

// ------------------------------------------------------------------------------------------------ GEMM
struct Mx6P {
  const uint8_t* A; const uint8_t* W; const uint8_t* sa; const uint8_t* sw;
  const bf16_t* bias; bf16_t* C; const bf16_t* resid; const bf16_t* gate0; const bf16_t* gate1;
  long long M, N, K, ldc, ldr, rows_per_batch, split, gate_stride;
  long long rb_pitch;          // bytes of one row block of a packed operand: 1536 K / 64
  int rbm, rbn;                // row blocks of A and W
  int tiles_m, tiles_n, group_m;
};

// the 4-byte form of glds16_sbase (common.h): source = sbase (wave-uniform) + voff (per-lane bytes), LDS destination lds_addr + 4 lane
__device__ __forceinline__ void glds4_sbase(const void* sbase, unsigned voff, unsigned lds_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 4\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(sbase), "s"(lds_addr)
               : "memory");
}

// a lane's operand of one tile at `tile` (LDS): 16 + 8 bytes into the six registers the f6 form reads
__device__ __forceinline__ i32x8 mx6_frag(const char* tile, const int lane) {
  const u32x4 x = *(const u32x4*)(tile + lane * 16);
  const u32x2 y = *(const u32x2*)(tile + MX6_LO + lane * 8);
  return i32x8{(int)x[0], (int)x[1], (int)x[2], (int)x[3], (int)y[0], (int)y[1], 0, 0};
}

template <int EPI>
__global__ __launch_bounds__(512) void gemm_mxfp6_kernel(const Mx6P p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NW = 8, PPW = 48 / NW;                     // 48 pieces of 1 KiB per stage, 6 per wave: piece q is third q % 3 of row block q / 3
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform, and known to be: the DMA's bases sit in SGPRs)
  const int wm = wave >> 2, wn = wave & 3;
  const int r32 = lane & 31, hh = lane >> 5;

  long long bm0, bn0;
  fp8_tile_origin(p.tiles_m, p.tiles_n, p.group_m, bm0, bn0);

  // DMA sources: a piece's row block is the wave's (uniform base, K-tile 0); the lane's 16 bytes of the piece are the per-lane offset
  const uint8_t* gsrc[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int q = wave + i * NW, rbi = q / 3, part = q % 3;
    if (rbi < 8) {
      int rb = (int)(bm0 / 32) + rbi;
      rb = rb < p.rbm ? rb : p.rbm - 1;                    // clamp: row blocks behind the last re-read it, their stores are masked
      gsrc[i] = p.A + rb * p.rb_pitch + part * 1024;
    } else {
      int rb = (int)(bn0 / 32) + rbi - 8;
      rb = rb < p.rbn ? rb : p.rbn - 1;
      gsrc[i] = p.W + rb * p.rb_pitch + part * 1024;
    }
  }
  // the scale words: waves 0 .. 3 fetch those of activation rows 64 wave + lane, waves 4 .. 7 those of W rows 64 (wave - 4) + lane (the host checked
  // that rows * K / 32 fits the 32-bit lane offset)
  const uint8_t* ssrc = wave < 4 ? p.sa : p.sw;
  unsigned soff;
  {
    long long row = (wave < 4 ? bm0 + wave * 64 : bn0 + (wave - 4) * 64) + lane;
    const long long rows = wave < 4 ? p.M : p.N;
    row = row < rows ? row : rows - 1;
    soff = (unsigned)(row * (p.K / 32));
  }
  const unsigned smem_u = (unsigned)(size_t)smem;
  auto issue = [&](int stage, int kt) {
    const unsigned base = smem_u + stage * MX6_STAGE;
#pragma unroll
    for (int i = 0; i < PPW; ++i) glds16_sbase(gsrc[i] + (long long)kt * MX6_RB, lane * 16, base + (wave + i * NW) * 1024);
    glds4_sbase(ssrc + kt * 4, soff, smem_u + MX6_SC + stage * 2048 + wave * 256);
  };

  f32x16 acc[4][2] = {};
  const int nk = (int)(p.K / F8_BK);
  const unsigned sh = 8u * hh;                             // the bit of the lane's block in a k-step's half of the scale word
  issue(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");   // tile kt landed for every wave; every wave finished reading the other stage
    const char* st = smem + (kt & 1) * MX6_STAGE;
    const unsigned* scs = (const unsigned*)(smem + MX6_SC + (kt & 1) * 2048);
    unsigned sw[2], sa[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) sw[j] = scs[256 + wn * 64 + j * 32 + r32];
#pragma unroll
    for (int i = 0; i < 4; ++i) sa[i] = scs[wm * 128 + i * 32 + r32];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      i32x8 wf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) wf[j] = mx6_frag(st + (8 + wn * 2 + j) * MX6_RB + ks * MX6_TILE, lane);
      if (ks == 0 && kt + 1 < nk) issue((kt + 1) & 1, kt + 1);        // the next tile's DMA requests go out under the first fragments' LDS latency
      const int s_w[2] = {(int)((sw[0] >> (16 * ks + sh)) & 0xffu), (int)((sw[1] >> (16 * ks + sh)) & 0xffu)};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const i32x8 af = mx6_frag(st + (wm * 4 + i) * MX6_RB + ks * MX6_TILE, lane);
        const int s_a = (int)((sa[i] >> (16 * ks + sh)) & 0xffu);
        acc[i][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[0], af, acc[i][0], 2, 2, 0, s_w[0], 0, s_a);
        acc[i][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[1], af, acc[i][1], 2, 2, 0, s_w[1], 0, s_a);
      }
    }
  }

  // ---- epilogue: that of gemm_fp8_kernel (LDS-staged; bias / activation / gate in the accumulator layout, the residual add in the row layout)
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
  __syncthreads();   // every wave is done with the stages that these per-wave regions overlay (no DMA is in flight: the last tile issued none)
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

// tiles of a [rows, K] operand; 0 when the shape has none
inline long long mx6_tiles(long long rows, long long K) { return (rows < 1 || K < 64 || K % 64 != 0) ? 0 : (rows + 31) / 32 * (K / 64); }

}  // namespace

extern "C" int mrag_mxfp6_launch_counts(uint64_t* out_host, int32_t n) {
  for (int i = 0; out_host && i < n && i < 3; ++i) out_host[i] = __atomic_load_n(&g_mx6_launches[i], __ATOMIC_RELAXED);
  return 3;
}

extern "C" int64_t mrag_mxfp6_packed_bytes(int64_t M, int64_t K) { return mx6_tiles(M, K) * MX6_TILE; }

extern "C" int64_t mrag_mxfp6_scale_bytes(int64_t M, int64_t K) { return mx6_tiles(M, K) ? M * (K / 32) : 0; }

extern "C" int mrag_quant_rows_mxfp6(void* stream, const void* x, void* xq, void* scale, int64_t M, int64_t K, int64_t ldx) {
  if (!x || !xq || !scale || M < 1 || K < 1 || M > 0x7fffffffll) return MRAG_EINVAL;
  if (K % 64 != 0 || K > (1ll << 30) || ldx % 8 != 0 || ldx < K) return MRAG_ENOTSUP;
  if (((uintptr_t)x | (uintptr_t)xq) & 15) return MRAG_ENOTSUP;
  const long long ntiles = mx6_tiles(M, K);
  if ((ntiles + 3) / 4 > 0x7fffffffll) return MRAG_ENOTSUP;
  MRAG_LAUNCH(quant_mxfp6_kernel, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (uint8_t*)xq, (uint8_t*)scale, (long long)M,
              (int)(K / 64), (long long)ldx, ntiles);
  MRAG_LAUNCH_CHECK();
  (void)__atomic_fetch_add(&g_mx6_launches[1], 1ull, __ATOMIC_RELAXED);
  return MRAG_OK;
}

extern "C" int mrag_dequant_rows_mxfp6(void* stream, const void* xq, const void* scale, void* y, int64_t M, int64_t K, int64_t ldy) {
  if (!xq || !scale || !y || M < 1 || K < 1 || M > 0x7fffffffll) return MRAG_EINVAL;
  if (K % 64 != 0 || K > (1ll << 30) || ldy % 8 != 0 || ldy < K) return MRAG_ENOTSUP;
  if (((uintptr_t)y | (uintptr_t)xq) & 15) return MRAG_ENOTSUP;
  const long long ntiles = mx6_tiles(M, K);
  if ((ntiles + 3) / 4 > 0x7fffffffll) return MRAG_ENOTSUP;
  MRAG_LAUNCH(dequant_mxfp6_kernel, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)xq, (const uint8_t*)scale, (bf16_t*)y, (long long)M,
              (int)(K / 64), (long long)ldy, ntiles);
  MRAG_LAUNCH_CHECK();
  (void)__atomic_fetch_add(&g_mx6_launches[2], 1ull, __ATOMIC_RELAXED);
  return MRAG_OK;
}

extern "C" int mrag_gemm_mxfp6(void* stream, const mrag_gemm_fp8_args* a, const void* a_scale, const void* w_scale) {
  if (!a || !a->A8 || !a->W8 || !a_scale || !w_scale || !a->C) return MRAG_EINVAL;
  if (a->M < 1 || a->N < 1 || a->K < 1) return MRAG_EINVAL;
  const int epi = a->epilogue;
  const bool gated = epi == MRAG_EPI_GATE_RESID;
  if (epi != MRAG_EPI_NONE && epi != MRAG_EPI_RESID && epi != MRAG_EPI_GELU_TANH && !gated) return MRAG_ENOTSUP;
  if (a->K % F8_BK != 0 || a->N % 16 != 0 || a->M > 0x7fffffffll || a->N > 0x7fffffffll) return MRAG_ENOTSUP;
  if (a->M * (a->K / 32) > 0xffffffffll || a->N * (a->K / 32) > 0xffffffffll) return MRAG_ENOTSUP;   // a scale row's offset is a 32-bit lane offset
  if (a->ldc < a->N) return MRAG_EINVAL;
  // 16-byte aligned packed operands (the DMA moves 16-byte chunks), word-aligned scale rows (K / 32 is a multiple of 4), 16-byte rows of C / resid
  // (the staged epilogue's row segments), 8-byte bias / gate reads
  if ((((uintptr_t)a->A8 | (uintptr_t)a->W8) & 15) || (((uintptr_t)a_scale | (uintptr_t)w_scale) & 3) || (a->bias && ((uintptr_t)a->bias & 7))) return MRAG_EINVAL;
  const bool res = epi == MRAG_EPI_RESID || gated;
  if (res && (!a->resid || a->ldr < a->N)) return MRAG_EINVAL;
  if (!rows_16B_aligned(a->C, a->ldc, res ? a->resid : nullptr, a->ldr)) return MRAG_EINVAL;
  if (gated) {
    if (!a->gate0 || !a->gate1 || a->rows_per_batch < 1) return MRAG_EINVAL;
    if ((((uintptr_t)a->gate0 | (uintptr_t)a->gate1) & 7) || a->gate_stride % 4 != 0) return MRAG_EINVAL;
  }
  const long long tiles_m = (a->M + F8_BM - 1) / F8_BM, tiles_n = (a->N + F8_BN - 1) / F8_BN;
  if (tiles_m * tiles_n > 0x7fffffffll) return MRAG_ENOTSUP;
  Mx6P p{};
  p.A = (const uint8_t*)a->A8; p.W = (const uint8_t*)a->W8; p.sa = (const uint8_t*)a_scale; p.sw = (const uint8_t*)w_scale;
  p.bias = (const bf16_t*)a->bias; p.C = (bf16_t*)a->C; p.resid = res ? (const bf16_t*)a->resid : nullptr;
  p.M = a->M; p.N = a->N; p.K = a->K; p.ldc = a->ldc; p.ldr = a->ldr;
  if (gated) {
    p.gate0 = (const bf16_t*)a->gate0; p.gate1 = (const bf16_t*)a->gate1;
    p.rows_per_batch = a->rows_per_batch; p.split = a->split; p.gate_stride = a->gate_stride;
  }
  p.rb_pitch = a->K / 64 * MX6_TILE;
  p.rbm = (int)((a->M + 31) / 32); p.rbn = (int)((a->N + 31) / 32);
  p.tiles_m = (int)tiles_m; p.tiles_n = (int)tiles_n; p.group_m = 4;
  void (*kernel)(Mx6P);
  switch (epi) {
    case MRAG_EPI_NONE: kernel = gemm_mxfp6_kernel<MRAG_EPI_NONE>; break;
    case MRAG_EPI_RESID: kernel = gemm_mxfp6_kernel<MRAG_EPI_RESID>; break;
    case MRAG_EPI_GELU_TANH: kernel = gemm_mxfp6_kernel<MRAG_EPI_GELU_TANH>; break;
    default: kernel = gemm_mxfp6_kernel<MRAG_EPI_GATE_RESID>; break;
  }
  const int rc = launch_dyn_lds(kernel, dim3((unsigned)(tiles_m * tiles_n)), dim3(512), F8_EPI_LDS, (hipStream_t)stream, p);
  if (rc != MRAG_OK) return rc;
  (void)__atomic_fetch_add(&g_mx6_launches[0], 1ull, __ATOMIC_RELAXED);
  return MRAG_OK;
}
