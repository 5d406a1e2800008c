// conv_fp8.hip -- the opt-in e4m3 path of the 3x3 convolutions (layers.conv3x3: the UNets' ResBlocks and the VAE decoders' ResnetBlocks):
//
//   mrag_conv_fp8   y[n, ho, wo, co] = epilogue(2^-ew[co] * sum_{ky,kx,ci} 2^-ex[pixel(n, ho+ky-1, wo+kx-1)] x8[..] W8[co, (ky,kx,ci)] + bias[co])
//                   3x3, stride 1, zero padding 1, as an implicit GEMM (M = N H W output pixels, N = Cout, K = 9 Cin) on
//                   v_mfma_scale_f32_32x32x64_f8f6f4.  x8 / ex come from mrag_quant_rows_e4m3 over the N H W pixel rows of Cin channels (one
//                   power-of-two exponent per INPUT pixel), W8 / ew from the same quantiser over the [Cout, 9 Cin] tap-major weight.
//
// Why a per-pixel exponent survives the gather: at Cin % 64 == 0 one MFMA k-step of 64 e4m3 lies inside ONE tap, and the instruction's E8M0 scale operand
// applies per lane to that lane's own row's 32 k's (gemm_fp8_tile.h, operand maps).  So for every k-step a lane passes 127 - e of the SOURCE pixel its output
// row reads under that step's tap.  A padded tap gathers zero bytes; its scale is immaterial.
//
// Kernel shape: the e4m3 256x256 tile of gemm_fp8_tile.h (shared with gemm_fp8_kernel: stages, fragment reads, k-step schedule, staged epilogue) with the
// tap walk and the border predicate of gemm_tile.h's CONV == 1 addressing on the activation operand.
// K-tile: 128 bytes = TWO 64-channel steps, each a whole step of one tap, addressed independently.  A DMA lane moves one 16-byte chunk of one step
// (logical chunk c of its row: step c >> 2), so it walks ITS step's (tap, channel block) and the two halves of a K-tile may lie in different taps
// (Cin = 320: five steps per tap, 45 steps, the tap changes in the middle of every fifth tile).  This keeps the LDS image, the two-step fragment schedule
// and the one barrier per 128 bytes of gemm_fp8_kernel; a 64-byte K-tile would halve the MFMA work per barrier.  When 9 Cin / 64 is odd the last tile's
// second step is dead: its activation chunks gather zeros and its weight chunks re-read the last live step (finite bytes: 0 x finite = 0).
// The scale bytes of a tile's 256 rows x 9 taps are computed once in the prologue (a global load of the source pixel's exponent each) and parked in LDS
// behind the staged epilogue's region: one word per (tap, 32-row block group, row) holding the four row blocks' bytes.  A k-step reads its word with a
// hand-written ds_read_b32 in front of the fragment reads, so nothing inside the MFMA loop touches vmcnt but the DMA.
// Source offsets are 32-bit: activations in bytes relative to the first sample a workgroup touches, weight rows in bytes relative to W (mrag_conv_fp8
// returns MRAG_ENOTSUP past them: the guard of mrag_conv_bf16 restated for bytes).
#include "gemm_fp8_tile.h"

// host-side relaxed launch counter (mrag_conv_fp8_launch_counts): slot 0 the convolution
static unsigned long long g_conv8_launches[1];

namespace {

__device__ __attribute__((aligned(64))) unsigned char g_zero_px[64];   // what a padded tap gathers

struct Conv8P {
  const uint8_t* X; const uint8_t* W; const int* ex; const int* ew;
  const bf16_t* bias; bf16_t* Y; const bf16_t* resid;
  long long M;
  int N, H, Wd, Cin, ctiles, steps, nk;
  int tiles_m, tiles_n, group_m, wide;
};

constexpr int C8_SC_OFF = F8_EPI_LDS;                     // 144 KiB: the scale words sit behind the epilogue's per-wave regions (which overlay the stages)
constexpr int C8_SC_TAPS = 10;                             // nine taps + the dead step's row (scale 1)
constexpr int C8_LDS = C8_SC_OFF + C8_SC_TAPS * 2 * 32 * 4;
static_assert(C8_LDS <= 160 * 1024, "stages, epilogue region and scale words fit the CU's LDS");

template <int EPI>
__global__ __launch_bounds__(512) void conv_fp8_kernel(const Conv8P p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NW = 8, APW = F8_BM / 8 / NW, WPW = F8_BN / 8 / NW;   // 64 pieces of 1 KiB per stage, 8 per wave: the first 4 are activation rows, the others W rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int r32 = lane & 31, hh = lane >> 5;

  long long bm0, bn0;
  fp8_tile_origin(p.tiles_m, p.tiles_n, p.group_m, bm0, bn0);

  const int HW = p.H * p.Wd;
  const long long n0 = bm0 / HW;                                       // the first sample this workgroup touches
  const uint8_t* xbase = p.X + n0 * (long long)HW * p.Cin;            // workgroup-uniform

  // ---- scale words: thread t < 256 owns output row bm0 + t and writes, per tap, the byte 127 - e of the pixel that row reads under the tap
  // (word [(tap, t >> 7, t & 31)], byte (t >> 5) & 3: the row block inside the wave's 128 rows)
  if (tid < F8_BM) {
    unsigned char* sc = (unsigned char*)(smem + C8_SC_OFF) + (((tid >> 7) * 32 + (tid & 31)) << 2) + ((tid >> 5) & 3);
    long long row = bm0 + tid;
    row = row < p.M ? row : p.M - 1;
    const int xo = (int)(row % p.Wd);
    const long long r2 = row / p.Wd;
    const int yo = (int)(r2 % p.H);
    const long long pix0 = (r2 - yo) * p.Wd;                           // first pixel of the row's sample
    int ev[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {                                // nine independent loads (a padded tap re-reads the row's own pixel: unused)
      const int yi = yo + tap / 3 - 1, xi = xo + tap % 3 - 1;
      const bool ok = (unsigned)yi < (unsigned)p.H && (unsigned)xi < (unsigned)p.Wd;
      ev[tap] = p.ex[pix0 + (ok ? (long long)yi * p.Wd + xi : (long long)yo * p.Wd + xo)];
    }
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) sc[tap * 256] = (unsigned char)(127 - ev[tap]);
    sc[9 * 256] = 127;
  }

  // ---- per-lane DMA state.  The lane moves logical chunk `chunk` of its row: bytes 16 sub .. + 15 of step `hs` of the K-tile
  const int chunk = (lane & 7) ^ (lane >> 3);                          // source-side swizzle: row & 7 == lane >> 3
  const int hs = chunk >> 2, sub = chunk & 3;
  int ayx[APW], apix[APW];                                             // per activation piece: (yo << 16 | xo) and the row's own pixel, bytes from xbase (+ 16 sub)
  unsigned woff[WPW];                                                  // per weight piece: the row, bytes from W (+ 16 sub)
#pragma unroll
  for (int i = 0; i < APW; ++i) {
    long long row = bm0 + (wave + i * NW) * 8 + (lane >> 3);
    row = row < p.M ? row : p.M - 1;                                   // clamp: tail rows re-read a valid row, stores are masked
    const int xo = (int)(row % p.Wd);
    const long long r2 = row / p.Wd;
    const int yo = (int)(r2 % p.H);
    const long long n = r2 / p.H;
    ayx[i] = (yo << 16) | xo;
    apix[i] = (int)(((n - n0) * HW + (long long)yo * p.Wd + xo) * p.Cin) + sub * 16;   // (< 2^31: checked by mrag_conv_fp8)
  }
#pragma unroll
  for (int i = 0; i < WPW; ++i) {
    long long row = bn0 + (wave + i * NW) * 8 + (lane >> 3);
    row = row < p.N ? row : p.N - 1;
    woff[i] = (unsigned)(row * 9 * p.Cin) + (unsigned)(sub * 16);      // (< 2^32: checked by mrag_conv_fp8)
  }
  // the lane's step of the next K-tile to request, as (step, tap, channel block): walked, two steps per tile
  const int ct = p.ctiles;
  int ls = hs, ltap = (hs && ct == 1) ? 1 : 0, lcb = (hs && ct != 1) ? 1 : 0;
  auto issue = [&](int stage) {
    char* base = smem + stage * F8_STAGE;
    const bool live = ls < p.steps;
    const unsigned hlim = live ? (unsigned)p.H : 0u;                   // a dead step (odd 9 Cin / 64: the last tile's second half) gathers zeros
    const int ky = ltap / 3, kx = ltap - 3 * ky;
    const int dlt = ((ky - 1) * p.Wd + (kx - 1)) * p.Cin + lcb * 64;   // from the row's own pixel to this step's source
#pragma unroll
    for (int i = 0; i < APW; ++i) {
      const int yi = (ayx[i] >> 16) + ky - 1, xi = (ayx[i] & 0xffff) + kx - 1;
      const bool ok = (unsigned)yi < hlim && (unsigned)xi < (unsigned)p.Wd;
      const unsigned char* src = ok ? xbase + (apix[i] + dlt) : g_zero_px + sub * 16;
      glds16(src, base + (wave + i * NW) * 1024);
    }
    const unsigned wk = (unsigned)(live ? ls : p.steps - 1) * 64u;     // a dead step re-reads the last live one (against zero activation bytes)
#pragma unroll
    for (int i = 0; i < WPW; ++i) glds16(p.W + ((size_t)woff[i] + wk), base + (wave + (APW + i) * NW) * 1024);
    ls += 2; lcb += 2;
    if (lcb >= ct) { lcb -= ct; ++ltap; }
    if (lcb >= ct) { lcb -= ct; ++ltap; }
  };

  int sw[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) sw[j] = fp8_row_scale(p.ew, bn0 + wn * 64 + j * 32 + r32, p.N);
  f32x16 acc[4][2] = {};
  // fragment read addresses: the lane's first activation / W row in stage 0, its scale word under tap 0, and its chunks' offsets inside a row
  const unsigned smem_u = (unsigned)(size_t)smem;
  const unsigned rowA = smem_u + (wm * 128 + r32) * 128, rowW = smem_u + F8_BM * 128 + (wn * 64 + r32) * 128;
  const unsigned scA = smem_u + C8_SC_OFF + ((wm * 32 + r32) << 2);     // + 256 tap: the word of this lane's rows under that tap
  unsigned ca[2][2];                                         // [k-step][half]
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int c = 0; c < 2; ++c) ca[ks][c] = fp8_frag_chunk(ks, hh, c, r32);

  // the tap of the two steps of the K-tile being multiplied (workgroup-uniform walk, as the lanes' above)
  int ut[2] = {0, ct == 1 ? 1 : 0}, uc[2] = {0, ct == 1 ? 0 : 1};

  __syncthreads();                                           // the scale words are in LDS (compiler-made stores: retired in front of the first DMA)
  issue(0);
  for (int kt = 0; kt < p.nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");   // tile kt landed for every wave; every wave finished reading the other stage
    const unsigned so = (unsigned)((kt & 1) * F8_STAGE);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      Fp8Frag f;
      fp8_tile_read<true>(f, rowW + so + ca[ks][0], rowW + so + ca[ks][1], rowA + so + ca[ks][0], rowA + so + ca[ks][1], scA + (unsigned)(ut[ks] << 8));
      if (ks == 0 && kt + 1 < p.nk) issue((kt + 1) & 1);            // the next tile's eight DMA requests go out under the first fragments' LDS latency
      fp8_tile_mfma<true>(acc, f, sw);
      uc[ks] += 2;
      if (uc[ks] >= ct) { uc[ks] -= ct; ++ut[ks]; }
      if (uc[ks] >= ct) { uc[ks] -= ct; ++ut[ks]; }
    }
  }

  // ---- epilogue, LDS-staged (gemm_fp8_tile.h): bias in the accumulator layout, rounded to bf16, the residual added in the row layout (so y may alias
  // resid: a lane reads what it overwrites first)
  char* wbase = smem + wave * (128 * F8_ROWB);
  __syncthreads();   // every wave is done with the operand stages that these per-wave regions overlay (no DMA is in flight: the last tile issued none)
  // (the lane's eight bias quads depend on the column only: loaded once, in one memory latency, not per row block)
  float bv[2][4][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      long long n = bn0 + wn * 64 + j * 32 + 8 * g + 4 * hh;
      n = n < p.N ? n : p.N - 4;   // clamped columns are never stored
      u32x2 bb = u32x2{0u, 0u};
      if (p.bias) bb = *(const u32x2*)(p.bias + n);
      fp8_unpack_bf4(bb, bv[j][g]);
    }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lrow = i * 32 + r32;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int lcol = j * 32 + 8 * g + 4 * hh;
        u32x2 out;
        out[0] = pack_bf2(acc[i][j][4 * g] + bv[j][g][0], acc[i][j][4 * g + 1] + bv[j][g][1]);
        out[1] = pack_bf2(acc[i][j][4 * g + 2] + bv[j][g][2], acc[i][j][4 * g + 3] + bv[j][g][3]);
        *(u32x2*)(wbase + lrow * F8_ROWB + lcol * 2) = out;
      }
    }
  }
  // row layout: lane -> row (lane >> 3) of an 8-row group, 16-byte chunk (lane & 7).  p.wide: the rows of y / resid are 16-byte aligned (Cout % 8 == 0
  // and aligned bases) and move as whole 16-byte lanes; otherwise (Cout % 8 == 4, or an 8-byte aligned base) as two 8-byte halves, the last one of a row
  // possibly alone.  Residual loads are unconditional from a clamped address (all 16 rows in one memory latency for the tail of the workgroup).
  const int rsub = lane >> 3, ch = lane & 7;
  const long long n = bn0 + wn * 64 + ch * 8;
  const bool ok_lo = n + 4 <= p.N, ok_hi = n + 8 <= p.N;
  const long long m0 = bm0 + wm * 128 + rsub;
  u32x4 rpre[16];
  if constexpr (EPI == MRAG_EPI_RESID) {
    if (p.wide) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const long long m = m0 + g * 8;
        rpre[g] = *(const u32x4*)((m < p.M && ok_hi) ? p.resid + m * p.N + n : p.resid);
      }
    } else {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const long long m = m0 + g * 8;
        const u32x2 lo = *(const u32x2*)((m < p.M && ok_lo) ? p.resid + m * p.N + n : p.resid);
        const u32x2 hi = *(const u32x2*)((m < p.M && ok_hi) ? p.resid + m * p.N + n + 4 : p.resid);
        rpre[g] = u32x4{lo[0], lo[1], hi[0], hi[1]};
      }
    }
  }
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const long long m = m0 + g * 8;
    u32x4 val = *(const u32x4*)(wbase + (g * 8 + rsub) * F8_ROWB + ch * 16);
    if constexpr (EPI == MRAG_EPI_RESID) val = fp8_add_bf8(val, rpre[g]);
    if (m < p.M) {
      bf16_t* q = p.Y + m * p.N + n;
      if (p.wide) {
        if (ok_hi) *(u32x4*)q = val;
      } else {
        if (ok_lo) *(u32x2*)q = u32x2{val[0], val[1]};
        if (ok_hi) *(u32x2*)(q + 4) = u32x2{val[2], val[3]};
      }
    }
  }
}

}  // namespace

extern "C" int mrag_conv_fp8_launch_counts(uint64_t* out_host, int32_t n) {
  for (int i = 0; out_host && i < n && i < 1; ++i) out_host[i] = __atomic_load_n(&g_conv8_launches[i], __ATOMIC_RELAXED);
  return 1;
}

extern "C" int mrag_conv_fp8(void* stream, const mrag_conv_fp8_args* a) {
  if (!a || !a->x8 || !a->W8 || !a->x_exp || !a->w_exp || !a->y) return MRAG_EINVAL;
  if (a->N <= 0 || a->H <= 0 || a->Wd <= 0 || a->Cin <= 0 || a->Cout <= 0) return MRAG_EINVAL;
  if (a->epilogue == MRAG_EPI_RESID && !a->resid) return MRAG_EINVAL;
  // 16-byte DMA chunks of both operands; 8-byte row pieces of y / resid (Cout % 4 == 0) and bias reads
  if ((((uintptr_t)a->x8 | (uintptr_t)a->W8) & 15) || (((uintptr_t)a->x_exp | (uintptr_t)a->w_exp) & 3)) return MRAG_EINVAL;
  if (((uintptr_t)a->y & 7) || (a->bias && ((uintptr_t)a->bias & 7))) return MRAG_EINVAL;
  if (a->epilogue == MRAG_EPI_RESID && ((uintptr_t)a->resid & 7)) return MRAG_EINVAL;
  // what stays on mrag_conv_bf16
  if (a->epilogue != MRAG_EPI_NONE && a->epilogue != MRAG_EPI_RESID) return MRAG_ENOTSUP;
  if (a->stride != 1 || a->upsample != 0 || a->asym_pad != 0 || a->t_taps != 0) return MRAG_ENOTSUP;
  if (a->Cin % 64 != 0 || a->Cout % 4 != 0) return MRAG_ENOTSUP;   // one k-step = 64 channels of one tap
  if (a->Cout <= 8) return MRAG_ENOTSUP;   // the convolutions that write a model's output (to 4 or 8 channels) stay bf16: 4 or 8 live columns of a 256-wide tile
  // 32-bit source offsets (the guard of mrag_conv_bf16, in bytes): activations relative to the first sample a workgroup touches -- a 256-row tile
  // spans at most 255 / (H W) + 2 samples -- and weight rows relative to W; (yo, xo) ride in one word; the exponents are indexed by pixel
  const long long HW = (long long)a->H * a->Wd, M = (long long)a->N * HW;
  if (a->H > 32767 || a->Wd > 32767 || M > 0x7fffffffll) return MRAG_ENOTSUP;
  if ((255 / HW + 2) * HW * a->Cin >= (1LL << 31) || (long long)a->Cout * 9 * a->Cin >= (1LL << 32)) return MRAG_ENOTSUP;
  const long long tiles_m = (M + F8_BM - 1) / F8_BM, tiles_n = ((long long)a->Cout + F8_BN - 1) / F8_BN;
  if (tiles_m * tiles_n > 0x7fffffffll) return MRAG_ENOTSUP;
  Conv8P p{};
  p.X = (const uint8_t*)a->x8; p.W = (const uint8_t*)a->W8; p.ex = a->x_exp; p.ew = a->w_exp;
  p.bias = (const bf16_t*)a->bias; p.Y = (bf16_t*)a->y; p.resid = a->epilogue == MRAG_EPI_RESID ? (const bf16_t*)a->resid : nullptr;
  p.M = M; p.N = a->Cout; p.H = a->H; p.Wd = a->Wd; p.Cin = a->Cin;
  p.ctiles = a->Cin / 64; p.steps = 9 * p.ctiles; p.nk = (p.steps + 1) / 2;
  p.tiles_m = (int)tiles_m; p.tiles_n = (int)tiles_n; p.group_m = 4;
  p.wide = a->Cout % 8 == 0 && (((uintptr_t)a->y | (uintptr_t)p.resid) & 15) == 0;   // 16-byte aligned rows of y / resid
  const dim3 grid((unsigned)(tiles_m * tiles_n)), block(512);
  hipStream_t s = (hipStream_t)stream;
  const int rc = a->epilogue == MRAG_EPI_RESID ? launch_dyn_lds(conv_fp8_kernel<MRAG_EPI_RESID>, grid, block, C8_LDS, s, p)
                                               : launch_dyn_lds(conv_fp8_kernel<MRAG_EPI_NONE>, grid, block, C8_LDS, s, p);
  if (rc != MRAG_OK) return rc;
  (void)__atomic_fetch_add(&g_conv8_launches[0], 1ull, __ATOMIC_RELAXED);
  return MRAG_OK;
}
