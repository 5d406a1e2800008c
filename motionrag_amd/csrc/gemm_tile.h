// gemm_tile.h -- C[M,N] = epilogue(A[M,K] . W[N,K]^T + bias), bf16 in, fp32 accumulate.
//
// Stands behind every nn.Linear on the MotionRAG hot path (see include/mrag_hip.h).
// CDNA4 design (not a port of anything):
//   * v_mfma_f32_16x16x32_bf16, 64-lane wavefronts, wave tile (TM*16) x (TN*16);
//   * both operands are K-contiguous (activations [M,K], nn.Linear weight [N,K]), so A and W
//     tiles use the same LDS image: [rows][64 k] bf16 = 128-byte rows, filled by 16-byte
//     global_load_lds (LDS-DMA, no VGPR round trip), XOR-swizzled on the SOURCE address
//     (chunk ^= row & 7) and un-swizzled on the ds_read_b128 -> conflict-free fragment reads;
//   * two LDS stages; the DMA for K-tile t+1 is issued before the MFMAs of tile t and is
//     retired by the one vmcnt(0)+barrier per K-tile;
//   * operands swapped in the MFMA (W fragment as A-operand) so each lane owns 4 consecutive
//     output columns of one row -> 8-byte bf16 stores and a lane-local fused epilogue;
//   * 1-D grid with a bijective XCD remap so tiles that share an A row-panel sit on one L2.
// The tiled kernel and its launcher template.  Included by the two units that instantiate it: gemm_tiled.hip (linears) and gemm_conv.hip (convolutions).
#pragma once
#include "gemm_common.h"

namespace {

// zero source for the taps that fall outside the image / clip (never written)
__device__ __attribute__((aligned(128))) bf16_t g_zero_row[64];

// ---- direct epilogue (accumulator layout): lane owns row m = .. + (lane & 15), columns n0 + (lane >> 4) * 4 + {0..3} of every 16x16 tile; 8-byte stores.
// Same rounding points as the LDS-staged epilogue (so a GEMM gives the same bits whichever tile configuration its size selects).
template <int TM, int TN, int EPI>
__device__ __forceinline__ void epilogue_direct(const GemmP& p, f32x4 (&acc)[TM][TN], const long long bm0, const long long bn0, const int wrow0, const int wcol0, const int lane) {
  const int frag_row = lane & 15, frag_q = lane >> 4;
  long long wg_b = 0, wg_pos = 0;
  if constexpr (EPI == MRAG_EPI_GATE_RESID) {
    wg_b = bm0 / p.rows_per_batch;
    wg_pos = bm0 - wg_b * p.rows_per_batch;
  }
  auto row_bp = [&](long long m, long long& b, long long& pos) {
    b = wg_b; pos = wg_pos + (m - bm0);
    while (pos >= p.rows_per_batch) { pos -= p.rows_per_batch; ++b; }
  };
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const long long m = bm0 + wrow0 + i * 16 + frag_row;
    if (m >= p.M) continue;
    const bf16_t* gate = nullptr;
    if constexpr (EPI == MRAG_EPI_GATE_RESID) {
      long long b, pos;
      row_bp(m, b, pos);
      gate = (pos < p.split ? p.gate0 : p.gate1) + b * p.gate_stride;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const long long n = bn0 + wcol0 + j * 16 + frag_q * 4;
      if (n >= p.N) continue;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
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
      if constexpr (EPI == MRAG_EPI_RESID) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= p.acc_scale;
      }
      if constexpr (EPI == MRAG_EPI_GATE_RESID || EPI == MRAG_EPI_RESID) {
        // the same rounding points as the LDS-staged epilogue above and as the reference's bf16 tensors (`x + gate * linear(.)`: the gated
        // projection is a bf16 tensor before the residual add) -- so a GEMM gives the same bits whichever tile configuration its size selects
        // (a sequence-sharded rank runs smaller problems than the unsharded model)
        const u32x2 rr = *(const u32x2*)(p.resid + m * p.ldr + n);
        v[0] = bf_round(v[0]) + __uint_as_float(rr[0] << 16); v[1] = bf_round(v[1]) + __uint_as_float(rr[0] & 0xffff0000u);
        v[2] = bf_round(v[2]) + __uint_as_float(rr[1] << 16); v[3] = bf_round(v[3]) + __uint_as_float(rr[1] & 0xffff0000u);
      }
      u32x2 out;
      out[0] = pack_bf2(v[0], v[1]);
      out[1] = pack_bf2(v[2], v[3]);
      *(u32x2*)(p.C + m * p.ldc + n) = out;
    }
  }
}

// One output tile (SK: one run of K-tiles [kt0, kt0 + nk) of it).  `wg` = the tile's index in the logical order.
template <int WM, int WN, int TM, int TN, int EPI, int CONV, bool SK>
__device__ __forceinline__ void gemm_tile(const GemmP& p, const int wg, const int kt0, const int nk, const int sk_tile, const int sk_unit) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NW = WM * WN;
  constexpr int BM = WM * TM * 16, BN = WN * TN * 16, BK = 64;
  constexpr int STAGE_BYTES = (BM + BN) * BK * 2;
  constexpr int PIECES = (BM + BN) / 8;   // 1 KiB LDS-DMA pieces per stage (8 rows x 128 B)
  constexpr int PPW = PIECES / NW;        // pieces per wave
  static_assert(PIECES % NW == 0, "piece split");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;

  // logical tile order: groups of GROUP_M m-tiles walked n-major, so the ~32 workgroups resident on one XCD (a contiguous
  // run of the logical order after the XCD remap) form a GROUP_M x 8 block that shares GROUP_M A-panels and 8 W-panels
  // per K-step through that XCD's L2 (instead of 1 A-panel and 32 W-panels)
  const int gw = p.group_m * p.tiles_n;
  const int first_m = (wg / gw) * p.group_m;
  const int gsz = min(p.tiles_m - first_m, p.group_m);
  const int tile_m = first_m + (wg % gw) % gsz, tile_n = (wg % gw) / gsz;
  const long long bm0 = (long long)tile_m * BM, bn0 = (long long)tile_n * BN;

  // ---- per-lane DMA sources (k = 0), one per piece this wave stages.
  // Plain GEMM, and the convolutions on every tile but 256x256: a 64-bit row pointer per piece (+ per A piece of a convolution the tap-independent position and
  // the walked tap cursor: cv_y, cv_x, cv_src, cv_step).  The 8-wave 256x256 tile runs at exactly 256 VGPRs (128 accumulators, two sets of 48 fragment
  // registers): there those 36 registers were 44-51 SPILLED VGPRs -- two scratch reloads per K-tile, each behind an `s_waitcnt vmcnt(0)` that also drains the
  // LDS-DMA ring (round-5 review; tools/check_scratch.py).  SLIM form (256x256 convolutions only; the other tiles have the registers and measured 1 % slower on
  // it: profiles/r6_conv_scratch_ab.txt): per A piece the current tap's source as ONE 32-bit offset in 16-byte units relative to a workgroup-uniform base
  // (`cv_base`, an SGPR pair), per W piece a 32-bit byte offset for the scalar-base form of the DMA: 8 registers.  What a tap change needs to recompute the
  // offsets -- the tap-independent position (y << 16 | x, or the frame index) and the sample's offset, two words per piece -- is parked in LDS (lane-linear
  // words behind the operand stages, GemmP::cv_lds): read back once per tap by ds_read, which counts on lgkmcnt and leaves the DMA ring alone.
  constexpr int APW = BM / 8 / NW;          // a wave's first APW pieces are A rows (piece = wave + i * NW < BM / 8)
  static_assert((BM / 8) % NW == 0, "A pieces split evenly over the waves");
  constexpr bool SLIM = CONV != 0 && TM == 8 && TN == 4 && WM == 2 && WN == 4;
  static_assert(!SLIM || APW <= 4, "the parked conv state is read back by four hand-written statements");
  constexpr int CV_NONE = (int)0x80000000;  // cv_cur: the tap falls outside the image / clip -> the zero row
  const bf16_t* gsrc[SLIM ? 1 : PPW];
  int cv_y[(CONV != 0 && !SLIM) ? APW : 1], cv_x[(CONV != 0 && !SLIM) ? APW : 1];      // legacy conv form: per A piece
  int cv_cur[SLIM ? APW : 1];
  const unsigned cv_park = (unsigned)(size_t)smem + (unsigned)p.cv_lds + (unsigned)tid * 4u;   // word k of this lane at + k * NW * 256: k = 2 i (position), 2 i + 1 (sample offset)
  auto cv_put = [&](int k, int v) { *(int*)(smem + p.cv_lds + (k * NW * 64 + tid) * 4) = v; };
  unsigned cv_woff[SLIM ? PPW - APW : 1];
  const bf16_t* cv_base = p.A;              // workgroup-uniform
  const int cv_c8 = (int)(p.cv_C >> 3);     // 16-byte units per pixel
  if constexpr (SLIM && CONV == 1) {        // the sample (input frame stack position) of the tile's first row
    const long long n0 = bm0 / ((long long)p.cv_Wo * p.cv_Ho);
    const long long n0_in = p.cv_tf ? n0 + 2 * (n0 / p.cv_tf) : n0;
    cv_base = p.A + n0_in * p.cv_H * p.cv_W * p.cv_C;
  } else if constexpr (SLIM && CONV == 2) {
    cv_base = p.A + bm0 * p.cv_C;
  }
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int piece = wave + i * NW;  // pieces [0, BM/8) are A rows, the rest W rows
    const int r = piece * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ (lane >> 3);  // source-side swizzle: row&7 == lane>>3
    if (piece < BM / 8) {
      long long row = bm0 + r;
      row = row < p.M ? row : p.M - 1;  // clamp: tail rows re-read a valid row, stores are masked
      if constexpr (CONV == 1) {         // row = (n, yo, xo) of the output image: keep (yo*stride - pad, xo*stride - pad) and the sample's position
        const int xo = (int)(row % p.cv_Wo);
        const long long r2 = row / p.cv_Wo;
        const int yo = (int)(r2 % p.cv_Ho);
        const long long n = r2 / p.cv_Ho;
        const long long n_in = p.cv_tf ? n + 2 * (n / p.cv_tf) : n;   // 3-D: sample s's output frame t reads input frames s (T + 2) + t + {0, 1, 2}
        if constexpr (SLIM) {
          const long long n0 = bm0 / ((long long)p.cv_Wo * p.cv_Ho);
          const long long n0_in = p.cv_tf ? n0 + 2 * (n0 / p.cv_tf) : n0;
          cv_put(2 * i, (int)(((unsigned)(yo * p.cv_stride - p.cv_pad) << 16) | ((unsigned)(xo * p.cv_stride - p.cv_pad) & 0xffffu)));
          cv_put(2 * i + 1, (int)(n_in - n0_in) * (p.cv_H * p.cv_W * cv_c8) + chunk);
        } else {
          gsrc[i] = p.A + n_in * p.cv_H * p.cv_W * p.cv_C + chunk * 8;
          cv_y[i < APW ? i : 0] = yo * p.cv_stride - p.cv_pad;
          cv_x[i < APW ? i : 0] = xo * p.cv_stride - p.cv_pad;
        }
      } else if constexpr (CONV == 2) {  // row = (b, t, hw): keep the row's position and t
        if constexpr (SLIM) {
          cv_put(2 * i, (int)((row / p.cv_HW) % p.cv_T));
          cv_put(2 * i + 1, (int)(row - bm0) * cv_c8 + chunk);
        } else {
          gsrc[i] = p.A + row * p.cv_C + chunk * 8;
          cv_y[i < APW ? i : 0] = (int)((row / p.cv_HW) % p.cv_T);
        }
      } else {
        gsrc[i] = p.A + row * p.lda + chunk * 8 + (SK ? (long long)kt0 * BK : 0);
      }
    } else {
      long long row = bn0 + (r - BM);
      row = row < p.N ? row : p.N - 1;
      if constexpr (SLIM) cv_woff[i >= APW ? i - APW : 0] = (unsigned)((row * p.ldw + chunk * 8) * 2);   // (< 4 GiB: checked by mrag_conv_bf16)
      else gsrc[i] = p.W + row * p.ldw + chunk * 8 + (SK ? (long long)kt0 * BK : 0);
    }
  }

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment read offsets (bytes) inside a stage: rows of A start at 0, rows of W at BM*128
  const int frag_row = lane & 15, frag_q = lane >> 4, swz = lane & 7;
  const int a_off = (wm * TM * 16 + frag_row) * 128;
  const int w_off = BM * 128 + (wn * TN * 16 + frag_row) * 128;

  // DMA source of piece i for K-tile kt.  Plain GEMM: the row pointer advanced by kt * 64.  Convolutions: K-tile kt is channel
  // block (kt % ctiles) of tap (kt / ctiles); the lane's row is the tap-shifted pixel (or frame), or the zero row outside.
  // The K-tiles are requested in order (0, 1, 2, ...), so the (tap, channel block) pair is WALKED: the tap geometry (bounds test, pixel
  // offset) is redone only when the tap changes -- every Cin / 64 K-tiles -- and leaves one 32-bit offset per piece (cv_cur); a K-tile's
  // request adds the channel block and the workgroup's base to it (a handful of vector instructions per piece, no persistent pointer).
  const bf16_t* cv_src[(CONV != 0 && !SLIM) ? APW : 1];   // legacy form, per A piece: this lane's source at the current (tap, channel block)
  int cv_step[(CONV != 0 && !SLIM) ? APW : 1];            // 64 elements per channel block inside the image, 0 on the zero row
  int cv_kt = -1, cv_tap = 0, cv_cblk = -1;
  auto cv_prepare = [&](int kt) {
    if constexpr (CONV != 0) {
      if (kt == cv_kt) return;
      cv_kt = kt;
      bool new_tap = kt == 0;
      if (++cv_cblk == p.cv_ctiles) { cv_cblk = 0; ++cv_tap; new_tap = true; }
      if (new_tap) {
#pragma unroll
        for (int i = 0; i < APW; ++i) {
          bool ok;
          if constexpr (SLIM) {
            int off, yx, nb;
            // (hand-written reads: a compiler-made LDS load would be ordered behind the LDS-DMA pieces in flight -- `s_waitcnt vmcnt(0)`, the drain this form removes)
            if (i == 0) asm volatile("ds_read_b32 %0, %2\n\tds_read_b32 %1, %2 offset:%3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(yx), "=&v"(nb) : "v"(cv_park), "n"(NW * 256) : "memory");
            else if (i == 1) asm volatile("ds_read_b32 %0, %2 offset:%3\n\tds_read_b32 %1, %2 offset:%4\n\ts_waitcnt lgkmcnt(0)" : "=&v"(yx), "=&v"(nb) : "v"(cv_park), "n"(2 * NW * 256), "n"(3 * NW * 256) : "memory");
            else if (i == 2) asm volatile("ds_read_b32 %0, %2 offset:%3\n\tds_read_b32 %1, %2 offset:%4\n\ts_waitcnt lgkmcnt(0)" : "=&v"(yx), "=&v"(nb) : "v"(cv_park), "n"(4 * NW * 256), "n"(5 * NW * 256) : "memory");
            else asm volatile("ds_read_b32 %0, %2 offset:%3\n\tds_read_b32 %1, %2 offset:%4\n\ts_waitcnt lgkmcnt(0)" : "=&v"(yx), "=&v"(nb) : "v"(cv_park), "n"(6 * NW * 256), "n"(7 * NW * 256) : "memory");
            if constexpr (CONV == 1) {
              const int kt3 = p.cv_tf ? cv_tap / 9 : 0, tap9 = cv_tap - 9 * kt3;   // taps in (kt, ky, kx) order; kt3 = 0 for the 2-D convolution
              const int ky = tap9 / 3, kx = tap9 - 3 * ky;
              const int yi = (yx >> 16) + ky, xi = (int)(short)(yx & 0xffff) + kx;
              ok = (unsigned)yi < (unsigned)p.cv_Hi && (unsigned)xi < (unsigned)p.cv_Wi;
              off = nb + ((yi >> p.cv_up) * p.cv_W + (xi >> p.cv_up)) * cv_c8 + kt3 * (int)(p.cv_fs >> 3);
            } else {
              const int t = yx + cv_tap - 1;
              ok = (unsigned)t < (unsigned)p.cv_T;
              off = nb + (cv_tap - 1) * (int)p.cv_HW * cv_c8;
            }
            cv_cur[i] = ok ? off : CV_NONE;
          } else {
            long long off;
            if constexpr (CONV == 1) {
              const int kt3 = p.cv_tf ? cv_tap / 9 : 0, tap9 = cv_tap - 9 * kt3;
              const int ky = tap9 / 3, kx = tap9 - 3 * ky;
              const int yi = cv_y[i] + ky, xi = cv_x[i] + kx;
              ok = (unsigned)yi < (unsigned)p.cv_Hi && (unsigned)xi < (unsigned)p.cv_Wi;
              off = ((long long)(yi >> p.cv_up) * p.cv_W + (xi >> p.cv_up)) * p.cv_C + kt3 * p.cv_fs;
            } else {
              const int t = cv_y[i] + cv_tap - 1;
              ok = (unsigned)t < (unsigned)p.cv_T;
              off = (long long)(cv_tap - 1) * p.cv_HW * p.cv_C;
            }
            cv_src[i] = ok ? gsrc[i] + off : g_zero_row + (lane & 7) * 8;
            cv_step[i] = ok ? 64 : 0;
          }
        }
      } else if constexpr (!SLIM) {
#pragma unroll
        for (int i = 0; i < APW; ++i) cv_src[i] += cv_step[i];
      }
    }
  };
  // request piece i of K-tile kt into `dst` (the piece's 1-KiB slot of a stage).  Convolutions: cv_prepare(kt) ran for this K-tile.
  auto dma_piece = [&](int i, int kt, char* dst) {
    if constexpr (CONV == 0) {
      glds16(gsrc[i] + (long long)kt * BK, dst);
    } else if constexpr (!SLIM) {
      glds16(i >= APW ? gsrc[i] + (long long)kt * BK : cv_src[i < APW ? i : 0], dst);      // weight rows [Cout, taps * Cin] are plain
    } else {
      if (i >= APW) {                                          // weight rows: scalar base + the lane's byte offset
        glds16_sbase(p.W + (long long)kt * BK, cv_woff[i - APW], (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)dst));   // (wave-uniform by construction; the asm wants it in an SGPR)
      } else {
        const int c = cv_cur[i];
        const bf16_t* in_img = cv_base + ((long long)(c + cv_cblk * 8) << 3);
        glds16(c == CV_NONE ? g_zero_row + (lane & 7) * 8 : in_img, dst);
      }
    }
  };
  auto issue = [&](int stage, int kt) {
    char* base = smem + stage * STAGE_BYTES;
    cv_prepare(kt);
#pragma unroll
    for (int i = 0; i < PPW; ++i) dma_piece(i, kt, base + (wave + i * NW) * 1024);  // wave-uniform base (+ lane*16 by HW)
  };

  issue(0, 0);
  if constexpr (TM == 8 && TN == 4 && WM == 2 && WN == 4) {
    // ---- 256x256 tile: all 12 fragments of a 32-deep k-step are requested by ONE asm statement and released to the MFMAs by
    // COUNTED s_waitcnt lgkmcnt(N) (LDS reads return in order), the second k-step's 12 reads are issued while the first
    // k-step's MFMAs run -> the LDS latency is paid once per K-tile instead of eight times (hipcc's own schedule: read
    // pair -> lgkmcnt(0) -> 8 MFMAs).  At most 15 LDS reads are outstanding (lgkmcnt is a 4-bit counter).
    //
    // Software pipeline across the per-tile barrier: the fragments of k-step (t, 0) are already in registers when tile t's MFMAs
    // start, the reads of (t, 1) fly under the 32 MFMAs of (t, 0), and the ONE barrier per K-tile sits between the two k-steps:
    // behind it every wave has finished reading stage t (so the DMA of tile t+2 may overwrite it) and tile t+1 has landed (so
    // the reads of (t+1, 0) are issued right there, under the MFMAs of (t, 1)).  No fragment latency is exposed at the tile
    // boundary (measured before: ~350 cycles of first-fragment wait + ~500 of barrier per 2048-cycle MFMA body).
#define MRAG_READ12(W, A, AW, AA)                                                                                   \
      asm volatile(                                                                                                  \
          "ds_read_b128 %0, %12 offset:32768\n\tds_read_b128 %1, %12 offset:34816\n\t"                               \
          "ds_read_b128 %2, %12 offset:36864\n\tds_read_b128 %3, %12 offset:38912\n\t"                               \
          "ds_read_b128 %4, %13\n\tds_read_b128 %5, %13 offset:2048\n\t"                                             \
          "ds_read_b128 %6, %13 offset:4096\n\tds_read_b128 %7, %13 offset:6144\n\t"                                 \
          "ds_read_b128 %8, %13 offset:8192\n\tds_read_b128 %9, %13 offset:10240\n\t"                                \
          "ds_read_b128 %10, %13 offset:12288\n\tds_read_b128 %11, %13 offset:14336"                                  \
          : "=&v"(W[0]), "=&v"(W[1]), "=&v"(W[2]), "=&v"(W[3]), "=&v"(A[0]), "=&v"(A[1]), "=&v"(A[2]), "=&v"(A[3]),    \
            "=&v"(A[4]), "=&v"(A[5]), "=&v"(A[6]), "=&v"(A[7])                                                       \
          : "v"(AW), "v"(AA)                                                                                         \
          : "memory")
#define MRAG_WAIT12(N, W, A)                                                                                         \
      asm volatile("s_waitcnt lgkmcnt(" #N ")"                                                                        \
                   : "+v"(W[0]), "+v"(W[1]), "+v"(W[2]), "+v"(W[3]), "+v"(A[0]), "+v"(A[1]), "+v"(A[2]), "+v"(A[3]),   \
                     "+v"(A[4]), "+v"(A[5]), "+v"(A[6]), "+v"(A[7])                                                  \
                   :: "memory")
#define MRAG_ROW(I, W, X)                                                                                                       \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) acc[I][j] =                                                                 \
          __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, W[j]), __builtin_bit_cast(bf16x8, X), acc[I][j], 0, 0, 0)
    const unsigned smem_u = (unsigned)(size_t)smem;
    const unsigned c0 = ((frag_q + 0) ^ swz) * 16, c1 = ((frag_q + 4) ^ swz) * 16;
    const unsigned offA = a_off, offW = w_off - BM * 128;   // the W reads carry offset:32768 (= BM * 128) in the instruction
    u32x4 w0[4], a0[8], w1[4], a1[8];
    if (nk > 1) {
      issue(1, 1);
      asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" :: "n"(PPW) : "memory");   // tile 0 landed everywhere, tile 1 in flight
    } else {
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }
    MRAG_READ12(w0, a0, smem_u + offW + c0, smem_u + offA + c0);
    for (int kt = 0; kt < nk; ++kt) {
      const unsigned st = smem_u + (kt & 1) * STAGE_BYTES;
      MRAG_WAIT12(0, w0, a0);            // the (t, 0) fragments (requested one k-step ago) are here
      MRAG_ROW(0, w0, a0[0]);
      MRAG_READ12(w1, a1, st + offW + c1, st + offA + c1);   // behind the first MFMAs: the 12 KB read burst of 8 waves takes up to ~380 cycles to issue
      MRAG_ROW(1, w0, a0[1]); MRAG_ROW(2, w0, a0[2]); MRAG_ROW(3, w0, a0[3]);
      MRAG_ROW(4, w0, a0[4]); MRAG_ROW(5, w0, a0[5]); MRAG_ROW(6, w0, a0[6]); MRAG_ROW(7, w0, a0[7]);
      __builtin_amdgcn_sched_barrier(0);
      MRAG_WAIT12(0, w1, a1);            // this wave is done reading stage t
      const bool more = kt + 1 < nk, more2 = kt + 2 < nk;
      if (more) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");   // tile t+1 landed for every wave; stage t is free
      // the 8 LDS-DMA pieces of tile t+2 go into stage t, ONE PER ROW GROUP between the MFMAs (a burst of 8 costs ~100 cycles
      // each at issue, measured with s_memtime stamps)
      char* nbase = smem + (kt & 1) * STAGE_BYTES;
#define MRAG_PIECE(I) if (more2) dma_piece(I, kt + 2, nbase + (wave + (I) * NW) * 1024)
      MRAG_ROW(0, w1, a1[0]);
      if (more) {
        const unsigned sn = smem_u + ((kt + 1) & 1) * STAGE_BYTES;
        MRAG_READ12(w0, a0, sn + offW + c0, sn + offA + c0);
      }
      if (more2) cv_prepare(kt + 2);
      MRAG_PIECE(0);
      MRAG_ROW(1, w1, a1[1]); MRAG_PIECE(1);
      MRAG_ROW(2, w1, a1[2]); MRAG_PIECE(2);
      MRAG_ROW(3, w1, a1[3]); MRAG_PIECE(3);
      MRAG_ROW(4, w1, a1[4]); MRAG_PIECE(4);
      MRAG_ROW(5, w1, a1[5]); MRAG_PIECE(5);
      MRAG_ROW(6, w1, a1[6]); MRAG_PIECE(6);
      MRAG_ROW(7, w1, a1[7]); MRAG_PIECE(7);
      __builtin_amdgcn_sched_barrier(0);
#undef MRAG_PIECE
    }
#undef MRAG_READ12
#undef MRAG_WAIT12
#undef MRAG_ROW
  } else {
    for (int kt = 0; kt < nk; ++kt) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();  // tile kt landed for every wave; everyone finished reading the other stage
      if (kt + 1 < nk) issue((kt + 1) & 1, kt + 1);
      const char* st = smem + (kt & 1) * STAGE_BYTES;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int coff = ((frag_q + 4 * ks) ^ swz) * 16;
        bf16x8 wf[TN], af[TM];
#pragma unroll
        for (int j = 0; j < TN; ++j) wf[j] = *(const bf16x8*)(st + w_off + j * 16 * 128 + coff);
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = *(const bf16x8*)(st + a_off + i * 16 * 128 + coff);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
      }
    }
  }

  if constexpr (SK) {
    if (nk != (int)(p.K / BK)) {   // a partial run of this tile's K-tiles (workgroup-uniform)
      // Contributors of tail tile T are the units whose iteration range [b(u), b(u + 1)), b(u) = u I / U, meets [T nk_full, (T + 1) nk_full): consecutive
      // units, numbered in K order.  Every contributor parks its fp32 accumulators in its own slot and takes a ticket; the LAST arriver sums the
      // slots in K order -- a fixed order, so the result does not depend on who arrives last (bit-reproducible run to run) -- and runs the epilogue.
      const int nkf = (int)(p.K / BK), I = p.sk_rem * nkf, U = p.sk_units;
      auto owner = [&](int it) {   // the unit whose range holds iteration `it`
        int u = (int)(((long long)it * U) / I);
        while ((int)(((long long)(u + 1) * I) / U) <= it) ++u;
        while ((int)(((long long)u * I) / U) > it) --u;
        return u;
      };
      const int u_first = owner(sk_tile * nkf), u_last = owner(sk_tile * nkf + nkf - 1);
      const int part = sk_unit - u_first, nparts = u_last - u_first + 1;
      float* slot0 = p.sk_part + (size_t)sk_tile * p.sk_maxparts * (BM * BN);
      float* mine = slot0 + (size_t)part * (BM * BN) + ((size_t)wave * (TM * TN) * 64 + lane) * 4;   // lane-linear: every store / load instruction moves 1 KiB
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) *(f32x4*)(mine + (size_t)(i * TN + j) * 256) = acc[i][j];
      unsigned* flag = (unsigned*)(smem + SK_FLAG_OFF);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();                                   // every wave's slot stores have left
      if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the write-back must not be overtaken by the ticket (guide, compiler hazard of the release)
        const unsigned old = __hip_atomic_fetch_add(p.sk_ticket + sk_tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = old == (unsigned)(nparts - 1);
        if (last) {
          __hip_atomic_store(p.sk_ticket + sk_tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");                                            // this CU's L1 forgets the other contributors' lines
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag = last ? 1u : 0u;
      }
      __syncthreads();
      if (*flag == 0u) return;
      const float* src0 = slot0 + ((size_t)wave * (TM * TN) * 64 + lane) * 4;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = *(const f32x4*)(src0 + (size_t)(i * TN + j) * 256);
      for (int q = 1; q < nparts; ++q) {
        const float* sq = src0 + (size_t)q * (BM * BN);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] += *(const f32x4*)(sq + (size_t)(i * TN + j) * 256);
      }
    }
  }

  // (batch, position-in-batch) of a row without a 64-bit division per row (~100 vector instructions each): ONE division per workgroup for
  // its first row, then rows advance by < 256 -- a short subtract loop (rows_per_batch is 17 776 on the DiT; tiny values still terminate)
  long long wg_b = 0, wg_pos = 0;
  if constexpr (EPI == MRAG_EPI_GATE_RESID || EPI == MRAG_EPI_QKNORM_ROPE) {
    wg_b = bm0 / p.rows_per_batch;
    wg_pos = bm0 - wg_b * p.rows_per_batch;
  }
  auto row_bp = [&](long long m, long long& b, long long& pos) {
    b = wg_b; pos = wg_pos + (m - bm0);
    while (pos >= p.rows_per_batch) { pos -= p.rows_per_batch; ++b; }
  };
  // ---- epilogue: lane owns row m = .. + (lane & 15), columns n0 + (lane >> 4) * 4 + {0..3}
  constexpr bool STAGED = (TM == 8 && TN == 4 && WM == 2 && WN == 4);
  if (STAGED && p.staged && !is_geglu<EPI>) {   // GEGLU has its own staged form below ([M, N/2] output)
    // The accumulator layout gives 8-byte pieces of 16 different rows per store instruction (32-byte row segments): the store
    // tail was ~24 % of a K = 3072 workgroup.  Stage the wave's 128 x 64 bf16 tile through LDS (row pitch 144 B) and write
    // whole 128-byte row segments with 16-byte lanes; bias / activation / gate are applied in the accumulator layout, the
    // residual add in the row layout (same rounding points as the reference's bf16 tensors: gate * out, then + residual).
    constexpr int ROWB = 144;
    char* wbase = smem + wave * (128 * ROWB);
    // QKNORM_ROPE: the wave's 64 columns are one head (256-wide tiles, 64-column wave tiles); in the row layout below 8 lanes x 8 features
    // hold a row: per-head LayerNorm across those 8 lanes, RoPE on the lane's 4 (even, odd) pairs, Q pre-multiplied -- the arithmetic of
    // qknorm_rope_kernel (norm.hip).  The fp32 cos / sin rows cost 64 B per lane and row group (1 KB per lane over the tile); issued
    // inside the per-row `is a video row` branch they serialised 16 global-load latencies per workgroup.  They are fetched UNCONDITIONALLY
    // instead (text rows read table row 0 and discard it) through a ring of QK_RING row groups of registers, each slot refilled as it is
    // consumed.  MI355X, M = 35 552, N = 9216, K = 3072 (interleaved A/B): 1.99-2.01 ms before, 1.925 ms with a ring of 3 or 4; rings of
    // 5+ make hipcc spill the table registers and lose the gain again.  The ring is filled after the accumulators are staged: requesting
    // the first row groups before that measured equal (1.925 vs 1.927 ms).
    constexpr int QK_RING = 4;   // row groups in flight, 16 registers each
    f32x4 qk_tab[EPI == MRAG_EPI_QKNORM_ROPE ? QK_RING : 1][4];
    unsigned qk_video = 0;              // bit g: row group g's row lies past the text rows (RoPE applies)
    int qk_which = 2;                   // 0 = Q, 1 = K, 2 = V columns (wave-uniform)
    bool has_rope = false;
    const int rsub = lane >> 3, chunk = lane & 7;   // row layout: lane -> row (lane >> 3) of an 8-row group, 16-byte chunk (lane & 7)
    auto qk_fetch = [&](int g) {
      if constexpr (EPI == MRAG_EPI_QKNORM_ROPE) {
        const long long m = bm0 + wm * TM * 16 + g * 8 + rsub;
        long long rb, rpos;
        row_bp(m < p.M ? m : p.M - 1, rb, rpos);
        const int pos = (int)rpos - p.rope_text_len;
        if (pos >= 0) qk_video |= 1u << g;
        const long long ro = (long long)(pos > 0 ? pos : 0) * 64 + chunk * 8;
        f32x4(&dst)[4] = qk_tab[g % QK_RING];
        dst[0] = *(const f32x4*)(p.rcos + ro); dst[1] = *(const f32x4*)(p.rcos + ro + 4);
        dst[2] = *(const f32x4*)(p.rsin + ro); dst[3] = *(const f32x4*)(p.rsin + ro + 4);
      }
    };
    if constexpr (EPI == MRAG_EPI_QKNORM_ROPE) {
      qk_which = p.qk_first + (int)((bn0 + wn * TN * 16) / p.qk_D);
      has_rope = p.rcos != nullptr && qk_which < 2;
    }
    __syncthreads();   // every wave is done with the operand stages that these per-wave regions overlay
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const long long m = bm0 + wm * TM * 16 + i * 16 + frag_row;
      const bf16_t* gate = nullptr;
      if constexpr (EPI == MRAG_EPI_GATE_RESID) {
        const long long mc = m < p.M ? m : p.M - 1;
        long long b, pos;
        row_bp(mc, b, pos);
        gate = (pos < p.split ? p.gate0 : p.gate1) + b * p.gate_stride;
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        long long n = bn0 + wn * TN * 16 + j * 16 + frag_q * 4;
        n = n < p.N ? n : p.N - 4;   // clamped columns are never stored
        float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
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
        if constexpr (EPI == MRAG_EPI_RESID) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] *= p.acc_scale;
        }
        u32x2 out;
        out[0] = pack_bf2(v[0], v[1]);
        out[1] = pack_bf2(v[2], v[3]);
        *(u32x2*)(wbase + (i * 16 + frag_row) * ROWB + (j * 16 + frag_q * 4) * 2) = out;
      }
    }
    // row layout: one instruction = 8 x 128 contiguous bytes
    const long long n = bn0 + wn * TN * 16 + chunk * 8;
    // residual epilogues: all 16 residual vectors of the lane are requested up front (the accumulator registers are free once the tile sits
    // in LDS), so the tail of a workgroup pays ONE memory latency instead of four batches of four
    u32x4 rpre[16];
    if constexpr (EPI == MRAG_EPI_GATE_RESID || EPI == MRAG_EPI_RESID) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const long long m = bm0 + wm * TM * 16 + g * 8 + rsub;
        rpre[g] = (m < p.M && n + 8 <= p.N) ? *(const u32x4*)(p.resid + m * p.ldr + n) : u32x4{0u, 0u, 0u, 0u};
      }
    }
    bool qk_done = false;
    if constexpr (EPI == MRAG_EPI_QKNORM_ROPE) {
      if (qk_which < 2) {
        qk_done = true;
        const bf16_t* gm = qk_which ? p.kg : p.qg;
        const bf16_t* bt = qk_which ? p.kb : p.qb;
        const int d0 = chunk * 8;
        float gam[8], bet[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { gam[e] = 1.f; bet[e] = 0.f; }
        if (gm) {
          const u32x4 graw = *(const u32x4*)(gm + d0);
#pragma unroll
          for (int e = 0; e < 4; ++e) { gam[2 * e] = __uint_as_float(graw[e] << 16); gam[2 * e + 1] = __uint_as_float(graw[e] & 0xffff0000u); }
          if (bt) {
            const u32x4 braw = *(const u32x4*)(bt + d0);
#pragma unroll
            for (int e = 0; e < 4; ++e) { bet[2 * e] = __uint_as_float(braw[e] << 16); bet[2 * e + 1] = __uint_as_float(braw[e] & 0xffff0000u); }
          }
        }
        if (has_rope) {
#pragma unroll
          for (int g = 0; g < QK_RING; ++g) qk_fetch(g);
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          __builtin_amdgcn_sched_barrier(0);   // one row group at a time: hoisting all 16 LDS reads / address computations spills the ring
          const int row = g * 8 + rsub;
          const long long m = bm0 + wm * TM * 16 + row;
          u32x4 val = *(const u32x4*)(wbase + row * ROWB + chunk * 16);
          val = qk_row_math(val, gm != nullptr, bt != nullptr, gam, bet, p.qk_eps, has_rope, (qk_video >> g) & 1u, qk_tab[g % QK_RING], qk_which == 0 && p.q_premul != 1.0f, p.q_premul);
          if (has_rope && g + QK_RING < 16) qk_fetch(g + QK_RING);   // refill the slot just consumed
          if (m < p.M) *(u32x4*)(p.C + m * p.ldc + n) = val;
        }
      }
    }
    if (!qk_done)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int row = g * 8 + rsub;
      const long long m = bm0 + wm * TM * 16 + row;
      u32x4 val = *(const u32x4*)(wbase + row * ROWB + chunk * 16);
      if (m < p.M && n + 8 <= p.N) {
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
      } else if (m < p.M && n + 4 <= p.N) {   // N % 8 == 4 tail
        u32x2 half = {val[0], val[1]};
        if constexpr (EPI == MRAG_EPI_GATE_RESID || EPI == MRAG_EPI_RESID) {
          const u32x2 rr = *(const u32x2*)(p.resid + m * p.ldr + n);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const float lo = __uint_as_float(half[e] << 16) + __uint_as_float(rr[e] << 16);
            const float hi = __uint_as_float(half[e] & 0xffff0000u) + __uint_as_float(rr[e] & 0xffff0000u);
            half[e] = pack_bf2(lo, hi);
          }
        }
        *(u32x2*)(p.C + m * p.ldc + n) = half;
      }
    }
    return;
  }
  // ---- the 256x320 tile (TN = 5: 80 columns = 160 bytes per wave row; the UNets' level-0 convolutions and linears, N = 320 / 960): the same staging in two
  // halves of 64 rows (8 waves x 64 x 176 B fit the operand stages; 128 rows would not).  In the row layout ten lanes hold a 160-byte row segment, so a store /
  // residual-load instruction moves 6.4 whole segments instead of 8-byte pieces of 16 rows -- the direct form cost the residual convolutions ~100 us each at level 0.
  constexpr bool STAGED5 = (TM == 8 && TN == 5 && WM == 2 && WN == 4 && !SK);
  constexpr bool EPI5 = (EPI == MRAG_EPI_NONE || EPI == MRAG_EPI_GELU_TANH || EPI == MRAG_EPI_GELU_ERF || EPI == MRAG_EPI_SILU || EPI == MRAG_EPI_RESID);
  if constexpr (STAGED5 && EPI5) {
    if (p.staged) {
      __syncthreads();   // every wave is done with the operand stages that the per-wave regions overlay
      const long long n0w = bn0 + wn * 80;
      if (n0w + 80 <= p.N) {
        constexpr int ROWB5 = 176;                      // 160 + 16: the 8-byte writes of 16 rows spread over the banks
        char* wbase = smem + wave * (64 * ROWB5);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 5; ++j) {
              const long long n = n0w + j * 16 + frag_q * 4;
              const f32x4 a4 = acc[half * 4 + i][j];
              float v[4] = {a4[0], a4[1], a4[2], a4[3]};
              if (p.bias) {
                const u32x2 bb = *(const u32x2*)(p.bias + n);
                v[0] += __uint_as_float(bb[0] << 16); v[1] += __uint_as_float(bb[0] & 0xffff0000u);
                v[2] += __uint_as_float(bb[1] << 16); v[3] += __uint_as_float(bb[1] & 0xffff0000u);
              }
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] = epi_act<EPI>(v[e]);
              if constexpr (EPI == MRAG_EPI_RESID) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] *= p.acc_scale;
              }
              u32x2 out;
              out[0] = pack_bf2(v[0], v[1]);
              out[1] = pack_bf2(v[2], v[3]);
              *(u32x2*)(wbase + (i * 16 + frag_row) * ROWB5 + (j * 16 + frag_q * 4) * 2) = out;
            }
          }
          // row layout: chunk index c = t * 64 + lane of the half's 64 x 10 sixteen-byte chunks
          const long long mrow0 = bm0 + wm * 128 + half * 64;
#pragma unroll
          for (int tb = 0; tb < 10; tb += 5) {            // (five residual vectors in flight: ten cost the 160 accumulator registers a spill)
            u32x4 rpre[5];
            if constexpr (EPI == MRAG_EPI_RESID) {
#pragma unroll
              for (int t = 0; t < 5; ++t) {
                const unsigned c = (unsigned)((tb + t) * 64 + lane), row = (c * 6554u) >> 16, ch = c - row * 10u;
                const long long m = mrow0 + row;
                rpre[t] = m < p.M ? *(const u32x4*)(p.resid + m * p.ldr + n0w + ch * 8) : u32x4{0u, 0u, 0u, 0u};
              }
            }
#pragma unroll
            for (int t = 0; t < 5; ++t) {
              const unsigned c = (unsigned)((tb + t) * 64 + lane), row = (c * 6554u) >> 16, ch = c - row * 10u;
              const long long m = mrow0 + row;
              u32x4 val = *(const u32x4*)(wbase + row * ROWB5 + ch * 16);
              if constexpr (EPI == MRAG_EPI_RESID) {
                const u32x4 rr = rpre[t];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const float lo = __uint_as_float(val[e] << 16) + __uint_as_float(rr[e] << 16);
                  const float hi = __uint_as_float(val[e] & 0xffff0000u) + __uint_as_float(rr[e] & 0xffff0000u);
                  val[e] = pack_bf2(lo, hi);
                }
              }
              if (m < p.M) *(u32x4*)(p.C + m * p.ldc + n0w + ch * 8) = val;
            }
          }
        }
      } else {
        epilogue_direct<TM, TN, EPI>(p, acc, bm0, bn0, wm * TM * 16, wn * TN * 16, lane);
      }
      return;
    }
  }
  if constexpr (is_geglu<EPI> && TN % 2 != 0) {
    return;   // never dispatched: the value / gate pairing needs an even number of 16-column tiles per wave
  } else if constexpr (is_geglu<EPI>) {
    // W rows arrive interleaved in 16-row groups: [value 16m..16m+15 | gate 16m..16m+15], so the even 16-column MFMA tile
    // holds the values and the odd one the gates of the SAME 16 outputs in the same lanes: C[m, j] = v * gelu_erf(g),
    // C is [M, N/2].  Removes the [M, N] round trip and the separate GEGLU pass (6 % of an SVD / DynamiCrafter step).
    if constexpr (TM == 8 && TN == 4 && WM == 2 && WN == 4) {
      if (p.staged) {
        // LDS-staged form (as above): the wave's 128 x 32 outputs go through LDS (row pitch 80 B) and leave as 64-byte row segments with
        // 16-byte lanes instead of 8-byte pieces of 16 rows per store.  The UNets' GEGLU projections have K = 320 ... 1280, i.e. 5-20
        // K-tiles per workgroup, so the store tail is most of a workgroup's life there.
        constexpr int ROWB = 80;
        char* wbase = smem + wave * (128 * ROWB);
        __syncthreads();   // every wave is done with the operand stages that these per-wave regions overlay
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
          for (int j = 0; j < TN; j += 2) {
            long long n = bn0 + wn * TN * 16 + j * 16 + frag_q * 4;   // value columns; gates at n + 16
            n = n + 20 <= p.N ? n : p.N - 20;                          // clamped columns are never stored
            float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            float g[4] = {acc[i][j + 1][0], acc[i][j + 1][1], acc[i][j + 1][2], acc[i][j + 1][3]};
            if (p.bias) {
              const u32x2 bv = *(const u32x2*)(p.bias + n), bg = *(const u32x2*)(p.bias + n + 16);
              v[0] += __uint_as_float(bv[0] << 16); v[1] += __uint_as_float(bv[0] & 0xffff0000u);
              v[2] += __uint_as_float(bv[1] << 16); v[3] += __uint_as_float(bv[1] & 0xffff0000u);
              g[0] += __uint_as_float(bg[0] << 16); g[1] += __uint_as_float(bg[0] & 0xffff0000u);
              g[2] += __uint_as_float(bg[1] << 16); g[3] += __uint_as_float(bg[1] & 0xffff0000u);
            }
            geglu4<EPI == EPI_GEGLU_TANH>(v, g);
            u32x2 out;
            out[0] = pack_bf2(v[0], v[1]);
            out[1] = pack_bf2(v[2], v[3]);
            *(u32x2*)(wbase + (i * 16 + frag_row) * ROWB + ((j >> 1) * 16 + frag_q * 4) * 2) = out;
          }
        }
        // row layout: lane -> row (lane >> 2) of a 16-row group, 16-byte chunk (lane & 3): one instruction = 16 x 64 contiguous bytes
        const int rs = lane >> 2, ch = lane & 3;
        const long long no = ((bn0 + wn * TN * 16) >> 1) + ch * 8;
#pragma unroll
        for (int g8 = 0; g8 < 8; ++g8) {
          const int row = g8 * 16 + rs;
          const long long m = bm0 + wm * TM * 16 + row;
          const u32x4 val = *(const u32x4*)(wbase + row * ROWB + ch * 16);
          if (m < p.M && 2 * (no + 8) <= p.N) *(u32x4*)(p.C + m * p.ldc + no) = val;
        }
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const long long m = bm0 + wm * TM * 16 + i * 16 + frag_row;
      if (m >= p.M) continue;
#pragma unroll
      for (int j = 0; j < TN; j += 2) {
        const long long n = bn0 + wn * TN * 16 + j * 16 + frag_q * 4;   // value columns; gates at n + 16
        if (n >= p.N) continue;
        float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
        float g[4] = {acc[i][j + 1][0], acc[i][j + 1][1], acc[i][j + 1][2], acc[i][j + 1][3]};
        if (p.bias) {
          const u32x2 bv = *(const u32x2*)(p.bias + n), bg = *(const u32x2*)(p.bias + n + 16);
          v[0] += __uint_as_float(bv[0] << 16); v[1] += __uint_as_float(bv[0] & 0xffff0000u);
          v[2] += __uint_as_float(bv[1] << 16); v[3] += __uint_as_float(bv[1] & 0xffff0000u);
          g[0] += __uint_as_float(bg[0] << 16); g[1] += __uint_as_float(bg[0] & 0xffff0000u);
          g[2] += __uint_as_float(bg[1] << 16); g[3] += __uint_as_float(bg[1] & 0xffff0000u);
        }
        // the reference rounds both halves of proj(x) to bf16 before the product (nn.Linear output dtype)
        geglu4<EPI == EPI_GEGLU_TANH>(v, g);
        u32x2 out;
        out[0] = pack_bf2(v[0], v[1]);
        out[1] = pack_bf2(v[2], v[3]);
        const long long no = ((bn0 + wn * TN * 16 + j * 16) >> 1) + frag_q * 4;
        *(u32x2*)(p.C + m * p.ldc + no) = out;
      }
    }
    return;
  }
  epilogue_direct<TM, TN, EPI>(p, acc, bm0, bn0, wm * TM * 16, wn * TN * 16, lane);
}

template <int WM, int WN, int TM, int TN, int EPI, int CONV = 0, bool SK = false>
__global__ __launch_bounds__(WM* WN * 64) void gemm_bf16_kernel(const GemmP p) {
  if constexpr (!SK) {
    // the grid is the logical tile range [0, gridDim.x): every tile, or the whole rounds in front of a stream-K tail launch
    gemm_tile<WM, WN, TM, TN, EPI, CONV, false>(p, xcd_remap(blockIdx.x, gridDim.x), 0, (int)(p.K / 64), 0, 0);
  } else {
    // the tail launch: sk_units runs of K-tiles share the sk_rem tiles behind logical tile sk_main evenly.  A run touches at most two tiles, and
    // each of its (at most) two pieces is a workgroup of its own -- blockIdx = 2 unit + piece -- so this wrapper is straight-line code: a loop
    // over the pieces made hipcc keep the whole argument struct in SGPRs across it (106 SGPRs, 40-86 spilled VGPRs, reloads inside the K loop)
    // Runs are dealt to XCDs in contiguous chunks, like the tiles of the main launch: consecutive runs work on neighbouring tiles (shared A / W
    // panels) at nearly the same K offset, so an XCD's L2 serves the panels once instead of every CU streaming its own from HBM
    const int nkf = (int)(p.K / 64), I = p.sk_rem * nkf, unit = xcd_remap(blockIdx.x >> 1, p.sk_units);
    const int it0 = (int)(((long long)unit * I) / p.sk_units), it1 = (int)(((long long)(unit + 1) * I) / p.sk_units);
    const int T0 = it0 / nkf, cut = min(it1, (T0 + 1) * nkf);          // the first piece ends at its tile's last K-tile
    const int it = (blockIdx.x & 1) ? cut : it0, end = (blockIdx.x & 1) ? it1 : cut;
    if (it >= end) return;
    const int T = it / nkf;
    gemm_tile<WM, WN, TM, TN, EPI, CONV, true>(p, p.sk_main + T, it - T * nkf, end - it, T, unit);
  }
}

// one tile shape: the epilogues that exist on it (convolutions carry bias / residual only), the kernel counted, the stream-K tail behind the whole rounds
template <int WM, int WN, int TM, int TN, int CONV = 0>
int launch_cfg(hipStream_t s, const GemmP& p0, int epi, const SkPlan* sk = nullptr) {
  constexpr int BM = WM * TM * 16, BN = WN * TN * 16;
  GemmP p = p0;
  p.tiles_m = (int)((p.M + BM - 1) / BM);
  p.tiles_n = (int)((p.N + BN - 1) / BN);
  p.group_m = group_m_of(p.tuning);
  const dim3 grid(sk ? sk->n_main : p.tiles_m * p.tiles_n), block(WM * WN * 64);   // with a stream-K plan: the whole rounds here, the tail as a second launch
  // the LDS-staged epilogue needs 16-byte aligned rows of C (and of the residual); otherwise the direct 8-byte store path runs
  p.staged = rows_16B_aligned(p.C, p.ldc, p.resid, p.ldr);
  if ((p.tuning & MRAG_GEMM_TUNE_NO_STAGED) || ((epi == MRAG_EPI_GEGLU || epi == EPI_GEGLU_TANH) && (p.N % 32 != 0 || (p.tuning & MRAG_GEMM_TUNE_GEGLU_NO_STAGED)))) p.staged = 0;
  if (epi == MRAG_EPI_QKNORM_ROPE && !((WM == 2 && WN == 4 && TM == 8 && TN == 4) && p.staged)) return MRAG_ENOTSUP;   // lives in the LDS-staged epilogue
  const size_t lds_stages = 2 * (BM + BN) * 64 * 2;
  size_t lds = (WM == 2 && WN == 4 && TM == 8 && TN == 4 && lds_stages < 8 * 128 * 144) ? 8 * 128 * 144 : lds_stages;
  if constexpr (CONV != 0 && WM == 2 && WN == 4 && TM == 8 && TN == 4) {   // the SLIM form's eight parked words per lane (gemm_tile: cv_park)
    p.cv_lds = (int)lds;
    lds += (size_t)WM * WN * 64 * 32;
  }
  if (sk && !(WM == 2 && WN == 4 && TM == 8 && TN == 4 && CONV == 0)) return MRAG_ENOTSUP;   // the stream-K tail exists on the linears' 8-wave 256x256 tile only
  int rc;
  if constexpr (CONV != 0) {   // convolutions carry bias / residual only
    switch (epi) {
      case MRAG_EPI_NONE: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_NONE, CONV>, grid, block, lds, s, p); break;
      case MRAG_EPI_RESID: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_RESID, CONV>, grid, block, lds, s, p); break;
      default: return MRAG_EINVAL;
    }
  } else {
    switch (epi) {
      case MRAG_EPI_NONE: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_NONE, CONV>, grid, block, lds, s, p); break;
      case MRAG_EPI_GELU_TANH: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_GELU_TANH, CONV>, grid, block, lds, s, p); break;
      case MRAG_EPI_GELU_ERF: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_GELU_ERF, CONV>, grid, block, lds, s, p); break;
      case MRAG_EPI_RESID: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_RESID, CONV>, grid, block, lds, s, p); break;
      case MRAG_EPI_GATE_RESID: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_GATE_RESID, CONV>, grid, block, lds, s, p); break;
      case MRAG_EPI_SILU: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_SILU, CONV>, grid, block, lds, s, p); break;
      case MRAG_EPI_GEGLU: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_GEGLU, CONV>, grid, block, lds, s, p); break;
      case EPI_GEGLU_TANH: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, EPI_GEGLU_TANH, CONV>, grid, block, lds, s, p); break;
      case MRAG_EPI_QKNORM_ROPE: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_QKNORM_ROPE, CONV>, grid, block, lds, s, p); break;
      default: return MRAG_EINVAL;
    }
  }
  if (rc != MRAG_OK) return rc;
  {
    constexpr int tile = (BM == 256 && BN == 320) ? 1 : (BM == 256 && BN == 128) ? 2 : (BM == 128 && BN == 128) ? 3 : (BM == 192) ? 4 : 0;   // 0: 256x256 (8 or 16 waves)
    constexpr int ids[3][5] = {{MRAG_K_GEMM_256x256, MRAG_K_GEMM_256x320, MRAG_K_GEMM_256x128, MRAG_K_GEMM_128x128, MRAG_K_GEMM_192x256},
                               {MRAG_K_CONV3_256x256, MRAG_K_CONV3_256x320, MRAG_K_CONV3_256x128, MRAG_K_CONV3_128x128, MRAG_K_CONV3_192x256},
                               {MRAG_K_CONVT_256x256, MRAG_K_CONVT_256x320, MRAG_K_CONVT_256x128, MRAG_K_CONVT_128x128, MRAG_K_CONVT_192x256}};
    MRAG_COUNT(ids[CONV][tile]);
  }
  if constexpr (WM == 2 && WN == 4 && TM == 8 && TN == 4 && CONV == 0) {
    if (sk) {   // the partial last round.  Its own launch: the main kernel keeps its register allocation, and whole rounds end together anyway
      const dim3 tgrid(2 * sk->units);
      switch (epi) {
        case MRAG_EPI_NONE: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_NONE, 0, true>, tgrid, block, lds + 16, s, p); break;
        case MRAG_EPI_GELU_TANH: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_GELU_TANH, 0, true>, tgrid, block, lds + 16, s, p); break;
        case MRAG_EPI_RESID: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_RESID, 0, true>, tgrid, block, lds + 16, s, p); break;
        case MRAG_EPI_GATE_RESID: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_GATE_RESID, 0, true>, tgrid, block, lds + 16, s, p); break;
        case MRAG_EPI_QKNORM_ROPE: rc = launch_dyn_lds(gemm_bf16_kernel<WM, WN, TM, TN, MRAG_EPI_QKNORM_ROPE, 0, true>, tgrid, block, lds + 16, s, p); break;
        default: return MRAG_EINVAL;   // mrag_gemm_bf16 plans a tail for these five only
      }
      if (rc != MRAG_OK) return rc;
      MRAG_COUNT(MRAG_K_GEMM_STREAMK_TAIL);
    }
  }
  return MRAG_OK;
}

}  // namespace
