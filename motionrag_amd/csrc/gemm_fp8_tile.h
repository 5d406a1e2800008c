// gemm_fp8_tile.h -- the e4m3 256x256 tile that gemm_fp8_kernel (gemm_fp8.hip) and conv_fp8_kernel (conv_fp8.hip) are built on: everything between
// "the operand bytes are on their way to LDS" and "the wave's bf16 tile sits in LDS".  The kernels keep what differs: how the DMA lanes address their
// operands (plain rows / the tap walk with its border predicate), where the activation rows' scales come from, and the row-layout store.
//
// Tile shape: 256x256 on 8 waves (2 x 4, 128 rows x 64 columns each: 4 x 2 accumulators of 32x32), K-tiles of 128 bytes = two 64-deep MFMA steps, two
// LDS stages of 64 KiB filled by 16-byte global_load_lds in 1-KiB pieces (8 rows x 128 B; activation rows first, then W rows) with the XOR swizzle on the
// SOURCE address (chunk ^= row & 7) and on the ds_read_b128 -- the LDS image and idiom of gemm_tile.h with bytes for bf16 pairs.  A kernel issues the DMA
// of K-tile t + 1 behind the barrier that opens tile t (between fp8_tile_read and fp8_tile_mfma of k-step 0: after the reads, in front of their first wait) and
// retires it by the vmcnt(0) in front of the next barrier.  The fragment reads are hand-written (a compiler-made LDS load would be ordered behind the DMA
// in flight: vmcnt(0)) and released to the MFMAs by counted lgkmcnt.
// Operand maps as measured (tools/exp/fp8_layout_probe.hip): lane l holds A[row l & 31][k = 32 (l >> 5) + byte], B likewise.  W is the A operand
// and the activations the B operand, so a lane owns 4 consecutive output columns of one row per register quad (C/D: column = lane & 31 -> m,
// row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) -> n).  The rows' power-of-two exponents ride the instruction's E8M0 scale operands (127 - e per lane: a
// lane's scale byte applies to its own row's 32 k's).
// Epilogue: the LDS-staged form of gemm_tile.h (same rounding points: bias / activation / gate in the accumulator layout, rounded to bf16, the residual
// added in the row layout, so the output may alias the residual); the per-wave regions (128 rows, pitch 144 B) overlay the operand stages.
// Form: the helpers compute values from values (no per-lane state struct, no array filled behind a reference), which is what kept both kernels'
// instruction streams what they were when the code moved here (profiles/fp8_tile_refactor.txt).  For the same reason conv_fp8_kernel keeps its own lines
// for the accumulator-to-LDS store (its bias adds interleave with the packing) and both kernels spell rowA / rowW themselves.
#pragma once
#include "gemm_common.h"

namespace {

constexpr int F8_BM = 256, F8_BN = 256, F8_BK = 128;        // BK in bytes == e4m3 elements: two 64-deep steps
constexpr int F8_STAGE = (F8_BM + F8_BN) * F8_BK;          // 64 KiB
constexpr int F8_ROWB = 144;                               // staged epilogue: row pitch of a wave's 128 x 64 bf16 tile
constexpr int F8_EPI_LDS = 8 * 128 * F8_ROWB;              // 144 KiB: the epilogue's per-wave regions overlay the two operand stages (128 KiB)
static_assert(F8_EPI_LDS >= 2 * F8_STAGE, "the operand stages fit the allocation");

// logical tile order of gemm_tile.h: groups of group_m m-tiles walked n-major behind the XCD remap -> first row / column of this workgroup's tile
__device__ __forceinline__ void fp8_tile_origin(const int tiles_m, const int tiles_n, const int group_m, long long& bm0, long long& bn0) {
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int gw = group_m * tiles_n;
  const int first_m = (wg / gw) * group_m;
  const int gsz = min(tiles_m - first_m, group_m);
  const int tile_m = first_m + (wg % gw) % gsz, tile_n = (wg % gw) / gsz;
  bm0 = (long long)tile_m * F8_BM;
  bn0 = (long long)tile_n * F8_BN;
}

// E8M0 scale operand of a W row (A operand) or an activation row (B operand) from its exponent: the byte 127 - e in all four positions; rows behind the
// last one take the last one's (their products are never stored).  T: the caller's type of `rows` (its arithmetic is the caller's)
template <class T>
__device__ __forceinline__ int fp8_row_scale(const int* e, long long row, const T rows) {
  row = row < rows ? row : rows - 1;
  return ((127 - e[row]) & 0xff) * 0x01010101;
}

// fragment read addresses: a lane reads row r32 of each 32-row block (pitch 4096) of its wave's rows (LDS row pitch 128: the activation rows, then F8_BM
// rows on W's); of the 64-byte k-step ks bytes 32 hh .. + 31 as two 16-byte chunks c, un-swizzled by row & 7 -> the chunk's byte offset inside the row
__device__ __forceinline__ unsigned fp8_frag_chunk(const int ks, const int hh, const int c, const int r32) { return (unsigned)(((4 * ks + 2 * hh + c) ^ (r32 & 7)) << 4); }

// ---- the k-step.  SCALE_WORD says where the four activation-row scale operands come from: false, the caller's four registers `sa` (gemm_fp8_kernel: a
// row's scale is the same in every step); true, one LDS word per step at `sc_addr` holding the four row blocks' bytes (conv_fp8_kernel: the scale is
// that of the pixel a row reads under the step's tap), read by a ds_read_b32 in front of the fragment reads and spread by v_perm_b32.  LDS reads return
// in order and the word is released with the first pair of rows, so the counted waits are the same in both forms.
struct Fp8Frag {
  u32x4 w[4], a[8];
  unsigned s;   // SCALE_WORD only
};

// twelve reads of one k-step in one statement (W blocks first)
#define MRAG_FP8_READ12                                                                                                              \
  "ds_read_b128 %0, %[w0]\n\tds_read_b128 %1, %[w1]\n\tds_read_b128 %2, %[w0] offset:4096\n\tds_read_b128 %3, %[w1] offset:4096\n\t" \
  "ds_read_b128 %4, %[a0]\n\tds_read_b128 %5, %[a1]\n\tds_read_b128 %6, %[a0] offset:4096\n\tds_read_b128 %7, %[a1] offset:4096\n\t" \
  "ds_read_b128 %8, %[a0] offset:8192\n\tds_read_b128 %9, %[a1] offset:8192\n\tds_read_b128 %10, %[a0] offset:12288\n\tds_read_b128 %11, %[a1] offset:12288"
#define MRAG_FP8_READ12_OUT(F)                                                                                                        \
  "=&v"(F.w[0]), "=&v"(F.w[1]), "=&v"(F.w[2]), "=&v"(F.w[3]), "=&v"(F.a[0]), "=&v"(F.a[1]), "=&v"(F.a[2]), "=&v"(F.a[3]), "=&v"(F.a[4]), "=&v"(F.a[5]), \
      "=&v"(F.a[6]), "=&v"(F.a[7])
// a wait names the registers it releases ("+v"): the MFMAs that read them cannot be scheduled in front of it
#define MRAG_FP8_WAIT(N, ...) asm volatile("s_waitcnt lgkmcnt(" #N ")" : __VA_ARGS__ :: "memory")
#define MRAG_FP8_W(F) "+v"(F.w[0]), "+v"(F.w[1]), "+v"(F.w[2]), "+v"(F.w[3])

// the reads of one k-step: w0, w1 / a0, a1 the two chunks of the lane's first W / activation row (row + stage + fp8_frag_chunk)
template <bool SCALE_WORD>
__device__ __forceinline__ void fp8_tile_read(Fp8Frag& f, const unsigned w0, const unsigned w1, const unsigned a0, const unsigned a1, const unsigned sc_addr = 0) {
  if constexpr (SCALE_WORD)
    asm volatile("ds_read_b32 %12, %[sc]\n\t" MRAG_FP8_READ12
                 : MRAG_FP8_READ12_OUT(f), "=&v"(f.s)
                 : [w0] "v"(w0), [w1] "v"(w1), [a0] "v"(a0), [a1] "v"(a1), [sc] "v"(sc_addr)
                 : "memory");
  else
    asm volatile(MRAG_FP8_READ12 : MRAG_FP8_READ12_OUT(f) : [w0] "v"(w0), [w1] "v"(w1), [a0] "v"(a0), [a1] "v"(a1) : "memory");
}

__device__ __forceinline__ i32x8 fp8_frag8(const u32x4 x, const u32x4 y) {
  return i32x8{(int)x[0], (int)x[1], (int)x[2], (int)x[3], (int)y[0], (int)y[1], (int)y[2], (int)y[3]};
}

// row block I against both column blocks
template <bool SCALE_WORD, int I>
__device__ __forceinline__ void fp8_tile_row(f32x16 (&acc)[4][2], const Fp8Frag& f, const int (&sw)[2], const int* sa) {
  const i32x8 af = fp8_frag8(f.a[2 * I], f.a[2 * I + 1]);
  int s;
  if constexpr (SCALE_WORD) s = (int)__builtin_amdgcn_perm(f.s, f.s, 0x01010101u * I);   // byte I of the word, replicated
  else s = sa[I];
  acc[I][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fp8_frag8(f.w[0], f.w[1]), af, acc[I][0], 0, 0, 0, sw[0], 0, s);
  acc[I][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fp8_frag8(f.w[2], f.w[3]), af, acc[I][1], 0, 0, 0, sw[1], 0, s);
}

// the waits and the eight MFMAs behind fp8_tile_read (sa: the four scale registers, unread when SCALE_WORD).  The order below is the schedule (hipcc would
// gather the four waits in front of the first MFMA): each pair of MFMAs starts when ITS rows are here
template <bool SCALE_WORD>
__device__ __forceinline__ void fp8_tile_mfma(f32x16 (&acc)[4][2], Fp8Frag& f, const int (&sw)[2], const int* sa = nullptr) {
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (SCALE_WORD) MRAG_FP8_WAIT(6, "+v"(f.s), MRAG_FP8_W(f), "+v"(f.a[0]), "+v"(f.a[1]));
  else MRAG_FP8_WAIT(6, MRAG_FP8_W(f), "+v"(f.a[0]), "+v"(f.a[1]));
  fp8_tile_row<SCALE_WORD, 0>(acc, f, sw, sa);
  __builtin_amdgcn_sched_barrier(0);
  MRAG_FP8_WAIT(4, "+v"(f.a[2]), "+v"(f.a[3]));
  fp8_tile_row<SCALE_WORD, 1>(acc, f, sw, sa);
  __builtin_amdgcn_sched_barrier(0);
  MRAG_FP8_WAIT(2, "+v"(f.a[4]), "+v"(f.a[5]));
  fp8_tile_row<SCALE_WORD, 2>(acc, f, sw, sa);
  __builtin_amdgcn_sched_barrier(0);
  MRAG_FP8_WAIT(0, "+v"(f.a[6]), "+v"(f.a[7]));
  fp8_tile_row<SCALE_WORD, 3>(acc, f, sw, sa);
  __builtin_amdgcn_sched_barrier(0);
}
#undef MRAG_FP8_READ12
#undef MRAG_FP8_READ12_OUT
#undef MRAG_FP8_WAIT
#undef MRAG_FP8_W

// ---- the staged epilogue's common parts

// four consecutive bf16 (a bias / gate quad of the lane's four columns) as floats
__device__ __forceinline__ void fp8_unpack_bf4(const u32x2 b, float (&o)[4]) {
  o[0] = __uint_as_float(b[0] << 16); o[1] = __uint_as_float(b[0] & 0xffff0000u);
  o[2] = __uint_as_float(b[1] << 16); o[3] = __uint_as_float(b[1] & 0xffff0000u);
}

// v += such a quad (the bias)
__device__ __forceinline__ void fp8_add_bf4(const bf16_t* src, float (&v)[4]) {
  const u32x2 b = *(const u32x2*)src;
  v[0] += __uint_as_float(b[0] << 16); v[1] += __uint_as_float(b[0] & 0xffff0000u);
  v[2] += __uint_as_float(b[1] << 16); v[3] += __uint_as_float(b[1] & 0xffff0000u);
}

// an accumulator quad, rounded to bf16, to (lrow, lcol) of the wave's region
__device__ __forceinline__ void fp8_stage_quad(char* wbase, const int lrow, const int lcol, const float (&v)[4]) {
  u32x2 out;
  out[0] = pack_bf2(v[0], v[1]);
  out[1] = pack_bf2(v[2], v[3]);
  *(u32x2*)(wbase + lrow * F8_ROWB + lcol * 2) = out;
}

// eight packed bf16 plus eight packed bf16 (the residual in the row layout), rounded once
__device__ __forceinline__ u32x4 fp8_add_bf8(u32x4 val, const u32x4 rr) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float lo = __uint_as_float(val[e] << 16) + __uint_as_float(rr[e] << 16);
    const float hi = __uint_as_float(val[e] & 0xffff0000u) + __uint_as_float(rr[e] & 0xffff0000u);
    val[e] = pack_bf2(lo, hi);
  }
  return val;
}

}  // namespace
