// ff_fused.hip -- the UNets' 320-channel feed-forward in ONE launch (mrag_ff_fused_bf16, opt-in through layers.set_ff_fusion):
//   y = x + W2 . (value * gelu_erf(gate)) + b2,   [value | gate] = W1 . LayerNorm(x) + b1          (C = 320, inner % 64 == 0)
// Today's path is three launches (LayerNorm, the GEGLU projection, the output projection with its residual) that move the normalised rows once and the
// 4 C wide hidden tensor twice through HBM.  Here neither leaves the chip: a workgroup owns FF_ROWS = 128 rows, a wave 32 of them, for the whole product.
//
// Per wave (one per SIMD, the whole 512-entry register file):
//   xn   the wave's 32 normalised rows as the B fragments of v_mfma_f32_32x32x16_bf16, 20 k-steps x 4 = 80 registers (rounded to bf16 once: the
//        LayerNorm launch's output);
//   O    the 32 x 320 fp32 outputs, TRANSPOSED (O^T = W2 . P^T: channel tiles of 32 on the registers, the row on the lane), 10 x 16 = 160 registers,
//        initialised with x + b2, so that the residual needs no second pass and the epilogue is one rounding;
//   S    one 32 x 32 score tile S^T = W1t . xn^T per step: the A operand's 32 rows are 16 value rows and the 16 gate rows of the same hidden units,
//        so value and gate of a hidden unit meet in ONE lane (registers q and q + 8) and value * gelu(gate) is lane-local; the 8 products of a lane
//        are, packed to bf16, the B fragment of the second product (a 32x32 accumulator tile is the next MFMA's operand when that sums over the
//        tile's rows).  A lane's A row a reads W1 row pi(a) (bits 2 and 3 of the hidden index swapped), which makes fragment element j of lane half
//        h the hidden unit 8 h + j: W2's A fragment is then 16 contiguous bytes.
// W1 (interleaved, ops.geglu_interleave) and W2 are streamed through LDS in chunks of FF_CHUNK = 32 hidden units (64 W1 rows = 40 KB + a [320, 32] slice of
// W2 = 20 KB), two stages, filled by LDS-DMA one chunk ahead; both stay in L2 (2.4 MB at inner = 1280).  The images are 16-byte granule permutations of
// the sources (the DMA's destination is lane-linear, its source address per lane), chosen so that every ds_read_b128 lane group meets 16 distinct slots:
//   W1 row rho (640 B): granule g at g ^ ((rho >> 1) & 7);   W2 channel c (64 B): granule q at q ^ ((c >> 2) & 3).
// One barrier per chunk: wave-local vmcnt(0), barrier (chunk c has landed everywhere, chunk c - 1's stage is free), then the DMA of chunk c + 1.
#include "common.h"
#include "../../include/mrag_hip.h"

namespace {

constexpr int FF_C = 320, FF_ROWS = MRAG_FF_FUSED_ROWS, FF_CHUNK = 32;
constexpr int FF_W1_BYTES = 2 * FF_CHUNK * FF_C * 2, FF_W2_BYTES = FF_C * FF_CHUNK * 2, FF_B1_OFF = FF_W1_BYTES + FF_W2_BYTES;
constexpr int FF_STAGE = FF_B1_OFF + 1024;                   // (the chunk's 128 bytes of b1 arrive as one whole 1 KiB DMA piece: lanes 8 .. 63 repeat them)
constexpr long long FF_MAX_INNER = 1ll << 20;                // a lane's W2 source offset (row x inner x 2 bytes) stays below 2^32
static_assert(FF_ROWS == 128, "four waves of 32 rows");

struct FfP {
  const bf16_t* x; const bf16_t* gamma; const bf16_t* beta; const bf16_t* w1; const bf16_t* b1; const bf16_t* w2; const bf16_t* b2; bf16_t* out;
  long long rows, inner, ldx, ldo;
  float eps;
};

unsigned long long g_ff_fused_launches[1];

__device__ __forceinline__ void unpack8f(const u32x4 a, float (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[2 * e] = __uint_as_float(a[e] << 16); v[2 * e + 1] = __uint_as_float(a[e] & 0xffff0000u); }
}

// The loop's fragment reads are inline asm with counted waits placed by hand (FF_WAIT): hipcc waits for its own ds_reads with lgkmcnt(0) here, which
// drains every read issued since -- the prefetch with them.  LDS returns in order, so "at most N outstanding" retires all but the youngest N reads.
// (The sched_barrier behind the wait: hipcc moves register-only MFMAs across an asm wait despite its memory clobber.)
#define FF_DS(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
#define FF_SB __builtin_amdgcn_sched_barrier(0)
#define FF_WAIT(n) do { asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory"); FF_SB; } while (0)
// k-steps 4 G .. 4 G + 3 of score tile TILE (0 / 1) of the stage, S^T += W1t . xn^T, as a read and a use; `a`: the LDS addresses of the lane's row at its four granule offsets
template <int TILE, int G>
__device__ __forceinline__ void score_read(bf16x8 (&f)[4], const unsigned (&a)[4]) {
  FF_DS(f[0], a[0], TILE * 20480 + G * 128); FF_DS(f[1], a[1], TILE * 20480 + G * 128);
  FF_DS(f[2], a[2], TILE * 20480 + G * 128); FF_DS(f[3], a[3], TILE * 20480 + G * 128);
}
template <int G>
__device__ __forceinline__ void score_mma(f32x16& s, const bf16x8 (&f)[4], const bf16x8 (&xn)[20]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[k], xn[4 * G + k], s, 0, 0, 0);
}
// output tiles T0 .. T0 + N - 1 of O^T += W2s . P^T; `w`: the LDS address of the lane's row of the step's W2 slice (tile t at + 2048 t)
template <int T0, int N>
__device__ __forceinline__ void out_read(bf16x8 (&f)[4], const unsigned w) {
  FF_DS(f[0], w, T0 * 2048); FF_DS(f[1], w, (T0 + 1) * 2048);
  if constexpr (N == 4) { FF_DS(f[2], w, (T0 + 2) * 2048); FF_DS(f[3], w, (T0 + 3) * 2048); }
}
template <int T0, int N>
__device__ __forceinline__ void out_mma(f32x16 (&O)[10], const bf16x8 (&f)[4], const bf16x8 p) {
#pragma unroll
  for (int k = 0; k < N; ++k) O[T0 + k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[k], p, O[T0 + k], 0, 0, 0);
}
// hidden units 2 E and 2 E + 1 of the lane: (value + bias) * gelu_erf(gate + bias) in fp32, rounded to bf16 once (the hidden tensor of the unfused path);
// `bv` / `bg`: the lane's eight value / gate biases as packed bf16
template <int E>
__device__ __forceinline__ unsigned geglu_pair(const f32x16& s, const u32x4 bv, const u32x4 bg) {
  const float v0 = s[2 * E] + __uint_as_float(bv[E] << 16), v1 = s[2 * E + 1] + __uint_as_float(bv[E] & 0xffff0000u);
  const float g0 = s[8 + 2 * E] + __uint_as_float(bg[E] << 16), g1 = s[9 + 2 * E] + __uint_as_float(bg[E] & 0xffff0000u);
  return pack_bf2(v0 * gelu_erf_f(g0), v1 * gelu_erf_f(g1));
}

__global__ __launch_bounds__(256) void ff_fused_kernel(const FfP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, half = lane >> 5;
  const long long nch = p.inner / FF_CHUNK;

  // ---- the DMA's per-lane source offsets.  Piece d = (4 i + wave) * 64 + lane of a stage is destination granule d.
  unsigned off1[10], off2[5];
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int d = (4 * i + wave) * 64 + lane, rho = d / 40, g = (d - rho * 40) ^ ((rho >> 1) & 7);
    off1[i] = (unsigned)(rho * 640 + g * 16);
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int d = (4 * i + wave) * 64 + lane, c = d >> 2, q = (d & 3) ^ ((c >> 2) & 3);
    off2[i] = (unsigned)c * (unsigned)p.inner * 2u + (unsigned)(q * 16);
  }
  // a chunk's 16 pieces per wave: 10 of W1, 5 of W2, and the chunk's b1 (wave 0 alone).  (Spread over the loop's MFMA groups instead of issued in a row
  // behind the barrier they measured 3 % slower.)
  auto issue = [&](const long long chunk, const int buf) {
    const char* s1 = (const char*)p.w1 + chunk * FF_W1_BYTES;
    const char* s2 = (const char*)p.w2 + chunk * (FF_CHUNK * 2);
    char* dst = smem + buf * FF_STAGE;
#pragma unroll
    for (int i = 0; i < 10; ++i) glds16(s1 + off1[i], dst + (4 * i + wave) * 1024);
#pragma unroll
    for (int i = 0; i < 5; ++i) glds16(s2 + off2[i], dst + FF_W1_BYTES + (4 * i + wave) * 1024);
    if (p.b1 && wave == 0) glds16(p.b1 + chunk * (2 * FF_CHUNK) + (lane & 7) * 8, dst + FF_B1_OFF);
  };

  // ---- the lane's read offsets.  A row a = r of a score tile is W1 row pi(a) of the tile's 32: 16 (a >> 4) + the hidden index with bits 2 and 3 swapped
  const int rho = (r & 16) | (r & 3) | ((r >> 1) & 4) | ((r << 1) & 8);
  const int gx = half ^ ((rho >> 1) & 7);
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  unsigned go[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) go[j] = (unsigned)(rho * 640 + ((2 * j) ^ gx) * 16);
  unsigned w2o[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) w2o[s] = (unsigned)(FF_W1_BYTES + r * 64 + ((2 * s + half) ^ ((r >> 2) & 3)) * 16);

  // ---- the wave's 32 rows, as the B fragments will hold them: lane (r, half) has channels 16 ks + 8 half .. + 7 of row r
  const long long row = (long long)blockIdx.x * FF_ROWS + wave * 32 + r;
  const bool ok = row < p.rows;                               // rows past the end re-read the last valid row (every load unconditional); their stores are skipped
  const bf16_t* xr = p.x + (ok ? row : p.rows - 1) * p.ldx;
  u32x4 raw[20];
#pragma unroll
  for (int ks = 0; ks < 20; ++ks) raw[ks] = *(const u32x4*)(xr + 16 * ks + 8 * half);
  // gamma | beta | b2 (640 B each; 1 / 0 / 0 where null: exact) into the second stage, which the DMA first writes behind the loop's first barrier.  Every
  // ordinary load of the prologue is issued AND consumed in front of the first DMA: behind one, hipcc waits for each with vmcnt(0), one round trip per load.
  char* const par = smem + FF_STAGE;
  if (wave < 3 && lane < 40) {
    const bf16_t* src = wave == 0 ? p.gamma : (wave == 1 ? p.beta : p.b2);
    u32x4 v = wave == 0 ? u32x4{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u} : u32x4{0u, 0u, 0u, 0u};
    if (src) v = *(const u32x4*)(src + 8 * lane);
    *(u32x4*)(par + wave * 640 + lane * 16) = v;
  }
  if (!p.b1 && wave == 3 && lane < 16) *(u32x4*)(smem + (lane >> 3) * FF_STAGE + FF_B1_OFF + (lane & 7) * 16) = u32x4{0u, 0u, 0u, 0u};   // no b1: both stages' bias pieces stay zero
  float sum = 0.f;
#pragma unroll
  for (int ks = 0; ks < 20; ++ks) {
    float v[8]; unpack8f(raw[ks], v);
#pragma unroll
    for (int e = 0; e < 8; ++e) sum += v[e];
  }
  sum += __shfl_xor(sum, 32);                                   // the other half of the row sits on lane ^ 32
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  issue(0, 0);

  // ---- LayerNorm in fp32 (the arithmetic of layernorm_kernel), rounded to bf16 into the B fragments
  bf16x8 xn[20];
  {
    const float mean = sum / (float)FF_C;
    float sq = 0.f;
#pragma unroll
    for (int ks = 0; ks < 20; ++ks) {
      float v[8]; unpack8f(raw[ks], v);
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = __fsub_rn(v[e], mean); sq = __builtin_fmaf(d, d, sq); }
    }
    sq += __shfl_xor(sq, 32);
    const float rstd = rsqrtf(sq / (float)FF_C + p.eps);
#pragma unroll
    for (int ks = 0; ks < 20; ++ks) {
      float v[8], g[8], b[8], o[8];
      unpack8f(raw[ks], v);
      unpack8f(*(const u32x4*)(par + (16 * ks + 8 * half) * 2), g);
      unpack8f(*(const u32x4*)(par + 640 + (16 * ks + 8 * half) * 2), b);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(v[e], mean), rstd), g[e]), b[e]);
      xn[ks] = __builtin_bit_cast(bf16x8, u32x4{pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7])});
    }
  }
  // ---- the output accumulators start as x + b2: tile t, register 4 m + i is channel 32 t + 8 m + 4 half + i of the lane's row.  Of k-step ks = 2 t + u the
  // lane holds channels 16 u + 8 half .. + 7 of the tile and needs 16 u + 4 half .. + 3 and 16 u + 8 + 4 half .. + 3: one 8-byte exchange with lane ^ 32.
  f32x16 O[10];
#pragma unroll
  for (int ks = 0; ks < 20; ++ks) {
    const int t = ks >> 1, u = ks & 1;
    const unsigned r0 = (unsigned)__shfl_xor((int)(half ? raw[ks][0] : raw[ks][2]), 32), r1 = (unsigned)__shfl_xor((int)(half ? raw[ks][1] : raw[ks][3]), 32);
    const u32x2 lo = half ? u32x2{r0, r1} : u32x2{raw[ks][0], raw[ks][1]}, hi = half ? u32x2{raw[ks][2], raw[ks][3]} : u32x2{r0, r1};
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const int m = 2 * u + w;
      const u32x2 xv = w ? hi : lo;
      const u32x2 bb = *(const u32x2*)(par + 1280 + (32 * t + 8 * m + 4 * half) * 2);
      O[t][4 * m + 0] = __uint_as_float(xv[0] << 16) + __uint_as_float(bb[0] << 16);
      O[t][4 * m + 1] = __uint_as_float(xv[0] & 0xffff0000u) + __uint_as_float(bb[0] & 0xffff0000u);
      O[t][4 * m + 2] = __uint_as_float(xv[1] << 16) + __uint_as_float(bb[1] << 16);
      O[t][4 * m + 3] = __uint_as_float(xv[1] & 0xffff0000u) + __uint_as_float(bb[1] & 0xffff0000u);
    }
  }

  for (long long c = 0; c < nch; ++c) {
    const int buf = (int)(c & 1);
    // this wave's pieces of chunk c have landed; behind the barrier everyone's have, and every wave has finished reading the other stage
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (c + 1 < nch) issue(c + 1, buf ^ 1);
    // Four sections, the vector work of one tile's GEGLU beside the matrix work of the next section:
    //   A  S_a;   B  S_b beside GEGLU(S_a);   C  O += W2_a . P_a beside GEGLU(S_b);   D  O += W2_b . P_b
    // in 16 groups of (mostly) four MFMAs.  Group i issues the fragment reads of group i + 2 (three register sets), waits until group i's have landed -- the
    // count is the reads of groups i + 1 and i + 2 -- and runs its MFMAs: a read has two groups' matrix time to land.  b1 joins in the GEGLU (beside
    // MFMAs), not in the accumulators' initial value; its four reads go first, so every later wait retires them.
    const unsigned sl = lds0 + (unsigned)(buf * FF_STAGE);
    const unsigned a[4] = {sl + go[0], sl + go[1], sl + go[2], sl + go[3]}, wa = sl + w2o[0], wb = sl + w2o[1], bl = sl + FF_B1_OFF + half * 16;
    bf16x8 fx[4], fy[4], fz[4];
    u32x4 bva, bga, bvb, bgb, pa, pb;
    f32x16 sa = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sb = sa;
    FF_DS(bva, bl, 0); FF_DS(bga, bl, 32); FF_DS(bvb, bl, 64); FF_DS(bgb, bl, 96);          // the lane's b1 pieces: step s value / gate at 64 s + {0, 32} bytes
    score_read<0, 0>(fx, a); score_read<0, 1>(fy, a);
    score_read<0, 2>(fz, a); FF_WAIT(8); score_mma<0>(sa, fx, xn); FF_SB;
    score_read<0, 3>(fx, a); FF_WAIT(8); score_mma<1>(sa, fy, xn); FF_SB;
    score_read<0, 4>(fy, a); FF_WAIT(8); score_mma<2>(sa, fz, xn); FF_SB;
    score_read<1, 0>(fz, a); FF_WAIT(8); score_mma<3>(sa, fx, xn); FF_SB;
    score_read<1, 1>(fx, a); FF_WAIT(8); score_mma<4>(sa, fy, xn); FF_SB;
    score_read<1, 2>(fy, a); FF_WAIT(8); score_mma<0>(sb, fz, xn); pa[0] = geglu_pair<0>(sa, bva, bga); FF_SB;
    score_read<1, 3>(fz, a); FF_WAIT(8); score_mma<1>(sb, fx, xn); pa[1] = geglu_pair<1>(sa, bva, bga); FF_SB;
    score_read<1, 4>(fx, a); FF_WAIT(8); score_mma<2>(sb, fy, xn); pa[2] = geglu_pair<2>(sa, bva, bga); FF_SB;
    out_read<0, 4>(fy, wa); FF_WAIT(8); score_mma<3>(sb, fz, xn); pa[3] = geglu_pair<3>(sa, bva, bga); FF_SB;
    out_read<4, 4>(fz, wa); FF_WAIT(8); score_mma<4>(sb, fx, xn); FF_SB;
    const bf16x8 pfa = __builtin_bit_cast(bf16x8, pa);
    out_read<8, 2>(fx, wa); FF_WAIT(6); out_mma<0, 4>(O, fy, pfa); pb[0] = geglu_pair<0>(sb, bvb, bgb); pb[1] = geglu_pair<1>(sb, bvb, bgb); FF_SB;
    out_read<0, 4>(fy, wb); FF_WAIT(6); out_mma<4, 4>(O, fz, pfa); pb[2] = geglu_pair<2>(sb, bvb, bgb); pb[3] = geglu_pair<3>(sb, bvb, bgb); FF_SB;
    out_read<4, 4>(fz, wb); FF_WAIT(8); out_mma<8, 2>(O, fx, pfa); FF_SB;
    const bf16x8 pfb = __builtin_bit_cast(bf16x8, pb);
    out_read<8, 2>(fx, wb); FF_WAIT(6); out_mma<0, 4>(O, fy, pfb); FF_SB;
    FF_WAIT(2); out_mma<4, 4>(O, fz, pfb); FF_SB;
    FF_WAIT(0); out_mma<8, 2>(O, fx, pfb); FF_SB;
                                           // (every read of the stage has landed: the next barrier frees it)
  }

  // ---- one rounding to bf16; 8 bytes per register quad, straight from the accumulator layout
  if (ok) {
    bf16_t* orow = p.out + row * p.ldo;
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
      for (int m = 0; m < 4; ++m)
        *(u32x2*)(orow + 32 * t + 8 * m + 4 * half) = u32x2{pack_bf2(O[t][4 * m], O[t][4 * m + 1]), pack_bf2(O[t][4 * m + 2], O[t][4 * m + 3])};
  }
}

#undef FF_DS
#undef FF_SB
#undef FF_WAIT

}  // namespace

extern "C" int mrag_ff_fused_supported(int64_t C, int64_t inner) { return C == FF_C && inner >= 64 && inner % 64 == 0 && inner <= FF_MAX_INNER ? 1 : 0; }

extern "C" int mrag_ff_fused_launch_counts(uint64_t* out_host, int32_t n) {
  for (int i = 0; out_host && i < n && i < 1; ++i) out_host[i] = __atomic_load_n(&g_ff_fused_launches[i], __ATOMIC_RELAXED);
  return 1;
}

extern "C" int mrag_ff_fused_bf16(void* stream, const mrag_ff_fused_args* a) {
  if (!a) return MRAG_EINVAL;
  if (!mrag_ff_fused_supported(a->C, a->inner)) return MRAG_ENOTSUP;
  if (!a->x || !a->out || !a->w1 || !a->w2 || a->rows <= 0) return MRAG_EINVAL;
  if (((uintptr_t)a->x | (uintptr_t)a->out | (uintptr_t)a->w1 | (uintptr_t)a->w2) & 15) return MRAG_EINVAL;
  if (((uintptr_t)a->ln_gamma | (uintptr_t)a->ln_beta | (uintptr_t)a->b1 | (uintptr_t)a->b2) & 15) return MRAG_EINVAL;   // (null passes)
  if (a->ldx < FF_C || a->ldo < FF_C || a->ldx % 8 != 0 || a->ldo % 8 != 0) return MRAG_EINVAL;
  if (a->rows > (1ll << 36) || a->ldx > (1ll << 24) || a->ldo > (1ll << 24)) return MRAG_ENOTSUP;                        // (byte extents and the grid stay in range)
  const uintptr_t x0 = (uintptr_t)a->x, x1 = x0 + (uintptr_t)(((a->rows - 1) * a->ldx + FF_C) * 2);
  const uintptr_t o0 = (uintptr_t)a->out, o1 = o0 + (uintptr_t)(((a->rows - 1) * a->ldo + FF_C) * 2);
  if (o0 < x1 && x0 < o1) return MRAG_EINVAL;                  // a workgroup reads its rows of x for the whole product: out must not overlap x
  const long long blocks = (a->rows + FF_ROWS - 1) / FF_ROWS;
  if (blocks > 0x7fffffffll) return MRAG_ENOTSUP;
  FfP p{};
  p.x = (const bf16_t*)a->x; p.gamma = (const bf16_t*)a->ln_gamma; p.beta = (const bf16_t*)a->ln_beta;
  p.w1 = (const bf16_t*)a->w1; p.b1 = (const bf16_t*)a->b1; p.w2 = (const bf16_t*)a->w2; p.b2 = (const bf16_t*)a->b2; p.out = (bf16_t*)a->out;
  p.rows = a->rows; p.inner = a->inner; p.ldx = a->ldx; p.ldo = a->ldo; p.eps = a->eps;
  const int rc = launch_dyn_lds(ff_fused_kernel, dim3((unsigned)blocks), dim3(256), (size_t)(2 * FF_STAGE), (hipStream_t)stream, p);
  if (rc != MRAG_OK) return rc;
  (void)__atomic_fetch_add(&g_ff_fused_launches[0], 1ull, __ATOMIC_RELAXED);
  return MRAG_OK;
}
