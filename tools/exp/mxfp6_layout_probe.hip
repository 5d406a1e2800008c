// mxfp6_layout_probe.hip -- developer probe: which (lane, 6-bit field) of the six A / B operand registers of v_mfma_scale_f32_32x32x64_f8f6f4 with
// cbsz:2 blgp:2 (OCP e2m3 on both sides) holds which (row, k) element, how a field's six bits decode, and which k's a lane's scale byte covers.  The
// guide gives the bf16 maps only and says to check other dtypes with exact data.  Method of fp8_layout_probe.hip: A = one-hot at (lane L, field j),
// B = bit p of the B position's index as 0.0 / 1.0; D over all p spells, per column, the index of the B position that multiplies A's one-hot element.
// Hypothesis under test: field j of a lane is bits 6 j .. 6 j + 5 of the lane's 192-bit operand (register 0 lowest), code = sign | exp(2) | mant(3).
//   hipcc --offload-arch=gfx950 -O2 tools/exp/mxfp6_layout_probe.hip -o tools/exp/mxfp6_layout_probe && tools/exp/mxfp6_layout_probe
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr unsigned ONE = 0x08;   // 1.0 in OCP e2m3 (bias 1: exponent field 1, mantissa 0)

__device__ __host__ inline void set_field(unsigned (&w)[8], int j, unsigned code) {
  const int bit = 6 * j, r = bit >> 5, s = bit & 31;
  w[r] |= code << s;
  if (s > 26) w[r + 1] |= code >> (32 - s);
}

__device__ inline f32x16 mfma6(const unsigned (&a)[8], const unsigned (&b)[8], int sa, int sb) {
  f32x16 c = {0};
  const i32x8 av = {(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], 0, 0};
  const i32x8 bv = {(int)b[0], (int)b[1], (int)b[2], (int)b[3], (int)b[4], (int)b[5], 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c, 2, 2, 0, sa, 0, sb);
}

// one block per A position (lane aL, field aj): out_row = the D row that sees it, out_bpos[col] = index (lane * 32 + field) of the B position it meets
__global__ void probe(int* out_row, int* out_bpos, float* out_val) {
  constexpr int BITS = 11;                         // 64 lanes * 32 fields
  const int lane = threadIdx.x, apos = blockIdx.x, aL = apos / 32, aj = apos % 32;
  unsigned a[8] = {0};
  if (lane == aL) set_field(a, aj, ONE);
  float dsum[16][BITS + 1];
  for (int p = 0; p <= BITS; ++p) {
    unsigned b[8] = {0};
    for (int j = 0; j < 32; ++j) {
      const int idx = lane * 32 + j;
      if (p == BITS || ((idx >> p) & 1)) set_field(b, j, ONE);
    }
    const f32x16 c = mfma6(a, b, 0x7f7f7f7f, 0x7f7f7f7f);
    for (int r = 0; r < 16; ++r) dsum[r][p] = c[r];
  }
  for (int r = 0; r < 16; ++r) {
    if (dsum[r][BITS] != 0.f) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), col = lane & 31;
      int idx = 0;
      for (int p = 0; p < BITS; ++p) idx |= (dsum[r][p] != 0.f ? 1 : 0) << p;
      out_row[apos] = row;
      out_bpos[apos * 32 + col] = idx;
      if (col == 0) out_val[apos] = dsum[r][BITS];
    }
  }
}

// decode: A = code c (block c of 64) in field 5 of lane 3, B all ones -> D[3][0] = value of the code.  Every lane stores its register (a store under
// `lane == 0` lets the compiler sink the MFMA and the operand set-up under that lane mask)
__global__ void decode_probe(float* out) {
  const int lane = threadIdx.x, code = blockIdx.x;
  unsigned a[8] = {0}, b[8] = {0};
  if (lane == 3) set_field(a, 5, (unsigned)code);
  for (int j = 0; j < 32; ++j) set_field(b, j, ONE);
  const f32x16 c = mfma6(a, b, 0x7f7f7f7f, 0x7f7f7f7f);
  out[code * 64 + lane] = c[3];                    // lane 0: col 0, row 3
}

// scale: all-ones operands; lane L's A scale byte 0 = 128 (2^1) (block L), or its B scale byte (block 64 + L): which D rows / columns double?
__global__ void scale_probe(float* out) {
  const int lane = threadIdx.x, L = blockIdx.x & 63, side = blockIdx.x >> 6;
  unsigned ones[8] = {0};
  for (int j = 0; j < 32; ++j) set_field(ones, j, ONE);
  const int s = (lane == L) ? 0x7f7f7f80 : 0x7f7f7f7f;
  const f32x16 c = mfma6(ones, ones, side ? 0x7f7f7f7f : s, side ? s : 0x7f7f7f7f);
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), col = lane & 31;
    out[(blockIdx.x * 32 + row) * 32 + col] = c[r];
  }
}

int main() {
  const int npos = 64 * 32;
  int *d_row, *d_b;
  float *d_v, *d_dec, *d_sc;
  hipMalloc(&d_row, npos * sizeof(int));
  hipMalloc(&d_b, npos * 32 * sizeof(int));
  hipMalloc(&d_v, npos * sizeof(float));
  hipMalloc(&d_dec, 64 * 64 * sizeof(float));
  hipMalloc(&d_sc, 128 * 32 * 32 * sizeof(float));
  hipMemset(d_row, 0xff, npos * sizeof(int));
  hipMemset(d_b, 0xff, npos * 32 * sizeof(int));
  hipMemset(d_v, 0, npos * sizeof(float));
  hipLaunchKernelGGL(probe, dim3(npos), dim3(64), 0, 0, d_row, d_b, d_v);
  hipLaunchKernelGGL(decode_probe, dim3(64), dim3(64), 0, 0, d_dec);
  hipLaunchKernelGGL(scale_probe, dim3(128), dim3(64), 0, 0, d_sc);
  if (hipDeviceSynchronize() != hipSuccess) { printf("probe failed: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
  std::vector<int> row(npos), bp(npos * 32);
  std::vector<float> val(npos), dec(64 * 64), sc(128 * 32 * 32);
  hipMemcpy(row.data(), d_row, npos * sizeof(int), hipMemcpyDeviceToHost);
  hipMemcpy(bp.data(), d_b, npos * 32 * sizeof(int), hipMemcpyDeviceToHost);
  hipMemcpy(val.data(), d_v, npos * sizeof(float), hipMemcpyDeviceToHost);
  hipMemcpy(dec.data(), d_dec, 64 * 64 * sizeof(float), hipMemcpyDeviceToHost);
  hipMemcpy(sc.data(), d_sc, sc.size() * sizeof(float), hipMemcpyDeviceToHost);

  printf("=== v_mfma_scale_f32_32x32x64_f8f6f4 cbsz:2 blgp:2 (e2m3 x e2m3, scales 2^0): 32 fields of 6 bits per lane\n");
  int bad_row = 0, bad_val = 0, same = 0, tot = 0;
  for (int a = 0; a < npos; ++a) {
    if (row[a] != (a / 32) % 32) ++bad_row;
    if (val[a] != 1.0f) ++bad_val;
    for (int c = 0; c < 32; ++c) {
      const int b = bp[a * 32 + c];
      if (b < 0) continue;
      ++tot;
      if ((b / 32) % 32 == c && (b / 32) / 32 == (a / 32) / 32 && b % 32 == a % 32) ++same;
    }
  }
  printf("row(L, j) == L %% 32 for all A positions: %s (%d mismatches)\n", bad_row ? "NO" : "yes", bad_row);
  printf("one-hot 1.0 x 1.0 gives exactly 1.0 at every A position: %s (%d mismatches)\n", bad_val ? "NO" : "yes", bad_val);
  printf("B position for A(L, j) at column c is (lane c + 32 * (L / 32), field j): %d of %d (want %d)\n", same, tot, npos * 32);
  for (int L : {0, 1, 31, 32, 33, 63}) {
    printf("A lane %2d row %2d | B(lane,field) at col 0 for j=0..31:", L, row[L * 32]);
    for (int j = 0; j < 32; ++j) {
      const int b = bp[(L * 32 + j) * 32];
      printf(" (%d,%d)", b < 0 ? -1 : b / 32, b < 0 ? -1 : b % 32);
    }
    printf("\n");
  }
  // decode against sign | exp(2) | mant(3), bias 1, subnormals at exponent field 0
  int bad_dec = 0;
  for (int c = 0; c < 64; ++c) {
    const int e = (c >> 3) & 3, m = c & 7;
    float want = e ? (1.0f + m / 8.0f) * (float)(1 << (e - 1)) : m / 8.0f;
    if (c & 32) want = -want;
    if (dec[c * 64] != want) ++bad_dec;
  }
  printf("code -> value is sign | exp(2) | mant(3) with bias 1: %s (%d of 64 mismatches)\ncodes 0..63:", bad_dec ? "NO" : "yes", bad_dec);
  for (int c = 0; c < 64; ++c) printf(" %g", dec[c * 64]);
  printf("\n");
  // scale: lane L's byte must double exactly the products of row / column L & 31 over its own 32 k's: D = 64 -> 96 there, 64 elsewhere
  int bad_sc = 0;
  for (int blk = 0; blk < 128; ++blk)
    for (int r = 0; r < 32; ++r)
      for (int c = 0; c < 32; ++c) {
        const int L = blk & 63, side = blk >> 6;
        const bool hit = side ? (c == (L & 31)) : (r == (L & 31));   // D row = A's row, D column = B's row
        if (sc[(blk * 32 + r) * 32 + c] != (hit ? 96.0f : 64.0f)) ++bad_sc;
      }
  printf("a lane's scale byte 0 applies to its own row's 32 k's only (A side: D row L & 31, B side: D column L & 31): %s (%d mismatches)\n", bad_sc ? "NO" : "yes", bad_sc);
  printf("A-scale lane 33 doubled: D[1][0] = %g, D[0][0] = %g; B-scale lane 33 doubled: D[0][1] = %g, D[0][0] = %g\n", sc[(33 * 32 + 1) * 32], sc[(33 * 32) * 32],
         sc[((64 + 33) * 32) * 32 + 1], sc[((64 + 33) * 32) * 32]);
  return 0;
}
