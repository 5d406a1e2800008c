// attn_ip_folded.hip -- the finishing kernel of the folded motion-adapter ("ip") branch of the DiT blocks.
// hidden += scale * softmax(scores / 8) . V_ip with scores = hidden . M^T already produced by the GEMM, M = K_ip . W_q_ip per head
// (see include/mrag_hip.h: mrag_ip_attn_folded_bf16).  One wavefront owns 16 rows x one head at a time: the 32 (25 valid) scores of a
// (row, head) are 64 contiguous bytes = the 16x16x32 B-operand layout (row = lane & 15, 8 keys per lane >> 4) straight from global
// memory, the softmax is 8 registers x 4 lane groups, V^T of the block's heads sits transposed in LDS as the A operand, and
// O^T = V^T . P^T.  HBM-bound (546 MB per launch at the DiT shape: 109 MB of scores, 218 MB of `hidden` in and out), so the layout is chosen for the
// MEMORY side (round 5): the four MFMAs of a head take V^T rows in the PERMUTED feature order
//     d(m, t) = 8 (m >> 2) + 4 (t & 1) + (m & 3) + 32 (t >> 1)          m = A row of MFMA t
// so that lane (row, kq) ends up with features 8 kq .. 8 kq + 7 (MFMAs 0, 1) and 32 + 8 kq .. 32 + 8 kq + 7 (MFMAs 2, 3): `hidden` is read and written
// as TWO 16-byte accesses per lane, each instruction covering 64 contiguous bytes per row, instead of the four 8-byte accesses (32 contiguous bytes per
// row and instruction) the natural order d = 16 t + m gives -- half the vector-memory instructions and twice the bytes per cache-line request.  The V^T
// image is XOR-swizzled by (d >> 3) & 3 on its 16-byte key chunks: the permuted rows of one MFMA then hit 16 distinct bank groups (the plain
// image is 4-way conflicted for either order).
#include "common.h"
#include "../../include/mrag_hip.h"

struct IpFoldP {
  const bf16_t* scores; const bf16_t* v; bf16_t* o;
  long long rows, s_ld, o_ld, v_bs, v_ks, rows_per_batch;
  int H, keys, kv_div, ks;   // ks: elements between the heads' score blocks (32: 64-byte aligned blocks; 26: the packed form of the one-launch score GEMM)
  float qscale, out_scale;
};

constexpr int IPFOLD_HG = 4;   // heads whose V^T image a workgroup keeps in LDS (4 KB each); MI355X, DiT shape: 16 -> 196 us, 8 -> 194, 4 -> 185 (more workgroups in flight)
MRAG_KERNEL_HOST_HIDDEN __global__ __launch_bounds__(256) void ip_attn_folded_kernel(const IpFoldP p) {
  constexpr int HG = IPFOLD_HG;                            // heads per block
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* vt = (bf16_t*)smem;                               // [HG][64 d][4 swizzled chunks of 8 keys]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const int h0 = blockIdx.y * HG, kb = blockIdx.z;          // blockIdx.z = K/V batch (one V^T image per block)
  const int nh = min(HG, p.H - h0);
  for (int i = threadIdx.x; i < HG * 64 * 32 / 8; i += 256) ((u32x4*)vt)[i] = u32x4{0u, 0u, 0u, 0u};   // padding keys / heads
  __syncthreads();
  // Key SLOTS.  The four lanes of a (row, head) read the four ALIGNED 16-byte chunks that cover the head's score block: with the packed blocks (ks = 26: a
  // block starts every 52 bytes) the block begins s = (ks h) mod 8 elements into its first chunk, so key k of head h sits in MFMA slot k + s -- the contraction
  // does not care which slot a key occupies as long as the V^T image uses the same one, and the slots in front of / behind the block (neighbouring heads'
  // scores) are masked.  ks = 32: s = 0, the round-5 layout.  (The first packed form read 16 bytes from 4-byte aligned addresses: + 9 us per launch.)
  for (int i = threadIdx.x; i < p.keys * nh * 8; i += 256) {     // 16-byte chunk (key, head, 8 features) -> 8 transposed LDS elements
    const int c8 = i & 7, hl = (i >> 3) % nh, key = (i >> 3) / nh;
    const int slot = key + ((p.ks * (h0 + hl)) & 7);
    const u32x4 raw = *(const u32x4*)(p.v + (long long)kb * p.v_bs + (long long)key * p.v_ks + (h0 + hl) * 64 + c8 * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int d = c8 * 8 + e;                                  // (d >> 3) & 3 == c8 & 3
      vt[(hl * 64 + d) * 32 + ((((slot >> 3) ^ (c8 & 3)) << 3) | (slot & 7))] = (bf16_t)((e & 1) ? (raw[e >> 1] >> 16) : (raw[e >> 1] & 0xffffu));
    }
  }
  __syncthreads();
  // A-operand addresses of the four MFMAs: V^T row d(r16, t), key chunk kq (swizzled by (d >> 3) & 3 = r16 >> 2)
  const int dbase = 8 * (r16 >> 2) + (r16 & 3), kchunk = (kq ^ (r16 >> 2)) << 3;
  // this K/V batch covers q batches [kb * kv_div, (kb + 1) * kv_div): rows [row_lo, row_hi)
  const long long row_lo = (long long)kb * p.kv_div * p.rows_per_batch, row_hi = row_lo + (long long)p.kv_div * p.rows_per_batch;
  for (long long g0 = row_lo + ((long long)blockIdx.x * 4 + wave) * 16; g0 < row_hi; g0 += (long long)gridDim.x * 64) {
    const long long row = g0 + r16;
    const long long rc = row < row_hi ? row : row_hi - 1;
    // the row's scores and current values of the NEXT head are requested while this head is processed (latency-bound kernel)
    u32x4 raw_n = *(const u32x4*)(p.scores + rc * p.s_ld + ((h0 * p.ks) & ~7) + kq * 8);   // (nontemporal loads of the scores measured no different: profiles/r6_ip_attn_folded_packed_aligned.txt)
    u32x4 old_n[2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) old_n[hf] = *(const u32x4*)(p.o + rc * p.o_ld + h0 * 64 + 32 * hf + 8 * kq);
    for (int hl = 0; hl < nh; ++hl) {
      const int h = h0 + hl;
      const u32x4 raw = raw_n;
      bf16_t* op = p.o + rc * p.o_ld + h * 64;
      const u32x4 old[2] = {old_n[0], old_n[1]};
      if (hl + 1 < nh) {
        raw_n = *(const u32x4*)(p.scores + rc * p.s_ld + (((h + 1) * p.ks) & ~7) + kq * 8);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) old_n[hf] = *(const u32x4*)(op + 64 + 32 * hf + 8 * kq);
      }
      float sv[8], m = -INFINITY;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sv[2 * e] = __uint_as_float(raw[e] << 16) * p.qscale;
        sv[2 * e + 1] = __uint_as_float(raw[e] & 0xffff0000u) * p.qscale;
      }
      const int shift = (p.ks * h) & 7;                           // slot of key 0 (wave-uniform)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if ((unsigned)(kq * 8 + e - shift) >= (unsigned)p.keys) sv[e] = -INFINITY;
        m = fmaxf(m, sv[e]);
      }
      m = fmaxf(m, __shfl_xor(m, 16));
      m = fmaxf(m, __shfl_xor(m, 32));
      float l = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) { sv[e] = __builtin_amdgcn_exp2f(sv[e] - m); l += sv[e]; }
      l += __shfl_xor(l, 16);
      l += __shfl_xor(l, 32);
      const u32x4 pw = {pack_bf2(sv[0], sv[1]), pack_bf2(sv[2], sv[3]), pack_bf2(sv[4], sv[5]), pack_bf2(sv[6], sv[7])};
      const bf16x8 pb = __builtin_bit_cast(bf16x8, pw);
      const float inv = p.out_scale / l;
      const bf16_t* vh = vt + hl * 64 * 32 + kchunk;
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {                            // features 32 hf + 8 kq .. + 7 of this lane's row
        u32x4 nw;
#pragma unroll
        for (int q = 0; q < 2; ++q) {                             // MFMA t = 2 hf + q: features 32 hf + 8 kq + 4 q .. + 3
          const bf16x8 va = *(const bf16x8*)(vh + (dbase + 4 * q + 32 * hf) * 32);
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb, acc, 0, 0, 0);     // acc[i] = out[row = r16][d = 32 hf + 8 kq + 4 q + i]
          const unsigned o0 = old[hf][2 * q], o1 = old[hf][2 * q + 1];
          nw[2 * q] = pack_bf2(__uint_as_float(o0 << 16) + acc[0] * inv, __uint_as_float(o0 & 0xffff0000u) + acc[1] * inv);
          nw[2 * q + 1] = pack_bf2(__uint_as_float(o1 << 16) + acc[2] * inv, __uint_as_float(o1 & 0xffff0000u) + acc[3] * inv);
        }
        if (row < row_hi) *(u32x4*)(op + 32 * hf + 8 * kq) = nw;
      }
    }
  }
}

extern "C" int mrag_ip_attn_folded_bf16(void* stream, const void* scores, const void* v, void* hidden, int32_t B, int64_t S, int32_t H, int32_t keys,
                                        int32_t kv_batch_div, int64_t scores_ld, int64_t hidden_ld, int64_t v_batch_stride, int64_t v_key_stride,
                                        float scale, float out_scale, int32_t key_stride) {
  if (!scores || !v || !hidden || B <= 0 || S <= 0 || H <= 0 || keys <= 0 || keys > 32 || kv_batch_div <= 0 || B % kv_batch_div) return MRAG_EINVAL;
  const int ks = key_stride == 0 ? 32 : key_stride;
  if (ks < keys || ks > 32) return MRAG_EINVAL;
  for (int h = 0; h < H && h < 8; ++h)                                            // a block's keys must fit the 32 slots of the aligned chunks that cover it ((ks h) mod 8 repeats with period <= 8)
    if (((ks * h) & 7) + keys > 32) return MRAG_EINVAL;
  if (scores_ld % 8 || hidden_ld % 8 || scores_ld < (((int64_t)(H - 1) * ks) & ~7LL) + 32 || hidden_ld < (int64_t)H * 64) return MRAG_EINVAL;   // a lane group reads the 32 elements from the aligned chunk that holds a block's start
  if (((uintptr_t)scores & 15) || ((uintptr_t)hidden & 15) || ((uintptr_t)v & 15) || v_batch_stride % 8 || v_key_stride % 8) return MRAG_EINVAL;
  IpFoldP p{};
  p.scores = (const bf16_t*)scores; p.v = (const bf16_t*)v; p.o = (bf16_t*)hidden;
  p.rows = (long long)B * S; p.s_ld = scores_ld; p.o_ld = hidden_ld; p.v_bs = v_batch_stride; p.v_ks = v_key_stride; p.rows_per_batch = S;
  p.H = H; p.keys = keys; p.kv_div = kv_batch_div; p.ks = ks; p.qscale = scale * 1.4426950408889634f; p.out_scale = out_scale;
  constexpr int HG = IPFOLD_HG;
  const size_t lds = HG * 64 * 32 * sizeof(bf16_t);
  const long long groups = ((long long)kv_batch_div * S + 63) / 64;
  // ONE round of resident workgroups (each pays a V^T fill and then walks its share of the rows): the count the RUNTIME reports for this kernel's registers
  // and LDS.  Until round 6 the grid assumed eight workgroups per CU from the LDS size alone; the kernel's 72 VGPRs allow seven -- 2 040 workgroups on 1 792
  // slots, i.e. a second round for an eighth of them.
  static int wg_per_cu = 0;                                  // (a property of the code object; the benign race writes the same value)
  if (wg_per_cu == 0) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)ip_attn_folded_kernel, 256, lds) != hipSuccess || n <= 0) n = 4;
    wg_per_cu = n;
  }
  const long long per = (256LL * wg_per_cu) / (((H + HG - 1) / HG) * (long long)(B / kv_batch_div));
  const unsigned gx = (unsigned)(groups < (per > 1 ? per : 1) ? groups : (per > 1 ? per : 1));
  const int rc = launch_dyn_lds(ip_attn_folded_kernel, dim3(gx, (unsigned)((H + HG - 1) / HG), (unsigned)(B / kv_batch_div)), dim3(256), lds, (hipStream_t)stream, p);
  if (rc != MRAG_OK) return rc;
  MRAG_COUNT(MRAG_K_IP_ATTN_FOLDED);
  return MRAG_OK;
}
