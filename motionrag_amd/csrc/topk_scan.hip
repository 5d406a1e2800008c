// topk_scan.hip -- the flat scan of the retrieval (topk_scan_kernel, plain and fused) and the merge of partial lists (topk_merge_kernel): see topk.hip
#include "topk_common.h"

namespace {

// Distance of one (query, row) pair = 16 interleaved fp32 fmaf chains + a fixed 4-level pairwise tree (the definition
// oracle/topk_oracle.c mode 0 restates):
//   chain l (0..15) runs over k = 64 j + 4 l + c, j = 0.., c = 0..3, in that order;  d = tree(p[0..15]) with
//   p[l] += p[l ^ 8], then ^4, ^2, ^1 (float addition is commutative, so every lane of the butterfly holds the same bits).
// Mapping: 16 lanes share a row (lane s owns chain s: one 16-byte load per 64-float block -> the 16 lanes read 256
// contiguous bytes), a wavefront streams 4 rows per load instruction straight from HBM into registers (no LDS staging of the
// database), 16 such row-quads make the 64-row batch whose candidates sit one per lane for the bitonic selection.
// The queries (QT per workgroup pass) live in LDS and are read as 16-lane-contiguous ds_read_b128.
template <int METRIC, int QT, int JC, bool FUSED = false, int NQD = 16>
__global__ __launch_bounds__(256, QT == 16 ? 3 : 4) void topk_scan_kernel(const TopkP p) {   // <= 168 / 128 VGPRs: 3-4 waves per SIMD stream
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* qs = (float*)smem;                      // [QT][dimp], dimp = dim rounded up to 64, zero padded
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, s = lane & 15;
  const int q0 = blockIdx.y * QT;
  const int slice = blockIdx.x;
  const int nj = (p.dim + 63) / 64, dimp = nj * 64;

  // QT == 1: qs[k].  Query tiles: query-minor image qs[(block j, lane s)][c][qi] (quad pitch QS = 4 QT + 4 floats, conflict-free for the 16
  // lanes of a row) so one ds_read_b128 returns the SAME feature of 4 queries -> packed fp32 math (v_pk_add_f32 / v_pk_fma_f32) on query pairs
  constexpr int QS = 4 * QT + 4;
  if constexpr (QT == 1) {
    for (int i = tid; i < dimp; i += blockDim.x) qs[i] = (q0 < p.nq && i < p.dim) ? p.q[(long long)q0 * p.dim + i] : 0.f;
  } else {
    for (int i = tid; i < QT * dimp; i += blockDim.x) {
      const int qi = i / dimp, k = i - qi * dimp;
      qs[(k >> 2) * QS + (k & 3) * QT + qi] = (q0 + qi < p.nq && k < p.dim) ? p.q[(long long)(q0 + qi) * p.dim + k] : 0.f;
    }
  }
  __syncthreads();
  int excl[QT];
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) excl[qi] = (p.excl && q0 + qi < p.nq) ? p.excl[q0 + qi] : INT_MIN;
  Cand run[QT];
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) { run[qi].d = INFINITY; run[qi].r = INT_MAX; }

  const long long row_begin = (long long)slice * p.rows_per_slice;
  long long row_end = row_begin + p.rows_per_slice;
  if (row_end > p.n_rows) row_end = p.n_rows;
  const int nchunk = nj / JC;                    // JC divides nj (host picks JC)
  const bool tail = (p.dim & 63) != 0;           // last 64-block is partial: lanes past the row end contribute exact zeros

  // a wave scans NQD row-quads (4 NQD rows) per pass: 64 rows, or 16 for small databases (4x the waves -> 4x the bytes in flight: a 10 k-row
  // scan is latency-bound, 157 waves with 12 KB in flight each reached 0.7 TB/s)
  for (long long r0 = row_begin + wave * (4 * NQD); r0 < row_end; r0 += (blockDim.x >> 6) * (4 * NQD)) {
    // (quad t, chunk ch) stream
    auto load = [&](int t, int ch, f32x4* dst) {
      long long row = r0 + 4 * t + g;
      if (row >= p.n_rows) row = p.n_rows - 1;
      const float* base = p.db + row * p.dim + 4 * s;
#pragma unroll
      for (int jj = 0; jj < JC; ++jj) {
        const int j = ch * JC + jj;
        if (tail && 64 * j + 4 * s >= p.dim) dst[jj] = f32x4{0.f, 0.f, 0.f, 0.f};
        else dst[jj] = __builtin_nontemporal_load((const f32x4*)(base + 64 * j));
      }
    };
    float dist[QT], acc[1] = {0.f};
    f32x2 acc2[QT / 2 > 0 ? QT / 2 : 1];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) dist[qi] = 0.f;
#pragma unroll
    for (int i = 0; i < (QT / 2 > 0 ? QT / 2 : 1); ++i) acc2[i] = f32x2{0.f, 0.f};
    int lt = 0, lch = 0;                          // next (quad, chunk) to request
    auto advance = [&]() { if (++lch == nchunk) { lch = 0; ++lt; } };
    int t = 0, ch = 0;                            // (quad, chunk) being consumed
    auto consume = [&](const f32x4* xb) {
#pragma unroll
      for (int jj = 0; jj < JC; ++jj) {
        const f32x4 x = xb[jj];
        if constexpr (QT == 1) {
          const f32x4 qv = *(const f32x4*)(qs + (ch * JC + jj) * 64 + 4 * s);
          if constexpr (METRIC == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float df = qv[e] - x[e]; acc[0] = __builtin_fmaf(df, df, acc[0]); }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[0] = __builtin_fmaf(qv[e], x[e], acc[0]);
          }
        } else {
          // chain order per query is unchanged (feature c = 0..3 in sequence); two queries share one packed instruction
          const float* qp = qs + ((ch * JC + jj) * 16 + s) * QS;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const f32x2 xc = {x[c], x[c]};
#pragma unroll
            for (int qb = 0; qb < QT / 4; ++qb) {
              const f32x4 qv = *(const f32x4*)(qp + c * QT + qb * 4);
              const f32x2 qlo = {qv[0], qv[1]}, qhi = {qv[2], qv[3]};
              if constexpr (METRIC == 0) {
                const f32x2 dlo = qlo - xc, dhi = qhi - xc;
                acc2[2 * qb] = __builtin_elementwise_fma(dlo, dlo, acc2[2 * qb]);
                acc2[2 * qb + 1] = __builtin_elementwise_fma(dhi, dhi, acc2[2 * qb + 1]);
              } else {
                acc2[2 * qb] = __builtin_elementwise_fma(qlo, xc, acc2[2 * qb]);
                acc2[2 * qb + 1] = __builtin_elementwise_fma(qhi, xc, acc2[2 * qb + 1]);
              }
            }
          }
        }
      }
      if (++ch == nchunk) {                       // row-quad t finished: fixed tree over the 16 chains, lane s keeps quad s
        ch = 0;
#pragma unroll
        for (int qi = 0; qi < QT; ++qi) {
          float v;
          if constexpr (QT == 1) { v = acc[0]; acc[0] = 0.f; }
          else { v = acc2[qi >> 1][qi & 1]; }
          v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
          if (t == s) dist[qi] = v;
        }
        if constexpr (QT > 1) {
#pragma unroll
          for (int i = 0; i < QT / 2; ++i) acc2[i] = f32x2{0.f, 0.f};
        }
        ++t;
      }
    };
    const int nit = NQD * nchunk;
    if constexpr (QT == 1) {
      // single query: latency-bound -> 4-deep register ring, statically indexed (step loop unrolled by 4; nit % 4 == 0)
      constexpr int PF = 4;
      f32x4 ring[PF][JC];
#pragma unroll
      for (int u = 0; u < PF - 1; ++u) {
        if (lt < NQD) { load(lt, lch, ring[u]); advance(); }
      }
      for (int it = 0; it < nit; it += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
          if (lt < NQD) { load(lt, lch, ring[(u + PF - 1) % PF]); advance(); }
          if (it + u < nit) consume(ring[u]);         // nit = NQD * nchunk need not be a multiple of the ring depth
        }
      }
    } else {
      // query tiles: the 4 / 16 chains need the registers and the issue slots -> two steps ahead, rotated by moves
      f32x4 cur[JC], n1[JC], n2[JC];
      load(lt, lch, cur); advance();
      if (lt < NQD) { load(lt, lch, n1); advance(); }
      for (int it = 0; it < nit; ++it) {
        if (lt < NQD) { load(lt, lch, n2); advance(); }
        consume(cur);
#pragma unroll
        for (int jj = 0; jj < JC; ++jj) { cur[jj] = n1[jj]; n1[jj] = n2[jj]; }
      }
    }
    const long long myrow = r0 + 4 * s + g;      // the row whose distance this lane captured
    const bool valid = myrow < row_end && s < NQD;
    const int grp = (valid && p.group) ? p.group[myrow] : INT_MIN + 1;
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
      Cand c;
      const float d = METRIC == 0 ? dist[qi] : 1.0f - dist[qi];
      const bool ok = valid && !(p.group && grp == excl[qi]) && (q0 + qi < p.nq);
      c.d = ok ? d : INFINITY;
      c.r = ok ? (int)myrow : INT_MAX;
      // skip the sort when nothing in this 64-row batch can enter the current top-k
      const Cand kth = cand_shfl(run[qi], p.k - 1);
      if (!__any(cand_less(c, kth))) continue;
      c = wave_sort(c, lane);
      run[qi] = wave_merge_top(run[qi], c, lane);
    }
  }
  if constexpr (FUSED) {
    // the four waves' lists meet in LDS first: ONE list per workgroup leaves (p.wpb = 1), so the last arriver bounds and merges a quarter of the lists
    // (10 000 rows: 157 instead of 628; 10^6 rows: 512 instead of 2 048 -- the merge was half of the 33 us of a 10 000-row search)
    __syncthreads();                                               // the query image is dead: LDS scratch
    Cand* pm = (Cand*)smem;                                        // [QT][3][64]
#pragma unroll
    for (int qi = 0; qi < QT; ++qi)
      if (wave > 0) pm[(qi * 3 + wave - 1) * 64 + lane] = run[qi];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int qi = 0; qi < QT; ++qi) {
#pragma unroll
        for (int w = 0; w < 3; ++w) run[qi] = wave_merge_top(run[qi], pm[(qi * 3 + w) * 64 + lane], lane);
        if (q0 + qi < p.nq) p.ws[((long long)(q0 + qi) * p.slices + slice) * 64 + lane] = run[qi];
      }
    }
  } else {
    // partial result of this wave: [query][part][64]
    const int part = slice * p.wpb + wave, nparts = p.slices * p.wpb;
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
      if (q0 + qi < p.nq) p.ws[((long long)(q0 + qi) * nparts + part) * 64 + lane] = run[qi];
    }
  }
  if constexpr (FUSED) {
    // ONE launch for the latency-bound single-query search: the workgroup that arrives LAST at this query tile's counter merges the lists.
    // Placement-independent hand-off (cdna guide, Guideline 16, counter form): plain stores -> every wave drains -> barrier -> one lane:
    // agent-scope release, asm wait, relaxed agent fetch_add; the last arriver: agent-scope acquire, wait, barrier, plain loads.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* flag = (unsigned*)smem;                              // the query image is dead: LDS scratch for the flag and the merge
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned t = __hip_atomic_fetch_add(p.tickets + blockIdx.y, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned last = t == (unsigned)p.slices - 1;
      if (last) {
        __hip_atomic_store(p.tickets + blockIdx.y, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // zero again for the next call
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      *flag = last;
    }
    __syncthreads();
    const bool last = *flag != 0;
    __syncthreads();
    if (!last) return;
    for (int qi = 0; qi < QT; ++qi)
      if (q0 + qi < p.nq) merge_query<64>(p, q0 + qi, (Cand*)smem);
  }
}

template <int LIST>
__global__ __launch_bounds__(256) void topk_merge_kernel(const TopkP p) {
  __shared__ Cand sh[257];
  merge_query<LIST>(p, blockIdx.x, sh);
}

using TopkKernel = void (*)(TopkP);

// the 12 plain and 16 fused instantiations: (qt, jc) = (1, 1) (1, 4) (4, 1) (4, 2) and, plain only, (16, 1) (16, 2), per metric
template <int M, int Q, int J>
TopkKernel scan_variant(bool fused, bool small) {
  if constexpr (Q <= 4) {
    if (fused) return small ? topk_scan_kernel<M, Q, J, true, 4> : topk_scan_kernel<M, Q, J, true, 16>;
  } else if (fused) return nullptr;
  return topk_scan_kernel<M, Q, J>;
}
template <int M>
TopkKernel scan_kernel(int qt, int jc, bool fused, bool small) {
  switch (qt * 8 + jc) {
    case 1 * 8 + 1: return scan_variant<M, 1, 1>(fused, small);
    case 1 * 8 + 4: return scan_variant<M, 1, 4>(fused, small);
    case 4 * 8 + 1: return scan_variant<M, 4, 1>(fused, small);
    case 4 * 8 + 2: return scan_variant<M, 4, 2>(fused, small);
    case 16 * 8 + 1: return scan_variant<M, 16, 1>(fused, small);
    case 16 * 8 + 2: return scan_variant<M, 16, 2>(fused, small);
    default: return nullptr;
  }
}

}  // namespace

extern "C" int launch_topk_scan(hipStream_t s, const TopkP& p, int qt, int jc, bool fused, bool small, dim3 grid, size_t lds) {
  const TopkKernel kfn = p.metric == 0 ? scan_kernel<0>(qt, jc, fused, small) : scan_kernel<1>(qt, jc, fused, small);
  if (!kfn) return MRAG_ENOTSUP;
  return launch_dyn_lds(kfn, grid, dim3(256), lds, s, p);
}

extern "C" int launch_topk_merge(hipStream_t s, const TopkP& p, int list) {
  if (list != 64 && list != 16 && list != 32) return MRAG_ENOTSUP;
  const TopkKernel kfn = list == 64 ? topk_merge_kernel<64> : list == 32 ? topk_merge_kernel<32> : topk_merge_kernel<16>;
  MRAG_LAUNCH(kfn, dim3(p.nq), dim3(256), 0, s, p);
  return (int)hipGetLastError();
}
