// topk_common.h -- what the retrieval units share.  One kernel family per unit, so that a family can be read, edited and rebuilt alone:
//   topk.hip        the entry points, the planners, the choice of form; the gathered re-rank (topk_rerank_kernel)
//   topk_scan.hip   the flat scan, plain and fused, and the merge of partial lists (launch_topk_scan, launch_topk_merge)
//   topk_mfma.hip   the streaming fan-out form: |q|^2 pre-pass + fp32-MFMA kernel (launch_topk_mfma)
//   topk_dense.hip  the dense fan-out forms: one launch with the grid wait, or two launches (launch_topk_dense)
// Here: the candidate type with its order, shuffle, sort and merge helpers, the kernels' parameter blocks, the order-1 distance chain, the tail of every
// merge (finish_query, merge_query), the stage counts that the planners share with the kernels, and the family launchers' declarations.
#pragma once
#include "common.h"
#include "../../include/mrag_hip.h"
#include <limits.h>
#include <type_traits>

namespace {

// compile-time loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>)
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (N > 0) {
    static_for<N - 1>(f);
    f(std::integral_constant<int, N - 1>{});
  }
}

struct Cand { float d; int r; };

__device__ __forceinline__ bool cand_less(const Cand a, const Cand b) { return a.d < b.d || (a.d == b.d && a.r < b.r); }

// rank of this lane's candidate among the candidates of lanes 0 .. n - 1 (n wave-uniform): the number of them that come before it in the strict order
// (distance, row).  Lane j's candidate reaches every lane through v_readlane (an SGPR broadcast) as ONE 64-bit key -- the order-preserving image of the
// distance (float_key below; -0 counted as +0, as cand_less does) over the row -- so a step is two readlanes, one 64-bit compare and an add: n short steps
// without memory.  (A 64-lane bitonic network is 21 dependent shuffle stages; counting over an LDS array exposed one LDS round trip per element.)
__device__ __forceinline__ int cand_rank(const Cand c, const int n) {
  const unsigned u = __float_as_uint(c.d + 0.0f);
  const unsigned long long kc = ((unsigned long long)((u & 0x80000000u) ? ~u : (u | 0x80000000u)) << 32) | (unsigned)c.r;
  const int klo = (int)(unsigned)kc, khi = (int)(unsigned)(kc >> 32);
  int rank = 0;
#pragma unroll 8
  for (int j = 0; j < n; ++j) {
    const unsigned long long ko = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(khi, j) << 32) | (unsigned)__builtin_amdgcn_readlane(klo, j);
    rank += ko < kc ? 1 : 0;
  }
  return rank;
}

__device__ __forceinline__ Cand cand_shfl_xor(const Cand c, int m) {
  Cand o; o.d = __shfl_xor(c.d, m); o.r = __shfl_xor(c.r, m); return o;
}
__device__ __forceinline__ Cand cand_shfl(const Cand c, int src) {
  Cand o; o.d = __shfl(c.d, src); o.r = __shfl(c.r, src); return o;
}

// ascending bitonic sort of one Cand per lane across the 64-lane wavefront
__device__ __forceinline__ Cand wave_sort(Cand c, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const Cand o = cand_shfl_xor(c, j);
      const bool up = (lane & k) == 0 || k == 64;
      const bool lower = (lane & j) == 0;
      const bool take_min = (lower == up);
      const bool o_less = cand_less(o, c);
      if (take_min == o_less) c = o;
    }
  }
  return c;
}

// c is bitonic across the wave -> ascending
__device__ __forceinline__ Cand wave_bitonic_merge(Cand c, int lane) {
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    const Cand o = cand_shfl_xor(c, j);
    const bool lower = (lane & j) == 0;
    const bool o_less = cand_less(o, c);
    if (lower == o_less) c = o;
  }
  return c;
}

// run: sorted ascending top-64; batch: sorted ascending 64 new candidates -> new top-64 of the union
__device__ __forceinline__ Cand wave_merge_top(Cand run, Cand batch, int lane) {
  const Cand rev = cand_shfl(batch, 63 - lane);
  const Cand m = cand_less(rev, run) ? rev : run;  // 64 smallest of the 128, bitonic
  return wave_bitonic_merge(m, lane);
}

// the scan and every merge (topk_scan.hip; finish_query below)
struct TopkP {
  const float* db; const int* group; const float* q; const int* excl;
  Cand* ws; int* out_rows; float* out_dist;
  long long n_rows; int dim, nq, k, metric, slices, rows_per_slice;
  const int* post_group;  // postfilter: group ids consulted AFTER selection (then `group` above is null and the scan excludes nothing)
  unsigned* tickets;    // FUSED: one arrival counter per query tile (zero between calls)
  int wpb;              // waves per workgroup: always 4 (small databases spread by giving each WAVE 16 rows instead of 64: small_db())
  int rescore;          // merge (LIST = 16 / 32, metric l2 of the fan-out form): the nearest candidates (16; max(16, k) at depth 32) are re-scored with the direct sum of (q - x)^2 and re-ranked
};

// candidates the first score selects for query lists of compile-time depth DEPTH (16: k <= 16; 32: the wide lists, 17 <= k <= 32) -- oracle/topk_oracle.c's `keep`
template <int DEPTH>
__device__ __forceinline__ int topk_keep(const TopkP& p) {
  if constexpr (DEPTH > 16) return p.rescore ? (p.k > 16 ? p.k : 16) : p.k;
  else return p.rescore ? 16 : p.k;
}

// the streaming fan-out form (topk_mfma.hip)
struct TopkMP {
  const float* db; const int* group; const float* q; const int* excl; const float* qq;
  unsigned* tau_g;        // [nq] the best k-th distance any workgroup has published for the query, as an order-preserving unsigned key (atomicMin)
  Cand* lists;            // [nq][nparts][LIST]: LIST = the kernel's list depth (16 or 32)
  long long n_rows; int dim, nq, k, nparts, rows_per_part, nslab;
};

// the dense fan-out forms (topk_dense.hip)
struct TopkDP {
  const float* db; const int* group; const float* q; const int* excl;
  float* dist;            // [nq][ld] first scores
  float* gmin;            // [nq][ld / 32]: the smallest first score of every 32-row group (a wave's rows of a workgroup's row block)
  unsigned* sync;         // [7]: seq | {arrivals, go, claims} x 2 (see the kernel's hand-off): zero before the first call on a workspace
  long long n_rows; int dim, nq, nslab, ld, total, spin_limit;
  TopkP mp;               // what finish_query needs (k, rescore, outputs, post-filter ids)
};

// order-preserving map float -> unsigned (a < b  <=>  key(a) < key(b), -0 < +0): the shared thresholds are lowered with atomicMin
__device__ __forceinline__ unsigned float_key(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float key_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// The order-1 distance of ONE (query, row) pair on 16 lanes (the second scoring of finish_query and the gathered re-rank, topk_rerank_kernel): lane s16
// of the 16 runs chain s16 -- features 64 j + 4 s16 + {0, 1, 2, 3} (dim % 4 == 0), j ascending -- and chain16_fold adds the 16 partial sums in the fixed
// butterfly: bit for bit what the scan kernel gives the pair ("dot": the caller takes 1 - the folded chain).  The loads of twelve steps (all of a 768-d row)
// are issued together and the chain then runs over registers: as a plain loop every step waited for its own two loads -- twelve memory round trips per
// candidate, ~10 us of the merge.  (A step past the row loads nothing and adds fmaf(0, 0, acc) = acc: a sum of squares is never -0, and 1 - (+-0) = 1.)
template <int METRIC>
__device__ __forceinline__ float chain16_partial(const float* x, const float* qv, const int dim, const int s16) {
  float acc = 0.f;
  constexpr int UB = 12;
  for (int kb = 4 * s16; kb < dim; kb += 64 * UB) {
    float4 xv[UB], q4[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int k0 = kb + 64 * u;
      const bool in = k0 < dim;
      xv[u] = in ? *(const float4*)(x + k0) : float4{0.f, 0.f, 0.f, 0.f};
      q4[u] = in ? *(const float4*)(qv + k0) : float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      if constexpr (METRIC == 0) {
        float df = q4[u].x - xv[u].x; acc = __builtin_fmaf(df, df, acc);
        df = q4[u].y - xv[u].y; acc = __builtin_fmaf(df, df, acc);
        df = q4[u].z - xv[u].z; acc = __builtin_fmaf(df, df, acc);
        df = q4[u].w - xv[u].w; acc = __builtin_fmaf(df, df, acc);
      } else {
        acc = __builtin_fmaf(q4[u].x, xv[u].x, acc);
        acc = __builtin_fmaf(q4[u].y, xv[u].y, acc);
        acc = __builtin_fmaf(q4[u].z, xv[u].z, acc);
        acc = __builtin_fmaf(q4[u].w, xv[u].w, acc);
      }
    }
  }
  return acc;
}
// p[l] += p[l ^ 8], ^ 4, ^ 2, ^ 1 across the 16 lanes of a pair (every lane ends with the same bits)
__device__ __forceinline__ float chain16_fold(float acc) {
  acc += __shfl_xor(acc, 8); acc += __shfl_xor(acc, 4); acc += __shfl_xor(acc, 2); acc += __shfl_xor(acc, 1);
  return acc;
}

// one workgroup (4 waves) per query: merge the per-wave partial lists (each sorted ascending, 64 entries).
// Phase A bounds the answer: the k-th smallest of the lists' MINIMA is an upper bound of the final k-th distance, so only lists
// whose minimum does not exceed it can contribute (about k of thousands).  Phase B merges just those.  The result is the
// unique top-k under the total order (distance, row), whatever the merge order.
// `sh` = 4 x 64 candidates + 1 of LDS scratch.
// LIST = entries per partial list: 64 (the scan kernel's per-wave lists) or 16 / 32 (the fan-out kernel's per-workgroup lists; lanes >= LIST read +inf)
// the tail of every merge: `run` = the sorted nearest candidates of query q across the lanes of the group's first wave (lt < 64) -> second scoring
// (p.rescore), filter order, output.  lt = thread index inside the 256-thread group that merges this query (the merge kernels: threadIdx.x; the
// one-launch fan-out form runs two groups per 512-thread workgroup), sh = the group's 257-candidate scratch, store = false: a group without a
// query of its own walks through the barriers only.  DEPTH = 16, or 32 for the wide lists (17 <= k <= 32): the second scoring then takes the max(16, k)
// nearest in DEPTH / 16 passes of the group.
template <int DEPTH = 16>
__device__ __forceinline__ void finish_query(const TopkP& p, const int q, Cand run, Cand* sh, const int lt, const bool store) {
  const int lane = lt & 63, wave = lt >> 6;
  Cand inf; inf.d = INFINITY; inf.r = INT_MAX;
  if (p.rescore) {
    // The fan-out form scores "l2" through |q|^2 + |x|^2 - 2 q.x: good for SELECTING neighbours, but its absolute error is an ulp of |q|^2 + |x|^2
    // (~1e-4 on unnormalised 768-d embeddings) -- a row's distance to itself came out as 1e-3, near-duplicates as noise or negative, and `_distance`
    // feeds condition_fusion's weights (src/projects/condition/utils.py:7-36).  So the 16 nearest candidates under that score are scored
    // AGAIN here with the scan kernel's definition -- the direct sum of (q - x)^2 on 16 interleaved fmaf chains + the fixed tree, oracle mode 0 -- and
    // re-ranked: the distances a row gets no longer depend on the call shape, and ranks among near neighbours follow the exact form.  16 lanes per
    // candidate, 16 candidates per pass of the group.  (DEPTH = 32: the first keep = max(16, k) lanes are the candidates -- a 22nd nearest under the first
    // score must not enter a list of 21 through the second --, two passes.)
    __syncthreads();
    if (wave == 0) {
      if constexpr (DEPTH > 16) sh[lane] = lane < topk_keep<DEPTH>(p) ? run : inf;
      else sh[lane] = run;
    }
    __syncthreads();
    const int s16 = lt & 15;
    Cand cc[DEPTH / 16];
    float acc[DEPTH / 16];
#pragma unroll
    for (int ps = 0; ps < DEPTH / 16; ++ps) {
      cc[ps] = sh[16 * ps + (lt >> 4)];                     // (256 threads: 16 candidates per pass)
      acc[ps] = 0.f;
      if (cc[ps].r != INT_MAX) acc[ps] = chain16_partial<0>(p.db + (long long)cc[ps].r * p.dim, p.q + (long long)q * p.dim, p.dim, s16);
      acc[ps] = chain16_fold(acc[ps]);
    }
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < DEPTH / 16; ++ps)
      if (s16 == 0 && cc[ps].r != INT_MAX) sh[16 * ps + (lt >> 4)].d = acc[ps];
    __syncthreads();
    if (wave == 0) {                                        // re-rank the (up to) DEPTH by counting: sh[0..DEPTH - 1] -> sh[64..64 + DEPTH - 1]
      const Cand c = lane < DEPTH ? sh[lane] : inf;
      const bool have = c.r != INT_MAX;
      const int rank = cand_rank(c, DEPTH);
      if (lane < DEPTH) sh[64 + lane] = inf;
      __builtin_amdgcn_wave_barrier();
      if (have) sh[64 + rank] = c;
      __builtin_amdgcn_wave_barrier();
      run = lane < DEPTH ? sh[64 + lane] : inf;
    }
  }
  if (wave == 0 && store) {
    if (p.post_group) {
      // lancedb's postfilter: the k nearest are final; rows of the excluded group leave the list, the rest keep their order and move up
      const bool ok = lane < p.k && run.r != INT_MAX;
      const bool keep = ok && p.post_group[ok ? run.r : 0] != p.excl[q];
      const unsigned long long m = __ballot(keep);
      const int pos = __popcll(m & ((1ull << lane) - 1ull));
      const int kept = __popcll(m);
      if (keep) {
        p.out_rows[(long long)q * p.k + pos] = run.r;
        p.out_dist[(long long)q * p.k + pos] = run.d;
      }
      if (lane >= kept && lane < p.k) {
        p.out_rows[(long long)q * p.k + lane] = -1;
        p.out_dist[(long long)q * p.k + lane] = INFINITY;
      }
    } else if (lane < p.k) {
      const bool ok = run.r != INT_MAX;
      p.out_rows[(long long)q * p.k + lane] = ok ? run.r : -1;
      p.out_dist[(long long)q * p.k + lane] = run.d;
    }
  }
  __syncthreads();
}

template <int LIST>
__device__ __forceinline__ void merge_query(const TopkP& p, int q, Cand* sh) {
  Cand* thr_s = sh + 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int nparts = p.slices * p.wpb;
  const Cand* lists = p.ws + (long long)q * nparts * LIST;
  Cand inf; inf.d = INFINITY; inf.r = INT_MAX;
  Cand best = inf;
  for (int base = wave * 64; base < nparts; base += nw * 64) {
    const int part = base + lane;
    Cand m = part < nparts ? lists[(long long)part * LIST] : inf;
    m = wave_sort(m, lane);
    best = wave_merge_top(best, m, lane);
  }
  sh[wave * 64 + lane] = best;
  __syncthreads();
  if (wave == 0) {
    for (int w = 1; w < nw; ++w) best = wave_merge_top(best, sh[w * 64 + lane], lane);
    if (lane == topk_keep<(LIST == 32 ? 32 : 16)>(p) - 1) *thr_s = best;   // k-th smallest minimum (the 16th -- max(16, k)-th at LIST = 32 -- when a second scoring follows: it takes that many nearest)
  }
  __syncthreads();
  const Cand thr = *thr_s;
  Cand run = inf;
  for (int base = wave * 64; base < nparts; base += nw * 64) {
    const int part = base + lane;
    const Cand m = part < nparts ? lists[(long long)part * LIST] : inf;
    unsigned long long todo = __ballot(part < nparts && !cand_less(thr, m));   // min <= thr
    while (todo) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      const Cand c = lane < LIST ? lists[(long long)(base + src) * LIST + lane] : inf;
      run = wave_merge_top(run, c, lane);
    }
  }
  __syncthreads();
  sh[wave * 64 + lane] = run;
  __syncthreads();
  if (wave == 0)
    for (int w = 1; w < nw; ++w) run = wave_merge_top(run, sh[w * 64 + lane], lane);
  finish_query<(LIST == 32 ? 32 : 16)>(p, q, run, sh, tid, true);
}

// ---- what the fan-out kernels (topk_mfma.hip, topk_dense.hip) share
__device__ __attribute__((aligned(128))) float g_topk_zero[32];    // source of feature chunks past `dim` (never written)

constexpr int mfma_stages(int TN) { return TN >= 8 ? 2 : TN == 4 ? 3 : TN == 2 ? 4 : 3; }   // TN = 1: three stages keep two workgroups per CU (67 KB each)

constexpr int dense_stages(int tiles) { return tiles == 1 ? 2 : 3; }   // 32 queries per workgroup: two 20-KB stages, THREE workgroups per CU (10 000 x 256: 632 workgroups = 2.47 per CU)

}  // namespace

// The family launchers, one per unit (MRAG_FAMILY_LAUNCHER, common.h).  Each looks its kernel up by the template arguments and returns MRAG_ENOTSUP when
// no instantiation matches, else the status of its launches.
// topk_scan.hip: topk_scan_kernel<metric, qt, jc> (fused: <.., true, small ? 4 : 16>); topk_merge_kernel<list>, list = 64, 16 or 32
MRAG_FAMILY_LAUNCHER launch_topk_scan(hipStream_t s, const TopkP& p, int qt, int jc, bool fused, bool small, dim3 grid, size_t lds);
MRAG_FAMILY_LAUNCHER launch_topk_merge(hipStream_t s, const TopkP& p, int list);
// topk_mfma.hip: topk_qq_kernel, then topk_mfma_kernel<metric, tn / wn, wn, list> (tn = 32-query tiles per workgroup; list = 16, or 32 with tn <= 4 and wn = 1)
MRAG_FAMILY_LAUNCHER launch_topk_mfma(hipStream_t s, const TopkMP& m, int metric, int tn, int wn, int list, dim3 grid, size_t lds);
// topk_dense.hip: topk_dense_kernel<metric, tn, wn, qbu> and, when the grid is not resident at once (or d.total is 0), topk_dense_finish_kernel;
// resident_only: MRAG_ENOTSUP instead of the two-launch form; depth = 16, or 32 for 17 <= k <= 32 (own instantiations where a second scoring follows: "l2")
MRAG_FAMILY_LAUNCHER launch_topk_dense(hipStream_t s, const TopkDP& d, int metric, int tn, int wn, int qbu, int depth, dim3 grid, size_t lds, bool resident_only);
