// topk_dense.hip -- the dense fan-out forms of the retrieval (topk_dense_kernel, topk_dense_finish_kernel): see topk.hip
#include "topk_common.h"

namespace {

// ---------------------------------------------------------------------------------------------- fan-out, ONE launch: tables that fit one round of workgroups
// BASELINE config #1's own table (10 000 rows x 256 queries) is ONE row block per workgroup of the streaming form (topk_mfma.hip): every workgroup paid its ~6
// workgroup-synchronous selection rounds on a cold list (half of its time), and the call was three launches (|q|^2 pre-pass, fan-out, merge: 6.5 + 115 + 14 us
// + the gaps between them).  This form drops the in-kernel selection and the extra launches:
//   * the same LDS-DMA / fp32-MFMA stream over ONE row block per workgroup; |q|^2 is accumulated from the query fragments the MFMAs read anyway (the same
//     two half-block chains, added once: bit-identical to topk_qq_kernel), |x|^2 as there;
//   * the workgroup's 128 x QB first scores go through an LDS tile into a DENSE [query][row] matrix in the workspace (512-byte runs per query; rows past the
//     table, excluded rows and NaNs as +inf) -- 10 MB at 10 000 x 256;
//   * every workgroup then arrives at one counter and waits for the others (the plan launches this form only when the whole grid is resident at once --
//     hipOccupancyMaxActiveBlocksPerMultiprocessor x 256 CUs; the wait is BOUNDED: a workgroup that gives up simply leaves), and the workgroups that have
//     seen everybody arrive -- always including the last arriver -- CLAIM queries from a second counter and finish them: thread minima -> the 16th (k-th)
//     smallest minimum bounds the answer -> the few scores under that bound are compacted per wave, sorted and merged -> finish_query (second scoring,
//     filter order, output).  The result is the top-k under the total order (first score, row), i.e. what the streaming form and oracle mode 2 define.
//   * the counters live in words 8..14 of the workspace's first 64 bytes (two sets used alternately: a call's last arriver zeroes the other set).
// agent-coherent accesses of the one-launch form's hand-over data (first scores, group minima): written THROUGH the XCD's L2 (sc1) and read past it, i.e. what an
// agent-scope atomic store / load compiles to, 16 bytes wide.  Nothing of the hand-over is then dirty in an L2, and the arrival needs no release fence: a
// `buffer_wbl2` per workgroup walks the whole L2 (632 workgroups: 57 us of a 130-us call; 158: 11 us) -- a wait for the stores' acknowledgements is enough.
__device__ __forceinline__ void store_agent_x4(float* ptr, const f32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(ptr), "v"(v) : "memory");
}
__device__ __forceinline__ float load_agent(const float* ptr) { return __hip_atomic_load(ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

constexpr int DENSE_SLEEP = 32;     // x 64 cycles between two looks at the `go` word (~1 us)
constexpr int DENSE_BUF = 128;      // per-wave compaction buffer of the finishing phase: < 64 left over + <= 64 new candidates per step
constexpr int DENSE_SCR = ((257 + 4 * DENSE_BUF) * 8 + (2 + 2048 + 2 + 2048) * 4 + 15) / 16 * 16;   // bytes of finishing scratch per 256-thread group: candidates | 2 counters, list of passing groups | the group minima (ld / 32 <= 2 048)

// finish query q from the dense first scores: one 256-thread group (lt = 0..255); scratch `sh` (257 candidates), `bufs` (4 x DENSE_BUF candidates) and
// `ctr` (2 + ld / 32 ints: listed groups, surviving scores, the list).  The 32-row groups' minima bound the answer (the keep-th smallest of the lanes'
// minima: `keep` groups hold a score at or under it, so the keep-th nearest row does too); only the groups whose minimum passes the bound are read at all --
// about `keep` runs of 128 bytes out of the query's 40 KB at 10 000 rows -- and ALL of them at once: the passing groups are listed first, then every thread
// loads its elements of the list (one memory round trip; the first form walked the groups two at a time, a dependent load each: 18 us per query).  The
// scores at or under the bound (about `keep` again) meet in one LDS array and are ordered by counting ranks.
// DEPTH = 16, or 32 for the wide lists with a second scoring (keep = max(16, k) <= 32).  Nothing below is sized by `keep` beyond keep <= 64 (the bound is a
// rank among the 64 lane minima; every merge carries 64 candidates): the compaction array holds CAP scores whatever `keep` is, more than CAP take the
// per-wave path, whose buffer holds < 64 left over + <= 64 new entries per step.
template <int DEPTH = 16>
__device__ __forceinline__ void dense_select(const TopkDP& p, const int q, const bool store, const int lt, Cand* sh, Cand* bufs, int* ctr) {
  constexpr int CAP = 4 * DENSE_BUF;
  const int lane = lt & 63, wave = lt >> 6;
  const int ngrp = p.ld >> 5;
  const float* D = p.dist + (long long)q * p.ld;
  const float* G = p.gmin + (long long)q * ngrp;
  const int keep = topk_keep<DEPTH>(p.mp);
  int* glist = ctr + 2;
  float* gsh = (float*)(glist + 2048 + 2);              // [ngrp]: the query's group minima, loaded ONCE by the 256 threads (two loads in flight each)
  Cand inf; inf.d = INFINITY; inf.r = INT_MAX;
  if (lt < 2) ctr[lt] = 0;
  // (every wave loading all of the minima for itself -- 8 waves x 128 workgroups x 5 uncached loads on 323 KB, i.e. on a handful of memory channels -- made
  // this first access after the wait 5 us)
  for (int g0 = 0; g0 < ngrp; g0 += 512) {
    float gv[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int g = g0 + u * 256 + lt;
      const float* a = G + (g < ngrp ? g : 0);
      asm volatile("global_load_dword %0, %1, off sc1" : "=v"(gv[u]) : "v"(a) : "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(gv[0]), "+v"(gv[1]) :: "memory");
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int g = g0 + u * 256 + lt;
      if (g < ngrp) gsh[g] = gv[u];
    }
  }
  __syncthreads();
  // ---- the bound, by every wave for itself: lane minima over ALL groups (g = lane + 64 i), the keep-th smallest of the 64 by rank counting
  Cand m = inf;
  for (int g = lane; g < ngrp; g += 64) {
    const float v = gsh[g];
    const bool b = v < m.d;
    m.d = b ? v : m.d; m.r = b ? g : m.r;
  }
  float thr;
  {
    const int rank = cand_rank(m, 64);
    const unsigned long long bal = __ballot(rank == keep - 1 && m.d < INFINITY);
    thr = bal ? __shfl(m.d, __builtin_ctzll(bal)) : INFINITY;   // (+inf when fewer than `keep` lanes saw a finite score: every finite score passes then)
  }
  __syncthreads();                                      // (the counters are zero; the rank scratch is free again)
  // ---- the groups with a score at or under the bound, listed (any order: the result is the top of a strict total order)
  for (int g = lane + 64 * wave; g < ngrp; g += 256) {
    const float gm = gsh[g];
    const bool pass = gm < INFINITY && gm <= thr;
    const unsigned long long bal = __ballot(pass);
    if (bal) {
      int pos = 0;
      if (lane == 0) pos = atomicAdd(ctr, __popcll(bal));
      pos = __shfl(pos, 0);
      if (pass) glist[pos + __popcll(bal & ((1ull << lane) - 1ull))] = g;
    }
  }
  __syncthreads();
  const int nel = ctr[0] * 32;
  // ---- their scores: four independent loads per thread and step; the ones at or under the bound are appended to `bufs`
  for (int e0 = 0; e0 < nel; e0 += 1024) {
    Cand c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * 256 + lt;
      const bool in = e < nel;
      c[u].r = in ? glist[e >> 5] * 32 + (e & 31) : INT_MAX;
      const float* a = D + (in ? c[u].r : 0);
      asm volatile("global_load_dword %0, %1, off sc1" : "=v"(c[u].d) : "v"(a) : "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(c[0].d), "+v"(c[1].d), "+v"(c[2].d), "+v"(c[3].d) :: "memory");
#pragma unroll
    for (int u = 0; u < 4; ++u) c[u].d = c[u].r != INT_MAX ? c[u].d : INFINITY;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool pass = c[u].d < INFINITY && c[u].d <= thr;
      const unsigned long long bal = __ballot(pass);
      if (bal) {
        int pos = 0;
        if (lane == 0) pos = atomicAdd(ctr + 1, __popcll(bal));
        pos = __shfl(pos, 0) + __popcll(bal & ((1ull << lane) - 1ull));
        if (pass && pos < CAP) bufs[pos] = c[u];
      }
    }
  }
  __syncthreads();
  const int ns = ctr[1];
  Cand run = inf;
  if (ns <= CAP) {
    if (wave == 0) {
      if (ns <= 64) {                                   // the usual case: one rank count puts them in order
        const Cand c = lane < ns ? bufs[lane] : inf;
        const int rank = cand_rank(c, ns);
        if (lane < ns) sh[rank] = c;
        __builtin_amdgcn_wave_barrier();
        run = lane < ns ? sh[lane] : inf;
      } else {
        for (int b0 = 0; b0 < ns; b0 += 64) {
          const Cand c = b0 + lane < ns ? bufs[b0 + lane] : inf;
          run = wave_merge_top(run, wave_sort(c, lane), lane);
        }
      }
    }
  } else {
    // more scores at or under the bound than the array holds (thousands of equal scores, or a table with fewer than `keep` finite scores per lane): the
    // listed groups are read again, every wave compacts its own share, sorts 64 at a time and merges; the four runs meet in wave 0
    __syncthreads();
    Cand* buf = bufs + wave * DENSE_BUF;
    int cnt = 0;
    for (int e0 = 0; e0 < nel; e0 += 256) {
      const int e = e0 + lt;
      Cand c;
      c.r = e < nel ? glist[e >> 5] * 32 + (e & 31) : INT_MAX;
      c.d = e < nel ? load_agent(D + c.r) : INFINITY;
      const bool pass = c.d < INFINITY && c.d <= thr;
      const unsigned long long bal = __ballot(pass);
      if (pass) buf[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = c;
      cnt += __popcll(bal);
      __builtin_amdgcn_wave_barrier();                  // (one wave, in-order LDS: the reads below see the writes above)
      if (cnt >= 64) {
        cnt -= 64;
        const Cand t = buf[cnt + lane];
        run = wave_merge_top(run, wave_sort(t, lane), lane);
        __builtin_amdgcn_wave_barrier();
      }
    }
    const Cand t = lane < cnt ? buf[lane] : inf;
    run = wave_merge_top(run, wave_sort(t, lane), lane);
    __syncthreads();
    sh[wave * 64 + lane] = run;
    __syncthreads();
    if (wave == 0)
      for (int w = 1; w < 4; ++w) run = wave_merge_top(run, sh[w * 64 + lane], lane);
  }
  finish_query<DEPTH>(p.mp, q, run, sh, lt, store);
}

// QBU = queries a workgroup USES of the 32 TN WN its LDS image holds.  96 of 128 (the eight-wave workgroup whose second query group computes ONE of its two tiles):
// three 32-query tiles per workgroup -- BASELINE config #1's 632 tiles then quantise to 3 per busy CU (237 workgroups) instead of 4 (158), with two waves per SIMD.
template <int METRIC, int TN, int WN, int QBU = 32 * TN * WN, int DEPTH = 16>
__global__ __launch_bounds__(256 * WN, TN * WN == 1 ? 3 : WN == 1 ? 2 : 1) void topk_dense_kernel(const TopkDP p) {   // (waves per SIMD: 3 / 2 / 2 workgroups per CU)
  constexpr int WM = 4, NW = WM * WN, NT = 64 * NW, RB = 32 * WM, QB = 32 * TN * WN, NST = dense_stages(TN * WN);
  static_assert(QBU % 32 == 0 && QBU <= QB && QBU > QB - 32 * TN, "only the last query group may run short");
  constexpr int STAGE = (RB + QB) * 128, NPIECE = (RB + QB) / 8, PPW = NPIECE / NW, NTAB = (RB / 8) / NW;
  constexpr int LD = RB + 4;                           // floats per query of the LDS score tile (16-byte aligned rows, spread over the banks)
  constexpr int NG = NT / 256;                         // 256-thread groups of the finishing phase
  static_assert(NPIECE % NW == 0 && (RB / 8) % NW == 0 && PPW == NTAB + TN, "every wave issues the same number of LDS-DMA pieces per slab (the counted vmcnt wait relies on it)");
  static_assert(NST * STAGE >= QB * LD * 4, "the score tile overlays the drained operand ring");
  constexpr int SCR = DENSE_SCR;
  static_assert(NST * STAGE >= NG * SCR, "the finishing phase's scratch overlays it as well");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xxs = (float*)(smem + NST * STAGE);           // [4][32]: |x|^2 of the wave's 32 rows
  unsigned* flag = (unsigned*)(xxs + 128);
  float* gml = xxs + 132;                              // [QB][4]: the waves' minima per query (16-byte aligned)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & (WM - 1), wn = wave / WM;
  const int r32 = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.y * QBU, part = blockIdx.x;
  const bool all_tiles = QBU == QB || (wn * TN + TN) * 32 <= QBU;   // (wave-uniform) this wave's query group computes all of its TN tiles
  const long long row_begin = (long long)part * RB;
  const long long row_end = row_begin + RB < p.n_rows ? row_begin + RB : p.n_rows;

  int exclv[TN]; bool qok[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int qi = q0 + (wn * TN + j) * 32 + r32;
    qok[j] = qi < p.nq && (wn * TN + j) * 32 < QBU;
    exclv[j] = (p.excl && p.group && qok[j]) ? p.excl[qi] : INT_MIN;
  }
  // ---- the LDS-DMA stream of topk_mfma_kernel over the row block's slabs (same image, same swizzle, same counted wait)
  const int chunk = (lane & 7) ^ ((4 * (wave & 1) + (lane >> 4)) & 7);
  const float* qptr[TN];
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    int qi = q0 + 8 * (wave + NW * i) + (lane >> 3);
    qi = qi < p.nq ? qi : p.nq - 1;
    qptr[i] = p.q + (long long)qi * p.dim;
  }
  const float* aptr[NTAB];
#pragma unroll
  for (int i = 0; i < NTAB; ++i) {
    long long row = row_begin + 8 * (wave + NW * i) + (lane >> 3);
    row = row < p.n_rows ? row : p.n_rows - 1;
    aptr[i] = p.db + row * p.dim;
  }
  int d_s = 0;
  auto issue_piece = [&](auto I, const int stage) {
    constexpr int i = decltype(I)::value;
    const int ds = d_s < p.nslab ? d_s : p.nslab - 1;   // (past the end the last slab is re-read into a stage nobody reads again: every iteration issues PPW pieces)
    const int kk = ds * 32 + chunk * 4;
    const float* src = i < NTAB ? aptr[i < NTAB ? i : 0] : qptr[i < NTAB ? 0 : i - NTAB];
    src = kk < p.dim ? src + kk : g_topk_zero + chunk * 4;
    char* dst = smem + stage * STAGE + ((i < NTAB ? 0 : RB / 8) + wave + NW * (i < NTAB ? i : i - NTAB)) * 1024;
    glds16(src, dst);
  };
  auto issue_phase = [&](auto C, const int stage) {
    constexpr int c = decltype(C)::value;
    static_for<PPW>([&](auto I) __attribute__((always_inline)) {
      if constexpr ((4 * decltype(I)::value) / PPW == c) issue_piece(I, stage);
    });
    if constexpr (c == 3) ++d_s;
  };
  auto issue_all = [&](const int stage) {
    issue_phase(std::integral_constant<int, 0>{}, stage); issue_phase(std::integral_constant<int, 1>{}, stage);
    issue_phase(std::integral_constant<int, 2>{}, stage); issue_phase(std::integral_constant<int, 3>{}, stage);
  };
  f32x16 acc[TN];
  float qq[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    qq[j] = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  }
  float xx = 0.f;
#pragma unroll
  for (int i = 0; i < NST - 1; ++i) issue_all(i);
  int stg = 0;
  for (int it = 0; it < p.nslab; ++it) {
    // (the invariant of topk_mfma_kernel's counted wait holds here as well: no vector-memory op between a stage's DMA pieces and this wait)
#ifdef MRAG_DIAG_VMCNT0
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PPW * (NST - 2)) : "memory");
#endif
    __syncthreads();
    const int nstage = stg == 0 ? NST - 1 : stg - 1;
    const char* st = smem + stg * STAGE;
    stg = stg + 1 == NST ? 0 : stg + 1;
    const char* arow = st + (wm * 32 + r32) * 128;
    const char* qrow = st + (RB + wn * TN * 32 + r32) * 128;
    const int sw = (r32 >> 1) & 7;
    auto slab = [&](auto NTL) __attribute__((always_inline)) {           // NTL = tiles this wave computes (TN, or fewer in a short last query group)
      constexpr int ntl = decltype(NTL)::value;
      static_for<4>([&](auto C) __attribute__((always_inline)) {
        constexpr int c = decltype(C)::value;
        const int off = ((2 * c + h) ^ sw) * 16;
        const f32x4 a4 = *(const f32x4*)(arow + off);
        f32x4 b4[ntl];
#pragma unroll
        for (int j = 0; j < ntl; ++j) b4[j] = *(const f32x4*)(qrow + j * 32 * 128 + off);
        if constexpr (METRIC == 0) {                   // the half-block chains of |x|^2 (this lane's row) and |q|^2 (this lane's query of every tile)
#pragma unroll
          for (int t = 0; t < 4; ++t) xx = __builtin_fmaf(a4[t], a4[t], xx);
#pragma unroll
          for (int j = 0; j < ntl; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) qq[j] = __builtin_fmaf(b4[j][t], b4[j][t], qq[j]);
        }
#pragma unroll
        for (int j = 0; j < ntl; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[0], b4[j][0], acc[j], 0, 0, 0);
        issue_phase(C, nstage);
#pragma unroll
        for (int t = 1; t < 4; ++t)
#pragma unroll
          for (int j = 0; j < ntl; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[t], b4[j][t], acc[j], 0, 0, 0);
      });
    };
    if constexpr (QBU == QB) slab(std::integral_constant<int, TN>{});
    else {
      if (all_tiles) slab(std::integral_constant<int, TN>{});
      else slab(std::integral_constant<int, (QBU / 32) % TN>{});
    }
  }
  (void)all_tiles;
  // ---- first scores of the row block
  if constexpr (METRIC == 0) {
    const float xf = xx + __shfl_xor(xx, 32);          // the two half-row chains, added once (either lane: the same two addends)
    if (h == 0 && wn == 0) xxs[wm * 32 + r32] = xf;
#pragma unroll
    for (int j = 0; j < TN; ++j) qq[j] = qq[j] + __shfl_xor(qq[j], 32);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the ring's last (redundant) slabs have landed: the stages are free for the score tile
  __syncthreads();
  const long long blk_row0 = row_begin + wm * 32;
  int gid[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) gid[reg] = INT_MIN + 1;
  if (p.group) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const long long grow = blk_row0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      gid[reg] = p.group[grow < row_end ? grow : row_end - 1];
    }
  }
  float* tile = (float*)smem;                          // [QB][LD]
  float mn[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) mn[j] = INFINITY;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int qn = (wn * TN + j) * 32 + r32;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int reg = 4 * g4 + e, i = e + 8 * g4 + 4 * h;
        const bool valid = blk_row0 + i < row_end;
        const float xi = METRIC == 0 ? xxs[wm * 32 + i] : 0.f;
        const float dot = acc[j][reg];
        const float d = METRIC == 0 ? __builtin_fmaf(-2.0f, dot, qq[j] + xi) : 1.0f - dot;
        o[e] = (valid && qok[j] && d <= INFINITY && gid[reg] != exclv[j]) ? d : INFINITY;   // (NaN scores drop out: the compare is false)
      }
      *(f32x4*)(tile + qn * LD + wm * 32 + 8 * g4 + 4 * h) = o;
      mn[j] = fminf(fminf(mn[j], fminf(o[0], o[1])), fminf(o[2], o[3]));
    }
    mn[j] = fminf(mn[j], __shfl_xor(mn[j], 32));
    if (h == 0) gml[qn * 4 + wm] = mn[j];
  }
  __syncthreads();
  if (tid < QBU && q0 + tid < p.nq) store_agent_x4(p.gmin + ((long long)(q0 + tid) * (p.ld >> 5) + part * 4), *(const f32x4*)(gml + tid * 4));
  for (int idx = tid; idx < QBU * (RB / 4); idx += NT) {
    const int qn = idx / (RB / 4), c4 = idx % (RB / 4);
    if (q0 + qn < p.nq) store_agent_x4(p.dist + (long long)(q0 + qn) * p.ld + row_begin + c4 * 4, *(const f32x4*)(tile + qn * LD + c4 * 4));
  }
  if (p.total == 0) return;                            // the two-launch form: topk_dense_finish_kernel follows (kernel boundary = the hand-over)
  // ---- arrive; wait (bounded) until the grid has arrived; finish the queries of this workgroup's arrival ticket.
  // Words (the workspace's zeroed first 64 bytes, words 8..14): seq | set 0 {arrivals, go, claims} | set 1 {..}.  A call uses set (seq & 1); its last arriver
  // zeroes the OTHER set, publishes `go` and bumps seq, so nothing is reset behind anybody's back and no exit counter is needed (a third same-address atomic
  // per workgroup).  The waiters poll `go`, not the arrival counter (632 pollers on the word the late arrivers still have to increment cost 55 us).
  //   go = 1: every workgroup is here -> STATIC shares: arrival ticket t finishes queries t, t + total, .. (no claim traffic);
  //   go = 2: somebody gave up waiting (it added 0x10000 to the arrival word before it left, so the last arriver -- whose own increment returns the word --
  //           cannot miss it) -> the workgroups that are here CLAIM queries from the set's third word; the last arriver is always among them.
  //   A workgroup that gives up and learns from its own 0x10000 increment that everybody HAS arrived meanwhile stays: `go` is already on its way.
  // Hand-off: agent-coherent (write-through) stores of the scores -> every wave waits for their acknowledgements -> barrier -> one lane: relaxed agent
  // fetch_add; waiters: relaxed agent loads of `go`, barrier, agent-coherent loads of the scores (store_agent_x4 / load_agent above: no L2-wide fences).
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  unsigned seq = 0, ret = 0;                           // (lane 0's)
  unsigned *set = nullptr, *other = nullptr;
  if (tid == 0) {
    seq = __hip_atomic_load(p.sync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    set = p.sync + 1 + 3 * (seq & 1u);
    other = p.sync + 1 + 3 * ((seq & 1u) ^ 1u);
    ret = __hip_atomic_fetch_add(set, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    flag[1] = ret & 0xffffu;
    const unsigned ticket = ret & 0xffffu;
    unsigned mode = 0;
    if (ticket + 1u == (unsigned)p.total) {
      mode = (ret >> 16) ? 2u : 1u;
      __hip_atomic_store(other + 0, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(other + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(other + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(set + 1, mode, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(p.sync, seq + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      for (int spin = 0; spin < p.spin_limit && !mode; ++spin) {
        __builtin_amdgcn_s_sleep(DENSE_SLEEP);
        mode = __hip_atomic_load(set + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (!mode) {
        const unsigned r2 = __hip_atomic_fetch_add(set, 0x10000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((r2 & 0xffffu) == (unsigned)p.total)
          do {
            __builtin_amdgcn_s_sleep(DENSE_SLEEP);
            mode = __hip_atomic_load(set + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          } while (!mode);
      }
    }
    flag[0] = mode; flag[2] = seq & 1u;
  }
  __syncthreads();
  const unsigned mode = flag[0], ticket = flag[1];
  unsigned* claims = p.sync + 1 + 3 * flag[2] + 2;
  __syncthreads();
  if (mode == 0) return;
  Cand* sh = (Cand*)(smem + (tid >> 8) * SCR);
  Cand* bufs = sh + 257;
  int* glist = (int*)(bufs + 4 * DENSE_BUF);   // (2 counters + the list)
  if (mode == 1) {
    for (long long idx = ticket; idx * NG < p.nq; idx += p.total) {
      const int q = (int)idx * NG + (tid >> 8);
      dense_select<DEPTH>(p, q < p.nq ? q : p.nq - 1, q < p.nq, tid & 255, sh, bufs, glist);
    }
    return;
  }
  for (;;) {
    if (tid == 0) flag[0] = __hip_atomic_fetch_add(claims, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const unsigned claim = flag[0];
    __syncthreads();
    if ((long long)claim * NG >= p.nq) break;
    const int q = (int)claim * NG + (tid >> 8);
    dense_select<DEPTH>(p, q < p.nq ? q : p.nq - 1, q < p.nq, tid & 255, sh, bufs, glist);
  }
}

// the finishing phase as a launch of its own (a workgroup per query): the dense form of tables whose grid is not resident at once
template <int DEPTH>
__global__ __launch_bounds__(256) void topk_dense_finish_kernel(const TopkDP p) {
  __shared__ __attribute__((aligned(16))) char scr[DENSE_SCR];
  Cand* sh = (Cand*)scr;
  Cand* bufs = sh + 257;
  dense_select<DEPTH>(p, blockIdx.x, true, threadIdx.x, sh, bufs, (int*)(bufs + 4 * DENSE_BUF));
}

// compute units of the current device (the grid wait of the one-launch form is taken only when the runtime's occupancy x this count holds the whole grid)
inline int dense_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 1;
    cus = n;
  }
  return cus;
}

// one instantiation: the occupancy query (once per instantiation and process), the launch and, without the grid wait, the finishing launch
template <int M, int T, int W, int U, int DEPTH>
int launch_dense(hipStream_t s, TopkDP d, dim3 grid, size_t lds, bool resident_only) {
  auto kfn = topk_dense_kernel<M, T, W, U, DEPTH>;
  static int occ = -1;
  if (occ < 0) {
    hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    int o = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, (const void*)kfn, 256 * W, lds);
    if (e != hipSuccess) return (int)e;
    occ = o;
  }
  if (d.total && (long long)d.total > (long long)dense_cus() * occ) d.total = 0;   // (fewer resident workgroups than planned: no wait, two launches)
  if (!d.total && resident_only) return MRAG_ENOTSUP;
  MRAG_LAUNCH(kfn, grid, dim3(256 * W), lds, s, d);
  MRAG_LAUNCH_CHECK();
  MRAG_COUNT(MRAG_K_TOPK_DENSE);
  if (d.total == 0) {
    MRAG_LAUNCH(topk_dense_finish_kernel<DEPTH>, dim3(d.nq), dim3(256), 0, s, d);
    MRAG_LAUNCH_CHECK();
    MRAG_COUNT(MRAG_K_TOPK_DENSE_FINISH);
  }
  return MRAG_OK;
}

// the 8 instantiations of depth 16: (tn, wn, queries used) = (1, 1, 32) (2, 1, 64) (2, 2, 128) (2, 2, 96), per metric; depth 32: the same four for "l2" (its
// second scoring is what the depth changes; "dot" selects `k` of up to 64 in the depth-16 code as it stands)
template <int M, int DEPTH>
int launch_dense_tile(hipStream_t s, const TopkDP& d, int tn, int wn, int qbu, dim3 grid, size_t lds, bool resident_only) {
  switch ((tn * 8 + wn) * 256 + qbu) {
    case (1 * 8 + 1) * 256 + 32: return launch_dense<M, 1, 1, 32, DEPTH>(s, d, grid, lds, resident_only);
    case (2 * 8 + 1) * 256 + 64: return launch_dense<M, 2, 1, 64, DEPTH>(s, d, grid, lds, resident_only);
    case (2 * 8 + 2) * 256 + 128: return launch_dense<M, 2, 2, 128, DEPTH>(s, d, grid, lds, resident_only);
    case (2 * 8 + 2) * 256 + 96: return launch_dense<M, 2, 2, 96, DEPTH>(s, d, grid, lds, resident_only);
    default: return MRAG_ENOTSUP;
  }
}

}  // namespace

extern "C" int launch_topk_dense(hipStream_t s, const TopkDP& d, int metric, int tn, int wn, int qbu, int depth, dim3 grid, size_t lds, bool resident_only) {
  if (depth != 16 && depth != 32) return MRAG_ENOTSUP;
  if (metric != 0) return launch_dense_tile<1, 16>(s, d, tn, wn, qbu, grid, lds, resident_only);
  return depth == 32 ? launch_dense_tile<0, 32>(s, d, tn, wn, qbu, grid, lds, resident_only) : launch_dense_tile<0, 16>(s, d, tn, wn, qbu, grid, lds, resident_only);
}
