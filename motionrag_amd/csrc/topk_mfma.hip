// topk_mfma.hip -- the streaming fan-out form of the retrieval: |q|^2 pre-pass (topk_qq_kernel) and the fp32-MFMA kernel (topk_mfma_kernel): see topk.hip
#include "topk_common.h"

namespace {

// ---------------------------------------------------------------------------------------------- fan-out form: >= 16 queries per call
// The caller that builds the retrieval tables searches in batches (src/data/datamodule.py:231-236 issues one query per annotation; attach_ref_videos
// batches 256): the scan kernel (topk_scan.hip) re-streams the database once per 16 queries and spends its time in fp32 vector FMAs (N = 10 k, Q = 256: 16 passes,
// 246 us).  Here the batch is an fp32 MATRIX product on v_mfma_f32_32x32x2_f32 -- 64 FLOP per cycle and SIMD, the vector unit's peak rate with one VGPR per
// operand and the VALU left free -- and the database is streamed ONCE per 256 queries.  The instruction's result is bit for bit a k-ordered fmaf chain
// (MI355X guide, "FP32-input MFMA"), so the distances are DEFINED: one chain per (query, row) in the feature order 8c, 8c+4, 8c+1, 8c+5, ... (an MFMA takes
// feature k from lanes 0-31 and k' from lanes 32-63; a lane's four MFMAs of a 32-byte block use the four floats of ONE ds_read_b128), squared norms as two
// chains (oracle/topk_oracle.c mode 2 restates it; bit-exact tests).  L2 goes through |q|^2 + |x|^2 - 2 q.x.
//   * workgroup = 4 waves x 32 database rows, every wave against the workgroup's 32 TN queries (TN = 8 / 4 / 2 / 1 tiles of 32: the plan takes the largest
//     TN that still gives the chip >= 256 workgroups, so a 10 k-row table is cut along the QUERIES as well -- grid.y -- instead of leaving CUs idle);
//   * both operands ride the LDS: 32-feature slabs (128-byte rows, 16-byte chunks XOR-swizzled by row & 7 on the DMA's source side) in a ring of NST stages
//     (2 at TN = 8, where a slab is 8 192 MFMA cycles per wave; 3-4 at the narrow tiles, whose 1-2 k cycles per slab are shorter than one DMA round trip):
//     the LDS-DMA of slab i + NST - 1 is issued under the MFMAs of slab i behind a COUNTED vmcnt wait; the stream runs across the row blocks of a workgroup;
//   * accumulator layout: lane (n = lane & 31, h = lane >> 5) holds query n of a 32-query tile against rows (reg & 3) + 8 (reg >> 2) + 4 h: after a row block a
//     lane tests its 16 rows against ITS query's current k-th distance (a register).  Survivors are rare once the lists are warm; they go, one per lane and
//     round, through per-query slots to the query's OWNER thread, which inserts them into the workgroup's sorted top-LIST list in LDS and republishes the
//     threshold -- best candidates first, so the thresholds of a cold list converge in about k rounds;
//   * per-workgroup lists [query][part][LIST] leave through the workspace and the merge kernel (the same LIST) finishes, filter order included;
//   * LIST = 16 (k <= 16) or 32 (the wide lists, 17 <= k <= 32: twice the owner's insertion chain and list registers; at most 128 queries per workgroup,
//     since 256 lists of 33 + 9 entries beside the two-stage ring exceed the CU's 160 KB, and four waves, since the eight-wave tile's 256 registers per lane
//     do not hold the 32-deep chain: it spilled to scratch inside the selection).

// per call: the shared thresholds start at +inf; |q|^2 of every query in the fan-out kernel's order (chains over features
// 8c + t and 8c + 4 + t, added once) when the metric needs it.  One wave per query: the row comes into LDS with coalesced 16-byte loads, then lane 0 runs the
// `lo` chain and lane 1 the `hi` chain over ds_read_b128 quads -- the chains are sequential by definition (dim / 2 dependent FMAs each), the loads need not be
// (a thread per query, the first form, took 91 us at 256 queries x 768: a serial walk over a 3 KB-strided row)
__global__ __launch_bounds__(64) void topk_qq_kernel(const float* q, float* qq, unsigned* tau_g, int nq, int dim, int want_qq) {
  __shared__ __attribute__((aligned(16))) float row[1024];   // dim <= 1024 (mrag_topk_f32)
  const int i = blockIdx.x, lane = threadIdx.x;
  if (lane == 0) tau_g[i] = 0xff800000u;             // float_key(+inf): no threshold yet
  if (!want_qq) return;
  const float4* src = (const float4*)(q + (long long)i * dim);
  const int nquad = dim >> 2;                        // dim % 4 == 0 (mrag_topk_f32)
  for (int c = lane; c < nquad; c += 64) ((float4*)row)[c] = src[c];
  __syncthreads();
  if (lane < 2) {                                    // lane 0: quads 0, 2, 4, .. (features 8c + t); lane 1: quads 1, 3, 5, .. (8c + 4 + t; none for the last block of an odd quad count)
    float acc = 0.f;
    for (int c = lane; c < nquad; c += 2) {
      const float4 v = ((const float4*)row)[c];
      acc = __builtin_fmaf(v.x, v.x, acc); acc = __builtin_fmaf(v.y, v.y, acc); acc = __builtin_fmaf(v.z, v.z, acc); acc = __builtin_fmaf(v.w, v.w, acc);
    }
    const float other = __shfl_xor(acc, 1);
    if (lane == 0) qq[i] = acc + other;              // lo + hi
  }
}

// WN = 2: eight waves -- four row groups x two query groups of TN tiles each -- so every SIMD holds TWO waves and one's LDS-read / DMA-issue / barrier
// stalls pass under the other's MFMAs (the 256-query workgroup: TN = 4, WN = 2; as four waves of TN = 8 its matrix pipe idled a quarter of the stream)
template <int METRIC, int TN, int WN, int LIST = 16>
__global__ __launch_bounds__(256 * WN) void topk_mfma_kernel(const TopkMP p) {
  static_assert(LIST == 16 || (LIST == 32 && TN <= 4 && WN == 1), "list depth: 16, or 32 on four-wave tiles of at most 128 queries");
  constexpr int WM = 4, NW = WM * WN, NT = 64 * NW, RB = 32 * WM, QB = 32 * TN * WN, NST = mfma_stages(TN * WN);
  constexpr int STAGE = (RB + QB) * 128, NPIECE = (RB + QB) / 8, PPW = NPIECE / NW, NTAB = (RB / 8) / NW, LSTR = LIST + 1, NSLOT = 2 * WM;   // (LSTR odd: the owners' list reads spread over the banks)
  static_assert(NPIECE % NW == 0 && (RB / 8) % NW == 0 && PPW == NTAB + TN, "every wave issues the same number of LDS-DMA pieces per slab (the counted vmcnt wait relies on it)");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Cand* lists = (Cand*)(smem + NST * STAGE);        // [QB][LSTR]: sorted ascending, entries >= k stay +inf
  Cand* slots = lists + QB * LSTR;                  // [QB][NSLOT]: this round's candidate of each (wave, half) for the query
  Cand* taus = slots + QB * NSLOT;                  // [QB]: the query's k-th best so far
  float* xxs = (float*)(taus + QB);                 // [4][32]: |x|^2 of the wave's 32 rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & (WM - 1), wn = wave / WM;
  const int r32 = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.y * QB, part = blockIdx.x;
  const long long row_begin = (long long)part * p.rows_per_part;
  long long row_end = row_begin + p.rows_per_part;
  if (row_end > p.n_rows) row_end = p.n_rows;
  const int nblk = row_end > row_begin ? (int)((row_end - row_begin + RB - 1) / RB) : 0;
  Cand inf; inf.d = INFINITY; inf.r = INT_MAX;
  for (int i = tid; i < QB * LSTR; i += NT) lists[i] = inf;
  for (int i = tid; i < QB; i += NT) taus[i] = inf;

  // per lane: the query of each of its TN tiles
  // (scalars and scalar arrays only below: a private ARRAY OF STRUCTS is not promoted to registers by hipcc -- it lives in scratch, and every scratch access is a
  // vector-memory operation whose s_waitcnt vmcnt(0) also waits for the whole LDS-DMA ring: measured 50 k cycles per selection round)
  float qqv[TN]; int exclv[TN]; bool qok[TN]; float tau_d[TN]; int tau_r[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int qi = q0 + (wn * TN + j) * 32 + r32;
    qok[j] = qi < p.nq;
    qqv[j] = (METRIC == 0 && qok[j]) ? p.qq[qi] : 0.f;
    exclv[j] = (p.excl && p.group && qok[j]) ? p.excl[qi] : INT_MIN;
    tau_d[j] = INFINITY; tau_r[j] = INT_MAX;
  }

  // ---- the LDS-DMA stream: item `it` = (row block, feature slab), stage it % NST.  Per wave and slab: NTAB pieces of table rows + TN pieces of query rows
  // (1 KiB = 8 rows x 128 bytes each).  The row pointers are kept in registers (queries: fixed; table rows: per row block), so a piece costs one 64-bit add;
  // the pieces of slab it + NST - 1 are issued in four portions BETWEEN the MFMA groups of slab it (an LDS-DMA instruction takes ~100 cycles to issue: a
  // burst of 12 in front of the MFMAs idled the matrix pipe for a fifth of a slab).
  // LDS image: 128-byte rows, the 16-byte chunk c of row r stored at chunk c ^ ((r >> 1) & 7).  ds_read_b128 serves a wave in four 16-lane groups
  // ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32: MI355X_MICROARCH.md, LDS) over a 256-byte bank row, i.e. a group's 8 even and 8 odd rows
  // must each hit 8 distinct chunks: (r >> 1) & 7 is distinct over them, r & 7 (the first form) was not -- every fragment read was a 2-way conflict
  // (SQ_LDS_BANK_CONFLICT = 54 % of SQ_LDS_IDX_ACTIVE).  A DMA piece is 8 rows starting at row 8 P, P = wave + NW i: (r >> 1) & 7 = (4 (wave & 1) + (lane >> 4)) & 7.
  const int chunk = (lane & 7) ^ ((4 * (wave & 1) + (lane >> 4)) & 7);   // source chunk of this lane inside its 128-byte slab row
  const float* qptr[TN];
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    int qi = q0 + 8 * (wave + NW * i) + (lane >> 3);
    qi = qi < p.nq ? qi : p.nq - 1;
    qptr[i] = p.q + (long long)qi * p.dim;
  }
  const float* aptr[NTAB];
  int d_blk = 0, d_s = 0;
  auto set_rows = [&](const int blk_) {
#pragma unroll
    for (int i = 0; i < NTAB; ++i) {
      long long row = row_begin + (long long)blk_ * RB + 8 * (wave + NW * i) + (lane >> 3);
      row = row < p.n_rows ? row : p.n_rows - 1;     // (past the table -- also past the END of the stream -- the last row is re-read and never used)
      aptr[i] = p.db + row * p.dim;
    }
  };
  set_rows(0);
  auto issue_piece = [&](auto I, const int stage) {  // piece I (< NTAB: table rows, else query rows) of the cursor's slab
    constexpr int i = decltype(I)::value;
    const int kk = d_s * 32 + chunk * 4;
    const float* src = i < NTAB ? aptr[i < NTAB ? i : 0] : qptr[i < NTAB ? 0 : i - NTAB];
    src = kk < p.dim ? src + kk : g_topk_zero + chunk * 4;
    char* dst = smem + stage * STAGE + ((i < NTAB ? 0 : RB / 8) + wave + NW * (i < NTAB ? i : i - NTAB)) * 1024;
    glds16(src, dst);
  };
  auto advance = [&]() {
    if (++d_s == p.nslab) { d_s = 0; ++d_blk; set_rows(d_blk); }
  };
  auto issue_phase = [&](auto C, const int stage) {  // the pieces of phase C = 0..3 of a slab: piece i belongs to phase (4 i) / PPW
    constexpr int c = decltype(C)::value;
    static_for<PPW>([&](auto I) __attribute__((always_inline)) {
      if constexpr ((4 * decltype(I)::value) / PPW == c) issue_piece(I, stage);
    });
    if constexpr (c == 3) advance();
  };
  auto issue_all = [&](const int stage) {
    issue_phase(std::integral_constant<int, 0>{}, stage); issue_phase(std::integral_constant<int, 1>{}, stage);
    issue_phase(std::integral_constant<int, 2>{}, stage); issue_phase(std::integral_constant<int, 3>{}, stage);
  };

  f32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  float xx = 0.f;
  const int total = nblk * p.nslab;
  __syncthreads();                                   // lists / thresholds initialised
  // prologue: NST - 1 slabs in flight.  Past the end of the stream `issue` keeps requesting (the cursor clamps to the table's last row and re-reads a slab into a
  // stage nobody reads again), so EVERY iteration issues exactly PPW pieces per wave and one counted wait fits all of them
#pragma unroll
  for (int i = 0; i < NST - 1; ++i) issue_all(i);
  int s = 0, blk = 0, stg = 0;
  for (int it = 0; it < total; ++it) {
    // INVARIANT of the counted wait: no vector-memory op may be issued between a stage's DMA pieces and their counted wait.  vmcnt retires in order and counts EVERY
    // vector-memory op of the wave, so the group-id loads, the tau_g atomics and the list stores of the selection all sit BEHIND this wait in program order; a later
    // edit that puts a global access in front of it silently lets the MFMAs read a half-landed stage.  -DMRAG_DIAG_VMCNT0 turns the counted waits into vmcnt(0): the
    // results must not change.
#ifdef MRAG_DIAG_VMCNT0
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PPW * (NST - 2)) : "memory");   // all but the newest NST - 2 slabs have landed: slab `it` is in LDS
#endif
    __syncthreads();                                 // ... for every wave; and every wave is done reading the stage that slab it + NST - 1 overwrites
    const int nstage = stg == 0 ? NST - 1 : stg - 1; // slab it + NST - 1 -> stage (it + NST - 1) % NST
    const char* st = smem + stg * STAGE;
    stg = stg + 1 == NST ? 0 : stg + 1;
    const char* arow = st + (wm * 32 + r32) * 128;
    const char* qrow = st + (RB + wn * TN * 32 + r32) * 128;
    const int sw = (r32 >> 1) & 7;
    static_for<4>([&](auto C) __attribute__((always_inline)) {
      constexpr int c = decltype(C)::value;
      const int off = ((2 * c + h) ^ sw) * 16;
      const f32x4 a4 = *(const f32x4*)(arow + off);
      if constexpr (METRIC == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) xx = __builtin_fmaf(a4[t], a4[t], xx);
      }
      f32x4 b4[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) b4[j] = *(const f32x4*)(qrow + j * 32 * 128 + off);
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[0], b4[j][0], acc[j], 0, 0, 0);
      issue_phase(C, nstage);                          // (behind the first MFMAs of the group: the DMA's issue time passes under the matrix pipe)
#pragma unroll
      for (int t = 1; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[t], b4[j][t], acc[j], 0, 0, 0);
    });
    if (++s < p.nslab) continue;
    // ---- end of a row block: distances, then the selection rounds
    s = 0;
    const long long blk_row0 = row_begin + (long long)blk * RB + wm * 32;
    ++blk;
    if constexpr (METRIC == 0) {
      const float xf = xx + __shfl_xor(xx, 32);      // the two half-row chains, added once (either lane: the same two addends)
      if (h == 0 && wn == 0) xxs[wm * 32 + r32] = xf;   // (the query groups hold the same rows: one writes)
      xx = 0.f;
    }
    __syncthreads();
    int gid[16];                                      // the rows' video ids (prefilter): 16 independent loads, one wait
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) gid[reg] = INT_MIN + 1;
    if (p.group) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const long long grow = blk_row0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        gid[reg] = p.group[grow < row_end ? grow : row_end - 1];
      }
    }
    // the SHARED threshold of each query: the smallest k-th distance any workgroup has published so far.  A row farther than that has k rows in front of it
    // somewhere in the table and cannot be in the answer (equal distances stay: `<=`), so it never becomes a candidate here -- a workgroup sees 1 / parts of
    // the table and its own k-th distance alone admits parts-times more rows (3.5 workgroup-synchronous rounds per row block instead of ~1).  Reading a
    // stale value is harmless (the thresholds only fall).
    float gt[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) gt[j] = qok[j] ? key_float(__hip_atomic_load(p.tau_g + q0 + (wn * TN + j) * 32 + r32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : -INFINITY;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int i = (reg & 3) + 8 * (reg >> 2) + 4 * h;
      const long long grow = blk_row0 + i;
      const bool valid = grow < row_end;
      const float xi = METRIC == 0 ? xxs[wm * 32 + i] : 0.f;
      const int gi = gid[reg];
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const float dot = acc[j][reg];
        const float d = METRIC == 0 ? __builtin_fmaf(-2.0f, dot, qqv[j] + xi) : 1.0f - dot;
        acc[j][reg] = (valid && d <= gt[j] && gi != exclv[j]) ? d : INFINITY;     // (gt = -inf for a query past the batch; NaN distances drop out too)
      }
    }
    float bd[TN];                                     // the lane's best remaining row of each tile (re-scanned only after it was consumed)
    int br[TN];
    auto rescan = [&](auto J) __attribute__((always_inline)) {
      constexpr int j = decltype(J)::value;
      // branch-free (hipcc turned the compare-and-keep form into a chain of exec-masked branches, ~370 instructions per tile): the minimum by v_min, then the
      // LOWEST register that holds it (the lowest row among equal distances)
      float m = acc[j][0];
#pragma unroll
      for (int reg = 1; reg < 16; ++reg) m = fminf(m, acc[j][reg]);
      int r = 0;
#pragma unroll
      for (int reg = 15; reg >= 1; --reg) r = acc[j][reg] == m ? reg : r;
      r = acc[j][0] == m ? 0 : r;
      bd[j] = m; br[j] = r;
    };
    static_for<TN>([&](auto J) __attribute__((always_inline)) { rescan(J); });
    for (;;) {
      bool any = false;
      int bsel[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int brow = bd[j] < INFINITY ? (int)(blk_row0 + (br[j] & 3) + 8 * (br[j] >> 2) + 4 * h) : INT_MAX;
        const bool pass = bd[j] < tau_d[j] || (bd[j] == tau_d[j] && brow < tau_r[j]);
        Cand c;
        c.d = pass ? bd[j] : INFINITY;
        c.r = pass ? brow : INT_MAX;
        slots[((wn * TN + j) * 32 + r32) * NSLOT + wm * 2 + h] = c;
        bsel[j] = pass ? br[j] : -1;
        any |= pass;
      }
      if (!__syncthreads_or(any ? 1 : 0)) break;
      if (tid < QB) {                                 // the owner of query tid: at most NSLOT insertions into its sorted list
        // the list and the round's candidates come into REGISTERS in two bursts of independent LDS reads; every insertion is then a fixed chain of
        // compare / select steps (the list keeps its best LIST: entries k .. LIST - 1 are harmless extras, the threshold is entry k - 1).  A pointer-chasing
        // insertion in LDS cost ~20 k cycles per round -- two dependent LDS accesses per shifted entry -- and the rounds are workgroup-synchronous.
        Cand* Lp = lists + tid * LSTR;
        float Ld[LIST], cd[NSLOT];
        int Lr[LIST], cr[NSLOT];
        bool anyc = false;
#pragma unroll
        for (int si = 0; si < NSLOT; ++si) {
          const Cand c = slots[tid * NSLOT + si];
          cd[si] = c.d; cr[si] = c.r;
          anyc |= c.r != INT_MAX;
        }
        if (anyc) {
#pragma unroll
          for (int e = 0; e < LIST; ++e) { const Cand l = Lp[e]; Ld[e] = l.d; Lr[e] = l.r; }
          auto less = [](float ad, int ar, float bd2, int br2) { return ad < bd2 || (ad == bd2 && ar < br2); };
          // one insertion per loop trip, best candidate first: the trip count is the LARGEST number of candidates any owner of the wave holds this round
          // (1-2 once the lists are warm), not NSLOT -- a wave pays every trip of its busiest lane with all 64 lanes
          for (;;) {
            float md = INFINITY;
            int mr = INT_MAX, ms = -1;
#pragma unroll
            for (int si = 0; si < NSLOT; ++si)
              if (less(cd[si], cr[si], md, mr)) { md = cd[si]; mr = cr[si]; ms = si; }
            if (mr == INT_MAX) break;
#pragma unroll
            for (int si = 0; si < NSLOT; ++si)
              if (si == ms) { cd[si] = INFINITY; cr[si] = INT_MAX; }
#pragma unroll
            for (int e = LIST - 1; e >= 1; --e) {
              const bool before_prev = less(md, mr, Ld[e - 1], Lr[e - 1]), before_this = less(md, mr, Ld[e], Lr[e]);
              Ld[e] = before_prev ? Ld[e - 1] : (before_this ? md : Ld[e]);
              Lr[e] = before_prev ? Lr[e - 1] : (before_this ? mr : Lr[e]);
            }
            const bool b0 = less(md, mr, Ld[0], Lr[0]);
            Ld[0] = b0 ? md : Ld[0];
            Lr[0] = b0 ? mr : Lr[0];
          }
          float thd = Ld[0];
          int thr = Lr[0];
#pragma unroll
          for (int e = 0; e < LIST; ++e) {
            Cand l; l.d = Ld[e]; l.r = Lr[e];
            Lp[e] = l;
            if (e == p.k - 1) { thd = Ld[e]; thr = Lr[e]; }
          }
          Cand th; th.d = thd; th.r = thr;
          taus[tid] = th;
          if (thr != INT_MAX && q0 + tid < p.nq) atomicMin(p.tau_g + q0 + tid, float_key(thd));   // a full list: publish its k-th distance
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const Cand tq = taus[(wn * TN + j) * 32 + r32];
        tau_d[j] = tq.d; tau_r[j] = tq.r;
      }
      static_for<TN>([&](auto J) __attribute__((always_inline)) {
        constexpr int j = decltype(J)::value;
        if (__any(bsel[j] >= 0)) {                    // (wave-uniform: most tiles of most rounds have nothing to consume)
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) acc[j][reg] = reg == bsel[j] ? INFINITY : acc[j][reg];   // consumed
          rescan(J);
        }
      });
    }
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the ring's last NST - 1 (redundant) slabs must have landed before the workgroup gives its LDS back
  __syncthreads();
  if (tid < QB && q0 + tid < p.nq) {
    Cand* out = p.lists + ((long long)(q0 + tid) * p.nparts + part) * LIST;
    const Cand* L = lists + tid * LSTR;
    for (int e = 0; e < LIST; ++e) out[e] = e < p.k ? L[e] : inf;
  }
}

using MfmaKernel = void (*)(TopkMP);

// the 10 instantiations of depth 16: (tiles per query group, query groups) = (1, 1) (2, 1) (4, 1) (4, 2) (2, 2), per metric (256 queries per workgroup: eight
// waves of four tiles); the 6 of depth 32: (1, 1) (2, 1) (4, 1)
template <int M, int LIST>
MfmaKernel mfma_kernel(int tn, int wn) {
  switch (tn * 8 + wn) {
    case 1 * 8 + 1: return topk_mfma_kernel<M, 1, 1, LIST>;
    case 2 * 8 + 1: return topk_mfma_kernel<M, 2, 1, LIST>;
    case 4 * 8 + 1: return topk_mfma_kernel<M, 4, 1, LIST>;
    case 8 * 8 + 2:
      if constexpr (LIST == 16) return topk_mfma_kernel<M, 4, 2, LIST>;
      else return nullptr;
    case 4 * 8 + 2:
      if constexpr (LIST == 16) return topk_mfma_kernel<M, 2, 2, LIST>;
      else return nullptr;
    default: return nullptr;
  }
}

}  // namespace

extern "C" int launch_topk_mfma(hipStream_t s, const TopkMP& m, int metric, int tn, int wn, int list, dim3 grid, size_t lds) {
  if (list != 16 && list != 32) return MRAG_ENOTSUP;
  const MfmaKernel kfn = list == 16 ? (metric == 0 ? mfma_kernel<0, 16>(tn, wn) : mfma_kernel<1, 16>(tn, wn))
                                    : (metric == 0 ? mfma_kernel<0, 32>(tn, wn) : mfma_kernel<1, 32>(tn, wn));
  if (!kfn) return MRAG_ENOTSUP;
  MRAG_LAUNCH(topk_qq_kernel, dim3(m.nq), dim3(64), 0, s, m.q, const_cast<float*>(m.qq), m.tau_g, m.nq, m.dim, metric == 0 ? 1 : 0);
  MRAG_LAUNCH_CHECK();
  return launch_dyn_lds(kfn, grid, dim3(256 * wn), lds, s, m);
}
