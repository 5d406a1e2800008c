// topk.hip -- retrieval: flat-scan distance + top-k over the reference-motion database (gfx950).
//
// Stands behind `table.search(vec).limit(k)[.where('video != ...')]` (lancedb 0.14.0, flat scan,
// src/data/rag.py:54; caller src/data/datamodule.py:231-236).  HBM-bound: the [N, D] fp32 database is
// streamed once per tile of 16 queries.
//
//   * 16 lanes share a database row: lane s owns one of 16 interleaved fp32 fmaf chains (16-byte loads, the 16 lanes read
//     256 contiguous bytes), a wavefront streams 4 rows per load instruction from HBM straight into registers with a
//     one-step register prefetch; the 16 partial sums fold through a fixed butterfly -> bit-identical to
//     oracle/topk_oracle.c mode 0 and independent of grid shape;
//   * the query vectors (1, 4 or 16 per workgroup pass) sit in LDS and are read 16-lane-contiguous;
//   * selection: each wavefront keeps, per query, a sorted top-64 spread over its 64 lanes.  A new
//     64-row batch is bitonic-sorted with wave shuffles and merged (elementwise min against the
//     reversed batch, then one bitonic merge); batches that cannot enter the current top-k are
//     skipped with one ballot;
//   * order is (distance asc, row asc) -> deterministic ties; excluded rows (`video != self`)
//     and padding carry distance +inf / row INT_MAX and come out as row -1;
//   * filter order (lancedb's `where(filter, prefilter=...)`): prefilter -> excluded rows never enter the selection (k results whenever k
//     rows pass); postfilter (lancedb 0.14.0's default) -> the k nearest rows are selected WITHOUT the filter, the excluded ones are then
//     dropped from that list and the survivors move up (possibly fewer than k results; the tail is row -1 / +inf).
#include "topk_common.h"

namespace {

constexpr int ROWS = 256;      // rows per workgroup iteration (4 waves x 64 lanes)

// the fan-out plan: queries per workgroup (32 TN), parts (workgroups along the table), rows per part
// `list` = the per-query list depth of the kernels: 16 (k <= 16), or 32 (the wide lists, 17 <= k <= 32).  At depth 32 the 256-query workgroup does not fit the CU's
// 160 KB of LDS (98 304 of ring + 256 x 42 x 8 = 184 320 bytes), so the wide plan's tile stops at TN = 4 (128 queries: 141 312 bytes); per_cu, parts and WN follow
// from the wide LDS size, and the wide workgroup is always four waves: the eight-wave 128-query kernel (2 tiles x 2 query groups, 256 registers per lane) spilled 8 - 12
// registers of the 32-deep insertion chain to scratch and is not built.  Nothing in the plan depends on `list` at depth 16.
struct MfmaPlan { int TN, WN, QB, RB, gy, parts, rows_per_part; size_t lds, bytes; };
inline MfmaPlan plan_mfma(long long n_rows, int nq, int list = 16) {
  MfmaPlan pl;
  const int qtiles = (nq + 31) / 32;
  pl.RB = 128;
  const long long blocks = (n_rows + pl.RB - 1) / pl.RB;
  // Query tile (32 TN queries per workgroup).  A table that fits ONE round of workgroups with one row block each takes the SMALLEST tile that still fits the
  // round (512 workgroups at TN = 1 -- two per CU --, 256 above): every workgroup pays its pipeline fill and the ~6 selection rounds of a cold list once, so
  // more, smaller workgroups finish sooner (4 000 rows x 256 queries: 94 / 111 / 137 / 191 us at TN = 1 / 2 / 4 / 8; 10 000 rows: 166 / 169 / 140 / 190;
  // 20 000 rows: 221 / 225 / 231 / 190; profiles/r5_topk_query_tile_by_table_size.txt).  A larger table streams: the widest tile the batch fills (one pass
  // over the table per 256 queries).
  int widest = 1;
  for (int t = list > 16 ? 4 : 8; t >= 1; t >>= 1)
    if (t <= qtiles) { widest = t; break; }
  pl.TN = widest;
  for (int t = 1; t <= widest; t <<= 1)
    if (blocks * ((qtiles + t - 1) / t) <= (t == 1 ? 512 : 256)) { pl.TN = t; break; }
  pl.QB = 32 * pl.TN;
  pl.lds = (size_t)mfma_stages(pl.TN) * (pl.RB + pl.QB) * 128 + (size_t)pl.QB * (list + 1 + 8 + 1) * sizeof(Cand) + 4 * 32 * sizeof(float);
  pl.gy = (nq + pl.QB - 1) / pl.QB;
  int per_cu = (int)((160 * 1024) / pl.lds);
  per_cu = per_cu < 1 ? 1 : per_cu > 2 ? 2 : per_cu;                  // (160-208 VGPRs at TN <= 2: two workgroups per CU; depth 32: 284 at TN = 1, where a grid of two per CU runs its second half as a second round)
  long long parts = (256LL * per_cu + pl.gy - 1) / pl.gy;
  parts = parts < 1 ? 1 : parts > blocks ? blocks : parts;
  const long long bpp = (blocks + parts - 1) / parts;
  pl.parts = (int)((blocks + bpp - 1) / bpp);
  // waves: the 256-query workgroup is eight waves (two query groups of four tiles); so is the 128-query workgroup of a ONE-row-block plan (two groups of two tiles):
  // its 64 MFMAs per slab and wave were the long pole of a 10 000-row search (42 us on 158 workgroups), and two waves per SIMD halve them
  pl.WN = list > 16 ? 1 : (pl.TN == 8 || (pl.TN == 4 && bpp == 1)) ? 2 : 1;
  pl.rows_per_part = (int)(bpp * pl.RB);
  pl.bytes = 2 * (((size_t)nq * sizeof(float) + 255) / 256 * 256) + (size_t)nq * pl.parts * list * sizeof(Cand);   // |q|^2, shared thresholds, per-workgroup lists
  return pl;
}

inline bool mfma_applies(int nq, int k, int dim) { return nq >= 16 && k <= 16 && dim % 4 == 0; }
// the wide lists (17 <= k <= 32): only for a caller that names the fan-out form (order 2 - 4).  They select other rows than the scan form at the list's edge,
// so `order = 0` never takes them (mfma_auto below)
inline bool mfma_applies_wide(int nq, int k, int dim) { return nq >= 16 && k > 16 && k <= 32 && dim % 4 == 0; }
inline int mfma_list(int k) { return k > 16 ? 32 : 16; }

// the plan of the dense forms: `ok` = the first scores fit the workspace (<= 65 536 rows, <= 64 MB); `resident` = a tile exists whose whole grid is on the chip at
// once -> ONE launch with the grid wait (checked against the runtime's occupancy at launch); otherwise TWO launches: the same kernel without the wait, then
// topk_dense_finish_kernel (a workgroup per query) -- still no pre-pass and no in-kernel selection rounds (20 000 x 256: 200 -> ~100 us).
struct DensePlan { bool ok, resident; int TN, WN, QB, gy, parts, ld; size_t lds, bytes; };   // QB = queries a workgroup covers (96: the eight-wave workgroup of three tiles)
inline size_t dense_lds(int tn, int wn) {
  return (size_t)dense_stages(tn * wn) * (128 + 32 * tn * wn) * 128 + 132 * sizeof(float) + (size_t)32 * tn * wn * 4 * sizeof(float);   // ring | |x|^2, flag | group minima
}
inline DensePlan plan_dense(long long n_rows, int nq, int dim = 768) {
  DensePlan pl{};
  const int qtiles = (nq + 31) / 32;
  const long long blocks = (n_rows + 127) / 128;
  if (blocks > 512 || (long long)nq * blocks * 128 > (16LL << 20)) return pl;          // (<= 64 MB of first scores)
  pl.ok = true; pl.parts = (int)blocks; pl.ld = (int)blocks * 128;
  pl.bytes = (size_t)nq * pl.ld * sizeof(float) + (size_t)nq * (pl.ld / 32) * sizeof(float);     // first scores | group minima (the same for every tile)
  // Tile = the cheapest of (TN, WN) = 128 queries on eight waves, 64 on four / eight, 32 on four under a two-term model measured at 10 000 x 256 x 768
  // (profiles/r6_topk_one_launch.txt): the busiest CU's MFMA time -- workgroups per CU x 32-query tiles per workgroup x 0.49 us per 32-feature slab -- plus the
  // arrivals at the grid wait, which are same-address atomics and serialise at ~0.045 us each (632 workgroups of 32 queries: 35 + 28 us; 158 of 128: 47 + 7).
  // Small tables take the small tiles (4 000 x 256: 256 workgroups of one tile), BASELINE config #1's takes 128 queries per workgroup.  A grid that is not
  // resident at once (two launches, no wait) is priced by its work per CU plus one workgroup's duration (the tail): it takes the small tiles.  The three-tile
  // workgroup (96 of the 128 queries an eight-wave workgroup holds) exists for config #1's size: 632 tiles = 237 x 3 -> 3 per busy CU (75.7 us) instead of 158 x 4 (80.8).
  const int cand[4][3] = {{2, 2, 0}, {2, 2, 3}, {2, 1, 0}, {1, 1, 0}};                           // TN, WN, tiles used (0 = all).  (64 queries on EIGHT waves -- TN 1, WN 2 -- measured 3 % behind four waves and was never the rule's choice: not instantiated)
  double best = 0;
  bool have = false;
  for (int pass = 0; pass < 2 && !have; ++pass)                                        // pass 0: resident grids; pass 1: any
    for (const auto& c : cand) {
      const int held = c[0] * c[1], tiles = c[2] ? c[2] : held, qb = 32 * tiles, gy = (nq + qb - 1) / qb;
      const int cap = held == 1 ? 3 : held == 2 ? 2 : 1;                                // (the kernels' launch bounds: workgroups per CU)
      int per_cu = (int)((160 * 1024) / dense_lds(c[0], c[1]));
      per_cu = per_cu > cap ? cap : per_cu;
      if (qb > 32 * qtiles && qb > 32) continue;                                       // (a tile wider than the batch)
      const long long wgs = blocks * gy;
      const bool res = wgs <= 256LL * per_cu;
      if (pass == 0 && !res) continue;
      const double slab = ((dim + 31) / 32) * 0.49;
      const double t = res ? (double)((wgs + 255) / 256) * tiles * slab + 0.045 * (double)wgs
                           : ((double)wgs * tiles / 256.0 + tiles) * slab;              // (dispatched as CUs free up: the work per CU + one workgroup's duration as the tail)
      if (have && t >= best) continue;
      best = t; have = true;
      pl.resident = res; pl.TN = c[0]; pl.WN = c[1]; pl.QB = qb; pl.gy = gy;
      pl.lds = dense_lds(c[0], c[1]);
    }
  pl.ok = have;
  if (!have) pl.bytes = 0;
  return pl;
}
// `order = 0` (automatic) takes the fan-out form whenever it applies.  Measured on MI355X (tools/topk_sizes.py, k = 12, D = 768; fan-out / scan kernel):
// 1 000 rows x 256 queries 94 / 164 us, 10 000 x 256 140 / 228 us, 10^5 x 256 0.59 / 2.0 ms, 10^6 x 256 3.8 / 17.2 ms; 10 000 x 16 90 / 158 us
// (profiles/r5_topk_fanout_vs_scan_by_size.txt).  (Until the |q|^2 pre-pass became a wave per query -- it took 91 us as a thread per query -- the two forms were
// equal at 10 000 rows and the switch sat at 32 768.)
inline bool mfma_auto(long long n_rows, int nq, int k, int dim) { (void)n_rows; return mfma_applies(nq, k, dim); }

inline int pick_qt(int nq) { return nq >= 9 ? 16 : nq >= 2 ? 4 : 1; }   // queries per workgroup pass

inline bool small_db(long long n_rows, int nq) { return nq <= 4 && n_rows < 256LL * ROWS; }   // < 65 536 rows, <= 4 queries: 16 rows per wave

void plan(long long n_rows, int nq, int* slices, int* rows_per_slice) {
  const int QT = pick_qt(nq);
  const int ntq = (nq + QT - 1) / QT;
  // workgroups along the database.  A single query (QT = 1) streams best with 512: two workgroups per CU, ~2 000 rows each at 10^6 rows, and only
  // 2 048 per-wave lists for the last arriver to merge -- 523 us = 5.88 TB/s at 10^6 rows against 627 us with 2 048 slices, 6.60 against 6.23 TB/s
  // at 4 x 10^6 (256: 4.1 TB/s, 384: 5.2, 768: 5.8; round 4).  Query tiles keep 2 048 (1 024 costs them 15 %).
  const int MAX_SLICES = QT == 1 ? 512 : 2048;
  const int ROWS = small_db(n_rows, nq) ? 64 : 256;     // rows per workgroup pass (4 waves x 16 or 64 rows; 8 rows per wave measured slower:
                                                        // 34.0 vs 27.5 us at 10 k rows -- the 1 256-list merge of the last arriver then dominates)
  long long tiles = (n_rows + ROWS - 1) / ROWS;
  long long s = MAX_SLICES / ntq;
  if (s < 1) s = 1;
  if (s > tiles) s = tiles;
  long long tps = (tiles + s - 1) / s;  // tiles per slice
  s = (tiles + tps - 1) / tps;
  *slices = (int)s;
  *rows_per_slice = (int)(tps * ROWS);
}

}  // namespace

constexpr int64_t kTicketBytes = 64;     // arrival counters of the fused single-launch form (<= 4 queries = 1 query tile ... 4 tiles of QT = 1)

static int64_t topk_workspace_need(int64_t n_rows, int32_t n_queries, int list) {
  if (n_rows <= 0 || n_queries <= 0) return 0;
  int slices, rps;
  plan(n_rows, n_queries, &slices, &rps);
  const int64_t scan = kTicketBytes + (int64_t)n_queries * slices * 4 * 64 * (int64_t)sizeof(Cand);
  const int64_t fan = n_queries >= 16 ? kTicketBytes + (int64_t)plan_mfma(n_rows, n_queries, list).bytes : 0;   // either form fits (the `order` argument picks one)
  const int64_t dense = n_queries >= 16 ? kTicketBytes + (int64_t)plan_dense(n_rows, n_queries).bytes : 0;  // (0 bytes when the one-launch plan does not apply)
  const int64_t m = scan > fan ? scan : fan;
  return m > dense ? m : dense;
}

extern "C" int64_t mrag_topk_workspace_bytes(int64_t n_rows, int32_t n_queries) { return topk_workspace_need(n_rows, n_queries, 16); }

extern "C" int64_t mrag_topk_workspace_bytes_k(int64_t n_rows, int32_t n_queries, int32_t k) {
  const int64_t base = topk_workspace_need(n_rows, n_queries, 16);
  if (k <= 16) return base;
  const int64_t wide = topk_workspace_need(n_rows, n_queries, 32);          // (the wide plan has other tiles and parts: never report less than the plain need)
  return wide > base ? wide : base;
}

extern "C" int mrag_topk_f32(void* stream, const float* db, const int32_t* group, int64_t n_rows, int32_t dim, const float* queries,
                             const int32_t* exclude, int32_t n_queries, int32_t k, int32_t metric, int32_t* out_rows, float* out_dist,
                             void* workspace, int64_t workspace_bytes, int32_t postfilter, int32_t order) {
  if (!db || !queries || !out_rows || !out_dist || !workspace) return MRAG_EINVAL;
  if (n_rows <= 0 || n_rows > INT_MAX - 1 || n_queries <= 0 || dim <= 0) return MRAG_EINVAL;
  if (k <= 0 || k > 64) return MRAG_ENOTSUP;
  if (dim % 4 != 0 || dim > 1024) return MRAG_ENOTSUP;
  if (metric != 0 && metric != 1) return MRAG_EINVAL;
  if (exclude && !group) return MRAG_EINVAL;
  if (((uintptr_t)db | (uintptr_t)queries) & 15) return MRAG_EINVAL;
  // (the need of THIS call: the wide lists' where the caller names the fan-out form at k > 16; the plain need for k <= 16 and for orders 0 / 1, whose callers size by mrag_topk_workspace_bytes)
  const bool wide = order >= 2 && order <= 4 && k > 16 && k <= 32;
  if (workspace_bytes < (wide ? mrag_topk_workspace_bytes_k(n_rows, n_queries, k) : mrag_topk_workspace_bytes(n_rows, n_queries))) return MRAG_EINVAL;
  TopkP p{};
  if (postfilter != 0 && postfilter != 1) return MRAG_EINVAL;
  const bool post = postfilter && exclude;
  p.db = db; p.group = (exclude && !post) ? group : nullptr; p.post_group = post ? group : nullptr; p.q = queries; p.excl = exclude;
  p.tickets = (unsigned*)workspace; p.ws = (Cand*)((char*)workspace + kTicketBytes); p.out_rows = out_rows; p.out_dist = out_dist;
  p.n_rows = n_rows; p.dim = dim; p.nq = n_queries; p.k = k; p.metric = metric;
  plan(n_rows, n_queries, &p.slices, &p.rows_per_slice);
  p.wpb = 4;
  const bool small = small_db(n_rows, n_queries);
  hipStream_t s = (hipStream_t)stream;
  if (order < 0 || order > 4) return MRAG_EINVAL;
  if (order >= 2 && !mfma_applies(n_queries, k, dim) && !mfma_applies_wide(n_queries, k, dim)) return MRAG_ENOTSUP;
  const int list = mfma_list(k);                          // (32 only behind order >= 2: mfma_auto refuses k > 16)
  if (order >= 2 || (order == 0 && mfma_auto(n_rows, n_queries, k, dim))) {
    // ---- the fan-out form in ONE launch: tables whose grid is resident at once (order 3 = never, order 4 = this form without waiting: diagnostics)
    if (order != 3) {
      const DensePlan dp = plan_dense(n_rows, n_queries, dim);
      if (dp.ok) {
        TopkDP d{};
        d.db = db; d.group = p.group; d.q = queries; d.excl = exclude; d.n_rows = n_rows; d.dim = dim; d.nq = n_queries; d.nslab = (dim + 31) / 32;
        d.dist = (float*)((char*)workspace + kTicketBytes); d.sync = (unsigned*)workspace + 8;
        d.gmin = d.dist + (size_t)n_queries * dp.ld;
        d.ld = dp.ld; d.total = dp.resident ? dp.parts * dp.gy : 0;
        d.spin_limit = order == 4 ? 0 : 40000;                // x ~1 us of s_sleep: a workgroup that has not seen the grid arrive by then leaves (the last arriver finishes alone)
        d.mp = p; d.mp.rescore = metric == 0 ? 1 : 0;
        return launch_topk_dense(s, d, metric, dp.TN, dp.WN, dp.QB, list, dim3(dp.parts, dp.gy), dp.lds, order == 4);
      }
      if (order == 4) return MRAG_ENOTSUP;
    }
    // ---- the fan-out form: one fp32 MFMA pass over the table per 256 queries
    const MfmaPlan pl = plan_mfma(n_rows, n_queries, list);
    TopkMP m{};
    m.db = db; m.group = p.group; m.q = queries; m.excl = exclude; m.n_rows = n_rows; m.dim = dim; m.nq = n_queries;
    m.k = metric == 0 && k < 16 ? 16 : k;      // "l2": the second scoring takes the max(16, k) nearest under the first score, so the lists (and their thresholds) are that deep
    m.nparts = pl.parts; m.rows_per_part = pl.rows_per_part; m.nslab = (dim + 31) / 32;
    const size_t qbytes = ((size_t)n_queries * sizeof(float) + 255) / 256 * 256;
    m.qq = (float*)((char*)workspace + kTicketBytes);
    m.tau_g = (unsigned*)((char*)workspace + kTicketBytes + qbytes);
    m.lists = (Cand*)((char*)workspace + kTicketBytes + 2 * qbytes);
    int rc = launch_topk_mfma(s, m, metric, pl.TN, pl.WN, list, dim3(pl.parts, pl.gy), pl.lds);   // (|q|^2 pre-pass, then the fan-out kernel)
    if (rc != MRAG_OK) return rc;
    MRAG_COUNT(MRAG_K_TOPK_MFMA);
    p.ws = m.lists; p.slices = pl.parts; p.wpb = 1; p.rescore = metric == 0 ? 1 : 0;
    rc = launch_topk_merge(s, p, list);
    if (rc != MRAG_OK) return rc;
    MRAG_COUNT(MRAG_K_TOPK_MERGE);
    return MRAG_OK;
  }
  const int QT = pick_qt(n_queries), nj = (dim + 63) / 64;
  // blocks of 64 floats per register-ring step: 4 for the single query, 2 for query tiles (their chains need the registers)
  const int JCsel = QT == 1 ? (nj % 4 == 0 ? 4 : 1) : (nj % 2 == 0 ? 2 : 1);
  size_t lds = (QT == 1 ? (size_t)nj * 64 : (size_t)nj * 16 * (4 * QT + 4)) * sizeof(float);
  const dim3 grid(p.slices, (n_queries + QT - 1) / QT);
  // <= 4 queries (the interactive search of rag.py:63-80): ONE launch, the last workgroup to arrive merges (needs the first 64 workspace
  // bytes ZERO on entry -- see the header; the kernel leaves them zero)
  const bool fused = n_queries <= 4 && ((uintptr_t)workspace & 15) == 0;
  if (small && !fused) return MRAG_EINVAL;                                          // the small-database plan exists only in the fused form
  if (fused) {
    const size_t need = (size_t)(QT * 3 * 64 > 257 ? QT * 3 * 64 : 257) * sizeof(Cand);   // the four-wave pre-merge ([QT][3][64]) / the last arriver's merge scratch
    if (lds < need) lds = need;
    p.wpb = 1;                                                                          // one list per workgroup leaves the fused kernel
  }
  int rc = launch_topk_scan(s, p, QT, JCsel, fused, small, grid, lds);
  if (rc != MRAG_OK) return rc;
  if (fused) {
    MRAG_COUNT(MRAG_K_TOPK_SCAN_FUSED_MERGE);
    return MRAG_OK;
  }
  MRAG_COUNT(MRAG_K_TOPK_SCAN);
  rc = launch_topk_merge(s, p, 64);
  if (rc != MRAG_OK) return rc;
  MRAG_COUNT(MRAG_K_TOPK_MERGE);
  return MRAG_OK;
}

// ---------------------------------------------------------------------------------------------- gathered re-rank: every query scores ITS OWN short list of rows
// Stage 2 of the reference's text-then-image retrieval (src/data/rag.py:101-130: the rows of a text search become a temporary table, in rank order, that an
// image search then ranks; caller src/data/datamodule.py:239-245 with top_k = (2 n + 3, n)).  One 256-thread workgroup per query: 16 lanes per candidate, 16
// candidates per pass (<= 4 passes), distances in the order-1 form (chain16_partial / chain16_fold: the bits the scan kernel gives the pair), parked in LDS;
// the first wave then ranks the <= 64 (distance, POSITION in the list) pairs by counting and writes the first k.  An entry outside [0, n_rows) is absent.
// ~22 MB of rows at 256 x 21 x 1 024 floats: launch- and latency-bound, no pipeline.
namespace {

struct RerankP {
  const float* db; const float* q; const int* cand; int* out_rows; int* out_pos; float* out_dist;
  long long n_rows; int dim, n_cand, k;
};

template <int METRIC>
__global__ __launch_bounds__(256) void topk_rerank_kernel(const RerankP p) {
  __shared__ float sd[64];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int c16 = tid >> 4, s16 = tid & 15;
  const float* qv = p.q + (long long)q * p.dim;
  const int* cr = p.cand + (long long)q * p.n_cand;
  for (int base = 0; base < p.n_cand; base += 16) {
    const int pos = base + c16;
    const int row = pos < p.n_cand ? cr[pos] : -1;
    const bool have = row >= 0 && row < p.n_rows;
    float acc = 0.f;
    if (have) acc = chain16_partial<METRIC>(p.db + (long long)row * p.dim, qv, p.dim, s16);
    acc = chain16_fold(acc);
    if (s16 == 0 && have) sd[pos] = METRIC == 0 ? acc : 1.0f - acc;
  }
  __syncthreads();
  if (tid >= 64) return;
  const int row = lane < p.n_cand ? cr[lane] : -1;
  const bool have = row >= 0 && row < p.n_rows;
  Cand c;
  c.d = have ? sd[lane] : INFINITY;
  c.r = have ? lane : INT_MAX;                               // the tie rule: position in the list, not the row number
  const int rank = cand_rank(c, p.n_cand);                   // distinct positions -> distinct ranks among the present entries
  const int found = __popcll(__ballot(have));
  const long long o = (long long)q * p.k;
  if (have && rank < p.k) {
    p.out_rows[o + rank] = row;
    if (p.out_pos) p.out_pos[o + rank] = lane;
    p.out_dist[o + rank] = c.d;
  }
  if (lane >= found && lane < p.k) {
    p.out_rows[o + lane] = -1;
    if (p.out_pos) p.out_pos[o + lane] = -1;
    p.out_dist[o + lane] = INFINITY;
  }
}

}  // namespace

extern "C" int mrag_topk_rerank_f32(void* stream, const float* db, int64_t n_rows, int32_t dim, const float* queries, int32_t n_queries,
                                    const int32_t* cand_rows, int32_t n_cand, int32_t k, int32_t metric, int32_t* out_rows, int32_t* out_pos,
                                    float* out_dist) {
  if (!db || !queries || !cand_rows || !out_rows || !out_dist) return MRAG_EINVAL;
  if (n_rows <= 0 || n_rows > INT_MAX - 1 || n_queries <= 0 || dim <= 0) return MRAG_EINVAL;
  if (metric != 0 && metric != 1) return MRAG_EINVAL;
  if (k <= 0 || n_cand <= 0 || k > n_cand) return MRAG_EINVAL;
  if (n_cand > 64 || dim % 4 != 0) return MRAG_ENOTSUP;
  if (((uintptr_t)db | (uintptr_t)queries) & 15) return MRAG_EINVAL;
  RerankP p{};
  p.db = db; p.q = queries; p.cand = cand_rows; p.out_rows = out_rows; p.out_pos = out_pos; p.out_dist = out_dist;
  p.n_rows = n_rows; p.dim = dim; p.n_cand = n_cand; p.k = k;
  hipStream_t s = (hipStream_t)stream;
  if (metric == 0) MRAG_LAUNCH(topk_rerank_kernel<0>, dim3(n_queries), dim3(256), 0, s, p);
  else MRAG_LAUNCH(topk_rerank_kernel<1>, dim3(n_queries), dim3(256), 0, s, p);
  MRAG_LAUNCH_CHECK();
  MRAG_COUNT(MRAG_K_TOPK_RERANK);
  return MRAG_OK;
}

