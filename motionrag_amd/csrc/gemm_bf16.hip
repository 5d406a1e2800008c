// gemm_bf16.hip -- C[M,N] = epilogue(A[M,K] . W[N,K]^T + bias), bf16 in, fp32 accumulate: the entry point behind every nn.Linear on the MotionRAG hot path
// (see include/mrag_hip.h).  Dispatch only: which kernel family takes a problem.  The families live one per unit (gemm_common.h lists them).
#include "gemm_common.h"

namespace {

// where the few-row kernel runs: measured against the 128 x 128 tile on MI355X (tools/skinny_sweep.py, profiles/r5_gemm_skinny_sweep.txt)
inline bool skinny_applies(const mrag_gemm_args* a, int epi) {
  // (W is read once per 32-row tile, through L2: past ~134 MB of such reads the tiled kernel's larger tiles win again -- [256 x 10240 x 4096] 115 vs 50 us,
  // [256 x 4096 x 4096] 49 vs 47, [128 x 4096 x 4096] 27 vs 47, [250 x 1024 x 4096] 25 vs 46; a single row tile streams any weight once: the UNets' batched
  // time-embedding projection, 32 x 36 480 x 1 280)
  const long long row_tiles = (a->M + SKM_ROWS - 1) / SKM_ROWS;
  return a->M <= 256 && row_tiles * a->N * a->K <= 8LL * 4096 * 2048 && a->K >= 256 && a->N >= 256 &&
         !(a->tuning & MRAG_GEMM_TUNE_NO_SKINNY) && ((a->tuning >> 4) & 0xf) == 0 &&
         (epi == MRAG_EPI_NONE || epi == MRAG_EPI_GELU_TANH || epi == MRAG_EPI_GELU_ERF || epi == MRAG_EPI_SILU || epi == MRAG_EPI_RESID) &&
         (!a->bias || (((uintptr_t)a->bias) & 7) == 0);
}

inline bool k320_applies(const mrag_gemm_args* a, int epi) {
  // (the GEGLU projection, N = 2 560 = eight slices, is instantiated and bit-equal but NOT dispatched: 758 vs 683 us -- a tile costs ~12 k cycles here whatever
  // the slice count, so eight passes over the activations lose against the persistent four-wave kernel; N = 960 gains 8 %, N = 320 40 %)
  return a->K == 320 && a->N % 320 == 0 && a->N <= 960 && a->M >= 16384 && (epi == MRAG_EPI_NONE || epi == MRAG_EPI_RESID) &&
         !(a->tuning & (MRAG_GEMM_TUNE_NO_WIDE | MRAG_GEMM_TUNE_NO_STAGED | MRAG_GEMM_TUNE_GEGLU_NO_STAGED | MRAG_GEMM_TUNE_STREAMK)) &&
         rows_16B_aligned(a->C, a->ldc, a->resid, a->ldr) && (!a->bias || (((uintptr_t)a->bias) & 7) == 0);
}

}  // namespace

extern "C" int mrag_gemm_bf16(void* stream, const mrag_gemm_args* a) {
  if (!a || !a->A || !a->W || !a->C) return MRAG_EINVAL;
  if (a->M <= 0 || a->N <= 0 || a->K <= 0) return MRAG_EINVAL;
  if (a->K % 64 != 0 || a->N % 4 != 0) return MRAG_ENOTSUP;
  if (a->epilogue == MRAG_EPI_GEGLU && a->N % 32 != 0) return MRAG_ENOTSUP;
  if (a->lda % 8 != 0 || a->ldw % 8 != 0 || a->ldc % 4 != 0) return MRAG_EINVAL;
  if (((uintptr_t)a->A | (uintptr_t)a->W) & 15) return MRAG_EINVAL;
  if ((uintptr_t)a->C & 7) return MRAG_EINVAL;
  if ((a->epilogue == MRAG_EPI_RESID || a->epilogue == MRAG_EPI_GATE_RESID) &&
      (!a->resid || a->ldr % 4 != 0 || ((uintptr_t)a->resid & 7)))
    return MRAG_EINVAL;
  if (a->epilogue == MRAG_EPI_GATE_RESID &&
      (!a->gate0 || !a->gate1 || a->rows_per_batch <= 0 || a->gate_stride % 4 != 0)) return MRAG_EINVAL;
  GemmP p{};
  p.A = (const bf16_t*)a->A; p.W = (const bf16_t*)a->W; p.bias = (const bf16_t*)a->bias;
  p.C = (bf16_t*)a->C; p.resid = (const bf16_t*)a->resid;
  p.gate0 = (const bf16_t*)a->gate0; p.gate1 = (const bf16_t*)a->gate1;
  p.M = a->M; p.N = a->N; p.K = a->K; p.lda = a->lda; p.ldw = a->ldw; p.ldc = a->ldc; p.ldr = a->ldr;
  p.rows_per_batch = a->rows_per_batch; p.split = a->split; p.gate_stride = a->gate_stride;
  p.acc_scale = a->acc_scale == 0.0f ? 1.0f : a->acc_scale;
  if (a->w_batch_stride < 0 || a->w_batch_stride % 8 != 0) return MRAG_EINVAL;
  if (a->a_ln != 0 && a->a_ln != 1) return MRAG_EINVAL;
  if (a->a_ln) {
    if ((((uintptr_t)a->a_ln_gamma | (uintptr_t)a->a_ln_beta) & 15) || a->K > 8192) return MRAG_EINVAL;
    p.lna = 1; p.lna_g = (const bf16_t*)a->a_ln_gamma; p.lna_b = (const bf16_t*)a->a_ln_beta; p.lna_eps = a->a_ln_eps;
  }
  p.w_bstride = a->w_batch_stride;
  if (a->epilogue == MRAG_EPI_GEGLU && a->geglu_act != 0 && a->geglu_act != 1) return MRAG_EINVAL;
  if (a->epilogue == MRAG_EPI_QKNORM_ROPE) {
    if (a->qk_dmodel <= 0 || a->qk_dmodel % 64 != 0 || a->N % a->qk_dmodel != 0 || a->qk_first < 0 || a->qk_first + a->N / a->qk_dmodel > 3 ||
        a->rows_per_batch <= 0) return MRAG_EINVAL;
    if ((a->rope_cos != nullptr) != (a->rope_sin != nullptr) || (((uintptr_t)a->rope_cos | (uintptr_t)a->rope_sin) & 15)) return MRAG_EINVAL;
    if (((uintptr_t)a->q_gamma | (uintptr_t)a->q_beta | (uintptr_t)a->k_gamma | (uintptr_t)a->k_beta) & 15) return MRAG_EINVAL;
    p.qg = (const bf16_t*)a->q_gamma; p.qb = (const bf16_t*)a->q_beta; p.kg = (const bf16_t*)a->k_gamma; p.kb = (const bf16_t*)a->k_beta;
    p.rcos = a->rope_cos; p.rsin = a->rope_sin; p.qk_D = a->qk_dmodel; p.rope_text_len = a->rope_text_len; p.qk_first = a->qk_first; p.qk_eps = a->qk_eps; p.q_premul = a->q_premul;
  }
  hipStream_t s = (hipStream_t)stream;
  // big problems: 256x256 tiles, 8 waves (1 workgroup per CU); small ones: 128x128, 4 waves,
  // so that a few hundred rows still spread over the 256 CUs.
  const long long t256 = ((a->M + 255) / 256) * ((a->N + 255) / 256);
  p.tuning = a->tuning;
  const int epi = (a->epilogue == MRAG_EPI_GEGLU && a->geglu_act == 1) ? EPI_GEGLU_TANH : a->epilogue;   // the tanh gate is its own instantiation
  if (const int cfg = (a->tuning >> 4) & 0xf) {   // developer knob (tools/microbench.py); 0 = the shipped choice below
    if (cfg == 1 && t256 >= 192) return launch_tiled(s, p, epi, TILE_256x256_W16, nullptr);
    if (cfg == 2) return launch_tiled(s, p, epi, TILE_128x128, nullptr);
    // 3: 256x256, 4 waves, persistent, hand-scheduled; 4: the same whatever the tile count (small-M experiments: T5 11.3 -> 13.6 ms; 256x128 8-wave tiles: 12.9 ms -- the 128x128 tile stays)
    if (cfg == 4 || (cfg == 3 && t256 >= 192)) {
      const int rc = launch_w4(s, p, epi);
      if (rc != MRAG_ENOTSUP) return rc;
    }
  }
  // problems made of whole 128-column wave tiles: the persistent four-wave kernel -- 3-13 % ahead of the 8-wave 256x256 tile on the DiT's shapes, 8-27 %
  // on the UNets' N = 640 / 1280 linears (where it also replaces the 256x320 tile); behind the 8-wave tile where the epilogue of one wave per SIMD outweighs
  // a short K loop (GELU below K = 1536, anything below K = 320), and on shapes that would take its general epilogue path (profiles/r3_gemm_w4_ab.txt)
  if (a->w_batch_stride != 0) {
    // per-sample weights (the motion branch's folded score GEMM): the persistent four-wave kernel only -- whole 128-column wave tiles, aligned rows, no
    // epilogue; anything else is the caller's loop over the samples
    if (epi != MRAG_EPI_NONE || a->N % 128 != 0 || a->K < 320 || a->rows_per_batch <= 0 || a->M % a->rows_per_batch != 0 || a->ldc % 8 != 0 || (((uintptr_t)a->C) & 15) ||
        (a->tuning & (MRAG_GEMM_TUNE_NO_W4 | MRAG_GEMM_TUNE_NO_STAGED)))
      return MRAG_ENOTSUP;
    return launch_w4(s, p, epi);
  }
  if (a->a_ln) return skinny_applies(a, epi) ? launch_skinny(s, p, epi) : MRAG_ENOTSUP;   // the LayerNorm-in-the-A-load form lives in the few-row kernel only: the caller runs LayerNorm + GEMM otherwise
  if (skinny_applies(a, epi)) return launch_skinny(s, p, epi);       // M <= 256: eight waves split K, no LDS ring (gemm_skinny_kernel)
  if (k320_applies(a, epi)) return launch_k320(s, p, epi);           // K = 320, N = 320 .. 2 560: the weight in registers, activations streamed (gemm_k320_kernel)
  const bool w4_ok = t256 >= 192 && !(a->tuning & (MRAG_GEMM_TUNE_NO_W4 | MRAG_GEMM_TUNE_NO_STAGED | MRAG_GEMM_TUNE_STREAMK | MRAG_GEMM_TUNE_NO_WIDE)) && a->N % 128 == 0 &&
      a->K >= (epi == MRAG_EPI_GELU_TANH ? 1536 : 320) &&
      (epi == MRAG_EPI_NONE || epi == MRAG_EPI_GELU_TANH || epi == MRAG_EPI_RESID || epi == MRAG_EPI_GATE_RESID || epi == MRAG_EPI_QKNORM_ROPE || epi == MRAG_EPI_GEGLU ||
       epi == EPI_GEGLU_TANH) &&
      rows_16B_aligned(a->C, a->ldc, a->resid, a->ldr);
  const bool w4_tail = w4_ok && tail_rect_wanted(t256, epi, a->tuning);
  // (first: a problem that the 320-wide tile finishes in fewer rounds -- see wide_rounds_pay; the persistent kernel walks the same 256x256 tile grid)
  if (t256 >= 192 && !wide_n_pays(a->N, a->tuning) && wide_rounds_pay(a->M, a->N, a->tuning, w4_tail) && !(a->tuning & MRAG_GEMM_TUNE_STREAMK) && a->epilogue != MRAG_EPI_GEGLU &&
      a->epilogue != MRAG_EPI_QKNORM_ROPE)
    return launch_tiled(s, p, epi, TILE_256x320, nullptr);
  if (w4_ok) {
    const int rc = launch_w4(s, p, epi);
    if (rc != MRAG_ENOTSUP) return rc;
  }
  if (t256 >= 192 && wide_n_pays(a->N, a->tuning) && a->epilogue != MRAG_EPI_GEGLU) return launch_tiled(s, p, epi, TILE_256x320, nullptr);   // 256x320 tile
  if (t256 >= 192 && a->workspace && (a->tuning & MRAG_GEMM_TUNE_STREAMK) &&
      (epi == MRAG_EPI_NONE || epi == MRAG_EPI_GELU_TANH || epi == MRAG_EPI_RESID || epi == MRAG_EPI_GATE_RESID || epi == MRAG_EPI_QKNORM_ROPE)) {
    const SkPlan pl = plan_streamk(a->M, a->N, a->K);
    if (pl.use && a->workspace_bytes >= (int64_t)pl.bytes) {
      if ((uintptr_t)a->workspace & 15) return MRAG_EINVAL;
      p.sk_ticket = (unsigned*)a->workspace;
      p.sk_part = (float*)((char*)a->workspace + SK_TICKET_BYTES);
      p.sk_main = pl.n_main; p.sk_rem = pl.rem; p.sk_units = pl.units; p.sk_maxparts = pl.maxparts;
      const hipError_t e = hipMemsetAsync(a->workspace, 0, SK_TICKET_BYTES, s);   // the tickets start at zero whatever an earlier (aborted) launch left
      if (e != hipSuccess) return (int)e;
      const int rc = launch_tiled(s, p, epi, TILE_256x256, &pl);
      if (rc != MRAG_ENOTSUP) return rc;
    }
  }
  if (t256 >= 192) return launch_tiled(s, p, epi, TILE_256x256, nullptr);
  return launch_tiled(s, p, epi, TILE_128x128, nullptr);
}

extern "C" int64_t mrag_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 64 != 0) return 0;
  if (wide_n_pays(N)) return 0;
  const SkPlan pl = plan_streamk(M, N, K);
  return pl.use ? (int64_t)pl.bytes : 0;
}
