// gemm_conv.hip -- the 3x3 (x3) and (3,1,1) convolutions as implicit GEMMs: the CONV == 1 / 2 instantiations of gemm_tile.h and their tile choice.
#include "gemm_tile.h"

extern "C" int mrag_conv_bf16(void* stream, const mrag_conv_args* a) {
  if (!a || !a->x || !a->W || !a->y) return MRAG_EINVAL;
  if (a->N <= 0 || a->H <= 0 || a->Wd <= 0 || a->Cin <= 0 || a->Cout <= 0) return MRAG_EINVAL;
  if (a->Cin % 64 != 0 || a->Cout % 4 != 0) return MRAG_ENOTSUP;   // one K-tile = 64 channels of one tap
  if (a->mode != MRAG_CONV_3X3 && a->mode != MRAG_CONV_T3) return MRAG_EINVAL;
  if (a->epilogue != MRAG_EPI_NONE && a->epilogue != MRAG_EPI_RESID) return MRAG_EINVAL;
  if (((uintptr_t)a->x | (uintptr_t)a->W) & 15) return MRAG_EINVAL;
  if ((uintptr_t)a->y & 7) return MRAG_EINVAL;
  if (a->epilogue == MRAG_EPI_RESID && (!a->resid || ((uintptr_t)a->resid & 7))) return MRAG_EINVAL;
  GemmP p{};
  p.A = (const bf16_t*)a->x; p.W = (const bf16_t*)a->W; p.bias = (const bf16_t*)a->bias; p.C = (bf16_t*)a->y; p.resid = (const bf16_t*)a->resid;
  p.N = a->Cout; p.ldc = a->Cout; p.ldr = a->Cout; p.cv_C = a->Cin; p.cv_ctiles = a->Cin / 64;
  p.acc_scale = a->acc_scale == 0.0f ? 1.0f : a->acc_scale;
  hipStream_t s = (hipStream_t)stream;
  // the implicit GEMM walks its sources with 32-bit offsets (gemm_tile): positions in 16-byte units relative to the first sample a workgroup touches
  // (at most a few frames apart), weight rows in bytes relative to W
  if ((long long)a->H * a->Wd * (a->Cin / 8) * 6 >= (1LL << 31) || (long long)a->Cout * 27 * a->Cin * 2 >= (1LL << 32)) return MRAG_ENOTSUP;
  if (a->mode == MRAG_CONV_3X3) {
    if ((a->stride != 1 && a->stride != 2) || (a->upsample != 0 && a->upsample != 1)) return MRAG_EINVAL;
    p.cv_H = a->H; p.cv_W = a->Wd; p.cv_up = a->upsample; p.cv_stride = a->stride;
    p.cv_Hi = a->upsample ? 2 * a->H : a->H; p.cv_Wi = a->upsample ? 2 * a->Wd : a->Wd;
    if (a->asym_pad != 0 && (a->asym_pad != 1 || a->stride != 2 || a->upsample)) return MRAG_EINVAL;
    p.cv_pad = a->asym_pad ? 0 : 1;
    // padding 1 / 1: Ho = (Hi + 2 - 3) / stride + 1; padding 0 / 1: Ho = (Hi + 1 - 3) / stride + 1
    p.cv_Ho = (p.cv_Hi + p.cv_pad - 2) / a->stride + 1; p.cv_Wo = (p.cv_Wi + p.cv_pad - 2) / a->stride + 1;
    p.M = (long long)a->N * p.cv_Ho * p.cv_Wo; p.K = 9LL * a->Cin; p.ldw = p.K;
    if (a->t_taps != 0) {   // causal 3x3x3 over frame stacks that already hold the two leading context frames
      if (a->t_taps != 3 || a->t_frames <= 0 || a->N % a->t_frames != 0 || a->stride != 1 || a->upsample || a->asym_pad) return MRAG_EINVAL;
      p.cv_tf = a->t_frames; p.cv_fs = (long long)a->H * a->Wd * a->Cin; p.K = 27LL * a->Cin; p.ldw = p.K;
    }
    const long long t256 = ((p.M + 255) / 256) * ((p.N + 255) / 256);
    if (t256 >= 192 && (wide_n_pays(p.N) || wide_rounds_pay(p.M, p.N))) return launch_cfg<2, 4, 8, 5, 1>(s, p, a->epilogue);
    if (t256 >= 192 && narrow_n_pays(p.N)) return launch_cfg<4, 2, 4, 4, 1>(s, p, a->epilogue);   // 256x128 tile, 8 waves of 64x64
    if (t256 >= 192 && short_rows_pay(p.M, p.N)) return launch_cfg<2, 4, 6, 4, 1>(s, p, a->epilogue);   // 192x256 tile
    if (t256 >= 192) return launch_cfg<2, 4, 8, 4, 1>(s, p, a->epilogue);
    return launch_cfg<2, 2, 4, 4, 1>(s, p, a->epilogue);
  }
  // (3,1,1) temporal convolution over x [(N = B) x (H = T), Wd = HW, Cin]
  p.cv_T = a->H; p.cv_HW = a->Wd;
  p.M = (long long)a->N * a->H * a->Wd; p.K = 3LL * a->Cin; p.ldw = p.K;
  const long long t256 = ((p.M + 255) / 256) * ((p.N + 255) / 256);
  if (t256 >= 192 && (wide_n_pays(p.N) || wide_rounds_pay(p.M, p.N))) return launch_cfg<2, 4, 8, 5, 2>(s, p, a->epilogue);
  if (t256 >= 192 && short_rows_pay(p.M, p.N)) return launch_cfg<2, 4, 6, 4, 2>(s, p, a->epilogue);      // 192x256 tile
  if (t256 >= 192) return launch_cfg<2, 4, 8, 4, 2>(s, p, a->epilogue);
  return launch_cfg<2, 2, 4, 4, 2>(s, p, a->epilogue);
}
