// gemm_tiled.hip -- the tile shapes of the linears (CONV == 0 instantiations of gemm_tile.h) and the stream-K tail, behind one launcher.
#include "gemm_tile.h"

extern "C" int launch_tiled(hipStream_t s, const GemmP& p, int epi, int tile, const SkPlan* sk) {
  switch (tile) {
    case TILE_256x256_W16: return launch_cfg<4, 4, 4, 4>(s, p, epi, sk);   // 256x256, 16 waves (4 per SIMD)
    case TILE_128x128: return launch_cfg<2, 2, 4, 4>(s, p, epi, sk);       // 128x128, 4 waves, 2 workgroups per CU
    case TILE_256x320: return launch_cfg<2, 4, 8, 5>(s, p, epi, sk);       // 256x320, 8 waves
    case TILE_256x256: return launch_cfg<2, 4, 8, 4>(s, p, epi, sk);       // 256x256, 8 waves; the only shape with a stream-K tail
    default: return MRAG_EINVAL;
  }
}
