// hp_bwd3_f16_3d_nocol.hip -- instances of the pixel-stationary 16-bit backward kernel without column rows (hp_bwd3_kernel.hpp,
// COLS = false: backwards that want no weight gradients): F16, 3-D
#include "hp_bwd3_kernel.hpp"

namespace mdconv {

int hp_bwd3_f16_3d_nocol(const Geom &g, const HpDims &hd, const Tensors &t, const void *xt, const void *wpb, void *gcol, int *cnt,
                        hipStream_t stream) {
  return g.modulated ? dispatch_bwd3<3, true, F16, F16::Raw, false>(g, hd, t, xt, wpb, gcol, nullptr, cnt, stream)
                     : dispatch_bwd3<3, false, F16, F16::Raw, false>(g, hd, t, xt, wpb, gcol, nullptr, cnt, stream);
}

}  // namespace mdconv
