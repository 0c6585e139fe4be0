// hp_bwd3_bf16_2d_nocol.hip -- instances of the pixel-stationary 16-bit backward kernel without column rows (hp_bwd3_kernel.hpp,
// COLS = false: backwards that want no weight gradients): BF16, 2-D
#include "hp_bwd3_kernel.hpp"

namespace mdconv {

int hp_bwd3_bf16_2d_nocol(const Geom &g, const HpDims &hd, const Tensors &t, const void *xt, const void *wpb, void *gcol, int *cnt,
                         hipStream_t stream) {
  return g.modulated ? dispatch_bwd3<2, true, BF16, BF16::Raw, false>(g, hd, t, xt, wpb, gcol, nullptr, cnt, stream)
                     : dispatch_bwd3<2, false, BF16, BF16::Raw, false>(g, hd, t, xt, wpb, gcol, nullptr, cnt, stream);
}

}  // namespace mdconv
