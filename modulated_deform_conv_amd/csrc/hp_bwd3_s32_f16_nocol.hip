// hp_bwd3_s32_f16_nocol.hip -- instances of the pixel-stationary 16-bit backward kernel without column rows (hp_bwd3_kernel.hpp,
// COLS = false: backwards that want no weight gradients) for fp32 offsets and masks (MDCONV_SAMPLING_F32): F16, 2-D and 3-D
#include "hp_bwd3_kernel.hpp"

namespace mdconv {

int hp_bwd3_s32_f16_nocol(const Geom &g, const HpDims &hd, const Tensors &t, const void *xt, const void *wpb, void *gcol, int *cnt,
                         hipStream_t stream) {
  if (g.nd == 2)
    return g.modulated ? dispatch_bwd3<2, true, F16, float, false>(g, hd, t, xt, wpb, gcol, nullptr, cnt, stream)
                       : dispatch_bwd3<2, false, F16, float, false>(g, hd, t, xt, wpb, gcol, nullptr, cnt, stream);
  return g.modulated ? dispatch_bwd3<3, true, F16, float, false>(g, hd, t, xt, wpb, gcol, nullptr, cnt, stream)
                     : dispatch_bwd3<3, false, F16, float, false>(g, hd, t, xt, wpb, gcol, nullptr, cnt, stream);
}

}  // namespace mdconv
