// dcn3_fwd.hip -- forward of the DCNv3 core operator (dcn3_plan.hpp).
//
// Lane = one 16-byte channel vector of one (output pixel, group) pair; the VL lanes of a pair are adjacent and the pairs of
// a pixel follow each other, so the output store and every corner load are contiguous 16-byte pieces across neighbouring
// lanes.  Taps outside: the VL lanes of a pair build the sampling state of VL consecutive taps at once -- lane j the state
// of tap t0 + j, from one offset pair and one mask value -- and then walk those taps together, each state broadcast from
// the lane that built it (a wave shuffle; VL = 1: the lane's own).  fp32 accumulators, one rounding at the store.  No
// workspace, no LDS, no atomics.
#include "dcn3_plan.hpp"

namespace mdconv {

namespace {

template <int DT>
__global__ __launch_bounds__(256) void dcn3_fwd_kernel(Dcn3Geom g, const void *__restrict__ input, const void *__restrict__ offset,
                                                        const void *__restrict__ mask, void *__restrict__ output) {
  constexpr int NV = Dcn3Vec<DT>::NV;
  const Dcn3Lane ln = dcn3_lane(g, g.N * g.G);
  const Dcn3Pix px = dcn3_pix(g, ln.pair);
  const rsrc_t r_in = make_rsrc(input, (size_t)g.B * g.S_i * g.C * g.esz);
  for (int rd = 0; rd < g.rounds; ++rd) {   // one round unless a group has more than 64 vectors
    const int v = rd * g.VL + ln.j;
    const bool on = ln.live && v < g.V;
    const unsigned vbyte = on ? (unsigned)v * 16u : (unsigned)kDcn3Oob;   // (a parked corner stays out of range with it)
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    for (int t0 = 0; t0 < g.K; t0 += g.VL) {
      Dcn3Tap mine;
      dcn3_build_tap<DT>(g, px, ln.pair, t0 + ln.j, ln.live && t0 + ln.j < g.K, offset, mask, mine);
      const int nt = min(g.VL, g.K - t0);
      for (int jj = 0; jj < nt; ++jj) {
        const Dcn3Tap t = g.VL > 1 ? dcn3_tap_from(mine, ln.first + jj) : mine;
        float4 raw[4];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) raw[ci] = buf_load4(r_in, (int)min((unsigned)t.off[ci] + vbyte, (unsigned)kDcn3Oob), 0);
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          const float w = t.m * dcn3_corner_weight(t.lx, t.ly, ci);
          float x[NV];
          dcn3_unpack<DT>(raw[ci], x);
#pragma unroll
          for (int i = 0; i < NV; ++i) acc[i] = fmaf(w, x[i], acc[i]);
        }
      }
    }
    if (on) ((float4 *)output)[(int64_t)ln.pair * g.V + v] = dcn3_pack<DT>(acc);
  }
}

}  // namespace

int dcn3_fwd_launch(const Dcn3Plan &p, const Dcn3Tensors &t, hipStream_t stream) {
  const Dcn3Geom &g = p.g;
  const dim3 grid(dcn3_grid(g, (int64_t)g.N * g.G));
#define DCN3_FWD(DT) hipLaunchKernelGGL((dcn3_fwd_kernel<DT>), grid, dim3(256), 0, stream, g, t.input, t.offset, t.mask, t.output)
  if (p.dtype == MDCONV_F32) DCN3_FWD(MDCONV_F32);
  else if (p.dtype == MDCONV_F16) DCN3_FWD(MDCONV_F16);
  else DCN3_FWD(MDCONV_BF16);
#undef DCN3_FWD
  return check_launch("dcn3_fwd");
}

}  // namespace mdconv
