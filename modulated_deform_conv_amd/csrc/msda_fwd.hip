// msda_fwd.hip -- forward of multi-scale deformable attention (msda_plan.hpp).
//
// The structure of dcn3_fwd.hip: lane = one 16-byte channel vector of one (query, head) pair; the VL lanes of a pair build
// the sampling state of VL consecutive taps at once -- lane j the state of tap t0 + j, from one location pair and one
// attention weight, with the extents and the start row of the tap's level -- and then walk those taps together, each state
// broadcast from the lane that built it (a wave shuffle; VL = 1: the lane's own).  fp32 accumulators, one rounding at the
// store.  No workspace, no LDS, no atomics.
#include "msda_plan.hpp"

namespace mdconv {

namespace {

template <int DT, int CT>
__global__ __launch_bounds__(256) void msda_fwd_kernel(MsdaGeom g, const void *__restrict__ value, const void *__restrict__ loc,
                                                        const void *__restrict__ attn, void *__restrict__ output) {
  constexpr int NV = Dcn3Vec<DT>::NV;
  const Dcn3Lane ln = dcn3_lane_of(g.lgVL, g.npairs);
  const int pair_byte = msda_pair_byte(g, ln.pair);
  const rsrc_t r_val = make_rsrc(value, (size_t)g.N * g.S * g.C * g.esz);
  for (int rd = 0; rd < g.rounds; ++rd) {   // one round unless a head has more than 64 vectors
    const int v = rd * g.VL + ln.j;
    const bool on = ln.live && v < g.V;
    const unsigned vbyte = on ? (unsigned)v * 16u : (unsigned)kDcn3Oob;   // (a parked corner stays out of range with it)
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    for (int t0 = 0; t0 < g.K; t0 += g.VL) {
      Dcn3Tap mine;
      int H, W;
      msda_build_tap<CT>(g, pair_byte, ln.pair, t0 + ln.j, ln.live && t0 + ln.j < g.K, loc, attn, mine, H, W);
      const int nt = min(g.VL, g.K - t0);
      for (int jj = 0; jj < nt; ++jj) {
        const Dcn3Tap t = g.VL > 1 ? dcn3_tap_from(mine, ln.first + jj) : mine;
        float4 raw[4];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) raw[ci] = buf_load4(r_val, (int)min((unsigned)t.off[ci] + vbyte, (unsigned)kDcn3Oob), 0);
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

int msda_fwd_launch(const MsdaPlan &p, const MsdaTensors &t, hipStream_t stream) {
  const MsdaGeom &g = p.g;
  const dim3 grid(msda_grid(g, g.npairs));
#define MSDA_FWD(DT, CT) \
  hipLaunchKernelGGL((msda_fwd_kernel<DT, CT>), grid, dim3(256), 0, stream, g, t.value, t.loc, t.attn, t.output)
  MSDA_DISPATCH(p, MSDA_FWD);
#undef MSDA_FWD
  return check_launch("msda_fwd");
}

}  // namespace mdconv
