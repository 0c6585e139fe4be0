// msda3_fwd.hip -- the forward of 3-D multi-scale deformable attention (msda3_plan.hpp).
//
// Lane = one 16-byte channel vector of one (query, head) pair, the lane mapping of the sampling core (samp_lane_of): the VL
// lanes of a pair are adjacent, heads of more than 64 vectors take rounds.  Taps outside: the VL lanes of a pair build the
// state of VL consecutive taps at once -- lane j the state of tap t0 + j, from one (x, y, z) triple and one attention weight --
// and then walk those taps together, each state broadcast from the lane that built it (eight wave shuffles; VL = 1: the
// lane's own).  Per tap eight 16-byte corner loads with 32-bit offsets, parked out of range where a corner is not read.  fp32
// accumulators, one rounding at the store.  No workspace, no LDS, no atomics.
#include "msda3_plan.hpp"

namespace mdconv {

namespace {

template <int DT, int CT>
__global__ __launch_bounds__(256) void msda3_fwd_kernel(Msda3Geom g, const void *__restrict__ value, const void *__restrict__ loc,
                                                         const void *__restrict__ attn, void *__restrict__ output) {
  constexpr int NV = SampVec<DT>::NV;
  const SampLane ln = samp_lane_of(g.ln.lgVL, g.npairs);
  const unsigned pair_byte = msda3_pair_byte(g, ln.pair);
  const unsigned row_bytes = (unsigned)(g.C * g.ln.esz);
  const rsrc_t r_in = make_rsrc(value, (size_t)g.N * g.S * g.C * g.ln.esz);
  for (int rd = 0; rd < g.ln.rounds; ++rd) {   // one round unless a head has more than 64 vectors
    const int v = rd * g.ln.VL + ln.j;
    const bool on = ln.live && v < g.ln.V;
    const unsigned vbyte = on ? (unsigned)v * 16u : (unsigned)kSampOob;   // (a parked corner stays out of range with it)
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    for (int t0 = 0; t0 < g.K; t0 += g.ln.VL) {
      Msda3Tap mine;
      float fx, fy, fz;
      msda3_build_tap<CT>(g, pair_byte, ln.pair, t0 + ln.j, ln.live && t0 + ln.j < g.K, loc, attn, mine, fx, fy, fz);
      const int nt = min(g.ln.VL, g.K - t0);
      for (int jj = 0; jj < nt; ++jj) {
        const Msda3Tap t = g.ln.VL > 1 ? msda3_tap_from(mine, ln.first + jj) : mine;
        float4 raw[8];
#pragma unroll
        for (int ci = 0; ci < 8; ++ci)
          raw[ci] = buf_load4(r_in, (int)min(msda3_corner_off(t, ci, row_bytes) + vbyte, (unsigned)kSampOob), 0);
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) {
          const float w = t.m * msda3_corner_weight(t.lx, t.ly, t.lz, ci);
          float x[NV];
          samp_unpack<DT>(raw[ci], x);
#pragma unroll
          for (int i = 0; i < NV; ++i) acc[i] = fmaf(w, x[i], acc[i]);
        }
      }
    }
    if (on) ((float4 *)output)[(int64_t)ln.pair * g.ln.V + v] = samp_pack<DT>(acc);
  }
}

}  // namespace

int msda3_fwd_launch(const Msda3Plan &p, const Msda3Tensors &t, hipStream_t stream) {
  const Msda3Geom &g = p.g;
#define MSDA3_FWD(DT, CT)                                                                                               \
  hipLaunchKernelGGL((msda3_fwd_kernel<DT, CT>), dim3(samp_grid(g.ln.lgVL, g.npairs)), dim3(256), 0, stream, g, t.value, \
                     t.loc, t.attn, t.output)
  SAMP_DISPATCH(p, MSDA3_FWD);
#undef MSDA3_FWD
  return check_launch("msda3_fwd");
}

}  // namespace mdconv
