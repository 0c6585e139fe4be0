// dagg_fwd.hip -- the forward of deformable aggregation (dagg_plan.hpp).
//
// Lane = one 16-byte channel vector of one ANCHOR: the VL lanes of an anchor are adjacent (samp_lane_of with the anchor's
// row as the head), rows of more than 64 vectors take rounds; a channel group is a run of VG vectors.  The unit of the walk
// is a (point, camera): the VL lanes of an anchor read VL consecutive units at once -- lane j the location and gate of
// unit t0 + j -- and then walk them together, each broadcast from the lane that read it (three wave shuffles; VL = 1: the
// lane's own).  A gated-out unit is skipped for all L levels and all groups by one branch that is uniform across the
// anchor's lanes, before a weight or a feature row is touched.  Inside a unit the L levels are a loop over the level table;
// per level a lane loads the weight of its group and four 16-byte corner vectors with 32-bit offsets, parked out of range
// where a corner is not read.  fp32 accumulators, one rounding at the store.  No workspace, no LDS, no atomics.
#include "dagg_plan.hpp"

namespace mdconv {

namespace {

template <int DT, int CT>
__global__ __launch_bounds__(256) void dagg_fwd_kernel(DaggGeom g, const void *__restrict__ feature, const void *__restrict__ loc,
                                                        const void *__restrict__ wts, void *__restrict__ output) {
  constexpr int NV = SampVec<DT>::NV;
  const SampLane ln = samp_lane_of(g.ln.lgVL, g.nanchors);
  const int img_row = (ln.pair / g.A) * g.S;   // the image's first row of `feature`
  const unsigned row_bytes = (unsigned)(g.C * g.ln.esz);
  const rsrc_t r_in = make_rsrc(feature, (size_t)g.B * g.S * g.C * g.ln.esz);
  for (int rd = 0; rd < g.ln.rounds; ++rd) {   // one round unless a row has more than 64 vectors
    const int v = rd * g.ln.VL + ln.j;
    const bool on = ln.live && v < g.ln.V;
    const unsigned vbyte = on ? (unsigned)v * 16u : (unsigned)kSampOob;   // (a parked corner stays out of range with it)
    const int grp = on ? v / g.VG : 0;
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    for (int t0 = 0; t0 < g.U; t0 += g.ln.VL) {
      const DaggUnit mine = dagg_unit<CT>(loc, ln.pair * g.U + t0 + ln.j, ln.live && t0 + ln.j < g.U);
      const int nt = min(g.ln.VL, g.U - t0);
      for (int jj = 0; jj < nt; ++jj) {
        const DaggUnit u = g.ln.VL > 1 ? dagg_unit_from(mine, ln.first + jj) : mine;
        if (!u.in) continue;   // uniform across the anchor's lanes
        const int unit = t0 + jj;
        const int cam_row = img_row + (unit % g.cams) * g.S_cam;
        const int wrow = (ln.pair * g.U + unit) * g.L * g.G + grp;   // the lane's weight on level 0
        for (int l = 0; l < g.L; ++l) {
          int H, W, start;
          dagg_level(g, l, H, W, start);
          SampSample s;
          dagg_sample(u, H, W, s);
          unsigned off[4];
          dagg_corner_offs(s, H, W, cam_row + start, row_bytes, off);
          const float m = samp_ld<CT>(wts, wrow + l * g.G);
          float4 raw[4];
#pragma unroll
          for (int ci = 0; ci < 4; ++ci) raw[ci] = buf_load4(r_in, (int)min(off[ci] + vbyte, (unsigned)kSampOob), 0);
#pragma unroll
          for (int ci = 0; ci < 4; ++ci) {
            const float w = m * samp_corner_weight(s.lx, s.ly, ci);
            float x[NV];
            samp_unpack<DT>(raw[ci], x);
#pragma unroll
            for (int i = 0; i < NV; ++i) acc[i] = fmaf(w, x[i], acc[i]);
          }
        }
      }
    }
    if (on) ((float4 *)output)[(int64_t)ln.pair * g.ln.V + v] = samp_pack<DT>(acc);
  }
}

}  // namespace

int dagg_fwd_launch(const DaggPlan &p, const DaggTensors &t, hipStream_t stream) {
  const DaggGeom &g = p.g;
#define DAGG_FWD(DT, CT)                                                                                                \
  hipLaunchKernelGGL((dagg_fwd_kernel<DT, CT>), dim3(samp_grid(g.ln.lgVL, g.nanchors)), dim3(256), 0, stream, g, t.feature, \
                     t.loc, t.wts, t.output)
  SAMP_DISPATCH(p, DAGG_FWD);
#undef DAGG_FWD
  return check_launch("dagg_fwd");
}

}  // namespace mdconv
