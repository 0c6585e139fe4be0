// droi_fwd.hip -- the forward of deformable RoI pooling (droi_plan.hpp).
//
// Lane = one 16-byte channel vector of one bin, the lane mapping of the sampling core (samp_lane_of): the VL lanes of a bin are
// adjacent, bins of more than 64 vectors take rounds.  The RoI's geometry and the bin's offset are read once per bin (the
// lanes of a bin read the same addresses); the walk over the bin's gh x gw samples is uniform across the bin's lanes and
// costs four 16-byte corner loads per sample, parked out of range where a corner is not read.  fp32 accumulators, one
// rounding at the store.  No workspace, no LDS, no atomics.
#include "droi_plan.hpp"

namespace mdconv {

namespace {

template <int DT, int CT>
__global__ __launch_bounds__(256) void droi_fwd_kernel(DroiGeom g, const void *__restrict__ input, const float *__restrict__ rois,
                                                        const void *__restrict__ offset, void *__restrict__ output) {
  constexpr int NV = SampVec<DT>::NV;
  const SampLane ln = samp_lane_of(g.ln.lgVL, g.nbins);
  DroiBin bn;
  droi_bin<CT>(g, rois, offset, ln.pair, bn);
  const rsrc_t r_in = make_rsrc(input, (size_t)g.B * g.H * g.W * g.C * g.ln.esz);
  const unsigned row_bytes = (unsigned)(g.C * g.ln.esz);
  for (int rd = 0; rd < g.ln.rounds; ++rd) {   // one round unless a bin has more than 64 vectors
    const int v = rd * g.ln.VL + ln.j;
    const bool on = ln.live && v < g.ln.V;
    const unsigned vbyte = on ? (unsigned)v * 16u : (unsigned)kSampOob;   // (a parked corner stays out of range with it)
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    for (int iy = 0; iy < bn.gh; ++iy) {
      const DroiAxis ay = droi_axis(bn.y0 + ((float)iy + 0.5f) * bn.sy, g.H);
      for (int ix = 0; ix < bn.gw; ++ix) {
        const DroiAxis ax = droi_axis(bn.x0 + ((float)ix + 0.5f) * bn.sx, g.W);
        const unsigned base = (unsigned)(bn.img_row + ay.lo * g.W + ax.lo) * row_bytes;
        float4 raw[4];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          const unsigned off = droi_corner_read(ay, ax, ci, g.H, g.W)
                                   ? base + (unsigned)((ci >> 1) * g.W + (ci & 1)) * row_bytes : (unsigned)kSampOob;
          raw[ci] = buf_load4(r_in, (int)min(off + vbyte, (unsigned)kSampOob), 0);
        }
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          const float w = samp_corner_weight(ax.l, ay.l, ci);
          float x[NV];
          samp_unpack<DT>(raw[ci], x);
#pragma unroll
          for (int i = 0; i < NV; ++i) acc[i] = fmaf(w, x[i], acc[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] *= bn.inv_cnt;
    if (on) ((float4 *)output)[(int64_t)ln.pair * g.ln.V + v] = samp_pack<DT>(acc);
  }
}

}  // namespace

int droi_fwd_launch(const DroiPlan &p, const DroiTensors &t, hipStream_t stream) {
  const DroiGeom &g = p.g;
#define DROI_FWD(DT, CT)                                                                                                   \
  hipLaunchKernelGGL((droi_fwd_kernel<DT, CT>), dim3(samp_grid(g.ln.lgVL, g.nbins)), dim3(256), 0, stream, g, t.input, \
                     (const float *)t.rois, t.offset, t.output)
  SAMP_DISPATCH(p, DROI_FWD);
#undef DROI_FWD
  return check_launch("droi_fwd");
}

}  // namespace mdconv
