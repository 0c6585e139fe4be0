// droi_bwd.hip -- the offset gradient of deformable RoI pooling (droi_plan.hpp), without atomics.
//
// The lane mapping and the sample walk of the forward (droi_fwd.hip).  Per sample a lane takes the dot products of its
// grad_output vector with the four corner vectors in-lane and weighs them with the derivatives of the bilinear weights along
// x and along y -- zero along an axis whose coordinate is clamped, and a gated-out sample reads nothing -- summing over the
// bin's samples and over the rounds in registers.  One xor butterfly over the bin's lanes follows (a fixed order), and the
// bin's lane 0 stores the (x, y) pair times gamma * rw / cnt and gamma * rh / cnt, in the coordinate type and in the caller's
// write mode.  A bin is owned by one group of lanes: nothing is shared between workgroups.
#include "droi_plan.hpp"

namespace mdconv {

namespace {

template <int DT, int CT>
__global__ __launch_bounds__(256) void droi_bwd_offset_kernel(DroiGeom g, const void *__restrict__ input,
                                                               const float *__restrict__ rois, const void *__restrict__ offset,
                                                               const void *__restrict__ grad_output, void *__restrict__ grad_offset) {
  constexpr int NV = SampVec<DT>::NV;
  const SampLane ln = samp_lane_of(g.ln.lgVL, g.nbins);
  DroiBin bn;
  droi_bin<CT>(g, rois, offset, ln.pair, bn);
  const rsrc_t r_in = make_rsrc(input, (size_t)g.B * g.H * g.W * g.C * g.ln.esz);
  const rsrc_t r_go = make_rsrc(grad_output, (size_t)g.nbins * g.C * g.ln.esz);
  const unsigned row_bytes = (unsigned)(g.C * g.ln.esz);
  const unsigned go_row = (unsigned)ln.pair * row_bytes;   // the bin's channel row of grad_output
  float s_x = 0.f, s_y = 0.f;
  for (int rd = 0; rd < g.ln.rounds; ++rd) {   // one round unless a bin has more than 64 vectors
    const int v = rd * g.ln.VL + ln.j;
    const bool on = ln.live && v < g.ln.V;
    const unsigned vbyte = on ? (unsigned)v * 16u : (unsigned)kSampOob;
    float go[NV];
    samp_unpack<DT>(buf_load4(r_go, (int)min(go_row + vbyte, (unsigned)kSampOob), 0), go);
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
        float t_x = 0.f, t_y = 0.f;
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          float x[NV];
          samp_unpack<DT>(raw[ci], x);
          float dot = 0.f;
#pragma unroll
          for (int i = 0; i < NV; ++i) dot = fmaf(go[i], x[i], dot);
          t_x = fmaf(samp_corner_dx(ay.l, ci), dot, t_x);
          t_y = fmaf(samp_corner_dy(ax.l, ci), dot, t_y);
        }
        s_x += ax.free ? t_x : 0.f;
        s_y += ay.free ? t_y : 0.f;
      }
    }
  }
  for (int d = g.ln.VL >> 1; d >= 1; d >>= 1) {
    s_x += __shfl_xor(s_x, d, 64);
    s_y += __shfl_xor(s_y, d, 64);
  }
  // (a RoI that contributes nothing leaves the caller's values untouched in accumulate mode, bit for bit)
  if (ln.live && ln.j == 0 && (bn.ok || !g.acc)) {
    const int npb = g.PH * g.PW;
    const int r = ln.pair / npb, cell = ln.pair - r * npb;
    const int e = r * 2 * npb + cell;
    samp_st<CT>(grad_offset, e, bn.ok ? s_x * (bn.fx * bn.inv_cnt) : 0.f, g.acc != 0);
    samp_st<CT>(grad_offset, e + npb, bn.ok ? s_y * (bn.fy * bn.inv_cnt) : 0.f, g.acc != 0);
  }
}

}  // namespace

int droi_bwd_offset_launch(const DroiPlan &p, const DroiTensors &t, hipStream_t stream) {
  const DroiGeom &g = p.g;
#define DROI_BWD(DT, CT)                                                                                                 \
  hipLaunchKernelGGL((droi_bwd_offset_kernel<DT, CT>), dim3(samp_grid(g.ln.lgVL, g.nbins)), dim3(256), 0, stream, g, \
                     t.input, (const float *)t.rois, t.offset, t.grad_output, t.grad_offset)
  SAMP_DISPATCH(p, DROI_BWD);
#undef DROI_BWD
  return check_launch("droi_bwd_offset");
}

}  // namespace mdconv
