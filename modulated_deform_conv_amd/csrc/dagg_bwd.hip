// dagg_bwd.hip -- the weight and location gradients of deformable aggregation (dagg_plan.hpp), without atomics.
//
// The lane mapping and the unit walk of the forward (dagg_fwd.hip): an anchor is owned by one run of VL lanes, nothing is
// shared between waves.  Per (unit, level, round) a lane takes the dot products of its grad_output vector with the four
// corner vectors in-lane and weighs them three ways: the bilinear weights (s_m) and their derivatives along x and y.
//  - grad_weights[unit, l, g] is the sum of s_m over the lanes of group g.  Where a group is an aligned run of a power of
//    two of lanes inside one round (g.seg) that is a segmented xor butterfly, and the group's first lane stores; G
//    neighbouring elements leave in one instruction.  Otherwise (VG no power of two, or a group wider than a round) the
//    groups a round touches are summed one after the other by a butterfly over all VL lanes with the other groups masked
//    out; a group that continues in the next round carries its partial sum there -- only the last group of a round can --
//    and is stored where it ends.  Either way the order is fixed and each element is rounded once.
//  - grad_sampling_location[unit] is the sum over ALL lanes, rounds and levels of weight x derivative x (W_l, H_l): a lane
//    adds up its own share over levels and rounds, ONE butterfly over the VL lanes per unit ends it, and lane j keeps the
//    sums of unit t0 + j, so after VL units each lane stores one (x, y) pair next to its neighbours'.
// A gated-out unit reads nothing: in overwrite mode its L * G weight gradients and its (x, y) are stored as zeros, in
// accumulate mode they are not touched.  On the lattice the fractions are those of the cell floor(x), floor(y), so the
// derivative is the right-sided one.
#include "dagg_plan.hpp"

namespace mdconv {

namespace {

template <int DT, int CT>
__global__ __launch_bounds__(256) void dagg_bwd_coord_kernel(DaggGeom g, const void *__restrict__ feature,
                                                              const void *__restrict__ loc, const void *__restrict__ wts,
                                                              const void *__restrict__ grad_output, void *__restrict__ grad_loc,
                                                              void *__restrict__ grad_wts) {
  constexpr int NV = SampVec<DT>::NV;
  const SampLane ln = samp_lane_of(g.ln.lgVL, g.nanchors);
  const int img_row = (ln.pair / g.A) * g.S;
  const unsigned row_bytes = (unsigned)(g.C * g.ln.esz);
  const rsrc_t r_in = make_rsrc(feature, (size_t)g.B * g.S * g.C * g.ln.esz);
  const rsrc_t r_go = make_rsrc(grad_output, (size_t)g.nanchors * g.C * g.ln.esz);
  const unsigned go_row = (unsigned)ln.pair * (unsigned)g.ln.V * 16u;   // the anchor's row of grad_output
  const int LG = g.L * g.G;
  float go0[NV];   // the first round's vector (the only one unless a row has more than 64 vectors)
  samp_unpack<DT>(buf_load4(r_go, ln.live && ln.j < g.ln.V ? (int)(go_row + (unsigned)ln.j * 16u) : kSampOob, 0), go0);
  for (int t0 = 0; t0 < g.U; t0 += g.ln.VL) {
    const int my_unit = t0 + ln.j;
    const bool my_on = ln.live && my_unit < g.U;
    const DaggUnit mine = dagg_unit<CT>(loc, ln.pair * g.U + my_unit, my_on);
    float r_x = 0.f, r_y = 0.f;   // the sums of my_unit
    const int nt = min(g.ln.VL, g.U - t0);
    for (int jj = 0; jj < nt; ++jj) {
      const DaggUnit u = g.ln.VL > 1 ? dagg_unit_from(mine, ln.first + jj) : mine;
      const int unit = t0 + jj;
      const int wrow = (ln.pair * g.U + unit) * LG;   // the unit's first element of weights / grad_weights
      if (!u.in) {   // uniform across the anchor's lanes
        if (!g.acc && ln.live)
          for (int i = ln.j; i < LG; i += g.ln.VL) samp_st<CT>(grad_wts, wrow + i, 0.f, false);
        continue;
      }
      const int cam_row = img_row + (unit % g.cams) * g.S_cam;
      float a_x = 0.f, a_y = 0.f;   // the lane's share of the unit's location gradient
      for (int l = 0; l < g.L; ++l) {
        int H, W, start;
        dagg_level(g, l, H, W, start);
        SampSample s;
        dagg_sample(u, H, W, s);
        unsigned off[4];
        dagg_corner_offs(s, H, W, cam_row + start, row_bytes, off);
        float carry = 0.f;   // of a group that began in an earlier round
        for (int rd = 0; rd < g.ln.rounds; ++rd) {
          const int v = rd * g.ln.VL + ln.j;
          const bool on = ln.live && v < g.ln.V;
          const unsigned vbyte = on ? (unsigned)v * 16u : (unsigned)kSampOob;
          const int grp = on ? v / g.VG : 0;
          float go[NV];
          if (rd == 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i) go[i] = go0[i];
          } else {
            samp_unpack<DT>(buf_load4(r_go, (int)min(go_row + vbyte, (unsigned)kSampOob), 0), go);
          }
          float4 raw[4];
#pragma unroll
          for (int ci = 0; ci < 4; ++ci) raw[ci] = buf_load4(r_in, (int)min(off[ci] + vbyte, (unsigned)kSampOob), 0);
          float s_m = 0.f, s_x = 0.f, s_y = 0.f;
#pragma unroll
          for (int ci = 0; ci < 4; ++ci) {
            float x[NV];
            samp_unpack<DT>(raw[ci], x);
            float dot = 0.f;
#pragma unroll
            for (int i = 0; i < NV; ++i) dot = fmaf(go[i], x[i], dot);
            s_m = fmaf(samp_corner_weight(s.lx, s.ly, ci), dot, s_m);
            s_x = fmaf(samp_corner_dx(s.ly, ci), dot, s_x);
            s_y = fmaf(samp_corner_dy(s.lx, ci), dot, s_y);
          }
          const float m = on ? samp_ld<CT>(wts, wrow + l * g.G + grp) : 0.f;
          a_x = fmaf(m * (float)W, s_x, a_x);
          a_y = fmaf(m * (float)H, s_y, a_y);
          if (g.seg) {
            for (int d = g.VG >> 1; d >= 1; d >>= 1) s_m += __shfl_xor(s_m, d, 64);
            if (on && (v & (g.VG - 1)) == 0) samp_st<CT>(grad_wts, wrow + l * g.G + grp, s_m, g.acc != 0);
          } else {
            const int v_end = min(g.ln.V, (rd + 1) * g.ln.VL);   // one past the round's last vector
            const int g_lo = rd * g.ln.VL / g.VG, g_hi = (v_end - 1) / g.VG;
            for (int gg = g_lo; gg <= g_hi; ++gg) {
              float sum = on && grp == gg ? s_m : 0.f;
              for (int d = g.ln.VL >> 1; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
              if (gg == g_lo) sum += carry;
              if ((gg + 1) * g.VG > v_end) {
                carry = sum;   // the group goes on in the next round
              } else {
                if (ln.live && ln.j == 0) samp_st<CT>(grad_wts, wrow + l * g.G + gg, sum, g.acc != 0);
                carry = 0.f;
              }
            }
          }
        }
      }
      for (int d = g.ln.VL >> 1; d >= 1; d >>= 1) {
        a_x += __shfl_xor(a_x, d, 64);
        a_y += __shfl_xor(a_y, d, 64);
      }
      if (jj == ln.j) {   // u is `mine`
        r_x = a_x;
        r_y = a_y;
      }
    }
    if (my_on && (mine.in || !g.acc)) {
      const int e = 2 * (ln.pair * g.U + my_unit);
      samp_st<CT>(grad_loc, e, r_x, g.acc != 0);
      samp_st<CT>(grad_loc, e + 1, r_y, g.acc != 0);
    }
  }
}

}  // namespace

int dagg_bwd_coord_launch(const DaggPlan &p, const DaggTensors &t, hipStream_t stream) {
  const DaggGeom &g = p.g;
#define DAGG_BWD(DT, CT)                                                                                            \
  hipLaunchKernelGGL((dagg_bwd_coord_kernel<DT, CT>), dim3(samp_grid(g.ln.lgVL, g.nanchors)), dim3(256), 0, stream, g, \
                     t.feature, t.loc, t.wts, t.grad_output, t.grad_loc, t.grad_wts)
  SAMP_DISPATCH(p, DAGG_BWD);
#undef DAGG_BWD
  return check_launch("dagg_bwd_coord");
}

}  // namespace mdconv
