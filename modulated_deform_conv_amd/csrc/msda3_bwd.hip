// msda3_bwd.hip -- the coordinate gradients of 3-D multi-scale deformable attention (msda3_plan.hpp), without atomics.
//
// The lane mapping and the tap walk of the forward (msda3_fwd.hip).  Per (pair, tap) a lane takes the dot products of its
// grad_output vector with the eight corner vectors in-lane and weighs them four ways -- the trilinear weights (the attention
// weight's gradient) and their derivatives along x, y and z (the location's gradient) -- and the four sums over the pair's
// lanes are taken by xor butterflies inside the wave: a fixed order, every lane ends with the same bits.  Lane j keeps the
// sums of tap t0 + j, so after VL taps each lane stores one attention gradient and one (x, y, z) triple -- times the attention
// weight and W_l / H_l / T_l -- next to its neighbours', in the coordinate type and in the caller's write mode.  A gated-out
// sample reads nothing: its four sums are exact zeros.  On the lattice the fractions are those of the cell floor(x), floor(y),
// floor(z), so the derivative is the right-sided one.  A pair is owned by one group of lanes: nothing is shared between
// workgroups.
#include "msda3_plan.hpp"

namespace mdconv {

namespace {

template <int DT, int CT>
__global__ __launch_bounds__(256) void msda3_bwd_coord_kernel(Msda3Geom g, const void *__restrict__ value,
                                                               const void *__restrict__ loc, const void *__restrict__ attn,
                                                               const void *__restrict__ grad_output, void *__restrict__ grad_loc,
                                                               void *__restrict__ grad_attn) {
  constexpr int NV = SampVec<DT>::NV;
  const SampLane ln = samp_lane_of(g.ln.lgVL, g.npairs);
  const unsigned pair_byte = msda3_pair_byte(g, ln.pair);
  const unsigned row_bytes = (unsigned)(g.C * g.ln.esz);
  const rsrc_t r_in = make_rsrc(value, (size_t)g.N * g.S * g.C * g.ln.esz);
  const rsrc_t r_go = make_rsrc(grad_output, (size_t)g.npairs * g.D * g.ln.esz);
  const unsigned go_row = (unsigned)ln.pair * (unsigned)g.ln.V * 16u;   // the pair's channel row of grad_output
  float go0[NV];   // the first round's vector (the only one unless a head has more than 64 vectors)
  samp_unpack<DT>(buf_load4(r_go, ln.live && ln.j < g.ln.V ? (int)(go_row + (unsigned)ln.j * 16u) : kSampOob, 0), go0);
  for (int t0 = 0; t0 < g.K; t0 += g.ln.VL) {
    const int my_tap = t0 + ln.j;
    const bool my_on = ln.live && my_tap < g.K;
    Msda3Tap mine;
    float fx, fy, fz;   // of my_tap
    msda3_build_tap<CT>(g, pair_byte, ln.pair, my_tap, my_on, loc, attn, mine, fx, fy, fz);
    float r_m = 0.f, r_x = 0.f, r_y = 0.f, r_z = 0.f;   // the sums of my_tap
    const int nt = min(g.ln.VL, g.K - t0);
    for (int jj = 0; jj < nt; ++jj) {
      const Msda3Tap t = g.ln.VL > 1 ? msda3_tap_from(mine, ln.first + jj) : mine;
      float s_m = 0.f, s_x = 0.f, s_y = 0.f, s_z = 0.f;
      for (int rd = 0; rd < g.ln.rounds; ++rd) {
        const int v = rd * g.ln.VL + ln.j;
        const bool on = ln.live && v < g.ln.V;
        const unsigned vbyte = on ? (unsigned)v * 16u : (unsigned)kSampOob;
        float go[NV];
        if (rd == 0) {
#pragma unroll
          for (int i = 0; i < NV; ++i) go[i] = go0[i];
        } else {
          samp_unpack<DT>(buf_load4(r_go, (int)min(go_row + vbyte, (unsigned)kSampOob), 0), go);
        }
        float4 raw[8];
#pragma unroll
        for (int ci = 0; ci < 8; ++ci)
          raw[ci] = buf_load4(r_in, (int)min(msda3_corner_off(t, ci, row_bytes) + vbyte, (unsigned)kSampOob), 0);
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) {
          float x[NV];
          samp_unpack<DT>(raw[ci], x);
          float dot = 0.f;
#pragma unroll
          for (int i = 0; i < NV; ++i) dot = fmaf(go[i], x[i], dot);
          s_m = fmaf(msda3_corner_weight(t.lx, t.ly, t.lz, ci), dot, s_m);
          s_x = fmaf(msda3_corner_dx(t.ly, t.lz, ci), dot, s_x);
          s_y = fmaf(msda3_corner_dy(t.lx, t.lz, ci), dot, s_y);
          s_z = fmaf(msda3_corner_dz(t.lx, t.ly, ci), dot, s_z);
        }
      }
      for (int d = g.ln.VL >> 1; d >= 1; d >>= 1) {
        s_m += __shfl_xor(s_m, d, 64);
        s_x += __shfl_xor(s_x, d, 64);
        s_y += __shfl_xor(s_y, d, 64);
        s_z += __shfl_xor(s_z, d, 64);
      }
      if (jj == ln.j) {   // t is `mine`
        r_m = s_m;
        r_x = s_x * (t.m * fx);
        r_y = s_y * (t.m * fy);
        r_z = s_z * (t.m * fz);
      }
    }
    if (my_on) {
      const int e = ln.pair * g.K + my_tap;   // the element of attention_weights; (x, y, z) at three times that
      samp_st<CT>(grad_attn, e, r_m, g.acc != 0);
      samp_st<CT>(grad_loc, 3 * e, r_x, g.acc != 0);
      samp_st<CT>(grad_loc, 3 * e + 1, r_y, g.acc != 0);
      samp_st<CT>(grad_loc, 3 * e + 2, r_z, g.acc != 0);
    }
  }
}

}  // namespace

int msda3_bwd_coord_launch(const Msda3Plan &p, const Msda3Tensors &t, hipStream_t stream) {
  const Msda3Geom &g = p.g;
#define MSDA3_BWD(DT, CT)                                                                                          \
  hipLaunchKernelGGL((msda3_bwd_coord_kernel<DT, CT>), dim3(samp_grid(g.ln.lgVL, g.npairs)), dim3(256), 0, stream, g, \
                     t.value, t.loc, t.attn, t.grad_output, t.grad_loc, t.grad_attn)
  SAMP_DISPATCH(p, MSDA3_BWD);
#undef MSDA3_BWD
  return check_launch("msda3_bwd_coord");
}

}  // namespace mdconv
