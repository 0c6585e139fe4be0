// msda_bwd.hip -- grad_sampling_locations and grad_attention_weights of multi-scale deformable attention (msda_plan.hpp),
// without atomics.
//
// The structure of dcn3_bwd.hip on the lane mapping and the tap walk of the forward (msda_fwd.hip): per (pair, tap) a lane
// takes the dot products of its grad_output vector with the four corner vectors in-lane, weighs them three ways -- the
// bilinear weights (grad_attention_weights), their derivatives along x and along y (grad_sampling_locations) -- and the
// three sums over the pair's lanes are taken by an xor butterfly inside the wave: a fixed order, every lane ends with the
// same bits.  Lane j keeps the sums of tap t0 + j, so after VL taps each lane stores one weight gradient and one (x, y)
// pair -- times the attention weight and the extent of the tap's own level, W for x and H for y -- next to its
// neighbours', in the coordinate type and in the caller's write mode.
#include "msda_plan.hpp"

namespace mdconv {

namespace {

template <int DT, int CT>
__global__ __launch_bounds__(256) void msda_bwd_coord_kernel(MsdaGeom g, const void *__restrict__ value,
                                                              const void *__restrict__ loc, const void *__restrict__ attn,
                                                              const void *__restrict__ grad_output, void *__restrict__ grad_loc,
                                                              void *__restrict__ grad_attn) {
  constexpr int NV = Dcn3Vec<DT>::NV;
  const Dcn3Lane ln = dcn3_lane_of(g.lgVL, g.npairs);
  const int pair_byte = msda_pair_byte(g, ln.pair);
  const rsrc_t r_val = make_rsrc(value, (size_t)g.N * g.S * g.C * g.esz);
  const rsrc_t r_go = make_rsrc(grad_output, (size_t)g.npairs * g.D * g.esz);
  const unsigned go_row = (unsigned)ln.pair * (unsigned)g.V * 16u;   // the pair's channel row of grad_output
  float go0[NV];   // the first round's vector (the only one unless a head has more than 64 vectors)
  dcn3_unpack<DT>(buf_load4(r_go, ln.live && ln.j < g.V ? (int)(go_row + (unsigned)ln.j * 16u) : kDcn3Oob, 0), go0);
  for (int t0 = 0; t0 < g.K; t0 += g.VL) {
    const int my_tap = t0 + ln.j;
    const bool my_on = ln.live && my_tap < g.K;
    Dcn3Tap mine;
    int H, W;   // of my_tap's level
    msda_build_tap<CT>(g, pair_byte, ln.pair, my_tap, my_on, loc, attn, mine, H, W);
    float r_m = 0.f, r_x = 0.f, r_y = 0.f;   // the sums of my_tap
    const int nt = min(g.VL, g.K - t0);
    for (int jj = 0; jj < nt; ++jj) {
      const Dcn3Tap t = g.VL > 1 ? dcn3_tap_from(mine, ln.first + jj) : mine;
      float s_m = 0.f, s_x = 0.f, s_y = 0.f;
      for (int rd = 0; rd < g.rounds; ++rd) {
        const int v = rd * g.VL + ln.j;
        const bool on = ln.live && v < g.V;
        const unsigned vbyte = on ? (unsigned)v * 16u : (unsigned)kDcn3Oob;
        float go[NV];
        if (rd == 0) {
#pragma unroll
          for (int i = 0; i < NV; ++i) go[i] = go0[i];
        } else {
          dcn3_unpack<DT>(buf_load4(r_go, (int)min(go_row + vbyte, (unsigned)kDcn3Oob), 0), go);
        }
        float4 raw[4];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) raw[ci] = buf_load4(r_val, (int)min((unsigned)t.off[ci] + vbyte, (unsigned)kDcn3Oob), 0);
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          float x[NV];
          dcn3_unpack<DT>(raw[ci], x);
          float dot = 0.f;
#pragma unroll
          for (int i = 0; i < NV; ++i) dot = fmaf(go[i], x[i], dot);
          s_m = fmaf(dcn3_corner_weight(t.lx, t.ly, ci), dot, s_m);
          s_x = fmaf(dcn3_corner_dx(t.ly, ci), dot, s_x);
          s_y = fmaf(dcn3_corner_dy(t.lx, ci), dot, s_y);
        }
      }
      for (int d = g.VL >> 1; d >= 1; d >>= 1) {
        s_m += __shfl_xor(s_m, d, 64);
        s_x += __shfl_xor(s_x, d, 64);
        s_y += __shfl_xor(s_y, d, 64);
      }
      if (jj == ln.j) {   // t is `mine`
        r_m = s_m;
        r_x = s_x * (t.m * (float)W);
        r_y = s_y * (t.m * (float)H);
      }
    }
    if (my_on) {
      const int e = ln.pair * g.K + my_tap;
      dcn3_st<CT>(grad_attn, e, r_m, g.acc != 0);
      dcn3_st<CT>(grad_loc, 2 * e, r_x, g.acc != 0);
      dcn3_st<CT>(grad_loc, 2 * e + 1, r_y, g.acc != 0);
    }
  }
}

}  // namespace

int msda_bwd_coord_launch(const MsdaPlan &p, const MsdaTensors &t, hipStream_t stream) {
  const MsdaGeom &g = p.g;
  const dim3 grid(msda_grid(g, g.npairs));
#define MSDA_BWD(DT, CT)                                                                                                  \
  hipLaunchKernelGGL((msda_bwd_coord_kernel<DT, CT>), grid, dim3(256), 0, stream, g, t.value, t.loc, t.attn, t.grad_output, \
                     t.grad_loc, t.grad_attn)
  MSDA_DISPATCH(p, MSDA_BWD);
#undef MSDA_BWD
  return check_launch("msda_bwd_coord");
}

}  // namespace mdconv
