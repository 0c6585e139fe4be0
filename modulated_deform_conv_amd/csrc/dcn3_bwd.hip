// dcn3_bwd.hip -- grad_offset and grad_mask of the DCNv3 core operator (dcn3_plan.hpp), without atomics.
//
// The lane mapping and the tap walk of the forward (dcn3_fwd.hip): lane = one 16-byte channel vector of one (output pixel,
// group) pair, the VL lanes of a pair build VL taps at once and walk them together.  Per (pair, tap) a lane takes the dot
// products of its grad_output vector with the four corner vectors in-lane, weighs them three ways -- the bilinear weights
// (grad_mask), their derivatives along x and along y (grad_offset) -- and the three sums over the pair's lanes are taken
// by an xor butterfly inside the wave: a fixed order, every lane ends with the same bits.  Lane j keeps the sums of tap
// t0 + j, so after VL taps each lane stores one mask gradient and one (x, y) pair, next to its neighbours', in the
// caller's write mode.
#include "dcn3_plan.hpp"

namespace mdconv {

namespace {

template <int DT>
__global__ __launch_bounds__(256) void dcn3_bwd_coord_kernel(Dcn3Geom g, const void *__restrict__ input,
                                                              const void *__restrict__ offset, const void *__restrict__ mask,
                                                              const void *__restrict__ grad_output, void *__restrict__ grad_offset,
                                                              void *__restrict__ grad_mask) {
  constexpr int NV = Dcn3Vec<DT>::NV;
  const Dcn3Lane ln = dcn3_lane(g, g.N * g.G);
  const Dcn3Pix px = dcn3_pix(g, ln.pair);
  const rsrc_t r_in = make_rsrc(input, (size_t)g.B * g.S_i * g.C * g.esz);
  const rsrc_t r_go = make_rsrc(grad_output, (size_t)g.N * g.C * g.esz);
  const unsigned go_row = (unsigned)ln.pair * (unsigned)g.V * 16u;   // the pair's channel row of grad_output
  float go0[NV];   // the first round's vector (the only one unless a group has more than 64 vectors)
  dcn3_unpack<DT>(buf_load4(r_go, ln.live && ln.j < g.V ? (int)(go_row + (unsigned)ln.j * 16u) : kDcn3Oob, 0), go0);
  for (int t0 = 0; t0 < g.K; t0 += g.VL) {
    const int my_tap = t0 + ln.j;
    const bool my_on = ln.live && my_tap < g.K;
    Dcn3Tap mine;
    dcn3_build_tap<DT>(g, px, ln.pair, my_tap, my_on, offset, mask, mine);
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
        for (int ci = 0; ci < 4; ++ci) raw[ci] = buf_load4(r_in, (int)min((unsigned)t.off[ci] + vbyte, (unsigned)kDcn3Oob), 0);
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
      if (jj == ln.j) {
        const float ms = t.m * g.scale;
        r_m = s_m;
        r_x = s_x * ms;
        r_y = s_y * ms;
      }
    }
    if (my_on) {
      const int e = ln.pair * g.K + my_tap;
      dcn3_st<DT>(grad_mask, e, r_m, g.acc != 0);
      dcn3_st<DT>(grad_offset, 2 * e, r_x, g.acc != 0);
      dcn3_st<DT>(grad_offset, 2 * e + 1, r_y, g.acc != 0);
    }
  }
}

}  // namespace

int dcn3_bwd_coord_launch(const Dcn3Plan &p, const Dcn3Tensors &t, hipStream_t stream) {
  const Dcn3Geom &g = p.g;
  const dim3 grid(dcn3_grid(g, (int64_t)g.N * g.G));
#define DCN3_BWD(DT)                                                                                                  \
  hipLaunchKernelGGL((dcn3_bwd_coord_kernel<DT>), grid, dim3(256), 0, stream, g, t.input, t.offset, t.mask, t.grad_output, \
                     t.grad_offset, t.grad_mask)
  if (p.dtype == MDCONV_F32) DCN3_BWD(MDCONV_F32);
  else if (p.dtype == MDCONV_F16) DCN3_BWD(MDCONV_F16);
  else DCN3_BWD(MDCONV_BF16);
#undef DCN3_BWD
  return check_launch("dcn3_bwd_coord");
}

}  // namespace mdconv
