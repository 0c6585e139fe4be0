// dw_fwd.hip -- forward of the depthwise family (dw_plan.hpp).
//
// Lane = output pixel (the NCHW offset, mask and output streams are coalesced along pixels), workgroup = 256 pixels x a slab
// of CS channels inside one deformable group.  Taps outside, channels inside: the sampling state of a tap is built once per
// lane and reused by every channel of the slab; a sample costs 2^(nd-1) pair loads (PairLoad of direct_kernels.hip: the two
// neighbours along the contiguous axis in one 8-byte load, the element the reference does not read selected away).  The
// K x M weights of a channel are wave-uniform: they come from scalar loads.  No workspace, no LDS.
#include "dw_plan.hpp"
#include "mfma_tile.hpp"   // raw buffer loads

namespace mdconv {

namespace {

template <int ND, int M, int CS>
__global__ __launch_bounds__(256) void dw_fwd_kernel(Geom g, const float *__restrict__ input, const float *__restrict__ weight,
                                                      const float *__restrict__ bias, const float *__restrict__ offset,
                                                      const float *__restrict__ mask, float *__restrict__ output) {
  constexpr int NP = 1 << (ND - 1);
  const int n_raw = blockIdx.x * 256 + threadIdx.x;
  const bool live = n_raw < g.N;
  const int n = live ? n_raw : g.N - 1;
  const int b = n / g.S_o;
  const int pix = n - b * g.S_o;
  const int c0 = blockIdx.y * CS;   // CS divides C_in / deformable_groups: the slab lies inside one deformable group
  const int dg = c0 / g.Cdg;
  int o[ND];
  out_coords<ND>(g, pix, o);
  const bool pair = g.in_sz[ND - 1] >= 2;
  const rsrc_t r_in = make_rsrc(input, (size_t)g.B * g.C * g.S_i * sizeof(float));

  float acc[CS][M];
#pragma unroll
  for (int cc = 0; cc < CS; ++cc)
#pragma unroll
    for (int m = 0; m < M; ++m) acc[cc][m] = 0.f;

  const int64_t obase = ((int64_t)(b * g.DG + dg) * (ND * g.K)) * g.S_o + pix;
  const int64_t mbase = ((int64_t)(b * g.DG + dg) * g.K) * g.S_o + pix;
  for (int tap = 0; tap < g.K; ++tap) {
    float delta[ND];
#pragma unroll
    for (int a = 0; a < ND; ++a) delta[a] = offset[obase + (int64_t)(ND * tap + a) * g.S_o];
    const float mk = g.modulated ? mask[mbase + (int64_t)tap * g.S_o] : 1.f;
    int t[ND];
    tap_coords<ND>(g, tap, t);
    TapCoef<ND, float> tc;
    make_tap<ND, float>(g, o, t, delta, false, tc);
    if (pair) {
      int pidx[NP];
      float px[NP], py[NP];
      bool prx[NP], pry[NP];
      make_pairs<ND, float>(g, tc, mk, pidx, px, py);   // mask folded into the weights
      make_pairs_read<ND, float>(g, tc, prx, pry);
#pragma unroll
      for (int cc = 0; cc < CS; ++cc) {
        const int c = c0 + cc;
        const unsigned plane_off = (unsigned)(b * g.C + c) * (unsigned)g.S_i;
        float val = 0.f;
#pragma unroll
        for (int pi = 0; pi < NP; ++pi) {
          const float2 v = buf_load2(r_in, (int)((plane_off + (unsigned)pidx[pi]) * 4u), 0);
          // an element the reference never reads (weight 0) must not turn a non-finite neighbour into NaN
          val += (prx[pi] ? px[pi] * v.x : 0.f) + (pry[pi] ? py[pi] * v.y : 0.f);
        }
#pragma unroll
        for (int m = 0; m < M; ++m) acc[cc][m] = fmaf(weight[(int64_t)(c * M + m) * g.K + tap], val, acc[cc][m]);
      }
    } else {   // a last axis of one element: corner by corner
#pragma unroll
      for (int cc = 0; cc < CS; ++cc) {
        const int c = c0 + cc;
        const float *plane = input + (int64_t)(b * g.C + c) * g.S_i;
        float val = 0.f;
#pragma unroll
        for (int ci = 0; ci < (1 << ND); ++ci)
          if (corner_is_read<ND, float>(tc, ci)) val += corner_weight<ND, float>(tc, ci) * plane[corner_index<ND, float>(tc, ci)];
        val *= mk;
#pragma unroll
        for (int m = 0; m < M; ++m) acc[cc][m] = fmaf(weight[(int64_t)(c * M + m) * g.K + tap], val, acc[cc][m]);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int cc = 0; cc < CS; ++cc)
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int och = (c0 + cc) * M + m;
      const float bv = g.with_bias ? bias[och] : 0.f;
      output[(int64_t)(b * g.O + och) * g.S_o + pix] = acc[cc][m] + bv;
    }
}

template <int ND, int M>
int launch_cs(const DwPlan &p, const Tensors &t, hipStream_t stream) {
  const Geom &g = p.g;
  const dim3 grid((g.N + 255) / 256, g.C / p.cs);
#define DW_FWD(CS)                                                                                                   \
  hipLaunchKernelGGL((dw_fwd_kernel<ND, M, CS>), grid, dim3(256), 0, stream, g, (const float *)t.input,              \
                     (const float *)t.weight, (const float *)t.bias, (const float *)t.offset, (const float *)t.mask, \
                     (float *)t.output)
  if (p.cs == 8) DW_FWD(8); else DW_FWD(4);
#undef DW_FWD
  return check_launch("dw_fwd");
}
template <int ND>
int launch_m(const DwPlan &p, const Tensors &t, hipStream_t stream) {
  switch (p.M) {
    case 1: return launch_cs<ND, 1>(p, t, stream);
    case 2: return launch_cs<ND, 2>(p, t, stream);
    case 3: return launch_cs<ND, 3>(p, t, stream);
    default: return launch_cs<ND, 4>(p, t, stream);
  }
}

}  // namespace

int dw_fwd_launch(const DwPlan &p, const Tensors &t, hipStream_t stream) {
  return p.g.nd == 2 ? launch_m<2>(p, t, stream) : launch_m<3>(p, t, stream);
}

}  // namespace mdconv
