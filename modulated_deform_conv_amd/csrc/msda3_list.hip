// msda3_list.hip -- the scatter lists of grad_value of 3-D multi-scale deformable attention (msda3_plan.hpp): the callable of
// scatter_lists_build, counting or filling.  The gather over them is samp_gather_kernel (samp_gather.hip) as it stands, with
// N images of S rows and M heads of D channels.
//
// Thread = sample id = pair * K + tap, the element index of attention_weights and a third of the location's, so both tensors
// are read coalesced.  Per corner the forward reads (msda3_sample: up to eight) one 16-byte entry {tap * Lq + q, corner
// weight x attention weight, tap, q} goes to the list of value row start_l + (z * H_l + y) * W_l + x in the segment of
// (image, head), over all S rows of the concatenated levels; a sample reaches a row through one corner, so word 0 is unique
// inside a list (the order csr_sort_rows fixes).  A gated-out sample emits nothing.
#include "msda3_plan.hpp"

namespace mdconv {

namespace {

template <int CT, bool FILL>
__global__ __launch_bounds__(256) void msda3_list_kernel(Msda3Geom g, const void *__restrict__ loc, const void *__restrict__ attn,
                                                          int *__restrict__ cnt, const int *__restrict__ rowptr,
                                                          int4 *__restrict__ entries, int64_t seg_stride) {
  const int total = g.npairs * g.K;   // elements of attention_weights: below 2^30
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const int pair = id / g.K, tap = id - pair * g.K;
  const int nq = pair / g.M, m = pair - nq * g.M;
  const int n = nq / g.Lq, q = nq - n * g.Lq;
  const int seg = n * g.M + m;
  const float f = FILL ? samp_ld<CT>(attn, id) : 1.f;
  int T, H, W, start;
  msda3_level(g, tap / g.P, T, H, W, start);
  Msda3Sample s;
  msda3_position<CT>(loc, 3 * id, T, H, W, s);
  const int row0 = start + (s.z0 * H + s.y0) * W + s.x0;   // (may lie before the level; a corner that is read does not)
#pragma unroll
  for (int ci = 0; ci < 8; ++ci) {
    if (!((s.read >> ci) & 1u)) continue;
    const int row = row0 + msda3_corner_step(ci, H, W);
    int *c = cnt + (int64_t)seg * g.S + row;
    if (!FILL) {
      atomicAdd(c, 1);
    } else {
      const int slot = rowptr[(int64_t)seg * (g.S + 1) + row] + atomicSub(c, 1) - 1;
      entries[(int64_t)seg * seg_stride + slot] =
          make_int4(tap * g.Lq + q, __float_as_int(msda3_corner_weight(s.lx, s.ly, s.lz, ci) * f), tap, q);
    }
  }
}

}  // namespace

void msda3_list_launch(const Msda3Plan &p, const Msda3Tensors &t, bool fill, int *cnt, const int *rowptr, void *entries,
                       hipStream_t stream) {
  const Msda3Geom &g = p.g;
  const int64_t stride = p.lists.seg_stride;
  const dim3 grid((unsigned)(((int64_t)g.npairs * g.K + 255) / 256));
#define MSDA3_LIST(CT)                                                                                                   \
  do {                                                                                                                   \
    if (fill)                                                                                                            \
      hipLaunchKernelGGL((msda3_list_kernel<CT, true>), grid, dim3(256), 0, stream, g, t.loc, t.attn, cnt, rowptr,        \
                         (int4 *)entries, stride);                                                                       \
    else                                                                                                                 \
      hipLaunchKernelGGL((msda3_list_kernel<CT, false>), grid, dim3(256), 0, stream, g, t.loc, t.attn, cnt, rowptr,       \
                         (int4 *)entries, stride);                                                                       \
  } while (0)
  if (p.coord_dtype == MDCONV_F32) MSDA3_LIST(MDCONV_F32);   // (by coordinate type: three instances)
  else if (p.coord_dtype == MDCONV_F16) MSDA3_LIST(MDCONV_F16);
  else MSDA3_LIST(MDCONV_BF16);
#undef MSDA3_LIST
}

}  // namespace mdconv
