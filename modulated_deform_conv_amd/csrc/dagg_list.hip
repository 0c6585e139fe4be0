// dagg_list.hip -- the scatter lists of grad_feature of deformable aggregation (dagg_plan.hpp): the callable of
// scatter_lists_build, counting or filling.  The gather over them is dagg_gather_kernel (dagg_gather.hip).
//
// Thread = sample id = (anchor * U + unit) * L + l.  One segment per IMAGE, one list per feature row, SHARED BY ALL GROUPS:
// per corner the forward reads one 16-byte entry {id, corner weight WITHOUT the group weight, 0, anchor} goes to the list
// of row cam * S_cam + start_l + y * W_l + x (word 2 is padding: the list builder's entries are 16 bytes and the gather
// reads words 0, 1 and 3); the gather multiplies by weights[id * G + g] of its lane's group.  That is
// G times fewer entries and G times fewer integer atomics than a segment per (image, group).  A sample reaches a row
// through one corner, so word 0 is unique inside a list (the order csr_sort_rows fixes).  A gated-out unit emits nothing
// and reads nothing but its location.
#include "dagg_plan.hpp"

namespace mdconv {

namespace {

template <int CT, bool FILL>
__global__ __launch_bounds__(256) void dagg_list_kernel(DaggGeom g, const void *__restrict__ loc, int *__restrict__ cnt,
                                                         const int *__restrict__ rowptr, int4 *__restrict__ entries,
                                                         int64_t seg_stride) {
  const int total = g.nanchors * g.U * g.L;   // elements of `weights` / G: below 2^31
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const int au = id / g.L, l = id - au * g.L;
  const DaggUnit u = dagg_unit<CT>(loc, au, true);
  if (!u.in) return;
  const int anchor = au / g.U, unit = au - anchor * g.U;
  const int b = anchor / g.A;
  int H, W, start;
  dagg_level(g, l, H, W, start);
  SampSample s;
  dagg_sample(u, H, W, s);
  const int map_row = (unit % g.cams) * g.S_cam + start;
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    if (!samp_corner_read(s, ci, H, W)) continue;
    const int row = map_row + samp_corner_pixel(s, ci, W);
    int *c = cnt + (int64_t)b * g.S + row;
    if (!FILL) {
      atomicAdd(c, 1);
    } else {
      const int slot = rowptr[(int64_t)b * (g.S + 1) + row] + atomicSub(c, 1) - 1;
      entries[(int64_t)b * seg_stride + slot] = make_int4(id, __float_as_int(samp_corner_weight(s.lx, s.ly, ci)), 0, anchor);
    }
  }
}

}  // namespace

void dagg_list_launch(const DaggPlan &p, const DaggTensors &t, bool fill, int *cnt, const int *rowptr, void *entries,
                      hipStream_t stream) {
  const DaggGeom &g = p.g;
  const int64_t stride = p.lists.seg_stride;
  const dim3 grid((unsigned)(((int64_t)g.nanchors * g.U * g.L + 255) / 256));
#define DAGG_LIST(CT)                                                                                                     \
  do {                                                                                                                    \
    if (fill)                                                                                                             \
      hipLaunchKernelGGL((dagg_list_kernel<CT, true>), grid, dim3(256), 0, stream, g, t.loc, cnt, rowptr, (int4 *)entries, \
                         stride);                                                                                         \
    else                                                                                                                  \
      hipLaunchKernelGGL((dagg_list_kernel<CT, false>), grid, dim3(256), 0, stream, g, t.loc, cnt, rowptr, (int4 *)entries, \
                         stride);                                                                                         \
  } while (0)
  if (p.coord_dtype == MDCONV_F32) DAGG_LIST(MDCONV_F32);   // (by coordinate type: three instances)
  else if (p.coord_dtype == MDCONV_F16) DAGG_LIST(MDCONV_F16);
  else DAGG_LIST(MDCONV_BF16);
#undef DAGG_LIST
}

}  // namespace mdconv
