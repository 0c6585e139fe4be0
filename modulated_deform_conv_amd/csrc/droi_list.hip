// droi_list.hip -- the scatter lists of grad_input of deformable RoI pooling (droi_plan.hpp): the callable of
// scatter_lists_build, counting or filling.  The gather over them is samp_gather_kernel (samp_gather.hip) as it stands, with
// one image of B*H*W rows and one head of C channels.
//
// Thread = sample id over R*PH*PW * gcap * gcap: id = (bin * gcap + iy) * gcap + ix.  A sample beyond the RoI's own grid, one
// the gate drops and every sample of a RoI that contributes nothing emit nothing.  Per corner the forward reads one 16-byte
// entry {sample id, weight / cnt, unused, bin} goes to the list of row b*H*W + y*W + x, in ONE segment of B*H*W rows; a
// sample reaches a row through one corner, so word 0 is unique inside a list (the order csr_sort_rows fixes).
#include "droi_plan.hpp"

namespace mdconv {

namespace {

template <int CT, bool FILL>
__global__ __launch_bounds__(256) void droi_list_kernel(DroiGeom g, const float *__restrict__ rois, const void *__restrict__ offset,
                                                         int *__restrict__ cnt, const int *__restrict__ rowptr,
                                                         int4 *__restrict__ entries) {
  const int per_bin = g.gcap * g.gcap;
  const int total = g.nbins * per_bin;   // below 2^29 (the plan's rule)
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const int bin = id / per_bin, rem = id - bin * per_bin;
  const int iy = rem / g.gcap, ix = rem - iy * g.gcap;
  DroiBin bn;
  droi_bin<CT>(g, rois, offset, bin, bn);
  if (iy >= bn.gh || ix >= bn.gw) return;
  const DroiAxis ay = droi_axis(bn.y0 + ((float)iy + 0.5f) * bn.sy, g.H);
  const DroiAxis ax = droi_axis(bn.x0 + ((float)ix + 0.5f) * bn.sx, g.W);
  const int row0 = bn.img_row + ay.lo * g.W + ax.lo;
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    if (!droi_corner_read(ay, ax, ci, g.H, g.W)) continue;
    const int row = row0 + (ci >> 1) * g.W + (ci & 1);
    int *c = cnt + row;
    if (!FILL) {
      atomicAdd(c, 1);
    } else {
      const int slot = rowptr[row] + atomicSub(c, 1) - 1;
      entries[slot] = make_int4(id, __float_as_int(samp_corner_weight(ax.l, ay.l, ci) * bn.inv_cnt), 0, bin);
    }
  }
}

}  // namespace

void droi_list_launch(const DroiPlan &p, const DroiTensors &t, bool fill, int *cnt, const int *rowptr, void *entries,
                      hipStream_t stream) {
  const DroiGeom &g = p.g;
  const dim3 grid((unsigned)(((int64_t)g.nbins * g.gcap * g.gcap + 255) / 256));
#define DROI_LIST(CT)                                                                                                   \
  do {                                                                                                                  \
    if (fill)                                                                                                           \
      hipLaunchKernelGGL((droi_list_kernel<CT, true>), grid, dim3(256), 0, stream, g, (const float *)t.rois, t.offset, cnt, \
                         rowptr, (int4 *)entries);                                                                      \
    else                                                                                                                \
      hipLaunchKernelGGL((droi_list_kernel<CT, false>), grid, dim3(256), 0, stream, g, (const float *)t.rois, t.offset, cnt, \
                         rowptr, (int4 *)entries);                                                                      \
  } while (0)
  if (p.coord_dtype == MDCONV_F32) DROI_LIST(MDCONV_F32);   // (by coordinate type: three instances)
  else if (p.coord_dtype == MDCONV_F16) DROI_LIST(MDCONV_F16);
  else DROI_LIST(MDCONV_BF16);
#undef DROI_LIST
}

}  // namespace mdconv
