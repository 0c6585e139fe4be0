// dagg_gather.hip -- grad_feature of deformable aggregation (dagg_plan.hpp), without floating-point atomics: the scatter of
// the published operator inverted into lists (scatter_lists_build with dagg_list_kernel), then this gather.
//
// Lane = one 16-byte channel vector of one feature row (image, row): the anchor mapping of the forward with the feature row
// as the owner.  A lane walks its row's list once; per entry {id, corner weight, 0 (padding), anchor} it loads the weight of
// its own group, weights[id * G + g], and one 16-byte vector of the anchor's grad_output row -- contiguous across the row's
// lanes --, accumulates in fp32 and stores 16 bytes in the caller's mode.  A row that no sample touches is written as zeros
// in overwrite mode and is neither read nor written in accumulate mode (so it keeps its bits, a -0.0 included, and most rows
// of a call are such rows).  In deterministic mode the lists are sorted; without it the order of a list is the order its
// integer atomics arrived in, and the gradient agrees from call to call to rounding.
#include "dagg_plan.hpp"

namespace mdconv {

namespace {

template <int DT, int CT>
__global__ __launch_bounds__(256) void dagg_gather_kernel(DaggGeom g, int64_t seg_stride, const void *__restrict__ grad_output,
                                                           const void *__restrict__ wts, const int *__restrict__ rowptr,
                                                           const int4 *__restrict__ entries, void *__restrict__ grad_feature) {
  constexpr int NV = SampVec<DT>::NV;
  const SampLane ln = samp_lane_of(g.ln.lgVL, g.B * g.S);   // pair = b * S + row
  const int b = ln.pair / g.S, r = ln.pair - b * g.S;
  const int *rp = rowptr + (int64_t)b * (g.S + 1) + r;
  const int e0 = rp[0], e1 = ln.live ? rp[1] : e0;
  if (g.acc && e0 == e1) return;   // an empty list adds nothing: the row stays as it is
  const int4 *ent = entries + (int64_t)b * seg_stride;
  const rsrc_t r_go = make_rsrc(grad_output, (size_t)g.nanchors * g.C * g.ln.esz);
  const unsigned row_bytes = (unsigned)(g.C * g.ln.esz);
  for (int rd = 0; rd < g.ln.rounds; ++rd) {   // one round unless a row has more than 64 vectors
    const int v = rd * g.ln.VL + ln.j;
    if (!(ln.live && v < g.ln.V)) continue;
    const int grp = v / g.VG;
    const unsigned vbyte = (unsigned)v * 16u;
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    for (int e = e0; e < e1; ++e) {
      const int4 en = ent[e];
      const float w = __int_as_float(en.y) * samp_ld<CT>(wts, en.x * g.G + grp);
      float x[NV];
      samp_unpack<DT>(buf_load4(r_go, (int)((unsigned)en.w * row_bytes + vbyte), 0), x);
#pragma unroll
      for (int i = 0; i < NV; ++i) acc[i] = fmaf(w, x[i], acc[i]);
    }
    float4 *dst = (float4 *)grad_feature + (int64_t)ln.pair * g.ln.V + v;
    if (g.acc) {
      float old[NV];
      samp_unpack<DT>(*dst, old);
#pragma unroll
      for (int i = 0; i < NV; ++i) acc[i] += old[i];
    }
    *dst = samp_pack<DT>(acc);
  }
}

}  // namespace

int dagg_gather_launch(const DaggPlan &p, const DaggTensors &t, const int *rowptr, const void *entries, hipStream_t stream) {
  const DaggGeom &g = p.g;
  const dim3 grid(samp_grid(g.ln.lgVL, (int64_t)g.B * g.S));
  const int64_t stride = p.lists.seg_stride;
#define DAGG_GATHER(DT, CT)                                                                                        \
  hipLaunchKernelGGL((dagg_gather_kernel<DT, CT>), grid, dim3(256), 0, stream, g, stride, t.grad_output, t.wts, rowptr, \
                     (const int4 *)entries, t.grad_feature)
  SAMP_DISPATCH(p, DAGG_GATHER);
#undef DAGG_GATHER
  return check_launch("dagg_gather");
}

}  // namespace mdconv
