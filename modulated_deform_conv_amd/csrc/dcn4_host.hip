// dcn4_host.hip -- plan and execution of the DCNv4 operator (dcn4_plan.hpp): the sampling core's kernels (samp_core.hpp)
// instantiated with Dcn4Op -- and, for MDCONV_FLAG_SOFTMAX, with Dcn4SoftOp --, offset_mask in the values' type or in fp32.
// offset_mask is both the core's `coord` and its `factor`, grad_offset_mask both gradient tensors; the gather is the one
// every sampling operator shares.
#include "dcn4_plan.hpp"

namespace mdconv {

// the five (value type, coordinate type) pairings: `call(DT, CT)` for the plan's
#define DCN4_DISPATCH(p, call)                                                       \
  do {                                                                               \
    if ((p).dtype == MDCONV_F32) call(MDCONV_F32, MDCONV_F32);                       \
    else if ((p).dtype == MDCONV_F16 && (p).coord_dtype == MDCONV_F16) call(MDCONV_F16, MDCONV_F16); \
    else if ((p).dtype == MDCONV_F16) call(MDCONV_F16, MDCONV_F32);                  \
    else if ((p).coord_dtype == MDCONV_BF16) call(MDCONV_BF16, MDCONV_BF16);         \
    else call(MDCONV_BF16, MDCONV_F32);                                              \
  } while (0)
// the list kernels depend on the coordinate type alone
#define DCN4_DISPATCH_CT(p, call)                              \
  do {                                                         \
    if ((p).coord_dtype == MDCONV_F32) call(MDCONV_F32);       \
    else if ((p).coord_dtype == MDCONV_F16) call(MDCONV_F16);  \
    else call(MDCONV_BF16);                                    \
  } while (0)

bool dcn4_plan(const mdconv_dcnv4_desc *d, bool backward, Dcn4Plan *p, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = nullptr;
  const int64_t lim = (int64_t)1 << 31;
  const int esz = d->dtype == MDCONV_F32 ? 4 : 2, csz = d->coord_dtype == MDCONV_F32 ? 4 : 2;
  const int64_t Ho = (d->in_sz[0] + 2 * (int64_t)d->pad[0] - ((int64_t)d->dil[0] * (d->k_sz[0] - 1) + 1)) / d->stride[0] + 1;
  const int64_t Wo = (d->in_sz[1] + 2 * (int64_t)d->pad[1] - ((int64_t)d->dil[1] * (d->k_sz[1] - 1) + 1)) / d->stride[1] + 1;
  const int64_t grid = (int64_t)d->k_sz[0] * d->k_sz[1];
  const int64_t K = grid - (d->remove_center ? 1 : 0);
  const int64_t C = (int64_t)d->groups * d->group_channels;
  const int64_t S_i = (int64_t)d->in_sz[0] * d->in_sz[1], S_o = Ho * Wo;
  const bool skip_input = backward && (d->flags & MDCONV_FLAG_NO_GRAD_INPUT);
  const int64_t seg_stride = K * S_o * 4;
  // (each product is checked with its factors bounded by the checks before it, so none overflows 64 bits; the row length
  // is formed for K <= 4096 only and stays below 2^45)
  const int64_t OM = K > 4096 ? 0 : dcn4_row_len(d->groups, K);
  if (esz == 4 && d->group_channels % 4) *why = "group_channels is not a multiple of 4 (fp32 rows of 16 bytes)";
  else if (esz == 2 && d->group_channels % 8) *why = "group_channels is not a multiple of 8 (16-bit rows of 16 bytes)";
  else if (K > 4096) *why = "the kernel has more than 4096 taps";
  else if (C >= lim || S_i >= lim || S_o >= lim || d->batch * S_i >= lim || d->batch * S_o >= lim ||
           d->batch * S_i * C >= lim / esz || d->batch * S_o * C >= lim / esz ||
           d->batch * S_o * d->groups >= lim || OM >= lim || d->batch * S_o * OM >= lim / csz)
    *why = "a tensor of the call has 2^31 bytes or more";
  else if (backward && !skip_input && (seg_stride >= lim || (int64_t)d->batch * d->groups > 65535))
    *why = "batch * groups exceeds 65535 or K * output pixels * 4 reaches 2^31 (the scatter lists of grad_input)";
  if (*why) return false;

  Dcn4Plan q = {};
  Dcn4Geom &g = q.g;
  g.B = d->batch; g.G = d->groups; g.D = d->group_channels; g.C = (int)C; g.K = (int)K;
  g.H = d->in_sz[0]; g.W = d->in_sz[1]; g.Ho = (int)Ho; g.Wo = (int)Wo; g.kh = d->k_sz[0]; g.kw = d->k_sz[1];
  g.sh = d->stride[0]; g.sw = d->stride[1]; g.ph = d->pad[0]; g.pw = d->pad[1]; g.dh = d->dil[0]; g.dw = d->dil[1];
  g.ch = (g.dh * (g.kh - 1)) >> 1;
  g.cw = (g.dw * (g.kw - 1)) >> 1;
  g.S_i = (int)S_i; g.S_o = (int)S_o; g.N = (int)(d->batch * S_o);
  g.ln = samp_lanes(g.D, esz);
  g.scale = d->offset_scale;
  g.acc = d->accumulate;
  g.OM = (int)OM;
  g.K3 = (int)(3 * K);
  g.center = d->remove_center ? (int)((grid - 1) / 2) : (int)K;
  q.dtype = d->dtype;
  q.coord_dtype = d->coord_dtype;
  q.backward = backward;
  q.det = backward && (d->flags & MDCONV_FLAG_DETERMINISTIC);
  q.skip_input = skip_input;
  q.softmax = (d->flags & MDCONV_FLAG_SOFTMAX) != 0;
  q.off_stats = 0;
  q.total = 0;
  if (backward && !skip_input) {
    Bump ws;
    q.lists = scatter_lists_take(ws, g.B * g.G, g.S_i, seg_stride, q.det);
    // (fda_plan's rule: the list kernels take a tap's weight from the statistics the coordinate kernel stored)
    if (q.softmax) q.off_stats = ws.take((size_t)Dcn4Op::npairs(g) * sizeof(float2));
    q.total = ws.off;
  }
  *p = q;
  return true;
}

// the geometry of the softmax kernels: the plan's, and where the statistics go (nullptr: nobody will read them)
static Dcn4SoftGeom dcn4_soft_geom(const Dcn4Plan &p, void *stats) {
  Dcn4SoftGeom g;
  (Dcn4Geom &)g = p.g;
  g.stats = (float2 *)stats;
  return g;
}

static int dcn4_soft_backward(const Dcn4Plan &p, const Dcn4Tensors &t, void *ws, hipStream_t stream) {
  const ScatterLists &L = p.lists;
  int rc;
  // (the coordinate kernel stores the pairs' softmax statistics for the list kernels, which run behind it on the stream)
  const Dcn4SoftGeom g = dcn4_soft_geom(p, p.skip_input ? nullptr : (char *)ws + p.off_stats);
#define DCN4_BWD(DT, CT)                                                                                             \
  samp_bwd_coord_launch<Dcn4SoftOp, DT, CT>(g, t.input, t.offset_mask, t.offset_mask, t.grad_output, t.grad_offset_mask, \
                                            t.grad_offset_mask, stream)
  DCN4_DISPATCH(p, DCN4_BWD);
#undef DCN4_BWD
  if ((rc = check_launch("dcn4_soft_bwd_coord"))) return rc;
  if (p.skip_input) return MDCONV_OK;
  rc = scatter_lists_build(L, ws, p.det, stream, [&](bool fill, int *cnt, const int *rowptr, void *entries) {
#define DCN4_LIST(CT) \
  samp_list_launch<Dcn4SoftOp, CT>(g, fill, t.offset_mask, t.offset_mask, cnt, rowptr, entries, L.seg_stride, stream)
    DCN4_DISPATCH_CT(p, DCN4_LIST);
#undef DCN4_LIST
  });
  if (rc) return rc;
  const SampGather ga = {g.B, g.S_i, g.S_o, g.G, g.D, g.C, g.ln, g.acc};
  return samp_gather_launch(ga, p.dtype, L.seg_stride, t.grad_output, (const int *)((char *)ws + L.off_rowptr),
                            (char *)ws + L.off_entries, t.grad_input, stream);
}

int dcn4_forward(const Dcn4Plan &p, const Dcn4Tensors &t, hipStream_t stream) {
  if (p.softmax) {
    const Dcn4SoftGeom sg = dcn4_soft_geom(p, nullptr);
#define DCN4_FWD(DT, CT) samp_fwd_launch<Dcn4SoftOp, DT, CT>(sg, t.input, t.offset_mask, t.offset_mask, t.output, stream)
    DCN4_DISPATCH(p, DCN4_FWD);
#undef DCN4_FWD
    return check_launch("dcn4_soft_fwd");
  }
#define DCN4_FWD(DT, CT) samp_fwd_launch<Dcn4Op, DT, CT>(p.g, t.input, t.offset_mask, t.offset_mask, t.output, stream)
  DCN4_DISPATCH(p, DCN4_FWD);
#undef DCN4_FWD
  return check_launch("dcn4_fwd");
}

int dcn4_backward(const Dcn4Plan &p, const Dcn4Tensors &t, void *ws, hipStream_t stream) {
  if (p.softmax) return dcn4_soft_backward(p, t, ws, stream);
  const Dcn4Geom &g = p.g;
  const ScatterLists &L = p.lists;
  int rc;
  // (the coordinate kernel also zeroes the padding columns of grad_offset_mask in overwrite mode: Dcn4Op::finish_pair)
#define DCN4_BWD(DT, CT)                                                                                         \
  samp_bwd_coord_launch<Dcn4Op, DT, CT>(g, t.input, t.offset_mask, t.offset_mask, t.grad_output, t.grad_offset_mask, \
                                        t.grad_offset_mask, stream)
  DCN4_DISPATCH(p, DCN4_BWD);
#undef DCN4_BWD
  if ((rc = check_launch("dcn4_bwd_coord"))) return rc;
  if (p.skip_input) return MDCONV_OK;
  rc = scatter_lists_build(L, ws, p.det, stream, [&](bool fill, int *cnt, const int *rowptr, void *entries) {
#define DCN4_LIST(CT) \
  samp_list_launch<Dcn4Op, CT>(g, fill, t.offset_mask, t.offset_mask, cnt, rowptr, entries, L.seg_stride, stream)
    DCN4_DISPATCH_CT(p, DCN4_LIST);
#undef DCN4_LIST
  });
  if (rc) return rc;
  const SampGather ga = {g.B, g.S_i, g.S_o, g.G, g.D, g.C, g.ln, g.acc};
  return samp_gather_launch(ga, p.dtype, L.seg_stride, t.grad_output, (const int *)((char *)ws + L.off_rowptr),
                            (char *)ws + L.off_entries, t.grad_input, stream);
}

}  // namespace mdconv
