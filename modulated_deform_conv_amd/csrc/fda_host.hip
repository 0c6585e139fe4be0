// fda_host.hip -- plan and execution of packed deformable attention (fda_plan.hpp): the sampling core's kernels
// (samp_core.hpp) instantiated with FdaOp for the five (value type, coordinate type) pairings.  sampling_loc_attn is both the
// core's `coord` and its `factor`, grad_sampling_loc_attn both gradient tensors; the gather is the one every sampling
// operator shares.  The operator's C entry points (include/mdconv.h) follow, on the entry-point layer of samp_api.hpp.
#include "fda_plan.hpp"
#include "samp_api.hpp"

namespace mdconv {

bool fda_plan(const mdconv_fda_desc *d, bool backward, FdaPlan *p, const char **why) {
  // the geometry, the shape rule and the lists are MSDA's for the same fields
  mdconv_msda_desc md = {};
  md.dtype = d->dtype; md.coord_dtype = d->coord_dtype;
  md.batch = d->batch; md.heads = d->heads; md.head_channels = d->head_channels;
  md.queries = d->queries; md.levels = d->levels; md.points = d->points;
  for (int l = 0; l < MDCONV_MSDA_MAX_LEVELS; ++l) {
    md.level_sz[l][0] = d->level_sz[l][0];
    md.level_sz[l][1] = d->level_sz[l][1];
  }
  md.accumulate = d->accumulate; md.flags = d->flags;
  MsdaPlan m;
  if (!msda_plan(&md, backward, &m, why)) return false;
  // ... plus the packed tensor, half again as large as sampling_locations (which passed: the product stays below 2^33)
  if ((int64_t)m.g.npairs * m.g.K * 3 * (int64_t)dtype_bytes(d->coord_dtype) >= (int64_t)1 << 31) {
    *why = "a tensor of the call has 2^31 bytes or more";
    return false;
  }
  FdaPlan q = {};
  (MsdaGeom &)q.g = m.g;
  q.g.K3 = 3 * m.g.K;
  q.g.stats = nullptr;
  q.dtype = m.dtype;
  q.coord_dtype = m.coord_dtype;
  q.backward = backward;
  q.det = m.det;
  q.skip_value = m.skip_value;
  q.lists = m.lists;
  q.off_stats = 0;
  q.total = 0;
  if (backward && !q.skip_value) {
    Bump ws;
    ws.off = m.total;
    q.off_stats = ws.take((size_t)m.g.npairs * sizeof(float2));
    q.total = ws.off;
  }
  *p = q;
  return true;
}

int fda_forward(const FdaPlan &p, const FdaTensors &t, hipStream_t stream) {
#define FDA_FWD(DT, CT) samp_fwd_launch<FdaOp, DT, CT>(p.g, t.value, t.loc_attn, t.loc_attn, t.output, stream)
  SAMP_DISPATCH(p, FDA_FWD);
#undef FDA_FWD
  return check_launch("fda_fwd");
}

int fda_backward(const FdaPlan &p, const FdaTensors &t, void *ws, hipStream_t stream) {
  FdaGeom g = p.g;
  const ScatterLists &L = p.lists;
  int rc;
  // (the coordinate kernel stores the pairs' softmax statistics for the list kernels, which run behind it on the stream)
  g.stats = p.skip_value ? nullptr : (float2 *)((char *)ws + p.off_stats);
#define FDA_BWD(DT, CT)                                                                                              \
  samp_bwd_coord_launch<FdaOp, DT, CT>(g, t.value, t.loc_attn, t.loc_attn, t.grad_output, t.grad_loc_attn, t.grad_loc_attn, \
                                       stream)
  SAMP_DISPATCH(p, FDA_BWD);
#undef FDA_BWD
  if ((rc = check_launch("fda_bwd_coord"))) return rc;
  if (p.skip_value) return MDCONV_OK;
  const SampGather ga = {g.N, g.S, g.Lq, g.M, g.D, g.C, g.ln, g.acc};
  return samp_lists_gather(L, ws, p.det, ga, p.dtype, t.grad_output, t.grad_value, stream,
                           [&](bool fill, int *cnt, const int *rowptr, void *entries) {
#define FDA_LIST(DT, CT) samp_list_launch<FdaOp, CT>(g, fill, t.loc_attn, t.loc_attn, cnt, rowptr, entries, L.seg_stride, stream)
    SAMP_DISPATCH(p, FDA_LIST);   // (by coordinate type: three instances)
#undef FDA_LIST
  });
}

static int fda_validate(const mdconv_fda_desc *d, bool) { return attn_validate("fda", d); }
static const SampOp<mdconv_fda_desc, FdaPlan> kFda = {"fda", fda_validate, fda_plan};

}  // namespace mdconv

using namespace mdconv;

extern "C" {

int mdconv_fda_value_len(const mdconv_fda_desc *d) {
  clear_error();
  if (fda_validate(d, false)) return -1;
  const int64_t S = level_rows(d);
  if (S < 0) set_error("fda: the levels have 2^31 rows or more");
  return (int)S;
}

int mdconv_fda_loc_attn_len(const mdconv_fda_desc *d) {
  clear_error();
  if (fda_validate(d, false)) return -1;
  const long long len = 3LL * d->levels * d->points;
  if (len >= (1LL << 31)) {
    set_error("fda: a row of sampling_loc_attn has 2^31 elements or more");
    return -1;
  }
  return (int)len;
}

size_t mdconv_fda_workspace_bytes(const mdconv_fda_desc *d, int backward) {
  clear_error();
  return samp_workspace_bytes(kFda, d, backward);
}

int mdconv_fda_forward(const mdconv_fda_desc *d, const void *value, const void *sampling_loc_attn, void *output,
                       void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kFda, d, false, workspace, workspace_bytes,
      [&] {
        return check_args({{value, "value", 16}, {sampling_loc_attn, "sampling_loc_attn", dtype_bytes(d->coord_dtype)},
                           {output, "output", 16}});
      },
      [&](const FdaPlan &p) {
        FdaTensors t = {};
        t.value = value; t.loc_attn = sampling_loc_attn; t.output = output;
        return fda_forward(p, t, (hipStream_t)stream);
      });
}

int mdconv_fda_backward(const mdconv_fda_desc *d, const void *value, const void *sampling_loc_attn, const void *grad_output,
                        void *grad_value, void *grad_sampling_loc_attn, void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kFda, d, true, workspace, workspace_bytes,
      [&] {
        const size_t cs = dtype_bytes(d->coord_dtype);
        return check_args({{value, "value", 16}, {sampling_loc_attn, "sampling_loc_attn", cs}, {grad_output, "grad_output", 16},
                           {grad_sampling_loc_attn, "grad_sampling_loc_attn", cs},
                           {grad_value, "grad_value", 16, !(d->flags & MDCONV_FLAG_NO_GRAD_INPUT)}});
      },
      [&](const FdaPlan &p) {
        FdaTensors t = {};
        t.value = value; t.loc_attn = sampling_loc_attn; t.grad_output = grad_output;
        t.grad_value = grad_value; t.grad_loc_attn = grad_sampling_loc_attn;
        return fda_backward(p, t, workspace, (hipStream_t)stream);
      });
}

}  // extern "C"
