// fdap_host.hip -- plan and execution of packed deformable attention with a point count per level (fdap_plan.hpp): the
// sampling core's kernels (samp_core.hpp) instantiated with FdapOp for the five (value type, coordinate type) pairings.
// sampling_loc_attn is both the core's `coord` and its `factor`, grad_sampling_loc_attn both gradient tensors; the gather is
// the one every sampling operator shares.  The operator's C entry points (include/mdconv_fdap.h) follow, on the entry-point
// layer of samp_api.hpp with the argument tables of mdconv_fda_*.
#include "fdap_plan.hpp"
#include "samp_api.hpp"

namespace mdconv {

bool fdap_plan(const mdconv_fdap_desc *d, bool backward, FdapPlan *p, const char **why) {
  // the geometry, the shape rule and the lists are MSDAP's for the same fields
  mdconv_msdap_desc md = {};
  md.dtype = d->dtype; md.coord_dtype = d->coord_dtype;
  md.batch = d->batch; md.heads = d->heads; md.head_channels = d->head_channels;
  md.queries = d->queries; md.levels = d->levels;
  for (int l = 0; l < MDCONV_MSDA_MAX_LEVELS; ++l) {
    md.points[l] = d->points[l];
    md.level_sz[l][0] = d->level_sz[l][0];
    md.level_sz[l][1] = d->level_sz[l][1];
  }
  md.accumulate = d->accumulate; md.flags = d->flags;
  MsdapPlan m;
  if (!msdap_plan(&md, backward, &m, why)) return false;
  // ... plus the packed tensor, half again as large as sampling_locations (which passed: the product stays below 2^33)
  if ((int64_t)m.g.npairs * m.g.K * 3 * (int64_t)dtype_bytes(d->coord_dtype) >= (int64_t)1 << 31) {
    *why = "a tensor of the call has 2^31 bytes or more";
    return false;
  }
  FdapPlan q = {};
  (MsdapGeom &)q.g = m.g;
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

int fdap_forward(const FdapPlan &p, const FdaTensors &t, hipStream_t stream) {
#define FDAP_FWD(DT, CT) samp_fwd_launch<FdapOp, DT, CT>(p.g, t.value, t.loc_attn, t.loc_attn, t.output, stream)
  SAMP_DISPATCH(p, FDAP_FWD);
#undef FDAP_FWD
  return check_launch("fdap_fwd");
}

int fdap_backward(const FdapPlan &p, const FdaTensors &t, void *ws, hipStream_t stream) {
  FdapGeom g = p.g;
  const ScatterLists &L = p.lists;
  int rc;
  // (the coordinate kernel stores the pairs' softmax statistics for the list kernels, which run behind it on the stream)
  g.stats = p.skip_value ? nullptr : (float2 *)((char *)ws + p.off_stats);
#define FDAP_BWD(DT, CT)                                                                                               \
  samp_bwd_coord_launch<FdapOp, DT, CT>(g, t.value, t.loc_attn, t.loc_attn, t.grad_output, t.grad_loc_attn, t.grad_loc_attn, \
                                        stream)
  SAMP_DISPATCH(p, FDAP_BWD);
#undef FDAP_BWD
  if ((rc = check_launch("fdap_bwd_coord"))) return rc;
  if (p.skip_value) return MDCONV_OK;
  const SampGather ga = {g.N, g.S, g.Lq, g.M, g.D, g.C, g.ln, g.acc};
  return samp_lists_gather(L, ws, p.det, ga, p.dtype, t.grad_output, t.grad_value, stream,
                           [&](bool fill, int *cnt, const int *rowptr, void *entries) {
#define FDAP_LIST(DT, CT) samp_list_launch<FdapOp, CT>(g, fill, t.loc_attn, t.loc_attn, cnt, rowptr, entries, L.seg_stride, stream)
    SAMP_DISPATCH(p, FDAP_LIST);   // (by coordinate type: three instances)
#undef FDAP_LIST
  });
}

// the validation of mdconv_msdap_* under this operator's name: the levels are validated before their counts are read
static int fdap_validate(const mdconv_fdap_desc *d, bool) {
  const char *op = "fdap";
  if (int rc = desc_dtypes(op, d)) return rc;
  if (d->batch <= 0 || d->heads <= 0 || d->head_channels <= 0 || d->queries <= 0) {
    set_error("%s: batch, heads, head_channels and queries must be positive (%d, %d, %d, %d)", op, d->batch, d->heads,
              d->head_channels, d->queries);
    return MDCONV_EINVAL;
  }
  if (int rc = desc_levels(op, d)) return rc;
  for (int l = 0; l < d->levels; ++l)
    if (d->points[l] <= 0) {
      set_error("%s: level %d has a non-positive point count (%d)", op, l, d->points[l]);
      return MDCONV_EINVAL;
    }
  return desc_modes(op, d);
}
static const SampOp<mdconv_fdap_desc, FdapPlan> kFdap = {"fdap", fdap_validate, fdap_plan};

}  // namespace mdconv

using namespace mdconv;

extern "C" {

int mdconv_fdap_value_len(const mdconv_fdap_desc *d) {
  clear_error();
  if (fdap_validate(d, false)) return -1;
  const int64_t S = level_rows(d);
  if (S < 0) set_error("fdap: the levels have 2^31 rows or more");
  return (int)S;
}

int mdconv_fdap_loc_attn_len(const mdconv_fdap_desc *d) {
  clear_error();
  if (fdap_validate(d, false)) return -1;
  int64_t len = 0;   // every count is positive and below 2^31: below 2^36
  for (int l = 0; l < d->levels; ++l) len += 3 * (int64_t)d->points[l];
  if (len >= ((int64_t)1 << 31)) {
    set_error("fdap: a row of sampling_loc_attn has 2^31 elements or more");
    return -1;
  }
  return (int)len;
}

size_t mdconv_fdap_workspace_bytes(const mdconv_fdap_desc *d, int backward) {
  clear_error();
  return samp_workspace_bytes(kFdap, d, backward);
}

int mdconv_fdap_forward(const mdconv_fdap_desc *d, const void *value, const void *sampling_loc_attn, void *output,
                        void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kFdap, d, false, workspace, workspace_bytes,
      [&] {
        return check_args({{value, "value", 16}, {sampling_loc_attn, "sampling_loc_attn", dtype_bytes(d->coord_dtype)},
                           {output, "output", 16}});
      },
      [&](const FdapPlan &p) {
        FdaTensors t = {};
        t.value = value; t.loc_attn = sampling_loc_attn; t.output = output;
        return fdap_forward(p, t, (hipStream_t)stream);
      });
}

int mdconv_fdap_backward(const mdconv_fdap_desc *d, const void *value, const void *sampling_loc_attn, const void *grad_output,
                         void *grad_value, void *grad_sampling_loc_attn, void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kFdap, d, true, workspace, workspace_bytes,
      [&] {
        const size_t cs = dtype_bytes(d->coord_dtype);
        return check_args({{value, "value", 16}, {sampling_loc_attn, "sampling_loc_attn", cs}, {grad_output, "grad_output", 16},
                           {grad_sampling_loc_attn, "grad_sampling_loc_attn", cs},
                           {grad_value, "grad_value", 16, !(d->flags & MDCONV_FLAG_NO_GRAD_INPUT)}});
      },
      [&](const FdapPlan &p) {
        FdaTensors t = {};
        t.value = value; t.loc_attn = sampling_loc_attn; t.grad_output = grad_output;
        t.grad_value = grad_value; t.grad_loc_attn = grad_sampling_loc_attn;
        return fdap_backward(p, t, workspace, (hipStream_t)stream);
      });
}

}  // extern "C"
