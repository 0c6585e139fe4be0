// afda_host.hip -- plan and execution of anchored packed deformable attention (afda_plan.hpp): the sampling core's kernels
// (samp_core.hpp) instantiated with AfdaOp for the five (value type, coordinate type) pairings -- as many instances as
// FdapOp has: Lr, R and offset_scale are run-time data of the geometry.  offs_attn is both the core's `coord` and its
// `factor`, grad_offs_attn both gradient tensors; the reference tensor travels in the geometry.  grad_reference_points takes
// two stages: partial rows per (query, head) out of the coordinate backward (AfdaOp::tap_grads), then afda_ref_reduce_kernel
// over the heads.  The gather is the one every sampling operator shares.  The operator's C entry points
// (include/mdconv_afda.h) follow, on the entry-point layer of samp_api.hpp.
#include "afda_plan.hpp"
#include "samp_api.hpp"

namespace mdconv {

bool afda_plan(const mdconv_afda_desc *d, bool backward, AfdaPlan *p, const char **why) {
  // the geometry, the shape rule, the lists and the statistics are FDAP's for the same fields
  mdconv_fdap_desc fd = {};
  fd.dtype = d->dtype; fd.coord_dtype = d->coord_dtype;
  fd.batch = d->batch; fd.heads = d->heads; fd.head_channels = d->head_channels;
  fd.queries = d->queries; fd.levels = d->levels;
  for (int l = 0; l < MDCONV_MSDA_MAX_LEVELS; ++l) {
    fd.points[l] = d->points[l];
    fd.level_sz[l][0] = d->level_sz[l][0];
    fd.level_sz[l][1] = d->level_sz[l][1];
  }
  fd.accumulate = d->accumulate; fd.flags = d->flags;
  FdapPlan f;
  if (!fdap_plan(&fd, backward, &f, why)) return false;
  // ... plus the reference tensor, and the partial rows of its gradient: 4 * Lr * R bytes per pair (npairs is below 2^29)
  const int row = d->ref_levels * d->ref_comps;
  if ((int64_t)f.g.npairs * row * 4 >= (int64_t)1 << 31) {
    *why = "a tensor of the call has 2^31 bytes or more";
    return false;
  }
  AfdaPlan q = {};
  AfdaGeom &g = q.g;
  (FdapGeom &)g = f.g;
  g.ref = nullptr;
  g.gpart = nullptr;
  g.Lr = d->ref_levels;
  g.R = d->ref_comps;
  g.oscale = d->offset_scale;
  for (int l = 0; l < MDCONV_MSDA_MAX_LEVELS; ++l) {
    const bool used = l < d->levels;
    g.inv_points[l] = used ? 1.f / (float)d->points[l] : 1.f;
    g.invW[l] = 1.f / (float)g.lvW[l];
    g.invH[l] = 1.f / (float)g.lvH[l];
  }
  q.dtype = f.dtype;
  q.coord_dtype = f.coord_dtype;
  q.backward = backward;
  q.det = f.det;
  q.skip_value = f.skip_value;
  q.grad_ref = backward && d->grad_reference;
  q.lists = f.lists;
  q.off_stats = f.off_stats;
  q.off_gpart = 0;
  q.total = f.total;
  if (q.grad_ref) {
    Bump ws;
    ws.off = f.total;
    q.off_gpart = ws.take((size_t)g.npairs * row * sizeof(float));
    q.total = ws.off;
  }
  *p = q;
  return true;
}

int afda_forward(const AfdaPlan &p, const AfdaTensors &t, hipStream_t stream) {
  AfdaGeom g = p.g;
  g.ref = (const float *)t.ref;
#define AFDA_FWD(DT, CT) samp_fwd_launch<AfdaOp, DT, CT>(g, t.value, t.offs_attn, t.offs_attn, t.output, stream)
  SAMP_DISPATCH(p, AFDA_FWD);
#undef AFDA_FWD
  return check_launch("afda_fwd");
}

int afda_backward(const AfdaPlan &p, const AfdaTensors &t, void *ws, hipStream_t stream) {
  AfdaGeom g = p.g;
  const ScatterLists &L = p.lists;
  int rc;
  g.ref = (const float *)t.ref;
  // (the coordinate kernel stores the pairs' softmax statistics for the list kernels and the partial rows of
  // grad_reference_points for the reduction, which run behind it on the stream)
  g.stats = p.skip_value ? nullptr : (float2 *)((char *)ws + p.off_stats);
  g.gpart = p.grad_ref ? (float *)((char *)ws + p.off_gpart) : nullptr;
#define AFDA_BWD(DT, CT)                                                                                                \
  samp_bwd_coord_launch<AfdaOp, DT, CT>(g, t.value, t.offs_attn, t.offs_attn, t.grad_output, t.grad_offs_attn, t.grad_offs_attn, \
                                        stream)
  SAMP_DISPATCH(p, AFDA_BWD);
#undef AFDA_BWD
  if ((rc = check_launch("afda_bwd_coord"))) return rc;
  if (p.grad_ref) {
    const int row = g.Lr * g.R, total = g.N * g.Lq * row;
    hipLaunchKernelGGL(afda_ref_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, g.gpart,
                       (float *)t.grad_ref, total, row, g.M, g.acc);
    if ((rc = check_launch("afda_ref_reduce"))) return rc;
  }
  if (p.skip_value) return MDCONV_OK;
  const SampGather ga = {g.N, g.S, g.Lq, g.M, g.D, g.C, g.ln, g.acc};
  return samp_lists_gather(L, ws, p.det, ga, p.dtype, t.grad_output, t.grad_value, stream,
                           [&](bool fill, int *cnt, const int *rowptr, void *entries) {
#define AFDA_LIST(DT, CT) samp_list_launch<AfdaOp, CT>(g, fill, t.offs_attn, t.offs_attn, cnt, rowptr, entries, L.seg_stride, stream)
    SAMP_DISPATCH(p, AFDA_LIST);   // (by coordinate type: three instances)
#undef AFDA_LIST
  });
}

// the validation of mdconv_fdap_* under this operator's name, then the four fields of the reference
static int afda_validate(const mdconv_afda_desc *d, bool) {
  const char *op = "afda";
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
  if (int rc = desc_modes(op, d)) return rc;
  if (d->ref_levels != 1 && d->ref_levels != d->levels) {
    set_error("%s: ref_levels must be 1 or levels (%d), is %d", op, d->levels, d->ref_levels);
    return MDCONV_EINVAL;
  }
  if (d->ref_comps != 2 && d->ref_comps != 4) {
    set_error("%s: ref_comps must be 2 or 4, is %d", op, d->ref_comps);
    return MDCONV_EINVAL;
  }
  if (int rc = desc_finite(op, "offset_scale", d->offset_scale)) return rc;
  if (d->grad_reference != 0 && d->grad_reference != 1) {
    set_error("%s: grad_reference must be 0 or 1, is %d", op, d->grad_reference);
    return MDCONV_EINVAL;
  }
  return MDCONV_OK;
}
static const SampOp<mdconv_afda_desc, AfdaPlan> kAfda = {"afda", afda_validate, afda_plan};

}  // namespace mdconv

using namespace mdconv;

extern "C" {

int mdconv_afda_value_len(const mdconv_afda_desc *d) {
  clear_error();
  if (afda_validate(d, false)) return -1;
  const int64_t S = level_rows(d);
  if (S < 0) set_error("afda: the levels have 2^31 rows or more");
  return (int)S;
}

int mdconv_afda_offs_attn_len(const mdconv_afda_desc *d) {
  clear_error();
  if (afda_validate(d, false)) return -1;
  int64_t len = 0;   // every count is positive and below 2^31: below 2^36
  for (int l = 0; l < d->levels; ++l) len += 3 * (int64_t)d->points[l];
  if (len >= ((int64_t)1 << 31)) {
    set_error("afda: a row of offs_attn has 2^31 elements or more");
    return -1;
  }
  return (int)len;
}

size_t mdconv_afda_workspace_bytes(const mdconv_afda_desc *d, int backward) {
  clear_error();
  return samp_workspace_bytes(kAfda, d, backward);
}

int mdconv_afda_forward(const mdconv_afda_desc *d, const void *value, const void *reference_points, const void *offs_attn,
                        void *output, void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kAfda, d, false, workspace, workspace_bytes,
      [&] {
        return check_args({{value, "value", 16}, {reference_points, "reference_points", 4},
                           {offs_attn, "offs_attn", dtype_bytes(d->coord_dtype)}, {output, "output", 16}});
      },
      [&](const AfdaPlan &p) {
        AfdaTensors t = {};
        t.value = value; t.ref = reference_points; t.offs_attn = offs_attn; t.output = output;
        return afda_forward(p, t, (hipStream_t)stream);
      });
}

int mdconv_afda_backward(const mdconv_afda_desc *d, const void *value, const void *reference_points, const void *offs_attn,
                         const void *grad_output, void *grad_value, void *grad_reference_points, void *grad_offs_attn,
                         void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kAfda, d, true, workspace, workspace_bytes,
      [&] {
        const size_t cs = dtype_bytes(d->coord_dtype);
        return check_args({{value, "value", 16}, {reference_points, "reference_points", 4}, {offs_attn, "offs_attn", cs},
                           {grad_output, "grad_output", 16}, {grad_offs_attn, "grad_offs_attn", cs},
                           {grad_value, "grad_value", 16, !(d->flags & MDCONV_FLAG_NO_GRAD_INPUT)},
                           {grad_reference_points, "grad_reference_points", 4, d->grad_reference != 0}});
      },
      [&](const AfdaPlan &p) {
        AfdaTensors t = {};
        t.value = value; t.ref = reference_points; t.offs_attn = offs_attn; t.grad_output = grad_output;
        t.grad_value = grad_value; t.grad_ref = grad_reference_points; t.grad_offs_attn = grad_offs_attn;
        return afda_backward(p, t, workspace, (hipStream_t)stream);
      });
}

}  // extern "C"
