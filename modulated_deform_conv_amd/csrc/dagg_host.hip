// dagg_host.hip -- deformable aggregation (dagg_plan.hpp): the plan, the execution and the C entry points of
// include/mdconv_dagg.h, on the entry-point layer of samp_api.hpp like those of every sampling operator.
#include "dagg_plan.hpp"
#include "samp_api.hpp"

namespace mdconv {

bool dagg_plan(const mdconv_dagg_desc *d, bool backward, DaggPlan *p, const char **why) {
  *why = nullptr;
  const int64_t lim = (int64_t)1 << 31;
  const int esz = (int)dtype_bytes(d->dtype), csz = (int)dtype_bytes(d->coord_dtype);
  const int Dg = d->channels / d->groups;
  const int64_t C = d->channels;
  const int64_t S_cam = level_rows(d);   // -1: 2^31 rows or more
  const bool skip_feature = backward && (d->flags & MDCONV_FLAG_NO_GRAD_INPUT);
  const int64_t anchors = (int64_t)d->batch * d->anchors;   // below 2^62
  const int64_t U = (int64_t)d->points * d->cams;           // below 2^62
  // (each product is checked with its factors bounded by the checks before it, so none overflows 64 bits)
  if (esz == 4 && Dg % 4) *why = "channels / groups is not a multiple of 4 (fp32 group rows of 16 bytes)";
  else if (esz == 2 && Dg % 8) *why = "channels / groups is not a multiple of 8 (16-bit group rows of 16 bytes)";
  else if (S_cam < 0 || S_cam * d->cams >= lim || S_cam * d->cams * d->batch >= lim ||
           S_cam * d->cams * d->batch * C >= lim / esz || anchors >= lim || anchors * C >= lim / esz || U >= lim ||
           anchors * U >= lim / (2 * csz) || anchors * U * d->levels >= lim ||
           anchors * U * d->levels * d->groups >= lim / csz)
    *why = "a tensor of the call has 2^31 rows or bytes or more";
  else if (backward && !skip_feature && d->batch > 65535) *why = "batch exceeds 65535 (the scatter lists of grad_feature)";
  else if (backward && !skip_feature && (int64_t)d->anchors * U * d->levels * 4 >= lim)
    *why = "the list stride anchors * points * cams * levels * 4 reaches 2^31 (the scatter lists of grad_feature)";
  if (*why) return false;

  DaggPlan q = {};
  DaggGeom &g = q.g;
  g.B = d->batch; g.cams = d->cams; g.L = d->levels; g.C = (int)C; g.G = d->groups; g.Dg = Dg; g.A = d->anchors;
  g.P = d->points; g.U = (int)U; g.S_cam = (int)S_cam; g.S = (int)(S_cam * d->cams); g.nanchors = (int)anchors;
  level_fill(g, d);
  g.ln = samp_lanes(g.C, esz);
  g.VG = Dg * esz / 16;
  g.seg = (g.VG & (g.VG - 1)) == 0 && g.VG <= g.ln.VL;
  g.acc = d->accumulate;
  q.dtype = d->dtype;
  q.coord_dtype = d->coord_dtype;
  q.skip_feature = skip_feature;
  samp_plan_lists(q, backward, d->flags, skip_feature, g.B, g.S, (int64_t)d->anchors * U * d->levels * 4);
  *p = q;
  return true;
}

int dagg_forward(const DaggPlan &p, const DaggTensors &t, hipStream_t stream) { return dagg_fwd_launch(p, t, stream); }

int dagg_backward(const DaggPlan &p, const DaggTensors &t, void *ws, hipStream_t stream) {
  const ScatterLists &L = p.lists;
  int rc;
  if ((rc = dagg_bwd_coord_launch(p, t, stream))) return rc;
  if (p.skip_feature) return MDCONV_OK;
  rc = scatter_lists_build(L, ws, p.det, stream, [&](bool fill, int *cnt, const int *rowptr, void *entries) {
    dagg_list_launch(p, t, fill, cnt, rowptr, entries, stream);
  });
  if (rc) return rc;
  return dagg_gather_launch(p, t, (const int *)((char *)ws + L.off_rowptr), (char *)ws + L.off_entries, stream);
}

// the descriptor's own validation; the shape rule is dagg_plan's
static int dagg_validate(const mdconv_dagg_desc *d, bool) {
  int rc;
  if ((rc = desc_dtypes("dagg", d))) return rc;
  if (d->batch <= 0 || d->cams <= 0 || d->channels <= 0 || d->groups <= 0 || d->anchors <= 0 || d->points <= 0) {
    set_error("dagg: batch, cams, channels, groups, anchors and points must be positive (%d, %d, %d, %d, %d, %d)", d->batch,
              d->cams, d->channels, d->groups, d->anchors, d->points);
    return MDCONV_EINVAL;
  }
  if (d->channels % d->groups) {
    set_error("dagg: channels (%d) is not a multiple of groups (%d)", d->channels, d->groups);
    return MDCONV_EINVAL;
  }
  if ((rc = desc_levels("dagg", d))) return rc;
  return desc_modes("dagg", d);
}
static const SampOp<mdconv_dagg_desc, DaggPlan> kDagg = {"dagg", dagg_validate, dagg_plan};

}  // namespace mdconv

using namespace mdconv;

extern "C" {

int mdconv_dagg_feature_len(const mdconv_dagg_desc *d) {
  clear_error();
  if (dagg_validate(d, false)) return -1;
  const int64_t S = level_rows(d);
  if (S < 0 || S * d->cams >= (1LL << 31)) {
    set_error("dagg: the maps of an image have 2^31 rows or more");
    return -1;
  }
  return (int)(S * d->cams);
}

size_t mdconv_dagg_workspace_bytes(const mdconv_dagg_desc *d, int backward) {
  clear_error();
  return samp_workspace_bytes(kDagg, d, backward);
}

int mdconv_dagg_forward(const mdconv_dagg_desc *d, const void *feature, const void *sampling_location, const void *weights,
                        void *output, void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kDagg, d, false, workspace, workspace_bytes,
      [&] {
        const size_t cs = dtype_bytes(d->coord_dtype);
        return check_args({{feature, "feature", 16}, {sampling_location, "sampling_location", cs}, {weights, "weights", cs},
                           {output, "output", 16}});
      },
      [&](const DaggPlan &p) {
        DaggTensors t = {};
        t.feature = feature; t.loc = sampling_location; t.wts = weights; t.output = output;
        return dagg_forward(p, t, (hipStream_t)stream);
      });
}

int mdconv_dagg_backward(const mdconv_dagg_desc *d, const void *feature, const void *sampling_location, const void *weights,
                         const void *grad_output, void *grad_feature, void *grad_sampling_location, void *grad_weights,
                         void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kDagg, d, true, workspace, workspace_bytes,
      [&] {
        const size_t cs = dtype_bytes(d->coord_dtype);
        return check_args({{feature, "feature", 16}, {sampling_location, "sampling_location", cs}, {weights, "weights", cs},
                           {grad_output, "grad_output", 16}, {grad_sampling_location, "grad_sampling_location", cs},
                           {grad_weights, "grad_weights", cs},
                           {grad_feature, "grad_feature", 16, !(d->flags & MDCONV_FLAG_NO_GRAD_INPUT)}});
      },
      [&](const DaggPlan &p) {
        DaggTensors t = {};
        t.feature = feature; t.loc = sampling_location; t.wts = weights; t.grad_output = grad_output;
        t.grad_feature = p.skip_feature ? nullptr : grad_feature; t.grad_loc = grad_sampling_location; t.grad_wts = grad_weights;
        return dagg_backward(p, t, workspace, (hipStream_t)stream);
      });
}

}  // extern "C"
