// dagg_host.hip -- deformable aggregation (dagg_plan.hpp): the plan, the execution and the C entry points of
// include/mdconv_dagg.h.  The entry points live here, beside their plan, and not in mdconv_api.hip: the operator has a
// header of its own and nothing of the existing interface changes.
#include <stdint.h>

#include "dagg_plan.hpp"

namespace mdconv {

bool dagg_plan(const mdconv_dagg_desc *d, bool backward, DaggPlan *p, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = nullptr;
  const int64_t lim = (int64_t)1 << 31;
  const int esz = d->dtype == MDCONV_F32 ? 4 : 2;
  const int csz = d->coord_dtype == MDCONV_F32 ? 4 : 2;
  const int Dg = d->channels / d->groups;
  const int64_t C = d->channels;
  int64_t S_cam = 0;
  bool level_big = false;
  for (int l = 0; l < d->levels; ++l) {
    const int64_t rows = (int64_t)d->level_sz[l][0] * d->level_sz[l][1];   // below 2^62
    if (rows >= lim) level_big = true;   // (and stays out of the sum, which then cannot overflow)
    else S_cam += rows;
  }
  const bool skip_feature = backward && (d->flags & MDCONV_FLAG_NO_GRAD_INPUT);
  const int64_t anchors = (int64_t)d->batch * d->anchors;   // below 2^62
  const int64_t U = (int64_t)d->points * d->cams;           // below 2^62
  // (each product is checked with its factors bounded by the checks before it, so none overflows 64 bits)
  if (esz == 4 && Dg % 4) *why = "channels / groups is not a multiple of 4 (fp32 group rows of 16 bytes)";
  else if (esz == 2 && Dg % 8) *why = "channels / groups is not a multiple of 8 (16-bit group rows of 16 bytes)";
  else if (level_big || S_cam >= lim || S_cam * d->cams >= lim || S_cam * d->cams * d->batch >= lim ||
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
  int start = 0;
  for (int l = 0; l < MDCONV_MSDA_MAX_LEVELS; ++l) {
    const bool used = l < d->levels;
    g.lvH[l] = used ? d->level_sz[l][0] : 1;
    g.lvW[l] = used ? d->level_sz[l][1] : 1;
    g.lvS[l] = used ? start : 0;
    if (used) start += g.lvH[l] * g.lvW[l];
  }
  g.ln = samp_lanes(g.C, esz);
  g.VG = Dg * esz / 16;
  g.seg = (g.VG & (g.VG - 1)) == 0 && g.VG <= g.ln.VL;
  g.acc = d->accumulate;
  q.dtype = d->dtype;
  q.coord_dtype = d->coord_dtype;
  q.backward = backward;
  q.det = backward && (d->flags & MDCONV_FLAG_DETERMINISTIC);
  q.skip_feature = skip_feature;
  q.total = 0;
  if (backward && !skip_feature) {
    Bump ws;
    q.lists = scatter_lists_take(ws, g.B, g.S, (int64_t)d->anchors * U * d->levels * 4, q.det);
    q.total = ws.off;
  }
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

// ---- the checks of the entry points, in the order of the other operators (mdconv_api.hip) ----
static void clear_error() { set_error("%s", ""); }

static int dagg_validate(const mdconv_dagg_desc *d) {
  if (!d) {
    set_error("descriptor pointer is NULL");
    return MDCONV_EINVAL;
  }
  if (d->dtype != MDCONV_F32 && d->dtype != MDCONV_F16 && d->dtype != MDCONV_BF16) {
    set_error("dagg: dtype %d is not MDCONV_F32, MDCONV_F16 or MDCONV_BF16 (the dtype flags do not apply)", d->dtype);
    return MDCONV_EINVAL;
  }
  if (d->coord_dtype != d->dtype && d->coord_dtype != MDCONV_F32) {
    set_error("dagg: coord_dtype %d is neither dtype (%d) nor MDCONV_F32", d->coord_dtype, d->dtype);
    return MDCONV_EINVAL;
  }
  if (d->batch <= 0 || d->cams <= 0 || d->channels <= 0 || d->groups <= 0 || d->anchors <= 0 || d->points <= 0) {
    set_error("dagg: batch, cams, channels, groups, anchors and points must be positive (%d, %d, %d, %d, %d, %d)", d->batch,
              d->cams, d->channels, d->groups, d->anchors, d->points);
    return MDCONV_EINVAL;
  }
  if (d->channels % d->groups) {
    set_error("dagg: channels (%d) is not a multiple of groups (%d)", d->channels, d->groups);
    return MDCONV_EINVAL;
  }
  if (d->levels < 1 || d->levels > MDCONV_MSDA_MAX_LEVELS) {
    set_error("dagg: levels must be 1..%d, is %d", MDCONV_MSDA_MAX_LEVELS, d->levels);
    return MDCONV_EINVAL;
  }
  for (int l = 0; l < d->levels; ++l)
    if (d->level_sz[l][0] <= 0 || d->level_sz[l][1] <= 0) {
      set_error("dagg: level %d has a non-positive extent (%d x %d)", l, d->level_sz[l][0], d->level_sz[l][1]);
      return MDCONV_EINVAL;
    }
  if (d->accumulate != 0 && d->accumulate != 1) {
    set_error("dagg: accumulate must be 0 or 1, is %d", d->accumulate);
    return MDCONV_EINVAL;
  }
  if (d->flags & ~(MDCONV_FLAG_DETERMINISTIC | MDCONV_FLAG_NO_GRAD_INPUT)) {
    set_error("dagg: unknown bits 0x%x in flags; the flags are MDCONV_FLAG_DETERMINISTIC (1) and MDCONV_FLAG_NO_GRAD_INPUT (4)",
              (unsigned)(d->flags & ~(MDCONV_FLAG_DETERMINISTIC | MDCONV_FLAG_NO_GRAD_INPUT)));
    return MDCONV_EINVAL;
  }
  return MDCONV_OK;
}
static int dagg_refuse(const char *why) {
  set_error("dagg: outside the shape rule of the operator: %s", why);
  return MDCONV_EUNSUPPORTED;
}
static int dagg_require(const void *p, const char *name) {
  if (!p) {
    set_error("%s pointer is NULL", name);
    return MDCONV_ENULL;
  }
  return MDCONV_OK;
}
// pointer classes (include/mdconv_dagg.h): `align` = 16 ("16-byte") or the element size ("element")
static int dagg_aligned(const void *p, const char *name, size_t align) {
  if (p && ((uintptr_t)p & (align - 1)) != 0) {
    set_error("%s pointer must be %zu-byte aligned", name, align);
    return MDCONV_EINVAL;
  }
  return MDCONV_OK;
}
static int dagg_check_ws(void *ws, size_t have, size_t need) {
  if (need == 0) return MDCONV_OK;
  if (!ws || have < need) {
    set_error("workspace too small: need %zu bytes, have %zu", need, have);
    return MDCONV_EWORKSPACE;
  }
  if (((uintptr_t)ws & 15) != 0) {
    set_error("workspace must be 16-byte aligned");
    return MDCONV_EWORKSPACE;
  }
  return MDCONV_OK;
}

}  // namespace mdconv

using namespace mdconv;

extern "C" {

int mdconv_dagg_feature_len(const mdconv_dagg_desc *d) {
  clear_error();
  if (dagg_validate(d)) return -1;
  long long S = 0;
  bool big = false;
  for (int l = 0; l < d->levels; ++l) {
    const long long rows = (long long)d->level_sz[l][0] * d->level_sz[l][1];   // below 2^62
    if (rows >= (1LL << 31)) big = true;
    else S += rows;   // (8 terms below 2^31)
  }
  if (big || S * d->cams >= (1LL << 31)) {
    set_error("dagg: the maps of an image have 2^31 rows or more");
    return -1;
  }
  return (int)(S * d->cams);
}

size_t mdconv_dagg_workspace_bytes(const mdconv_dagg_desc *d, int backward) {
  DaggPlan p;
  const char *why;
  clear_error();
  if (dagg_validate(d)) return 0;
  if (!dagg_plan(d, backward != 0, &p, &why)) {
    dagg_refuse(why);
    return 0;
  }
  return p.total;
}

int mdconv_dagg_forward(const mdconv_dagg_desc *d, const void *feature, const void *sampling_location, const void *weights,
                        void *output, void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  int rc = dagg_validate(d);
  if (rc) return rc;
  if ((rc = dagg_require(feature, "feature")) || (rc = dagg_require(sampling_location, "sampling_location")) ||
      (rc = dagg_require(weights, "weights")) || (rc = dagg_require(output, "output")))
    return rc;
  const size_t csz = d->coord_dtype == MDCONV_F32 ? 4 : 2;
  if ((rc = dagg_aligned(feature, "feature", 16)) || (rc = dagg_aligned(sampling_location, "sampling_location", csz)) ||
      (rc = dagg_aligned(weights, "weights", csz)) || (rc = dagg_aligned(output, "output", 16)))
    return rc;
  DaggPlan p;
  const char *why;
  if (!dagg_plan(d, false, &p, &why)) return dagg_refuse(why);
  if ((rc = dagg_check_ws(workspace, workspace_bytes, p.total))) return rc;
  DaggTensors t = {};
  t.feature = feature; t.loc = sampling_location; t.wts = weights; t.output = output;
  return dagg_forward(p, t, (hipStream_t)stream);
}

int mdconv_dagg_backward(const mdconv_dagg_desc *d, const void *feature, const void *sampling_location, const void *weights,
                         const void *grad_output, void *grad_feature, void *grad_sampling_location, void *grad_weights,
                         void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  int rc = dagg_validate(d);
  if (rc) return rc;
  const bool with_feature = !(d->flags & MDCONV_FLAG_NO_GRAD_INPUT);
  if ((rc = dagg_require(feature, "feature")) || (rc = dagg_require(sampling_location, "sampling_location")) ||
      (rc = dagg_require(weights, "weights")) || (rc = dagg_require(grad_output, "grad_output")) ||
      (rc = dagg_require(grad_sampling_location, "grad_sampling_location")) || (rc = dagg_require(grad_weights, "grad_weights")))
    return rc;
  if (with_feature && (rc = dagg_require(grad_feature, "grad_feature"))) return rc;
  const size_t csz = d->coord_dtype == MDCONV_F32 ? 4 : 2;
  if ((rc = dagg_aligned(feature, "feature", 16)) || (rc = dagg_aligned(sampling_location, "sampling_location", csz)) ||
      (rc = dagg_aligned(weights, "weights", csz)) || (rc = dagg_aligned(grad_output, "grad_output", 16)) ||
      (rc = dagg_aligned(grad_sampling_location, "grad_sampling_location", csz)) ||
      (rc = dagg_aligned(grad_weights, "grad_weights", csz)))
    return rc;
  if (with_feature && (rc = dagg_aligned(grad_feature, "grad_feature", 16))) return rc;
  DaggPlan p;
  const char *why;
  if (!dagg_plan(d, true, &p, &why)) return dagg_refuse(why);
  if ((rc = dagg_check_ws(workspace, workspace_bytes, p.total))) return rc;
  DaggTensors t = {};
  t.feature = feature; t.loc = sampling_location; t.wts = weights; t.grad_output = grad_output;
  t.grad_feature = with_feature ? grad_feature : nullptr; t.grad_loc = grad_sampling_location; t.grad_wts = grad_weights;
  return dagg_backward(p, t, workspace, (hipStream_t)stream);
}

}  // extern "C"
