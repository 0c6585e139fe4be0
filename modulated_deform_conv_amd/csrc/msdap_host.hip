// msdap_host.hip -- plan and execution of multi-scale deformable attention with a point count per level (msdap_plan.hpp):
// the sampling core's kernels (samp_core.hpp) instantiated with MsdapOp for the five (value type, coordinate type) pairings,
// and the operator's C entry points (include/mdconv_msdap.h) on the entry-point layer of samp_api.hpp.  The list build and the
// channels-last gather are the shared ones (samp_lists_gather).
#include "msdap_plan.hpp"
#include "samp_api.hpp"

namespace mdconv {

// K of a validated descriptor (every count positive): below 2^34
static int64_t msdap_taps(const mdconv_msdap_desc *d) {
  int64_t K = 0;
  for (int l = 0; l < d->levels; ++l) K += d->points[l];
  return K;
}

bool msdap_plan(const mdconv_msdap_desc *d, bool backward, MsdapPlan *p, const char **why) {
  *why = nullptr;
  const int64_t lim = (int64_t)1 << 31;
  const int esz = (int)dtype_bytes(d->dtype), csz = (int)dtype_bytes(d->coord_dtype);
  const int64_t K = msdap_taps(d);
  const int64_t C = (int64_t)d->heads * d->head_channels;
  const int64_t pairs = (int64_t)d->batch * d->queries;   // times heads below, once both factors are bounded
  const int64_t S = level_rows(d);                        // -1: 2^31 rows or more
  const bool skip_value = backward && (d->flags & MDCONV_FLAG_NO_GRAD_INPUT);
  const int64_t seg_stride = (K <= 4096 ? K : 0) * d->queries * 4;   // K <= 4096 once checked: no overflow
  // (the rules of msda_plan in its order, levels * points replaced by K; each product is checked with its factors bounded by
  // the checks before it, so none overflows 64 bits)
  if (esz == 4 && d->head_channels % 4) *why = "head_channels is not a multiple of 4 (fp32 rows of 16 bytes)";
  else if (esz == 2 && d->head_channels % 8) *why = "head_channels is not a multiple of 8 (16-bit rows of 16 bytes)";
  else if (K > 4096) *why = "the sum of points exceeds 4096";
  else if (S < 0 || C >= lim || pairs >= lim || d->batch * S >= lim || d->batch * S * C >= lim / esz ||
           pairs * C >= lim / esz || pairs * d->heads >= lim || pairs * d->heads * K * 2 * csz >= lim)
    *why = "a tensor of the call has 2^31 bytes or more";
  else if (backward && !skip_value && (int64_t)d->batch * d->heads > 65535)
    *why = "batch * heads exceeds 65535 (the scatter lists of grad_value)";
  else if (backward && !skip_value && seg_stride >= lim)
    *why = "the list stride (sum of points) * queries * 4 reaches 2^31 (the scatter lists of grad_value)";
  if (*why) return false;

  MsdapPlan q = {};
  MsdapGeom &g = q.g;
  g.N = d->batch; g.M = d->heads; g.D = d->head_channels; g.C = (int)C; g.Lq = d->queries; g.L = d->levels; g.P = 0;
  g.K = (int)K; g.S = (int)S; g.npairs = (int)(pairs * d->heads);
  level_fill(g, d);
  int first = 0;
  for (int l = 0; l < MDCONV_MSDA_MAX_LEVELS; ++l) {
    g.pfx[l] = l < d->levels ? first : (int)K;
    if (l < d->levels) first += d->points[l];
  }
  g.ln = samp_lanes(g.D, esz);
  g.acc = d->accumulate;
  q.dtype = d->dtype;
  q.coord_dtype = d->coord_dtype;
  q.skip_value = skip_value;
  samp_plan_lists(q, backward, d->flags, skip_value, g.N * g.M, g.S, seg_stride);
  *p = q;
  return true;
}

int msdap_forward(const MsdapPlan &p, const MsdaTensors &t, hipStream_t stream) {
#define MSDAP_FWD(DT, CT) samp_fwd_launch<MsdapOp, DT, CT>(p.g, t.value, t.loc, t.attn, t.output, stream)
  SAMP_DISPATCH(p, MSDAP_FWD);
#undef MSDAP_FWD
  return check_launch("msdap_fwd");
}

int msdap_backward(const MsdapPlan &p, const MsdaTensors &t, void *ws, hipStream_t stream) {
  const MsdapGeom &g = p.g;
  const ScatterLists &L = p.lists;
  int rc;
#define MSDAP_BWD(DT, CT) \
  samp_bwd_coord_launch<MsdapOp, DT, CT>(g, t.value, t.loc, t.attn, t.grad_output, t.grad_loc, t.grad_attn, stream)
  SAMP_DISPATCH(p, MSDAP_BWD);
#undef MSDAP_BWD
  if ((rc = check_launch("msdap_bwd_coord"))) return rc;
  if (p.skip_value) return MDCONV_OK;
  const SampGather ga = {g.N, g.S, g.Lq, g.M, g.D, g.C, g.ln, g.acc};
  return samp_lists_gather(L, ws, p.det, ga, p.dtype, t.grad_output, t.grad_value, stream,
                           [&](bool fill, int *cnt, const int *rowptr, void *entries) {
#define MSDAP_LIST(DT, CT) samp_list_launch<MsdapOp, CT>(g, fill, t.loc, t.attn, cnt, rowptr, entries, L.seg_stride, stream)
    SAMP_DISPATCH(p, MSDAP_LIST);   // (by coordinate type: three instances)
#undef MSDAP_LIST
  });
}

// attn_validate (samp_api.hpp) with a count per level: the levels are validated before their counts are read
static int msdap_validate(const mdconv_msdap_desc *d, bool) {
  const char *op = "msdap";
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
static const SampOp<mdconv_msdap_desc, MsdapPlan> kMsdap = {"msdap", msdap_validate, msdap_plan};

}  // namespace mdconv

using namespace mdconv;

extern "C" {

int mdconv_msdap_value_len(const mdconv_msdap_desc *d) {
  clear_error();
  if (msdap_validate(d, false)) return -1;
  const int64_t S = level_rows(d);
  if (S < 0) set_error("msdap: the levels have 2^31 rows or more");
  return (int)S;
}

int mdconv_msdap_points_len(const mdconv_msdap_desc *d) {
  clear_error();
  if (msdap_validate(d, false)) return -1;
  const int64_t K = msdap_taps(d);
  if (K >= ((int64_t)1 << 31)) {
    set_error("msdap: the sum of points reaches 2^31");
    return -1;
  }
  return (int)K;
}

size_t mdconv_msdap_workspace_bytes(const mdconv_msdap_desc *d, int backward) {
  clear_error();
  return samp_workspace_bytes(kMsdap, d, backward);
}

int mdconv_msdap_forward(const mdconv_msdap_desc *d, const void *value, const void *sampling_locations,
                         const void *attention_weights, void *output, void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kMsdap, d, false, workspace, workspace_bytes,
      [&] {
        const size_t cs = dtype_bytes(d->coord_dtype);
        return check_args({{value, "value", 16}, {sampling_locations, "sampling_locations", cs},
                           {attention_weights, "attention_weights", cs}, {output, "output", 16}});
      },
      [&](const MsdapPlan &p) {
        MsdaTensors t = {};
        t.value = value; t.loc = sampling_locations; t.attn = attention_weights; t.output = output;
        return msdap_forward(p, t, (hipStream_t)stream);
      });
}

int mdconv_msdap_backward(const mdconv_msdap_desc *d, const void *value, const void *sampling_locations,
                          const void *attention_weights, const void *grad_output, void *grad_value,
                          void *grad_sampling_locations, void *grad_attention_weights, void *workspace,
                          size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kMsdap, d, true, workspace, workspace_bytes,
      [&] {
        const size_t cs = dtype_bytes(d->coord_dtype);
        return check_args({{value, "value", 16}, {sampling_locations, "sampling_locations", cs},
                           {attention_weights, "attention_weights", cs}, {grad_output, "grad_output", 16},
                           {grad_sampling_locations, "grad_sampling_locations", cs},
                           {grad_attention_weights, "grad_attention_weights", cs},
                           {grad_value, "grad_value", 16, !(d->flags & MDCONV_FLAG_NO_GRAD_INPUT)}});
      },
      [&](const MsdapPlan &p) {
        MsdaTensors t = {};
        t.value = value; t.loc = sampling_locations; t.attn = attention_weights; t.grad_output = grad_output;
        t.grad_value = grad_value; t.grad_loc = grad_sampling_locations; t.grad_attn = grad_attention_weights;
        return msdap_backward(p, t, workspace, (hipStream_t)stream);
      });
}

}  // extern "C"
