// msda3_host.hip -- plan and execution of 3-D multi-scale deformable attention (msda3_plan.hpp): the family's own forward,
// coordinate-gradient and list kernels, the list builder and the channels-last gather of the sampling operators; and the
// operator's C entry points (include/mdconv.h) on the entry-point layer of samp_api.hpp.
#include "msda3_plan.hpp"
#include "samp_api.hpp"

namespace mdconv {

bool msda3_plan(const mdconv_msda3d_desc *d, bool backward, Msda3Plan *p, const char **why) {
  *why = nullptr;
  const int64_t lim = (int64_t)1 << 31;
  const int esz = (int)dtype_bytes(d->dtype), csz = (int)dtype_bytes(d->coord_dtype);
  const int64_t K = (int64_t)d->levels * d->points;
  const int64_t C = (int64_t)d->heads * d->head_channels;
  const int64_t pairs = (int64_t)d->batch * d->queries;   // times heads below, once both factors are bounded
  const int64_t S = level_rows(d);                        // T_l * H_l * W_l over the levels; -1: 2^31 rows or more
  const bool skip_value = backward && (d->flags & MDCONV_FLAG_NO_GRAD_INPUT);
  const int64_t seg_stride = K * d->queries * 8;   // K <= 4096 once checked: no overflow
  // (each product is checked with its factors bounded by the checks before it, so none overflows 64 bits)
  if (esz == 4 && d->head_channels % 4) *why = "head_channels is not a multiple of 4 (fp32 rows of 16 bytes)";
  else if (esz == 2 && d->head_channels % 8) *why = "head_channels is not a multiple of 8 (16-bit rows of 16 bytes)";
  else if (K > 4096) *why = "levels * points exceeds 4096";
  else if (S < 0 || C >= lim || pairs >= lim || d->batch * S >= lim || d->batch * S * C >= lim / esz ||
           pairs * C >= lim / esz || pairs * d->heads >= lim || pairs * d->heads * K * 3 * csz >= lim)
    *why = "a tensor of the call has 2^31 bytes or more";
  else if (backward && !skip_value && (int64_t)d->batch * d->heads > 65535)
    *why = "batch * heads exceeds 65535 (the scatter lists of grad_value)";
  else if (backward && !skip_value && seg_stride >= lim)
    *why = "the list stride levels * points * queries * 8 reaches 2^31 (the scatter lists of grad_value)";
  if (*why) return false;

  Msda3Plan q = {};
  Msda3Geom &g = q.g;
  g.N = d->batch; g.M = d->heads; g.D = d->head_channels; g.C = (int)C; g.Lq = d->queries; g.L = d->levels; g.P = d->points;
  g.K = (int)K; g.S = (int)S; g.npairs = (int)(pairs * d->heads);
  level_fill(g, d);
  g.ln = samp_lanes(g.D, esz);
  g.acc = d->accumulate;
  q.dtype = d->dtype;
  q.coord_dtype = d->coord_dtype;
  q.skip_value = skip_value;
  samp_plan_lists(q, backward, d->flags, skip_value, g.N * g.M, g.S, seg_stride);
  *p = q;
  return true;
}

int msda3_forward(const Msda3Plan &p, const Msda3Tensors &t, hipStream_t stream) { return msda3_fwd_launch(p, t, stream); }

int msda3_backward(const Msda3Plan &p, const Msda3Tensors &t, void *ws, hipStream_t stream) {
  const Msda3Geom &g = p.g;
  const ScatterLists &L = p.lists;
  int rc;
  if ((rc = msda3_bwd_coord_launch(p, t, stream))) return rc;
  if (p.skip_value) return MDCONV_OK;
  const SampGather ga = {g.N, g.S, g.Lq, g.M, g.D, g.C, g.ln, g.acc};
  return samp_lists_gather(L, ws, p.det, ga, p.dtype, t.grad_output, t.grad_value, stream,
                           [&](bool fill, int *cnt, const int *rowptr, void *entries) {
    msda3_list_launch(p, t, fill, cnt, rowptr, entries, stream);
  });
}

static int msda3d_validate(const mdconv_msda3d_desc *d, bool) { return attn_validate("msda3d", d); }
static const SampOp<mdconv_msda3d_desc, Msda3Plan> kMsda3d = {"msda3d", msda3d_validate, msda3_plan};

}  // namespace mdconv

using namespace mdconv;

extern "C" {

int mdconv_msda3d_value_len(const mdconv_msda3d_desc *d) {
  clear_error();
  if (msda3d_validate(d, false)) return -1;
  const int64_t S = level_rows(d);
  if (S < 0) set_error("msda3d: the levels have 2^31 rows or more");
  return (int)S;
}

size_t mdconv_msda3d_workspace_bytes(const mdconv_msda3d_desc *d, int backward) {
  clear_error();
  return samp_workspace_bytes(kMsda3d, d, backward);
}

int mdconv_msda3d_forward(const mdconv_msda3d_desc *d, const void *value, const void *sampling_locations,
                          const void *attention_weights, void *output, void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kMsda3d, d, false, workspace, workspace_bytes,
      [&] {
        const size_t cs = dtype_bytes(d->coord_dtype);
        return check_args({{value, "value", 16}, {sampling_locations, "sampling_locations", cs},
                           {attention_weights, "attention_weights", cs}, {output, "output", 16}});
      },
      [&](const Msda3Plan &p) {
        Msda3Tensors t = {};
        t.value = value; t.loc = sampling_locations; t.attn = attention_weights; t.output = output;
        return msda3_forward(p, t, (hipStream_t)stream);
      });
}

int mdconv_msda3d_backward(const mdconv_msda3d_desc *d, const void *value, const void *sampling_locations,
                           const void *attention_weights, const void *grad_output, void *grad_value,
                           void *grad_sampling_locations, void *grad_attention_weights, void *workspace,
                           size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kMsda3d, d, true, workspace, workspace_bytes,
      [&] {
        const size_t cs = dtype_bytes(d->coord_dtype);
        return check_args({{value, "value", 16}, {sampling_locations, "sampling_locations", cs},
                           {attention_weights, "attention_weights", cs}, {grad_output, "grad_output", 16},
                           {grad_sampling_locations, "grad_sampling_locations", cs},
                           {grad_attention_weights, "grad_attention_weights", cs},
                           {grad_value, "grad_value", 16, !(d->flags & MDCONV_FLAG_NO_GRAD_INPUT)}});
      },
      [&](const Msda3Plan &p) {
        Msda3Tensors t = {};
        t.value = value; t.loc = sampling_locations; t.attn = attention_weights; t.grad_output = grad_output;
        t.grad_value = grad_value; t.grad_loc = grad_sampling_locations; t.grad_attn = grad_attention_weights;
        return msda3_backward(p, t, workspace, (hipStream_t)stream);
      });
}

}  // extern "C"
