// dcn3_host.hip -- plan and execution of the DCNv3 core operator (dcn3_plan.hpp): the sampling core's kernels (samp_core.hpp)
// instantiated with Dcn3Op, coordinates in the values' type; and the operator's C entry points (include/mdconv.h) on the
// entry-point layer of samp_api.hpp.
#include "dcn3_plan.hpp"
#include "samp_api.hpp"

namespace mdconv {

// `call(DT, CT)` for the plan's type: the coordinates have the values', so three of the five pairings of SAMP_DISPATCH
// (which would instantiate the other two)
#define DCN3_DISPATCH(p, call)                                       \
  do {                                                               \
    if ((p).dtype == MDCONV_F32) call(MDCONV_F32, MDCONV_F32);       \
    else if ((p).dtype == MDCONV_F16) call(MDCONV_F16, MDCONV_F16);  \
    else call(MDCONV_BF16, MDCONV_BF16);                             \
  } while (0)

bool dcn3_plan(const mdconv_dcnv3_desc *d, bool backward, Dcn3Plan *p, const char **why) {
  *why = nullptr;
  const int64_t lim = (int64_t)1 << 31;
  const int esz = (int)dtype_bytes(d->dtype);
  const int64_t Ho = dcn_out_size(d, 0), Wo = dcn_out_size(d, 1);
  const int64_t K = (int64_t)d->k_sz[0] * d->k_sz[1];
  const int64_t C = (int64_t)d->groups * d->group_channels;
  const int64_t S_i = (int64_t)d->in_sz[0] * d->in_sz[1], S_o = Ho * Wo;
  const bool skip_input = backward && (d->flags & MDCONV_FLAG_NO_GRAD_INPUT);
  const int64_t seg_stride = K * S_o * 4;
  // (each product is checked with its factors bounded by the checks before it, so none overflows 64 bits)
  if (esz == 4 && d->group_channels % 4) *why = "group_channels is not a multiple of 4 (fp32 rows of 16 bytes)";
  else if (esz == 2 && d->group_channels % 8) *why = "group_channels is not a multiple of 8 (16-bit rows of 16 bytes)";
  else if (K > 4096) *why = "the kernel has more than 4096 taps";
  else if (C >= lim || S_i >= lim || S_o >= lim || d->batch * S_i >= lim || d->batch * S_o >= lim ||
           d->batch * S_i * C >= lim / esz || d->batch * S_o * C >= lim / esz ||
           d->batch * S_o * d->groups >= lim || d->batch * S_o * d->groups * K * 2 * esz >= lim)
    *why = "a tensor of the call has 2^31 bytes or more";
  else if (backward && !skip_input && (seg_stride >= lim || (int64_t)d->batch * d->groups > 65535))
    *why = "batch * groups exceeds 65535 or K * output pixels * 4 reaches 2^31 (the scatter lists of grad_input)";
  if (*why) return false;

  Dcn3Plan q = {};
  Dcn3Geom &g = q.g;
  g.B = d->batch; g.G = d->groups; g.D = d->group_channels; g.C = (int)C; g.K = (int)K;
  g.H = d->in_sz[0]; g.W = d->in_sz[1]; g.Ho = (int)Ho; g.Wo = (int)Wo; g.kh = d->k_sz[0]; g.kw = d->k_sz[1];
  g.sh = d->stride[0]; g.sw = d->stride[1]; g.ph = d->pad[0]; g.pw = d->pad[1]; g.dh = d->dil[0]; g.dw = d->dil[1];
  g.ch = (g.dh * (g.kh - 1)) >> 1;
  g.cw = (g.dw * (g.kw - 1)) >> 1;
  g.S_i = (int)S_i; g.S_o = (int)S_o; g.N = (int)(d->batch * S_o);
  g.ln = samp_lanes(g.D, esz);
  g.scale = d->offset_scale;
  g.acc = d->accumulate;
  q.dtype = d->dtype;
  q.skip_input = skip_input;
  samp_plan_lists(q, backward, d->flags, skip_input, g.B * g.G, g.S_i, seg_stride);
  *p = q;
  return true;
}

int dcn3_forward(const Dcn3Plan &p, const Dcn3Tensors &t, hipStream_t stream) {
#define DCN3_FWD(DT, CT) samp_fwd_launch<Dcn3Op, DT, CT>(p.g, t.input, t.offset, t.mask, t.output, stream)
  DCN3_DISPATCH(p, DCN3_FWD);
#undef DCN3_FWD
  return check_launch("dcn3_fwd");
}

int dcn3_backward(const Dcn3Plan &p, const Dcn3Tensors &t, void *ws, hipStream_t stream) {
  const Dcn3Geom &g = p.g;
  const ScatterLists &L = p.lists;
  int rc;
#define DCN3_BWD(DT, CT) \
  samp_bwd_coord_launch<Dcn3Op, DT, CT>(g, t.input, t.offset, t.mask, t.grad_output, t.grad_offset, t.grad_mask, stream)
  DCN3_DISPATCH(p, DCN3_BWD);
#undef DCN3_BWD
  if ((rc = check_launch("dcn3_bwd_coord"))) return rc;
  if (p.skip_input) return MDCONV_OK;
  const SampGather ga = {g.B, g.S_i, g.S_o, g.G, g.D, g.C, g.ln, g.acc};
  return samp_lists_gather(L, ws, p.det, ga, p.dtype, t.grad_output, t.grad_input, stream,
                           [&](bool fill, int *cnt, const int *rowptr, void *entries) {
#define DCN3_LIST(DT, CT) samp_list_launch<Dcn3Op, CT>(g, fill, t.offset, t.mask, cnt, rowptr, entries, L.seg_stride, stream)
    DCN3_DISPATCH(p, DCN3_LIST);
#undef DCN3_LIST
  });
}

// the descriptor's own validation; the shape rule is dcn3_plan's
static int dcn3_validate(const mdconv_dcnv3_desc *d, bool) {
  int rc;
  if ((rc = desc_dtype("dcnv3", d)) || (rc = desc_dcn_geometry("dcnv3", d)) || (rc = desc_modes("dcnv3", d))) return rc;
  return desc_finite("dcnv3", "offset_scale", d->offset_scale);
}
static const SampOp<mdconv_dcnv3_desc, Dcn3Plan> kDcn3 = {"dcnv3", dcn3_validate, dcn3_plan};

}  // namespace mdconv

using namespace mdconv;

extern "C" {

int mdconv_dcnv3_out_size(const mdconv_dcnv3_desc *d, int axis) {
  if (!d || axis < 0 || axis > 1 || d->stride[axis] <= 0) return -1;
  return (d->in_sz[axis] + 2 * d->pad[axis] - (d->dil[axis] * (d->k_sz[axis] - 1) + 1)) / d->stride[axis] + 1;
}

// (the one query that leaves the error text of the call before it in place when it succeeds)
size_t mdconv_dcnv3_workspace_bytes(const mdconv_dcnv3_desc *d, int backward) { return samp_workspace_bytes(kDcn3, d, backward); }

int mdconv_dcnv3_forward(const mdconv_dcnv3_desc *d, const void *input, const void *offset, const void *mask,
                         void *output, void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kDcn3, d, false, workspace, workspace_bytes,
      [&] {
        const size_t es = dtype_bytes(d->dtype);
        return check_args({{input, "input", 16}, {offset, "offset", es}, {mask, "mask", es}, {output, "output", 16}});
      },
      [&](const Dcn3Plan &p) {
        Dcn3Tensors t = {};
        t.input = input; t.offset = offset; t.mask = mask; t.output = output;
        return dcn3_forward(p, t, (hipStream_t)stream);
      });
}

int mdconv_dcnv3_backward(const mdconv_dcnv3_desc *d, const void *input, const void *offset, const void *mask,
                          const void *grad_output, void *grad_input, void *grad_offset, void *grad_mask,
                          void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kDcn3, d, true, workspace, workspace_bytes,
      [&] {
        const size_t es = dtype_bytes(d->dtype);
        return check_args({{input, "input", 16}, {offset, "offset", es}, {mask, "mask", es}, {grad_output, "grad_output", 16},
                           {grad_offset, "grad_offset", es}, {grad_mask, "grad_mask", es},
                           {grad_input, "grad_input", 16, !(d->flags & MDCONV_FLAG_NO_GRAD_INPUT)}});
      },
      [&](const Dcn3Plan &p) {
        Dcn3Tensors t = {};
        t.input = input; t.offset = offset; t.mask = mask; t.grad_output = grad_output;
        t.grad_input = grad_input; t.grad_offset = grad_offset; t.grad_mask = grad_mask;
        return dcn3_backward(p, t, workspace, (hipStream_t)stream);
      });
}

}  // extern "C"
