// dcn4_host.hip -- plan and execution of the DCNv4 operator (dcn4_plan.hpp): the sampling core's kernels (samp_core.hpp)
// instantiated with Dcn4Op -- and, for MDCONV_FLAG_SOFTMAX, with Dcn4SoftOp --, offset_mask in the values' type or in fp32.
// offset_mask is both the core's `coord` and its `factor`, grad_offset_mask both gradient tensors; the gather is the one
// every sampling operator shares.  The operator's C entry points (include/mdconv.h) follow, on the entry-point layer of
// samp_api.hpp.
#include "dcn4_plan.hpp"
#include "samp_api.hpp"

namespace mdconv {

// the list kernels depend on the coordinate type alone
#define DCN4_DISPATCH_CT(p, call)                              \
  do {                                                         \
    if ((p).coord_dtype == MDCONV_F32) call(MDCONV_F32);       \
    else if ((p).coord_dtype == MDCONV_F16) call(MDCONV_F16);  \
    else call(MDCONV_BF16);                                    \
  } while (0)

bool dcn4_plan(const mdconv_dcnv4_desc *d, bool backward, Dcn4Plan *p, const char **why) {
  *why = nullptr;
  const int64_t lim = (int64_t)1 << 31;
  const int esz = (int)dtype_bytes(d->dtype), csz = (int)dtype_bytes(d->coord_dtype);
  const int64_t Ho = dcn_out_size(d, 0), Wo = dcn_out_size(d, 1);
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
  q.skip_input = skip_input;
  q.softmax = (d->flags & MDCONV_FLAG_SOFTMAX) != 0;
  q.off_stats = 0;
  Bump ws = samp_plan_lists(q, backward, d->flags, skip_input, g.B * g.G, g.S_i, seg_stride);
  if (backward && !skip_input && q.softmax) {
    // (fda_plan's rule: the list kernels take a tap's weight from the statistics the coordinate kernel stored)
    q.off_stats = ws.take((size_t)Dcn4Op::npairs(g) * sizeof(float2));
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
  SAMP_DISPATCH(p, DCN4_BWD);
#undef DCN4_BWD
  if ((rc = check_launch("dcn4_soft_bwd_coord"))) return rc;
  if (p.skip_input) return MDCONV_OK;
  const SampGather ga = {g.B, g.S_i, g.S_o, g.G, g.D, g.C, g.ln, g.acc};
  return samp_lists_gather(L, ws, p.det, ga, p.dtype, t.grad_output, t.grad_input, stream,
                           [&](bool fill, int *cnt, const int *rowptr, void *entries) {
#define DCN4_LIST(CT) \
  samp_list_launch<Dcn4SoftOp, CT>(g, fill, t.offset_mask, t.offset_mask, cnt, rowptr, entries, L.seg_stride, stream)
    DCN4_DISPATCH_CT(p, DCN4_LIST);
#undef DCN4_LIST
  });
}

int dcn4_forward(const Dcn4Plan &p, const Dcn4Tensors &t, hipStream_t stream) {
  if (p.softmax) {
    const Dcn4SoftGeom sg = dcn4_soft_geom(p, nullptr);
#define DCN4_FWD(DT, CT) samp_fwd_launch<Dcn4SoftOp, DT, CT>(sg, t.input, t.offset_mask, t.offset_mask, t.output, stream)
    SAMP_DISPATCH(p, DCN4_FWD);
#undef DCN4_FWD
    return check_launch("dcn4_soft_fwd");
  }
#define DCN4_FWD(DT, CT) samp_fwd_launch<Dcn4Op, DT, CT>(p.g, t.input, t.offset_mask, t.offset_mask, t.output, stream)
  SAMP_DISPATCH(p, DCN4_FWD);
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
  SAMP_DISPATCH(p, DCN4_BWD);
#undef DCN4_BWD
  if ((rc = check_launch("dcn4_bwd_coord"))) return rc;
  if (p.skip_input) return MDCONV_OK;
  const SampGather ga = {g.B, g.S_i, g.S_o, g.G, g.D, g.C, g.ln, g.acc};
  return samp_lists_gather(L, ws, p.det, ga, p.dtype, t.grad_output, t.grad_input, stream,
                           [&](bool fill, int *cnt, const int *rowptr, void *entries) {
#define DCN4_LIST(CT) \
  samp_list_launch<Dcn4Op, CT>(g, fill, t.offset_mask, t.offset_mask, cnt, rowptr, entries, L.seg_stride, stream)
    DCN4_DISPATCH_CT(p, DCN4_LIST);
#undef DCN4_LIST
  });
}

// the descriptor's own validation; the shape rule is dcn4_plan's
static int dcn4_validate(const mdconv_dcnv4_desc *d, bool) {
  int rc;
  if ((rc = desc_dtypes("dcnv4", d)) || (rc = desc_dcn_geometry("dcnv4", d))) return rc;
  if (d->remove_center != 0 && d->remove_center != 1) {
    set_error("dcnv4: remove_center must be 0 or 1, is %d", d->remove_center);
    return MDCONV_EINVAL;
  }
  if (d->remove_center && (d->k_sz[0] % 2 == 0 || d->k_sz[1] % 2 == 0 || (d->k_sz[0] == 1 && d->k_sz[1] == 1))) {
    set_error("dcnv4: remove_center needs an odd kernel with a tap left (%d x %d)", d->k_sz[0], d->k_sz[1]);
    return MDCONV_EINVAL;
  }
  if ((rc = desc_modes("dcnv4", d, true))) return rc;
  return desc_finite("dcnv4", "offset_scale", d->offset_scale);
}
static const SampOp<mdconv_dcnv4_desc, Dcn4Plan> kDcn4 = {"dcnv4", dcn4_validate, dcn4_plan};

}  // namespace mdconv

using namespace mdconv;

extern "C" {

int mdconv_dcnv4_out_size(const mdconv_dcnv4_desc *d, int axis) {
  if (!d || axis < 0 || axis > 1 || d->stride[axis] <= 0) return -1;
  return (d->in_sz[axis] + 2 * d->pad[axis] - (d->dil[axis] * (d->k_sz[axis] - 1) + 1)) / d->stride[axis] + 1;
}

int mdconv_dcnv4_offset_mask_len(const mdconv_dcnv4_desc *d) {
  clear_error();
  if (dcn4_validate(d, false)) return -1;
  const long long K = (long long)d->k_sz[0] * d->k_sz[1] - d->remove_center;   // below 2^62
  if (K >= (1LL << 31) / 3 / d->groups) {   // G * K * 3 + 7 stays below 2^31
    set_error("dcnv4: a row of offset_mask has 2^31 elements or more");
    return -1;
  }
  return (int)dcn4_row_len(d->groups, K);
}

size_t mdconv_dcnv4_workspace_bytes(const mdconv_dcnv4_desc *d, int backward) {
  clear_error();
  return samp_workspace_bytes(kDcn4, d, backward);
}

int mdconv_dcnv4_forward(const mdconv_dcnv4_desc *d, const void *input, const void *offset_mask, void *output,
                         void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kDcn4, d, false, workspace, workspace_bytes,
      [&] {
        return check_args({{input, "input", 16}, {offset_mask, "offset_mask", dtype_bytes(d->coord_dtype)},
                           {output, "output", 16}});
      },
      [&](const Dcn4Plan &p) {
        Dcn4Tensors t = {};
        t.input = input; t.offset_mask = offset_mask; t.output = output;
        return dcn4_forward(p, t, (hipStream_t)stream);
      });
}

int mdconv_dcnv4_backward(const mdconv_dcnv4_desc *d, const void *input, const void *offset_mask, const void *grad_output,
                          void *grad_input, void *grad_offset_mask, void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kDcn4, d, true, workspace, workspace_bytes,
      [&] {
        const size_t cs = dtype_bytes(d->coord_dtype);
        return check_args({{input, "input", 16}, {offset_mask, "offset_mask", cs}, {grad_output, "grad_output", 16},
                           {grad_offset_mask, "grad_offset_mask", cs},
                           {grad_input, "grad_input", 16, !(d->flags & MDCONV_FLAG_NO_GRAD_INPUT)}});
      },
      [&](const Dcn4Plan &p) {
        Dcn4Tensors t = {};
        t.input = input; t.offset_mask = offset_mask; t.grad_output = grad_output;
        t.grad_input = grad_input; t.grad_offset_mask = grad_offset_mask;
        return dcn4_backward(p, t, workspace, (hipStream_t)stream);
      });
}

}  // extern "C"
