// droi_host.hip -- plan and execution of deformable RoI pooling (droi_plan.hpp): the family's own forward, offset-gradient
// and list kernels, the list builder and the channels-last gather of the sampling operators; and the operator's C entry
// points (include/mdconv.h) on the entry-point layer of samp_api.hpp.
#include "droi_plan.hpp"
#include "samp_api.hpp"

namespace mdconv {

bool droi_plan(const mdconv_droi_desc *d, bool backward, DroiPlan *p, const char **why) {
  *why = nullptr;
  const int64_t lim = (int64_t)1 << 31;
  const int esz = (int)dtype_bytes(d->dtype), csz = (int)dtype_bytes(d->coord_dtype);
  const int64_t gcap = d->sampling_ratio > 0 ? d->sampling_ratio : d->max_grid;   // 1..16
  const int64_t rows_in = (int64_t)d->batch * d->height;                           // times width below
  const int64_t bins = (int64_t)d->rois * d->pooled_h;                             // times pooled_w below
  const bool skip_input = backward && (d->flags & MDCONV_FLAG_NO_GRAD_INPUT);
  // (each product is checked with its factors bounded by the checks before it, so none overflows 64 bits)
  if (((int64_t)d->channels * esz) % 16) *why = "channels * element size is not a multiple of 16 (rows of 16-byte vectors)";
  else if (rows_in >= lim || rows_in * d->width >= lim || rows_in * d->width * d->channels >= lim / esz || bins >= lim ||
           bins * d->pooled_w >= lim || bins * d->pooled_w * d->channels >= lim / esz || bins * d->pooled_w * 2 * csz >= lim ||
           (int64_t)d->rois * 20 >= lim)
    *why = "a tensor of the call has 2^31 bytes or more";
  else if (bins * d->pooled_w * gcap * gcap * 4 >= lim)
    *why = "rois * pooled_h * pooled_w * grid^2 * 4 reaches 2^31 (grid = sampling_ratio, or max_grid when that is 0)";
  if (*why) return false;

  DroiPlan q = {};
  DroiGeom &g = q.g;
  g.B = d->batch; g.H = d->height; g.W = d->width; g.C = d->channels;
  g.R = d->rois; g.PH = d->pooled_h; g.PW = d->pooled_w;
  g.ratio = d->sampling_ratio; g.gcap = (int)gcap;
  g.nbins = (int)(bins * d->pooled_w);
  g.with_offset = d->with_offset != 0;
  g.acc = d->accumulate;
  g.scale = d->spatial_scale; g.gamma = d->gamma;
  g.ln = samp_lanes(g.C, esz);
  q.dtype = d->dtype;
  q.coord_dtype = d->coord_dtype;
  q.skip_input = skip_input;
  samp_plan_lists(q, backward, d->flags, skip_input, 1, g.B * g.H * g.W, (int64_t)g.nbins * g.gcap * g.gcap * 4);
  *p = q;
  return true;
}

int droi_forward(const DroiPlan &p, const DroiTensors &t, hipStream_t stream) { return droi_fwd_launch(p, t, stream); }

int droi_backward(const DroiPlan &p, const DroiTensors &t, void *ws, hipStream_t stream) {
  const DroiGeom &g = p.g;
  const ScatterLists &L = p.lists;
  int rc;
  if (g.with_offset && (rc = droi_bwd_offset_launch(p, t, stream))) return rc;
  if (p.skip_input) return MDCONV_OK;
  const SampGather ga = {1, g.B * g.H * g.W, g.nbins, 1, g.C, g.C, g.ln, g.acc};
  return samp_lists_gather(L, ws, p.det, ga, p.dtype, t.grad_output, t.grad_input, stream,
                           [&](bool fill, int *cnt, const int *rowptr, void *entries) {
    droi_list_launch(p, t, fill, cnt, rowptr, entries, stream);
  });
}

// the descriptor's own validation; the shape rule is droi_plan's
static int droi_validate(const mdconv_droi_desc *d, bool backward) {
  int rc;
  if ((rc = desc_dtypes("droi", d))) return rc;
  if (d->batch <= 0 || d->channels <= 0 || d->height <= 0 || d->width <= 0 || d->rois <= 0 || d->pooled_h <= 0 ||
      d->pooled_w <= 0) {
    set_error("droi: batch, channels, height, width, rois, pooled_h and pooled_w must be positive (%d, %d, %d, %d, %d, %d, %d)",
              d->batch, d->channels, d->height, d->width, d->rois, d->pooled_h, d->pooled_w);
    return MDCONV_EINVAL;
  }
  if (d->sampling_ratio < 0 || d->sampling_ratio > 16) {
    set_error("droi: sampling_ratio must be 0 (adaptive) or 1..16, is %d", d->sampling_ratio);
    return MDCONV_EINVAL;
  }
  if (d->max_grid < 1 || d->max_grid > 16) {
    set_error("droi: max_grid must be 1..16, is %d", d->max_grid);
    return MDCONV_EINVAL;
  }
  if ((rc = desc_finite("droi", "spatial_scale", d->spatial_scale)) || (rc = desc_finite("droi", "gamma", d->gamma)) ||
      (rc = desc_modes("droi", d)))
    return rc;
  if (backward && !d->with_offset && (d->flags & MDCONV_FLAG_NO_GRAD_INPUT)) {
    set_error("droi: a backward with with_offset == 0 and MDCONV_FLAG_NO_GRAD_INPUT has nothing to compute");
    return MDCONV_EINVAL;
  }
  return MDCONV_OK;
}
static const SampOp<mdconv_droi_desc, DroiPlan> kDroi = {"droi", droi_validate, droi_plan};

}  // namespace mdconv

using namespace mdconv;

extern "C" {

size_t mdconv_droi_workspace_bytes(const mdconv_droi_desc *d, int backward) {
  clear_error();
  return samp_workspace_bytes(kDroi, d, backward);
}

int mdconv_droi_forward(const mdconv_droi_desc *d, const void *input, const void *rois, const void *offset, void *output,
                        void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kDroi, d, false, workspace, workspace_bytes,
      [&] {
        return check_args({{input, "input", 16}, {rois, "rois", 4}, {output, "output", 16},
                           {offset, "offset", dtype_bytes(d->coord_dtype), d->with_offset != 0}});
      },
      [&](const DroiPlan &p) {
        DroiTensors t = {};
        t.input = input; t.rois = rois; t.offset = offset; t.output = output;
        return droi_forward(p, t, (hipStream_t)stream);
      });
}

int mdconv_droi_backward(const mdconv_droi_desc *d, const void *input, const void *rois, const void *offset,
                         const void *grad_output, void *grad_input, void *grad_offset, void *workspace,
                         size_t workspace_bytes, void *stream) {
  clear_error();
  return samp_entry(
      kDroi, d, true, workspace, workspace_bytes,
      [&] {
        const size_t cs = dtype_bytes(d->coord_dtype);
        const bool off = d->with_offset != 0;
        return check_args({{input, "input", 16}, {rois, "rois", 4}, {grad_output, "grad_output", 16},
                           {offset, "offset", cs, off}, {grad_offset, "grad_offset", cs, off},
                           {grad_input, "grad_input", 16, !(d->flags & MDCONV_FLAG_NO_GRAD_INPUT)}});
      },
      [&](const DroiPlan &p) {
        DroiTensors t = {};
        t.input = input; t.rois = rois; t.offset = offset; t.grad_output = grad_output;
        t.grad_input = grad_input; t.grad_offset = grad_offset;
        return droi_backward(p, t, workspace, (hipStream_t)stream);
      });
}

}  // extern "C"
