// droi_host.hip -- plan and execution of deformable RoI pooling (droi_plan.hpp): the family's own forward, offset-gradient
// and list kernels, the list builder and the channels-last gather of the sampling operators.
#include "droi_plan.hpp"

namespace mdconv {

bool droi_plan(const mdconv_droi_desc *d, bool backward, DroiPlan *p, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = nullptr;
  const int64_t lim = (int64_t)1 << 31;
  const int esz = d->dtype == MDCONV_F32 ? 4 : 2;
  const int csz = d->coord_dtype == MDCONV_F32 ? 4 : 2;
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
  q.backward = backward;
  q.det = backward && (d->flags & MDCONV_FLAG_DETERMINISTIC);
  q.skip_input = skip_input;
  q.total = 0;
  if (backward && !skip_input) {
    Bump ws;
    q.lists = scatter_lists_take(ws, 1, g.B * g.H * g.W, (int64_t)g.nbins * g.gcap * g.gcap * 4, q.det);
    q.total = ws.off;
  }
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
  rc = scatter_lists_build(L, ws, p.det, stream, [&](bool fill, int *cnt, const int *rowptr, void *entries) {
    droi_list_launch(p, t, fill, cnt, rowptr, entries, stream);
  });
  if (rc) return rc;
  const SampGather ga = {1, g.B * g.H * g.W, g.nbins, 1, g.C, g.C, g.ln, g.acc};
  return samp_gather_launch(ga, p.dtype, L.seg_stride, t.grad_output, (const int *)((char *)ws + L.off_rowptr),
                            (char *)ws + L.off_entries, t.grad_input, stream);
}

}  // namespace mdconv
