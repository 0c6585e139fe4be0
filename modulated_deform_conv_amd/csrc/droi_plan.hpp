// droi_plan.hpp -- deformable RoI pooling (include/mdconv.h "Deformable RoI pooling"): RoIAlign whose bins are shifted by a
// learnt offset, on channels-last tensors, fp32 / fp16 / bf16 values with offsets in the same type or in fp32.  A small
// kernel family of its own beside the sampling core (samp_core.hpp), of which it uses the generic pieces only -- the lane
// mapping, the 16-byte vector helpers, the list builder and the channels-last gather.  The operator itself does not fit the
// core's policy interface: the number of samples of a bin varies per RoI, the coordinate gradient is one (x, y) pair per BIN
// (summed over samples and channels), and the border rule is RoIAlign's clamp, not the zero-padding gate of samp_sample.
// A call is planned ONCE: droi_plan() decides whether the family takes it and lays its workspace out, the byte count
// reported to the caller is the plan's `total`, and droi_forward / droi_backward take the plan.
#pragma once
#include "samp_core.hpp"

namespace mdconv {

// Device-side geometry (POD, passed by value as a kernel argument).
struct DroiGeom {
  int B, H, W, C, R, PH, PW;
  int ratio, gcap;       // sampling_ratio (0 = adaptive) and the bound of the grid per axis: ratio, or max_grid
  int nbins;             // R * PH * PW
  int with_offset, acc;  // acc: backward write mode, 1 = add to the caller's gradient buffers, 0 = overwrite
  float scale, gamma;
  SampLanes ln;          // of a bin's C channels
};

struct DroiTensors {
  const void *input, *rois, *offset, *grad_output;
  void *output, *grad_input, *grad_offset;
};

struct DroiPlan {
  DroiGeom g;
  int dtype, coord_dtype;   // MDCONV_F32 / MDCONV_F16 / MDCONV_BF16
  bool backward;
  bool det;                 // MDCONV_FLAG_DETERMINISTIC: the lists are sorted before the gather
  bool skip_input;          // MDCONV_FLAG_NO_GRAD_INPUT: no lists, no sort, no gather, no workspace
  ScatterLists lists;       // grad_input: ONE segment of B*H*W lists, R*PH*PW*gcap*gcap*4 entries
  size_t total;             // workspace bytes
};

// false: outside the shape rule; *why names the rule it breaks.  The descriptor has passed validation (the operator's *_host.hip).
bool droi_plan(const mdconv_droi_desc *d, bool backward, DroiPlan *p, const char **why);
int droi_forward(const DroiPlan &p, const DroiTensors &t, hipStream_t stream);
int droi_backward(const DroiPlan &p, const DroiTensors &t, void *ws, hipStream_t stream);

// the kernels (droi_fwd.hip, droi_bwd.hip, droi_list.hip), by the plan's (value type, coordinate type)
int droi_fwd_launch(const DroiPlan &p, const DroiTensors &t, hipStream_t stream);
int droi_bwd_offset_launch(const DroiPlan &p, const DroiTensors &t, hipStream_t stream);
void droi_list_launch(const DroiPlan &p, const DroiTensors &t, bool fill, int *cnt, const int *rowptr, void *entries,
                      hipStream_t stream);


#ifdef __HIPCC__
// ---- the arithmetic the three kernels share, so that they agree bit for bit on every sample ----
// What the samples of a bin have in common.  `ok` false: the RoI contributes nothing (gh = gw = 0 then, so no walk runs).
struct DroiBin {
  bool ok;
  int img_row;     // b * H * W: the row of pixel (0, 0) of the RoI's image
  int gh, gw;      // the RoI's grid
  float y0, x0;    // y(iy) = y0 + (iy + 0.5) * sy, x(ix) = x0 + (ix + 0.5) * sx
  float sy, sx;
  float inv_cnt;   // 1 / max(gh * gw, 1)
  float fy, fx;    // d y / d offset = gamma * rh, d x / d offset = gamma * rw
};
__device__ __forceinline__ bool droi_finite(float v) { return v - v == 0.f; }
__device__ __forceinline__ int droi_grid(const DroiGeom &g, float bin) {
  if (g.ratio > 0) return g.ratio;
  // (clamped as a float: NaN and wild sizes never reach the int conversion; fmaxf(NaN, 0) is 0)
  return (int)fminf(fmaxf(ceilf(bin), 0.f), (float)g.gcap);
}
// bin = (r * PH + ph) * PW + pw; the offset elements of the bin are r*2*PH*PW + ph*PW + pw (x) and that + PH*PW (y)
template <int CT>
__device__ __forceinline__ void droi_bin(const DroiGeom &g, const float *__restrict__ rois, const void *__restrict__ offset,
                                         int bin, DroiBin &q) {
  const int npb = g.PH * g.PW;
  const int r = bin / npb, cell = bin - r * npb;
  const int ph = cell / g.PW, pw = cell - ph * g.PW;
  const float f0 = rois[5 * r], x1 = rois[5 * r + 1], y1 = rois[5 * r + 2], x2 = rois[5 * r + 3], y2 = rois[5 * r + 4];
  const bool fin = droi_finite(f0) && droi_finite(x1) && droi_finite(y1) && droi_finite(x2) && droi_finite(y2);
  q.ok = fin && f0 >= 0.f && f0 < (float)g.B && f0 == floorf(f0);
  const int b = q.ok ? (int)f0 : 0;
  q.img_row = b * g.H * g.W;
  const float x1s = x1 * g.scale - 0.5f, y1s = y1 * g.scale - 0.5f;
  const float x2s = x2 * g.scale - 0.5f, y2s = y2 * g.scale - 0.5f;
  const float rw = x2s - x1s, rh = y2s - y1s;
  const float bw = rw / (float)g.PW, bh = rh / (float)g.PH;
  q.gh = q.ok ? droi_grid(g, bh) : 0;
  q.gw = q.ok ? droi_grid(g, bw) : 0;
  q.inv_cnt = 1.f / (float)max(q.gh * q.gw, 1);
  float ox = 0.f, oy = 0.f;
  if (g.with_offset) {
    const int e = r * 2 * npb + cell;
    ox = samp_ld<CT>(offset, e);
    oy = samp_ld<CT>(offset, e + npb);
  }
  q.fx = g.gamma * rw;
  q.fy = g.gamma * rh;
  q.x0 = x1s + q.fx * ox + (float)pw * bw;
  q.y0 = y1s + q.fy * oy + (float)ph * bh;
  q.sx = bw / (float)max(q.gw, 1);
  q.sy = bh / (float)max(q.gh, 1);
}

// One axis of RoIAlign's sample at `loc` on an axis of `size` pixels.
struct DroiAxis {
  bool in;     // the gate: -1 <= loc <= size (NaN fails)
  bool free;   // the coordinate is not clamped (0 <= loc < size-1): the derivative along this axis is not zero
  int lo;      // low neighbour, 0..size-1; the high one is lo + 1 where `free`, else coincides and carries weight 0
  float l;     // fractional part
};
__device__ __forceinline__ DroiAxis droi_axis(float loc, int size) {
  DroiAxis a;
  a.in = loc >= -1.f && loc <= (float)size;
  const float c = a.in ? fmaxf(loc, 0.f) : 0.f;   // (gated before the int conversion)
  const float fl = floorf(c);
  const int lo = (int)fl;
  const bool top = lo >= size - 1;
  a.lo = top ? size - 1 : lo;
  a.l = top ? 0.f : c - fl;
  a.free = a.in && loc >= 0.f && !top;
  return a;
}
// Is corner ci = 2*cy + cx of the sample read?  The high neighbour of an axis whose low one is the last pixel coincides with
// it and carries weight 0: it is parked, so nothing outside the image is ever addressed.
__device__ __forceinline__ bool droi_corner_read(const DroiAxis &ay, const DroiAxis &ax, int ci, int H, int W) {
  return ay.in && ax.in && ay.lo + (ci >> 1) < H && ax.lo + (ci & 1) < W;
}
#endif  // __HIPCC__

}  // namespace mdconv
