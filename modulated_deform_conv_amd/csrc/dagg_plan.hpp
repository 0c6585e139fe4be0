// dagg_plan.hpp -- deformable aggregation (include/mdconv_dagg.h): key-point features pulled out of `cams` cameras x L
// pyramid levels in one call, on channels-last tensors, fp32 / fp16 / bf16 values with coordinates in the same type or in
// fp32.  A kernel family of its own (dagg_fwd.hip, dagg_bwd.hip, dagg_list.hip, dagg_gather.hip), NOT a policy of the
// sampling core: one location per (anchor, point, camera) is shared by all levels and all channel groups, so the owner of a
// walk is the ANCHOR -- its whole channel row -- and not an (anchor, group) pair, the weight is per lane (its group's), and
// the location's gradient is a sum over every lane and level of the anchor.  What the family takes from
// the core as it stands: the lane mapping (SampLanes, samp_lanes, samp_grid, samp_lane_of) with the anchor's row as the
// "head", the 16-byte vector helpers (samp_ld / samp_st, samp_pack / samp_unpack, kSampOob, the raw buffer loads), the
// corner rule (samp_sample, samp_corner_read / _pixel / _weight / _dx / _dy) and the list builder (scatter_lists_take /
// scatter_lists_build / csr_sort_rows).
//   anchor = b * A + a                 the owner; its V = C * esz / 16 channel vectors are VL adjacent lanes (rounds beyond 64)
//   unit   = p * cams + cam            one location, one gate; U = P * cams units per anchor
//   anchor * U + unit                  half the element index of the location's x; the gate is 0 < x < 1 and 0 < y < 1
//   id = (anchor * U + unit) * L + l   a sample; id * G + g is the element index of `weights`
// A call is planned ONCE: dagg_plan() decides whether the family takes it and lays its workspace out, the byte count
// reported to the caller is the plan's `total`, and dagg_forward / dagg_backward take the plan.
#pragma once
#include "../../include/mdconv_dagg.h"
#include "samp_core.hpp"

namespace mdconv {

// Device-side geometry (POD, passed by value as a kernel argument).  The level table is read with constant indices only
// (dagg_level: an unrolled select chain on the loop's level), so it stays in scalar registers.
struct DaggGeom {
  int B, cams, L, C, G, Dg, A, P;   // C = G * Dg
  int U;                            // P * cams: the units of an anchor
  int S_cam, S;                     // feature rows per camera and per image (S = cams * S_cam)
  int nanchors;                     // B * A
  int VG;                           // 16-byte vectors per group
  int seg;                          // 1: VG is a power of two of at most VL, a group is an aligned run of lanes of one round
  SampLanes ln;                     // of the anchor's row: V = C * esz / 16
  int acc;                          // backward: 1 = add to the caller's gradient buffers, 0 = overwrite
  int lvH[MDCONV_MSDA_MAX_LEVELS], lvW[MDCONV_MSDA_MAX_LEVELS];   // extents, the same for every camera
  int lvS[MDCONV_MSDA_MAX_LEVELS];                               // start row inside a camera
};

struct DaggTensors {
  const void *feature, *loc, *wts, *grad_output;
  void *output, *grad_feature, *grad_loc, *grad_wts;
};

struct DaggPlan {
  DaggGeom g;
  int dtype, coord_dtype;   // MDCONV_F32 / MDCONV_F16 / MDCONV_BF16
  bool backward;
  bool det;                 // MDCONV_FLAG_DETERMINISTIC: the lists are sorted before the gather
  bool skip_feature;        // MDCONV_FLAG_NO_GRAD_INPUT: no lists, no sort, no gather, no workspace
  ScatterLists lists;       // grad_feature: per image a segment of S lists shared by all groups, A * U * L * 4 entries
  size_t total;             // workspace bytes
};

// false: outside the shape rule; *why names the rule it breaks.  The descriptor has passed validation (dagg_host.hip).
bool dagg_plan(const mdconv_dagg_desc *d, bool backward, DaggPlan *p, const char **why);
int dagg_forward(const DaggPlan &p, const DaggTensors &t, hipStream_t stream);
int dagg_backward(const DaggPlan &p, const DaggTensors &t, void *ws, hipStream_t stream);

// the kernels (dagg_fwd.hip, dagg_bwd.hip, dagg_list.hip, dagg_gather.hip), by the plan's (value type, coordinate type)
int dagg_fwd_launch(const DaggPlan &p, const DaggTensors &t, hipStream_t stream);
int dagg_bwd_coord_launch(const DaggPlan &p, const DaggTensors &t, hipStream_t stream);
void dagg_list_launch(const DaggPlan &p, const DaggTensors &t, bool fill, int *cnt, const int *rowptr, void *entries,
                      hipStream_t stream);
int dagg_gather_launch(const DaggPlan &p, const DaggTensors &t, const int *rowptr, const void *entries, hipStream_t stream);


#ifdef __HIPCC__
// ---- the unit: one stored location and its gate, as the lanes of an anchor share it ----
// The gate is taken on the stored elements, converted exactly to fp32, before any arithmetic: IN iff 0 < x < 1 and
// 0 < y < 1, so NaN, +-Inf, exactly 0 and exactly 1 are OUT.  A unit that is gated out reads nothing further.
struct DaggUnit {
  float x, y;
  int in;
};
template <int CT> __device__ __forceinline__ DaggUnit dagg_unit(const void *loc, int au, bool on) {
  DaggUnit u;
  u.x = u.y = 0.f;
  u.in = 0;
  if (on) {
    u.x = samp_ld<CT>(loc, 2 * au);
    u.y = samp_ld<CT>(loc, 2 * au + 1);
    u.in = u.x > 0.f && u.x < 1.f && u.y > 0.f && u.y < 1.f;
  }
  return u;
}
// the unit lane `src` of the wave built
__device__ __forceinline__ DaggUnit dagg_unit_from(const DaggUnit &mine, int src) {
  DaggUnit u;
  u.x = __shfl(mine.x, src, 64);
  u.y = __shfl(mine.y, src, 64);
  u.in = __shfl(mine.in, src, 64);
  return u;
}
// extents and start row (inside a camera) of level `l` (0 <= l < L <= 8): constant indices into the kernel argument
__device__ __forceinline__ void dagg_level(const DaggGeom &g, int l, int &H, int &W, int &start) {
  H = g.lvH[0]; W = g.lvW[0]; start = g.lvS[0];
#pragma unroll
  for (int i = 1; i < MDCONV_MSDA_MAX_LEVELS; ++i)
    if (l == i) { H = g.lvH[i]; W = g.lvW[i]; start = g.lvS[i]; }
}
// The sample of a gated-in unit on a level of H x W: pixel coordinates x * W - 0.5, y * H - 0.5, one fused rounding each,
// once for the three kernels so they agree to the bit.  Inside the gate they lie in (-0.5, size - 0.5], which passes
// samp_sample's own gate; the corner rule (a corner outside the map is not read) is the core's.
__device__ __forceinline__ void dagg_sample(const DaggUnit &u, int H, int W, SampSample &s) {
  samp_sample(fmaf(u.y, (float)H, -0.5f), fmaf(u.x, (float)W, -0.5f), H, W, s);
}
// the byte offsets of the four corners in `feature` (row_bytes = C * esz) from the row of pixel (0, 0) of the map, kSampOob
// for a corner that is not read: a parked corner's load gives zeros, so no weight carries a validity factor
__device__ __forceinline__ void dagg_corner_offs(const SampSample &s, int H, int W, int map_row, unsigned row_bytes,
                                                 unsigned (&off)[4]) {
#pragma unroll
  for (int ci = 0; ci < 4; ++ci)
    off[ci] = samp_corner_read(s, ci, H, W) ? (unsigned)(map_row + samp_corner_pixel(s, ci, W)) * row_bytes : (unsigned)kSampOob;
}
#endif  // __HIPCC__

}  // namespace mdconv
