// msdap_plan.hpp -- multi-scale deformable attention with a point count per level (include/mdconv_msdap.h): the operator of
// msda_plan.hpp whose levels each own points[l] taps, as RT-DETRv2's num_points_list has it (D-FINE / DEIM: (3, 6, 3)).  The
// sampling core (samp_core.hpp) under the policy MsdapOp below, which is MsdaOp but for ONE thing: the level of a tap.  The taps
// are level-major, K = sum_l points[l], pair * K + tap is the element index of attention_weights as before, and a tap's level
// comes from the exclusive prefix sums of the counts instead of tap / P.  Planned once like its parent: msdap_plan() decides
// whether the family takes the call and lays its workspace out.
#pragma once
#include "../../include/mdconv_msdap.h"
#include "msda_plan.hpp"

namespace mdconv {

// MsdaGeom (whose P has no meaning here and is 0) and the exclusive prefix sums of the point counts: pfx[l] is the first tap
// of level l, and K for the levels not in use, so no tap reaches them.  Like the level table it is read with constant indices
// only (MsdapOp::level_of_tap), so it stays in scalar registers.
struct MsdapGeom : MsdaGeom {
  int pfx[MDCONV_MSDA_MAX_LEVELS];
};

struct MsdapPlan {
  MsdapGeom g;
  int dtype, coord_dtype;   // MDCONV_F32 / MDCONV_F16 / MDCONV_BF16
  bool backward;
  bool det;                 // MDCONV_FLAG_DETERMINISTIC: the lists are sorted before the gather
  bool skip_value;          // MDCONV_FLAG_NO_GRAD_INPUT: no lists, no sort, no gather, no workspace
  ScatterLists lists;       // grad_value: per (image, head) a segment of S lists, K * Lq * 4 entries
  size_t total;             // workspace bytes
};

// false: outside the shape rule; *why names the rule it breaks.  The descriptor has passed validation (msdap_host.hip).
bool msdap_plan(const mdconv_msdap_desc *d, bool backward, MsdapPlan *p, const char **why);
int msdap_forward(const MsdapPlan &p, const MsdaTensors &t, hipStream_t stream);
int msdap_backward(const MsdapPlan &p, const MsdaTensors &t, void *ws, hipStream_t stream);


#ifdef __HIPCC__
// The policy: everything of MsdaOp that does not ask for a tap's level is inherited as it stands (MsdapGeom is an MsdaGeom);
// tap_state and list_item_at do, and build_tap and list_item are restated only because they name those two.
struct MsdapOp : MsdaOp {
  typedef MsdapGeom Geom;

  // Extents and start row of the level that owns `tap` (0 <= tap < K).  The level is the number of i in 1..7 with
  // tap >= pfx[i]: seven compares against scalars and their sum, in place of an integer division by a run-time P, and then
  // the select chain of MsdaOp::level.  (Selecting the row in the compare chain itself -- pfx never decreases, so the last i
  // that holds wins -- saves the sum and costs registers: the bf16 coordinate backward takes 97 VGPRs that way, 95 this way,
  // which is the step from 5 waves per SIMD to 4; profiles/msdap.md.)
  static __device__ __forceinline__ void level_of_tap(const Geom &g, int tap, int &H, int &W, int &start) {
    int l = 0;
#pragma unroll
    for (int i = 1; i < MDCONV_MSDA_MAX_LEVELS; ++i) l += tap >= g.pfx[i];
    level(g, l, H, W, start);
  }
  template <int CT>
  static __device__ __forceinline__ void build_tap(const Geom &g, const Ctx &pair_byte, int pair, int tap, bool on, const void *loc,
                                                   const void *attn, SampTap &t, float &fx, float &fy) {
    samp_tap_clear(t);
    fx = fy = 1.f;
    if (!on) return;
    tap_state<CT>(g, pair_byte, tap, loc, coord_index(g, pair_byte, pair, tap, 0), attn, factor_index(g, pair_byte, pair, tap), t,
                  fx, fy);
  }
  // MsdaOp::tap_state with the level found by level_of_tap
  template <int CT>
  static __device__ __forceinline__ void tap_state(const Geom &g, const Ctx &pair_byte, int tap, const void *loc, int ec,
                                                   const void *attn, int ef, SampTap &t, float &fx, float &fy) {
    int H, W, start;
    level_of_tap(g, tap, H, W, start);
    fx = (float)W;
    fy = (float)H;
    SampSample s;
    position<CT>(loc, ec, H, W, s);
    t.lx = s.lx;
    t.ly = s.ly;
    t.m = samp_ld<CT>(attn, ef);
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
      if (samp_corner_read(s, ci, H, W)) t.off[ci] = pair_byte + (start + samp_corner_pixel(s, ci, W)) * g.C * g.ln.esz;
  }
  // MsdaOp::list_item_at with the level found by level_of_tap
  template <int CT>
  static __device__ __forceinline__ void list_item_at(const Geom &g, int pair, int tap, const void *loc, int ec, SampItem &it) {
    const int nq = pair / g.M, m = pair - nq * g.M;
    const int n = nq / g.Lq, q = nq - n * g.Lq;
    it.seg = n * g.M + m;
    it.tap = tap; it.q = q; it.rows_out = g.Lq;
    level_of_tap(g, tap, it.H, it.W, it.row0);
    position<CT>(loc, ec, it.H, it.W, it.s);
  }
  template <int CT> static __device__ __forceinline__ void list_item(const Geom &g, int id, const void *loc, SampItem &it) {
    const int pair = id / g.K, tap = id - pair * g.K;
    list_item_at<CT>(g, pair, tap, loc, 2 * id, it);
  }
};
#endif  // __HIPCC__

}  // namespace mdconv
