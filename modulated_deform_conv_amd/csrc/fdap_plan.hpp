// fdap_plan.hpp -- packed deformable attention with a point count per level (include/mdconv_fdap.h): the operator of
// msdap_plan.hpp (levels that each own points[l] taps, level-major, K = sum_l points[l]) with the packed tensor and the
// in-kernel softmax of fda_plan.hpp -- sampling_loc_attn [N, Lq, M, 3K], per (query, head) the 2K location coordinates and
// then the K attention LOGITS.  The sampling core (samp_core.hpp) under the policy FdapOp below, which is to MsdapOp what FdaOp
// is to MsdaOp: MsdapOp's pairs, prefix-sum level lookup, positions and list items, with the addressing of the packed row and
// a factor that is a function of the pair's logits.  Nothing of either parent is restated: the weight is fda_weight, the
// context FdaPair, the tap state and the list item MsdapOp's.  Planned once like its siblings: fdap_plan() decides whether
// the family takes the call (msdap_plan's rule plus the packed tensor's size) and lays its workspace out.
#pragma once
#include "../../include/mdconv_fdap.h"
#include "fda_plan.hpp"
#include "msdap_plan.hpp"

namespace mdconv {

// Device-side geometry (POD, passed by value as a kernel argument): MSDAP's (level table and prefix sums, both read with
// constant indices only, so both stay in scalar registers), the row length, and where the per-pair softmax statistics go.
struct FdapGeom : MsdapGeom {
  int K3;          // 3 * K: the elements of a (query, head)
  float2 *stats;   // backward with grad_value: (max, 1 / sum) per pair, in the workspace; else nullptr
};

struct FdapPlan {
  FdapGeom g;               // (g.stats is set by fdap_backward, from the workspace it is handed)
  int dtype, coord_dtype;   // MDCONV_F32 / MDCONV_F16 / MDCONV_BF16
  bool backward;
  bool det;                 // MDCONV_FLAG_DETERMINISTIC: the lists are sorted before the gather
  bool skip_value;          // MDCONV_FLAG_NO_GRAD_INPUT: no lists, no statistics, no sort, no gather, no workspace
  ScatterLists lists;       // grad_value: MSDAP's lists of the same shape
  size_t off_stats;         // 8 bytes per pair behind the lists
  size_t total;             // workspace bytes
};

// false: outside the shape rule; *why names the rule it breaks.  The descriptor has passed validation (fdap_host.hip).
bool fdap_plan(const mdconv_fdap_desc *d, bool backward, FdapPlan *p, const char **why);
int fdap_forward(const FdapPlan &p, const FdaTensors &t, hipStream_t stream);
int fdap_backward(const FdapPlan &p, const FdaTensors &t, void *ws, hipStream_t stream);

#ifdef __HIPCC__
// The operator policy of the sampling core: coord = factor = sampling_loc_attn, sampled tensor = value.  FdaOp's members with
// MsdapOp in the place of MsdaOp: where a (pair, tap) lives in the row and the softmax are FdaOp's, the level of a tap comes
// from the prefix sums (MsdapOp::tap_state / list_item_at).
struct FdapOp {
  typedef FdapGeom Geom;
  typedef FdaPair Ctx;
  static constexpr bool kPairSum = true;
  static __host__ __device__ __forceinline__ int npairs(const Geom &g) { return MsdapOp::npairs(g); }
  static __device__ __forceinline__ size_t sampled_bytes(const Geom &g) { return MsdapOp::sampled_bytes(g); }
  static __device__ __forceinline__ int list_rows(const Geom &g) { return MsdapOp::list_rows(g); }

  static __device__ __forceinline__ Ctx ctx(const Geom &g, int pair) {
    Ctx p;
    p.byte = MsdapOp::ctx(g, pair);
    p.mx = 0.f;
    p.inv = 1.f;
    return p;
  }
  // the pair's 3K elements: (x, y) of tap 0 .. K-1, then the K logits
  static __device__ __forceinline__ int coord_index(const Geom &g, const Ctx &, int pair, int tap, int xy) {
    return pair * g.K3 + 2 * tap + xy;
  }
  static __device__ __forceinline__ int factor_index(const Geom &g, const Ctx &, int pair, int tap) {
    return pair * g.K3 + 2 * g.K + tap;
  }
  static __device__ __forceinline__ int list_factor_index(const Geom &g, int id) {
    const int pair = id / g.K, tap = id - pair * g.K;
    return pair * g.K3 + 2 * g.K + tap;
  }
  // FdaOp::begin_pair over this row: lane j takes the logits j, j + VL, ... below K -- a lane with none (K < VL) and the taps
  // from K on enter neither the maximum nor the sum -- and two xor butterflies leave every lane with the same bits.  fp32
  // and max-subtracted.  Where the lists will need them (g.stats) the pair's lane 0 stores the two.
  template <int CT>
  static __device__ __forceinline__ void begin_pair(const Geom &g, Ctx &cx, const SampLane &ln, const void *om) {
    const int e0 = ln.pair * g.K3 + 2 * g.K;
    float mx = -INFINITY;
    for (int tap = ln.j; tap < g.K; tap += g.ln.VL) mx = fmaxf(mx, samp_ld<CT>(om, e0 + tap));
    for (int d = g.ln.VL >> 1; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
    float sum = 0.f;
    for (int tap = ln.j; tap < g.K; tap += g.ln.VL) sum += expf(samp_ld<CT>(om, e0 + tap) - mx);
    for (int d = g.ln.VL >> 1; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    cx.mx = mx;
    cx.inv = 1.f / sum;
    if (g.stats && ln.live && ln.j == 0) g.stats[ln.pair] = make_float2(cx.mx, cx.inv);
  }
  template <int CT>
  static __device__ __forceinline__ void build_tap(const Geom &g, const Ctx &cx, int pair, int tap, bool on, const void *om,
                                                   const void *, SampTap &t, float &fx, float &fy) {
    samp_tap_clear(t);
    fx = fy = 1.f;
    if (!on) return;
    MsdapOp::tap_state<CT>(g, cx.byte, tap, om, coord_index(g, cx, pair, tap, 0), om, factor_index(g, cx, pair, tap), t, fx, fy);
    t.m = fda_weight(t.m, cx.mx, cx.inv);   // (tap_state left the logit there)
  }
  // d(sum_s a[s] g[s]) / d(logit t) = a[t] * (g[t] - sum_s a[s] g[s]); a gated-out tap has g[t] = 0 and keeps -a[t] * S
  static __device__ __forceinline__ float factor_grad(float a, float gsum, float s_pair) { return a * (gsum - s_pair); }
  template <int CT> static __device__ __forceinline__ void finish_pair(const Geom &, const Ctx &, const SampLane &, void *) {}
  // thread = sample: the weight from the statistics the coordinate kernel stored, not from a reduction per thread
  static __device__ __forceinline__ float list_factor(const Geom &g, int id, float logit) {
    const float2 st = g.stats[id / g.K];
    return fda_weight(logit, st.x, st.y);
  }
  // sample id = pair * K + tap
  template <int CT> static __device__ __forceinline__ void list_item(const Geom &g, int id, const void *om, SampItem &it) {
    const int pair = id / g.K, tap = id - pair * g.K;
    MsdapOp::list_item_at<CT>(g, pair, tap, om, pair * g.K3 + 2 * tap, it);
  }
};
#endif  // __HIPCC__

}  // namespace mdconv
