// fda_plan.hpp -- packed deformable attention (include/mdconv.h "Packed deformable attention"): multi-scale deformable
// attention with ONE packed coordinate tensor -- sampling_loc_attn [N, Lq, M, 3K], per (query, head) the 2K location
// coordinates and then the K attention LOGITS -- and the softmax over the K taps inside the operator.  The sampling core
// (samp_core.hpp) under the policy FdaOp below: MsdaOp's pairs, level table, positions and list items, with the addressing
// of the packed row and a factor that is a function of the pair's logits.  A call is planned ONCE, like its siblings:
// fda_plan() decides whether the family takes it (msda_plan's rule plus the packed tensor's size) and lays its workspace
// out, the byte count reported to the caller is the plan's `total`, and fda_forward / fda_backward take the plan.
// Written from memory of the published operator ("FlashDeformAttn" of the DCNv4 package) and UNPINNED against its code.
#pragma once
#include "msda_plan.hpp"

namespace mdconv {

// Device-side geometry (POD, passed by value as a kernel argument): MSDA's, the row length, and where the per-pair softmax
// statistics go.
struct FdaGeom : MsdaGeom {
  int K3;          // 3 * K: the elements of a (query, head)
  float2 *stats;   // backward with grad_value: (max, 1 / sum) per pair, in the workspace; else nullptr
};

struct FdaTensors {
  const void *value, *loc_attn, *grad_output;
  void *output, *grad_value, *grad_loc_attn;
};

struct FdaPlan {
  FdaGeom g;                // (g.stats is set by fda_backward, from the workspace it is handed)
  int dtype, coord_dtype;   // MDCONV_F32 / MDCONV_F16 / MDCONV_BF16
  bool backward;
  bool det;                 // MDCONV_FLAG_DETERMINISTIC: the lists are sorted before the gather
  bool skip_value;          // MDCONV_FLAG_NO_GRAD_INPUT: no lists, no statistics, no sort, no gather, no workspace
  ScatterLists lists;       // grad_value: MSDA's lists of the same shape
  size_t off_stats;         // 8 bytes per pair behind the lists
  size_t total;             // workspace bytes
};

// false: outside the shape rule; *why names the rule it breaks.  The descriptor has passed validation (the operator's *_host.hip).
bool fda_plan(const mdconv_fda_desc *d, bool backward, FdaPlan *p, const char **why);
int fda_forward(const FdaPlan &p, const FdaTensors &t, hipStream_t stream);
int fda_backward(const FdaPlan &p, const FdaTensors &t, void *ws, hipStream_t stream);

#ifdef __HIPCC__
// What the taps of a pair have in common: MsdaOp's byte offset, and the statistics of the pair's softmax.
struct FdaPair {
  int byte;
  float mx, inv;   // the largest logit of the pair, and 1 / sum exp(logit - mx)
};

// THE weight of a tap: the forward, the coordinate backward and the list kernel all take it from here, from the same two
// statistics, so the three agree to the bit.
__device__ __forceinline__ float fda_weight(float logit, float mx, float inv) { return expf(logit - mx) * inv; }

// The operator policy of the sampling core: coord = factor = sampling_loc_attn, sampled tensor = value.  Pairs, context,
// level table, positions and list items are MsdaOp's; what differs is where a (pair, tap) lives in the row, and that the
// factor of a tap is the softmax weight of its logit.
struct FdaOp {
  typedef FdaGeom Geom;
  typedef FdaPair Ctx;
  static constexpr bool kPairSum = true;
  static __host__ __device__ __forceinline__ int npairs(const Geom &g) { return MsdaOp::npairs(g); }
  static __device__ __forceinline__ size_t sampled_bytes(const Geom &g) { return MsdaOp::sampled_bytes(g); }
  static __device__ __forceinline__ int list_rows(const Geom &g) { return MsdaOp::list_rows(g); }

  static __device__ __forceinline__ Ctx ctx(const Geom &g, int pair) {
    Ctx p;
    p.byte = MsdaOp::ctx(g, pair);
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
  // The statistics of the pair's softmax, by the pair's VL lanes together: lane j takes the logits j, j + VL, ... below K
  // -- a lane with none (K < VL) and the taps from K on enter neither the maximum nor the sum -- and two xor butterflies
  // leave every lane with the same bits.  fp32 and max-subtracted: the largest term of the sum is exactly 1.  Where the
  // lists will need them (g.stats) the pair's lane 0 stores the two.
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
    MsdaOp::tap_state<CT>(g, cx.byte, tap, om, coord_index(g, cx, pair, tap, 0), om, factor_index(g, cx, pair, tap), t, fx, fy);
    t.m = fda_weight(t.m, cx.mx, cx.inv);   // (tap_state left the logit there)
  }
  // d(sum_s a[s] g[s]) / d(logit t) = a[t] * (g[t] - sum_s a[s] g[s])
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
    MsdaOp::list_item_at<CT>(g, pair, tap, om, pair * g.K3 + 2 * tap, it);
  }
};
#endif  // __HIPCC__

}  // namespace mdconv
