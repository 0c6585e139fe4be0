// dcn4_plan.hpp -- the DCNv4 operator (include/mdconv.h "DCNv4 operator"): the DCNv3 core operator's sampling with ONE packed
// coordinate tensor -- offset_mask [B, Ho, Wo, OM], per group 2K offsets then K masks, the row padded to a multiple of 8
// elements -- optionally without the kernel's centre tap (remove_center), masks of any sign and size, and coordinates in the
// values' type or in fp32.  The sampling core (samp_core.hpp) under the policy Dcn4Op below: Dcn3Op's pairs, context,
// positions and lists, with the addressing of the packed row.  A call is planned ONCE, like its siblings: dcn4_plan() decides
// whether the family takes it and lays its workspace out, the byte count reported to the caller is the plan's `total`, and
// dcn4_forward / dcn4_backward take the plan.
//
// With MDCONV_FLAG_SOFTMAX the masks are LOGITS and the operator takes their softmax itself -- DCNv3's softmax over the K
// masks of a group, inside the kernel: the policy Dcn4SoftOp below, which is to Dcn4Op what FdaOp is to MsdaOp.  Semantics:
//  - the softmax runs over ALL K tensor taps of the (output pixel, group); with remove_center K = kh * kw - 1;
//  - taps the gate drops are included: they count in the normaliser and add nothing to the output, which is what a framework
//    softmax in front of the operator does.  Such a tap's logit gradient is -a[t] * S (S: the pair sum), not zero; its offset
//    gradients are exactly zero; when every tap of a pair is gated out, S = 0 and all gradients of the pair are exactly zero;
//  - with K = 1 the weight is exactly 1 and the logit gradient exactly 0;
//  - the padding columns of the row stay unread.
#pragma once
#include "dcn3_plan.hpp"
#include "fda_plan.hpp"   // fda_weight: THE weight of a tap from (logit, max, 1 / sum)

namespace mdconv {

// Device-side geometry (POD, passed by value as a kernel argument): DCNv3's, with K = kh * kw - remove_center, and the row.
struct Dcn4Geom : Dcn3Geom {
  int OM;       // elements per row of offset_mask: G * 3K rounded up to a multiple of 8
  int K3;       // 3 * K: the elements of a group
  int center;   // tensor taps from this one on sit one kernel-grid position further (remove_center); else K: none does
};

// ... and with the softmax, where the per-pair statistics go
struct Dcn4SoftGeom : Dcn4Geom {
  float2 *stats;   // backward with grad_input: (max, 1 / sum) per pair, in the workspace; else nullptr
};

struct Dcn4Tensors {
  const void *input, *offset_mask, *grad_output;
  void *output, *grad_input, *grad_offset_mask;
};

struct Dcn4Plan {
  Dcn4Geom g;
  int dtype, coord_dtype;   // MDCONV_F32 / MDCONV_F16 / MDCONV_BF16
  bool backward;
  bool det;                 // MDCONV_FLAG_DETERMINISTIC: the lists are sorted before the gather
  bool skip_input;          // MDCONV_FLAG_NO_GRAD_INPUT: no lists, no sort, no gather, no workspace
  bool softmax;             // MDCONV_FLAG_SOFTMAX: the masks are logits (Dcn4SoftOp)
  ScatterLists lists;       // grad_input: per (image, group) a segment of S_i lists, K * S_o * 4 entries
  size_t off_stats;         // softmax: 8 bytes per pair behind the lists
  size_t total;             // workspace bytes
};

// elements per row of offset_mask for G groups of K taps
inline int64_t dcn4_row_len(int64_t G, int64_t K) { return (G * K * 3 + 7) / 8 * 8; }

// false: outside the shape rule; *why names the rule it breaks.  The descriptor has passed validation (the operator's *_host.hip).
bool dcn4_plan(const mdconv_dcnv4_desc *d, bool backward, Dcn4Plan *p, const char **why);
int dcn4_forward(const Dcn4Plan &p, const Dcn4Tensors &t, hipStream_t stream);
int dcn4_backward(const Dcn4Plan &p, const Dcn4Tensors &t, void *ws, hipStream_t stream);

#ifdef __HIPCC__
struct Dcn4Pix : Dcn3Pix {
  int grp_elem;   // element of offset_mask where the pair's group starts: n * OM + group * 3K
  int last;       // the pair is the last group of its pixel: its lanes own the row's padding
};

// The operator policy of the sampling core: coord = factor = offset_mask, sampled tensor = input.  Pairs, context, positions
// and lists are Dcn3Op's; what differs is where a (pair, tap) lives in the row, and which kernel-grid position it has.
struct Dcn4Op : SampPlainFactor {
  typedef Dcn4Geom Geom;
  typedef Dcn4Pix Ctx;
  static __host__ __device__ __forceinline__ int npairs(const Geom &g) { return Dcn3Op::npairs(g); }
  static __device__ __forceinline__ size_t sampled_bytes(const Geom &g) { return Dcn3Op::sampled_bytes(g); }
  static __device__ __forceinline__ int list_rows(const Geom &g) { return Dcn3Op::list_rows(g); }

  static __device__ __forceinline__ int group_elem(const Geom &g, int pair) {
    const int n = pair / g.G, grp = pair - n * g.G;
    return n * g.OM + grp * g.K3;
  }
  static __device__ __forceinline__ Ctx ctx(const Geom &g, int pair) {
    Ctx p;
    (Dcn3Pix &)p = Dcn3Op::ctx(g, pair);
    p.grp_elem = group_elem(g, pair);
    p.last = pair % g.G == g.G - 1;
    return p;
  }
  // tensor tap -> kernel-grid position u = i * kh + j: the centre of the grid is skipped with remove_center
  static __device__ __forceinline__ int grid_tap(const Geom &g, int tap) { return tap + (tap >= g.center ? 1 : 0); }
  // the group's 3K elements: (x, y) of tap 0 .. K-1, then the K masks
  static __device__ __forceinline__ int coord_index(const Geom &, const Ctx &px, int, int tap, int xy) {
    return px.grp_elem + 2 * tap + xy;
  }
  static __device__ __forceinline__ int factor_index(const Geom &g, const Ctx &px, int, int tap) {
    return px.grp_elem + 2 * g.K + tap;
  }
  static __device__ __forceinline__ int list_factor_index(const Geom &g, int id) {
    const int pair = id / g.K, tap = id - pair * g.K;
    return group_elem(g, pair) + 2 * g.K + tap;
  }
  template <int CT>
  static __device__ __forceinline__ void build_tap(const Geom &g, const Ctx &px, int pair, int tap, bool on, const void *om,
                                                   const void *, SampTap &t, float &fx, float &fy) {
    samp_tap_clear(t);
    fx = fy = g.scale;
    if (!on) return;
    Dcn3Op::tap_state<CT>(g, px, grid_tap(g, tap), om, coord_index(g, px, pair, tap, 0), coord_index(g, px, pair, tap, 1), om,
                          factor_index(g, px, pair, tap), t);
  }
  // Overwrite mode owes the row's padding exact zeros (accumulate mode leaves it alone): the lanes of a pixel's last pair
  // store them, lane j the columns G * 3K + j, + VL, ... -- at most 7 elements per pixel, no pass over the tensor.
  template <int CT>
  static __device__ __forceinline__ void finish_pair(const Geom &g, const Ctx &px, const SampLane &ln, void *grad_om) {
    if (g.acc || !ln.live || !px.last) return;
    const int row_end = px.grp_elem - (g.G - 1) * g.K3 + g.OM;   // one past the row
    for (int e = px.grp_elem + g.K3 + ln.j; e < row_end; e += g.ln.VL) samp_st<CT>(grad_om, e, 0.f, false);
  }
  // sample id = pair * K + tap
  template <int CT> static __device__ __forceinline__ void list_item(const Geom &g, int id, const void *om, SampItem &it) {
    const int pair = id / g.K, tap = id - pair * g.K;
    const int ex = group_elem(g, pair) + 2 * tap;
    Dcn3Op::list_item_at<CT>(g, pair, tap, grid_tap(g, tap), om, ex, ex + 1, it);
  }
};

// What the taps of a pair have in common under the softmax: Dcn4Op's, and the statistics of the pair's K logits.
struct Dcn4SoftPix : Dcn4Pix {
  float mx, inv;   // the largest logit of the pair, and 1 / sum exp(logit - mx)
};

// The policy of MDCONV_FLAG_SOFTMAX: pairs, context, grid_tap, the three index functions, positions, the gate, the padding
// rule and the list items are Dcn4Op's, called; what differs is that the factor of a tap is the softmax weight of its logit
// (fda_weight, the one function the forward, the coordinate backward and the list kernel share).
struct Dcn4SoftOp {
  typedef Dcn4SoftGeom Geom;
  typedef Dcn4SoftPix Ctx;
  static constexpr bool kPairSum = true;
  static __host__ __device__ __forceinline__ int npairs(const Geom &g) { return Dcn4Op::npairs(g); }
  static __device__ __forceinline__ size_t sampled_bytes(const Geom &g) { return Dcn4Op::sampled_bytes(g); }
  static __device__ __forceinline__ int list_rows(const Geom &g) { return Dcn4Op::list_rows(g); }

  static __device__ __forceinline__ Ctx ctx(const Geom &g, int pair) {
    Ctx p;
    (Dcn4Pix &)p = Dcn4Op::ctx(g, pair);
    p.mx = 0.f;
    p.inv = 1.f;
    return p;
  }
  static __device__ __forceinline__ int coord_index(const Geom &g, const Ctx &px, int pair, int tap, int xy) {
    return Dcn4Op::coord_index(g, px, pair, tap, xy);
  }
  static __device__ __forceinline__ int factor_index(const Geom &g, const Ctx &px, int pair, int tap) {
    return Dcn4Op::factor_index(g, px, pair, tap);
  }
  static __device__ __forceinline__ int list_factor_index(const Geom &g, int id) { return Dcn4Op::list_factor_index(g, id); }
  // The statistics of the pair's softmax, by the pair's VL lanes together: lane j takes the logits j, j + VL, ... below K
  // -- a lane with none (K < VL) enters neither the maximum nor the sum, and the row's padding is never read -- and two xor
  // butterflies leave every lane with the same bits.  fp32 and max-subtracted: the largest term of the sum is exactly 1.
  // Where the lists will need them (g.stats) the pair's lane 0 stores the two.
  template <int CT>
  static __device__ __forceinline__ void begin_pair(const Geom &g, Ctx &cx, const SampLane &ln, const void *om) {
    const int e0 = cx.grp_elem + 2 * g.K;
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
    Dcn4Op::build_tap<CT>(g, cx, pair, tap, on, om, om, t, fx, fy);
    if (on) t.m = fda_weight(t.m, cx.mx, cx.inv);   // (Dcn4Op left the logit there; a gated-out tap keeps its weight)
  }
  // d(sum_s a[s] g[s]) / d(logit t) = a[t] * (g[t] - sum_s a[s] g[s])
  static __device__ __forceinline__ float factor_grad(float a, float gsum, float s_pair) { return a * (gsum - s_pair); }
  template <int CT>
  static __device__ __forceinline__ void finish_pair(const Geom &g, const Ctx &cx, const SampLane &ln, void *grad_om) {
    Dcn4Op::finish_pair<CT>(g, cx, ln, grad_om);
  }
  // thread = sample: the weight from the statistics the coordinate kernel stored, not from a reduction per thread
  static __device__ __forceinline__ float list_factor(const Geom &g, int id, float logit) {
    const float2 st = g.stats[id / g.K];
    return fda_weight(logit, st.x, st.y);
  }
  template <int CT> static __device__ __forceinline__ void list_item(const Geom &g, int id, const void *om, SampItem &it) {
    Dcn4Op::list_item<CT>(g, id, om, it);
  }
};
#endif  // __HIPCC__

}  // namespace mdconv
