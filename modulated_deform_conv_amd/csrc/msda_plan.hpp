// msda_plan.hpp -- multi-scale deformable attention (include/mdconv.h "Multi-scale deformable attention"): the sampling
// operator of Deformable-DETR-style attention on channels-last tensors, fp32 / fp16 / bf16 values with coordinates in the
// same type or in fp32.  The sampling core (samp_core.hpp) under the policy MsdaOp below: pair = (n * Lq + q) * M + m, the
// sampled tensor is a concatenation of levels of different extents, the positions arrive normalised, and tap = l * P + p, so
// pair * K + tap is the element index of attention_weights.  A call is planned ONCE: msda_plan() decides whether the family
// takes it and lays its workspace out, the byte count reported to the caller is the plan's `total`, and msda_forward /
// msda_backward take the plan.
#pragma once
#include "samp_core.hpp"

namespace mdconv {

// Device-side geometry (POD, passed by value as a kernel argument).  The level table is read with constant indices only
// (MsdaOp::level: an unrolled select chain), so it stays in scalar registers: a per-lane dynamic index would go through scratch.
struct MsdaGeom {
  int N, M, D, C, Lq, L, P, K;   // C = M * D, K = L * P
  int S;                         // value rows per image
  int npairs;                    // N * Lq * M
  SampLanes ln;
  int acc;                       // backward: 1 = add to the caller's gradient buffers, 0 = overwrite
  int lvH[MDCONV_MSDA_MAX_LEVELS], lvW[MDCONV_MSDA_MAX_LEVELS], lvS[MDCONV_MSDA_MAX_LEVELS];   // extents and start row
};

struct MsdaTensors {
  const void *value, *loc, *attn, *grad_output;
  void *output, *grad_value, *grad_loc, *grad_attn;
};

struct MsdaPlan {
  MsdaGeom g;
  int dtype, coord_dtype;   // MDCONV_F32 / MDCONV_F16 / MDCONV_BF16
  bool backward;
  bool det;                 // MDCONV_FLAG_DETERMINISTIC: the lists are sorted before the gather
  bool skip_value;          // MDCONV_FLAG_NO_GRAD_INPUT: no lists, no sort, no gather, no workspace
  ScatterLists lists;       // grad_value: per (image, head) a segment of S lists, K * Lq * 4 entries
  size_t total;             // workspace bytes
};

// false: outside the shape rule; *why names the rule it breaks.  The descriptor has passed validation (the operator's *_host.hip).
bool msda_plan(const mdconv_msda_desc *d, bool backward, MsdaPlan *p, const char **why);
int msda_forward(const MsdaPlan &p, const MsdaTensors &t, hipStream_t stream);
int msda_backward(const MsdaPlan &p, const MsdaTensors &t, void *ws, hipStream_t stream);


#ifdef __HIPCC__
// The operator policy of the sampling core: coord = sampling_locations, factor = attention_weights, sampled tensor = value.
// What the taps of a pair have in common (Ctx): the byte offset of (image n, value row 0, head m) in `value`.
struct MsdaOp : SampPlainFactor {
  typedef MsdaGeom Geom;
  typedef int Ctx;
  static __host__ __device__ __forceinline__ int npairs(const Geom &g) { return g.npairs; }
  static __device__ __forceinline__ size_t sampled_bytes(const Geom &g) { return (size_t)g.N * g.S * g.C * g.ln.esz; }
  static __device__ __forceinline__ int list_rows(const Geom &g) { return g.S; }

  static __device__ __forceinline__ Ctx ctx(const Geom &g, int pair) {
    const int nq = pair / g.M, m = pair - nq * g.M;
    const int n = nq / g.Lq;
    return (n * g.S * g.C + m * g.D) * g.ln.esz;
  }
  // extents and start row of level `l` (0 <= l < L <= 8): constant indices into the kernel argument
  static __device__ __forceinline__ void level(const Geom &g, int l, int &H, int &W, int &start) {
    H = g.lvH[0]; W = g.lvW[0]; start = g.lvS[0];
#pragma unroll
    for (int i = 1; i < MDCONV_MSDA_MAX_LEVELS; ++i)
      if (l == i) { H = g.lvH[i]; W = g.lvW[i]; start = g.lvS[i]; }
  }
  // the sample whose x is element ec of sampling_locations (y follows), in the pixel coordinates of its level
  template <int CT> static __device__ __forceinline__ void position(const void *loc, int ec, int H, int W, SampSample &s) {
    const float x = samp_ld<CT>(loc, ec) * (float)W - 0.5f;
    const float y = samp_ld<CT>(loc, ec + 1) * (float)H - 0.5f;
    samp_sample(y, x, H, W, s);
  }
  // sampling_locations [.., M, L, P, 2] and attention_weights [.., M, L, P]: element e = pair * K + tap of the weights,
  // twice that of the locations
  static __device__ __forceinline__ int coord_index(const Geom &g, const Ctx &, int pair, int tap, int xy) {
    return 2 * (pair * g.K + tap) + xy;
  }
  static __device__ __forceinline__ int factor_index(const Geom &g, const Ctx &, int pair, int tap) { return pair * g.K + tap; }
  static __device__ __forceinline__ int list_factor_index(const Geom &, int id) { return id; }
  template <int CT> static __device__ __forceinline__ void finish_pair(const Geom &, const Ctx &, const SampLane &, void *) {}
  // fx, fy: the extents of the tap's level, W for x and H for y (the positions are normalised)
  template <int CT>
  static __device__ __forceinline__ void build_tap(const Geom &g, const Ctx &pair_byte, int pair, int tap, bool on, const void *loc,
                                                   const void *attn, SampTap &t, float &fx, float &fy) {
    samp_tap_clear(t);
    fx = fy = 1.f;
    if (!on) return;
    tap_state<CT>(g, pair_byte, tap, loc, coord_index(g, pair_byte, pair, tap, 0), attn, factor_index(g, pair_byte, pair, tap), t,
                  fx, fy);
  }
  // the state of tap `tap` (which names its level) from the elements ec (its x; y follows) and ef (its factor)
  template <int CT>
  static __device__ __forceinline__ void tap_state(const Geom &g, const Ctx &pair_byte, int tap, const void *loc, int ec,
                                                   const void *attn, int ef, SampTap &t, float &fx, float &fy) {
    int H, W, start;
    level(g, tap / g.P, H, W, start);
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
  // the item of tap `tap` of `pair` from the element ec that holds its x; lists per (image, head, value row over all S rows of
  // the concatenated levels).  (The segment and the key words are stated before the level select: after it the fill instance
  // takes 28 VGPRs instead of 26.)
  template <int CT>
  static __device__ __forceinline__ void list_item_at(const Geom &g, int pair, int tap, const void *loc, int ec, SampItem &it) {
    const int nq = pair / g.M, m = pair - nq * g.M;
    const int n = nq / g.Lq, q = nq - n * g.Lq;
    it.seg = n * g.M + m;
    it.tap = tap; it.q = q; it.rows_out = g.Lq;
    level(g, tap / g.P, it.H, it.W, it.row0);
    position<CT>(loc, ec, it.H, it.W, it.s);
  }
  // sample id = pair * K + tap
  template <int CT> static __device__ __forceinline__ void list_item(const Geom &g, int id, const void *loc, SampItem &it) {
    const int pair = id / g.K, tap = id - pair * g.K;
    list_item_at<CT>(g, pair, tap, loc, 2 * id, it);
  }
};
#endif  // __HIPCC__

}  // namespace mdconv
