// dcn3_plan.hpp -- the DCNv3 core operator (include/mdconv.h "DCNv3 core operator"): grouped deformable sampling on
// channels-last tensors, fp32 / fp16 / bf16, with a constant group weight -- no contraction at all, so the family is VALU
// kernels: the sampling core (samp_core.hpp) under the policy Dcn3Op below, pair = (output pixel, group).  Like the depthwise
// family (dw_plan.hpp) a call is planned ONCE: dcn3_plan() decides whether the family takes it and lays its workspace out, the
// byte count reported to the caller is the plan's `total`, and dcn3_forward / dcn3_backward take the plan.
#pragma once
#include "samp_core.hpp"

namespace mdconv {

// Device-side geometry (POD, passed by value as a kernel argument).
struct Dcn3Geom {
  int B, G, D, C, K;    // C = G * D, K = kh * kw
  int H, W, Ho, Wo, kh, kw;
  int sh, sw, ph, pw, dh, dw;
  int ch, cw;           // (dil * (k - 1)) >> 1 per axis
  int S_i, S_o, N;      // H * W, Ho * Wo, B * S_o
  SampLanes ln;
  float scale;          // offset_scale
  int acc;              // backward: 1 = add to the caller's gradient buffers, 0 = overwrite
};

struct Dcn3Tensors {
  const void *input, *offset, *mask, *grad_output;
  void *output, *grad_input, *grad_offset, *grad_mask;
};

struct Dcn3Plan {
  Dcn3Geom g;
  int dtype;            // MDCONV_F32 / MDCONV_F16 / MDCONV_BF16
  bool backward;
  bool det;             // MDCONV_FLAG_DETERMINISTIC: the lists are sorted before the gather
  bool skip_input;      // MDCONV_FLAG_NO_GRAD_INPUT: no lists, no sort, no gather, no workspace
  ScatterLists lists;   // grad_input: per (image, group) a segment of S_i lists, K * S_o * 4 entries
  size_t total;         // workspace bytes
};

// false: outside the shape rule; *why names the rule it breaks.  The descriptor has passed validation (the operator's *_host.hip).
bool dcn3_plan(const mdconv_dcnv3_desc *d, bool backward, Dcn3Plan *p, const char **why);
int dcn3_forward(const Dcn3Plan &p, const Dcn3Tensors &t, hipStream_t stream);
int dcn3_backward(const Dcn3Plan &p, const Dcn3Tensors &t, void *ws, hipStream_t stream);

#ifdef __HIPCC__
struct Dcn3Pix {   // what the taps of one (output pixel, group) have in common
  int img_pix;     // b * S_i
  int grp_byte;    // group * D * esz
  float base_h, base_w;
};

// The operator policy of the sampling core: coord = offset (x, y per tap), factor = mask, sampled tensor = input.
struct Dcn3Op : SampPlainFactor {
  typedef Dcn3Geom Geom;
  typedef Dcn3Pix Ctx;
  static __host__ __device__ __forceinline__ int npairs(const Geom &g) { return g.N * g.G; }
  static __device__ __forceinline__ size_t sampled_bytes(const Geom &g) { return (size_t)g.B * g.S_i * g.C * g.ln.esz; }
  static __device__ __forceinline__ int list_rows(const Geom &g) { return g.S_i; }

  static __device__ __forceinline__ Ctx ctx(const Geom &g, int pair) {
    const int n = pair / g.G, grp = pair - n * g.G;
    const int b = n / g.S_o, pix = n - b * g.S_o;
    const int ho = pix / g.Wo, wo = pix - ho * g.Wo;
    Ctx p;
    p.img_pix = b * g.S_i;
    p.grp_byte = grp * g.D * g.ln.esz;
    p.base_h = (float)(ho * g.sh - g.ph + g.ch);
    p.base_w = (float)(wo * g.sw - g.pw + g.cw);
    return p;
  }
  // the position of tap = i * kh + j (i: the kernel's width index) from the offsets (x, y) of the tap
  static __device__ __forceinline__ void position(const Geom &g, const Ctx &px, int tap, float off_x, float off_y, SampSample &s) {
    const int i = tap / g.kh, j = tap - i * g.kh;
    const float loc_w = px.base_w + ((float)(i * g.dw - g.cw) + off_x) * g.scale;
    const float loc_h = px.base_h + ((float)(j * g.dh - g.ch) + off_y) * g.scale;
    samp_sample(loc_h, loc_w, g.H, g.W, s);
  }
  // offset [.., G, K, 2] and mask [.., G, K]: element pair * K + tap of the mask, twice that of the offset
  static __device__ __forceinline__ int coord_index(const Geom &g, const Ctx &, int pair, int tap, int xy) {
    return 2 * (pair * g.K + tap) + xy;
  }
  static __device__ __forceinline__ int factor_index(const Geom &g, const Ctx &, int pair, int tap) { return pair * g.K + tap; }
  static __device__ __forceinline__ int list_factor_index(const Geom &, int id) { return id; }
  template <int CT>
  static __device__ __forceinline__ void build_tap(const Geom &g, const Ctx &px, int pair, int tap, bool on, const void *offset,
                                                   const void *mask, SampTap &t, float &fx, float &fy) {
    samp_tap_clear(t);
    fx = fy = g.scale;
    // (the indices are taken behind the `on` test: taken at the call they would stay live up to the kernel's stores)
    if (!on) return;
    tap_state<CT>(g, px, tap, offset, coord_index(g, px, pair, tap, 0), coord_index(g, px, pair, tap, 1), mask,
                  factor_index(g, px, pair, tap), t);
  }
  // the state of the tap at kernel-grid position `grid_tap` from the elements ex, ey (offset) and ef (mask)
  template <int CT>
  static __device__ __forceinline__ void tap_state(const Geom &g, const Ctx &px, int grid_tap, const void *offset, int ex, int ey,
                                                   const void *mask, int ef, SampTap &t) {
    SampSample s;
    position(g, px, grid_tap, samp_ld<CT>(offset, ex), samp_ld<CT>(offset, ey), s);
    t.lx = s.lx;
    t.ly = s.ly;
    t.m = samp_ld<CT>(mask, ef);
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
      if (samp_corner_read(s, ci, g.H, g.W))
        t.off[ci] = (px.img_pix + samp_corner_pixel(s, ci, g.W)) * g.C * g.ln.esz + px.grp_byte;
  }
  template <int CT> static __device__ __forceinline__ void finish_pair(const Geom &, const Ctx &, const SampLane &, void *) {}
  // the item of tap `tap` of `pair`, at kernel-grid position `grid_tap`, from the elements ex, ey; lists per (image, group, input pixel)
  template <int CT>
  static __device__ __forceinline__ void list_item_at(const Geom &g, int pair, int tap, int grid_tap, const void *offset, int ex,
                                                      int ey, SampItem &it) {
    const int n = pair / g.G, grp = pair - n * g.G;
    const int b = n / g.S_o, pix = n - b * g.S_o;
    position(g, ctx(g, pair), grid_tap, samp_ld<CT>(offset, ex), samp_ld<CT>(offset, ey), it.s);
    it.H = g.H; it.W = g.W;
    it.seg = b * g.G + grp; it.row0 = 0;
    it.tap = tap; it.q = pix; it.rows_out = g.S_o;
  }
  // sample id = pair * K + tap
  template <int CT> static __device__ __forceinline__ void list_item(const Geom &g, int id, const void *offset, SampItem &it) {
    const int pair = id / g.K, tap = id - pair * g.K;
    list_item_at<CT>(g, pair, tap, tap, offset, 2 * id, 2 * id + 1, it);
  }
};
#endif  // __HIPCC__

}  // namespace mdconv
