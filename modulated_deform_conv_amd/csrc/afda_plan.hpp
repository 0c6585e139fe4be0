// afda_plan.hpp -- anchored packed deformable attention (include/mdconv_afda.h): the operator of fdap_plan.hpp that takes the
// packed row of RAW offsets and logits plus the reference points or boxes, and does the reference arithmetic of the decoder
// blocks in the kernels.  The sampling core (samp_core.hpp) under the policy AfdaOp below, which sits on FdapOp as FdapOp sits
// on MsdapOp: FdapOp's pairs, row addressing, softmax, weight and list factor; what differs is how a tap's position comes
// about -- ONE function, afda_location, for the forward, the coordinate backward and the list kernel, so their gates agree --
// and one more result, grad_reference_points, which the coordinate backward sums through the core's tap_grads hook.  Lr, R
// and offset_scale are run-time data of the geometry (wave-uniform branches): the instances are FdapOp's in number.
#pragma once
#include "../../include/mdconv_afda.h"
#include "fdap_plan.hpp"

namespace mdconv {

// Device-side geometry (POD, passed by value as a kernel argument): FDAP's, the reference tensor and its form, and the
// per-level tables the location needs -- all read with constant indices only, like pfx[] and the level table.
struct AfdaGeom : FdapGeom {
  const float *ref;   // reference_points [N * Lq, Lr, R]
  float *gpart;       // backward with grad_reference: one partial row [Lr * R] per pair, in the workspace; else nullptr
  int Lr, R;
  float oscale;       // offset_scale (R == 4)
  float inv_points[MDCONV_MSDA_MAX_LEVELS];                           // s_k of a tap of level l: 1 / points[l]
  float invW[MDCONV_MSDA_MAX_LEVELS], invH[MDCONV_MSDA_MAX_LEVELS];   // R == 2: 1 / W_l, 1 / H_l
};

struct AfdaTensors {
  const void *value, *ref, *offs_attn, *grad_output;
  void *output, *grad_value, *grad_ref, *grad_offs_attn;
};

struct AfdaPlan {
  AfdaGeom g;               // (g.ref, g.stats and g.gpart are set by the run, from its arguments and workspace)
  int dtype, coord_dtype;   // MDCONV_F32 / MDCONV_F16 / MDCONV_BF16
  bool backward;
  bool det;                 // MDCONV_FLAG_DETERMINISTIC: the lists are sorted before the gather
  bool skip_value;          // MDCONV_FLAG_NO_GRAD_INPUT: no lists, no statistics, no sort, no gather
  bool grad_ref;            // the backward computes grad_reference_points
  ScatterLists lists;       // grad_value: FDAP's lists of the same shape
  size_t off_stats;         // FDAP's statistics
  size_t off_gpart;         // grad_ref: 4 * Lr * R bytes per pair behind FDAP's workspace
  size_t total;             // workspace bytes
};

// false: outside the shape rule; *why names the rule it breaks.  The descriptor has passed validation (afda_host.hip).
bool afda_plan(const mdconv_afda_desc *d, bool backward, AfdaPlan *p, const char **why);
int afda_forward(const AfdaPlan &p, const AfdaTensors &t, hipStream_t stream);
int afda_backward(const AfdaPlan &p, const AfdaTensors &t, void *ws, hipStream_t stream);

#ifdef __HIPCC__
// What the taps of a pair have in common: FdaPair, the pair's reference row where there is one for all levels (Lr == 1),
// and the running sums of the reference row the coordinate backward is in.
struct AfdaPair : FdaPair {
  float ref[4];
  float racc[4];
};

// What a tap's level contributes to its position: extents, start row, and the scales of its offsets.
struct AfdaLevel {
  int l, H, W, start;
  float sk;        // 1 / points[l]
  float iW, iH;    // 1 / W, 1 / H (R == 2)
};

// THE position function: the normalised location of a tap from its reference row, its offset pair and its level, in fp32,
// and the factors sx, sy its offsets were scaled by.  fmaf, so that every kernel forms the same bits.
__device__ __forceinline__ void afda_location(const AfdaGeom &g, const AfdaLevel &lv, const float (&ref)[4], float dx, float dy,
                                              float &loc_x, float &loc_y, float &sx, float &sy) {
  if (g.R == 4) {
    sx = lv.sk * ref[2] * g.oscale;
    sy = lv.sk * ref[3] * g.oscale;
  } else {
    sx = lv.iW;
    sy = lv.iH;
  }
  loc_x = fmaf(dx, sx, ref[0]);
  loc_y = fmaf(dy, sy, ref[1]);
}

struct AfdaOp : FdapOp {
  typedef AfdaGeom Geom;
  typedef AfdaPair Ctx;
  static constexpr bool kTapGrads = true;   // the core calls tap_grads after every tap batch of the coordinate backward

  // MsdapOp::level_of_tap that also names the level, and the select chains of the level's scales
  static __device__ __forceinline__ void level_of_tap(const Geom &g, int tap, AfdaLevel &lv) {
    int l = 0;
#pragma unroll
    for (int i = 1; i < MDCONV_MSDA_MAX_LEVELS; ++i) l += tap >= g.pfx[i];
    lv.l = l;
    MsdaOp::level(g, l, lv.H, lv.W, lv.start);
    lv.sk = g.inv_points[0];
    lv.iW = g.invW[0];
    lv.iH = g.invH[0];
    if (g.R == 4) {
#pragma unroll
      for (int i = 1; i < MDCONV_MSDA_MAX_LEVELS; ++i)
        if (l == i) lv.sk = g.inv_points[i];
    } else {
#pragma unroll
      for (int i = 1; i < MDCONV_MSDA_MAX_LEVELS; ++i)
        if (l == i) { lv.iW = g.invW[i]; lv.iH = g.invH[i]; }
    }
  }
  // reference row `r` of the pair's query: 2 or 4 floats (an "element" tensor: scalar loads)
  static __device__ __forceinline__ void load_ref(const Geom &g, int pair, int r, float (&ref)[4]) {
    const float *p = g.ref + ((pair / g.M) * g.Lr + r) * g.R;
    ref[0] = p[0];
    ref[1] = p[1];
    ref[2] = ref[3] = 0.f;
    if (g.R == 4) { ref[2] = p[2]; ref[3] = p[3]; }
  }
  // the sample of (pair, tap) whose dx is element ec of offs_attn (dy follows): afda_location, then MsdaOp::position's
  // arithmetic on the location
  template <int CT>
  static __device__ __forceinline__ void sample_of(const Geom &g, const AfdaLevel &lv, const float (&ref)[4], const void *om, int ec,
                                                   SampSample &s, float &sx, float &sy) {
    float loc_x, loc_y;
    afda_location(g, lv, ref, samp_ld<CT>(om, ec), samp_ld<CT>(om, ec + 1), loc_x, loc_y, sx, sy);
    const float x = loc_x * (float)lv.W - 0.5f;
    const float y = loc_y * (float)lv.H - 0.5f;
    samp_sample(y, x, lv.H, lv.W, s);
  }

  static __device__ __forceinline__ Ctx ctx(const Geom &g, int pair) {
    Ctx p;
    p.byte = MsdapOp::ctx(g, pair);
    p.mx = 0.f;
    p.inv = 1.f;
    load_ref(g, pair, 0, p.ref);   // (Lr == L: row 0, which the taps of level 0 replace by their own load of it)
#pragma unroll
    for (int c = 0; c < 4; ++c) p.racc[c] = 0.f;
    return p;
  }
  // FdapOp::build_tap with the position from the reference.  fx, fy: what the stored offset gradient carries beyond the
  // pixel-space gradient -- the extent times the offset's scale -- and 0, selected, for a tap that is gated out: its sums are
  // exact zeros, but its scale may be NaN (a non-finite reference row).
  template <int CT>
  static __device__ __forceinline__ void build_tap(const Geom &g, const Ctx &cx, int pair, int tap, bool on, const void *om,
                                                   const void *, SampTap &t, float &fx, float &fy) {
    samp_tap_clear(t);
    fx = fy = 1.f;
    if (!on) return;
    AfdaLevel lv;
    level_of_tap(g, tap, lv);
    float ref[4] = {cx.ref[0], cx.ref[1], cx.ref[2], cx.ref[3]};
    if (g.Lr != 1) load_ref(g, pair, lv.l, ref);
    SampSample s;
    float sx, sy;
    sample_of<CT>(g, lv, ref, om, coord_index(g, cx, pair, tap, 0), s, sx, sy);
    fx = s.inside ? (float)lv.W * sx : 0.f;
    fy = s.inside ? (float)lv.H * sy : 0.f;
    t.lx = s.lx;
    t.ly = s.ly;
    t.m = fda_weight(samp_ld<CT>(om, factor_index(g, cx, pair, tap)), cx.mx, cx.inv);
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
      if (samp_corner_read(s, ci, lv.H, lv.W)) t.off[ci] = cx.byte + (lv.start + samp_corner_pixel(s, ci, lv.W)) * g.C * g.ln.esz;
  }
  // sample id = pair * K + tap
  template <int CT> static __device__ __forceinline__ void list_item(const Geom &g, int id, const void *om, SampItem &it) {
    const int pair = id / g.K, tap = id - pair * g.K;
    const int nq = pair / g.M, m = pair - nq * g.M;
    const int n = nq / g.Lq, q = nq - n * g.Lq;
    it.seg = n * g.M + m;
    it.tap = tap; it.q = q; it.rows_out = g.Lq;
    AfdaLevel lv;
    level_of_tap(g, tap, lv);
    it.H = lv.H; it.W = lv.W; it.row0 = lv.start;
    float ref[4], sx, sy;
    load_ref(g, pair, g.Lr != 1 ? lv.l : 0, ref);
    sample_of<CT>(g, lv, ref, om, pair * g.K3 + 2 * tap, it.s, sx, sy);
  }

  // grad_reference_points, stage 1 (the core's hook, after the tap batch [t0, t0 + VL) of the coordinate backward): lane j
  // holds the pixel-space location gradients gx, gy of its tap my_tap.  What the tap owes its reference row --
  // (gx * W, gy * H) to (rx, ry) and, for boxes, those times the scaled offsets to (rw, rh) -- is summed over the pair's lanes
  // by the xor butterfly, per reference row under an unrolled constant loop (a row's taps are consecutive),
  // added to the row's running sums in batch order, and stored by the pair's lane 0 once the row's last tap is behind: one
  // partial row per pair in the workspace, every element written exactly once, in a fixed order.  A gated-out tap has
  // gx = gy = 0 exactly (nothing was loaded for it), and its offsets or box may be NaN: its products are SELECTED to zero.
  template <int CT>
  static __device__ __forceinline__ void tap_grads(const Geom &g, Ctx &cx, const SampLane &ln, int t0, int my_tap, bool my_on,
                                                   float gx, float gy, const void *om) {
    if (!g.gpart) return;
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    if (my_on) {
      AfdaLevel lv;
      level_of_tap(g, my_tap, lv);
      c[0] = gx * (float)lv.W;
      c[1] = gy * (float)lv.H;
      if (g.R == 4) {
        const int ec = coord_index(g, cx, ln.pair, my_tap, 0);
        const float kx = samp_ld<CT>(om, ec) * (lv.sk * g.oscale), ky = samp_ld<CT>(om, ec + 1) * (lv.sk * g.oscale);
        c[2] = gx != 0.f ? c[0] * kx : 0.f;
        c[3] = gy != 0.f ? c[1] * ky : 0.f;
      }
    }
    const int t1 = t0 + g.ln.VL;
#pragma unroll
    for (int i = 0; i < MDCONV_MSDA_MAX_LEVELS; ++i) {
      // the taps [lo, hi) read reference row i: level i's for Lr == L, all K in row 0 for Lr == 1; lo == hi: no such row
      const int lo = g.Lr != 1 ? g.pfx[i] : (i == 0 ? 0 : g.K);
      const int hi = g.Lr != 1 ? (i + 1 < MDCONV_MSDA_MAX_LEVELS ? g.pfx[i + 1] : g.K) : g.K;
      if (lo >= hi || lo >= t1 || hi <= t0) continue;   // (wave-uniform) no row i, or no tap of this batch reads it
      const bool mine = my_on && my_tap >= lo && my_tap < hi;
      float s[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] = mine ? c[k] : 0.f;
      for (int d = g.ln.VL >> 1; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += __shfl_xor(s[k], d, 64);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) cx.racc[k] = lo >= t0 ? s[k] : cx.racc[k] + s[k];   // the row begins in this batch, or goes on
      if (hi <= t1 && ln.live && ln.j == 0) {   // the row ends in this batch
        float *dst = g.gpart + (ln.pair * g.Lr + i) * g.R;
        dst[0] = cx.racc[0];
        dst[1] = cx.racc[1];
        if (g.R == 4) { dst[2] = cx.racc[2]; dst[3] = cx.racc[3]; }
      }
    }
  }
};

// grad_reference_points, stage 2: thread = one element of [N * Lq, Lr * R]; the partial rows of the M heads of the query in
// head order, stored in the write mode.
__global__ __launch_bounds__(256) void afda_ref_reduce_kernel(const float *__restrict__ gpart, float *__restrict__ grad_ref,
                                                               int total, int row, int M, int acc) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int nq = e / row, c = e - nq * row;
  float s = 0.f;
  for (int m = 0; m < M; ++m) s += gpart[(nq * M + m) * row + c];
  grad_ref[e] = acc ? grad_ref[e] + s : s;
}
#endif  // __HIPCC__

}  // namespace mdconv
