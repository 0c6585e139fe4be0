// dcn4_plan.hpp -- the DCNv4 operator (include/mdconv.h "DCNv4 operator"): the DCNv3 core operator's sampling with ONE packed
// coordinate tensor -- offset_mask [B, Ho, Wo, OM], per group 2K offsets then K masks, the row padded to a multiple of 8
// elements -- optionally without the kernel's centre tap (remove_center), masks of any sign and size, and coordinates in the
// values' type or in fp32.  The sampling core (samp_core.hpp) under the policy Dcn4Op below: Dcn3Op's pairs, context,
// positions and lists, with the addressing of the packed row.  A call is planned ONCE, like its siblings: dcn4_plan() decides
// whether the family takes it and lays its workspace out, the byte count reported to the caller is the plan's `total`, and
// dcn4_forward / dcn4_backward take the plan.
#pragma once
#include "dcn3_plan.hpp"

namespace mdconv {

// Device-side geometry (POD, passed by value as a kernel argument): DCNv3's, with K = kh * kw - remove_center, and the row.
struct Dcn4Geom : Dcn3Geom {
  int OM;       // elements per row of offset_mask: G * 3K rounded up to a multiple of 8
  int K3;       // 3 * K: the elements of a group
  int center;   // tensor taps from this one on sit one kernel-grid position further (remove_center); else K: none does
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
  ScatterLists lists;       // grad_input: per (image, group) a segment of S_i lists, K * S_o * 4 entries
  size_t total;             // workspace bytes
};

// elements per row of offset_mask for G groups of K taps
inline int64_t dcn4_row_len(int64_t G, int64_t K) { return (G * K * 3 + 7) / 8 * 8; }

// false: outside the shape rule; *why names the rule it breaks.  The descriptor has passed validation (mdconv_api.hip).
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
#endif  // __HIPCC__

}  // namespace mdconv
