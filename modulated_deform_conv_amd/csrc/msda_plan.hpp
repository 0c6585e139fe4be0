// msda_plan.hpp -- multi-scale deformable attention (include/mdconv.h "Multi-scale deformable attention"): the sampling
// operator of Deformable-DETR-style attention on channels-last tensors, fp32 / fp16 / bf16 values with coordinates in the
// same type or in fp32.  A sibling of the DCNv3 core operator (dcn3_plan.hpp), whose structure, lane mapping and device
// helpers it shares: a call is planned ONCE, msda_plan() decides whether the family takes it and lays its workspace out,
// the byte count reported to the caller is the plan's `total`, and msda_forward / msda_backward take the plan.  What
// differs from DCNv3: the sampled tensor is a concatenation of levels of different extents, the outputs are queries, and
// the positions arrive normalised.
//
// Lane mapping of every kernel: a lane owns one 16-byte channel vector (4 floats / 8 halves) of one (query, head) PAIR,
// pair = (n * Lq + q) * M + m; the VL lanes of a pair are adjacent and the pairs of a query follow each other, so a wave's
// stores and each of its corner loads are contiguous 16-byte pieces.  Taps: tap = l * P + p, so pair * K + tap is the
// element index of attention_weights.  Heads of more than 64 vectors take `rounds` > 1 passes over the vectors.
#pragma once
#include "dcn3_plan.hpp"   // the 16-byte vector helpers, the lane mapping and the tap state

namespace mdconv {

// Device-side geometry (POD, passed by value as a kernel argument).  The level table is read with constant indices only
// (msda_level: an unrolled select chain), so it stays in scalar registers: a per-lane dynamic index would go through scratch.
struct MsdaGeom {
  int N, M, D, C, Lq, L, P, K;   // C = M * D, K = L * P
  int S;                         // value rows per image
  int npairs;                    // N * Lq * M
  int V, VL, lgVL, rounds;
  int esz;                       // bytes per value element
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
  // grad_value (msda_gi.hip): scatter lists per (image, head, value row), one entry per corner the forward read
  int nseg;                 // N * M
  int64_t seg_stride;       // entries per segment: K * Lq * 4
  size_t off_cnt, off_rowptr, off_entries, off_sort;
  size_t total;             // workspace bytes
};

// false: outside the shape rule; *why names the rule it breaks.  The descriptor has passed validation (mdconv_api.hip).
bool msda_plan(const mdconv_msda_desc *d, bool backward, MsdaPlan *p, const char **why);
int msda_forward(const MsdaPlan &p, const MsdaTensors &t, hipStream_t stream);
int msda_backward(const MsdaPlan &p, const MsdaTensors &t, void *ws, hipStream_t stream);

// ---- kernels' launchers (one translation unit each) ----
int msda_fwd_launch(const MsdaPlan &p, const MsdaTensors &t, hipStream_t stream);
int msda_bwd_coord_launch(const MsdaPlan &p, const MsdaTensors &t, hipStream_t stream);
int msda_lists_launch(const MsdaPlan &p, const MsdaTensors &t, int *cnt, int *rowptr, void *entries, void *sort_scratch,
                      hipStream_t stream);
int msda_gather_launch(const MsdaPlan &p, const MsdaTensors &t, const int *rowptr, const void *entries, hipStream_t stream);

// workgroups of 256 lanes that cover `npairs` pairs
inline int msda_grid(const MsdaGeom &g, int64_t npairs) {
  const int64_t per_block = 4 * (64 >> g.lgVL);
  return (int)((npairs + per_block - 1) / per_block);
}

// the five (value type, coordinate type) pairings: `call(DT, CT)` for the plan's
#define MSDA_DISPATCH(p, call)                                                       \
  do {                                                                               \
    if ((p).dtype == MDCONV_F32) call(MDCONV_F32, MDCONV_F32);                       \
    else if ((p).dtype == MDCONV_F16 && (p).coord_dtype == MDCONV_F16) call(MDCONV_F16, MDCONV_F16); \
    else if ((p).dtype == MDCONV_F16) call(MDCONV_F16, MDCONV_F32);                  \
    else if ((p).coord_dtype == MDCONV_BF16) call(MDCONV_BF16, MDCONV_BF16);         \
    else call(MDCONV_BF16, MDCONV_F32);                                              \
  } while (0)

// ---- device side, shared by the three kernel files ----------------------------------------------
#ifdef __HIPCC__
// extents and start row of level `l` (0 <= l < L <= 8): constant indices into the kernel argument
__device__ __forceinline__ void msda_level(const MsdaGeom &g, int l, int &H, int &W, int &start) {
  H = g.lvH[0]; W = g.lvW[0]; start = g.lvS[0];
#pragma unroll
  for (int i = 1; i < MDCONV_MSDA_MAX_LEVELS; ++i)
    if (l == i) { H = g.lvH[i]; W = g.lvW[i]; start = g.lvS[i]; }
}

// the sample of element e = pair * K + tap of the coordinate tensors, in the pixel coordinates of its level
template <int CT>
__device__ __forceinline__ void msda_position(const void *loc, int e, int H, int W, Dcn3Sample &s) {
  const float x = dcn3_ld<CT>(loc, 2 * e) * (float)W - 0.5f;
  const float y = dcn3_ld<CT>(loc, 2 * e + 1) * (float)H - 0.5f;
  dcn3_sample(y, x, H, W, s);
}

// What the taps of a pair have in common: the byte offset of (image n, value row 0, head m) in `value`.
__device__ __forceinline__ int msda_pair_byte(const MsdaGeom &g, int pair) {
  const int nq = pair / g.M, m = pair - nq * g.M;
  const int n = nq / g.Lq;
  return (n * g.S * g.C + m * g.D) * g.esz;
}

// Sampling state of one (query, head, tap) as the lanes of the pair share it (Dcn3Tap: fractional parts, the attention
// weight in `m`, per corner the byte offset of the head's channel row in `value`, kDcn3Oob for a corner that is not read).
// H and W of the tap's level come back for the coordinate gradients' factors.
template <int CT>
__device__ __forceinline__ void msda_build_tap(const MsdaGeom &g, int pair_byte, int pair, int tap, bool on, const void *loc,
                                               const void *attn, Dcn3Tap &t, int &H, int &W) {
  t.lx = t.ly = t.m = 0.f;
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) t.off[ci] = kDcn3Oob;
  H = W = 1;
  if (!on) return;
  int start;
  msda_level(g, tap / g.P, H, W, start);
  const int e = pair * g.K + tap;
  Dcn3Sample s;
  msda_position<CT>(loc, e, H, W, s);
  t.lx = s.lx;
  t.ly = s.ly;
  t.m = dcn3_ld<CT>(attn, e);
#pragma unroll
  for (int ci = 0; ci < 4; ++ci)
    if (dcn3_corner_read(s, ci, H, W)) t.off[ci] = pair_byte + (start + dcn3_corner_pixel(s, ci, W)) * g.C * g.esz;
}
#endif  // __HIPCC__

}  // namespace mdconv
