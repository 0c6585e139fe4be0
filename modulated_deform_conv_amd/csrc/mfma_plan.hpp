// mfma_plan.hpp -- the plans of the fp32 matrix-core family (host only).  A call is planned ONCE: mfma_plan() decides
// how it runs and lays its workspace out, the byte count reported to the caller is the plan's `total`, and execution takes
// the plan -- sub-plans included -- instead of deriving any of it again, so size and use cannot drift apart.
#pragma once
#include "host_util.hpp"
#include "mfma_kernels.hpp"
#include "mfma_tile.hpp"

namespace mdconv {

// ---- native tiling (mfma_kernels.hip): batch chunks below 2 GiB per tensor, fp16 / bf16 through fp32 copies ----
struct Plan {
  int Bc;             // images per chunk; a call has at most two chunk sizes: Bc and the tail B % Bc
  bool half_io;
  Geom gc;            // geometry of a full chunk
  // backward: workspace layout of a full chunk and of the tail chunk (laid out anew, it can need MORE than a full one)
  BwdDims bd, bd_tail;
  size_t core_bytes;  // workspace of the fp32 kernels for one chunk: the larger need of the two chunk sizes
  size_t off_w, off_b, off_x, off_off, off_m, off_go, off_out, off_gi, off_goff, off_gm, off_gw, off_gb;
  size_t total;
  Skip skip;          // backward: gradients the call leaves out -- their stages are not run, their slots take no bytes
};
// false: the kernels do not tile `g` (or one image exceeds 32-bit buffer offsets).  `skip` never changes the answer,
// the chunks or the tiling.
bool native_plan(const Geom &g, int dtype, bool backward, Plan *p, Skip skip = Skip());
// `g` is the geometry `p` was made for; with_bias alone may differ from it where the caller sized for the larger need
// (split plans: the slices of a conv group after the first run without bias)
int native_forward(const Geom &g, int dtype, const Plan &p, const Tensors &t, void *ws, hipStream_t stream);
int native_backward(const Geom &g, int dtype, const Plan &p, const Tensors &t, void *ws, hipStream_t stream);

// ---- deformable groups the kernels do not tile, as DG single-group slices (mfma_plans.hip) ----
struct SplitPlan {     // backward
  Geom gs;             // one slice: DG = 1, C = C_in / DG, the conv groups / output channels it touches; without bias
  bool copy_w, copy_go;
  size_t off_x, off_off, off_m, off_go, off_w, off_gi, off_goff, off_gm, off_gw, off_sub, total;
  // The first slice of a conv group carries grad_bias and then has the grad_bias stage buffer in its layout: `first` is
  // planned from the geometry that slice runs with (gs with the caller's with_bias) and sizes the slices' workspace,
  // `rest` from gs itself
  Plan first, rest;
};
struct SplitFwdPlan {
  Geom gs;
  bool copy_w, copy_out;
  size_t off_x, off_off, off_m, off_w, off_out, off_sub, total;
  Plan sub;            // of gs (the forward's layout does not depend on with_bias)
};
// ---- the same shapes, and channel counts off the kernels' tiles, as ONE zero-padded problem (mfma_plans.hip) ----
struct PadPlan {
  Geom gp;            // the padded problem
  bool pad_c, pad_o;  // input channels / output channels padded
  // channel groups of the input (conv groups, else deformable groups): count, channels each (caller's / padded);
  // output groups (conv groups): count, channels each; weight sub-rows per output channel ([O][DG][C_dg][K] with one conv group)
  int ng, cin, cinp, nog, og, ogp, wsub;
  size_t off_x, off_w, off_gi, off_gw, off_o, off_b, off_gb, off_sub, total;   // off_o: output (forward) / grad_output (backward)
  Plan sub;           // of gp
};

// The plan of one call of the family.
struct MfmaPlan {
  enum Kind { NATIVE, PADDED, SPLIT_FWD, SPLIT_BWD } kind;
  bool backward;
  size_t total;       // workspace bytes
  Skip skip;          // backward: gradients the call leaves out
  Plan native;
  PadPlan pad;
  SplitFwdPlan split_fwd;
  SplitPlan split_bwd;
};
// Priority: padded where the padded problem is the faster one (pad_channels_preferred), native, padded, split.
// false: the family does not run this shape / dtype.  `wgrad32` (a 16-bit backward with fp32 grad_weight / grad_bias,
// MDCONV_WGRAD_F32) sizes the padded / sliced plans' grad_weight rows for 4-byte elements; it never changes the kind.
// `skip` (a backward without grad_input / without the weight gradients) never changes the kind either: the plans drop the
// skipped gradients' stages, copies and workspace slots (MfmaPlan::skip).
bool mfma_plan(const Geom &g, int dtype, bool backward, MfmaPlan *p, bool wgrad32 = false, Skip skip = Skip());
int mfma_forward(const Geom &g, int dtype, const MfmaPlan &p, const Tensors &t, void *ws, hipStream_t stream);
int mfma_backward(const Geom &g, int dtype, const MfmaPlan &p, const Tensors &t, void *ws, hipStream_t stream);

// ---- 16-bit tensors through fp32 copies in the workspace (f32_copies.hip) ----
// ... on the shape-generic backward kernels: one rounding per gradient instead of one per atomic add
struct D16Plan { size_t off_x, off_off, off_m, off_w, off_go, off_gi, off_goff, off_gm, off_gw, off_gb, total; };
D16Plan direct16_plan(const Geom &g);
// (`skip`: the weight kernel is not run / the narrowing copies of the skipped gradients are left out; the layout stays)
int direct16_backward(const Geom &g, int dtype, const D16Plan &p, const Tensors &t, void *ws, hipStream_t stream, Skip skip = Skip());

// ... with fp32 offsets / masks (MDCONV_SAMPLING_F32) on the fp32 kernels: fp32 copies of the 16-bit tensors, the caller's
// fp32 offsets / masks / grad_offset / grad_mask as they are; on the matrix kernels (`mfma`: their fp32 plan is `inner`,
// behind the copies) or on the shape-generic ones
struct S32Plan {
  size_t off_x, off_w, off_b, off_o, off_gi, off_gw, off_inner, total;   // off_o: output / grad_output
  bool mfma;
  MfmaPlan inner;
  Skip skip;   // backward: gradients the call leaves out (no fp32 buffer, no copies for them on the matrix kernels)
};
// want_mfma: take the matrix kernels where they have an fp32 plan for `g` (p->mfma tells)
void samp32_plan(const Geom &g, bool backward, bool want_mfma, S32Plan *p, Skip skip = Skip());
int samp32_forward(const Geom &g, int dtype, const S32Plan &p, const Tensors &t, void *ws, hipStream_t stream);
int samp32_backward(const Geom &g, int dtype, const S32Plan &p, const Tensors &t, void *ws, hipStream_t stream);

}  // namespace mdconv
