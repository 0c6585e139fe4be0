// hp_plan.hpp -- the plan of the native 16-bit (fp16 / bf16) family (host only).  A call is planned ONCE: hp_plan() decides
// whether the family takes it, the geometry its kernels run, the batch chunks, every chunk size's dimensions and kernels
// and the workspace layout; the byte count reported to the caller is the plan's `total`, and hp_forward / hp_backward
// take the plan instead of deriving any of it again, so size and use cannot drift apart (hp_host.hip).
#pragma once
#include "host_util.hpp"
#include "hp_kernels.hpp"

namespace mdconv {

// one chunk size of a call: its geometry, dimensions and kernel
struct HpChunk {
  Geom gc;
  HpDims hd;
  bool fwd2;                          // forward: hp_fwd2 (quad-contiguous gathers) or hp_fwd
  enum Bwd { BWD1, BWD2, BWD3 } bwd;  // backward: hp_bwd (lane = pixel), hp_bwd2 (tap-stationary), hp_bwd3 + hp_gemm2
};
struct HpFwdLayout { size_t off_xt, off_w, off_tab, total; };
struct HpBwdLayout {
  size_t off_xt, off_w, off_tab, off_gcol, off_col, off_part, off_gw32, off_cnt, off_rowptr, off_entries, off_sums, off_sort;
  // HpPlan::io32: the bf16 copy of one chunk's fp32 grad_output (behind the slots of the bf16 call); HpPlan::out_cl: the
  // [B, C_out, spatial] copy of one chunk's channels-last grad_output (the two modes exclude each other by dtype)
  size_t off_go16;
  size_t total;
};

struct HpPlan {
  Geom g;                  // the geometry the kernels run: the caller's, its group-padded or its width-padded form
  int Bc;                  // images per full chunk; a call has at most two chunk sizes: Bc and the tail B % Bc
  HpChunk full, tail;      // tail == full when B % Bc == 0
  HpFwdLayout fwd;         // the layout of the planned direction, built for the full chunk (the tail fits: checked)
  HpBwdLayout bwd;
  bool two_pass_gather;    // grad_input gather in two passes (MDCONV_HP_C2I, default) or one
  bool forward_preferred;  // forward only: false = a few pixel tiles over many K stages, the fp32 matrix kernels are faster
  size_t total;            // workspace bytes
  // backward: gradients the call leaves out (MDCONV_FLAG_NO_GRAD_INPUT / _WEIGHT).  Their stages are not run -- GEMM-2, the
  // split-K reduce and grad_bias; the list build, the sort and the gather -- and the slots only those stages use take no
  // bytes; hp_bwd3 chunks of a call without weight gradients run the kernel's variant without column rows.
  Skip skip;
  // fp32 tensors on the bf16 kernels (MDCONV_FLAG_MATH_BF16): the plan of the bf16 call with fp32 offsets / masks and fp32
  // weight gradients, whose layout passes read fp32 input and weights, whose forward and grad_input gather store fp32, and
  // whose backward converts each chunk's grad_output into off_go16 -- the one slot the mode adds
  bool io32;
  // Result layouts (MDCONV_FLAG_OUTPUT_CHANNELS_LAST / _GRAD_INPUT_CHANNELS_LAST): `out_cl` -- the forward stores `output`
  // as [B, spatial..., C_out] (the store policy of hp_fwd / hp_fwd2), the backward brings each chunk's channels-last
  // grad_output into off_go16 (hp_nhwc_to_nchw), the one slot the flag adds, and sums grad_bias from that copy; `gi_cl` --
  // the gather stores grad_input as [B, spatial..., C_in] (backward with grad_input only; no bytes).  Neither changes the
  // geometry, the chunks or their kernels: a channels-last tensor is batch-major too.
  // `layout_refusal`: null, or the rule a requested layout breaks (the text of mdconv_result_layout_supported's answer 0)
  bool out_cl, gi_cl;
  const char *layout_refusal;
};
// false: the family does not take the call.  `skip` never changes the answer, the geometry, the chunks or their kernels;
// nor does `io32` (with dtype MDCONV_BF16: the call's tensors are fp32, Tensors::io32).
// `out_cl` / `gi_cl`: the result layouts the call asks for (16-bit tensors only); recorded, sized and judged here --
// HpPlan::layout_refusal -- so that the query, the sizing and the execution cannot drift apart.
bool hp_plan(const Geom &g, int dtype, bool backward, HpPlan *p, Skip skip = Skip(), bool io32 = false, bool out_cl = false,
             bool gi_cl = false);
int hp_forward(int dtype, const HpPlan &p, const Tensors &t, void *ws, hipStream_t stream);
int hp_backward(int dtype, const HpPlan &p, const Tensors &t, void *ws, hipStream_t stream);

}  // namespace mdconv
