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
  size_t off_xt, off_w, off_tab, off_gcol, off_col, off_part, off_gw32, off_cnt, off_rowptr, off_entries, off_sums, off_sort, total;
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
};
// false: the family does not take the call.  `skip` never changes the answer, the geometry, the chunks or their kernels.
bool hp_plan(const Geom &g, int dtype, bool backward, HpPlan *p, Skip skip = Skip());
int hp_forward(int dtype, const HpPlan &p, const Tensors &t, void *ws, hipStream_t stream);
int hp_backward(int dtype, const HpPlan &p, const Tensors &t, void *ws, hipStream_t stream);

}  // namespace mdconv
