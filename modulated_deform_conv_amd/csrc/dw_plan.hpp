// dw_plan.hpp -- the plan of the depthwise family (host only): fp32 layers with groups == C_in.  Such a layer has no
// contraction over input channels -- a gather, one multiply per tap and channel, three reductions -- so it runs on VALU
// kernels of its own (dw_fwd.hip, dw_bwd.hip, dw_gi.hip) instead of a 16-times-padded seat at the MFMA tiles.
// A call is planned ONCE: dw_plan() decides whether the family takes it and lays its workspace out, the byte count reported
// to the caller is the plan's `total`, and dw_forward / dw_backward take the plan instead of deriving any of it again.
#pragma once
#include "host_util.hpp"
#include "mfma_kernels.hpp"   // zero_bytes, record_weight_ready

namespace mdconv {

constexpr int kDwTile = 64;        // backward: output pixels per workgroup (lane = pixel, the four waves split the channels)
constexpr int kDwRowGroup = 32;    // grad_weight: partial rows summed per workgroup of the first reduce stage
constexpr int kDwMaxSplit = 8;     // backward: most workgroups that share the channels of one deformable group

struct DwPlan {
  Geom g;             // the caller's geometry (acc_* and det as the call sets them)
  bool backward;
  Skip skip;          // backward: gradients the call leaves out -- their stages are not run, their slots take no bytes
  int M;              // channel multiplier C_out / C_in (1 .. 4)
  int cs;             // forward: channels per thread (8 where the deformable groups allow, else 4)
  // backward, coordinate and weight gradients (dw_bwd.hip)
  int tiles;          // pixel tiles of kDwTile = partial rows of grad_weight / grad_bias
  int csplit;         // workgroups per (pixel tile, deformable group); > 1: grad_offset / grad_mask go through partial slices
  int row_len;        // floats per partial row: C_out * K weight sums, then C_out bias sums (with bias)
  int row_groups;     // rows of the second reduce stage (0: one stage)
  // backward, grad_input (dw_gi.hip): scatter lists per (image, deformable group, input pixel), one entry per corner:
  // B * DG segments of S_i lists, K * S_o * 2^nd entries per segment
  ScatterLists lists;
  int cs_gi;          // channels per thread of the gather (8 / 4)
  size_t off_goff, off_gm, off_wpart, off_wstage, off_wt;
  size_t total;       // workspace bytes
};

// false: the family does not take the call; *why names the rule it breaks (the text of a forced MDCONV_PATH_DEPTHWISE
// refusal).  `skip` never changes the answer.
bool dw_plan(const Geom &g, int dtype, bool backward, DwPlan *p, Skip skip, const char **why);
int dw_forward(const DwPlan &p, const Tensors &t, hipStream_t stream);
// records the weights-ready event itself once grad_weight / grad_bias are final (not with skip.weight: the caller has)
int dw_backward(const DwPlan &p, const Tensors &t, void *ws, hipStream_t stream);

// ---- kernels' launchers (one translation unit each, so the instances compile side by side) ----
int dw_fwd_launch(const DwPlan &p, const Tensors &t, hipStream_t stream);
// part_off / part_m: slices [csplit][...] of the shape of grad_offset / grad_mask (csplit > 1), wpart: [tiles][row_len]
int dw_bwd_coord_launch(const DwPlan &p, const Tensors &t, float *part_off, float *part_m, float *wpart, hipStream_t stream);
// dst[grp][e] (+)= sum over the rows r of group grp, in row order, of src[r * stride + e]: groups of `group` rows, e < len
int dw_reduce_rows(const float *src, int64_t stride, int nrows, int len, int group, float *dst, int64_t dst_stride, bool acc,
                   hipStream_t stream);
// the list kernel, counting or filling (the callable of scatter_lists_build)
void dw_list_launch(const DwPlan &p, const Tensors &t, bool fill, int *cnt, const int *rowptr, void *entries, hipStream_t stream);
int dw_weight_table_launch(const DwPlan &p, const float *weight, float *wt, hipStream_t stream);   // wt[tap][C_out]
int dw_gather_launch(const DwPlan &p, const Tensors &t, const int *rowptr, const void *entries, const float *wt, hipStream_t stream);

}  // namespace mdconv
