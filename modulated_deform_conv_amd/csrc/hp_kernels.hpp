// hp_kernels.hpp -- dimensions and launchers of the native 16-bit (fp16 / bf16) path (hp_*.hip); its plan: hp_plan.hpp.
#pragma once
#include "hp_common.hpp"

namespace mdconv {

// hp_host.hip (the planner and the kernel sequences: hp_plan.hpp)
HpDims hp_dims(const Geom &g);

// hp_prep.hip
// `f32src` (fp32 tensors on the bf16 kernels, Tensors::io32): `x` / `w` are fp32 and are rounded to bf16 inside the pass
int hp_nchw_to_nhwc(const Geom &g, const HpDims &hd, const void *x, void *xt, bool f32src, hipStream_t stream);
int hp_pack_fwd_weights(const Geom &g, const HpDims &hd, int dtype, const void *w, bool f32src, void *wpf,
                        int2 *ctab, hipStream_t stream);
int hp_pack_bwd_weights(const Geom &g, const HpDims &hd, int dtype, const void *w, bool f32src, void *wpb,
                        int4 *btab, hipStream_t stream);
// the inverse layout pass for a channels-last grad_output (Tensors::out_cl): dst[b][o][pix] = src[b][pix][o], 16-bit elements,
// O a multiple of 8 -- the copy of one chunk the backward kernels read (HpBwdLayout::off_go16)
int hp_nhwc_to_nchw(const Geom &g, const void *src, void *dst, hipStream_t stream);
// the bf16 copy of an fp32 grad_output (Tensors::io32), `n` elements
int hp_f32_to_bf16(const float *src, void *dst, int64_t n, hipStream_t stream);
// gw32 != nullptr (calls cut into batch chunks): running fp32 sum; grad_weight is written by the last chunk
// `ranges` = pixel ranges per tap in `part` (hd.ranges_w after hp_gemm2, hd.ranges after hp_bwd)
// `wgrad32`: grad_weight / grad_bias are fp32 buffers and receive the fp32 sums (Tensors::wgrad32)
int hp_reduce_grad_weight(const Geom &g, const HpDims &hd, int ranges, int dtype, const float *part,
                          const int4 *btab, void *grad_weight, bool wgrad32, float *gw32, bool first, bool last,
                          hipStream_t stream);
int hp_grad_bias(const Geom &g, int dtype, const void *grad_output, void *grad_bias, bool wgrad32,
                 hipStream_t stream);

// the same sum, bit for bit, from a channels-last grad_output [B, spatial..., C_out] (Tensors::out_cl, calls cut into batch chunks)
int hp_grad_bias_cl(const Geom &g, int dtype, const void *grad_output, void *grad_bias, bool wgrad32,
                    hipStream_t stream);

// hp_fwd.hip
int hp_forward_launch(const Geom &g, const HpDims &hd, int dtype, const Tensors &t, const void *xt,
                      const void *wpf, const int2 *ctab, hipStream_t stream);

// channels-last output (t.out_cl): instances in hp_fwd_cl.hip, reached through hp_forward_launch
int hp_forward_launch_cl(const Geom &g, const HpDims &hd, int dtype, const Tensors &t, const void *xt,
                         const void *wpf, const int2 *ctab, hipStream_t stream);

// hp_fwd2.hip: the same contraction with quad-contiguous (line-wide) gathers
int hp_forward2_launch(const Geom &g, const HpDims &hd, int dtype, const Tensors &t, const void *xt,
                       const void *wpf, const int2 *ctab, hipStream_t stream);

int hp_forward2_launch_cl(const Geom &g, const HpDims &hd, int dtype, const Tensors &t, const void *xt,
                          const void *wpf, const int2 *ctab, hipStream_t stream);   // hp_fwd2_cl.hip

// hp_bwd.hip: GEMM-1 + coordinate gradients + grad_col + GEMM-2, one gather pass
int hp_backward_launch(const Geom &g, const HpDims &hd, int dtype, const Tensors &t, const void *xt,
                       const void *wpb, const int4 *btab, void *gcol, float *part, int *cnt,
                       hipStream_t stream);
// fp32 offsets / masks (t.samp32): instances in hp_bwd_s32.hip, reached through hp_backward_launch
int hp_backward_launch_s32(const Geom &g, const HpDims &hd, int dtype, const Tensors &t, const void *xt,
                           const void *wpb, const int4 *btab, void *gcol, float *part, int *cnt,
                           hipStream_t stream);

// hp_bwd2.hip: the same kernel with line-wide gathers (thread roles change between phases)
size_t hp_bwd2_lds_bytes(const Geom &g, const HpDims &hd);
int hp_backward2_launch(const Geom &g, const HpDims &hd, int dtype, const Tensors &t, const void *xt,
                        const void *wpb, const int4 *btab, void *gcol, float *part, int *cnt,
                        hipStream_t stream);
int hp_backward2_launch_s32(const Geom &g, const HpDims &hd, int dtype, const Tensors &t, const void *xt,
                            const void *wpb, const int4 *btab, void *gcol, float *part, int *cnt,
                            hipStream_t stream);   // hp_bwd2_s32.hip

// hp_bwd3.hip: pixel-stationary GEMM-1 + coordinate gradients + grad_col rows + column rows (GEMM-2 is
// hp_gemm2.hip); one conv group, 1 / 2 / 4 deformable groups, Cp a power of two.  colbuf == nullptr (no GEMM-2 follows:
// MDCONV_FLAG_NO_GRAD_WEIGHT) launches the variant of the kernel that neither builds nor stores the column rows.
bool hp_bwd3_supported(const Geom &g, const HpDims &hd);
size_t hp_bwd3_lds_bytes(const Geom &g, const HpDims &hd);
int hp_backward3_launch(const Geom &g, const HpDims &hd, int dtype, const Tensors &t, const void *xt,
                        const void *wpb, void *gcol, void *colbuf, int *cnt, hipStream_t stream);

// hp_gemm2.hip: grad_W partials = grad_out . col^T over the column rows, dense, split over pixel ranges
size_t hp_gemm2_lds_bytes(const HpDims &hd);
int hp_gemm2_launch(const Geom &g, const HpDims &hd, int dtype, const Tensors &t, const int4 *btab,
                    const void *colbuf, float *part, hipStream_t stream);

// hp_col2im.hip: inverse scatter map (counting pass inside the fused backward kernel) + gather
int hp_csr_zero(const Geom &g, int *cnt, hipStream_t stream);
int hp_csr_build(const Geom &g, int dtype, const Tensors &t, int *cnt, int *rowptr, void *entries,
                 hipStream_t stream);
int hp_col2im(const Geom &g, const HpDims &hd, int dtype, const Tensors &t, const void *gcol,
              const int *rowptr, const void *entries, hipStream_t stream);
// channels-last grad_input (t.gi_cl): instances in hp_col2im_cl.hip, reached through hp_col2im / hp_col2im2 (pass 2)
int hp_col2im_cl(const Geom &g, const HpDims &hd, int dtype, const Tensors &t, const void *gcol,
                 const int *rowptr, const void *entries, hipStream_t stream);
int hp_col2im_combine_cl(const Geom &g, const HpDims &hd, int dtype, const Tensors &t, const void *sums, hipStream_t stream);
// two-pass gather: per-anchor partial sums (every grad_col row read once) -> stencil + transpose
size_t hp_col2im_sums_bytes(const Geom &g, const HpDims &hd, int dtype);
int hp_col2im2(const Geom &g, const HpDims &hd, int dtype, const Tensors &t, const void *gcol,
               const int *rowptr, const void *entries, void *sums, hipStream_t stream);

}  // namespace mdconv
