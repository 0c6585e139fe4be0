// samp_gather.hip -- the gradient of the sampled tensor of the channels-last sampling operators (samp_core.hpp: grad_input of
// the DCNv3 core operator, grad_value of deformable attention), without floating-point atomics: the scatter of the published
// operators inverted into lists (scatter_lists_build with samp_list_kernel), then this gather.
//
// Lane = one 16-byte channel vector of one (row of the sampled tensor, head) pair, the lane mapping of the forward.  A lane
// walks its pair's list once; per entry it loads one 16-byte vector of grad_output at (output row, head) -- contiguous across
// the pair's lanes -- accumulates in fp32 and stores 16 bytes in the caller's mode, so a row that no sample touches is written
// (zero) or left (accumulate) by the same kernel.  In deterministic mode the lists are sorted; without it the order of a list
// is the order its integer atomics arrived in, and the gradient agrees from call to call to rounding.
#include "samp_core.hpp"

namespace mdconv {

namespace {

template <int DT>
__global__ __launch_bounds__(256) void samp_gather_kernel(SampGather g, int64_t seg_stride, const void *__restrict__ grad_output,
                                                           const int *__restrict__ rowptr, const int4 *__restrict__ entries,
                                                           void *__restrict__ grad_in) {
  constexpr int NV = SampVec<DT>::NV;
  const SampLane ln = samp_lane_of(g.ln.lgVL, g.imgs * g.rows_in * g.heads);   // pair = (img * rows_in + r) * heads + head
  const int n = ln.pair / g.heads, head = ln.pair - n * g.heads;
  const int img = n / g.rows_in, r = n - img * g.rows_in;
  const int seg = img * g.heads + head;
  const int *rp = rowptr + (int64_t)seg * (g.rows_in + 1) + r;
  const int e0 = rp[0], e1 = ln.live ? rp[1] : e0;
  const int4 *ent = entries + (int64_t)seg * seg_stride;
  const rsrc_t r_go = make_rsrc(grad_output, (size_t)g.imgs * g.rows_out * g.C * g.ln.esz);
  const unsigned img_row = (unsigned)(img * g.rows_out);
  const unsigned row_bytes = (unsigned)(g.C * g.ln.esz), head_byte = (unsigned)(head * g.D * g.ln.esz);
  for (int rd = 0; rd < g.ln.rounds; ++rd) {   // one round unless a head has more than 64 vectors
    const int v = rd * g.ln.VL + ln.j;
    if (!(ln.live && v < g.ln.V)) continue;
    const unsigned vbyte = head_byte + (unsigned)v * 16u;
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    for (int e = e0; e < e1; ++e) {
      const int4 en = ent[e];
      const float w = __int_as_float(en.y);
      float x[NV];
      samp_unpack<DT>(buf_load4(r_go, (int)((img_row + (unsigned)en.w) * row_bytes + vbyte), 0), x);
#pragma unroll
      for (int i = 0; i < NV; ++i) acc[i] = fmaf(w, x[i], acc[i]);
    }
    float4 *dst = (float4 *)grad_in + (int64_t)ln.pair * g.ln.V + v;
    if (g.acc) {
      float old[NV];
      samp_unpack<DT>(*dst, old);
#pragma unroll
      for (int i = 0; i < NV; ++i) acc[i] += old[i];
    }
    *dst = samp_pack<DT>(acc);
  }
}

}  // namespace

int samp_gather_launch(const SampGather &ga, int dtype, int64_t seg_stride, const void *grad_output, const int *rowptr,
                       const void *entries, void *grad_in, hipStream_t stream) {
  const dim3 grid(samp_grid(ga.ln.lgVL, (int64_t)ga.imgs * ga.rows_in * ga.heads));
#define SAMP_GATHER(DT)                                                                                            \
  hipLaunchKernelGGL((samp_gather_kernel<DT>), grid, dim3(256), 0, stream, ga, seg_stride, grad_output, rowptr,   \
                     (const int4 *)entries, grad_in)
  if (dtype == MDCONV_F32) SAMP_GATHER(MDCONV_F32);
  else if (dtype == MDCONV_F16) SAMP_GATHER(MDCONV_F16);
  else SAMP_GATHER(MDCONV_BF16);
#undef SAMP_GATHER
  return check_launch("samp_gather");
}

}  // namespace mdconv
