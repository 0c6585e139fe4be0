// dcn3_gi.hip -- grad_input of the DCNv3 core operator (dcn3_plan.hpp), without floating-point atomics: the scatter of
// the published operator inverted into lists, then a gather (the method of dw_gi.hip, for this operator's layouts).
//
// Lists: per (image, group, input pixel) one 16-byte entry per corner the forward read -- {sample = tap * S_o + pixel,
// corner weight x mask, tap, pixel} -- built in three passes (count with integer atomics, exclusive scan with
// csr_scan_chunk, fill); in deterministic mode csr_sort_rows brings every list into canonical order (ascending sample; a
// sample reaches a pixel through one corner).  Thread = sample in the order of `offset` and `mask`, so both are read
// coalesced.
// Gather: lane = one 16-byte channel vector of one (input pixel, group) pair, the lane mapping of the forward.  A lane walks
// its pair's list once; per entry it loads one 16-byte vector of grad_output at (output pixel, group) -- contiguous across
// the pair's lanes -- accumulates in fp32 and stores 16 bytes in the caller's mode.  Without the sort the order of a list
// is the order its integer atomics arrived in: grad_input then agrees from call to call to rounding.
#include "dcn3_plan.hpp"

namespace mdconv {

namespace {

__global__ __launch_bounds__(256) void dcn3_scan_kernel(int S, const int *__restrict__ cnt, int *__restrict__ rowptr) {
  csr_scan_chunk(S, cnt, rowptr);   // mdconv_common.hpp
}

// thread = sample (output pixel, group, tap).  FILL false: count the entries per target; true: after the scan, take slots
// from the back of each list (the counters run down to zero) and write the entries.
template <int DT, bool FILL>
__global__ __launch_bounds__(256) void dcn3_list_kernel(Dcn3Geom g, const void *__restrict__ offset, const void *__restrict__ mask,
                                                         int *__restrict__ cnt, const int *__restrict__ rowptr,
                                                         int4 *__restrict__ entries, int64_t seg_stride) {
  const int total = g.N * g.G * g.K;   // elements of `mask`: below 2^30
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const int pair = id / g.K, tap = id - pair * g.K;
  const int n = pair / g.G, grp = pair - n * g.G;
  const int b = n / g.S_o, pix = n - b * g.S_o;
  const Dcn3Pix px = dcn3_pix(g, pair);
  Dcn3Sample s;
  dcn3_position(g, px, tap, dcn3_ld<DT>(offset, 2 * id), dcn3_ld<DT>(offset, 2 * id + 1), s);
  const float mk = FILL ? dcn3_ld<DT>(mask, id) : 1.f;
  const int seg = b * g.G + grp;
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    if (!dcn3_corner_read(s, ci, g.H, g.W)) continue;
    const int q = dcn3_corner_pixel(s, ci, g.W);
    int *c = cnt + (int64_t)seg * g.S_i + q;
    if (!FILL) {
      atomicAdd(c, 1);
    } else {
      const int slot = rowptr[(int64_t)seg * (g.S_i + 1) + q] + atomicSub(c, 1) - 1;
      entries[(int64_t)seg * seg_stride + slot] =
          make_int4(tap * g.S_o + pix, __float_as_int(dcn3_corner_weight(s.lx, s.ly, ci) * mk), tap, pix);
    }
  }
}

template <int DT>
__global__ __launch_bounds__(256) void dcn3_gather_kernel(Dcn3Geom g, int64_t seg_stride, const void *__restrict__ grad_output,
                                                           const int *__restrict__ rowptr, const int4 *__restrict__ entries,
                                                           void *__restrict__ grad_input) {
  constexpr int NV = Dcn3Vec<DT>::NV;
  const Dcn3Lane ln = dcn3_lane(g, g.B * g.S_i * g.G);   // pair = (b * S_i + q) * G + group
  const int n = ln.pair / g.G, grp = ln.pair - n * g.G;
  const int b = n / g.S_i, q = n - b * g.S_i;
  const int seg = b * g.G + grp;
  const int *rp = rowptr + (int64_t)seg * (g.S_i + 1) + q;
  const int e0 = rp[0], e1 = ln.live ? rp[1] : e0;
  const int4 *ent = entries + (int64_t)seg * seg_stride;
  const rsrc_t r_go = make_rsrc(grad_output, (size_t)g.N * g.C * g.esz);
  const unsigned img_row = (unsigned)(b * g.S_o);
  const unsigned row_bytes = (unsigned)(g.C * g.esz), grp_byte = (unsigned)(grp * g.D * g.esz);
  for (int rd = 0; rd < g.rounds; ++rd) {   // one round unless a group has more than 64 vectors
    const int v = rd * g.VL + ln.j;
    if (!(ln.live && v < g.V)) continue;
    const unsigned vbyte = grp_byte + (unsigned)v * 16u;
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    for (int e = e0; e < e1; ++e) {
      const int4 en = ent[e];
      const float w = __int_as_float(en.y);
      float x[NV];
      dcn3_unpack<DT>(buf_load4(r_go, (int)((img_row + (unsigned)en.w) * row_bytes + vbyte), 0), x);
#pragma unroll
      for (int i = 0; i < NV; ++i) acc[i] = fmaf(w, x[i], acc[i]);
    }
    float4 *dst = (float4 *)grad_input + (int64_t)ln.pair * g.V + v;
    if (g.acc) {
      float old[NV];
      dcn3_unpack<DT>(*dst, old);
#pragma unroll
      for (int i = 0; i < NV; ++i) acc[i] += old[i];
    }
    *dst = dcn3_pack<DT>(acc);
  }
}

int grid_1d(int64_t n) { return (int)((n + 255) / 256); }

}  // namespace

int dcn3_lists_launch(const Dcn3Plan &p, const Dcn3Tensors &t, int *cnt, int *rowptr, void *entries, void *sort_scratch,
                      hipStream_t stream) {
  const Dcn3Geom &g = p.g;
  const dim3 grid(grid_1d((int64_t)g.N * g.G * g.K));
  int rc;
#define DCN3_LIST(DT, FILL)                                                                                           \
  hipLaunchKernelGGL((dcn3_list_kernel<DT, FILL>), grid, dim3(256), 0, stream, g, t.offset, t.mask, cnt, (const int *)rowptr, \
                     (int4 *)entries, p.seg_stride)
#define DCN3_LIST_DT(FILL)                                                                                            \
  do {                                                                                                                \
    if (p.dtype == MDCONV_F32) DCN3_LIST(MDCONV_F32, FILL);                                                           \
    else if (p.dtype == MDCONV_F16) DCN3_LIST(MDCONV_F16, FILL);                                                      \
    else DCN3_LIST(MDCONV_BF16, FILL);                                                                                \
  } while (0)
  DCN3_LIST_DT(false);
  if ((rc = check_launch("dcn3_list_count"))) return rc;
  hipLaunchKernelGGL(dcn3_scan_kernel, dim3((g.S_i + kScanChunk - 1) / kScanChunk, p.nseg), dim3(256), 0, stream, g.S_i, cnt, rowptr);
  if ((rc = check_launch("dcn3_scan"))) return rc;
  DCN3_LIST_DT(true);
#undef DCN3_LIST_DT
#undef DCN3_LIST
  if ((rc = check_launch("dcn3_list_fill"))) return rc;
  if (!sort_scratch) return MDCONV_OK;
  return csr_sort_rows(rowptr, entries, sort_scratch, 1, g.S_i, p.seg_stride, p.nseg, stream);
}

int dcn3_gather_launch(const Dcn3Plan &p, const Dcn3Tensors &t, const int *rowptr, const void *entries, hipStream_t stream) {
  const Dcn3Geom &g = p.g;
  const dim3 grid(dcn3_grid(g, (int64_t)g.B * g.S_i * g.G));
#define DCN3_GATHER(DT)                                                                                               \
  hipLaunchKernelGGL((dcn3_gather_kernel<DT>), grid, dim3(256), 0, stream, g, p.seg_stride, t.grad_output, rowptr,     \
                     (const int4 *)entries, t.grad_input)
  if (p.dtype == MDCONV_F32) DCN3_GATHER(MDCONV_F32);
  else if (p.dtype == MDCONV_F16) DCN3_GATHER(MDCONV_F16);
  else DCN3_GATHER(MDCONV_BF16);
#undef DCN3_GATHER
  return check_launch("dcn3_gather");
}

}  // namespace mdconv
