// msda_gi.hip -- grad_value of multi-scale deformable attention (msda_plan.hpp), without floating-point atomics: the
// scatter of the published operator inverted into lists, then a gather (the method of dcn3_gi.hip, for this operator's
// layouts).
//
// Lists: per (image, head, value row over all S rows of the concatenated levels) one 16-byte entry per corner the forward
// read -- {sample = tap * Lq + q, corner weight x attention weight, tap, q} -- built in three passes (count with integer
// atomics, exclusive scan with csr_scan_chunk, fill); in deterministic mode csr_sort_rows brings every list into canonical
// order (ascending sample; a sample reaches a row through one corner).  Thread = sample in the order of the coordinate
// tensors, so both are read coalesced.
// Gather: lane = one 16-byte channel vector of one (value row, head) pair, pair = (n * S + s) * M + m: the lane mapping of
// the forward.  A lane walks its pair's list once; per entry it loads one 16-byte vector of grad_output at (query, head)
// -- contiguous across the pair's lanes -- accumulates in fp32 and stores 16 bytes in the caller's mode, so a row that no
// sample touches is written (zero) or left (accumulate) by the same kernel.  Without the sort the order of a list is the
// order its integer atomics arrived in: grad_value then agrees from call to call to rounding.
#include "msda_plan.hpp"

namespace mdconv {

namespace {

__global__ __launch_bounds__(256) void msda_scan_kernel(int S, const int *__restrict__ cnt, int *__restrict__ rowptr) {
  csr_scan_chunk(S, cnt, rowptr);   // mdconv_common.hpp
}

// thread = sample (query, head, tap).  FILL false: count the entries per target; true: after the scan, take slots from the
// back of each list (the counters run down to zero) and write the entries.
template <int CT, bool FILL>
__global__ __launch_bounds__(256) void msda_list_kernel(MsdaGeom g, const void *__restrict__ loc, const void *__restrict__ attn,
                                                         int *__restrict__ cnt, const int *__restrict__ rowptr,
                                                         int4 *__restrict__ entries, int64_t seg_stride) {
  const int total = g.npairs * g.K;   // elements of attention_weights: below 2^30
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const int pair = id / g.K, tap = id - pair * g.K;
  const int nq = pair / g.M, m = pair - nq * g.M;
  const int n = nq / g.Lq, q = nq - n * g.Lq;
  int H, W, start;
  msda_level(g, tap / g.P, H, W, start);
  Dcn3Sample s;
  msda_position<CT>(loc, id, H, W, s);
  const float a = FILL ? dcn3_ld<CT>(attn, id) : 1.f;
  const int seg = n * g.M + m;
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    if (!dcn3_corner_read(s, ci, H, W)) continue;
    const int row = start + dcn3_corner_pixel(s, ci, W);
    int *c = cnt + (int64_t)seg * g.S + row;
    if (!FILL) {
      atomicAdd(c, 1);
    } else {
      const int slot = rowptr[(int64_t)seg * (g.S + 1) + row] + atomicSub(c, 1) - 1;
      entries[(int64_t)seg * seg_stride + slot] =
          make_int4(tap * g.Lq + q, __float_as_int(dcn3_corner_weight(s.lx, s.ly, ci) * a), tap, q);
    }
  }
}

template <int DT>
__global__ __launch_bounds__(256) void msda_gather_kernel(MsdaGeom g, int64_t seg_stride, const void *__restrict__ grad_output,
                                                           const int *__restrict__ rowptr, const int4 *__restrict__ entries,
                                                           void *__restrict__ grad_value) {
  constexpr int NV = Dcn3Vec<DT>::NV;
  const Dcn3Lane ln = dcn3_lane_of(g.lgVL, g.N * g.S * g.M);   // pair = (n * S + s) * M + m
  const int ns = ln.pair / g.M, m = ln.pair - ns * g.M;
  const int n = ns / g.S, s = ns - n * g.S;
  const int seg = n * g.M + m;
  const int *rp = rowptr + (int64_t)seg * (g.S + 1) + s;
  const int e0 = rp[0], e1 = ln.live ? rp[1] : e0;
  const int4 *ent = entries + (int64_t)seg * seg_stride;
  const rsrc_t r_go = make_rsrc(grad_output, (size_t)g.npairs * g.D * g.esz);
  const unsigned img_row = (unsigned)(n * g.Lq);
  const unsigned row_bytes = (unsigned)(g.C * g.esz), head_byte = (unsigned)(m * g.D * g.esz);
  for (int rd = 0; rd < g.rounds; ++rd) {   // one round unless a head has more than 64 vectors
    const int v = rd * g.VL + ln.j;
    if (!(ln.live && v < g.V)) continue;
    const unsigned vbyte = head_byte + (unsigned)v * 16u;
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
    float4 *dst = (float4 *)grad_value + (int64_t)ln.pair * g.V + v;
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

int msda_lists_launch(const MsdaPlan &p, const MsdaTensors &t, int *cnt, int *rowptr, void *entries, void *sort_scratch,
                      hipStream_t stream) {
  const MsdaGeom &g = p.g;
  const dim3 grid(grid_1d((int64_t)g.npairs * g.K));
  int rc;
#define MSDA_LIST(CT, FILL)                                                                                        \
  hipLaunchKernelGGL((msda_list_kernel<CT, FILL>), grid, dim3(256), 0, stream, g, t.loc, t.attn, cnt, (const int *)rowptr, \
                     (int4 *)entries, p.seg_stride)
#define MSDA_LIST_CT(FILL)                                                                                         \
  do {                                                                                                             \
    if (p.coord_dtype == MDCONV_F32) MSDA_LIST(MDCONV_F32, FILL);                                                  \
    else if (p.coord_dtype == MDCONV_F16) MSDA_LIST(MDCONV_F16, FILL);                                             \
    else MSDA_LIST(MDCONV_BF16, FILL);                                                                             \
  } while (0)
  MSDA_LIST_CT(false);
  if ((rc = check_launch("msda_list_count"))) return rc;
  hipLaunchKernelGGL(msda_scan_kernel, dim3((g.S + kScanChunk - 1) / kScanChunk, p.nseg), dim3(256), 0, stream, g.S, cnt, rowptr);
  if ((rc = check_launch("msda_scan"))) return rc;
  MSDA_LIST_CT(true);
#undef MSDA_LIST_CT
#undef MSDA_LIST
  if ((rc = check_launch("msda_list_fill"))) return rc;
  if (!sort_scratch) return MDCONV_OK;
  return csr_sort_rows(rowptr, entries, sort_scratch, 1, g.S, p.seg_stride, p.nseg, stream);
}

int msda_gather_launch(const MsdaPlan &p, const MsdaTensors &t, const int *rowptr, const void *entries, hipStream_t stream) {
  const MsdaGeom &g = p.g;
  const dim3 grid(msda_grid(g, (int64_t)g.N * g.S * g.M));
#define MSDA_GATHER(DT)                                                                                            \
  hipLaunchKernelGGL((msda_gather_kernel<DT>), grid, dim3(256), 0, stream, g, p.seg_stride, t.grad_output, rowptr, \
                     (const int4 *)entries, t.grad_value)
  if (p.dtype == MDCONV_F32) MSDA_GATHER(MDCONV_F32);
  else if (p.dtype == MDCONV_F16) MSDA_GATHER(MDCONV_F16);
  else MSDA_GATHER(MDCONV_BF16);
#undef MSDA_GATHER
  return check_launch("msda_gather");
}

}  // namespace mdconv
