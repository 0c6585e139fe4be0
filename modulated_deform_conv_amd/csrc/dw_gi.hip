// dw_gi.hip -- grad_input of the depthwise family (dw_plan.hpp), without floating-point atomics: the scatter of the
// reference inverted into lists, then a gather.
//
// Lists: per (image, deformable group, input pixel) one entry per corner the reference scatters to -- {sample = tap * S_o +
// pixel, scatter weight x mask, tap, pixel} -- built in the three passes of the fp32 matrix family (count with integer
// atomics, exclusive scan, fill: scatter_lists_build); in deterministic mode csr_sort_rows brings every list into canonical
// order (ascending sample; a sample reaches a pixel through one corner).  The lists do not depend on the channel.
// Gather: lane = input pixel, workgroup = 256 pixels of one image x a slab of CS channels of one deformable group.  A lane
// walks its list once and rebuilds grad_col(c, tap, p) = sum_m w[cM + m, tap] * go[cM + m, p] for its CS channels on the fly
// from grad_output and the [tap][C_out] weight table -- grad_col rows are never stored -- and stores NCHW, coalesced along
// the pixels, in the caller's mode.  Without the sort the order of a list is the order its integer atomics arrived in:
// grad_input then agrees from call to call to rounding, as on the matrix families.
#include "dw_plan.hpp"

namespace mdconv {

namespace {

// thread = sample (image, deformable group, tap, output pixel).  FILL false: count the entries per target; true: after the
// scan, take slots from the back of each list (the counters run down to zero) and write the entries.
template <int ND, bool FILL>
__global__ __launch_bounds__(256) void dw_list_kernel(Geom g, const float *__restrict__ offset, const float *__restrict__ mask,
                                                       int *__restrict__ cnt, const int *__restrict__ rowptr,
                                                       int4 *__restrict__ entries, int64_t seg_stride) {
  const int64_t total = (int64_t)g.B * g.DG * g.K * g.S_o;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const int pix = (int)(id % g.S_o);
  const int64_t r = id / g.S_o;
  const int tap = (int)(r % g.K);
  const int seg = (int)(r / g.K);   // b * DG + dg
  int o[ND], t[ND];
  out_coords<ND>(g, pix, o);
  tap_coords<ND>(g, tap, t);
  float delta[ND];
  const int64_t obase = ((int64_t)seg * (ND * g.K) + ND * tap) * g.S_o + pix;
#pragma unroll
  for (int a = 0; a < ND; ++a) delta[a] = offset[obase + (int64_t)a * g.S_o];
  TapCoef<ND, float> tc;
  make_tap<ND, float>(g, o, t, delta, true, tc);
  const float mk = (FILL && g.modulated) ? mask[((int64_t)seg * g.K + tap) * g.S_o + pix] : 1.f;
#pragma unroll
  for (int ci = 0; ci < (1 << ND); ++ci) {
    const float w = corner_weight_atom<ND, float>(tc, ci);
    if (w == 0.f) continue;   // the reference scatters nothing there (weight 0: outside the image or gated off)
    const int q = corner_index<ND, float>(tc, ci);
    int *c = cnt + (int64_t)seg * g.S_i + q;
    if (!FILL) {
      atomicAdd(c, 1);
    } else {
      const int slot = rowptr[(int64_t)seg * (g.S_i + 1) + q] + atomicSub(c, 1) - 1;
      entries[(int64_t)seg * seg_stride + slot] = make_int4(tap * g.S_o + pix, __float_as_int(w * mk), tap, pix);
    }
  }
}

// wt[tap][o] = weight[o][tap]
__global__ __launch_bounds__(256) void dw_weight_table_kernel(int O, int K, const float *__restrict__ weight, float *__restrict__ wt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= O * K) return;
  const int tap = i / O, o = i - tap * O;
  wt[i] = weight[(int64_t)o * K + tap];
}

template <int M, int CS>
__global__ __launch_bounds__(256) void dw_gather_kernel(Geom g, int64_t seg_stride, const float *__restrict__ grad_output,
                                                         const float *__restrict__ wt, const int *__restrict__ rowptr,
                                                         const int4 *__restrict__ entries, float *__restrict__ grad_input) {
  const int qtiles = (g.S_i + 255) / 256;
  const int b = blockIdx.x / qtiles;
  const int q = (blockIdx.x - b * qtiles) * 256 + threadIdx.x;
  if (q >= g.S_i) return;
  const int c0 = blockIdx.y * CS;   // CS divides C_in / deformable_groups
  const int seg = b * g.DG + c0 / g.Cdg;
  const int *rp = rowptr + (int64_t)seg * (g.S_i + 1) + q;
  const int e0 = rp[0], e1 = rp[1];
  const int4 *ent = entries + (int64_t)seg * seg_stride;
  const float *go = grad_output + (int64_t)(b * g.O + c0 * M) * g.S_o;
  float acc[CS];
#pragma unroll
  for (int cc = 0; cc < CS; ++cc) acc[cc] = 0.f;
  for (int e = e0; e < e1; ++e) {
    const int4 en = ent[e];
    const float w = __int_as_float(en.y);
    const float4 *wrow = (const float4 *)(wt + (int64_t)en.z * g.O + c0 * M);   // CS * M floats, 16-byte aligned (4 | C_in)
    float wv[CS * M];
#pragma unroll
    for (int i = 0; i < CS * M / 4; ++i) {
      const float4 x = wrow[i];
      wv[4 * i] = x.x; wv[4 * i + 1] = x.y; wv[4 * i + 2] = x.z; wv[4 * i + 3] = x.w;
    }
    const float *gp = go + en.w;
#pragma unroll
    for (int cc = 0; cc < CS; ++cc) {
      float gcol = 0.f;
#pragma unroll
      for (int m = 0; m < M; ++m) gcol = fmaf(wv[cc * M + m], gp[(int64_t)(cc * M + m) * g.S_o], gcol);
      acc[cc] = fmaf(w, gcol, acc[cc]);
    }
  }
#pragma unroll
  for (int cc = 0; cc < CS; ++cc) {
    float *d = grad_input + (int64_t)(b * g.C + c0 + cc) * g.S_i + q;
    *d = g.acc_data ? *d + acc[cc] : acc[cc];
  }
}

int grid_1d(int64_t n) { return (int)((n + 255) / 256); }

}  // namespace

int dw_weight_table_launch(const DwPlan &p, const float *weight, float *wt, hipStream_t stream) {
  const Geom &g = p.g;
  hipLaunchKernelGGL(dw_weight_table_kernel, dim3(grid_1d((int64_t)g.O * g.K)), dim3(256), 0, stream, g.O, g.K, weight, wt);
  return check_launch("dw_weight_table");
}

void dw_list_launch(const DwPlan &p, const Tensors &t, bool fill, int *cnt, const int *rowptr, void *entries, hipStream_t stream) {
  const Geom &g = p.g;
  const int64_t samples = (int64_t)g.B * g.DG * g.K * g.S_o;   // < 2^29: the offset tensor is below 2^31 bytes
  const dim3 grid(grid_1d(samples));
#define DW_LIST(ND, FILL)                                                                                              \
  hipLaunchKernelGGL((dw_list_kernel<ND, FILL>), grid, dim3(256), 0, stream, g, (const float *)t.offset, (const float *)t.mask, \
                     cnt, rowptr, (int4 *)entries, p.lists.seg_stride)
  if (fill) { if (g.nd == 2) DW_LIST(2, true); else DW_LIST(3, true); }
  else { if (g.nd == 2) DW_LIST(2, false); else DW_LIST(3, false); }
#undef DW_LIST
}

int dw_gather_launch(const DwPlan &p, const Tensors &t, const int *rowptr, const void *entries, const float *wt, hipStream_t stream) {
  const Geom &g = p.g;
  const dim3 grid(g.B * ((g.S_i + 255) / 256), g.C / p.cs_gi);
#define DW_GATHER(M, CS)                                                                                               \
  hipLaunchKernelGGL((dw_gather_kernel<M, CS>), grid, dim3(256), 0, stream, g, p.lists.seg_stride, (const float *)t.grad_output, wt, \
                     rowptr, (const int4 *)entries, (float *)t.grad_input)
#define DW_GATHER_CS(M) do { if (p.cs_gi == 8) DW_GATHER(M, 8); else DW_GATHER(M, 4); } while (0)
  switch (p.M) {
    case 1: DW_GATHER_CS(1); break;
    case 2: DW_GATHER_CS(2); break;
    case 3: DW_GATHER_CS(3); break;
    default: DW_GATHER_CS(4); break;
  }
#undef DW_GATHER_CS
#undef DW_GATHER
  return check_launch("dw_gather");
}

}  // namespace mdconv
