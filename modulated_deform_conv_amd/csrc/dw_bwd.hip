// dw_bwd.hip -- backward of the depthwise family (dw_plan.hpp): grad_offset, grad_mask, grad_weight and grad_bias in one
// kernel, without floating-point atomics.
//
// Workgroup = kDwTile output pixels (lane = pixel) x the channels of one deformable group (or one of `csplit` shares of
// them); the four waves take the group's four-channel chunks in turn.  Taps outside, channels inside.
//   grad_col(c, tap, p) = sum_m w[cM + m, tap] * go[cM + m, p] is a rank-1 product: computed in registers, never stored.
//   grad_offset / grad_mask: summed over the wave's channels inside the lane, over the four waves through LDS in wave order.
//     One share per group (csplit == 1): stored from there in the caller's mode.  Several: each share stores its slice, and
//     dw_reduce_rows adds the slices in order.
//   grad_weight / grad_bias: every (output channel, tap) belongs to one wave of one workgroup per pixel tile; its sum over the
//     tile's 64 pixels (a fixed butterfly) is element (channel, tap) of the tile's partial row, and dw_reduce_rows adds the
//     rows in row order (the split-K pattern of reduce_weight_kernel).
#include "dw_plan.hpp"

namespace mdconv {

namespace {

__device__ __forceinline__ float dw_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int ND, int M>
__global__ __launch_bounds__(256) void dw_bwd_coord_kernel(Geom g, int csplit, int row_len, const float *__restrict__ input,
                                                            const float *__restrict__ weight, const float *__restrict__ offset,
                                                            const float *__restrict__ mask, const float *__restrict__ grad_output,
                                                            float *__restrict__ grad_offset, float *__restrict__ grad_mask,
                                                            float *__restrict__ part_off, float *__restrict__ part_m,
                                                            float *__restrict__ wpart) {
  constexpr int CS = 4, NC = 1 << ND;
  __shared__ float red[4][ND + 1][kDwTile];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = blockIdx.x;
  const int dg = blockIdx.y / csplit, share = blockIdx.y - dg * csplit;
  const int n_raw = tile * kDwTile + lane;
  const bool live = n_raw < g.N;
  const int n = live ? n_raw : g.N - 1;
  const int b = n / g.S_o;
  const int pix = n - b * g.S_o;
  int o[ND];
  out_coords<ND>(g, pix, o);
  const int nchunk = g.Cdg / CS;
  const int64_t obase = ((int64_t)(b * g.DG + dg) * (ND * g.K)) * g.S_o + pix;
  const int64_t mbase = ((int64_t)(b * g.DG + dg) * g.K) * g.S_o + pix;
  const int64_t n_off = (int64_t)g.B * g.DG * ND * g.K * g.S_o;
  float *wrow = wpart ? wpart + (int64_t)tile * row_len : nullptr;

  for (int tap = 0; tap < g.K; ++tap) {
    float delta[ND];
#pragma unroll
    for (int a = 0; a < ND; ++a) delta[a] = offset[obase + (int64_t)(ND * tap + a) * g.S_o];
    const float mk = g.modulated ? mask[mbase + (int64_t)tap * g.S_o] : 1.f;
    int t[ND];
    tap_coords<ND>(g, tap, t);
    TapCoef<ND, float> tc;
    make_tap<ND, float>(g, o, t, delta, true, tc);
    int cidx[NC];
    float cw[NC], cdw[ND][NC];
    bool cr[NC];
#pragma unroll
    for (int ci = 0; ci < NC; ++ci) {
      cidx[ci] = corner_index<ND, float>(tc, ci);
      cw[ci] = corner_weight<ND, float>(tc, ci);
      cr[ci] = corner_is_read<ND, float>(tc, ci);
#pragma unroll
      for (int a = 0; a < ND; ++a) cdw[a][ci] = corner_dweight<ND, float>(tc, ci, a);
    }
    float goff[ND], gm = 0.f;
#pragma unroll
    for (int a = 0; a < ND; ++a) goff[a] = 0.f;

    for (int j = share * 4 + wave; j < nchunk; j += 4 * csplit) {   // wave-uniform
#pragma unroll
      for (int cc = 0; cc < CS; ++cc) {
        const int c = dg * g.Cdg + j * CS + cc;
        float go[M], gcol = 0.f;
#pragma unroll
        for (int m = 0; m < M; ++m) {
          go[m] = live ? grad_output[(int64_t)(b * g.O + c * M + m) * g.S_o + pix] : 0.f;
          gcol = fmaf(weight[(int64_t)(c * M + m) * g.K + tap], go[m], gcol);
        }
        const float *plane = input + (int64_t)(b * g.C + c) * g.S_i;
        float v[NC], val = 0.f;
#pragma unroll
        for (int ci = 0; ci < NC; ++ci) {
          v[ci] = cr[ci] ? plane[cidx[ci]] : 0.f;   // never read by the reference otherwise
          val += cw[ci] * v[ci];
        }
#pragma unroll
        for (int a = 0; a < ND; ++a) {
          float dv = 0.f;
#pragma unroll
          for (int ci = 0; ci < NC; ++ci) dv += cdw[a][ci] * v[ci];
          goff[a] += dv * gcol;
        }
        gm += val * gcol;
        if (wrow) {
          const float col = live ? val * mk : 0.f;   // the re-materialised forward column; lanes past the last pixel add nothing
#pragma unroll
          for (int m = 0; m < M; ++m) {
            const float s = dw_wave_sum(go[m] * col);
            if (lane == 0) wrow[(int64_t)(c * M + m) * g.K + tap] = s;
            if (g.with_bias && tap == 0) {
              const float sb = dw_wave_sum(go[m]);
              if (lane == 0) wrow[(int64_t)g.O * g.K + c * M + m] = sb;
            }
          }
        }
      }
    }
    const bool gate = !g.range_gate || tc.inside;
#pragma unroll
    for (int a = 0; a < ND; ++a) red[wave][a][lane] = gate ? goff[a] * mk : 0.f;
    red[wave][ND][lane] = gm;
    __syncthreads();
    // wave a sums component a (the nd offset axes, then the mask) over the four waves, in wave order
    if (wave <= ND && (wave < ND || g.modulated) && live) {
      const float s = ((red[0][wave][lane] + red[1][wave][lane]) + red[2][wave][lane]) + red[3][wave][lane];
      if (wave < ND) {
        const int64_t at = obase + (int64_t)(ND * tap + wave) * g.S_o;
        if (csplit > 1) part_off[(int64_t)share * n_off + at] = s;
        else grad_offset[at] = g.acc_data ? grad_offset[at] + s : s;
      } else {
        const int64_t at = mbase + (int64_t)tap * g.S_o;
        if (csplit > 1) part_m[(int64_t)share * (n_off / ND) + at] = s;
        else grad_mask[at] = g.acc_data ? grad_mask[at] + s : s;
      }
    }
    __syncthreads();
  }
}

// dst[grp * dst_stride + e] (+)= sum over the rows r of group grp, in row order, of src[r * stride + e]
__global__ __launch_bounds__(256) void dw_reduce_rows_kernel(const float *__restrict__ src, int64_t stride, int nrows, int len,
                                                              int group, float *__restrict__ dst, int64_t dst_stride, int acc) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= len) return;
  const int r0 = blockIdx.y * group, r1 = min(nrows, r0 + group);
  const float *s = src + e;
  float sum = 0.f;
  int r = r0;
  for (; r + 8 <= r1; r += 8) {   // eight loads in flight, one chain of adds in row order
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = s[(int64_t)(r + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += v[u];
  }
  for (; r < r1; ++r) sum += s[(int64_t)r * stride];
  float *d = dst + (int64_t)blockIdx.y * dst_stride + e;
  *d = acc ? *d + sum : sum;
}

}  // namespace

int dw_reduce_rows(const float *src, int64_t stride, int nrows, int len, int group, float *dst, int64_t dst_stride, bool acc,
                   hipStream_t stream) {
  if (len <= 0 || nrows <= 0) return MDCONV_OK;
  const dim3 grid((len + 255) / 256, (nrows + group - 1) / group);
  hipLaunchKernelGGL(dw_reduce_rows_kernel, grid, dim3(256), 0, stream, src, stride, nrows, len, group, dst, dst_stride, acc ? 1 : 0);
  return check_launch("dw_reduce_rows");
}

int dw_bwd_coord_launch(const DwPlan &p, const Tensors &t, float *part_off, float *part_m, float *wpart, hipStream_t stream) {
  const Geom &g = p.g;
  const dim3 grid(p.tiles, g.DG * p.csplit);
#define DW_BWD(ND, M)                                                                                                     \
  hipLaunchKernelGGL((dw_bwd_coord_kernel<ND, M>), grid, dim3(256), 0, stream, g, p.csplit, p.row_len,                    \
                     (const float *)t.input, (const float *)t.weight, (const float *)t.offset, (const float *)t.mask,     \
                     (const float *)t.grad_output, (float *)t.grad_offset, (float *)t.grad_mask, part_off, part_m, wpart)
#define DW_BWD_M(ND)                      \
  switch (p.M) {                          \
    case 1: DW_BWD(ND, 1); break;         \
    case 2: DW_BWD(ND, 2); break;         \
    case 3: DW_BWD(ND, 3); break;         \
    default: DW_BWD(ND, 4); break;        \
  }
  if (g.nd == 2) { DW_BWD_M(2) } else { DW_BWD_M(3) }
#undef DW_BWD_M
#undef DW_BWD
  return check_launch("dw_bwd_coord");
}

}  // namespace mdconv
