// mfma_col2im.hip -- step 3 of the fp32 backward (overview: mfma_bwd_data.hip): grad_input from grad_col and the
// inverted scatter map, 2-D pair-keyed lists (the 3-D sample-keyed lists: mfma_csr3d.hip).
//
//   grad_input[b][c][q] (+)= sum over the entries e of anchor q of wx_e * gcol[b][src_e][c]
//                           + sum over the entries e of anchor q-1 of wy_e * gcol[b][src_e][c]
//
// A file of its own: these kernels are plain VALU + vector-memory code that runs BESIDE GEMM-2 on the forked stream, and
// they are compiled with the default flags (mfma_bwd_data.hip turns the SLP vectoriser off for GEMM-1's drain).
// What was tried on that co-run and what it gave: profiles/gather_corun.md.
#include "mfma_kernels.hpp"
#include "mfma_tile.hpp"

namespace mdconv {

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
// constant address space: a wave-uniform address read through it is a scalar load.  rowptr / entries are written by the
// kernels BEFORE the gather and by nobody during it.
typedef const __attribute__((address_space(4))) int *kint_p;
typedef const __attribute__((address_space(4))) i32x4 *kent_p;

// the two accumulators of a lane's 4 channels as register pairs: one v_pk_fma_f32 per pair
struct Acc4 { f32x2 lo, hi; };
__device__ __forceinline__ void acc_fma(Acc4 &a, float w, const float4 &v) {
  const f32x2 w2 = {w, w};
  a.lo = __builtin_elementwise_fma(w2, (f32x2){v.x, v.y}, a.lo);
  a.hi = __builtin_elementwise_fma(w2, (f32x2){v.z, v.w}, a.hi);
}

// ---------------------------------------------------------------------------------------------
// workgroup = 32 consecutive q of one image x 256 channels; a wave WALKS a run of 8 consecutive
// anchors with two accumulators per lane: `cur` (target = the anchor) and `nxt` (target = anchor
// + 1); after an anchor, cur is the finished target, nxt becomes cur.  Every grad_col row is
// thus read once per corner PAIR.  The run starts one anchor early to pick up the carry; rows of
// the image need no special case: pairs never straddle a row (make_pairs), so the anchor in the
// last column has an empty list and hands a zero carry to the next row.
// ---------------------------------------------------------------------------------------------
constexpr int kRun = 8;   // targets per wave run

// N list entries from `at`: the list is wave-uniform, so entries, row addresses and weights stay in SGPRs (scalar loads, no
// VALU instruction per entry); N row loads in flight, then the sums in list order.
template <int N>
__device__ __forceinline__ void gather_step(const rsrc_t &r_gc, kent_p ent, int at, int c_voff, int row_bytes,
                                            Acc4 &cur, Acc4 &nxt) {
  float4 v[N];
  float wx[N], wy[N];
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const i32x4 e = ent[at + u];
    wx[u] = __int_as_float(e.y);
    wy[u] = __int_as_float(e.z);
    v[u] = buf_load4(r_gc, c_voff, e.x * row_bytes);
  }
#pragma unroll
  for (int u = 0; u < N; ++u) {
    acc_fma(cur, wx[u], v[u]);
    acc_fma(nxt, wy[u], v[u]);
  }
}

template <int ND>
__global__ __launch_bounds__(256) void col2im_gather_kernel(Geom g, const float *__restrict__ gcol,
                                                            const int *__restrict__ rowptr,
                                                            const int4 *__restrict__ entries,
                                                            float *__restrict__ grad_input) {
  constexpr int NP = 1 << (ND - 1);
  constexpr int QT = 4 * kRun;
  __shared__ float tile[256 * (QT + 1)];   // [c][q], pitch 33
  const int qtiles = (g.S_i + QT - 1) / QT;
  // keep neighbouring q tiles on ONE XCD: the rows they share are then re-read from its L2
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int b = bid / qtiles;
  const int q0 = (bid - b * qtiles) * QT;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const rsrc_t r_gc = make_rsrc(gcol + (size_t)b * g.K * g.S_o * g.C, (size_t)g.K * g.S_o * g.C * 4);
  for (int cb = blockIdx.y * 256; cb < g.C; cb += gridDim.y * 256) {
    const int seg = b * g.DG + cb / g.Cdg;   // C_dg is a multiple of 256 here (or DG == 1)
    const int *rp = rowptr + (int64_t)seg * (g.S_i + 1);
    const int4 *ent = entries + (int64_t)seg * ((int64_t)g.K * g.S_o * NP);
    const int c4 = cb + lane * 4;
    const int c_voff = (c4 < g.C ? c4 : 0) * 4;   // C % 4 == 0
    const int qs = q0 + wave * kRun;              // first target of this wave's run
    // The list of an anchor is wave-uniform: its bounds and entries come over the scalar path, 16 entries a step.
    const kint_p rps = (kint_p)rp;
    const kent_p ents = (kent_p)ent;
    Acc4 cur = {{0.f, 0.f}, {0.f, 0.f}}, nxt = cur;
    for (int a = qs - 1; a < qs + kRun; ++a) {
      if (a >= 0 && a < g.S_i) {
        const int e0 = rps[a], e1 = rps[a + 1];
        int at = e0;
        for (; at + 16 <= e1; at += 16) gather_step<16>(r_gc, ents, at, c_voff, g.C * 4, cur, nxt);
        // the rest of the list in exact steps of 8 / 4 / 2 / 1: no padded rows
        if ((e1 - at) & 8) { gather_step<8>(r_gc, ents, at, c_voff, g.C * 4, cur, nxt); at += 8; }
        if ((e1 - at) & 4) { gather_step<4>(r_gc, ents, at, c_voff, g.C * 4, cur, nxt); at += 4; }
        if ((e1 - at) & 2) { gather_step<2>(r_gc, ents, at, c_voff, g.C * 4, cur, nxt); at += 2; }
        if ((e1 - at) & 1) gather_step<1>(r_gc, ents, at, c_voff, g.C * 4, cur, nxt);
      }
      if (a >= qs) {
        float *tp = tile + (lane * 4) * (QT + 1) + (a - q0);
        tp[0] = cur.lo.x; tp[QT + 1] = cur.lo.y; tp[2 * (QT + 1)] = cur.hi.x; tp[3 * (QT + 1)] = cur.hi.y;
      }
      cur = nxt;
      nxt.lo = nxt.hi = (f32x2){0.f, 0.f};
    }
    __syncthreads();
    // transpose out: thread = (channel, 8 consecutive q); a wave covers 8 channels x 32 q
    {
      const int cl = threadIdx.x >> 2, qs8 = (threadIdx.x & 3) * 8;
      for (int cc = cl; cc < 256; cc += 64) {
        const int c = cb + cc;
        if (c < g.C) {
          float *dst = grad_input + ((int64_t)b * g.C + c) * g.S_i + q0 + qs8;
          const float *src = tile + cc * (QT + 1) + qs8;
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (q0 + qs8 + k < g.S_i) dst[k] = g.acc_data ? dst[k] + src[k] : src[k];
        }
      }
    }
    __syncthreads();
  }
}

// Deformable groups narrower than 256 channels: LPD = C_dg / 4 lanes cover one group, so a wave
// walks 64 / LPD runs of ONE group at a time (lane = (run j, channel quad r)); each lane group
// follows its own lists.  Entries are fetched LPD at a time (lane r <- entry r) and broadcast
// inside the lane group with a width-limited shuffle.
template <int ND, int LPD>
__global__ __launch_bounds__(256) void col2im_gather_grouped_kernel(
    Geom g, const float *__restrict__ gcol, const int *__restrict__ rowptr,
    const int4 *__restrict__ entries, float *__restrict__ grad_input) {
  constexpr int NP = 1 << (ND - 1);
  constexpr int QT = 4 * kRun, NQ = 64 / LPD;   // targets per tile, runs per wave
  constexpr int CDG = LPD * 4;                    // channels per deformable group
  constexpr int DPB = 256 / CDG;                  // groups per 256-channel block
  constexpr int RPT = QT / kRun;                  // runs per tile (4)
  constexpr int UB = LPD < 16 ? LPD : 16;         // row loads in flight per step
  __shared__ float tile[256 * (QT + 1)];          // [c][q], pitch 33
  const int qtiles = (g.S_i + QT - 1) / QT;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int b = bid / qtiles;
  const int q0 = (bid - b * qtiles) * QT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane / LPD, r = lane % LPD;
  const rsrc_t r_gc = make_rsrc(gcol + (size_t)b * g.K * g.S_o * g.C, (size_t)g.K * g.S_o * g.C * 4);
  for (int cb = 0; cb < g.C; cb += 256) {
    // work items of the block: (group d of DPB) x (RPT / NQ sets of NQ runs)
    for (int item = wave; item < DPB * (RPT / NQ); item += 4) {
      const int d = item / (RPT / NQ), run = (item % (RPT / NQ)) * NQ + j;
      const int c4 = cb + d * CDG + r * 4;
      const int qs = q0 + run * kRun;
      const bool chan_on = c4 < g.C;
      const int seg = b * g.DG + min(c4, g.C - 1) / g.Cdg;
      const int *rp = rowptr + (int64_t)seg * (g.S_i + 1);
      const int4 *ent = entries + (int64_t)seg * ((int64_t)g.K * g.S_o * NP);
      const int c_voff = (chan_on ? c4 : 0) * 4;
      float4 cur = make_float4(0.f, 0.f, 0.f, 0.f), nxt = cur;
      for (int step = 0; step <= kRun; ++step) {
        const int a = qs - 1 + step;
        const bool on = chan_on && a >= 0 && a < g.S_i;
        const int e0 = on ? rp[a] : 0, e1 = on ? rp[a + 1] : 0;
        for (int base = e0; __any(base < e1); base += LPD) {
          const int cnt = max(0, min(LPD, e1 - base));
          const int4 mine = (r < cnt) ? ent[base + r] : make_int4(0, 0, 0, 0);   // weights 0, row 0 beyond
#pragma unroll
          for (int u0 = 0; u0 < LPD; u0 += UB) {
            float4 v[UB];
            float wx[UB], wy[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
              const int src = __shfl(mine.x, u0 + u, LPD);
              wx[u] = __int_as_float(__shfl(mine.y, u0 + u, LPD));
              wy[u] = __int_as_float(__shfl(mine.z, u0 + u, LPD));
              v[u] = buf_load4(r_gc, src * g.C * 4 + c_voff, 0);
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
              cur.x = fmaf(wx[u], v[u].x, cur.x); cur.y = fmaf(wx[u], v[u].y, cur.y);
              cur.z = fmaf(wx[u], v[u].z, cur.z); cur.w = fmaf(wx[u], v[u].w, cur.w);
              nxt.x = fmaf(wy[u], v[u].x, nxt.x); nxt.y = fmaf(wy[u], v[u].y, nxt.y);
              nxt.z = fmaf(wy[u], v[u].z, nxt.z); nxt.w = fmaf(wy[u], v[u].w, nxt.w);
            }
          }
        }
        if (step > 0) {
          float *tp = tile + (d * CDG + r * 4) * (QT + 1) + (a - q0);
          tp[0] = cur.x; tp[QT + 1] = cur.y; tp[2 * (QT + 1)] = cur.z; tp[3 * (QT + 1)] = cur.w;
        }
        cur = nxt;
        nxt = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    __syncthreads();
    {
      const int cl = threadIdx.x >> 2, qs8 = (threadIdx.x & 3) * 8;
      for (int cc = cl; cc < 256; cc += 64) {
        const int c = cb + cc;
        if (c < g.C) {
          float *dst = grad_input + ((int64_t)b * g.C + c) * g.S_i + q0 + qs8;
          const float *src = tile + cc * (QT + 1) + qs8;
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (q0 + qs8 + k < g.S_i) dst[k] = g.acc_data ? dst[k] + src[k] : src[k];
        }
      }
    }
    __syncthreads();
  }
}


// Few channels (C_in = 64 or 128, one deformable group): with lanes = channel quads only C/4 lanes
// of a wave would carry data, so a wave walks 64 / LPD runs side by side (lane = (run j, channel
// quad r)), all of the same image; tile = 4 * (64 / LPD) runs of kRun targets.
template <int ND, int LPD>
__global__ __launch_bounds__(256) void col2im_gather_narrow_kernel(
    Geom g, const float *__restrict__ gcol, const int *__restrict__ rowptr,
    const int4 *__restrict__ entries, float *__restrict__ grad_input) {
  constexpr int NP = 1 << (ND - 1);
  constexpr int NQ = 64 / LPD, RUNS = 4 * NQ, QT = RUNS * kRun;   // runs per wave / tile, targets
  constexpr int CW = LPD * 4;                                      // channels (== C_in)
  constexpr int UB = LPD < 16 ? LPD : 16;
  __shared__ float tile[CW * (QT + 1)];                            // [c][q]
  const int qtiles = (g.S_i + QT - 1) / QT;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int b = bid / qtiles;
  const int q0 = (bid - b * qtiles) * QT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane / LPD, r = lane % LPD;
  const rsrc_t r_gc = make_rsrc(gcol + (size_t)b * g.K * g.S_o * g.C, (size_t)g.K * g.S_o * g.C * 4);
  const int *rp = rowptr + (int64_t)b * (g.S_i + 1);
  const int4 *ent = entries + (int64_t)b * ((int64_t)g.K * g.S_o * NP);
  const int qs = q0 + (wave * NQ + j) * kRun;
  const int c_voff = r * 16;
  float4 cur = make_float4(0.f, 0.f, 0.f, 0.f), nxt = cur;
  for (int step = 0; step <= kRun; ++step) {
    const int a = qs - 1 + step;
    const bool on = a >= 0 && a < g.S_i;
    const int e0 = on ? rp[a] : 0, e1 = on ? rp[a + 1] : 0;
    for (int base = e0; __any(base < e1); base += LPD) {
      const int cnt = max(0, min(LPD, e1 - base));
      const int4 mine = (r < cnt) ? ent[base + r] : make_int4(0, 0, 0, 0);   // weights 0, row 0 beyond
#pragma unroll
      for (int u0 = 0; u0 < LPD; u0 += UB) {
        float4 v[UB];
        float wx[UB], wy[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const int src = __shfl(mine.x, u0 + u, LPD);
          wx[u] = __int_as_float(__shfl(mine.y, u0 + u, LPD));
          wy[u] = __int_as_float(__shfl(mine.z, u0 + u, LPD));
          v[u] = buf_load4(r_gc, src * g.C * 4 + c_voff, 0);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          cur.x = fmaf(wx[u], v[u].x, cur.x); cur.y = fmaf(wx[u], v[u].y, cur.y);
          cur.z = fmaf(wx[u], v[u].z, cur.z); cur.w = fmaf(wx[u], v[u].w, cur.w);
          nxt.x = fmaf(wy[u], v[u].x, nxt.x); nxt.y = fmaf(wy[u], v[u].y, nxt.y);
          nxt.z = fmaf(wy[u], v[u].z, nxt.z); nxt.w = fmaf(wy[u], v[u].w, nxt.w);
        }
      }
    }
    if (step > 0) {
      float *tp = tile + (r * 4) * (QT + 1) + (a - q0);
      tp[0] = cur.x; tp[QT + 1] = cur.y; tp[2 * (QT + 1)] = cur.z; tp[3 * (QT + 1)] = cur.w;
    }
    cur = nxt;
    nxt = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  // transpose out: rows of 32 consecutive q per channel (whole 128-byte lines)
  for (int x = threadIdx.x; x < CW * (QT / 8); x += 256) {
    const int c = x / (QT / 8), qs8 = (x % (QT / 8)) * 8;
    float *dst = grad_input + ((int64_t)b * g.C + c) * g.S_i + q0 + qs8;
    const float *src = tile + c * (QT + 1) + qs8;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (q0 + qs8 + k < g.S_i) dst[k] = g.acc_data ? dst[k] + src[k] : src[k];
  }
}

}  // namespace

int col2im_f32(const Geom &g, const BwdDims &bd, const Tensors &t, const float *gcol,
               const int *rowptr, const void *entries, float *sums, hipStream_t stream) {
  if (bd.sample_keyed) return col2im3d_f32(g, bd, t, gcol, rowptr, entries, sums, stream);
  const int qtiles = (g.S_i + 31) / 32;
  const dim3 grid(g.B * qtiles, 1);
#define LAUNCH_GG(ND, LPD)                                                                      \
  hipLaunchKernelGGL((col2im_gather_grouped_kernel<ND, LPD>), grid, dim3(256), 0, stream, g,    \
                     gcol, rowptr, (const int4 *)entries, (float *)t.grad_input)
#define LAUNCH_NARROW(ND, LPD)                                                                  \
  do {                                                                                          \
    const int qt = 4 * (64 / LPD) * kRun;                                                       \
    hipLaunchKernelGGL((col2im_gather_narrow_kernel<ND, LPD>), dim3(g.B * ((g.S_i + qt - 1) / qt)), \
                       dim3(256), 0, stream, g, gcol, rowptr, (const int4 *)entries,            \
                       (float *)t.grad_input);                                                  \
  } while (0)
  // (2-D only from here: the pair-keyed lists)
  if (g.DG == 1 && g.C == 64) {
    LAUNCH_NARROW(2, 16);
  } else if (g.DG == 1 && g.C == 128) {
    LAUNCH_NARROW(2, 32);
  } else if (g.DG > 1 && g.Cdg == 64) {
    LAUNCH_GG(2, 16);
  } else if (g.DG > 1 && g.Cdg == 128) {
    LAUNCH_GG(2, 32);
  } else {
    hipLaunchKernelGGL((col2im_gather_kernel<2>), grid, dim3(256), 0, stream, g, gcol, rowptr,
                       (const int4 *)entries, (float *)t.grad_input);
  }
#undef LAUNCH_GG
#undef LAUNCH_NARROW
  return check_launch("col2im_gather");
}

}  // namespace mdconv
