// samp_core.hpp -- the sampling core of the channels-last sampling operators: the DCNv3 core operator (dcn3_plan.hpp) and
// multi-scale deformable attention (msda_plan.hpp).  Both read four corner vectors of a sampled tensor per (pair, tap), weigh
// them bilinearly times one more factor (mask / attention weight) and sum over the taps; they differ in how a tap's position
// comes about and in their layouts.  Everything else lives here once: the lane mapping, the 16-byte vector helpers, the
// sampling arithmetic, and the forward, coordinate-backward and list kernels as templates over an OPERATOR POLICY.
//
// Lane mapping of every kernel: a lane owns one 16-byte channel vector (4 floats / 8 halves) of one PAIR -- (output pixel,
// group) or (query, head), head fastest; the VL lanes of a pair (VL = the vectors per head V rounded up to a power of two, at
// most 64) are adjacent and the pairs of a pixel follow each other, so a wave's stores and each of its corner loads are
// contiguous 16-byte pieces.  Heads of more than 64 vectors (D > 256 fp32) take `rounds` > 1 passes over the vectors.
//
// An operator policy `Op` (Dcn3Op, MsdaOp, Dcn4Op, FdaOp, Dcn4SoftOp) supplies only what differs:
//   Op::Geom                       the kernel argument (POD, by value); it has K, D, acc and the lane geometry `ln`
//   Op::npairs(g), Op::sampled_bytes(g)
//   Op::Ctx, Op::ctx(g, pair)      what the taps of a pair have in common
//   Op::coord_index(g, cx, pair, tap, xy)   the element of `coord` that holds x (xy = 0) / y (xy = 1) of (pair, tap)
//   Op::factor_index(g, cx, pair, tap)   the element of `factor` that holds the factor of (pair, tap)
//   Op::build_tap<CT>(...)         the SampTap of (pair, tap), read from those two elements, and the factors fx, fy of the x
//                                  and y gradient sums
//   Op::finish_pair<CT>(...)       what the coordinate backward owes the gradient tensors beyond the taps (row padding)
//   Op::list_rows(g), Op::list_item<CT>(g, id, coord, it)   the scatter lists: targets per segment, and sample id -> SampItem
//   Op::list_factor_index(g, id)   factor_index by sample id = pair * K + tap
// The policy owns the addressing: the kernels never form an element index themselves, and the gradients go to the elements
// their forward values came from.  `coord` and `factor` may therefore be ONE tensor (the packed offset_mask rows of
// Dcn4Op), and so may grad_coord and grad_factor; see the qualifiers of samp_bwd_coord_kernel.
// A policy whose factor is a FUNCTION of the stored elements of its pair (FdaOp, Dcn4SoftOp: a softmax over the pair's
// logits) also has
//   Op::begin_pair<CT>(g, cx, ln, factor)   the pair's statistics into its context, taken by the pair's lanes together
//   Op::kPairSum, Op::factor_grad(a, gsum, s_pair)   the stored gradient of (pair, tap) from the tap's factor a, the sum
//                                  gsum the coordinate backward holds for it, and s_pair = sum over the pair's taps of a * gsum
//   Op::list_factor(g, id, raw)    the factor of sample id from its stored element
// and every other policy inherits the identities of SampPlainFactor.
// A policy with one more gradient summed from its taps' location gradients (AfdaOp) also has kTapGrads and tap_grads; see
// SampTapGrads below.
#pragma once
#include "host_util.hpp"
#include "mfma_tile.hpp"   // raw buffer loads

namespace mdconv {

// Lane geometry of a head of D channels of `esz` bytes (POD, part of every kernel argument).
struct SampLanes {
  int V, VL, lgVL, rounds;
  int esz;   // bytes per element
};
inline SampLanes samp_lanes(int D, int esz) {
  SampLanes l;
  l.esz = esz;
  l.V = D * esz / 16;
  l.lgVL = 0;
  while ((1 << l.lgVL) < l.V && l.lgVL < 6) ++l.lgVL;
  l.VL = 1 << l.lgVL;
  l.rounds = (l.V + l.VL - 1) / l.VL;
  return l;
}
// workgroups of 256 lanes that cover `npairs` pairs
inline int samp_grid(int lgVL, int64_t npairs) {
  const int64_t per_block = 4 * (64 >> lgVL);
  return (int)((npairs + per_block - 1) / per_block);
}

// The channels-last gather over scatter lists (samp_gather.hip): the gradient of the sampled tensor, [imgs][rows_in][heads * D],
// from grad_output [imgs][rows_out][heads * D] and the lists of scatter_lists_build (one segment per (image, head), one list
// per row; word 3 of an entry is the row of grad_output inside its image, word 1 the weight).
struct SampGather {
  int imgs, rows_in, rows_out, heads, D, C;   // C = heads * D
  SampLanes ln;
  int acc;   // 1 = add to the caller's buffer, 0 = overwrite
};
int samp_gather_launch(const SampGather &ga, int dtype, int64_t seg_stride, const void *grad_output, const int *rowptr,
                       const void *entries, void *grad_in, hipStream_t stream);
// The backward tail of the families that gather channels-last: the lists into the workspace (scatter_lists_build with the
// family's list kernel, `launch_list`), then the gather over them.
template <class Launch>
static int samp_lists_gather(const ScatterLists &L, void *ws, bool det, const SampGather &ga, int dtype, const void *grad_output,
                             void *grad_in, hipStream_t stream, Launch launch_list) {
  if (int rc = scatter_lists_build(L, ws, det, stream, launch_list)) return rc;
  return samp_gather_launch(ga, dtype, L.seg_stride, grad_output, (const int *)((char *)ws + L.off_rowptr),
                            (char *)ws + L.off_entries, grad_in, stream);
}

// the five (value type, coordinate type) pairings of a sampling operator: `call(DT, CT)` for the plan's
#define SAMP_DISPATCH(p, call)                                                       \
  do {                                                                               \
    if ((p).dtype == MDCONV_F32) call(MDCONV_F32, MDCONV_F32);                       \
    else if ((p).dtype == MDCONV_F16 && (p).coord_dtype == MDCONV_F16) call(MDCONV_F16, MDCONV_F16); \
    else if ((p).dtype == MDCONV_F16) call(MDCONV_F16, MDCONV_F32);                  \
    else if ((p).coord_dtype == MDCONV_BF16) call(MDCONV_BF16, MDCONV_BF16);         \
    else call(MDCONV_BF16, MDCONV_F32);                                              \
  } while (0)

#ifdef __HIPCC__
constexpr int kSampOob = 0x7ffffff0;   // out-of-range buffer offset: loads give 0 (every tensor is below 2^31 bytes)

// ---- the 16 bytes of a channel vector <-> its 4 / 8 values ----
template <int DT> struct SampVec { static constexpr int NV = DT == MDCONV_F32 ? 4 : 8; };

template <int DT> __device__ __forceinline__ float samp_ld(const void *p, int i) {
  if (DT == MDCONV_F32) return ((const float *)p)[i];
  if (DT == MDCONV_F16) return __half2float(((const __half *)p)[i]);
  return bf16_bits_to_float(((const unsigned short *)p)[i]);
}
// dst[i] = v, or dst[i] += v in the tensor's type (`acc`)
template <int DT> __device__ __forceinline__ void samp_st(void *p, int i, float v, bool acc) {
  if (acc) v += samp_ld<DT>(p, i);
  if (DT == MDCONV_F32) ((float *)p)[i] = v;
  else if (DT == MDCONV_F16) ((__half *)p)[i] = __float2half(v);
  else ((unsigned short *)p)[i] = float_to_bf16_bits(v);
}
template <int DT> __device__ __forceinline__ float samp_widen16(unsigned h) {
  return DT == MDCONV_F16 ? __half2float(__ushort_as_half((unsigned short)h)) : bf16_bits_to_float((unsigned short)h);
}
template <int DT> __device__ __forceinline__ unsigned samp_narrow16(float v) {
  return DT == MDCONV_F16 ? (unsigned)__half_as_ushort(__float2half(v)) : (unsigned)float_to_bf16_bits(v);
}
template <int DT> __device__ __forceinline__ void samp_unpack(const float4 &raw, float (&f)[SampVec<DT>::NV]) {
  if (DT == MDCONV_F32) {
    f[0] = raw.x; f[1] = raw.y; f[2] = raw.z; f[3] = raw.w;
  } else {
    const unsigned u[4] = {__float_as_uint(raw.x), __float_as_uint(raw.y), __float_as_uint(raw.z), __float_as_uint(raw.w)};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[(2 * i) % SampVec<DT>::NV] = samp_widen16<DT>(u[i] & 0xffffu);
      f[(2 * i + 1) % SampVec<DT>::NV] = samp_widen16<DT>(u[i] >> 16);
    }
  }
}
template <int DT> __device__ __forceinline__ float4 samp_pack(const float (&f)[SampVec<DT>::NV]) {
  if (DT == MDCONV_F32) return make_float4(f[0], f[1], f[2], f[3]);
  unsigned u[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    u[i] = samp_narrow16<DT>(f[(2 * i) % SampVec<DT>::NV]) | (samp_narrow16<DT>(f[(2 * i + 1) % SampVec<DT>::NV]) << 16);
  return make_float4(__uint_as_float(u[0]), __uint_as_float(u[1]), __uint_as_float(u[2]), __uint_as_float(u[3]));
}

// ---- sampling arithmetic ----
// A sibling of make_tap (mdconv_common.hpp) with these operators' gate; the four reference flavours there are not involved.
// The sample at (loc_h, loc_w) has the neighbours (y0 + cy, x0 + cx), corner ci = 2 * cy + cx, with the bilinear weights
// (cy ? ly : 1 - ly) * (cx ? lx : 1 - lx).  A corner is READ iff the sample passes the gate -1 < loc < size on both axes and
// the corner lies inside the image; every other corner contributes nothing to any result and is never loaded.
struct SampSample {
  float lx, ly;   // fractional parts
  int x0, y0;     // low neighbour (may be -1)
  bool inside;    // the gate
};
__device__ __forceinline__ void samp_sample(float loc_h, float loc_w, int H, int W, SampSample &s) {
  s.inside = loc_h > -1.f && loc_w > -1.f && loc_h < (float)H && loc_w < (float)W;
  // clamp before the int conversion so wild offsets (and NaN, which fails the gate) cannot overflow
  const float yc = s.inside ? loc_h : 0.f, xc = s.inside ? loc_w : 0.f;
  const float fy = floorf(yc), fx = floorf(xc);
  s.y0 = (int)fy;
  s.x0 = (int)fx;
  s.ly = yc - fy;
  s.lx = xc - fx;
}
__device__ __forceinline__ bool samp_corner_read(const SampSample &s, int ci, int H, int W) {
  const int y = s.y0 + (ci >> 1), x = s.x0 + (ci & 1);
  return s.inside && y >= 0 && y < H && x >= 0 && x < W;
}
__device__ __forceinline__ int samp_corner_pixel(const SampSample &s, int ci, int W) {
  return (s.y0 + (ci >> 1)) * W + s.x0 + (ci & 1);
}
__device__ __forceinline__ float samp_corner_weight(float lx, float ly, int ci) {
  return ((ci >> 1) ? ly : 1.f - ly) * ((ci & 1) ? lx : 1.f - lx);
}
// d(weight)/d(loc_w) and d(weight)/d(loc_h) of corner ci
__device__ __forceinline__ float samp_corner_dx(float ly, int ci) { return ((ci >> 1) ? ly : 1.f - ly) * ((ci & 1) ? 1.f : -1.f); }
__device__ __forceinline__ float samp_corner_dy(float lx, int ci) { return ((ci & 1) ? lx : 1.f - lx) * ((ci >> 1) ? 1.f : -1.f); }

// ---- lanes and taps ----
// The lane's place: j = its lane inside pair `pair` of `npairs`.  Lanes beyond the last pair are not live; they keep a valid
// pair (the last) so that everything they compute stays in bounds.
struct SampLane {
  bool live;
  int pair, j, first;   // first: the wave lane of the pair's lane 0
};
__device__ __forceinline__ SampLane samp_lane_of(int lgVL, int npairs) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  SampLane l;
  l.j = lane & ((1 << lgVL) - 1);
  l.first = lane - l.j;
  const int pair = wave * (64 >> lgVL) + (lane >> lgVL);
  l.live = pair < npairs;
  l.pair = l.live ? pair : npairs - 1;
  return l;
}

// Sampling state of one (pair, tap), as the lanes of the pair share it: fractional parts, the tap's factor (mask / attention
// weight), and per corner the byte offset of the head's channel row in the sampled tensor -- kSampOob for a corner that is
// not read, whose load then gives zeros, so no weight needs a validity factor.
struct SampTap {
  float lx, ly, m;
  int off[4];
};
// the state of a tap that is not on: nothing is read
__device__ __forceinline__ void samp_tap_clear(SampTap &t) {
  t.lx = t.ly = t.m = 0.f;
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) t.off[ci] = kSampOob;
}
// the state lane `src` of the wave built
__device__ __forceinline__ SampTap samp_tap_from(const SampTap &mine, int src) {
  SampTap t;
  t.lx = __shfl(mine.lx, src, 64);
  t.ly = __shfl(mine.ly, src, 64);
  t.m = __shfl(mine.m, src, 64);
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) t.off[ci] = __shfl(mine.off[ci], src, 64);
  return t;
}

// What a policy inherits whose factor IS the stored element (a mask, an attention weight): no statistics, the factor's
// gradient is the sum the coordinate backward holds, and the lists take the element as it stands.
struct SampPlainFactor {
  static constexpr bool kPairSum = false;
  template <int CT, class G, class C>
  static __device__ __forceinline__ void begin_pair(const G &, C &, const SampLane &, const void *) {}
  static __device__ __forceinline__ float factor_grad(float, float gsum, float) { return gsum; }
  template <class G> static __device__ __forceinline__ float list_factor(const G &, int, float raw) { return raw; }
};

// A policy with one more gradient, summed from the pixel-space location gradients of its taps (AfdaOp: the reference points
// its positions start from), declares `static constexpr bool kTapGrads = true` and has
//   Op::tap_grads<CT>(g, cx, ln, t0, my_tap, my_on, gx, gy, coord)   after the tap batch that begins at t0 of the coordinate
//                                  backward: gx, gy are the lane's sums of its tap my_tap times the tap's factor, before fx, fy
// For every other policy the hook does not exist: the kernel's call is discarded at compile time.
template <class Op, class = void> struct SampTapGrads { static constexpr bool value = false; };
template <class Op> struct SampTapGrads<Op, decltype((void)Op::kTapGrads)> { static constexpr bool value = Op::kTapGrads; };

// ---- forward ----
// Taps outside: the VL lanes of a pair build the sampling state of VL consecutive taps at once -- lane j the state of tap
// t0 + j, from one coordinate pair and one factor -- and then walk those taps together, each state broadcast from the lane that
// built it (a wave shuffle; VL = 1: the lane's own).  fp32 accumulators, one rounding at the store.  No workspace, no LDS, no
// atomics.
template <class Op, int DT, int CT>
__global__ __launch_bounds__(256) void samp_fwd_kernel(typename Op::Geom g, const void *__restrict__ sampled,
                                                        const void *__restrict__ coord, const void *__restrict__ factor,
                                                        void *__restrict__ output) {
  constexpr int NV = SampVec<DT>::NV;
  const SampLane ln = samp_lane_of(g.ln.lgVL, Op::npairs(g));
  typename Op::Ctx cx = Op::ctx(g, ln.pair);
  Op::template begin_pair<CT>(g, cx, ln, factor);
  const rsrc_t r_in = make_rsrc(sampled, Op::sampled_bytes(g));
  for (int rd = 0; rd < g.ln.rounds; ++rd) {   // one round unless a head has more than 64 vectors
    const int v = rd * g.ln.VL + ln.j;
    const bool on = ln.live && v < g.ln.V;
    const unsigned vbyte = on ? (unsigned)v * 16u : (unsigned)kSampOob;   // (a parked corner stays out of range with it)
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    for (int t0 = 0; t0 < g.K; t0 += g.ln.VL) {
      SampTap mine;
      float fx, fy;
      Op::template build_tap<CT>(g, cx, ln.pair, t0 + ln.j, ln.live && t0 + ln.j < g.K, coord, factor, mine, fx, fy);
      const int nt = min(g.ln.VL, g.K - t0);
      for (int jj = 0; jj < nt; ++jj) {
        const SampTap t = g.ln.VL > 1 ? samp_tap_from(mine, ln.first + jj) : mine;
        float4 raw[4];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) raw[ci] = buf_load4(r_in, (int)min((unsigned)t.off[ci] + vbyte, (unsigned)kSampOob), 0);
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          const float w = t.m * samp_corner_weight(t.lx, t.ly, ci);
          float x[NV];
          samp_unpack<DT>(raw[ci], x);
#pragma unroll
          for (int i = 0; i < NV; ++i) acc[i] = fmaf(w, x[i], acc[i]);
        }
      }
    }
    if (on) ((float4 *)output)[(int64_t)ln.pair * g.ln.V + v] = samp_pack<DT>(acc);
  }
}

// ---- the pair sum of a policy with kPairSum ----
// s_pair = sum over the taps of the pair of factor x (the weighted dot products of the tap), which is the dot product of the
// pair's grad_output row with its output row in fp32 -- taken from fp32 sums of this call, never from a stored (rounded)
// output.  A walk over the taps before the walk of samp_bwd_coord_kernel, with that kernel's loads and none of its
// derivative arithmetic: a lane adds up factor x its own partial dot products over every tap and round, and ONE butterfly
// over the pair's lanes ends it, so every lane of the pair returns the same bits.
template <class Op, int DT, int CT>
__device__ __forceinline__ float samp_pair_sum(const typename Op::Geom &g, const typename Op::Ctx &cx, const SampLane &ln,
                                               const rsrc_t &r_in, const rsrc_t &r_go, unsigned go_row,
                                               const float (&go0)[SampVec<DT>::NV], const void *coord, const void *factor) {
  constexpr int NV = SampVec<DT>::NV;
  float sum = 0.f;
  for (int t0 = 0; t0 < g.K; t0 += g.ln.VL) {
    SampTap mine;
    float fx, fy;
    Op::template build_tap<CT>(g, cx, ln.pair, t0 + ln.j, ln.live && t0 + ln.j < g.K, coord, factor, mine, fx, fy);
    const int nt = min(g.ln.VL, g.K - t0);
    for (int jj = 0; jj < nt; ++jj) {
      const SampTap t = g.ln.VL > 1 ? samp_tap_from(mine, ln.first + jj) : mine;
      float s_m = 0.f;
      for (int rd = 0; rd < g.ln.rounds; ++rd) {
        const int v = rd * g.ln.VL + ln.j;
        const bool on = ln.live && v < g.ln.V;
        const unsigned vbyte = on ? (unsigned)v * 16u : (unsigned)kSampOob;
        float go[NV];
        if (rd == 0) {
#pragma unroll
          for (int i = 0; i < NV; ++i) go[i] = go0[i];
        } else {
          samp_unpack<DT>(buf_load4(r_go, (int)min(go_row + vbyte, (unsigned)kSampOob), 0), go);
        }
        float4 raw[4];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) raw[ci] = buf_load4(r_in, (int)min((unsigned)t.off[ci] + vbyte, (unsigned)kSampOob), 0);
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          float x[NV];
          samp_unpack<DT>(raw[ci], x);
          float dot = 0.f;
#pragma unroll
          for (int i = 0; i < NV; ++i) dot = fmaf(go[i], x[i], dot);
          s_m = fmaf(samp_corner_weight(t.lx, t.ly, ci), dot, s_m);
        }
      }
      sum = fmaf(t.m, s_m, sum);
    }
  }
  for (int d = g.ln.VL >> 1; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
  return sum;
}

// ---- coordinate gradients, without atomics ----
// The lane mapping and the tap walk of the forward.  Per (pair, tap) a lane takes the dot products of its grad_output vector
// with the four corner vectors in-lane, weighs them three ways -- the bilinear weights (the factor's gradient), their
// derivatives along x and along y (the coordinates' gradient) -- and the three sums over the pair's lanes are taken by an xor
// butterfly inside the wave: a fixed order, every lane ends with the same bits.  Lane j keeps the sums of tap t0 + j, so after
// VL taps each lane stores one factor gradient and one (x, y) pair -- times the factor and the operator's fx, fy -- next to
// its neighbours', in the coordinate type and in the caller's write mode.  What is stored as the factor gradient is
// Op::factor_grad(factor, sum, s_pair): the sum itself for a plain factor, and for a policy with kPairSum a function of the
// pair sum as well, which samp_pair_sum takes in a walk of its own before this one.
// On `__restrict__` now that coord / factor, and grad_coord / grad_factor, may each be ONE tensor: the qualifier promises that
// an OBJECT modified during the call is reached through one of the qualified pointers only -- it speaks of the elements
// accessed, not of the allocations.  coord and factor are only read, so for them it promises nothing aliasing could break.
// Of the gradient tensor every element is reached through exactly one pointer: an (x, y) element (Op::coord_index) through
// grad_coord, a factor element (Op::factor_index) through grad_factor, row padding (Op::finish_pair) through grad_coord; the
// two index sets of a policy are disjoint, accumulate mode reads an element through the pointer that then writes it, and
// samp_st stores exactly the element's 2 or 4 bytes.  So the promise holds and the qualifiers stay.
template <class Op, int DT, int CT>
__global__ __launch_bounds__(256) void samp_bwd_coord_kernel(typename Op::Geom g, const void *__restrict__ sampled,
                                                              const void *__restrict__ coord, const void *__restrict__ factor,
                                                              const void *__restrict__ grad_output, void *__restrict__ grad_coord,
                                                              void *__restrict__ grad_factor) {
  constexpr int NV = SampVec<DT>::NV;
  const SampLane ln = samp_lane_of(g.ln.lgVL, Op::npairs(g));
  typename Op::Ctx cx = Op::ctx(g, ln.pair);
  Op::template begin_pair<CT>(g, cx, ln, factor);
  const rsrc_t r_in = make_rsrc(sampled, Op::sampled_bytes(g));
  const rsrc_t r_go = make_rsrc(grad_output, (size_t)Op::npairs(g) * g.D * g.ln.esz);
  const unsigned go_row = (unsigned)ln.pair * (unsigned)g.ln.V * 16u;   // the pair's channel row of grad_output
  float go0[NV];   // the first round's vector (the only one unless a head has more than 64 vectors)
  samp_unpack<DT>(buf_load4(r_go, ln.live && ln.j < g.ln.V ? (int)(go_row + (unsigned)ln.j * 16u) : kSampOob, 0), go0);
  float s_pair = 0.f;
  if (Op::kPairSum) s_pair = samp_pair_sum<Op, DT, CT>(g, cx, ln, r_in, r_go, go_row, go0, coord, factor);
  for (int t0 = 0; t0 < g.K; t0 += g.ln.VL) {
    const int my_tap = t0 + ln.j;
    const bool my_on = ln.live && my_tap < g.K;
    SampTap mine;
    float fx, fy;   // of my_tap
    Op::template build_tap<CT>(g, cx, ln.pair, my_tap, my_on, coord, factor, mine, fx, fy);
    float r_m = 0.f, r_x = 0.f, r_y = 0.f;   // the sums of my_tap
    float h_x = 0.f, h_y = 0.f;              // (kTapGrads) its pixel-space location gradients
    const int nt = min(g.ln.VL, g.K - t0);
    for (int jj = 0; jj < nt; ++jj) {
      const SampTap t = g.ln.VL > 1 ? samp_tap_from(mine, ln.first + jj) : mine;
      float s_m = 0.f, s_x = 0.f, s_y = 0.f;
      for (int rd = 0; rd < g.ln.rounds; ++rd) {
        const int v = rd * g.ln.VL + ln.j;
        const bool on = ln.live && v < g.ln.V;
        const unsigned vbyte = on ? (unsigned)v * 16u : (unsigned)kSampOob;
        float go[NV];
        if (rd == 0) {
#pragma unroll
          for (int i = 0; i < NV; ++i) go[i] = go0[i];
        } else {
          samp_unpack<DT>(buf_load4(r_go, (int)min(go_row + vbyte, (unsigned)kSampOob), 0), go);
        }
        float4 raw[4];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) raw[ci] = buf_load4(r_in, (int)min((unsigned)t.off[ci] + vbyte, (unsigned)kSampOob), 0);
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          float x[NV];
          samp_unpack<DT>(raw[ci], x);
          float dot = 0.f;
#pragma unroll
          for (int i = 0; i < NV; ++i) dot = fmaf(go[i], x[i], dot);
          s_m = fmaf(samp_corner_weight(t.lx, t.ly, ci), dot, s_m);
          s_x = fmaf(samp_corner_dx(t.ly, ci), dot, s_x);
          s_y = fmaf(samp_corner_dy(t.lx, ci), dot, s_y);
        }
      }
      for (int d = g.ln.VL >> 1; d >= 1; d >>= 1) {
        s_m += __shfl_xor(s_m, d, 64);
        s_x += __shfl_xor(s_x, d, 64);
        s_y += __shfl_xor(s_y, d, 64);
      }
      if (jj == ln.j) {   // t is `mine`
        r_m = Op::factor_grad(t.m, s_m, s_pair);
        r_x = s_x * (t.m * fx);
        r_y = s_y * (t.m * fy);
        if constexpr (SampTapGrads<Op>::value) {
          h_x = s_x * t.m;
          h_y = s_y * t.m;
        }
      }
    }
    if (my_on) {
      samp_st<CT>(grad_factor, Op::factor_index(g, cx, ln.pair, my_tap), r_m, g.acc != 0);
      samp_st<CT>(grad_coord, Op::coord_index(g, cx, ln.pair, my_tap, 0), r_x, g.acc != 0);
      samp_st<CT>(grad_coord, Op::coord_index(g, cx, ln.pair, my_tap, 1), r_y, g.acc != 0);
    }
    if constexpr (SampTapGrads<Op>::value) Op::template tap_grads<CT>(g, cx, ln, t0, my_tap, my_on, h_x, h_y, coord);
  }
  Op::template finish_pair<CT>(g, cx, ln, grad_coord);
}

// ---- scatter lists of the sampled tensor's gradient (scatter_lists_build, mdconv_common.hpp) ----
// Per (segment = image x head, target row) one 16-byte entry per corner the forward read -- {sample = tap * rows_out + q,
// corner weight x factor, tap, q}; a sample reaches a row through one corner, so word 0 is unique inside a list.
struct SampItem {
  SampSample s;
  int H, W;       // the extents `s` lies in
  int seg, row0;  // the segment, and the row of pixel (0, 0) inside it
  int tap, q, rows_out;   // q: the sample's row of grad_output inside its image, of rows_out
};
// thread = sample, in the order of `coord` and `factor` (which may be one tensor; both are only read), so both are read
// coalesced.  FILL false: count the entries per target; true: after the scan, take slots from the back of each list (the
// counters run down to zero) and write the entries.
template <class Op, int CT, bool FILL>
__global__ __launch_bounds__(256) void samp_list_kernel(typename Op::Geom g, const void *__restrict__ coord,
                                                         const void *__restrict__ factor, int *__restrict__ cnt,
                                                         const int *__restrict__ rowptr, int4 *__restrict__ entries,
                                                         int64_t seg_stride) {
  const int total = Op::npairs(g) * g.K;   // elements of `factor`: below 2^30
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const float f = FILL ? Op::list_factor(g, id, samp_ld<CT>(factor, Op::list_factor_index(g, id))) : 1.f;
  SampItem it;
  Op::template list_item<CT>(g, id, coord, it);
  const int rows = Op::list_rows(g);
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    if (!samp_corner_read(it.s, ci, it.H, it.W)) continue;
    const int row = it.row0 + samp_corner_pixel(it.s, ci, it.W);
    int *c = cnt + (int64_t)it.seg * rows + row;
    if (!FILL) {
      atomicAdd(c, 1);
    } else {
      const int slot = rowptr[(int64_t)it.seg * (rows + 1) + row] + atomicSub(c, 1) - 1;
      entries[(int64_t)it.seg * seg_stride + slot] =
          make_int4(it.tap * it.rows_out + it.q, __float_as_int(samp_corner_weight(it.s.lx, it.s.ly, ci) * f), it.tap, it.q);
    }
  }
}

// ---- launches of the three kernels for one (Op, DT, CT) ----
template <class Op, int DT, int CT>
void samp_fwd_launch(const typename Op::Geom &g, const void *sampled, const void *coord, const void *factor, void *output,
                     hipStream_t stream) {
  hipLaunchKernelGGL((samp_fwd_kernel<Op, DT, CT>), dim3(samp_grid(g.ln.lgVL, Op::npairs(g))), dim3(256), 0, stream, g, sampled,
                     coord, factor, output);
}
template <class Op, int DT, int CT>
void samp_bwd_coord_launch(const typename Op::Geom &g, const void *sampled, const void *coord, const void *factor,
                           const void *grad_output, void *grad_coord, void *grad_factor, hipStream_t stream) {
  hipLaunchKernelGGL((samp_bwd_coord_kernel<Op, DT, CT>), dim3(samp_grid(g.ln.lgVL, Op::npairs(g))), dim3(256), 0, stream, g,
                     sampled, coord, factor, grad_output, grad_coord, grad_factor);
}
template <class Op, int CT>
void samp_list_launch(const typename Op::Geom &g, bool fill, const void *coord, const void *factor, int *cnt, const int *rowptr,
                      void *entries, int64_t seg_stride, hipStream_t stream) {
  const dim3 grid((unsigned)(((int64_t)Op::npairs(g) * g.K + 255) / 256));
  if (fill)
    hipLaunchKernelGGL((samp_list_kernel<Op, CT, true>), grid, dim3(256), 0, stream, g, coord, factor, cnt, rowptr, (int4 *)entries,
                       seg_stride);
  else
    hipLaunchKernelGGL((samp_list_kernel<Op, CT, false>), grid, dim3(256), 0, stream, g, coord, factor, cnt, rowptr,
                       (int4 *)entries, seg_stride);
}
#endif  // __HIPCC__

}  // namespace mdconv
