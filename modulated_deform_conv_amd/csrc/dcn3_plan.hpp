// dcn3_plan.hpp -- the DCNv3 core operator (include/mdconv.h "DCNv3 core operator"): grouped deformable sampling on
// channels-last tensors, fp32 / fp16 / bf16, with a constant group weight -- no contraction at all, so the family is VALU
// kernels of its own (dcn3_fwd.hip, dcn3_bwd.hip, dcn3_gi.hip) like the depthwise family (dw_plan.hpp), whose pattern this
// follows: a call is planned ONCE, dcn3_plan() decides whether the family takes it and lays its workspace out, the byte
// count reported to the caller is the plan's `total`, and dcn3_forward / dcn3_backward take the plan.
//
// Lane mapping of every kernel: a lane owns one 16-byte channel vector (4 floats / 8 halves) of one (pixel, group) PAIR;
// the VL lanes of a pair (VL = the vectors per group V rounded up to a power of two, at most 64) are adjacent and the
// pairs of a pixel follow each other, so a wave's stores and each of its corner loads are contiguous 16-byte pieces.
// Groups of more than 64 vectors (D > 256 fp32) take `rounds` > 1 passes over the vectors.
#pragma once
#include "host_util.hpp"
#include "mfma_kernels.hpp"   // zero_bytes
#include "mfma_tile.hpp"      // raw buffer loads

namespace mdconv {

// Device-side geometry (POD, passed by value as a kernel argument).
struct Dcn3Geom {
  int B, G, D, C, K;    // C = G * D, K = kh * kw
  int H, W, Ho, Wo, kh, kw;
  int sh, sw, ph, pw, dh, dw;
  int ch, cw;           // (dil * (k - 1)) >> 1 per axis
  int S_i, S_o, N;      // H * W, Ho * Wo, B * S_o
  int V, VL, lgVL, rounds;
  int esz;              // bytes per element
  float scale;          // offset_scale
  int acc;              // backward: 1 = add to the caller's gradient buffers, 0 = overwrite
};

struct Dcn3Tensors {
  const void *input, *offset, *mask, *grad_output;
  void *output, *grad_input, *grad_offset, *grad_mask;
};

struct Dcn3Plan {
  Dcn3Geom g;
  int dtype;            // MDCONV_F32 / MDCONV_F16 / MDCONV_BF16
  bool backward;
  bool det;             // MDCONV_FLAG_DETERMINISTIC: the lists are sorted before the gather
  bool skip_input;      // MDCONV_FLAG_NO_GRAD_INPUT: no lists, no sort, no gather, no workspace
  // grad_input (dcn3_gi.hip): scatter lists per (image, group, input pixel), one entry per corner the forward read
  int nseg;             // B * G
  int64_t seg_stride;   // entries per segment: K * S_o * 4
  size_t off_cnt, off_rowptr, off_entries, off_sort;
  size_t total;         // workspace bytes
};

// false: outside the shape rule; *why names the rule it breaks.  The descriptor has passed validation (mdconv_api.hip).
bool dcn3_plan(const mdconv_dcnv3_desc *d, bool backward, Dcn3Plan *p, const char **why);
int dcn3_forward(const Dcn3Plan &p, const Dcn3Tensors &t, hipStream_t stream);
int dcn3_backward(const Dcn3Plan &p, const Dcn3Tensors &t, void *ws, hipStream_t stream);

// ---- kernels' launchers (one translation unit each) ----
int dcn3_fwd_launch(const Dcn3Plan &p, const Dcn3Tensors &t, hipStream_t stream);
int dcn3_bwd_coord_launch(const Dcn3Plan &p, const Dcn3Tensors &t, hipStream_t stream);
int dcn3_lists_launch(const Dcn3Plan &p, const Dcn3Tensors &t, int *cnt, int *rowptr, void *entries, void *sort_scratch,
                      hipStream_t stream);
int dcn3_gather_launch(const Dcn3Plan &p, const Dcn3Tensors &t, const int *rowptr, const void *entries, hipStream_t stream);

// workgroups of 256 lanes that cover `npairs` (pixel, group) pairs
inline int dcn3_grid(const Dcn3Geom &g, int64_t npairs) {
  const int64_t per_block = 4 * (64 >> g.lgVL);
  return (int)((npairs + per_block - 1) / per_block);
}

// ---- device side, shared by the three kernel files ----------------------------------------------
#ifdef __HIPCC__
constexpr int kDcn3Oob = 0x7ffffff0;   // out-of-range buffer offset: loads give 0 (every tensor is below 2^31 bytes)

template <int DT> struct Dcn3Vec { static constexpr int NV = DT == MDCONV_F32 ? 4 : 8; };

template <int DT> __device__ __forceinline__ float dcn3_ld(const void *p, int i) {
  if (DT == MDCONV_F32) return ((const float *)p)[i];
  if (DT == MDCONV_F16) return __half2float(((const __half *)p)[i]);
  return bf16_bits_to_float(((const unsigned short *)p)[i]);
}
// dst[i] = v, or dst[i] += v in the tensor's type (`acc`)
template <int DT> __device__ __forceinline__ void dcn3_st(void *p, int i, float v, bool acc) {
  if (acc) v += dcn3_ld<DT>(p, i);
  if (DT == MDCONV_F32) ((float *)p)[i] = v;
  else if (DT == MDCONV_F16) ((__half *)p)[i] = __float2half(v);
  else ((unsigned short *)p)[i] = float_to_bf16_bits(v);
}
template <int DT> __device__ __forceinline__ float dcn3_widen16(unsigned h) {
  return DT == MDCONV_F16 ? __half2float(__ushort_as_half((unsigned short)h)) : bf16_bits_to_float((unsigned short)h);
}
template <int DT> __device__ __forceinline__ unsigned dcn3_narrow16(float v) {
  return DT == MDCONV_F16 ? (unsigned)__half_as_ushort(__float2half(v)) : (unsigned)float_to_bf16_bits(v);
}
// the 16 bytes of a channel vector <-> its 4 / 8 values
template <int DT> __device__ __forceinline__ void dcn3_unpack(const float4 &raw, float (&f)[Dcn3Vec<DT>::NV]) {
  if (DT == MDCONV_F32) {
    f[0] = raw.x; f[1] = raw.y; f[2] = raw.z; f[3] = raw.w;
  } else {
    const unsigned u[4] = {__float_as_uint(raw.x), __float_as_uint(raw.y), __float_as_uint(raw.z), __float_as_uint(raw.w)};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[(2 * i) % Dcn3Vec<DT>::NV] = dcn3_widen16<DT>(u[i] & 0xffffu);
      f[(2 * i + 1) % Dcn3Vec<DT>::NV] = dcn3_widen16<DT>(u[i] >> 16);
    }
  }
}
template <int DT> __device__ __forceinline__ float4 dcn3_pack(const float (&f)[Dcn3Vec<DT>::NV]) {
  if (DT == MDCONV_F32) return make_float4(f[0], f[1], f[2], f[3]);
  unsigned u[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    u[i] = dcn3_narrow16<DT>(f[(2 * i) % Dcn3Vec<DT>::NV]) | (dcn3_narrow16<DT>(f[(2 * i + 1) % Dcn3Vec<DT>::NV]) << 16);
  return make_float4(__uint_as_float(u[0]), __uint_as_float(u[1]), __uint_as_float(u[2]), __uint_as_float(u[3]));
}

// The lane's place: pair = pixel * G + group over `npairs` pairs, j = its lane inside the pair.  Lanes beyond the last
// pair are not live; they keep a valid pair (the last) so that everything they compute stays in bounds.
struct Dcn3Lane {
  bool live;
  int pair, j, first;   // first: the wave lane of the pair's lane 0
};
__device__ __forceinline__ Dcn3Lane dcn3_lane_of(int lgVL, int npairs) {   // (msda_plan.hpp shares the mapping)
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  Dcn3Lane l;
  l.j = lane & ((1 << lgVL) - 1);
  l.first = lane - l.j;
  const int pair = wave * (64 >> lgVL) + (lane >> lgVL);
  l.live = pair < npairs;
  l.pair = l.live ? pair : npairs - 1;
  return l;
}
__device__ __forceinline__ Dcn3Lane dcn3_lane(const Dcn3Geom &g, int npairs) { return dcn3_lane_of(g.lgVL, npairs); }

// Sampling state of one (output pixel, group, tap), as the lanes of the pair share it: fractional parts, mask, and per
// corner the byte offset of the group's channel row in `input` -- kDcn3Oob for a corner that is not read, whose load then
// gives zeros, so no weight needs a validity factor.
struct Dcn3Tap {
  float lx, ly, m;
  int off[4];
};
struct Dcn3Pix {   // what the taps of one (output pixel, group) have in common
  int img_pix;     // b * S_i
  int grp_byte;    // group * D * esz
  float base_h, base_w;
};
__device__ __forceinline__ Dcn3Pix dcn3_pix(const Dcn3Geom &g, int pair) {
  const int n = pair / g.G, grp = pair - n * g.G;
  const int b = n / g.S_o, pix = n - b * g.S_o;
  const int ho = pix / g.Wo, wo = pix - ho * g.Wo;
  Dcn3Pix p;
  p.img_pix = b * g.S_i;
  p.grp_byte = grp * g.D * g.esz;
  p.base_h = (float)(ho * g.sh - g.ph + g.ch);
  p.base_w = (float)(wo * g.sw - g.pw + g.cw);
  return p;
}
// the position of tap = i * kh + j (i: the kernel's width index) from the offsets (x, y) of the tap
__device__ __forceinline__ void dcn3_position(const Dcn3Geom &g, const Dcn3Pix &px, int tap, float off_x, float off_y,
                                              Dcn3Sample &s) {
  const int i = tap / g.kh, j = tap - i * g.kh;
  const float loc_w = px.base_w + ((float)(i * g.dw - g.cw) + off_x) * g.scale;
  const float loc_h = px.base_h + ((float)(j * g.dh - g.ch) + off_y) * g.scale;
  dcn3_sample(loc_h, loc_w, g.H, g.W, s);
}
template <int DT>
__device__ __forceinline__ void dcn3_build_tap(const Dcn3Geom &g, const Dcn3Pix &px, int pair, int tap, bool on,
                                               const void *offset, const void *mask, Dcn3Tap &t) {
  t.lx = t.ly = t.m = 0.f;
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) t.off[ci] = kDcn3Oob;
  if (!on) return;
  const int e = pair * g.K + tap;
  Dcn3Sample s;
  dcn3_position(g, px, tap, dcn3_ld<DT>(offset, 2 * e), dcn3_ld<DT>(offset, 2 * e + 1), s);
  t.lx = s.lx;
  t.ly = s.ly;
  t.m = dcn3_ld<DT>(mask, e);
#pragma unroll
  for (int ci = 0; ci < 4; ++ci)
    if (dcn3_corner_read(s, ci, g.H, g.W)) t.off[ci] = (px.img_pix + dcn3_corner_pixel(s, ci, g.W)) * g.C * g.esz + px.grp_byte;
}
// the state lane `src` of the wave built
__device__ __forceinline__ Dcn3Tap dcn3_tap_from(const Dcn3Tap &mine, int src) {
  Dcn3Tap t;
  t.lx = __shfl(mine.lx, src, 64);
  t.ly = __shfl(mine.ly, src, 64);
  t.m = __shfl(mine.m, src, 64);
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) t.off[ci] = __shfl(mine.off[ci], src, 64);
  return t;
}
#endif  // __HIPCC__

}  // namespace mdconv
