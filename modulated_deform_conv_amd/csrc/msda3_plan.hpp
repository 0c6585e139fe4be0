// msda3_plan.hpp -- 3-D multi-scale deformable attention (include/mdconv.h "3-D multi-scale deformable attention"):
// deformable attention over volumes on channels-last tensors, fp32 / fp16 / bf16 values with coordinates in the same type or
// in fp32.  A kernel family of its own (msda3_fwd.hip, msda3_bwd.hip, msda3_list.hip), NOT a policy of the sampling core: a
// tap has eight corners and three fractions, the coordinate backward four sums, and widening SampTap or the core's butterfly
// would cost registers in every existing instance.  What the family takes from the core as it
// stands: the lane mapping (SampLanes, samp_lanes, samp_grid, samp_lane_of), the 16-byte vector helpers (samp_ld / samp_st,
// samp_pack / samp_unpack, kSampOob, the raw buffer loads), the list builder (scatter_lists_take / scatter_lists_build /
// csr_sort_rows) and the channels-last gather (samp_gather_launch), which walks rows and entries and never knew a dimension.
// pair = (n * Lq + q) * M + m, tap = l * P + p, so pair * K + tap is the element index of attention_weights and three times
// that the element of a sample's x in sampling_locations.  A call is planned ONCE: msda3_plan() decides whether the family
// takes it and lays its workspace out, the byte count reported to the caller is the plan's `total`, and msda3_forward /
// msda3_backward take the plan.
#pragma once
#include "samp_core.hpp"

namespace mdconv {

// Device-side geometry (POD, passed by value as a kernel argument).  The level table is read with constant indices only
// (msda3_level: an unrolled select chain), so it stays in scalar registers: a per-lane dynamic index would go through scratch.
struct Msda3Geom {
  int N, M, D, C, Lq, L, P, K;   // C = M * D, K = L * P
  int S;                         // value rows per image
  int npairs;                    // N * Lq * M
  SampLanes ln;
  int acc;                       // backward: 1 = add to the caller's gradient buffers, 0 = overwrite
  int lvT[MDCONV_MSDA_MAX_LEVELS], lvH[MDCONV_MSDA_MAX_LEVELS], lvW[MDCONV_MSDA_MAX_LEVELS];   // extents
  int lvS[MDCONV_MSDA_MAX_LEVELS];                                                             // start row
};

struct Msda3Tensors {
  const void *value, *loc, *attn, *grad_output;
  void *output, *grad_value, *grad_loc, *grad_attn;
};

struct Msda3Plan {
  Msda3Geom g;
  int dtype, coord_dtype;   // MDCONV_F32 / MDCONV_F16 / MDCONV_BF16
  bool backward;
  bool det;                 // MDCONV_FLAG_DETERMINISTIC: the lists are sorted before the gather
  bool skip_value;          // MDCONV_FLAG_NO_GRAD_INPUT: no lists, no sort, no gather, no workspace
  ScatterLists lists;       // grad_value: per (image, head) a segment of S lists, K * Lq * 8 entries
  size_t total;             // workspace bytes
};

// false: outside the shape rule; *why names the rule it breaks.  The descriptor has passed validation (the operator's *_host.hip).
bool msda3_plan(const mdconv_msda3d_desc *d, bool backward, Msda3Plan *p, const char **why);
int msda3_forward(const Msda3Plan &p, const Msda3Tensors &t, hipStream_t stream);
int msda3_backward(const Msda3Plan &p, const Msda3Tensors &t, void *ws, hipStream_t stream);

// the kernels (msda3_fwd.hip, msda3_bwd.hip, msda3_list.hip), by the plan's (value type, coordinate type)
int msda3_fwd_launch(const Msda3Plan &p, const Msda3Tensors &t, hipStream_t stream);
int msda3_bwd_coord_launch(const Msda3Plan &p, const Msda3Tensors &t, hipStream_t stream);
void msda3_list_launch(const Msda3Plan &p, const Msda3Tensors &t, bool fill, int *cnt, const int *rowptr, void *entries,
                       hipStream_t stream);


#ifdef __HIPCC__
// ---- the sampling arithmetic, once for the three kernels, so they agree to the bit on every sample ----
// The sample at (z, y, x) in the voxel coordinates of a level of T x H x W has the neighbours (z0 + cz, y0 + cy, x0 + cx),
// corner ci = 4 * cz + 2 * cy + cx, with the trilinear weights (cz ? lz : 1 - lz) * (cy ? ly : 1 - ly) * (cx ? lx : 1 - lx).
// A corner is READ iff the sample passes the gate -1 < coordinate < size on all three axes and the corner lies inside the
// level: bit ci of `read`.  Every other corner contributes nothing to any result and is never loaded.
struct Msda3Sample {
  float lx, ly, lz;   // fractional parts
  int x0, y0, z0;     // low neighbour (may be -1)
  unsigned read;      // bit ci: corner ci is read; 0 for a sample the gate leaves out
};
__device__ __forceinline__ void msda3_sample(float z, float y, float x, int T, int H, int W, Msda3Sample &s) {
  const bool inside = z > -1.f && y > -1.f && x > -1.f && z < (float)T && y < (float)H && x < (float)W;
  // clamp before the int conversion so wild locations (and NaN, which fails the gate) cannot overflow
  const float zc = inside ? z : 0.f, yc = inside ? y : 0.f, xc = inside ? x : 0.f;
  const float fz = floorf(zc), fy = floorf(yc), fx = floorf(xc);
  s.z0 = (int)fz; s.y0 = (int)fy; s.x0 = (int)fx;
  s.lz = zc - fz; s.ly = yc - fy; s.lx = xc - fx;
  // per axis: bit 0 = the low neighbour is inside, bit 1 = the high one
  const unsigned ax = (s.x0 >= 0 ? 1u : 0u) | (s.x0 + 1 < W ? 2u : 0u);
  const unsigned ay = (s.y0 >= 0 ? 1u : 0u) | (s.y0 + 1 < H ? 2u : 0u);
  const unsigned az = (s.z0 >= 0 ? 1u : 0u) | (s.z0 + 1 < T ? 2u : 0u);
  unsigned read = 0;
#pragma unroll
  for (int ci = 0; ci < 8; ++ci)
    if (((az >> (ci >> 2)) & (ay >> ((ci >> 1) & 1)) & (ax >> (ci & 1)) & 1u) != 0) read |= 1u << ci;
  s.read = inside ? read : 0u;
}
// rows from the row of (z0, y0, x0) to corner ci's
__device__ __forceinline__ int msda3_corner_step(int ci, int H, int W) { return ((ci >> 2) * H + ((ci >> 1) & 1)) * W + (ci & 1); }
// the trilinear weight of corner ci and its derivatives along x, y and z
__device__ __forceinline__ float msda3_w1(float l, int hi) { return hi ? l : 1.f - l; }
__device__ __forceinline__ float msda3_sign(int hi) { return hi ? 1.f : -1.f; }
__device__ __forceinline__ float msda3_corner_weight(float lx, float ly, float lz, int ci) {
  return msda3_w1(lz, ci >> 2) * msda3_w1(ly, (ci >> 1) & 1) * msda3_w1(lx, ci & 1);
}
__device__ __forceinline__ float msda3_corner_dx(float ly, float lz, int ci) {
  return msda3_w1(lz, ci >> 2) * msda3_w1(ly, (ci >> 1) & 1) * msda3_sign(ci & 1);
}
__device__ __forceinline__ float msda3_corner_dy(float lx, float lz, int ci) {
  return msda3_w1(lz, ci >> 2) * msda3_w1(lx, ci & 1) * msda3_sign((ci >> 1) & 1);
}
__device__ __forceinline__ float msda3_corner_dz(float lx, float ly, int ci) {
  return msda3_w1(ly, (ci >> 1) & 1) * msda3_w1(lx, ci & 1) * msda3_sign(ci >> 2);
}

// extents and start row of level `l` (0 <= l < L <= 8): constant indices into the kernel argument
__device__ __forceinline__ void msda3_level(const Msda3Geom &g, int l, int &T, int &H, int &W, int &start) {
  T = g.lvT[0]; H = g.lvH[0]; W = g.lvW[0]; start = g.lvS[0];
#pragma unroll
  for (int i = 1; i < MDCONV_MSDA_MAX_LEVELS; ++i)
    if (l == i) { T = g.lvT[i]; H = g.lvH[i]; W = g.lvW[i]; start = g.lvS[i]; }
}
// the sample whose x is element ec of sampling_locations (y and z follow), in the voxel coordinates of its level
template <int CT>
__device__ __forceinline__ void msda3_position(const void *loc, int ec, int T, int H, int W, Msda3Sample &s) {
  const float x = samp_ld<CT>(loc, ec) * (float)W - 0.5f;
  const float y = samp_ld<CT>(loc, ec + 1) * (float)H - 0.5f;
  const float z = samp_ld<CT>(loc, ec + 2) * (float)T - 0.5f;
  msda3_sample(z, y, x, T, H, W, s);
}

// ---- the state of one (pair, tap), as the lanes of the pair share it ----
// Eight words instead of the twelve of "eight offsets, three fractions, the factor": the byte offset of the head's channel
// row at the LOW neighbour (z0, y0, x0) -- formed in wrapping unsigned arithmetic, it is meaningful only together with a
// corner that is read --, the mask of the corners read, and the byte strides of one step along y and along z in the tap's
// level (the step along x is the row, the same on every level).  A corner's offset is base + steps where its bit is set and
// kSampOob where not: a parked corner's load gives zeros, so no weight needs a validity factor.
struct Msda3Tap {
  float lx, ly, lz, m;
  unsigned base, read, sy, sz;
};
__device__ __forceinline__ void msda3_tap_clear(Msda3Tap &t) {
  t.lx = t.ly = t.lz = t.m = 0.f;
  t.base = t.read = t.sy = t.sz = 0u;
}
// the state lane `src` of the wave built
__device__ __forceinline__ Msda3Tap msda3_tap_from(const Msda3Tap &mine, int src) {
  Msda3Tap t;
  t.lx = __shfl(mine.lx, src, 64);
  t.ly = __shfl(mine.ly, src, 64);
  t.lz = __shfl(mine.lz, src, 64);
  t.m = __shfl(mine.m, src, 64);
  t.base = __shfl(mine.base, src, 64);
  t.read = __shfl(mine.read, src, 64);
  t.sy = __shfl(mine.sy, src, 64);
  t.sz = __shfl(mine.sz, src, 64);
  return t;
}
// the byte offset of corner ci of tap t (row_bytes = C * esz), kSampOob if it is not read
__device__ __forceinline__ unsigned msda3_corner_off(const Msda3Tap &t, int ci, unsigned row_bytes) {
  const unsigned off = t.base + ((ci & 1) ? row_bytes : 0u) + (((ci >> 1) & 1) ? t.sy : 0u) + ((ci >> 2) ? t.sz : 0u);
  return ((t.read >> ci) & 1u) ? off : (unsigned)kSampOob;
}
// the byte offset of (image n, value row 0, head m) in `value`, for pair = (n * Lq + q) * M + m
__device__ __forceinline__ unsigned msda3_pair_byte(const Msda3Geom &g, int pair) {
  const int nq = pair / g.M, m = pair - nq * g.M;
  const int n = nq / g.Lq;
  return (unsigned)((n * g.S * g.C + m * g.D) * g.ln.esz);
}
// The state of tap `tap` of `pair` (which names its level), and the factors fx, fy, fz of the three coordinate gradients:
// the extents W, H, T of the tap's level (the positions are normalised).  `on` false: a tap that is not there reads nothing.
template <int CT>
__device__ __forceinline__ void msda3_build_tap(const Msda3Geom &g, unsigned pair_byte, int pair, int tap, bool on,
                                                const void *loc, const void *attn, Msda3Tap &t, float &fx, float &fy,
                                                float &fz) {
  msda3_tap_clear(t);
  fx = fy = fz = 1.f;
  if (!on) return;
  const int e = pair * g.K + tap;
  int T, H, W, start;
  msda3_level(g, tap / g.P, T, H, W, start);
  fx = (float)W; fy = (float)H; fz = (float)T;
  Msda3Sample s;
  msda3_position<CT>(loc, 3 * e, T, H, W, s);
  const unsigned row_bytes = (unsigned)(g.C * g.ln.esz);
  t.lx = s.lx; t.ly = s.ly; t.lz = s.lz;
  t.m = samp_ld<CT>(attn, e);
  t.read = s.read;
  t.sy = (unsigned)W * row_bytes;
  t.sz = (unsigned)(H * W) * row_bytes;
  t.base = pair_byte + (unsigned)(start + (s.z0 * H + s.y0) * W + s.x0) * row_bytes;
}
#endif  // __HIPCC__

}  // namespace mdconv
