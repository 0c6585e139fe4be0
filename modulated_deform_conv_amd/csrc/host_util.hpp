// host_util.hpp -- host-side helpers shared by the kernel families' planners (mfma_kernels.hip, mfma_plans.hip,
// f32_copies.hip, hp_host.hip): workspace layout, batch chunks, and the layout / conversion kernels of util_kernels.hip.
#pragma once
#include <stdlib.h>

#include "mdconv_common.hpp"

namespace mdconv {

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace layout: 256-byte aligned slots handed out front to back
struct Bump {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t at = off;
    off += align_up(bytes);
    return at;
  }
};

// the slots of scatter lists (ScatterLists, mdconv_common.hpp); the sort scratch only in deterministic mode
inline ScatterLists scatter_lists_take(Bump &ws, int nseg, int rows, int64_t seg_stride, bool det) {
  ScatterLists L = {nseg, rows, seg_stride};
  L.off_cnt = ws.take((size_t)nseg * rows * 4);
  L.off_rowptr = ws.take((size_t)nseg * (rows + 1) * 4);
  L.off_entries = ws.take((size_t)nseg * (size_t)seg_stride * 16);
  L.off_sort = ws.take(det ? csr_sort_scratch_bytes(1, seg_stride, nseg) : 0);
  return L;
}

// the geometry of `bc` images of a call
inline Geom chunk_geom(const Geom &g, int bc) {
  Geom c = g;
  c.B = bc;
  c.N = bc * g.S_o;
  return c;
}

// Most bytes a per-chunk tensor may have: the family's own ceiling (32-bit buffer offsets), which
// MDCONV_CHUNK_LIMIT_BYTES (read once) lowers so tests can force multi-chunk execution
inline size_t chunk_limit(size_t ceiling) {
  static const long long env = getenv("MDCONV_CHUNK_LIMIT_BYTES") ? atoll(getenv("MDCONV_CHUNK_LIMIT_BYTES")) : 0;
  return env > 0 && (size_t)env < ceiling ? (size_t)env : ceiling;
}

// ---- util_kernels.hip: plain kernels instead of memset / memcpy nodes (those made HIP graph replay fault) ----
// fp16 / bf16 <-> fp32 (`accum`: add to the 16-bit destination)
int widen(int dtype, const void *src, float *dst, int64_t n, hipStream_t s);
int narrow(int dtype, const float *src, void *dst, int64_t n, bool accum, hipStream_t s);
// the fp32-destination twin of narrow (MDCONV_WGRAD_F32): dst = src, or dst += src with `accum` -- nothing is rounded
int store_f32(const float *src, float *dst, int64_t n, bool accum, hipStream_t s);
// grad_weight / grad_bias of a 16-bit call on their way out of an fp32 buffer: rounded once, or kept fp32 (t.wgrad32)
inline int narrow_wgrad(int dtype, const Tensors &t, const float *src, void *dst, int64_t n, bool accum, hipStream_t s) {
  return t.wgrad32 ? store_f32(src, (float *)dst, n, accum, s) : narrow(dtype, src, dst, n, accum, s);
}
// strided row copy; pitches and widths in bytes, multiples of 2
int copy_rows(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows, hipStream_t stream);
// dst[r][0 .. dwidth) = src[r][0 .. width) followed by zeros
int pad_rows(void *dst, size_t dwidth, const void *src, size_t width, size_t rows, hipStream_t stream);
// rows in groups of `inner` (padded: `inner_p`), `outer` groups: rows widened with zeros, zero rows for inner <= r < inner_p;
// and the inverse
int pad_rows_grouped(void *dst, size_t dwidth, const void *src, size_t width, size_t inner, size_t inner_p, size_t outer,
                     hipStream_t stream);
int unpad_rows_grouped(void *dst, size_t width, const void *src, size_t swidth, size_t inner, size_t inner_p, size_t outer,
                       hipStream_t stream);
// dst[r][0 .. width) += src[r][0 .. width), fp32 elements
int add_rows(float *dst, int64_t dpitch, const float *src, int64_t width, int64_t rows, hipStream_t stream);

}  // namespace mdconv
