// util_kernels.hip -- the layout and conversion kernels every kernel family's host code uses (host_util.hpp): clearing,
// fp16 / bf16 <-> fp32, strided row copies, zero padding of rows and its inverse, row sums.
//
// All of them are KERNELS rather than hipMemsetAsync / hipMemcpy2DAsync: memset and memcpy nodes made HIP graph replay
// fault (tools/graph_check.py), and the library promises plain kernel sequences that capture cleanly.
#include "host_util.hpp"
#include "mfma_kernels.hpp"

namespace mdconv {

namespace {

__global__ __launch_bounds__(256) void zero_words_kernel(unsigned *__restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0u;
}
__global__ __launch_bounds__(256) void zero_halfwords_kernel(unsigned short *__restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0;
}

template <typename H>
__global__ __launch_bounds__(256) void widen_kernel(const H *__restrict__ src, float *__restrict__ dst, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    dst[i] = ld(src + i);
}
template <typename H, bool ACCUM>
__global__ __launch_bounds__(256) void narrow_kernel(const float *__restrict__ src, H *__restrict__ dst, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    st(dst + i, ACCUM ? ld(dst + i) + src[i] : src[i]);
}
template <bool ACCUM>
__global__ __launch_bounds__(256) void store_f32_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    dst[i] = ACCUM ? dst[i] + src[i] : src[i];
}

template <typename W>
__global__ __launch_bounds__(256) void copy_rows_kernel(W *__restrict__ dst, int64_t dpitch, const W *__restrict__ src,
                                                        int64_t spitch, int64_t width, int64_t rows) {
  const int64_t n = width * rows;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / width, c = i - r * width;
    dst[r * dpitch + c] = src[r * spitch + c];
  }
}

// dst[r][0 .. dwidth) = src[r][0 .. width) followed by zeros (element = W)
template <typename W>
__global__ __launch_bounds__(256) void pad_rows_kernel(W *__restrict__ dst, int64_t dwidth, const W *__restrict__ src,
                                                       int64_t width, int64_t rows) {
  const int64_t n = dwidth * rows;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / dwidth, c = i - r * dwidth;
    dst[i] = c < width ? src[r * width + c] : (W)0;
  }
}
// Rows in groups of `inner` (padded: `inner_p`), `outer` groups: dst row (q, r) = src row (q, r) widened to dwidth with zeros for
// r < inner, a zero row for inner <= r < inner_p (weights: the rows of one conv group's output channels, padded to the kernels' floor)
template <typename W>
__global__ __launch_bounds__(256) void pad_rows_grouped_kernel(W *__restrict__ dst, int64_t dwidth, const W *__restrict__ src,
                                                               int64_t width, int64_t inner, int64_t inner_p, int64_t outer) {
  const int64_t n = dwidth * inner_p * outer;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t rd = i / dwidth, c = i - rd * dwidth;
    const int64_t q = rd / inner_p, r = rd - q * inner_p;
    dst[i] = (r < inner && c < width) ? src[(q * inner + r) * width + c] : (W)0;
  }
}
// the inverse: dst row (q, r) (width elements) = the first `width` elements of src row (q, r) of the padded layout
template <typename W>
__global__ __launch_bounds__(256) void unpad_rows_grouped_kernel(W *__restrict__ dst, int64_t width, const W *__restrict__ src,
                                                                 int64_t swidth, int64_t inner, int64_t inner_p, int64_t outer) {
  const int64_t n = width * inner * outer;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t rs = i / width, c = i - rs * width;
    const int64_t q = rs / inner, r = rs - q * inner;
    dst[i] = src[(q * inner_p + r) * swidth + c];
  }
}

__global__ __launch_bounds__(256) void add_rows_kernel(float *__restrict__ dst, int64_t dpitch,
                                                       const float *__restrict__ src, int64_t width, int64_t rows) {
  const int64_t n = width * rows;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / width;
    dst[r * dpitch + (i - r * width)] += src[i];
  }
}

// Byte counts and addresses that are all 4-byte aligned move as 4-byte words, anything else as 2-byte halfwords (the
// element sizes are 2 and 4): the launchers below run their kernel for W = unsigned or unsigned short accordingly.
bool word_aligned(size_t sizes, const void *a, const void *b = nullptr) {
  return ((sizes | (uintptr_t)a | (uintptr_t)b) & 3) == 0;
}
// grid-stride launch of `n` elements: 256 threads, at most `cap` workgroups
dim3 grid_for(int64_t n, int64_t cap) {
  const int64_t b = (n + 255) / 256;
  return dim3((unsigned)(b > cap ? cap : (b < 1 ? 1 : b)));
}

template <typename W>
void copy_rows_t(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows, hipStream_t stream) {
  constexpr size_t es = sizeof(W);
  hipLaunchKernelGGL(copy_rows_kernel<W>, grid_for((int64_t)(width / es) * (int64_t)rows, 16384), dim3(256), 0, stream, (W *)dst,
                     (int64_t)(dpitch / es), (const W *)src, (int64_t)(spitch / es), (int64_t)(width / es), (int64_t)rows);
}
template <typename W>
void pad_rows_t(void *dst, size_t dwidth, const void *src, size_t width, size_t rows, hipStream_t stream) {
  constexpr size_t es = sizeof(W);
  hipLaunchKernelGGL(pad_rows_kernel<W>, grid_for((int64_t)(dwidth / es) * (int64_t)rows, 16384), dim3(256), 0, stream, (W *)dst,
                     (int64_t)(dwidth / es), (const W *)src, (int64_t)(width / es), (int64_t)rows);
}
template <typename W>
void pad_rows_grouped_t(void *dst, size_t dwidth, const void *src, size_t width, size_t inner, size_t inner_p, size_t outer,
                        hipStream_t stream) {
  constexpr size_t es = sizeof(W);
  hipLaunchKernelGGL(pad_rows_grouped_kernel<W>, grid_for((int64_t)(dwidth / es) * (int64_t)(inner_p * outer), 16384), dim3(256), 0,
                     stream, (W *)dst, (int64_t)(dwidth / es), (const W *)src, (int64_t)(width / es), (int64_t)inner,
                     (int64_t)inner_p, (int64_t)outer);
}
template <typename W>
void unpad_rows_grouped_t(void *dst, size_t width, const void *src, size_t swidth, size_t inner, size_t inner_p, size_t outer,
                          hipStream_t stream) {
  constexpr size_t es = sizeof(W);
  hipLaunchKernelGGL(unpad_rows_grouped_kernel<W>, grid_for((int64_t)(width / es) * (int64_t)(inner * outer), 16384), dim3(256), 0,
                     stream, (W *)dst, (int64_t)(width / es), (const W *)src, (int64_t)(swidth / es), (int64_t)inner,
                     (int64_t)inner_p, (int64_t)outer);
}
template <typename H> void narrow_t(const float *src, void *dst, int64_t n, bool accum, hipStream_t s) {
  if (accum)
    hipLaunchKernelGGL((narrow_kernel<H, true>), grid_for(n, 16384), dim3(256), 0, s, src, (H *)dst, n);
  else
    hipLaunchKernelGGL((narrow_kernel<H, false>), grid_for(n, 16384), dim3(256), 0, s, src, (H *)dst, n);
}

}  // namespace

int zero_bytes(void *p, size_t bytes, hipStream_t s) {
  if (bytes == 0 || p == nullptr) return MDCONV_OK;
  if (word_aligned(bytes, p)) {
    const int64_t n = (int64_t)(bytes / 4);
    hipLaunchKernelGGL(zero_words_kernel, grid_for(n, 8192), dim3(256), 0, s, (unsigned *)p, n);
  } else {
    const int64_t n = (int64_t)(bytes / 2);
    hipLaunchKernelGGL(zero_halfwords_kernel, grid_for(n, 8192), dim3(256), 0, s, (unsigned short *)p, n);
  }
  return check_launch("zero");
}

// 16-bit tensors the native kernels do not take (hp_plan) run through fp32 copies: fp16 and bf16
int widen(int dtype, const void *src, float *dst, int64_t n, hipStream_t s) {
  if (n == 0) return MDCONV_OK;
  if (dtype == MDCONV_BF16)
    hipLaunchKernelGGL(widen_kernel<bf16_t>, grid_for(n, 16384), dim3(256), 0, s, (const bf16_t *)src, dst, n);
  else
    hipLaunchKernelGGL(widen_kernel<__half>, grid_for(n, 16384), dim3(256), 0, s, (const __half *)src, dst, n);
  return check_launch("widen");
}
int narrow(int dtype, const float *src, void *dst, int64_t n, bool accum, hipStream_t s) {
  if (n == 0) return MDCONV_OK;
  if (dtype == MDCONV_BF16) narrow_t<bf16_t>(src, dst, n, accum, s);
  else narrow_t<__half>(src, dst, n, accum, s);
  return check_launch("narrow");
}
int store_f32(const float *src, float *dst, int64_t n, bool accum, hipStream_t s) {
  if (n == 0) return MDCONV_OK;
  if (accum) hipLaunchKernelGGL(store_f32_kernel<true>, grid_for(n, 16384), dim3(256), 0, s, src, dst, n);
  else hipLaunchKernelGGL(store_f32_kernel<false>, grid_for(n, 16384), dim3(256), 0, s, src, dst, n);
  return check_launch("store_f32");
}

int copy_rows(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows, hipStream_t stream) {
  if (width == 0 || rows == 0) return MDCONV_OK;
  if (word_aligned(dpitch | spitch | width, dst, src)) copy_rows_t<unsigned>(dst, dpitch, src, spitch, width, rows, stream);
  else copy_rows_t<unsigned short>(dst, dpitch, src, spitch, width, rows, stream);
  return check_launch("copy_rows");
}
int pad_rows(void *dst, size_t dwidth, const void *src, size_t width, size_t rows, hipStream_t stream) {
  if (word_aligned(dwidth | width, dst, src)) pad_rows_t<unsigned>(dst, dwidth, src, width, rows, stream);
  else pad_rows_t<unsigned short>(dst, dwidth, src, width, rows, stream);
  return check_launch("pad_rows");
}
int pad_rows_grouped(void *dst, size_t dwidth, const void *src, size_t width, size_t inner, size_t inner_p, size_t outer,
                     hipStream_t stream) {
  if (word_aligned(dwidth | width, dst, src)) pad_rows_grouped_t<unsigned>(dst, dwidth, src, width, inner, inner_p, outer, stream);
  else pad_rows_grouped_t<unsigned short>(dst, dwidth, src, width, inner, inner_p, outer, stream);
  return check_launch("pad_rows_grouped");
}
int unpad_rows_grouped(void *dst, size_t width, const void *src, size_t swidth, size_t inner, size_t inner_p, size_t outer,
                       hipStream_t stream) {
  if (word_aligned(swidth | width, dst, src)) unpad_rows_grouped_t<unsigned>(dst, width, src, swidth, inner, inner_p, outer, stream);
  else unpad_rows_grouped_t<unsigned short>(dst, width, src, swidth, inner, inner_p, outer, stream);
  return check_launch("unpad_rows_grouped");
}
int add_rows(float *dst, int64_t dpitch, const float *src, int64_t width, int64_t rows, hipStream_t stream) {
  hipLaunchKernelGGL(add_rows_kernel, grid_for(width * rows, 8192), dim3(256), 0, stream, dst, dpitch, src, width, rows);
  return check_launch("add_rows");
}

}  // namespace mdconv
