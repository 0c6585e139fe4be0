// csr_sort.hip -- deterministic mode (MDCONV_FLAG_DETERMINISTIC): canonical order of the inverted scatter map.
//
// The fill passes (csr_fill_kernel, csr_fill3d_kernel, hp_csr_fill_kernel) take an entry's slot inside its list from an
// integer-atomic cursor, so the order inside a list is the atomics' arrival order, and the gathers sum in list order:
// grad_input is reproducible to rounding only.  This pass runs between fill and gather and sorts every list ascending by
// word 0 of the entry's first int4 (tap * S_o + output pixel in all three entry formats), ties broken by the remaining
// words as unsigned integers -- a total order on the entries' CONTENT, so the sorted list is a pure function of the set
// of entries whatever order the fill left.  Word 0 is unique inside a list by construction; nothing here relies on it
// (equal keys cost a second, exact ranking pass).
//
// One kernel, no atomics, no host synchronisation.  A workgroup owns a chunk of 64 consecutive rows, 16 per wave:
//   * rows of up to 64 entries: a wave holds the row in registers (lane = entry), ranks every entry against the keys
//     of the other lanes (v_readlane, one step per entry) and stores to row start + rank -- in place, the whole row is
//     loaded before the first store;
//   * longer rows are noted in LDS and sorted by the whole workgroup after a barrier: 256 entries at a time in
//     registers, ranked against the row's keys streamed through LDS in blocks of kKeyBlock (broadcast reads), written
//     to a scratch copy of the row (same position in a buffer shaped like `entries`) and copied back.  O(n^2 / 256) per
//     row: correct at any length (a row is K * S_o entries when every sample of an image lands on one pixel), fast it
//     is not -- real layers have rows of a few dozen entries.
#include "mdconv_common.hpp"
#include "mfma_kernels.hpp"   // zero_bytes

namespace mdconv {

namespace {

constexpr int kRowsPerWave = 16;
constexpr int kRowsPerChunk = 4 * kRowsPerWave;
constexpr int kKeyBlock = 2048;

// total order on entries: word 0 as the signed key, then the remaining words as unsigned integers
template <int W> struct Entry { int4 v[W]; };

template <int W> __device__ __forceinline__ bool entry_less(const Entry<W> &a, const Entry<W> &b, bool *equal) {
  *equal = false;
  if (a.v[0].x != b.v[0].x) return a.v[0].x < b.v[0].x;
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const unsigned aw[4] = {(unsigned)a.v[i].x, (unsigned)a.v[i].y, (unsigned)a.v[i].z, (unsigned)a.v[i].w};
    const unsigned bw[4] = {(unsigned)b.v[i].x, (unsigned)b.v[i].y, (unsigned)b.v[i].z, (unsigned)b.v[i].w};
#pragma unroll
    for (int k = (i == 0 ? 1 : 0); k < 4; ++k)
      if (aw[k] != bw[k]) return aw[k] < bw[k];
  }
  *equal = true;
  return false;
}

template <int W> __device__ __forceinline__ Entry<W> load_entry(const int4 *p) {
  Entry<W> e;
#pragma unroll
  for (int i = 0; i < W; ++i) e.v[i] = p[i];
  return e;
}
template <int W> __device__ __forceinline__ void store_entry(int4 *p, const Entry<W> &e) {
#pragma unroll
  for (int i = 0; i < W; ++i) p[i] = e.v[i];
}
template <int W> __device__ __forceinline__ Entry<W> shfl_entry(const Entry<W> &e, int j) {
  Entry<W> r;
#pragma unroll
  for (int i = 0; i < W; ++i)
    r.v[i] = make_int4(__shfl(e.v[i].x, j, 64), __shfl(e.v[i].y, j, 64), __shfl(e.v[i].z, j, 64), __shfl(e.v[i].w, j, 64));
  return r;
}

// a row of 2 .. 64 entries, one wave, in place.  `row` = first int4 of the row, len is wave-uniform
template <int W> __device__ __forceinline__ void sort_row_wave(int4 *row, int len, int lane) {
  const bool on = lane < len;
  Entry<W> mine;
#pragma unroll
  for (int i = 0; i < W; ++i) mine.v[i] = make_int4(0x7fffffff, 0, 0, 0);
  if (on) mine = load_entry<W>(row + (int64_t)lane * W);
  const int key = mine.v[0].x;
  int rank = 0;
  bool tie = false;
  for (int j = 0; j < len; ++j) {
    const int kj = __builtin_amdgcn_readlane(key, j);
    rank += kj < key ? 1 : 0;
    tie = tie || (kj == key && j != lane);
  }
  if (__any(on && tie)) {   // equal keys: rank on the whole entry (identical entries keep their relative order)
    rank = 0;
    for (int j = 0; j < len; ++j) {
      const Entry<W> ej = shfl_entry<W>(mine, j);
      bool eq;
      const bool lt = entry_less<W>(ej, mine, &eq);
      rank += (lt || (eq && j < lane)) ? 1 : 0;
    }
  }
  if (on) store_entry<W>(row + (int64_t)rank * W, mine);
}

// a row of any length, the whole workgroup (256 threads): rank into `tmp`, copy back.  All arguments are
// workgroup-uniform; every thread of the workgroup calls it.
template <int W> __device__ __forceinline__ void sort_row_block(int4 *row, int4 *tmp, int len, int *keys) {
  const int tid = threadIdx.x;
  for (int base = 0; base < len; base += 256) {
    const int i = base + tid;
    const bool on = i < len;
    Entry<W> mine;
#pragma unroll
    for (int k = 0; k < W; ++k) mine.v[k] = make_int4(0x7fffffff, 0, 0, 0);
    if (on) mine = load_entry<W>(row + (int64_t)i * W);
    const int key = mine.v[0].x;
    int rank = 0;
    bool tie = false;
    for (int c0 = 0; c0 < len; c0 += kKeyBlock) {
      const int n = min(kKeyBlock, len - c0);
      __syncthreads();   // the previous block of keys has been read
      for (int j = tid; j < kKeyBlock; j += 256) keys[j] = j < n ? row[(int64_t)(c0 + j) * W].x : 0x7fffffff;
      __syncthreads();
      const int n4 = (n + 3) / 4;
      for (int j4 = 0; j4 < n4; ++j4) {
        const int4 k4 = reinterpret_cast<const int4 *>(keys)[j4];   // same address in every lane: a broadcast
        const int j = c0 + j4 * 4;
        rank += (k4.x < key ? 1 : 0) + (k4.y < key ? 1 : 0) + (k4.z < key ? 1 : 0) + (k4.w < key ? 1 : 0);
        tie = tie || (k4.x == key && j != i) || (k4.y == key && j + 1 != i) || (k4.z == key && j + 2 != i) ||
              (k4.w == key && j + 3 != i);
      }
    }
    if (on && tie) {   // equal keys (the padding of the last key block included): exact rank against the row itself
      rank = 0;
      for (int j = 0; j < len; ++j) {
        const Entry<W> ej = load_entry<W>(row + (int64_t)j * W);
        bool eq;
        const bool lt = entry_less<W>(ej, mine, &eq);
        rank += (lt || (eq && j < i)) ? 1 : 0;
      }
    }
    if (on) store_entry<W>(tmp + (int64_t)rank * W, mine);
  }
  __threadfence_block();
  __syncthreads();   // the row is complete in tmp, and nobody reads `row` any more
  for (int64_t x = tid; x < (int64_t)len * W; x += 256) row[x] = tmp[x];
}

// rowptr [nseg][S_e + 1], entries / scratch [nseg][seg_stride entries of W int4]; rows = nseg * S_e
template <int W>
__global__ __launch_bounds__(256) void csr_sort_rows_kernel(const int *__restrict__ rowptr, int4 *entries, int4 *scratch,
                                                            int S_e, int64_t seg_stride, int64_t rows) {
  __shared__ __attribute__((aligned(16))) int keys[kKeyBlock];
  __shared__ unsigned long_rows[4];   // per wave: bit k = its row k is longer than a wave
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t chunks = (rows + kRowsPerChunk - 1) / kRowsPerChunk;
  for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const int64_t r0 = chunk * kRowsPerChunk + wave * kRowsPerWave;
    // bounds of the wave's rows: lane k < 16 holds row r0 + k
    int e0 = 0, e1 = 0;
    int64_t seg_base = 0;
    if (lane < kRowsPerWave && r0 + lane < rows) {
      const int64_t seg = (r0 + lane) / S_e;
      const int a = (int)(r0 + lane - seg * S_e);
      const int *rp = rowptr + seg * (S_e + 1) + a;
      e0 = rp[0];
      e1 = rp[1];
      seg_base = seg * seg_stride;
    }
    unsigned longer = 0;
    for (int k = 0; k < kRowsPerWave; ++k) {
      const int s = __builtin_amdgcn_readlane(e0, k);
      const int len = __builtin_amdgcn_readlane(e1, k) - s;
      if (len < 2) continue;
      if (len > 64) { longer |= 1u << k; continue; }
      const int64_t sb = ((int64_t)__builtin_amdgcn_readlane((int)(seg_base >> 32), k) << 32) |
                         (unsigned)__builtin_amdgcn_readlane((int)(seg_base & 0xffffffff), k);
      sort_row_wave<W>(entries + (sb + s) * W, len, lane);
    }
    if (lane == 0) long_rows[wave] = longer;
    __syncthreads();
    for (int w = 0; w < 4; ++w) {
      unsigned m = long_rows[w];   // workgroup-uniform
      while (m) {
        const int k = __ffs(m) - 1;
        m &= m - 1;
        const int64_t r = chunk * kRowsPerChunk + w * kRowsPerWave + k;
        const int64_t seg = r / S_e;
        const int a = (int)(r - seg * S_e);
        const int *rp = rowptr + seg * (S_e + 1) + a;
        const int s = rp[0], len = rp[1] - s;
        const int64_t at = (seg * seg_stride + s) * W;
        sort_row_block<W>(entries + at, scratch + at, len, keys);
        __syncthreads();
      }
    }
    __syncthreads();   // long_rows is rewritten by the next chunk
  }
}

}  // namespace

size_t csr_sort_scratch_bytes(int width, int64_t seg_stride, int nseg) {
  return (size_t)nseg * (size_t)seg_stride * (size_t)width * sizeof(int4);
}

int csr_sort_rows(const int *rowptr, void *entries, void *scratch, int width, int S_e, int64_t seg_stride, int nseg,
                  hipStream_t stream) {
  const int64_t rows = (int64_t)nseg * S_e;
  if (rows <= 0) return MDCONV_OK;
  const int64_t chunks = (rows + kRowsPerChunk - 1) / kRowsPerChunk;
  const dim3 grid((unsigned)(chunks > 16384 ? 16384 : chunks));
  if (width == 1)
    hipLaunchKernelGGL(csr_sort_rows_kernel<1>, grid, dim3(256), 0, stream, rowptr, (int4 *)entries, (int4 *)scratch, S_e,
                       seg_stride, rows);
  else
    hipLaunchKernelGGL(csr_sort_rows_kernel<2>, grid, dim3(256), 0, stream, rowptr, (int4 *)entries, (int4 *)scratch, S_e,
                       seg_stride, rows);
  return check_launch("csr_sort_rows");
}

// ---- the list build of the VALU families (ScatterLists, mdconv_common.hpp) ----
namespace {
__global__ __launch_bounds__(256) void lists_scan_kernel(int S, const int *__restrict__ cnt, int *__restrict__ rowptr) {
  csr_scan_chunk(S, cnt, rowptr);
}
int csr_scan_launch(int S, int nseg, const int *cnt, int *rowptr, hipStream_t stream) {
  hipLaunchKernelGGL(lists_scan_kernel, dim3((S + kScanChunk - 1) / kScanChunk, nseg), dim3(256), 0, stream, S, cnt, rowptr);
  return check_launch("lists_scan");
}
}  // namespace

int scatter_lists_build(const ScatterLists &L, void *ws, bool det, hipStream_t stream,
                        const std::function<void(bool fill, int *cnt, const int *rowptr, void *entries)> &launch_list) {
  char *base = (char *)ws;
  int *cnt = (int *)(base + L.off_cnt), *rowptr = (int *)(base + L.off_rowptr);
  int rc;
  if ((rc = zero_bytes(cnt, (size_t)L.nseg * L.rows * 4, stream))) return rc;
  launch_list(false, cnt, rowptr, base + L.off_entries);
  if ((rc = check_launch("lists_count"))) return rc;
  if ((rc = csr_scan_launch(L.rows, L.nseg, cnt, rowptr, stream))) return rc;
  launch_list(true, cnt, rowptr, base + L.off_entries);
  if ((rc = check_launch("lists_fill"))) return rc;
  if (!det) return MDCONV_OK;
  return csr_sort_rows(rowptr, base + L.off_entries, base + L.off_sort, 1, L.rows, L.seg_stride, L.nseg, stream);
}

}  // namespace mdconv
