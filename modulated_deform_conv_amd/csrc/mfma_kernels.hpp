// mfma_kernels.hpp -- entry points of the MFMA implicit-GEMM path (see mfma_*.hip).
#pragma once
#include "mdconv_common.hpp"

namespace mdconv {

// the family's plans and their execution: mfma_plan.hpp (host code only)
bool mfma_supported(const Geom &g, int dtype, bool backward);            // mfma_plan() finds a plan
size_t mfma_workspace_bytes(const Geom &g, int dtype, bool backward);    // its `total` (0: none)

// records the calling thread's "grad_weight / grad_bias are final" event on `stream`
// (include/mdconv.h: mdconv_stream_wait_weight_ready)
int record_weight_ready(hipStream_t stream);

// Two independent tails of a backward on two streams: fork_side_stream() returns a library-owned stream (own
// hardware queue) that waits for everything enqueued on `stream` so far -- or nullptr (MDCONV_BWD_FORK=0);
// join_side_stream() makes `stream` wait for it.  Captures into HIP graphs.
hipStream_t fork_side_stream(hipStream_t stream);
int join_side_stream(hipStream_t stream);

// geometry variant of the fp32 matrix kernels a call launched (mdconv_last_geometry): 0 = run-time, 1 = canonical 3x3
void note_geometry_variant(int v);

// clears `bytes` (a multiple of 2) of device memory with a kernel (graph-capture friendly)
int zero_bytes(void *p, size_t bytes, hipStream_t stream);

// benchmark hooks (include/mdconv.h: mdconv_profile_*)
void profile_mark(int which, bool begin, hipStream_t stream, const char *name = nullptr);

}  // namespace mdconv
