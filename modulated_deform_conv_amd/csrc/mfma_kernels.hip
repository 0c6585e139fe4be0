// mfma_kernels.hip -- the fp32 matrix-core family as the kernels tile it: workspace layout of the backward (bwd_dims),
// the batch-chunk plan, the fork / join of the backward's two tails, weight packing, and the kernel sequences of the
// native forward / backward.  Shapes the kernels do not tile: mfma_plans.hip.
#include "mfma_plan.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <mutex>
#include <vector>

namespace mdconv {

namespace {

// W[g*Og + o][c][tap]  ->  wp (MFMA-fragment order, mfma_tile.hpp) and wq[g][tap][o][c], zero padded.
__global__ __launch_bounds__(256) void pack_weights_kernel(Geom g, PackDims pd,
                                                           const float *__restrict__ w,
                                                           float *__restrict__ wp,
                                                           float *__restrict__ wq) {
  const int64_t total = (int64_t)g.G * g.K * pd.Cgp * pd.Ogp;
  const int mblks = pd.Ogp / 32, cchunks = pd.Cgp / kBK;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    // decode i as a wp index: [grp][tap][cchunk][mblk][q][lane][s]
    int64_t r = i;
    const int s = (int)(r & 3); r >>= 2;
    const int lane = (int)(r & 63); r >>= 6;
    const int q = (int)(r & 1); r >>= 1;
    const int mblk = (int)(r % mblks); r /= mblks;
    const int cchunk = (int)(r % cchunks); r /= cchunks;
    const int tap = (int)(r % g.K);
    const int grp = (int)(r / g.K);
    const int o = mblk * 32 + (lane & 31);
    const int c = cchunk * kBK + 8 * q + 4 * (lane >> 5) + s;
    const float v = (o < g.Og && c < g.Cg)
                        ? w[((int64_t)(grp * g.Og + o) * g.Cg + c) * g.K + tap] : 0.f;
    wp[i] = v;
    if (wq) wq[(((int64_t)grp * g.K + tap) * pd.Ogp + o) * pd.Cgp + c] = v;
  }
}

bool bwd_fork_enabled();   // defined with the fork / join helpers below

}  // namespace

int device_cus() {
  static std::atomic<int> cus{0};
  int n = cus.load(std::memory_order_relaxed);
  if (n) return n;
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
    n = prop.multiProcessorCount;
  else
    n = 256;
  (void)hipGetLastError();
  cus.store(n, std::memory_order_relaxed);
  return n;
}

int pack_weights_f32(const Geom &g, const PackDims &pd, const float *weight, float *wp, float *wq,
                     hipStream_t stream) {
  const int64_t total = (int64_t)g.G * g.K * pd.Cgp * pd.Ogp;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pack_weights_kernel, dim3(blocks), dim3(256), 0, stream, g, pd, weight, wp, wq);
  return check_launch("pack_weights");
}

// `skip`: a backward without grad_input / without the weight gradients -- the slots only the skipped stages write take no
// bytes; everything GEMM-1 and the requested stages use (tiling, split-K count, the slots GEMM-1 itself writes) is unchanged,
// so the requested gradients are the same sums in the same order
BwdDims bwd_dims(const Geom &g, Skip skip) {
  BwdDims bd;
  bd.Np = (g.N + 31) / 32 * 32;
  // 64 x 64 tiles (all four waves busy when C_out <= 64) were measured SLOWER than 256 x 32 tiles
  // with idle waves at cfg4 for the NCHW gathers (GEMM-2 5.4 -> 8 ms: bound by the cache-line
  // traffic of the 8-corner gathers, not by the matrix work), so that variant stays an experiment.
  // With channels-last gathers the tile is always 64 input channels wide.
  bd.cl = bwd_channels_last(g) ? 1 : 0;
  bd.wtile = 0;
  if (bd.cl) bd.wtile = g.O <= 64 ? 1 : (g.O <= 128 ? 2 : 3);
  const int rm = bd.cl ? (bd.wtile == 1 ? 64 : (bd.wtile == 2 ? 128 : 256)) : (bd.wtile ? 64 : 256);
  const int cn = bd.cl ? 64 : (bd.wtile ? 64 : 32);
  bd.OgpB = (g.O + rm - 1) / rm * rm;
  bd.mblks = bd.OgpB / 32;
  bd.mtiles = bd.OgpB / rm;
  bd.Cp = (g.C + cn - 1) / cn * cn;
  bd.cblks = bd.Cp / cn;
  const int col_tiles = bd.mtiles * g.K * bd.cblks;
  const int pairs = bd.Np / 32;
  // Split-K so that the grid is ONE full dispatch round: every workgroup does the same work, so a grid of
  // 1.36 x the resident slots (cfg2 in round 3: 36 column tiles x 29 splits = 1044 workgroups on 256 CUs x 3)
  // runs its last 276 workgroups one per CU at half the matrix rate -- 0.68 of peak where the steady state
  // reaches 0.8+.  slots = CUs x resident workgroups of the instance that will run (hipOccupancy).
  const bool padn = bd.Np != g.N;
  const int occ = bd.cl ? mfma_bwd_weight_cl_occupancy(g.nd, padn, bd.wtile)
                        : mfma_bwd_weight_occupancy(g.nd, padn, bd.wtile);
  // ... minus one per CU when the grad_input gather runs beside this kernel on the forked stream: a full round of
  // 164-register workgroups leaves the gather no wave slot until the round retires, and the two tails then run one
  // after the other (cfg2, 36 column tiles: 21 splits = 756 workgroups -> GEMM-2 1.00 ms then gather 0.30 ms,
  // backward 2.35 ms; 14 splits = 504 workgroups, two per CU -> both done after 0.96 ms, backward 2.25 ms)
  const int occ_run = bwd_fork_enabled() && occ > 1 ? occ - 1 : occ;
  const int slots = device_cus() * occ_run;
  int splits = slots / col_tiles;
  if (splits > pairs) splits = pairs;
  if (splits < 1) splits = 1;
  bd.pairs_per_split = (pairs + splits - 1) / splits;
  bd.splits = (pairs + bd.pairs_per_split - 1) / bd.pairs_per_split;
  static const bool debug_plan = getenv("MDCONV_DEBUG_PLAN") != nullptr;
  if (debug_plan)
    fprintf(stderr, "[mdconv] GEMM-2 plan: cl %d wtile %d col_tiles %d occ %d slots %d splits %d x %d pairs\n", bd.cl,
            bd.wtile, col_tiles, occ, slots, bd.splits, bd.pairs_per_split);
  bd.ochunks = (g.O + 63) / 64 * 4;   // K loop of GEMM-1 is unrolled 4x
  bd.waves_c = g.C > 128 ? 4 : (g.C > 64 ? 2 : 1);
  // The grad_out tile ([32 * 4 / waves_c pixels] x C_out) lives in LDS: when it does not fit with the natural wave split
  // (C_in <= 64 and C_out > ~192 in 3-D: 128 pixels x 256 channels = 133 KB + the drain's tiles), more waves go along the
  // channels -- the extra ones own zero-padded channel blocks and idle through the drain -- and the pixel tile shrinks
  // with them.  Half the matrix rate of GEMM-1 at such shapes, against the shape-generic kernels they used to fall to (~10x).
  for (;;) {
    bd.cblks_q = (g.C + 64 * bd.waves_c - 1) / (64 * bd.waves_c) * (2 * bd.waves_c);
    // GEMM-1 drain: channels-last (line-wide gathers through an LDS hand-over, mfma_bwd_data.hip)
    // whenever the backward has the channels-last copy -- except for straight-line 2-D shapes whose
    // LDS (grad_out tile + parked accumulators) would then allow only one workgroup per CU
    // (C_in = 128, C_out = 256: 1.56 -> 1.70 ms).  MDCONV_BD_CL = 0 / 1 overrides.
    // Reduction buffer [tap group][64-channel blocks to reduce][nd + 1][pixels of the tile]: groups of
    // 3 taps instead of 9 where that keeps the kernel under 80 KB of LDS (two workgroups per CU).
    const int red_per_tap = 128 * (g.DG > 1 ? bd.cblks_q / (2 * bd.waves_c) : 1) * (g.nd + 1);
    const bool single_owner = g.DG == 1 && bd.waves_c == 1 && bd.cblks_q == 2;   // direct writes, no buffer
    auto size_red = [&]() {
      bd.tap_group = 9;
      bd.red_floats = single_owner ? 0 : bd.tap_group * red_per_tap;
      if (bd.red_floats && bwd_data_lds_bytes(g, bd) > 80 * 1024) {
        bd.tap_group = 3;
        bd.red_floats = bd.tap_group * red_per_tap;
      }
    };
    {
      const int nbatch = g.nd == 2 ? 4 : 8, nquads = bd.ochunks / 4;
      const bool straight = g.nd == 2 && g.G == 1 && nquads % nbatch == 0 && nquads / nbatch <= 2;
      static const int bd_cl_env = getenv("MDCONV_BD_CL") ? atoi(getenv("MDCONV_BD_CL")) : -1;
      bd.cl_drain = bd.cl;
      size_red();
      if (bd.cl && straight && (bd_cl_env == 0 || (bd_cl_env < 0 && bwd_data_lds_bytes(g, bd) > 80 * 1024))) {
        bd.cl_drain = 0;
        size_red();
      }
    }
    if (bwd_data_lds_bytes(g, bd) <= kBwdDataLdsCap || bd.waves_c == 4) break;
    bd.waves_c *= 2;
  }
  const int nc = 1 << g.nd;
  size_t off = 0;
  bd.off_wq = off;   off += align_up((size_t)g.K * bd.ochunks * bd.cblks_q * 2 * 64 * 16);
  bd.off_ga = off;   off += align_up((size_t)bd.Np * bd.OgpB * sizeof(float));
  bd.off_table = off; off += align_up((size_t)g.DG * g.K * bd.Np * 2 * (1 << g.nd) * sizeof(int));
  bd.off_part = off; off += skip.weight ? 0 : align_up((size_t)bd.splits * g.K * bd.OgpB * bd.Cp * sizeof(float));
  bd.off_gcol = off; off += align_up((size_t)g.B * g.C * g.K * g.S_o * sizeof(float));
  // scatter lists: 2-D one entry per corner pair keyed by the pair's first pixel; 3-D one entry per
  // sample keyed by its low corner in the extended anchor space (4x fewer entries and atomics)
  bd.sample_keyed = g.nd == 3 ? 1 : 0;
  bd.S_e = bd.sample_keyed ? hp_anchor_space(g) : g.S_i;
  bd.off_cnt = off;  off += align_up((size_t)g.B * g.DG * bd.S_e * sizeof(int));
  // (the counters stay with NO_GRAD_INPUT: GEMM-1's counting pass writes them)
  bd.off_rowptr = off; off += skip.input ? 0 : align_up((size_t)g.B * g.DG * (bd.S_e + 1) * sizeof(int));
  bd.off_entries = off; off += skip.input ? 0 : align_up((size_t)g.B * g.DG * g.K * g.S_o * (bd.sample_keyed ? 32 : (nc / 2) * 16));
  bd.bias_tiles = (g.N + 32 * (4 / bd.waves_c) - 1) / (32 * (4 / bd.waves_c));
  bd.off_bias = off; off += align_up((size_t)bd.bias_tiles * g.O * sizeof(float));
  bd.off_xt = off;   off += bd.cl ? align_up((size_t)g.B * g.S_i * g.C * sizeof(float)) : 0;
  static const int c2i_env = getenv("MDCONV_C2I3D") ? atoi(getenv("MDCONV_C2I3D")) : 2;
  bd.two_pass = bd.sample_keyed && c2i_env >= 2 ? 1 : 0;
  bd.off_sums = off; off += bd.two_pass && !skip.input ? align_up(col2im3d_sums_bytes(g)) : 0;
  bd.off_bstage = off; off += g.with_bias && !skip.weight ? align_up(grad_bias_stage_bytes(g)) : 0;
  // deterministic mode: scratch of the list sort, shaped like the entries (csr_sort.hip); after everything else, so the
  // default layout is untouched
  bd.off_sort = off;
  off += g.det && !skip.input ? align_up(csr_sort_scratch_bytes(bd.sample_keyed ? 2 : 1, (int64_t)g.K * g.S_o * (bd.sample_keyed ? 1 : nc / 2),
                                                 g.B * g.DG)) : 0;
  bd.off_end = off;
  return bd;
}

// ---------------------------------------------------------------------------------------------
// Execution plan: batch chunking + fp16 I/O.
//  * The kernels address tensors with 32-bit byte offsets (raw buffer loads), so a call is cut
//    into chunks of Bc images such that every per-chunk tensor (and the grad_col workspace)
//    stays below 2 GiB.  grad_weight / grad_bias accumulate across chunks by construction.
//    (This is the only thing left of the reference's `in_step` chunk loop.)
//  * fp16 tensors are computed in fp32: each chunk is widened into fp32 copies in the workspace,
//    run through the fp32 kernels (coordinates and accumulation in fp32) and
//    narrowed back; grad_weight / grad_bias are accumulated in fp32 over all chunks.
// ---------------------------------------------------------------------------------------------
namespace {

// 2 GiB minus slack
constexpr size_t kChunkCeiling = ((size_t)1 << 31) - (1 << 16);

size_t fwd_core_bytes(const Geom &gc) {
  const PackDims pd = pack_dims(gc);
  size_t n = align_up((size_t)gc.G * gc.K * pd.Cgp * pd.Ogp * sizeof(float));
  if (fwd_channels_last(gc)) n += align_up(fwd_cl_bytes(gc));   // NHWC copy of the input chunk
  n += align_up(fwd_tail_bytes(gc));                            // tap-range partials of the last dispatch round
  return n;
}

// chunking and workspace layout of a shape the kernels tile (native_plan)
bool make_plan(const Geom &g, int dtype, bool backward, Skip skip, Plan *p) {
  const size_t per_in = (size_t)g.C * g.S_i * 4, per_out = (size_t)g.O * g.S_o * 4;
  const size_t per_col = (size_t)g.C * g.K * g.S_o * 4;
  size_t per = per_in > per_out ? per_in : per_out;
  if (backward) {
    // every workspace buffer the backward kernels address with 32-bit buffer offsets must stay
    // below the limit for one chunk: grad_col, the packed grad_out (rows padded to the GEMM-2 tile:
    // up to 256 output channels even for small C_out), the tap table and the scatter lists
    const BwdDims b1 = bwd_dims(chunk_geom(g, 1));
    const size_t per_ga = (size_t)g.S_o * b1.OgpB * 4;
    const size_t per_tab = (size_t)g.DG * g.K * g.S_o * 2 * (1 << g.nd) * 4;
    const size_t per_ent = (size_t)g.DG * g.K * g.S_o * 32;   // 2 pair entries (2-D) or 1 sample entry (3-D)
    if (per_col > per) per = per_col;
    if (per_ga > per) per = per_ga;
    if (per_tab > per) per = per_tab;
    if (per_ent > per) per = per_ent;
  }
  const size_t kLim = chunk_limit(kChunkCeiling);
  if (per >= kLim) return false;
  int bc = (int)(kLim / per);
  if (bc > g.B) bc = g.B;
  p->Bc = bc;
  p->half_io = dtype == MDCONV_F16 || dtype == MDCONV_BF16;
  p->skip = backward ? skip : Skip();
  p->gc = chunk_geom(g, bc);
  if (backward) p->bd = bwd_dims(p->gc, skip);
  p->core_bytes = backward ? p->bd.off_end : fwd_core_bytes(p->gc);
  // A shorter last chunk lays its workspace out anew (bwd_dims per chunk) and can need MORE than a full one: below the
  // channels-last threshold GEMM-2 pads its rows to 256 output channels and its split-K partials grow (C = O = 64 at
  // 32 x 32: chunks of 8 images 35.7 MB, a last chunk of 5 images 43.8 MB), and the split-K count follows the occupancy
  // of the instance N % 32 selects.  A call has at most two chunk sizes: size the kernels' part for the larger need.
  // (Single-chunk calls skip this.  With MDCONV_DEBUG_PLAN, bwd_dims prints a GEMM-2 plan line for every sizing done
  // here -- one image, the full chunk, the tail; the chunks that are launched run with these layouts.)
  if (g.B % bc) {
    const Geom gt = chunk_geom(g, g.B % bc);
    if (backward) p->bd_tail = bwd_dims(gt, skip);
    const size_t tail_bytes = backward ? p->bd_tail.off_end : fwd_core_bytes(gt);
    if (tail_bytes > p->core_bytes) p->core_bytes = tail_bytes;
  }
  Bump ws{p->core_bytes};
  p->off_w = p->off_b = p->off_x = p->off_off = p->off_m = p->off_go = p->off_out = 0;
  p->off_gi = p->off_goff = p->off_gm = p->off_gw = p->off_gb = 0;
  if (p->half_io) {
    const size_t n_w = (size_t)g.O * g.Cg * g.K * 4, n_x = (size_t)bc * g.C * g.S_i * 4, n_o = (size_t)bc * g.O * g.S_o * 4;
    const size_t n_off = (size_t)bc * g.DG * g.nd * g.K * g.S_o * 4, n_m = (size_t)bc * g.DG * g.K * g.S_o * 4;
    p->off_w = ws.take(n_w);
    p->off_b = ws.take((size_t)g.O * 4);
    p->off_x = ws.take(n_x);
    p->off_off = ws.take(n_off);
    p->off_m = ws.take(n_m);
    if (!backward) {
      p->off_out = ws.take(n_o);
    } else {
      p->off_go = ws.take(n_o);
      p->off_gi = ws.take(skip.input ? 0 : n_x);
      p->off_goff = ws.take(n_off);
      p->off_gm = ws.take(n_m);
      p->off_gw = ws.take(skip.weight ? 0 : n_w);
      p->off_gb = ws.take(skip.weight ? 0 : (size_t)g.O * 4);
    }
  }
  p->total = ws.off;
  return true;
}

// Fork / join helper for the one piece of the backward that does not depend on its neighbour: the
// grad_input gather (CSR build + col2im, HBM-bound) needs GEMM-1's grad_col and counters only, GEMM-2
// (matrix-bound) needs GEMM-1's packed grad_out and tap table only.  One side stream and two events
// per (device, caller stream), created on first use and kept (bounded like the weights-ready events).
struct Fork { hipStream_t side; hipEvent_t fork, join, bias; };
std::mutex g_fork_mu;
std::vector<std::pair<std::pair<int, hipStream_t>, Fork>> g_forks;
bool get_fork(hipStream_t stream, Fork *out) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  std::lock_guard<std::mutex> lock(g_fork_mu);
  for (auto &e : g_forks)
    if (e.first.first == dev && e.first.second == stream) { *out = e.second; return true; }
  // Entries are never destroyed: another host thread may be between fork and join on any of them (advisor,
  // round 3).  Past 64 distinct (device, stream) callers a new one simply runs its backward unforked.
  if (g_forks.size() >= 64) return false;
  Fork f;
  // A stream of ANOTHER priority class: HIP multiplexes the streams of one class over a few hardware queues,
  // and once a process holds more streams (RCCL's, after init_process_group) the side stream can land on the
  // caller's queue -- the two tails then run one after the other again (measured: 3.44 -> 3.65 ms per cfg2
  // step under torchrun).  Priority classes have their own queues.
  int least = 0, greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (hipStreamCreateWithPriority(&f.side, hipStreamNonBlocking, greatest) != hipSuccess) return false;
  if (hipEventCreateWithFlags(&f.fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&f.join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&f.bias, hipEventDisableTiming) != hipSuccess)
    return false;
  g_forks.push_back({{dev, stream}, f});
  *out = f;
  return true;
}
// MDCONV_BWD_FORK = 0 / 1: run the grad_input gather beside GEMM-2 on a forked stream (read once).
// On by default: cfg2 3.68 -> 3.40 ms per step (GEMM-2 1.06 -> 1.10 ms, the 0.33 ms of CSR build +
// gather disappear under it); round 1 had measured a loss with the NCHW GEMM-2, whose gathers kept
// the L2 as busy as the col2im gather does -- the channels-last GEMM-2 leaves the L2 mostly idle.
int bwd_fork_mode() {
  static const int on = getenv("MDCONV_BWD_FORK") ? atoi(getenv("MDCONV_BWD_FORK")) : 1;
  return on;
}
bool bwd_fork_enabled() { return bwd_fork_mode() != 0; }

// fp32 backward of one chunk (all kernels accumulate into the grad_* pointers of `t`).
// Order on the caller's stream:
//   pack_wq, zero counters
//   -> GEMM-1 (+ coordinate gradients, grad_col, and for GEMM-2: packed grad_out, tap table,
//      grad_bias partials; CSR counting pass)
//   -> GEMM-2, split-K reduce, grad_bias -> [weights-ready event] -> CSR scan + fill -> col2im
// grad_weight / grad_bias are produced BEFORE the grad_input gather so that a data-parallel
// all-reduce of them can run under the gather (mdconv_stream_wait_weight_ready).
// The grad_input gather (CSR scan + fill -> col2im, HBM-bound) shares nothing with GEMM-2 (matrix-bound)
// and runs beside it on a forked stream that re-joins before this function returns (get_fork).
// `bd`: the layout the plan sized the workspace with for this chunk size (Plan::bd / bd_tail).
// `skip`: the tail of a gradient the call leaves out is not enqueued (and with one tail, or none, nothing is forked);
// GEMM-1 runs as it is -- its side products for the skipped tail (packed grad_out, tap table and grad_bias partials for
// GEMM-2; grad_col rows and counters for the gather) go to the workspace and are left there.
int backward_chunk_f32(const Geom &g, const BwdDims &bd, const Tensors &t, char *base, hipStream_t stream,
                       bool weights_final, Skip skip) {
  float *wq = (float *)(base + bd.off_wq);
  float *ga = (float *)(base + bd.off_ga);
  int *table = (int *)(base + bd.off_table);
  float *part = (float *)(base + bd.off_part);
  float *gcol = (float *)(base + bd.off_gcol);
  int *cnt = (int *)(base + bd.off_cnt), *rowptr = (int *)(base + bd.off_rowptr);
  void *entries = base + bd.off_entries;
  int rc;
  float *bias_part = g.with_bias ? (float *)(base + bd.off_bias) : nullptr;
  float *bstage = g.with_bias ? (float *)(base + bd.off_bstage) : nullptr;
  // channels-last copy of the input for the 3-D gathers of GEMM-1's drain and of GEMM-2
  float *xt = bd.cl ? (float *)(base + bd.off_xt) : nullptr;
  // pack_wq, counter clearing and the layout pass: one launch
  if ((rc = bwd_prep_f32(g, bd, (const float *)t.weight, wq, cnt, (const float *)t.input, xt, stream))) return rc;
  profile_mark(1, true, stream, "mfma_bwd_data_kernel");
  rc = mfma_bwd_data_f32(g, bd, t, wq, gcol, ga, bias_part, cnt, table, xt, stream);
  profile_mark(1, false, stream);
  if (rc) return rc;
  Fork fk;
  const bool fork = !skip.input && !skip.weight && bwd_fork_enabled() && get_fork(stream, &fk);
  hipStream_t gs = stream;   // stream of the grad_input gather
  // GEMM-2 + split-K reduction; grad_bias behind them unless the forked stream already took it
  auto gemm2 = [&](bool bias_here) {
    int r = mfma_bwd_weight_f32(g, bd, t, ga, table, part, bias_part, xt, stream);
    if (!r && bias_here) r = grad_bias_f32(g, bd, bias_part, bstage, (float *)t.grad_bias, stream);
    if (!r && !bias_here && g.with_bias && hipStreamWaitEvent(stream, fk.bias, 0) != hipSuccess) {
      set_error("backward fork failed");
      r = MDCONV_ELAUNCH;
    }
    if (!r && weights_final) r = record_weight_ready(stream);
    return r;
  };
  if (fork) {
    if (hipEventRecord(fk.fork, stream) != hipSuccess || hipStreamWaitEvent(fk.side, fk.fork, 0) != hipSuccess) {
      set_error("backward fork failed");
      return MDCONV_ELAUNCH;
    }
    gs = fk.side;
  } else if (!skip.weight) {
    if ((rc = gemm2(true))) return rc;
  }
  if (skip.input) return MDCONV_OK;
  const bool gemm2_first = fork && bwd_fork_mode() == 2;   // (experiment: GEMM-2 enqueued before the gather)
  rc = MDCONV_OK;
  // forked: grad_bias first on the side stream (beside GEMM-2, off the critical path), its event for the caller's stream
  if (fork && g.with_bias) {
    rc = grad_bias_f32(g, bd, bias_part, bstage, (float *)t.grad_bias, gs);
    if (!rc && hipEventRecord(fk.bias, gs) != hipSuccess) { set_error("backward fork failed"); rc = MDCONV_ELAUNCH; }
  }
  if (!rc && gemm2_first) rc = gemm2(false);
  if (!rc) rc = csr_build_f32(g, bd, t, cnt, rowptr, entries, gs);
  // deterministic mode: the lists in canonical order before the gather sums them (on the gather's stream)
  if (!rc && g.det)
    rc = csr_sort_rows(rowptr, entries, base + bd.off_sort, bd.sample_keyed ? 2 : 1, bd.S_e,
                       (int64_t)g.K * g.S_o * (bd.sample_keyed ? 1 : (1 << g.nd) / 2), g.B * g.DG, gs);
  if (!rc) {
    profile_mark(3, true, gs, bd.sample_keyed ? (bd.two_pass ? "col2im3d_sums_kernel" : "col2im3d_kernel") : "col2im_gather_kernel");
    rc = col2im_f32(g, bd, t, gcol, rowptr, entries, (float *)(base + bd.off_sums), gs);
    profile_mark(3, false, gs);
  }
  if (fork) {
    if (!rc && !gemm2_first) rc = gemm2(false);
    // join on every path after the fork (error returns included): the side stream must not outlive the call
    if ((hipEventRecord(fk.join, fk.side) != hipSuccess || hipStreamWaitEvent(stream, fk.join, 0) != hipSuccess) && !rc) {
      set_error("backward join failed");
      rc = MDCONV_ELAUNCH;
    }
  }
  return rc;
}

}  // namespace

// fork / join for the other kernel families (hp_host.hip): side stream that waits for everything enqueued on
// `stream` so far, or nullptr when forking is off or unavailable; join makes `stream` wait for the side stream
hipStream_t fork_side_stream(hipStream_t stream) {
  Fork fk;
  if (!bwd_fork_enabled() || !get_fork(stream, &fk)) return nullptr;
  if (hipEventRecord(fk.fork, stream) != hipSuccess || hipStreamWaitEvent(fk.side, fk.fork, 0) != hipSuccess) return nullptr;
  return fk.side;
}
int join_side_stream(hipStream_t stream) {
  Fork fk;
  if (!get_fork(stream, &fk)) return MDCONV_ELAUNCH;
  if (hipEventRecord(fk.join, fk.side) != hipSuccess || hipStreamWaitEvent(stream, fk.join, 0) != hipSuccess) {
    set_error("backward join failed");
    return MDCONV_ELAUNCH;
  }
  return MDCONV_OK;
}

bool native_plan(const Geom &g, int dtype, bool backward, Plan *p, Skip skip) {
  if (dtype != MDCONV_F32 && dtype != MDCONV_F16 && dtype != MDCONV_BF16) return false;
  if (g.in_sz[g.nd - 1] < 2) return false;   // paired-corner gathers need 2 columns
  if (!backward) {
    if (g.Cg < 16 || g.Og < 16) return false;  // MFMA tiles would be mostly padding
    if (!(g.DG == 1 || (g.Cdg % (2 * kBK) == 0 && g.Cg % (2 * kBK) == 0))) return false;
  } else {
    // conv groups run as a block-diagonal dense weight (GEMM-1 skips the empty o-chunks, GEMM-2
    // the empty waves); deformable groups must be whole 64-channel blocks
    if (g.C < 16 || g.O < 16 || g.C % 8) return false;
    if (!(g.DG == 1 || g.Cdg == 64 || g.Cdg == 128 || g.Cdg % 256 == 0)) return false;
  }
  if (!make_plan(g, dtype, backward, skip, p)) return false;   // one image must fit 32-bit buffer offsets
  // the grad_out tile of GEMM-1 lives in LDS: sized for the whole call's pixel count (a single chunk: its own layout)
  return !backward || bwd_data_lds_bytes(g, p->Bc == g.B ? p->bd : bwd_dims(g)) <= kBwdDataLdsCap;
}

int native_forward(const Geom &g, int dtype, const Plan &p, const Tensors &t, void *ws, hipStream_t stream) {
  char *base = (char *)ws;
  const size_t es = p.half_io ? 2 : 4;
  const int nc_off = g.DG * g.nd * g.K, nc_m = g.DG * g.K;
  int rc;
  const float *w32 = (const float *)t.weight, *b32 = (const float *)t.bias;
  if (p.half_io) {
    if ((rc = widen(dtype, t.weight, (float *)(base + p.off_w), (int64_t)g.O * g.Cg * g.K, stream))) return rc;
    if (g.with_bias && (rc = widen(dtype, t.bias, (float *)(base + p.off_b), g.O, stream))) return rc;
    w32 = (const float *)(base + p.off_w);
    b32 = (const float *)(base + p.off_b);
  }
  const PackDims pd = pack_dims(p.gc);
  float *wp = (float *)base;
  if ((rc = pack_weights_f32(p.gc, pd, w32, wp, nullptr, stream))) return rc;
  for (int b0 = 0; b0 < g.B; b0 += p.Bc) {
    const int bc = g.B - b0 < p.Bc ? g.B - b0 : p.Bc;
    const Geom gc = chunk_geom(g, bc);
    Tensors tc = {};
    const char *x = (const char *)t.input + (size_t)b0 * g.C * g.S_i * es;
    const char *of = (const char *)t.offset + (size_t)b0 * nc_off * g.S_o * es;
    const char *mk = t.mask ? (const char *)t.mask + (size_t)b0 * nc_m * g.S_o * es : nullptr;
    char *out = (char *)t.output + (size_t)b0 * g.O * g.S_o * es;
    tc.weight = w32;
    tc.bias = b32;
    if (p.half_io) {
      if ((rc = widen(dtype, x, (float *)(base + p.off_x), (int64_t)bc * g.C * g.S_i, stream))) return rc;
      if ((rc = widen(dtype, of, (float *)(base + p.off_off), (int64_t)bc * nc_off * g.S_o, stream))) return rc;
      if (mk && (rc = widen(dtype, mk, (float *)(base + p.off_m), (int64_t)bc * nc_m * g.S_o, stream))) return rc;
      tc.input = base + p.off_x;
      tc.offset = base + p.off_off;
      tc.mask = mk ? base + p.off_m : nullptr;
      tc.output = base + p.off_out;
    } else {
      tc.input = x; tc.offset = of; tc.mask = mk; tc.output = out;
    }
    profile_mark(0, true, stream, fwd_channels_last(gc) ? "mfma_fwd_cl_kernel" : "mfma_fwd_kernel");
    if (fwd_channels_last(gc)) {
      float *xt = (float *)(base + align_up((size_t)gc.G * gc.K * pd.Cgp * pd.Ogp * sizeof(float)));
      float *part = (float *)((char *)xt + align_up(fwd_cl_bytes(gc)));
      rc = mfma_forward_cl_f32(gc, pd, tc, wp, fwd_tail_bytes(gc) ? part : nullptr, xt, stream);
    } else {
      float *part = (float *)(base + align_up((size_t)gc.G * gc.K * pd.Cgp * pd.Ogp * sizeof(float)));
      rc = mfma_forward_f32(gc, pd, tc, wp, fwd_tail_bytes(gc) ? part : nullptr, stream);
    }
    profile_mark(0, false, stream);
    if (rc) return rc;
    if (p.half_io && (rc = narrow(dtype, (const float *)tc.output, out, (int64_t)bc * g.O * g.S_o, false, stream)))
      return rc;
  }
  return MDCONV_OK;
}

int native_backward(const Geom &g, int dtype, const Plan &p, const Tensors &t, void *ws, hipStream_t stream) {
  char *base = (char *)ws;
  const Skip skip = p.skip;
  const size_t es = p.half_io ? 2 : 4;
  const int nc_off = g.DG * g.nd * g.K, nc_m = g.DG * g.K;
  const int64_t n_w = (int64_t)g.O * g.Cg * g.K;
  int rc;
  if (p.half_io) {
    if ((rc = widen(dtype, t.weight, (float *)(base + p.off_w), n_w, stream))) return rc;
  }
  for (int b0 = 0; b0 < g.B; b0 += p.Bc) {
    const int bc = g.B - b0 < p.Bc ? g.B - b0 : p.Bc;
    Geom gc = chunk_geom(g, bc);
    const BwdDims &bd = bc == p.Bc ? p.bd : p.bd_tail;
    // grad_weight / grad_bias: chunks after the first always add; the fp32 temporaries of the fp16
    // path are fresh memory, so every kernel overwrites them (no zero fills) and the caller's mode
    // is applied when they are narrowed back
    gc.acc_w = (b0 > 0) ? 1 : (p.half_io ? 0 : g.acc_w);
    gc.acc_data = p.half_io ? 0 : g.acc_data;
    const size_t o_x = (size_t)b0 * g.C * g.S_i, o_off = (size_t)b0 * nc_off * g.S_o;
    const size_t o_m = (size_t)b0 * nc_m * g.S_o, o_go = (size_t)b0 * g.O * g.S_o;
    Tensors tc = t;
    if (p.half_io) {
      const int64_t n_x = (int64_t)bc * g.C * g.S_i, n_off = (int64_t)bc * nc_off * g.S_o;
      const int64_t n_m = (int64_t)bc * nc_m * g.S_o, n_go = (int64_t)bc * g.O * g.S_o;
      if ((rc = widen(dtype, (const char *)t.input + o_x * es, (float *)(base + p.off_x), n_x, stream))) return rc;
      if ((rc = widen(dtype, (const char *)t.offset + o_off * es, (float *)(base + p.off_off), n_off, stream))) return rc;
      if (t.mask && (rc = widen(dtype, (const char *)t.mask + o_m * es, (float *)(base + p.off_m), n_m, stream))) return rc;
      if ((rc = widen(dtype, (const char *)t.grad_output + o_go * es, (float *)(base + p.off_go), n_go, stream))) return rc;
      tc.input = base + p.off_x; tc.offset = base + p.off_off; tc.mask = t.mask ? base + p.off_m : nullptr;
      tc.weight = base + p.off_w; tc.grad_output = base + p.off_go;
      tc.grad_input = skip.input ? nullptr : base + p.off_gi; tc.grad_offset = base + p.off_goff;
      tc.grad_mask = t.grad_mask ? base + p.off_gm : nullptr;
      tc.grad_weight = skip.weight ? nullptr : base + p.off_gw; tc.grad_bias = skip.weight ? nullptr : base + p.off_gb;
      if ((rc = backward_chunk_f32(gc, bd, tc, base, stream, false, skip))) return rc;
      if (!skip.input &&
          (rc = narrow(dtype, (const float *)tc.grad_input, (char *)t.grad_input + o_x * es, n_x, g.acc_data != 0, stream)))
        return rc;
      if ((rc = narrow(dtype, (const float *)tc.grad_offset, (char *)t.grad_offset + o_off * es, n_off, g.acc_data != 0, stream))) return rc;
      if (t.grad_mask &&
          (rc = narrow(dtype, (const float *)tc.grad_mask, (char *)t.grad_mask + o_m * es, n_m, g.acc_data != 0, stream)))
        return rc;
    } else {
      tc.input = (const char *)t.input + o_x * es;
      tc.offset = (const char *)t.offset + o_off * es;
      tc.mask = t.mask ? (const char *)t.mask + o_m * es : nullptr;
      tc.grad_output = (const char *)t.grad_output + o_go * es;
      tc.grad_input = skip.input ? nullptr : (char *)t.grad_input + o_x * es;
      tc.grad_offset = (char *)t.grad_offset + o_off * es;
      tc.grad_mask = t.grad_mask ? (char *)t.grad_mask + o_m * es : nullptr;
      if ((rc = backward_chunk_f32(gc, bd, tc, base, stream, b0 + bc >= g.B, skip))) return rc;
    }
  }
  if (p.half_io && !skip.weight) {
    // (fp32 grad_weight / grad_bias, t.wgrad32: the sums as they are, copied or added)
    if ((rc = narrow_wgrad(dtype, t, (const float *)(base + p.off_gw), t.grad_weight, n_w, g.acc_w != 0, stream))) return rc;
    if (g.with_bias && (rc = narrow_wgrad(dtype, t, (const float *)(base + p.off_gb), t.grad_bias, g.O, g.acc_w != 0, stream)))
      return rc;
    if ((rc = record_weight_ready(stream))) return rc;
  }
  return MDCONV_OK;
}

}  // namespace mdconv
