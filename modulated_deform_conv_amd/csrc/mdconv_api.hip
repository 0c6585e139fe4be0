// mdconv_api.hip -- the convolution API of the C ABI (include/mdconv.h): descriptor validation, path selection, and the
// eight entry points that replace the reference's MDCONV_CUDA exports
// (mdeformable_conv.cu:460-465 registers two; modulated_deform_conv.py calls all eight:
//  :28, :57, :112, :142, :194, :225, :281, :313); and what the whole library has once: the thread-local error text
// (set_error, mdconv_last_error) and check_launch.  The sampling operators' entry points live beside their planners in the
// operators' *_host.hip, on the entry-point layer of samp_api.hpp, whose pointer checks the entry points here use too.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <iterator>
#include <map>
#include <mutex>
#include <utility>

#include "mdconv_common.hpp"
#include "dw_plan.hpp"
#include "hp_plan.hpp"
#include "mfma_plan.hpp"
#include "samp_api.hpp"   // require, require_aligned, check_ws

namespace mdconv {

static thread_local char g_err[512] = "";
static thread_local int g_last_path = 0;
static thread_local int g_last_kernels = 0;
static thread_local int g_last_geometry = 0;   // MDCONV_GEOMETRY_* of the fp32 matrix kernels the last call launched
// ABI v1 call modes (descriptors without MDCONV_DESC_V2); v2 descriptors carry their own
static thread_local int g_accumulate = 1;
static thread_local int g_input_layout = 0;   // MDCONV_LAYOUT_*
// "grad_weight / grad_bias are final" events: one per (device, producer stream), shared by all
// host threads (autograd runs the backward on its own worker thread), plus the most recent one per
// device for the stream-less legacy query
static std::mutex g_wready_mu;
struct WReady { hipEvent_t ev; unsigned long long tick; };
static std::map<std::pair<int, hipStream_t>, WReady> g_wready;
static std::map<int, hipEvent_t> g_wready_latest;
static unsigned long long g_wready_tick = 0;
constexpr size_t kWReadyMax = 64;   // streams remembered per process; least recently used are dropped
static std::atomic<int> g_path{-1};  // -1 = not initialised from the environment yet

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: HIP launch failed: %s", what, hipGetErrorString(e));
    return MDCONV_ELAUNCH;
  }
  return MDCONV_OK;
}

static int current_path() {
  int p = g_path.load(std::memory_order_relaxed);
  if (p < 0) {
    const char *e = getenv("MDCONV_PATH");
    p = MDCONV_PATH_AUTO;
    if (e && !strcmp(e, "direct")) p = MDCONV_PATH_DIRECT;
    if (e && !strcmp(e, "mfma")) p = MDCONV_PATH_MFMA;
    if (e && !strcmp(e, "depthwise")) p = MDCONV_PATH_DEPTHWISE;
    int expect = -1;
    g_path.compare_exchange_strong(expect, p);
    p = g_path.load();
  }
  return p;
}

static int desc_ndim(const mdconv_desc *d) { return d->ndim & ~MDCONV_DESC_V2; }

// Call modes of one call: from the descriptor (ABI v2) or from the v1 setters of the calling thread / process.
// math_bf16: MDCONV_FLAG_MATH_BF16 -- the fp32 call may run on the bf16 kernels (plan_call decides whether it does)
// out_cl / gi_cl: MDCONV_FLAG_OUTPUT_CHANNELS_LAST / MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST (16-bit tensors only)
struct Modes { int accumulate, input_layout, path, deterministic, math_bf16; Skip skip; int out_cl, gi_cl; };
static int call_modes(const mdconv_desc *d, Modes *m) {
  m->deterministic = m->math_bf16 = m->out_cl = m->gi_cl = 0;   // v1 descriptors end before the flag word: they never request a flag
  m->skip = Skip();
  if (!(d->ndim & MDCONV_DESC_V2)) {
    m->accumulate = g_accumulate;
    m->input_layout = g_input_layout;
    m->path = current_path();
    return MDCONV_OK;
  }
  if ((d->accumulate != 0 && d->accumulate != 1) ||
      (d->input_layout != MDCONV_LAYOUT_NCHW && d->input_layout != MDCONV_LAYOUT_CHANNELS_LAST) ||
      d->path < MDCONV_PATH_AUTO || d->path > MDCONV_PATH_DEPTHWISE) {
    set_error("bad call mode in the descriptor (accumulate=%d, input_layout=%d, path=%d)", d->accumulate,
              d->input_layout, d->path);
    return MDCONV_EINVAL;
  }
  for (int i = 0; i < 4; ++i)
    if (d->reserved[i] != 0) {
      set_error("mdconv_desc.reserved must be 0");
      return MDCONV_EINVAL;
    }
  const int layouts = MDCONV_FLAG_OUTPUT_CHANNELS_LAST | MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST;
  const int known = MDCONV_FLAG_DETERMINISTIC | MDCONV_FLAG_NO_GRAD_INPUT | MDCONV_FLAG_NO_GRAD_WEIGHT | MDCONV_FLAG_MATH_BF16 | layouts;
  if (d->reserved[4] & ~known) {
    set_error("unknown bits 0x%x in the flags word of the descriptor (mdconv_desc.reserved[4]); the flags are "
              "MDCONV_FLAG_DETERMINISTIC (1), MDCONV_FLAG_NO_GRAD_INPUT (4), MDCONV_FLAG_NO_GRAD_WEIGHT (8), "
              "MDCONV_FLAG_MATH_BF16 (32), MDCONV_FLAG_OUTPUT_CHANNELS_LAST (64) and MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST (128)",
              (unsigned)(d->reserved[4] & ~known));
    return MDCONV_EINVAL;
  }
  if (d->reserved[4] & layouts) {
    const int dt = d->dtype & ~(MDCONV_SAMPLING_F32 | MDCONV_WGRAD_F32);   // (fill_geom has validated the dtype word)
    if (dt != MDCONV_F16 && dt != MDCONV_BF16) {
      set_error("%s needs fp16 or bf16 tensors, dtype is %s (fp32 tensors under MDCONV_FLAG_MATH_BF16 included)",
                (d->reserved[4] & MDCONV_FLAG_OUTPUT_CHANNELS_LAST) ? "MDCONV_FLAG_OUTPUT_CHANNELS_LAST" : "MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST",
                dt == MDCONV_F64 ? "MDCONV_F64" : "MDCONV_F32");
      return MDCONV_EINVAL;
    }
    m->out_cl = (d->reserved[4] & MDCONV_FLAG_OUTPUT_CHANNELS_LAST) ? 1 : 0;
    m->gi_cl = (d->reserved[4] & MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST) ? 1 : 0;
  }
  if (d->reserved[4] & MDCONV_FLAG_MATH_BF16) {
    const int dt = d->dtype & ~(MDCONV_SAMPLING_F32 | MDCONV_WGRAD_F32);   // (fill_geom has validated the dtype word)
    if (dt != MDCONV_F32) {
      set_error("MDCONV_FLAG_MATH_BF16 needs fp32 tensors, dtype is %s",
                dt == MDCONV_F64 ? "MDCONV_F64" : (dt == MDCONV_F16 ? "MDCONV_F16" : "MDCONV_BF16"));
      return MDCONV_EINVAL;
    }
    m->math_bf16 = 1;
  }
  m->deterministic = (d->reserved[4] & MDCONV_FLAG_DETERMINISTIC) ? 1 : 0;
  m->skip.input = (d->reserved[4] & MDCONV_FLAG_NO_GRAD_INPUT) != 0;
  m->skip.weight = (d->reserved[4] & MDCONV_FLAG_NO_GRAD_WEIGHT) != 0;
  m->accumulate = d->accumulate;
  m->input_layout = d->input_layout;
  m->path = d->path == MDCONV_PATH_AUTO ? current_path() : d->path;
  return MDCONV_OK;
}

int fill_geom(const mdconv_desc *d, Geom *g) {
  if (!d) {
    set_error("descriptor is NULL");
    return MDCONV_ENULL;
  }
  const int ndim = desc_ndim(d);
  if (ndim != 2 && ndim != 3) {
    set_error("ndim must be 2 or 3 (got %d)", ndim);
    return MDCONV_EINVAL;
  }
  const int dt = d->dtype & ~(MDCONV_SAMPLING_F32 | MDCONV_WGRAD_F32);
  if (dt != MDCONV_F32 && dt != MDCONV_F16 && dt != MDCONV_F64 && dt != MDCONV_BF16) {
    set_error("unsupported dtype %d", d->dtype);
    return MDCONV_EINVAL;
  }
  if ((d->dtype & MDCONV_SAMPLING_F32) && dt != MDCONV_F16 && dt != MDCONV_BF16) {
    set_error("MDCONV_SAMPLING_F32 needs fp16 or bf16 tensors, dtype is %s", dt == MDCONV_F32 ? "MDCONV_F32" : "MDCONV_F64");
    return MDCONV_EINVAL;
  }
  if ((d->dtype & MDCONV_WGRAD_F32) && dt != MDCONV_F16 && dt != MDCONV_BF16) {
    set_error("MDCONV_WGRAD_F32 needs fp16 or bf16 tensors, dtype is %s", dt == MDCONV_F32 ? "MDCONV_F32" : "MDCONV_F64");
    return MDCONV_EINVAL;
  }
  if (d->batch <= 0 || d->c_in <= 0 || d->c_out <= 0 || d->groups <= 0 || d->dgroups <= 0) {
    set_error("batch/channels/groups must be positive");
    return MDCONV_EINVAL;
  }
  if (d->in_step <= 0) {  // the reference divides by it (config.h:43-60)
    set_error("in_step must be positive (got %d)", d->in_step);
    return MDCONV_EINVAL;
  }
  if (d->c_in % d->groups || d->c_out % d->groups) {
    set_error("Input shape and kernel channels wont match: channels %d / %d not divisible by group %d",
              d->c_in, d->c_out, d->groups);
    return MDCONV_EINVAL;
  }
  if (d->c_in % d->dgroups) {
    set_error("channels %d not divisible by deformable_group %d", d->c_in, d->dgroups);
    return MDCONV_EINVAL;
  }
  memset(g, 0, sizeof(*g));
  g->nd = ndim;
  g->B = d->batch;
  g->C = d->c_in;
  g->O = d->c_out;
  g->G = d->groups;
  g->DG = d->dgroups;
  int64_t S_i = 1, S_o = 1, K = 1;
  for (int a = 0; a < 3; ++a) {
    const bool used = a < ndim;
    const int n = used ? d->in_sz[a] : 1, k = used ? d->k_sz[a] : 1, s = used ? d->stride[a] : 1;
    const int p = used ? d->pad[a] : 0, dl = used ? d->dil[a] : 1;
    if (n <= 0 || k <= 0 || s <= 0 || dl <= 0 || p < 0) {
      set_error("bad size/kernel/stride/dilation/padding on axis %d", a);
      return MDCONV_EINVAL;
    }
    const int o = (n + 2 * p - (dl * (k - 1) + 1)) / s + 1;
    if (n + 2 * p - (dl * (k - 1) + 1) < 0 || o <= 0) {
      set_error("empty output on axis %d", a);
      return MDCONV_EINVAL;
    }
    g->in_sz[a] = n;
    g->ksz[a] = k;
    g->stride[a] = s;
    g->pad[a] = p;
    g->dil[a] = dl;
    g->out_sz[a] = o;
    S_i *= n;
    S_o *= o;
    K *= k;
  }
  const int64_t lim = 0x7fffffffLL;
  if (S_i > lim || S_o * d->batch > lim || K > 4096 ||
      (int64_t)d->batch * d->c_in * S_i > (int64_t)1 << 40) {
    set_error("tensor too large for 32-bit pixel indexing");
    return MDCONV_EUNSUPPORTED;
  }
  g->S_i = (int)S_i;
  g->S_o = (int)S_o;
  g->K = (int)K;
  g->N = (int)(S_o * d->batch);
  g->Cg = d->c_in / d->groups;
  g->Og = d->c_out / d->groups;
  g->Cdg = d->c_in / d->dgroups;
  g->with_bias = d->with_bias ? 1 : 0;
  g->modulated = d->modulated ? 1 : 0;
  g->acc_data = g->acc_w = 1;
  // gating flavours of the four reference files
  const bool mdcn2d = ndim == 2 && d->modulated;
  const bool dcn2d = ndim == 2 && !d->modulated;
  g->load_eps = mdcn2d ? 0 : 1;
  g->atom_eps = dcn2d ? 0 : 1;
  g->range_gate = mdcn2d ? 1 : 0;
  return MDCONV_OK;
}

// One line on stderr, once per process, when a shape with matrix-sized channel counts runs on the
// shape-generic VALU kernels (an order of magnitude slower than the matrix-core kernels): nothing else tells the user
// (mdconv_last_kernels() reports it per call; MDCONV_QUIET=1 silences the line).
static void note_direct_fallback(const Geom &g, int dtype, bool backward, int path) {
  static std::atomic<bool> said{false};
  if (g.Cg < 16 || g.Og < 16 || dtype == MDCONV_F64 || path == MDCONV_PATH_DIRECT) return;
  if (!backward && g.Cg < 64) return;   // narrow conv groups: the shape-generic forward is no slower (mfma_plans.hip)
  if (said.exchange(true)) return;
  const char *q = getenv("MDCONV_QUIET");
  if (q && atoi(q) != 0) return;
  fprintf(stderr,
          "mdconv: %s of a %d-D shape with C_in=%d C_out=%d groups=%d deformable_groups=%d runs on the shape-generic "
          "kernels (the matrix-core kernels need %s); expect it to be ~10x slower. This note is printed once.\n",
          backward ? "backward" : "forward", g.nd, g.C, g.O, g.G, g.DG,
          "with several deformable groups: one conv group and C_in/deformable_groups of at least 8, or with conv groups "
          "C_in/deformable_groups a multiple of 8, at least 16, aligned with them");
}

// element type of the call's tensors (the dtype flags stripped), whether offset / mask are fp32, and whether a backward's
// grad_weight / grad_bias are (the forward ignores that bit: one descriptor serves both directions)
static int base_dtype(const mdconv_desc *d) { return d->dtype & ~(MDCONV_SAMPLING_F32 | MDCONV_WGRAD_F32); }
static int sampling_f32(const mdconv_desc *d) { return (d->dtype & MDCONV_SAMPLING_F32) ? 1 : 0; }
static int wgrad_f32(const mdconv_desc *d, bool backward) { return backward && (d->dtype & MDCONV_WGRAD_F32) ? 1 : 0; }

// ---------------------------------------------------------------------------------------------
// The plan of one call: the kernel family it runs on, the copies it runs through and its workspace -- the one routing
// decision, made by plan_call() and read by run_forward / run_backward, mdconv_workspace_bytes,
// mdconv_deterministic_supported and mdconv_input_layout_supported.
// ---------------------------------------------------------------------------------------------
enum Route {
  ROUTE_DW,              // depthwise kernels (fp32, groups == C_in)
  ROUTE_HP,              // native 16-bit kernels
  ROUTE_HP_F32,          // ... bf16 instances of them for fp32 tensors (MDCONV_FLAG_MATH_BF16): fp32 in and out, `hp` made for it
  ROUTE_F32,             // fp32 matrix kernels (16-bit tensors: chunk-wise fp32 copies inside the family)
  ROUTE_F32_SAMP32,      // ... through the fp32 copies of a call with fp32 offsets / masks (`s32`)
  ROUTE_DIRECT,          // shape-generic kernels
  ROUTE_DIRECT_16,       // ... 16-bit backward through fp32 copies (`d16`)
  ROUTE_DIRECT_SAMP32    // ... through the fp32 copies of a call with fp32 offsets / masks (`s32`)
};
// A call can be refused; `route` and the byte counts then still say where it would have gone (the sizing query reports them).
enum Refusal { REFUSE_NONE, REFUSE_CHANNELS_LAST, REFUSE_PATH_MFMA, REFUSE_DETERMINISTIC, REFUSE_RESULT_LAYOUT, REFUSE_PATH_DEPTHWISE };
struct CallPlan {
  Route route;
  Refusal refused;
  size_t bytes;      // workspace the route needs
  size_t reported;   // what mdconv_workspace_bytes answers: `bytes`, but see the few-tile forwards in plan_call
  DwPlan dw;         // ROUTE_DW
  const char *dw_reason;   // REFUSE_PATH_DEPTHWISE: the rule of the family the call breaks
  HpPlan hp;         // ROUTE_HP, ROUTE_HP_F32
  MfmaPlan f32;      // ROUTE_F32
  S32Plan s32;       // ROUTE_*_SAMP32
  D16Plan d16;       // ROUTE_DIRECT_16
  Skip skip;         // backward: gradients the call leaves out
  size_t scratch_gi; // ROUTE_DIRECT with skip.input: bytes of the grad_input scratch (the route's whole workspace)
  const char *layout_reason;   // REFUSE_RESULT_LAYOUT: the rule the flagged call breaks
};
static bool route_is_direct(Route r) { return r == ROUTE_DIRECT || r == ROUTE_DIRECT_16 || r == ROUTE_DIRECT_SAMP32; }

// `g` with in_cl and det set; `dt` the tensors' element type, `s32` fp32 offsets / masks, `path` the caller's MDCONV_PATH_*.
// `wg32` (fp32 grad_weight / grad_bias of a 16-bit backward) never changes the route: only the fp32 matrix family's padded /
// sliced plans hold grad_weight rows in the caller's element size, and size them for it.
// `skip` (a backward without grad_input / without the weight gradients) never changes the route either: the plans drop the
// stages and workspace slots of the skipped gradients, and the shape-generic data kernel scatters an unwanted grad_input
// into scratch (CallPlan::scratch_gi, appended to the route's workspace).
// `mb16` (MDCONV_FLAG_MATH_BF16, fp32 tensors) is a permission: the call takes ROUTE_HP_F32 where its bf16 form is a native
// 16-bit call -- hp_plan takes it and, a forward, prefers it -- and is planned as without the flag everywhere else
// (MDCONV_PATH_DIRECT, an fp32 channels-last input, few-tile forwards, shapes outside hp_plan).
// One size rule on top, from measurement (profiles/math_bf16.md): layers of fewer than 16 input or 16 output channels are declined.
// The bf16 kernels pad channels to blocks of 32, and with the rule off such layers did not gain: DCN2d 4 -> 4 at 8 x 8 ran 0.121 ms
// against 0.089 ms exact, MDCN2d 8 -> 8 at 56 x 56, B = 8 0.224 against 0.229 (inside the +-3 % spread), 4 -> 4 there 0.222 against 0.238.
// Narrow CONV GROUPS of a wide layer are taken (256 -> 256 in 32 groups of 8, 56 x 56, B = 8: 0.33 against 0.97 ms).
// `out_cl` / `gi_cl` (the result-layout flags) never change the route either: hp_plan records them, and plan_call below refuses
// the flagged call the route does not honour.
// Depthwise layers come first: under MDCONV_PATH_AUTO a call dw_plan takes runs on the depthwise kernels -- but for the one size
// rule of dw_declined_by_size above -- with or without `mb16` -- the flag is a permission, and the family is exact; MDCONV_PATH_DEPTHWISE
// runs there or is refused with dw_plan's rule; MDCONV_PATH_DIRECT and MDCONV_PATH_MFMA never look at the family.
// The one size rule of the depthwise family under MDCONV_PATH_AUTO, from measurement (profiles/depthwise.md, the `rule_*` rows;
// step times in ms, earlier route against the family).  With several deformable groups the earlier route is the shape-generic
// forward and the matrix backward, whose dense C x C GEMMs are tiled natively where C_in / deformable_groups is a multiple of 64:
// cheap while C_in is small, and faster than the family's list build and gather from a few thousand pixels.  Declined, in both
// directions and whatever the flags: deformable_groups > 1, C_in / deformable_groups a multiple of 64, C_in <= 256 and at
// least 4096 output pixels -- 128 channels in 2 groups at 6272 / 9408 / 25088 pixels 0.17 / 0.21 / 0.36 against 0.18 / 0.24 / 0.50;
// 256 in 4 groups at 6272 / 25088 pixels 0.23 / 0.70 against 0.28 / 0.91.  Taken, because they gain or tie: 256 in 4 groups at 1568
// pixels (0.145 against 0.123), 512 channels at every size measured (8 groups of 64: 0.21 against 0.15 at 1568 pixels, 0.89 against
// 0.92 at 12544, inside the 5 % spread; 2 groups of 256: 0.45 against 0.40 at 6272, 1.66 against 1.55 at 25088), groups of 16 / 32
// channels (0.71 against 0.23, 0.48 against 0.32, 2.20 against 1.72, 3-D 2.15 against 1.48), and every layer with ONE deformable
// group, which the matrix family pads to 16 channels per conv group (256 -> 256 at 56 x 56, B = 8: 4.21 against 0.74).
static bool dw_declined_by_size(const Geom &g) { return g.DG > 1 && g.Cdg % 64 == 0 && g.C <= 256 && g.N >= 4096; }
static void plan_route(const Geom &g, int dt, int s32, int wg32, int path, bool backward, CallPlan *cp, Skip skip, int mb16,
                       bool out_cl, bool gi_cl) {
  const bool half = dt == MDCONV_F16 || dt == MDCONV_BF16;
  if (!backward) skip = Skip();
  cp->skip = skip;
  cp->scratch_gi = 0;
  cp->dw_reason = nullptr;
  if (path == MDCONV_PATH_AUTO || path == MDCONV_PATH_DEPTHWISE) {
    if (dw_plan(g, dt, backward, &cp->dw, skip, &cp->dw_reason) && !(path == MDCONV_PATH_AUTO && dw_declined_by_size(g))) {
      cp->route = ROUTE_DW;
      cp->refused = REFUSE_NONE;
      cp->bytes = cp->reported = cp->dw.total;
      return;
    }
    if (path == MDCONV_PATH_DEPTHWISE) {
      cp->route = ROUTE_DIRECT;
      cp->refused = REFUSE_PATH_DEPTHWISE;
      cp->bytes = cp->reported = 0;
      return;
    }
  }
  if (mb16 && dt == MDCONV_F32 && path != MDCONV_PATH_DIRECT && !g.in_cl && g.C >= 16 && g.O >= 16 &&
      hp_plan(g, MDCONV_BF16, backward, &cp->hp, skip, true) && cp->hp.forward_preferred) {
    cp->route = ROUTE_HP_F32;
    cp->refused = REFUSE_NONE;
    cp->bytes = cp->reported = cp->hp.total;
    return;
  }
  const bool hp = path != MDCONV_PATH_DIRECT && hp_plan(g, dt, backward, &cp->hp, skip, false, out_cl, gi_cl);
  cp->refused = g.in_cl && !(hp && g.C % 32 == 0) ? REFUSE_CHANNELS_LAST : REFUSE_NONE;
  const size_t hp_bytes = hp ? cp->hp.total : 0;
  // 16-bit forwards of a few tiles run faster on the fp32 kernels (HpPlan::forward_preferred)
  const bool few_tile = hp && !cp->hp.forward_preferred;
  if (hp && !few_tile) {
    cp->route = ROUTE_HP;
    cp->bytes = cp->reported = hp_bytes;
    return;
  }
  // fp32 sampling outside the native 16-bit kernels runs the fp32 kernels of the family the 16-bit call would take, so the
  // matrix family needs a plan for both dtypes
  bool mfma = false;
  if (path != MDCONV_PATH_DIRECT) {
    if (s32) {
      if (mfma_supported(g, dt, backward)) samp32_plan(g, backward, true, &cp->s32, skip), mfma = cp->s32.mfma;
    } else {
      mfma = mfma_plan(g, dt, backward, &cp->f32, wg32 != 0, skip);
    }
  }
  if (mfma) {
    cp->route = s32 ? ROUTE_F32_SAMP32 : ROUTE_F32;
    cp->bytes = s32 ? cp->s32.total : cp->f32.total;
  } else if (s32) {
    cp->route = ROUTE_DIRECT_SAMP32;
    samp32_plan(g, backward, false, &cp->s32, skip);
    cp->bytes = cp->s32.total;
  } else if (backward && half) {   // 16-bit atomics round at every add: fp32 copies for the scatter kernels
    cp->route = ROUTE_DIRECT_16;
    cp->d16 = direct16_plan(g);
    cp->bytes = cp->d16.total;
  } else {
    cp->route = ROUTE_DIRECT;
    // the fused data kernel scatters grad_input whether it is wanted or not: scratch of the tensor's size for it
    if (skip.input) cp->scratch_gi = (size_t)g.B * g.C * g.S_i * (dt == MDCONV_F64 ? 8 : (dt == MDCONV_F32 ? 4 : 2));
    cp->bytes = cp->scratch_gi;
  }
  cp->reported = cp->bytes;
  if (few_tile) {
    // ... unless the input is channels-last, which only the native kernels read in place -- and which a sizing query
    // made without the layout cannot know: the reported size is enough for either family
    if (hp_bytes > cp->reported) cp->reported = hp_bytes;
    if (g.in_cl) {
      cp->route = ROUTE_HP;
      cp->bytes = hp_bytes;
    }
  }
  if (cp->refused || !route_is_direct(cp->route)) return;
  if (path == MDCONV_PATH_MFMA) cp->refused = REFUSE_PATH_MFMA;
  else if (g.det) cp->refused = REFUSE_DETERMINISTIC;   // the shape-generic backward sums in arrival order
}
// The plan of a call: its route (plan_route), and the verdict on the result-layout flags -- honoured exactly where the native
// 16-bit plan takes this direction and the rows of every flagged tensor are whole 16-byte pieces (hp_plan's layout_refusal);
// any other flagged call is refused before anything is launched.  grad_input's flag: backward with grad_input only.
static void plan_call(const Geom &g, int dt, int s32, int wg32, int path, bool backward, CallPlan *cp, Skip skip = Skip(),
                      int mb16 = 0, bool out_cl = false, bool gi_cl = false) {
  cp->layout_reason = nullptr;
  gi_cl = gi_cl && backward && !skip.input;
  plan_route(g, dt, s32, wg32, path, backward, cp, skip, mb16, out_cl, gi_cl);
  if (cp->refused || !(out_cl || gi_cl)) return;
  if (cp->route != ROUTE_HP)
    cp->layout_reason = "the call does not run on the native 16-bit kernels (mdconv_last_kernels() would not be MDCONV_KERNELS_HP)";
  else
    cp->layout_reason = cp->hp.layout_refusal;
  if (cp->layout_reason) cp->refused = REFUSE_RESULT_LAYOUT;
}
static void set_layout_refusal(const CallPlan &cp, bool backward) {
  set_error("result layouts (MDCONV_FLAG_OUTPUT_CHANNELS_LAST / MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST): this %s cannot honour "
            "the flags -- %s", backward ? "backward" : "forward", cp.layout_reason);
}
// why a backward ends on the shape-generic kernels (the text of the deterministic-mode refusal)
static const char *direct_reason(const Geom &g, int dt, int path) {
  if (path == MDCONV_PATH_DIRECT) return "the call selects MDCONV_PATH_DIRECT";
  if (dt == MDCONV_F64) return "fp64 tensors have no matrix-core kernels";
  if (g.in_sz[g.nd - 1] < 2) return "the last input axis is shorter than 2 (the matrix-core gathers read column pairs)";
  if (g.C < 16 || g.O < 16 || g.C % 8)
    return "the matrix-core backward needs C_in and C_out of at least 16 and C_in a multiple of 8";
  if (g.DG > 1) return "the matrix-core backward needs C_in / deformable_groups of at least 8, aligned with the conv groups";
  return "the shape is outside the matrix-core backward (grad_out tile beyond the LDS, or one image beyond 32-bit offsets)";
}

static void set_det_refusal(const Geom &g, int dt, int path) {
  set_error("deterministic mode (MDCONV_FLAG_DETERMINISTIC): this backward would run on the shape-generic kernels, which "
            "scatter grad_input and grad_weight with floating-point atomics (sums in arrival order) -- %s",
            direct_reason(g, dt, path));
}

// the error of a refused call (nothing has been launched)
static int refuse(const CallPlan &cp, const Geom &g, int dt, int path, bool backward) {
  if (cp.refused == REFUSE_CHANNELS_LAST)
    set_error("channels-last input is only supported by the native 16-bit kernels with C_in a multiple of 32");
  else if (cp.refused == REFUSE_PATH_MFMA)
    set_error("MDCONV_PATH=mfma but this shape/dtype is not supported by the MFMA kernels");
  else if (cp.refused == REFUSE_RESULT_LAYOUT)
    set_layout_refusal(cp, backward);
  else if (cp.refused == REFUSE_PATH_DEPTHWISE)
    set_error("MDCONV_PATH=depthwise but the depthwise kernels do not take this call: %s", cp.dw_reason);
  else
    set_det_refusal(g, dt, path);
  return MDCONV_EUNSUPPORTED;
}

void note_geometry_variant(int v) { g_last_geometry = v; }

static int run_forward(const mdconv_desc *d, int nd, int modulated, Tensors t, void *ws,
                       size_t ws_bytes, void *stream) {
  g_err[0] = 0;
  g_last_geometry = 0;
  Geom g;
  int rc = fill_geom(d, &g);
  if (rc) return rc;
  if (g.nd != nd || (d->modulated != 0) != (modulated != 0)) {
    set_error("descriptor (ndim=%d, modulated=%d) does not match this entry point", g.nd,
              d->modulated);
    return MDCONV_EINVAL;
  }
  Modes md;
  if ((rc = call_modes(d, &md))) return rc;
  if ((rc = require(t.input, "input")) || (rc = require(t.weight, "weight")) ||
      (rc = require(t.offset, "offset")) || (rc = require(t.output, "output")))
    return rc;
  if (modulated && (rc = require(t.mask, "mask"))) return rc;
  if (g.with_bias && (rc = require(t.bias, "bias"))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int path = md.path;
  const int dt = base_dtype(d), s32 = sampling_f32(d);
  t.samp32 = s32;
  g.in_cl = md.input_layout == MDCONV_LAYOUT_CHANNELS_LAST ? 1 : 0;
  {   // pointer alignment: "element", but 16 bytes for the tensors the kernels move as channels-last vectors
    const size_t es = dtype_bytes(dt), es_s = s32 ? 4 : es;
    if ((rc = require_aligned(t.input, "input", g.in_cl ? 16 : es)) || (rc = require_aligned(t.weight, "weight", es)) ||
        (rc = require_aligned(t.offset, "offset", es_s)) || (rc = require_aligned(t.output, "output", md.out_cl ? 16 : es)))
      return rc;
    if (modulated && (rc = require_aligned(t.mask, "mask", es_s))) return rc;
    if (g.with_bias && (rc = require_aligned(t.bias, "bias", es))) return rc;
  }
  CallPlan cp;
  plan_call(g, dt, s32, 0, path, false, &cp, Skip(), md.math_bf16, md.out_cl != 0, false);
  if (cp.refused) return refuse(cp, g, dt, path, false);
  switch (cp.route) {
    case ROUTE_DW:   // no workspace
      g_last_path = MDCONV_PATH_DEPTHWISE;
      g_last_kernels = MDCONV_KERNELS_DEPTHWISE;
      return dw_forward(cp.dw, t, s);
    case ROUTE_HP_F32:   // the bf16 kernels on the caller's fp32 tensors
      if ((rc = check_ws(ws, ws_bytes, cp.bytes))) return rc;
      g_last_path = MDCONV_PATH_MFMA;
      g_last_kernels = MDCONV_KERNELS_HP;
      return hp_forward(MDCONV_BF16, cp.hp, t, ws, s);
    case ROUTE_HP:
      if ((rc = check_ws(ws, ws_bytes, cp.bytes))) return rc;
      g_last_path = MDCONV_PATH_MFMA;
      g_last_kernels = MDCONV_KERNELS_HP;
      return hp_forward(dt, cp.hp, t, ws, s);
    case ROUTE_F32:
    case ROUTE_F32_SAMP32:
      g_last_path = MDCONV_PATH_MFMA;
      g_last_kernels = MDCONV_KERNELS_F32;
      if ((rc = check_ws(ws, ws_bytes, cp.bytes))) return rc;
      if (cp.route == ROUTE_F32_SAMP32) return samp32_forward(g, dt, cp.s32, t, ws, s);
      return mfma_forward(g, dt, cp.f32, t, ws, s);
    default:
      g_last_path = MDCONV_PATH_DIRECT;
      g_last_kernels = MDCONV_KERNELS_DIRECT;
      note_direct_fallback(g, dt, false, path);
      if (cp.route != ROUTE_DIRECT_SAMP32) return direct_forward(g, dt, t, s);
      if ((rc = check_ws(ws, ws_bytes, cp.bytes))) return rc;
      return samp32_forward(g, dt, cp.s32, t, ws, s);
  }
}

static int run_backward(const mdconv_desc *d, int nd, int modulated, Tensors t, void *ws,
                        size_t ws_bytes, void *stream) {
  g_err[0] = 0;
  g_last_geometry = 0;
  Geom g;
  int rc = fill_geom(d, &g);
  if (rc) return rc;
  if (g.nd != nd || (d->modulated != 0) != (modulated != 0)) {
    set_error("descriptor (ndim=%d, modulated=%d) does not match this entry point", g.nd,
              d->modulated);
    return MDCONV_EINVAL;
  }
  Modes md;
  if ((rc = call_modes(d, &md))) return rc;
  const Skip skip = md.skip;
  // a skipped gradient's pointers are neither required nor used: the call goes on as if they were NULL
  if (skip.input) t.grad_input = nullptr;
  if (skip.weight) t.grad_weight = t.grad_bias = nullptr;
  if ((rc = require(t.input, "input")) || (rc = require(t.weight, "weight")) ||
      (rc = require(t.offset, "offset")) || (rc = require(t.grad_output, "grad_output")) ||
      (!skip.input && (rc = require(t.grad_input, "grad_input"))) ||
      (!skip.weight && (rc = require(t.grad_weight, "grad_weight"))) ||
      (rc = require(t.grad_offset, "grad_offset")))
    return rc;
  if (modulated && ((rc = require(t.mask, "mask")) || (rc = require(t.grad_mask, "grad_mask"))))
    return rc;
  if (g.with_bias && !skip.weight && (rc = require(t.grad_bias, "grad_bias"))) return rc;
  hipStream_t s = (hipStream_t)stream;
  g.acc_data = g.acc_w = md.accumulate;
  const int path = md.path;
  const int dt = base_dtype(d), s32 = sampling_f32(d);
  t.samp32 = s32;
  t.wgrad32 = wgrad_f32(d, true);
  g.in_cl = md.input_layout == MDCONV_LAYOUT_CHANNELS_LAST ? 1 : 0;
  g.det = md.deterministic;
  {   // pointer alignment: "element", but 16 bytes for the tensors the kernels move as channels-last vectors
    const size_t es = dtype_bytes(dt), es_s = s32 ? 4 : es, es_w = t.wgrad32 ? 4 : es;
    if ((rc = require_aligned(t.input, "input", g.in_cl ? 16 : es)) || (rc = require_aligned(t.weight, "weight", es)) ||
        (rc = require_aligned(t.offset, "offset", es_s)) || (rc = require_aligned(t.grad_output, "grad_output", es)) ||
        (rc = require_aligned(t.grad_input, "grad_input", md.gi_cl ? 16 : es)) ||
        (rc = require_aligned(t.grad_weight, "grad_weight", es_w)) || (rc = require_aligned(t.grad_offset, "grad_offset", es_s)))
      return rc;
    if (modulated && ((rc = require_aligned(t.mask, "mask", es_s)) || (rc = require_aligned(t.grad_mask, "grad_mask", es_s))))
      return rc;
    if (g.with_bias && !skip.weight && (rc = require_aligned(t.grad_bias, "grad_bias", es_w))) return rc;
  }
  CallPlan cp;
  plan_call(g, dt, s32, t.wgrad32, path, true, &cp, skip, md.math_bf16, md.out_cl != 0, md.gi_cl != 0);
  if (cp.refused) return refuse(cp, g, dt, path, true);
  // the workspace check; without weight gradients there is nothing to wait for, so the weights-ready event goes in front
  // of the call's first kernel
  auto ready = [&]() -> int {
    const int r = check_ws(ws, ws_bytes, cp.bytes);
    return r || !skip.weight ? r : record_weight_ready(s);
  };
  if (cp.route == ROUTE_DW) {
    if ((rc = ready())) return rc;
    g_last_path = MDCONV_PATH_DEPTHWISE;
    g_last_kernels = MDCONV_KERNELS_DEPTHWISE;
    return dw_backward(cp.dw, t, ws, s);
  }
  if (cp.route == ROUTE_HP || cp.route == ROUTE_HP_F32) {
    if ((rc = ready())) return rc;
    g_last_path = MDCONV_PATH_MFMA;
    g_last_kernels = MDCONV_KERNELS_HP;
    if (cp.route == ROUTE_HP) return hp_backward(dt, cp.hp, t, ws, s);
    // the bf16 kernels on the caller's fp32 tensors (HpPlan::io32)
    return hp_backward(MDCONV_BF16, cp.hp, t, ws, s);
  }
  if (cp.route == ROUTE_F32 || cp.route == ROUTE_F32_SAMP32) {
    g_last_path = MDCONV_PATH_MFMA;
    g_last_kernels = MDCONV_KERNELS_F32;
    if ((rc = ready())) return rc;
    if (cp.route == ROUTE_F32_SAMP32) return samp32_backward(g, dt, cp.s32, t, ws, s);
    return mfma_backward(g, dt, cp.f32, t, ws, s);
  }
  g_last_path = MDCONV_PATH_DIRECT;
  g_last_kernels = MDCONV_KERNELS_DIRECT;
  note_direct_fallback(g, dt, true, path);
  if ((rc = ready())) return rc;
  if (cp.route == ROUTE_DIRECT_SAMP32) return samp32_backward(g, dt, cp.s32, t, ws, s);
  if (cp.route == ROUTE_DIRECT_16) {
    if ((rc = direct16_backward(g, dt, cp.d16, t, ws, s, skip))) return rc;
    return skip.weight ? MDCONV_OK : record_weight_ready(s);
  }
  if (skip.input) t.grad_input = ws;   // scratch: scattered into, never read (CallPlan::scratch_gi)
  if (!md.accumulate) {
    // the direct kernels scatter with atomics, so "overwrite" means: clear first
    const size_t es = dt == MDCONV_F64 ? 8 : (dt == MDCONV_F32 ? 4 : 2);
    const size_t n_off = (size_t)g.B * g.DG * g.nd * g.K * g.S_o, n_m = (size_t)g.B * g.DG * g.K * g.S_o;
    if (!skip.input && (rc = zero_bytes(t.grad_input, (size_t)g.B * g.C * g.S_i * es, s))) return rc;
    if ((rc = zero_bytes(t.grad_offset, n_off * es, s))) return rc;
    if (!skip.weight && (rc = zero_bytes(t.grad_weight, (size_t)g.O * g.Cg * g.K * es, s))) return rc;
    if (modulated && (rc = zero_bytes(t.grad_mask, n_m * es, s))) return rc;
    if (g.with_bias && !skip.weight && (rc = zero_bytes(t.grad_bias, (size_t)g.O * es, s))) return rc;
  }
  if ((rc = direct_backward(g, dt, t, s, skip.weight ? 1 : 3))) return rc;
  return skip.weight ? MDCONV_OK : record_weight_ready(s);
}

int record_weight_ready(hipStream_t stream) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return MDCONV_ELAUNCH;
  std::lock_guard<std::mutex> lock(g_wready_mu);
  const auto key = std::make_pair(dev, stream);
  auto it = g_wready.find(key);
  if (it == g_wready.end()) {
    if (g_wready.size() >= kWReadyMax) {   // programs that create and destroy many streams: evict the oldest
      auto old = g_wready.begin();
      for (auto j = g_wready.begin(); j != g_wready.end(); ++j)
        if (j->second.tick < old->second.tick) old = j;
      for (auto j = g_wready_latest.begin(); j != g_wready_latest.end();)
        j = (j->second == old->second.ev) ? g_wready_latest.erase(j) : std::next(j);
      (void)hipEventDestroy(old->second.ev);
      g_wready.erase(old);
    }
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
      set_error("hipEventCreate failed");
      return MDCONV_ELAUNCH;
    }
    it = g_wready.emplace(key, WReady{ev, 0}).first;
  }
  it->second.tick = ++g_wready_tick;
  if (hipEventRecord(it->second.ev, stream) != hipSuccess) {
    set_error("hipEventRecord failed");
    return MDCONV_ELAUNCH;
  }
  g_wready_latest[dev] = it->second.ev;
  return MDCONV_OK;
}

static int wait_weight_ready(hipStream_t waiter, bool keyed, hipStream_t producer) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return MDCONV_ELAUNCH;
  // the wait is enqueued UNDER the lock: record_weight_ready() may evict and destroy the least recently used event
  // of another stream at any time, and an event copied out of the table could be gone by the time it is waited on
  std::lock_guard<std::mutex> lock(g_wready_mu);
  hipEvent_t ev = nullptr;
  if (keyed) {
    auto it = g_wready.find(std::make_pair(dev, producer));
    if (it != g_wready.end()) ev = it->second.ev;
  } else {
    auto it = g_wready_latest.find(dev);
    if (it != g_wready_latest.end()) ev = it->second;
  }
  if (!ev) {
    set_error(keyed ? "no backward has been issued on that stream of this device"
                    : "no backward has been issued on this device");
    return MDCONV_EINVAL;
  }
  if (hipStreamWaitEvent(waiter, ev, 0) != hipSuccess) {
    set_error("hipStreamWaitEvent failed");
    return MDCONV_ELAUNCH;
  }
  return MDCONV_OK;
}

}  // namespace mdconv

using namespace mdconv;

extern "C" {

int mdconv_abi_version(void) { return MDCONV_ABI_VERSION; }
const char *mdconv_last_error(void) { return g_err; }

int mdconv_out_size(const mdconv_desc *d, int axis) {
  if (!d || axis < 0 || axis > 2) return -1;
  if (axis >= desc_ndim(d)) return 1;
  return (d->in_sz[axis] + 2 * d->pad[axis] - (d->dil[axis] * (d->k_sz[axis] - 1) + 1)) /
             d->stride[axis] + 1;
}

size_t mdconv_workspace_bytes(const mdconv_desc *d, int backward) {
  Geom g;
  Modes md;
  if (fill_geom(d, &g) || call_modes(d, &md)) return 0;
  g.in_cl = md.input_layout == MDCONV_LAYOUT_CHANNELS_LAST ? 1 : 0;   // (the plan of a channels-last call, where the caller says so)
  g.det = backward ? md.deterministic : 0;   // the list sort's scratch (backward on the matrix-core kernels only)
  CallPlan cp;
  plan_call(g, base_dtype(d), sampling_f32(d), wgrad_f32(d, backward != 0), md.path, backward != 0, &cp, md.skip, md.math_bf16,
            md.out_cl != 0, md.gi_cl != 0);
  return cp.reported;
}

int mdconv_result_layout_supported(const mdconv_desc *d, int backward) {
  Geom g;
  Modes md;
  if (fill_geom(d, &g) || call_modes(d, &md)) return 0;
  g.in_cl = md.input_layout == MDCONV_LAYOUT_CHANNELS_LAST ? 1 : 0;
  g.det = backward ? md.deterministic : 0;
  CallPlan cp;
  plan_call(g, base_dtype(d), sampling_f32(d), wgrad_f32(d, backward != 0), md.path, backward != 0, &cp, md.skip, md.math_bf16,
            md.out_cl != 0, md.gi_cl != 0);
  if (cp.refused != REFUSE_RESULT_LAYOUT) return 1;
  set_layout_refusal(cp, backward != 0);   // the rule, for mdconv_last_error()
  return 0;
}

int mdconv_planned_kernels(const mdconv_desc *d, int backward) {
  Geom g;
  Modes md;
  if (fill_geom(d, &g) || call_modes(d, &md)) return 0;
  g.in_cl = md.input_layout == MDCONV_LAYOUT_CHANNELS_LAST ? 1 : 0;
  g.det = backward ? md.deterministic : 0;
  const int dt = base_dtype(d);
  CallPlan cp;
  plan_call(g, dt, sampling_f32(d), wgrad_f32(d, backward != 0), md.path, backward != 0, &cp, md.skip, md.math_bf16, md.out_cl != 0,
            md.gi_cl != 0);
  if (cp.refused) {
    refuse(cp, g, dt, md.path, backward != 0);   // the rule, for mdconv_last_error()
    return 0;
  }
  switch (cp.route) {
    case ROUTE_DW: return MDCONV_KERNELS_DEPTHWISE;
    case ROUTE_HP: case ROUTE_HP_F32: return MDCONV_KERNELS_HP;
    case ROUTE_F32: case ROUTE_F32_SAMP32: return MDCONV_KERNELS_F32;
    default: return MDCONV_KERNELS_DIRECT;
  }
}

int mdconv_math_bf16_used(const mdconv_desc *d, int backward) {
  Geom g;
  Modes md;
  if (fill_geom(d, &g) || call_modes(d, &md) || !md.math_bf16) return 0;
  g.in_cl = md.input_layout == MDCONV_LAYOUT_CHANNELS_LAST ? 1 : 0;
  g.det = backward ? md.deterministic : 0;
  CallPlan cp;
  plan_call(g, base_dtype(d), 0, 0, md.path, backward != 0, &cp, md.skip, 1);
  return cp.route == ROUTE_HP_F32;
}

int mdconv_set_input_layout(int layout) {
  const int prev = g_input_layout;
  if (layout == MDCONV_LAYOUT_NCHW || layout == MDCONV_LAYOUT_CHANNELS_LAST) g_input_layout = layout;
  return prev;
}

int mdconv_input_layout_supported(const mdconv_desc *d, int layout, int backward) {
  Geom g;
  Modes md;
  if (fill_geom(d, &g) || call_modes(d, &md)) return 0;
  if (layout == MDCONV_LAYOUT_NCHW) return 1;
  if (layout != MDCONV_LAYOUT_CHANNELS_LAST) return 0;
  g.in_cl = 1;   // the plan of a channels-last call (the group-padded layout needs the library's own input copy)
  CallPlan cp;
  plan_call(g, base_dtype(d), sampling_f32(d), wgrad_f32(d, backward != 0), md.path, backward != 0, &cp);
  return cp.refused != REFUSE_CHANNELS_LAST && cp.refused != REFUSE_PATH_DEPTHWISE;
}

int mdconv_deterministic_supported(const mdconv_desc *d, int backward) {
  Geom g;
  Modes md;
  if (fill_geom(d, &g) || call_modes(d, &md)) return 0;
  if (!backward) return 1;   // every forward is a fixed-order sum per output element
  g.in_cl = md.input_layout == MDCONV_LAYOUT_CHANNELS_LAST ? 1 : 0;
  g.det = 1;
  CallPlan cp;
  plan_call(g, base_dtype(d), sampling_f32(d), wgrad_f32(d, true), md.path, true, &cp, Skip(), md.math_bf16);
  if (cp.refused == REFUSE_PATH_DEPTHWISE) {   // the call itself would be refused
    refuse(cp, g, base_dtype(d), md.path, true);
    return 0;
  }
  if (!route_is_direct(cp.route)) return 1;
  set_det_refusal(g, base_dtype(d), md.path);   // the reason, for mdconv_last_error()
  return 0;
}

int mdconv_set_accumulate(int on) {
  const int prev = g_accumulate;
  g_accumulate = on ? 1 : 0;
  return prev;
}

int mdconv_stream_wait_weight_ready(void *stream) {
  return wait_weight_ready((hipStream_t)stream, false, nullptr);
}

int mdconv_stream_wait_weight_ready_on(void *stream, void *producer_stream) {
  return wait_weight_ready((hipStream_t)stream, true, (hipStream_t)producer_stream);
}

int mdconv_set_path(int path) {
  const int prev = current_path();
  if (path >= MDCONV_PATH_AUTO && path <= MDCONV_PATH_DEPTHWISE) g_path.store(path);
  return prev;
}
int mdconv_last_path(void) { return g_last_path; }
int mdconv_last_kernels(void) { return g_last_kernels; }
int mdconv_last_geometry(void) { return g_last_geometry; }
int mdconv_geometry_is_canonical(const mdconv_desc *d) {
  Geom g;
  return fill_geom(d, &g) == MDCONV_OK && geom_is_canon3x3(g) ? 1 : 0;
}

int mdconv_deform_conv2d_forward(const mdconv_desc *d, const void *input, const void *weight,
                                 const void *bias, const void *offset, void *output,
                                 void *workspace, size_t workspace_bytes, void *stream) {
  Tensors t = {};
  t.input = input; t.weight = weight; t.bias = bias; t.offset = offset; t.output = output;
  return run_forward(d, 2, 0, t, workspace, workspace_bytes, stream);
}

int mdconv_deform_conv2d_backward(const mdconv_desc *d, const void *input, const void *weight,
                                  const void *bias, const void *offset, void *grad_input,
                                  void *grad_weight, void *grad_bias, void *grad_offset,
                                  const void *grad_output, void *workspace,
                                  size_t workspace_bytes, void *stream) {
  Tensors t = {};
  t.input = input; t.weight = weight; t.bias = bias; t.offset = offset;
  t.grad_output = grad_output; t.grad_input = grad_input; t.grad_weight = grad_weight;
  t.grad_bias = grad_bias; t.grad_offset = grad_offset;
  return run_backward(d, 2, 0, t, workspace, workspace_bytes, stream);
}

int mdconv_modulated_deform_conv2d_forward(const mdconv_desc *d, const void *input,
                                           const void *weight, const void *bias,
                                           const void *offset, const void *mask, void *output,
                                           void *workspace, size_t workspace_bytes, void *stream) {
  Tensors t = {};
  t.input = input; t.weight = weight; t.bias = bias; t.offset = offset; t.mask = mask;
  t.output = output;
  return run_forward(d, 2, 1, t, workspace, workspace_bytes, stream);
}

int mdconv_modulated_deform_conv2d_backward(const mdconv_desc *d, const void *input,
                                            const void *weight, const void *bias,
                                            const void *offset, const void *mask,
                                            const void *grad_output, void *grad_input,
                                            void *grad_offset, void *grad_mask, void *grad_weight,
                                            void *grad_bias, void *workspace,
                                            size_t workspace_bytes, void *stream) {
  Tensors t = {};
  t.input = input; t.weight = weight; t.bias = bias; t.offset = offset; t.mask = mask;
  t.grad_output = grad_output; t.grad_input = grad_input; t.grad_weight = grad_weight;
  t.grad_bias = grad_bias; t.grad_offset = grad_offset; t.grad_mask = grad_mask;
  return run_backward(d, 2, 1, t, workspace, workspace_bytes, stream);
}

int mdconv_deform_conv3d_forward(const mdconv_desc *d, const void *input, const void *weight,
                                 const void *bias, const void *offset, void *output,
                                 void *workspace, size_t workspace_bytes, void *stream) {
  Tensors t = {};
  t.input = input; t.weight = weight; t.bias = bias; t.offset = offset; t.output = output;
  return run_forward(d, 3, 0, t, workspace, workspace_bytes, stream);
}

int mdconv_deform_conv3d_backward(const mdconv_desc *d, const void *input, const void *weight,
                                  const void *bias, const void *offset, void *grad_input,
                                  void *grad_weight, void *grad_bias, void *grad_offset,
                                  const void *grad_output, void *workspace,
                                  size_t workspace_bytes, void *stream) {
  Tensors t = {};
  t.input = input; t.weight = weight; t.bias = bias; t.offset = offset;
  t.grad_output = grad_output; t.grad_input = grad_input; t.grad_weight = grad_weight;
  t.grad_bias = grad_bias; t.grad_offset = grad_offset;
  return run_backward(d, 3, 0, t, workspace, workspace_bytes, stream);
}

int mdconv_modulated_deform_conv3d_forward(const mdconv_desc *d, const void *input,
                                           const void *weight, const void *bias,
                                           const void *offset, const void *mask, void *output,
                                           void *workspace, size_t workspace_bytes, void *stream) {
  Tensors t = {};
  t.input = input; t.weight = weight; t.bias = bias; t.offset = offset; t.mask = mask;
  t.output = output;
  return run_forward(d, 3, 1, t, workspace, workspace_bytes, stream);
}

int mdconv_modulated_deform_conv3d_backward(const mdconv_desc *d, const void *input,
                                            const void *weight, const void *bias,
                                            const void *offset, const void *mask,
                                            void *grad_input, void *grad_weight, void *grad_bias,
                                            void *grad_offset, void *grad_mask,
                                            const void *grad_output, void *workspace,
                                            size_t workspace_bytes, void *stream) {
  Tensors t = {};
  t.input = input; t.weight = weight; t.bias = bias; t.offset = offset; t.mask = mask;
  t.grad_output = grad_output; t.grad_input = grad_input; t.grad_weight = grad_weight;
  t.grad_bias = grad_bias; t.grad_offset = grad_offset; t.grad_mask = grad_mask;
  return run_backward(d, 3, 1, t, workspace, workspace_bytes, stream);
}

}  // extern "C"
