// mfma_plans.hip -- the plan of a call of the fp32 matrix-core family (mfma_plan.hpp): shapes the kernels tile run
// natively (mfma_kernels.hip); deformable groups and channel counts they do not tile run as one zero-padded problem or as
// single-group slices through the same kernels.
#include "mfma_plan.hpp"

#include <stdlib.h>
#include <string.h>

namespace mdconv {

// ---------------------------------------------------------------------------------------------
// Backward for deformable groups the kernels above do not tile (C_in / DG of 16, 24, 32, 40 ...): the
// gradients of deformable group dg involve its own input channels, offsets and masks and nothing of the
// other groups (mdeformable_conv.cu:231 indexes the offsets by c / channel_per_deformable_group), so the
// call is DG independent single-group problems over channel slices -- each copied into the workspace
// (strided 2-D copies, a few % of the kernels' traffic), run through the same matrix-core pipeline and
// copied back.  Slower per sample than a native tiling (C_in / DG = 32 fills half of a 64-channel tile)
// but an order of magnitude faster than the shape-generic scatter kernels these shapes used to reach.
// ---------------------------------------------------------------------------------------------
namespace {
bool split_slice_geom(const Geom &g, Geom *out, bool *copy_w, bool *copy_go) {
  if (g.DG <= 1 || g.Cdg < 16 || g.Cdg % 8) return false;
  Geom s = g;
  s.DG = 1; s.C = g.Cdg; s.Cdg = g.Cdg; s.with_bias = 0;
  if (g.Cg % g.Cdg == 0) {          // the slice lies inside one conv group
    s.G = 1; s.Cg = g.Cdg; s.O = s.Og = g.Og;
    *copy_w = g.Cg != g.Cdg;
  } else if (g.Cdg % g.Cg == 0) {   // the slice is a run of whole conv groups
    s.G = g.Cdg / g.Cg; s.Cg = g.Cg; s.Og = g.Og; s.O = s.G * g.Og;
    *copy_w = false;
  } else {
    return false;
  }
  *copy_go = s.O != g.O;
  *out = s;
  return true;
}
bool split_plan(const Geom &g, int dtype, bool wgrad32, Skip skip, SplitPlan *p) {
  if (!split_slice_geom(g, &p->gs, &p->copy_w, &p->copy_go)) return false;
  // The slices' workspace is sized from the geometry the FIRST slice of a conv group runs with (split_backward): that
  // slice carries grad_bias and has the grad_bias stage buffer at the end of its layout -- sized without it, it wrote
  // 32 * C_out * 4 bytes past the workspace (found by tools/fuzz_more.py in round 5; tests/test_gpu_workspace_guard.py)
  Geom first = p->gs;
  first.with_bias = g.with_bias;
  if (!native_plan(first, dtype, true, &p->first, skip)) return false;
  p->rest = p->first;
  if (first.with_bias && !native_plan(p->gs, dtype, true, &p->rest, skip)) return false;
  const size_t es = dtype == MDCONV_F32 ? 4 : 2;
  const size_t es_w = wgrad32 ? 4 : es;   // grad_weight rows (fp32 with MDCONV_WGRAD_F32)
  const Geom &s = p->gs;
  Bump ws;
  p->off_x = ws.take((size_t)g.B * s.C * g.S_i * es);
  p->off_off = ws.take((size_t)g.B * g.nd * g.K * g.S_o * es);
  p->off_m = ws.take(g.modulated ? (size_t)g.B * g.K * g.S_o * es : 0);
  p->off_go = ws.take(p->copy_go ? (size_t)g.B * s.O * g.S_o * es : 0);
  p->off_w = ws.take(p->copy_w ? (size_t)s.O * s.Cg * g.K * es : 0);
  p->off_gi = ws.take(skip.input ? 0 : (size_t)g.B * s.C * g.S_i * es);   // (a selective backward: no slice of a skipped gradient)
  p->off_goff = ws.take((size_t)g.B * g.nd * g.K * g.S_o * es);
  p->off_gm = ws.take(g.modulated ? (size_t)g.B * g.K * g.S_o * es : 0);
  p->off_gw = ws.take(p->copy_w && !skip.weight ? (size_t)s.O * s.Cg * g.K * es_w : 0);
  p->off_sub = ws.off;
  p->total = ws.off + p->first.total;
  return true;
}

int split_backward(const Geom &g, int dtype, const SplitPlan &p, const Tensors &t, void *ws, hipStream_t stream) {
  char *base = (char *)ws;
  const size_t es = dtype == MDCONV_F32 ? 4 : 2;
  const size_t es_w = wgrad_bytes(dtype, t);   // grad_weight / grad_bias elements
  const Geom &s = p.gs;
  const size_t w_x = (size_t)s.C * g.S_i * es, p_x = (size_t)g.C * g.S_i * es;
  const size_t w_off = (size_t)g.nd * g.K * g.S_o * es, p_off = w_off * g.DG;
  const size_t w_m = (size_t)g.K * g.S_o * es, p_m = w_m * g.DG;
  const size_t w_go = (size_t)s.O * g.S_o * es, p_go = (size_t)g.O * g.S_o * es;
  const size_t w_w = (size_t)s.Cg * g.K * es, p_w = (size_t)g.Cg * g.K * es;
  const size_t w_gw = (size_t)s.Cg * g.K * es_w, p_gw = (size_t)g.Cg * g.K * es_w;
  const Skip skip = p.first.skip;   // skipped gradients: no slice buffer, no copies in or out, NULL for the slices
  int rc;
  for (int dg = 0; dg < g.DG; ++dg) {
    const int c0 = dg * g.Cdg;            // first input channel of the slice
    const int grp = c0 / g.Cg;            // first conv group it touches
    const int o0 = grp * g.Og;            // first output channel of those groups
    const int cw = c0 - grp * g.Cg;       // channel offset inside the group's weight rows
    Tensors ts = t;
    const char *src_x = (const char *)t.input + (size_t)c0 * g.S_i * es;
    const char *src_off = (const char *)t.offset + (size_t)dg * w_off;
    char *dst_gi = skip.input ? nullptr : (char *)t.grad_input + (size_t)c0 * g.S_i * es;
    char *dst_goff = (char *)t.grad_offset + (size_t)dg * w_off;
    char *dst_gw = skip.weight ? nullptr : (char *)t.grad_weight + ((size_t)o0 * g.Cg + cw) * g.K * es_w;
    if ((rc = copy_rows(base + p.off_x, w_x, src_x, p_x, w_x, g.B, stream))) return rc;
    if ((rc = copy_rows(base + p.off_off, w_off, src_off, p_off, w_off, g.B, stream))) return rc;
    ts.input = base + p.off_x; ts.offset = base + p.off_off;
    ts.grad_input = skip.input ? nullptr : base + p.off_gi; ts.grad_offset = base + p.off_goff;
    if (g.modulated) {
      if ((rc = copy_rows(base + p.off_m, w_m, (const char *)t.mask + (size_t)dg * w_m, p_m, w_m, g.B, stream))) return rc;
      ts.mask = base + p.off_m; ts.grad_mask = base + p.off_gm;
    }
    ts.grad_output = (const char *)t.grad_output + (size_t)o0 * g.S_o * es;
    if (p.copy_go) {
      if ((rc = copy_rows(base + p.off_go, w_go, ts.grad_output, p_go, w_go, g.B, stream))) return rc;
      ts.grad_output = base + p.off_go;
    }
    ts.weight = (const char *)t.weight + ((size_t)o0 * g.Cg + cw) * g.K * es;
    ts.grad_weight = dst_gw;
    if (p.copy_w) {
      if ((rc = copy_rows(base + p.off_w, w_w, ts.weight, p_w, w_w, s.O, stream))) return rc;
      ts.weight = base + p.off_w; ts.grad_weight = skip.weight ? nullptr : base + p.off_gw;
    }
    Geom gs = s;
    // grad_bias belongs to the output channels: once per conv group, with the first slice that touches it
    gs.with_bias = g.with_bias && cw == 0 ? 1 : 0;
    ts.bias = nullptr;
    ts.grad_bias = gs.with_bias && !skip.weight ? (char *)t.grad_bias + (size_t)o0 * es_w : nullptr;
    if (g.acc_data) {   // accumulate mode: the slice starts from the caller's values
      if (!skip.input && (rc = copy_rows(base + p.off_gi, w_x, dst_gi, p_x, w_x, g.B, stream))) return rc;
      if ((rc = copy_rows(base + p.off_goff, w_off, dst_goff, p_off, w_off, g.B, stream))) return rc;
      if (g.modulated &&
          (rc = copy_rows(base + p.off_gm, w_m, (const char *)t.grad_mask + (size_t)dg * w_m, p_m, w_m, g.B, stream)))
        return rc;
    }
    if (g.acc_w && p.copy_w && !skip.weight && (rc = copy_rows(base + p.off_gw, w_gw, dst_gw, p_gw, w_gw, s.O, stream))) return rc;
    if ((rc = native_backward(gs, dtype, gs.with_bias ? p.first : p.rest, ts, base + p.off_sub, stream))) return rc;
    if (!skip.input && (rc = copy_rows(dst_gi, p_x, base + p.off_gi, w_x, w_x, g.B, stream))) return rc;
    if ((rc = copy_rows(dst_goff, p_off, base + p.off_goff, w_off, w_off, g.B, stream))) return rc;
    if (g.modulated &&
        (rc = copy_rows((char *)t.grad_mask + (size_t)dg * w_m, p_m, base + p.off_gm, w_m, w_m, g.B, stream)))
      return rc;
    if (p.copy_w && !skip.weight && (rc = copy_rows(dst_gw, p_gw, base + p.off_gw, w_gw, w_gw, s.O, stream))) return rc;
  }
  return skip.weight ? MDCONV_OK : record_weight_ready(stream);   // after the last slice's copies
}
}  // namespace

// Forward of the same shapes: the slices of one conv group add up in its output channels, so each slice's
// output goes to a workspace tile and is copied (first slice of the conv group: it carries the bias) or added
// (fp32 only: adding rounded 16-bit outputs would round DG times) into the caller's rows.
namespace {
bool split_fwd_plan(const Geom &g, int dtype, SplitFwdPlan *p) {
  if (!split_slice_geom(g, &p->gs, &p->copy_w, &p->copy_out)) return false;
  if (g.Cg > g.Cdg && dtype != MDCONV_F32) return false;   // slices of one conv group are summed: fp32 only
  // narrow conv groups are cheap on the shape-generic forward (C=128, 8 groups of 16, DG=4, 64x64, B=16: 0.3 ms
  // faster there than as four slices with mostly-padding tiles); wide ones are not (one group, DG=8: 0.25 ms slower)
  if (g.Cg < 64) return false;
  if (!native_plan(p->gs, dtype, false, &p->sub)) return false;
  const size_t es = dtype == MDCONV_F32 ? 4 : 2;
  const Geom &s = p->gs;
  Bump ws;
  p->off_x = ws.take((size_t)g.B * s.C * g.S_i * es);
  p->off_off = ws.take((size_t)g.B * g.nd * g.K * g.S_o * es);
  p->off_m = ws.take(g.modulated ? (size_t)g.B * g.K * g.S_o * es : 0);
  p->off_w = ws.take(p->copy_w ? (size_t)s.O * s.Cg * g.K * es : 0);
  p->off_out = ws.take((size_t)g.B * s.O * g.S_o * es);
  p->off_sub = ws.off;
  p->total = ws.off + p->sub.total;
  return true;
}
int split_forward(const Geom &g, int dtype, const SplitFwdPlan &p, const Tensors &t, void *ws, hipStream_t stream) {
  char *base = (char *)ws;
  const size_t es = dtype == MDCONV_F32 ? 4 : 2;
  const Geom &s = p.gs;
  const size_t w_x = (size_t)s.C * g.S_i * es, p_x = (size_t)g.C * g.S_i * es;
  const size_t w_off = (size_t)g.nd * g.K * g.S_o * es, p_off = w_off * g.DG;
  const size_t w_m = (size_t)g.K * g.S_o * es, p_m = w_m * g.DG;
  const size_t w_out = (size_t)s.O * g.S_o * es, p_out = (size_t)g.O * g.S_o * es;
  const size_t w_w = (size_t)s.Cg * g.K * es, p_w = (size_t)g.Cg * g.K * es;
  int rc;
  for (int dg = 0; dg < g.DG; ++dg) {
    const int c0 = dg * g.Cdg, grp = c0 / g.Cg, o0 = grp * g.Og, cw = c0 - grp * g.Cg;
    Tensors ts = t;
    if ((rc = copy_rows(base + p.off_x, w_x, (const char *)t.input + (size_t)c0 * g.S_i * es, p_x, w_x, g.B, stream))) return rc;
    if ((rc = copy_rows(base + p.off_off, w_off, (const char *)t.offset + (size_t)dg * w_off, p_off, w_off, g.B, stream))) return rc;
    ts.input = base + p.off_x; ts.offset = base + p.off_off;
    if (g.modulated) {
      if ((rc = copy_rows(base + p.off_m, w_m, (const char *)t.mask + (size_t)dg * w_m, p_m, w_m, g.B, stream))) return rc;
      ts.mask = base + p.off_m;
    }
    ts.weight = (const char *)t.weight + ((size_t)o0 * g.Cg + cw) * g.K * es;
    if (p.copy_w) {
      if ((rc = copy_rows(base + p.off_w, w_w, ts.weight, p_w, w_w, s.O, stream))) return rc;
      ts.weight = base + p.off_w;
    }
    Geom gs = s;
    gs.with_bias = g.with_bias && cw == 0 ? 1 : 0;
    ts.bias = gs.with_bias ? (const char *)t.bias + (size_t)o0 * es : nullptr;
    ts.output = base + p.off_out;
    if ((rc = native_forward(gs, dtype, p.sub, ts, base + p.off_sub, stream))) return rc;
    char *dst = (char *)t.output + (size_t)o0 * g.S_o * es;
    if (cw == 0) {
      if ((rc = copy_rows(dst, p_out, base + p.off_out, w_out, w_out, g.B, stream))) return rc;
    } else {
      if ((rc = add_rows((float *)dst, (int64_t)g.O * g.S_o, (const float *)(base + p.off_out), (int64_t)s.O * g.S_o, (int64_t)g.B,
                         stream)))
        return rc;
    }
  }
  return MDCONV_OK;
}
}  // namespace

// ---------------------------------------------------------------------------------------------
// The same shapes as ONE padded problem (round 6): every deformable group widened to a size the kernels tile (forward: whole
// 32-channel K stages; backward: 64 / 128 / n x 256 channels) with zero input planes and zero weight rows in between -- the
// padding channels add nothing to any output, and their own gradient rows are never copied back.  One launch sequence over
// C' = DG x padded-group channels instead of DG sequences over mostly-padding tiles plus their copies: faster on all 13 shapes
// measured, 4x growth included (fp32, 4 groups: 64 -> 64 at 56 x 56, B = 16 1.44 -> 1.00 ms; 192 -> 192 at 20 x 20 0.70 -> 0.30;
// 3-D 64 -> 64 2.41 -> 1.12; profiles/r06_experiments.md 18).  Taken when the padded problem is at most a few times
// the caller's (kPadMaxGrowth); one conv group only (conv groups keep the slices above).
// ---------------------------------------------------------------------------------------------
namespace {
// 16 -> 16 channels in 2 groups (8 -> 32 forward, 8 -> 64 backward): 0.39 ms on the shape-generic kernels, 0.25 padded; in 4 groups
// (4 -> 32 / 64) at 40 x 40, B = 8: 0.43 ms generic against 0.34 padded, and the generic kernels fall further behind with every output
// channel (16 -> 256 in 4 groups: 1.76 vs 0.64 ms; 3-D: 5.68 vs 1.27); groups of 2 channels (32x) lose at 16 output channels
// (profiles/r06_experiments.md 20, 24)
constexpr int kPadMaxGrowth = 16;
// MDCONV_PAD_CHANNELS = 0 | 1: never / wherever eligible (the test suite's way to reach the plan with small shapes); read once
int pad_channels_env() {
  static const int v = getenv("MDCONV_PAD_CHANNELS") ? atoi(getenv("MDCONV_PAD_CHANNELS")) : -1;
  return v;
}
// MDCONV_DG_PLAN = pad | split forces one plan where both exist (developer A/B; default: by growth)
int dg_plan_env() {
  static const int v = [] {
    const char *e = getenv("MDCONV_DG_PLAN");
    return !e ? 0 : (!strcmp(e, "pad") ? 1 : (!strcmp(e, "split") ? 2 : 0));
  }();
  return v;
}
// ONE deformable group and one conv group: two kinds of shapes run as a padded problem although nothing about their groups
// needs it (profiles/r06_experiments.md 22, 23).
//  * C_in not a multiple of the 64-channel slab of the channels-last kernels.  Such shapes are tiled natively, but by the NCHW
//    kernels, whose 2^nd corner loads go to one channel PLANE each; padded to the next multiple of 64 they take the channels-last
//    kernels.  3-D from 2048 output pixels (32 -> 64 at 16 x 56 x 56, B = 2: 3.33 -> 1.80 ms; 16 -> 16 at 16 x 32 x 32: 0.98 -> 0.72;
//    160 channels at 1568 pixels: +7 %, hence the floor); 2-D only for 32 <= C_in < 64 from 8192 pixels, where the backward is
//    channels-last anyway (48 -> 48 at 56 x 56, B = 16: 0.41 -> 0.34 ms; 96 / 160 channels lose 10-15 %).
//  * Fewer than 16 input or output channels: below the matrix kernels' floor, i.e. the shape-generic kernels -- whose cost grows
//    with C_in x C_out x taps per thread.  Output channels are padded to 16 (zero weight rows, zero grad_output planes, a
//    workspace tile for the output), input channels to 64: 3-D 64 -> 8 at 8 x 28 x 28: 6.92 -> 0.45 ms, 2-D 64 -> 8 at 56 x 56,
//    B = 16: 3.08 -> 0.32 ms, 3-D 8 -> 8 at 16 x 32 x 32: 1.81 -> 0.73 ms, 2-D 8 -> 8 at 112 x 112, B = 8: 0.81 -> 0.57 ms.  Not for
//    grids of a few hundred pixels (4 -> 4 at 8 x 8, BASELINE configs[0]: 0.13 ms generic, 0.21 padded), nor in 2-D below 8 input
//    channels (3 -> 16 at 112 x 112: 0.38 -> 0.55 ms) or 8192 pixels (ties).
// (pad_channels_env overrides the size rules.)
bool pad_channels_preferred(const Geom &g) {
  const int env = pad_channels_env();
  if (env == 0 || g.DG != 1) return false;
  if (g.G != 1)   // conv groups: the 3-D slab rule per group (3-D 200 -> 64 in 2 groups at 8 x 20 x 20: 1.19 ms, 256 -> 64: 0.61)
    // (at most 2x: 64 -> 128 in 4 groups of 16 -> 64 at 8 x 14 x 14 lost 26 %)
    return g.nd == 3 && g.Cg >= 32 && g.Cg % 64 != 0 && (env > 0 || g.N >= 2048);
  const bool tiny_c = g.C < 16, tiny_o = g.O < 16;
  if (!tiny_c && !tiny_o && g.C % 64 == 0) return false;
  if (env > 0) return true;
  if (tiny_c) return g.nd == 3 ? g.N >= 512 : (g.C >= 8 && g.N >= 8192);
  if (tiny_o) return g.N >= 512;
  if (g.nd == 3) return g.N >= 2048;
  return g.C >= 32 && g.C < 64 && g.N >= 8192;
}
// padded channels of one deformable group for the plan of `g` (0 = no plan).  native_ok: the direction is tiled natively.
int pad_group_channels(const Geom &g, bool backward, bool native_ok) {
  const int env = pad_channels_env();
  if (g.DG == 1) {
    if (pad_channels_preferred(g)) {
      if (g.C % 64 == 0) return g.C;
      const bool to_slab = g.nd == 3 || g.C < 16 || (g.C >= 32 && g.C < 64 && g.N >= 8192);
      return to_slab ? (g.C + 63) / 64 * 64 : (g.C + 7) / 8 * 8;   // (else only C_out is padded: the NCHW kernels need 8 | C_in)
    }
    // What the kernels do not tile at all -- C_in that is not a multiple of 8 in the backward (100 -> 100 at 40 x 40, B = 8:
    // 4.85 ms on the shape-generic kernels, 0.27 ms as 104 channels), channel counts below 16 that the size rules above leave
    // alone: the smallest padded problem, from 512 output pixels (experiment log 24).
    if (native_ok || env == 0 || g.N < 512) return 0;
    const int c8 = (g.C + 7) / 8 * 8;
    return c8 < 16 ? 16 : c8;
  }
  if (native_ok) return 0;
  const int cdp_b = g.Cdg <= 64 ? 64 : (g.Cdg <= 128 ? 128 : (g.Cdg + 255) / 256 * 256);
  const int cdp_f = (g.Cdg + 2 * kBK - 1) / (2 * kBK) * (2 * kBK);
  // (the cap looks at the backward's padding in both directions: a padded forward in front of a generic backward is no gain)
  if (dg_plan_env() != 1 && cdp_b > kPadMaxGrowth * g.Cdg) return 0;
  return backward ? cdp_b : cdp_f;
}
// native_ok: the kernels tile `g` itself
bool pad_plan(const Geom &g, int dtype, bool backward, bool native_ok, bool wgrad32, Skip skip, PadPlan *p) {
  if (dg_plan_env() == 2) return false;
  Geom gp = g;
  if (g.G == 1) {
    const int cdp = pad_group_channels(g, backward, native_ok);
    if (cdp == 0) return false;
    // output channels below the kernels' floor of 16: padded too (with several deformable groups from 512 output pixels)
    const int Op = g.O < 16 && (g.DG == 1 || g.N >= 512) ? 16 : g.O;
    p->ng = g.DG; p->cin = g.Cdg; p->cinp = cdp;
    p->nog = 1; p->og = g.O; p->ogp = Op;
    p->wsub = g.DG;
    gp.C = gp.Cg = g.DG * cdp;
    gp.Cdg = cdp;
    gp.O = gp.Og = Op;
  } else {
    // conv groups (one deformable group): per-group channel counts the kernels do not tile -- C_in / G not a multiple of 8 or
    // below 16, fewer than 16 output channels per group -- padded PER CONV GROUP, from 512 output pixels (experiment log 28)
    const int env = pad_channels_env();
    p->nog = g.G; p->og = g.Og; p->ogp = g.Og < 16 ? 16 : g.Og;
    if (g.DG == 1) {
      const bool slab = pad_channels_preferred(g);   // 3-D: whole 64-channel slabs per group for the channels-last kernels
      if (env == 0 || (!slab && (native_ok || g.N < 512))) return false;
      const int c8 = (g.Cg + 7) / 8 * 8;
      p->ng = g.G; p->cin = g.Cg; p->cinp = slab ? (g.Cg + 63) / 64 * 64 : (c8 < 16 ? 16 : c8);
      p->wsub = 1;
      gp.Cg = p->cinp;
      gp.C = gp.Cdg = g.G * p->cinp;
    } else {
      // conv groups AND deformable groups the kernels do not tile, NESTED (one grouping refines the other, so that padding the
      // finer groups by the same amount keeps every channel in its conv group and its deformable group): the deformable group
      // goes to the next size the kernels tile that the finer groups divide (experiment log 29)
      if (native_ok || env == 0 || g.N < 512) return false;
      const int u = g.Cg < g.Cdg ? g.Cg : g.Cdg;   // the finer group
      if (g.Cg % u || g.Cdg % u) return false;
      const int m = g.Cdg / u;                      // finer groups per deformable group
      int cdp = 0;
      if (backward) {
        for (int cand : {64, 128, 256, 512, 768, 1024})
          if (cand >= g.Cdg && cand % m == 0) { cdp = cand; break; }
      } else {
        cdp = (g.Cdg + 2 * kBK * m - 1) / (2 * kBK * m) * (2 * kBK * m);   // finer groups of whole 32-channel stages
      }
      if (cdp == 0 || cdp > kPadMaxGrowth * g.Cdg) return false;
      p->ng = g.C / u; p->cin = u; p->cinp = cdp / m;
      p->wsub = g.Cg / u;
      gp.Cg = p->wsub * p->cinp;
      gp.Cdg = cdp;
      gp.C = p->ng * p->cinp;
    }
    gp.Og = p->ogp;
    gp.O = g.G * p->ogp;
  }
  p->pad_c = p->cinp != p->cin;
  p->pad_o = p->ogp != p->og;
  if (!p->pad_c && !p->pad_o) return false;
  if (!native_plan(gp, dtype, backward, &p->sub, skip)) return false;
  p->gp = gp;
  const size_t es = dtype == MDCONV_F32 ? 4 : 2;
  const size_t es_w = wgrad32 ? 4 : es;   // grad_weight / grad_bias (fp32 with MDCONV_WGRAD_F32)
  Bump ws;
  p->off_x = ws.take(p->pad_c ? (size_t)g.B * gp.C * g.S_i * es : 0);
  p->off_w = ws.take((size_t)gp.O * gp.Cg * g.K * es);
  // (a selective backward: no padded buffer of a skipped gradient)
  p->off_gi = ws.take(backward && p->pad_c && !skip.input ? (size_t)g.B * gp.C * g.S_i * es : 0);
  p->off_gw = ws.take(backward && !skip.weight ? (size_t)gp.O * gp.Cg * g.K * es_w : 0);
  p->off_o = ws.take(p->pad_o ? (size_t)g.B * gp.O * g.S_o * es : 0);
  p->off_b = ws.take(p->pad_o && g.with_bias && !backward ? (size_t)gp.O * es : 0);
  p->off_gb = ws.take(p->pad_o && g.with_bias && backward && !skip.weight ? (size_t)gp.O * es_w : 0);
  p->off_sub = ws.off;
  p->total = ws.off + p->sub.total;
  return true;
}
// input [B][groups][cin][S_i] -> [B][groups][cinp][S_i]; weight [groups_o][og][wsub][cin][K] -> [groups_o][ogp][wsub][cinp][K] (the
// rows og .. ogp - 1 of every output group zero): rows of one (image | output channel, group), contiguous on both sides
int pad_inputs(const Geom &g, int dtype, const PadPlan &p, const Tensors &t, char *base, Tensors *tp, hipStream_t stream) {
  const size_t es = dtype == MDCONV_F32 ? 4 : 2;
  int rc;
  if (p.pad_c) {
    if ((rc = pad_rows(base + p.off_x, (size_t)p.cinp * g.S_i * es, t.input, (size_t)p.cin * g.S_i * es, (size_t)g.B * p.ng, stream)))
      return rc;
    tp->input = base + p.off_x;
  }
  if ((rc = pad_rows_grouped(base + p.off_w, (size_t)p.cinp * g.K * es, t.weight, (size_t)p.cin * g.K * es, (size_t)p.og * p.wsub,
                             (size_t)p.ogp * p.wsub, p.nog, stream)))
    return rc;
  tp->weight = base + p.off_w;
  return MDCONV_OK;
}
int pad_forward(const Geom &g, int dtype, const PadPlan &p, const Tensors &t, void *ws, hipStream_t stream) {
  char *base = (char *)ws;
  const size_t es = dtype == MDCONV_F32 ? 4 : 2;
  int rc;
  Tensors tp = t;
  if ((rc = pad_inputs(g, dtype, p, t, base, &tp, stream))) return rc;
  if (p.pad_o) {   // the kernels write ogp output channels per group (and read as many bias values): a workspace tile, real rows copied out
    if (g.with_bias) {
      if ((rc = pad_rows(base + p.off_b, (size_t)p.ogp * es, t.bias, (size_t)p.og * es, p.nog, stream))) return rc;
      tp.bias = base + p.off_b;
    }
    tp.output = base + p.off_o;
  }
  if ((rc = native_forward(p.gp, dtype, p.sub, tp, base + p.off_sub, stream))) return rc;
  if (!p.pad_o) return MDCONV_OK;
  const size_t w_o = (size_t)p.og * g.S_o * es;
  return copy_rows(t.output, w_o, base + p.off_o, (size_t)p.ogp * g.S_o * es, w_o, (size_t)g.B * p.nog, stream);
}
int pad_backward(const Geom &g, int dtype, const PadPlan &p, const Tensors &t, void *ws, hipStream_t stream) {
  char *base = (char *)ws;
  const size_t es = dtype == MDCONV_F32 ? 4 : 2;
  const size_t w_x = (size_t)p.cin * g.S_i * es, p_x = (size_t)p.cinp * g.S_i * es;
  const size_t w_o = (size_t)p.og * g.S_o * es, p_o = (size_t)p.ogp * g.S_o * es;
  const size_t es_w = wgrad_bytes(dtype, t);   // grad_weight / grad_bias elements
  const size_t w_gw = (size_t)p.cin * g.K * es_w, p_gw = (size_t)p.cinp * g.K * es_w;
  const size_t wi = (size_t)p.og * p.wsub, wip = (size_t)p.ogp * p.wsub;   // weight rows of one output group (caller's / padded)
  const Skip skip = p.sub.skip;   // skipped gradients: no padded buffer, no copies in or out (the caller's pointers are NULL)
  int rc;
  Tensors tp = t;   // grad_offset / grad_mask have no channel axis: written in place, in the caller's mode
  if ((rc = pad_inputs(g, dtype, p, t, base, &tp, stream))) return rc;
  // accumulate modes: the padded gradient buffers start from the caller's values (like the slices above)
  if (p.pad_c && !skip.input) {
    if (g.acc_data && (rc = pad_rows(base + p.off_gi, p_x, t.grad_input, w_x, (size_t)g.B * p.ng, stream))) return rc;
    tp.grad_input = base + p.off_gi;
  }
  if (!skip.weight) {
    if (g.acc_w && (rc = pad_rows_grouped(base + p.off_gw, p_gw, t.grad_weight, w_gw, wi, wip, p.nog, stream))) return rc;
    tp.grad_weight = base + p.off_gw;
  }
  if (p.pad_o) {
    if ((rc = pad_rows(base + p.off_o, p_o, t.grad_output, w_o, (size_t)g.B * p.nog, stream))) return rc;   // zero planes for the padding channels
    tp.grad_output = base + p.off_o;
    if (g.with_bias && !skip.weight) {
      if (g.acc_w && (rc = pad_rows(base + p.off_gb, (size_t)p.ogp * es_w, t.grad_bias, (size_t)p.og * es_w, p.nog, stream))) return rc;
      tp.grad_bias = base + p.off_gb;
    }
  }
  if ((rc = native_backward(p.gp, dtype, p.sub, tp, base + p.off_sub, stream))) return rc;
  if (p.pad_c && !skip.input && (rc = copy_rows(t.grad_input, w_x, base + p.off_gi, p_x, w_x, (size_t)g.B * p.ng, stream))) return rc;
  if (skip.weight) return MDCONV_OK;
  if ((rc = unpad_rows_grouped(t.grad_weight, w_gw, base + p.off_gw, p_gw, wi, wip, p.nog, stream))) return rc;
  if (p.pad_o && g.with_bias &&
      (rc = copy_rows(t.grad_bias, (size_t)p.og * es_w, base + p.off_gb, (size_t)p.ogp * es_w, (size_t)p.og * es_w, p.nog, stream)))
    return rc;
  return record_weight_ready(stream);   // after the copy back
}
}  // namespace

bool mfma_plan(const Geom &g, int dtype, bool backward, MfmaPlan *p, bool wgrad32, Skip skip) {
  p->backward = backward;
  if (!backward) skip = Skip();
  p->skip = skip;
  const bool native_ok = native_plan(g, dtype, backward, &p->native, skip);
  // the padded problem where it is the faster one (pad_channels_preferred), else native tiling, else padded, else slices
  if ((pad_channels_preferred(g) || !native_ok) && pad_plan(g, dtype, backward, native_ok, wgrad32, skip, &p->pad)) {
    p->kind = MfmaPlan::PADDED;
    p->total = p->pad.total;
  } else if (native_ok) {
    p->kind = MfmaPlan::NATIVE;
    p->total = p->native.total;
  } else if (backward) {
    if (!split_plan(g, dtype, wgrad32, skip, &p->split_bwd)) return false;
    p->kind = MfmaPlan::SPLIT_BWD;
    p->total = p->split_bwd.total;
  } else {
    if (!split_fwd_plan(g, dtype, &p->split_fwd)) return false;
    p->kind = MfmaPlan::SPLIT_FWD;
    p->total = p->split_fwd.total;
  }
  return true;
}

bool mfma_supported(const Geom &g, int dtype, bool backward) {
  MfmaPlan p;
  return mfma_plan(g, dtype, backward, &p);
}

size_t mfma_workspace_bytes(const Geom &g, int dtype, bool backward) {
  MfmaPlan p;
  return mfma_plan(g, dtype, backward, &p) ? p.total : 0;
}

int mfma_forward(const Geom &g, int dtype, const MfmaPlan &p, const Tensors &t, void *ws, hipStream_t stream) {
  switch (p.kind) {
    case MfmaPlan::NATIVE: return native_forward(g, dtype, p.native, t, ws, stream);
    case MfmaPlan::PADDED: return pad_forward(g, dtype, p.pad, t, ws, stream);
    case MfmaPlan::SPLIT_FWD: return split_forward(g, dtype, p.split_fwd, t, ws, stream);
    default: set_error("mfma_forward: no plan"); return MDCONV_EUNSUPPORTED;
  }
}

int mfma_backward(const Geom &g, int dtype, const MfmaPlan &p, const Tensors &t, void *ws, hipStream_t stream) {
  switch (p.kind) {
    case MfmaPlan::NATIVE: return native_backward(g, dtype, p.native, t, ws, stream);
    case MfmaPlan::PADDED: return pad_backward(g, dtype, p.pad, t, ws, stream);
    case MfmaPlan::SPLIT_BWD: return split_backward(g, dtype, p.split_bwd, t, ws, stream);
    default: set_error("mfma_backward: no plan"); return MDCONV_EUNSUPPORTED;
  }
}

}  // namespace mdconv
