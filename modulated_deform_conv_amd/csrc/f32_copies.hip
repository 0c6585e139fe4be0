// f32_copies.hip -- 16-bit calls that run on fp32 kernels through fp32 copies in the workspace: the shape-generic
// backward (direct16) and calls with fp32 offsets / masks outside the native 16-bit kernels (samp32).
#include "mfma_plan.hpp"

namespace mdconv {

// ---------------------------------------------------------------------------------------------
// 16-bit tensors on the shape-generic backward: it scatters grad_input / grad_weight with atomics,
// and a 16-bit atomic rounds at EVERY add (bf16: 2^-9 each).  So the call runs on fp32 copies in
// the workspace -- fresh, zeroed gradient buffers -- and each gradient is rounded once on the way out.
// ---------------------------------------------------------------------------------------------
D16Plan direct16_plan(const Geom &g) {
  D16Plan p;
  Bump ws;
  const size_t n_x = (size_t)g.B * g.C * g.S_i * 4, n_off = (size_t)g.B * g.DG * g.nd * g.K * g.S_o * 4;
  const size_t n_m = (size_t)g.B * g.DG * g.K * g.S_o * 4, n_w = (size_t)g.O * g.Cg * g.K * 4, n_go = (size_t)g.B * g.O * g.S_o * 4;
  p.off_x = ws.take(n_x); p.off_off = ws.take(n_off); p.off_m = ws.take(n_m); p.off_w = ws.take(n_w); p.off_go = ws.take(n_go);
  p.off_gi = ws.take(n_x); p.off_goff = ws.take(n_off); p.off_gm = ws.take(n_m); p.off_gw = ws.take(n_w);
  p.off_gb = ws.take((size_t)g.O * 4);
  p.total = ws.off;
  return p;
}

int direct16_backward(const Geom &g, int dtype, const D16Plan &p, const Tensors &t, void *ws, hipStream_t stream, Skip skip) {
  char *base = (char *)ws;
  const int64_t n_x = (int64_t)g.B * g.C * g.S_i, n_off = (int64_t)g.B * g.DG * g.nd * g.K * g.S_o;
  const int64_t n_m = (int64_t)g.B * g.DG * g.K * g.S_o, n_w = (int64_t)g.O * g.Cg * g.K, n_go = (int64_t)g.B * g.O * g.S_o;
  int rc;
  if ((rc = widen(dtype, t.input, (float *)(base + p.off_x), n_x, stream))) return rc;
  if ((rc = widen(dtype, t.offset, (float *)(base + p.off_off), n_off, stream))) return rc;
  if (t.mask && (rc = widen(dtype, t.mask, (float *)(base + p.off_m), n_m, stream))) return rc;
  if ((rc = widen(dtype, t.weight, (float *)(base + p.off_w), n_w, stream))) return rc;
  if ((rc = widen(dtype, t.grad_output, (float *)(base + p.off_go), n_go, stream))) return rc;
  if ((rc = zero_bytes(base + p.off_gi, p.total - p.off_gi, stream))) return rc;   // the five gradient buffers are contiguous
  Tensors tc = t;
  tc.wgrad32 = 0;   // every tensor of the inner call is fp32
  tc.input = base + p.off_x; tc.offset = base + p.off_off; tc.mask = t.mask ? base + p.off_m : nullptr;
  tc.weight = base + p.off_w; tc.grad_output = base + p.off_go;
  tc.grad_input = base + p.off_gi; tc.grad_offset = base + p.off_goff;
  tc.grad_mask = t.grad_mask ? base + p.off_gm : nullptr;
  tc.grad_weight = base + p.off_gw; tc.grad_bias = base + p.off_gb;
  Geom gc = g;
  gc.acc_data = gc.acc_w = 1;   // the kernels add into the zeroed fp32 buffers
  // a selective backward: the weight kernel is not run, a skipped gradient stays in its fp32 buffer
  if ((rc = direct_backward(gc, MDCONV_F32, tc, stream, skip.weight ? 1 : 3))) return rc;
  if (!skip.input && (rc = narrow(dtype, (const float *)tc.grad_input, t.grad_input, n_x, g.acc_data != 0, stream))) return rc;
  if ((rc = narrow(dtype, (const float *)tc.grad_offset, t.grad_offset, n_off, g.acc_data != 0, stream))) return rc;
  if (t.grad_mask && (rc = narrow(dtype, (const float *)tc.grad_mask, t.grad_mask, n_m, g.acc_data != 0, stream))) return rc;
  if (skip.weight) return MDCONV_OK;
  if ((rc = narrow_wgrad(dtype, t, (const float *)tc.grad_weight, t.grad_weight, n_w, g.acc_w != 0, stream))) return rc;
  if (g.with_bias && (rc = narrow_wgrad(dtype, t, (const float *)tc.grad_bias, t.grad_bias, g.O, g.acc_w != 0, stream))) return rc;
  return MDCONV_OK;
}

// ---------------------------------------------------------------------------------------------
// 16-bit tensors with fp32 offsets / masks (MDCONV_SAMPLING_F32) where the native 16-bit kernels do not run: the call
// becomes an fp32 call of the same kernel family -- fp32 copies of input / weight / bias / grad_output in the workspace
// (the route every such 16-bit call takes anyway, one rounding per result), the caller's fp32 offset / mask read in place
// and its grad_offset / grad_mask written in place in the caller's mode (no widen, no narrow).  grad_input / grad_weight /
// grad_bias go through fp32 buffers that start from the caller's values in accumulate mode.
// ---------------------------------------------------------------------------------------------
void samp32_plan(const Geom &g, bool backward, bool want_mfma, S32Plan *p, Skip skip) {
  if (!backward) skip = Skip();
  p->skip = skip;
  p->mfma = want_mfma && mfma_plan(g, MDCONV_F32, backward, &p->inner, false, skip);
  // a selective backward on the matrix kernels: no fp32 buffer for a skipped gradient (the shape-generic data kernel
  // scatters grad_input whether it is wanted or not, so that route keeps the buffers)
  const bool no_gi = skip.input && p->mfma, no_gw = skip.weight && p->mfma;
  Bump ws;
  const size_t n_x = (size_t)g.B * g.C * g.S_i * 4, n_w = (size_t)g.O * g.Cg * g.K * 4, n_o = (size_t)g.B * g.O * g.S_o * 4;
  p->off_x = ws.take(n_x); p->off_w = ws.take(n_w); p->off_b = ws.take((size_t)g.O * 4); p->off_o = ws.take(n_o);
  p->off_gi = p->off_gw = ws.off;
  if (backward) { p->off_gi = ws.take(no_gi ? 0 : n_x); p->off_gw = ws.take(no_gw ? 0 : n_w + (size_t)g.O * 4); }   // grad_bias follows grad_weight
  p->off_inner = ws.off;
  p->total = ws.off + (p->mfma ? p->inner.total : 0);
}

int samp32_forward(const Geom &g, int dtype, const S32Plan &p, const Tensors &t, void *ws, hipStream_t stream) {
  const bool mfma = p.mfma;
  char *base = (char *)ws;
  const int64_t n_x = (int64_t)g.B * g.C * g.S_i, n_w = (int64_t)g.O * g.Cg * g.K, n_o = (int64_t)g.B * g.O * g.S_o;
  int rc;
  if ((rc = widen(dtype, t.input, (float *)(base + p.off_x), n_x, stream))) return rc;
  if ((rc = widen(dtype, t.weight, (float *)(base + p.off_w), n_w, stream))) return rc;
  if (g.with_bias && (rc = widen(dtype, t.bias, (float *)(base + p.off_b), g.O, stream))) return rc;
  Tensors tc = t;
  tc.samp32 = 0;   // every tensor of the inner call is fp32
  tc.input = base + p.off_x; tc.weight = base + p.off_w; tc.bias = g.with_bias ? base + p.off_b : nullptr;
  tc.output = base + p.off_o;
  rc = mfma ? mfma_forward(g, MDCONV_F32, p.inner, tc, base + p.off_inner, stream) : direct_forward(g, MDCONV_F32, tc, stream);
  if (rc) return rc;
  return narrow(dtype, (const float *)tc.output, t.output, n_o, false, stream);
}

int samp32_backward(const Geom &g, int dtype, const S32Plan &p, const Tensors &t, void *ws, hipStream_t stream) {
  const bool mfma = p.mfma;
  char *base = (char *)ws;
  const int64_t n_x = (int64_t)g.B * g.C * g.S_i, n_w = (int64_t)g.O * g.Cg * g.K, n_o = (int64_t)g.B * g.O * g.S_o;
  const int64_t n_off = (int64_t)g.B * g.DG * g.nd * g.K * g.S_o, n_m = (int64_t)g.B * g.DG * g.K * g.S_o;
  float *gi = (float *)(base + p.off_gi), *gw = (float *)(base + p.off_gw), *gb = gw + n_w;
  const Skip skip = p.skip;   // skipped gradients: no copies in or out; the matrix kernels get NULL for them
  int rc;
  if ((rc = widen(dtype, t.input, (float *)(base + p.off_x), n_x, stream))) return rc;
  if ((rc = widen(dtype, t.weight, (float *)(base + p.off_w), n_w, stream))) return rc;
  if ((rc = widen(dtype, t.grad_output, (float *)(base + p.off_o), n_o, stream))) return rc;
  // the shape-generic kernels add with atomics: their buffers start from the caller's values or from zero
  if (skip.input) {
    if (mfma) gi = nullptr;   // (the shape-generic data kernel scatters into the uninitialised buffer: never read)
  } else if (g.acc_data || !mfma) {
    if (g.acc_data) rc = widen(dtype, t.grad_input, gi, n_x, stream);
    else rc = zero_bytes(gi, (size_t)n_x * 4, stream);
    if (rc) return rc;
  }
  if (skip.weight) {
    gw = gb = nullptr;
  } else if (g.acc_w || !mfma) {
    if (g.acc_w && t.wgrad32) {   // fp32 grad_weight / grad_bias: the caller's values as they are, not through 16 bits
      if ((rc = store_f32((const float *)t.grad_weight, gw, n_w, false, stream))) return rc;
      if (g.with_bias && (rc = store_f32((const float *)t.grad_bias, gb, g.O, false, stream))) return rc;
    } else if (g.acc_w) {
      if ((rc = widen(dtype, t.grad_weight, gw, n_w, stream))) return rc;
      if (g.with_bias && (rc = widen(dtype, t.grad_bias, gb, g.O, stream))) return rc;
    } else if ((rc = zero_bytes(gw, (size_t)(n_w + g.O) * 4, stream))) {
      return rc;
    }
  }
  if (!mfma && !g.acc_data) {
    if ((rc = zero_bytes(t.grad_offset, (size_t)n_off * 4, stream))) return rc;
    if (t.grad_mask && (rc = zero_bytes(t.grad_mask, (size_t)n_m * 4, stream))) return rc;
  }
  Tensors tc = t;
  tc.samp32 = tc.wgrad32 = 0;   // every tensor of the inner call is fp32
  tc.input = base + p.off_x; tc.weight = base + p.off_w; tc.grad_output = base + p.off_o;
  tc.bias = nullptr;   // (the backward reads no bias)
  tc.grad_input = gi; tc.grad_weight = gw; tc.grad_bias = g.with_bias ? gb : nullptr;
  Geom gc = g;
  if (!mfma) gc.acc_data = gc.acc_w = 1;
  rc = mfma ? mfma_backward(gc, MDCONV_F32, p.inner, tc, base + p.off_inner, stream)
            : direct_backward(gc, MDCONV_F32, tc, stream, skip.weight ? 1 : 3);
  if (rc) return rc;
  // grad_weight / grad_bias first: the weights-ready event (mdconv_stream_wait_weight_ready) is recorded again once they
  // are in the caller's buffers
  if (!skip.weight) {
    if ((rc = narrow_wgrad(dtype, t, gw, t.grad_weight, n_w, false, stream))) return rc;
    if (g.with_bias && (rc = narrow_wgrad(dtype, t, gb, t.grad_bias, g.O, false, stream))) return rc;
    if ((rc = record_weight_ready(stream))) return rc;
  }
  return skip.input ? MDCONV_OK : narrow(dtype, gi, t.grad_input, n_x, false, stream);
}

}  // namespace mdconv
