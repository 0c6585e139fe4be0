// msda3_host.hip -- plan and execution of 3-D multi-scale deformable attention (msda3_plan.hpp): the family's own forward,
// coordinate-gradient and list kernels, the list builder and the channels-last gather of the sampling operators.
#include "msda3_plan.hpp"

namespace mdconv {

bool msda3_plan(const mdconv_msda3d_desc *d, bool backward, Msda3Plan *p, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = nullptr;
  const int64_t lim = (int64_t)1 << 31;
  const int esz = d->dtype == MDCONV_F32 ? 4 : 2;
  const int csz = d->coord_dtype == MDCONV_F32 ? 4 : 2;
  const int64_t K = (int64_t)d->levels * d->points;
  const int64_t C = (int64_t)d->heads * d->head_channels;
  const int64_t pairs = (int64_t)d->batch * d->queries;   // times heads below, once both factors are bounded
  int64_t S = 0;
  bool level_big = false;
  for (int l = 0; l < d->levels; ++l) {
    const int64_t plane = (int64_t)d->level_sz[l][1] * d->level_sz[l][2];   // below 2^62
    const int64_t rows = plane < lim ? plane * d->level_sz[l][0] : lim;     // T_l * H_l * W_l, checked per level
    if (rows >= lim) level_big = true;   // (and stays out of the sum, which then cannot overflow)
    else S += rows;
  }
  const bool skip_value = backward && (d->flags & MDCONV_FLAG_NO_GRAD_INPUT);
  const int64_t seg_stride = K * d->queries * 8;   // K <= 4096 once checked: no overflow
  // (each product is checked with its factors bounded by the checks before it, so none overflows 64 bits)
  if (esz == 4 && d->head_channels % 4) *why = "head_channels is not a multiple of 4 (fp32 rows of 16 bytes)";
  else if (esz == 2 && d->head_channels % 8) *why = "head_channels is not a multiple of 8 (16-bit rows of 16 bytes)";
  else if (K > 4096) *why = "levels * points exceeds 4096";
  else if (level_big || C >= lim || S >= lim || pairs >= lim || d->batch * S >= lim || d->batch * S * C >= lim / esz ||
           pairs * C >= lim / esz || pairs * d->heads >= lim || pairs * d->heads * K * 3 * csz >= lim)
    *why = "a tensor of the call has 2^31 bytes or more";
  else if (backward && !skip_value && (int64_t)d->batch * d->heads > 65535)
    *why = "batch * heads exceeds 65535 (the scatter lists of grad_value)";
  else if (backward && !skip_value && seg_stride >= lim)
    *why = "the list stride levels * points * queries * 8 reaches 2^31 (the scatter lists of grad_value)";
  if (*why) return false;

  Msda3Plan q = {};
  Msda3Geom &g = q.g;
  g.N = d->batch; g.M = d->heads; g.D = d->head_channels; g.C = (int)C; g.Lq = d->queries; g.L = d->levels; g.P = d->points;
  g.K = (int)K; g.S = (int)S; g.npairs = (int)(pairs * d->heads);
  int start = 0;
  for (int l = 0; l < MDCONV_MSDA_MAX_LEVELS; ++l) {
    const bool used = l < d->levels;
    g.lvT[l] = used ? d->level_sz[l][0] : 1;
    g.lvH[l] = used ? d->level_sz[l][1] : 1;
    g.lvW[l] = used ? d->level_sz[l][2] : 1;
    g.lvS[l] = used ? start : 0;
    if (used) start += g.lvT[l] * g.lvH[l] * g.lvW[l];
  }
  g.ln = samp_lanes(g.D, esz);
  g.acc = d->accumulate;
  q.dtype = d->dtype;
  q.coord_dtype = d->coord_dtype;
  q.backward = backward;
  q.det = backward && (d->flags & MDCONV_FLAG_DETERMINISTIC);
  q.skip_value = skip_value;
  q.total = 0;
  if (backward && !skip_value) {
    Bump ws;
    q.lists = scatter_lists_take(ws, g.N * g.M, g.S, seg_stride, q.det);
    q.total = ws.off;
  }
  *p = q;
  return true;
}

int msda3_forward(const Msda3Plan &p, const Msda3Tensors &t, hipStream_t stream) { return msda3_fwd_launch(p, t, stream); }

int msda3_backward(const Msda3Plan &p, const Msda3Tensors &t, void *ws, hipStream_t stream) {
  const Msda3Geom &g = p.g;
  const ScatterLists &L = p.lists;
  int rc;
  if ((rc = msda3_bwd_coord_launch(p, t, stream))) return rc;
  if (p.skip_value) return MDCONV_OK;
  rc = scatter_lists_build(L, ws, p.det, stream, [&](bool fill, int *cnt, const int *rowptr, void *entries) {
    msda3_list_launch(p, t, fill, cnt, rowptr, entries, stream);
  });
  if (rc) return rc;
  const SampGather ga = {g.N, g.S, g.Lq, g.M, g.D, g.C, g.ln, g.acc};
  return samp_gather_launch(ga, p.dtype, L.seg_stride, t.grad_output, (const int *)((char *)ws + L.off_rowptr),
                            (char *)ws + L.off_entries, t.grad_value, stream);
}

}  // namespace mdconv
