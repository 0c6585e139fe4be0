// msda_host.hip -- plan and execution of multi-scale deformable attention (msda_plan.hpp): the sampling core's kernels
// (samp_core.hpp) instantiated with MsdaOp for the five (value type, coordinate type) pairings.
#include "msda_plan.hpp"

namespace mdconv {

bool msda_plan(const mdconv_msda_desc *d, bool backward, MsdaPlan *p, const char **why) {
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
    const int64_t rows = (int64_t)d->level_sz[l][0] * d->level_sz[l][1];
    if (rows >= lim) level_big = true;   // (and stays out of the sum, which then cannot overflow)
    else S += rows;
  }
  const bool skip_value = backward && (d->flags & MDCONV_FLAG_NO_GRAD_INPUT);
  const int64_t seg_stride = K * d->queries * 4;   // K <= 4096 once checked: no overflow
  // (each product is checked with its factors bounded by the checks before it, so none overflows 64 bits)
  if (esz == 4 && d->head_channels % 4) *why = "head_channels is not a multiple of 4 (fp32 rows of 16 bytes)";
  else if (esz == 2 && d->head_channels % 8) *why = "head_channels is not a multiple of 8 (16-bit rows of 16 bytes)";
  else if (K > 4096) *why = "levels * points exceeds 4096";
  else if (level_big || C >= lim || S >= lim || pairs >= lim || d->batch * S >= lim || d->batch * S * C >= lim / esz ||
           pairs * C >= lim / esz || pairs * d->heads >= lim || pairs * d->heads * K * 2 * csz >= lim)
    *why = "a tensor of the call has 2^31 bytes or more";
  else if (backward && !skip_value && (int64_t)d->batch * d->heads > 65535)
    *why = "batch * heads exceeds 65535 (the scatter lists of grad_value)";
  else if (backward && !skip_value && seg_stride >= lim)   // (stated for the 32-bit slots of the lists; sampling_locations,
                                                          // K * Lq * 2 elements per pair, is at least as large in bytes)
    *why = "the list stride levels * points * queries * 4 reaches 2^31 (the scatter lists of grad_value)";
  if (*why) return false;

  MsdaPlan q = {};
  MsdaGeom &g = q.g;
  g.N = d->batch; g.M = d->heads; g.D = d->head_channels; g.C = (int)C; g.Lq = d->queries; g.L = d->levels; g.P = d->points;
  g.K = (int)K; g.S = (int)S; g.npairs = (int)(pairs * d->heads);
  int start = 0;
  for (int l = 0; l < MDCONV_MSDA_MAX_LEVELS; ++l) {
    const bool used = l < d->levels;
    g.lvH[l] = used ? d->level_sz[l][0] : 1;
    g.lvW[l] = used ? d->level_sz[l][1] : 1;
    g.lvS[l] = used ? start : 0;
    if (used) start += g.lvH[l] * g.lvW[l];
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

int msda_forward(const MsdaPlan &p, const MsdaTensors &t, hipStream_t stream) {
#define MSDA_FWD(DT, CT) samp_fwd_launch<MsdaOp, DT, CT>(p.g, t.value, t.loc, t.attn, t.output, stream)
  MSDA_DISPATCH(p, MSDA_FWD);
#undef MSDA_FWD
  return check_launch("msda_fwd");
}

int msda_backward(const MsdaPlan &p, const MsdaTensors &t, void *ws, hipStream_t stream) {
  const MsdaGeom &g = p.g;
  const ScatterLists &L = p.lists;
  int rc;
#define MSDA_BWD(DT, CT) \
  samp_bwd_coord_launch<MsdaOp, DT, CT>(g, t.value, t.loc, t.attn, t.grad_output, t.grad_loc, t.grad_attn, stream)
  MSDA_DISPATCH(p, MSDA_BWD);
#undef MSDA_BWD
  if ((rc = check_launch("msda_bwd_coord"))) return rc;
  if (p.skip_value) return MDCONV_OK;
  rc = scatter_lists_build(L, ws, p.det, stream, [&](bool fill, int *cnt, const int *rowptr, void *entries) {
#define MSDA_LIST(DT, CT) samp_list_launch<MsdaOp, CT>(g, fill, t.loc, t.attn, cnt, rowptr, entries, L.seg_stride, stream)
    MSDA_DISPATCH(p, MSDA_LIST);   // (by coordinate type: three instances)
#undef MSDA_LIST
  });
  if (rc) return rc;
  const SampGather ga = {g.N, g.S, g.Lq, g.M, g.D, g.C, g.ln, g.acc};
  return samp_gather_launch(ga, p.dtype, L.seg_stride, t.grad_output, (const int *)((char *)ws + L.off_rowptr),
                            (char *)ws + L.off_entries, t.grad_value, stream);
}

}  // namespace mdconv
