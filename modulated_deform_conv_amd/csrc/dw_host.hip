// dw_host.hip -- plan and execution of the depthwise family (dw_plan.hpp).
#include "dw_plan.hpp"

namespace mdconv {

bool dw_plan(const Geom &g, int dtype, bool backward, DwPlan *p, Skip skip, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = nullptr;
  const int64_t lim = (int64_t)1 << 31;
  const int64_t n_off = (int64_t)g.B * g.DG * g.nd * g.K * g.S_o;
  const int64_t seg_stride = (int64_t)g.K * g.S_o * (1 << g.nd);
  if (dtype != MDCONV_F32) *why = "the tensors are not fp32 (MDCONV_F32)";
  else if (g.G != g.C || g.C < 2) *why = "the layer is not depthwise: groups == C_in >= 2";
  else if (g.C % 4) *why = "C_in is not a multiple of 4";
  else if (g.O % g.C || g.O / g.C > 4) *why = "the channel multiplier C_out / C_in is not 1, 2, 3 or 4";
  else if (g.Cdg % 4) *why = "C_in / deformable_groups is not a multiple of 4";
  else if (g.in_cl) *why = "the input is channels-last (fp32 inputs are [B, C, spatial...])";
  else if ((int64_t)g.B * g.C * g.S_i * 4 >= lim || (int64_t)g.B * g.O * g.S_o * 4 >= lim || n_off * 4 >= lim ||
           (int64_t)g.O * g.K * 4 >= lim)
    *why = "a tensor of the call has 2^31 bytes or more (the family has no batch chunks)";
  else if (seg_stride >= lim || g.C / 4 > 65535)
    *why = "K * output pixels * 2^ndim reaches 2^31 (scatter-list offsets), or C_in exceeds the grid";
  if (*why) return false;

  DwPlan q = {};
  q.g = g;
  q.backward = backward;
  q.skip = backward ? skip : Skip();
  q.M = g.O / g.C;
  q.cs = g.Cdg % 8 == 0 ? 8 : 4;
  q.cs_gi = q.cs;
  q.total = 0;
  if (backward) {
    q.tiles = (g.N + kDwTile - 1) / kDwTile;
    const int nchunk = g.Cdg / 4;            // four-channel chunks of one deformable group, dealt to the waves in turn
    const int max_split = (nchunk + 3) / 4;  // beyond it a workgroup would have a wave without channels
    // enough workgroups for the 256 CUs where the pixel tiles alone are few (512 -> 512 at 14 x 14, B = 8: 25 tiles)
    int cs = (int)((1024 + (int64_t)q.tiles * g.DG - 1) / ((int64_t)q.tiles * g.DG));
    if (cs > kDwMaxSplit) cs = kDwMaxSplit;
    if (cs > max_split) cs = max_split;
    if (cs < 1) cs = 1;
    if ((int64_t)g.DG * cs > 65535) { *why = "deformable_groups exceeds the grid"; return false; }
    q.csplit = cs;
    Bump ws;
    q.off_goff = ws.take(cs > 1 ? (size_t)cs * n_off * 4 : 0);
    q.off_gm = ws.take(cs > 1 && g.modulated ? (size_t)cs * (n_off / g.nd) * 4 : 0);
    if (!q.skip.weight) {
      q.row_len = g.O * g.K + (g.with_bias ? g.O : 0);
      q.row_groups = q.tiles > kDwRowGroup ? (q.tiles + kDwRowGroup - 1) / kDwRowGroup : 0;
      q.off_wpart = ws.take((size_t)q.tiles * q.row_len * 4);
      q.off_wstage = ws.take((size_t)q.row_groups * q.row_len * 4);
    }
    if (!q.skip.input) {
      q.off_wt = ws.take((size_t)g.O * g.K * 4);
      q.lists = scatter_lists_take(ws, g.B * g.DG, g.S_i, seg_stride, g.det != 0);
    }
    q.total = ws.off;
  }
  *p = q;
  return true;
}

int dw_forward(const DwPlan &p, const Tensors &t, hipStream_t stream) { return dw_fwd_launch(p, t, stream); }

int dw_backward(const DwPlan &p, const Tensors &t, void *ws, hipStream_t stream) {
  const Geom &g = p.g;
  char *base = (char *)ws;
  int rc;
  float *part_off = p.csplit > 1 ? (float *)(base + p.off_goff) : nullptr;
  float *part_m = p.csplit > 1 && g.modulated ? (float *)(base + p.off_gm) : nullptr;
  float *wpart = p.skip.weight ? nullptr : (float *)(base + p.off_wpart);
  if ((rc = dw_bwd_coord_launch(p, t, part_off, part_m, wpart, stream))) return rc;
  if (!p.skip.weight) {
    // the partial rows of the pixel tiles, added in row order (two stages from kDwRowGroup rows)
    const float *rows = wpart;
    int nrows = p.tiles;
    if (p.row_groups) {
      float *stage = (float *)(base + p.off_wstage);
      if ((rc = dw_reduce_rows(wpart, p.row_len, p.tiles, p.row_len, kDwRowGroup, stage, p.row_len, false, stream))) return rc;
      rows = stage;
      nrows = p.row_groups;
    }
    if ((rc = dw_reduce_rows(rows, p.row_len, nrows, g.O * g.K, nrows, (float *)t.grad_weight, 0, g.acc_w != 0, stream))) return rc;
    if (g.with_bias &&
        (rc = dw_reduce_rows(rows + (size_t)g.O * g.K, p.row_len, nrows, g.O, nrows, (float *)t.grad_bias, 0, g.acc_w != 0, stream)))
      return rc;
    if ((rc = record_weight_ready(stream))) return rc;
  }
  if (p.csplit > 1) {
    const int64_t n_off = (int64_t)g.B * g.DG * g.nd * g.K * g.S_o;
    if ((rc = dw_reduce_rows(part_off, n_off, p.csplit, (int)n_off, p.csplit, (float *)t.grad_offset, 0, g.acc_data != 0, stream)))
      return rc;
    if (g.modulated && (rc = dw_reduce_rows(part_m, n_off / g.nd, p.csplit, (int)(n_off / g.nd), p.csplit, (float *)t.grad_mask, 0,
                                            g.acc_data != 0, stream)))
      return rc;
  }
  if (p.skip.input) return MDCONV_OK;
  float *wt = (float *)(base + p.off_wt);
  if ((rc = dw_weight_table_launch(p, (const float *)t.weight, wt, stream))) return rc;
  rc = scatter_lists_build(p.lists, ws, g.det != 0, stream, [&](bool fill, int *cnt, const int *rowptr, void *entries) {
    dw_list_launch(p, t, fill, cnt, rowptr, entries, stream);
  });
  if (rc) return rc;
  return dw_gather_launch(p, t, (const int *)(base + p.lists.off_rowptr), base + p.lists.off_entries, wt, stream);
}

}  // namespace mdconv
