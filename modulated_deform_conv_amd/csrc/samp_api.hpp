// samp_api.hpp -- the entry-point layer, host only: what every C entry point does before it launches anything, written
// once.  The pointer checks are the convolution API's as well (mdconv_api.hip); everything below them serves the sampling
// operators (DCNv3, DCNv4, multi-scale deformable attention in 2-D and 3-D, packed deformable attention, deformable RoI
// pooling, deformable aggregation), whose extern "C" functions live beside their planner in the operator's *_host.hip.
//
// The order of checks of a sampling entry point (samp_entry; DESIGN.md, "The entry-point layer"):
//   1. the descriptor's own validation          MDCONV_EINVAL         the operator's *_validate, from the desc_* pieces here
//   2. every pointer the call uses is non-NULL  MDCONV_ENULL          check_args, in the order of the argument table
//   3. every such pointer is in its class       MDCONV_EINVAL         check_args again, in the same order
//   4. the shape rule (the operator's *_plan)   MDCONV_EUNSUPPORTED   samp_refuse
//   5. the workspace                            MDCONV_EWORKSPACE     check_ws
// and then the operator's run.  The sizing query (samp_workspace_bytes) is steps 1 and 4.
// Everything here has internal linkage: the library exports the C API and nothing of this layer.
#pragma once
#include <stdint.h>

#include <initializer_list>

#include "host_util.hpp"

namespace mdconv {

static inline void clear_error() { set_error("%s", ""); }

// ---- the pointer checks ----
static inline int require(const void *p, const char *name) {
  if (!p) {
    set_error("%s pointer is NULL", name);
    return MDCONV_ENULL;
  }
  return MDCONV_OK;
}

// Pointer alignment ("Pointer alignment"; include/mdconv.h states the class of every argument): a tensor pointer is
// aligned to its class -- `align` = the tensor's element size ("element": every access through it is one element wide, a raw
// buffer load at an element-aligned offset, or behind a pointer test with an element-wise fallback) or 16 ("16-byte": the
// kernels move 16-byte vectors through it).  Checked after the NULL checks and before the shape rule and the workspace; a
// pointer the call ignores (NULL where that is allowed, a skipped gradient, bias without with_bias) is not looked at.
static inline int require_aligned(const void *p, const char *name, size_t align) {
  if (p && ((uintptr_t)p & (align - 1)) != 0) {
    set_error("%s pointer must be %zu-byte aligned", name, align);
    return MDCONV_EINVAL;
  }
  return MDCONV_OK;
}
static inline size_t dtype_bytes(int dt) { return dt == MDCONV_F64 ? 8 : (dt == MDCONV_F32 ? 4 : 2); }

static inline int check_ws(void *ws, size_t have, size_t need) {
  if (need == 0) return MDCONV_OK;
  if (!ws || have < need) {
    set_error("workspace too small: need %zu bytes, have %zu", need, have);
    return MDCONV_EWORKSPACE;
  }
  if (((uintptr_t)ws & 15) != 0) {
    set_error("workspace must be 16-byte aligned");
    return MDCONV_EWORKSPACE;
  }
  return MDCONV_OK;
}

// The argument table of an entry point: its tensor pointers, each once, IN THE ORDER THEY ARE CHECKED -- the pointers every
// call needs first, then the ones a call may ignore (`used` false: the gradient of the sampled tensor under
// MDCONV_FLAG_NO_GRAD_INPUT; offset / grad_offset of deformable RoI pooling without with_offset).  All NULL checks run before
// the first alignment check.
struct SampArg {
  const void *p;
  const char *name;
  size_t align;   // 16, or the element size
  bool used = true;
};
static inline int check_args(std::initializer_list<SampArg> args) {
  int rc;
  for (const SampArg &a : args)
    if (a.used && (rc = require(a.p, a.name))) return rc;
  for (const SampArg &a : args)
    if (a.used && (rc = require_aligned(a.p, a.name, a.align))) return rc;
  return MDCONV_OK;
}

// ---- the descriptor checks the operators share, under the operator's name ----
// NULL descriptor and dtype; coord_dtype (every operator but DCNv3, whose coordinates have the values' type)
template <class Desc> static int desc_dtype(const char *op, const Desc *d) {
  if (!d) {
    set_error("descriptor pointer is NULL");
    return MDCONV_EINVAL;
  }
  if (d->dtype != MDCONV_F32 && d->dtype != MDCONV_F16 && d->dtype != MDCONV_BF16) {
    set_error("%s: dtype %d is not MDCONV_F32, MDCONV_F16 or MDCONV_BF16 (the dtype flags do not apply)", op, d->dtype);
    return MDCONV_EINVAL;
  }
  return MDCONV_OK;
}
template <class Desc> static int desc_dtypes(const char *op, const Desc *d) {
  if (int rc = desc_dtype(op, d)) return rc;
  if (d->coord_dtype != d->dtype && d->coord_dtype != MDCONV_F32) {
    set_error("%s: coord_dtype %d is neither dtype (%d) nor MDCONV_F32", op, d->coord_dtype, d->dtype);
    return MDCONV_EINVAL;
  }
  return MDCONV_OK;
}
// accumulate, and flags against the operator's mask: the two flags of every operator, MDCONV_FLAG_SOFTMAX where `softmax`
template <class Desc> static int desc_modes(const char *op, const Desc *d, bool softmax = false) {
  if (d->accumulate != 0 && d->accumulate != 1) {
    set_error("%s: accumulate must be 0 or 1, is %d", op, d->accumulate);
    return MDCONV_EINVAL;
  }
  const int allowed = MDCONV_FLAG_DETERMINISTIC | MDCONV_FLAG_NO_GRAD_INPUT | (softmax ? MDCONV_FLAG_SOFTMAX : 0);
  if (d->flags & ~allowed) {
    set_error("%s: unknown bits 0x%x in flags; the flags are MDCONV_FLAG_DETERMINISTIC (1)%s MDCONV_FLAG_NO_GRAD_INPUT (4)%s", op,
              (unsigned)(d->flags & ~allowed), softmax ? "," : " and", softmax ? " and MDCONV_FLAG_SOFTMAX (256)" : "");
    return MDCONV_EINVAL;
  }
  return MDCONV_OK;
}
// the level table: the count, and the extents of the levels in use -- rows of (H, W) or of (T, H, W)
template <class Desc> static int desc_levels(const char *op, const Desc *d) {
  if (d->levels < 1 || d->levels > MDCONV_MSDA_MAX_LEVELS) {
    set_error("%s: levels must be 1..%d, is %d", op, MDCONV_MSDA_MAX_LEVELS, d->levels);
    return MDCONV_EINVAL;
  }
  constexpr int kAxes = (int)(sizeof(d->level_sz[0]) / sizeof(int));
  for (int l = 0; l < d->levels; ++l) {
    const int *e = d->level_sz[l];
    bool bad = false;
    for (int a = 0; a < kAxes; ++a) bad = bad || e[a] <= 0;
    if (bad) {
      if (kAxes == 2) set_error("%s: level %d has a non-positive extent (%d x %d)", op, l, e[0], e[1]);
      else set_error("%s: level %d has a non-positive extent (%d x %d x %d)", op, l, e[0], e[1], e[kAxes - 1]);
      return MDCONV_EINVAL;
    }
  }
  return MDCONV_OK;
}
static inline int desc_finite(const char *op, const char *field, float v) {
  if (!(v == v) || v - v != 0.f) {
    set_error("%s: %s is not finite", op, field);
    return MDCONV_EINVAL;
  }
  return MDCONV_OK;
}
// the convolution-style geometry of DCNv3 and DCNv4, whose descriptors name it alike
template <class Desc> static int desc_dcn_geometry(const char *op, const Desc *d) {
  if (d->batch <= 0 || d->groups <= 0 || d->group_channels <= 0) {
    set_error("%s: batch, groups and group_channels must be positive (%d, %d, %d)", op, d->batch, d->groups, d->group_channels);
    return MDCONV_EINVAL;
  }
  for (int a = 0; a < 2; ++a) {
    if (d->in_sz[a] <= 0 || d->k_sz[a] <= 0 || d->stride[a] <= 0 || d->dil[a] <= 0 || d->pad[a] < 0) {
      set_error("%s: bad geometry on axis %d (in_sz=%d, k_sz=%d, stride=%d, pad=%d, dil=%d)", op, a, d->in_sz[a], d->k_sz[a],
                d->stride[a], d->pad[a], d->dil[a]);
      return MDCONV_EINVAL;
    }
    const long long span = (long long)d->dil[a] * (d->k_sz[a] - 1) + 1;
    if ((long long)d->in_sz[a] + 2LL * d->pad[a] < span) {
      set_error("%s: the output extent on axis %d is below 1 (in_sz=%d, pad=%d, dilated kernel %lld)", op, a, d->in_sz[a],
                d->pad[a], span);
      return MDCONV_EINVAL;
    }
  }
  return MDCONV_OK;
}
// (in_sz + 2 pad - dilated kernel) / stride + 1 of a validated DCNv3 / DCNv4 descriptor; mdconv_dcnv*_out_size guards itself
template <class Desc> static int64_t dcn_out_size(const Desc *d, int a) {
  return (d->in_sz[a] + 2 * (int64_t)d->pad[a] - ((int64_t)d->dil[a] * (d->k_sz[a] - 1) + 1)) / d->stride[a] + 1;
}

// the whole validation of the three attention operators (msda, fda, msda3d), whose descriptors have the same fields
template <class Desc> static int attn_validate(const char *op, const Desc *d) {
  if (int rc = desc_dtypes(op, d)) return rc;
  if (d->batch <= 0 || d->heads <= 0 || d->head_channels <= 0 || d->queries <= 0 || d->points <= 0) {
    set_error("%s: batch, heads, head_channels, queries and points must be positive (%d, %d, %d, %d, %d)", op, d->batch, d->heads,
              d->head_channels, d->queries, d->points);
    return MDCONV_EINVAL;
  }
  if (int rc = desc_levels(op, d)) return rc;
  return desc_modes(op, d);
}

static inline int samp_refuse(const char *op, const char *why) {
  set_error("%s: outside the shape rule of the operator: %s", op, why);
  return MDCONV_EUNSUPPORTED;
}

// ---- the skeleton ----
// What an operator is to it: its name in the error texts, its validation, its planner (false: outside the shape rule, *why
// names the rule; the plan's `total` is the workspace).
template <class Desc, class Plan> struct SampOp {
  const char *name;
  int (*validate)(const Desc *d, bool backward);
  bool (*plan)(const Desc *d, bool backward, Plan *p, const char **why);
};
// the plan of a validated descriptor, or the refusal under the operator's name
template <class Desc, class Plan>
static int samp_planned(const SampOp<Desc, Plan> &op, const Desc *d, bool backward, Plan *p) {
  const char *why;
  return op.plan(d, backward, p, &why) ? MDCONV_OK : samp_refuse(op.name, why);
}
// `args()` checks the argument table (it may read the validated descriptor), `run(plan)` fills the operator's tensors and
// executes.  The caller has cleared the error text.
template <class Desc, class Plan, class Args, class Run>
static int samp_entry(const SampOp<Desc, Plan> &op, const Desc *d, bool backward, void *ws, size_t ws_bytes, Args args, Run run) {
  int rc;
  Plan p;
  if ((rc = op.validate(d, backward)) || (rc = args()) || (rc = samp_planned(op, d, backward, &p)) ||
      (rc = check_ws(ws, ws_bytes, p.total)))
    return rc;
  return run(p);
}
template <class Desc, class Plan>
static size_t samp_workspace_bytes(const SampOp<Desc, Plan> &op, const Desc *d, int backward) {
  Plan p;
  if (op.validate(d, backward != 0) || samp_planned(op, d, backward != 0, &p)) return 0;
  return p.total;
}

// ---- planner helpers ----
// Rows of the levels of a validated descriptor, H * W or T * H * W each: -1 where a level or the sum reaches 2^31 (a level
// that does stays out of the sum, and no product is formed from a factor of 2^31 or more, so nothing overflows 64 bits).
template <class Desc> static int64_t level_rows(const Desc *d) {
  constexpr int kAxes = (int)(sizeof(d->level_sz[0]) / sizeof(int));
  const int64_t lim = (int64_t)1 << 31;
  int64_t S = 0;
  for (int l = 0; l < d->levels; ++l) {
    int64_t rows = 1;
    for (int a = kAxes - 1; a >= 0; --a) rows = rows < lim ? rows * d->level_sz[l][a] : lim;
    if (rows >= lim) return -1;
    S += rows;
  }
  return S < lim ? S : -1;
}
// the level tables of a *Geom: extents and start row of the levels in use, (1, 1) at row 0 for the others
template <class Geom, class Desc> static void level_fill(Geom &g, const Desc *d) {
  constexpr int kAxes = (int)(sizeof(d->level_sz[0]) / sizeof(int));
  int start = 0;
  for (int l = 0; l < MDCONV_MSDA_MAX_LEVELS; ++l) {
    const bool used = l < d->levels;
    int rows = 1;
    if constexpr (kAxes == 3) rows = g.lvT[l] = used ? d->level_sz[l][0] : 1;
    g.lvH[l] = used ? d->level_sz[l][kAxes - 2] : 1;
    g.lvW[l] = used ? d->level_sz[l][kAxes - 1] : 1;
    g.lvS[l] = used ? start : 0;
    if (used) start += rows * g.lvH[l] * g.lvW[l];
  }
}
// The tail of a planner: the direction, deterministic mode, and the scatter lists of the sampled tensor's gradient -- the
// operator's whole workspace unless it takes more from the returned Bump -- where the backward computes that gradient
// (`skip`: MDCONV_FLAG_NO_GRAD_INPUT, stated by the caller, whose plan names the field after its tensor).
template <class Plan>
static Bump samp_plan_lists(Plan &q, bool backward, int flags, bool skip, int nseg, int rows, int64_t seg_stride) {
  Bump ws;
  q.backward = backward;
  q.det = backward && (flags & MDCONV_FLAG_DETERMINISTIC);
  if (backward && !skip) q.lists = scatter_lists_take(ws, nseg, rows, seg_stride, q.det);
  q.total = ws.off;
  return ws;
}

}  // namespace mdconv
