/*
 * mdconv_afda.h -- anchored packed deformable attention: the C ABI of one more sampling operator of libmdconv_hip.so, in
 * a header of its own.  It includes mdconv.h (the error codes, the dtype enum, the flags, MDCONV_MSDA_MAX_LEVELS,
 * mdconv_last_error) and follows its conventions: dense row-major tensors on the current HIP device, `stream` a
 * hipStream_t, a caller-owned workspace, 0 or a negative MDCONV_E* code.  The ABI version stays MDCONV_ABI_VERSION (2):
 * nothing in mdconv.h changes.
 *
 * The operator is mdconv_fdap_* (mdconv_fdap.h) with the reference arithmetic of the decoder blocks inside the kernels: it
 * takes the packed row of RAW sampling offsets and attention logits, as one linear layer produced it, and the reference
 * points or boxes, and forms the sampling locations itself (the decoder attention of RT-DETRv2, D-FINE and DEIM; with
 * two-component references the form of the Deformable-DETR and DINO decoders).  N images, M heads of D channels, Lq queries,
 * L levels (1..MDCONV_MSDA_MAX_LEVELS), level l with points[l] points, K = sum_l points[l] taps per (query, head):
 *     value             [N, S, M, D]     S = sum_l H_l*W_l: the levels concatenated in order, each row-major (y*W_l + x)
 *     reference_points  [N, Lq, Lr, R]   ALWAYS fp32; Lr = 1 (one row for all levels) or Lr = L (one per level); R = 2
 *                                        (x, y) or R = 4 (x, y, w, h); normalised (0..1 spans a level)
 *     offs_attn         [N, Lq, M, 3K]   coord_dtype; per (query, head): (dx, dy) of tap 0 .. K-1, then the K attention
 *                                        LOGITS; the taps are LEVEL-MAJOR as in mdconv_msdap.h; no padding columns
 *     output            [N, Lq, M*D]
 *     l = the level of tap k (prefix sums of points[]);   r = l if Lr == L, else 0;   s_k = 1 / points[l]
 *     R == 4:  loc_x = rx + dx * s_k * rw * offset_scale        loc_y = ry + dy * s_k * rh * offset_scale
 *     R == 2:  loc_x = rx + dx / W_l                            loc_y = ry + dy / H_l
 *     x = loc_x * W_l - 0.5,   y = loc_y * H_l - 0.5            (pixel coordinates in the tap's level l)
 *     a[n,q,m,:] = softmax over ALL K logits of (n, q, m), in fp32 with the maximum subtracted
 *     out[n,q,m,:] = sum_k a[n,q,m,k] * bilinear(value[n, start_l(k) + ., m, :], y, x)
 * The normalised location is formed in fp32 (for R == 2 by a multiplication with the fp32 reciprocal of the extent) and from
 * there on the operator IS mdconv_fdap_*: where the factors make the location the stored offset -- references (0, 0, 1, 1)
 * and s_k * offset_scale = 1 with both powers of two -- output, packed gradient and (with MDCONV_FLAG_DETERMINISTIC)
 * grad_value are those of mdconv_fdap_* on the same memory, bit for bit.
 *  - The gate, the bilinear sample, the lattice rule and the softmax are those of mdconv_fdap.h, word for word.  A sample
 *    contributes iff -1 < x < W_l and -1 < y < H_l; a NaN or infinite offset, or a NaN or infinite element in the tap's
 *    reference row, makes the coordinate non-finite and the tap GATED OUT.  A gated-out tap contributes EXACTLY zero to the
 *    output, to grad_value, to its own offset gradient and to grad_reference_points (selected, not multiplied: no 0 * NaN);
 *    it keeps its share of the softmax, so its logit gradient is -a[t] * S.  Non-finite LOGITS: unspecified.
 *  - The backward takes no `output`.  With G_x, G_y the pixel-space location gradients of tap k (a[k] times the derivative
 *    of the bilinear sample along x / y dotted with grad_output):
 *      grad_offs_attn         the layout of offs_attn.  Offsets, R == 4: G_x * W_l * (s_k * rw * offset_scale), likewise y
 *                             with H_l and rh; R == 2: G_x * W_l * (1 / W_l), likewise y.  Logits: a[t] * (g[t] - S) as in
 *                             mdconv_fdap.h.
 *      grad_reference_points  [N, Lq, Lr, R], fp32: rx += G_x * W_l, ry += G_y * H_l, and for R == 4 rw += G_x * W_l * dx *
 *                             s_k * offset_scale, rh likewise -- summed over the M heads and the taps that read row r in a
 *                             FIXED order, without floating-point atomics: bit-identical from call to call.
 *    `accumulate` is the write mode of mdconv_desc.accumulate, for all three gradients.  With grad_reference == 0
 *    grad_reference_points may be NULL and is never touched, its stage and its workspace are left out, and every other
 *    result is bit for bit that of the full call.
 *  - dtype (MDCONV_F32, MDCONV_F16 or MDCONV_BF16) is the type of value, output, grad_output and grad_value; coord_dtype is
 *    the type of offs_attn and its gradient: equal to dtype, or MDCONV_F32 -- five pairings.  The two reference tensors are
 *    fp32 in every pairing.  All arithmetic is fp32, each result is rounded once.
 *  - Every points[l] with l < levels is positive, else MDCONV_EINVAL naming the level.  ref_levels is 1 or `levels`,
 *    ref_comps 2 or 4, offset_scale finite (unused for R == 2), grad_reference 0 or 1, else MDCONV_EINVAL.
 *  - Shape rule (else MDCONV_EUNSUPPORTED, with the rule in the error message, before anything is launched): that of
 *    mdconv_fdap.h with offs_attn in the place of sampling_loc_attn.
 *  - flags: MDCONV_FLAG_DETERMINISTIC and MDCONV_FLAG_NO_GRAD_INPUT only (the latter: no grad_value, which may then be NULL
 *    and is never touched; the other gradients are bit for bit those of the full call).  output, grad_offs_attn and
 *    grad_reference_points are bit-identical from call to call, grad_value is with MDCONV_FLAG_DETERMINISTIC.
 *  - Pointer alignment ("Pointer alignment" in mdconv.h): value, output, grad_output and grad_value are "16-byte";
 *    reference_points and grad_reference_points (fp32) and offs_attn and grad_offs_attn (coord_dtype) are "element".
 *  - A call checks in this order: the descriptor (MDCONV_EINVAL), the pointers -- NULL (MDCONV_ENULL), then alignment
 *    (MDCONV_EINVAL, naming the argument) --, the shape rule (MDCONV_EUNSUPPORTED), the workspace (MDCONV_EWORKSPACE: size
 *    and 16-byte alignment).
 *  - The workspace figure is exact: that of mdconv_fdap_* for the shape (0 for the forward and with
 *    MDCONV_FLAG_NO_GRAD_INPUT) plus, with grad_reference, 4 * Lr * R bytes per (query, head) rounded up to 256.  A call is a
 *    plain chain of kernels on the caller's stream: no second stream, no host synchronisation; it captures into a HIP graph.
 *  Written from memory of the published blocks (RT-DETRv2's MSDeformableAttention and the Deformable-DETR decoder) and
 *  UNPINNED against their code; the yardstick is the published location formulas in framework operators in front of the
 *  yardstick of mdconv_fdap.h ("Anchored packed deformable attention").
 */
#ifndef MDCONV_AFDA_H_
#define MDCONV_AFDA_H_

#include "mdconv.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mdconv_afda_desc {
  int dtype;           /* value, output, grad_output, grad_value: MDCONV_F32 / MDCONV_F16 / MDCONV_BF16 */
  int coord_dtype;     /* offs_attn and its gradient: `dtype` or MDCONV_F32 */
  int batch;           /* N */
  int heads;           /* M */
  int head_channels;   /* D */
  int queries;         /* Lq */
  int levels;          /* L, 1..MDCONV_MSDA_MAX_LEVELS */
  int points[MDCONV_MSDA_MAX_LEVELS];       /* points of the first `levels` levels, each positive; the others are ignored */
  int level_sz[MDCONV_MSDA_MAX_LEVELS][2];  /* (H_l, W_l) of the first `levels` rows; the others are ignored */
  int accumulate;      /* backward write mode: 1 = add to grad_*, 0 = overwrite */
  int flags;           /* MDCONV_FLAG_DETERMINISTIC | MDCONV_FLAG_NO_GRAD_INPUT */
  int ref_levels;      /* Lr: 1 or `levels` */
  int ref_comps;       /* R: 2 (x, y) or 4 (x, y, w, h) */
  float offset_scale;  /* R == 4 only; finite */
  int grad_reference;  /* backward: 1 = grad_reference_points is computed, 0 = it is not (and may be NULL) */
} mdconv_afda_desc;
/* `mdconv_afda_desc d = MDCONV_AFDA_DESC_INIT;` then fill in the shape (fp32, accumulate, no flags, one box per query,
 * offset_scale 0.5, with grad_reference) */
#define MDCONV_AFDA_DESC_INIT { 0, 0, 0, 0, 0, 0, 0, {0}, {{0, 0}}, 1, 0, 1, 4, 0.5f, 1 }

/* S, the rows of `value` per image: the sum of H_l*W_l over the levels; -1 for a bad descriptor. */
int mdconv_afda_value_len(const mdconv_afda_desc *d);
/* 3K, the elements of offs_attn per (query, head): three times the sum of points[l]; -1 for a bad descriptor. */
int mdconv_afda_offs_attn_len(const mdconv_afda_desc *d);
/* Scratch bytes of the forward (backward = 0: always 0) or the backward (backward = 1) of `d`; 0 for a descriptor that is
 * invalid or outside the shape rule. */
size_t mdconv_afda_workspace_bytes(const mdconv_afda_desc *d, int backward);
int mdconv_afda_forward(const mdconv_afda_desc *d, const void *value, const void *reference_points, const void *offs_attn,
                        void *output, void *workspace, size_t workspace_bytes, void *stream);
int mdconv_afda_backward(const mdconv_afda_desc *d, const void *value, const void *reference_points, const void *offs_attn,
                         const void *grad_output, void *grad_value, void *grad_reference_points, void *grad_offs_attn,
                         void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MDCONV_AFDA_H_ */
