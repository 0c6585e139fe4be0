/*
 * mdconv_fdap.h -- packed deformable attention with a point count per level: the C ABI of one more sampling operator of
 * libmdconv_hip.so, in a header of its own.  It includes mdconv.h (the error codes, the dtype enum, the flags,
 * MDCONV_MSDA_MAX_LEVELS, mdconv_last_error) and follows its conventions: dense row-major tensors on the current HIP
 * device, `stream` a hipStream_t, a caller-owned workspace, 0 or a negative MDCONV_E* code.  The ABI version stays
 * MDCONV_ABI_VERSION (2): nothing in mdconv.h changes.
 *
 * The operator is the union of two existing ones: the tap layout of mdconv_msdap.h (levels that each own points[l] taps;
 * RT-DETRv2's `num_points_list`, D-FINE and DEIM: (3, 6, 3)) with the packed tensor and the in-kernel softmax of "Packed
 * deformable attention" of mdconv.h (mdconv_fda_*).  N images, M heads of D channels, Lq queries, L levels
 * (1..MDCONV_MSDA_MAX_LEVELS), level l with points[l] points, K = sum_l points[l] taps per (query, head):
 *     value              [N, S, M, D]     S = sum_l H_l*W_l: the levels concatenated in order, each row-major (y*W_l + x)
 *     sampling_loc_attn  [N, Lq, M, 3K]   per (query, head): the 2K location coordinates, (x, y) of tap 0 .. K-1, normalised
 *                                         (0..1 spans the tap's level), then the K attention LOGITS; no padding columns
 *     output             [N, Lq, M*D]
 *     the taps are LEVEL-MAJOR: level 0 owns taps 0 .. points[0]-1, level 1 the next points[1], and so on
 *     a[n,q,m,:] = softmax over ALL K logits of (n, q, m), in fp32 with the maximum subtracted
 *     x = loc_x * W_l - 0.5,   y = loc_y * H_l - 0.5                    (pixel coordinates in the tap's level l)
 *     out[n,q,m,:] = sum_k a[n,q,m,k] * bilinear(value[n, start_l(k) + ., m, :], y, x)
 * With equal counts this is mdconv_fda_* on the same memory, bit for bit (grad_value with MDCONV_FLAG_DETERMINISTIC).
 * Everything else is the contract of the two operators, word for word:
 *  - start_l is the cumulative sum of the extents before level l: the level starts are not an input.
 *  - bilinear reads the four neighbours of (y, x); a neighbour outside the level contributes zero and is never loaded.  A
 *    sample contributes iff -1 < x < W_l and -1 < y < H_l; a NaN or infinite coordinate (a location that overflows once
 *    scaled by the extent included) therefore contributes nothing, to the output and to every gradient, and its location
 *    gradient is exactly zero.  For finite coordinates the OUTPUT equals grid_sample with zero padding and align_corners =
 *    false everywhere, and so do the gradients off the lattice and away from the edge of the gate.  On the lattice the
 *    derivative is the right-sided one of the cell floor(x), floor(y); a gated-out sample has location gradient exactly
 *    zero, also at x == -1 and x == W_l exactly.
 *  - The softmax includes the logits of taps whose sample is gated out: such a tap takes its share of the weight and
 *    contributes nothing.  Its LOGIT gradient is therefore -a[t] * S, not zero -- the mathematics of the softmax, as for
 *    mdconv_fda_* -- where S is the pair sum below.  Non-finite LOGITS: the result is unspecified, as for mdconv_fda_*.
 *  - The backward takes no `output`.  It returns grad_value and grad_sampling_loc_attn in the layouts of their forward
 *    tensors: the location gradients (which carry the factors W_l for x and H_l for y) in the first 2K elements of a row,
 *    the logit gradients a[t] * (g[t] - S) behind them, with g[t] the dot product of grad_output with the tap's bilinear
 *    sample and S = sum_t a[t] g[t], both from fp32 sums of the call.  `accumulate` is the write mode of
 *    mdconv_desc.accumulate.
 *  - dtype (MDCONV_F32, MDCONV_F16 or MDCONV_BF16) is the type of value, output, grad_output and grad_value; coord_dtype is
 *    the type of sampling_loc_attn and its gradient: equal to dtype, or MDCONV_F32 -- five pairings.  All arithmetic is
 *    fp32, each result is rounded once.
 *  - Every points[l] with l < levels is positive, else MDCONV_EINVAL naming the level; entries beyond `levels` are ignored.
 *  - Shape rule (else MDCONV_EUNSUPPORTED, with the rule in the error message, before anything is launched): that of
 *    mdconv_msdap.h -- D a multiple of 4 for fp32 and of 8 for 16-bit values (rows of 16 bytes), every tensor below 2^31
 *    bytes, K <= 4096, and for a backward with grad_value N*M <= 65535 and the list stride K*Lq*4 below 2^31 -- with the
 *    packed tensor among the tensors: N*Lq*M*3K elements of coord_dtype stay below 2^31 bytes.
 *  - flags: MDCONV_FLAG_DETERMINISTIC and MDCONV_FLAG_NO_GRAD_INPUT only (the latter: no grad_value); any other bit is
 *    MDCONV_EINVAL.  No result is summed with floating-point atomics: output and grad_sampling_loc_attn are bit-identical
 *    from call to call, grad_value is with MDCONV_FLAG_DETERMINISTIC and agrees to rounding otherwise.  With
 *    MDCONV_FLAG_NO_GRAD_INPUT grad_value may be NULL and is never touched; the packed gradient is bit for bit that of the
 *    full call.  Forwards ignore both flags.
 *  - Pointer alignment ("Pointer alignment" in mdconv.h): value, output, grad_output and grad_value are "16-byte";
 *    sampling_loc_attn and grad_sampling_loc_attn are "element" (coord_dtype).
 *  - A call checks in this order: the descriptor (MDCONV_EINVAL), the pointers -- NULL (MDCONV_ENULL), then alignment
 *    (MDCONV_EINVAL, naming the argument) --, the shape rule (MDCONV_EUNSUPPORTED), the workspace (MDCONV_EWORKSPACE: size
 *    and 16-byte alignment).
 *  - The workspace figure is exact: that of mdconv_msdap_* for the shape plus 8 bytes per (query, head) for the softmax
 *    statistics (rounded up to 256), 0 for the forward and 0 with MDCONV_FLAG_NO_GRAD_INPUT.  A call is a plain chain of
 *    kernels on the caller's stream: no second stream, no host synchronisation; it captures into a HIP graph.
 *  Like its two parents, written from memory of the published operators and UNPINNED against their code; the yardstick is
 *  a softmax over the K logits in front of the per-level grid_sample composition ("Packed deformable
 *  attention with a point count per level").
 */
#ifndef MDCONV_FDAP_H_
#define MDCONV_FDAP_H_

#include "mdconv.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mdconv_fdap_desc {
  int dtype;           /* value, output, grad_output, grad_value: MDCONV_F32 / MDCONV_F16 / MDCONV_BF16 */
  int coord_dtype;     /* sampling_loc_attn and its gradient: `dtype` or MDCONV_F32 */
  int batch;           /* N */
  int heads;           /* M */
  int head_channels;   /* D */
  int queries;         /* Lq */
  int levels;          /* L, 1..MDCONV_MSDA_MAX_LEVELS */
  int points[MDCONV_MSDA_MAX_LEVELS];       /* points of the first `levels` levels, each positive; the others are ignored */
  int level_sz[MDCONV_MSDA_MAX_LEVELS][2];  /* (H_l, W_l) of the first `levels` rows; the others are ignored */
  int accumulate;      /* backward write mode: 1 = add to grad_*, 0 = overwrite */
  int flags;           /* MDCONV_FLAG_DETERMINISTIC | MDCONV_FLAG_NO_GRAD_INPUT */
} mdconv_fdap_desc;
/* `mdconv_fdap_desc d = MDCONV_FDAP_DESC_INIT;` then fill in the shape (fp32, accumulate, no flags) */
#define MDCONV_FDAP_DESC_INIT { 0, 0, 0, 0, 0, 0, 0, {0}, {{0, 0}}, 1, 0 }

/* S, the rows of `value` per image: the sum of H_l*W_l over the levels; -1 for a bad descriptor. */
int mdconv_fdap_value_len(const mdconv_fdap_desc *d);
/* 3K, the elements of sampling_loc_attn per (query, head): three times the sum of points[l]; -1 for a bad descriptor. */
int mdconv_fdap_loc_attn_len(const mdconv_fdap_desc *d);
/* Scratch bytes of the forward (backward = 0: always 0) or the backward (backward = 1) of `d`; 0 for a descriptor that is
 * invalid or outside the shape rule. */
size_t mdconv_fdap_workspace_bytes(const mdconv_fdap_desc *d, int backward);
int mdconv_fdap_forward(const mdconv_fdap_desc *d, const void *value, const void *sampling_loc_attn, void *output,
                        void *workspace, size_t workspace_bytes, void *stream);
int mdconv_fdap_backward(const mdconv_fdap_desc *d, const void *value, const void *sampling_loc_attn, const void *grad_output,
                         void *grad_value, void *grad_sampling_loc_attn, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MDCONV_FDAP_H_ */
