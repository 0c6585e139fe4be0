/*
 * mdconv_dagg.h -- deformable aggregation: the C ABI of one more sampling operator of libmdconv_hip.so, in a header of its
 * own.  It includes mdconv.h (the error codes, the dtype enum, the flags, MDCONV_MSDA_MAX_LEVELS, mdconv_last_error) and
 * follows its conventions: dense row-major tensors on the current HIP device, `stream` a hipStream_t, a caller-owned
 * workspace, 0 or a negative MDCONV_E* code.  The ABI version stays MDCONV_ABI_VERSION (2): nothing in mdconv.h changes.
 *
 * The operator is the `deformable_aggregation` of multi-camera 3-D detectors (Sparse4D v2 / v3, SparseDrive): for every
 * anchor, P key points are projected into `cams` cameras, and the features of all cameras and all L pyramid levels at
 * those points are summed with one weight per (point, camera, level, channel group).  B images, `cams` cameras, L levels
 * (1..MDCONV_MSDA_MAX_LEVELS), C = G*Dg channels in G groups, A anchors, P points:
 *     feature            [B, S, C]              channels-last.  The maps are concatenated camera-major, level-minor:
 *                                               (cam 0, level 0), (cam 0, level 1), ..., (cam 1, level 0), ...; each map
 *                                               row-major (y*W_l + x).  EVERY CAMERA HAS THE SAME LEVEL EXTENTS (H_l, W_l):
 *                                               S_cam = sum_l H_l*W_l, S = cams*S_cam (mdconv_dagg_feature_len), and map
 *                                               (cam, l) starts at row cam*S_cam + start_l, start_l the cumulative sum.
 *                                               Cameras of different resolutions are outside the operator (a documented
 *                                               limit: the descriptor cannot express them).
 *     sampling_location  [B, A, P, cams, 2]     last axis (x, y), normalised: 0..1 spans the map
 *     weights            [B, A, P, cams, L, G]
 *     output             [B, A, C]
 *     gate(b,a,p,cam) = 0 < x < 1 and 0 < y < 1, taken on the stored elements (converted exactly to fp32) before any
 *                       arithmetic: NaN, +-Inf, exactly 0.0 and exactly 1.0 are OUT
 *     output[b,a,g*Dg+d] = sum_{p,cam,l} gate(b,a,p,cam) * weights[b,a,p,cam,l,g]
 *                                        * bilinear(map (cam, l) of image b, x*W_l - 0.5, y*H_l - 0.5)[g*Dg+d]
 *  - bilinear reads the four neighbours; a neighbour outside the map contributes zero and is never loaded.  Inside the gate
 *    this is grid_sample (mode "bilinear", zero padding, align_corners = false) at grid = 2*loc - 1, in the output and, off
 *    the lattice, in the gradients.  On the lattice (an integer pixel coordinate) the derivative is the right-sided one of
 *    the cell floor(x), floor(y), as for the other sampling operators.
 *  - A gated-out (b, a, p, cam) reads neither `feature` nor its L*G weights: a NaN weight there reaches no result.  Its
 *    elements of grad_weights and grad_sampling_location are exact zeros in overwrite mode and are not touched in
 *    accumulate mode; likewise a row of grad_feature that no sample touches is zero in overwrite mode and is neither read nor
 *    written in accumulate mode (it keeps its bits).  A call with NaN, Inf or huge locations equals, bit for bit, the call with those locations at -3.0.
 *  - The backward returns grad_feature, grad_sampling_location and grad_weights in the layouts of their forward tensors.
 *    grad_weights has one element per (b,a,p,cam,l,g); grad_sampling_location[b,a,p,cam,:] is the sum over all L levels
 *    and all G groups of weight * d(sample)/d(x, y) * (W_l, H_l).  `accumulate` is the write mode of mdconv_desc.accumulate.
 *  - dtype (MDCONV_F32, MDCONV_F16 or MDCONV_BF16) is the type of feature, output, grad_output and grad_feature; coord_dtype
 *    is the type of sampling_location, weights and their gradients: equal to dtype, or MDCONV_F32 -- the five pairings of
 *    the attention operators.  All arithmetic is fp32, each stored element is rounded once.
 *  - Shape rule (else MDCONV_EUNSUPPORTED, with the rule in mdconv_last_error(), before anything is launched): Dg a multiple
 *    of 4 for fp32 and of 8 for 16-bit values (group rows of 16 bytes); B*S rows and every tensor below 2^31 (rows, bytes);
 *    and for a backward with grad_feature B <= 65535 and the list stride A*P*cams*L*4 below 2^31.
 *  - flags: MDCONV_FLAG_DETERMINISTIC and MDCONV_FLAG_NO_GRAD_INPUT only (the latter: no grad_feature); any other bit is
 *    MDCONV_EINVAL.  No result is summed with floating-point atomics: output, grad_weights and grad_sampling_location are
 *    bit-identical from call to call, grad_feature is with MDCONV_FLAG_DETERMINISTIC and agrees to rounding otherwise.  With
 *    MDCONV_FLAG_NO_GRAD_INPUT grad_feature may be NULL and is never touched; the other gradients are bit for bit those of
 *    the full call.  Forwards ignore both flags.
 *  - Pointer alignment ("Pointer alignment" in mdconv.h): feature, output, grad_output and grad_feature are "16-byte";
 *    sampling_location, weights and their gradients are "element" (coord_dtype).
 *  - A call checks in this order: the descriptor (MDCONV_EINVAL), the pointers -- NULL (MDCONV_ENULL), then alignment
 *    (MDCONV_EINVAL, naming the argument) --, the shape rule (MDCONV_EUNSUPPORTED), the workspace (MDCONV_EWORKSPACE: size
 *    and 16-byte alignment).
 *  - The workspace figure is exact, 0 for the forward and with MDCONV_FLAG_NO_GRAD_INPUT, and honours
 *    MDCONV_FLAG_DETERMINISTIC.  A call is a plain chain of kernels on the caller's stream: no second stream, no host
 *    synchronisation; it captures into a HIP graph.
 *  The published operator's source was not available to this project: the contract above is this project's statement of
 *  it, and fidelity to the published CUDA operator is UNPINNED.  The yardstick is the per-(camera, level) grid_sample
 *  composition times the gate ("Deformable aggregation").
 */
#ifndef MDCONV_DAGG_H_
#define MDCONV_DAGG_H_

#include "mdconv.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mdconv_dagg_desc {
  int dtype;           /* feature, output, grad_output, grad_feature: MDCONV_F32 / MDCONV_F16 / MDCONV_BF16 */
  int coord_dtype;     /* sampling_location, weights and their gradients: `dtype` or MDCONV_F32 */
  int batch;           /* B */
  int cams;            /* cameras per image */
  int levels;          /* L, 1..MDCONV_MSDA_MAX_LEVELS */
  int level_sz[MDCONV_MSDA_MAX_LEVELS][2];  /* (H_l, W_l) of the first `levels` rows, of every camera; the others are ignored */
  int channels;        /* C = groups * Dg */
  int groups;          /* G, a divisor of `channels` */
  int anchors;         /* A */
  int points;          /* P */
  int accumulate;      /* backward write mode: 1 = add to grad_*, 0 = overwrite */
  int flags;           /* MDCONV_FLAG_DETERMINISTIC | MDCONV_FLAG_NO_GRAD_INPUT */
} mdconv_dagg_desc;
/* `mdconv_dagg_desc d = MDCONV_DAGG_DESC_INIT;` then fill in the shape (fp32, accumulate, no flags) */
#define MDCONV_DAGG_DESC_INIT { 0, 0, 0, 0, 0, {{0, 0}}, 0, 0, 0, 0, 1, 0 }

/* S, the rows of `feature` per image: cams * sum_l H_l*W_l; -1 for a bad descriptor. */
int mdconv_dagg_feature_len(const mdconv_dagg_desc *d);
/* Scratch bytes of the forward (backward = 0: always 0) or the backward (backward = 1) of `d`; 0 for a descriptor that is
 * invalid or outside the shape rule. */
size_t mdconv_dagg_workspace_bytes(const mdconv_dagg_desc *d, int backward);
int mdconv_dagg_forward(const mdconv_dagg_desc *d, const void *feature, const void *sampling_location, const void *weights,
                        void *output, void *workspace, size_t workspace_bytes, void *stream);
int mdconv_dagg_backward(const mdconv_dagg_desc *d, const void *feature, const void *sampling_location, const void *weights,
                         const void *grad_output, void *grad_feature, void *grad_sampling_location, void *grad_weights,
                         void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MDCONV_DAGG_H_ */
