/*
 * mdconv.h -- C ABI of the MI355X-native (gfx950) deformable-convolution library
 * (libmdconv_hip.so).
 *
 * This is the drop-in boundary.  The reference's boundary is the CPython extension module
 * `MDCONV_CUDA` (reference setup.py:37, imported at modulated_deform_conv.py:7) whose eight free
 * functions take at::Tensor handles.  Each entry point below replaces exactly one of those
 * eight; the tensor handles become plain device pointers, the shapes travel in `mdconv_desc`.
 * The Python-side binding that re-creates the `MDCONV_CUDA` module on top of this ABI is
 * modulated_deform_conv_amd/MDCONV_CUDA.py (ctypes); INTEGRATION.md shows the stub.
 *
 * Conventions
 *  - All tensors are contiguous, row-major, on the current HIP device, in the layouts of the
 *    reference:
 *      input  [B, C_in, H, W(, L)]           weight [C_out, C_in/groups, kh, kw(, kl)]
 *      bias   [C_out] (ignored when !with_bias)  output [B, C_out, Ho, Wo(, Lo)]
 *      offset [B, DG*nd*K, Ho, Wo(, Lo)], channel = dg*nd*K + nd*tap + axis, axis order (h, w[, l])
 *      mask   [B, DG*K,    Ho, Wo(, Lo)], channel = dg*K + tap,   tap = (i*kw + j)[*kl + k]
 *  - `stream` is a hipStream_t (NULL = the null stream).  Calls are asynchronous on it.
 *  - `workspace` is caller-owned device scratch of at least mdconv_workspace_bytes() bytes,
 *    16-byte aligned; it may be NULL when that function returns 0.
 *  - Pointer alignment.  Every tensor pointer has one of two classes (the audit behind them: DESIGN.md, "Pointer alignment"):
 *    "element" -- aligned to the tensor's element (2, 4 or 8 bytes), which every dense view of a framework tensor is, at any
 *    storage offset -- or "16-byte".  The eight entry points of this section take every tensor "element" (offset, mask and
 *    their gradients: 4 bytes with MDCONV_SAMPLING_F32; grad_weight and grad_bias: 4 bytes with MDCONV_WGRAD_F32), with three
 *    exceptions, the tensors the kernels move as channels-last vectors: `input` with MDCONV_LAYOUT_CHANNELS_LAST, the forward's
 *    `output` with MDCONV_FLAG_OUTPUT_CHANNELS_LAST and `grad_input` with MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST are "16-byte".
 *    (A channels-last `grad_output` stays "element"; the backward never reads `bias`: that pointer is not looked at.)  The
 *    sampling operators further down take the sampled tensor, `output`, `grad_output` and the sampled tensor's gradient
 *    "16-byte" and every coordinate tensor "element"; each states its rule.  A pointer below its class is MDCONV_EINVAL, with
 *    the argument's name and the alignment in mdconv_last_error(): checked after the NULL checks (MDCONV_ENULL) and before the
 *    shape rule, the routing refusals (MDCONV_EUNSUPPORTED) and the workspace (MDCONV_EWORKSPACE); nothing is launched.
 *    Pointers a call ignores (a skipped gradient, `bias` without with_bias, `offset` without with_offset) are not checked.
 *    Results do not depend on the alignment: DESIGN.md lists, per tensor, which are bit-identical at any address.
 *  - Backward entry points ACCUMULATE into every grad_* buffer, which is what the reference's
 *    caller-allocated entry points do (deformable_conv.cu:327-333; the Python wrapper zero-fills,
 *    modulated_deform_conv.py:53-56).  For the modulated-2D op, whose reference entry point
 *    allocates zeros itself (mdeformable_conv.cu:404-411), the binding passes uninitialised
 *    buffers and asks for overwrite mode in the descriptor (`accumulate = 0`, ABI v2).
 *  - `in_step` is accepted for signature parity (reference README.md:30-31) and validated
 *    (> 0); results never depend on it (the reference's own modulated-2D op is in_step-invariant).
 *  - Return value: 0 on success, a negative MDCONV_E* code otherwise; mdconv_last_error() gives
 *    the message for the calling thread.  Unlike the reference (which printf()s and swallows
 *    launch errors, mdeformable_conv.cu:113-117) kernel launch failures are reported.
 */
#ifndef MDCONV_H_
#define MDCONV_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  v1: the eight entry points, call modes as thread-local / process-wide setters
 * (mdconv_set_accumulate, mdconv_set_input_layout, mdconv_set_path).  v2 (this header): the call
 * modes travel IN THE DESCRIPTOR (`accumulate`, `input_layout`, `path`), so a C caller has no hidden
 * state between its calls.  Binary compatibility: a v2 caller ORs MDCONV_DESC_V2 into `ndim`; the
 * library reads the v2 tail of the struct only then.  A descriptor without the tag (a caller built
 * against the v1 header, whose struct ends at `with_bias`) keeps v1 behaviour: the setters apply. */
#define MDCONV_ABI_VERSION 2
#define MDCONV_DESC_V2 0x100   /* flag in mdconv_desc.ndim: the descriptor carries the v2 fields */

/* AT_DISPATCH_FLOATING_TYPES_AND_HALF (mdeformable_conv.cu:101) + bfloat16 */
enum { MDCONV_F32 = 0, MDCONV_F16 = 1, MDCONV_F64 = 2, MDCONV_BF16 = 3 };
/* "fp32 sampling": flag ORed into mdconv_desc.dtype -- MDCONV_F16 | MDCONV_SAMPLING_F32 or
 * MDCONV_BF16 | MDCONV_SAMPLING_F32.  offset, mask, grad_offset and grad_mask are then fp32 while
 * input, weight, bias, output, grad_output, grad_input, grad_weight and grad_bias keep the 16-bit
 * type: sampling positions are not rounded to 16 bits (a bf16 offset of 32-64 px is a multiple of
 * 0.25 px).  Every shape and call mode of the 16-bit type runs with it, on the same kernel family.
 * With MDCONV_F32 / MDCONV_F64 the flag is MDCONV_EINVAL. */
#define MDCONV_SAMPLING_F32 0x10
/* "fp32 weight gradients": flag ORed into mdconv_desc.dtype next to MDCONV_SAMPLING_F32 (the two combine freely) --
 * MDCONV_F16 | MDCONV_WGRAD_F32, MDCONV_BF16 | MDCONV_SAMPLING_F32 | MDCONV_WGRAD_F32, ...  The backward's grad_weight and
 * grad_bias are then fp32 buffers ([C_out, C_in/groups, k...] and [C_out] floats) while every other tensor keeps its type.
 * Every 16-bit backward sums these two gradients in fp32 and rounds them once on the way out; with the flag that last
 * rounding is left out: overwrite mode (`accumulate` = 0) stores the fp32 sums, accumulate mode adds them to the buffers in
 * fp32 (grad = grad + sum, one fp32 add per element).  So a sum over B x S_o samples that exceeds the fp16 range stays
 * finite, fp32 master weights receive all 24 bits, and micro-batches or data-parallel ranks accumulate without a 16-bit
 * round trip.  The flag never changes the route of a call (kernel family, plan, batch chunks); the workspace can grow by
 * the wider grad_weight rows of a padded or sliced plan (mdconv_workspace_bytes honours the flag).  The weights-ready event
 * is recorded once the fp32 buffers are final.  Forward entry points accept and ignore the flag, so one descriptor serves
 * both directions.  With MDCONV_F32 / MDCONV_F64 the flag is MDCONV_EINVAL.
 * (The value skips 0x20: callers and tests written against earlier releases rely on `MDCONV_F16 | 0x20` being
 * MDCONV_EINVAL, like every other dtype value that was invalid before the flag existed; it still is.) */
#define MDCONV_WGRAD_F32 0x40

enum {
  MDCONV_OK = 0,
  MDCONV_EINVAL = -1,    /* bad descriptor / shape mismatch (reference: AT_ERROR -> RuntimeError) */
  MDCONV_ENULL = -2,     /* a required pointer is NULL */
  MDCONV_EWORKSPACE = -3,/* workspace too small / misaligned */
  MDCONV_ELAUNCH = -4,   /* HIP launch or runtime error */
  MDCONV_EUNSUPPORTED = -5
};

/* Kernel-path selector (tests and benchmarks): AUTO picks the depthwise kernels for the layers they take (below), else
 * the MFMA implicit-GEMM kernels when the shape qualifies and the direct (VALU) kernels otherwise.
 * MDCONV_PATH_DEPTHWISE forces the depthwise family: the call runs on it or returns MDCONV_EUNSUPPORTED, with the rule it
 * breaks in mdconv_last_error(), before anything is launched (the contract of MDCONV_PATH_MFMA).  MDCONV_PATH_DIRECT and
 * MDCONV_PATH_MFMA never reach that family: they route a depthwise layer as releases without it did.
 * Under AUTO one size rule applies, from measurement: several deformable groups of a multiple of 64 channels, with C_in <= 256 and
 * at least 4096 output pixels, keep the route of earlier releases (faster there); MDCONV_PATH_DEPTHWISE takes them.
 * Depthwise layers (the shape rule of the family): MDCONV_F32 tensors, input [B, C, spatial...], groups == C_in >= 2,
 * C_in a multiple of 4, C_out / C_in of 1, 2, 3 or 4, C_in / deformable_groups a multiple of 4, every tensor below 2^31
 * bytes; 2-D and 3-D, modulated or not, any kernel size, stride, padding and dilation, with or without bias.  No result is
 * summed with floating-point atomics: output, grad_offset, grad_mask, grad_weight and grad_bias are bit-identical from call
 * to call, grad_input is under MDCONV_FLAG_DETERMINISTIC and agrees to rounding otherwise.  MDCONV_FLAG_MATH_BF16 has
 * nothing to do there (mdconv_math_bf16_used answers 0): the call runs exact. */
enum { MDCONV_PATH_AUTO = 0, MDCONV_PATH_DIRECT = 1, MDCONV_PATH_MFMA = 2, MDCONV_PATH_DEPTHWISE = 3 };

typedef struct mdconv_desc {
  int ndim;       /* 2 or 3, | MDCONV_DESC_V2 when the v2 fields below are filled in */
  int modulated;  /* 0 = DeformConv (DCNv1), 1 = ModulatedDeformConv (DCNv2) */
  int dtype;      /* MDCONV_F32 / F16 / F64 / BF16 -- element type of every tensor (offset / mask and their
                     gradients: fp32 when MDCONV_SAMPLING_F32 is ORed in; grad_weight / grad_bias: fp32 when
                     MDCONV_WGRAD_F32 is, see above) */
  int batch;      /* B */
  int c_in;       /* C_in  */
  int c_out;      /* C_out */
  int in_sz[3];   /* H, W, L   (L = 1 when ndim == 2) */
  int k_sz[3];    /* kh, kw, kl (kl = 1 when ndim == 2) */
  int stride[3];  /* (…, 1)  */
  int pad[3];     /* (…, 0)  */
  int dil[3];     /* (…, 1)  */
  int groups;     /* `group` of the reference signature */
  int dgroups;    /* `deformable_group` */
  int in_step;    /* accepted, validated > 0, otherwise unused */
  int with_bias;
  /* ---- ABI v2: read only when ndim carries MDCONV_DESC_V2 (use MDCONV_DESC_INIT) ---- */
  int accumulate;   /* backward write mode: 1 = ACCUMULATE into grad_* (the reference's caller-allocated
                       entry points), 0 = OVERWRITE grad_* (buffers need not be initialised) */
  int input_layout; /* MDCONV_LAYOUT_NCHW or MDCONV_LAYOUT_CHANNELS_LAST (see below) */
  int path;         /* MDCONV_PATH_AUTO = the process default (MDCONV_PATH / mdconv_set_path), or a forced
                       MDCONV_PATH_DIRECT / MDCONV_PATH_MFMA / MDCONV_PATH_DEPTHWISE for this call */
  int reserved[5];  /* reserved[0..3] must be 0; reserved[4] is the per-call FLAGS word (MDCONV_FLAG_*, below):
                       any bit other than the flags defined here is MDCONV_EINVAL */
} mdconv_desc;

/* Per-call flags, in the last slot of the v2 tail (`flags` = mdconv_desc.reserved[4]; MDCONV_DESC_FLAGS(&d) names it).
 * A descriptor without MDCONV_DESC_V2 ends before the word and never requests a flag.
 *
 * MDCONV_FLAG_DETERMINISTIC -- deterministic mode.  With the flag, on one device, one build of the library and the
 * same descriptor and inputs, EVERY output of forward and backward is bit-identical from call to call: in accumulate
 * and in overwrite mode, eager or replayed from a HIP graph, whatever else runs on the GPU.  Nothing is promised across
 * batch sizes, devices or builds.  Without it all results but one already are (on the matrix-core kernels): grad_input
 * sums the entries of its scatter lists in the order the list build's integer atomics arrived, so it is reproducible
 * to rounding only.  The flag adds one pass that sorts every list into a canonical order before the gather
 * (DESIGN.md section 4.6); the workspace may grow with it (mdconv_workspace_bytes honours the flag).
 * The shape-generic kernels scatter with floating-point atomics and cannot give the guarantee: a backward with the flag
 * that would run on them returns MDCONV_EUNSUPPORTED before anything is launched (the message names the shape rule);
 * mdconv_deterministic_supported() tells beforehand.  The forward is always deterministic and ignores the flag. */
#define MDCONV_FLAG_DETERMINISTIC 1
/* MDCONV_FLAG_NO_GRAD_INPUT, MDCONV_FLAG_NO_GRAD_WEIGHT -- selective backward (what `output_mask` is to
 * aten::convolution_backward).  NO_GRAD_INPUT: grad_input is not wanted.  NO_GRAD_WEIGHT: grad_weight and grad_bias are not
 * wanted.  Both together are valid: only grad_offset (and grad_mask) are computed.
 *  - Pointer rule: the pointers of a skipped gradient (grad_input; grad_weight and grad_bias) may be NULL.  They are never
 *    read or written, NULL or not, in accumulate and in overwrite mode.
 *  - The routing of a flagged call is that of the same call without the flags (kernel family, plan, batch chunks, kernel
 *    per chunk); only the stages that produce the skipped gradients are left out.  On the matrix-core kernels
 *    (mdconv_last_kernels() = MDCONV_KERNELS_F32 / MDCONV_KERNELS_HP) every requested gradient holds exactly what the call
 *    without the flags stores: grad_offset, grad_mask, grad_weight and grad_bias bit for bit, grad_input bit for bit under
 *    MDCONV_FLAG_DETERMINISTIC and to rounding otherwise, as between any two calls.  On the shape-generic kernels
 *    (floating-point atomics) the requested gradients agree to rounding.
 *  - mdconv_workspace_bytes honours the flags and is exact for the flagged call: never larger than without them on the
 *    matrix-core kernels; on the shape-generic kernels NO_GRAD_INPUT adds scratch the fused data kernel scatters into.
 *  - With NO_GRAD_WEIGHT there is nothing to wait for: the weights-ready event is recorded on the caller's stream before
 *    the call's first kernel, so mdconv_stream_wait_weight_ready* after such a call succeeds at once and never refers to
 *    an older backward.
 *  - Forward entry points accept and ignore both flags, so one descriptor serves both directions.
 * (The values skip 2: callers and tests written against earlier releases rely on flags words 2 and 3 being
 * MDCONV_EINVAL, like every other value that was invalid before these flags existed; they still are.) */
#define MDCONV_FLAG_NO_GRAD_INPUT 4
#define MDCONV_FLAG_NO_GRAD_WEIGHT 8
/* MDCONV_FLAG_MATH_BF16 -- fp32 tensors, bf16 matrix math (what torch.set_float32_matmul_precision("medium") is to the
 * reference's addmm_ calls).  A PERMISSION for MDCONV_F32 calls, like allow_tf32: a forward / backward whose bf16 form the
 * native 16-bit kernels take (the forward: and prefer; at least 16 input and 16 output channels) runs on those kernels; any other flagged call runs exactly as
 * without the flag -- same route, same bits, same workspace -- and none is refused over it.  mdconv_math_bf16_used() tells
 * beforehand; the two directions of one layer can differ.  Where the mode is taken:
 *  - input, weight and grad_output are rounded to bf16 (to nearest even) as matrix operands, inside the layout passes;
 *  - offset, mask, grad_offset and grad_mask stay fp32 end to end (as with MDCONV_SAMPLING_F32);
 *  - grad_weight and grad_bias are the unrounded fp32 sums (as with MDCONV_WGRAD_F32); bias is added in fp32;
 *  - output and grad_input are fp32, stored from fp32 accumulators; accumulate mode adds to the caller's buffers in fp32;
 *  - MDCONV_FLAG_DETERMINISTIC, _NO_GRAD_INPUT and _NO_GRAD_WEIGHT act as on a bf16 call;
 *  - mdconv_workspace_bytes, mdconv_deterministic_supported and mdconv_last_kernels() (MDCONV_KERNELS_HP) answer for the
 *    route the flagged call takes.  An fp32 channels-last input stays refused.
 * With MDCONV_F16, MDCONV_BF16 or MDCONV_F64 tensors the flag is MDCONV_EINVAL; v1 descriptors never request it.
 * (The value skips 16, which stays MDCONV_EINVAL like 2 above.) */
#define MDCONV_FLAG_MATH_BF16 32
/* MDCONV_FLAG_OUTPUT_CHANNELS_LAST, MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST -- channels-last results of the native 16-bit
 * kernels, for models that run in torch.channels_last / channels_last_3d.
 *  - OUTPUT_CHANNELS_LAST is the layout of the output-shaped tensor of the call: the forward's `output` is
 *    [B, spatial..., C_out]; the backward's `grad_output` is.  The forward kernels store that layout from their accumulators
 *    (same accumulators, one rounding: the values are those of the unflagged call, permuted); the backward brings each batch
 *    chunk of grad_output into the layout its matrix kernels read with one pass inside the call, and sums grad_bias from that
 *    copy (a call cut into batch chunks: from the caller's tensor, in the same order); grad_bias is bit for bit the
 *    unflagged call's.
 *  - GRAD_INPUT_CHANNELS_LAST: the backward's `grad_input` is [B, spatial..., C_in], in overwrite and in accumulate mode
 *    (accumulate mode reads and adds in that layout).  Forwards accept and ignore the flag; with MDCONV_FLAG_NO_GRAD_INPUT it
 *    is accepted and has nothing to do.
 *  - Every other tensor keeps its layout: offset, mask and their gradients, weight, bias and their gradients, and `input`
 *    (mdconv_desc.input_layout, below).
 *  - MDCONV_F16 / MDCONV_BF16 only; they combine freely with MDCONV_SAMPLING_F32, MDCONV_WGRAD_F32, MDCONV_FLAG_DETERMINISTIC,
 *    _NO_GRAD_INPUT and _NO_GRAD_WEIGHT.  With MDCONV_F32 (MDCONV_FLAG_MATH_BF16 included) or MDCONV_F64 they are
 *    MDCONV_EINVAL; v1 descriptors never request them.
 *  - A flag never changes the route of a call: same kernel family, plan, padded geometry, batch chunks and kernel per chunk
 *    as the unflagged call.  The flags are honoured exactly where the native 16-bit plan takes this direction of the call
 *    (mdconv_last_kernels() = MDCONV_KERNELS_HP) and the channel count of every flagged tensor is a multiple of 8 (16-byte
 *    rows): C_out for the output side, C_in for grad_input.  mdconv_result_layout_supported() tells beforehand; a flagged
 *    call for which it answers 0 returns MDCONV_EUNSUPPORTED before anything is launched.
 *  - mdconv_workspace_bytes honours the flags and is exact: the forward's figure is unchanged; a backward with
 *    OUTPUT_CHANNELS_LAST grows by one batch chunk's grad_output in 16 bits (one workspace slot) and by nothing else;
 *    GRAD_INPUT_CHANNELS_LAST adds nothing. */
#define MDCONV_FLAG_OUTPUT_CHANNELS_LAST 64
#define MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST 128
/* MDCONV_FLAG_SOFTMAX -- a flag of the DCNv4 operator's descriptor (mdconv_dcnv4_desc.flags, below) ALONE: the masks of the
 * packed row are logits and the operator takes their softmax itself.  Every other descriptor -- this one (reserved[4]), DCNv3,
 * multi-scale and packed deformable attention -- refuses the bit as unknown (MDCONV_EINVAL). */
#define MDCONV_FLAG_SOFTMAX 256
#define MDCONV_DESC_FLAGS(d) ((d)->reserved[4])

/* Initialiser of a v2 descriptor: `mdconv_desc d = MDCONV_DESC_INIT(2);` then fill in the shape.
 * (reference semantics by default: accumulate, NCHW input, process-default path) */
#define MDCONV_DESC_INIT(nd) { (nd) | MDCONV_DESC_V2, 0, 0, 0, 0, 0, {0, 0, 1}, {0, 0, 1}, {1, 1, 1}, \
                               {0, 0, 0}, {1, 1, 1}, 1, 1, 64, 0, 1, 0, 0, {0, 0, 0, 0, 0} }

int mdconv_abi_version(void);
const char *mdconv_last_error(void);

/* Output extent on `axis`: (n + 2p - (d(k-1)+1))/s + 1   (mdeformable_conv.cu:150-153). */
int mdconv_out_size(const mdconv_desc *d, int axis);

/* Scratch bytes needed by the forward (backward = 0) or backward (backward = 1) of `d`. */
size_t mdconv_workspace_bytes(const mdconv_desc *d, int backward);

/* Process-wide default kernel path (MDCONV_PATH_*) for descriptors that do not name one; returns the
 * previous value.  The environment variable MDCONV_PATH=auto|direct|mfma|depthwise sets the initial default.
 * Per call: mdconv_desc.path (ABI v2). */
int mdconv_set_path(int path);
/* Path the last forward / backward call of this thread actually ran (MDCONV_PATH_DIRECT/MFMA/DEPTHWISE). */
int mdconv_last_path(void);
/* Kernel family behind it: the shape-generic VALU kernels, the fp32 MFMA kernels (also used for
 * 16-bit tensors through fp32 copies when the native kernels do not cover the shape), the
 * native fp16 / bf16 MFMA kernels, or the depthwise kernels (no matrix instructions, no atomics on results). */
enum { MDCONV_KERNELS_DIRECT = 1, MDCONV_KERNELS_F32 = 2, MDCONV_KERNELS_HP = 3, MDCONV_KERNELS_DEPTHWISE = 4 };
int mdconv_last_kernels(void);
/* Geometry variant of the fp32 MFMA kernels the last call of this thread launched (the forward GEMM of a forward, GEMM-1 of a
 * backward): CANON3X3 = the instances with the geometry of a standard DCNv2 layer compiled in (2-D, 3x3, stride 1, pad 1,
 * dilation 1, one conv group, one deformable group, modulated), RUNTIME = the instances of any shape -- also for every call
 * that ran no fp32 MFMA kernel.  The results of the two are bit-identical; MDCONV_GEOM_FIXED=0 in the environment (read once)
 * keeps every call on RUNTIME. */
enum { MDCONV_GEOMETRY_RUNTIME = 0, MDCONV_GEOMETRY_CANON3X3 = 1 };
int mdconv_last_geometry(void);
/* 1 when the geometry of `d` is the canonical one (the match rule alone, decided without a device: a matching call runs the
 * CANON3X3 instances where it reaches the wide forward tile / the straight-line GEMM-1), else 0 -- also for an invalid `d`. */
int mdconv_geometry_is_canonical(const mdconv_desc *d);
/* The MDCONV_KERNELS_* family the forward (backward = 0) / backward (backward = 1) of `d` would run on -- the routing of the
 * call itself (`path`, `input_layout`, the flags), decided without a device -- or 0 for an invalid descriptor and for a call
 * that would be refused (MDCONV_EUNSUPPORTED).  The two directions of one layer can differ. */
int mdconv_planned_kernels(const mdconv_desc *d, int backward);

/* Per-kernel timing for benchmarks: when enabled, the four dominant kernels are bracketed by HIP
 * events ON THE CALLER'S STREAM.  After a stream/device synchronise, mdconv_profile_read() returns
 * the number of launches of kernel `which` (0 = forward GEMM, 1 = backward data GEMM [the fused
 * backward kernel of the 16-bit path], 2 = backward weight GEMM, 3 = grad_input gather, 4 = coordinate gradients [fp32 split drain]) recorded
 * since the last reset and their total duration in ms; mdconv_profile_name() the name of the kernel
 * variant that ran in that slot last (as rocprofv3 prints it, without template arguments). */
int mdconv_profile_enable(int on);
int mdconv_profile_read(int which, double *total_ms);
const char *mdconv_profile_name(int which);
void mdconv_profile_reset(void);

/* ABI v1 setter, kept for callers built against the v1 header: backward write mode of the calling
 * thread for descriptors WITHOUT MDCONV_DESC_V2 (1 = accumulate, the default; 0 = overwrite).  Returns
 * the previous mode.  v2 descriptors carry `accumulate` themselves and ignore it. */
int mdconv_set_accumulate(int on);

/* Memory format of `input`, mdconv_desc.input_layout:
 * MDCONV_LAYOUT_NCHW (default, the reference's [B, C, spatial...]) or MDCONV_LAYOUT_CHANNELS_LAST
 * ([B, spatial..., C], torch.channels_last / channels_last_3d).  Channels-last input is what the
 * native 16-bit kernels gather from, so it saves their layout pass; it is accepted for fp16 / bf16
 * tensors with C_in a multiple of 32 only (MDCONV_EUNSUPPORTED otherwise).  Every other tensor,
 * grad_input included, keeps the reference layout unless the call asks otherwise (MDCONV_FLAG_OUTPUT_CHANNELS_LAST /
 * MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST above: output / grad_output and grad_input).
 * mdconv_set_input_layout() is the ABI v1 setter (calling thread, descriptors without MDCONV_DESC_V2);
 * it returns the previous setting. */
enum { MDCONV_LAYOUT_NCHW = 0, MDCONV_LAYOUT_CHANNELS_LAST = 1 };
int mdconv_set_input_layout(int layout);
/* 1 if the forward (backward = 0) / backward (backward = 1) of `d` accepts `input` in `layout`,
 * else 0.  The two directions differ (the native 16-bit backward covers fewer shapes than the
 * forward), so a caller that saved a channels-last input for its backward asks here and makes a
 * contiguous copy when the answer is 0 (modulated_deform_conv_amd/MDCONV_CUDA.py does). */
int mdconv_input_layout_supported(const mdconv_desc *d, int layout, int backward);

/* 1 if the forward (backward = 0) / backward (backward = 1) of `d` honours the result-layout flags set in `d`
 * (MDCONV_FLAG_OUTPUT_CHANNELS_LAST / MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST), else 0 with the rule in mdconv_last_error(): the
 * native 16-bit plan takes this direction of the call as it is routed (`path`, `input_layout`, few-tile forwards and
 * shapes that run through fp32 copies included) and C_out (output side) / C_in (grad_input) is a multiple of 8.  The two
 * directions of one layer can differ.  1 for a descriptor without the flags; 0 for an invalid descriptor. */
int mdconv_result_layout_supported(const mdconv_desc *d, int backward);

/* 1 if the forward (backward = 0) / backward (backward = 1) of `d` can run in deterministic mode
 * (MDCONV_FLAG_DETERMINISTIC; the flag itself need not be set in `d`), else 0.  Every forward can.  A backward can
 * exactly when it runs on the fp32 matrix-core kernels or the native 16-bit kernels -- decided by the routing of the
 * call itself (`path`, fp32 sampling, padded / split / chunked plans included); 0 for calls that end on the
 * shape-generic kernels: narrow channel counts, MDCONV_PATH_DIRECT, every fp64 call -- mdconv_last_error() then names
 * the shape rule.  0 for an invalid descriptor. */
int mdconv_deterministic_supported(const mdconv_desc *d, int backward);

/* 1 if the forward (backward = 0) / backward (backward = 1) of `d` -- an MDCONV_F32 descriptor WITH MDCONV_FLAG_MATH_BF16 --
 * would run on the bf16 kernels, else 0: an unflagged or invalid descriptor, MDCONV_PATH_DIRECT, a channels-last input,
 * forwards of a few pixel tiles (which the fp32 kernels run faster), layers of fewer than 16 input or 16 output channels
 * (measured: no gain, profiles/math_bf16.md) and shapes outside the native 16-bit kernels. */
int mdconv_math_bf16_used(const mdconv_desc *d, int backward);

/* Multi-GPU overlap: every backward records an event on its stream as soon
 * as grad_weight and grad_bias are final -- before the grad_input gather is enqueued.
 * mdconv_stream_wait_weight_ready_on() makes `stream` (a hipStream_t, e.g. the communication
 * stream) wait for that point of the LAST backward issued on `producer_stream` of the current
 * device, whichever host thread issued it (PyTorch runs autograd backwards on worker threads), so
 * the all-reduce of grad_weight || grad_bias runs under the rest of the backward.
 * mdconv_stream_wait_weight_ready() is the stream-less form: the most recent backward on the
 * current device (use the keyed form when several streams run backwards concurrently).
 * Both return MDCONV_EINVAL if no such backward has been issued.  The library keeps one event per
 * (device, stream handle) for the most recently used streams (64 per process; older entries are
 * destroyed).  A stream handle the runtime recycles after hipStreamDestroy matches the event of the
 * destroyed stream until the first backward on the new one: wait only for backwards you issued. */
int mdconv_stream_wait_weight_ready(void *stream);
int mdconv_stream_wait_weight_ready_on(void *stream, void *producer_stream);

/* --- replaces deform_conv2d_forward_cuda (deformable_conv.cu:117-123) ---------------------- */
int mdconv_deform_conv2d_forward(const mdconv_desc *d, const void *input, const void *weight,
                                 const void *bias, const void *offset, void *output,
                                 void *workspace, size_t workspace_bytes, void *stream);
/* --- replaces deform_conv2d_backward_cuda (deformable_conv.cu:327-333) --------------------- */
int mdconv_deform_conv2d_backward(const mdconv_desc *d, const void *input, const void *weight,
                                  const void *bias, const void *offset, void *grad_input,
                                  void *grad_weight, void *grad_bias, void *grad_offset,
                                  const void *grad_output, void *workspace,
                                  size_t workspace_bytes, void *stream);
/* --- replaces modulated_deform_conv2d_forward_cuda (mdeformable_conv.cu:120-126) ----------- */
int mdconv_modulated_deform_conv2d_forward(const mdconv_desc *d, const void *input,
                                           const void *weight, const void *bias,
                                           const void *offset, const void *mask, void *output,
                                           void *workspace, size_t workspace_bytes, void *stream);
/* --- replaces modulated_deform_conv2d_backward_cuda (mdeformable_conv.cu:361-366) ---------- */
int mdconv_modulated_deform_conv2d_backward(const mdconv_desc *d, const void *input,
                                            const void *weight, const void *bias,
                                            const void *offset, const void *mask,
                                            const void *grad_output, void *grad_input,
                                            void *grad_offset, void *grad_mask, void *grad_weight,
                                            void *grad_bias, void *workspace,
                                            size_t workspace_bytes, void *stream);
/* --- replaces deform_conv3d_forward_cuda (deformable_conv3d.cu:160-167) -------------------- */
int mdconv_deform_conv3d_forward(const mdconv_desc *d, const void *input, const void *weight,
                                 const void *bias, const void *offset, void *output,
                                 void *workspace, size_t workspace_bytes, void *stream);
/* --- replaces deform_conv3d_backward_cuda (deformable_conv3d.cu:434-442) ------------------- */
int mdconv_deform_conv3d_backward(const mdconv_desc *d, const void *input, const void *weight,
                                  const void *bias, const void *offset, void *grad_input,
                                  void *grad_weight, void *grad_bias, void *grad_offset,
                                  const void *grad_output, void *workspace,
                                  size_t workspace_bytes, void *stream);
/* --- replaces modulated_deform_conv3d_forward_cuda (mdeformable_conv3d.cu:170-177) --------- */
int mdconv_modulated_deform_conv3d_forward(const mdconv_desc *d, const void *input,
                                           const void *weight, const void *bias,
                                           const void *offset, const void *mask, void *output,
                                           void *workspace, size_t workspace_bytes, void *stream);
/* --- replaces modulated_deform_conv3d_backward_cuda (mdeformable_conv3d.cu:443-451) -------- */
int mdconv_modulated_deform_conv3d_backward(const mdconv_desc *d, const void *input,
                                            const void *weight, const void *bias,
                                            const void *offset, const void *mask,
                                            void *grad_input, void *grad_weight, void *grad_bias,
                                            void *grad_offset, void *grad_mask,
                                            const void *grad_output, void *workspace,
                                            size_t workspace_bytes, void *stream);

/* --- DCNv3 core operator: grouped deformable sampling on channels-last tensors -----------------
 * The sampling operator of the InternImage-style "DCNv3" block: no weight, no bias -- the learned weights live in the
 * linear layers around it.  An operator of its own with a descriptor of its own; nothing about the eight entry points
 * above changes.  2-D only.  G groups of D channels, C = G * D, K = kh * kw; every tensor dense and row-major:
 *     input   [B, H,  W,  G*D]          output  [B, Ho, Wo, G*D]
 *     offset  [B, Ho, Wo, G*K*2]        last axis = (group, tap, (x, y))  -- x (width) first
 *     mask    [B, Ho, Wo, G*K]          last axis = (group, tap)
 *     tap = i*kh + j, i in [0, kw) indexes the kernel's WIDTH, j in [0, kh) its height (width-major)
 *     Ho = (H + 2*pad_h - (dil_h*(kh-1)+1)) / stride_h + 1      (Wo alike)
 *     c_w = (dil_w*(kw-1)) >> 1,  c_h = (dil_h*(kh-1)) >> 1
 *     loc_w = wo*stride_w - pad_w + c_w + (i*dil_w - c_w + off_x) * offset_scale
 *     loc_h = ho*stride_h - pad_h + c_h + (j*dil_h - c_h + off_y) * offset_scale
 *     out[b,ho,wo,g,d] = sum_tap mask[b,ho,wo,g,tap] * bilinear(input[b,:,:,g,d], loc_h, loc_w)
 *  - bilinear reads the four neighbours of (loc_h, loc_w); a neighbour outside the image contributes zero and is never
 *    loaded.  A sample contributes iff -1 < loc < size on every axis; a NaN or infinite coordinate (an offset that overflows
 *    once scaled by offset_scale included) therefore contributes nothing, to the output and to every gradient, and has
 *    gradient exactly zero.
 *  - On the lattice (loc_h or loc_w a whole number) the interpolant has a kink and the derivative is a convention: the cell
 *    is floor(loc) and the fractional part loc - floor(loc) = 0 belongs to it, so grad_offset is the RIGHT-SIDED derivative --
 *    along x the difference of the neighbours at x0 + 1 and x0 (a neighbour outside the image counting as zero), weighted
 *    along y -- and grad_input goes to the low neighbours alone.  A gated-out sample has gradient exactly zero in
 *    grad_offset and grad_mask, also at loc == -1 and at loc == size exactly, where a step inwards would read the image.
 *  - The backward returns grad_input, grad_offset (which carries the factor offset_scale) and grad_mask in the layouts of
 *    input, offset and mask; `accumulate` is the write mode of mdconv_desc.accumulate.
 *  - dtype: MDCONV_F32, MDCONV_F16 or MDCONV_BF16, one type for all tensors of a call (no dtype flags); coordinates,
 *    interpolation weights and every sum are fp32.
 *  - Shape rule (else MDCONV_EUNSUPPORTED, with the rule in the error message, before anything is launched): D a multiple
 *    of 4 for fp32 and of 8 for 16-bit tensors (rows of 16 bytes), every tensor below 2^31 bytes, K <= 4096, and for a
 *    backward with grad_input B*G <= 65535.
 *  - flags: MDCONV_FLAG_DETERMINISTIC and MDCONV_FLAG_NO_GRAD_INPUT only; any other bit is MDCONV_EINVAL.  No result is
 *    summed with floating-point atomics: output, grad_offset and grad_mask are bit-identical from call to call, grad_input
 *    is with MDCONV_FLAG_DETERMINISTIC and agrees to rounding otherwise.  With MDCONV_FLAG_NO_GRAD_INPUT grad_input may be
 *    NULL and is never touched; the other gradients are bit for bit those of the full call.  Forwards ignore both flags.
 *  - Pointer alignment ("Pointer alignment" at the top of this header): input, output, grad_output and grad_input are 16-byte aligned; offset, mask and their gradients to their element.
 *  - A call checks in this order: the descriptor (MDCONV_EINVAL), the pointers -- NULL (MDCONV_ENULL), then alignment
 *    (MDCONV_EINVAL, naming the argument) --, the shape rule (MDCONV_EUNSUPPORTED), the workspace (MDCONV_EWORKSPACE: size and
 *    16-byte alignment, as above).
 *  - The workspace figure is exact, 0 for the forward, and honours both flags.  A call is a plain chain of kernels on the
 *    caller's stream: no second stream, no host synchronisation; it captures into a HIP graph. */
typedef struct mdconv_dcnv3_desc {
  int dtype;           /* MDCONV_F32 / MDCONV_F16 / MDCONV_BF16 */
  int batch;           /* B */
  int groups;          /* G */
  int group_channels;  /* D */
  int in_sz[2];        /* H, W */
  int k_sz[2];         /* kh, kw */
  int stride[2];       /* (h, w) */
  int pad[2];
  int dil[2];
  float offset_scale;
  int accumulate;      /* backward write mode: 1 = add to grad_*, 0 = overwrite */
  int flags;           /* MDCONV_FLAG_DETERMINISTIC | MDCONV_FLAG_NO_GRAD_INPUT */
} mdconv_dcnv3_desc;
/* `mdconv_dcnv3_desc d = MDCONV_DCNV3_DESC_INIT;` then fill in the shape (stride 1, no padding, dilation 1, offset_scale 1,
 * accumulate, no flags) */
#define MDCONV_DCNV3_DESC_INIT { 0, 0, 0, 0, {0, 0}, {0, 0}, {1, 1}, {0, 0}, {1, 1}, 1.0f, 1, 0 }

/* Output extent on `axis` (0 = height, 1 = width); -1 for a bad argument. */
int mdconv_dcnv3_out_size(const mdconv_dcnv3_desc *d, int axis);
/* Scratch bytes of the forward (backward = 0: always 0) or the backward (backward = 1) of `d`; 0 for a descriptor that is
 * invalid or outside the shape rule. */
size_t mdconv_dcnv3_workspace_bytes(const mdconv_dcnv3_desc *d, int backward);
int mdconv_dcnv3_forward(const mdconv_dcnv3_desc *d, const void *input, const void *offset, const void *mask,
                         void *output, void *workspace, size_t workspace_bytes, void *stream);
int mdconv_dcnv3_backward(const mdconv_dcnv3_desc *d, const void *input, const void *offset, const void *mask,
                          const void *grad_output, void *grad_input, void *grad_offset, void *grad_mask,
                          void *workspace, size_t workspace_bytes, void *stream);

/* --- Multi-scale deformable attention: the sampling operator of Deformable-DETR-style attention -----
 * ("MSDeformAttn": Deformable-DETR encoders and decoders, Mask2Former's pixel decoder, DINO, RT-DETR.)  The operator the
 * DCNv3 core operator was derived from; an operator of its own with a descriptor of its own, nothing above changes.
 * N images, M heads of D channels, Lq queries, L levels of P points; every tensor dense and row-major:
 *     value               [N, S, M, D]         S = sum_l H_l*W_l: the levels concatenated in order, each row-major (y*W_l + x)
 *     sampling_locations  [N, Lq, M, L, P, 2]  last axis (x, y), normalised: 0..1 spans the level
 *     attention_weights   [N, Lq, M, L, P]
 *     output              [N, Lq, M*D]
 *     x = loc_x * W_l - 0.5,   y = loc_y * H_l - 0.5                    (pixel coordinates in level l)
 *     out[n,q,m,:] = sum_{l,p} attn[n,q,m,l,p] * bilinear(value[n, start_l + ., m, :], y, x)
 *  - start_l is the cumulative sum of the extents before level l: the level starts are not an input.
 *  - bilinear reads the four neighbours of (y, x); a neighbour outside the level contributes zero and is never loaded.  A
 *    sample contributes iff -1 < x < W_l and -1 < y < H_l (the gate of the DCNv3 core operator); a NaN or infinite
 *    coordinate (a location that overflows once scaled by the extent included) therefore contributes nothing, to the output
 *    and to every gradient, and has gradient exactly zero.  For finite coordinates the OUTPUT equals grid_sample with zero padding and align_corners = false everywhere, and
 *    so do the gradients off the lattice and away from the edge of the gate.  On the lattice the derivative is that
 *    operator's convention: the right-sided one of the cell floor(x), floor(y); and a gated-out sample has gradient exactly
 *    zero in grad_sampling_locations and grad_attention_weights, also at x == -1 and x == W_l exactly -- at x == -1
 *    grid_sample returns a non-zero derivative (its interpolant rises into column 0 there), this operator returns zero.
 *  - The backward returns grad_value, grad_sampling_locations (which carries the factors W_l for x and H_l for y) and
 *    grad_attention_weights in the layouts of their forward tensors; `accumulate` is the write mode of mdconv_desc.accumulate.
 *  - dtype (MDCONV_F32, MDCONV_F16 or MDCONV_BF16) is the type of value, output, grad_output and grad_value; coord_dtype is
 *    the type of sampling_locations, attention_weights and their gradients: equal to dtype, or MDCONV_F32 (a bf16
 *    normalised location resolves 0.4 px on a level 100 pixels wide).  All arithmetic is fp32, each result is rounded once.
 *  - Shape rule (else MDCONV_EUNSUPPORTED, with the rule in the error message, before anything is launched): D a multiple
 *    of 4 for fp32 and of 8 for 16-bit values (rows of 16 bytes), every tensor below 2^31 bytes, L*P <= 4096, and for a
 *    backward with grad_value N*M <= 65535 and L*P*Lq*4 below 2^31.
 *  - flags: MDCONV_FLAG_DETERMINISTIC and MDCONV_FLAG_NO_GRAD_INPUT only (the latter: no grad_value); any other bit is
 *    MDCONV_EINVAL.  No result is summed with floating-point atomics: output and the two coordinate gradients are
 *    bit-identical from call to call, grad_value is with MDCONV_FLAG_DETERMINISTIC and agrees to rounding otherwise.  With
 *    MDCONV_FLAG_NO_GRAD_INPUT grad_value may be NULL and is never touched; the other gradients are bit for bit those of the
 *    full call.  Forwards ignore both flags.
 *  - Pointer alignment ("Pointer alignment" at the top of this header): value, output, grad_output and grad_value are 16-byte aligned; sampling_locations, attention_weights and their gradients to
 *    their element (coord_dtype).
 *  - A call checks in this order: the descriptor (MDCONV_EINVAL), the pointers -- NULL (MDCONV_ENULL), then alignment
 *    (MDCONV_EINVAL, naming the argument) --, the shape rule (MDCONV_EUNSUPPORTED), the workspace (MDCONV_EWORKSPACE: size and
 *    16-byte alignment, as above).
 *  - The workspace figure is exact, 0 for the forward, and honours both flags.  A call is a plain chain of kernels on the
 *    caller's stream: no second stream, no host synchronisation; it captures into a HIP graph.
 *  Written from memory of the published operator and UNPINNED against its code. */
#define MDCONV_MSDA_MAX_LEVELS 8
typedef struct mdconv_msda_desc {
  int dtype;           /* value, output, grad_output, grad_value: MDCONV_F32 / MDCONV_F16 / MDCONV_BF16 */
  int coord_dtype;     /* sampling_locations, attention_weights and their gradients: `dtype` or MDCONV_F32 */
  int batch;           /* N */
  int heads;           /* M */
  int head_channels;   /* D */
  int queries;         /* Lq */
  int levels;          /* L, 1..MDCONV_MSDA_MAX_LEVELS */
  int points;          /* P */
  int level_sz[MDCONV_MSDA_MAX_LEVELS][2];  /* (H_l, W_l) of the first `levels` rows; the others are ignored */
  int accumulate;      /* backward write mode: 1 = add to grad_*, 0 = overwrite */
  int flags;           /* MDCONV_FLAG_DETERMINISTIC | MDCONV_FLAG_NO_GRAD_INPUT */
} mdconv_msda_desc;
/* `mdconv_msda_desc d = MDCONV_MSDA_DESC_INIT;` then fill in the shape (fp32, accumulate, no flags) */
#define MDCONV_MSDA_DESC_INIT { 0, 0, 0, 0, 0, 0, 0, 0, {{0, 0}}, 1, 0 }

/* S, the rows of `value` per image: the sum of H_l*W_l over the levels; -1 for a bad descriptor. */
int mdconv_msda_value_len(const mdconv_msda_desc *d);
/* Scratch bytes of the forward (backward = 0: always 0) or the backward (backward = 1) of `d`; 0 for a descriptor that is
 * invalid or outside the shape rule. */
size_t mdconv_msda_workspace_bytes(const mdconv_msda_desc *d, int backward);
int mdconv_msda_forward(const mdconv_msda_desc *d, const void *value, const void *sampling_locations,
                        const void *attention_weights, void *output, void *workspace, size_t workspace_bytes, void *stream);
int mdconv_msda_backward(const mdconv_msda_desc *d, const void *value, const void *sampling_locations,
                         const void *attention_weights, const void *grad_output, void *grad_value,
                         void *grad_sampling_locations, void *grad_attention_weights, void *workspace,
                         size_t workspace_bytes, void *stream);

/* --- 3-D multi-scale deformable attention: the operator above over volumes ------------------------
 * (Deformable transformer stages of volumetric and video models: CoTr-style 3-D deformable encoders for CT / MR volumes,
 * spatio-temporal deformable attention over (T, H, W) feature pyramids.)  An operator of its own with a descriptor of its
 * own and kernels of its own; nothing above changes.  N images, M heads of D channels, Lq queries, L levels
 * (1..MDCONV_MSDA_MAX_LEVELS) of P points; every tensor dense and row-major:
 *     value               [N, S, M, D]         S = sum_l T_l*H_l*W_l: the levels concatenated in order, each row-major
 *                                              ((z*H_l + y)*W_l + x)
 *     sampling_locations  [N, Lq, M, L, P, 3]  last axis (x, y, z), normalised: 0..1 spans the level (grid_sample's order
 *                                              for 5-D inputs)
 *     attention_weights   [N, Lq, M, L, P]
 *     output              [N, Lq, M*D]
 *     x = loc_x * W_l - 0.5,   y = loc_y * H_l - 0.5,   z = loc_z * T_l - 0.5       (voxel coordinates in level l)
 *     out[n,q,m,:] = sum_{l,p} attn[n,q,m,l,p] * trilinear(value[n, start_l + ., m, :], z, y, x)
 *  - start_l is the cumulative sum of the extents before level l: the level starts are not an input.
 *  - trilinear reads the eight neighbours of (z, y, x); a neighbour outside the level contributes zero and is never loaded.
 *    A sample contributes iff -1 < coordinate < size on every one of the three axes (the 2-D operator's gate on three axes); a
 *    NaN or infinite coordinate therefore contributes nothing, to the output and to every gradient, and has gradient exactly
 *    zero.  For finite coordinates the OUTPUT equals grid_sample (mode "bilinear", zero padding,
 *    align_corners = false) on 5-D input everywhere, and so do the gradients off the lattice and away from the edge of the
 *    gate.  On the lattice the derivative is the right-sided one of the cell floor(x), floor(y), floor(z); a gated-out
 *    sample has gradient exactly zero in grad_sampling_locations and grad_attention_weights, -1 and size included.
 *  - The backward returns grad_value, grad_sampling_locations (which carries the factors W_l for x, H_l for y and T_l for z)
 *    and grad_attention_weights in the layouts of their forward tensors; `accumulate` is the write mode of
 *    mdconv_desc.accumulate.
 *  - dtype (MDCONV_F32, MDCONV_F16 or MDCONV_BF16) is the type of value, output, grad_output and grad_value; coord_dtype is
 *    the type of sampling_locations, attention_weights and their gradients: equal to dtype, or MDCONV_F32 -- the five
 *    pairings of the 2-D operator.  All arithmetic is fp32, each result is rounded once.
 *  - Shape rule (else MDCONV_EUNSUPPORTED, with the rule in the error message, before anything is launched): D a multiple
 *    of 4 for fp32 and of 8 for 16-bit values (rows of 16 bytes), T_l*H_l*W_l of every level and every tensor below 2^31
 *    (rows, bytes), L*P <= 4096, and for a backward with grad_value N*M <= 65535 and L*P*Lq*8 below 2^31.
 *  - flags: MDCONV_FLAG_DETERMINISTIC and MDCONV_FLAG_NO_GRAD_INPUT only (the latter: no grad_value); any other bit is
 *    MDCONV_EINVAL.  No result is summed with floating-point atomics: output and the two coordinate gradients are
 *    bit-identical from call to call, grad_value is with MDCONV_FLAG_DETERMINISTIC and agrees to rounding otherwise.  With
 *    MDCONV_FLAG_NO_GRAD_INPUT grad_value may be NULL and is never touched; the other gradients are bit for bit those of the
 *    full call.  Forwards ignore both flags.
 *  - Pointer alignment ("Pointer alignment" at the top of this header): value, output, grad_output and grad_value are 16-byte aligned; sampling_locations, attention_weights and their gradients to
 *    their element (coord_dtype).
 *  - A call checks in this order: the descriptor (MDCONV_EINVAL), the pointers -- NULL (MDCONV_ENULL), then alignment
 *    (MDCONV_EINVAL, naming the argument) --, the shape rule (MDCONV_EUNSUPPORTED), the workspace (MDCONV_EWORKSPACE: size and
 *    16-byte alignment, as above).
 *  - The workspace figure is exact, 0 for the forward, and honours both flags.  A call is a plain chain of kernels on the
 *    caller's stream: no second stream, no host synchronisation; it captures into a HIP graph.
 *  No published operator is the model: the published MSDeformAttn kernel is 2-D only, so fidelity to any published operator
 *  is UNPINNED; the yardstick is the per-level grid_sample composition on 5-D tensors. */
typedef struct mdconv_msda3d_desc {
  int dtype;           /* value, output, grad_output, grad_value: MDCONV_F32 / MDCONV_F16 / MDCONV_BF16 */
  int coord_dtype;     /* sampling_locations, attention_weights and their gradients: `dtype` or MDCONV_F32 */
  int batch;           /* N */
  int heads;           /* M */
  int head_channels;   /* D */
  int queries;         /* Lq */
  int levels;          /* L, 1..MDCONV_MSDA_MAX_LEVELS */
  int points;          /* P */
  int level_sz[MDCONV_MSDA_MAX_LEVELS][3];  /* (T_l, H_l, W_l) of the first `levels` rows; the others are ignored */
  int accumulate;      /* backward write mode: 1 = add to grad_*, 0 = overwrite */
  int flags;           /* MDCONV_FLAG_DETERMINISTIC | MDCONV_FLAG_NO_GRAD_INPUT */
} mdconv_msda3d_desc;
/* `mdconv_msda3d_desc d = MDCONV_MSDA3D_DESC_INIT;` then fill in the shape (fp32, accumulate, no flags) */
#define MDCONV_MSDA3D_DESC_INIT { 0, 0, 0, 0, 0, 0, 0, 0, {{0, 0, 0}}, 1, 0 }

/* S, the rows of `value` per image: the sum of T_l*H_l*W_l over the levels; -1 for a bad descriptor. */
int mdconv_msda3d_value_len(const mdconv_msda3d_desc *d);
/* Scratch bytes of the forward (backward = 0: always 0) or the backward (backward = 1) of `d`; 0 for a descriptor that is
 * invalid or outside the shape rule. */
size_t mdconv_msda3d_workspace_bytes(const mdconv_msda3d_desc *d, int backward);
int mdconv_msda3d_forward(const mdconv_msda3d_desc *d, const void *value, const void *sampling_locations,
                          const void *attention_weights, void *output, void *workspace, size_t workspace_bytes, void *stream);
int mdconv_msda3d_backward(const mdconv_msda3d_desc *d, const void *value, const void *sampling_locations,
                           const void *attention_weights, const void *grad_output, void *grad_value,
                           void *grad_sampling_locations, void *grad_attention_weights, void *workspace,
                           size_t workspace_bytes, void *stream);

/* --- DCNv4 operator: the DCNv3 core operator's sampling with one packed coordinate tensor ----------
 * The sampling operator of the "DCNv4" block, the successor of DCNv3: no weight, no bias, no softmax over the taps -- the
 * masks are whatever the linear layer before it produced, of any sign and size -- unless MDCONV_FLAG_SOFTMAX asks for one.  An operator of its own with a descriptor of
 * its own; nothing above changes.  2-D only.  G groups of D channels; every tensor dense and row-major:
 *     input        [B, H,  W,  G*D]          output  [B, Ho, Wo, G*D]
 *     offset_mask  [B, Ho, Wo, OM]           OM = ceil(G*K*3 / 8) * 8        (mdconv_dcnv4_offset_mask_len)
 *        row = for g in 0..G-1: { (x, y) of tap 0, ..., (x, y) of tap K-1, mask of tap 0, ..., mask of tap K-1 },
 *              then OM - G*K*3 padding columns
 *        element of (g, tap): x at g*3K + 2*tap, y at g*3K + 2*tap + 1, mask at g*3K + 2K + tap
 *     K = kh*kw - (remove_center ? 1 : 0)
 *     kernel-grid tap u = i*kh + j, i in [0, kw) the kernel's WIDTH index, j in [0, kh) its height index (as in DCNv3)
 *     with remove_center the grid tap (kh*kw - 1)/2 is skipped: tensor tap t maps to u = t + (t >= (kh*kw - 1)/2)
 *     Ho, Wo, c_h, c_w, loc_h, loc_w, the gate (a sample contributes iff -1 < loc < size on every axis; a NaN or infinite
 *     coordinate therefore contributes nothing and has gradient exactly zero), the corner rule and the derivative on the
 *     lattice (the right-sided one of the cell floor(loc); exactly zero for a gated-out sample, loc == -1 and loc == size
 *     included):
 *     exactly those of the DCNv3 core operator above, with (i, j) taken from u
 *     out[b,ho,wo,g,:] = sum_t mask[t] * bilinear(input[b,:,:,g,:], loc_h(t), loc_w(t))
 *  - The padding columns of offset_mask are never read into any result (they may hold NaN).  The backward returns grad_input
 *    and grad_offset_mask in the layouts of input and offset_mask (the offset gradients carry the factor offset_scale);
 *    `accumulate` is the write mode of mdconv_desc.accumulate: in overwrite mode the padding columns of grad_offset_mask
 *    come back as exact zeros, in accumulate mode they are not touched.
 *  - dtype (MDCONV_F32, MDCONV_F16 or MDCONV_BF16) is the type of input, output, grad_output and grad_input; coord_dtype is
 *    the type of offset_mask and its gradient: equal to dtype, or MDCONV_F32 (a bf16 offset of a few pixels resolves no
 *    better than 1/32 px).  All arithmetic is fp32, each result is rounded once.
 *  - Descriptor rules beyond DCNv3's (MDCONV_EINVAL): remove_center is 0 or 1, and 1 only with odd kh and kw that are not
 *    both 1 (K = 0); coord_dtype is dtype or MDCONV_F32.
 *  - Shape rule (else MDCONV_EUNSUPPORTED, with the rule in the error message, before anything is launched): D a multiple
 *    of 4 for fp32 and of 8 for 16-bit values (rows of 16 bytes), every tensor -- offset_mask included -- below 2^31 bytes,
 *    K <= 4096, and for a backward with grad_input B*G <= 65535 and K*Ho*Wo*4 below 2^31.
 *  - flags: MDCONV_FLAG_DETERMINISTIC, MDCONV_FLAG_NO_GRAD_INPUT and MDCONV_FLAG_SOFTMAX (next item) only; any other bit is
 *    MDCONV_EINVAL.  No result is
 *    summed with floating-point atomics: output and grad_offset_mask are bit-identical from call to call, grad_input is with
 *    MDCONV_FLAG_DETERMINISTIC and agrees to rounding otherwise.  With MDCONV_FLAG_NO_GRAD_INPUT grad_input may be NULL and
 *    is never touched; grad_offset_mask is bit for bit that of the full call.  Forwards ignore both flags.
 *  - MDCONV_FLAG_SOFTMAX (256; this descriptor only): the K mask elements of a group are LOGITS, and the weight of tap t is
 *        a[t] = exp(logit[t] - max) / sum_s exp(logit[s] - max)         (fp32, the maximum subtracted: any finite logits)
 *    in the place of mask[t] above -- DCNv3's softmax over the masks of a group, inside the operator; nothing of the size of
 *    the masks is materialised.  The softmax runs over ALL K tensor taps of the (output pixel, group) -- K = kh*kw - 1 with
 *    remove_center.  Taps the gate drops are included: they count in the normaliser and add nothing to the output, which is
 *    what a framework softmax in front of the operator does.  The padding columns stay unread.  Gradients: with g[t] the
 *    gradient the mask of tap t has without the flag and S = sum_s a[s] g[s], the logit's gradient is a[t] * (g[t] - S);
 *    a gated-out tap therefore has the logit gradient -a[t] * S, not zero, and offset gradients of exactly zero; when every
 *    tap of a pair is gated out all its gradients are exactly zero; with K = 1 the weight is exactly 1 and the logit
 *    gradient exactly 0.  S is taken from fp32 sums of the call, never from a stored output.  The forward honours this flag
 *    (and ignores the other two, as before).  Everything else -- shape rule, order of checks, write modes, the padding of
 *    grad_offset_mask, no floating-point atomics, determinism, one stream, HIP graphs -- is as without the flag.  Workspace:
 *    a backward with grad_input has the figure without the flag plus 8 * B*Ho*Wo*G bytes rounded up to a 256-byte slot (the
 *    pairs' softmax statistics, behind the lists); with MDCONV_FLAG_NO_GRAD_INPUT it is 0 and nothing is stored; the
 *    forward's is 0.  The compile-time `softmax` switch of the published kernels is what this flag is modelled on, from
 *    memory and UNPINNED like the rest.
 *  - Pointer alignment ("Pointer alignment" at the top of this header): input, output, grad_output and grad_input are 16-byte aligned; offset_mask and its gradient to their element (coord_dtype).
 *  - A call checks in this order: the descriptor (MDCONV_EINVAL), the pointers -- NULL (MDCONV_ENULL), then alignment
 *    (MDCONV_EINVAL, naming the argument) --, the shape rule (MDCONV_EUNSUPPORTED), the workspace (MDCONV_EWORKSPACE: size and
 *    16-byte alignment, as above).
 *  - The workspace figure is exact, 0 for the forward, honours the flags and does not depend on coord_dtype.  A call is a
 *    plain chain of kernels on the caller's stream: no second stream, no host synchronisation; it captures into a HIP graph.
 *  Written from memory of the published operator and UNPINNED against its code. */
typedef struct mdconv_dcnv4_desc {
  int dtype;           /* input, output, grad_output, grad_input: MDCONV_F32 / MDCONV_F16 / MDCONV_BF16 */
  int coord_dtype;     /* offset_mask and its gradient: `dtype` or MDCONV_F32 */
  int batch;           /* B */
  int groups;          /* G */
  int group_channels;  /* D */
  int in_sz[2];        /* H, W */
  int k_sz[2];         /* kh, kw */
  int stride[2];       /* (h, w) */
  int pad[2];
  int dil[2];
  float offset_scale;
  int remove_center;   /* 1 = the centre tap of the (odd) kernel is left out: K = kh*kw - 1 */
  int accumulate;      /* backward write mode: 1 = add to grad_*, 0 = overwrite */
  int flags;           /* MDCONV_FLAG_DETERMINISTIC | MDCONV_FLAG_NO_GRAD_INPUT | MDCONV_FLAG_SOFTMAX */
} mdconv_dcnv4_desc;
/* `mdconv_dcnv4_desc d = MDCONV_DCNV4_DESC_INIT;` then fill in the shape (fp32, stride 1, no padding, dilation 1,
 * offset_scale 1, the full kernel, accumulate, no flags) */
#define MDCONV_DCNV4_DESC_INIT { 0, 0, 0, 0, 0, {0, 0}, {0, 0}, {1, 1}, {0, 0}, {1, 1}, 1.0f, 0, 1, 0 }

/* Output extent on `axis` (0 = height, 1 = width); -1 for a bad argument. */
int mdconv_dcnv4_out_size(const mdconv_dcnv4_desc *d, int axis);
/* OM, the elements per row of offset_mask; -1 for a bad descriptor. */
int mdconv_dcnv4_offset_mask_len(const mdconv_dcnv4_desc *d);
/* Scratch bytes of the forward (backward = 0: always 0) or the backward (backward = 1) of `d`; 0 for a descriptor that is
 * invalid or outside the shape rule. */
size_t mdconv_dcnv4_workspace_bytes(const mdconv_dcnv4_desc *d, int backward);
int mdconv_dcnv4_forward(const mdconv_dcnv4_desc *d, const void *input, const void *offset_mask, void *output,
                         void *workspace, size_t workspace_bytes, void *stream);
int mdconv_dcnv4_backward(const mdconv_dcnv4_desc *d, const void *input, const void *offset_mask, const void *grad_output,
                          void *grad_input, void *grad_offset_mask, void *workspace, size_t workspace_bytes, void *stream);

/* --- Packed deformable attention: multi-scale deformable attention with one packed tensor and its softmax inside ----
 * The second operator of the "DCNv4" package ("FlashDeformAttn"), which bears the relation to multi-scale deformable
 * attention above that the DCNv4 operator bears to DCNv3: the locations and the attention LOGITS arrive in one tensor, as the
 * linear layers produced them, and the softmax over the K = L*P taps of a (query, head) runs inside the operator.  An
 * operator of its own with a descriptor of its own; nothing above changes.  N, M, D, Lq, L, P, S and `value` as for
 * multi-scale deformable attention; every tensor dense and row-major:
 *     value              [N, S, M, D]
 *     sampling_loc_attn  [N, Lq, M, 3K]        (mdconv_fda_loc_attn_len; no padding columns)
 *        row of a (query, head) = { (x, y) of tap 0, ..., (x, y) of tap K-1, logit of tap 0, ..., logit of tap K-1 }
 *        tap = l*P + p;  x at 2*tap, y at 2*tap + 1 (normalised, as above), logit at 2K + tap
 *     output             [N, Lq, M*D]
 *     a[t] = exp(logit[t] - max_s logit[s]) / sum_s exp(logit[s] - max_s logit[s])        (fp32)
 *     out[n,q,m,:] = sum_t a[t] * bilinear(value[n, start_l + ., m, :], y_t, x_t)
 *     pixel coordinates, level starts, the gate (a tap contributes iff -1 < loc < size on every axis; a NaN or infinite
 *     coordinate therefore contributes nothing and has gradient exactly zero), the corner rule and the derivative on the
 *     lattice (the right-sided one of the cell floor(loc); a gated-out tap has location gradients of exactly zero, loc == -1 and
 *     loc == size included, and g[t] = 0 in the logit gradient below): exactly those of multi-scale deformable attention above
 *  - The logits must be finite.  They may be large: the maximum is subtracted before the exponential.
 *  - The backward returns grad_value and grad_sampling_loc_attn in the layouts of value and sampling_loc_attn: the location
 *    gradients are those of multi-scale deformable attention with a[t] as the weight, the logit gradient is
 *    a[t] * (g[t] - sum_s a[s] g[s]) with g[t] the gradient that operator returns for the weight of tap t.  It takes no
 *    `output`: the sum is taken from fp32 sums inside the call.  `accumulate` is the write mode of mdconv_desc.accumulate.
 *  - dtype (MDCONV_F32, MDCONV_F16 or MDCONV_BF16) is the type of value, output, grad_output and grad_value; coord_dtype is
 *    the type of sampling_loc_attn and its gradient: equal to dtype, or MDCONV_F32.  All arithmetic is fp32, the softmax
 *    included, each result is rounded once.
 *  - Shape rule (else MDCONV_EUNSUPPORTED, with the rule in the error message, before anything is launched): that of
 *    multi-scale deformable attention -- D a multiple of 4 for fp32 and of 8 for 16-bit values, every tensor below 2^31
 *    bytes, L*P <= 4096, and for a backward with grad_value N*M <= 65535 and L*P*Lq*4 below 2^31 -- with sampling_loc_attn,
 *    N*Lq*M*3K elements, among the tensors.
 *  - flags: MDCONV_FLAG_DETERMINISTIC and MDCONV_FLAG_NO_GRAD_INPUT only (the latter: no grad_value); any other bit is
 *    MDCONV_EINVAL.  No result is summed with floating-point atomics: output and grad_sampling_loc_attn are bit-identical
 *    from call to call, grad_value is with MDCONV_FLAG_DETERMINISTIC and agrees to rounding otherwise.  With
 *    MDCONV_FLAG_NO_GRAD_INPUT grad_value may be NULL and is never touched; grad_sampling_loc_attn is bit for bit that of the
 *    full call.  Forwards ignore both flags.
 *  - Pointer alignment ("Pointer alignment" at the top of this header): value, output, grad_output and grad_value are 16-byte aligned; sampling_loc_attn and its gradient to their element
 *    (coord_dtype).
 *  - A call checks in this order: the descriptor (MDCONV_EINVAL), the pointers -- NULL (MDCONV_ENULL), then alignment
 *    (MDCONV_EINVAL, naming the argument) --, the shape rule (MDCONV_EUNSUPPORTED), the workspace (MDCONV_EWORKSPACE: size and
 *    16-byte alignment, as above).
 *  - The workspace figure is exact, 0 for the forward, and honours both flags: a backward with grad_value takes the scatter
 *    lists of multi-scale deformable attention for the same shape plus 8 bytes per (query, head).  A call is a plain chain of
 *    kernels on the caller's stream: no second stream, no host synchronisation; it captures into a HIP graph.
 *  Written from memory of the published operator and UNPINNED against its code. */
typedef struct mdconv_fda_desc {
  int dtype;           /* value, output, grad_output, grad_value: MDCONV_F32 / MDCONV_F16 / MDCONV_BF16 */
  int coord_dtype;     /* sampling_loc_attn and its gradient: `dtype` or MDCONV_F32 */
  int batch;           /* N */
  int heads;           /* M */
  int head_channels;   /* D */
  int queries;         /* Lq */
  int levels;          /* L, 1..MDCONV_MSDA_MAX_LEVELS */
  int points;          /* P */
  int level_sz[MDCONV_MSDA_MAX_LEVELS][2];  /* (H_l, W_l) of the first `levels` rows; the others are ignored */
  int accumulate;      /* backward write mode: 1 = add to grad_*, 0 = overwrite */
  int flags;           /* MDCONV_FLAG_DETERMINISTIC | MDCONV_FLAG_NO_GRAD_INPUT */
} mdconv_fda_desc;
/* `mdconv_fda_desc d = MDCONV_FDA_DESC_INIT;` then fill in the shape (fp32, accumulate, no flags) */
#define MDCONV_FDA_DESC_INIT { 0, 0, 0, 0, 0, 0, 0, 0, {{0, 0}}, 1, 0 }

/* S, the rows of `value` per image: the sum of H_l*W_l over the levels; -1 for a bad descriptor. */
int mdconv_fda_value_len(const mdconv_fda_desc *d);
/* 3K = 3*L*P, the elements of sampling_loc_attn per (query, head); -1 for a bad descriptor. */
int mdconv_fda_loc_attn_len(const mdconv_fda_desc *d);
/* Scratch bytes of the forward (backward = 0: always 0) or the backward (backward = 1) of `d`; 0 for a descriptor that is
 * invalid or outside the shape rule. */
size_t mdconv_fda_workspace_bytes(const mdconv_fda_desc *d, int backward);
int mdconv_fda_forward(const mdconv_fda_desc *d, const void *value, const void *sampling_loc_attn, void *output,
                       void *workspace, size_t workspace_bytes, void *stream);
int mdconv_fda_backward(const mdconv_fda_desc *d, const void *value, const void *sampling_loc_attn, const void *grad_output,
                        void *grad_value, void *grad_sampling_loc_attn, void *workspace, size_t workspace_bytes, void *stream);

/* --- Deformable RoI pooling: RoIAlign whose bins are shifted by a learnt offset, channels-last -------
 * ("deform_roi_pool": the dpool / mdpool heads of Deformable ConvNets v1 / v2 detectors.)  An operator of its own with a
 * descriptor of its own; nothing above changes.  B images of H x W pixels and C channels, R regions pooled into PH x PW bins;
 * every tensor dense and row-major:
 *     input    [B, H, W, C]         dtype
 *     rois     [R, 5]               fp32 always: (batch index, x1, y1, x2, y2) in image coordinates
 *     offset   [R, 2, PH, PW]       coord_dtype; plane 0 = x (width), plane 1 = y; absent with with_offset == 0 (pointer ignored)
 *     output   [R, PH, PW, C]       dtype
 *     b   = (int) rois[r,0]
 *     x1s = x1*spatial_scale - 0.5  (y1s, x2s, y2s alike: no rounding, no minimum size)
 *     rw  = x2s - x1s,  rh = y2s - y1s,  bw = rw / PW,  bh = rh / PH
 *     gh  = sampling_ratio > 0 ? sampling_ratio : min(max(ceil(rh / PH), 0), max_grid)        (gw from rw / PW alike)
 *     cnt = max(gh*gw, 1)
 *     dx  = gamma * rw * offset[r,0,ph,pw],  dy = gamma * rh * offset[r,1,ph,pw]               (0 without offset)
 *     y(iy) = y1s + dy + ph*bh + (iy + 0.5) * bh / gh,   x(ix) = x1s + dx + pw*bw + (ix + 0.5) * bw / gw
 *     output[r,ph,pw,c] = (1/cnt) * sum_{iy<gh, ix<gw} bil(input[b,:,:,c], y(iy), x(ix))
 *  - bil(y, x) is RoIAlign's sample: it contributes iff -1 <= y <= H and -1 <= x <= W (RoIAlign's gate is closed); a NaN or
 *    infinite coordinate -- a NaN or infinite offset, or one that overflows once scaled by gamma * rw -- therefore contributes
 *    nothing, to the output and to every gradient, and the grad_offset of its bin is exactly zero.  Otherwise y = max(y, 0), y_lo = floor(y); if y_lo >= H-1 then y_lo = y_hi = H-1 and y = H-1, else
 *    y_hi = y_lo + 1; the same for x; the value is the bilinear mix of the four (possibly coinciding) neighbours.  No element
 *    outside the image is ever loaded.  All arithmetic is fp32, each result is rounded once.
 *  - A RoI contributes NOTHING when its batch index is not an integer in [0, B) or any of its five numbers is not finite: its
 *    output rows are zero, its grad_offset rows are exact zeros (overwrite) or untouched (accumulate), it adds nothing to
 *    grad_input, and nothing is read through it.  A RoI with rh <= 0 or rw <= 0 under the adaptive rule (sampling_ratio == 0)
 *    has no samples and gives zeros the same way.
 *  - max_grid (1..16) is read only with sampling_ratio == 0: it bounds the workspace without reading `rois` on the host.
 *    When no RoI of a call exceeds it the result is the published adaptive rule.
 *  - The backward returns grad_input [B,H,W,C] (the four interpolation weights / cnt; coinciding corners add) and
 *    grad_offset [R,2,PH,PW] = gamma*rw/cnt * sum_c grad_output[r,ph,pw,c] * sum_samples d bil/dx (rh and d/dy for plane 1);
 *    rois get no gradient.  grad_offset is the derivative of the function the forward computes, in the lattice convention of
 *    the operators above: the right-sided derivative of the cell floor(loc), exactly zero along an axis where the coordinate
 *    is clamped (loc < 0 or loc >= size-1), exactly zero outside the gate.  `accumulate` is the backward's write mode
 *    (mdconv_desc.accumulate); the forward writes every output row.
 *  - dtype (MDCONV_F32, MDCONV_F16 or MDCONV_BF16) is the type of input, output, grad_output and grad_input; coord_dtype is
 *    the type of offset and grad_offset: equal to dtype, or MDCONV_F32.
 *  - Shape rule (else MDCONV_EUNSUPPORTED, with the rule in the error message, before anything is launched): C * element size
 *    a multiple of 16, every tensor below 2^31 bytes, and R*PH*PW*Gcap*Gcap*4 below 2^31 with Gcap = sampling_ratio, or
 *    max_grid when that is 0.
 *  - flags: MDCONV_FLAG_DETERMINISTIC and MDCONV_FLAG_NO_GRAD_INPUT only; any other bit is MDCONV_EINVAL, and so is a
 *    backward that has neither grad_offset (with_offset == 0) nor grad_input (MDCONV_FLAG_NO_GRAD_INPUT) to compute.  No
 *    result is summed with floating-point atomics: output and grad_offset are bit-identical from call to call, grad_input is
 *    with MDCONV_FLAG_DETERMINISTIC and agrees to rounding otherwise.  With MDCONV_FLAG_NO_GRAD_INPUT grad_input may be NULL
 *    and is never touched, the workspace is 0, and grad_offset is bit for bit the full call's.  Forwards ignore both flags.
 *  - Pointer alignment ("Pointer alignment" at the top of this header): input, output, grad_output and grad_input are 16-byte aligned; rois to 4 bytes, offset and grad_offset to their element
 *    (coord_dtype).
 *  - A call checks in this order: the descriptor (MDCONV_EINVAL), the pointers -- NULL (MDCONV_ENULL), then alignment
 *    (MDCONV_EINVAL, naming the argument) --, the shape rule (MDCONV_EUNSUPPORTED), the workspace (MDCONV_EWORKSPACE: size and
 *    16-byte alignment, as above).
 *  - The workspace figure is exact, 0 for the forward, independent of coord_dtype, and honours both flags.  A call is a plain
 *    chain of kernels on the caller's stream: no second stream, no host synchronisation; it captures into a HIP graph.
 *  Written from memory of the published operator and UNPINNED against its code; where the published kernels
 *  are remembered to differ (the offset gradient in the clamped zones) this text is the specification. */
typedef struct mdconv_droi_desc {
  int dtype;           /* input, output, grad_output, grad_input: MDCONV_F32 / MDCONV_F16 / MDCONV_BF16 */
  int coord_dtype;     /* offset and grad_offset: `dtype` or MDCONV_F32 */
  int batch;           /* B */
  int channels;        /* C */
  int height, width;   /* H, W */
  int rois;            /* R */
  int pooled_h, pooled_w;   /* PH, PW */
  int sampling_ratio;  /* 0 = adaptive (bounded by max_grid), else 1..16 samples per bin and axis */
  int max_grid;        /* 1..16; read only with sampling_ratio == 0 */
  float spatial_scale;
  float gamma;
  int with_offset;     /* 0 = plain RoIAlign sampling: offset and grad_offset are ignored */
  int accumulate;      /* backward write mode: 1 = add to grad_*, 0 = overwrite */
  int flags;           /* MDCONV_FLAG_DETERMINISTIC | MDCONV_FLAG_NO_GRAD_INPUT */
} mdconv_droi_desc;
/* `mdconv_droi_desc d = MDCONV_DROI_DESC_INIT;` then fill in the shape (fp32, adaptive grid up to 8, scale 1, gamma 0.1,
 * with offset, accumulate, no flags) */
#define MDCONV_DROI_DESC_INIT { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 8, 1.0f, 0.1f, 1, 1, 0 }

/* Scratch bytes of the forward (backward = 0: always 0) or the backward (backward = 1) of `d`; 0 for a descriptor that is
 * invalid or outside the shape rule. */
size_t mdconv_droi_workspace_bytes(const mdconv_droi_desc *d, int backward);
int mdconv_droi_forward(const mdconv_droi_desc *d, const void *input, const void *rois, const void *offset, void *output,
                        void *workspace, size_t workspace_bytes, void *stream);
int mdconv_droi_backward(const mdconv_droi_desc *d, const void *input, const void *rois, const void *offset,
                         const void *grad_output, void *grad_input, void *grad_offset, void *workspace,
                         size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MDCONV_H_ */
