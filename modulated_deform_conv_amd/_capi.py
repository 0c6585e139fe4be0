"""ctypes loader for libmdconv_hip.so -- the C ABI declared in include/mdconv.h.

There is no CPU fallback: if the HIP library is missing or fails to load, importing the product
raises, loudly.
"""
import ctypes
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MDCONV_LIB") or os.path.join(HERE, "libmdconv_hip.so")

F32, F16, F64, BF16 = 0, 1, 2, 3
SAMPLING_F32 = 0x10   # MDCONV_SAMPLING_F32: ORed into F16 / BF16, offset / mask and their gradients are fp32
WGRAD_F32 = 0x40      # MDCONV_WGRAD_F32: ORed into F16 / BF16, the backward's grad_weight / grad_bias are fp32
PATH_AUTO, PATH_DIRECT, PATH_MFMA, PATH_DEPTHWISE = 0, 1, 2, 3
ABI_VERSION = 2
DESC_V2 = 0x100   # MDCONV_DESC_V2: the descriptor carries accumulate / input_layout / path
FLAG_DETERMINISTIC = 1   # MDCONV_FLAG_DETERMINISTIC, in the flags word (MdconvDesc.flags = reserved[4])
FLAG_NO_GRAD_INPUT = 4   # MDCONV_FLAG_NO_GRAD_INPUT: the backward leaves grad_input out (value 2 stays invalid)
FLAG_NO_GRAD_WEIGHT = 8  # MDCONV_FLAG_NO_GRAD_WEIGHT: the backward leaves grad_weight and grad_bias out
FLAG_MATH_BF16 = 32      # MDCONV_FLAG_MATH_BF16: fp32 tensors may run on the bf16 matrix kernels (value 16 stays invalid)
FLAG_OUTPUT_CHANNELS_LAST = 64        # MDCONV_FLAG_OUTPUT_CHANNELS_LAST: output (forward) / grad_output (backward) is channels-last
FLAG_GRAD_INPUT_CHANNELS_LAST = 128   # MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST: the backward's grad_input is channels-last
FLAG_SOFTMAX = 256       # MDCONV_FLAG_SOFTMAX: MdconvDcnv4Desc.flags alone -- the masks are logits, softmax over the taps in-kernel

EXPORTS = (
    "mdconv_abi_version", "mdconv_last_error", "mdconv_out_size", "mdconv_workspace_bytes",
    "mdconv_set_path", "mdconv_last_path", "mdconv_last_kernels",
    "mdconv_profile_enable", "mdconv_profile_read", "mdconv_profile_reset", "mdconv_profile_name",
    "mdconv_stream_wait_weight_ready", "mdconv_stream_wait_weight_ready_on", "mdconv_set_accumulate", "mdconv_set_input_layout",
    "mdconv_input_layout_supported", "mdconv_deterministic_supported", "mdconv_math_bf16_used",
    "mdconv_result_layout_supported", "mdconv_planned_kernels",
    "mdconv_deform_conv2d_forward", "mdconv_deform_conv2d_backward",
    "mdconv_modulated_deform_conv2d_forward", "mdconv_modulated_deform_conv2d_backward",
    "mdconv_deform_conv3d_forward", "mdconv_deform_conv3d_backward",
    "mdconv_modulated_deform_conv3d_forward", "mdconv_modulated_deform_conv3d_backward",
    "mdconv_dcnv3_out_size", "mdconv_dcnv3_workspace_bytes", "mdconv_dcnv3_forward", "mdconv_dcnv3_backward",
    "mdconv_msda_value_len", "mdconv_msda_workspace_bytes", "mdconv_msda_forward", "mdconv_msda_backward",
    "mdconv_dcnv4_out_size", "mdconv_dcnv4_offset_mask_len", "mdconv_dcnv4_workspace_bytes", "mdconv_dcnv4_forward",
    "mdconv_dcnv4_backward",
    "mdconv_fda_value_len", "mdconv_fda_loc_attn_len", "mdconv_fda_workspace_bytes", "mdconv_fda_forward", "mdconv_fda_backward",
    "mdconv_droi_workspace_bytes", "mdconv_droi_forward", "mdconv_droi_backward",
    "mdconv_msda3d_value_len", "mdconv_msda3d_workspace_bytes", "mdconv_msda3d_forward", "mdconv_msda3d_backward",
    "mdconv_last_geometry", "mdconv_geometry_is_canonical",
)

# include/mdconv_dagg.h (deformable aggregation): a header of its own, so a tuple of its own -- EXPORTS is mdconv.h's
EXPORTS_DAGG = ("mdconv_dagg_feature_len", "mdconv_dagg_workspace_bytes", "mdconv_dagg_forward", "mdconv_dagg_backward")
# include/mdconv_msdap.h (deformable attention with a point count per level): likewise
EXPORTS_MSDAP = ("mdconv_msdap_value_len", "mdconv_msdap_points_len", "mdconv_msdap_workspace_bytes", "mdconv_msdap_forward",
                 "mdconv_msdap_backward")
# include/mdconv_fdap.h (packed deformable attention with a point count per level): likewise
EXPORTS_FDAP = ("mdconv_fdap_value_len", "mdconv_fdap_loc_attn_len", "mdconv_fdap_workspace_bytes", "mdconv_fdap_forward",
                "mdconv_fdap_backward")
# include/mdconv_afda.h (anchored packed deformable attention: reference points and raw offsets): likewise
EXPORTS_AFDA = ("mdconv_afda_value_len", "mdconv_afda_offs_attn_len", "mdconv_afda_workspace_bytes", "mdconv_afda_forward",
                "mdconv_afda_backward")

# The descriptor-only queries of the sampling operators, operator -> names: every operator has
# mdconv_<op>_workspace_bytes(desc, backward) -> size_t besides; out_size takes (desc, axis), a *_len (desc); all return int.
SAMP_QUERIES = {"dcnv3": ("out_size",), "msda": ("value_len",), "dcnv4": ("out_size", "offset_mask_len"),
                "fda": ("value_len", "loc_attn_len"), "droi": (), "msda3d": ("value_len",), "dagg": ("feature_len",),
                "msdap": ("value_len", "points_len"), "fdap": ("value_len", "loc_attn_len"),
                "afda": ("value_len", "offs_attn_len")}


class MdconvDesc(ctypes.Structure):
    """Mirror of ``struct mdconv_desc`` (include/mdconv.h, ABI v2: the call modes travel in the descriptor)."""
    _fields_ = [("ndim", ctypes.c_int), ("modulated", ctypes.c_int), ("dtype", ctypes.c_int),
                ("batch", ctypes.c_int), ("c_in", ctypes.c_int), ("c_out", ctypes.c_int),
                ("in_sz", ctypes.c_int * 3), ("k_sz", ctypes.c_int * 3),
                ("stride", ctypes.c_int * 3), ("pad", ctypes.c_int * 3), ("dil", ctypes.c_int * 3),
                ("groups", ctypes.c_int), ("dgroups", ctypes.c_int), ("in_step", ctypes.c_int),
                ("with_bias", ctypes.c_int),
                ("accumulate", ctypes.c_int), ("input_layout", ctypes.c_int), ("path", ctypes.c_int),
                ("reserved", ctypes.c_int * 5)]

    @property
    def flags(self):
        """The per-call flags word (MDCONV_FLAG_*): the last slot of the v2 tail, ``reserved[4]``."""
        return self.reserved[4]

    @flags.setter
    def flags(self, value):
        self.reserved[4] = int(value)


class MdconvDcnv3Desc(ctypes.Structure):
    """Mirror of ``struct mdconv_dcnv3_desc`` (include/mdconv.h, "DCNv3 core operator"); axis order (h, w)."""
    _fields_ = [("dtype", ctypes.c_int), ("batch", ctypes.c_int), ("groups", ctypes.c_int),
                ("group_channels", ctypes.c_int), ("in_sz", ctypes.c_int * 2), ("k_sz", ctypes.c_int * 2),
                ("stride", ctypes.c_int * 2), ("pad", ctypes.c_int * 2), ("dil", ctypes.c_int * 2),
                ("offset_scale", ctypes.c_float), ("accumulate", ctypes.c_int), ("flags", ctypes.c_int)]


class MdconvDcnv4Desc(ctypes.Structure):
    """Mirror of ``struct mdconv_dcnv4_desc`` (include/mdconv.h, "DCNv4 operator"); axis order (h, w)."""
    _fields_ = [("dtype", ctypes.c_int), ("coord_dtype", ctypes.c_int), ("batch", ctypes.c_int), ("groups", ctypes.c_int),
                ("group_channels", ctypes.c_int), ("in_sz", ctypes.c_int * 2), ("k_sz", ctypes.c_int * 2),
                ("stride", ctypes.c_int * 2), ("pad", ctypes.c_int * 2), ("dil", ctypes.c_int * 2),
                ("offset_scale", ctypes.c_float), ("remove_center", ctypes.c_int), ("accumulate", ctypes.c_int),
                ("flags", ctypes.c_int)]


MSDA_MAX_LEVELS = 8   # MDCONV_MSDA_MAX_LEVELS


class MdconvMsdaDesc(ctypes.Structure):
    """Mirror of ``struct mdconv_msda_desc`` (include/mdconv.h, "Multi-scale deformable attention"); ``level_sz`` rows
    are (H, W)."""
    _fields_ = [("dtype", ctypes.c_int), ("coord_dtype", ctypes.c_int), ("batch", ctypes.c_int), ("heads", ctypes.c_int),
                ("head_channels", ctypes.c_int), ("queries", ctypes.c_int), ("levels", ctypes.c_int),
                ("points", ctypes.c_int), ("level_sz", (ctypes.c_int * 2) * MSDA_MAX_LEVELS),
                ("accumulate", ctypes.c_int), ("flags", ctypes.c_int)]


class MdconvFdaDesc(ctypes.Structure):
    """Mirror of ``struct mdconv_fda_desc`` (include/mdconv.h, "Packed deformable attention"): the fields of
    ``MdconvMsdaDesc``; ``level_sz`` rows are (H, W)."""
    _fields_ = list(MdconvMsdaDesc._fields_)


class MdconvMsda3dDesc(ctypes.Structure):
    """Mirror of ``struct mdconv_msda3d_desc`` (include/mdconv.h, "3-D multi-scale deformable attention"): the fields of
    ``MdconvMsdaDesc`` with ``level_sz`` rows of (T, H, W)."""
    _fields_ = [(n, (ctypes.c_int * 3) * MSDA_MAX_LEVELS) if n == "level_sz" else (n, t) for n, t in MdconvMsdaDesc._fields_]


class MdconvDroiDesc(ctypes.Structure):
    """Mirror of ``struct mdconv_droi_desc`` (include/mdconv.h, "Deformable RoI pooling")."""
    _fields_ = [("dtype", ctypes.c_int), ("coord_dtype", ctypes.c_int), ("batch", ctypes.c_int), ("channels", ctypes.c_int),
                ("height", ctypes.c_int), ("width", ctypes.c_int), ("rois", ctypes.c_int), ("pooled_h", ctypes.c_int),
                ("pooled_w", ctypes.c_int), ("sampling_ratio", ctypes.c_int), ("max_grid", ctypes.c_int),
                ("spatial_scale", ctypes.c_float), ("gamma", ctypes.c_float), ("with_offset", ctypes.c_int),
                ("accumulate", ctypes.c_int), ("flags", ctypes.c_int)]


class MdconvDaggDesc(ctypes.Structure):
    """Mirror of ``struct mdconv_dagg_desc`` (include/mdconv_dagg.h); ``level_sz`` rows are (H, W), of every camera."""
    _fields_ = [("dtype", ctypes.c_int), ("coord_dtype", ctypes.c_int), ("batch", ctypes.c_int), ("cams", ctypes.c_int),
                ("levels", ctypes.c_int), ("level_sz", (ctypes.c_int * 2) * MSDA_MAX_LEVELS), ("channels", ctypes.c_int),
                ("groups", ctypes.c_int), ("anchors", ctypes.c_int), ("points", ctypes.c_int),
                ("accumulate", ctypes.c_int), ("flags", ctypes.c_int)]


class MdconvMsdapDesc(ctypes.Structure):
    """Mirror of ``struct mdconv_msdap_desc`` (include/mdconv_msdap.h): ``MdconvMsdaDesc`` with a count per level in
    ``points``; ``level_sz`` rows are (H, W)."""
    _fields_ = [(n, ctypes.c_int * MSDA_MAX_LEVELS) if n == "points" else (n, t) for n, t in MdconvMsdaDesc._fields_]


class MdconvFdapDesc(ctypes.Structure):
    """Mirror of ``struct mdconv_fdap_desc`` (include/mdconv_fdap.h): the fields of ``MdconvMsdapDesc``."""
    _fields_ = list(MdconvMsdapDesc._fields_)


class MdconvAfdaDesc(ctypes.Structure):
    """Mirror of ``struct mdconv_afda_desc`` (include/mdconv_afda.h): the fields of ``MdconvFdapDesc`` and the four of the
    reference tensor."""
    _fields_ = list(MdconvFdapDesc._fields_) + [("ref_levels", ctypes.c_int), ("ref_comps", ctypes.c_int),
                                                ("offset_scale", ctypes.c_float), ("grad_reference", ctypes.c_int)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libmdconv_hip.so is not built (%s). Run `python -m modulated_deform_conv_amd._build` "
                "(needs hipcc); there is no CPU fallback." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.mdconv_abi_version.restype = ctypes.c_int
        L.mdconv_last_error.restype = ctypes.c_char_p
        L.mdconv_out_size.restype = ctypes.c_int
        L.mdconv_workspace_bytes.restype = ctypes.c_size_t
        L.mdconv_workspace_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.mdconv_set_path.restype = ctypes.c_int
        L.mdconv_set_path.argtypes = [ctypes.c_int]
        L.mdconv_last_path.restype = ctypes.c_int
        L.mdconv_profile_enable.restype = ctypes.c_int
        L.mdconv_profile_read.restype = ctypes.c_int
        L.mdconv_profile_reset.restype = None
        L.mdconv_profile_name.restype = ctypes.c_char_p
        L.mdconv_profile_name.argtypes = [ctypes.c_int]
        L.mdconv_set_accumulate.restype = ctypes.c_int
        L.mdconv_set_accumulate.argtypes = [ctypes.c_int]
        L.mdconv_set_input_layout.restype = ctypes.c_int
        L.mdconv_set_input_layout.argtypes = [ctypes.c_int]
        L.mdconv_stream_wait_weight_ready.restype = ctypes.c_int
        L.mdconv_stream_wait_weight_ready.argtypes = [ctypes.c_void_p]
        L.mdconv_stream_wait_weight_ready_on.restype = ctypes.c_int
        L.mdconv_stream_wait_weight_ready_on.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.mdconv_last_kernels.restype = ctypes.c_int
        L.mdconv_input_layout_supported.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.mdconv_deterministic_supported.restype = ctypes.c_int
        L.mdconv_deterministic_supported.argtypes = [ctypes.c_void_p, ctypes.c_int]
        # (MDCONV_LIB may name a build from before the query existed -- the A/B tools measure such builds' exact calls)
        has_math_query = hasattr(L, "mdconv_math_bf16_used")
        if has_math_query:
            L.mdconv_math_bf16_used.argtypes = [ctypes.c_void_p, ctypes.c_int]
        # (likewise a build from before the result-layout query: it honours no result layout)
        has_layout_query = hasattr(L, "mdconv_result_layout_supported")
        if has_layout_query:
            L.mdconv_result_layout_supported.argtypes = [ctypes.c_void_p, ctypes.c_int]
        # (likewise a build from before the depthwise family: planned_kernels() raises there)
        has_plan_query = hasattr(L, "mdconv_planned_kernels")
        if has_plan_query:
            L.mdconv_planned_kernels.argtypes = [ctypes.c_void_p, ctypes.c_int]
        missing = (() if has_math_query else ("mdconv_math_bf16_used",)) + (() if has_layout_query else ("mdconv_result_layout_supported",))
        missing += () if has_plan_query else ("mdconv_planned_kernels",)
        # (likewise a build from before the canonical-geometry instances: last_geometry() says 'runtime' there)
        missing += tuple(n for n in ("mdconv_last_geometry", "mdconv_geometry_is_canonical") if not hasattr(L, n))
        # (likewise a build from before one of the sampling operators: that operator's wrapper raises there)
        missing += tuple(n for n in EXPORTS + EXPORTS_DAGG + EXPORTS_MSDAP + EXPORTS_FDAP + EXPORTS_AFDA
                         if n.startswith(tuple("mdconv_%s_" % op for op in SAMP_QUERIES)) and not hasattr(L, n))
        for name in EXPORTS[11:] + EXPORTS_DAGG + EXPORTS_MSDAP + EXPORTS_FDAP + EXPORTS_AFDA:
            if name not in missing:
                getattr(L, name).restype = ctypes.c_int
        for op, queries in SAMP_QUERIES.items():
            if not hasattr(L, "mdconv_%s_workspace_bytes" % op):
                continue
            ws = getattr(L, "mdconv_%s_workspace_bytes" % op)
            ws.restype, ws.argtypes = ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int]
            for q in queries:
                getattr(L, "mdconv_%s_%s" % (op, q)).argtypes = [ctypes.c_void_p] + ([ctypes.c_int] if q == "out_size" else [])
        if L.mdconv_abi_version() != ABI_VERSION:
            raise ImportError("libmdconv_hip.so ABI version mismatch")
        _lib = L
    return _lib


def last_error():
    return lib().mdconv_last_error().decode("utf-8", "replace")


VECTOR_ALIGN = 16   # bytes: the "16-byte" pointer class of include/mdconv.h ("Pointer alignment")


def aligned_input(t):
    """A read-only tensor of the "16-byte" pointer class as the library takes it: `t` itself when its address is a multiple
    of 16, else a fresh copy (the allocator's alignment) -- a dense view at an odd storage offset (a slice of a flat
    parameter buffer, a piece of torch.split) is aligned to its element only.  "element"-class tensors need nothing: a
    tensor's address is always a multiple of its element size."""
    if t is None or t.numel() == 0 or t.data_ptr() % VECTOR_ALIGN == 0:
        return t
    import torch
    return t.clone(memory_format=torch.preserve_format)


def require_aligned_result(op, name, t):
    """A caller-supplied result buffer of the "16-byte" pointer class must be 16-byte aligned: the library writes into the
    caller's tensor, never into a silent temporary."""
    if t is not None and t.numel() > 0 and t.data_ptr() % VECTOR_ALIGN:
        raise ValueError("%s: %s must be %d-byte aligned (its address is %d mod %d: a view at a storage offset?); pass an "
                         "aligned buffer and copy" % (op, name, VECTOR_ALIGN, t.data_ptr() % VECTOR_ALIGN, VECTOR_ALIGN))


def set_path(path):
    """Force the kernel path: 'auto' | 'direct' | 'mfma' | 'depthwise'.  Returns the previous setting."""
    names = {"auto": PATH_AUTO, "direct": PATH_DIRECT, "mfma": PATH_MFMA, "depthwise": PATH_DEPTHWISE}
    prev = lib().mdconv_set_path(names[path] if isinstance(path, str) else int(path))
    return {v: k for k, v in names.items()}[prev]


def last_path():
    return {0: "none", PATH_DIRECT: "direct", PATH_MFMA: "mfma", PATH_DEPTHWISE: "depthwise"}[lib().mdconv_last_path()]


def last_kernels():
    """Kernel family of the last call: 'direct' | 'f32' (fp32 MFMA kernels) | 'hp' (native 16-bit) | 'depthwise'."""
    return KERNELS[lib().mdconv_last_kernels()]


KERNELS = {0: "none", 1: "direct", 2: "f32", 3: "hp", 4: "depthwise"}   # MDCONV_KERNELS_*


def last_geometry():
    """Geometry variant of the fp32 MFMA kernels the last call launched (its forward GEMM / GEMM-1): 'canon3x3' (the
    instances with a standard 3x3 DCNv2 layer's geometry compiled in) | 'runtime' (any shape; also when the call ran no
    fp32 MFMA kernel).  ``MDCONV_GEOM_FIXED=0`` in the environment keeps every call on 'runtime'."""
    L = lib()
    return "canon3x3" if hasattr(L, "mdconv_last_geometry") and L.mdconv_last_geometry() == 1 else "runtime"


def planned_kernels(desc, backward):
    """Kernel family the forward (``backward`` false) / backward of ``desc`` (an ``MdconvDesc``) would run on, by the
    names of ``last_kernels()``; 'none' for an invalid descriptor or a call that would be refused (``last_error()`` then
    has the rule).  Host-side planning only: no device is needed."""
    return KERNELS[lib().mdconv_planned_kernels(ctypes.byref(desc), int(bool(backward)))]


PROFILE_SLOTS = 5   # forward GEMM, backward data GEMM, backward weight GEMM, grad_input gather


_modes = threading.local()   # Python-side default of mdconv_desc.accumulate for descriptors built in this thread


def accumulate_mode():
    """Value for ``mdconv_desc.accumulate`` of a descriptor built now (1 unless inside ``overwrite_grads``)."""
    return getattr(_modes, "accumulate", 1)


class overwrite_grads:
    """Context manager: backward entry points of MDCONV_CUDA called inside WRITE their gradients instead of
    adding to them (``mdconv_desc.accumulate = 0``, include/mdconv.h), so the buffers may be torch.empty.
    The mode travels in each call's descriptor; no library state is touched."""

    def __enter__(self):
        self._prev = accumulate_mode()
        _modes.accumulate = 0

    def __exit__(self, *exc):
        _modes.accumulate = self._prev
        return False


def deterministic_override():
    """True / False inside a ``deterministic`` context manager of this thread, None outside."""
    return getattr(_modes, "deterministic", None)


def deterministic_mode():
    """Whether a descriptor built now asks for deterministic mode (``MDCONV_FLAG_DETERMINISTIC``, include/mdconv.h):
    the innermost ``deterministic`` context manager of this thread when one is active, otherwise
    ``torch.are_deterministic_algorithms_enabled()`` -- read at the call, so a backward issued from an autograd worker
    thread follows the process-wide torch setting."""
    over = deterministic_override()
    if over is not None:
        return bool(over)
    import torch
    return bool(torch.are_deterministic_algorithms_enabled())


class deterministic:
    """Context manager: calls of MDCONV_CUDA issued inside by this thread run in deterministic mode (``on=True``: every
    gradient bit-identical from call to call; a backward that would run on the shape-generic kernels raises) or out
    of it (``on=False``), whatever ``torch.use_deterministic_algorithms`` says.  Thread-local, nests, and travels in
    each call's descriptor like ``overwrite_grads``.  (A backward that autograd runs on a worker thread is outside the
    ``with`` block of the thread that called ``.backward()``: use the torch setting there.)"""

    def __init__(self, on=True):
        self._on = bool(on)

    def __enter__(self):
        self._prev = deterministic_override()
        _modes.deterministic = self._on
        return self

    def __exit__(self, *exc):
        _modes.deterministic = self._prev
        return False


def weight_grads_f32_mode():
    """True inside a ``weight_grads_f32`` context manager of this thread (innermost one: its ``on``), else False."""
    return bool(getattr(_modes, "weight_grads_f32", False))


class weight_grads_f32:
    """Context manager: fp16 / bf16 backwards issued inside by this thread hand back fp32 weight and bias gradients
    (``MDCONV_WGRAD_F32``, include/mdconv.h) wherever this package allocates them: the fp32 sums every 16-bit backward
    holds, without the final rounding to 16 bits.  ``MDCONV_CUDA.modulated_deform_conv2d_backward_cuda`` returns fp32
    ``grad_weight`` / ``grad_bias``; the autograd Functions called inside with 16-bit data and fp32 ``weight`` (AMP with
    fp32 master weights) cast the parameters themselves and return the unrounded gradients.  The caller-allocated entry
    points need no context: they take the mode from the dtype of the ``grad_weight`` they are handed.  ``on=False``
    switches the mode off inside an outer block.  Thread-local, nests, and travels in each call's descriptor like
    ``overwrite_grads``."""

    def __init__(self, on=True):
        self._on = bool(on)

    def __enter__(self):
        self._prev = weight_grads_f32_mode()
        _modes.weight_grads_f32 = self._on
        return self

    def __exit__(self, *exc):
        _modes.weight_grads_f32 = self._prev
        return False


def fp32_math_override():
    """``"bf16"`` / ``"fp32"`` inside an ``fp32_math`` context manager of this thread, None outside."""
    return getattr(_modes, "fp32_math", None)


def fp32_math_mode():
    """The matrix arithmetic of an fp32 call issued now: ``"bf16"`` (its descriptor carries ``MDCONV_FLAG_MATH_BF16``,
    include/mdconv.h) or ``"fp32"``.  The innermost ``fp32_math`` context manager of this thread when one is active, otherwise
    ``"bf16"`` exactly when ``torch.get_float32_matmul_precision() == "medium"`` ("bfloat16 for internal computations, if a
    fast algorithm is available") -- read at the call.  "high" and "highest" stay exact: there is no TF32-class kernel."""
    over = fp32_math_override()
    if over is not None:
        return over
    import torch
    return "bf16" if torch.get_float32_matmul_precision() == "medium" else "fp32"


class fp32_math:
    """Context manager: fp32 calls of MDCONV_CUDA issued inside by this thread may run their matrix products in bf16
    (``"bf16"``: ``MDCONV_FLAG_MATH_BF16`` -- fp32 tensors in and out, bf16 operands, fp32 sampling, accumulation and weight
    gradients, wherever the native 16-bit kernels take the shape; other shapes run exactly as without it) or run exact
    (``"fp32"``), whatever ``torch.set_float32_matmul_precision`` says.  No effect on fp16 / bf16 / fp64 tensors.
    Thread-local, nests, and travels in each call's descriptor like ``overwrite_grads``; the autograd Functions record the
    mode in forward and enter it in backward themselves."""

    def __init__(self, mode="bf16"):
        if mode not in ("bf16", "fp32"):
            raise ValueError('fp32_math mode must be "bf16" or "fp32", got %r' % (mode,))
        self._mode = mode

    def __enter__(self):
        self._prev = fp32_math_override()
        _modes.fp32_math = self._mode
        return self

    def __exit__(self, *exc):
        _modes.fp32_math = self._prev
        return False


def channels_last_results_mode():
    """True inside a ``channels_last_results`` context manager of this thread (innermost one: its ``on``), else False."""
    return bool(getattr(_modes, "channels_last_results", False))


class channels_last_results:
    """Context manager: fp16 / bf16 calls of MDCONV_CUDA issued inside by this thread accept dense channels-last
    (``torch.channels_last`` / ``channels_last_3d``) ``output``, ``grad_output`` and ``grad_input`` tensors
    (``MDCONV_FLAG_OUTPUT_CHANNELS_LAST`` / ``MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST``, include/mdconv.h): where the native
    16-bit kernels take the call they store / read that layout themselves, elsewhere the binding goes through a contiguous
    temporary like any PyTorch operator, so no call raises over the mode.  The entry points that allocate their results
    (the modulated 2-D pair, the autograd Functions) allocate ``output`` and ``grad_input`` channels-last when the
    ``input`` they are given is.  Outside the mode nothing changes: such tensors have to be contiguous.  ``on=False``
    switches the mode off inside an outer block.  Thread-local, nests, and travels in each call's descriptor like
    ``overwrite_grads``; the autograd Functions record the mode in forward and enter it in backward themselves."""

    def __init__(self, on=True):
        self._on = bool(on)

    def __enter__(self):
        self._prev = channels_last_results_mode()
        _modes.channels_last_results = self._on
        return self

    def __exit__(self, *exc):
        _modes.channels_last_results = self._prev
        return False


def skipped_grads():
    """``(input, weight)``: the gradients a backward issued now by this thread leaves out -- the innermost ``skip_grads``
    context manager, ``(False, False)`` outside one."""
    return getattr(_modes, "skip_grads", (False, False))


def skip_flags():
    """``skipped_grads()`` as bits of the descriptor's flags word."""
    skip_input, skip_weight = skipped_grads()
    return (FLAG_NO_GRAD_INPUT if skip_input else 0) | (FLAG_NO_GRAD_WEIGHT if skip_weight else 0)


class skip_grads:
    """Context manager: backward entry points of MDCONV_CUDA called inside by this thread leave out ``grad_input``
    (``input=True``) and / or ``grad_weight`` and ``grad_bias`` (``weight=True``): ``MDCONV_FLAG_NO_GRAD_INPUT`` /
    ``MDCONV_FLAG_NO_GRAD_WEIGHT`` (include/mdconv.h).  The stages that produce them are not run; the other gradients are
    what the full call stores.  The caller-allocated entry points accept ``None`` (or any tensor, which stays untouched) for
    a skipped gradient; ``modulated_deform_conv2d_backward_cuda`` returns ``None`` there.  The autograd Functions enter it
    by themselves from ``ctx.needs_input_grad``.  Thread-local, nests (the innermost block decides both switches), and
    travels in each call's descriptor like ``overwrite_grads``."""

    def __init__(self, input=False, weight=False):
        self._skip = (bool(input), bool(weight))

    def __enter__(self):
        self._prev = skipped_grads()
        _modes.skip_grads = self._skip
        return self

    def __exit__(self, *exc):
        _modes.skip_grads = self._prev
        return False


def stream_wait_weight_ready(stream, producer=None):
    """Make `stream` (a torch.cuda.Stream) wait until grad_weight / grad_bias of the last backward
    issued on `producer` (a torch.cuda.Stream; default: the most recent backward on the current
    device) are final -- the grad_input gather may still be running.  Works whichever host thread
    issued that backward (autograd worker threads included)."""
    if producer is None:
        rc = lib().mdconv_stream_wait_weight_ready(ctypes.c_void_p(stream.cuda_stream))
    else:
        rc = lib().mdconv_stream_wait_weight_ready_on(ctypes.c_void_p(stream.cuda_stream),
                                                      ctypes.c_void_p(producer.cuda_stream))
    if rc != 0:
        raise RuntimeError(last_error())


def profile_enable(on=True):
    return bool(lib().mdconv_profile_enable(int(on)))


def profile_reset():
    lib().mdconv_profile_reset()


def profile_read():
    """{kernel name: (launches, average ms)} -- call after torch.cuda.synchronize()."""
    out = {}
    for which in range(PROFILE_SLOTS):
        tot = ctypes.c_double(0)
        n = lib().mdconv_profile_read(which, ctypes.byref(tot))
        name = lib().mdconv_profile_name(which).decode()
        if n and name:
            out[name] = (n, tot.value / n)
    return out
