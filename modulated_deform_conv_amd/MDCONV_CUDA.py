"""``MDCONV_CUDA`` -- the reference's extension-module surface on top of libmdconv_hip.so.

The reference builds a pybind11 module of this name (setup.py:37) and its Python wrapper calls
eight functions of it positionally (modulated_deform_conv.py:28, 57, 112, 142, 194, 225, 281,
313; only two are actually registered in the reference snapshot, mdeformable_conv.cu:460-465 --
SURVEY.md R2).  This module exports all eight with the same positional signatures, argument
meaning, return values and error behaviour (RuntimeError for non-contiguous tensors and for
kernel/channel mismatches, mdeformable_conv.cu:127-148), and forwards to the C ABI
(include/mdconv.h) through ctypes.  Torch is plumbing here: device memory, the current stream,
the caching allocator for the scratch workspace.

Put this directory on ``sys.path`` (or ``import modulated_deform_conv_amd.MDCONV_CUDA as
MDCONV_CUDA``) and the reference's own ``modulated_deform_conv.py`` runs unchanged.
"""
import ctypes
import warnings

import torch

from . import _capi
from .distributed import fused_grad_buffers

_DTYPES = {torch.float32: _capi.F32, torch.float16: _capi.F16, torch.float64: _capi.F64,
           torch.bfloat16: _capi.BF16}


def _is_channels_last(t):
    """`t` is a dense channels-last tensor the native 16-bit kernels can gather from directly
    (torch.channels_last / channels_last_3d, fp16 / bf16, C a multiple of 32)."""
    if t.dim() not in (4, 5) or t.dtype not in (torch.float16, torch.bfloat16) or t.shape[1] % 32:
        return False
    fmt = torch.channels_last if t.dim() == 4 else torch.channels_last_3d
    return t.is_contiguous(memory_format=fmt)


def _cl_result(t):
    """`t` is a dense channels-last (torch.channels_last / channels_last_3d) fp16 / bf16 tensor that is not contiguous as
    well: the layout the result-layout flags name (include/mdconv.h: MDCONV_FLAG_OUTPUT_CHANNELS_LAST /
    MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST)."""
    if t is None or t.dim() not in (4, 5) or t.dtype not in (torch.float16, torch.bfloat16) or t.is_contiguous():
        return False
    return t.is_contiguous(memory_format=torch.channels_last if t.dim() == 4 else torch.channels_last_3d)


_CL_RESULTS = ("output", "grad_output", "grad_input")


def _check_contig(**tensors):
    cl_results = _capi.channels_last_results_mode()
    for name, t in tensors.items():
        if t is None:   # a gradient the call leaves out (_capi.skip_grads)
            continue
        # extension of the reference's check (mdeformable_conv.cu:127-131): a channels-last `input`
        # is accepted where the kernels consume that layout anyway -- and, inside
        # _capi.channels_last_results, a channels-last 16-bit output / grad_output / grad_input
        if not t.is_contiguous() and not (name == "input" and _is_channels_last(t)) \
                and not (cl_results and name in _CL_RESULTS and _cl_result(t)):
            raise RuntimeError("%s tensor has to be contiguous" % name)


def _result_flags(d, input, backward, out_like, grad_input=None):
    """Inside _capi.channels_last_results: sets the result-layout flags of `d` from the layouts of the output-shaped tensor
    (`output` / `grad_output`) and of `grad_input`, as far as this direction honours them (include/mdconv.h:
    mdconv_result_layout_supported -- both, else the output side alone, else grad_input alone), and returns the flags it
    set.  `d` is complete but for them (dtype flags, input layout of the `input` that is handed over)."""
    want = (_capi.FLAG_OUTPUT_CHANNELS_LAST if _cl_result(out_like) else 0) | \
        (_capi.FLAG_GRAD_INPUT_CHANNELS_LAST if backward and _cl_result(grad_input) else 0)
    if not want or not _capi.channels_last_results_mode():
        return 0
    query = getattr(_capi.lib(), "mdconv_result_layout_supported", None)
    d.input_layout = int(not input.is_contiguous() and _is_channels_last(input))
    tried = []
    for flags in (want, want & _capi.FLAG_OUTPUT_CHANNELS_LAST, want & _capi.FLAG_GRAD_INPUT_CHANNELS_LAST):
        if flags and flags not in tried and query is not None:
            tried.append(flags)
            d.flags |= flags
            if query(ctypes.byref(d), int(backward)):
                return flags
            d.flags &= ~flags
    return 0


def _backward_layouts(d, input, grad_output, grad_input):
    """Inside _capi.channels_last_results: a channels-last `grad_output` / `grad_input` goes to the library as it is where
    the backward honours the layout (`_result_flags`); otherwise the call runs on contiguous temporaries, like any other
    PyTorch operator would.  Returns (grad_output, grad_input, final): the tensors to hand over and, when `grad_input` is
    such a temporary, the caller's tensor it is copied into after the call."""
    if not _capi.channels_last_results_mode():
        return grad_output, grad_input, None
    got = _result_flags(d, input, True, grad_output, grad_input)
    final = None
    if _cl_result(grad_output) and not got & _capi.FLAG_OUTPUT_CHANNELS_LAST:
        grad_output = grad_output.contiguous()
    if _cl_result(grad_input) and not got & _capi.FLAG_GRAD_INPUT_CHANNELS_LAST:
        final = grad_input
        grad_input = grad_input.contiguous() if d.accumulate else torch.empty_like(grad_input, memory_format=torch.contiguous_format)
    if got & _capi.FLAG_GRAD_INPUT_CHANNELS_LAST:
        _capi.require_aligned_result("MDCONV_CUDA", "grad_input", grad_input)   # stored as vectors: pointer class "16-byte"
    return grad_output, grad_input, final


def channels_last_results_supported(nd, modulated, input, weight, ksz, stride, pad, dil, group, deformable_group, in_step,
                                    with_bias, backward):
    """Whether, inside _capi.channels_last_results, the forward stores a channels-last `output` (backward = False) / the
    backward a channels-last `grad_input` (True) for this call by itself: what an entry point that allocates its results
    asks before it picks their memory format (a channels-last `input` is what makes it ask)."""
    if not _capi.channels_last_results_mode() or not (_is_channels_last(input) and not input.is_contiguous()):
        return False
    query = getattr(_capi.lib(), "mdconv_result_layout_supported", None)
    if query is None:
        return False
    d = _desc(nd, modulated, input, weight, ksz, stride, pad, dil, group, deformable_group, in_step, with_bias)
    d.input_layout = int(bool(_capi.lib().mdconv_input_layout_supported(ctypes.byref(d), 1, int(backward))))
    d.flags |= _capi.FLAG_GRAD_INPUT_CHANNELS_LAST if backward else _capi.FLAG_OUTPUT_CHANNELS_LAST
    return bool(query(ctypes.byref(d), int(backward)))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() > 0 else 0)


def _skipped(grad_input, grad_weight, grad_bias):
    """The gradients of a caller-allocated backward with the ones `_capi.skip_grads` leaves out replaced by None: whatever
    the caller passed there (None, or any tensor) is neither checked nor handed to the library."""
    skip_input, skip_weight = _capi.skipped_grads()
    return (None if skip_input else grad_input,) + ((None, None) if skip_weight else (grad_weight, grad_bias))


def _desc(nd, modulated, input, weight, ksz, stride, pad, dil, group, deformable_group, in_step,
          with_bias):
    if input.dim() != nd + 2 or weight.dim() != nd + 2:
        raise RuntimeError("expected %d-D input and weight, got %d-D and %d-D"
                           % (nd + 2, input.dim(), weight.dim()))
    if not input.is_cuda:
        raise NotImplementedError  # reference: modulated_deform_conv.py:22-23
    if input.dtype not in _DTYPES:
        raise RuntimeError('"deform_conv" not implemented for %s' % input.dtype)
    if tuple(weight.shape[2:]) != tuple(ksz):
        raise RuntimeError("Input shape and kernel shape wont match: (%s vs %s)."
                           % ("x".join(map(str, ksz)), "x".join(map(str, weight.shape[2:]))))
    if input.shape[1] != weight.shape[1] * group:
        raise RuntimeError("Input shape and kernel channels wont match: (%d vs %d)."
                           % (input.shape[1], weight.shape[1] * group))
    d = _capi.MdconvDesc()
    d.ndim, d.modulated, d.dtype = nd | _capi.DESC_V2, int(modulated), _DTYPES[input.dtype]
    d.accumulate, d.input_layout, d.path = _capi.accumulate_mode(), 0, _capi.PATH_AUTO
    # deterministic mode (include/mdconv.h: MDCONV_FLAG_DETERMINISTIC): the one place the flag enters a descriptor, so
    # workspace sizing and every entry point see it
    d.flags = _capi.FLAG_DETERMINISTIC if _capi.deterministic_mode() else 0
    # selective backward (_capi.skip_grads; include/mdconv.h: MDCONV_FLAG_NO_GRAD_INPUT / _WEIGHT; forwards ignore the flags)
    d.flags |= _capi.skip_flags()
    # fp32 tensors, bf16 matrix math (_capi.fp32_math / torch.set_float32_matmul_precision("medium"); include/mdconv.h:
    # MDCONV_FLAG_MATH_BF16): a permission for fp32 calls only -- the library refuses the flag on any other dtype
    if input.dtype == torch.float32 and _capi.fp32_math_mode() == "bf16":
        d.flags |= _capi.FLAG_MATH_BF16
    d.batch, d.c_in, d.c_out = input.shape[0], input.shape[1], weight.shape[0]
    fill = lambda v, f: tuple(int(x) for x in v) + (f,) * (3 - nd)
    d.in_sz = (ctypes.c_int * 3)(*fill(input.shape[2:], 1))
    d.k_sz = (ctypes.c_int * 3)(*fill(ksz, 1))
    d.stride = (ctypes.c_int * 3)(*fill(stride, 1))
    d.pad = (ctypes.c_int * 3)(*fill(pad, 0))
    d.dil = (ctypes.c_int * 3)(*fill(dil, 1))
    d.groups, d.dgroups, d.in_step, d.with_bias = int(group), int(deformable_group), int(in_step), int(bool(with_bias))
    return d


def _layout(d, input, backward):
    """A channels-last `input` stays as it is where the kernels of this direction gather from that
    layout (include/mdconv.h: mdconv_input_layout_supported -- the native 16-bit backward covers
    fewer shapes than the forward, and MDCONV_PATH / MDCONV_HP can switch those kernels off);
    otherwise the call runs on a contiguous copy, like any other PyTorch operator would."""
    if input.is_contiguous():
        return input   # (pointer class "element", include/mdconv.h: a view at any storage offset goes as it is)
    if _capi.lib().mdconv_input_layout_supported(ctypes.byref(d), 1, int(backward)):
        return _capi.aligned_input(input)   # the kernels gather 16-byte vectors from it: pointer class "16-byte", copied if below
    return input.contiguous()


def _out_shape(d, nd):
    L = _capi.lib()
    return tuple(L.mdconv_out_size(ctypes.byref(d), a) for a in range(nd))


def _check_side(d, nd, K, offset, mask, other, other_name, osz):
    """Shape/dtype/device checks the reference omits (a wrong shape would read out of bounds)."""
    exp_off = (d.batch, d.dgroups * nd * K) + osz
    if tuple(offset.shape) != exp_off:
        raise RuntimeError("offset shape %s, expected %s" % (tuple(offset.shape), exp_off))
    if mask is not None:
        exp_m = (d.batch, d.dgroups * K) + osz
        if tuple(mask.shape) != exp_m:
            raise RuntimeError("mask shape %s, expected %s" % (tuple(mask.shape), exp_m))
    n_out = d.batch * d.c_out * _prod(osz)
    if other is not None and other.numel() != n_out:   # the reference .view()s it to this shape
        raise RuntimeError("%s has %d elements, expected %s" % (other_name, other.numel(),
                                                                (d.batch, d.c_out) + osz))


def _sampling_f32(input, offset, mask=None):
    """fp16 / bf16 tensors with fp32 `offset` and `mask` ("fp32 sampling", include/mdconv.h: MDCONV_SAMPLING_F32):
    sampling positions are not rounded to 16 bits.  Any other mix of dtypes is refused by `_same`."""
    return (input.dtype in (torch.float16, torch.bfloat16) and offset.dtype == torch.float32
            and (mask is None or mask.numel() == 0 or mask.dtype == torch.float32))


def _check_dtypes(d, input, offset, mask, **tensors):
    """`offset` / `mask` (and, in `tensors`, grad_offset / grad_mask) share the input's dtype, or are all fp32 with
    fp16 / bf16 tensors, which sets MDCONV_SAMPLING_F32 in the descriptor; every other tensor has the input's dtype."""
    side = {k: tensors.pop(k) for k in ("grad_offset", "grad_mask") if k in tensors}
    if not _sampling_f32(input, offset, mask):
        _same(input, offset=offset, mask=mask, **side, **tensors)
        return
    _same(input, **tensors)
    if offset.device != input.device:
        raise RuntimeError("offset must be on the device of input (%s), got %s" % (input.device, offset.device))
    _same(offset, mask=mask, **side)
    d.dtype |= _capi.SAMPLING_F32


def _wgrad_f32(d, input, grad_weight, grad_bias, with_bias):
    """fp16 / bf16 tensors with fp32 `grad_weight` (and `grad_bias`, where the call has one): "fp32 weight gradients"
    (include/mdconv.h: MDCONV_WGRAD_F32) -- sets the bit in the descriptor and returns True.  One fp32 and one 16-bit
    tensor of the pair is refused, like any other mix of dtypes."""
    if input.dtype not in (torch.float16, torch.bfloat16):
        return False
    has_bias = with_bias and grad_bias is not None and grad_bias.numel() > 0
    if grad_weight.dtype != torch.float32 and not (has_bias and grad_bias.dtype == torch.float32):
        return False
    for name, g in (("grad_weight", grad_weight),) + ((("grad_bias", grad_bias),) if has_bias else ()):
        if g.dtype != torch.float32 or g.device != input.device:
            raise RuntimeError("%s must be fp32 on the device of input when the other weight gradient is fp32 "
                               "(fp32 weight gradients), got %s/%s" % (name, g.dtype, g.device))
    d.dtype |= _capi.WGRAD_F32
    return True


def _same(ref, **tensors):
    for name, t in tensors.items():
        if t is None or t.numel() == 0:
            continue
        if t.dtype != ref.dtype or t.device != ref.device:
            raise RuntimeError("%s must have the dtype/device of input (%s/%s), got %s/%s"
                               % (name, ref.dtype, ref.device, t.dtype, t.device))


_warned_nondeterministic = False


def _check_deterministic(L, d):
    """A backward in deterministic mode the library cannot run deterministically (it would end on the shape-generic
    kernels: floating-point atomics): RuntimeError -- or, when the mode comes from torch.use_deterministic_algorithms
    with warn_only=True, one UserWarning per process and the call runs without the flag."""
    global _warned_nondeterministic
    if L.mdconv_deterministic_supported(ctypes.byref(d), 1):
        return
    msg = _capi.last_error()   # the library's reason: floating-point atomics, and the shape rule that sent the call there
    if _capi.deterministic_override() is None and torch.is_deterministic_algorithms_warn_only_enabled():
        if not _warned_nondeterministic:
            _warned_nondeterministic = True
            warnings.warn("modulated_deform_conv_amd: " + msg + "; running it non-deterministically "
                          "(torch.use_deterministic_algorithms(True, warn_only=True)). This warning is issued once.",
                          UserWarning, stacklevel=3)
        d.flags &= ~_capi.FLAG_DETERMINISTIC
        return
    raise RuntimeError("modulated_deform_conv_amd does not have a deterministic implementation of this backward: " + msg
                       + ". Use torch.use_deterministic_algorithms(True, warn_only=True) or "
                       "modulated_deform_conv_amd._capi.deterministic(False) to run it anyway.")


def _run(fn_name, d, backward, args_before_ws, input):
    L = _capi.lib()
    d.input_layout = int(not input.is_contiguous() and _is_channels_last(input))
    if backward and d.flags & _capi.FLAG_DETERMINISTIC:
        _check_deterministic(L, d)
    with torch.cuda.device(input.device):
        ws_bytes = L.mdconv_workspace_bytes(ctypes.byref(d), int(backward))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=input.device) if ws_bytes else None
        stream = torch.cuda.current_stream().cuda_stream
        rc = getattr(L, fn_name)(ctypes.byref(d), *args_before_ws,
                                 ctypes.c_void_p(ws.data_ptr() if ws is not None else 0),
                                 ctypes.c_size_t(ws_bytes), ctypes.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (fn_name, rc, _capi.last_error()))


def _prod(v):
    p = 1
    for x in v:
        p *= int(x)
    return p


def _forward(nd, modulated, fn_name, input, weight, bias, offset, mask, output, ksz, stride, pad,
             dil, group, deformable_group, in_step, with_bias):
    tensors = dict(input=input, weight=weight, bias=bias, offset=offset)
    if modulated:
        tensors["mask"] = mask
    if output is not None:
        tensors["output"] = output
    _check_contig(**tensors)
    d = _desc(nd, modulated, input, weight, ksz, stride, pad, dil, group, deformable_group, in_step,
              with_bias)
    cl_input = input if output is None and _capi.channels_last_results_mode() else None
    input = _layout(d, input, False)
    osz = _out_shape(d, nd)
    _check_side(d, nd, _prod(ksz), offset, mask if modulated else None, output, "output", osz)
    _check_dtypes(d, input, offset, mask if modulated else None, weight=weight,
                  bias=bias if with_bias else None, output=output)
    if with_bias and bias.numel() != d.c_out:
        raise RuntimeError("bias has %d elements, expected %d" % (bias.numel(), d.c_out))
    final = None
    if output is None:
        # (inside _capi.channels_last_results: channels-last when the `input` the caller gave is and the forward stores it)
        fmt = torch.contiguous_format
        if cl_input is not None and channels_last_results_supported(nd, modulated, cl_input, weight, ksz, stride, pad, dil, group,
                                                        deformable_group, in_step, with_bias, False):
            fmt = torch.channels_last if nd == 2 else torch.channels_last_3d
        output = torch.empty((d.batch, d.c_out) + osz, dtype=input.dtype, device=input.device, memory_format=fmt)
    if _cl_result(output):
        if _result_flags(d, input, False, output):
            _capi.require_aligned_result("MDCONV_CUDA", "output", output)   # stored as vectors: pointer class "16-byte"
        else:
            final, output = output, torch.empty_like(output, memory_format=torch.contiguous_format)   # (the fallback: copied below)
    args = [_ptr(input), _ptr(weight), _ptr(bias), _ptr(offset)]
    if modulated:
        args.append(_ptr(mask))
    args.append(_ptr(output))
    _run(fn_name, d, False, args, input)
    if final is not None:
        final.copy_(output)
        output = final
    return output


# --------------------------------------------------------------------------------- 2-D, DCNv1
def deform_conv2d_forward_cuda(input, weight, bias, offset, output, kernel_h, kernel_w, stride_h,
                               stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
                               deformable_group, in_step, with_bias):
    """reference deformable_conv.cu:117-123; writes ``output`` in place, returns 0."""
    _forward(2, False, "mdconv_deform_conv2d_forward", input, weight, bias, offset, None, output,
             (kernel_h, kernel_w), (stride_h, stride_w), (pad_h, pad_w), (dilation_h, dilation_w),
             group, deformable_group, in_step, with_bias)
    return 0


def deform_conv2d_backward_cuda(input, weight, bias, offset, grad_input, grad_weight, grad_bias,
                                grad_offset, grad_output, kernel_h, kernel_w, stride_h, stride_w,
                                pad_h, pad_w, dilation_h, dilation_w, group, deformable_group,
                                in_step, with_bias):
    """reference deformable_conv.cu:327-333; accumulates into the four grad tensors, returns 0."""
    grad_input, grad_weight, grad_bias = _skipped(grad_input, grad_weight, grad_bias)
    _check_contig(input=input, weight=weight, bias=bias, offset=offset, grad_input=grad_input,
                  grad_weight=grad_weight, grad_bias=grad_bias, grad_offset=grad_offset,
                  grad_output=grad_output)
    d = _desc(2, False, input, weight, (kernel_h, kernel_w), (stride_h, stride_w), (pad_h, pad_w),
              (dilation_h, dilation_w), group, deformable_group, in_step, with_bias)
    input = _layout(d, input, True)
    osz = _out_shape(d, 2)
    _check_side(d, 2, kernel_h * kernel_w, offset, None, grad_output, "grad_output", osz)
    _backward_checks(input, weight, offset, None, grad_input, grad_weight, grad_bias, grad_offset,
                     None, grad_output, d, with_bias)
    grad_output, grad_input, final = _backward_layouts(d, input, grad_output, grad_input)
    _run("mdconv_deform_conv2d_backward", d, True,
         [_ptr(input), _ptr(weight), _ptr(bias), _ptr(offset), _ptr(grad_input), _ptr(grad_weight),
          _ptr(grad_bias), _ptr(grad_offset), _ptr(grad_output)], input)
    if final is not None:
        final.copy_(grad_input)
    return 0


def _backward_checks(input, weight, offset, mask, grad_input, grad_weight, grad_bias, grad_offset,
                     grad_mask, grad_output, d, with_bias):
    # (None: a gradient the call leaves out, _capi.skip_grads -- nothing to check)
    wgrads = {} if grad_weight is None or _wgrad_f32(d, input, grad_weight, grad_bias, with_bias) else dict(
        grad_weight=grad_weight, grad_bias=grad_bias if with_bias else None)
    _check_dtypes(d, input, offset, mask, weight=weight, grad_input=grad_input, grad_offset=grad_offset,
                  grad_mask=grad_mask, grad_output=grad_output, **wgrads)
    for name, g, ref in (("grad_input", grad_input, input), ("grad_weight", grad_weight, weight),
                         ("grad_offset", grad_offset, offset), ("grad_mask", grad_mask, mask)):
        if ref is not None and g is not None and g.numel() != ref.numel():
            raise RuntimeError("%s has %d elements, expected %d" % (name, g.numel(), ref.numel()))
    if with_bias and grad_weight is not None and grad_bias.numel() != d.c_out:
        raise RuntimeError("grad_bias has %d elements, expected %d" % (grad_bias.numel(), d.c_out))


# --------------------------------------------------------------------------------- 2-D, DCNv2
def modulated_deform_conv2d_forward_cuda(input, weight, bias, offset, mask, kernel_h, kernel_w,
                                         stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
                                         group, deformable_group, in_step, with_bias):
    """reference mdeformable_conv.cu:120-126; returns a NEW tensor [B, O, Ho, Wo]."""
    return _forward(2, True, "mdconv_modulated_deform_conv2d_forward", input, weight, bias, offset,
                    mask, None, (kernel_h, kernel_w), (stride_h, stride_w), (pad_h, pad_w),
                    (dilation_h, dilation_w), group, deformable_group, in_step, with_bias)


def modulated_deform_conv2d_backward_cuda(input, weight, bias, offset, mask, grad_output, kernel_h,
                                          kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
                                          dilation_w, group, deformable_group, in_step, with_bias):
    """reference mdeformable_conv.cu:361-366, 456; returns the tuple
    (grad_input, grad_offset, grad_mask, grad_weight, grad_bias) of new tensors."""
    return _modulated2d_backward(True, input, weight, bias, offset, mask, grad_output, kernel_h, kernel_w, stride_h,
                                 stride_w, pad_h, pad_w, dilation_h, dilation_w, group, deformable_group, in_step, with_bias)


def _modulated2d_backward(fused, input, weight, bias, offset, mask, grad_output, kernel_h, kernel_w, stride_h, stride_w,
                          pad_h, pad_w, dilation_h, dilation_w, group, deformable_group, in_step, with_bias):
    """`fused`: grad_weight and grad_bias are views of ONE buffer (the data-parallel exchange reduces it in place);
    False for torch.library operators, whose returns must not share storage (ops.py)."""
    _check_contig(input=input, weight=weight, bias=bias, offset=offset, mask=mask)
    if not (_capi.channels_last_results_mode() and _cl_result(grad_output)):   # (inside the mode: channels-last as it is)
        grad_output = grad_output.contiguous()
    d = _desc(2, True, input, weight, (kernel_h, kernel_w), (stride_h, stride_w), (pad_h, pad_w),
              (dilation_h, dilation_w), group, deformable_group, in_step, with_bias)
    # (inside _capi.channels_last_results: grad_input channels-last when the `input` the caller gave is and the backward stores it)
    gi_fmt = torch.channels_last if channels_last_results_supported(
        2, True, input, weight, (kernel_h, kernel_w), (stride_h, stride_w), (pad_h, pad_w), (dilation_h, dilation_w), group,
        deformable_group, in_step, with_bias, True) else torch.contiguous_format
    input = _layout(d, input, True)
    osz = _out_shape(d, 2)
    _check_side(d, 2, kernel_h * kernel_w, offset, mask, grad_output, "grad_output", osz)
    # the reference allocates zeros here (mdeformable_conv.cu:404-411) and adds into them; this
    # entry point owns its results, so it allocates uninitialised memory and asks the library to
    # WRITE the gradients (mdconv_desc.accumulate = 0: no zero fills, no read-modify-write)
    skip_input, skip_weight = _capi.skipped_grads()   # (inside _capi.skip_grads: None for what the call leaves out)
    grad_input = None if skip_input else torch.empty_like(input, memory_format=gi_fmt)
    grad_offset = torch.empty_like(offset)
    grad_mask = torch.empty_like(mask)
    # grad_weight || grad_bias live in ONE flat buffer: the data-parallel exchange is then a single in-place all-reduce
    # (distributed.py: fused_grad_buffers / FusedGradAllReduce)
    # (inside _capi.weight_grads_f32(): fp32 for 16-bit tensors -- the unrounded sums, reduced in place by the exchange)
    wdt = torch.float32 if _capi.weight_grads_f32_mode() and input.dtype in (torch.float16, torch.bfloat16) else None
    if skip_weight:
        grad_weight = grad_bias = None
    else:
        grad_weight, grad_bias = fused_grad_buffers(weight, bias, wdt) if fused else (torch.empty_like(weight), torch.empty_like(bias))
    _backward_checks(input, weight, offset, mask, grad_input, grad_weight, grad_bias, grad_offset,
                     grad_mask, grad_output, d, with_bias)
    d.accumulate = 0
    grad_output, grad_input, final = _backward_layouts(d, input, grad_output, grad_input)   # (`final`: dropped, the temporary is the result)
    _run("mdconv_modulated_deform_conv2d_backward", d, True,
         [_ptr(input), _ptr(weight), _ptr(bias), _ptr(offset), _ptr(mask), _ptr(grad_output),
          _ptr(grad_input), _ptr(grad_offset), _ptr(grad_mask), _ptr(grad_weight),
          _ptr(grad_bias)], input)
    return (grad_input, grad_offset, grad_mask, grad_weight, grad_bias)


# --------------------------------------------------------------------------------- 3-D, DCNv1
def deform_conv3d_forward_cuda(input, weight, bias, offset, output, kernel_h, kernel_w, kernel_l,
                               stride_h, stride_w, stride_l, pad_h, pad_w, pad_l, dilation_h,
                               dilation_w, dilation_l, group, deformable_group, in_step, with_bias):
    """reference deformable_conv3d.cu:160-167; writes ``output`` in place, returns 0."""
    _forward(3, False, "mdconv_deform_conv3d_forward", input, weight, bias, offset, None, output,
             (kernel_h, kernel_w, kernel_l), (stride_h, stride_w, stride_l), (pad_h, pad_w, pad_l),
             (dilation_h, dilation_w, dilation_l), group, deformable_group, in_step, with_bias)
    return 0


def deform_conv3d_backward_cuda(input, weight, bias, offset, grad_input, grad_weight, grad_bias,
                                grad_offset, grad_output, kernel_h, kernel_w, kernel_l, stride_h,
                                stride_w, stride_l, pad_h, pad_w, pad_l, dilation_h, dilation_w,
                                dilation_l, group, deformable_group, in_step, with_bias):
    """reference deformable_conv3d.cu:434-442; accumulates, returns 0."""
    grad_input, grad_weight, grad_bias = _skipped(grad_input, grad_weight, grad_bias)
    _check_contig(input=input, weight=weight, bias=bias, offset=offset, grad_input=grad_input,
                  grad_weight=grad_weight, grad_bias=grad_bias, grad_offset=grad_offset,
                  grad_output=grad_output)
    ksz = (kernel_h, kernel_w, kernel_l)
    d = _desc(3, False, input, weight, ksz, (stride_h, stride_w, stride_l), (pad_h, pad_w, pad_l),
              (dilation_h, dilation_w, dilation_l), group, deformable_group, in_step, with_bias)
    input = _layout(d, input, True)
    osz = _out_shape(d, 3)
    _check_side(d, 3, _prod(ksz), offset, None, grad_output, "grad_output", osz)
    _backward_checks(input, weight, offset, None, grad_input, grad_weight, grad_bias, grad_offset,
                     None, grad_output, d, with_bias)
    grad_output, grad_input, final = _backward_layouts(d, input, grad_output, grad_input)
    _run("mdconv_deform_conv3d_backward", d, True,
         [_ptr(input), _ptr(weight), _ptr(bias), _ptr(offset), _ptr(grad_input), _ptr(grad_weight),
          _ptr(grad_bias), _ptr(grad_offset), _ptr(grad_output)], input)
    if final is not None:
        final.copy_(grad_input)
    return 0


# --------------------------------------------------------------------------------- 3-D, DCNv2
def modulated_deform_conv3d_forward_cuda(input, weight, bias, offset, mask, output, kernel_h,
                                         kernel_w, kernel_l, stride_h, stride_w, stride_l, pad_h,
                                         pad_w, pad_l, dilation_h, dilation_w, dilation_l, group,
                                         deformable_group, in_step, with_bias):
    """reference mdeformable_conv3d.cu:170-177; writes ``output`` in place, returns 0."""
    _forward(3, True, "mdconv_modulated_deform_conv3d_forward", input, weight, bias, offset, mask,
             output, (kernel_h, kernel_w, kernel_l), (stride_h, stride_w, stride_l),
             (pad_h, pad_w, pad_l), (dilation_h, dilation_w, dilation_l), group, deformable_group,
             in_step, with_bias)
    return 0


def modulated_deform_conv3d_backward_cuda(input, weight, bias, offset, mask, grad_input,
                                          grad_weight, grad_bias, grad_offset, grad_mask,
                                          grad_output, kernel_h, kernel_w, kernel_l, stride_h,
                                          stride_w, stride_l, pad_h, pad_w, pad_l, dilation_h,
                                          dilation_w, dilation_l, group, deformable_group, in_step,
                                          with_bias):
    """reference mdeformable_conv3d.cu:443-451; accumulates, returns 0."""
    grad_input, grad_weight, grad_bias = _skipped(grad_input, grad_weight, grad_bias)
    _check_contig(input=input, weight=weight, bias=bias, offset=offset, mask=mask,
                  grad_input=grad_input, grad_weight=grad_weight, grad_bias=grad_bias,
                  grad_offset=grad_offset, grad_mask=grad_mask, grad_output=grad_output)
    ksz = (kernel_h, kernel_w, kernel_l)
    d = _desc(3, True, input, weight, ksz, (stride_h, stride_w, stride_l), (pad_h, pad_w, pad_l),
              (dilation_h, dilation_w, dilation_l), group, deformable_group, in_step, with_bias)
    input = _layout(d, input, True)
    osz = _out_shape(d, 3)
    _check_side(d, 3, _prod(ksz), offset, mask, grad_output, "grad_output", osz)
    _backward_checks(input, weight, offset, mask, grad_input, grad_weight, grad_bias, grad_offset,
                     grad_mask, grad_output, d, with_bias)
    grad_output, grad_input, final = _backward_layouts(d, input, grad_output, grad_input)
    _run("mdconv_modulated_deform_conv3d_backward", d, True,
         [_ptr(input), _ptr(weight), _ptr(bias), _ptr(offset), _ptr(mask), _ptr(grad_input),
          _ptr(grad_weight), _ptr(grad_bias), _ptr(grad_offset), _ptr(grad_mask),
          _ptr(grad_output)], input)
    if final is not None:
        final.copy_(grad_input)
    return 0
