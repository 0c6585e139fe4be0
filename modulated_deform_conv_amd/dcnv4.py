"""DCNv4 operator on the MI355X-native backend: the DCNv3 core operator's sampling with one packed coordinate tensor
(include/mdconv.h, "DCNv4 operator"; INTEGRATION.md has the contract and what is unpinned).

    dcnv4_forward / dcnv4_backward   the entry points on dense CUDA tensors
    DCNv4Function   autograd.Function over mdconv_dcnv4_forward / mdconv_dcnv4_backward
    dcnv4_core      the functional form
    DCNv4           nn.Module: the block around the operator, composed from framework operators

The operator has no weight and, by default, no softmax: ``input [B, H, W, G*D]``, ``offset_mask [B, Ho, Wo, OM]`` ->
``output [B, Ho, Wo, G*D]``.  A row of ``offset_mask`` holds, per group, the (x, y) offsets of the K taps and then their K
masks, and is padded to ``OM = ceil(G*K*3 / 8) * 8`` elements (``offset_mask_len``); ``K = kh*kw``, minus one with
``remove_center``.  With ``softmax=True`` (``MDCONV_FLAG_SOFTMAX``) the K masks of a group are logits and the kernels take
their softmax themselves -- DCNv3's softmax over the taps, over all K tensor taps, gated-out ones included.  ``input`` is fp32 / fp16 / bf16; ``offset_mask`` has its dtype or is fp32.  CPU tensors raise
``NotImplementedError``: there is no CPU or PyTorch fallback.
"""
import ctypes
import functools

import torch
import torch.nn as nn
from torch.amp import custom_bwd, custom_fwd
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from . import _capi, _samp
from ._samp import DTYPES as _DTYPES, ptr as _ptr

__all__ = ["dcnv4_forward", "dcnv4_backward", "offset_mask_len", "DCNv4Function", "dcnv4_core", "DCNv4"]



def offset_mask_len(kernel, group, remove_center=False):
    """OM: the elements per row of ``offset_mask`` for ``group`` groups of a ``kernel`` (int or (h, w)) kernel."""
    kh, kw = _pair(kernel)
    return (int(group) * (kh * kw - int(bool(remove_center))) * 3 + 7) // 8 * 8


def _desc(input, offset_mask, kernel, stride, pad, dilation, group, group_channels, offset_scale, remove_center,
          accumulate=1, flags=0):
    if input.dtype not in _DTYPES or offset_mask.dtype not in _DTYPES:
        raise TypeError("dcnv4: dtypes %s / %s are not float32, float16 or bfloat16" % (input.dtype, offset_mask.dtype))
    if input.dim() != 4:
        raise ValueError("dcnv4: input must be [B, H, W, group * group_channels], got %s" % (tuple(input.shape),))
    d = _capi.MdconvDcnv4Desc()
    d.dtype, d.coord_dtype = _DTYPES[input.dtype], _DTYPES[offset_mask.dtype]
    d.batch, d.groups, d.group_channels = int(input.shape[0]), int(group), int(group_channels)
    d.in_sz = (ctypes.c_int * 2)(int(input.shape[1]), int(input.shape[2]))
    for name, v in (("k_sz", kernel), ("stride", stride), ("pad", pad), ("dil", dilation)):
        setattr(d, name, (ctypes.c_int * 2)(*(int(x) for x in _pair(v))))
    d.offset_scale, d.remove_center = float(offset_scale), int(bool(remove_center))
    d.accumulate, d.flags = int(accumulate), int(flags)
    return d


def _check(d, input, offset_mask, **others):
    """Shapes, dtypes, devices and density of the tensors of a call; ``others`` have the shape of ``output``."""
    L = _capi.lib()
    if input.shape[3] != d.groups * d.group_channels:
        raise ValueError("dcnv4: input must be [B, H, W, group * group_channels = %d], got %s" % (
            d.groups * d.group_channels, tuple(input.shape)))
    if offset_mask.dtype != input.dtype and offset_mask.dtype != torch.float32:
        raise ValueError("dcnv4: offset_mask is %s, input is %s: it must have input's dtype or float32" % (
            offset_mask.dtype, input.dtype))
    om = int(L.mdconv_dcnv4_offset_mask_len(ctypes.byref(d)))
    if om < 0:
        raise ValueError("dcnv4: %s" % _capi.last_error())
    ho, wo = (int(L.mdconv_dcnv4_out_size(ctypes.byref(d), a)) for a in (0, 1))
    K = d.k_sz[0] * d.k_sz[1] - d.remove_center
    if tuple(offset_mask.shape) != (d.batch, ho, wo, om):
        raise ValueError("dcnv4: offset_mask must be %s -- OM = %d: %d groups x %d taps x 3, padded to a multiple of 8 -- got %s" % (
            (d.batch, ho, wo, om), om, d.groups, K, tuple(offset_mask.shape)))
    shape = (d.batch, ho, wo, d.groups * d.group_channels)
    for name, t in others.items():
        if tuple(t.shape) != shape:
            raise ValueError("dcnv4: %s must be %s, got %s" % (name, shape, tuple(t.shape)))
    for name, t in dict(input=input, offset_mask=offset_mask, **others).items():
        if (name != "offset_mask" and t.dtype != input.dtype) or t.device != input.device:
            raise ValueError("dcnv4: %s is %s on %s, input is %s on %s (input, output and grad_output share one dtype and "
                             "every tensor one device)" % (name, t.dtype, t.device, input.dtype, input.device))
        if not t.is_contiguous():
            raise ValueError("dcnv4: %s must be dense and row-major (contiguous)" % name)
    return shape


# the call itself (the seam the tests replace): workspace query, allocation, current stream, call, RuntimeError
_run = functools.partial(_samp.run, "mdconv_dcnv4")


def dcnv4_forward(input, offset_mask, kernel, stride, pad, dilation, group, group_channels, offset_scale,
                  remove_center=False, output=None, softmax=False):
    """The forward entry point on dense CUDA tensors; allocates ``output`` unless it is given.  ``softmax``: the masks are
    logits (``MDCONV_FLAG_SOFTMAX``)."""
    if not input.is_cuda:
        raise NotImplementedError
    d = _desc(input, offset_mask, kernel, stride, pad, dilation, group, group_channels, offset_scale, remove_center,
              flags=_capi.FLAG_SOFTMAX if softmax else 0)
    others = {} if output is None else dict(output=output)
    shape = _check(d, input, offset_mask, **others)
    # pointer classes (include/mdconv.h): input and output are "16-byte", offset_mask "element"
    _capi.require_aligned_result("dcnv4", "output", output)
    input = _capi.aligned_input(input)
    if output is None:
        output = torch.empty(shape, dtype=input.dtype, device=input.device)
    _run("mdconv_dcnv4_forward", d, False, [_ptr(input), _ptr(offset_mask), _ptr(output)], input)
    return output


def dcnv4_backward(input, offset_mask, grad_output, kernel, stride, pad, dilation, group, group_channels, offset_scale,
                   remove_center=False, grads=None, need_grad_input=True, deterministic=None, accumulate=None, softmax=False):
    """The backward entry point.  ``grads`` = (grad_input | None, grad_offset_mask): caller-allocated buffers the gradients
    are ADDED to (their padding columns stay untouched); without it fresh tensors are written, the padding columns of
    grad_offset_mask as zeros.  ``need_grad_input`` false: grad_input is neither computed nor allocated
    (``MDCONV_FLAG_NO_GRAD_INPUT``) and None is returned there.  ``deterministic`` None follows
    ``_capi.deterministic_mode()``.  ``accumulate`` false with ``grads``: the caller's buffers are overwritten instead.
    ``softmax``: the masks are logits (``MDCONV_FLAG_SOFTMAX``), and their columns of grad_offset_mask the logits' gradients.
    Returns (grad_input | None, grad_offset_mask)."""
    if not input.is_cuda:
        raise NotImplementedError
    flags = _samp.backward_flags(deterministic, need_grad_input)
    flags |= _capi.FLAG_SOFTMAX if softmax else 0
    d = _desc(input, offset_mask, kernel, stride, pad, dilation, group, group_channels, offset_scale, remove_center,
              accumulate=int(grads is not None if accumulate is None else bool(accumulate)), flags=flags)
    _check(d, input, offset_mask, grad_output=grad_output)
    # pointer classes (include/mdconv.h): input, grad_output and grad_input are "16-byte", offset_mask and its gradient "element"
    if grads is not None and need_grad_input:
        _capi.require_aligned_result("dcnv4", "grad_input", grads[0])
    input, grad_output = _capi.aligned_input(input), _capi.aligned_input(grad_output)
    if grads is None:
        grads = (torch.empty_like(input) if need_grad_input else None, torch.empty_like(offset_mask))
    gi, gom = grads
    _samp.check_grads("dcnv4", (("grad_input", gi, input), ("grad_offset_mask", gom, offset_mask)),
                      may_be_none=() if need_grad_input else ("grad_input",))
    _run("mdconv_dcnv4_backward", d, True,
         [_ptr(input), _ptr(offset_mask), _ptr(grad_output), _ptr(gi if need_grad_input else None), _ptr(gom)], input)
    return (gi if need_grad_input else None), gom


class DCNv4Function(Function):
    """``DCNv4Function.apply(input, offset_mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
    dilation_w, group, group_channels, offset_scale, im2col_step, remove_center[, softmax])`` -- the argument order of the
    published operator, then the optional ``softmax`` (the masks are logits); ``im2col_step`` is accepted for signature
    parity and unused.  Under ``torch.autocast`` ``input`` runs in the
    autocast dtype.  ``offset_mask`` keeps its dtype when that is the dtype ``input`` runs in or float32 (the mixed call)
    and is cast to the former otherwise.  The gradients go back in the dtypes the caller's tensors have."""

    @staticmethod
    @custom_fwd(device_type="cuda")
    def forward(ctx, input, offset_mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
                group, group_channels, offset_scale, im2col_step=256, remove_center=False, softmax=False):
        if not input.is_cuda:
            raise NotImplementedError
        ctx.geo = ((kernel_h, kernel_w), (stride_h, stride_w), (pad_h, pad_w), (dilation_h, dilation_w), group,
                   group_channels, offset_scale, bool(remove_center))
        ctx.softmax = bool(softmax)
        ctx.in_dtypes = (input.dtype, offset_mask.dtype)
        if torch.is_autocast_enabled("cuda"):
            input = input.to(torch.get_autocast_dtype("cuda"))
        if offset_mask.dtype not in (input.dtype, torch.float32):
            offset_mask = offset_mask.to(input.dtype)
        input, offset_mask = input.contiguous(), offset_mask.contiguous()
        if any(ctx.needs_input_grad[:2]):
            ctx.save_for_backward(input, offset_mask)
        return dcnv4_forward(input, offset_mask, *ctx.geo, softmax=ctx.softmax)

    @staticmethod
    @custom_bwd(device_type="cuda")
    @once_differentiable
    def backward(ctx, grad_output):
        if not grad_output.is_cuda:
            raise NotImplementedError
        input, offset_mask = ctx.saved_tensors
        grad_output = grad_output.to(input.dtype).contiguous()
        # selective backward: grad_input is neither computed nor allocated when `input` needs no gradient
        grads = dcnv4_backward(input, offset_mask, grad_output, *ctx.geo, need_grad_input=bool(ctx.needs_input_grad[0]),
                               softmax=ctx.softmax)
        back = _samp.back
        return tuple(back(g, dt) for g, dt in zip(grads, ctx.in_dtypes)) + (None,) * 14


def dcnv4_core(input, offset_mask, kernel, stride, pad, dilation, group, group_channels, offset_scale, remove_center=False,
               softmax=False):
    """Functional form; ``kernel``, ``stride``, ``pad`` and ``dilation`` are ints or (h, w) pairs.  ``softmax``: the K masks
    of a group are logits and the operator takes their softmax."""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = (_pair(v) for v in (kernel, stride, pad, dilation))
    return DCNv4Function.apply(input, offset_mask, kh, kw, sh, sw, ph, pw, dh, dw, group, group_channels, offset_scale, 256,
                               remove_center, softmax)


class DCNv4(nn.Module):
    """The DCNv4 block on ``[N, L, C]`` token tensors with ``shape=(H, W)``, ``L = H * W``: ``value_proj``, the
    ``offset_mask`` linear (on the tokens, or on a depthwise convolution ``offset_mask_dw`` of them when
    ``dw_kernel_size`` is given) whose ``OM`` outputs are the operator's packed tensor as they are -- no softmax, or with
    ``softmax=True`` the operator's own over the masks of a group --, the operator, ``output_proj`` (``output_bias`` false: without bias).  ``without_pointwise`` leaves both projections out.
    Everything but the operator is a framework operator.  ``offset_mask`` starts at zero, the projections with Xavier.
    Module and parameter names are written from memory of the published block and UNPINNED against it;
    its ``center_feature_scale`` variant is not provided."""

    def __init__(self, channels=64, kernel_size=3, stride=1, pad=1, dilation=1, group=4, offset_scale=1.0,
                 dw_kernel_size=None, remove_center=False, output_bias=True, without_pointwise=False, softmax=False):
        super().__init__()
        if channels % group:
            raise ValueError("channels must be divisible by group, but got %d and %d" % (channels, group))
        self.channels, self.kernel_size, self.dw_kernel_size = channels, kernel_size, dw_kernel_size
        self.stride, self.pad, self.dilation = stride, pad, dilation
        self.group, self.group_channels, self.offset_scale = group, channels // group, offset_scale
        self.remove_center, self.without_pointwise = bool(remove_center), bool(without_pointwise)
        self.softmax = bool(softmax)
        if dw_kernel_size is not None:
            self.offset_mask_dw = nn.Conv2d(channels, channels, dw_kernel_size, stride=1, padding=(dw_kernel_size - 1) // 2,
                                            groups=channels)
        self.offset_mask = nn.Linear(channels, offset_mask_len(kernel_size, group, remove_center))
        if not without_pointwise:
            self.value_proj = nn.Linear(channels, channels)
            self.output_proj = nn.Linear(channels, channels, bias=output_bias)
        self._core = dcnv4_core
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.zeros_(self.offset_mask.weight)
        nn.init.zeros_(self.offset_mask.bias)
        if not self.without_pointwise:
            for lin in (self.value_proj, self.output_proj):
                nn.init.xavier_uniform_(lin.weight)
                if lin.bias is not None:
                    nn.init.zeros_(lin.bias)

    def forward(self, input, shape=None):
        N, L, C = input.shape
        if shape is None:
            H = W = int(round(L ** 0.5))
        else:
            H, W = shape
        if H * W != L:
            raise ValueError("DCNv4: shape %s does not have the %d tokens of the input" % ((H, W), L))
        x = input if self.without_pointwise else self.value_proj(input)
        tokens = input
        if self.dw_kernel_size is not None:
            tokens = self.offset_mask_dw(input.reshape(N, H, W, C).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).reshape(N, L, C)
        # (the operator's row is the linear layer's output as it stands; it needs the operator's output extent, which is
        # (H, W) for the block's stride-1 "same" geometry)
        offset_mask = self.offset_mask(tokens).reshape(N, H, W, -1)
        # (the keyword is passed only when set: a core swapped in for the plain operator need not know it)
        extra = dict(softmax=True) if self.softmax else {}
        x = self._core(x.reshape(N, H, W, C), offset_mask, self.kernel_size, self.stride, self.pad, self.dilation, self.group,
                       self.group_channels, self.offset_scale, self.remove_center, **extra)
        x = x.reshape(N, -1, C)
        return x if self.without_pointwise else self.output_proj(x)

    def extra_repr(self):
        return "channels=%d, kernel_size=%d, stride=%d, pad=%d, dilation=%d, group=%d, offset_scale=%g, remove_center=%s%s" % (
            self.channels, self.kernel_size, self.stride, self.pad, self.dilation, self.group, self.offset_scale,
            self.remove_center, ", softmax=True" if self.softmax else "")
