"""DCNv3 core operator on the MI355X-native backend: grouped deformable sampling on channels-last tensors
(include/mdconv.h, "DCNv3 core operator"; INTEGRATION.md has the contract and what is unpinned).

    DCNv3Function   autograd.Function over mdconv_dcnv3_forward / mdconv_dcnv3_backward
    dcnv3_core      the functional form
    DCNv3           nn.Module: the block around the operator, composed from framework operators
    DCNv3Fused      the same block, parameters and checkpoints on the DCNv4 operator with its in-kernel softmax (dcnv4.py):
                    one linear layer for offsets and mask logits, no framework softmax

The operator has no weight: ``input [B, H, W, G*D]``, ``offset [B, Ho, Wo, G*K*2]`` ((x, y) per tap, taps width-major),
``mask [B, Ho, Wo, G*K]`` -> ``output [B, Ho, Wo, G*D]``, fp32 / fp16 / bf16, one dtype per call.  CPU tensors raise
``NotImplementedError``: there is no CPU or PyTorch fallback.
"""
import ctypes
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.amp import custom_bwd, custom_fwd
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from . import _capi, _samp
from ._samp import DTYPES as _DTYPES, ptr as _ptr

__all__ = ["DCNv3Function", "dcnv3_core", "DCNv3", "DCNv3Fused"]



def _desc(input, kernel, stride, pad, dilation, group, group_channels, offset_scale, accumulate=1, flags=0):
    if input.dtype not in _DTYPES:
        raise TypeError("dcnv3: dtype %s is not float32, float16 or bfloat16" % input.dtype)
    d = _capi.MdconvDcnv3Desc()
    d.dtype, d.batch, d.groups, d.group_channels = _DTYPES[input.dtype], input.shape[0], int(group), int(group_channels)
    d.in_sz = (ctypes.c_int * 2)(int(input.shape[1]), int(input.shape[2]))
    for name, v in (("k_sz", kernel), ("stride", stride), ("pad", pad), ("dil", dilation)):
        setattr(d, name, (ctypes.c_int * 2)(*(int(x) for x in _pair(v))))
    d.offset_scale, d.accumulate, d.flags = float(offset_scale), int(accumulate), int(flags)
    return d


def _out_hw(d):
    L = _capi.lib()
    return tuple(int(L.mdconv_dcnv3_out_size(ctypes.byref(d), a)) for a in (0, 1))


def _check(d, input, offset, mask, **others):
    """Shapes, dtypes, devices and density of the tensors of a call; ``others`` have the shape of ``output``."""
    if input.dim() != 4 or input.shape[3] != d.groups * d.group_channels:
        raise ValueError("dcnv3: input must be [B, H, W, group * group_channels = %d], got %s" % (
            d.groups * d.group_channels, tuple(input.shape)))
    ho, wo = _out_hw(d)
    if ho < 1 or wo < 1:
        raise ValueError("dcnv3: the output extent is below 1 (%d x %d)" % (ho, wo))
    K = d.k_sz[0] * d.k_sz[1]
    want = dict(offset=(d.batch, ho, wo, d.groups * K * 2), mask=(d.batch, ho, wo, d.groups * K))
    want.update({k: (d.batch, ho, wo, d.groups * d.group_channels) for k in others})
    for name, t in dict(offset=offset, mask=mask, **others).items():
        if tuple(t.shape) != want[name]:
            raise ValueError("dcnv3: %s must be %s, got %s" % (name, want[name], tuple(t.shape)))
    for name, t in dict(input=input, offset=offset, mask=mask, **others).items():
        if t.dtype != input.dtype or t.device != input.device:
            raise ValueError("dcnv3: %s is %s on %s, input is %s on %s (one dtype and one device per call)" % (
                name, t.dtype, t.device, input.dtype, input.device))
        if not t.is_contiguous():
            raise ValueError("dcnv3: %s must be dense and row-major (contiguous)" % name)
    return (d.batch, ho, wo, d.groups * d.group_channels)


# the call itself (the seam the tests replace): workspace query, allocation, current stream, call, RuntimeError
_run = functools.partial(_samp.run, "mdconv_dcnv3")


def dcnv3_forward(input, offset, mask, kernel, stride, pad, dilation, group, group_channels, offset_scale, output=None):
    """The forward entry point on dense CUDA tensors; allocates ``output`` unless it is given."""
    if not input.is_cuda:
        raise NotImplementedError
    d = _desc(input, kernel, stride, pad, dilation, group, group_channels, offset_scale)
    others = {} if output is None else dict(output=output)
    shape = _check(d, input, offset, mask, **others)
    # pointer classes (include/mdconv.h): input and output are "16-byte", offset and mask "element"
    _capi.require_aligned_result("dcnv3", "output", output)
    input = _capi.aligned_input(input)
    if output is None:
        output = torch.empty(shape, dtype=input.dtype, device=input.device)
    _run("mdconv_dcnv3_forward", d, False, [_ptr(input), _ptr(offset), _ptr(mask), _ptr(output)], input)
    return output


def dcnv3_backward(input, offset, mask, grad_output, kernel, stride, pad, dilation, group, group_channels, offset_scale,
                   grads=None, need_grad_input=True, deterministic=None, accumulate=None):
    """The backward entry point.  ``grads`` = (grad_input | None, grad_offset, grad_mask): caller-allocated buffers the
    gradients are ADDED to; without it fresh tensors are written.  ``need_grad_input`` false: grad_input is neither computed
    nor allocated (``MDCONV_FLAG_NO_GRAD_INPUT``) and None is returned there.  ``deterministic`` None follows
    ``_capi.deterministic_mode()``.  ``accumulate`` false with ``grads``: the caller's buffers are overwritten instead.
    Returns (grad_input | None, grad_offset, grad_mask)."""
    if not input.is_cuda:
        raise NotImplementedError
    flags = _samp.backward_flags(deterministic, need_grad_input)
    d = _desc(input, kernel, stride, pad, dilation, group, group_channels, offset_scale,
              accumulate=int(grads is not None if accumulate is None else bool(accumulate)), flags=flags)
    _check(d, input, offset, mask, grad_output=grad_output)
    # pointer classes (include/mdconv.h): input, grad_output and grad_input are "16-byte", the coordinate tensors "element"
    if grads is not None and need_grad_input:
        _capi.require_aligned_result("dcnv3", "grad_input", grads[0])
    input, grad_output = _capi.aligned_input(input), _capi.aligned_input(grad_output)
    if grads is None:
        grads = (torch.empty_like(input) if need_grad_input else None, torch.empty_like(offset), torch.empty_like(mask))
    gi, goff, gm = grads
    _samp.check_grads("dcnv3", (("grad_input", gi, input), ("grad_offset", goff, offset), ("grad_mask", gm, mask)),
                      may_be_none=() if need_grad_input else ("grad_input",))
    _run("mdconv_dcnv3_backward", d, True,
         [_ptr(input), _ptr(offset), _ptr(mask), _ptr(grad_output), _ptr(gi if need_grad_input else None), _ptr(goff), _ptr(gm)],
         input)
    return (gi if need_grad_input else None), goff, gm


class DCNv3Function(Function):
    """``DCNv3Function.apply(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
    dilation_w, group, group_channels, offset_scale, im2col_step=256)`` -- the argument order of the published operator;
    ``im2col_step`` is accepted for signature parity and unused.  Under ``torch.autocast`` the three tensors run in the
    autocast dtype and the gradients go back in the dtypes the caller's tensors have."""

    @staticmethod
    @custom_fwd(device_type="cuda")
    def forward(ctx, input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
                group, group_channels, offset_scale, im2col_step=256):
        if not input.is_cuda:
            raise NotImplementedError
        ctx.geo = ((kernel_h, kernel_w), (stride_h, stride_w), (pad_h, pad_w), (dilation_h, dilation_w), group,
                   group_channels, offset_scale)
        ctx.in_dtypes = (input.dtype, offset.dtype, mask.dtype)
        if torch.is_autocast_enabled("cuda"):
            dt = torch.get_autocast_dtype("cuda")
            input, offset, mask = (t if t.dtype == dt else t.to(dt) for t in (input, offset, mask))
        input, offset, mask = input.contiguous(), offset.contiguous(), mask.contiguous()
        if input.requires_grad or offset.requires_grad or mask.requires_grad or any(ctx.needs_input_grad[:3]):
            ctx.save_for_backward(input, offset, mask)
        return dcnv3_forward(input, offset, mask, *ctx.geo)

    @staticmethod
    @custom_bwd(device_type="cuda")
    @once_differentiable
    def backward(ctx, grad_output):
        if not grad_output.is_cuda:
            raise NotImplementedError
        input, offset, mask = ctx.saved_tensors
        grad_output = grad_output.contiguous()
        if grad_output.dtype != input.dtype:
            grad_output = grad_output.to(input.dtype)
        # selective backward: grad_input is neither computed nor allocated when `input` needs no gradient
        grads = dcnv3_backward(input, offset, mask, grad_output, *ctx.geo, need_grad_input=bool(ctx.needs_input_grad[0]))
        back = _samp.back
        return tuple(back(g, dt) for g, dt in zip(grads, ctx.in_dtypes)) + (None,) * 12


def dcnv3_core(input, offset, mask, kernel, stride, pad, dilation, group, group_channels, offset_scale):
    """Functional form; ``kernel``, ``stride``, ``pad`` and ``dilation`` are ints or (h, w) pairs."""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = (_pair(v) for v in (kernel, stride, pad, dilation))
    return DCNv3Function.apply(input, offset, mask, kh, kw, sh, sw, ph, pw, dh, dw, group, group_channels, offset_scale)


class _ToChannelsLast(nn.Module):
    def forward(self, x):
        return x.permute(0, 2, 3, 1)


class DCNv3(nn.Module):
    """The DCNv3 block on ``[B, H, W, C]`` tensors: input projection, the offset branch (depthwise conv, LayerNorm, GELU, then
    the ``offset`` and ``mask`` linears with a softmax over the taps of each group), the core operator, output projection.
    Everything but the core operator is a framework operator.  Module and parameter names follow the published block
    (``dw_conv.0``, ``dw_conv.1.1``, ``offset``, ``mask``, ``input_proj``, ``output_proj``) so that a checkpoint can load --
    written from memory of that code and UNPINNED against it; the ``center_feature_scale`` and
    ``remove_center`` variants are not provided (``remove_center`` is an option of the DCNv4 operator, ``dcnv4.py``)."""

    def __init__(self, channels=64, kernel_size=3, dw_kernel_size=None, stride=1, pad=1, dilation=1, group=4,
                 offset_scale=1.0):
        super().__init__()
        if channels % group:
            raise ValueError("channels must be divisible by group, but got %d and %d" % (channels, group))
        dw_kernel_size = kernel_size if dw_kernel_size is None else dw_kernel_size
        self.channels, self.kernel_size, self.dw_kernel_size = channels, kernel_size, dw_kernel_size
        self.stride, self.pad, self.dilation = stride, pad, dilation
        self.group, self.group_channels, self.offset_scale = group, channels // group, offset_scale
        self.dw_conv = nn.Sequential(
            nn.Conv2d(channels, channels, kernel_size=dw_kernel_size, stride=1, padding=(dw_kernel_size - 1) // 2, groups=channels),
            nn.Sequential(_ToChannelsLast(), nn.LayerNorm(channels, eps=1e-6)),
            nn.GELU())
        self.offset = nn.Linear(channels, group * kernel_size * kernel_size * 2)
        self.mask = nn.Linear(channels, group * kernel_size * kernel_size)
        self.input_proj = nn.Linear(channels, channels)
        self.output_proj = nn.Linear(channels, channels)
        self._core = dcnv3_core
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.offset, self.mask):
            nn.init.zeros_(lin.weight)
            nn.init.zeros_(lin.bias)
        for lin in (self.input_proj, self.output_proj):
            nn.init.xavier_uniform_(lin.weight)
            nn.init.zeros_(lin.bias)

    def forward(self, input):
        B, H, W, _ = input.shape
        x = self.input_proj(input)
        x1 = self.dw_conv(input.permute(0, 3, 1, 2))
        offset = self.offset(x1)
        mask = F.softmax(self.mask(x1).reshape(B, H, W, self.group, -1), -1).reshape(B, H, W, -1)
        # (softmax runs in fp32 under autocast: one dtype per call)
        x = self._core(x, offset.to(x.dtype), mask.to(x.dtype), self.kernel_size, self.stride, self.pad, self.dilation,
                       self.group, self.group_channels, self.offset_scale)
        return self.output_proj(x)

    def extra_repr(self):
        return "channels=%d, kernel_size=%d, stride=%d, pad=%d, dilation=%d, group=%d, offset_scale=%g" % (
            self.channels, self.kernel_size, self.stride, self.pad, self.dilation, self.group, self.offset_scale)


class DCNv3Fused(DCNv3):
    """``DCNv3`` with the constructor, parameters, initialisation and ``state_dict`` keys of ``DCNv3`` -- the same
    checkpoints load -- on the DCNv4 operator with ``softmax=True``: what ``FlashDeformAttn`` is to ``MSDeformAttn``.  The
    forward gathers ONE packed weight ``[OM, C]`` and bias ``[OM]`` from ``offset.weight / bias`` and ``mask.weight / bias``
    through a fixed row index (``pack_index``: per group the 2K offset rows, then the K mask rows, then zero rows for the
    row's padding; autograd carries the gradients back to both parameters), runs one ``F.linear`` whose output is the
    operator's packed row as it stands, and calls ``dcnv4_core(..., softmax=True)``: no framework softmax, no
    activation-sized concatenation, no cast of a materialised mask.  Under autocast the packed row has the autocast dtype
    and the softmax is taken in fp32 inside the kernels."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        from .dcnv4 import dcnv4_core
        self._core = dcnv4_core
        # (not persistent: the state_dict keys are DCNv3's)
        self.register_buffer("pack_index", self.make_pack_index(self.group, self.kernel_size * self.kernel_size),
                             persistent=False)

    @staticmethod
    def make_pack_index(group, K):
        """Rows of ``cat([offset rows (G*K*2), mask rows (G*K), one zero row])`` in the order of the packed row."""
        om = (group * K * 3 + 7) // 8 * 8
        idx = []
        for g in range(group):
            idx += range(g * 2 * K, (g + 1) * 2 * K)
            idx += range(group * 2 * K + g * K, group * 2 * K + (g + 1) * K)
        idx += [group * 3 * K] * (om - group * 3 * K)
        return torch.tensor(idx, dtype=torch.long)

    def packed_linear(self):
        """(weight [OM, C], bias [OM]) of the one linear layer; tiny tensors, differentiable to the four parameters."""
        w = torch.cat([self.offset.weight, self.mask.weight, self.offset.weight.new_zeros(1, self.channels)], 0)
        b = torch.cat([self.offset.bias, self.mask.bias, self.offset.bias.new_zeros(1)], 0)
        return w.index_select(0, self.pack_index), b.index_select(0, self.pack_index)

    def forward(self, input):
        x = self.input_proj(input)
        x1 = self.dw_conv(input.permute(0, 3, 1, 2))
        offset_mask = F.linear(x1, *self.packed_linear())
        x = self._core(x, offset_mask, self.kernel_size, self.stride, self.pad, self.dilation, self.group,
                       self.group_channels, self.offset_scale, False, softmax=True)
        return self.output_proj(x)
