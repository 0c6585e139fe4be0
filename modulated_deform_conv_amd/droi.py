"""Deformable RoI pooling on the MI355X-native backend: RoIAlign whose bins are shifted by a learnt offset, the "dpool" /
"mdpool" heads of Deformable ConvNets v1 / v2 detectors (include/mdconv.h, "Deformable RoI pooling"; INTEGRATION.md has the
contract and what is unpinned).

    deform_roi_pool_forward / deform_roi_pool_backward   the entry points on dense channels-last CUDA buffers
    DeformRoIPoolFunction    autograd.Function over mdconv_droi_forward / mdconv_droi_backward, on logical NCHW tensors
    deform_roi_pool          the functional form
    DeformRoIPool, DeformRoIPoolPack, ModulatedDeformRoIPoolPack   nn.Modules

The entry points take ``input [B, H, W, C]``, ``rois [R, 5]`` (fp32: batch index, x1, y1, x2, y2), ``offset [R, 2, PH, PW]``
(plane 0 = x, plane 1 = y; or None) and give ``output [R, PH, PW, C]``.  ``input`` is fp32 / fp16 / bf16; ``offset`` has its
dtype or is fp32.  CPU tensors raise ``NotImplementedError``: there is no CPU or PyTorch fallback.
"""
import functools

import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _capi, _samp
from ._samp import DTYPES as _DTYPES, ptr as _ptr

__all__ = ["deform_roi_pool_forward", "deform_roi_pool_backward", "DeformRoIPoolFunction", "deform_roi_pool", "DeformRoIPool",
           "DeformRoIPoolPack", "ModulatedDeformRoIPoolPack"]



def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _desc(input, rois, offset, output_size, spatial_scale, sampling_ratio, gamma, max_grid, accumulate=1, flags=0):
    if input.dtype not in _DTYPES or (offset is not None and offset.dtype not in _DTYPES):
        raise TypeError("droi: dtypes %s / %s are not float32, float16 or bfloat16" % (
            input.dtype, None if offset is None else offset.dtype))
    if input.dim() != 4 or rois.dim() != 2:
        raise ValueError("droi: input must be [B, H, W, C] and rois [R, 5], got %s and %s" % (tuple(input.shape), tuple(rois.shape)))
    ph, pw = _pair(output_size)
    d = _capi.MdconvDroiDesc()
    d.dtype = _DTYPES[input.dtype]
    d.coord_dtype = d.dtype if offset is None else _DTYPES[offset.dtype]
    d.batch, d.height, d.width, d.channels = (int(s) for s in input.shape)
    d.rois, d.pooled_h, d.pooled_w = int(rois.shape[0]), ph, pw
    d.sampling_ratio, d.max_grid = int(sampling_ratio), int(max_grid)
    d.spatial_scale, d.gamma = float(spatial_scale), float(gamma)
    d.with_offset = int(offset is not None)
    d.accumulate, d.flags = int(accumulate), int(flags)
    return d


def _check(d, input, rois, offset, **others):
    """Shapes, dtypes, devices and density of the tensors of a call; ``others`` have the shape of ``output``."""
    R, PH, PW = d.rois, d.pooled_h, d.pooled_w
    want = dict(input=tuple(input.shape), rois=(R, 5), offset=(R, 2, PH, PW))
    want.update({k: (R, PH, PW, d.channels) for k in others})
    tensors = dict(input=input, rois=rois, **others)
    if offset is not None:
        tensors["offset"] = offset
    for name, t in tensors.items():
        if tuple(t.shape) != want[name]:
            raise ValueError("droi: %s must be %s, got %s" % (name, want[name], tuple(t.shape)))
        like = torch.float32 if name == "rois" else offset.dtype if name == "offset" else input.dtype
        if t.dtype != like or t.device != input.device:
            raise ValueError("droi: %s is %s on %s; input is %s on %s (input, output and grad_output share one dtype, rois are "
                             "float32, offset has input's dtype or float32)" % (name, t.dtype, t.device, input.dtype, input.device))
        if not t.is_contiguous():
            raise ValueError("droi: %s must be dense and row-major (contiguous)" % name)
    if offset is not None and offset.dtype != input.dtype and offset.dtype != torch.float32:
        raise ValueError("droi: offset is %s, input is %s: it must have input's dtype or float32" % (offset.dtype, input.dtype))
    return (R, PH, PW, d.channels)


# the call itself (the seam the tests replace): workspace query, allocation, current stream, call, RuntimeError
_run = functools.partial(_samp.run, "mdconv_droi",
                         missing_msg="the loaded libmdconv_hip.so has no deformable RoI pooling (built before it existed)")


def deform_roi_pool_forward(input, rois, offset, output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1, max_grid=8,
                            output=None):
    """The forward entry point on dense channels-last CUDA buffers; allocates ``output [R, PH, PW, C]`` unless it is given.
    ``offset`` None: plain RoIAlign sampling."""
    if not input.is_cuda:
        raise NotImplementedError
    d = _desc(input, rois, offset, output_size, spatial_scale, sampling_ratio, gamma, max_grid)
    others = {} if output is None else dict(output=output)
    shape = _check(d, input, rois, offset, **others)
    # pointer classes (include/mdconv.h): input and output are "16-byte", rois and offset "element"
    _capi.require_aligned_result("droi", "output", output)
    input = _capi.aligned_input(input)
    if output is None:
        output = torch.empty(shape, dtype=input.dtype, device=input.device)
    _run("mdconv_droi_forward", d, False, [_ptr(input), _ptr(rois), _ptr(offset), _ptr(output)], input)
    return output


def deform_roi_pool_backward(input, rois, offset, grad_output, output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1,
                             max_grid=8, grads=None, need_grad_input=True, deterministic=None, accumulate=None):
    """The backward entry point.  ``grads`` = (grad_input | None, grad_offset | None): caller-allocated buffers the gradients
    are ADDED to; without it fresh tensors are written.  ``need_grad_input`` false: grad_input is neither computed nor
    allocated (``MDCONV_FLAG_NO_GRAD_INPUT``, no workspace) and None is returned there; grad_offset is None when ``offset``
    is.  ``deterministic`` None follows ``_capi.deterministic_mode()``.  ``accumulate`` false with ``grads``: the caller's
    buffers are overwritten instead.  Returns the two gradients in that order; ``rois`` have none."""
    if not input.is_cuda:
        raise NotImplementedError
    flags = _samp.backward_flags(deterministic, need_grad_input)
    d = _desc(input, rois, offset, output_size, spatial_scale, sampling_ratio, gamma, max_grid,
              accumulate=int(grads is not None if accumulate is None else bool(accumulate)), flags=flags)
    _check(d, input, rois, offset, grad_output=grad_output)
    # pointer classes (include/mdconv.h): input, grad_output and grad_input are "16-byte", rois, offset and grad_offset "element"
    if grads is not None and need_grad_input:
        _capi.require_aligned_result("droi", "grad_input", grads[0])
    input, grad_output = _capi.aligned_input(input), _capi.aligned_input(grad_output)
    if grads is None:
        grads = (torch.empty_like(input) if need_grad_input else None, None if offset is None else torch.empty_like(offset))
    gi, go = grads
    _samp.check_grads("droi", [(name, g, like) for name, g, like, needed in (
        ("grad_input", gi, input, need_grad_input), ("grad_offset", go, offset, offset is not None)) if needed])
    _run("mdconv_droi_backward", d, True,
         [_ptr(input), _ptr(rois), _ptr(offset), _ptr(grad_output), _ptr(gi if need_grad_input else None),
          _ptr(go if offset is not None else None)], input)
    return (gi if need_grad_input else None), (go if offset is not None else None)


class DeformRoIPoolFunction(Function):
    """``DeformRoIPoolFunction.apply(input, rois, offset, output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1)`` --
    the argument order of the published operator, on LOGICAL NCHW tensors: ``input [B, C, H, W]``, ``rois [R, 5]``,
    ``offset [R, 2, PH, PW]`` (or None, or an empty tensor: no offset) -> ``[R, C, PH, PW]``.  An eighth argument
    ``max_grid`` (default 8) bounds the adaptive grid.  The kernels are channels-last: a ``torch.channels_last`` input is used
    through a permute view WITHOUT a copy, a contiguous (NCHW) one pays one layout copy per call; the result is a permute
    view of the channels-last buffer (a ``torch.channels_last`` tensor), and so is the gradient of ``input``.  Under
    ``torch.autocast`` ``input`` runs in the autocast dtype; ``rois`` are cast to fp32; an fp32 ``offset`` stays fp32 (the
    mixed call), any other runs in input's dtype.  ``grad_input`` is left out when ``input`` needs no gradient.  The gradients
    go back in the dtypes the caller's tensors have."""

    @staticmethod
    def forward(ctx, input, rois, offset, output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1, max_grid=8):
        if not input.is_cuda:
            raise NotImplementedError
        if offset is not None and offset.numel() == 0:
            offset = None
        ctx.in_dtypes = (input.dtype, None if offset is None else offset.dtype)
        ctx.has_offset = offset is not None
        if torch.is_autocast_enabled("cuda"):
            input = input.to(torch.get_autocast_dtype("cuda"))
        ctx.args = (_pair(output_size), float(spatial_scale), int(sampling_ratio), float(gamma), int(max_grid))
        cl = input.permute(0, 2, 3, 1).contiguous()   # a view of a channels_last input, one copy of a contiguous one
        rois = rois.to(torch.float32).contiguous()
        if offset is not None:
            offset = offset.to(input.dtype if offset.dtype != torch.float32 else torch.float32).contiguous()
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(cl, rois, *(() if offset is None else (offset,)))
        out = deform_roi_pool_forward(cl, rois, offset, *ctx.args)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        if not grad_output.is_cuda:
            raise NotImplementedError
        cl, rois = ctx.saved_tensors[:2]
        offset = ctx.saved_tensors[2] if ctx.has_offset else None
        need_gi = bool(ctx.needs_input_grad[0])
        need_go = offset is not None and bool(ctx.needs_input_grad[2])
        gi = go = None
        if need_gi or need_go:
            g = grad_output.to(cl.dtype).permute(0, 2, 3, 1).contiguous()
            # selective backward: grad_input is neither computed nor allocated when `input` needs no gradient
            gi, go = deform_roi_pool_backward(cl, rois, offset, g, *ctx.args, need_grad_input=need_gi)
        back = _samp.back
        di, do = ctx.in_dtypes
        gi = None if gi is None else back(gi, di).permute(0, 3, 1, 2)
        return gi, None, (back(go, do) if need_go else None), None, None, None, None, None


def deform_roi_pool(input, rois, offset, output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1, max_grid=8):
    """Functional form of ``DeformRoIPoolFunction``; ``max_grid`` (1..16) bounds the adaptive grid of ``sampling_ratio=0``:
    a RoI whose bins are taller or wider than ``max_grid`` pixels of the feature map is sampled ``max_grid`` times per axis."""
    return DeformRoIPoolFunction.apply(input, rois, offset, output_size, spatial_scale, sampling_ratio, gamma, max_grid)


class DeformRoIPool(nn.Module):
    """``DeformRoIPool(output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1)``; ``forward(input, rois, offset=None)``
    on logical NCHW tensors.  Constructor and attribute names follow the published module from memory: UNPINNED
    (INTEGRATION.md)."""

    def __init__(self, output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1, max_grid=8):
        super().__init__()
        self.output_size = _pair(output_size)
        self.spatial_scale, self.sampling_ratio, self.gamma, self.max_grid = float(spatial_scale), int(sampling_ratio), float(gamma), int(max_grid)

    def _pool(self, input, rois, offset):
        return deform_roi_pool(input, rois, offset, self.output_size, self.spatial_scale, self.sampling_ratio, self.gamma,
                               self.max_grid)

    def forward(self, input, rois, offset=None):
        return self._pool(input, rois, offset)

    def extra_repr(self):
        return "output_size=%s, spatial_scale=%g, sampling_ratio=%d, gamma=%g" % (
            self.output_size, self.spatial_scale, self.sampling_ratio, self.gamma)


class DeformRoIPoolPack(DeformRoIPool):
    """Deformable RoI pooling that predicts its own offsets: pool without offset, ``offset_fc`` (three linears with ReLU,
    the last zero-initialised) on the NCHW-order flatten of that result, then pool again with the offsets.  Parameter names
    (``offset_fc.0 / .2 / .4``) follow the published module from memory: UNPINNED."""

    def __init__(self, output_size, output_channels, deform_fc_channels=1024, spatial_scale=1.0, sampling_ratio=0, gamma=0.1,
                 max_grid=8):
        super().__init__(output_size, spatial_scale, sampling_ratio, gamma, max_grid)
        self.output_channels, self.deform_fc_channels = output_channels, deform_fc_channels
        ph, pw = self.output_size
        self.offset_fc = nn.Sequential(
            nn.Linear(ph * pw * output_channels, deform_fc_channels), nn.ReLU(inplace=True),
            nn.Linear(deform_fc_channels, deform_fc_channels), nn.ReLU(inplace=True),
            nn.Linear(deform_fc_channels, ph * pw * 2))
        nn.init.zeros_(self.offset_fc[-1].weight)
        nn.init.zeros_(self.offset_fc[-1].bias)

    def _offset(self, x):
        ph, pw = self.output_size
        return self.offset_fc(x.reshape(x.shape[0], -1)).view(x.shape[0], 2, ph, pw)

    def forward(self, input, rois):
        if input.shape[1] != self.output_channels:
            raise ValueError("input has %d channels, the module was built for %d" % (input.shape[1], self.output_channels))
        x = self._pool(input, rois, None)
        return self._pool(input, rois, self._offset(x))


class ModulatedDeformRoIPoolPack(DeformRoIPoolPack):
    """``DeformRoIPoolPack`` plus ``mask_fc`` (two linears with a ReLU between, the last zero-initialised, then a sigmoid) on
    the same flatten, multiplied into the pooled result per bin.  Parameter names (``offset_fc``, ``mask_fc.0 / .2``) follow
    the published module from memory: UNPINNED."""

    def __init__(self, output_size, output_channels, deform_fc_channels=1024, spatial_scale=1.0, sampling_ratio=0, gamma=0.1,
                 max_grid=8):
        super().__init__(output_size, output_channels, deform_fc_channels, spatial_scale, sampling_ratio, gamma, max_grid)
        ph, pw = self.output_size
        self.mask_fc = nn.Sequential(
            nn.Linear(ph * pw * output_channels, deform_fc_channels), nn.ReLU(inplace=True),
            nn.Linear(deform_fc_channels, ph * pw), nn.Sigmoid())
        nn.init.zeros_(self.mask_fc[2].weight)
        nn.init.zeros_(self.mask_fc[2].bias)

    def forward(self, input, rois):
        if input.shape[1] != self.output_channels:
            raise ValueError("input has %d channels, the module was built for %d" % (input.shape[1], self.output_channels))
        ph, pw = self.output_size
        x = self._pool(input, rois, None)
        pooled = self._pool(input, rois, self._offset(x))
        mask = self.mask_fc(x.reshape(x.shape[0], -1)).view(x.shape[0], 1, ph, pw)
        return pooled * mask
