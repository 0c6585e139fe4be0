"""Packed deformable attention with a point count per level on the MI355X-native backend: the tap layout of the real-time
DETR line (RT-DETRv2's ``num_points_list``; D-FINE and DEIM ship (3, 6, 3)) with ONE packed tensor per (query, head) -- the
sampling locations and the attention LOGITS, as the linear layers produced them -- and the softmax over all K taps inside
the operator (include/mdconv_fdap.h; INTEGRATION.md has the contract and what is unpinned).

    flash_deform_attn_points_forward / flash_deform_attn_points_backward   the entry points on dense CUDA tensors
    FlashDeformAttnPointsFunction   autograd.Function over mdconv_fdap_forward / mdconv_fdap_backward
    flash_deform_attn_points        the functional form
    MSDeformableAttentionFused      nn.Module: ``MSDeformableAttention``'s block (same parameters, same checkpoints) around
                                    this operator
    pack_loc_attn_points / unpack_loc_attn_points   the packed layout from and to ``MSDeformableAttention``-style tensors

``value [N, S, M, D]`` (the levels concatenated), ``sampling_loc_attn [N, Lq, M, 3K]`` (per (query, head): (x, y) of tap
0 .. K-1, normalised, then the K logits; K = ``sum(num_points_list)``, the taps level-major) -> ``output [N, Lq, M*D]``.
``value`` is fp32 / fp16 / bf16; the packed tensor has its dtype or is fp32.  With equal counts the operator is
``flash_deform_attn`` on the same memory.  CPU tensors raise ``NotImplementedError``: there is no CPU or PyTorch fallback.
"""
import functools

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _capi, _samp
from ._samp import DTYPES as _DTYPES, ptr as _ptr
from .msda import _shapes
from .msdap import MSDeformableAttention, _points

__all__ = ["flash_deform_attn_points_forward", "flash_deform_attn_points_backward", "FlashDeformAttnPointsFunction",
           "flash_deform_attn_points", "MSDeformableAttentionFused", "pack_loc_attn_points", "unpack_loc_attn_points"]


def pack_loc_attn_points(sampling_locations, attention_logits):
    """``[N, Lq, M, K, 2]`` locations and ``[N, Lq, M, K]`` logits -> the packed ``[N, Lq, M, 3K]`` tensor: one ``cat``."""
    N, Lq, M = sampling_locations.shape[:3]
    return torch.cat([sampling_locations.reshape(N, Lq, M, -1), attention_logits.reshape(N, Lq, M, -1)], -1)


def unpack_loc_attn_points(sampling_loc_attn, num_points_list):
    """The packed tensor (or its gradient) -> (``[N, Lq, M, K, 2]``, ``[N, Lq, M, K]``): two views."""
    N, Lq, M, K3 = sampling_loc_attn.shape
    K = sum(int(p) for p in num_points_list)
    if K3 != 3 * K:
        raise ValueError("fdap: a packed row of num_points_list %s has %d elements, got %d" % (
            tuple(num_points_list), 3 * K, K3))
    return sampling_loc_attn[..., :2 * K].unflatten(-1, (K, 2)), sampling_loc_attn[..., 2 * K:]


def _desc(value, loc_attn, shapes, points, accumulate=1, flags=0):
    if value.dtype not in _DTYPES or loc_attn.dtype not in _DTYPES:
        raise TypeError("fdap: dtypes %s / %s are not float32, float16 or bfloat16" % (value.dtype, loc_attn.dtype))
    if value.dim() != 4 or loc_attn.dim() != 4:
        raise ValueError("fdap: value must be [N, S, M, D] and sampling_loc_attn [N, Lq, M, 3*K], got %s and %s" % (
            tuple(value.shape), tuple(loc_attn.shape)))
    d = _capi.MdconvFdapDesc()
    d.dtype, d.coord_dtype = _DTYPES[value.dtype], _DTYPES[loc_attn.dtype]
    d.batch, d.heads, d.head_channels = int(value.shape[0]), int(value.shape[2]), int(value.shape[3])
    d.queries, d.levels = int(loc_attn.shape[1]), len(shapes)
    for l, ((h, w), p) in enumerate(zip(shapes, points)):
        d.level_sz[l][0], d.level_sz[l][1], d.points[l] = h, w, p
    d.accumulate, d.flags = int(accumulate), int(flags)
    return d


def _check(d, shapes, points, value, loc_attn, **others):
    """Shapes, dtypes, devices and density of the tensors of a call; ``others`` have the shape of ``output``."""
    N, M, D, Lq, K = d.batch, d.heads, d.head_channels, d.queries, sum(points)
    S = sum(h * w for h, w in shapes)
    if loc_attn.shape[3] != 3 * K:
        raise ValueError("fdap: sampling_loc_attn has %d elements per head, num_points_list %s asks for 3 * %d" % (
            loc_attn.shape[3], points, K))
    want = dict(value=(N, S, M, D), sampling_loc_attn=(N, Lq, M, 3 * K))
    want.update({k: (N, Lq, M * D) for k in others})
    tensors = dict(value=value, sampling_loc_attn=loc_attn, **others)
    for name, t in tensors.items():
        if tuple(t.shape) != want[name]:
            raise ValueError("fdap: %s must be %s, got %s" % (name, want[name], tuple(t.shape)))
        like = loc_attn if name == "sampling_loc_attn" else value
        if t.dtype != like.dtype or t.device != value.device:
            raise ValueError("fdap: %s is %s on %s; value is %s on %s and sampling_loc_attn is %s (value, output and "
                             "grad_output share one dtype, the packed tensor has it too or is float32)" % (
                                 name, t.dtype, t.device, value.dtype, value.device, loc_attn.dtype))
        if not t.is_contiguous():
            raise ValueError("fdap: %s must be dense and row-major (contiguous)" % name)
    if loc_attn.dtype != value.dtype and loc_attn.dtype != torch.float32:
        raise ValueError("fdap: sampling_loc_attn is %s, value is %s: it must have value's dtype or float32" % (
            loc_attn.dtype, value.dtype))
    return (N, Lq, M * D)


# the call itself (the seam the tests replace): workspace query, allocation, current stream, call, RuntimeError
_run = functools.partial(_samp.run, "mdconv_fdap")


def flash_deform_attn_points_forward(value, spatial_shapes, num_points_list, sampling_loc_attn, output=None):
    """The forward entry point on dense CUDA tensors; allocates ``output`` unless it is given."""
    shapes = _shapes(spatial_shapes)
    points = _points(num_points_list, len(shapes))
    d = _desc(value, sampling_loc_attn, shapes, points)
    others = {} if output is None else dict(output=output)
    shape = _check(d, shapes, points, value, sampling_loc_attn, **others)
    if not value.is_cuda:
        raise NotImplementedError
    # pointer classes (include/mdconv_fdap.h): value and output are "16-byte", sampling_loc_attn "element"
    _capi.require_aligned_result("fdap", "output", output)
    value = _capi.aligned_input(value)
    if output is None:
        output = torch.empty(shape, dtype=value.dtype, device=value.device)
    _run("mdconv_fdap_forward", d, False, [_ptr(value), _ptr(sampling_loc_attn), _ptr(output)], value)
    return output


def flash_deform_attn_points_backward(value, spatial_shapes, num_points_list, sampling_loc_attn, grad_output, grads=None,
                                      need_grad_value=True, deterministic=None, accumulate=None):
    """The backward entry point.  ``grads`` = (grad_value | None, grad_sampling_loc_attn): caller-allocated buffers the
    gradients are ADDED to; without it fresh tensors are written.  ``need_grad_value`` false: grad_value is neither computed
    nor allocated (``MDCONV_FLAG_NO_GRAD_INPUT``) and None is returned there.  ``deterministic`` None follows
    ``_capi.deterministic_mode()``.  ``accumulate`` false with ``grads``: the caller's buffers are overwritten instead.
    Takes no ``output``.  Returns the two gradients in that order."""
    shapes = _shapes(spatial_shapes)
    points = _points(num_points_list, len(shapes))
    flags = _samp.backward_flags(deterministic, need_grad_value)
    d = _desc(value, sampling_loc_attn, shapes, points,
              accumulate=int(grads is not None if accumulate is None else bool(accumulate)), flags=flags)
    _check(d, shapes, points, value, sampling_loc_attn, grad_output=grad_output)
    if not value.is_cuda:
        raise NotImplementedError
    # pointer classes (include/mdconv_fdap.h): value, grad_output and grad_value are "16-byte", the packed tensor and its
    # gradient "element"
    if grads is not None and need_grad_value:
        _capi.require_aligned_result("fdap", "grad_value", grads[0])
    value, grad_output = _capi.aligned_input(value), _capi.aligned_input(grad_output)
    if grads is None:
        grads = (torch.empty_like(value) if need_grad_value else None, torch.empty_like(sampling_loc_attn))
    gv, gla = grads
    _samp.check_grads("fdap", (("grad_value", gv, value), ("grad_sampling_loc_attn", gla, sampling_loc_attn)),
                      may_be_none=() if need_grad_value else ("grad_value",))
    _run("mdconv_fdap_backward", d, True,
         [_ptr(value), _ptr(sampling_loc_attn), _ptr(grad_output), _ptr(gv if need_grad_value else None), _ptr(gla)], value)
    return (gv if need_grad_value else None), gla


class FlashDeformAttnPointsFunction(Function):
    """``FlashDeformAttnPointsFunction.apply(value, spatial_shapes, num_points_list, sampling_loc_attn)``.
    ``spatial_shapes`` (rows of (H, W)) and ``num_points_list`` are host data: sequences, or tensors -- a CUDA tensor costs a
    ``.tolist()`` synchronisation per call and cannot be read during graph capture.  Under ``torch.autocast`` ``value`` runs
    in the autocast dtype; a packed tensor that is fp32 stays fp32 (the mixed call), another runs in value's dtype.  The
    gradients go back in the dtypes the caller's tensors have."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, num_points_list, sampling_loc_attn):
        if not value.is_cuda:
            raise NotImplementedError
        shapes = _shapes(spatial_shapes)
        points = _points(num_points_list, len(shapes))
        ctx.shapes, ctx.points = shapes, points
        ctx.in_dtypes = (value.dtype, sampling_loc_attn.dtype)
        if torch.is_autocast_enabled("cuda"):
            value = value.to(torch.get_autocast_dtype("cuda"))
        cdt = _samp.coord_dtype(value.dtype, sampling_loc_attn.dtype)
        value = value.contiguous()
        sampling_loc_attn = sampling_loc_attn.to(cdt).contiguous()
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(value, sampling_loc_attn)   # (no output: the backward does not take it)
        return flash_deform_attn_points_forward(value, shapes, points, sampling_loc_attn)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        if not grad_output.is_cuda:
            raise NotImplementedError
        value, loc_attn = ctx.saved_tensors
        grad_output = grad_output.to(value.dtype).contiguous()
        # selective backward: grad_value is neither computed nor allocated when `value` needs no gradient
        gv, gla = flash_deform_attn_points_backward(value, ctx.shapes, ctx.points, loc_attn, grad_output,
                                                    need_grad_value=bool(ctx.needs_input_grad[0]))
        back = _samp.back
        dv, dla = ctx.in_dtypes
        return back(gv, dv), None, None, (back(gla, dla) if ctx.needs_input_grad[3] else None)


def flash_deform_attn_points(value, spatial_shapes, num_points_list, sampling_loc_attn):
    """Functional form of ``FlashDeformAttnPointsFunction``."""
    return FlashDeformAttnPointsFunction.apply(value, spatial_shapes, num_points_list, sampling_loc_attn)


class MSDeformableAttentionFused(MSDeformableAttention):
    """``MSDeformableAttention`` on the packed operator: the same constructor, parameter names, buffer and initialisation,
    so the same checkpoints load, and the same ``forward`` arguments.  The block builds the packed tensor with one ``cat`` of
    the locations and the RAW logits of the ``attention_weights`` linear -- there is no framework softmax, forward or
    backward -- and under autocast that tensor is fp32 (the mixed call)."""

    def __init__(self, embed_dim=256, num_heads=8, num_levels=4, num_points=4, offset_scale=0.5, method="default"):
        super().__init__(embed_dim, num_heads, num_levels, num_points, offset_scale, method)
        self._core = flash_deform_attn_points

    def forward(self, query, reference_points, value, value_spatial_shapes, value_mask=None):
        N, Lq, _ = query.shape
        shapes, value = self._values(value, value_spatial_shapes, value_mask)
        logits = self.attention_weights(query).float().view(N, Lq, self.num_heads, sum(self.num_points_list))
        locations = self._locations(query, reference_points, shapes)
        # (the locations and the logits are fp32 under autocast, like the parent's: the core then takes fp32 coordinates)
        out = self._core(value, shapes, self.num_points_list, pack_loc_attn_points(locations, logits))
        return self.output_proj(out)
