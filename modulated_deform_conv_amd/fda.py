"""Packed deformable attention on the MI355X-native backend: multi-scale deformable attention that takes ONE packed tensor
per (query, head) -- the sampling locations and the attention LOGITS, as the linear layers produced them -- and runs the
softmax over the L*P taps inside the operator (include/mdconv.h, "Packed deformable attention"; INTEGRATION.md has the
contract and what is unpinned).

    flash_deform_attn_forward / flash_deform_attn_backward   the entry points on dense CUDA tensors
    FlashDeformAttnFunction   autograd.Function over mdconv_fda_forward / mdconv_fda_backward
    flash_deform_attn         the functional form
    FlashDeformAttn           nn.Module: ``MSDeformAttn``'s block (same parameters, same checkpoints) around this operator
    pack_loc_attn / unpack_loc_attn   the packed layout from and to ``MSDeformAttn``-style tensors

``value [N, S, M, D]`` (the levels concatenated), ``sampling_loc_attn [N, Lq, M, 3*L*P]`` (per (query, head): (x, y) of
tap 0 .. L*P-1, normalised, then the L*P logits; tap = l*P + p) -> ``output [N, Lq, M*D]``.  ``value`` is fp32 / fp16 / bf16;
the packed tensor has its dtype or is fp32.  CPU tensors raise ``NotImplementedError``: there is no CPU or PyTorch fallback.
"""
import functools

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _capi, _samp
from ._samp import DTYPES as _DTYPES, ptr as _ptr
from .msda import MSDeformAttn, _check_starts, _shapes

__all__ = ["flash_deform_attn_forward", "flash_deform_attn_backward", "FlashDeformAttnFunction", "flash_deform_attn",
           "FlashDeformAttn", "pack_loc_attn", "unpack_loc_attn"]



def pack_loc_attn(sampling_locations, attention_logits):
    """``[N, Lq, M, L, P, 2]`` locations and ``[N, Lq, M, L, P]`` (or ``[N, Lq, M, L*P]``) logits -> the packed
    ``[N, Lq, M, 3*L*P]`` tensor: one ``cat``."""
    N, Lq, M = sampling_locations.shape[:3]
    return torch.cat([sampling_locations.reshape(N, Lq, M, -1), attention_logits.reshape(N, Lq, M, -1)], -1)


def unpack_loc_attn(sampling_loc_attn, n_levels, n_points):
    """The packed tensor (or its gradient) -> (``[N, Lq, M, L, P, 2]``, ``[N, Lq, M, L, P]``): two views."""
    N, Lq, M, K3 = sampling_loc_attn.shape
    K = n_levels * n_points
    if K3 != 3 * K:
        raise ValueError("fda: a packed row of %d levels x %d points has %d elements, got %d" % (n_levels, n_points, 3 * K, K3))
    return (sampling_loc_attn[..., :2 * K].reshape(N, Lq, M, n_levels, n_points, 2),
            sampling_loc_attn[..., 2 * K:].reshape(N, Lq, M, n_levels, n_points))


def _desc(value, loc_attn, shapes, points, accumulate=1, flags=0):
    if value.dtype not in _DTYPES or loc_attn.dtype not in _DTYPES:
        raise TypeError("fda: dtypes %s / %s are not float32, float16 or bfloat16" % (value.dtype, loc_attn.dtype))
    if value.dim() != 4 or loc_attn.dim() != 4:
        raise ValueError("fda: value must be [N, S, M, D] and sampling_loc_attn [N, Lq, M, 3*L*P], got %s and %s" % (
            tuple(value.shape), tuple(loc_attn.shape)))
    if int(points) < 1:
        raise ValueError("fda: points per level must be positive, got %r" % (points,))
    d = _capi.MdconvFdaDesc()
    d.dtype, d.coord_dtype = _DTYPES[value.dtype], _DTYPES[loc_attn.dtype]
    d.batch, d.heads, d.head_channels = int(value.shape[0]), int(value.shape[2]), int(value.shape[3])
    d.queries, d.levels, d.points = int(loc_attn.shape[1]), len(shapes), int(points)
    for l, (h, w) in enumerate(shapes):
        d.level_sz[l][0], d.level_sz[l][1] = h, w
    d.accumulate, d.flags = int(accumulate), int(flags)
    return d


def _check(d, shapes, value, loc_attn, **others):
    """Shapes, dtypes, devices and density of the tensors of a call; ``others`` have the shape of ``output``."""
    N, M, D, Lq, L, P = d.batch, d.heads, d.head_channels, d.queries, d.levels, d.points
    S = sum(h * w for h, w in shapes)
    want = dict(value=(N, S, M, D), sampling_loc_attn=(N, Lq, M, 3 * L * P))
    want.update({k: (N, Lq, M * D) for k in others})
    tensors = dict(value=value, sampling_loc_attn=loc_attn, **others)
    for name, t in tensors.items():
        if tuple(t.shape) != want[name]:
            raise ValueError("fda: %s must be %s, got %s" % (name, want[name], tuple(t.shape)))
        like = loc_attn if name == "sampling_loc_attn" else value
        if t.dtype != like.dtype or t.device != value.device:
            raise ValueError("fda: %s is %s on %s; value is %s on %s and sampling_loc_attn is %s (value, output and "
                             "grad_output share one dtype, the packed tensor has it too or is float32)" % (
                                 name, t.dtype, t.device, value.dtype, value.device, loc_attn.dtype))
        if not t.is_contiguous():
            raise ValueError("fda: %s must be dense and row-major (contiguous)" % name)
    if loc_attn.dtype != value.dtype and loc_attn.dtype != torch.float32:
        raise ValueError("fda: sampling_loc_attn is %s, value is %s: it must have value's dtype or float32" % (
            loc_attn.dtype, value.dtype))
    return (N, Lq, M * D)


# the call itself (the seam the tests replace): workspace query, allocation, current stream, call, RuntimeError
_run = functools.partial(_samp.run, "mdconv_fda")


def flash_deform_attn_forward(value, spatial_shapes, sampling_loc_attn, points, output=None):
    """The forward entry point on dense CUDA tensors; ``points`` is P, the points per level.  Allocates ``output`` unless
    it is given."""
    if not value.is_cuda:
        raise NotImplementedError
    shapes = _shapes(spatial_shapes)
    d = _desc(value, sampling_loc_attn, shapes, points)
    others = {} if output is None else dict(output=output)
    shape = _check(d, shapes, value, sampling_loc_attn, **others)
    # pointer classes (include/mdconv.h): value and output are "16-byte", sampling_loc_attn "element"
    _capi.require_aligned_result("fda", "output", output)
    value = _capi.aligned_input(value)
    if output is None:
        output = torch.empty(shape, dtype=value.dtype, device=value.device)
    _run("mdconv_fda_forward", d, False, [_ptr(value), _ptr(sampling_loc_attn), _ptr(output)], value)
    return output


def flash_deform_attn_backward(value, spatial_shapes, sampling_loc_attn, points, grad_output, grads=None,
                               need_grad_value=True, deterministic=None, accumulate=True):
    """The backward entry point.  ``grads`` = (grad_value | None, grad_sampling_loc_attn): caller-allocated buffers the
    gradients are ADDED to (``accumulate`` false: written to, whatever the buffers hold); without it fresh tensors are
    written.  ``need_grad_value`` false: grad_value is neither computed nor allocated (``MDCONV_FLAG_NO_GRAD_INPUT``) and
    None is returned there.  ``deterministic`` None follows ``_capi.deterministic_mode()``.  Takes no ``output``.  Returns
    the two gradients in that order."""
    if not value.is_cuda:
        raise NotImplementedError
    shapes = _shapes(spatial_shapes)
    flags = _samp.backward_flags(deterministic, need_grad_value)
    d = _desc(value, sampling_loc_attn, shapes, points, accumulate=int(grads is not None and bool(accumulate)), flags=flags)
    _check(d, shapes, value, sampling_loc_attn, grad_output=grad_output)
    # pointer classes (include/mdconv.h): value, grad_output and grad_value are "16-byte", sampling_loc_attn and its gradient "element"
    if grads is not None and need_grad_value:
        _capi.require_aligned_result("fda", "grad_value", grads[0])
    value, grad_output = _capi.aligned_input(value), _capi.aligned_input(grad_output)
    if grads is None:
        grads = (torch.empty_like(value) if need_grad_value else None, torch.empty_like(sampling_loc_attn))
    gv, gla = grads
    _samp.check_grads("fda", (("grad_value", gv, value), ("grad_sampling_loc_attn", gla, sampling_loc_attn)),
                      may_be_none=() if need_grad_value else ("grad_value",))
    _run("mdconv_fda_backward", d, True,
         [_ptr(value), _ptr(sampling_loc_attn), _ptr(grad_output), _ptr(gv if need_grad_value else None), _ptr(gla)], value)
    return (gv if need_grad_value else None), gla


class FlashDeformAttnFunction(Function):
    """``FlashDeformAttnFunction.apply(value, spatial_shapes, level_start_index, sampling_loc_attn, im2col_step, K)`` --
    the argument order of the published operator, where ``K`` is the POINTS PER LEVEL (P); ``im2col_step`` must be a
    positive integer and is otherwise unused.  ``spatial_shapes`` is a sequence of (H, W) or a tensor; a CUDA tensor costs a
    ``.tolist()`` synchronisation per call and cannot be read during graph capture, so pass host data there.
    ``level_start_index`` is checked against the cumulative sums when it is host data and ignored otherwise.  Under
    ``torch.autocast`` ``value`` runs in the autocast dtype; a packed tensor that is fp32 stays fp32 (the mixed call), another
    runs in value's dtype.  The gradients go back in the dtypes the caller's tensors have."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, level_start_index, sampling_loc_attn, im2col_step=64, K=8):
        if not value.is_cuda:
            raise NotImplementedError
        if isinstance(im2col_step, bool) or not isinstance(im2col_step, int) or im2col_step < 1:
            raise ValueError("fda: im2col_step must be a positive integer, got %r" % (im2col_step,))
        shapes = _shapes(spatial_shapes)
        _check_starts(shapes, level_start_index)
        ctx.shapes, ctx.points = shapes, int(K)
        ctx.in_dtypes = (value.dtype, sampling_loc_attn.dtype)
        if torch.is_autocast_enabled("cuda"):
            value = value.to(torch.get_autocast_dtype("cuda"))
        cdt = _samp.coord_dtype(value.dtype, sampling_loc_attn.dtype)
        value = value.contiguous()
        sampling_loc_attn = sampling_loc_attn.to(cdt).contiguous()
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(value, sampling_loc_attn)   # (no output: the backward does not take it)
        return flash_deform_attn_forward(value, shapes, sampling_loc_attn, ctx.points)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        if not grad_output.is_cuda:
            raise NotImplementedError
        value, loc_attn = ctx.saved_tensors
        grad_output = grad_output.to(value.dtype).contiguous()
        # selective backward: grad_value is neither computed nor allocated when `value` needs no gradient
        gv, gla = flash_deform_attn_backward(value, ctx.shapes, loc_attn, ctx.points, grad_output,
                                             need_grad_value=bool(ctx.needs_input_grad[0]))
        back = _samp.back
        dv, dla = ctx.in_dtypes
        return back(gv, dv), None, None, (back(gla, dla) if ctx.needs_input_grad[3] else None), None, None


def flash_deform_attn(value, spatial_shapes, sampling_loc_attn, points, level_start_index=None):
    """Functional form of ``FlashDeformAttnFunction``; ``points`` is P, the points per level."""
    return FlashDeformAttnFunction.apply(value, spatial_shapes, level_start_index, sampling_loc_attn, 64, points)


class FlashDeformAttn(MSDeformAttn):
    """``MSDeformAttn`` on the packed operator: the same constructor, parameter names and initialisation, so the same
    checkpoints load, and the same ``forward`` arguments.  The block builds the packed tensor with one ``cat`` of the
    locations and the RAW logits of the ``attention_weights`` linear -- there is no framework softmax, forward or backward --
    and under autocast that tensor is fp32 (the mixed call).  Written from memory of the published block and UNPINNED
    against it."""

    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4):
        super().__init__(d_model, n_levels, n_heads, n_points)
        self._core = flash_deform_attn

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                input_padding_mask=None):
        N, Lq, _ = query.shape
        S = input_flatten.shape[1]
        shapes = _shapes(input_spatial_shapes)
        if len(shapes) != self.n_levels or sum(h * w for h, w in shapes) != S:
            raise ValueError("input_spatial_shapes %s does not describe %d levels of %d rows" % (shapes, self.n_levels, S))
        M, L, P = self.n_heads, self.n_levels, self.n_points
        value = self.value_proj(input_flatten)
        if input_padding_mask is not None:
            value = value.masked_fill(input_padding_mask[..., None], 0.0)
        value = value.view(N, S, M, self.d_model // M)
        offsets = self.sampling_offsets(query).float().view(N, Lq, M, L, P, 2)
        logits = self.attention_weights(query).float().view(N, Lq, M, L * P)
        ref = reference_points.float()
        if ref.shape[-1] == 2:
            wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32, device=query.device)   # (x, y) order
            locations = ref[:, :, None, :, None, :] + offsets / wh[None, None, None, :, None, :]
        elif ref.shape[-1] == 4:
            locations = ref[:, :, None, :, None, :2] + offsets / P * ref[:, :, None, :, None, 2:] * 0.5
        else:
            raise ValueError("the last dimension of reference_points must be 2 or 4, but is %d" % ref.shape[-1])
        # (the locations and the logits are fp32 under autocast, like MSDeformAttn's: the core then takes fp32 coordinates)
        out = self._core(value, shapes, pack_loc_attn(locations, logits), P, input_level_start_index)
        return self.output_proj(out)
