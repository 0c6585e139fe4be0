"""Multi-scale deformable attention on the MI355X-native backend: the sampling operator of Deformable-DETR-style
attention on channels-last tensors (include/mdconv.h, "Multi-scale deformable attention"; INTEGRATION.md has the contract
and what is unpinned).

    ms_deform_attn_forward / ms_deform_attn_backward   the entry points on dense CUDA tensors
    MSDeformAttnFunction   autograd.Function over mdconv_msda_forward / mdconv_msda_backward
    ms_deform_attn         the functional form
    MSDeformAttn           nn.Module: the attention block around the operator, composed from framework operators

``value [N, S, M, D]`` (the levels concatenated), ``sampling_locations [N, Lq, M, L, P, 2]`` ((x, y), normalised),
``attention_weights [N, Lq, M, L, P]`` -> ``output [N, Lq, M*D]``.  ``value`` is fp32 / fp16 / bf16; the two coordinate
tensors have its dtype or are fp32.  CPU tensors raise ``NotImplementedError``: there is no CPU or PyTorch fallback.
"""
import functools
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _capi, _samp
from ._samp import DTYPES as _DTYPES, ptr as _ptr

__all__ = ["ms_deform_attn_forward", "ms_deform_attn_backward", "MSDeformAttnFunction", "ms_deform_attn", "MSDeformAttn"]



def _shapes(spatial_shapes):
    """``spatial_shapes`` as a tuple of (H, W) ints.  A tensor is read with ``.tolist()``: for a CUDA tensor that is a
    host synchronisation (and impossible during graph capture) -- pass host data to avoid it."""
    if isinstance(spatial_shapes, torch.Tensor):
        spatial_shapes = spatial_shapes.tolist()
    shapes = tuple((int(h), int(w)) for h, w in spatial_shapes)
    if not 1 <= len(shapes) <= _capi.MSDA_MAX_LEVELS:
        raise ValueError("msda: 1..%d levels, got %d" % (_capi.MSDA_MAX_LEVELS, len(shapes)))
    return shapes


def _check_starts(shapes, level_start_index):
    """``level_start_index`` is not an input of the operator (the starts are the cumulative sums); host data is checked
    against them, a CUDA tensor is ignored rather than synchronised on."""
    if level_start_index is None or (isinstance(level_start_index, torch.Tensor) and level_start_index.is_cuda):
        return
    got = [int(v) for v in (level_start_index.tolist() if isinstance(level_start_index, torch.Tensor) else level_start_index)]
    want, _ = _samp.level_starts(shapes)
    if got != want:
        raise ValueError("msda: level_start_index %s is not the cumulative sum %s of spatial_shapes" % (got, want))


def _desc(value, loc, shapes, accumulate=1, flags=0):
    if value.dtype not in _DTYPES or loc.dtype not in _DTYPES:
        raise TypeError("msda: dtypes %s / %s are not float32, float16 or bfloat16" % (value.dtype, loc.dtype))
    if value.dim() != 4 or loc.dim() != 6:
        raise ValueError("msda: value must be [N, S, M, D] and sampling_locations [N, Lq, M, L, P, 2], got %s and %s" % (
            tuple(value.shape), tuple(loc.shape)))
    d = _capi.MdconvMsdaDesc()
    d.dtype, d.coord_dtype = _DTYPES[value.dtype], _DTYPES[loc.dtype]
    d.batch, d.heads, d.head_channels = int(value.shape[0]), int(value.shape[2]), int(value.shape[3])
    d.queries, d.levels, d.points = int(loc.shape[1]), len(shapes), int(loc.shape[4])
    for l, (h, w) in enumerate(shapes):
        d.level_sz[l][0], d.level_sz[l][1] = h, w
    d.accumulate, d.flags = int(accumulate), int(flags)
    return d


def _check(d, shapes, value, loc, attn, **others):
    """Shapes, dtypes, devices and density of the tensors of a call; ``others`` have the shape of ``output``."""
    N, M, D, Lq, L, P = d.batch, d.heads, d.head_channels, d.queries, d.levels, d.points
    S = sum(h * w for h, w in shapes)
    want = dict(value=(N, S, M, D), sampling_locations=(N, Lq, M, L, P, 2), attention_weights=(N, Lq, M, L, P))
    want.update({k: (N, Lq, M * D) for k in others})
    tensors = dict(value=value, sampling_locations=loc, attention_weights=attn, **others)
    for name, t in tensors.items():
        if tuple(t.shape) != want[name]:
            raise ValueError("msda: %s must be %s, got %s" % (name, want[name], tuple(t.shape)))
        like = loc if name in ("sampling_locations", "attention_weights") else value
        if t.dtype != like.dtype or t.device != value.device:
            raise ValueError("msda: %s is %s on %s; value is %s on %s and the coordinate tensors are %s (value, output and "
                             "grad_output share one dtype, the two coordinate tensors another: the same, or float32)" % (
                                 name, t.dtype, t.device, value.dtype, value.device, loc.dtype))
        if not t.is_contiguous():
            raise ValueError("msda: %s must be dense and row-major (contiguous)" % name)
    if loc.dtype != value.dtype and loc.dtype != torch.float32:
        raise ValueError("msda: the coordinate tensors are %s, value is %s: they must have value's dtype or float32" % (
            loc.dtype, value.dtype))
    return (N, Lq, M * D)


# the call itself (the seam the tests replace): workspace query, allocation, current stream, call, RuntimeError
_run = functools.partial(_samp.run, "mdconv_msda")


def ms_deform_attn_forward(value, spatial_shapes, sampling_locations, attention_weights, output=None):
    """The forward entry point on dense CUDA tensors; allocates ``output`` unless it is given."""
    if not value.is_cuda:
        raise NotImplementedError
    shapes = _shapes(spatial_shapes)
    d = _desc(value, sampling_locations, shapes)
    others = {} if output is None else dict(output=output)
    shape = _check(d, shapes, value, sampling_locations, attention_weights, **others)
    # pointer classes (include/mdconv.h): value and output are "16-byte", the locations and weights "element"
    _capi.require_aligned_result("msda", "output", output)
    value = _capi.aligned_input(value)
    if output is None:
        output = torch.empty(shape, dtype=value.dtype, device=value.device)
    _run("mdconv_msda_forward", d, False, [_ptr(value), _ptr(sampling_locations), _ptr(attention_weights), _ptr(output)], value)
    return output


def ms_deform_attn_backward(value, spatial_shapes, sampling_locations, attention_weights, grad_output, grads=None,
                            need_grad_value=True, deterministic=None, accumulate=None):
    """The backward entry point.  ``grads`` = (grad_value | None, grad_sampling_locations, grad_attention_weights):
    caller-allocated buffers the gradients are ADDED to; without it fresh tensors are written.  ``need_grad_value`` false:
    grad_value is neither computed nor allocated (``MDCONV_FLAG_NO_GRAD_INPUT``) and None is returned there.
    ``deterministic`` None follows ``_capi.deterministic_mode()``.  ``accumulate`` false with ``grads``: the caller's
    buffers are overwritten instead.  Returns the three gradients in that order."""
    if not value.is_cuda:
        raise NotImplementedError
    shapes = _shapes(spatial_shapes)
    flags = _samp.backward_flags(deterministic, need_grad_value)
    d = _desc(value, sampling_locations, shapes,
              accumulate=int(grads is not None if accumulate is None else bool(accumulate)), flags=flags)
    _check(d, shapes, value, sampling_locations, attention_weights, grad_output=grad_output)
    # pointer classes (include/mdconv.h): value, grad_output and grad_value are "16-byte", the coordinate tensors "element"
    if grads is not None and need_grad_value:
        _capi.require_aligned_result("msda", "grad_value", grads[0])
    value, grad_output = _capi.aligned_input(value), _capi.aligned_input(grad_output)
    if grads is None:
        grads = (torch.empty_like(value) if need_grad_value else None, torch.empty_like(sampling_locations),
                 torch.empty_like(attention_weights))
    gv, gl, ga = grads
    _samp.check_grads("msda", (("grad_value", gv, value), ("grad_sampling_locations", gl, sampling_locations), ("grad_attention_weights", ga, attention_weights)),
                      may_be_none=() if need_grad_value else ("grad_value",))
    _run("mdconv_msda_backward", d, True,
         [_ptr(value), _ptr(sampling_locations), _ptr(attention_weights), _ptr(grad_output),
          _ptr(gv if need_grad_value else None), _ptr(gl), _ptr(ga)], value)
    return (gv if need_grad_value else None), gl, ga


class MSDeformAttnFunction(Function):
    """``MSDeformAttnFunction.apply(value, spatial_shapes, level_start_index, sampling_locations, attention_weights,
    im2col_step)`` -- the argument order of the published operator; ``im2col_step`` is accepted for signature parity and
    unused.  ``spatial_shapes`` is a sequence of (H, W) or a tensor; a CUDA tensor costs a ``.tolist()`` synchronisation
    per call and cannot be read during graph capture, so pass host data there.  ``level_start_index`` is checked against
    the cumulative sums when it is host data and ignored otherwise.  Under ``torch.autocast`` ``value`` runs in the
    autocast dtype; coordinate tensors that are fp32 stay fp32 (the mixed call), others run in the autocast dtype.  The
    gradients go back in the dtypes the caller's tensors have."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step=64):
        if not value.is_cuda:
            raise NotImplementedError
        shapes = _shapes(spatial_shapes)
        _check_starts(shapes, level_start_index)
        ctx.shapes = shapes
        ctx.in_dtypes = (value.dtype, sampling_locations.dtype, attention_weights.dtype)
        if torch.is_autocast_enabled("cuda"):
            value = value.to(torch.get_autocast_dtype("cuda"))
        # one dtype for the two coordinate tensors: fp32 if either is (or if they disagree), else value's
        cdt = _samp.coord_dtype(value.dtype, sampling_locations.dtype, attention_weights.dtype)
        value = value.contiguous()
        sampling_locations = sampling_locations.to(cdt).contiguous()
        attention_weights = attention_weights.to(cdt).contiguous()
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(value, sampling_locations, attention_weights)
        return ms_deform_attn_forward(value, shapes, sampling_locations, attention_weights)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        if not grad_output.is_cuda:
            raise NotImplementedError
        value, loc, attn = ctx.saved_tensors
        grad_output = grad_output.to(value.dtype).contiguous()
        # selective backward: grad_value is neither computed nor allocated when `value` needs no gradient
        gv, gl, ga = ms_deform_attn_backward(value, ctx.shapes, loc, attn, grad_output,
                                             need_grad_value=bool(ctx.needs_input_grad[0]))
        back = _samp.back
        dv, dl, da = ctx.in_dtypes
        return back(gv, dv), None, None, back(gl, dl), back(ga, da), None


def ms_deform_attn(value, spatial_shapes, sampling_locations, attention_weights, level_start_index=None):
    """Functional form of ``MSDeformAttnFunction``."""
    return MSDeformAttnFunction.apply(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, 64)


class MSDeformAttn(nn.Module):
    """The multi-scale deformable attention block: value projection, the ``sampling_offsets`` and ``attention_weights``
    linears on the query (softmax over the L*P taps of a head), the core operator, output projection.  Everything but the
    core operator is a framework operator.  Parameter names (``sampling_offsets``, ``attention_weights``, ``value_proj``,
    ``output_proj``) and the initialisation -- the directional bias of ``sampling_offsets`` included -- follow the published
    block so that a checkpoint can load; written from memory of that code and UNPINNED against it."""

    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4):
        super().__init__()
        if d_model % n_heads:
            raise ValueError("d_model must be divisible by n_heads, but got %d and %d" % (d_model, n_heads))
        self.im2col_step = 64
        self.d_model, self.n_levels, self.n_heads, self.n_points = d_model, n_levels, n_heads, n_points
        self.sampling_offsets = nn.Linear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = nn.Linear(d_model, n_heads * n_levels * n_points)
        self.value_proj = nn.Linear(d_model, d_model)
        self.output_proj = nn.Linear(d_model, d_model)
        self._core = ms_deform_attn
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.zeros_(self.sampling_offsets.weight)
        # directional bias: head h looks along the angle 2 pi h / n_heads, point p at p + 1 steps, the same on every level
        thetas = torch.arange(self.n_heads, dtype=torch.float32) * (2.0 * math.pi / self.n_heads)
        grid = torch.stack([thetas.cos(), thetas.sin()], -1)
        grid = (grid / grid.abs().max(-1, keepdim=True)[0]).view(self.n_heads, 1, 1, 2).repeat(1, self.n_levels, self.n_points, 1)
        for i in range(self.n_points):
            grid[:, :, i, :] *= i + 1
        with torch.no_grad():
            self.sampling_offsets.bias.copy_(grid.reshape(-1))
        nn.init.zeros_(self.attention_weights.weight)
        nn.init.zeros_(self.attention_weights.bias)
        for lin in (self.value_proj, self.output_proj):
            nn.init.xavier_uniform_(lin.weight)
            nn.init.zeros_(lin.bias)

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                input_padding_mask=None):
        """``query [N, Lq, C]``, ``reference_points [N, Lq, L, 2]`` (x, y) or ``[N, Lq, L, 4]`` (x, y, w, h), normalised;
        ``input_flatten [N, S, C]``; ``input_spatial_shapes``: L rows (H, W), host data or a tensor (a CUDA tensor costs a
        synchronisation per call); ``input_padding_mask [N, S]``: True where the value is padding."""
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
        # (softmax and the locations run in fp32 under autocast: the core then takes fp32 coordinates)
        weights = F.softmax(self.attention_weights(query).float().view(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
        ref = reference_points.float()
        if ref.shape[-1] == 2:
            wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32, device=query.device)   # (x, y) order
            locations = ref[:, :, None, :, None, :] + offsets / wh[None, None, None, :, None, :]
        elif ref.shape[-1] == 4:
            locations = ref[:, :, None, :, None, :2] + offsets / P * ref[:, :, None, :, None, 2:] * 0.5
        else:
            raise ValueError("the last dimension of reference_points must be 2 or 4, but is %d" % ref.shape[-1])
        out = self._core(value, shapes, locations, weights, input_level_start_index)
        return self.output_proj(out)

    def extra_repr(self):
        return "d_model=%d, n_levels=%d, n_heads=%d, n_points=%d" % (self.d_model, self.n_levels, self.n_heads, self.n_points)
