"""Multi-scale deformable attention with a point count per level on the MI355X-native backend: the sampling operator of
the real-time DETR line (RT-DETRv2's ``num_points_list``; D-FINE and DEIM ship (3, 6, 3)) on channels-last tensors
(include/mdconv_msdap.h; INTEGRATION.md has the contract and what is unpinned).

    ms_deform_attn_points_forward / ms_deform_attn_points_backward   the entry points on dense CUDA tensors
    MSDeformAttnPointsFunction   autograd.Function over mdconv_msdap_forward / mdconv_msdap_backward
    ms_deform_attn_points        the functional form
    MSDeformableAttention        nn.Module: the RT-DETRv2 attention block around the operator, composed from framework operators

``value [N, S, M, D]`` (the levels concatenated), ``sampling_locations [N, Lq, M, K, 2]`` ((x, y), normalised),
``attention_weights [N, Lq, M, K]`` -> ``output [N, Lq, M*D]``; K = ``sum(num_points_list)`` and the taps are level-major:
level 0 owns the first ``num_points_list[0]`` taps, level 1 the next ``num_points_list[1]``, and so on.  ``value`` is fp32 /
fp16 / bf16; the two coordinate tensors have its dtype or are fp32.  With equal counts the operator is ``ms_deform_attn`` on
the same memory.  CPU tensors raise ``NotImplementedError``: there is no CPU or PyTorch fallback.
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
from .msda import _shapes

__all__ = ["ms_deform_attn_points_forward", "ms_deform_attn_points_backward", "MSDeformAttnPointsFunction",
           "ms_deform_attn_points", "MSDeformableAttention"]


def _points(num_points_list, levels):
    """``num_points_list`` as a tuple of ``levels`` positive ints.  A tensor is read with ``.tolist()``: for a CUDA tensor
    that is a host synchronisation (and impossible during graph capture) -- pass host data to avoid it."""
    if isinstance(num_points_list, torch.Tensor):
        num_points_list = num_points_list.tolist()
    points = tuple(int(p) for p in num_points_list)
    if len(points) != levels:
        raise ValueError("msdap: num_points_list has %d entries, spatial_shapes %d levels" % (len(points), levels))
    if any(p <= 0 for p in points):
        raise ValueError("msdap: num_points_list %s has a non-positive count" % (points,))
    return points


def _desc(value, loc, shapes, points, accumulate=1, flags=0):
    if value.dtype not in _DTYPES or loc.dtype not in _DTYPES:
        raise TypeError("msdap: dtypes %s / %s are not float32, float16 or bfloat16" % (value.dtype, loc.dtype))
    if value.dim() != 4 or loc.dim() != 5:
        raise ValueError("msdap: value must be [N, S, M, D] and sampling_locations [N, Lq, M, K, 2], got %s and %s" % (
            tuple(value.shape), tuple(loc.shape)))
    d = _capi.MdconvMsdapDesc()
    d.dtype, d.coord_dtype = _DTYPES[value.dtype], _DTYPES[loc.dtype]
    d.batch, d.heads, d.head_channels = int(value.shape[0]), int(value.shape[2]), int(value.shape[3])
    d.queries, d.levels = int(loc.shape[1]), len(shapes)
    for l, ((h, w), p) in enumerate(zip(shapes, points)):
        d.level_sz[l][0], d.level_sz[l][1], d.points[l] = h, w, p
    d.accumulate, d.flags = int(accumulate), int(flags)
    return d


def _check(d, shapes, points, value, loc, attn, **others):
    """Shapes, dtypes, devices and density of the tensors of a call; ``others`` have the shape of ``output``."""
    N, M, D, Lq, K = d.batch, d.heads, d.head_channels, d.queries, sum(points)
    S = sum(h * w for h, w in shapes)
    if loc.shape[3] != K:
        raise ValueError("msdap: sampling_locations has %d taps per head, num_points_list %s sums to %d" % (
            loc.shape[3], points, K))
    want = dict(value=(N, S, M, D), sampling_locations=(N, Lq, M, K, 2), attention_weights=(N, Lq, M, K))
    want.update({k: (N, Lq, M * D) for k in others})
    tensors = dict(value=value, sampling_locations=loc, attention_weights=attn, **others)
    for name, t in tensors.items():
        if tuple(t.shape) != want[name]:
            raise ValueError("msdap: %s must be %s, got %s" % (name, want[name], tuple(t.shape)))
        like = loc if name in ("sampling_locations", "attention_weights") else value
        if t.dtype != like.dtype or t.device != value.device:
            raise ValueError("msdap: %s is %s on %s; value is %s on %s and the coordinate tensors are %s (value, output and "
                             "grad_output share one dtype, the two coordinate tensors another: the same, or float32)" % (
                                 name, t.dtype, t.device, value.dtype, value.device, loc.dtype))
        if not t.is_contiguous():
            raise ValueError("msdap: %s must be dense and row-major (contiguous)" % name)
    if loc.dtype != value.dtype and loc.dtype != torch.float32:
        raise ValueError("msdap: the coordinate tensors are %s, value is %s: they must have value's dtype or float32" % (
            loc.dtype, value.dtype))
    return (N, Lq, M * D)


# the call itself (the seam the tests replace): workspace query, allocation, current stream, call, RuntimeError
_run = functools.partial(_samp.run, "mdconv_msdap")


def ms_deform_attn_points_forward(value, spatial_shapes, num_points_list, sampling_locations, attention_weights, output=None):
    """The forward entry point on dense CUDA tensors; allocates ``output`` unless it is given."""
    shapes = _shapes(spatial_shapes)
    points = _points(num_points_list, len(shapes))
    d = _desc(value, sampling_locations, shapes, points)
    others = {} if output is None else dict(output=output)
    shape = _check(d, shapes, points, value, sampling_locations, attention_weights, **others)
    if not value.is_cuda:
        raise NotImplementedError
    # pointer classes (include/mdconv_msdap.h): value and output are "16-byte", the locations and weights "element"
    _capi.require_aligned_result("msdap", "output", output)
    value = _capi.aligned_input(value)
    if output is None:
        output = torch.empty(shape, dtype=value.dtype, device=value.device)
    _run("mdconv_msdap_forward", d, False, [_ptr(value), _ptr(sampling_locations), _ptr(attention_weights), _ptr(output)], value)
    return output


def ms_deform_attn_points_backward(value, spatial_shapes, num_points_list, sampling_locations, attention_weights, grad_output,
                                   grads=None, need_grad_value=True, deterministic=None, accumulate=None):
    """The backward entry point.  ``grads`` = (grad_value | None, grad_sampling_locations, grad_attention_weights):
    caller-allocated buffers the gradients are ADDED to; without it fresh tensors are written.  ``need_grad_value`` false:
    grad_value is neither computed nor allocated (``MDCONV_FLAG_NO_GRAD_INPUT``) and None is returned there.
    ``deterministic`` None follows ``_capi.deterministic_mode()``.  ``accumulate`` false with ``grads``: the caller's
    buffers are overwritten instead.  Returns the three gradients in that order."""
    shapes = _shapes(spatial_shapes)
    points = _points(num_points_list, len(shapes))
    flags = _samp.backward_flags(deterministic, need_grad_value)
    d = _desc(value, sampling_locations, shapes, points,
              accumulate=int(grads is not None if accumulate is None else bool(accumulate)), flags=flags)
    _check(d, shapes, points, value, sampling_locations, attention_weights, grad_output=grad_output)
    if not value.is_cuda:
        raise NotImplementedError
    # pointer classes (include/mdconv_msdap.h): value, grad_output and grad_value are "16-byte", the coordinate tensors "element"
    if grads is not None and need_grad_value:
        _capi.require_aligned_result("msdap", "grad_value", grads[0])
    value, grad_output = _capi.aligned_input(value), _capi.aligned_input(grad_output)
    if grads is None:
        grads = (torch.empty_like(value) if need_grad_value else None, torch.empty_like(sampling_locations),
                 torch.empty_like(attention_weights))
    gv, gl, ga = grads
    _samp.check_grads("msdap", (("grad_value", gv, value), ("grad_sampling_locations", gl, sampling_locations),
                                ("grad_attention_weights", ga, attention_weights)),
                      may_be_none=() if need_grad_value else ("grad_value",))
    _run("mdconv_msdap_backward", d, True,
         [_ptr(value), _ptr(sampling_locations), _ptr(attention_weights), _ptr(grad_output),
          _ptr(gv if need_grad_value else None), _ptr(gl), _ptr(ga)], value)
    return (gv if need_grad_value else None), gl, ga


class MSDeformAttnPointsFunction(Function):
    """``MSDeformAttnPointsFunction.apply(value, spatial_shapes, num_points_list, sampling_locations, attention_weights)``.
    ``spatial_shapes`` (rows of (H, W)) and ``num_points_list`` are host data: sequences, or tensors -- a CUDA tensor costs a
    ``.tolist()`` synchronisation per call and cannot be read during graph capture.  Under ``torch.autocast`` ``value`` runs
    in the autocast dtype; coordinate tensors that are fp32 stay fp32 (the mixed call), others run in the autocast dtype.
    The gradients go back in the dtypes the caller's tensors have."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, num_points_list, sampling_locations, attention_weights):
        if not value.is_cuda:
            raise NotImplementedError
        shapes = _shapes(spatial_shapes)
        points = _points(num_points_list, len(shapes))
        ctx.shapes, ctx.points = shapes, points
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
        return ms_deform_attn_points_forward(value, shapes, points, sampling_locations, attention_weights)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        if not grad_output.is_cuda:
            raise NotImplementedError
        value, loc, attn = ctx.saved_tensors
        grad_output = grad_output.to(value.dtype).contiguous()
        # selective backward: grad_value is neither computed nor allocated when `value` needs no gradient
        gv, gl, ga = ms_deform_attn_points_backward(value, ctx.shapes, ctx.points, loc, attn, grad_output,
                                                    need_grad_value=bool(ctx.needs_input_grad[0]))
        back = _samp.back
        dv, dl, da = ctx.in_dtypes
        return back(gv, dv), None, None, back(gl, dl), back(ga, da)


def ms_deform_attn_points(value, spatial_shapes, num_points_list, sampling_locations, attention_weights):
    """Functional form of ``MSDeformAttnPointsFunction``."""
    return MSDeformAttnPointsFunction.apply(value, spatial_shapes, num_points_list, sampling_locations, attention_weights)


class MSDeformableAttention(nn.Module):
    """The deformable attention block of RT-DETRv2 (D-FINE and DEIM carry the same one): value projection, the
    ``sampling_offsets`` and ``attention_weights`` linears on the query (softmax over all K = sum(num_points) taps of a
    head), the core operator, output projection.  ``num_points`` is an int (every level) or a list with one count per
    level.  Everything but the core operator is a framework operator.  Parameter names (``sampling_offsets``,
    ``attention_weights``, ``value_proj``, ``output_proj``), the buffer ``num_points_scale`` (1/n repeated n times per level)
    and the initialisation -- the directional bias of ``sampling_offsets`` included -- follow the published block so that a
    checkpoint can load; written from memory of that code and UNPINNED against it.  ``method='discrete'``
    of the published block (samples rounded to one pixel, no location gradient: a deployment workaround for runtimes
    without grid_sample) is not implemented."""

    def __init__(self, embed_dim=256, num_heads=8, num_levels=4, num_points=4, offset_scale=0.5, method="default"):
        super().__init__()
        if method == "discrete":
            raise NotImplementedError("MSDeformableAttention: method='discrete' is not implemented (it rounds every sample to "
                                      "one pixel for runtimes without grid_sample); use method='default'")
        if method != "default":
            raise ValueError("MSDeformableAttention: method must be 'default', got %r" % (method,))
        if embed_dim % num_heads:
            raise ValueError("embed_dim must be divisible by num_heads, but got %d and %d" % (embed_dim, num_heads))
        if isinstance(num_points, (list, tuple)):
            if len(num_points) != num_levels:
                raise ValueError("num_points %s must have num_levels = %d entries" % (list(num_points), num_levels))
            num_points_list = [int(p) for p in num_points]
        else:
            num_points_list = [int(num_points)] * num_levels
        if any(p <= 0 for p in num_points_list):
            raise ValueError("num_points %s has a non-positive count" % (num_points_list,))
        self.embed_dim, self.num_heads, self.num_levels, self.offset_scale = embed_dim, num_heads, num_levels, offset_scale
        self.num_points_list, self.method = num_points_list, method
        self.head_dim = embed_dim // num_heads
        self.total_points = num_heads * sum(num_points_list)
        self.register_buffer("num_points_scale",
                             torch.tensor([1.0 / n for n in num_points_list for _ in range(n)], dtype=torch.float32))
        self.sampling_offsets = nn.Linear(embed_dim, self.total_points * 2)
        self.attention_weights = nn.Linear(embed_dim, self.total_points)
        self.value_proj = nn.Linear(embed_dim, embed_dim)
        self.output_proj = nn.Linear(embed_dim, embed_dim)
        self._core = ms_deform_attn_points
        self._reset_parameters()

    def _reset_parameters(self):
        nn.init.zeros_(self.sampling_offsets.weight)
        # directional bias: head h looks along the angle 2 pi h / num_heads; on every level point p sits at p + 1 steps, so the
        # pattern repeats per level with that level's point count
        thetas = torch.arange(self.num_heads, dtype=torch.float32) * (2.0 * math.pi / self.num_heads)
        grid = torch.stack([thetas.cos(), thetas.sin()], -1)
        grid = (grid / grid.abs().max(-1, keepdim=True)[0]).view(self.num_heads, 1, 2).repeat(1, sum(self.num_points_list), 1)
        steps = torch.cat([torch.arange(1, n + 1, dtype=torch.float32) for n in self.num_points_list])
        with torch.no_grad():
            self.sampling_offsets.bias.copy_((grid * steps.view(1, -1, 1)).reshape(-1))
        nn.init.zeros_(self.attention_weights.weight)
        nn.init.zeros_(self.attention_weights.bias)
        for lin in (self.value_proj, self.output_proj):
            nn.init.xavier_uniform_(lin.weight)
            nn.init.zeros_(lin.bias)

    def forward(self, query, reference_points, value, value_spatial_shapes, value_mask=None):
        """``query [N, Lq, C]``; ``reference_points``, normalised: boxes ``[N, Lq, 1, 4]`` (x, y, w, h; one box for all levels)
        or ``[N, Lq, L, 4]`` (one per level), or -- equal point counts only -- points ``[N, Lq, L, 2]`` (x, y);
        ``value [N, S, C]``; ``value_spatial_shapes``: L rows (H, W), host data or a tensor (a CUDA tensor costs a
        synchronisation per call); ``value_mask [N, S]``: True / 1 where the value is KEPT (the published block multiplies)."""
        N, Lq, _ = query.shape
        shapes, value = self._values(value, value_spatial_shapes, value_mask)
        K = sum(self.num_points_list)
        # (softmax and the locations run in fp32 under autocast: the core then takes fp32 coordinates)
        weights = F.softmax(self.attention_weights(query).float().view(N, Lq, self.num_heads, K), -1)
        locations = self._locations(query, reference_points, shapes)
        out = self._core(value, shapes, self.num_points_list, locations, weights)
        return self.output_proj(out)

    def _values(self, value, value_spatial_shapes, value_mask):
        """The level extents as host data and the projected, masked ``value [N, S, M, D]`` of a forward."""
        N, S = value.shape[:2]
        shapes = _shapes(value_spatial_shapes)
        if len(shapes) != self.num_levels or sum(h * w for h, w in shapes) != S:
            raise ValueError("value_spatial_shapes %s does not describe %d levels of %d rows" % (shapes, self.num_levels, S))
        value = self.value_proj(value)
        if value_mask is not None:
            value = value * value_mask.to(value.dtype).unsqueeze(-1)
        return shapes, value.view(N, S, self.num_heads, self.head_dim)

    def _locations(self, query, reference_points, shapes):
        """``sampling_locations [N, Lq, M, K, 2]`` of a forward, fp32: the reference points (or boxes) plus the scaled output
        of the ``sampling_offsets`` linear.  (A method of its own for ``MSDeformableAttentionFused``.)"""
        N, Lq, _ = query.shape
        M, L, K = self.num_heads, self.num_levels, sum(self.num_points_list)
        offsets = self.sampling_offsets(query).float().view(N, Lq, M, K, 2)
        ref = reference_points.float()
        if ref.dim() != 4 or ref.shape[:2] != (N, Lq):
            raise ValueError("reference_points must be [N, Lq, 1 or L, 2 or 4], got %s" % (tuple(reference_points.shape),))
        if ref.shape[2] == L and L > 1:   # one reference per level -> one per tap, level-major
            counts = torch.tensor(self.num_points_list, device=ref.device)
            ref = ref.repeat_interleave(counts, dim=2, output_size=K)
        elif ref.shape[2] != 1:
            raise ValueError("reference_points must have 1 or %d levels, got %d" % (L, ref.shape[2]))
        if ref.shape[-1] == 2:
            if len(set(self.num_points_list)) != 1 or reference_points.shape[2] != L:
                raise ValueError("two-component reference_points need equal point counts and one point per level; "
                                 "num_points is %s: pass boxes (x, y, w, h)" % (self.num_points_list,))
            wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32, device=query.device)   # (x, y) order
            wh = wh.repeat_interleave(self.num_points_list[0], dim=0)
            return ref[:, :, None, :, :] + offsets / wh[None, None, None, :, :]
        if ref.shape[-1] == 4:
            scale = self.num_points_scale.float()[None, None, None, :, None]
            return ref[:, :, None, :, :2] + offsets * scale * ref[:, :, None, :, 2:] * self.offset_scale
        raise ValueError("the last dimension of reference_points must be 2 or 4, but is %d" % ref.shape[-1])

    def extra_repr(self):
        return "embed_dim=%d, num_heads=%d, num_levels=%d, num_points=%s, offset_scale=%s" % (
            self.embed_dim, self.num_heads, self.num_levels, self.num_points_list, self.offset_scale)
