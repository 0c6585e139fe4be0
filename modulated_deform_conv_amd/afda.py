"""Anchored packed deformable attention on the MI355X-native backend: the decoder attention of the real-time DETR line
(RT-DETRv2, D-FINE, DEIM) and, with two-component references, of the Deformable-DETR / DINO decoders, taking what the
linear layers produce AS IT IS -- the packed row of RAW sampling offsets and attention LOGITS of one linear, and the
reference points or boxes.  The reference arithmetic, the softmax over all K taps and the sampling run inside the operator
(include/mdconv_afda.h; INTEGRATION.md has the contract and what is unpinned).

    anchored_deform_attn_forward / anchored_deform_attn_backward   the entry points on dense CUDA tensors
    AnchoredDeformAttnFunction      autograd.Function over mdconv_afda_forward / mdconv_afda_backward
    anchored_deform_attn            the functional form
    MSDeformableAttentionAnchored   nn.Module: ``MSDeformableAttention``'s block (same parameters, same checkpoints) as
                                    value_proj, ONE linear, this operator and output_proj

``value [N, S, M, D]`` (the levels concatenated), ``reference_points [N, Lq, Lr, R]`` (fp32; Lr = 1 or L; R = 2: (x, y), or
4: (x, y, w, h); normalised), ``offs_attn [N, Lq, M, 3K]`` (per (query, head): (dx, dy) of tap 0 .. K-1, then the K logits;
K = ``sum(num_points_list)``, the taps level-major) -> ``output [N, Lq, M*D]``.  ``value`` is fp32 / fp16 / bf16; the packed
tensor has its dtype or is fp32; the reference is always fp32, so a 16-bit packed row of offsets of a few units loses no
sub-pixel precision.  CPU tensors raise ``NotImplementedError``: there is no CPU or PyTorch fallback.
"""
import functools

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn import functional as F

from . import _capi, _samp
from ._samp import DTYPES as _DTYPES, ptr as _ptr
from .msda import _shapes
from .msdap import MSDeformableAttention, _points

__all__ = ["anchored_deform_attn_forward", "anchored_deform_attn_backward", "AnchoredDeformAttnFunction",
           "anchored_deform_attn", "MSDeformableAttentionAnchored"]


def _desc(value, ref, offs_attn, shapes, points, offset_scale, accumulate=1, flags=0, grad_reference=1):
    if value.dtype not in _DTYPES or offs_attn.dtype not in _DTYPES:
        raise TypeError("afda: dtypes %s / %s are not float32, float16 or bfloat16" % (value.dtype, offs_attn.dtype))
    if value.dim() != 4 or offs_attn.dim() != 4 or ref.dim() != 4:
        raise ValueError("afda: value must be [N, S, M, D], reference_points [N, Lq, Lr, R] and offs_attn [N, Lq, M, 3*K], "
                         "got %s, %s and %s" % (tuple(value.shape), tuple(ref.shape), tuple(offs_attn.shape)))
    d = _capi.MdconvAfdaDesc()
    d.dtype, d.coord_dtype = _DTYPES[value.dtype], _DTYPES[offs_attn.dtype]
    d.batch, d.heads, d.head_channels = int(value.shape[0]), int(value.shape[2]), int(value.shape[3])
    d.queries, d.levels = int(offs_attn.shape[1]), len(shapes)
    for l, ((h, w), p) in enumerate(zip(shapes, points)):
        d.level_sz[l][0], d.level_sz[l][1], d.points[l] = h, w, p
    d.accumulate, d.flags = int(accumulate), int(flags)
    d.ref_levels, d.ref_comps = int(ref.shape[2]), int(ref.shape[3])
    d.offset_scale, d.grad_reference = float(offset_scale), int(grad_reference)
    return d


def _check(d, shapes, points, value, ref, offs_attn, **others):
    """Shapes, dtypes, devices and density of the tensors of a call; ``others`` have the shape of ``output``."""
    N, M, D, Lq, K = d.batch, d.heads, d.head_channels, d.queries, sum(points)
    S = sum(h * w for h, w in shapes)
    if offs_attn.shape[3] != 3 * K:
        raise ValueError("afda: offs_attn has %d elements per head, num_points_list %s asks for 3 * %d" % (
            offs_attn.shape[3], points, K))
    if d.ref_levels not in (1, len(shapes)) or d.ref_comps not in (2, 4):
        raise ValueError("afda: reference_points must be [N, Lq, 1 or %d, 2 or 4], got %s" % (len(shapes), tuple(ref.shape)))
    if ref.dtype != torch.float32:
        raise ValueError("afda: reference_points is %s: it must be float32" % (ref.dtype,))
    want = dict(value=(N, S, M, D), reference_points=(N, Lq, d.ref_levels, d.ref_comps), offs_attn=(N, Lq, M, 3 * K))
    want.update({k: (N, Lq, M * D) for k in others})
    tensors = dict(value=value, reference_points=ref, offs_attn=offs_attn, **others)
    for name, t in tensors.items():
        if tuple(t.shape) != want[name]:
            raise ValueError("afda: %s must be %s, got %s" % (name, want[name], tuple(t.shape)))
        like = offs_attn if name == "offs_attn" else (ref if name == "reference_points" else value)
        if t.dtype != like.dtype or t.device != value.device:
            raise ValueError("afda: %s is %s on %s; value is %s on %s and offs_attn is %s (value, output and grad_output "
                             "share one dtype, the packed tensor has it too or is float32, reference_points is float32)" % (
                                 name, t.dtype, t.device, value.dtype, value.device, offs_attn.dtype))
        if not t.is_contiguous():
            raise ValueError("afda: %s must be dense and row-major (contiguous)" % name)
    if offs_attn.dtype != value.dtype and offs_attn.dtype != torch.float32:
        raise ValueError("afda: offs_attn is %s, value is %s: it must have value's dtype or float32" % (
            offs_attn.dtype, value.dtype))
    return (N, Lq, M * D)


# the call itself (the seam the tests replace): workspace query, allocation, current stream, call, RuntimeError
_run = functools.partial(_samp.run, "mdconv_afda")


def anchored_deform_attn_forward(value, spatial_shapes, num_points_list, reference_points, offs_attn, offset_scale=0.5,
                                 output=None):
    """The forward entry point on dense CUDA tensors; allocates ``output`` unless it is given."""
    shapes = _shapes(spatial_shapes)
    points = _points(num_points_list, len(shapes))
    d = _desc(value, reference_points, offs_attn, shapes, points, offset_scale)
    others = {} if output is None else dict(output=output)
    shape = _check(d, shapes, points, value, reference_points, offs_attn, **others)
    if not value.is_cuda:
        raise NotImplementedError
    # pointer classes (include/mdconv_afda.h): value and output are "16-byte", reference_points and offs_attn "element"
    _capi.require_aligned_result("afda", "output", output)
    value = _capi.aligned_input(value)
    if output is None:
        output = torch.empty(shape, dtype=value.dtype, device=value.device)
    _run("mdconv_afda_forward", d, False, [_ptr(value), _ptr(reference_points), _ptr(offs_attn), _ptr(output)], value)
    return output


def anchored_deform_attn_backward(value, spatial_shapes, num_points_list, reference_points, offs_attn, grad_output,
                                  offset_scale=0.5, grads=None, need_grad_value=True, need_grad_reference=True,
                                  deterministic=None, accumulate=None):
    """The backward entry point.  ``grads`` = (grad_value | None, grad_reference | None, grad_offs_attn): caller-allocated
    buffers the gradients are ADDED to; without it fresh tensors are written.  ``need_grad_value`` false: grad_value is
    neither computed nor allocated (``MDCONV_FLAG_NO_GRAD_INPUT``) and None is returned there; ``need_grad_reference`` false:
    likewise for grad_reference (``grad_reference = 0`` in the descriptor).  ``deterministic`` None follows
    ``_capi.deterministic_mode()``.  ``accumulate`` false with ``grads``: the caller's buffers are overwritten instead.
    Takes no ``output``.  Returns the three gradients in that order."""
    shapes = _shapes(spatial_shapes)
    points = _points(num_points_list, len(shapes))
    flags = _samp.backward_flags(deterministic, need_grad_value)
    d = _desc(value, reference_points, offs_attn, shapes, points, offset_scale,
              accumulate=int(grads is not None if accumulate is None else bool(accumulate)), flags=flags,
              grad_reference=int(bool(need_grad_reference)))
    _check(d, shapes, points, value, reference_points, offs_attn, grad_output=grad_output)
    if not value.is_cuda:
        raise NotImplementedError
    # pointer classes (include/mdconv_afda.h): value, grad_output and grad_value are "16-byte", the reference pair and the
    # packed pair "element"
    if grads is not None and need_grad_value:
        _capi.require_aligned_result("afda", "grad_value", grads[0])
    value, grad_output = _capi.aligned_input(value), _capi.aligned_input(grad_output)
    if grads is None:
        grads = (torch.empty_like(value) if need_grad_value else None,
                 torch.empty_like(reference_points) if need_grad_reference else None, torch.empty_like(offs_attn))
    gv, gr, goa = grads
    skipped = (() if need_grad_value else ("grad_value",)) + (() if need_grad_reference else ("grad_reference",))
    _samp.check_grads("afda", (("grad_value", gv, value), ("grad_reference", gr, reference_points),
                               ("grad_offs_attn", goa, offs_attn)), may_be_none=skipped)
    _run("mdconv_afda_backward", d, True,
         [_ptr(value), _ptr(reference_points), _ptr(offs_attn), _ptr(grad_output), _ptr(gv if need_grad_value else None),
          _ptr(gr if need_grad_reference else None), _ptr(goa)], value)
    return (gv if need_grad_value else None), (gr if need_grad_reference else None), goa


class AnchoredDeformAttnFunction(Function):
    """``AnchoredDeformAttnFunction.apply(value, spatial_shapes, num_points_list, reference_points, offs_attn,
    offset_scale)``.  ``spatial_shapes`` (rows of (H, W)) and ``num_points_list`` are host data: sequences, or tensors -- a
    CUDA tensor costs a ``.tolist()`` synchronisation per call and cannot be read during graph capture.  Under
    ``torch.autocast`` ``value`` runs in the autocast dtype; a packed tensor keeps its dtype if it is fp32 or equals value's
    (else it runs in fp32); ``reference_points`` is cast to fp32.  The gradients go back in the dtypes the caller's tensors
    have; grad_value and grad_reference are computed only for tensors that need them."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, num_points_list, reference_points, offs_attn, offset_scale=0.5):
        if not value.is_cuda:
            raise NotImplementedError
        shapes = _shapes(spatial_shapes)
        points = _points(num_points_list, len(shapes))
        ctx.shapes, ctx.points, ctx.offset_scale = shapes, points, float(offset_scale)
        ctx.in_dtypes = (value.dtype, reference_points.dtype, offs_attn.dtype)
        if torch.is_autocast_enabled("cuda"):
            value = value.to(torch.get_autocast_dtype("cuda"))
        cdt = _samp.coord_dtype(value.dtype, offs_attn.dtype)
        value = value.contiguous()
        reference_points = reference_points.float().contiguous()
        offs_attn = offs_attn.to(cdt).contiguous()
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(value, reference_points, offs_attn)   # (no output: the backward does not take it)
        return anchored_deform_attn_forward(value, shapes, points, reference_points, offs_attn, ctx.offset_scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        if not grad_output.is_cuda:
            raise NotImplementedError
        value, ref, offs_attn = ctx.saved_tensors
        grad_output = grad_output.to(value.dtype).contiguous()
        # selective backward: grad_value and grad_reference are neither computed nor allocated for tensors that need none
        gv, gr, goa = anchored_deform_attn_backward(value, ctx.shapes, ctx.points, ref, offs_attn, grad_output, ctx.offset_scale,
                                                    need_grad_value=bool(ctx.needs_input_grad[0]),
                                                    need_grad_reference=bool(ctx.needs_input_grad[3]))
        back = _samp.back
        dv, dr, do = ctx.in_dtypes
        return back(gv, dv), None, None, back(gr, dr), (back(goa, do) if ctx.needs_input_grad[4] else None), None


def anchored_deform_attn(value, spatial_shapes, num_points_list, reference_points, offs_attn, offset_scale=0.5):
    """Functional form of ``AnchoredDeformAttnFunction``."""
    return AnchoredDeformAttnFunction.apply(value, spatial_shapes, num_points_list, reference_points, offs_attn, offset_scale)


class MSDeformableAttentionAnchored(MSDeformableAttention):
    """``MSDeformableAttention`` on the anchored operator: the same constructor, parameter names, buffer and
    initialisation, so the same checkpoints load, and the same ``forward`` arguments.  The block is ``value_proj``, ONE
    linear, the operator and ``output_proj``: each forward builds the fused weight and bias of that linear from
    ``sampling_offsets`` and ``attention_weights`` (a weight-sized ``cat``, per head the head's 2K offset rows and then its K
    logit rows; autograd carries the parameter gradients back), and its output IS the packed row -- no ``cat`` of
    activations, no location arithmetic, no softmax and no fp32 copies in framework operators.  Under autocast the core
    receives the values and the packed row in the autocast dtype and the reference in fp32.  ``reference_points``:
    ``[N, Lq, 1 or L, 4]`` boxes or ``[N, Lq, L, 2]`` points (which, unlike the parent's, need no equal point counts)."""

    def __init__(self, embed_dim=256, num_heads=8, num_levels=4, num_points=4, offset_scale=0.5, method="default"):
        super().__init__(embed_dim, num_heads, num_levels, num_points, offset_scale, method)
        self._core = anchored_deform_attn

    def fused_linear(self):
        """Weight ``[M * 3K, C]`` and bias ``[M * 3K]`` of the one linear whose output is the packed row."""
        M, K, C = self.num_heads, sum(self.num_points_list), self.embed_dim
        so, aw = self.sampling_offsets, self.attention_weights
        weight = torch.cat([so.weight.view(M, 2 * K, C), aw.weight.view(M, K, C)], 1).reshape(M * 3 * K, C)
        bias = torch.cat([so.bias.view(M, 2 * K), aw.bias.view(M, K)], 1).reshape(M * 3 * K)
        return weight, bias

    def forward(self, query, reference_points, value, value_spatial_shapes, value_mask=None):
        N, Lq, _ = query.shape
        L = self.num_levels
        shapes, value = self._values(value, value_spatial_shapes, value_mask)
        if reference_points.dim() != 4 or tuple(reference_points.shape[:2]) != (N, Lq) or \
                tuple(reference_points.shape[2:]) not in ((1, 4), (L, 4), (L, 2)):
            raise ValueError("reference_points must be [N, Lq, 1 or %d, 4] or [N, Lq, %d, 2], got %s" % (
                L, L, tuple(reference_points.shape)))
        weight, bias = self.fused_linear()
        offs_attn = F.linear(query, weight, bias).view(N, Lq, self.num_heads, 3 * sum(self.num_points_list))
        out = self._core(value, shapes, self.num_points_list, reference_points, offs_attn, self.offset_scale)
        return self.output_proj(out)
