"""Deformable aggregation on the MI355X-native backend: the ``deformable_aggregation`` operator of multi-camera 3-D
detectors (Sparse4D v2 / v3, SparseDrive) on channels-last tensors (include/mdconv_dagg.h; INTEGRATION.md, "Deformable
aggregation", has the contract and what is unpinned).

    deformable_aggregation_forward / deformable_aggregation_backward   the entry points on dense CUDA tensors
    DeformableAggregationFunction   autograd.Function over mdconv_dagg_forward / mdconv_dagg_backward
    deformable_aggregation          the functional form
    feature_maps_format             a list of per-level maps [B, cams, C, H_l, W_l] -> the operator's ``feature``

``feature [B, S, C]`` (the maps concatenated camera-major, level-minor, each y*W + x; every camera has the same level
extents), ``sampling_location [B, A, P, cams, 2]`` ((x, y), normalised), ``weights [B, A, P, cams, L, G]`` ->
``output [B, A, C]``.  A (b, a, p, cam) contributes iff 0 < x < 1 and 0 < y < 1.  ``feature`` is fp32 / fp16 / bf16; the two
coordinate tensors have its dtype or are fp32.  CPU tensors raise ``NotImplementedError``: there is no CPU or PyTorch
fallback.  There is no ``nn.Module``: the published module wraps camera projection and anchor encoding, which is model code.
"""
import functools

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _capi, _samp
from ._samp import DTYPES as _DTYPES, ptr as _ptr

__all__ = ["deformable_aggregation_forward", "deformable_aggregation_backward", "DeformableAggregationFunction",
           "deformable_aggregation", "feature_maps_format"]

_SAME_EXTENTS = "every camera must have the same level extents (H_l, W_l)"


def _shapes(spatial_shape):
    """``spatial_shape`` as a tuple of (H, W) ints per level: a sequence of (H, W), or the published ``[cams, levels, 2]``
    (tensor or nested sequence), whose cameras must agree.  A tensor is read with ``.tolist()``: for a CUDA tensor that is
    a host synchronisation (and impossible during graph capture) -- pass host data to avoid it."""
    if isinstance(spatial_shape, torch.Tensor):
        spatial_shape = spatial_shape.tolist()
    rows = [list(r) for r in spatial_shape]
    if rows and rows[0] and isinstance(rows[0][0], (list, tuple)):   # [cams][levels][2]
        per_cam = [tuple((int(h), int(w)) for h, w in cam) for cam in rows]
        if any(c != per_cam[0] for c in per_cam):
            raise ValueError("dagg: %s; got %s" % (_SAME_EXTENTS, per_cam))
        shapes = per_cam[0]
    else:
        shapes = tuple((int(h), int(w)) for h, w in rows)
    if not 1 <= len(shapes) <= _capi.MSDA_MAX_LEVELS:
        raise ValueError("dagg: 1..%d levels, got %d" % (_capi.MSDA_MAX_LEVELS, len(shapes)))
    return shapes


def _check_starts(shapes, cams, scale_start_index):
    """``scale_start_index`` is not an input of the operator (the starts are the cumulative sums); host data is checked
    against them -- ``[cams, levels]`` rows of ``feature``, or the ``levels`` starts of camera 0 --, a CUDA tensor is ignored
    rather than synchronised on."""
    if scale_start_index is None or (isinstance(scale_start_index, torch.Tensor) and scale_start_index.is_cuda):
        return
    got = scale_start_index.tolist() if isinstance(scale_start_index, torch.Tensor) else list(scale_start_index)
    got = [int(v) for row in got for v in (row if isinstance(row, (list, tuple)) else [row])]
    starts, s = _samp.level_starts(shapes)
    want = [c * s + st for c in range(cams) for st in starts]
    if got != want and got != starts:
        raise ValueError("dagg: scale_start_index %s is not the cumulative sum %s of spatial_shape over cameras and levels" % (
            got, want))


def _desc(feature, loc, weights, shapes, accumulate=1, flags=0):
    if feature.dtype not in _DTYPES or loc.dtype not in _DTYPES:
        raise TypeError("dagg: dtypes %s / %s are not float32, float16 or bfloat16" % (feature.dtype, loc.dtype))
    if feature.dim() != 3 or loc.dim() != 5 or weights.dim() != 6:
        raise ValueError("dagg: feature must be [B, S, C], sampling_location [B, A, P, cams, 2] and weights "
                         "[B, A, P, cams, L, G], got %s, %s and %s" % (tuple(feature.shape), tuple(loc.shape), tuple(weights.shape)))
    d = _capi.MdconvDaggDesc()
    d.dtype, d.coord_dtype = _DTYPES[feature.dtype], _DTYPES[loc.dtype]
    d.batch, d.channels = int(feature.shape[0]), int(feature.shape[2])
    d.anchors, d.points, d.cams = int(loc.shape[1]), int(loc.shape[2]), int(loc.shape[3])
    d.levels, d.groups = len(shapes), int(weights.shape[5])
    for l, (h, w) in enumerate(shapes):
        d.level_sz[l][0], d.level_sz[l][1] = h, w
    d.accumulate, d.flags = int(accumulate), int(flags)
    return d


def _check(d, shapes, feature, loc, weights, **others):
    """Shapes, dtypes, devices and density of the tensors of a call; ``others`` have the shape of ``output``."""
    B, C, A, P, cams, L, G = d.batch, d.channels, d.anchors, d.points, d.cams, d.levels, d.groups
    S = cams * sum(h * w for h, w in shapes)
    if G <= 0 or C % G:
        raise ValueError("dagg: the channels (%d) are not a multiple of the groups (%d, the last axis of weights)" % (C, G))
    want = dict(feature=(B, S, C), sampling_location=(B, A, P, cams, 2), weights=(B, A, P, cams, L, G))
    want.update({k: (B, A, C) for k in others})
    tensors = dict(feature=feature, sampling_location=loc, weights=weights, **others)
    for name, t in tensors.items():
        if tuple(t.shape) != want[name]:
            raise ValueError("dagg: %s must be %s, got %s (S = cams * sum of H_l * W_l: %s)" % (
                name, want[name], tuple(t.shape), _SAME_EXTENTS))
        like = loc if name in ("sampling_location", "weights") else feature
        if t.dtype != like.dtype or t.device != feature.device:
            raise ValueError("dagg: %s is %s on %s; feature is %s on %s and the coordinate tensors are %s (feature, output and "
                             "grad_output share one dtype, the two coordinate tensors another: the same, or float32)" % (
                                 name, t.dtype, t.device, feature.dtype, feature.device, loc.dtype))
        if not t.is_contiguous():
            raise ValueError("dagg: %s must be dense and row-major (contiguous)" % name)
    if loc.dtype != feature.dtype and loc.dtype != torch.float32:
        raise ValueError("dagg: the coordinate tensors are %s, feature is %s: they must have feature's dtype or float32" % (
            loc.dtype, feature.dtype))
    return (B, A, C)


# the call itself (the seam the tests replace): workspace query, allocation, current stream, call, RuntimeError
_run = functools.partial(_samp.run, "mdconv_dagg",
                         missing_msg="this build of libmdconv_hip.so has no deformable aggregation (mdconv_dagg_*)")


def deformable_aggregation_forward(feature, spatial_shape, sampling_location, weights, output=None):
    """The forward entry point on dense CUDA tensors; allocates ``output`` unless it is given."""
    shapes = _shapes(spatial_shape)
    d = _desc(feature, sampling_location, weights, shapes)
    others = {} if output is None else dict(output=output)
    shape = _check(d, shapes, feature, sampling_location, weights, **others)
    if not feature.is_cuda:
        raise NotImplementedError
    # pointer classes (include/mdconv_dagg.h): feature and output are "16-byte", the locations and weights "element"
    _capi.require_aligned_result("dagg", "output", output)
    feature = _capi.aligned_input(feature)
    if output is None:
        output = torch.empty(shape, dtype=feature.dtype, device=feature.device)
    _run("mdconv_dagg_forward", d, False, [_ptr(feature), _ptr(sampling_location), _ptr(weights), _ptr(output)], feature)
    return output


def deformable_aggregation_backward(feature, spatial_shape, sampling_location, weights, grad_output, grads=None,
                                    need_grad_feature=True, deterministic=False, accumulate=None):
    """The backward entry point.  ``grads`` = (grad_feature | None, grad_sampling_location, grad_weights): caller-allocated
    buffers the gradients are ADDED to; without it fresh tensors are written.  ``need_grad_feature`` false: grad_feature is
    neither computed nor allocated (``MDCONV_FLAG_NO_GRAD_INPUT``) and None is returned there.  ``deterministic`` None
    follows ``_capi.deterministic_mode()``.  ``accumulate`` false with ``grads``: the caller's buffers are overwritten
    instead.  Returns the three gradients in that order."""
    shapes = _shapes(spatial_shape)
    flags = _samp.backward_flags(deterministic, need_grad_feature)
    d = _desc(feature, sampling_location, weights, shapes,
              accumulate=int(grads is not None if accumulate is None else bool(accumulate)), flags=flags)
    _check(d, shapes, feature, sampling_location, weights, grad_output=grad_output)
    if not feature.is_cuda:
        raise NotImplementedError
    # pointer classes (include/mdconv_dagg.h): feature, grad_output and grad_feature are "16-byte", the coordinate tensors "element"
    if grads is not None and need_grad_feature:
        _capi.require_aligned_result("dagg", "grad_feature", grads[0])
    feature, grad_output = _capi.aligned_input(feature), _capi.aligned_input(grad_output)
    if grads is None:
        grads = (torch.empty_like(feature) if need_grad_feature else None, torch.empty_like(sampling_location),
                 torch.empty_like(weights))
    gf, gl, gw = grads
    _samp.check_grads("dagg", (("grad_feature", gf, feature), ("grad_sampling_location", gl, sampling_location), ("grad_weights", gw, weights)),
                      may_be_none=() if need_grad_feature else ("grad_feature",))
    _run("mdconv_dagg_backward", d, True,
         [_ptr(feature), _ptr(sampling_location), _ptr(weights), _ptr(grad_output), _ptr(gf if need_grad_feature else None),
          _ptr(gl), _ptr(gw)], feature)
    return (gf if need_grad_feature else None), gl, gw


class DeformableAggregationFunction(Function):
    """``DeformableAggregationFunction.apply(mc_ms_feat, spatial_shape, scale_start_index, sampling_location, weights)`` --
    the published argument order.  ``spatial_shape`` is a sequence of (H, W) per level or the published
    ``[cams, levels, 2]``, whose cameras must agree (``ValueError`` otherwise); a CUDA tensor costs a ``.tolist()``
    synchronisation per call and cannot be read during graph capture, so pass host data there.  ``scale_start_index`` is
    checked against the cumulative sums when it is host data (a wrong one raises ``ValueError``) and ignored otherwise.
    Under ``torch.autocast`` ``mc_ms_feat`` runs in the autocast dtype.  The two coordinate tensors run in ONE dtype: the
    feature's (after autocast) when both already have it, and fp32 in every other case -- either is fp32 (the mixed call),
    they disagree, or they are 16-bit of another kind than the feature (fp16 coordinates under bf16 autocast run in fp32: a
    coordinate is never converted from one 16-bit type to the other).  The gradients go back in the dtypes the caller's
    tensors have."""

    @staticmethod
    def forward(ctx, mc_ms_feat, spatial_shape, scale_start_index, sampling_location, weights):
        shapes = _shapes(spatial_shape)
        if sampling_location.dim() == 5:   # (before the device check: a wrong one is a ValueError on any device)
            _check_starts(shapes, int(sampling_location.shape[3]), scale_start_index)
        ctx.shapes = shapes
        ctx.in_dtypes = (mc_ms_feat.dtype, sampling_location.dtype, weights.dtype)
        if mc_ms_feat.is_cuda and torch.is_autocast_enabled("cuda"):
            mc_ms_feat = mc_ms_feat.to(torch.get_autocast_dtype("cuda"))
        # one dtype for the two coordinate tensors: fp32 if either is (or if they disagree), else the feature's
        cdt = _samp.coord_dtype(mc_ms_feat.dtype, sampling_location.dtype, weights.dtype)
        mc_ms_feat = mc_ms_feat.contiguous()
        sampling_location = sampling_location.to(cdt).contiguous()
        weights = weights.to(cdt).contiguous()
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(mc_ms_feat, sampling_location, weights)
        return deformable_aggregation_forward(mc_ms_feat, shapes, sampling_location, weights)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        if not grad_output.is_cuda:
            raise NotImplementedError
        feature, loc, weights = ctx.saved_tensors
        grad_output = grad_output.to(feature.dtype).contiguous()
        # selective backward: grad_feature is neither computed nor allocated when the feature needs no gradient
        gf, gl, gw = deformable_aggregation_backward(feature, ctx.shapes, loc, weights, grad_output,
                                                     need_grad_feature=bool(ctx.needs_input_grad[0]), deterministic=None)
        back = _samp.back
        df, dl, dw = ctx.in_dtypes
        return back(gf, df), None, None, back(gl, dl), back(gw, dw)


def deformable_aggregation(feature, spatial_shape, sampling_location, weights, scale_start_index=None):
    """Functional form of ``DeformableAggregationFunction``.  A ``feature`` that needs no gradient runs the backward with
    ``MDCONV_FLAG_NO_GRAD_INPUT``."""
    return DeformableAggregationFunction.apply(feature, spatial_shape, scale_start_index, sampling_location, weights)


def feature_maps_format(feature_maps):
    """A list of per-level maps ``[B, cams, C, H_l, W_l]`` -> ``(feature [B, S, C], spatial_shape, scale_start_index)``:
    the maps channels-last and concatenated camera-major, level-minor.  ``spatial_shape`` ``[cams, levels, 2]`` and
    ``scale_start_index`` ``[cams, levels]`` are int64 HOST tensors, so passing them on costs no synchronisation."""
    if not feature_maps or any(m.dim() != 5 or m.shape[:3] != feature_maps[0].shape[:3] for m in feature_maps):
        raise ValueError("dagg: feature_maps must be a non-empty list of [B, cams, C, H_l, W_l] tensors that agree in B, cams, C")
    B, cams, C = (int(v) for v in feature_maps[0].shape[:3])
    shapes = [(int(m.shape[3]), int(m.shape[4])) for m in feature_maps]
    feature = torch.cat([m.permute(0, 1, 3, 4, 2).reshape(B, cams, h * w, C) for m, (h, w) in zip(feature_maps, shapes)], 2)
    s_cam = int(feature.shape[2])
    starts, _ = _samp.level_starts(shapes)
    spatial_shape = torch.tensor([shapes] * cams, dtype=torch.int64)
    scale_start_index = torch.tensor([[c * s_cam + st for st in starts] for c in range(cams)], dtype=torch.int64)
    return feature.reshape(B, cams * s_cam, C).contiguous(), spatial_shape, scale_start_index
