"""What the wrappers of the sampling operators (dcnv3, dcnv4, msda, fda, droi, msda3d, dagg) share around their C entry
points: the dtype table, the call itself with its workspace, and the small rules of the backward entry points and the
autograd Functions.  Descriptors, tensor checks and their texts stay with each operator."""
import ctypes
import math

import torch

from . import _capi

DTYPES = {torch.float32: _capi.F32, torch.float16: _capi.F16, torch.bfloat16: _capi.BF16}


def ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def run(prefix, fn_name, desc, backward, args, like, missing_msg=None):
    """``fn_name(desc, *args, workspace, workspace_bytes, stream)`` -- an entry point of the operator ``prefix``
    (``"mdconv_msda"``) -- on the device and current stream of ``like``, with the workspace ``<prefix>_workspace_bytes`` asks
    for.  ``missing_msg``: the ``RuntimeError`` of a library built before the operator existed (``MDCONV_LIB``).  Each wrapper
    binds its prefix once (``_run = functools.partial(run, prefix)``): that name is the seam the tests replace."""
    L = _capi.lib()
    if missing_msg is not None and not hasattr(L, prefix + "_workspace_bytes"):
        raise RuntimeError(missing_msg)
    with torch.cuda.device(like.device):
        ws_bytes = getattr(L, prefix + "_workspace_bytes")(ctypes.byref(desc), int(backward))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=like.device) if ws_bytes else None
        stream = torch.cuda.current_stream().cuda_stream
        rc = getattr(L, fn_name)(ctypes.byref(desc), *args, ptr(ws), ctypes.c_size_t(ws_bytes), ctypes.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (fn_name, rc, _capi.last_error()))


def backward_flags(deterministic, need_grad):
    """The flags word of a backward: ``deterministic`` None follows ``_capi.deterministic_mode()``; ``need_grad`` false
    leaves the sampled tensor's gradient out (``MDCONV_FLAG_NO_GRAD_INPUT``)."""
    det = _capi.deterministic_mode() if deterministic is None else bool(deterministic)
    return (_capi.FLAG_DETERMINISTIC if det else 0) | (0 if need_grad else _capi.FLAG_NO_GRAD_INPUT)


def check_grads(op, triples, may_be_none=()):
    """``triples`` of (name, gradient buffer, its forward tensor); a name in ``may_be_none`` may have no buffer."""
    for name, g, like in triples:
        if g is None and name in may_be_none:
            continue
        if g is None or g.shape != like.shape or g.dtype != like.dtype or g.device != like.device or not g.is_contiguous():
            raise ValueError("%s: %s must be a dense tensor of the shape, dtype and device of its forward tensor" % (op, name))


def back(g, dtype):
    """A gradient on its way out of an autograd Function: in the dtype the caller's tensor has."""
    return g if g is None or g.dtype == dtype else g.to(dtype)


def coord_dtype(value_dtype, *coord_dtypes):
    """One dtype for the coordinate tensors of a call: the values' when every one has it, else fp32."""
    return value_dtype if all(c == value_dtype for c in coord_dtypes) else torch.float32


def level_starts(shapes):
    """(start row of every level, rows of all levels) of ``shapes``, rows of (H, W) or (T, H, W)."""
    starts, s = [], 0
    for sz in shapes:
        starts.append(s)
        s += math.prod(sz)
    return starts, s
