"""Reference and inputs for packed deformable attention (include/mdconv.h, "Packed deformable attention"), independent of
the kernels' formulas: unpack the tensor, ``torch.softmax`` in fp64 over the L*P logits of a (query, head) -- on the values
the tensor holds -- and hand locations and weights to the references of multi-scale deformable attention
(``tests.msda_ref``: ``msda_ref`` on ``F.grid_sample``, ``msda_direct`` on explicit corners).  The gradient of the packed
tensor is the two gradients of that reference, the weights' taken back through the fp64 softmax, packed again.

``make_inputs`` draws the tensors of a case on top of ``msda_ref.make_inputs`` -- the same values, locations (with the
``MARGIN`` rule for gradient comparisons) and grad_output -- with logits ``randn * 3 + shift``."""
import torch

from tests import msda_ref as MR

MARGIN = MR.MARGIN


def pack(loc, logits):
    """[N, Lq, M, L, P, 2] and [N, Lq, M, L, P] -> [N, Lq, M, 3 * L * P]: the (x, y) pairs in tap order, then the logits."""
    N, Lq, Mh = loc.shape[:3]
    return torch.cat([loc.reshape(N, Lq, Mh, -1), logits.reshape(N, Lq, Mh, -1)], -1).contiguous()


def unpack(loc_attn, L, P):
    """Views of the packed tensor: locations [N, Lq, M, L, P, 2] and logits [N, Lq, M, L, P]."""
    K = L * P
    assert loc_attn.shape[-1] == 3 * K
    return loc_attn[..., :2 * K].unflatten(-1, (L, P, 2)), loc_attn[..., 2 * K:].unflatten(-1, (L, P))


def weights(logits):
    """fp64 softmax over the L*P taps of each (query, head); differentiable."""
    return torch.softmax(logits.double().flatten(-2), -1).view(logits.shape)


def fda_ref(value, shapes, loc_attn, P, fn=MR.msda_ref):
    """fp64 output from the values the tensors hold; differentiable in ``value`` and ``loc_attn``."""
    loc, logits = unpack(loc_attn, len(shapes), P)
    return fn(value, shapes, loc, weights(logits))


def fda_ref_grads(value, shapes, loc_attn, P, grad_output, fn=MR.msda_ref):
    """(output, grad_value, grad_sampling_loc_attn) in fp64: ``msda_ref_grads`` on the unpacked tensors with the fp64
    weights, the weights' gradient through the softmax, the two coordinate gradients packed again."""
    loc, logits = unpack(loc_attn.detach().double().cpu(), len(shapes), P)
    lg = logits.clone().requires_grad_(True)
    a = weights(lg)
    out, gv, gl, ga = MR.msda_ref_grads(value, shapes, loc, a.detach(), grad_output, fn=fn)
    glogit, = torch.autograd.grad(a, lg, ga)
    return out, gv, pack(gl, glogit)


def make_inputs(N, M, D, shapes, Lq, P, dtype=torch.float32, coord_dtype=None, seed=0, shift=0.0):
    """CPU tensors (value, sampling_loc_attn, grad_output): ``value`` and ``grad_output`` of ``dtype``, the packed tensor of
    ``coord_dtype`` (default: ``dtype``).  Values, locations and grad_output are those of ``msda_ref.make_inputs`` for the
    same arguments; the logits are ``randn * 3 + shift`` rounded to the coordinate dtype."""
    coord_dtype = dtype if coord_dtype is None else coord_dtype
    value, loc, _, go = MR.make_inputs(N, M, D, shapes, Lq, P, dtype=dtype, coord_dtype=coord_dtype, seed=seed)
    assert MR.min_lattice_distance(loc, shapes) >= MARGIN
    gen = torch.Generator().manual_seed(seed + 1000)
    logits = (torch.randn(N, Lq, M, len(shapes), P, generator=gen) * 3 + shift).to(coord_dtype)
    return value, pack(loc, logits), go


def make_lattice_inputs(N, M, D, shapes, P, dtype=torch.float32, coord_dtype=None, seed=0, shift=0.0):
    """CPU tensors (value, sampling_loc_attn, grad_output) on top of ``msda_ref.make_lattice_inputs`` -- every pixel
    coordinate an integer, its asserted conditions -- with the logits drawn as ``make_inputs`` draws them."""
    coord_dtype = dtype if coord_dtype is None else coord_dtype
    value, loc, _, go = MR.make_lattice_inputs(N, M, D, shapes, P, dtype=dtype, coord_dtype=coord_dtype, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1000)
    logits = (torch.randn(N, loc.shape[1], M, len(shapes), P, generator=gen) * 3 + shift).to(coord_dtype)
    return value, pack(loc, logits), go
