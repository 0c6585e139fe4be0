"""Reference and inputs for packed deformable attention with a point count per level (include/mdconv_fdap.h), independent
of the kernels' formulas: unpack the tensor, ``torch.softmax`` in fp64 over the K logits of a (query, head) -- on the values
the tensor holds -- and hand locations and weights to the references of deformable attention with a point count per level
(``tests.msdap_ref``: ``msdap_ref`` on ``F.grid_sample``, ``msdap_direct`` on explicit corners).  The gradient of the
packed tensor is the two gradients of that reference, the weights' taken back through the fp64 softmax, packed again.

``make_inputs`` / ``make_lattice_inputs`` draw the tensors of a case on top of ``msdap_ref``'s -- the same values, locations
(with the ``MARGIN`` rule and the asserted conditions) and grad_output -- with logits ``randn * 3 + shift``."""
import torch

from tests import msdap_ref as MR

MARGIN = MR.MARGIN


def pack(loc, logits):
    """[N, Lq, M, K, 2] and [N, Lq, M, K] -> [N, Lq, M, 3K]: the (x, y) pairs in tap order, then the logits."""
    N, Lq, Mh = loc.shape[:3]
    return torch.cat([loc.reshape(N, Lq, Mh, -1), logits.reshape(N, Lq, Mh, -1)], -1).contiguous()


def unpack(loc_attn, points):
    """Views of the packed tensor: locations [N, Lq, M, K, 2] and logits [N, Lq, M, K]."""
    K = sum(int(p) for p in points)
    assert loc_attn.shape[-1] == 3 * K
    return loc_attn[..., :2 * K].unflatten(-1, (K, 2)), loc_attn[..., 2 * K:]


def weights(logits):
    """fp64 softmax over the K taps of each (query, head); differentiable."""
    return torch.softmax(logits.double(), -1)


def fdap_ref(value, shapes, points, loc_attn, fn=MR.msdap_ref):
    """fp64 output from the values the tensors hold; differentiable in ``value`` and ``loc_attn``."""
    loc, logits = unpack(loc_attn, points)
    return fn(value, shapes, points, loc, weights(logits))


def fdap_ref_grads(value, shapes, points, loc_attn, grad_output, fn=MR.msdap_ref):
    """(output, grad_value, grad_sampling_loc_attn) in fp64: ``msdap_ref_grads`` on the unpacked tensors with the fp64
    weights, the weights' gradient through the softmax, the two coordinate gradients packed again."""
    loc, logits = unpack(loc_attn.detach().double().cpu(), points)
    lg = logits.clone().requires_grad_(True)
    a = weights(lg)
    out, gv, gl, ga = MR.msdap_ref_grads(value, shapes, points, loc, a.detach(), grad_output, fn=fn)
    glogit, = torch.autograd.grad(a, lg, ga)
    return out, gv, pack(gl, glogit)


def _logits(N, Lq, M, K, coord_dtype, seed, shift):
    gen = torch.Generator().manual_seed(seed + 1000)
    return (torch.randn(N, Lq, M, K, generator=gen) * 3 + shift).to(coord_dtype)


def make_inputs(N, M, D, shapes, points, Lq, dtype=torch.float32, coord_dtype=None, seed=0, shift=0.0):
    """CPU tensors (value, sampling_loc_attn, grad_output): ``value`` and ``grad_output`` of ``dtype``, the packed tensor of
    ``coord_dtype`` (default: ``dtype``).  Values, locations and grad_output are those of ``msdap_ref.make_inputs`` for the
    same arguments (which asserts the margin per level); the logits are ``randn * 3 + shift`` rounded to the coordinate
    dtype."""
    coord_dtype = dtype if coord_dtype is None else coord_dtype
    value, loc, _, go = MR.make_inputs(N, M, D, shapes, points, Lq, dtype=dtype, coord_dtype=coord_dtype, seed=seed)
    assert MR.min_lattice_distance(loc, shapes, points) >= MARGIN
    return value, pack(loc, _logits(N, Lq, M, sum(points), coord_dtype, seed, shift)), go


def make_lattice_inputs(N, M, D, shapes, points, dtype=torch.float32, coord_dtype=None, seed=0, shift=0.0):
    """CPU tensors (value, sampling_loc_attn, grad_output) on top of ``msdap_ref.make_lattice_inputs`` -- every pixel
    coordinate an integer, its asserted conditions -- with the logits drawn as ``make_inputs`` draws them."""
    coord_dtype = dtype if coord_dtype is None else coord_dtype
    value, loc, _, go = MR.make_lattice_inputs(N, M, D, shapes, points, dtype=dtype, coord_dtype=coord_dtype, seed=seed)
    return value, pack(loc, _logits(N, loc.shape[1], M, sum(points), coord_dtype, seed, shift)), go
