"""Reference and inputs for anchored packed deformable attention (include/mdconv_afda.h), independent of the kernels'
formulas: in fp64, from the values the tensors hold, the sampling locations by the published formulas in torch operators --
``reference + offsets * (1 / points) * wh * offset_scale`` for boxes, ``reference + offsets / (W, H)`` for points --, then the
reference of the packed operator (``tests.fdap_ref``: fp64 softmax, ``msdap_ref`` on ``F.grid_sample`` or ``msdap_direct`` on
explicit corners).  All three gradients come from autograd, grad_reference included.

``make_inputs`` draws the tensors of a case: boxes with centres in [0.2, 0.8] and sizes in [0.1, 0.4], offsets such that the
derived locations are ``msdap_ref.make_inputs``-like (uniform in [-0.15, 1.15], the ``MARGIN`` rule asserted per level on
the locations DERIVED from the rounded offsets, a gate that is neither all true nor all false), logits ``randn * 3 + shift``."""
import torch

from tests import fdap_ref as FR
from tests import msdap_ref as MR

MARGIN = MR.MARGIN


def tap_scales(ref, shapes, points, offset_scale):
    """fp64 [N, Lq, 1, K, 2] reference (x, y) of every tap and the factor its offsets are multiplied by, by the published
    formulas; differentiable in ``ref`` [N, Lq, Lr, R]."""
    L, K = len(shapes), sum(points)
    ref = ref.double()
    Lr, R = ref.shape[2], ref.shape[3]
    assert Lr in (1, L) and R in (2, 4)
    levels = torch.tensor(MR.tap_levels(points), device=ref.device)
    rows = ref[:, :, levels if Lr == L else torch.zeros_like(levels)]   # [N, Lq, K, R]
    if R == 4:
        num_points_scale = torch.tensor([1.0 / points[l] for l in MR.tap_levels(points)], dtype=torch.float64, device=ref.device)
        scale = num_points_scale[None, None, :, None] * rows[..., 2:] * float(offset_scale)
    else:
        scale = (1.0 / MR._tap_wh(shapes, points, ref.device))[None, None].expand(ref.shape[0], ref.shape[1], K, 2)
    return rows[:, :, None, :, :2], scale[:, :, None]


def locations(ref, shapes, points, offs, offset_scale=0.5):
    """fp64 sampling locations [N, Lq, M, K, 2] from the reference [N, Lq, Lr, R] and the offsets [N, Lq, M, K, 2]."""
    centre, scale = tap_scales(ref, shapes, points, offset_scale)
    return centre + offs.double() * scale


def afda_ref(value, shapes, points, ref, offs_attn, offset_scale=0.5, fn=MR.msdap_ref):
    """fp64 output from the values the tensors hold; differentiable in ``value``, ``ref`` and ``offs_attn``.  (The argument
    order of the operator's functional form: it can stand in for the module's core.)"""
    shapes = [(int(h), int(w)) for h, w in shapes]
    points = [int(p) for p in points]
    offs, logits = FR.unpack(offs_attn, points)
    loc = locations(ref, shapes, points, offs, offset_scale)
    out = fn(value.double(), shapes, points, loc, FR.weights(logits))
    return out.to(value.dtype)


def afda_ref_grads(value, shapes, points, ref, offs_attn, grad_output, offset_scale=0.5, fn=MR.msdap_ref):
    """(output, grad_value, grad_reference, grad_offs_attn) in fp64, by autograd through the whole composition."""
    v, r, oa = (t.detach().double().cpu().requires_grad_(True) for t in (value, ref, offs_attn))
    out = afda_ref(v, shapes, points, r, oa, offset_scale, fn=fn)
    gv, gr, goa = torch.autograd.grad(out, (v, r, oa), grad_output.detach().double().cpu())
    return out.detach(), gv, gr, goa


def derived(ref, shapes, points, offs_attn, offset_scale=0.5):
    """The fp64 locations the tensors of a call stand for (what ``min_lattice_distance`` and ``gate_of`` are asked about)."""
    return locations(ref, shapes, points, FR.unpack(offs_attn, points)[0], offset_scale).detach()


def make_refs(N, Lq, Lr, R, gen):
    """fp32 [N, Lq, Lr, R]: centres in [0.2, 0.8], sizes in [0.1, 0.4]."""
    centres = torch.rand(N, Lq, Lr, 2, generator=gen) * 0.6 + 0.2
    if R == 2:
        return centres.float()
    return torch.cat([centres, torch.rand(N, Lq, Lr, 2, generator=gen) * 0.3 + 0.1], -1).float()


def make_inputs(N, M, D, shapes, points, Lq, Lr=1, R=4, dtype=torch.float32, coord_dtype=None, seed=0, shift=0.0,
                offset_scale=0.5):
    """CPU tensors (value, reference_points, offs_attn, grad_output): ``value`` and ``grad_output`` of ``dtype``, the packed
    tensor of ``coord_dtype`` (default: ``dtype``), the reference fp32.  ``Lr``: 1, or any other number for "one row per
    level".  The offsets are what brings a location drawn uniformly in [-0.15, 1.15] about, ROUNDED to the coordinate dtype,
    and then -- as the kernel sees them -- nudged by 0.23 px until every derived pixel coordinate is at least MARGIN away
    from the lattice, which is asserted per level, as is a gate that is neither all true nor all false."""
    coord_dtype = dtype if coord_dtype is None else coord_dtype
    Lr = 1 if Lr == 1 else len(shapes)
    gen = torch.Generator().manual_seed(seed)
    K = sum(points)
    _, S = MR.level_starts(shapes)
    value = torch.randn(N, S, M, D, generator=gen).to(dtype)
    go = torch.randn(N, Lq, M * D, generator=gen).to(dtype)
    ref = make_refs(N, Lq, Lr, R, gen)
    target = torch.rand(N, Lq, M, K, 2, generator=gen, dtype=torch.float64) * 1.3 - 0.15
    wh = MR._tap_wh(shapes, points)
    # (the gate is neither all true nor all false whatever was drawn: the first tap of all sits at pixel (0.3, 0.3) of its
    # level, the last at (W + 0.5, 0.3) of its own)
    target[0, 0, 0, 0] = torch.tensor([0.8, 0.8], dtype=torch.float64) / wh[0]
    target[-1, -1, -1, -1] = torch.stack([wh[-1, 0] + 1.0, torch.tensor(0.8, dtype=torch.float64)]) / wh[-1]
    centre, scale = tap_scales(ref, shapes, points, offset_scale)
    offs = ((target - centre) / scale).to(coord_dtype)
    for _ in range(8):
        pix = (centre + offs.double() * scale) * wh - 0.5
        near = (pix - pix.round()).abs() < 2 * MARGIN
        if not near.any():
            break
        offs = torch.where(near, offs.double() + 0.23 / wh / scale, offs.double()).to(coord_dtype)
    offs_attn = FR.pack(offs, FR._logits(N, Lq, M, K, coord_dtype, seed, shift))
    check_inputs(ref, shapes, points, offs_attn, offset_scale)
    return value, ref, offs_attn, go


def check_inputs(ref, shapes, points, offs_attn, offset_scale=0.5):
    """The two conditions on the inputs of a gradient comparison, on the locations derived from the tensors as they are."""
    loc = derived(ref, shapes, points, offs_attn, offset_scale)
    for l in range(len(shapes)):
        assert MR.min_lattice_distance(loc, shapes, points, level=l) >= MARGIN, l
    gate = MR.gate_of(loc, shapes, points)
    assert bool(gate.any()) and not bool(gate.all())


def make_lattice_inputs(N, M, D, shapes, points, dtype=torch.float32, coord_dtype=None, seed=0, shift=0.0):
    """CPU tensors (value, reference_points [N, Lq, L, 2], offs_attn, grad_output) with every pixel coordinate an exact
    integer: the targets are ``msdap_ref.make_lattice_inputs``' (both edges of the gate per level, asserted there; without
    its two "one ulp inside" points, which no integer offset reaches), the reference of (image, query, level) is
    ``(c + 0.5) / extent`` of a pixel c inside the level and the offsets are the integer differences.  Power-of-two extents,
    so ``reference + offset / extent`` and ``* extent - 0.5`` are exact in fp32."""
    coord_dtype = dtype if coord_dtype is None else coord_dtype
    value, loc, _, go = MR.make_lattice_inputs(N, M, D, shapes, points, dtype=dtype, coord_dtype=torch.float16, seed=seed)
    Lq, K = loc.shape[1], sum(points)
    gen = torch.Generator().manual_seed(seed + 77)
    wh = MR._tap_wh(shapes, points)
    pix = loc.double() * wh - 0.5
    assert torch.equal(pix, pix.round())
    cells = torch.stack([torch.stack([torch.randint(0, w, (N, Lq), generator=gen), torch.randint(0, h, (N, Lq), generator=gen)], -1)
                         for h, w in shapes], 2).double()   # [N, Lq, L, 2] (x, y)
    lwh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)
    ref = ((cells + 0.5) / lwh).float()
    assert torch.equal(ref.double(), (cells + 0.5) / lwh)
    levels = torch.tensor(MR.tap_levels(points))
    offs = pix - cells[:, :, None, levels]
    assert torch.equal(offs.to(coord_dtype).double(), offs)
    offs_attn = FR.pack(offs.to(coord_dtype), FR._logits(N, Lq, M, K, coord_dtype, seed, shift))
    assert torch.equal(derived(ref, shapes, points, offs_attn) * wh - 0.5, pix)
    return value, ref, offs_attn, go
