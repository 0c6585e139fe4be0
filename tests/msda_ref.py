"""References for multi-scale deformable attention (include/mdconv.h, "Multi-scale deformable attention"), independent
of the kernels' formulas.

``msda_ref``: the plain-PyTorch composition -- ``F.grid_sample`` (zero padding, ``align_corners=False``) per level, times
the attention weights, summed over levels and points; gradients come from autograd.  ``msda_direct``: an explicit
four-corner gather with the operator's gate, written from the contract.  ``make_inputs`` draws the tensors of a case; for
gradient comparisons no pixel coordinate may lie within ``MARGIN`` px of an integer -- there the bilinear interpolant has
a kink and the reference's own derivative jumps -- which is a rule for the inputs (``min_lattice_distance`` measures it),
not an exclusion of elements."""
import torch
import torch.nn.functional as F

MARGIN = 0.05


def level_starts(shapes):
    starts, s = [], 0
    for h, w in shapes:
        starts.append(s)
        s += h * w
    return starts, s


def pixel_positions(loc, shapes):
    """(x, y) [N, Lq, M, L, P] in the pixel coordinates of each sample's level, fp64, straight from the contract."""
    loc = loc.double()
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64, device=loc.device)
    pix = loc * wh[None, None, None, :, None, :] - 0.5
    return pix[..., 0], pix[..., 1]


def min_lattice_distance(loc, shapes):
    """Smallest distance of any pixel coordinate to an integer."""
    d = torch.stack(pixel_positions(loc, shapes))
    return (d - d.round()).abs().min().item()


def msda_ref(value, shapes, loc, attn, *_unused):
    """fp64 composition from ``F.grid_sample``; differentiable.  Returns [N, Lq, M*D] in the dtype of ``value``."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    v, grids, a = value.double(), 2 * loc.double() - 1, attn.double()
    starts, total = level_starts(shapes)
    assert total == S and L == len(shapes)
    out = 0
    for l, (h, w) in enumerate(shapes):
        img = v[:, starts[l]:starts[l] + h * w].permute(0, 2, 3, 1).reshape(N * M, D, h, w)
        grid = grids[:, :, :, l].permute(0, 2, 1, 3, 4).reshape(N * M, Lq, P, 2)
        s = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)   # [N*M, D, Lq, P]
        wgt = a[:, :, :, l].permute(0, 2, 1, 3).reshape(N * M, 1, Lq, P)
        out = out + (s * wgt).sum(-1)
    return out.view(N, M, D, Lq).permute(0, 3, 1, 2).reshape(N, Lq, M * D).to(value.dtype)


def msda_direct(value, shapes, loc, attn):
    """fp64, the contract word for word: gate, four neighbours, neighbours outside the level left out; differentiable."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    v, a = value.double(), attn.double()
    starts, _ = level_starts(shapes)
    n_idx = torch.arange(N).view(N, 1, 1, 1).expand(N, Lq, M, P)
    m_idx = torch.arange(M).view(1, 1, M, 1).expand(N, Lq, M, P)
    out = torch.zeros(N, Lq, M, D, dtype=torch.float64)
    for l, (h, w) in enumerate(shapes):
        x = loc[:, :, :, l, :, 0].double() * w - 0.5   # [N, Lq, M, P]
        y = loc[:, :, :, l, :, 1].double() * h - 0.5
        gate = (x > -1) & (y > -1) & (x < w) & (y < h)
        x0, y0 = x.detach().floor(), y.detach().floor()
        lx, ly = x - x0, y - y0
        for cy in (0, 1):
            for cx in (0, 1):
                xi, yi = (x0 + cx).long(), (y0 + cy).long()
                read = gate & (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
                row = starts[l] + yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)
                wgt = (ly if cy else 1 - ly) * (lx if cx else 1 - lx) * a[:, :, :, l]
                wgt = torch.where(read, wgt, torch.zeros_like(wgt))
                out = out + (v[n_idx, row, m_idx] * wgt[..., None]).sum(3)
    return out.reshape(N, Lq, M * D).to(value.dtype)


def msda_ref_grads(value, shapes, loc, attn, grad_output, fn=msda_ref):
    """(output, grad_value, grad_sampling_locations, grad_attention_weights) in fp64 from the values the tensors hold."""
    v, l, a = (t.detach().double().cpu().requires_grad_(True) for t in (value, loc, attn))
    out = fn(v, shapes, l, a)
    gv, gl, ga = torch.autograd.grad(out, (v, l, a), grad_output.detach().double().cpu())
    return out.detach(), gv, gl, ga


def make_inputs(N, M, D, shapes, Lq, P, dtype=torch.float32, coord_dtype=None, seed=0):
    """CPU tensors (value, sampling_locations, attention_weights, grad_output): ``value`` and ``grad_output`` of ``dtype``,
    the two coordinate tensors of ``coord_dtype`` (default: ``dtype``).  Locations are uniform in [-0.15, 1.15], then -- as
    the kernel sees them, rounded to the coordinate dtype -- nudged by 0.23 / size until every pixel coordinate is at least
    MARGIN away from the lattice.  Attention weights are a softmax over the L*P taps of a head."""
    coord_dtype = dtype if coord_dtype is None else coord_dtype
    gen = torch.Generator().manual_seed(seed)
    L = len(shapes)
    _, S = level_starts(shapes)
    value = torch.randn(N, S, M, D, generator=gen).to(dtype)
    go = torch.randn(N, Lq, M * D, generator=gen).to(dtype)
    attn = F.softmax(torch.randn(N, Lq, M, L * P, generator=gen), -1).view(N, Lq, M, L, P).to(coord_dtype)
    loc = (torch.rand(N, Lq, M, L, P, 2, generator=gen) * 1.3 - 0.15).to(coord_dtype)
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)[None, None, None, :, None, :]
    for _ in range(8):
        pix = loc.double() * wh - 0.5
        near = (pix - pix.round()).abs() < 2 * MARGIN
        if not near.any():
            break
        loc = torch.where(near, loc.double() + 0.23 / wh, loc.double()).to(coord_dtype)
    assert min_lattice_distance(loc, shapes) >= MARGIN
    return value, loc, attn, go
