"""References for multi-scale deformable attention with a point count per level (include/mdconv_msdap.h), independent of
the kernels' formulas.

``msdap_ref``: the plain-PyTorch composition the published code runs -- the tap axis split by ``num_points_list``, one
``F.grid_sample`` (zero padding, ``align_corners=False``) per level, times the attention weights, summed; gradients come from
autograd.  ``msdap_direct``: a loop over the K taps, each an explicit four-corner gather with the operator's gate, written
from the contract; for tiny cases.  ``make_inputs`` draws the tensors of a case; as in tests/msda_ref.py no pixel coordinate
may lie within ``MARGIN`` px of an integer for a gradient comparison -- a rule for the inputs, measured per level by
``min_lattice_distance``."""
import torch
import torch.nn.functional as F

from tests.msda_ref import MARGIN, lattice_points, level_starts


def tap_levels(points):
    """The level of every tap, level-major: (3, 1, 2) -> [0, 0, 0, 1, 2, 2]."""
    return [l for l, p in enumerate(points) for _ in range(int(p))]


def _tap_wh(shapes, points, device=None):
    """[K, 2] fp64: (W, H) of the level of every tap."""
    return torch.tensor([[shapes[l][1], shapes[l][0]] for l in tap_levels(points)], dtype=torch.float64, device=device)


def pixel_positions(loc, shapes, points):
    """(x, y) [N, Lq, M, K] in the pixel coordinates of each tap's level, fp64, straight from the contract."""
    pix = loc.double() * _tap_wh(shapes, points, loc.device) - 0.5
    return pix[..., 0], pix[..., 1]


def min_lattice_distance(loc, shapes, points, level=None):
    """Smallest distance of any pixel coordinate (of the taps of ``level``, or of all) to an integer."""
    d = torch.stack(pixel_positions(loc, shapes, points))
    if level is not None:
        d = d[..., [k for k, l in enumerate(tap_levels(points)) if l == level]]
    return (d - d.round()).abs().min().item()


def gate_of(loc, shapes, points):
    """[N, Lq, M, K] bool: the sample passes the gate -1 < x < W_l, -1 < y < H_l."""
    x, y = pixel_positions(loc, shapes, points)
    wh = _tap_wh(shapes, points, loc.device)
    return (x > -1) & (y > -1) & (x < wh[:, 0]) & (y < wh[:, 1])


def msdap_ref(value, shapes, points, loc, attn):
    """fp64 composition from ``F.grid_sample``, one call per level; differentiable.  [N, Lq, M*D] in the dtype of ``value``."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    points = [int(p) for p in points]
    N, S, M, D = value.shape
    Lq, K = loc.shape[1], loc.shape[3]
    starts, total = level_starts(shapes)
    assert total == S and len(points) == len(shapes) and sum(points) == K and attn.shape == loc.shape[:-1]
    v = value.double()
    grids = (2 * loc.double() - 1).split(points, dim=3)
    weights = attn.double().split(points, dim=3)
    out = 0
    for l, (h, w) in enumerate(shapes):
        img = v[:, starts[l]:starts[l] + h * w].permute(0, 2, 3, 1).reshape(N * M, D, h, w)
        grid = grids[l].permute(0, 2, 1, 3, 4).reshape(N * M, Lq, points[l], 2)
        s = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)   # [N*M, D, Lq, P_l]
        wgt = weights[l].permute(0, 2, 1, 3).reshape(N * M, 1, Lq, points[l])
        out = out + (s * wgt).sum(-1)
    return out.view(N, M, D, Lq).permute(0, 3, 1, 2).reshape(N, Lq, M * D).to(value.dtype)


def msdap_direct(value, shapes, points, loc, attn):
    """fp64, the contract word for word, tap by tap: the tap's level from the running sum of the counts, the gate, four
    neighbours, neighbours outside the level left out; differentiable."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    N, S, M, D = value.shape
    Lq, K = loc.shape[1], loc.shape[3]
    v, a = value.double(), attn.double()
    starts, _ = level_starts(shapes)
    n_idx = torch.arange(N, device=value.device).view(N, 1, 1).expand(N, Lq, M)
    m_idx = torch.arange(M, device=value.device).view(1, 1, M).expand(N, Lq, M)
    out = torch.zeros(N, Lq, M, D, dtype=torch.float64, device=value.device)
    level, first = 0, 0
    for k in range(K):
        while k >= first + int(points[level]):
            first += int(points[level])
            level += 1
        h, w = shapes[level]
        x = loc[:, :, :, k, 0].double() * w - 0.5   # [N, Lq, M]
        y = loc[:, :, :, k, 1].double() * h - 0.5
        gate = (x > -1) & (y > -1) & (x < w) & (y < h)
        x0, y0 = x.detach().floor(), y.detach().floor()
        lx, ly = x - x0, y - y0
        for cy in (0, 1):
            for cx in (0, 1):
                xi, yi = (x0 + cx).long(), (y0 + cy).long()
                read = gate & (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
                row = starts[level] + yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)
                wgt = (ly if cy else 1 - ly) * (lx if cx else 1 - lx) * a[:, :, :, k]
                wgt = torch.where(read, wgt, torch.zeros_like(wgt))
                out = out + v[n_idx, row, m_idx] * wgt[..., None]
    return out.reshape(N, Lq, M * D).to(value.dtype)


def msdap_ref_grads(value, shapes, points, loc, attn, grad_output, fn=msdap_ref):
    """(output, grad_value, grad_sampling_locations, grad_attention_weights) in fp64 from the values the tensors hold."""
    v, l, a = (t.detach().double().cpu().requires_grad_(True) for t in (value, loc, attn))
    out = fn(v, shapes, points, l, a)
    gv, gl, ga = torch.autograd.grad(out, (v, l, a), grad_output.detach().double().cpu())
    return out.detach(), gv, gl, ga


def make_inputs(N, M, D, shapes, points, Lq, dtype=torch.float32, coord_dtype=None, seed=0):
    """CPU tensors (value, sampling_locations, attention_weights, grad_output): ``value`` and ``grad_output`` of ``dtype``,
    the two coordinate tensors of ``coord_dtype`` (default: ``dtype``).  Locations are uniform in [-0.15, 1.15], then -- as
    the kernel sees them, rounded to the coordinate dtype -- nudged by 0.23 / size until every pixel coordinate is at least
    MARGIN away from the lattice, which is asserted per level.  Attention weights are a softmax over the K taps of a head."""
    coord_dtype = dtype if coord_dtype is None else coord_dtype
    gen = torch.Generator().manual_seed(seed)
    K = sum(points)
    assert len(points) == len(shapes) and all(p > 0 for p in points)
    _, S = level_starts(shapes)
    value = torch.randn(N, S, M, D, generator=gen).to(dtype)
    go = torch.randn(N, Lq, M * D, generator=gen).to(dtype)
    attn = F.softmax(torch.randn(N, Lq, M, K, generator=gen), -1).to(coord_dtype)
    loc = (torch.rand(N, Lq, M, K, 2, generator=gen) * 1.3 - 0.15).to(coord_dtype)
    wh = _tap_wh(shapes, points)
    for _ in range(8):
        pix = loc.double() * wh - 0.5
        near = (pix - pix.round()).abs() < 2 * MARGIN
        if not near.any():
            break
        loc = torch.where(near, loc.double() + 0.23 / wh, loc.double()).to(coord_dtype)
    for l in range(len(shapes)):
        assert min_lattice_distance(loc, shapes, points, level=l) >= MARGIN, l
    return value, loc, attn, go


def make_lattice_inputs(N, M, D, shapes, points, dtype=torch.float32, coord_dtype=None, seed=0):
    """CPU tensors as ``make_inputs`` draws them, every pixel coordinate an integer, built per level in the manner of
    ``tests.msda_ref.make_lattice_inputs``: the first tap of (query q, head m, level l) walks ``lattice_points`` of the level
    (index q + 3 m), the level's other taps sit on pixels inside it.  Lq is what the longest enumeration needs.  fp32
    coordinates add the two "one ulp inside -1" points per level.  Asserted, as conditions on the inputs: at least half of
    the samples inside the gate, and per level a coordinate at -1, at size - 1 and at size."""
    coord_dtype = dtype if coord_dtype is None else coord_dtype
    gen = torch.Generator().manual_seed(seed)
    K = sum(points)
    _, S = level_starts(shapes)
    pts = [lattice_points(h, w, coord_dtype == torch.float32) for h, w in shapes]
    Lq = max(len(p) for p in pts)
    value = torch.randn(N, S, M, D, generator=gen).to(dtype)
    go = torch.randn(N, Lq, M * D, generator=gen).to(dtype)
    attn = F.softmax(torch.randn(N, Lq, M, K, generator=gen), -1).to(coord_dtype)
    loc = torch.zeros(N, Lq, M, K, 2, dtype=torch.float64)
    first = 0
    for l, (h, w) in enumerate(shapes):
        for q in range(Lq):
            for m in range(M):
                loc[:, q, m, first] = torch.tensor(pts[l][(q + 3 * m) % len(pts[l])], dtype=torch.float64)
        more = points[l] - 1
        if more:
            ix = torch.randint(0, w, (N, Lq, M, more), generator=gen)
            iy = torch.randint(0, h, (N, Lq, M, more), generator=gen)
            loc[:, :, :, first + 1:first + points[l], 0] = (ix + 0.5) / w
            loc[:, :, :, first + 1:first + points[l], 1] = (iy + 0.5) / h
        first += points[l]
    assert torch.equal(loc.to(coord_dtype).double(), loc), "the locations are exact in the coordinate dtype"
    loc = loc.to(coord_dtype)
    x, y = pixel_positions(loc, shapes, points)
    pix = torch.stack([x, y], -1)
    assert float((pix - pix.round()).abs().max()) <= 2.0 ** -24
    assert float(gate_of(loc, shapes, points).double().mean()) >= 0.5
    levels = tap_levels(points)
    for l, (h, w) in enumerate(shapes):
        taps = [k for k, lv in enumerate(levels) if lv == l]
        for a, size in ((0, w), (1, h)):
            c = pix[:, :, :, taps, a]
            assert bool((c == -1).any()) and bool((c == size - 1).any()) and bool((c == size).any()), (l, a)
    return value, loc, attn, go
