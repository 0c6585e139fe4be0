"""References for 3-D multi-scale deformable attention (include/mdconv.h, "3-D multi-scale deformable attention"),
independent of the kernels' formulas.

``msda3d_ref``: the plain-PyTorch composition -- ``F.grid_sample`` on 5-D input (zero padding, ``align_corners=False``) per
level, times the attention weights, summed over levels and points; gradients come from autograd.  ``msda3d_direct``: an
explicit eight-corner gather with the operator's gate, written from the contract.  ``make_inputs`` draws the tensors of a
case; for gradient comparisons no voxel coordinate may lie within ``MARGIN`` of an integer -- there the trilinear interpolant
has a kink and the reference's own derivative jumps -- which is a rule for the inputs (``min_lattice_distance`` measures
it), not an exclusion of elements.  ``spatial_shapes`` rows are (T, H, W); the last axis of the locations is (x, y, z)."""
import torch
import torch.nn.functional as F

MARGIN = 0.05


def level_starts(shapes):
    starts, s = [], 0
    for t, h, w in shapes:
        starts.append(s)
        s += t * h * w
    return starts, s


def _whd(shapes, device=None):
    """[L, 3] fp64: the extents in the order of the locations' last axis, (W, H, T)."""
    return torch.tensor([[w, h, t] for t, h, w in shapes], dtype=torch.float64, device=device)


def pixel_positions(loc, shapes):
    """(x, y, z) [N, Lq, M, L, P] in the voxel coordinates of each sample's level, fp64, straight from the contract."""
    loc = loc.double()
    pix = loc * _whd(shapes, loc.device)[None, None, None, :, None, :] - 0.5
    return pix[..., 0], pix[..., 1], pix[..., 2]


def min_lattice_distance(loc, shapes):
    """Smallest distance of any voxel coordinate to an integer."""
    d = torch.stack(pixel_positions(loc, shapes))
    return (d - d.round()).abs().min().item()


def gate_of(loc, shapes):
    """[N, Lq, M, L, P] bool: the sample passes the gate -1 < coordinate < size on all three axes."""
    x, y, z = pixel_positions(loc, shapes)
    s = _whd(shapes)[None, None, None, :, None, :]
    return (x > -1) & (y > -1) & (z > -1) & (x < s[..., 0]) & (y < s[..., 1]) & (z < s[..., 2])


def msda3d_ref(value, shapes, loc, attn, *_unused):
    """fp64 composition from ``F.grid_sample`` on [N*M, D, T, H, W]; differentiable.  Returns [N, Lq, M*D] in the dtype of
    ``value``."""
    shapes = [(int(t), int(h), int(w)) for t, h, w in shapes]
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    v, grids, a = value.double(), 2 * loc.double() - 1, attn.double()
    starts, total = level_starts(shapes)
    assert total == S and L == len(shapes)
    out = 0
    for l, (t, h, w) in enumerate(shapes):
        vol = v[:, starts[l]:starts[l] + t * h * w].permute(0, 2, 3, 1).reshape(N * M, D, t, h, w)
        grid = grids[:, :, :, l].permute(0, 2, 1, 3, 4).reshape(N * M, 1, Lq, P, 3)
        s = F.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=False)   # [N*M, D, 1, Lq, P]
        wgt = a[:, :, :, l].permute(0, 2, 1, 3).reshape(N * M, 1, Lq, P)
        out = out + (s[:, :, 0] * wgt).sum(-1)
    return out.view(N, M, D, Lq).permute(0, 3, 1, 2).reshape(N, Lq, M * D).to(value.dtype)


def msda3d_direct(value, shapes, loc, attn, *_unused):
    """fp64, the contract word for word: gate, eight neighbours, neighbours outside the level left out; differentiable."""
    shapes = [(int(t), int(h), int(w)) for t, h, w in shapes]
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    v, a = value.double(), attn.double()
    starts, _ = level_starts(shapes)
    n_idx = torch.arange(N, device=value.device).view(N, 1, 1, 1).expand(N, Lq, M, P)
    m_idx = torch.arange(M, device=value.device).view(1, 1, M, 1).expand(N, Lq, M, P)
    out = torch.zeros(N, Lq, M, D, dtype=torch.float64, device=value.device)
    for l, (t, h, w) in enumerate(shapes):
        x = loc[:, :, :, l, :, 0].double() * w - 0.5   # [N, Lq, M, P]
        y = loc[:, :, :, l, :, 1].double() * h - 0.5
        z = loc[:, :, :, l, :, 2].double() * t - 0.5
        gate = (x > -1) & (y > -1) & (z > -1) & (x < w) & (y < h) & (z < t)
        x0, y0, z0 = x.detach().floor(), y.detach().floor(), z.detach().floor()
        lx, ly, lz = x - x0, y - y0, z - z0
        for cz in (0, 1):
            for cy in (0, 1):
                for cx in (0, 1):
                    xi, yi, zi = (x0 + cx).long(), (y0 + cy).long(), (z0 + cz).long()
                    read = gate & (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h) & (zi >= 0) & (zi < t)
                    row = starts[l] + (zi.clamp(0, t - 1) * h + yi.clamp(0, h - 1)) * w + xi.clamp(0, w - 1)
                    wgt = (lz if cz else 1 - lz) * (ly if cy else 1 - ly) * (lx if cx else 1 - lx) * a[:, :, :, l]
                    wgt = torch.where(read, wgt, torch.zeros_like(wgt))
                    out = out + (v[n_idx, row, m_idx] * wgt[..., None]).sum(3)
    return out.reshape(N, Lq, M * D).to(value.dtype)


def msda3d_ref_grads(value, shapes, loc, attn, grad_output, fn=msda3d_ref):
    """(output, grad_value, grad_sampling_locations, grad_attention_weights) in fp64 from the values the tensors hold."""
    v, l, a = (t.detach().double().cpu().requires_grad_(True) for t in (value, loc, attn))
    out = fn(v, shapes, l, a)
    gv, gl, ga = torch.autograd.grad(out, (v, l, a), grad_output.detach().double().cpu())
    return out.detach(), gv, gl, ga


def make_inputs(N, M, D, shapes, Lq, P, dtype=torch.float32, coord_dtype=None, seed=0):
    """CPU tensors (value, sampling_locations, attention_weights, grad_output): ``value`` and ``grad_output`` of ``dtype``,
    the two coordinate tensors of ``coord_dtype`` (default: ``dtype``).  Locations are uniform in [-0.15, 1.15], then -- as
    the kernel sees them, rounded to the coordinate dtype -- nudged by 0.23 / size until every voxel coordinate on all three
    axes is at least MARGIN away from the lattice (asserted).  Attention weights are a softmax over the L*P taps of a head."""
    coord_dtype = dtype if coord_dtype is None else coord_dtype
    gen = torch.Generator().manual_seed(seed)
    L = len(shapes)
    _, S = level_starts(shapes)
    value = torch.randn(N, S, M, D, generator=gen).to(dtype)
    go = torch.randn(N, Lq, M * D, generator=gen).to(dtype)
    attn = F.softmax(torch.randn(N, Lq, M, L * P, generator=gen), -1).view(N, Lq, M, L, P).to(coord_dtype)
    loc = (torch.rand(N, Lq, M, L, P, 3, generator=gen) * 1.3 - 0.15).to(coord_dtype)
    whd = _whd(shapes)[None, None, None, :, None, :]
    for _ in range(8):
        pix = loc.double() * whd - 0.5
        near = (pix - pix.round()).abs() < 2 * MARGIN
        if not near.any():
            break
        loc = torch.where(near, loc.double() + 0.23 / whd, loc.double()).to(coord_dtype)
    assert min_lattice_distance(loc, shapes) >= MARGIN
    return value, loc, attn, go


# ---- on the lattice -------------------------------------------------------------------------------------------------
# At an integer voxel coordinate the operator's derivative is a convention (include/mdconv.h): the right-sided one of the
# cell floor(x), floor(y), floor(z), and zero for a sample the gate leaves out, -1 and size included.  ``msda3d_ref`` is no
# reference there (``F.grid_sample`` rounds to either side of the integer and has no gate at -1); ``msda3d_direct`` is.
def lattice_points(t, h, w, ulp_inside=False):
    """Normalised (x, y, z) triples on a level of power-of-two extents, where (i + 0.5) / size and back are exact: every
    coordinate i = -1 .. size of each axis -- both edges of the gate and one step beyond -- against every such coordinate of
    the next axis, with the third axis cycling through its own range (so each axis meets -1, size - 1 and size both with the
    others inside and with them outside).  ``ulp_inside`` (fp32 coordinates): plus one coordinate at -1 + one ulp per axis,
    the others inside, which reads voxel 0 of that axis with weight 2^-24 at full slope."""
    for s in (t, h, w):
        assert s & (s - 1) == 0, "power-of-two extents only: elsewhere loc * size - 0.5 is not exact"
    size = (w, h, t)   # by location axis: x, y, z
    pts = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        k = 0
        for ia in range(-1, size[a] + 1):
            for ib in range(-1, size[b] + 1):
                p = [0.0, 0.0, 0.0]
                p[a], p[b] = (ia + 0.5) / size[a], (ib + 0.5) / size[b]
                p[c] = ((k % size[c]) + 0.5) / size[c]   # inside
                k += 1
                pts.append(tuple(p))
    if ulp_inside:
        just_inside = torch.nextafter(torch.tensor(-1.0), torch.tensor(0.0)).item()
        for a in range(3):
            p = [(min(1, s - 1) + 0.5) / s for s in size]
            p[a] = (just_inside + 0.5) / size[a]
            pts.append(tuple(p))
    return pts


def make_lattice_inputs(N, M, D, shapes, P, dtype=torch.float32, coord_dtype=None, seed=0):
    """CPU tensors (value, sampling_locations, attention_weights, grad_output) as ``make_inputs`` draws them, every voxel
    coordinate an integer: point 0 of (query q, head m, level l) walks ``lattice_points`` of the level (index q + 3 m), the
    other points sit on voxels inside the level.  Lq is what the longest enumeration needs.  fp32 coordinates add the
    three "one ulp inside -1" points per level.  Asserted, as conditions on the inputs: every coordinate exact in the
    coordinate dtype, distance 0 everywhere but at those points, at least half of the samples inside the gate, and per level
    and axis a coordinate at -1, at size - 1 and at size."""
    coord_dtype = dtype if coord_dtype is None else coord_dtype
    gen = torch.Generator().manual_seed(seed)
    L = len(shapes)
    _, S = level_starts(shapes)
    pts = [lattice_points(t, h, w, coord_dtype == torch.float32) for t, h, w in shapes]
    Lq = max(len(p) for p in pts)
    value = torch.randn(N, S, M, D, generator=gen).to(dtype)
    go = torch.randn(N, Lq, M * D, generator=gen).to(dtype)
    attn = F.softmax(torch.randn(N, Lq, M, L * P, generator=gen), -1).view(N, Lq, M, L, P).to(coord_dtype)
    loc = torch.zeros(N, Lq, M, L, P, 3, dtype=torch.float64)
    for l, (t, h, w) in enumerate(shapes):
        for q in range(Lq):
            for m in range(M):
                loc[:, q, m, l, 0] = torch.tensor(pts[l][(q + 3 * m) % len(pts[l])], dtype=torch.float64)
        if P > 1:
            for a, s in enumerate((w, h, t)):
                i = torch.randint(0, s, (N, Lq, M, P - 1), generator=gen)
                loc[:, :, :, l, 1:, a] = (i + 0.5) / s
    assert torch.equal(loc.to(coord_dtype).double(), loc), "the locations are exact in the coordinate dtype"
    loc = loc.to(coord_dtype)
    pix = torch.stack(pixel_positions(loc, shapes), -1)
    off = (pix - pix.round()).abs() != 0
    n_ulp = 3 * L * N * M * -(-Lq // min(len(p) for p in pts)) if coord_dtype == torch.float32 else 0
    assert int(off.sum()) <= n_ulp and float((pix - pix.round()).abs().max()) <= 2.0 ** -24
    assert float(gate_of(loc, shapes).double().mean()) >= 0.5
    for l, (t, h, w) in enumerate(shapes):
        for a, size in ((0, w), (1, h), (2, t)):
            c = pix[:, :, :, l, :, a]
            assert bool((c == -1).any()) and bool((c == size - 1).any()) and bool((c == size).any()), (l, a)
    return value, loc, attn, go
