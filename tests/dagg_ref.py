"""References for deformable aggregation (include/mdconv_dagg.h), independent of the kernels' formulas.

``dagg_ref``: the plain-PyTorch composition -- ``F.grid_sample`` (zero padding, ``align_corners=False``) per (camera,
level) at ``grid = 2 * loc - 1``, times the gate and the group's weight, summed over points, cameras and levels; gradients
come from autograd.  ``dagg_direct``: an explicit four-corner gather written from the contract.  ``make_inputs`` draws the
tensors of a case; for gradient comparisons no pixel coordinate may lie within ``MARGIN`` px of an integer on ANY level that
shares the location -- there the bilinear interpolant has a kink and the reference's own derivative jumps -- which is a rule
for the inputs (``min_lattice_distance`` measures it), not an exclusion of elements."""
import torch
import torch.nn.functional as F

MARGIN = 0.05


def level_starts(shapes):
    starts, s = [], 0
    for h, w in shapes:
        starts.append(s)
        s += h * w
    return starts, s


def gate_of(loc):
    """[B, A, P, cams] bool: 0 < x < 1 and 0 < y < 1 on the stored elements (NaN, Inf, 0.0 and 1.0 are out)."""
    x, y = loc[..., 0].double(), loc[..., 1].double()
    return (x > 0) & (x < 1) & (y > 0) & (y < 1)


def pixel_positions(loc, shapes):
    """[B, A, P, cams, L, 2]: (x, y) in the pixel coordinates of every level that shares the location, fp64."""
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64, device=loc.device)
    return loc.double()[..., None, :] * wh - 0.5


def min_lattice_distance(loc, shapes):
    """Smallest distance of any pixel coordinate, on any level, to an integer."""
    d = pixel_positions(loc, shapes)
    return (d - d.round()).abs().min().item()


def _prepare(feature, shapes, loc, weights):
    """``dagg_ref``'s own reading of the tensors (``dagg_direct`` does not use it)."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    B, S, C = feature.shape
    A, P, cams = loc.shape[1:4]
    L, G = weights.shape[4:]
    starts, s_cam = level_starts(shapes)
    assert S == cams * s_cam and L == len(shapes) and C % G == 0
    gate = gate_of(loc.detach())
    # a gated-out location and its weights reach nothing, in value or in gradient (torch.where cuts the graph there)
    safe_loc = torch.where(gate[..., None], loc.double(), torch.full_like(loc.double(), 0.5))
    safe_w = torch.where(gate[..., None, None], weights.double(), torch.zeros_like(weights.double()))
    return shapes, (B, S, C, A, P, cams, L, G), starts, s_cam, gate, safe_loc, safe_w


def dagg_ref(feature, shapes, loc, weights, *_unused):
    """fp64 composition from ``F.grid_sample``; differentiable.  Returns [B, A, C] in the dtype of ``feature``."""
    shapes, (B, S, C, A, P, cams, L, G), starts, s_cam, gate, safe_loc, safe_w = _prepare(feature, shapes, loc, weights)
    f = feature.double()
    out = 0
    for cam in range(cams):
        grid = 2 * safe_loc[:, :, :, cam] - 1   # [B, A, P, 2]
        for l, (h, w) in enumerate(shapes):
            r0 = cam * s_cam + starts[l]
            img = f[:, r0:r0 + h * w].permute(0, 2, 1).reshape(B, C, h, w)
            s = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)   # [B, C, A, P]
            wgt = safe_w[:, :, :, cam, l].permute(0, 3, 1, 2).repeat_interleave(C // G, 1)             # [B, C, A, P]
            out = out + (s * wgt).sum(-1)
    return out.permute(0, 2, 1).to(feature.dtype)


def dagg_direct(feature, shapes, loc, weights):
    """fp64, the contract word for word, sharing no code with ``dagg_ref`` -- the gate included: the (b, a, p, cam) that pass
    0 < x < 1 and 0 < y < 1 are picked out of the raw tensors by index, and only they are ever looked at (so a gated-out
    location or weight, NaN or not, reaches neither a value nor a gradient); four neighbours each, neighbours outside the
    map left out; summed into their anchor's row.  Differentiable."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    B, S, C = feature.shape
    A, cams = loc.shape[1], loc.shape[3]
    G = weights.shape[5]
    starts, s_cam = level_starts(shapes)
    assert S == cams * s_cam and weights.shape[4] == len(shapes) and C % G == 0
    f, lc, wt = feature.double(), loc.double(), weights.double()
    with torch.no_grad():
        b, a, p, cam = ((lc[..., 0] > 0) & (lc[..., 0] < 1) & (lc[..., 1] > 0) & (lc[..., 1] < 1)).nonzero(as_tuple=True)
    xs, ys, ws = lc[b, a, p, cam, 0], lc[b, a, p, cam, 1], wt[b, a, p, cam]   # [T], [T], [T, L, G]
    out = torch.zeros(B * A, C, dtype=torch.float64, device=feature.device)
    for l, (h, w) in enumerate(shapes):
        x, y = xs * w - 0.5, ys * h - 0.5
        x0, y0 = x.detach().floor(), y.detach().floor()
        lx, ly = x - x0, y - y0
        wg = ws[:, l].repeat_interleave(C // G, -1)   # [T, C]
        for cy in (0, 1):
            for cx in (0, 1):
                xi, yi = (x0 + cx).long(), (y0 + cy).long()
                read = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
                row = cam * s_cam + starts[l] + yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)
                cw = (ly if cy else 1 - ly) * (lx if cx else 1 - lx)
                cw = torch.where(read, cw, torch.zeros_like(cw))
                out = out.index_add(0, b * A + a, f[b, row] * wg * cw[:, None])
    return out.view(B, A, C).to(feature.dtype)


def dagg_ref_grads(feature, shapes, loc, weights, grad_output, fn=dagg_ref):
    """(output, grad_feature, grad_sampling_location, grad_weights) in fp64 from the values the tensors hold."""
    f, l, w = (t.detach().double().cpu().requires_grad_(True) for t in (feature, loc, weights))
    out = fn(f, shapes, l, w)
    gf, gl, gw = torch.autograd.grad(out, (f, l, w), grad_output.detach().double().cpu(), allow_unused=True)
    gl = torch.zeros_like(l) if gl is None else gl
    gw = torch.zeros_like(w) if gw is None else gw
    return out.detach(), gf, gl, gw


def make_inputs(B, A, P, cams, shapes, G, Dg, dtype=torch.float32, coord_dtype=None, seed=0):
    """CPU tensors (feature, sampling_location, weights, grad_output): ``feature`` and ``grad_output`` of ``dtype``, the two
    coordinate tensors of ``coord_dtype`` (default: ``dtype``).  Locations are uniform in [-0.15, 1.15] -- about 59 % of the
    (anchor, point, camera) triples pass the gate, asserted to be at least a third -- then, as the kernel sees them, rounded
    to the coordinate dtype, nudged until every pixel coordinate on every level is at least MARGIN away from the lattice.
    Weights are a softmax over the P * cams * L taps of an (anchor, group)."""
    coord_dtype = dtype if coord_dtype is None else coord_dtype
    gen = torch.Generator().manual_seed(seed)
    L = len(shapes)
    _, s_cam = level_starts(shapes)
    C = G * Dg
    feature = torch.randn(B, cams * s_cam, C, generator=gen).to(dtype)
    go = torch.randn(B, A, C, generator=gen).to(dtype)
    weights = F.softmax(torch.randn(B, A, P * cams * L, G, generator=gen), 2).view(B, A, P, cams, L, G).to(coord_dtype)
    step = torch.tensor([0.23 / max(w for _, w in shapes), 0.23 / max(h for h, _ in shapes)], dtype=torch.float64)
    for _draw in range(16):   # (a case of a handful of triples is drawn again until a third of them pass the gate)
        loc = (torch.rand(B, A, P, cams, 2, generator=gen) * 1.3 - 0.15).to(coord_dtype)
        for _ in range(64):
            pix = pixel_positions(loc, shapes)
            near = ((pix - pix.round()).abs() < 2 * MARGIN).any(-2)   # [B, A, P, cams, 2]: near on some level
            if not near.any():
                break
            loc = torch.where(near, loc.double() + step, loc.double()).to(coord_dtype)
        if float(gate_of(loc).double().mean()) >= 1 / 3:
            break
    assert min_lattice_distance(loc, shapes) >= MARGIN
    assert float(gate_of(loc).double().mean()) >= 1 / 3
    return feature, loc, weights, go


# ---- the cases of the CPU and GPU tests: each the smallest shape at which its part can go wrong ----
CASES = {
    # one lane per anchor, odd extents, border corners
    "one_lane": dict(B=1, A=3, P=1, cams=1, shapes=[(5, 7)], G=1, Dg=4),
    # camera-major starts, a one-pixel level, G = 3 (no power of two), K = 18
    "cams_levels": dict(B=2, A=7, P=2, cams=3, shapes=[(4, 6), (2, 3), (1, 1)], G=3, Dg=8),
    # one wave per anchor in fp32
    "g8_d32": dict(B=2, A=10, P=4, cams=2, shapes=[(4, 4), (2, 2)], G=8, Dg=32),
    # 12 vectors per anchor in fp32: anchors do not tile a wave evenly
    "straddle": dict(B=1, A=23, P=2, cams=2, shapes=[(3, 5)], G=3, Dg=16),
    # 128 vectors per anchor in fp32: the location sum runs over two rounds
    "wide_anchor": dict(B=1, A=5, P=2, cams=2, shapes=[(4, 4)], G=4, Dg=128),
    # 65 vectors: 64 lanes, two rounds, one group across both
    "two_rounds": dict(B=1, A=4, P=2, cams=1, shapes=[(3, 4)], G=1, Dg=260),
    "two_rounds_16bit": dict(B=1, A=4, P=2, cams=1, shapes=[(3, 4)], G=1, Dg=520),
    # two groups of 65 vectors in three rounds: the middle round ends one group and begins the other (the carried sum)
    "groups_across_rounds": dict(B=1, A=3, P=2, cams=2, shapes=[(3, 4)], G=2, Dg=260),
    # the whole level select: eight levels of at most 12 pixels, mixed extents
    "eight_levels": dict(B=1, A=6, P=1, cams=2, shapes=[(3, 2), (2, 3), (1, 4), (4, 1), (2, 2), (1, 1), (3, 4), (2, 5)],
                         G=1, Dg=4),
    # K = 312: many unit batches and cameras
    "many_taps": dict(B=1, A=2, P=13, cams=6, shapes=[(8, 22), (4, 11), (2, 6), (1, 3)], G=2, Dg=4),
    # every gated-in sample of level 0 lands in one cell: four long lists per camera, empty rows elsewhere
    "crafted": dict(B=2, A=20, P=3, cams=2, shapes=[(4, 4), (2, 2)], G=2, Dg=4),
    # three groups of 3 vectors (fp32; 16-bit: Dg = 24) in 16 lanes: the masked butterfly inside ONE round, VG no power of two
    "odd_group": dict(B=1, A=5, P=2, cams=2, shapes=[(3, 4)], G=3, Dg=12),
    "odd_group_16bit": dict(B=1, A=5, P=2, cams=2, shapes=[(3, 4)], G=3, Dg=24),
    # eight groups of 24 vectors in three rounds: rounds 0 and 1 hold whole groups and end inside one; round 1 begins with a tail
    "carry_and_whole_groups": dict(B=1, A=3, P=2, cams=2, shapes=[(3, 4)], G=8, Dg=96),
    # one group of 128 vectors, wider than a round: the carried sum is consumed exactly at the second round's end
    "group_fills_two_rounds": dict(B=1, A=4, P=2, cams=2, shapes=[(3, 4)], G=1, Dg=512),
    # two groups of 64 vectors, VG = VL: the segmented butterfly over a whole round, one group per round
    "group_per_round": dict(B=1, A=4, P=2, cams=2, shapes=[(3, 4)], G=2, Dg=256),
}
# the four cases above: the (seg, rounds) of DaggGeom each one claims in fp32 (tests/test_dagg_cpu.py asserts them and the
# round boundaries from the lane geometry)
GROUP_CASES = {"odd_group": (0, 1), "odd_group_16bit": (0, 1), "carry_and_whole_groups": (0, 3), "group_fills_two_rounds": (0, 2),
               "group_per_round": (1, 2)}
CRAFTED_XY = ((1.3 + 0.5) / 4, (1.4 + 0.5) / 4)   # pixel (1.3, 1.4) of level 0, (0.4, 0.45) of level 1
CRAFTED_ROWS = [cam * 20 + r for cam in (0, 1) for r in (5, 6, 9, 10)]
CRAFTED_EMPTY = [cam * 20 + r for cam in (0, 1) for r in (0, 1, 2, 3, 4, 7, 8, 11, 12, 13, 14, 15)]


def case_inputs(name, dtype=torch.float32, coord_dtype=None):
    """The CPU tensors of a case of ``CASES``."""
    feature, loc, weights, go = make_inputs(dtype=dtype, coord_dtype=coord_dtype, seed=len(name) + 7, **CASES[name])
    if name == "crafted":
        at = torch.tensor(CRAFTED_XY, dtype=torch.float64).to(loc.dtype)
        loc = torch.where(gate_of(loc)[..., None], at, loc)
        assert min_lattice_distance(loc, CASES[name]["shapes"]) >= MARGIN
    return feature, loc, weights, go
