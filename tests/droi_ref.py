"""fp64 references of deformable RoI pooling (include/mdconv.h, "Deformable RoI pooling"), on the channels-last tensors of the
C contract: ``input [B, H, W, C]``, ``rois [R, 5]``, ``offset [R, 2, PH, PW]`` or None, ``output [R, PH, PW, C]``.

Two independent statements of the contract:

``droi_explicit``   an explicit four-corner gather (floor, clamp, four indexed loads) with CLOSED-FORM gradients in the
                    project's lattice convention: the right-sided derivative of the cell floor(loc), exactly zero along an
                    axis where the coordinate is clamped (loc < 0 or loc >= size - 1), exactly zero outside the gate.
``droi_autograd``   a differentiable torch composition with no floor and no index: the coordinate is clamped to
                    [0, size - 1] and the bilinear weights are the hat functions relu(1 - |c - i|) over ALL pixels i of the
                    axis, contracted with the image by einsum; its gradients come from autograd.

They agree wherever no sample coordinate is on the lattice; ``make_inputs`` draws the tensors of a case and ASSERTS that:
every sample coordinate of a live sample is at least ``MARGIN`` away from every integer (-1, 0, size - 1 and size are
integers), and under the adaptive rule every bin extent is ``GRID_MARGIN`` away from an integer, so that an fp32 and an fp64
ceil agree on the grid."""
import math

import torch

from tests.dcnv3_ref import MARGIN   # the lattice margin is the project's, not a second constant

GRID_MARGIN = 1e-3
F64 = torch.float64


def geometry(rois, offset, B, PH, PW, spatial_scale=1.0, sampling_ratio=0, gamma=0.1, max_grid=8):
    """The sample positions of a call, fp64, padded to the grid bound G = sampling_ratio or max_grid:
    ``y [R, PH, PW, G]``, ``x [R, PH, PW, G]``, ``live_y / live_x [R, G]`` (sample index below the RoI's own grid, and the RoI
    valid), ``b [R]`` (0 for an invalid RoI), ``cnt [R]``, ``fy / fx [R]`` = d y / d offset, d x / d offset, ``gh / gw [R]``,
    ``bh / bw [R]``.  ``offset`` may require grad: y and x are differentiable in it."""
    rois = rois.to(F64)
    R = rois.shape[0]
    G = sampling_ratio if sampling_ratio > 0 else max_grid
    f0 = rois[:, 0]
    finite = torch.isfinite(rois).all(1)
    valid = finite & (f0 >= 0) & (f0 < B) & (f0 == f0.floor())
    safe = torch.where(valid[:, None], rois, torch.zeros_like(rois))   # nothing is read through an invalid RoI
    b = safe[:, 0].long()
    x1s, y1s, x2s, y2s = (safe[:, i] * spatial_scale - 0.5 for i in (1, 2, 3, 4))
    rw, rh = x2s - x1s, y2s - y1s
    bw, bh = rw / PW, rh / PH
    if sampling_ratio > 0:
        gh = torch.full((R,), sampling_ratio, dtype=torch.long)
        gw = gh.clone()
    else:
        gh = bh.ceil().clamp(0, max_grid).long()
        gw = bw.ceil().clamp(0, max_grid).long()
    gh, gw = gh * valid, gw * valid
    cnt = (gh * gw).clamp(min=1).to(F64)
    idx = torch.arange(G)
    live_y, live_x = idx[None] < gh[:, None], idx[None] < gw[:, None]
    fx, fy = gamma * rw, gamma * rh
    if offset is None:
        dx = dy = torch.zeros(R, PH, PW, dtype=F64)
    else:
        off = offset.to(F64)
        dx, dy = fx[:, None, None] * off[:, 0], fy[:, None, None] * off[:, 1]
    ph = torch.arange(PH, dtype=F64)[None, :, None, None]
    pw = torch.arange(PW, dtype=F64)[None, None, :, None]
    half = (idx.to(F64) + 0.5)[None, None, None, :]
    y = (y1s[:, None, None] + dy)[..., None] + ph * bh[:, None, None, None] + half * (bh / gh.clamp(min=1))[:, None, None, None]
    x = (x1s[:, None, None] + dx)[..., None] + pw * bw[:, None, None, None] + half * (bw / gw.clamp(min=1))[:, None, None, None]
    return dict(y=y, x=x, live_y=live_y, live_x=live_x, b=b, cnt=cnt, fy=fy, fx=fx, gh=gh, gw=gw, bh=bh, bw=bw, valid=valid)


def _axis(loc, size):
    """RoIAlign's sample along one axis: gate, low / high neighbour, fractional part, and whether the coordinate is free."""
    inn = (loc >= -1) & (loc <= size)
    c = loc.clamp(min=0)
    fl = c.floor()
    top = fl >= size - 1
    lo = torch.where(top, torch.full_like(fl, size - 1), fl)
    lo = torch.where(inn, lo, torch.zeros_like(lo))
    hi = torch.where(top | ~inn, lo, lo + 1)
    frac = torch.where(top, torch.zeros_like(c), c - fl)
    free = inn & (loc >= 0) & ~top
    return inn, lo.long(), hi.long(), frac, free


def droi_explicit(input, rois, offset, output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1, max_grid=8,
                  grad_output=None):
    """The explicit route, fp64.  Returns ``output``, or with ``grad_output`` the tuple (output, grad_input, grad_offset)
    -- grad_offset None without offset -- from closed forms in the lattice convention."""
    PH, PW = output_size
    B, H, W, C = input.shape
    inp = input.to(F64)
    g = geometry(rois, None if offset is None else offset.detach(), B, PH, PW, spatial_scale, sampling_ratio, gamma, max_grid)
    R, G = g["y"].shape[0], g["y"].shape[3]
    iny, ylo, yhi, ly, fry = _axis(g["y"], H)   # [R, PH, PW, G]
    inx, xlo, xhi, lx, frx = _axis(g["x"], W)
    m = (g["live_y"][:, None, None, :, None] & g["live_x"][:, None, None, None, :] & iny[..., :, None] & inx[..., None, :])
    bb = g["b"][:, None, None, None, None].expand(R, PH, PW, G, G)
    ys = [t[..., :, None].expand(R, PH, PW, G, G) for t in (ylo, yhi)]
    xs = [t[..., None, :].expand(R, PH, PW, G, G) for t in (xlo, xhi)]
    LY, LX = ly[..., :, None], lx[..., None, :]
    wy, wx = [1 - LY, LY], [1 - LX, LX]
    v = [[inp[bb, ys[cy], xs[cx]] for cx in (0, 1)] for cy in (0, 1)]   # [R, PH, PW, G, G, C]
    mf = m.to(F64)
    val = sum((wy[cy] * wx[cx] * mf)[..., None] * v[cy][cx] for cy in (0, 1) for cx in (0, 1))
    inv = (1.0 / g["cnt"])[:, None, None]
    out = val.sum((3, 4)) * inv[..., None]
    if grad_output is None:
        return out
    go = grad_output.to(F64)
    gi = torch.zeros(B * H * W, C, dtype=F64)
    for cy in (0, 1):
        for cx in (0, 1):
            w = (wy[cy] * wx[cx] * mf) * inv[..., None, None]
            rows = (bb * H + ys[cy]) * W + xs[cx]
            contrib = w[..., None] * go[:, :, :, None, None, :]
            gi.index_add_(0, rows.reshape(-1), contrib.reshape(-1, C))
    gi = gi.view(B, H, W, C)
    goff = None
    if offset is not None:
        gov = go[:, :, :, None, None, :]
        ddx = (((1 - LY)[..., None] * (v[0][1] - v[0][0]) + LY[..., None] * (v[1][1] - v[1][0])) * gov).sum(-1)
        ddy = (((1 - LX)[..., None] * (v[1][0] - v[0][0]) + LX[..., None] * (v[1][1] - v[0][1])) * gov).sum(-1)
        ddx = ddx * mf * frx[..., None, :].to(F64)
        ddy = ddy * mf * fry[..., :, None].to(F64)
        gx = ddx.sum((3, 4)) * inv * g["fx"][:, None, None]
        gy = ddy.sum((3, 4)) * inv * g["fy"][:, None, None]
        goff = torch.stack([gx, gy], 1)
    return out, gi, goff


def droi_autograd_forward(input, rois, offset, output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1, max_grid=8):
    """The differentiable composition (no floor, no index into the image), fp64 tensors in, differentiable in ``input`` and
    ``offset``."""
    PH, PW = output_size
    B, H, W, C = input.shape
    g = geometry(rois, offset, B, PH, PW, spatial_scale, sampling_ratio, gamma, max_grid)
    y, x = g["y"], g["x"]
    gate_y = ((y >= -1) & (y <= H) & g["live_y"][:, None, None, :]).to(F64)
    gate_x = ((x >= -1) & (x <= W) & g["live_x"][:, None, None, :]).to(F64)
    hat_y = torch.relu(1 - (y.clamp(0, H - 1)[..., None] - torch.arange(H, dtype=F64)).abs()) * gate_y[..., None]   # [R,PH,PW,G,H]
    hat_x = torch.relu(1 - (x.clamp(0, W - 1)[..., None] - torch.arange(W, dtype=F64)).abs()) * gate_x[..., None]   # [R,PH,PW,G,W]
    # the sum over a bin's samples factorises: sum_iy sum_ix hat_y(iy) hat_x(ix)
    ky, kx = hat_y.sum(3), hat_x.sum(3)   # [R, PH, PW, H], [R, PH, PW, W]
    onehot = torch.nn.functional.one_hot(g["b"], B).to(F64) * g["valid"][:, None].to(F64)   # [R, B]
    out = torch.einsum("rb,rpqh,rpqw,bhwc->rpqc", onehot, ky, kx, input)
    return out / g["cnt"][:, None, None, None]


def droi_autograd(input, rois, offset, output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1, max_grid=8,
                  grad_output=None):
    """The autograd route, fp64: (output, grad_input, grad_offset) like ``droi_explicit``."""
    inp = input.detach().to(F64).requires_grad_(True)
    off = None if offset is None else offset.detach().to(F64).requires_grad_(True)
    out = droi_autograd_forward(inp, rois, off, output_size, spatial_scale, sampling_ratio, gamma, max_grid)
    if grad_output is None:
        return out.detach()
    out.backward(grad_output.to(F64))
    return out.detach(), inp.grad, None if off is None else (off.grad if off.grad is not None else torch.zeros_like(off))


def droi_nchw(input, rois, offset, output_size, spatial_scale=1.0, sampling_ratio=0, gamma=0.1, max_grid=8):
    """``droi_autograd_forward`` behind the logical-NCHW surface of the Python modules (differentiable, any float dtype in,
    the same dtype out): the stand-in for the native core in module tests."""
    off = None if offset is None or offset.numel() == 0 else offset.to(F64).cpu()
    out = droi_autograd_forward(input.permute(0, 2, 3, 1).to(F64).cpu(), rois.detach().cpu(), off, output_size, spatial_scale,
                                sampling_ratio, gamma, max_grid)
    return out.permute(0, 3, 1, 2).to(device=input.device, dtype=input.dtype)


def min_lattice_distance(rois, offset, B, PH, PW, spatial_scale=1.0, sampling_ratio=0, gamma=0.1, max_grid=8, per_bin=False):
    """Smallest distance of a live sample coordinate to an integer (so also to -1, 0, size - 1 and size); inf without a live
    sample.  ``per_bin``: the [R, PH, PW] tensor of minima instead."""
    g = geometry(rois, offset, B, PH, PW, spatial_scale, sampling_ratio, gamma, max_grid)
    inf = torch.full_like(g["y"], math.inf)
    dy = torch.where(g["live_y"][:, None, None, :].expand_as(g["y"]), (g["y"] - g["y"].round()).abs(), inf)
    dx = torch.where(g["live_x"][:, None, None, :].expand_as(g["x"]), (g["x"] - g["x"].round()).abs(), inf)
    d = torch.minimum(dy.min(3)[0], dx.min(3)[0])
    return d if per_bin else float(d.min())


def min_grid_distance(rois, B, PH, PW, spatial_scale=1.0, max_grid=8):
    """Adaptive rule: the smallest distance of a valid RoI's bin extent (rh / PH, rw / PW) to an integer in 0..max_grid, the
    places where ceil changes the grid."""
    g = geometry(rois, None, B, PH, PW, spatial_scale, 0, 0.0, max_grid)
    d = math.inf
    for ext in (g["bh"], g["bw"]):
        e = ext[g["valid"]]
        near = e.round().clamp(0, max_grid)
        d = min(d, float((e - near).abs().min()) if e.numel() else math.inf)
    return d


def random_rois(R, B, H, W, spatial_scale, gen, min_size=1.5):
    """R RoIs inside the image (in image coordinates, i.e. divided by spatial_scale), batch indices cycling through the images
    in an order that is NOT sorted."""
    x1 = torch.rand(R, generator=gen) * (W - min_size - 1)
    y1 = torch.rand(R, generator=gen) * (H - min_size - 1)
    w = min_size + torch.rand(R, generator=gen) * (W - 1 - x1 - min_size)
    h = min_size + torch.rand(R, generator=gen) * (H - 1 - y1 - min_size)
    b = torch.tensor([(B - 1 - i) % B for i in range(R)], dtype=torch.float32)
    box = (torch.stack([x1, y1, x1 + w, y1 + h], 1) + 0.5) / spatial_scale
    return torch.cat([b[:, None], box], 1).float()


def make_inputs(B, C, H, W, PH, PW, R=None, rois=None, spatial_scale=1.0, sampling_ratio=0, gamma=0.1, max_grid=8,
                with_offset=True, offset_std=1.0, dtype=torch.float32, coord_dtype=None, seed=0, off_lattice=True):
    """(input, rois, offset | None, grad_output) of a case, in the dtypes the kernel sees.  ``rois``: explicit rows, else R
    random ones.  With ``off_lattice`` the offsets (or, without offset, the random RoIs) are re-drawn bin by bin until every
    live sample coordinate is MARGIN away from the lattice, and that -- and GRID_MARGIN under the adaptive rule -- is
    ASSERTED on the tensors returned."""
    gen = torch.Generator().manual_seed(seed)
    cdt = coord_dtype or dtype
    inp = torch.randn(B, H, W, C, generator=gen).to(dtype)
    given = rois is not None
    rois = torch.tensor(rois, dtype=torch.float32) if given else random_rois(R, B, H, W, spatial_scale, gen)
    R = rois.shape[0]
    go = torch.randn(R, PH, PW, C, generator=gen).to(dtype)
    geo = (B, PH, PW, spatial_scale, sampling_ratio, gamma, max_grid)
    offset = (torch.randn(R, 2, PH, PW, generator=gen) * offset_std).to(cdt) if with_offset else None
    if off_lattice:
        for _ in range(200):
            d = min_lattice_distance(rois, offset, *geo, per_bin=True)
            bad = d < 2 * MARGIN
            if not bad.any():
                break
            if with_offset:
                fresh = (torch.randn(R, 2, PH, PW, generator=gen) * offset_std).to(cdt)
                offset = torch.where(bad[:, None], fresh, offset)
            else:
                assert not given, "explicit RoIs without offset put a sample within MARGIN of the lattice"
                fresh = random_rois(R, B, H, W, spatial_scale, gen)
                rois = torch.where(bad.flatten(1).any(1)[:, None], fresh, rois)
        assert min_lattice_distance(rois, offset, *geo) >= MARGIN
    if sampling_ratio == 0:
        assert min_grid_distance(rois, B, PH, PW, spatial_scale, max_grid) >= GRID_MARGIN
    return inp, rois, offset, go


def lattice_inputs(dtype=torch.float64, coord_dtype=None, C=4):
    """ONE RoI over a 6 x 5 image whose samples are exact in every dtype: rw = rh = 4 and gamma = 0.25, so an offset o moves a
    bin by o pixels; 2 x 2 bins of 2 px with ratio 2 put the samples of bin (ph, pw) at 2*ph + {0.5, 1.5} + o.  The offsets
    are multiples of 0.5 chosen per bin: on the lattice, in the clamped zones on both sides, exactly on the gate (-1 and
    size, which still pass), beyond it, and one free off-lattice bin."""
    H, W = 6, 5
    gen = torch.Generator().manual_seed(4)
    inp = torch.randn(1, H, W, C, generator=gen).to(dtype)
    rois = torch.tensor([[0.0, 0.5, 0.5, 4.5, 4.5]])
    # x of bin (0,0): {1, 2} on the lattice; (0,1): {-0.5, 0.5} clamped low and free; (1,0): {-1, 0} the gate's edge and the
    # lattice; (1,1): {2.75, 3.75} free
    off = torch.tensor([[[[0.5, -3.0], [-1.5, 0.25]],
                         # y of bin (0,0): {0, 1} on the lattice; (0,1): {0.75, 1.75} free; (1,0): {4.5, 5.5} free and clamped
                         # high (H - 1 = 5); (1,1): {6.5, 7.5} beyond the gate
                         [[-0.5, 0.25], [2.0, 4.0]]]]).to(coord_dtype or dtype)
    go = torch.randn(1, 2, 2, C, generator=gen).to(dtype)
    return inp, rois, off, go, dict(output_size=(2, 2), spatial_scale=1.0, sampling_ratio=2, gamma=0.25, max_grid=8)
