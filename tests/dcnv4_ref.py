"""Reference for the DCNv4 operator (include/mdconv.h, "DCNv4 operator"), independent of the kernels' formulas and of
``tests.dcnv3_ref``: an fp64 restatement straight from the contract -- unpack the row, form the positions, take the floor,
gather the four corners of every sample under the gate (-1 < loc < size) and the in-image rule, weigh them bilinearly times
the mask, sum over the taps.  Gradients come from autograd (the floor is piecewise constant, so the derivative of the
fractional parts is that of the positions).  ``pack`` / ``unpack`` translate between ``offset_mask`` and the DCNv3-style
``(offset, mask)`` pair.  ``make_inputs`` draws the tensors of a case: masks from ``randn`` (negative values and values above
one -- there is no softmax), offsets nudged until every sampling coordinate is at least ``dcnv3_ref.MARGIN`` from the lattice,
which is a rule for the inputs (``min_lattice_distance`` measures it), not an exclusion of elements."""
import torch

from tests.dcnv3_ref import MARGIN   # the lattice margin is the project's, not a second constant


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def taps(kernel, remove_center=False):
    kh, kw = _pair(kernel)
    return kh * kw - int(bool(remove_center))


def row_len(group, K):
    return (group * K * 3 + 7) // 8 * 8


def out_hw(H, W, kernel, stride, pad, dilation):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = map(_pair, (kernel, stride, pad, dilation))
    return (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def unpack(offset_mask, group, K):
    """(offset [B, Ho, Wo, G*K*2], mask [B, Ho, Wo, G*K]) of a packed tensor; the padding columns are not looked at."""
    B, Ho, Wo, _ = offset_mask.shape
    rows = offset_mask[..., :group * K * 3].reshape(B, Ho, Wo, group, K * 3)
    return rows[..., :2 * K].reshape(B, Ho, Wo, group * K * 2), rows[..., 2 * K:].reshape(B, Ho, Wo, group * K)


def pack(offset, mask, group, K, padding=0.0):
    """The packed tensor of (offset, mask); the padding columns hold ``padding``."""
    B, Ho, Wo, _ = mask.shape
    rows = torch.cat([offset.reshape(B, Ho, Wo, group, 2 * K), mask.reshape(B, Ho, Wo, group, K)], -1)
    rows = rows.reshape(B, Ho, Wo, group * K * 3)
    fill = rows.new_full((B, Ho, Wo, row_len(group, K) - group * K * 3), padding)
    return torch.cat([rows, fill], -1)


def grid_taps(kernel, remove_center):
    """Kernel-grid position u = i * kh + j of every tensor tap: all of them, or all but the centre."""
    kh, kw = _pair(kernel)
    u = list(range(kh * kw))
    if remove_center:
        u.remove((kh * kw - 1) // 2)
    return torch.tensor(u)


def positions(offset, H, W, kernel, stride, pad, dilation, group, offset_scale, remove_center=False):
    """(loc_h, loc_w) [B, Ho, Wo, G, K] in input pixel coordinates, fp64, from the unpacked offsets."""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = map(_pair, (kernel, stride, pad, dilation))
    B, Ho, Wo, _ = offset.shape
    u = grid_taps(kernel, remove_center).to(offset.device)
    off = offset.double().reshape(B, Ho, Wo, group, u.numel(), 2)
    i, j = (u // kh).double(), (u % kh).double()   # i: width index, j: height index
    c_h, c_w = (dh * (kh - 1)) >> 1, (dw * (kw - 1)) >> 1
    ho = torch.arange(Ho, dtype=torch.float64, device=offset.device).view(1, Ho, 1, 1, 1)
    wo = torch.arange(Wo, dtype=torch.float64, device=offset.device).view(1, 1, Wo, 1, 1)
    loc_w = wo * sw - pw + c_w + (i * dw - c_w + off[..., 0]) * offset_scale
    loc_h = ho * sh - ph + c_h + (j * dh - c_h + off[..., 1]) * offset_scale
    return loc_h, loc_w


def min_lattice_distance(offset_mask, H, W, kernel, stride, pad, dilation, group, offset_scale, remove_center=False):
    """Smallest distance of any sampling coordinate to an integer."""
    off, _ = unpack(offset_mask, group, taps(kernel, remove_center))
    d = torch.stack(positions(off, H, W, kernel, stride, pad, dilation, group, offset_scale, remove_center))
    return (d - d.round()).abs().min().item()


def dcnv4_ref(input, offset_mask, kernel, stride, pad, dilation, group, group_channels, offset_scale, remove_center=False):
    """fp64 restatement; differentiable.  Returns the result in the dtype of ``input``."""
    B, H, W, C = input.shape
    G, D, K = group, group_channels, taps(kernel, remove_center)
    offset, mask = unpack(offset_mask.double(), G, K)
    Ho, Wo = offset.shape[1:3]
    loc_h, loc_w = positions(offset, H, W, kernel, stride, pad, dilation, G, offset_scale, remove_center)
    gate = (loc_h > -1) & (loc_w > -1) & (loc_h < H) & (loc_w < W)
    y0, x0 = loc_h.detach().floor(), loc_w.detach().floor()
    ly, lx = loc_h - y0, loc_w - x0
    m = mask.reshape(B, Ho, Wo, G, K)
    x = input.double().reshape(B, H * W, G, D)
    out = []
    for g in range(G):
        acc = 0
        for cy in (0, 1):
            for cx in (0, 1):
                yy, xx = (y0[..., g, :] + cy).long(), (x0[..., g, :] + cx).long()
                read = gate[..., g, :] & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
                w = (ly[..., g, :] if cy else 1 - ly[..., g, :]) * (lx[..., g, :] if cx else 1 - lx[..., g, :])
                w = torch.where(read, w * m[..., g, :], torch.zeros_like(w))          # [B, Ho, Wo, K]
                pix = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(B, Ho * Wo * K, 1)
                v = torch.gather(x[:, :, g], 1, pix.expand(B, Ho * Wo * K, D)).reshape(B, Ho, Wo, K, D)
                acc = acc + (w.unsqueeze(-1) * v).sum(3)
        out.append(acc)
    return torch.cat(out, -1).to(input.dtype)


def dcnv4_ref_grads(input, offset_mask, grad_output, *geo):
    """(output, grad_input, grad_offset_mask) in fp64 from the values the tensors hold.  NaN padding columns take no part:
    their gradient is zero."""
    x, om = (t.detach().double().cpu().requires_grad_(True) for t in (input, offset_mask))
    out = dcnv4_ref(x, om, *geo)
    gi, gom = torch.autograd.grad(out, (x, om), grad_output.detach().double().cpu())
    return out.detach(), gi, gom


def make_inputs(B, G, D, H, W, kernel, stride=1, pad=0, dilation=1, offset_scale=1.0, remove_center=False,
                dtype=torch.float32, coord_dtype=None, seed=0, offset_range=1.5, integer_offsets=False, nan_padding=False):
    """CPU tensors (input, offset_mask, grad_output) -- values of ``dtype``, offset_mask of ``coord_dtype`` (default: the
    same) -- and the geometry tuple of the case.  The masks are N(0, 1).  The offsets are uniform in +-``offset_range``,
    then -- as the kernel sees them, rounded to ``coord_dtype`` -- nudged until every sampling coordinate is at least MARGIN
    away from the lattice.  ``integer_offsets``: integer-valued offsets instead (forward-only cases).  ``nan_padding``: the
    padding columns hold NaN instead of zeros."""
    cdt = dtype if coord_dtype is None else coord_dtype
    gen = torch.Generator().manual_seed(seed)
    K = taps(kernel, remove_center)
    Ho, Wo = out_hw(H, W, kernel, stride, pad, dilation)
    geo = (_pair(kernel), _pair(stride), _pair(pad), _pair(dilation), G, D, float(offset_scale), bool(remove_center))
    x = torch.randn(B, H, W, G * D, generator=gen).to(dtype)
    m = torch.randn(B, Ho, Wo, G * K, generator=gen).to(cdt)
    go = torch.randn(B, Ho, Wo, G * D, generator=gen).to(dtype)
    padding = float("nan") if nan_padding else 0.0
    if integer_offsets:
        off = torch.randint(-2, 3, (B, Ho, Wo, G * K * 2), generator=gen).to(cdt)
        return x, pack(off, m, G, K, padding), go, geo
    off = ((torch.rand(B, Ho, Wo, G * K * 2, generator=gen) * 2 - 1) * offset_range).to(cdt)
    for _ in range(8):
        loc_h, loc_w = positions(off, H, W, *geo[:4], G, offset_scale, remove_center)
        loc = torch.stack([loc_w, loc_h], -1).reshape(off.shape)
        near = (loc - loc.round()).abs() < 2 * MARGIN
        if not near.any():
            break
        off = torch.where(near, off.double() + 0.23 / offset_scale, off.double()).to(cdt)
    om = pack(off, m, G, K, padding)
    assert min_lattice_distance(om, H, W, *geo[:4], G, offset_scale, remove_center) >= MARGIN
    return x, om, go, geo


def gate_of(offset_mask, H, W, kernel, stride, pad, dilation, group, offset_scale, remove_center=False):
    """[B, Ho, Wo, G, K] bool: the sample passes the gate -1 < loc < size on both axes."""
    off, _ = unpack(offset_mask, group, taps(kernel, remove_center))
    loc_h, loc_w = positions(off, H, W, kernel, stride, pad, dilation, group, offset_scale, remove_center)
    return (loc_h > -1) & (loc_w > -1) & (loc_h < H) & (loc_w < W)


def make_lattice_inputs(mode, B, G, D, H, W, kernel, stride=1, pad=0, dilation=1, offset_scale=1.0, remove_center=False,
                        dtype=torch.float32, coord_dtype=None, seed=0, nan_padding=False):
    """CPU tensors (input, offset_mask, grad_output) and the geometry tuple, as ``make_inputs`` draws them, with sampling
    positions on the lattice: the modes and the asserted conditions of ``tests.dcnv3_ref.lattice_offsets``."""
    from tests.dcnv3_ref import lattice_offsets
    cdt = dtype if coord_dtype is None else coord_dtype
    gen = torch.Generator().manual_seed(seed)
    K = taps(kernel, remove_center)
    Ho, Wo = out_hw(H, W, kernel, stride, pad, dilation)
    geo = (_pair(kernel), _pair(stride), _pair(pad), _pair(dilation), G, D, float(offset_scale), bool(remove_center))
    x = torch.randn(B, H, W, G * D, generator=gen).to(dtype)
    m = torch.randn(B, Ho, Wo, G * K, generator=gen).to(cdt)
    go = torch.randn(B, Ho, Wo, G * D, generator=gen).to(dtype)
    off, _ = lattice_offsets(mode, (B, Ho, Wo, G * K * 2), offset_scale,
                             lambda o: positions(o, H, W, *geo[:4], G, offset_scale, remove_center), H, W, cdt, gen)
    return x, pack(off, m, G, K, float("nan") if nan_padding else 0.0), go, geo
