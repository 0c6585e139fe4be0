"""References for the DCNv3 core operator (include/mdconv.h, "DCNv3 core operator"), independent of the kernels' formulas.

``dcnv3_ref``: a plain-PyTorch restatement -- zero-pad the input, normalise the sampling positions, ``F.grid_sample`` per
group, multiply by the mask, sum over the taps; gradients come from autograd.  ``dcnv3_oracle``: the same call through the
CPU oracle's depthwise modulated 2-D operator with unit weights (NCHW, taps height-major, offsets remapped).
``make_inputs`` draws the tensors of a case; for gradient comparisons no sampling position may lie within ``MARGIN`` px of
an integer -- there the bilinear interpolant has a kink and the reference's own derivative jumps -- which is a rule for
the inputs (``min_lattice_distance`` measures it), not an exclusion of elements."""
import torch
import torch.nn.functional as F

MARGIN = 0.05


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_hw(H, W, kernel, stride, pad, dilation):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = map(_pair, (kernel, stride, pad, dilation))
    return (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def positions(offset, H, W, kernel, stride, pad, dilation, group, offset_scale, position_dtype=None):
    """(loc_h, loc_w) [B, Ho, Wo, G, K] in input pixel coordinates, fp64, straight from the contract.  ``position_dtype``
    (``torch.float32``): the same sums evaluated in that type, one rounding per operation in the contract's order --
    (tap + offset) * offset_scale, then + the pixel's base, which is a whole number -- and widened to fp64 again: what the
    positions are worth once fp32 arithmetic has formed them (half an ulp of the coordinate: 3e-5 px at 683)."""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = map(_pair, (kernel, stride, pad, dilation))
    B, Ho, Wo, _ = offset.shape
    K = kh * kw
    pdt = torch.float64 if position_dtype is None else position_dtype
    off = offset.double().reshape(B, Ho, Wo, group, K, 2).to(pdt)
    c_h, c_w = (dh * (kh - 1)) >> 1, (dw * (kw - 1)) >> 1
    i = torch.arange(kw, dtype=pdt).repeat_interleave(kh)   # tap = i * kh + j
    j = torch.arange(kh, dtype=pdt).repeat(kw)
    ho = torch.arange(Ho, dtype=pdt).view(1, Ho, 1, 1, 1)
    wo = torch.arange(Wo, dtype=pdt).view(1, 1, Wo, 1, 1)
    i, j = i.to(off.device), j.to(off.device)
    loc_w = wo.to(off.device) * sw - pw + c_w + (i * dw - c_w + off[..., 0]) * offset_scale
    loc_h = ho.to(off.device) * sh - ph + c_h + (j * dh - c_h + off[..., 1]) * offset_scale
    return loc_h.double(), loc_w.double()


def min_lattice_distance(offset, H, W, kernel, stride, pad, dilation, group, offset_scale):
    """Smallest distance of any sampling coordinate to an integer."""
    loc_h, loc_w = positions(offset, H, W, kernel, stride, pad, dilation, group, offset_scale)
    d = torch.stack([loc_h, loc_w])
    return (d - d.round()).abs().min().item()


def dcnv3_ref(input, offset, mask, kernel, stride, pad, dilation, group, group_channels, offset_scale, position_dtype=None):
    """fp64 restatement; differentiable.  Returns the result in the dtype of ``input``.  ``position_dtype``: see ``positions``."""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = map(_pair, (kernel, stride, pad, dilation))
    B, H, W, C = input.shape
    G, D, K = group, group_channels, kh * kw
    Ho, Wo = out_hw(H, W, kernel, stride, pad, dilation)
    x = F.pad(input.double(), (0, 0, pw, pw, ph, ph))             # [B, H + 2 ph, W + 2 pw, C], zeros around
    Hp, Wp = H + 2 * ph, W + 2 * pw
    loc_h, loc_w = positions(offset, H, W, kernel, stride, pad, dilation, group, offset_scale, position_dtype)
    # pixel p of the padded image sits at (2 p + 1) / size - 1 (align_corners=False)
    gx = (2 * (loc_w + pw) + 1) / Wp - 1
    gy = (2 * (loc_h + ph) + 1) / Hp - 1
    m = mask.double().reshape(B, Ho, Wo, G, K)
    outs = []
    for g in range(G):
        img = x[..., g * D:(g + 1) * D].permute(0, 3, 1, 2)       # [B, D, Hp, Wp]
        grid = torch.stack([gx[:, :, :, g], gy[:, :, :, g]], -1).reshape(B, Ho, Wo * K, 2)
        s = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        s = s.reshape(B, D, Ho, Wo, K) * m[:, :, :, g].unsqueeze(1)
        outs.append(s.sum(-1).permute(0, 2, 3, 1))                # [B, Ho, Wo, D]
    return torch.cat(outs, -1).to(input.dtype)


def dcnv3_ref_grads(input, offset, mask, grad_output, *geo, position_dtype=None):
    """(output, grad_input, grad_offset, grad_mask) in fp64 from the values the tensors hold."""
    x, o, m = (t.detach().double().cpu().requires_grad_(True) for t in (input, offset, mask))
    out = dcnv3_ref(x, o, m, *geo, position_dtype=position_dtype)
    gi, goff, gm = torch.autograd.grad(out, (x, o, m), grad_output.detach().double().cpu())
    return out.detach(), gi, goff, gm


def dcnv3_oracle(input, offset, mask, grad_output, kernel, stride, pad, dilation, group, group_channels, offset_scale):
    """(output, grad_input, grad_offset, grad_mask) in fp64 through the oracle's modulated 2-D operator: groups = C,
    deformable_groups = G, a weight of ones, taps transposed to height-major, and per tap
    off_h' = c_h + (j * dil_h - c_h + off_y) * offset_scale - j * dil_h (off_w' alike), in (h, w) order."""
    import oracle
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = map(_pair, (kernel, stride, pad, dilation))
    B, H, W, C = input.shape
    G, K = group, kh * kw
    Ho, Wo = out_hw(H, W, kernel, stride, pad, dilation)
    c_h, c_w = (dh * (kh - 1)) >> 1, (dw * (kw - 1)) >> 1
    off = offset.double().reshape(B, Ho, Wo, G, kw, kh, 2)        # [..., i, j, (x, y)]
    i = torch.arange(kw, dtype=torch.float64).view(kw, 1)
    j = torch.arange(kh, dtype=torch.float64).view(1, kh)
    off_w = c_w + (i * dw - c_w + off[..., 0]) * offset_scale - i * dw
    off_h = c_h + (j * dh - c_h + off[..., 1]) * offset_scale - j * dh
    # [B, Ho, Wo, G, i, j, (h, w)] -> [B, G, j, i, (h, w), Ho, Wo]
    o_nchw = torch.stack([off_h, off_w], -1).permute(0, 3, 5, 4, 6, 1, 2).reshape(B, G * K * 2, Ho, Wo).contiguous()
    m_nchw = mask.double().reshape(B, Ho, Wo, G, kw, kh).permute(0, 3, 5, 4, 1, 2).reshape(B, G * K, Ho, Wo).contiguous()
    x_nchw = input.double().permute(0, 3, 1, 2).contiguous()
    go_nchw = grad_output.double().permute(0, 3, 1, 2).contiguous()
    w = torch.ones(C, 1, kh, kw, dtype=torch.float64)
    args = ((sh, sw), (ph, pw), (dh, dw), C, G, 64)
    out = oracle.forward(oracle.MDCN2D, x_nchw, w, None, o_nchw, m_nchw, *args, dtype=torch.float64)
    g = oracle.backward(oracle.MDCN2D, x_nchw, w, None, o_nchw, m_nchw, go_nchw, *args, dtype=torch.float64)
    goff = g["grad_offset"].reshape(B, G, kh, kw, 2, Ho, Wo).permute(0, 5, 6, 1, 3, 2, 4)   # [B, Ho, Wo, G, i, j, (h, w)]
    goff = torch.stack([goff[..., 1], goff[..., 0]], -1) * offset_scale                      # (x, y), d off' / d off
    gm = g["grad_mask"].reshape(B, G, kh, kw, Ho, Wo).permute(0, 4, 5, 1, 3, 2)
    return (out.permute(0, 2, 3, 1).contiguous(), g["grad_input"].permute(0, 2, 3, 1).contiguous(),
            goff.reshape(B, Ho, Wo, G * K * 2).contiguous(), gm.reshape(B, Ho, Wo, G * K).contiguous())


def make_inputs(B, G, D, H, W, kernel, stride=1, pad=0, dilation=1, offset_scale=1.0, dtype=torch.float32, seed=0,
                offset_range=1.5, integer_offsets=False, offset_shift=0.0):
    """CPU tensors (input, offset, mask, grad_output) of ``dtype`` and the geometry tuple of the case.  The offsets are
    uniform in +-``offset_range`` (+ ``offset_shift``), then -- as the kernel sees them, rounded to ``dtype`` -- nudged
    until every sampling coordinate is at least MARGIN away from the lattice.  ``integer_offsets``: integer-valued
    offsets instead (forward-only cases)."""
    gen = torch.Generator().manual_seed(seed)
    kh, kw = _pair(kernel)
    K = kh * kw
    Ho, Wo = out_hw(H, W, kernel, stride, pad, dilation)
    geo = (_pair(kernel), _pair(stride), _pair(pad), _pair(dilation), G, D, float(offset_scale))
    x = torch.randn(B, H, W, G * D, generator=gen).to(dtype)
    m = torch.rand(B, Ho, Wo, G * K, generator=gen).to(dtype)
    go = torch.randn(B, Ho, Wo, G * D, generator=gen).to(dtype)
    if integer_offsets:
        off = torch.randint(-2, 3, (B, Ho, Wo, G * K * 2), generator=gen).to(dtype)
        return x, off, m, go, geo
    off = ((torch.rand(B, Ho, Wo, G * K * 2, generator=gen) * 2 - 1) * offset_range + offset_shift).to(dtype)
    for _ in range(8):
        loc_h, loc_w = positions(off, H, W, *geo[:4], G, offset_scale)
        loc = torch.stack([loc_w, loc_h], -1).reshape(off.shape)
        near = (loc - loc.round()).abs() < 2 * MARGIN
        if not near.any():
            break
        off = torch.where(near, off.double() + 0.23 / offset_scale, off.double()).to(dtype)
    assert min_lattice_distance(off, H, W, *geo[:4], G, offset_scale) >= MARGIN
    return x, off, m, go, geo


# ---- on the lattice -------------------------------------------------------------------------------------------------
# At an integer sampling position the bilinear interpolant has a kink and the operator's derivative is a convention
# (include/mdconv.h): the floor picks the cell, so the derivative is the right-sided one, and the gate -1 < loc < size
# decides whether a sample at -1 or at size contributes at all.  ``F.grid_sample`` is no reference there -- its fp64
# normalisation lands on either side of the integer and it has no gate at -1 -- so the lattice tests use ``dcnv3_direct``.
LATTICE_MODES = ("zero", "integer", "one_axis")


def dcnv3_direct(input, offset, mask, kernel, stride, pad, dilation, group, group_channels, offset_scale):
    """fp64, the contract word for word: positions, the gate, the floor (detached: it picks the cell and has no
    derivative), the four neighbours with their bilinear weights, neighbours outside the image left out; differentiable."""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = map(_pair, (kernel, stride, pad, dilation))
    B, H, W, C = input.shape
    G, D, K = group, group_channels, kh * kw
    Ho, Wo = out_hw(H, W, kernel, stride, pad, dilation)
    x = input.double().reshape(B, H * W, G, D)
    off = offset.double().reshape(B, Ho, Wo, G, K, 2)
    m = mask.double().reshape(B, Ho, Wo, G, K)
    c_h, c_w = (dh * (kh - 1)) >> 1, (dw * (kw - 1)) >> 1
    dev = input.device
    b_idx = torch.arange(B, device=dev).view(B, 1, 1, 1).expand(B, Ho, Wo, G)
    g_idx = torch.arange(G, device=dev).view(1, 1, 1, G).expand(B, Ho, Wo, G)
    ho = torch.arange(Ho, dtype=torch.float64, device=dev).view(1, Ho, 1, 1)
    wo = torch.arange(Wo, dtype=torch.float64, device=dev).view(1, 1, Wo, 1)
    out = torch.zeros(B, Ho, Wo, G, D, dtype=torch.float64, device=dev)
    for tap in range(K):
        i, j = tap // kh, tap % kh                                  # i: the kernel's width index
        loc_w = wo * sw - pw + c_w + (i * dw - c_w + off[..., tap, 0]) * offset_scale   # [B, Ho, Wo, G]
        loc_h = ho * sh - ph + c_h + (j * dh - c_h + off[..., tap, 1]) * offset_scale
        gate = (loc_h > -1) & (loc_w > -1) & (loc_h < H) & (loc_w < W)
        y0, x0 = loc_h.detach().floor(), loc_w.detach().floor()
        ly, lx = loc_h - y0, loc_w - x0
        for cy in (0, 1):
            for cx in (0, 1):
                yi, xi = (y0 + cy).long(), (x0 + cx).long()
                read = gate & (yi >= 0) & (yi < H) & (xi >= 0) & (xi < W)
                wgt = (ly if cy else 1 - ly) * (lx if cx else 1 - lx) * m[..., tap]
                wgt = torch.where(read, wgt, torch.zeros_like(wgt))
                row = yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)
                out = out + x[b_idx, row, g_idx] * wgt[..., None]
    return out.reshape(B, Ho, Wo, C).to(input.dtype)


def dcnv3_direct_grads(input, offset, mask, grad_output, *geo):
    """(output, grad_input, grad_offset, grad_mask) of ``dcnv3_direct`` in fp64 from the values the tensors hold."""
    x, o, m = (t.detach().double().cpu().requires_grad_(True) for t in (input, offset, mask))
    out = dcnv3_direct(x, o, m, *geo)
    gi, goff, gm = torch.autograd.grad(out, (x, o, m), grad_output.detach().double().cpu())
    return out.detach(), gi, goff, gm


def lattice_offsets(mode, shape, offset_scale, positions_of, H, W, dtype, gen):
    """Offsets [B, Ho, Wo, G*K*2] of ``dtype`` whose sampling positions lie on the lattice, and the mask of the offset
    elements meant to (same shape).  ``positions_of(offset)`` gives (loc_h, loc_w) [B, Ho, Wo, G, K] in fp64.
    ``zero``: all offsets 0.  ``integer``: whole pixels in {-1, 0, 1} (offsets of +-1 / offset_scale, which must be whole
    numbers: they are exact in every dtype).  ``one_axis``: x on the lattice and y under the MARGIN rule for even taps,
    the other way round for odd taps.  What the tensors must be is asserted -- conditions, not tolerances: distance 0 on
    the axes meant, at least half of the samples inside the gate, and among the lattice coordinates one at -1, one at
    size - 1 and one at size."""
    assert mode in LATTICE_MODES, mode
    # steps of one pixel where 1 / offset_scale is a whole number (scale 0.5: offsets of +-2), of offset_scale pixels otherwise
    unit = 1.0 / offset_scale if float(1.0 / offset_scale).is_integer() else 1.0
    assert float(unit * offset_scale).is_integer(), "whole pixels need offset_scale or its inverse to be a whole number"
    B, Ho, Wo, n = shape
    if mode == "zero":
        off = torch.zeros(shape)
    else:
        off = (torch.randint(-1, 2, shape, generator=gen) * unit)
    meant = torch.ones(shape, dtype=torch.bool)
    off = off.to(dtype)
    if mode == "one_axis":
        free = ((torch.rand(shape, generator=gen) * 2 - 1) * 1.5).to(dtype)
        for _ in range(8):
            loc_h, loc_w = positions_of(free)
            loc = torch.stack([loc_w, loc_h], -1).reshape(shape)
            near = (loc - loc.round()).abs() < 2 * MARGIN
            if not near.any():
                break
            free = torch.where(near, free.double() + 0.23 / offset_scale, free.double()).to(dtype)
        tap = torch.arange(n // 2).view(-1, 1)              # (group, tap) pairs; K taps per group follow each other
        K = positions_of(off)[0].shape[-1]
        odd = ((tap % K) % 2 == 1)
        xy = torch.arange(2).view(1, 2)
        meant = ((xy == 0) ^ odd).reshape(n).expand(shape)   # even taps: x on the lattice; odd taps: y
        off = torch.where(meant, off, free)
    loc_h, loc_w = positions_of(off)
    loc = torch.stack([loc_w, loc_h], -1).reshape(shape)
    size = torch.tensor([float(W), float(H)]).repeat(n // 2).expand(shape)
    dist = (loc - loc.round()).abs()
    assert float(dist[meant].max()) == 0.0, "lattice distance on the axes meant"
    assert float(dist[~meant].min()) >= MARGIN if (~meant).any() else True
    inside = (loc_h > -1) & (loc_w > -1) & (loc_h < H) & (loc_w < W)
    assert float(inside.double().mean()) >= 0.5, "inside the gate: %.2f" % float(inside.double().mean())
    for what, hit in (("-1", loc == -1), ("size - 1", loc == size - 1), ("size", loc == size)):
        assert bool((hit & meant).any()), "no lattice coordinate at " + what
    return off, meant


def gate_of(offset, H, W, kernel, stride, pad, dilation, group, offset_scale):
    """[B, Ho, Wo, G, K] bool: the sample passes the gate -1 < loc < size on both axes."""
    loc_h, loc_w = positions(offset, H, W, kernel, stride, pad, dilation, group, offset_scale)
    return (loc_h > -1) & (loc_w > -1) & (loc_h < H) & (loc_w < W)


def make_lattice_inputs(mode, B, G, D, H, W, kernel, stride=1, pad=0, dilation=1, offset_scale=1.0, dtype=torch.float32,
                        seed=0):
    """CPU tensors (input, offset, mask, grad_output) of ``dtype`` and the geometry tuple, as ``make_inputs`` draws them,
    with the offsets of ``lattice_offsets(mode)``."""
    gen = torch.Generator().manual_seed(seed)
    kh, kw = _pair(kernel)
    K = kh * kw
    Ho, Wo = out_hw(H, W, kernel, stride, pad, dilation)
    geo = (_pair(kernel), _pair(stride), _pair(pad), _pair(dilation), G, D, float(offset_scale))
    x = torch.randn(B, H, W, G * D, generator=gen).to(dtype)
    m = torch.rand(B, Ho, Wo, G * K, generator=gen).to(dtype)
    go = torch.randn(B, Ho, Wo, G * D, generator=gen).to(dtype)
    off, _ = lattice_offsets(mode, (B, Ho, Wo, G * K * 2), offset_scale,
                             lambda o: positions(o, H, W, *geo[:4], G, offset_scale), H, W, dtype, gen)
    return x, off, m, go, geo
