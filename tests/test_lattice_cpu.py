"""The references the lattice tests stand on (tests/test_gpu_lattice.py), checked on the CPU in fp64.

At an integer sampling position the bilinear interpolant has a kink; the operators' derivative there is a convention
(include/mdconv.h): the floor picks the cell, so the derivative is the right-sided one, and a sample the gate
-1 < loc < size leaves out -- loc == -1 and loc == size included -- has zero gradient.  Here:
  * ``dcnv3_direct`` equals the ``F.grid_sample`` reference off the lattice, and equals two independent statements of the
    contract -- ``dcnv4_ref`` through ``pack``, and the CPU oracle's modulated 2-D operator -- on it;
  * the convention is stated once without autograd: a forward difference of the reference's own output with step 2^-10
    (the interpolant is linear inside a cell, so the difference is exact up to rounding), and exact zeros outside the gate;
  * the ``grid_sample`` references disagree with all of that on the lattice, by more than the gradient's own size."""
import pytest
import torch

from tests import dcnv3_ref as R3
from tests import dcnv4_ref as R4
from tests import fda_ref as RF
from tests import msda_ref as RM
from tests.test_dcnv3_cpu import SHAPES
from tests.util import rel_err

F64 = torch.float64
STEP = 2.0 ** -10
NAMES = ("output", "grad_input", "grad_offset", "grad_mask")

LATTICE = {
    "3x3": dict(B=2, G=1, D=4, H=5, W=7, kernel=3, pad=1),
    "3x3_scale2": dict(B=2, G=2, D=4, H=8, W=9, kernel=3, pad=1, offset_scale=2.0),
    "3x5": dict(B=2, G=2, D=4, H=6, W=9, kernel=(3, 5), pad=(1, 2)),
    "5x3_s2_d2": dict(B=2, G=2, D=4, H=9, W=8, kernel=(5, 3), stride=2, pad=(2, 1), dilation=2, offset_scale=0.5),
}
ATTN = dict(N=1, M=2, D=4, shapes=[(8, 4), (2, 2), (1, 1)], P=2)
# (at zero offsets the stride-2 geometry has no sample at -1: it runs the modes that move the samples)
CASES = [(n, m) for n in sorted(LATTICE) for m in R3.LATTICE_MODES if (n, m) != ("5x3_s2_d2", "zero")]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_direct_equals_the_grid_sample_reference_off_the_lattice(name):
    x, off, m, go, geo = R3.make_inputs(dtype=F64, seed=11, offset_range=2.5, **SHAPES[name])
    want = R3.dcnv3_ref_grads(x, off, m, go, *geo)
    got = R3.dcnv3_direct_grads(x, off, m, go, *geo)
    for what, a, b in zip(NAMES, got, want):
        err = rel_err(a, b)
        print(name, what, "%.3e" % err)
        assert a.shape == b.shape and err <= 1e-10, (name, what, err)


@pytest.mark.parametrize("name, mode", CASES)
def test_three_statements_of_the_contract_agree_on_the_lattice(name, mode):
    """dcnv3_direct, dcnv4_ref (through pack) and the oracle's modulated 2-D operator: all four results, 1e-12."""
    x, off, m, go, geo = R3.make_lattice_inputs(mode, dtype=F64, seed=5, **LATTICE[name])
    G, K = geo[4], R4.taps(geo[0])
    direct = R3.dcnv3_direct_grads(x, off, m, go, *geo)
    out, gi, gom = R4.dcnv4_ref_grads(x, R4.pack(off, m, G, K), go, *geo, False)
    packed = (out, gi) + R4.unpack(gom, G, K)
    oracle = R3.dcnv3_oracle(x, off, m, go, *geo)
    for what, a, b, c in zip(NAMES, direct, packed, oracle):
        e4, eo = rel_err(b, a), rel_err(c, a)
        print(name, mode, what, "dcnv4_ref %.3e oracle %.3e" % (e4, eo))
        assert a.shape == b.shape == c.shape and e4 <= 1e-12 and eo <= 1e-12, (name, mode, what, e4, eo)


def _pair_dot(out, go, heads):
    """<grad_output, output> per pair (the last axis split into ``heads`` heads)."""
    p = (out.double() * go.double())
    return p.reshape(p.shape[:-1] + (heads, -1)).sum(-1)


def _check_convention(tag, grad, fd, gated_in, zero_too=()):
    """``grad`` and ``fd`` [..., taps, 2]; ``gated_in`` [..., taps]: the forward difference where the gate is passed, exact
    zeros -- in ``grad`` and in every tensor of ``zero_too`` [..., taps] -- where it is not."""
    assert bool(gated_in.any()) and bool((~gated_in).any()), tag
    scale = max(1.0, float(grad.abs().max()))
    err = float((grad - fd)[gated_in].abs().max()) / scale
    print(tag, "forward difference: %.3e of %.3e" % (err, scale))
    assert err <= 1e-9, (tag, err)
    assert float(grad[~gated_in].abs().max()) == 0.0, tag
    for z in zero_too:
        assert float(z[~gated_in].abs().max()) == 0.0, tag


@pytest.mark.parametrize("ref", ["dcnv3_direct", "dcnv4_ref"])
@pytest.mark.parametrize("name, mode", [c for c in CASES if c[0] in ("3x3", "5x3_s2_d2")])
def test_right_sided_convention_of_the_dcn_references(name, ref, mode):
    x, off, m, go, geo = R3.make_lattice_inputs(mode, dtype=F64, seed=6, **LATTICE[name])
    G, K = geo[4], R4.taps(geo[0])
    H, W = x.shape[1:3]
    if ref == "dcnv3_direct":
        fwd = lambda o: R3.dcnv3_direct(x, o, m, *geo)
        _, _, goff, gm = R3.dcnv3_direct_grads(x, off, m, go, *geo)
    else:
        fwd = lambda o: R4.dcnv4_ref(x, R4.pack(o, m, G, K), *geo)
        goff, gm = R4.unpack(R4.dcnv4_ref_grads(x, R4.pack(off, m, G, K), go, *geo)[2], G, K)
    shape = off.shape[:3] + (G, K, 2)
    base = _pair_dot(fwd(off), go, G)
    fd = torch.zeros(shape, dtype=F64)
    for t in range(K):
        for a in (0, 1):
            o = off.clone().reshape(shape)
            o[..., t, a] += STEP
            fd[..., t, a] = (_pair_dot(fwd(o.reshape(off.shape)), go, G) - base) / STEP
    gated_in = R3.gate_of(off, H, W, *geo[:4], G, geo[6])
    # a sample at loc == -1 enters the image under the step: its difference is not zero, its gradient is
    loc_h, loc_w = R3.positions(off, H, W, *geo[:4], G, geo[6])
    edge = ((loc_h == -1) & (loc_w > -1) & (loc_w < W)) | ((loc_w == -1) & (loc_h > -1) & (loc_h < H))
    assert bool(edge.any()) and float(fd[edge].abs().max()) > 0
    _check_convention("%s %s %s" % (name, ref, mode), goff.reshape(shape), fd, gated_in, [gm.reshape(shape[:-1])])


def test_right_sided_convention_of_the_attention_references():
    """msda_direct, and fda_ref_grads(fn=msda_direct): the location gradients.  (The packed operator's logit gradient of a
    gated-out tap is -a * S, not zero: the softmax couples the taps.)"""
    value, loc, attn, go = RM.make_lattice_inputs(dtype=F64, coord_dtype=torch.float32, seed=7, **ATTN)
    loc = loc.double()
    shapes, M, P = ATTN["shapes"], ATTN["M"], ATTN["P"]
    L = len(shapes)
    gated_in = RM.gate_of(loc, shapes).flatten(-2)
    _, _, gl, ga = RM.msda_ref_grads(value, shapes, loc, attn, go, fn=RM.msda_direct)
    la = RF.pack(loc, torch.randn(attn.shape, generator=torch.Generator().manual_seed(8), dtype=F64) * 3)
    _, _, gla = RF.fda_ref_grads(value, shapes, la, P, go, fn=RM.msda_direct)
    for tag, fwd, grad, zero_too in (
            ("msda_direct", lambda lc: RM.msda_direct(value, shapes, lc, attn), gl, [ga.flatten(-2)]),
            ("fda_ref", lambda lc: RF.fda_ref(value, shapes, RF.pack(lc, RF.unpack(la, L, P)[1]), P, fn=RM.msda_direct),
             RF.unpack(gla, L, P)[0], [])):
        base = _pair_dot(fwd(loc), go, M)
        fd = torch.zeros_like(loc)
        for l in range(L):
            for p in range(P):
                for a in (0, 1):
                    lc = loc.clone()
                    lc[:, :, :, l, p, a] += STEP
                    fd[:, :, :, l, p, a] = (_pair_dot(fwd(lc), go, M) - base) / STEP
        _check_convention(tag, grad.flatten(3, 4), fd.flatten(3, 4), gated_in, zero_too)


def test_grid_sample_references_are_no_reference_on_the_lattice():
    """Recorded so that nobody moves the lattice tests back onto them: on integer positions ``dcnv3_ref`` and ``msda_ref``
    agree with the floor-based references on the output, grad_input and the factor gradient, and differ in the coordinate
    gradient by more than 1.0 -- fp64 rounding inside ``grid_sample`` lands on either side of the integer, and it has no
    gate at -1."""
    x, off, m, go, geo = R3.make_lattice_inputs("zero", dtype=F64, seed=5, **LATTICE["3x3"])
    a, b = R3.dcnv3_ref_grads(x, off, m, go, *geo), R3.dcnv3_direct_grads(x, off, m, go, *geo)
    for i in (0, 1, 3):
        assert rel_err(a[i], b[i]) <= 1e-12, NAMES[i]
    diff = float((a[2] - b[2]).abs().max())
    print("dcnv3_ref against dcnv3_direct, zero offsets: grad_offset differs by %.2f of %.2f" % (diff, float(b[2].abs().max())))
    assert diff > 1.0
    value, loc, attn, go = RM.make_lattice_inputs(dtype=F64, coord_dtype=torch.float32, seed=7, **ATTN)
    a = RM.msda_ref_grads(value, ATTN["shapes"], loc, attn, go)
    b = RM.msda_ref_grads(value, ATTN["shapes"], loc, attn, go, fn=RM.msda_direct)
    diff = float((a[2] - b[2]).abs().max())
    print("msda_ref against msda_direct: grad_sampling_locations differs by %.2f of %.2f" % (diff, float(b[2].abs().max())))
    assert diff > 1.0
