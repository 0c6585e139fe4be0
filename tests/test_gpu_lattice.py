"""The four sampling operators ON the lattice (include/mdconv.h; csrc/samp_core.hpp): sampling positions that are whole
pixels, where every freshly constructed deformable layer starts training and where the bilinear interpolant has a kink.
The contract's derivative there is a convention -- the floor picks the cell, so it is the right-sided one, and a sample the
gate -1 < loc < size leaves out has zero gradient, loc == -1 and loc == size included -- and ``F.grid_sample`` does not
follow it (tests/test_lattice_cpu.py), so the references are the floor-based ones: ``dcnv3_direct``, ``dcnv4_ref``,
``msda_direct`` and ``fda_ref_grads(fn=msda_direct)``, in fp64 from the values the tensors hold.

Output and every gradient at the project's tolerances -- 1e-4 for fp32, ``TOL`` of tests/test_gpu_hp.py for fp16 / bf16,
value-typed results by the value dtype and coordinate gradients by the coordinate dtype -- with the backward in overwrite
mode into NaN-filled buffers, and for every gated-out sample the coordinate and factor gradients exactly 0.0 (the packed
attention's logit gradient is -a * S there and is compared).  The coordinate kernel and the list kernel each evaluate the
position themselves; on the lattice a disagreement between them moves a whole corner, so one case per operator runs with
the deterministic flag as well.  Then the four modules as constructed: one fp32 step and one step under autocast."""
import functools

import pytest
import torch

from tests import dcnv3_ref as R3
from tests import dcnv4_ref as R4
from tests import fda_ref as RF
from tests import msda_ref as RM
from tests.test_gpu_hp import TOL as TOL16
from tests.util import assert_close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(TOL16)
TOL[torch.float32] = 1e-4
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NAN = float("nan")

GEO = {
    # one lane per pair; odd extents
    "one_lane": dict(B=1, G=1, D=4, H=5, W=7, kernel=3, pad=1),
    # cross-lane sums of the coordinate gradients
    "g4_d16": dict(B=2, G=4, D=16, H=9, W=8, kernel=3, pad=1),
    # non-square kernel, stride 2, dilation 2, offset_scale 0.5: offsets of +-2 are whole pixels
    "rect": dict(B=2, G=3, D=8, H=6, W=5, kernel=(5, 3), stride=2, pad=(2, 1), dilation=2, offset_scale=0.5),
}
MODES = R3.LATTICE_MODES
DCN_CASES = ([("one_lane", F32, m) for m in MODES] + [("g4_d16", d, m) for d in (F32, F16, BF16) for m in MODES]
             + [("rect", F32, "integer"), ("rect", F16, "integer")])


def _dev(t):
    return tuple(v.to(DEV) for v in t)


def _nans(*like):
    return tuple(torch.full_like(v, NAN) for v in like)


def _compare(tag, names, got, want, tols):
    for what, a, b, tol in zip(names, got, want, tols):
        print("%s %s: max |want| %.3e" % (tag, what, float(b.abs().max())))
        assert_close("%s %s" % (tag, what), a, b, tol)


def _exact_zero(tag, t, where):
    bad = t.cpu()[where]
    assert bad.numel() > 0, tag
    assert float(bad.float().abs().max()) == 0.0 and not torch.isnan(bad.float()).any(), tag


# ---- DCNv3 ----
N3 = ("output", "grad_input", "grad_offset", "grad_mask")


@functools.lru_cache(maxsize=None)
def _case3(name, dtype, mode):
    x, off, m, go, geo = R3.make_lattice_inputs(mode, dtype=dtype, seed=len(name) + 3, **GEO[name])
    return (x, off, m, go), geo, R3.dcnv3_direct_grads(x, off, m, go, *geo)


def _native3(t, geo, deterministic=False):
    from modulated_deform_conv_amd import dcnv3
    x, off, m, go = t
    out = dcnv3.dcnv3_forward(x, off, m, *geo)
    g = dcnv3.dcnv3_backward(x, off, m, go, *geo, grads=_nans(x, off, m), accumulate=False, deterministic=deterministic)
    torch.cuda.synchronize()
    return (out,) + tuple(g)


@pytest.mark.parametrize("name, dtype, mode", DCN_CASES)
def test_dcnv3(name, dtype, mode):
    t, geo, want = _case3(name, dtype, mode)
    got = _native3(_dev(t), geo)
    _compare("dcnv3 %s %s %s" % (name, dtype, mode), N3, got, want, (TOL[dtype],) * 4)
    out_of_gate = ~R3.gate_of(t[1], t[0].shape[1], t[0].shape[2], *geo[:4], geo[4], geo[6])   # [B, Ho, Wo, G, K]
    _exact_zero("grad_mask", got[3].reshape(out_of_gate.shape), out_of_gate)
    _exact_zero("grad_offset", got[2].reshape(out_of_gate.shape + (2,)), out_of_gate)
    assert float(want[3].reshape(out_of_gate.shape)[out_of_gate].abs().max()) == 0.0


# ---- DCNv4 ----
N4 = ("output", "grad_input", "grad_offset_mask")
DCN4_CASES = ([(n, d, None, m, False, False) for n, d, m in DCN_CASES]
              + [("g4_d16", F32, None, "integer", True, False), ("rect", F32, None, "integer", True, False),
                 ("g4_d16", BF16, None, "one_axis", True, False),
                 ("g4_d16", BF16, F32, "integer", False, False), ("g4_d16", BF16, F32, "zero", False, False),
                 ("one_lane", F32, None, "integer", False, True), ("g4_d16", BF16, F32, "one_axis", False, True)])


@functools.lru_cache(maxsize=None)
def _case4(name, dtype, coord_dtype, mode, remove_center, nan_padding):
    x, om, go, geo = R4.make_lattice_inputs(mode, dtype=dtype, coord_dtype=coord_dtype, seed=len(name) + 3,
                                            remove_center=remove_center, nan_padding=nan_padding, **GEO[name])
    return (x, om, go), geo, R4.dcnv4_ref_grads(x, om, go, *geo)


def _native4(t, geo, deterministic=False):
    from modulated_deform_conv_amd import dcnv4
    x, om, go = t
    out = dcnv4.dcnv4_forward(x, om, *geo)
    g = dcnv4.dcnv4_backward(x, om, go, *geo, grads=_nans(x, om), accumulate=False, deterministic=deterministic)
    torch.cuda.synchronize()
    return (out,) + tuple(g)


@pytest.mark.parametrize("name, dtype, coord_dtype, mode, remove_center, nan_padding", DCN4_CASES)
def test_dcnv4(name, dtype, coord_dtype, mode, remove_center, nan_padding):
    t, geo, want = _case4(name, dtype, coord_dtype, mode, remove_center, nan_padding)
    G, K = geo[4], R4.taps(geo[0], remove_center)
    if nan_padding:
        assert t[1].shape[-1] > G * K * 3 and torch.isnan(t[1][..., G * K * 3:]).all()
    got = _native4(_dev(t), geo)
    assert got[2].dtype == t[1].dtype
    _compare("dcnv4 %s %s/%s %s rc=%d" % (name, dtype, coord_dtype, mode, remove_center), N4, got, want,
             (TOL[dtype], TOL[dtype], TOL[t[1].dtype]))
    out_of_gate = ~R4.gate_of(t[1], t[0].shape[1], t[0].shape[2], *geo[:4], G, geo[6], remove_center)
    goff, gm = R4.unpack(got[2].cpu(), G, K)
    _exact_zero("mask gradient", gm.reshape(out_of_gate.shape), out_of_gate)
    _exact_zero("offset gradient", goff.reshape(out_of_gate.shape + (2,)), out_of_gate)
    assert float(got[2][..., G * K * 3:].float().abs().sum()) == 0.0   # the padding columns: exact zeros in overwrite mode


# ---- attention ----
SHAPES = [(8, 4), (2, 2), (1, 1)]
HEADS = {"m2_d4": dict(M=2, D=4), "m8_d32": dict(M=8, D=32)}
ATTN_CASES = [("m2_d4", F32, None), ("m8_d32", F32, None), ("m8_d32", F16, None), ("m8_d32", BF16, None), ("m8_d32", BF16, F32)]
NM = ("output", "grad_value", "grad_sampling_locations", "grad_attention_weights")
NF = ("output", "grad_value", "grad_sampling_loc_attn")
P = 2


@functools.lru_cache(maxsize=None)
def _case_msda(name, dtype, coord_dtype):
    t = RM.make_lattice_inputs(N=1, shapes=SHAPES, P=P, dtype=dtype, coord_dtype=coord_dtype, seed=len(name) + 3, **HEADS[name])
    return t, RM.msda_ref_grads(t[0], SHAPES, t[1], t[2], t[3], fn=RM.msda_direct)


def _native_msda(t, deterministic=False):
    from modulated_deform_conv_amd import msda
    value, loc, attn, go = t
    out = msda.ms_deform_attn_forward(value, SHAPES, loc, attn)
    g = msda.ms_deform_attn_backward(value, SHAPES, loc, attn, go, grads=_nans(value, loc, attn), accumulate=False,
                                     deterministic=deterministic)
    torch.cuda.synchronize()
    return (out,) + tuple(g)


@pytest.mark.parametrize("name, dtype, coord_dtype", ATTN_CASES)
def test_msda(name, dtype, coord_dtype):
    t, want = _case_msda(name, dtype, coord_dtype)
    got = _native_msda(_dev(t))
    cdt = t[1].dtype
    _compare("msda %s %s/%s" % (name, dtype, coord_dtype), NM, got, want, (TOL[dtype], TOL[dtype], TOL[cdt], TOL[cdt]))
    out_of_gate = ~RM.gate_of(t[1], SHAPES)   # [N, Lq, M, L, P]
    _exact_zero("grad_attention_weights", got[3], out_of_gate)
    _exact_zero("grad_sampling_locations", got[2], out_of_gate)


@functools.lru_cache(maxsize=None)
def _case_fda(name, dtype, coord_dtype):
    t = RF.make_lattice_inputs(N=1, shapes=SHAPES, P=P, dtype=dtype, coord_dtype=coord_dtype, seed=len(name) + 3, **HEADS[name])
    return t, RF.fda_ref_grads(t[0], SHAPES, t[1], P, t[2], fn=RM.msda_direct)


def _native_fda(t, deterministic=False):
    from modulated_deform_conv_amd import fda
    value, la, go = t
    out = fda.flash_deform_attn_forward(value, SHAPES, la, P)
    g = fda.flash_deform_attn_backward(value, SHAPES, la, P, go, grads=_nans(value, la), accumulate=False,
                                       deterministic=deterministic)
    torch.cuda.synchronize()
    return (out,) + tuple(g)


@pytest.mark.parametrize("name, dtype, coord_dtype", ATTN_CASES)
def test_fda(name, dtype, coord_dtype):
    t, want = _case_fda(name, dtype, coord_dtype)
    got = _native_fda(_dev(t))
    cdt = t[1].dtype
    _compare("fda %s %s/%s" % (name, dtype, coord_dtype), NF, got, want, (TOL[dtype], TOL[dtype], TOL[cdt]))
    loc, _ = RF.unpack(t[1], len(SHAPES), P)
    out_of_gate = ~RM.gate_of(loc, SHAPES)
    gloc, glogit = RF.unpack(got[2].cpu(), len(SHAPES), P)
    _exact_zero("location gradients", gloc, out_of_gate)
    # (the logit gradient of a gated-out tap is -a * S: compared above, and not zero)
    assert float(RF.unpack(want[2], len(SHAPES), P)[1][out_of_gate].abs().max()) > 0
    assert float(glogit[out_of_gate].float().abs().max()) > 0


# ---- the lists: built from the list kernel's own position evaluation ----
@pytest.mark.parametrize("op", ["dcnv3", "dcnv4", "msda", "fda"])
def test_deterministic_flag_on_the_lattice(op):
    """grad_input / grad_value through the scatter lists: within tolerance and bit-identical between two calls; the other
    results are those of the unflagged call bit for bit."""
    if op == "dcnv3":
        t, geo, want = _case3("g4_d16", F32, "integer")
        run = lambda **kw: _native3(_dev(t), geo, **kw)
    elif op == "dcnv4":
        t, geo, want = _case4("g4_d16", F32, None, "integer", True, False)
        run = lambda **kw: _native4(_dev(t), geo, **kw)
    elif op == "msda":
        t, want = _case_msda("m8_d32", F32, None)
        run = lambda **kw: _native_msda(_dev(t), **kw)
    else:
        t, want = _case_fda("m8_d32", F32, None)
        run = lambda **kw: _native_fda(_dev(t), **kw)
    first, second, plain = run(deterministic=True), run(deterministic=True), run()
    assert_close("%s deterministic grad_input" % op, first[1], want[1], 1e-4)
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), "%s: result %d differs between two deterministic calls" % (op, i)
    for i in [0] + list(range(2, len(first))):
        assert torch.equal(first[i], plain[i]), "%s: result %d differs from the unflagged call" % (op, i)


# ---- the modules as constructed ----
def _step(mod, autocast, call, tensors, go):
    mod.zero_grad(set_to_none=True)
    leaves = [v.clone().requires_grad_(True) for v in tensors]
    if autocast:
        with torch.autocast("cuda", dtype=BF16):
            y = call(*leaves)
        assert y.dtype == BF16
    else:
        y = call(*leaves)
    y.backward(go.to(y.dtype))
    torch.cuda.synchronize()
    res = dict(output=y.detach(), **{"grad_leaf%d" % i: v.grad for i, v in enumerate(leaves)},
               **{k: p.grad for k, p in mod.named_parameters()})
    assert all(v is not None for v in res.values())
    return res


def _compare_steps(tag, native, ref, tol):
    assert sorted(native) == sorted(ref)
    for k in native:
        assert_close("%s %s" % (tag, k), native[k], ref[k], tol)


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
def test_fresh_dcnv3_module(autocast):
    """DCNv3 as constructed: the offset linear is zero, every sample sits on the lattice; what this pins is the gradient
    of that linear's weight and bias, the first thing the layer learns from."""
    from modulated_deform_conv_amd import DCNv3, dcnv3_core
    torch.manual_seed(31)
    mod = DCNv3(channels=32, kernel_size=3, group=4, offset_scale=1.0).to(DEV)
    x = torch.randn(2, 6, 5, 32, device=DEV)
    go = torch.randn(2, 6, 5, 32, device=DEV)
    seen = []

    def native(xx, off, m, *geo):
        seen.append(float(off.abs().max()))
        return dcnv3_core(xx, off, m, *geo)

    res = []
    for core in (native, R3.dcnv3_direct):
        mod._core = core
        res.append(_step(mod, autocast, mod, (x,), go))
    assert seen == [0.0]
    assert float(res[1]["offset.weight"].abs().max()) > 0 and float(res[1]["offset.bias"].abs().max()) > 0
    _compare_steps("DCNv3", res[0], res[1], TOL[BF16] if autocast else 1e-4)


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
def test_fresh_dcnv4_module(autocast):
    """DCNv4 as constructed: the offset_mask linear is zero -- offsets on the lattice, and masks of zero, so what reaches
    that linear is the mask columns' gradient (the samples themselves) and exact zeros in the offset columns."""
    from modulated_deform_conv_amd import DCNv4, dcnv4_core
    torch.manual_seed(32)
    mod = DCNv4(channels=32, kernel_size=3, group=4, offset_scale=1.0, dw_kernel_size=3, remove_center=True).to(DEV)
    x = torch.randn(2, 6 * 5, 32, device=DEV)
    go = torch.randn(2, 6 * 5, 32, device=DEV)
    seen = []

    def native(xx, om, *geo):
        seen.append(float(om.abs().max()))
        return dcnv4_core(xx, om, *geo)

    res = []
    for core in (native, R4.dcnv4_ref):
        mod._core = core
        res.append(_step(mod, autocast, lambda v: mod(v, shape=(6, 5)), (x,), go))
    assert seen == [0.0]
    assert float(res[1]["offset_mask.bias"].abs().max()) > 0
    _compare_steps("DCNv4", res[0], res[1], TOL[BF16] if autocast else 1e-4)


def _attention_inputs():
    """Power-of-two levels, reference points at pixel centres (every pixel coordinate -1 .. size of every level among them),
    and -- by the caller -- zeroed sampling offsets: the attention modules' directional bias is not on the lattice."""
    N, C = 2, 32
    S = sum(h * w for h, w in SHAPES)
    Lq = 12
    ref = torch.zeros(N, Lq, len(SHAPES), 2)
    for l, (h, w) in enumerate(SHAPES):
        for q in range(Lq):
            ref[:, q, l, 0] = ((q % (w + 2)) - 1 + 0.5) / w
            ref[:, q, l, 1] = (((q // 2) % (h + 2)) - 1 + 0.5) / h
    query = torch.randn(N, Lq, C, device=DEV)
    flat = torch.randn(N, S, C, device=DEV)
    pad = torch.zeros(N, S, dtype=torch.bool, device=DEV)
    pad[1, 5:9] = True
    go = torch.randn(N, Lq, C, device=DEV)
    starts = [0, 32, 36]
    return query, flat, ref.to(DEV), pad, go, starts


def _on_lattice(loc):
    x, y = RM.pixel_positions(loc, SHAPES)
    return float(torch.stack([x - x.round(), y - y.round()]).abs().max()) == 0.0 and float(x.min()) == -1.0


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
def test_fresh_msda_module(autocast):
    from modulated_deform_conv_amd import MSDeformAttn, ms_deform_attn
    torch.manual_seed(33)
    mod = MSDeformAttn(d_model=32, n_levels=3, n_heads=4, n_points=2).to(DEV)
    with torch.no_grad():
        mod.sampling_offsets.bias.zero_()
    query, flat, ref_pts, pad, go, starts = _attention_inputs()
    seen = []

    def native(value, shapes, loc, attn, st):
        seen.append(_on_lattice(loc))
        return ms_deform_attn(value, shapes, loc, attn, st)

    res = []
    for core in (native, lambda value, shapes, loc, attn, st: RM.msda_direct(value, shapes, loc, attn)):
        mod._core = core
        res.append(_step(mod, autocast, lambda q, f, r: mod(q, r, f, SHAPES, starts, pad), (query, flat, ref_pts), go))
    assert seen == [True]
    assert float(res[1]["sampling_offsets.weight"].abs().max()) > 0
    _compare_steps("MSDeformAttn", res[0], res[1], TOL[BF16] if autocast else 1e-4)


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
def test_fresh_fda_module(autocast):
    from modulated_deform_conv_amd import FlashDeformAttn, flash_deform_attn
    torch.manual_seed(34)
    mod = FlashDeformAttn(d_model=32, n_levels=3, n_heads=4, n_points=2).to(DEV)
    with torch.no_grad():
        mod.sampling_offsets.bias.zero_()
    query, flat, ref_pts, pad, go, starts = _attention_inputs()
    seen = []

    def native(value, shapes, la, points, st):
        seen.append(_on_lattice(RF.unpack(la, len(SHAPES), points)[0]))
        return flash_deform_attn(value, shapes, la, points, st)

    res = []
    for core in (native, lambda value, shapes, la, points, st: RF.fda_ref(value, shapes, la, points, fn=RM.msda_direct)):
        mod._core = core
        res.append(_step(mod, autocast, lambda q, f, r: mod(q, r, f, SHAPES, starts, pad), (query, flat, ref_pts), go))
    assert seen == [True]
    assert float(res[1]["sampling_offsets.weight"].abs().max()) > 0
    _compare_steps("FlashDeformAttn", res[0], res[1], TOL[BF16] if autocast else 1e-4)
