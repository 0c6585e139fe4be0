"""3-D multi-scale deformable attention on the GPU (include/mdconv.h, "3-D multi-scale deformable attention"): output and
the three gradients against ``tests.msda3d_ref.msda3d_ref`` (the per-level 5-D ``F.grid_sample`` composition) evaluated in
fp64 from the inputs as the kernel sees them (16-bit inputs rounded first), at the project's tolerances -- 1e-4 for fp32,
``TOL`` of tests/test_gpu_hp.py for fp16 / bf16, by the value dtype for value-typed results and by the coordinate dtype for
the two coordinate gradients -- on the smallest shapes at which each part can go wrong; a cross-pin against the 2-D operator
on levels of depth 1; the lattice against ``msda3d_direct``; and the call modes: accumulate, NO_GRAD_INPUT under a guarded
workspace, determinism, graph replay, the module under autocast, selective backward."""
import functools

import pytest
import torch

from tests import msda3d_ref as R
from tests import msda_ref as R2
from tests.test_gpu_hp import TOL as TOL16
from tests.util import assert_close, guarded_run

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(TOL16)
TOL[torch.float32] = 1e-4
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NAN = float("nan")

CASES = {
    # one lane per (query, head); three different odd extents; border corners
    "one_lane": dict(N=1, M=1, D=4, shapes=[(3, 5, 7)], Lq=3, P=1),
    # (x, y, z) order, W / H / T scaling, level starts, a one-voxel level, K = 6 not a multiple of VL
    "rect_levels": dict(N=2, M=3, D=8, shapes=[(4, 6, 5), (2, 3, 3), (1, 1, 1)], Lq=7, P=2),
    # K = 16 in several tap batches; butterflies of 8 / 4 lanes
    "m8_d32": dict(N=2, M=8, D=32, shapes=[(4, 4, 4), (2, 2, 2), (1, 2, 2), (1, 1, 1)], Lq=10, P=4),
    # 16 lanes per pair, 3 taps: idle state builders
    "k_below_vl": dict(N=1, M=2, D=64, shapes=[(2, 4, 4)], Lq=5, P=3),
    # three vectors per head in four lanes (one idle lane per pair in the butterfly)
    "three_vectors": dict(N=1, M=2, D=12, shapes=[(2, 5, 4), (1, 2, 3)], Lq=5, P=2),
    # 65 vectors per head: 64 lanes, two rounds
    "two_rounds": dict(N=1, M=1, D=260, shapes=[(2, 3, 4)], Lq=4, P=2),
    "two_rounds_16bit": dict(N=1, M=1, D=520, shapes=[(2, 3, 4)], Lq=4, P=2),
    # the whole level select: eight levels of at most 12 voxels, mixed extents
    "eight_levels": dict(N=1, M=1, D=4, shapes=[(1, 3, 2), (2, 2, 3), (3, 1, 4), (1, 4, 1), (2, 2, 2), (1, 1, 1), (3, 2, 2),
                                                (2, 1, 5)], Lq=6, P=1),
    # eight long lists: every sample of level 0 lands between voxels (1, 1, 1) and (2, 2, 2); empty rows elsewhere
    "crafted": dict(N=2, M=1, D=4, shapes=[(4, 4, 4), (2, 2, 2)], Lq=40, P=3),
    "far": dict(N=1, M=2, D=4, shapes=[(2, 8, 8), (3, 3, 3)], Lq=6, P=2),
}
CRAFTED_ROWS = [(z * 4 + y) * 4 + x for z in (1, 2) for y in (1, 2) for x in (1, 2)]
CRAFTED_EMPTY = [0, 3, 12, 15, 48, 51, 60, 63]   # the corners of level 0


@functools.lru_cache(maxsize=None)
def _case(name, dtype, coord_dtype=None):
    """CPU inputs of a case and its fp64 reference (output and the three gradients), computed once."""
    kw = CASES[name]
    shapes = kw["shapes"]
    value, loc, attn, go = R.make_inputs(dtype=dtype, coord_dtype=coord_dtype, seed=len(name) + 7, **kw)
    if name == "crafted":
        # level 0 (4 x 4 x 4): x = 1.3, y = 1.4, z = 1.6 in voxels is loc = (coordinate + 0.5) / size
        loc[:, :, :, 0, :, 0] = (1.3 + 0.5) / 4
        loc[:, :, :, 0, :, 1] = (1.4 + 0.5) / 4
        loc[:, :, :, 0, :, 2] = (1.6 + 0.5) / 4
    if name == "far":
        gen = torch.Generator().manual_seed(5)
        loc = torch.where(torch.rand(loc.shape, generator=gen) < 0.5, -3.0, 4.0).to(loc.dtype)
    else:
        assert R.min_lattice_distance(loc, shapes) >= R.MARGIN
    return (value, loc, attn, go), shapes, R.msda3d_ref_grads(value, shapes, loc, attn, go)


def _native(t, shapes, grads=None, need_grad_value=True, deterministic=False, accumulate=None):
    from modulated_deform_conv_amd import msda3d
    value, loc, attn, go = t
    out = msda3d.ms_deform_attn_3d_forward(value, shapes, loc, attn)
    g = msda3d.ms_deform_attn_3d_backward(value, shapes, loc, attn, go, grads=grads, need_grad_value=need_grad_value,
                                          deterministic=deterministic, accumulate=accumulate)
    torch.cuda.synchronize()
    return (out,) + tuple(g)


def _dev(t):
    return tuple(v.to(DEV) for v in t)


def _nans(*like):
    return tuple(torch.full_like(v, NAN) for v in like)


NAMES = ("output", "grad_value", "grad_sampling_locations", "grad_attention_weights")


def _tols(t):
    """Per result: value-typed results by the value dtype, the coordinate gradients by the coordinate dtype."""
    return (TOL[t[0].dtype], TOL[t[0].dtype], TOL[t[1].dtype], TOL[t[1].dtype])


def _compare(tag, got, want, tols):
    for what, a, b, tol in zip(NAMES, got, want, tols):
        if a is None:
            continue
        print("%s %s: max |want| %.3e" % (tag, what, float(b.abs().max())))
        assert_close("%s %s" % (tag, what), a, b, tol)


def _exact_zero(tag, t, where=None):
    bad = t.cpu() if where is None else t.cpu()[where]
    assert bad.numel() > 0, tag
    assert float(bad.float().abs().max()) == 0.0 and not torch.isnan(bad.float()).any(), tag


@pytest.mark.parametrize("name, dtype, coord_dtype", [
    ("one_lane", F32, None), ("rect_levels", F32, None), ("rect_levels", F16, None),
    ("m8_d32", F32, None), ("m8_d32", F16, None), ("m8_d32", BF16, None), ("m8_d32", F16, F32), ("m8_d32", BF16, F32),
    ("k_below_vl", F32, None), ("three_vectors", F32, None), ("two_rounds", F32, None), ("two_rounds_16bit", F16, None),
    ("eight_levels", F32, None), ("crafted", F32, None),
])
def test_against_reference(name, dtype, coord_dtype):
    t, shapes, want = _case(name, dtype, coord_dtype)
    got = _native(_dev(t), shapes)
    assert got[0].dtype == got[1].dtype == dtype and got[2].dtype == got[3].dtype == (coord_dtype or dtype)
    _compare("%s %s/%s" % (name, dtype, coord_dtype), got, want, _tols(t))


def test_crafted_lists():
    """The crafted case is what it claims: eight value rows of level 0 take every sample of that level, and rows that no
    sample touches exist -- their grad_value is exactly zero in overwrite mode, over NaN-filled buffers."""
    t, shapes, want = _case("crafted", F32)
    gv = want[1]
    assert float(gv[:, CRAFTED_ROWS].abs().min()) > 0 and float(gv[:, CRAFTED_EMPTY].abs().max()) == 0.0
    dt = _dev(t)
    got = _native(dt, shapes, grads=_nans(*dt[:3]), accumulate=False, deterministic=True)
    _exact_zero("untouched rows", got[1][:, CRAFTED_EMPTY])
    _compare("crafted deterministic", got, want, _tols(t))


@pytest.mark.parametrize("side", [-0.4, 1.2])
def test_one_axis_out(side):
    """The geometry of one_lane, each sample outside along exactly one axis -- x, y and z in turn: query q leaves along axis
    q -- and inside on the other two: a gate or a corner rule missing on one axis reads something.  Everything is exactly
    zero."""
    kw = CASES["one_lane"]
    shapes = kw["shapes"]
    value, loc, attn, go = R.make_inputs(dtype=F32, seed=3, **kw)
    assert loc.shape == (1, 3, 1, 1, 1, 3)
    loc = loc.clamp(0.2, 0.8)
    for q in range(3):
        loc[:, q, ..., q] = side
    x, y, z = R.pixel_positions(loc, shapes)
    out_axes = torch.stack([(x <= -1) | (x >= 7), (y <= -1) | (y >= 5), (z <= -1) | (z >= 3)], -1).reshape(3, 3)
    assert torch.equal(out_axes, torch.eye(3, dtype=torch.bool))
    want = R.msda3d_ref_grads(value, shapes, loc, attn, go)
    assert all(float(w.abs().max()) == 0.0 for w in want)
    dt = _dev((value, loc, attn, go))
    got = _native(dt, shapes, grads=_nans(*dt[:3]), accumulate=False)
    for what, g in zip(NAMES, got):
        _exact_zero("one axis out (%s): %s" % (side, what), g)


def test_samples_wholly_outside():
    """Locations of -3 / +4: nothing is read, the output and every gradient are exactly zero, the lists are empty."""
    t, shapes, want = _case("far", F32)
    assert all(float(w.abs().max()) == 0.0 for w in want)
    dt = _dev(t)
    got = _native(dt, shapes, grads=_nans(*dt[:3]), accumulate=False)
    for what, g in zip(NAMES, got):
        _exact_zero("far %s" % what, g)


def test_cross_pin_against_the_2d_operator():
    """Levels of depth 1 with loc_z = 0.5, that is z = 0 exactly: output, grad_value, grad_attention_weights and the x, y
    columns of the location gradient are those of ``ms_deform_attn`` on the same (H, W) levels (1e-4, fp32).  The z column is
    the lattice convention and is not compared."""
    from modulated_deform_conv_amd import msda
    shapes2 = [(6, 5), (3, 3), (1, 1)]
    shapes3 = [(1, h, w) for h, w in shapes2]
    value, loc2, attn, go = R2.make_inputs(N=2, M=3, D=8, shapes=shapes2, Lq=7, P=2, dtype=F32, seed=17)
    loc3 = torch.cat([loc2, torch.full(loc2.shape[:-1] + (1,), 0.5)], -1)
    assert float(R.pixel_positions(loc3, shapes3)[2].abs().max()) == 0.0
    v, l2, l3, a, g = (x.to(DEV) for x in (value, loc2, loc3, attn, go))
    want = (msda.ms_deform_attn_forward(v, shapes2, l2, a),) + tuple(msda.ms_deform_attn_backward(v, shapes2, l2, a, g))
    got = _native((v, l3, a, g), shapes3)
    torch.cuda.synchronize()
    assert float(want[0].abs().max()) > 0
    assert_close("cross-pin output", got[0], want[0].double().cpu(), 1e-4)
    assert_close("cross-pin grad_value", got[1], want[1].double().cpu(), 1e-4)
    assert_close("cross-pin grad_sampling_locations (x, y)", got[2][..., :2], want[2].double().cpu(), 1e-4)
    assert_close("cross-pin grad_attention_weights", got[3], want[3].double().cpu(), 1e-4)


# ---- on the lattice ----
LATTICE_SHAPES = [(2, 4, 2), (1, 2, 2)]
HEADS = {"m2_d4": dict(M=2, D=4), "m8_d32": dict(M=8, D=32)}


@functools.lru_cache(maxsize=None)
def _lattice_case(name, dtype, coord_dtype):
    t = R.make_lattice_inputs(N=1, shapes=LATTICE_SHAPES, P=2, dtype=dtype, coord_dtype=coord_dtype, seed=len(name) + 3,
                              **HEADS[name])
    fwd = R.msda3d_ref(t[0].double(), LATTICE_SHAPES, t[1].double(), t[2].double())
    return t, fwd, R.msda3d_ref_grads(t[0], LATTICE_SHAPES, t[1], t[2], t[3], fn=R.msda3d_direct)


@pytest.mark.parametrize("name, dtype, coord_dtype", [
    ("m2_d4", F32, None), ("m8_d32", F32, None), ("m8_d32", F16, None), ("m8_d32", BF16, None), ("m8_d32", BF16, F32)])
def test_on_the_lattice(name, dtype, coord_dtype):
    """Every voxel coordinate an integer, -1 .. size on each axis, and -1 + one ulp with fp32 coordinates: the forward against
    ``msda3d_ref``, the three gradients against ``msda3d_direct`` (``F.grid_sample`` is no reference there), gated-out samples
    exactly zero over NaN-filled buffers."""
    t, fwd, want = _lattice_case(name, dtype, coord_dtype)
    dt = _dev(t)
    got = _native(dt, LATTICE_SHAPES, grads=_nans(*dt[:3]), accumulate=False)
    assert_close("lattice output against grid_sample", got[0], fwd, TOL[dtype])
    _compare("lattice %s %s/%s" % (name, dtype, coord_dtype), got, want, _tols(t))
    out_of_gate = ~R.gate_of(t[1], LATTICE_SHAPES)   # [N, Lq, M, L, P]
    _exact_zero("grad_attention_weights", got[3], out_of_gate)
    _exact_zero("grad_sampling_locations", got[2], out_of_gate)
    assert float(want[3][out_of_gate].abs().max()) == 0.0 and float(want[2][out_of_gate].abs().max()) == 0.0


# ---- call modes ----
def test_accumulate_against_overwrite():
    """The three gradients added to non-zero buffers, fp16 values with fp32 coordinates: each buffer + gradient in its own
    dtype, rounded once."""
    t, shapes, want = _case("m8_d32", F16, F32)
    dt = _dev(t)
    gen = torch.Generator().manual_seed(9)
    base = tuple(torch.randn(v.shape, generator=gen).to(v.dtype) for v in t[:3])
    bufs = tuple(b.to(DEV) for b in base)
    got = _native(dt, shapes, grads=bufs)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got[1:], bufs))
    assert (bufs[0].dtype, bufs[1].dtype, bufs[2].dtype) == (F16, F32, F32)
    for what, a, b, w, tol in zip(NAMES[1:], got[1:], base, want[1:], _tols(t)[1:]):
        assert_close("accumulate %s" % what, a, b.double() + w, tol)
    # overwrite mode ignores what the buffers hold
    over = _native(dt, shapes)
    _compare("overwrite", over, want, _tols(t))


def _guard(monkeypatch, touched, calls):
    """tests.util.guarded_run in the place of msda3d._run; it sizes the workspace through ``mdconv_workspace_bytes`` of the
    library handle, which for this operator's descriptor is ``mdconv_msda3d_workspace_bytes``."""
    from modulated_deform_conv_amd import _capi, msda3d
    real = _capi.lib()

    class Lib:
        mdconv_workspace_bytes = staticmethod(real.mdconv_msda3d_workspace_bytes)

        def __getattr__(self, name):
            return getattr(real, name)

    proxy = Lib()
    monkeypatch.setattr(_capi, "lib", lambda: proxy)
    monkeypatch.setattr(msda3d, "_run", guarded_run(touched, calls))


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (BF16, F32)])
def test_no_grad_value_under_the_guarded_workspace(monkeypatch, dtype, coord_dtype):
    """NO_GRAD_INPUT: grad_value NULL, no workspace between pattern-filled margins; the coordinate gradients are bit for
    bit those of the full call.  The full and the deterministic call run guarded as well: the figure is exact."""
    t, shapes, want = _case("m8_d32", dtype, coord_dtype)
    dt = _dev(t)
    full = _native(dt, shapes)
    touched, calls = [], []
    _guard(monkeypatch, touched, calls)
    part = _native(dt, shapes, need_grad_value=False)
    again = _native(dt, shapes)
    det = _native(dt, shapes, deterministic=True)
    assert touched == [], touched
    sizes = [b for name, b in calls if name == "mdconv_msda3d_backward"]
    assert [b for name, b in calls if name == "mdconv_msda3d_forward"] == [0, 0, 0]
    assert sizes[0] == 0 < sizes[1] <= sizes[2], sizes
    assert part[1] is None
    for i in (0, 2, 3):
        assert torch.equal(part[i], full[i]) and torch.equal(again[i], full[i]) and torch.equal(det[i], full[i]), NAMES[i]
    _compare("guarded full", again, want, _tols(t))
    _compare("guarded deterministic", det, want, _tols(t))


@pytest.mark.parametrize("name, dtype, coord_dtype", [("crafted", F32, None), ("m8_d32", F32, None), ("m8_d32", F16, F32)])
def test_deterministic_mode(name, dtype, coord_dtype):
    """With the flag all four results are bit-identical between two eager runs and two replays of a HIP graph that holds
    forward + backward into caller buffers; without it the output and the coordinate gradients are as well and
    grad_value is within tolerance."""
    from modulated_deform_conv_amd import msda3d
    t, shapes, want = _case(name, dtype, coord_dtype)
    value, loc, attn, go = dt = _dev(t)
    first = _native(dt, shapes, deterministic=True)
    second = _native(dt, shapes, deterministic=True)
    for what, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), "deterministic %s differs between two runs" % what
    plain = [_native(dt, shapes) for _ in range(2)]
    for i in (0, 2, 3):
        assert torch.equal(plain[0][i], plain[1][i]) and torch.equal(plain[0][i], first[i]), NAMES[i]
    assert_close("unflagged grad_value", plain[0][1], want[1], TOL[dtype])
    _compare("deterministic", first, want, _tols(t))

    out = torch.empty_like(first[0])
    bufs = tuple(torch.empty_like(v) for v in (value, loc, attn))

    def step():
        msda3d.ms_deform_attn_3d_forward(value, shapes, loc, attn, output=out)
        for b in bufs:   # caller-allocated buffers are added to
            b.zero_()
        msda3d.ms_deform_attn_3d_backward(value, shapes, loc, attn, go, grads=bufs, deterministic=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(2):
        out.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for what, a, b in zip(NAMES, (out,) + bufs, first):
            assert torch.equal(a, b), "graph replay: %s differs from the eager deterministic run" % what


def test_module_step_under_autocast():
    """The MSDeformAttn3D module under torch.autocast(bfloat16), with a padding mask, against the same module with the core
    swapped for msda3d_ref: the Python surface and the autograd wiring (output, input gradients and every parameter
    gradient).  The core receives a bf16 value and fp32 coordinates: the mixed call."""
    from modulated_deform_conv_amd import MSDeformAttn3D, ms_deform_attn_3d
    torch.manual_seed(24)
    shapes = [(2, 4, 3), (2, 2, 2), (1, 2, 2)]
    starts = [0, 24, 32]
    S, N, Lq, C = 36, 2, 7, 32
    mod = MSDeformAttn3D(d_model=C, n_levels=3, n_heads=4, n_points=2).to(DEV)
    with torch.no_grad():   # offsets and weights that depend on the query
        mod.sampling_offsets.weight.normal_(0, 0.05)
        mod.attention_weights.weight.normal_(0, 0.2)
    query = torch.randn(N, Lq, C, device=DEV)
    flat = torch.randn(N, S, C, device=DEV)
    ref_pts = torch.rand(N, Lq, 3, 3, device=DEV) * 0.6 + 0.2
    pad = torch.zeros(N, S, dtype=torch.bool, device=DEV)
    pad[1, 20:26] = True
    pad[0, 34:] = True
    go = torch.randn(N, Lq, C, device=DEV)
    seen = []

    def native_core(value, spatial_shapes, loc, attn, level_starts):
        seen.append((value.dtype, loc.dtype, attn.dtype))
        return ms_deform_attn_3d(value, spatial_shapes, loc, attn, level_starts)

    results = []
    for core in (native_core, R.msda3d_ref):
        mod._core = core
        mod.zero_grad(set_to_none=True)
        qi, fi, ri = (v.clone().requires_grad_(True) for v in (query, flat, ref_pts))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = mod(qi, ri, fi, shapes, starts, pad)
        assert y.dtype == torch.bfloat16
        y.backward(go.to(y.dtype))
        torch.cuda.synchronize()
        results.append(dict(output=y.detach(), grad_query=qi.grad, grad_input=fi.grad, grad_reference=ri.grad,
                            **{k: p.grad for k, p in mod.named_parameters()}))
    assert seen == [(BF16, F32, F32)]
    native, ref = results
    assert all(v is not None for v in native.values())
    assert float(native["grad_input"][1, 20:26].abs().max()) == 0.0   # padded rows take no gradient
    assert float(native["grad_input"][0, 34:].abs().max()) == 0.0
    for k in native:
        assert_close("module %s" % k, native[k], ref[k], TOL[BF16])


def test_selective_backward_through_autograd():
    """``value`` needs no gradient: the backward runs with NO_GRAD_INPUT and still returns the other two; a tensor
    ``spatial_shapes`` and a host ``level_start_index`` are taken, a wrong one is refused."""
    from modulated_deform_conv_amd import MSDeformAttn3DFunction, ms_deform_attn_3d, msda3d
    t, shapes, want = _case("rect_levels", F32)
    value, loc, attn, go = _dev(t)
    loc.requires_grad_(True)
    attn.requires_grad_(True)
    flags = []
    real = msda3d.ms_deform_attn_3d_backward

    def spy(*args, **kw):
        flags.append(kw["need_grad_value"])
        return real(*args, **kw)

    msda3d.ms_deform_attn_3d_backward = spy
    try:
        out = MSDeformAttn3DFunction.apply(value, torch.tensor(shapes), torch.tensor([0, 120, 138]), loc, attn, 64)
        out.backward(go)
        assert value.grad is None
        assert_close("selective output", out.detach(), want[0], 1e-4)
        assert_close("selective grad_sampling_locations", loc.grad, want[2], 1e-4)
        assert_close("selective grad_attention_weights", attn.grad, want[3], 1e-4)
        with pytest.raises(ValueError):
            ms_deform_attn_3d(value, shapes, loc, attn, [0, 120, 139])
        # all three through autograd
        v2, l2, a2 = (v.detach().clone().requires_grad_(True) for v in (value, loc, attn))
        ms_deform_attn_3d(v2, shapes, l2, a2).backward(go)
        for what, a, b in zip(NAMES[1:], (v2.grad, l2.grad, a2.grad), want[1:]):
            assert_close("autograd %s" % what, a, b, 1e-4)
    finally:
        msda3d.ms_deform_attn_3d_backward = real
    assert flags == [False, True]
