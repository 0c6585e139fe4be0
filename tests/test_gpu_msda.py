"""Multi-scale deformable attention on the GPU (include/mdconv.h, "Multi-scale deformable attention"): output and the
three gradients against ``tests.msda_ref.msda_ref`` evaluated in fp64 from the inputs as the kernel sees them (16-bit inputs
rounded first), at the project's tolerances -- 1e-4 for fp32, ``TOL`` of tests/test_gpu_hp.py for fp16 / bf16, by the value
dtype for value-typed results and by the coordinate dtype for the two coordinate gradients -- on the smallest shapes at
which each part can go wrong, plus the call modes: accumulate, NO_GRAD_INPUT under a guarded workspace, determinism,
graph replay, and the module under autocast."""
import functools

import pytest
import torch

from tests import msda_ref as R
from tests.test_gpu_hp import TOL as TOL16
from tests.util import assert_close, guarded_run

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(TOL16)
TOL[torch.float32] = 1e-4
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16

CASES = {
    # one lane per (query, head); odd extents; border corners
    "one_lane": dict(N=1, M=1, D=4, shapes=[(5, 7)], Lq=3, P=1),
    # (x, y) order, W against H scaling, level starts, a 1x1 level, K = 6 not a multiple of VL
    "rect_levels": dict(N=2, M=3, D=8, shapes=[(6, 5), (3, 3), (1, 1)], Lq=7, P=2),
    # the canonical geometry; K = 16 in several tap batches; butterflies of 8 / 4 lanes
    "m8_d32": dict(N=2, M=8, D=32, shapes=[(8, 8), (4, 4), (2, 2), (1, 1)], Lq=10, P=4),
    # 16 lanes per pair, 3 taps: idle state builders
    "k_below_vl": dict(N=1, M=2, D=64, shapes=[(4, 4)], Lq=5, P=3),
    # three vectors per head in four lanes (one idle lane per pair in the butterfly)
    "three_vectors": dict(N=1, M=2, D=12, shapes=[(5, 4), (2, 3)], Lq=5, P=2),
    # 65 vectors per head: 64 lanes, two rounds
    "two_rounds": dict(N=1, M=1, D=260, shapes=[(3, 4)], Lq=4, P=2),
    "two_rounds_16bit": dict(N=1, M=1, D=520, shapes=[(3, 4)], Lq=4, P=2),
    # the whole level select
    "eight_levels": dict(N=1, M=1, D=4, shapes=[(3, 2), (2, 3), (1, 4), (4, 1), (2, 2), (1, 1), (3, 3), (2, 5)], Lq=6, P=1),
    # one long list per value row: every sample of level 0 lands between pixels (1, 1) and (2, 2); empty rows elsewhere
    "crafted": dict(N=2, M=1, D=4, shapes=[(4, 4), (2, 2)], Lq=40, P=3),
    "far": dict(N=1, M=2, D=4, shapes=[(8, 8), (3, 3)], Lq=6, P=2),
}


@functools.lru_cache(maxsize=None)
def _case(name, dtype, coord_dtype=None):
    """CPU inputs of a case and its fp64 reference (output and the three gradients), computed once."""
    kw = CASES[name]
    shapes = kw["shapes"]
    value, loc, attn, go = R.make_inputs(dtype=dtype, coord_dtype=coord_dtype, seed=len(name) + 7, **kw)
    if name == "crafted":
        # level 0 (4 x 4): x = 1.3, y = 1.4 in pixels is loc = (x + 0.5) / size
        loc[:, :, :, 0, :, 0] = (1.3 + 0.5) / 4
        loc[:, :, :, 0, :, 1] = (1.4 + 0.5) / 4
    if name == "far":
        gen = torch.Generator().manual_seed(5)
        loc = torch.where(torch.rand(loc.shape, generator=gen) < 0.5, -3.0, 4.0).to(loc.dtype)
    else:
        assert R.min_lattice_distance(loc, shapes) >= R.MARGIN
    return (value, loc, attn, go), shapes, R.msda_ref_grads(value, shapes, loc, attn, go)


def _native(t, shapes, grads=None, need_grad_value=True, deterministic=False):
    from modulated_deform_conv_amd import msda
    value, loc, attn, go = t
    out = msda.ms_deform_attn_forward(value, shapes, loc, attn)
    g = msda.ms_deform_attn_backward(value, shapes, loc, attn, go, grads=grads, need_grad_value=need_grad_value,
                                     deterministic=deterministic)
    torch.cuda.synchronize()
    return (out,) + tuple(g)


def _dev(t):
    return tuple(v.to(DEV) for v in t)


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
    """The crafted case is what it claims: four value rows of level 0 take every sample of that level, and rows that no
    sample touches exist -- their grad_value is exactly zero in overwrite mode."""
    t, shapes, want = _case("crafted", F32)
    gv = want[1]
    assert float(gv[:, [5, 6, 9, 10]].abs().min()) > 0 and float(gv[:, [0, 3, 12, 15]].abs().max()) == 0.0
    got = _native(_dev(t), shapes, deterministic=True)
    assert float(got[1][:, [0, 3, 12, 15]].abs().max()) == 0.0
    _compare("crafted deterministic", got, want, _tols(t))


def test_samples_wholly_outside():
    """Locations of -3 / +4: nothing is read, the output and every gradient are exactly zero, the lists are empty."""
    t, shapes, want = _case("far", F32)
    assert all(float(w.abs().max()) == 0.0 for w in want)
    got = _native(_dev(t), shapes)
    _compare("far", got, want, _tols(t))
    assert all(float(g.abs().max()) == 0.0 for g in got)


def test_forward_at_integer_positions():
    """Corner weights exactly 0 / 1 and both edges of the gate: locations (i + 0.5) / size on power-of-two extents give
    the pixel coordinate i exactly, i = -1 (gated out) .. size (gated out), with x = W - 1 inside, and x = -1 + one ulp,
    which reads column 0 with weight 2^-24.  Forward only: ``msda_ref`` (``F.grid_sample``) is no reference for the gradients
    on the lattice; the backward at these locations is tests/test_gpu_lattice.py, against ``msda_direct``."""
    from modulated_deform_conv_amd import msda
    shapes = [(8, 4), (2, 2)]
    N, M, D, P = 1, 2, 4, 2
    pts = []
    for l, (h, w) in enumerate(shapes):
        for ix in range(-1, w + 1):
            for iy in range(-1, h + 1):
                pts.append((l, (ix + 0.5) / w, (iy + 0.5) / h))
        just_inside = torch.nextafter(torch.tensor(-1.0), torch.tensor(0.0)).item()
        pts.append((l, (just_inside + 0.5) / w, (1 + 0.5) / h))
        pts.append((l, (1 + 0.5) / w, (just_inside + 0.5) / h))
    Lq = len(pts)
    gen = torch.Generator().manual_seed(3)
    value = torch.randn(N, sum(h * w for h, w in shapes), M, D, generator=gen)
    loc = torch.rand(N, Lq, M, len(shapes), P, 2, generator=gen)
    for q, (l, x, y) in enumerate(pts):
        loc[:, q, :, l, 0, 0], loc[:, q, :, l, 0, 1] = x, y
    attn = torch.softmax(torch.randn(N, Lq, M, len(shapes) * P, generator=gen), -1).view(N, Lq, M, len(shapes), P)
    x, y = R.pixel_positions(loc, shapes)
    on_lattice = ((x - x.round()).abs() == 0) & ((y - y.round()).abs() == 0)
    assert int(on_lattice.sum()) >= N * M * (Lq - 4) and float(x.min()) == -1.0
    want = R.msda_ref(value.double(), shapes, loc.double(), attn.double())
    assert rel_err_ok(R.msda_direct(value.double(), shapes, loc.double(), attn.double()), want)
    got = msda.ms_deform_attn_forward(value.to(DEV), shapes, loc.to(DEV), attn.to(DEV))
    assert_close("integer positions output", got, want, 1e-4)


def rel_err_ok(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


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
    """tests.util.guarded_run in the place of msda._run; it sizes the workspace through ``mdconv_workspace_bytes`` of the
    library handle, which for this operator's descriptor is ``mdconv_msda_workspace_bytes``."""
    from modulated_deform_conv_amd import _capi, msda
    real = _capi.lib()

    class Lib:
        mdconv_workspace_bytes = staticmethod(real.mdconv_msda_workspace_bytes)

        def __getattr__(self, name):
            return getattr(real, name)

    proxy = Lib()
    monkeypatch.setattr(_capi, "lib", lambda: proxy)
    monkeypatch.setattr(msda, "_run", guarded_run(touched, calls))


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
    sizes = [b for name, b in calls if name == "mdconv_msda_backward"]
    assert [b for name, b in calls if name == "mdconv_msda_forward"] == [0, 0, 0]
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
    from modulated_deform_conv_amd import msda
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
        msda.ms_deform_attn_forward(value, shapes, loc, attn, output=out)
        for b in bufs:   # caller-allocated buffers are added to
            b.zero_()
        msda.ms_deform_attn_backward(value, shapes, loc, attn, go, grads=bufs, deterministic=True)

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
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for what, a, b in zip(NAMES, (out,) + bufs, first):
            assert torch.equal(a, b), "graph replay: %s differs from the eager deterministic run" % what


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_module_step_under_autocast(ref_dim):
    """The MSDeformAttn module under torch.autocast(bfloat16), with a padding mask, against the same module with the core
    swapped for msda_ref: the Python surface and the autograd wiring (output, input gradients and every parameter
    gradient).  The core receives a bf16 value and fp32 coordinates: the mixed call."""
    from modulated_deform_conv_amd import MSDeformAttn, ms_deform_attn
    torch.manual_seed(21 + ref_dim)
    shapes = [(6, 5), (3, 3), (2, 2)]
    S, N, Lq, C = 43, 2, 7, 32
    mod = MSDeformAttn(d_model=C, n_levels=3, n_heads=4, n_points=2).to(DEV)
    with torch.no_grad():   # offsets and weights that depend on the query
        mod.sampling_offsets.weight.normal_(0, 0.05)
        mod.attention_weights.weight.normal_(0, 0.2)
    query = torch.randn(N, Lq, C, device=DEV)
    flat = torch.randn(N, S, C, device=DEV)
    ref_pts = torch.rand(N, Lq, 3, ref_dim, device=DEV) * 0.6 + 0.2
    pad = torch.zeros(N, S, dtype=torch.bool, device=DEV)
    pad[1, 25:30] = True
    pad[0, 41:] = True
    go = torch.randn(N, Lq, C, device=DEV)
    seen = []

    def native_core(value, spatial_shapes, loc, attn, starts):
        seen.append((value.dtype, loc.dtype, attn.dtype))
        return ms_deform_attn(value, spatial_shapes, loc, attn, starts)

    results = []
    for core in (native_core, R.msda_ref):
        mod._core = core
        mod.zero_grad(set_to_none=True)
        qi, fi, ri = (v.clone().requires_grad_(True) for v in (query, flat, ref_pts))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = mod(qi, ri, fi, shapes, [0, 30, 39], pad)
        assert y.dtype == torch.bfloat16
        y.backward(go.to(y.dtype))
        torch.cuda.synchronize()
        results.append(dict(output=y.detach(), grad_query=qi.grad, grad_input=fi.grad, grad_reference=ri.grad,
                            **{k: p.grad for k, p in mod.named_parameters()}))
    assert seen == [(BF16, F32, F32)]
    native, ref = results
    assert all(v is not None for v in native.values())
    assert float(native["grad_input"][1, 25:30].abs().max()) == 0.0   # padded rows take no gradient
    for k in native:
        assert_close("module %s" % k, native[k], ref[k], TOL[BF16])


def test_selective_backward_through_autograd():
    """``value`` needs no gradient: the backward runs with NO_GRAD_INPUT and still returns the other two; a tensor
    ``spatial_shapes`` and a host ``level_start_index`` are taken, a wrong one is refused."""
    from modulated_deform_conv_amd import MSDeformAttnFunction, ms_deform_attn
    t, shapes, want = _case("rect_levels", F32)
    value, loc, attn, go = _dev(t)
    loc.requires_grad_(True)
    attn.requires_grad_(True)
    out = MSDeformAttnFunction.apply(value, torch.tensor(shapes), torch.tensor([0, 30, 39]), loc, attn, 64)
    out.backward(go)
    assert value.grad is None
    assert_close("selective output", out.detach(), want[0], 1e-4)
    assert_close("selective grad_sampling_locations", loc.grad, want[2], 1e-4)
    assert_close("selective grad_attention_weights", attn.grad, want[3], 1e-4)
    with pytest.raises(ValueError):
        ms_deform_attn(value, shapes, loc, attn, [0, 30, 40])
    # all three through autograd
    v2, l2, a2 = (v.detach().clone().requires_grad_(True) for v in (value, loc, attn))
    ms_deform_attn(v2, shapes, l2, a2).backward(go)
    for what, a, b in zip(NAMES[1:], (v2.grad, l2.grad, a2.grad), want[1:]):
        assert_close("autograd %s" % what, a, b, 1e-4)
