"""Multi-scale deformable attention with a point count per level on the GPU (include/mdconv_msdap.h): output and the three
gradients against ``tests.msdap_ref.msdap_ref`` evaluated in fp64 from the inputs as the kernel sees them (16-bit inputs
rounded first), at the project's tolerances -- 1e-4 for fp32, ``TOL`` of tests/test_gpu_hp.py for fp16 / bf16, by the value
dtype for value-typed results and by the coordinate dtype for the two coordinate gradients -- on the smallest shapes at
which the level lookup can go wrong; bit-equality with ``ms_deform_attn`` at equal counts; the gate and the gradient
conventions; the call modes; random shapes; and the module under autocast."""
import ctypes
import functools
import random

import pytest
import torch

from tests import msda_ref as R0
from tests import msdap_ref as R
from tests.offset_views import at_offset
from tests.test_gpu_hp import TOL as TOL16
from tests.util import assert_close, guarded_run

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(TOL16)
TOL[torch.float32] = 1e-4
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PAIRINGS = ((F32, None), (F16, None), (BF16, None), (F16, F32), (BF16, F32))
NAMES = ("output", "grad_value", "grad_sampling_locations", "grad_attention_weights")

CASES = {
    # (a) level boundaries at non-multiples of anything; W against H; a 1x1 level; 4 lanes per pair, K = 6
    "rect_123": dict(N=2, M=3, D=8, shapes=[(6, 5), (3, 3), (1, 1)], points=(1, 2, 3), Lq=7),
    # (b) the D-FINE geometry: 8 lanes (fp32) / 4 lanes (16-bit) per pair, K = 12 -- a level boundary inside the first tap
    # batch (tap 3) and one inside the second (tap 9)
    "dfine": dict(N=2, M=8, D=32, shapes=[(8, 8), (4, 4), (2, 2)], points=(3, 6, 3), Lq=10),
    # (c) eight levels: the whole select chain, one lane per pair
    "eight_levels": dict(N=1, M=2, D=4, shapes=[(3, 2), (2, 3), (1, 4), (4, 1), (2, 2), (1, 1), (3, 3), (2, 5)],
                         points=(1, 3, 1, 2, 1, 1, 4, 1), Lq=6),
    # (d) one level owns more taps than a wave has lanes
    "long_level": dict(N=1, M=1, D=4, shapes=[(3, 3), (5, 4)], points=(1, 70), Lq=3),
    # (e) 16 lanes per pair, K = 3: idle state builders, the boundary among them
    "k_below_vl": dict(N=1, M=2, D=64, shapes=[(4, 4), (2, 3)], points=(2, 1), Lq=5),
    # 65 vectors per head: 64 lanes, two rounds
    "two_rounds": dict(N=1, M=1, D=260, shapes=[(3, 4), (2, 2)], points=(2, 3), Lq=4),
    "two_rounds_16bit": dict(N=1, M=1, D=520, shapes=[(3, 4), (2, 2)], points=(2, 3), Lq=4),
    "far": dict(N=1, M=2, D=4, shapes=[(8, 8), (3, 3)], points=(3, 1), Lq=6),
}


@functools.lru_cache(maxsize=None)
def _case(name, dtype, coord_dtype=None):
    """CPU inputs of a case and its fp64 reference (output and the three gradients), computed once."""
    kw = CASES[name]
    shapes, points = kw["shapes"], kw["points"]
    value, loc, attn, go = R.make_inputs(dtype=dtype, coord_dtype=coord_dtype, seed=len(name) + 7, **kw)
    if name == "far":
        gen = torch.Generator().manual_seed(5)
        loc = torch.where(torch.rand(loc.shape, generator=gen) < 0.5, -3.0, 4.0).to(loc.dtype)
    else:
        for l in range(len(shapes)):
            assert R.min_lattice_distance(loc, shapes, points, level=l) >= R.MARGIN
    return (value, loc, attn, go), shapes, points, R.msdap_ref_grads(value, shapes, points, loc, attn, go)


def _native(t, shapes, points, grads=None, need_grad_value=True, deterministic=False, accumulate=None):
    from modulated_deform_conv_amd import msdap
    value, loc, attn, go = t
    out = msdap.ms_deform_attn_points_forward(value, shapes, points, loc, attn)
    g = msdap.ms_deform_attn_points_backward(value, shapes, points, loc, attn, go, grads=grads, need_grad_value=need_grad_value,
                                             deterministic=deterministic, accumulate=accumulate)
    torch.cuda.synchronize()
    return (out,) + tuple(g)


def _dev(t):
    return tuple(v.to(DEV) for v in t)


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
    ("rect_123", F32, None), ("rect_123", F16, None),
    ("dfine", F32, None), ("dfine", F16, None), ("dfine", BF16, None), ("dfine", F16, F32), ("dfine", BF16, F32),
    ("eight_levels", F32, None), ("long_level", F32, None), ("k_below_vl", F32, None),
    ("two_rounds", F32, None), ("two_rounds_16bit", F16, None),
])
def test_against_reference(name, dtype, coord_dtype):
    t, shapes, points, want = _case(name, dtype, coord_dtype)
    got = _native(_dev(t), shapes, points)
    assert got[0].dtype == got[1].dtype == dtype and got[2].dtype == got[3].dtype == (coord_dtype or dtype)
    _compare("%s %s/%s" % (name, dtype, coord_dtype), got, want, _tols(t))


# ---- equality with the existing operator ----
@pytest.mark.parametrize("shapes, P, D", [([(8, 8), (4, 4), (2, 2), (1, 1)], 4, 32), ([(5, 7)], 5, 8)])
@pytest.mark.parametrize("dtype, coord_dtype", PAIRINGS)
def test_equal_counts_are_bit_identical_to_ms_deform_attn(shapes, P, D, dtype, coord_dtype):
    """With equal counts nothing but the level lookup differs from ``MsdaOp``: the output and the two coordinate gradients
    are bit-identical to ``ms_deform_attn_forward`` / ``_backward`` on the reshaped tensors, and so is grad_value under
    ``deterministic=True``."""
    from modulated_deform_conv_amd import msda
    L = len(shapes)
    N, M, Lq = 2, 8 if L > 1 else 3, 10
    value, loc, attn, go = dt = _dev(R.make_inputs(N=N, M=M, D=D, shapes=shapes, points=(P,) * L, Lq=Lq, dtype=dtype,
                                                   coord_dtype=coord_dtype, seed=31))
    got = _native(dt, shapes, (P,) * L, deterministic=True)
    loc6, attn5 = loc.view(N, Lq, M, L, P, 2), attn.view(N, Lq, M, L, P)
    out = msda.ms_deform_attn_forward(value, shapes, loc6, attn5)
    gv, gl, ga = msda.ms_deform_attn_backward(value, shapes, loc6, attn5, go, deterministic=True)
    torch.cuda.synchronize()
    assert float(got[0].float().abs().max()) > 0 and float(got[2].float().abs().max()) > 0
    for what, a, b in zip(NAMES, got, (out, gv, gl, ga)):
        assert torch.equal(a, b.view(a.shape)), "%s differs from ms_deform_attn (%d elements)" % (what, int((a != b.view(a.shape)).sum()))


# ---- the gate and the gradient conventions ----
def test_samples_wholly_outside():
    """Locations of -3 / +4: nothing is read, the output and every gradient are exactly zero, the lists are empty."""
    t, shapes, points, want = _case("far", F32)
    assert all(float(w.abs().max()) == 0.0 for w in want)
    got = _native(_dev(t), shapes, points)
    assert all(float(g.abs().max()) == 0.0 for g in got)


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (F16, None), (BF16, F32)])
def test_integer_positions_keep_the_pinned_convention(dtype, coord_dtype):
    """Every pixel coordinate an integer, both edges of the gate included, per level: the right-sided derivative of the cell
    floor(x), floor(y) and exact zeros outside the gate -- ``msdap_direct`` states it; ``F.grid_sample`` is no reference here."""
    shapes, points = [(8, 4), (2, 2), (1, 4)], (2, 1, 3)
    t = R.make_lattice_inputs(1, 2, 8, shapes, points, dtype=dtype, coord_dtype=coord_dtype, seed=2)
    want = R.msdap_ref_grads(*t[:1], shapes, points, *t[1:], fn=R.msdap_direct)
    got = _native(_dev(t), shapes, points, deterministic=True)
    _compare("lattice %s/%s" % (dtype, coord_dtype), got, want, _tols(t))
    gate = R.gate_of(t[1], shapes, points)
    assert not bool(gate.all())
    assert float(got[2].cpu()[~gate].float().abs().max()) == 0.0 and float(got[3].cpu()[~gate].float().abs().max()) == 0.0


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (F16, None), (BF16, F32)])
def test_nonfinite_coordinates_are_gated_out(dtype, coord_dtype):
    """NaN / +-Inf coordinates in a few taps of different levels contribute nothing: every result equals, bit for bit, the
    call with those coordinates far outside (-3), their own gradients are exact zeros over NaN-filled buffers, and nothing
    is non-finite."""
    t, shapes, points, _ = _case("dfine", dtype, coord_dtype)
    value, loc, attn, go = t
    inf, nan = float("inf"), float("nan")
    spots = [((0, 1, 2, 1, 0), nan), ((1, 3, 5, 4, 1), inf), ((0, 7, 0, 10, 0), -inf), ((0, 7, 0, 10, 1), -inf),
             ((1, 9, 7, 8, 0), nan), ((1, 9, 7, 9, 1), inf), ((0, 0, 0, 0, 0), -inf), ((1, 9, 7, 11, 1), nan)]
    assert {R.tap_levels(points)[s[3]] for s, _ in spots} == {0, 1, 2}
    bad, far = loc.clone(), loc.clone()
    for s, v in spots:
        bad[s] = v
        far[s] = -3.0

    def run(l):
        dt = _dev((value, l, attn, go))
        bufs = tuple(torch.full_like(v, nan) for v in dt[:3])
        return _native(dt, shapes, points, grads=bufs, deterministic=True, accumulate=False)

    base, got = run(far), run(bad)
    _compare("replaced", base, R.msdap_ref_grads(value, shapes, points, far, attn, go), _tols(t))
    for what, a, b in zip(NAMES, got, base):
        assert bool(torch.isfinite(a.float()).all()), what
        assert torch.equal(a, b), "%s differs from the run with the coordinates far outside (%d elements)" % (what, int((a != b).sum()))
    for s, _ in spots:
        assert float(got[2][s[:4]].float().abs().max()) == 0.0 and float(got[3][s[:4]]) == 0.0, s


# ---- call modes, on the D-FINE case ----
def test_accumulate_against_overwrite():
    """The three gradients added to non-zero buffers, fp16 values with fp32 coordinates: each buffer + gradient in its own
    dtype, rounded once; overwrite mode ignores what the buffers hold."""
    t, shapes, points, want = _case("dfine", F16, F32)
    dt = _dev(t)
    gen = torch.Generator().manual_seed(9)
    base = tuple(torch.randn(v.shape, generator=gen).to(v.dtype) for v in t[:3])
    bufs = tuple(b.to(DEV) for b in base)
    got = _native(dt, shapes, points, grads=bufs)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got[1:], bufs))
    for what, a, b, w, tol in zip(NAMES[1:], got[1:], base, want[1:], _tols(t)[1:]):
        assert_close("accumulate %s" % what, a, b.double() + w, tol)
    over = _native(dt, shapes, points, grads=tuple(b.to(DEV) for b in base), accumulate=False)
    fresh = _native(dt, shapes, points)
    _compare("overwrite", over, want, _tols(t))
    for i in (0, 2, 3):
        assert torch.equal(over[i], fresh[i]), NAMES[i]


def _guard(monkeypatch, touched, calls):
    """tests.util.guarded_run in the place of msdap._run; it sizes the workspace through ``mdconv_workspace_bytes`` of the
    library handle, which for this operator's descriptor is ``mdconv_msdap_workspace_bytes``."""
    from modulated_deform_conv_amd import _capi, msdap
    real = _capi.lib()

    class Lib:
        mdconv_workspace_bytes = staticmethod(real.mdconv_msdap_workspace_bytes)

        def __getattr__(self, name):
            return getattr(real, name)

    proxy = Lib()
    monkeypatch.setattr(_capi, "lib", lambda: proxy)
    monkeypatch.setattr(msdap, "_run", guarded_run(touched, calls))


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (BF16, F32)])
def test_no_grad_value_under_the_guarded_workspace(monkeypatch, dtype, coord_dtype):
    """NO_GRAD_INPUT: grad_value NULL, no workspace between pattern-filled margins; the coordinate gradients are bit for
    bit those of the full call.  The full and the deterministic call run guarded as well: the figure is exact."""
    t, shapes, points, want = _case("dfine", dtype, coord_dtype)
    dt = _dev(t)
    full = _native(dt, shapes, points)
    touched, calls = [], []
    _guard(monkeypatch, touched, calls)
    part = _native(dt, shapes, points, need_grad_value=False)
    again = _native(dt, shapes, points)
    det = _native(dt, shapes, points, deterministic=True)
    assert touched == [], touched
    sizes = [b for name, b in calls if name == "mdconv_msdap_backward"]
    assert [b for name, b in calls if name == "mdconv_msdap_forward"] == [0, 0, 0]
    assert sizes[0] == 0 < sizes[1] <= sizes[2], sizes
    assert part[1] is None
    for i in (0, 2, 3):
        assert torch.equal(part[i], full[i]) and torch.equal(again[i], full[i]) and torch.equal(det[i], full[i]), NAMES[i]
    _compare("guarded full", again, want, _tols(t))
    _compare("guarded deterministic", det, want, _tols(t))


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (F16, F32)])
def test_deterministic_mode_and_graph_replay(dtype, coord_dtype):
    """With the flag all four results are bit-identical between two eager runs and two replays of a HIP graph that holds
    forward + backward into caller buffers; without it the output and the coordinate gradients are as well and
    grad_value is within tolerance."""
    from modulated_deform_conv_amd import msdap
    t, shapes, points, want = _case("dfine", dtype, coord_dtype)
    value, loc, attn, go = dt = _dev(t)
    first = _native(dt, shapes, points, deterministic=True)
    second = _native(dt, shapes, points, deterministic=True)
    for what, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), "deterministic %s differs between two runs" % what
    plain = _native(dt, shapes, points)
    for i in (0, 2, 3):
        assert torch.equal(plain[i], first[i]), NAMES[i]
    assert_close("unflagged grad_value", plain[1], want[1], TOL[dtype])
    _compare("deterministic", first, want, _tols(t))

    out = torch.empty_like(first[0])
    bufs = tuple(torch.empty_like(v) for v in (value, loc, attn))

    def step():
        msdap.ms_deform_attn_points_forward(value, shapes, points, loc, attn, output=out)
        for b in bufs:   # caller-allocated buffers are added to
            b.zero_()
        msdap.ms_deform_attn_points_backward(value, shapes, points, loc, attn, go, grads=bufs, deterministic=True)

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


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (F16, None), (BF16, F32)])
def test_element_arguments_at_offsets(dtype, coord_dtype, k):
    """The "element" arguments -- sampling_locations, attention_weights and their gradients -- as views ``k`` elements past
    a 16-byte boundary, between guard margins: every result is bit for bit that of the call on freshly allocated tensors,
    and no margin changes."""
    t, shapes, points, _ = _case("dfine", dtype, coord_dtype)
    value, loc, attn, go = dt = _dev(t)
    want = _native(dt, shapes, points, deterministic=True)
    es = loc.element_size()
    views, checks = zip(*(at_offset(v, k, mod16=(k * es) % 16) for v in (loc, attn, torch.zeros_like(loc), torch.zeros_like(attn))))
    # (4 fp32 elements are 16 bytes: that view is on a 16-byte boundary again, one vector past the buffer's)
    assert all(v.data_ptr() % 16 == (k * es) % 16 for v in views) and ((k * es) % 16 != 0 or (es, k) == (4, 4))
    gv = torch.zeros_like(value)
    got = _native((value, views[0], views[1], go), shapes, points, grads=(gv, views[2], views[3]), deterministic=True,
                  accumulate=False)
    assert got[2].data_ptr() == views[2].data_ptr() and got[3].data_ptr() == views[3].data_ptr()
    for what, a, b in zip(NAMES, got, want):
        assert torch.equal(a, b), "%s at offset %d differs (%d elements)" % (what, k, int((a != b).sum()))
    for name, check in zip(("sampling_locations", "attention_weights", "grad_sampling_locations", "grad_attention_weights"), checks):
        check("%s at offset %d" % (name, k))


# ---- random shapes ----
def _random_case(seed):
    """A shape inside the shape rule by construction: D a multiple of 4 (fp32) or 8 (16-bit), K <= 72, tiny tensors.  The
    pairing and the level count walk their ranges with the seed (16 seeds: every L twice, the fp32 seeds 0, 5, 10, 15 every
    D once); counts, extents, N, M and Lq are drawn."""
    rng = random.Random(1000 + seed)
    dtype, coord_dtype = PAIRINGS[seed % len(PAIRINGS)]
    L = seed % 8 + 1
    kw = dict(N=rng.randint(1, 2), M=rng.randint(1, 4), D=(4, 8, 12, 32)[seed // 5 % 4] if dtype == F32 else rng.choice((8, 32)),
              shapes=[(rng.randint(1, 6), rng.randint(1, 6)) for _ in range(L)],
              points=tuple(rng.randint(1, 9) for _ in range(L)), Lq=rng.randint(1, 9))
    return kw, dtype, coord_dtype


def test_random_generator_covers_the_space():
    drawn = [_random_case(s) for s in range(16)]
    assert {len(kw["shapes"]) for kw, _, _ in drawn} == set(range(1, 9)) and {kw["D"] for kw, _, _ in drawn} == {4, 8, 12, 32}
    assert {(d, c) for _, d, c in drawn} == set(PAIRINGS)
    assert any(len(set(kw["points"])) > 2 for kw, _, _ in drawn)
    for kw, dtype, _ in drawn:
        assert kw["D"] % (4 if dtype == F32 else 8) == 0 and 1 <= sum(kw["points"]) <= 72


@pytest.mark.parametrize("seed", range(16))
def test_random_shapes(seed):
    kw, dtype, coord_dtype = _random_case(seed)
    t = R.make_inputs(dtype=dtype, coord_dtype=coord_dtype, seed=seed, **kw)
    want = R.msdap_ref_grads(t[0], kw["shapes"], kw["points"], t[1], t[2], t[3])
    got = _native(_dev(t), kw["shapes"], kw["points"], deterministic=bool(seed & 1))
    _compare("random %d %s" % (seed, kw), got, want, _tols(t))


# ---- the module and autograd ----
@pytest.mark.parametrize("ref_levels", [1, 3])
def test_module_step_under_autocast(ref_levels):
    """``MSDeformableAttention([3, 6, 3])`` under torch.autocast(bfloat16), with a value mask, against the same module with
    the core swapped for the reference composition: the Python surface and the autograd wiring (output, input gradients and
    every parameter gradient).  The core receives a bf16 value and fp32 coordinates: the mixed call."""
    from modulated_deform_conv_amd import MSDeformableAttention, ms_deform_attn_points
    torch.manual_seed(21 + ref_levels)
    shapes = [(6, 5), (3, 3), (2, 2)]
    S, N, Lq, C = 43, 2, 7, 32
    mod = MSDeformableAttention(embed_dim=C, num_heads=4, num_levels=3, num_points=[3, 6, 3]).to(DEV)
    with torch.no_grad():   # offsets and weights that depend on the query
        mod.sampling_offsets.weight.normal_(0, 0.05)
        mod.attention_weights.weight.normal_(0, 0.2)
    query = torch.randn(N, Lq, C, device=DEV)
    flat = torch.randn(N, S, C, device=DEV)
    boxes = torch.cat([torch.rand(N, Lq, ref_levels, 2, device=DEV) * 0.6 + 0.2, torch.rand(N, Lq, ref_levels, 2, device=DEV) * 0.3 + 0.1], -1)
    keep = torch.ones(N, S, dtype=torch.bool, device=DEV)
    keep[1, 25:30] = False
    go = torch.randn(N, Lq, C, device=DEV)
    seen = []

    def native_core(value, spatial_shapes, num_points_list, loc, attn):
        seen.append((value.dtype, loc.dtype, attn.dtype, tuple(loc.shape)))
        return ms_deform_attn_points(value, spatial_shapes, num_points_list, loc, attn)

    results = []
    for core in (native_core, R.msdap_ref):
        mod._core = core
        mod.zero_grad(set_to_none=True)
        qi, fi, ri = (v.clone().requires_grad_(True) for v in (query, flat, boxes))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = mod(qi, ri, fi, shapes, keep)
        assert y.dtype == torch.bfloat16
        y.backward(go.to(y.dtype))
        torch.cuda.synchronize()
        results.append(dict(output=y.detach(), grad_query=qi.grad, grad_input=fi.grad, grad_reference=ri.grad,
                            **{k: p.grad for k, p in mod.named_parameters()}))
    assert seen == [(BF16, F32, F32, (N, Lq, 4, 12, 2))]
    native, ref = results
    assert all(v is not None for v in native.values())
    assert float(native["grad_input"][1, 25:30].abs().max()) == 0.0   # masked rows take no gradient
    for k in native:
        assert_close("module %s" % k, native[k], ref[k], TOL[BF16])


def test_selective_backward_through_autograd(monkeypatch):
    """``value`` needs no gradient: the backward runs with NO_GRAD_INPUT -- no lists, no workspace -- returns None for
    grad_value and still returns the other two; tensor ``spatial_shapes`` and ``num_points_list`` are taken."""
    from modulated_deform_conv_amd import MSDeformAttnPointsFunction, _capi, ms_deform_attn_points, msdap
    t, shapes, points, want = _case("rect_123", F32)
    value, loc, attn, go = _dev(t)
    real, calls = msdap._run, []

    def spy(fn_name, d, backward, args, like):
        ws = _capi.lib().mdconv_msdap_workspace_bytes(ctypes.byref(d), int(backward))
        calls.append((fn_name, int(d.flags), int(ws), args[4].value if backward else None))
        return real(fn_name, d, backward, args, like)

    monkeypatch.setattr(msdap, "_run", spy)
    loc.requires_grad_(True)
    attn.requires_grad_(True)
    out = MSDeformAttnPointsFunction.apply(value, torch.tensor(shapes), torch.tensor(points), loc, attn)
    out.backward(go)
    assert value.grad is None
    assert [c[0] for c in calls] == ["mdconv_msdap_forward", "mdconv_msdap_backward"]
    assert calls[1][1] & _capi.FLAG_NO_GRAD_INPUT and calls[1][2] == 0 and not calls[1][3]   # no lists; grad_value NULL
    assert_close("selective output", out.detach(), want[0], 1e-4)
    assert_close("selective grad_sampling_locations", loc.grad, want[2], 1e-4)
    assert_close("selective grad_attention_weights", attn.grad, want[3], 1e-4)
    # all three through autograd
    del calls[:]
    v2, l2, a2 = (v.detach().clone().requires_grad_(True) for v in (value, loc, attn))
    ms_deform_attn_points(v2, shapes, points, l2, a2).backward(go)
    assert not calls[1][1] & _capi.FLAG_NO_GRAD_INPUT and calls[1][2] > 0 and calls[1][3]
    for what, a, b in zip(NAMES[1:], (v2.grad, l2.grad, a2.grad), want[1:]):
        assert_close("autograd %s" % what, a, b, 1e-4)
