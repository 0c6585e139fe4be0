"""Deformable aggregation on the GPU (include/mdconv_dagg.h): output and the three gradients against
``tests.dagg_ref.dagg_ref`` (the per-(camera, level) ``F.grid_sample`` composition times the gate) evaluated in fp64 from the
inputs as the kernel sees them (16-bit inputs rounded first), at the project's tolerances -- 1e-4 for fp32, ``TOL`` of
tests/test_gpu_hp.py for fp16 / bf16, by the value dtype for value-typed results and by the coordinate dtype for the two
coordinate gradients -- on the smallest shapes at which each part can go wrong (``tests.dagg_ref.CASES``); the gate at its
edges; non-finite locations; and the call modes: accumulate, NO_GRAD_INPUT under a guarded workspace, determinism, graph
replay, autocast, selective backward."""
import functools

import pytest
import torch

from tests import dagg_ref as R
from tests.test_gpu_hp import TOL as TOL16
from tests.util import assert_close, guarded_run

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(TOL16)
TOL[torch.float32] = 1e-4
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NAN, INF = float("nan"), float("inf")
NAMES = ("output", "grad_feature", "grad_sampling_location", "grad_weights")


@functools.lru_cache(maxsize=None)
def _case(name, dtype, coord_dtype=None):
    """CPU inputs of a case and its fp64 reference (output and the three gradients), computed once."""
    shapes = R.CASES[name]["shapes"]
    t = R.case_inputs(name, dtype, coord_dtype)
    assert R.min_lattice_distance(t[1], shapes) >= R.MARGIN
    return t, shapes, R.dagg_ref_grads(t[0], shapes, t[1], t[2], t[3])


def _native(t, shapes, grads=None, need_grad_feature=True, deterministic=False, accumulate=None):
    from modulated_deform_conv_amd import dagg
    feature, loc, weights, go = t
    out = dagg.deformable_aggregation_forward(feature, shapes, loc, weights)
    g = dagg.deformable_aggregation_backward(feature, shapes, loc, weights, go, grads=grads,
                                             need_grad_feature=need_grad_feature, deterministic=deterministic,
                                             accumulate=accumulate)
    torch.cuda.synchronize()
    return (out,) + tuple(g)


def _dev(t):
    return tuple(v.to(DEV) for v in t)


def _nans(*like):
    return tuple(torch.full_like(v, NAN) for v in like)


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
    ("one_lane", F32, None), ("cams_levels", F32, None), ("cams_levels", F16, None),
    ("g8_d32", F32, None), ("g8_d32", F16, None), ("g8_d32", BF16, None), ("g8_d32", F16, F32), ("g8_d32", BF16, F32),
    ("straddle", F32, None), ("straddle", BF16, F32), ("wide_anchor", F32, None), ("wide_anchor", F16, None),
    ("two_rounds", F32, None), ("two_rounds_16bit", F16, None), ("groups_across_rounds", F32, None), ("eight_levels", F32, None), ("many_taps", F32, None),
    ("cams_levels", BF16, F32), ("crafted", F32, None),
    ("odd_group", F32, None), ("odd_group_16bit", F16, None), ("odd_group_16bit", BF16, F32),
    ("carry_and_whole_groups", F32, None), ("group_fills_two_rounds", F32, None), ("group_per_round", F32, None),
])
def test_against_reference(name, dtype, coord_dtype):
    t, shapes, want = _case(name, dtype, coord_dtype)
    got = _native(_dev(t), shapes)
    assert got[0].dtype == got[1].dtype == dtype and got[2].dtype == got[3].dtype == (coord_dtype or dtype)
    _compare("%s %s/%s" % (name, dtype, coord_dtype), got, want, _tols(t))
    out_of_gate = ~R.gate_of(t[1])
    if bool(out_of_gate.any()):
        _exact_zero("grad_sampling_location", got[2], out_of_gate)
        _exact_zero("grad_weights", got[3], out_of_gate)


def test_crafted_lists():
    """The crafted case is what it claims: four feature rows per camera of level 0 take every sample of that level, and the
    other rows of level 0 are touched by nothing -- their grad_feature is exactly zero in overwrite mode, over NaN-filled
    buffers."""
    t, shapes, want = _case("crafted", F32)
    gf = want[1]
    assert float(gf[:, R.CRAFTED_ROWS].abs().min()) > 0 and float(gf[:, R.CRAFTED_EMPTY].abs().max()) == 0.0
    dt = _dev(t)
    got = _native(dt, shapes, grads=_nans(*dt[:3]), accumulate=False, deterministic=True)
    _exact_zero("untouched rows", got[1][:, R.CRAFTED_EMPTY])
    _compare("crafted deterministic", got, want, _tols(t))
    # accumulate mode: a row with an empty list is neither read nor written -- negative zeros there keep their sign
    bufs = tuple(torch.full_like(v, -0.0) for v in dt[:3])
    acc = _native(dt, shapes, grads=bufs)
    assert bool((acc[1][:, R.CRAFTED_EMPTY].view(torch.int32) == -2 ** 31).all())
    assert_close("accumulate onto -0.0", acc[1], want[1], 1e-4)


# ---- the gate ----
def _edge_inputs(dtype=F32):
    """cams_levels with crafted locations in image 0: exactly 0.0, exactly 1.0, one step inside both ends (pixel -0.5 and
    size - 0.5: half the weight falls outside the map), negative and above 1 -- in x with y inside, and in y with x inside."""
    feature, loc, weights, go = (v.clone() for v in R.case_inputs("cams_levels", dtype))
    one, zero = torch.tensor(1.0, dtype=loc.dtype), torch.tensor(0.0, dtype=loc.dtype)
    vals = [0.0, 1.0, torch.nextafter(zero, one).item(), torch.nextafter(one, zero).item(), -0.25, 1.5]
    inside = torch.tensor(0.43, dtype=loc.dtype).item()
    for i, v in enumerate(vals):
        loc[0, i, 0, 0] = torch.tensor([v, inside])
        loc[0, i, 1, 2] = torch.tensor([inside, v])
    gate = R.gate_of(loc)
    assert gate[0, :6, 0, 0].tolist() == gate[0, :6, 1, 2].tolist() == [False, False, True, True, False, False]
    return feature, loc, weights, go


def test_the_edges_of_the_gate():
    """0.0 and 1.0 are out, the next representable values inside are in; gated-out elements of both coordinate gradients are
    exact zeros over NaN-filled buffers, and NaN weights of gated-out triples reach no result."""
    t = _edge_inputs()
    shapes = R.CASES["cams_levels"]["shapes"]
    gate = R.gate_of(t[1])
    want = R.dagg_ref_grads(t[0], shapes, t[1], t[2], t[3])
    # what the two just-inside samples contribute is there: their weight gradients are not zero
    assert float(want[3][0, 2, 0, 0].abs().min()) > 0 and float(want[3][0, 3, 1, 2].abs().min()) > 0
    weights = t[2].clone()
    weights[~gate] = NAN
    dt = _dev((t[0], t[1], weights, t[3]))
    got = _native(dt, shapes, grads=_nans(*dt[:3]), accumulate=False, deterministic=True)
    _compare("gate edges", got, want, _tols(t))
    _exact_zero("grad_sampling_location", got[2], ~gate)
    _exact_zero("grad_weights", got[3], ~gate)
    clean = _native(_dev(t), shapes, deterministic=True)   # (sorted lists: grad_feature is bit-identical as well)
    for what, a, b in zip(NAMES, got, clean):
        assert torch.equal(a, b), "NaN weights of gated-out triples changed %s" % what


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (BF16, None), (F16, F32)])
def test_non_finite_locations(dtype, coord_dtype):
    """NaN, +-Inf and huge locations (in x, in y, in both) equal, bit for bit, the call with those locations at -3.0, in all
    four results, deterministic lists included."""
    t, shapes, _ = _case("g8_d32", dtype, coord_dtype)
    feature, loc, weights, go = t
    big = 3e38 if loc.dtype != F16 else 65504.0
    wild, tame = loc.clone(), loc.clone()
    vals = [NAN, INF, -INF, big, -big]
    for i, v in enumerate(vals):
        for k, xy in enumerate(((0,), (1,), (0, 1))):
            at = (i % 2, i, k, i % 2)
            tame[at] = -3.0
            for c in xy:
                wild[at + (c,)] = v
    assert not torch.isfinite(wild).all() and torch.isfinite(tame).all()
    assert torch.equal(R.gate_of(wild), R.gate_of(tame))
    a = _native(_dev((feature, wild, weights, go)), shapes, deterministic=True)
    b = _native(_dev((feature, tame, weights, go)), shapes, deterministic=True)
    for what, x, y in zip(NAMES, a, b):
        assert torch.isfinite(x.float()).all(), what
        assert torch.equal(x, y), what
    want = R.dagg_ref_grads(feature, shapes, tame, weights, go)
    _compare("tame", b, want, _tols(t))


def test_all_gated_out():
    """Every location outside: the output and every gradient are exact zeros over NaN-filled buffers (NaN weights included),
    the lists are empty, and accumulate mode leaves prefilled buffers unchanged bit for bit."""
    t, shapes, _ = _case("cams_levels", F32)
    gen = torch.Generator().manual_seed(5)
    loc = torch.where(torch.rand(t[1].shape, generator=gen) < 0.5, -3.0, 4.0)
    loc[0, 0] = 0.0
    loc[0, 1] = 1.0
    loc[0, 2, :, :, 0] = 0.5   # x inside, y outside
    assert not bool(R.gate_of(loc).any())
    dt = _dev((t[0], loc, torch.full_like(t[2], NAN), t[3]))
    got = _native(dt, shapes, grads=_nans(*dt[:3]), accumulate=False)
    for what, g in zip(NAMES, got):
        _exact_zero("all gated out: %s" % what, g)
    base = tuple(torch.randn(v.shape, generator=gen) for v in t[:3])
    for b in base:   # a negative zero stays one, in all three buffers: nothing is read, added to and written back
        b.view(-1)[:3] = -0.0
    assert all(bool((b.view(-1)[:3].view(torch.int32) == -2 ** 31).all()) for b in base)
    bufs = tuple(b.to(DEV) for b in base)
    got = _native(dt, shapes, grads=bufs)
    for what, a, b in zip(NAMES[1:], got[1:], base):
        assert torch.equal(a.cpu().view(torch.int32), b.view(torch.int32)), "accumulate changed %s" % what


# ---- call modes ----
def test_accumulate_against_overwrite():
    """The three gradients added to non-zero buffers, fp16 values with fp32 coordinates: each buffer + gradient in its own
    dtype, rounded once; gated-out elements are left as they were."""
    t, shapes, want = _case("g8_d32", F16, F32)
    dt = _dev(t)
    gen = torch.Generator().manual_seed(9)
    base = tuple(torch.randn(v.shape, generator=gen).to(v.dtype) for v in t[:3])
    bufs = tuple(b.to(DEV) for b in base)
    got = _native(dt, shapes, grads=bufs)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got[1:], bufs))
    assert (bufs[0].dtype, bufs[1].dtype, bufs[2].dtype) == (F16, F32, F32)
    for what, a, b, w, tol in zip(NAMES[1:], got[1:], base, want[1:], _tols(t)[1:]):
        assert_close("accumulate %s" % what, a, b.double() + w, tol)
    out_of_gate = ~R.gate_of(t[1])
    assert torch.equal(got[2].cpu()[out_of_gate], base[1][out_of_gate]) and torch.equal(got[3].cpu()[out_of_gate], base[2][out_of_gate])
    # overwrite mode ignores what the buffers hold
    over = _native(dt, shapes, grads=_nans(*dt[:3]), accumulate=False)
    _compare("overwrite", over, want, _tols(t))


def _guard(monkeypatch, touched, calls):
    """tests.util.guarded_run in the place of dagg._run; it sizes the workspace through ``mdconv_workspace_bytes`` of the
    library handle, which for this operator's descriptor is ``mdconv_dagg_workspace_bytes``."""
    from modulated_deform_conv_amd import _capi, dagg
    real = _capi.lib()

    class Lib:
        mdconv_workspace_bytes = staticmethod(real.mdconv_dagg_workspace_bytes)

        def __getattr__(self, name):
            return getattr(real, name)

    proxy = Lib()
    monkeypatch.setattr(_capi, "lib", lambda: proxy)
    monkeypatch.setattr(dagg, "_run", guarded_run(touched, calls))


@pytest.mark.parametrize("name, dtype, coord_dtype", [("g8_d32", F32, None), ("g8_d32", BF16, F32), ("cams_levels", F32, None)])
def test_no_grad_feature_under_the_guarded_workspace(monkeypatch, name, dtype, coord_dtype):
    """NO_GRAD_INPUT: grad_feature NULL, no workspace between pattern-filled margins; the coordinate gradients are bit for
    bit those of the full call.  The full and the deterministic call run guarded as well: the figure is exact."""
    t, shapes, want = _case(name, dtype, coord_dtype)
    dt = _dev(t)
    full = _native(dt, shapes)
    touched, calls = [], []
    _guard(monkeypatch, touched, calls)
    part = _native(dt, shapes, need_grad_feature=False)
    again = _native(dt, shapes)
    det = _native(dt, shapes, deterministic=True)
    assert touched == [], touched
    sizes = [b for name, b in calls if name == "mdconv_dagg_backward"]
    assert [b for name, b in calls if name == "mdconv_dagg_forward"] == [0, 0, 0]
    assert sizes[0] == 0 < sizes[1] < sizes[2], sizes
    assert part[1] is None
    for i in (0, 2, 3):
        assert torch.equal(part[i], full[i]) and torch.equal(again[i], full[i]) and torch.equal(det[i], full[i]), NAMES[i]
    _compare("guarded full", again, want, _tols(t))
    _compare("guarded deterministic", det, want, _tols(t))


@pytest.mark.parametrize("name, dtype, coord_dtype", [("crafted", F32, None), ("g8_d32", F32, None), ("g8_d32", F16, F32)])
def test_deterministic_mode(name, dtype, coord_dtype):
    """With the flag all four results are bit-identical between two eager runs and two replays of a HIP graph that holds
    forward + backward into caller buffers; without it the output and the coordinate gradients are as well and
    grad_feature is within tolerance."""
    from modulated_deform_conv_amd import dagg
    t, shapes, want = _case(name, dtype, coord_dtype)
    feature, loc, weights, go = dt = _dev(t)
    first = _native(dt, shapes, deterministic=True)
    second = _native(dt, shapes, deterministic=True)
    for what, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), "deterministic %s differs between two runs" % what
    plain = [_native(dt, shapes) for _ in range(2)]
    for i in (0, 2, 3):
        assert torch.equal(plain[0][i], plain[1][i]) and torch.equal(plain[0][i], first[i]), NAMES[i]
    assert_close("unflagged grad_feature", plain[0][1], want[1], TOL[dtype])
    _compare("deterministic", first, want, _tols(t))

    out = torch.empty_like(first[0])
    bufs = tuple(torch.empty_like(v) for v in (feature, loc, weights))

    def step():
        dagg.deformable_aggregation_forward(feature, shapes, loc, weights, output=out)
        dagg.deformable_aggregation_backward(feature, shapes, loc, weights, go, grads=bufs, deterministic=True, accumulate=False)

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
        for b in bufs:
            b.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for what, a, b in zip(NAMES, (out,) + bufs, first):
            assert torch.equal(a, b), "graph replay: %s differs from the eager deterministic run" % what


def test_autograd_and_autocast():
    """The differentiable call: all three gradients through autograd in fp32; under torch.autocast(bfloat16) the core
    receives a bf16 feature and fp32 coordinates (the mixed call) and the gradients come back in the callers' dtypes; the
    published argument order with a [cams, levels, 2] tensor and feature_maps_format's host tensors."""
    from modulated_deform_conv_amd import DeformableAggregationFunction, dagg, deformable_aggregation
    t, shapes, want = _case("cams_levels", F32)
    feature, loc, weights, go = _dev(t)
    f2, l2, w2 = (v.detach().clone().requires_grad_(True) for v in (feature, loc, weights))
    starts = torch.tensor([[c * 31 + s for s in (0, 24, 30)] for c in range(3)])
    out = DeformableAggregationFunction.apply(f2, torch.tensor([shapes] * 3), starts, l2, w2)
    out.backward(go)
    _compare("autograd", (out.detach(), f2.grad, l2.grad, w2.grad), want, _tols(t))
    seen = []
    real = dagg.deformable_aggregation_forward

    def spy(feature, shapes, loc, weights, output=None):
        seen.append((feature.dtype, loc.dtype, weights.dtype))
        return real(feature, shapes, loc, weights, output)

    dagg.deformable_aggregation_forward = spy
    try:
        f3, l3, w3 = (v.detach().clone().requires_grad_(True) for v in (feature, loc, weights))
        with torch.autocast("cuda", dtype=BF16):
            y = deformable_aggregation(f3, shapes, l3, w3)
        assert y.dtype == BF16
        y.backward(go.to(BF16))
        # the coordinate tensors run in one dtype: the feature's when both have it, fp32 otherwise -- fp16 coordinates
        # under bf16 autocast run in fp32, and their gradients come back in fp16
        f4 = feature.detach().clone()
        l4, w4 = (v.detach().to(F16).requires_grad_(True) for v in (loc, weights))
        with torch.autocast("cuda", dtype=BF16):
            y4 = deformable_aggregation(f4, shapes, l4, w4)
        y4.backward(go.to(BF16))
        assert y4.dtype == BF16 and (l4.grad.dtype, w4.grad.dtype) == (F16, F16)
        f5, l5, w5 = (v.detach().to(F16) for v in (feature, loc, weights))
        assert deformable_aggregation(f5, shapes, l5, w5).dtype == F16
        assert deformable_aggregation(f5, shapes, l5, w5.float()).dtype == F16
    finally:
        dagg.deformable_aggregation_forward = real
    assert seen[1:] == [(BF16, F32, F32), (F16, F16, F16), (F16, F32, F32)]
    seen = seen[:1]
    half = R.dagg_ref_grads(feature.to(BF16), shapes, l4.detach(), w4.detach(), go.to(BF16))
    _compare("fp16 coordinates under bf16 autocast", (y4.detach(), None, l4.grad, w4.grad), half, (TOL[BF16], TOL[BF16], TOL[F16], TOL[F16]))
    assert seen == [(BF16, F32, F32)]
    assert (f3.grad.dtype, l3.grad.dtype, w3.grad.dtype) == (F32, F32, F32)
    mixed = R.dagg_ref_grads(feature.to(BF16), shapes, loc, weights, go.to(BF16))
    _compare("autocast", (y.detach(), f3.grad, l3.grad, w3.grad), mixed, (TOL[BF16], TOL[BF16], TOL[F32], TOL[F32]))


def test_selective_backward_through_autograd():
    """``feature`` needs no gradient: the backward runs with NO_GRAD_INPUT and still returns the other two; a wrong host
    ``scale_start_index`` is refused."""
    from modulated_deform_conv_amd import dagg, deformable_aggregation
    t, shapes, want = _case("cams_levels", F32)
    feature, loc, weights, go = _dev(t)
    loc.requires_grad_(True)
    weights.requires_grad_(True)
    flags = []
    real = dagg.deformable_aggregation_backward

    def spy(*args, **kw):
        flags.append(kw["need_grad_feature"])
        return real(*args, **kw)

    dagg.deformable_aggregation_backward = spy
    try:
        out = deformable_aggregation(feature, shapes, loc, weights, [0, 24, 30])
        out.backward(go)
        assert feature.grad is None
        assert_close("selective output", out.detach(), want[0], 1e-4)
        assert_close("selective grad_sampling_location", loc.grad, want[2], 1e-4)
        assert_close("selective grad_weights", weights.grad, want[3], 1e-4)
        with pytest.raises(ValueError):
            deformable_aggregation(feature, shapes, loc, weights, [0, 24, 31])
    finally:
        dagg.deformable_aggregation_backward = real
    assert flags == [False]


def test_unaligned_views():
    """A ``feature`` view at an odd storage offset is copied to an aligned buffer (a read-only input); a caller's result
    buffer below the 16-byte class is refused, never replaced by a silent temporary."""
    from modulated_deform_conv_amd import dagg
    t, shapes, want = _case("one_lane", F32)
    feature, loc, weights, go = _dev(t)
    flat = torch.zeros(feature.numel() + 1, device=DEV)
    view = flat[1:].view_as(feature)
    view.copy_(feature)
    assert view.data_ptr() % 16 == 4
    out = dagg.deformable_aggregation_forward(view, shapes, loc, weights)
    assert_close("offset view", out, want[0], 1e-4)
    with pytest.raises(ValueError, match="16-byte aligned"):
        dagg.deformable_aggregation_forward(feature, shapes, loc, weights, output=torch.zeros(go.numel() + 1, device=DEV)[1:].view_as(go))
