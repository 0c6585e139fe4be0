"""Anchored packed deformable attention on the GPU (include/mdconv_afda.h): output and the three gradients against
``tests.afda_ref`` -- the published location formulas in fp64 torch operators, the fp64 softmax, the fp64 reference of
deformable attention with a point count per level -- at the project's tolerances: 1e-4 for fp32 results, ``TOL`` of
tests/test_gpu_hp.py for 16-bit ones, by the value dtype for value-typed results and by the coordinate dtype for the packed
gradient; grad_reference is an fp32 result in every pairing and holds 1e-4.  The geometries are ``CASES`` of
tests/test_gpu_msdap.py.  Beyond parity: bit-identity with ``flash_deform_attn_points`` where the location is the stored
offset, the lattice, non-finite offsets and references, grad_reference off, repeatability and graph replay, the write modes,
"element" arguments at offsets, random shapes, the module under autocast and the selective backward."""
import ctypes
import functools
import random

import pytest
import torch

from tests import afda_ref as R
from tests import fdap_ref as FR
from tests import msdap_ref as MR
from tests.offset_views import at_offset
from tests.test_gpu_hp import TOL as TOL16
from tests.test_gpu_msdap import CASES as MSDAP_CASES
from tests.util import assert_close, guarded_run

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(TOL16)
TOL[torch.float32] = 1e-4
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PAIRINGS = ((F32, None), (F16, None), (BF16, None), (F16, F32), (BF16, F32))
NAMES = ("output", "grad_value", "grad_reference", "grad_offs_attn")

CASES = {k: v for k, v in MSDAP_CASES.items() if k != "far"}
CASES["one_tap"] = dict(N=1, M=2, D=4, shapes=[(4, 5)], points=(1,), Lq=6)

# (case, (Lr, R), value dtype, coordinate dtype); Lr: 1, or "L" for one row per level
PARITY = (
    [("rect_123", form, F32, None) for form in ((1, 4), ("L", 4), (1, 2), ("L", 2))]
    + [("dfine", (1, 4), dt, cdt) for dt, cdt in PAIRINGS]
    + [("dfine", form, dt, cdt) for form in (("L", 4), ("L", 2)) for dt, cdt in ((F32, None), (BF16, F32))]
    + [("eight_levels", ("L", 4), F32, None), ("eight_levels", ("L", 2), F32, None), ("long_level", (1, 4), F32, None),
       ("k_below_vl", (1, 4), F32, None), ("k_below_vl", ("L", 4), F32, None), ("two_rounds", ("L", 4), F32, None),
       ("two_rounds_16bit", (1, 4), F16, None), ("one_tap", (1, 4), F32, None), ("one_tap", (1, 2), F32, None)])


@functools.lru_cache(maxsize=None)
def _case(name, form=(1, 4), dtype=F32, coord_dtype=None, offset_scale=0.5):
    """CPU inputs of a case and its fp64 reference (output and the three gradients), computed once and left unchanged."""
    kw = CASES[name]
    shapes, points = kw["shapes"], kw["points"]
    t = R.make_inputs(Lr=form[0], R=form[1], dtype=dtype, coord_dtype=coord_dtype, seed=len(name) + 7,
                      offset_scale=offset_scale, **kw)
    return t, shapes, points, R.afda_ref_grads(t[0], shapes, points, t[1], t[2], t[3], offset_scale)


def _dev(t):
    return tuple(v.to(DEV) for v in t)


def _native(t, shapes, points, offset_scale=0.5, grads=None, need_grad_value=True, need_grad_reference=True, deterministic=False,
            accumulate=None):
    from modulated_deform_conv_amd import afda
    value, ref, offs_attn, go = t
    out = afda.anchored_deform_attn_forward(value, shapes, points, ref, offs_attn, offset_scale)
    g = afda.anchored_deform_attn_backward(value, shapes, points, ref, offs_attn, go, offset_scale, grads=grads,
                                           need_grad_value=need_grad_value, need_grad_reference=need_grad_reference,
                                           deterministic=deterministic, accumulate=accumulate)
    torch.cuda.synchronize()
    return (out,) + tuple(g)


def _tols(t):
    """Per result: value-typed results by the value dtype, grad_reference fp32, the packed gradient by the coordinate dtype."""
    return (TOL[t[0].dtype], TOL[t[0].dtype], 1e-4, TOL[t[2].dtype])


def _compare(tag, got, want, tols):
    for what, a, b, tol in zip(NAMES, got, want, tols):
        if a is None:
            continue
        print("%s %s: max |want| %.3e" % (tag, what, float(b.abs().max())))
    for what, a, b, tol in zip(NAMES, got, want, tols):
        if a is not None:
            assert_close("%s %s" % (tag, what), a, b, tol)


# ---- parity ----
@pytest.mark.parametrize("name, form, dtype, coord_dtype", PARITY)
def test_against_reference(name, form, dtype, coord_dtype):
    """rect_123: all four forms, M = 3 heads (no power of two) in the head sum of grad_reference.  dfine: level boundaries
    inside two tap batches, all five pairings.  eight_levels: the whole select chain for the reference row and for s_k.
    long_level: K = 71, the reference sum crosses tap batches.  k_below_vl: idle lanes enter no sum.  two_rounds: heads of
    more than 64 vectors.  one_tap: the weight is 1."""
    t, shapes, points, want = _case(name, form, dtype, coord_dtype)
    got = _native(_dev(t), shapes, points)
    assert got[0].dtype == got[1].dtype == dtype and got[2].dtype == F32 and got[3].dtype == (coord_dtype or dtype)
    assert got[2].shape == t[1].shape == (t[0].shape[0], t[2].shape[1], 1 if form[0] == 1 else len(shapes), form[1])
    assert float(want[2].abs().max()) > 0
    _compare("%s %s %s/%s" % (name, form, dtype, coord_dtype), got, want, _tols(t))


def test_offset_scale_reaches_the_kernels():
    t, shapes, points, want = _case("dfine", ("L", 4), F32, None, 1.25)
    got = _native(_dev(t), shapes, points, 1.25)
    _compare("offset_scale 1.25", got, want, _tols(t))
    other = _native(_dev(t), shapes, points, 0.5)
    assert not torch.equal(other[0], got[0])


# ---- bit-identity with the existing operator ----
@pytest.mark.parametrize("Lr", [1, 3])
@pytest.mark.parametrize("points, offset_scale", [((4, 4, 4), 4.0), ((1, 1, 1), 1.0)])
@pytest.mark.parametrize("dtype, coord_dtype", PAIRINGS)
def test_unit_boxes_are_bit_identical_to_flash_deform_attn_points(Lr, points, offset_scale, dtype, coord_dtype):
    """References (0, 0, 1, 1) and s_k * offset_scale = 1, every factor a power of two: the location IS the stored offset, and
    the output, the packed gradient and grad_value under ``deterministic=True`` are those of
    ``flash_deform_attn_points_forward`` / ``_backward`` on the same packed memory, bit for bit."""
    from modulated_deform_conv_amd import fdap
    shapes = [(8, 8), (4, 4), (2, 2)]
    N, M, D, Lq = 2, 8, 32, 10
    value, loc_attn, go = _dev(FR.make_inputs(N=N, M=M, D=D, shapes=shapes, points=points, Lq=Lq, dtype=dtype,
                                              coord_dtype=coord_dtype, seed=31))
    ref = torch.tensor([0.0, 0.0, 1.0, 1.0], device=DEV).expand(N, Lq, Lr, 4).contiguous()
    got = _native((value, ref, loc_attn, go), shapes, points, offset_scale, deterministic=True)
    out = fdap.flash_deform_attn_points_forward(value, shapes, points, loc_attn)
    gv, gla = fdap.flash_deform_attn_points_backward(value, shapes, points, loc_attn, go, deterministic=True)
    torch.cuda.synchronize()
    assert all(float(g.float().abs().max()) > 0 for g in got)
    for what, a, b in zip(("output", "grad_value", "grad_offs_attn"), (got[0], got[1], got[3]), (out, gv, gla)):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a, b), "%s differs from flash_deform_attn_points (%d elements)" % (what, int((a != b).sum()))


# ---- the lattice ----
@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (F16, None), (BF16, F32)])
def test_integer_positions_keep_the_pinned_convention(dtype, coord_dtype):
    """Two-component references ``(c + 0.5) / extent`` and integer offsets: every pixel coordinate an exact integer, both edges
    of the gate included, per level.  The right-sided derivative of the cell floor(x), floor(y) and exact zeros for the
    offset gradients outside the gate -- ``msdap_direct`` behind the fp64 softmax states it."""
    shapes, points = [(8, 4), (2, 2), (1, 4)], (2, 1, 3)
    t = R.make_lattice_inputs(1, 2, 8, shapes, points, dtype=dtype, coord_dtype=coord_dtype, seed=2)
    want = R.afda_ref_grads(t[0], shapes, points, t[1], t[2], t[3], fn=MR.msdap_direct)
    got = _native(_dev(t), shapes, points, deterministic=True)
    _compare("lattice %s/%s" % (dtype, coord_dtype), got, want, _tols(t))
    gate = MR.gate_of(R.derived(t[1], shapes, points, t[2]), shapes, points)
    assert not bool(gate.all())
    goffs, glogit = FR.unpack(got[3].cpu(), points)
    assert float(goffs[~gate].float().abs().max()) == 0.0
    assert float(FR.unpack(want[3], points)[1][~gate].abs().max()) > 0 and float(glogit[~gate].float().abs().max()) > 0


# ---- non-finite offsets and references ----
@pytest.mark.parametrize("form", [(1, 4), ("L", 4), ("L", 2)])
@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (BF16, F32), (F16, None)])
def test_nonfinite_offsets_and_reference_rows_are_gated_out(form, dtype, coord_dtype):
    """NaN / +-Inf in a few offsets of all three levels and in one whole reference row contribute nothing: every result
    equals, bit for bit, the call with those taps far outside (offsets that put them there; the row's taps through their
    offsets, the row itself finite), their own offset gradients and that row's gradient are exact zeros over NaN-filled
    buffers, and nothing is non-finite.  (No non-finite logits: their result is unspecified.)"""
    t, shapes, points, _ = _case("dfine", form, dtype, coord_dtype)
    value, ref, oa, go = t
    K = sum(points)
    inf, nan = float("inf"), float("nan")
    spots = [((0, 1, 2, 1, 0), nan), ((1, 3, 5, 4, 1), inf), ((0, 7, 0, 10, 0), -inf), ((0, 7, 0, 10, 1), -inf),
             ((1, 9, 7, 8, 0), nan), ((1, 9, 7, 9, 1), inf), ((0, 0, 0, 0, 0), -inf), ((1, 9, 7, 11, 1), nan)]
    assert {MR.tap_levels(points)[s[3]] for s, _ in spots} == {0, 1, 2}
    row = (1, 4, ref.shape[2] - 1)   # (image, query, reference row): the last row of that query
    row_taps = [k for k, l in enumerate(MR.tap_levels(points)) if ref.shape[2] == 1 or l == row[2]]
    far_off = 4000.0   # times the smallest scale of this case (0.1 * 0.5 / 6, or 1 / 8) it is far beyond any level
    bad, far, bad_ref = oa.clone(), oa.clone(), ref.clone()
    for (n, q, m, tap, xy), v in spots:
        bad[n, q, m, 2 * tap + xy] = v
        far[n, q, m, 2 * tap + xy] = -far_off
    bad_ref[row] = torch.tensor([nan, 0.5, inf, 0.2][:ref.shape[3]])
    for tap in row_taps:
        far[row[0], row[1], :, 2 * tap] = far_off
    assert bool(torch.isfinite(bad[..., 2 * K:]).all())
    gate_far = MR.gate_of(R.derived(ref, shapes, points, far), shapes, points)
    assert not bool(gate_far[row[0], row[1]][:, row_taps].any()) and all(not bool(gate_far[n, q, m, tap]) for (n, q, m, tap, _), _ in spots)

    def run(r, o):
        dt = _dev((value, r, o, go))
        bufs = (torch.full_like(dt[0], nan), torch.full_like(dt[1], nan), torch.full_like(dt[2], nan))
        return _native(dt, shapes, points, grads=bufs, deterministic=True, accumulate=False)

    base, got = run(ref, far), run(bad_ref, bad)
    _compare("replaced", base, R.afda_ref_grads(value, shapes, points, ref, far, go), _tols(t))
    assert float(base[2][row].abs().max()) == 0.0
    for what, a, b in zip(NAMES, got, base):
        assert bool(torch.isfinite(a.float()).all()), what
        assert torch.equal(a, b), "%s differs from the run with the taps far outside (%d elements)" % (what, int((a != b).sum()))
    for (n, q, m, tap, _), _ in spots:
        assert float(got[3][n, q, m, 2 * tap:2 * tap + 2].float().abs().max()) == 0.0, (n, q, m, tap)
    for tap in row_taps:
        assert float(got[3][row[0], row[1], :, 2 * tap:2 * tap + 2].float().abs().max()) == 0.0, tap
    assert float(got[2][row].abs().max()) == 0.0


# ---- grad_reference off, the workspace ----
def _guard(monkeypatch, touched, calls):
    """tests.util.guarded_run in the place of afda._run; it sizes the workspace through ``mdconv_workspace_bytes`` of the
    library handle, which for this operator's descriptor is ``mdconv_afda_workspace_bytes``."""
    from modulated_deform_conv_amd import _capi, afda
    real = _capi.lib()

    class Lib:
        mdconv_workspace_bytes = staticmethod(real.mdconv_afda_workspace_bytes)

        def __getattr__(self, name):
            return getattr(real, name)

    proxy = Lib()
    monkeypatch.setattr(_capi, "lib", lambda: proxy)
    monkeypatch.setattr(afda, "_run", guarded_run(touched, calls))


def _fdap_bytes(t, shapes, points, flags):
    from modulated_deform_conv_amd import _capi, fdap
    d = fdap._desc(t[0], t[2], shapes, points, flags=flags)
    return _capi.lib().mdconv_fdap_workspace_bytes(ctypes.byref(d), 1)


@pytest.mark.parametrize("form", [(1, 4), ("L", 2)])
@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (BF16, F32)])
def test_no_grad_reference_under_the_guarded_workspace(monkeypatch, form, dtype, coord_dtype):
    """grad_reference == 0: the pointer NULL, the other results bit for bit those of the full call, the workspace figure that
    of mdconv_fdap_workspace_bytes -- between pattern-filled margins, as are the full and the deterministic call and the call
    with neither grad_value nor lists; every figure is exact."""
    from modulated_deform_conv_amd import _capi
    t, shapes, points, want = _case("dfine", form, dtype, coord_dtype)
    dt = _dev(t)
    full = _native(dt, shapes, points)
    fdap_plain, fdap_det = _fdap_bytes(dt, shapes, points, 0), _fdap_bytes(dt, shapes, points, _capi.FLAG_DETERMINISTIC)
    touched, calls = [], []
    _guard(monkeypatch, touched, calls)
    part = _native(dt, shapes, points, need_grad_reference=False)
    again = _native(dt, shapes, points)
    det = _native(dt, shapes, points, deterministic=True)
    det_part = _native(dt, shapes, points, deterministic=True, need_grad_reference=False)
    only_ref = _native(dt, shapes, points, need_grad_value=False)
    neither = _native(dt, shapes, points, need_grad_value=False, need_grad_reference=False)
    assert touched == [], touched
    sizes = [b for name, b in calls if name == "mdconv_afda_backward"]
    assert [b for name, b in calls if name == "mdconv_afda_forward"] == [0] * 6
    rows = (dt[1].numel() * dt[0].shape[2] * 4 + 255) // 256 * 256   # 4 * Lr * R bytes per (query, head)
    assert sizes == [fdap_plain, fdap_plain + rows, fdap_det + rows, fdap_det, rows, 0], (sizes, fdap_plain, fdap_det, rows)
    assert part[2] is None and det_part[2] is None and only_ref[1] is None and neither[1] is None and neither[2] is None
    for i in (0, 3):
        for other in (part, again, det, det_part, only_ref, neither):
            assert torch.equal(other[i], full[i]), NAMES[i]
    for other in (again, det, only_ref):
        assert torch.equal(other[2], full[2])
    assert torch.equal(det_part[1], det[1])
    _compare("guarded full", again, want, _tols(t))
    _compare("guarded deterministic", det, want, _tols(t))
    _compare("guarded without grad_reference", part, want, _tols(t))


# ---- repeatability ----
@pytest.mark.parametrize("form", [(1, 4), ("L", 4)])
@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (F16, F32)])
def test_repeatability_and_graph_replay(form, dtype, coord_dtype):
    """Output, packed gradient and grad_reference are bit-identical between two plain runs; with the flag all four results
    are, between two eager runs and two replays of a HIP graph that holds forward + backward into NaN-filled caller buffers."""
    from modulated_deform_conv_amd import afda
    t, shapes, points, want = _case("dfine", form, dtype, coord_dtype)
    value, ref, oa, go = dt = _dev(t)
    first = _native(dt, shapes, points, deterministic=True)
    second = _native(dt, shapes, points, deterministic=True)
    for what, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), "deterministic %s differs between two runs" % what
    plain = [_native(dt, shapes, points) for _ in range(2)]
    for i in (0, 2, 3):
        assert torch.equal(plain[0][i], plain[1][i]) and torch.equal(plain[0][i], first[i]), NAMES[i]
    assert_close("unflagged grad_value", plain[0][1], want[1], TOL[dtype])
    _compare("deterministic", first, want, _tols(t))

    out = torch.empty_like(first[0])
    bufs = (torch.empty_like(value), torch.empty_like(ref), torch.empty_like(oa))

    def step():
        afda.anchored_deform_attn_forward(value, shapes, points, ref, oa, output=out)
        afda.anchored_deform_attn_backward(value, shapes, points, ref, oa, go, grads=bufs, deterministic=True, accumulate=False)

    # (warm-up on the current stream: the step holds no autograd, and a stream taken from torch's pool here would move the
    # pool's round-robin for every test file that runs after this one)
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(2):
        for b in (out,) + bufs:
            b.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for what, a, b in zip(NAMES, (out,) + bufs, first):
            assert torch.equal(a, b), "graph replay: %s differs from the eager deterministic run" % what


# ---- the write modes ----
@pytest.mark.parametrize("form", [(1, 4), ("L", 4)])
def test_accumulate_against_overwrite(form):
    """fp16 values with an fp32 packed tensor.  Accumulate: each of the three buffers + its gradient in its own dtype, rounded
    once.  Overwrite into NaN-filled buffers: the gradient alone, bit for bit that of a call into fresh tensors."""
    t, shapes, points, want = _case("dfine", form, F16, F32)
    dt = _dev(t)
    gen = torch.Generator().manual_seed(9)
    base = tuple(torch.randn(v.shape, generator=gen).to(v.dtype) for v in t[:3])
    bufs = tuple(b.to(DEV) for b in base)
    got = _native(dt, shapes, points, grads=bufs)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got[1:], bufs))
    assert tuple(b.dtype for b in bufs) == (F16, F32, F32)
    for what, a, b, w, tol in zip(NAMES[1:], got[1:], base, want[1:], _tols(t)[1:]):
        assert_close("accumulate %s" % what, a, b.double() + w, tol)
    fresh = _native(dt, shapes, points, deterministic=True)
    nans = tuple(torch.full_like(b, float("nan")) for b in bufs)
    over = _native(dt, shapes, points, grads=nans, accumulate=False, deterministic=True)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(over[1:], nans))
    _compare("overwrite", over, want, _tols(t))
    for what, a, b in zip(NAMES, over, fresh):
        assert torch.equal(a, b), what


# ---- "element" arguments ----
@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("form, dtype, coord_dtype", [((1, 4), F32, None), (("L", 4), F16, None), (("L", 2), BF16, F32)])
def test_element_arguments_at_offsets(form, dtype, coord_dtype, k):
    """The "element" arguments -- offs_attn, reference_points and their gradients -- as views ``k`` elements past a 16-byte
    boundary, between guard margins: every result is bit for bit that of the call on freshly allocated tensors, and no margin
    changes."""
    t, shapes, points, _ = _case("dfine", form, dtype, coord_dtype)
    value, ref, oa, go = dt = _dev(t)
    want = _native(dt, shapes, points, deterministic=True)
    tensors = (oa, torch.zeros_like(oa), ref, torch.zeros_like(ref))
    views, checks = zip(*(at_offset(v, k, mod16=(k * v.element_size()) % 16) for v in tensors))
    assert all(v.data_ptr() % 16 == (k * v.element_size()) % 16 for v in views)
    gv = torch.zeros_like(value)
    got = _native((value, views[2], views[0], go), shapes, points, grads=(gv, views[3], views[1]), deterministic=True,
                  accumulate=False)
    assert got[3].data_ptr() == views[1].data_ptr() and got[2].data_ptr() == views[3].data_ptr()
    for what, a, b in zip(NAMES, got, want):
        assert torch.equal(a, b), "%s at offset %d differs (%d elements)" % (what, k, int((a != b).sum()))
    for name, check in zip(("offs_attn", "grad_offs_attn", "reference_points", "grad_reference_points"), checks):
        check("%s at offset %d" % (name, k))


# ---- random shapes ----
def _random_case(seed):
    """A shape inside the shape rule by construction, in the manner of tests/test_gpu_fdap.py: D a multiple of 4 (fp32) or
    8 (16-bit), K <= 72, tiny tensors; the pairing, the level count and the form walk their ranges with the seed."""
    rng = random.Random(3000 + seed)
    dtype, coord_dtype = PAIRINGS[seed % len(PAIRINGS)]
    L = seed % 8 + 1
    form = ((1, 4), ("L", 4), ("L", 2), (1, 2))[seed // 2 % 4]
    kw = dict(N=rng.randint(1, 2), M=rng.randint(1, 4), D=(4, 8, 12, 32)[seed // 5 % 4] if dtype == F32 else rng.choice((8, 32)),
              shapes=[(rng.randint(2, 6), rng.randint(2, 6)) for _ in range(L)],
              points=tuple(rng.randint(1, 9) for _ in range(L)), Lq=rng.randint(2, 9))
    return kw, form, dtype, coord_dtype


def test_random_generator_covers_the_space():
    drawn = [_random_case(s) for s in range(16)]
    assert {len(kw["shapes"]) for kw, _, _, _ in drawn} == set(range(1, 9)) and {kw["D"] for kw, _, _, _ in drawn} == {4, 8, 12, 32}
    assert {(d, c) for _, _, d, c in drawn} == set(PAIRINGS)
    assert {f for _, f, _, _ in drawn} == {(1, 4), ("L", 4), ("L", 2), (1, 2)}
    assert sum(len(set(kw["points"])) > 1 for kw, _, _, _ in drawn) >= 10   # unequal counts
    assert {kw["M"] for kw, _, _, _ in drawn} >= {1, 3}
    for kw, _, dtype, _ in drawn:
        assert kw["D"] % (4 if dtype == F32 else 8) == 0 and 1 <= sum(kw["points"]) <= 72


@pytest.mark.parametrize("seed", range(16))
def test_random_shapes(seed):
    kw, form, dtype, coord_dtype = _random_case(seed)
    t = R.make_inputs(Lr=form[0], R=form[1], dtype=dtype, coord_dtype=coord_dtype, seed=seed, **kw)
    want = R.afda_ref_grads(t[0], kw["shapes"], kw["points"], t[1], t[2], t[3])
    got = _native(_dev(t), kw["shapes"], kw["points"], deterministic=bool(seed & 1))
    _compare("random %d %s %s" % (seed, form, kw), got, want, _tols(t))


# ---- the module and autograd ----
@pytest.mark.parametrize("ref_levels", [1, 3])
def test_module_step_under_autocast(ref_levels):
    """``MSDeformableAttentionAnchored([3, 6, 3])`` under torch.autocast(bfloat16), with a value mask, against the same module
    with the core swapped for the reference, and against ``MSDeformableAttention`` loaded with the same ``state_dict``:
    output, input gradients, grad_reference and every parameter gradient at the bf16 tolerance.  The core receives a bf16
    value, a bf16 packed row and an fp32 reference."""
    from modulated_deform_conv_amd import MSDeformableAttention, MSDeformableAttentionAnchored, anchored_deform_attn
    torch.manual_seed(21 + ref_levels)
    shapes = [(6, 5), (3, 3), (2, 2)]
    S, N, Lq, C = 43, 2, 7, 32
    mod = MSDeformableAttentionAnchored(embed_dim=C, num_heads=4, num_levels=3, num_points=[3, 6, 3]).to(DEV)
    with torch.no_grad():   # offsets and logits that depend on the query
        mod.sampling_offsets.weight.normal_(0, 0.05)
        mod.attention_weights.weight.normal_(0, 0.2)
    parent = MSDeformableAttention(embed_dim=C, num_heads=4, num_levels=3, num_points=[3, 6, 3]).to(DEV)
    parent.load_state_dict(mod.state_dict())
    query = torch.randn(N, Lq, C, device=DEV)
    flat = torch.randn(N, S, C, device=DEV)
    boxes = torch.cat([torch.rand(N, Lq, ref_levels, 2, device=DEV) * 0.6 + 0.2, torch.rand(N, Lq, ref_levels, 2, device=DEV) * 0.3 + 0.1], -1)
    keep = torch.ones(N, S, dtype=torch.bool, device=DEV)
    keep[1, 25:30] = False
    go = torch.randn(N, Lq, C, device=DEV)
    seen = []

    def native_core(value, spatial_shapes, num_points_list, reference_points, offs_attn, offset_scale):
        seen.append((value.dtype, offs_attn.dtype, reference_points.dtype, tuple(offs_attn.shape), offset_scale))
        return anchored_deform_attn(value, spatial_shapes, num_points_list, reference_points, offs_attn, offset_scale)

    def run(m):
        m.zero_grad(set_to_none=True)
        qi, fi, ri = (v.clone().requires_grad_(True) for v in (query, flat, boxes))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(qi, ri, fi, shapes, keep)
        assert y.dtype == torch.bfloat16
        y.backward(go.to(y.dtype))
        torch.cuda.synchronize()
        return dict(output=y.detach(), grad_query=qi.grad, grad_input=fi.grad, grad_reference=ri.grad,
                    **{k: p.grad.clone() for k, p in m.named_parameters()})

    mod._core = native_core
    native = run(mod)
    mod._core = R.afda_ref
    ref = run(mod)
    theirs = run(parent)
    assert seen == [(BF16, BF16, F32, (N, Lq, 4, 36), 0.5)]
    assert all(v is not None for v in native.values()) and set(native) == set(theirs)
    assert native["grad_reference"].dtype == F32 and native["grad_reference"].shape == boxes.shape
    assert float(native["grad_input"][1, 25:30].abs().max()) == 0.0   # masked rows take no gradient
    for k in native:
        assert_close("module %s against the reference core" % k, native[k], ref[k], TOL[BF16])
        assert_close("module %s against MSDeformableAttention" % k, native[k], theirs[k], TOL[BF16])


def test_selective_backward_through_autograd(monkeypatch):
    """``reference_points`` needs no gradient: ``grad_reference == 0`` in the descriptor and a NULL pointer; ``value`` needs
    none: NO_GRAD_INPUT, grad_value NULL, and -- with the reference needing none either -- workspace 0.  Tensor
    ``spatial_shapes`` and ``num_points_list`` are taken."""
    from modulated_deform_conv_amd import AnchoredDeformAttnFunction, _capi, afda, anchored_deform_attn
    t, shapes, points, want = _case("rect_123", ("L", 4), F32, None)
    value, ref, oa, go = _dev(t)
    real, calls = afda._run, []

    def spy(fn_name, d, backward, args, like):
        ws = _capi.lib().mdconv_afda_workspace_bytes(ctypes.byref(d), int(backward))
        calls.append((fn_name, int(d.flags), int(d.grad_reference), int(ws), (args[4].value, args[5].value) if backward else None))
        return real(fn_name, d, backward, args, like)

    monkeypatch.setattr(afda, "_run", spy)
    o = oa.clone().requires_grad_(True)
    out = AnchoredDeformAttnFunction.apply(value, torch.tensor(shapes), torch.tensor(points), ref, o, 0.5)
    out.backward(go)
    assert value.grad is None and ref.grad is None
    assert [c[0] for c in calls] == ["mdconv_afda_forward", "mdconv_afda_backward"]
    assert calls[1][1] & _capi.FLAG_NO_GRAD_INPUT and calls[1][2] == 0 and calls[1][3] == 0 and calls[1][4] == (None, None)
    assert_close("selective output", out.detach(), want[0], 1e-4)
    assert_close("selective grad_offs_attn", o.grad, want[3], 1e-4)
    # value alone
    del calls[:]
    v = value.clone().requires_grad_(True)
    anchored_deform_attn(v, shapes, points, ref, oa).backward(go)
    assert oa.grad is None and ref.grad is None
    assert not calls[1][1] & _capi.FLAG_NO_GRAD_INPUT and calls[1][2] == 0 and calls[1][4][0] and not calls[1][4][1]
    assert_close("selective grad_value", v.grad, want[1], 1e-4)
    # the reference alone
    del calls[:]
    r = ref.clone().requires_grad_(True)
    anchored_deform_attn(value, shapes, points, r, oa).backward(go)
    assert calls[1][1] & _capi.FLAG_NO_GRAD_INPUT and calls[1][2] == 1 and calls[1][3] > 0 and not calls[1][4][0] and calls[1][4][1]
    assert_close("selective grad_reference", r.grad, want[2], 1e-4)
    # all three through autograd
    del calls[:]
    v2, r2, o2 = (x.detach().clone().requires_grad_(True) for x in (value, ref, oa))
    anchored_deform_attn(v2, shapes, points, r2, o2).backward(go)
    assert not calls[1][1] & _capi.FLAG_NO_GRAD_INPUT and calls[1][2] == 1 and all(calls[1][4])
    for what, a, b in zip(NAMES[1:], (v2.grad, r2.grad, o2.grad), want[1:]):
        assert_close("autograd %s" % what, a, b, 1e-4)
