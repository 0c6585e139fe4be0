"""Packed deformable attention with a point count per level on the GPU (include/mdconv_fdap.h): output and the two gradients
against ``tests.fdap_ref`` -- the fp64 softmax of the logits the tensor holds, then the fp64 reference of deformable
attention with a point count per level -- at the project's tolerances: 1e-4 for fp32, ``TOL`` of tests/test_gpu_hp.py for
fp16 / bf16, by the value dtype for value-typed results and by the coordinate dtype for the packed gradient.  The geometries
are ``CASES`` of tests/test_gpu_msdap.py: the smallest at which the level lookup and the strided softmax can go wrong.
Beyond parity: bit-equality with ``flash_deform_attn`` at equal counts, the softmax's range, the zero sum of the logit
gradients, the gate and the gradient conventions, the composed route, the call modes, random shapes, and the module under
autocast."""
import ctypes
import functools
import random

import pytest
import torch

from tests import fdap_ref as R
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
NAMES = ("output", "grad_value", "grad_sampling_loc_attn")

CASES = dict(MSDAP_CASES)
# one level, one tap: the softmax of one logit is 1, and its gradient is zero
CASES["one_tap"] = dict(N=1, M=2, D=4, shapes=[(4, 5)], points=(1,), Lq=6)
ONE_HOT_TAP = 5   # of dfine: a tap of level 1


@functools.lru_cache(maxsize=None)
def _case(name, dtype, coord_dtype=None, shift=0.0, one_hot=False):
    """CPU inputs of a case and its fp64 reference (output and the two gradients), computed once and left unchanged."""
    kw = CASES[name]
    shapes, points = kw["shapes"], kw["points"]
    value, loc_attn, go = R.make_inputs(dtype=dtype, coord_dtype=coord_dtype, seed=len(name) + 7, shift=shift, **kw)
    loc, logits = R.unpack(loc_attn, points)   # views
    if name == "far":
        gen = torch.Generator().manual_seed(5)
        loc.copy_(torch.where(torch.rand(loc.shape, generator=gen) < 0.5, -3.0, 4.0))
    else:
        for l in range(len(shapes)):
            assert MR.min_lattice_distance(loc, shapes, points, level=l) >= R.MARGIN
    if one_hot:   # one (query, head) nearly one-hot: weights 1 - (K - 1) e^-80 and e^-80
        logits[0, 0, 0] = -40.0
        logits[0, 0, 0, ONE_HOT_TAP] = 40.0
    return (value, loc_attn, go), shapes, points, R.fdap_ref_grads(value, shapes, points, loc_attn, go)


def _dev(t):
    return tuple(v.to(DEV) for v in t)


def _native(t, shapes, points, grads=None, need_grad_value=True, deterministic=False, accumulate=None):
    from modulated_deform_conv_amd import fdap
    value, loc_attn, go = t
    out = fdap.flash_deform_attn_points_forward(value, shapes, points, loc_attn)
    g = fdap.flash_deform_attn_points_backward(value, shapes, points, loc_attn, go, grads=grads, need_grad_value=need_grad_value,
                                               deterministic=deterministic, accumulate=accumulate)
    torch.cuda.synchronize()
    return (out,) + tuple(g)


def _tols(t):
    """Per result: value-typed results by the value dtype, the packed gradient by the coordinate dtype."""
    return (TOL[t[0].dtype], TOL[t[0].dtype], TOL[t[1].dtype])


def _compare(tag, got, want, tols):
    for what, a, b, tol in zip(NAMES, got, want, tols):
        if a is None:
            continue
        print("%s %s: max |want| %.3e" % (tag, what, float(b.abs().max())))
        assert_close("%s %s" % (tag, what), a, b, tol)


# ---- parity ----
@pytest.mark.parametrize("name, dtype, coord_dtype", [
    ("rect_123", F32, None), ("rect_123", F16, None),
    ("dfine", F32, None), ("dfine", F16, None), ("dfine", BF16, None), ("dfine", F16, F32), ("dfine", BF16, F32),
    ("eight_levels", F32, None), ("long_level", F32, None), ("k_below_vl", F32, None),
    ("two_rounds", F32, None), ("two_rounds_16bit", F16, None), ("one_tap", F32, None),
])
def test_against_reference(name, dtype, coord_dtype):
    """rect_123: K = 6, a 1x1 level, W against H.  dfine: K = 12, level boundaries at taps 3 and 9 inside two tap batches.
    eight_levels: the whole select chain.  long_level: K = 71, more taps than a wave has lanes -- the softmax strides.
    k_below_vl: K = 3 under 16 lanes -- idle lanes enter neither the maximum nor the sum.  one_tap: the weight is 1 and the
    logit gradient exactly zero."""
    t, shapes, points, want = _case(name, dtype, coord_dtype)
    got = _native(_dev(t), shapes, points)
    assert got[0].dtype == got[1].dtype == dtype and got[2].dtype == (coord_dtype or dtype)
    assert got[2].shape == t[1].shape and got[2].shape[-1] == 3 * sum(points)
    _compare("%s %s/%s" % (name, dtype, coord_dtype), got, want, _tols(t))
    if name == "one_tap":
        assert float(want[2][..., 2:].abs().max()) == 0.0 and float(got[2][..., 2:].abs().max()) == 0.0
        assert float(got[2][..., :2].abs().max()) > 0


# ---- equality with the existing packed operator ----
@pytest.mark.parametrize("shapes, P, D", [([(8, 8), (4, 4), (2, 2), (1, 1)], 4, 32), ([(5, 7)], 5, 8)])
@pytest.mark.parametrize("dtype, coord_dtype", PAIRINGS)
def test_equal_counts_are_bit_identical_to_flash_deform_attn(shapes, P, D, dtype, coord_dtype):
    """With equal counts nothing but the level lookup differs from ``FdaOp``: the output and the packed gradient are
    bit-identical to ``flash_deform_attn_forward`` / ``_backward`` on the same memory, and so is grad_value under
    ``deterministic=True``."""
    from modulated_deform_conv_amd import fda
    L = len(shapes)
    N, M, Lq = 2, 8 if L > 1 else 3, 10
    value, loc_attn, go = dt = _dev(R.make_inputs(N=N, M=M, D=D, shapes=shapes, points=(P,) * L, Lq=Lq, dtype=dtype,
                                                  coord_dtype=coord_dtype, seed=31))
    got = _native(dt, shapes, (P,) * L, deterministic=True)
    out = fda.flash_deform_attn_forward(value, shapes, loc_attn, P)
    gv, gla = fda.flash_deform_attn_backward(value, shapes, loc_attn, P, go, deterministic=True)
    torch.cuda.synchronize()
    K = L * P
    assert all(float(g.float().abs().max()) > 0 for g in got)
    assert float(got[2][..., :2 * K].float().abs().max()) > 0 and float(got[2][..., 2 * K:].float().abs().max()) > 0
    for what, a, b in zip(NAMES, got, (out, gv, gla)):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a, b), "%s differs from flash_deform_attn (%d elements)" % (what, int((a != b).sum()))


# ---- the softmax ----
@pytest.mark.parametrize("dtype, shift", [(F32, 90.0), (F16, 1000.0)])
def test_softmax_range(dtype, shift):
    """Logits around +90 in fp32 and around +1000 in fp16: exp of either overflows fp32 (e^88.8 is its largest finite
    value), so a softmax without the maximum subtracted returns inf / inf there."""
    t, shapes, points, want = _case("dfine", dtype, None, shift)
    logits = R.unpack(t[1], points)[1]
    assert float(logits.float().exp().max()) == float("inf")
    got = _native(_dev(t), shapes, points)
    assert all(bool(torch.isfinite(g.float()).all()) for g in got)
    _compare("range %s" % dtype, got, want, _tols(t))


def test_nearly_one_hot_pair():
    """One (query, head) with logits -40 but for +40 on a tap of level 1: the other weights are e^-80, far below fp32's
    epsilon beside 1 and still normal numbers; the pair's logit gradients and the location gradients of its other taps
    vanish with them."""
    t, shapes, points, want = _case("dfine", F32, None, 0.0, True)
    assert MR.tap_levels(points)[ONE_HOT_TAP] == 1
    got = _native(_dev(t), shapes, points)
    _compare("one-hot", got, want, _tols(t))
    K = sum(points)
    row = got[2][0, 0, 0].double().cpu()
    assert float(row[2 * K:].abs().max()) < 1e-30 and bool(torch.isfinite(row).all())
    others = [e for tap in range(K) if tap != ONE_HOT_TAP for e in (2 * tap, 2 * tap + 1)]
    assert float(row[others].abs().max()) < 1e-30
    assert float(want[2][0, 0, 0, 2 * ONE_HOT_TAP:2 * ONE_HOT_TAP + 2].abs().max()) > 0   # the hot tap's sample is read


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (BF16, F32), (F16, F32)])
def test_logit_gradients_sum_to_zero(dtype, coord_dtype):
    """sum_t a[t] (g[t] - S) = S - S: per (query, head) the logit gradients sum to zero -- gated-out taps (g = 0) included --
    within the coordinate tolerance times the largest logit gradient: 1e-4 for the fp32 packed gradient of all three value
    dtypes.  (What stands against it: the K = 12 stored values are rounded once each, at most 2^-24 of the largest, and the
    fp32 sums g[t] and S carry a few 1e-7 of the largest |g|.  A 16-bit packed gradient is left out: 12 roundings of 2^-11 /
    2^-8 of the largest could add up to more than that dtype's tolerance, so the bound would be no property of the operator
    there.)"""
    t, shapes, points, want = _case("dfine", dtype, coord_dtype)
    got = _native(_dev(t), shapes, points)
    assert got[2].dtype == F32
    glogit = got[2][..., 2 * sum(points):].double().cpu()
    largest = float(glogit.abs().max())
    worst = float(glogit.sum(-1).abs().max())
    print("zero sum %s/%s: largest logit gradient %.3e, worst pair sum %.3e" % (dtype, coord_dtype, largest, worst))
    assert largest > 0 and worst <= TOL[F32] * largest


def test_mixed_dtype_packed_gradient_at_fp32_tolerance():
    """bf16 values beside an fp32 packed tensor: the packed gradient is an fp32 result and holds 1e-4 -- the pair sum S comes
    from the fp32 sums of the call, not from a stored bf16 output."""
    t, shapes, points, want = _case("dfine", BF16, F32)
    got = _native(_dev(t), shapes, points)
    assert got[0].dtype == BF16 and got[2].dtype == F32
    K = sum(points)
    print("mixed: max |grad_sampling_loc_attn| %.3e" % float(want[2].abs().max()))
    assert_close("mixed grad_sampling_loc_attn", got[2], want[2], 1e-4)
    assert_close("mixed logit gradients", got[2][..., 2 * K:], want[2][..., 2 * K:], 1e-4)


# ---- the gate and the gradient conventions ----
def test_samples_wholly_outside():
    """Locations of -3 / +4: nothing is read; output, grad_value and the location gradients are exactly zero, and so are the
    logit gradients: g = 0 for every tap and S = 0."""
    t, shapes, points, want = _case("far", F32)
    assert all(float(w.abs().max()) == 0.0 for w in want)
    got = _native(_dev(t), shapes, points)
    assert all(float(g.abs().max()) == 0.0 for g in got)


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (F16, None), (BF16, F32)])
def test_integer_positions_keep_the_pinned_convention(dtype, coord_dtype):
    """Every pixel coordinate an integer, both edges of the gate included, per level: the right-sided derivative of the cell
    floor(x), floor(y) and exact zeros for the location gradients outside the gate -- ``msdap_direct`` behind the fp64
    softmax states it.  The LOGIT gradient of a gated-out tap is -a[t] S: not zero, and the reference's."""
    shapes, points = [(8, 4), (2, 2), (1, 4)], (2, 1, 3)
    t = R.make_lattice_inputs(1, 2, 8, shapes, points, dtype=dtype, coord_dtype=coord_dtype, seed=2)
    want = R.fdap_ref_grads(t[0], shapes, points, t[1], t[2], fn=MR.msdap_direct)
    got = _native(_dev(t), shapes, points, deterministic=True)
    _compare("lattice %s/%s" % (dtype, coord_dtype), got, want, _tols(t))
    loc = R.unpack(t[1], points)[0]
    gate = MR.gate_of(loc, shapes, points)
    assert not bool(gate.all())
    gloc, glogit = R.unpack(got[2].cpu(), points)
    assert float(gloc[~gate].float().abs().max()) == 0.0
    assert float(R.unpack(want[2], points)[1][~gate].abs().max()) > 0 and float(glogit[~gate].float().abs().max()) > 0


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (F16, None), (BF16, F32)])
def test_nonfinite_coordinates_are_gated_out(dtype, coord_dtype):
    """NaN / +-Inf coordinates in a few taps of all three levels contribute nothing: every result equals, bit for bit, the
    call with those coordinates far outside (-3), their own location gradients are exact zeros over NaN-filled buffers, and
    nothing is non-finite.  (No non-finite logits: their result is unspecified.)"""
    t, shapes, points, _ = _case("dfine", dtype, coord_dtype)
    value, loc_attn, go = t
    inf, nan = float("inf"), float("nan")
    # (image, query, head, tap, xy)
    spots = [((0, 1, 2, 1, 0), nan), ((1, 3, 5, 4, 1), inf), ((0, 7, 0, 10, 0), -inf), ((0, 7, 0, 10, 1), -inf),
             ((1, 9, 7, 8, 0), nan), ((1, 9, 7, 9, 1), inf), ((0, 0, 0, 0, 0), -inf), ((1, 9, 7, 11, 1), nan)]
    assert {MR.tap_levels(points)[s[3]] for s, _ in spots} == {0, 1, 2}
    bad, far = loc_attn.clone(), loc_attn.clone()
    for (n, q, m, tap, xy), v in spots:
        bad[n, q, m, 2 * tap + xy] = v
        far[n, q, m, 2 * tap + xy] = -3.0
    assert bool(torch.isfinite(bad[..., 2 * sum(points):]).all())

    def run(la):
        dt = _dev((value, la, go))
        bufs = tuple(torch.full_like(v, nan) for v in dt[:2])
        return _native(dt, shapes, points, grads=bufs, deterministic=True, accumulate=False)

    base, got = run(far), run(bad)
    _compare("replaced", base, R.fdap_ref_grads(value, shapes, points, far, go), _tols(t))
    for what, a, b in zip(NAMES, got, base):
        assert bool(torch.isfinite(a.float()).all()), what
        assert torch.equal(a, b), "%s differs from the run with the coordinates far outside (%d elements)" % (what, int((a != b).sum()))
    for (n, q, m, tap, _), _ in spots:
        assert float(got[2][n, q, m, 2 * tap:2 * tap + 2].float().abs().max()) == 0.0, (n, q, m, tap)


# ---- the composed route ----
@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (BF16, F32)])
def test_equals_ms_deform_attn_points_behind_a_framework_softmax(dtype, coord_dtype):
    """The native call against the composed route on the GPU: slices of the same packed tensor, ``torch.softmax``,
    ``ms_deform_attn_points``, autograd's concatenation of the two gradients."""
    from modulated_deform_conv_amd import flash_deform_attn_points, ms_deform_attn_points
    t, shapes, points, want = _case("dfine", dtype, coord_dtype)
    value, loc_attn, go = _dev(t)
    K = sum(points)
    N, Lq, M = loc_attn.shape[:3]
    results = []
    for route in ("native", "composed"):
        v, la = value.clone().requires_grad_(True), loc_attn.clone().requires_grad_(True)
        if route == "native":
            out = flash_deform_attn_points(v, shapes, points, la)
        else:
            loc = la[..., :2 * K].reshape(N, Lq, M, K, 2)
            attn = torch.softmax(la[..., 2 * K:], -1)
            out = ms_deform_attn_points(v, shapes, points, loc, attn)
        out.backward(go)
        torch.cuda.synchronize()
        results.append((out.detach(), v.grad, la.grad))
    native, composed = results
    for what, a, b, tol in zip(NAMES, native, composed, _tols(t)):
        assert a.dtype == b.dtype
        assert_close("equivalence %s" % what, a, b, tol)
    _compare("equivalence native", native, want, _tols(t))


# ---- call modes, on the D-FINE case ----
def test_accumulate_against_overwrite():
    """fp16 values with an fp32 packed tensor.  Accumulate: each buffer + gradient in its own dtype, rounded once.
    Overwrite into NaN-filled buffers: the gradient alone, bit for bit that of a call into fresh tensors."""
    t, shapes, points, want = _case("dfine", F16, F32)
    dt = _dev(t)
    gen = torch.Generator().manual_seed(9)
    base = tuple(torch.randn(v.shape, generator=gen).to(v.dtype) for v in t[:2])
    bufs = tuple(b.to(DEV) for b in base)
    got = _native(dt, shapes, points, grads=bufs)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got[1:], bufs))
    assert (bufs[0].dtype, bufs[1].dtype) == (F16, F32)
    for what, a, b, w, tol in zip(NAMES[1:], got[1:], base, want[1:], _tols(t)[1:]):
        assert_close("accumulate %s" % what, a, b.double() + w, tol)
    fresh = _native(dt, shapes, points, deterministic=True)
    nans = tuple(torch.full_like(b, float("nan")) for b in bufs)
    over = _native(dt, shapes, points, grads=nans, accumulate=False, deterministic=True)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(over[1:], nans))
    _compare("overwrite", over, want, _tols(t))
    for what, a, b in zip(NAMES, over, fresh):
        assert torch.equal(a, b), what


def _guard(monkeypatch, touched, calls):
    """tests.util.guarded_run in the place of fdap._run; it sizes the workspace through ``mdconv_workspace_bytes`` of the
    library handle, which for this operator's descriptor is ``mdconv_fdap_workspace_bytes``."""
    from modulated_deform_conv_amd import _capi, fdap
    real = _capi.lib()

    class Lib:
        mdconv_workspace_bytes = staticmethod(real.mdconv_fdap_workspace_bytes)

        def __getattr__(self, name):
            return getattr(real, name)

    proxy = Lib()
    monkeypatch.setattr(_capi, "lib", lambda: proxy)
    monkeypatch.setattr(fdap, "_run", guarded_run(touched, calls))


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (BF16, F32)])
def test_no_grad_value_under_the_guarded_workspace(monkeypatch, dtype, coord_dtype):
    """NO_GRAD_INPUT: grad_value NULL, no workspace (no lists, no statistics) between pattern-filled margins; the packed
    gradient is bit for bit that of the full call.  The full and the deterministic call run guarded as well, their
    workspace pattern-filled -- the list kernels read the statistics the coordinate kernel wrote, not zeros -- and the
    figure is exact."""
    t, shapes, points, want = _case("dfine", dtype, coord_dtype)
    dt = _dev(t)
    full = _native(dt, shapes, points)
    touched, calls = [], []
    _guard(monkeypatch, touched, calls)
    part = _native(dt, shapes, points, need_grad_value=False)
    again = _native(dt, shapes, points)
    det = _native(dt, shapes, points, deterministic=True)
    assert touched == [], touched
    sizes = [b for name, b in calls if name == "mdconv_fdap_backward"]
    assert [b for name, b in calls if name == "mdconv_fdap_forward"] == [0, 0, 0]
    assert sizes[0] == 0 < sizes[1] <= sizes[2], sizes
    assert part[1] is None
    for i in (0, 2):
        assert torch.equal(part[i], full[i]) and torch.equal(again[i], full[i]) and torch.equal(det[i], full[i]), NAMES[i]
    _compare("guarded full", again, want, _tols(t))
    _compare("guarded deterministic", det, want, _tols(t))


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (F16, F32)])
def test_deterministic_mode_and_graph_replay(dtype, coord_dtype):
    """With the flag all three results are bit-identical between two eager runs and two replays of a HIP graph that holds
    forward + backward into caller buffers; without it the output and the packed gradient are as well and grad_value is
    within tolerance."""
    from modulated_deform_conv_amd import fdap
    t, shapes, points, want = _case("dfine", dtype, coord_dtype)
    value, loc_attn, go = dt = _dev(t)
    first = _native(dt, shapes, points, deterministic=True)
    second = _native(dt, shapes, points, deterministic=True)
    for what, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), "deterministic %s differs between two runs" % what
    plain = [_native(dt, shapes, points) for _ in range(2)]
    for i in (0, 2):
        assert torch.equal(plain[0][i], plain[1][i]) and torch.equal(plain[0][i], first[i]), NAMES[i]
    assert_close("unflagged grad_value", plain[0][1], want[1], TOL[dtype])
    _compare("deterministic", first, want, _tols(t))

    out = torch.empty_like(first[0])
    bufs = (torch.empty_like(value), torch.empty_like(loc_attn))

    def step():
        fdap.flash_deform_attn_points_forward(value, shapes, points, loc_attn, output=out)
        fdap.flash_deform_attn_points_backward(value, shapes, points, loc_attn, go, grads=bufs, deterministic=True,
                                               accumulate=False)

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


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (F16, None), (BF16, F32)])
def test_element_arguments_at_offsets(dtype, coord_dtype, k):
    """The "element" arguments -- sampling_loc_attn and its gradient -- as views ``k`` elements past a 16-byte boundary,
    between guard margins: every result is bit for bit that of the call on freshly allocated tensors, and no margin
    changes."""
    t, shapes, points, _ = _case("dfine", dtype, coord_dtype)
    value, loc_attn, go = dt = _dev(t)
    want = _native(dt, shapes, points, deterministic=True)
    es = loc_attn.element_size()
    views, checks = zip(*(at_offset(v, k, mod16=(k * es) % 16) for v in (loc_attn, torch.zeros_like(loc_attn))))
    # (4 fp32 elements are 16 bytes: that view is on a 16-byte boundary again, one vector past the buffer's)
    assert all(v.data_ptr() % 16 == (k * es) % 16 for v in views) and ((k * es) % 16 != 0 or (es, k) == (4, 4))
    gv = torch.zeros_like(value)
    got = _native((value, views[0], go), shapes, points, grads=(gv, views[1]), deterministic=True, accumulate=False)
    assert got[2].data_ptr() == views[1].data_ptr()
    for what, a, b in zip(NAMES, got, want):
        assert torch.equal(a, b), "%s at offset %d differs (%d elements)" % (what, k, int((a != b).sum()))
    for name, check in zip(("sampling_loc_attn", "grad_sampling_loc_attn"), checks):
        check("%s at offset %d" % (name, k))


# ---- random shapes ----
def _random_case(seed):
    """A shape inside the shape rule by construction: D a multiple of 4 (fp32) or 8 (16-bit), K <= 72, tiny tensors.  The
    pairing and the level count walk their ranges with the seed (16 seeds: every L twice, the fp32 seeds 0, 5, 10, 15 every
    D once); counts, extents, N, M and Lq are drawn."""
    rng = random.Random(2000 + seed)
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
    assert sum(len(set(kw["points"])) > 1 for kw, _, _ in drawn) >= 10   # unequal counts
    for kw, dtype, _ in drawn:
        assert kw["D"] % (4 if dtype == F32 else 8) == 0 and 1 <= sum(kw["points"]) <= 72


@pytest.mark.parametrize("seed", range(16))
def test_random_shapes(seed):
    kw, dtype, coord_dtype = _random_case(seed)
    t = R.make_inputs(dtype=dtype, coord_dtype=coord_dtype, seed=seed, **kw)
    want = R.fdap_ref_grads(t[0], kw["shapes"], kw["points"], t[1], t[2])
    got = _native(_dev(t), kw["shapes"], kw["points"], deterministic=bool(seed & 1))
    _compare("random %d %s" % (seed, kw), got, want, _tols(t))


# ---- the module and autograd ----
@pytest.mark.parametrize("ref_levels", [1, 3])
def test_module_step_under_autocast(ref_levels):
    """``MSDeformableAttentionFused([3, 6, 3])`` under torch.autocast(bfloat16), with a value mask, against the same module
    with the core swapped for the reference, and against ``MSDeformableAttention`` loaded with the same ``state_dict``:
    output, input gradients and every parameter gradient at the bf16 tolerance.  The core receives a bf16 value and an fp32
    packed tensor: the mixed call."""
    from modulated_deform_conv_amd import MSDeformableAttention, MSDeformableAttentionFused, flash_deform_attn_points
    torch.manual_seed(21 + ref_levels)
    shapes = [(6, 5), (3, 3), (2, 2)]
    S, N, Lq, C = 43, 2, 7, 32
    mod = MSDeformableAttentionFused(embed_dim=C, num_heads=4, num_levels=3, num_points=[3, 6, 3]).to(DEV)
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

    def native_core(value, spatial_shapes, num_points_list, loc_attn):
        seen.append((value.dtype, loc_attn.dtype, tuple(loc_attn.shape)))
        return flash_deform_attn_points(value, spatial_shapes, num_points_list, loc_attn)

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
    mod._core = R.fdap_ref
    ref = run(mod)
    theirs = run(parent)
    assert seen == [(BF16, F32, (N, Lq, 4, 36))]
    assert all(v is not None for v in native.values()) and set(native) == set(theirs)
    assert float(native["grad_input"][1, 25:30].abs().max()) == 0.0   # masked rows take no gradient
    for k in native:
        assert_close("module %s against the reference core" % k, native[k], ref[k], TOL[BF16])
        assert_close("module %s against MSDeformableAttention" % k, native[k], theirs[k], TOL[BF16])


def test_selective_backward_through_autograd(monkeypatch):
    """``value`` needs no gradient: the backward runs with NO_GRAD_INPUT -- no lists, no statistics, no workspace -- with
    grad_value NULL, and still returns the packed gradient; the packed tensor needs none: only grad_value comes back.
    Tensor ``spatial_shapes`` and ``num_points_list`` are taken."""
    from modulated_deform_conv_amd import FlashDeformAttnPointsFunction, _capi, fdap, flash_deform_attn_points
    t, shapes, points, want = _case("rect_123", F32)
    value, loc_attn, go = _dev(t)
    real, calls = fdap._run, []

    def spy(fn_name, d, backward, args, like):
        ws = _capi.lib().mdconv_fdap_workspace_bytes(ctypes.byref(d), int(backward))
        calls.append((fn_name, int(d.flags), int(ws), args[3].value if backward else None))
        return real(fn_name, d, backward, args, like)

    monkeypatch.setattr(fdap, "_run", spy)
    la = loc_attn.clone().requires_grad_(True)
    out = FlashDeformAttnPointsFunction.apply(value, torch.tensor(shapes), torch.tensor(points), la)
    out.backward(go)
    assert value.grad is None
    assert [c[0] for c in calls] == ["mdconv_fdap_forward", "mdconv_fdap_backward"]
    assert calls[1][1] & _capi.FLAG_NO_GRAD_INPUT and calls[1][2] == 0 and not calls[1][3]   # no lists; grad_value NULL
    assert_close("selective output", out.detach(), want[0], 1e-4)
    assert_close("selective grad_sampling_loc_attn", la.grad, want[2], 1e-4)
    v = value.clone().requires_grad_(True)
    flash_deform_attn_points(v, shapes, points, loc_attn).backward(go)
    assert loc_attn.grad is None
    assert_close("selective grad_value", v.grad, want[1], 1e-4)
    # both through autograd
    del calls[:]
    v2, l2 = (x.detach().clone().requires_grad_(True) for x in (value, loc_attn))
    flash_deform_attn_points(v2, shapes, points, l2).backward(go)
    assert not calls[1][1] & _capi.FLAG_NO_GRAD_INPUT and calls[1][2] > 0 and calls[1][3]
    for what, a, b in zip(NAMES[1:], (v2.grad, l2.grad), want[1:]):
        assert_close("autograd %s" % what, a, b, 1e-4)
