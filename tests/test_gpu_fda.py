"""Packed deformable attention on the GPU (include/mdconv.h, "Packed deformable attention"): output and the two gradients
against ``tests.fda_ref`` -- the fp64 softmax of the logits the tensor holds, then the fp64 reference of multi-scale
deformable attention -- at the project's tolerances: 1e-4 for fp32, ``TOL`` of tests/test_gpu_hp.py for fp16 / bf16, by the
value dtype for value-typed results and by the coordinate dtype for the packed gradient.  The geometries are the small ones
of tests/test_gpu_msda.py::CASES.  Beyond parity: the softmax's range, the packed gradient of the mixed call, the zero sum of
the logit gradients, equivalence with ``ms_deform_attn`` behind a framework softmax, and the call modes -- accumulate and
overwrite, determinism, NO_GRAD_INPUT under a guarded workspace, selective backward, graph replay, the module under
autocast."""
import functools

import pytest
import torch

from tests import fda_ref as R
from tests.test_gpu_hp import TOL as TOL16
from tests.test_gpu_msda import CASES
from tests.util import assert_close, guarded_run

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(TOL16)
TOL[torch.float32] = 1e-4
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
ALL5 = ((F32, None), (F16, None), (BF16, None), (F16, F32), (BF16, F32))
NAMES = ("output", "grad_value", "grad_sampling_loc_attn")


@functools.lru_cache(maxsize=None)
def _case(name, dtype, coord_dtype=None, shift=0.0, one_hot=False):
    """CPU inputs of a case and its fp64 reference (output and the two gradients), computed once and left unchanged."""
    kw = CASES[name]
    shapes, P = kw["shapes"], kw["P"]
    value, loc_attn, go = R.make_inputs(dtype=dtype, coord_dtype=coord_dtype, seed=len(name) + 7, shift=shift, **kw)
    loc, logits = R.unpack(loc_attn, len(shapes), P)   # views
    if name == "crafted":
        # level 0 (4 x 4): x = 1.3, y = 1.4 in pixels is loc = (x + 0.5) / size
        loc[:, :, :, 0, :, 0] = (1.3 + 0.5) / 4
        loc[:, :, :, 0, :, 1] = (1.4 + 0.5) / 4
    if name == "far":
        gen = torch.Generator().manual_seed(5)
        loc.copy_(torch.where(torch.rand(loc.shape, generator=gen) < 0.5, -3.0, 4.0))
    else:
        assert R.MR.min_lattice_distance(loc, shapes) >= R.MARGIN
    if one_hot:   # one (query, head) nearly one-hot: weights 1 - (K - 1) e^-80 and e^-80
        logits[0, 0, 0] = -40.0
        logits[0, 0, 0, 0, 0] = 40.0
    return (value, loc_attn, go), shapes, P, R.fda_ref_grads(value, shapes, loc_attn, P, go)


def _dev(t):
    return tuple(v.to(DEV) for v in t)


def _native(t, shapes, P, grads=None, need_grad_value=True, deterministic=False, accumulate=True):
    from modulated_deform_conv_amd import fda
    value, loc_attn, go = t
    out = fda.flash_deform_attn_forward(value, shapes, loc_attn, P)
    g = fda.flash_deform_attn_backward(value, shapes, loc_attn, P, go, grads=grads, need_grad_value=need_grad_value,
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


PARITY = ([("one_lane", F32, None), ("three_vectors", F32, None), ("two_rounds", F32, None), ("eight_levels", F32, None),
           ("crafted", F32, None), ("far", F32, None)]
          + [(n, d, c) for n in ("rect_levels", "m8_d32", "k_below_vl") for d, c in ALL5]
          + [("two_rounds_16bit", d, c) for d, c in ALL5[1:]])


@pytest.mark.parametrize("name, dtype, coord_dtype", PARITY)
def test_against_reference(name, dtype, coord_dtype):
    """Every geometry over the dtype pairings it allows (D = 4, 12 and 260 are fp32 shapes).  one_lane has K = 1: weight 1,
    logit gradient 0.  crafted runs with the deterministic flag: one long list per value row.  far reads nothing: output,
    grad_value and every coordinate gradient -- the logits' too, g = 0 for every tap -- are exactly zero."""
    t, shapes, P, want = _case(name, dtype, coord_dtype)
    got = _native(_dev(t), shapes, P, deterministic=name == "crafted")
    assert got[0].dtype == got[1].dtype == dtype and got[2].dtype == (coord_dtype or dtype)
    _compare("%s %s/%s" % (name, dtype, coord_dtype), got, want, _tols(t))
    if name == "one_lane":
        assert float(want[2][..., 2:].abs().max()) == 0.0
    if name == "far":
        assert all(float(w.abs().max()) == 0.0 for w in want) and all(float(g.abs().max()) == 0.0 for g in got)


@pytest.mark.parametrize("name, dtype, shift", [("m8_d32", F32, 90.0), ("k_below_vl", F32, 90.0), ("m8_d32", F16, 1000.0),
                                                ("k_below_vl", F16, 1000.0)])
def test_softmax_range(name, dtype, shift):
    """Logits around +90 in fp32 and around +1000 in fp16: exp of either overflows fp32 (e^88.8 is its largest finite
    value), so a softmax without the maximum subtracted returns inf / inf there."""
    t, shapes, P, want = _case(name, dtype, None, shift)
    logits = R.unpack(t[1], len(shapes), P)[1]
    assert float(logits.float().exp().max()) == float("inf")
    _compare("range %s %s" % (name, dtype), _native(_dev(t), shapes, P), want, _tols(t))


def test_nearly_one_hot_pair():
    """One (query, head) with logits (+40, -40, ..., -40): the other weights are e^-80, far below fp32's epsilon beside 1
    and still normal numbers; the reference's logit gradients there are of the order e^-80 times the others'."""
    t, shapes, P, want = _case("m8_d32", F32, None, 0.0, True)
    got = _native(_dev(t), shapes, P)
    _compare("one-hot", got, want, _tols(t))
    K = len(shapes) * P
    pair = got[2][0, 0, 0, 2 * K:].double().cpu()
    assert float(pair.abs().max()) < 1e-30 and torch.isfinite(pair).all()
    # the pair's output is the first tap's sample alone: the location gradients of the other taps vanish with their weights
    assert float(got[2][0, 0, 0, 2:2 * K].abs().max()) < 1e-30


def test_mixed_dtype_packed_gradient_at_fp32_tolerance():
    """bf16 values beside an fp32 packed tensor: the packed gradient is an fp32 result and holds 1e-4.  The logit gradient
    needs the pair sum S = sum a g = dot(grad_output row, output row); taken from the stored bf16 output it is off by about
    4e-3 of scale (3.6e-3 to 6.0e-3 measured on the fp64 reference for this and two other geometries), taken from the fp32
    sums of the call by 1e-7 to 3e-7."""
    t, shapes, P, want = _case("m8_d32", BF16, F32)
    got = _native(_dev(t), shapes, P)
    assert got[0].dtype == BF16 and got[2].dtype == F32
    print("mixed: max |grad_sampling_loc_attn| %.3e" % float(want[2].abs().max()))
    assert_close("mixed grad_sampling_loc_attn", got[2], want[2], 1e-4)
    K = len(shapes) * P
    assert_close("mixed logit gradients", got[2][..., 2 * K:], want[2][..., 2 * K:], 1e-4)


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (BF16, F32), (F16, F32)])
def test_logit_gradients_sum_to_zero(dtype, coord_dtype):
    """sum_t a[t] (g[t] - S) = S - S: per (query, head) the logit gradients sum to zero, within the coordinate tolerance
    times the largest logit gradient -- 1e-4 for the fp32 packed gradient of all three value dtypes.  (What stands against
    it: the K = 16 stored values are rounded once each, at most 2^-24 of the largest, and the fp32 sums g[t] and S carry a
    few 1e-7 of the largest |g|.  A 16-bit packed gradient is left out: 16 roundings of 2^-11 / 2^-8 of the largest could
    add up to more than that dtype's tolerance, so the bound would be no property of the operator there.)"""
    t, shapes, P, want = _case("m8_d32", dtype, coord_dtype)
    got = _native(_dev(t), shapes, P)
    glogit = got[2][..., 2 * len(shapes) * P:].double().cpu()
    largest = float(glogit.abs().max())
    worst = float(glogit.sum(-1).abs().max())
    print("zero sum %s/%s: largest logit gradient %.3e, worst pair sum %.3e" % (dtype, coord_dtype, largest, worst))
    assert largest > 0 and worst <= TOL[t[1].dtype] * largest


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (BF16, F32)])
def test_equals_ms_deform_attn_behind_a_framework_softmax(dtype, coord_dtype):
    """The native call against the composed route on the GPU: slices of the same packed tensor, ``torch.softmax``,
    ``ms_deform_attn``, autograd's concatenation of the two gradients."""
    from modulated_deform_conv_amd import flash_deform_attn, ms_deform_attn
    t, shapes, P, want = _case("m8_d32", dtype, coord_dtype)
    value, loc_attn, go = _dev(t)
    L, K = len(shapes), len(shapes) * P
    N, Lq, M = loc_attn.shape[:3]
    results = []
    for route in ("native", "composed"):
        v, la = value.clone().requires_grad_(True), loc_attn.clone().requires_grad_(True)
        if route == "native":
            out = flash_deform_attn(v, shapes, la, P)
        else:
            loc = la[..., :2 * K].reshape(N, Lq, M, L, P, 2)
            attn = torch.softmax(la[..., 2 * K:], -1).reshape(N, Lq, M, L, P)
            out = ms_deform_attn(v, shapes, loc, attn)
        out.backward(go)
        torch.cuda.synchronize()
        results.append((out.detach(), v.grad, la.grad))
    native, composed = results
    for what, a, b, tol in zip(NAMES, native, composed, _tols(t)):
        assert a.dtype == b.dtype
        assert_close("equivalence %s" % what, a, b, tol)
    _compare("equivalence native", native, want, _tols(t))


def test_accumulate_against_overwrite():
    """fp16 values with an fp32 packed tensor.  Accumulate: each buffer + gradient in its own dtype, rounded once.
    Overwrite into NaN-filled buffers: the gradient alone, bit for bit that of a call into fresh tensors."""
    t, shapes, P, want = _case("m8_d32", F16, F32)
    dt = _dev(t)
    gen = torch.Generator().manual_seed(9)
    base = tuple(torch.randn(v.shape, generator=gen).to(v.dtype) for v in t[:2])
    bufs = tuple(b.to(DEV) for b in base)
    got = _native(dt, shapes, P, grads=bufs)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got[1:], bufs))
    assert (bufs[0].dtype, bufs[1].dtype) == (F16, F32)
    for what, a, b, w, tol in zip(NAMES[1:], got[1:], base, want[1:], _tols(t)[1:]):
        assert_close("accumulate %s" % what, a, b.double() + w, tol)
    fresh = _native(dt, shapes, P, deterministic=True)
    nans = tuple(torch.full_like(b, float("nan")) for b in bufs)
    over = _native(dt, shapes, P, grads=nans, accumulate=False, deterministic=True)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(over[1:], nans))
    _compare("overwrite", over, want, _tols(t))
    for what, a, b in zip(NAMES, over, fresh):
        assert torch.equal(a, b), what


@pytest.mark.parametrize("name, dtype, coord_dtype", [("crafted", F32, None), ("m8_d32", F32, None), ("m8_d32", F16, F32)])
def test_deterministic_mode(name, dtype, coord_dtype):
    """With the flag grad_value is bit-identical between two calls; output and the packed gradient are with and without it,
    and equal between the two; without it grad_value is within tolerance."""
    t, shapes, P, want = _case(name, dtype, coord_dtype)
    dt = _dev(t)
    first = _native(dt, shapes, P, deterministic=True)
    second = _native(dt, shapes, P, deterministic=True)
    for what, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), "deterministic %s differs between two runs" % what
    plain = [_native(dt, shapes, P) for _ in range(2)]
    for i in (0, 2):
        assert torch.equal(plain[0][i], plain[1][i]) and torch.equal(plain[0][i], first[i]), NAMES[i]
    assert_close("unflagged grad_value", plain[0][1], want[1], TOL[dtype])
    _compare("deterministic", first, want, _tols(t))


def _guard(monkeypatch, touched, calls):
    """tests.util.guarded_run in the place of fda._run; it sizes the workspace through ``mdconv_workspace_bytes`` of the
    library handle, which for this operator's descriptor is ``mdconv_fda_workspace_bytes``."""
    from modulated_deform_conv_amd import _capi, fda
    real = _capi.lib()

    class Lib:
        mdconv_workspace_bytes = staticmethod(real.mdconv_fda_workspace_bytes)

        def __getattr__(self, name):
            return getattr(real, name)

    proxy = Lib()
    monkeypatch.setattr(_capi, "lib", lambda: proxy)
    monkeypatch.setattr(fda, "_run", guarded_run(touched, calls))


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (BF16, F32)])
def test_no_grad_value_under_the_guarded_workspace(monkeypatch, dtype, coord_dtype):
    """NO_GRAD_INPUT: grad_value NULL, no workspace (no lists, no statistics) between pattern-filled margins; the packed
    gradient is bit for bit that of the full call.  The full and the deterministic call run guarded as well, their
    workspace pattern-filled -- the list kernels read the statistics the coordinate kernel wrote, not zeros -- and the
    figure is exact."""
    t, shapes, P, want = _case("m8_d32", dtype, coord_dtype)
    dt = _dev(t)
    full = _native(dt, shapes, P)
    touched, calls = [], []
    _guard(monkeypatch, touched, calls)
    part = _native(dt, shapes, P, need_grad_value=False)
    again = _native(dt, shapes, P)
    det = _native(dt, shapes, P, deterministic=True)
    assert touched == [], touched
    sizes = [b for name, b in calls if name == "mdconv_fda_backward"]
    assert [b for name, b in calls if name == "mdconv_fda_forward"] == [0, 0, 0]
    assert sizes[0] == 0 < sizes[1] <= sizes[2], sizes
    assert part[1] is None
    for i in (0, 2):
        assert torch.equal(part[i], full[i]) and torch.equal(again[i], full[i]) and torch.equal(det[i], full[i]), NAMES[i]
    _compare("guarded full", again, want, _tols(t))
    _compare("guarded deterministic", det, want, _tols(t))


def test_selective_backward_through_autograd():
    """``value`` needs no gradient: the backward runs with NO_GRAD_INPUT and still returns the packed gradient; the packed
    tensor needs none: only grad_value comes back.  A tensor ``spatial_shapes`` and a host ``level_start_index`` are taken,
    a wrong one is refused, and so is an ``im2col_step`` that is no positive integer."""
    from modulated_deform_conv_amd import FlashDeformAttnFunction, flash_deform_attn
    t, shapes, P, want = _case("rect_levels", F32)
    value, loc_attn, go = _dev(t)
    la = loc_attn.clone().requires_grad_(True)
    out = FlashDeformAttnFunction.apply(value, torch.tensor(shapes), torch.tensor([0, 30, 39]), la, 64, P)
    out.backward(go)
    assert value.grad is None
    assert_close("selective output", out.detach(), want[0], 1e-4)
    assert_close("selective grad_sampling_loc_attn", la.grad, want[2], 1e-4)
    v = value.clone().requires_grad_(True)
    flash_deform_attn(v, shapes, loc_attn, P, [0, 30, 39]).backward(go)
    assert loc_attn.grad is None
    assert_close("selective grad_value", v.grad, want[1], 1e-4)
    with pytest.raises(ValueError):
        flash_deform_attn(value, shapes, la, P, [0, 30, 40])
    for step in (0, -1, 2.5, None):
        with pytest.raises(ValueError):
            FlashDeformAttnFunction.apply(value, shapes, None, la, step, P)
    # both through autograd
    v2, l2 = (x.detach().clone().requires_grad_(True) for x in (value, loc_attn))
    flash_deform_attn(v2, shapes, l2, P).backward(go)
    for what, a, b in zip(NAMES[1:], (v2.grad, l2.grad), want[1:]):
        assert_close("autograd %s" % what, a, b, 1e-4)


def test_graph_capture_and_two_replays():
    """Forward + deterministic backward into caller buffers, captured once: two replays equal the eager run bit for bit."""
    from modulated_deform_conv_amd import fda
    t, shapes, P, want = _case("m8_d32", F16, F32)
    value, loc_attn, go = dt = _dev(t)
    eager = _native(dt, shapes, P, deterministic=True)
    out = torch.empty_like(eager[0])
    bufs = (torch.empty_like(value), torch.empty_like(loc_attn))

    def step():
        fda.flash_deform_attn_forward(value, shapes, loc_attn, P, output=out)
        fda.flash_deform_attn_backward(value, shapes, loc_attn, P, go, grads=bufs, deterministic=True, accumulate=False)

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
        for b in (out,) + bufs:
            b.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for what, a, b in zip(NAMES, (out,) + bufs, eager):
            assert torch.equal(a, b), "graph replay: %s differs from the eager deterministic run" % what


def test_module_step_under_autocast():
    """One FlashDeformAttn step under torch.autocast(bfloat16), with a padding mask, against MSDeformAttn with the same
    parameters (a state_dict copy): output, input gradients and every parameter gradient at the bf16 tolerance.  The core
    receives a bf16 value and an fp32 packed tensor: the mixed call."""
    from modulated_deform_conv_amd import FlashDeformAttn, MSDeformAttn, flash_deform_attn
    torch.manual_seed(23)
    shapes = [(6, 5), (3, 3), (2, 2)]
    S, N, Lq, C = 43, 2, 7, 32
    theirs = MSDeformAttn(d_model=C, n_levels=3, n_heads=4, n_points=2).to(DEV)
    with torch.no_grad():   # offsets and logits that depend on the query
        theirs.sampling_offsets.weight.normal_(0, 0.05)
        theirs.attention_weights.weight.normal_(0, 0.2)
    ours = FlashDeformAttn(d_model=C, n_levels=3, n_heads=4, n_points=2).to(DEV)
    ours.load_state_dict(theirs.state_dict())
    seen = []

    def native_core(value, spatial_shapes, loc_attn, points, starts):
        seen.append((value.dtype, loc_attn.dtype, tuple(loc_attn.shape)))
        return flash_deform_attn(value, spatial_shapes, loc_attn, points, starts)

    ours._core = native_core
    query = torch.randn(N, Lq, C, device=DEV)
    flat = torch.randn(N, S, C, device=DEV)
    ref_pts = torch.rand(N, Lq, 3, 2, device=DEV) * 0.6 + 0.2
    pad = torch.zeros(N, S, dtype=torch.bool, device=DEV)
    pad[1, 25:30] = True
    go = torch.randn(N, Lq, C, device=DEV)
    results = []
    for mod in (ours, theirs):
        qi, fi, ri = (v.clone().requires_grad_(True) for v in (query, flat, ref_pts))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = mod(qi, ri, fi, shapes, [0, 30, 39], pad)
        assert y.dtype == torch.bfloat16
        y.backward(go.to(y.dtype))
        torch.cuda.synchronize()
        results.append(dict(output=y.detach(), grad_query=qi.grad, grad_input=fi.grad, grad_reference=ri.grad,
                            **{k: p.grad for k, p in mod.named_parameters()}))
    assert seen == [(BF16, F32, (N, Lq, 4, 3 * 3 * 2))]
    a, b = results
    assert all(v is not None for v in a.values())
    assert float(a["grad_input"][1, 25:30].abs().max()) == 0.0   # padded rows take no gradient
    for k in a:
        assert_close("module %s" % k, a[k], b[k], TOL[BF16])
