"""The DCNv4 operator with its in-kernel softmax on the GPU (include/mdconv.h, MDCONV_FLAG_SOFTMAX): output and the two
gradients against ``tests.dcnv4_softmax_ref`` -- the fp64 softmax of the logits the tensor holds, over all K taps of a
(pixel, group), then the fp64 reference of the operator -- at the project's tolerances: 1e-4 for fp32, ``TOL`` of
tests/test_gpu_hp.py for fp16 / bf16, by the value dtype for value-typed results and by the coordinate dtype for the packed
gradient.  The geometries are the small ones of tests/test_gpu_dcnv4.py::CASES, each the smallest at which its hazard
exists.  Beyond parity: gated-out taps (all of a pair, and some), the softmax's range, the packed gradient of the mixed call,
the zero sum of the logit gradients, equivalence with the composed route, the row padding on both sides, and the call modes
-- accumulate and overwrite, determinism, graph replay, NO_GRAD_INPUT under a guarded workspace, the lattice, the modules."""
import functools

import pytest
import torch

from tests import dcnv4_ref as R
from tests import dcnv4_softmax_ref as RS
from tests.test_gpu_dcnv4 import CASES
from tests.test_gpu_hp import TOL as TOL16
from tests.util import assert_close, guarded_run

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(TOL16)
TOL[torch.float32] = 1e-4
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NAMES = ("output", "grad_input", "grad_offset_mask")


def _gk(name):
    kw = CASES[name]
    return kw["G"], R.taps(kw["kernel"], kw.get("remove_center", False))


@functools.lru_cache(maxsize=None)
def _case(name, dtype, coord_dtype=None, variant="", shift=0.0):
    """CPU inputs of a case and its fp64 reference (output, grad_input, grad_offset_mask), computed once and left
    unchanged.  The masks of ``make_inputs`` -- N(0, 1) -- are the logits.  Variants: ``nan`` (NaN in the padding columns),
    ``two_out`` (crafted: taps 0 and 4 of every pixel pushed out of the image), ``one_hot`` (one pair with the logits
    +40, -40, ...)."""
    kw = dict(CASES[name])
    G, K = _gk(name)
    x, om, go, geo = R.make_inputs(dtype=dtype, coord_dtype=coord_dtype, seed=len(name) + 7, nan_padding=variant == "nan", **kw)
    if name in ("crafted", "far"):
        off, m = R.unpack(om, G, K)
        if name == "crafted":
            # loc = wo + i - 1 + off_x (3x3, pad 1, scale 1): aim every tap of every pixel at (1.3, 1.4)
            loc_h, loc_w = R.positions(torch.zeros_like(off), 4, 4, *geo[:4], 1, 1.0)
            off = torch.stack([1.3 - loc_w, 1.4 - loc_h], -1).reshape(off.shape).to(om.dtype)
            if variant == "two_out":
                off = off.reshape(off.shape[:3] + (K, 2)).clone()
                off[..., 0, :] += 30.0
                off[..., 4, :] -= 30.0
                off = off.reshape(om.shape[:3] + (-1,))
        else:
            flip = torch.where(torch.rand(off.shape, generator=torch.Generator().manual_seed(5)) < 0.5, -20.0, 20.0)
            off = (off + flip).to(om.dtype)
        om = R.pack(off, m, G, K)
    if shift:
        om = RS.shift_logits(om, G, K, shift)
    if variant == "one_hot":
        om[0, 0, 0, 2 * K:3 * K] = -40.0
        om[0, 0, 0, 2 * K] = 40.0
    if name != "far" and variant != "two_out":
        assert R.min_lattice_distance(om, x.shape[1], x.shape[2], *geo[:4], geo[4], geo[6], geo[7]) >= R.MARGIN
    return (x, om, go), geo, RS.dcnv4_softmax_ref_grads(x, om, go, *geo)


def _native(t, geo, grads=None, need_grad_input=True, deterministic=False, accumulate=None, softmax=True):
    from modulated_deform_conv_amd import dcnv4
    x, om, go = t
    out = dcnv4.dcnv4_forward(x, om, *geo, softmax=softmax)
    g = dcnv4.dcnv4_backward(x, om, go, *geo, grads=grads, need_grad_input=need_grad_input, deterministic=deterministic,
                             accumulate=accumulate, softmax=softmax)
    torch.cuda.synchronize()
    return (out,) + tuple(g)


def _dev(t):
    return tuple(v.to(DEV) for v in t)


def _tols(t):
    """Per result: value-typed results by the value dtype, the gradient of offset_mask by the coordinate dtype."""
    return (TOL[t[0].dtype], TOL[t[0].dtype], TOL[t[1].dtype])


def _compare(tag, got, want, tols):
    for what, a, b, tol in zip(NAMES, got, want, tols):
        if a is None:
            continue
        print("%s %s: max |want| %.3e" % (tag, what, float(b.abs().max())))
        assert_close("%s %s" % (tag, what), a, b, tol)


PARITY = [
    ("one_lane", F32, None),                                                          # VL = 1, K = 9: the lane's own loop over taps
    ("g2_d32_rc", F32, None), ("g2_d32_rc", BF16, None), ("g2_d32_rc", F16, F32),     # K = 8 = VL, remove_center
    ("d64_1x1", BF16, None),                                                          # K = 1 < VL
    ("three_vectors", F32, None),                                                     # an idle lane in the butterflies
    ("two_rounds", F32, None), ("two_rounds_16bit", F16, None),                       # statistics across lane rounds
    ("g4_d16", F32, None), ("g4_d16", F16, None), ("g4_d16", BF16, None), ("g4_d16", BF16, F32),   # group stride 27 in 112
    ("rect_rc", F32, None), ("rect_rc", F16, F32),                                    # K = 14, tap-to-grid mapping
]


@pytest.mark.parametrize("name, dtype, coord_dtype", PARITY)
def test_against_reference(name, dtype, coord_dtype):
    t, geo, want = _case(name, dtype, coord_dtype)
    G, K = _gk(name)
    assert t[1].dtype == (coord_dtype or dtype)
    got = _native(_dev(t), geo)
    assert got[0].dtype == got[1].dtype == dtype and got[2].dtype == t[1].dtype
    _compare("%s %s/%s" % (name, dtype, coord_dtype), got, want, _tols(t))
    if K == 1:
        # the weight is exactly 1 -- the output is the plain operator's with masks of one -- and the logit gradient exactly 0
        glogit = R.unpack(got[2].cpu(), G, K)[1]
        assert float(glogit.float().abs().max()) == 0.0 and float(R.unpack(want[2], G, K)[1].abs().max()) == 0.0
        off, m = R.unpack(t[1], G, K)
        ones = _native(_dev((t[0], R.pack(off, torch.ones_like(m), G, K), t[2])), geo, softmax=False)
        assert torch.equal(ones[0], got[0])


def test_every_tap_gated_out():
    """Offsets of +-20 px: nothing is read; the weights still sum to one, S = 0, and the output and every gradient -- the
    logits' -a S included -- are exactly zero."""
    t, geo, want = _case("far", F32)
    assert all(float(w.abs().max()) == 0.0 for w in want)
    for det in (False, True):
        got = _native(_dev(t), geo, grads=tuple(torch.full_like(v, float("nan")) for v in _dev(t)[:2]), accumulate=False,
                      deterministic=det)
        assert all(float(g.abs().max()) == 0.0 for g in got)


def test_some_taps_gated_out():
    """crafted with taps 0 and 4 of every pixel out of the image: their logits count in the normaliser, their logit
    gradients are the reference's -a S and not zero, their offset gradients exactly zero."""
    t, geo, want = _case("crafted", F32, None, "two_out")
    G, K = _gk("crafted")
    gate = R.gate_of(t[1], 4, 4, *geo[:4], G, geo[6], geo[7])   # [B, Ho, Wo, G, K]
    assert not gate[..., 0].any() and not gate[..., 4].any() and gate[..., [1, 2, 3, 5, 6, 7, 8]].all()
    got = _native(_dev(t), geo, deterministic=True)
    _compare("two taps out", got, want, _tols(t))
    goff, glogit = (v.reshape(gate.shape + s) for v, s in zip(R.unpack(got[2].cpu(), G, K), ((2,), ())))
    wlogit = R.unpack(want[2], G, K)[1].reshape(gate.shape)
    x, om, go = t
    a = torch.softmax(R.unpack(om.double(), G, K)[1].reshape(gate.shape), -1)
    S = (go.double() * want[0]).sum(-1).reshape(gate.shape[:3] + (1, 1))
    assert_close("reference -a S", wlogit[~gate], (-a * S).expand(gate.shape)[~gate], 1e-12)
    assert float(wlogit[~gate].abs().min()) > 0 and float(glogit[~gate].abs().min()) > 0
    assert_close("gated-out logit gradients", glogit[~gate], wlogit[~gate], 1e-4)
    assert float(goff[~gate].abs().max()) == 0.0


@pytest.mark.parametrize("name, dtype, shift", [("g2_d32_rc", F32, 90.0), ("g4_d16", F32, 90.0), ("g2_d32_rc", F16, 1000.0),
                                                ("g4_d16", F16, 1000.0)])
def test_softmax_range(name, dtype, shift):
    """Logits around +90 in fp32 and around +1000 in fp16: exp of either overflows fp32 (e^88.8 is its largest finite
    value), so a softmax without the maximum subtracted returns inf / inf there."""
    t, geo, want = _case(name, dtype, None, "", shift)
    logits = R.unpack(t[1], *_gk(name))[1]
    assert float(logits.float().exp().max()) == float("inf") and torch.isfinite(logits.float()).all()
    _compare("range %s %s" % (name, dtype), _native(_dev(t), geo), want, _tols(t))


def test_nearly_one_hot_pair():
    """One (pixel, group) with logits (+40, -40, ..., -40): the other weights are e^-80, far below fp32's epsilon beside 1
    and still normal numbers; every result stays finite and at tolerance."""
    t, geo, want = _case("g4_d16", F32, None, "one_hot")
    K = _gk("g4_d16")[1]
    got = _native(_dev(t), geo)
    _compare("one-hot", got, want, _tols(t))
    pair = got[2][0, 0, 0, :3 * K].double().cpu()
    assert torch.isfinite(pair).all()
    assert float(pair[2 * K + 1:].abs().max()) < 1e-30 and float(pair[2:2 * K].abs().max()) < 1e-30


def test_mixed_dtype_packed_gradient_at_fp32_tolerance():
    """bf16 values beside an fp32 packed tensor: the packed gradient is an fp32 result and holds 1e-4 -- the pair sum S is
    taken from the fp32 sums of the call, not from the stored bf16 output."""
    t, geo, want = _case("g4_d16", BF16, F32)
    G, K = _gk("g4_d16")
    got = _native(_dev(t), geo)
    assert got[0].dtype == BF16 and got[2].dtype == F32
    print("mixed: max |grad_offset_mask| %.3e" % float(want[2].abs().max()))
    assert_close("mixed grad_offset_mask", got[2], want[2], 1e-4)
    assert_close("mixed logit gradients", R.unpack(got[2], G, K)[1], R.unpack(want[2], G, K)[1], 1e-4)


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (BF16, F32), (F16, F32)])
def test_logit_gradients_sum_to_zero(dtype, coord_dtype):
    """sum_t a[t] (g[t] - S) = S - S: per (pixel, group) the logit gradients sum to zero, within the coordinate tolerance
    times the largest logit gradient -- 1e-4 for the fp32 packed gradient of all three value dtypes.  (What stands against
    it: the K = 9 stored values are rounded once each, at most 2^-24 of the largest, and the fp32 sums g[t] and S carry a
    few 1e-7 of the largest |g|.  A 16-bit packed gradient is left out: 9 roundings of 2^-11 / 2^-8 of the largest could
    add up to more than that dtype's tolerance, so the bound would be no property of the operator there.)"""
    t, geo, want = _case("g4_d16", dtype, coord_dtype)
    G, K = _gk("g4_d16")
    got = _native(_dev(t), geo)
    assert got[2].dtype == F32
    glogit = R.unpack(got[2].double().cpu(), G, K)[1].reshape(got[2].shape[:3] + (G, K))
    largest = float(glogit.abs().max())
    worst = float(glogit.sum(-1).abs().max())
    print("zero sum %s/%s: largest logit gradient %.3e, worst pair sum %.3e" % (dtype, coord_dtype, largest, worst))
    assert largest > 0 and worst <= TOL[F32] * largest


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (BF16, F32)])
def test_equals_the_composed_route(dtype, coord_dtype):
    """The native call against the composed route on the GPU: the mask columns of the same packed tensor sliced,
    ``torch.softmax``, repacked, ``dcnv4_core`` without the flag, autograd through the lot."""
    from modulated_deform_conv_amd import dcnv4_core
    t, geo, want = _case("g4_d16", dtype, coord_dtype)
    G, K = _gk("g4_d16")
    x, om, go = _dev(t)
    B, Ho, Wo, _ = om.shape
    results = []
    for route in ("native", "composed"):
        xi, omi = x.clone().requires_grad_(True), om.clone().requires_grad_(True)
        if route == "native":
            out = dcnv4_core(xi, omi, *geo, softmax=True)
        else:
            off, logits = R.unpack(omi, G, K)
            m = torch.softmax(logits.reshape(B, Ho, Wo, G, K), -1).reshape(B, Ho, Wo, G * K)
            out = dcnv4_core(xi, R.pack(off, m, G, K), *geo)
        out.backward(go)
        torch.cuda.synchronize()
        results.append((out.detach(), xi.grad, omi.grad))
    native, composed = results
    for what, a, b, tol in zip(NAMES, native, composed, _tols(t)):
        assert a.dtype == b.dtype
        assert_close("equivalence %s" % what, a, b, tol)
    _compare("equivalence native", native, want, _tols(t))


@pytest.mark.parametrize("name, dtype, coord_dtype", [("one_lane", F32, None), ("g4_d16", BF16, None), ("rect_rc", F16, F32)])
def test_nan_in_the_padding_of_offset_mask_is_never_read(name, dtype, coord_dtype):
    """The padding columns of offset_mask hold NaN -- right behind the last group's logits: every result is finite and
    equals the reference (whose gradient of the padding is zero)."""
    t, geo, want = _case(name, dtype, coord_dtype, "nan")
    G, K = _gk(name)
    used = G * K * 3
    assert t[1].shape[-1] > used and torch.isnan(t[1][..., used:]).all() and torch.isfinite(t[1][..., :used]).all()
    for det in (False, True):
        got = _native(_dev(t), geo, deterministic=det)
        assert all(torch.isfinite(g.float()).all() for g in got)
        _compare("nan padding %s det=%d" % (name, det), got, want, _tols(t))


@pytest.mark.parametrize("name, dtype, coord_dtype", [("one_lane", F32, None), ("g4_d16", F16, None), ("rect_rc", BF16, F32),
                                                      ("d64_1x1", BF16, None)])
def test_padding_of_grad_offset_mask(name, dtype, coord_dtype):
    """Overwrite mode into NaN-prefilled buffers: exact zeros in the padding columns of grad_offset_mask (and no NaN left
    anywhere).  Accumulate mode: the padding columns of the caller's buffer are left bit for bit."""
    t, geo, want = _case(name, dtype, coord_dtype)
    x, om, go = _dev(t)
    G, K = _gk(name)
    used = G * K * 3
    assert om.shape[-1] > used
    bufs = (torch.full_like(x, float("nan")), torch.full_like(om, float("nan")))
    got = _native((x, om, go), geo, grads=bufs, accumulate=False)
    assert got[2].data_ptr() == bufs[1].data_ptr()
    assert torch.equal(got[2][..., used:], torch.zeros_like(got[2][..., used:]))
    _compare("overwrite into NaN %s" % name, got, want, _tols(t))
    # accumulate: a bit pattern (NaN with a payload among it) in the padding, zeros in the used columns
    bits = torch.int32 if om.dtype == F32 else torch.int16
    pattern = torch.randint(-2 ** 15, 2 ** 15 - 1, om.shape, generator=torch.Generator().manual_seed(3)).to(bits)
    pattern[..., used:][..., 0] = -1   # all ones: a NaN
    base = pattern.view(om.dtype).clone()
    base[..., :used] = 0
    before = base.view(bits).clone()
    acc = (torch.zeros_like(x), base.to(DEV))
    got = _native((x, om, go), geo, grads=acc)
    after = got[2].cpu().view(bits)
    assert torch.equal(after[..., used:], before[..., used:])
    assert_close("accumulate onto zeros %s" % name, got[2][..., :used], want[2][..., :used], _tols(t)[2])


def test_accumulate_against_overwrite():
    """The two gradients added to non-zero buffers, fp16: buffer + gradient, rounded once; overwrite mode ignores what the
    buffers hold."""
    dtype = F16
    t, geo, want = _case("g4_d16", dtype)
    x, om, go = _dev(t)
    gen = torch.Generator().manual_seed(9)
    base = tuple(torch.randn(v.shape, generator=gen).to(dtype) for v in (x, om))
    bufs = tuple(b.to(DEV) for b in base)
    got = _native((x, om, go), geo, grads=bufs)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got[1:], bufs))
    for what, a, b, w in zip(NAMES[1:], got[1:], base, want[1:]):
        assert_close("accumulate %s" % what, a, b.double() + w, TOL[dtype])
    fresh = _native((x, om, go), geo, deterministic=True)
    over = _native((x, om, go), geo, grads=bufs, accumulate=False, deterministic=True)
    _compare("overwrite", over, want, _tols(t))
    for what, a, b in zip(NAMES, over, fresh):
        assert torch.equal(a, b), what


@pytest.mark.parametrize("name, dtype, coord_dtype", [("crafted", F32, None), ("g4_d16", F32, None), ("g4_d16", F16, None),
                                                      ("rect_rc", BF16, F32)])
def test_deterministic_mode(name, dtype, coord_dtype):
    """With the flag all three results are bit-identical between two eager runs and a run replayed from a HIP graph;
    without it the output and grad_offset_mask are as well."""
    from modulated_deform_conv_amd import dcnv4
    t, geo, want = _case(name, dtype, coord_dtype)
    x, om, go = _dev(t)
    first = _native((x, om, go), geo, deterministic=True)
    second = _native((x, om, go), geo, deterministic=True)
    for what, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), "deterministic %s differs between two runs" % what
    plain = [_native((x, om, go), geo) for _ in range(2)]
    for i in (0, 2):
        assert torch.equal(plain[0][i], plain[1][i]) and torch.equal(plain[0][i], first[i]), NAMES[i]
    assert_close("unflagged grad_input", plain[0][1], want[1], TOL[dtype])
    _compare("deterministic", first, want, _tols(t))

    out = torch.empty_like(first[0])
    bufs = tuple(torch.empty_like(v) for v in (x, om))

    def step():
        dcnv4.dcnv4_forward(x, om, *geo, output=out, softmax=True)
        dcnv4.dcnv4_backward(x, om, go, *geo, grads=bufs, deterministic=True, accumulate=False, softmax=True)

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
        for what, a, b in zip(NAMES, (out,) + bufs, first):
            assert torch.equal(a, b), "graph replay: %s differs from the eager deterministic run" % what


def _guard(monkeypatch, touched, calls):
    """tests.util.guarded_run in the place of dcnv4._run; it sizes the workspace through ``mdconv_workspace_bytes`` of the
    library handle, which for this operator's descriptor is ``mdconv_dcnv4_workspace_bytes``."""
    from modulated_deform_conv_amd import _capi, dcnv4
    real = _capi.lib()

    class Lib:
        mdconv_workspace_bytes = staticmethod(real.mdconv_dcnv4_workspace_bytes)

        def __getattr__(self, name):
            return getattr(real, name)

    proxy = Lib()
    monkeypatch.setattr(_capi, "lib", lambda: proxy)
    monkeypatch.setattr(dcnv4, "_run", guarded_run(touched, calls))


@pytest.mark.parametrize("dtype, coord_dtype", [(F32, None), (BF16, None), (BF16, F32)])
def test_no_grad_input_under_the_guarded_workspace(monkeypatch, dtype, coord_dtype):
    """NO_GRAD_INPUT: grad_input NULL, no workspace (no lists, no statistics) between pattern-filled margins;
    grad_offset_mask is bit for bit that of the full call.  The full and the deterministic call run guarded as well, their
    workspace pattern-filled -- the list kernels read the statistics the coordinate kernel wrote, not zeros -- and the
    figure is exact: the unflagged one plus 8 bytes per (pixel, group), rounded up to 256."""
    t, geo, want = _case("g4_d16", dtype, coord_dtype)
    G, K = _gk("g4_d16")
    dt = _dev(t)
    full = _native(dt, geo)
    touched, calls = [], []
    _guard(monkeypatch, touched, calls)
    _native(dt, geo, softmax=False)
    _native(dt, geo, softmax=False, deterministic=True)
    unflagged = [b for name, b in calls if name == "mdconv_dcnv4_backward"]
    del calls[:]
    part = _native(dt, geo, need_grad_input=False)
    again = _native(dt, geo)
    det = _native(dt, geo, deterministic=True)
    assert touched == [], touched
    sizes = [b for name, b in calls if name == "mdconv_dcnv4_backward"]
    assert [b for name, b in calls if name == "mdconv_dcnv4_forward"] == [0, 0, 0]
    B, Ho, Wo, _ = t[1].shape
    stats = (8 * B * Ho * Wo * G + 255) // 256 * 256
    assert sizes == [0, unflagged[0] + stats, unflagged[1] + stats] and unflagged[0] > 0, (sizes, unflagged, stats)
    assert part[1] is None
    for i in (0, 2):
        assert torch.equal(part[i], full[i]) and torch.equal(again[i], full[i]) and torch.equal(det[i], full[i]), NAMES[i]
    _compare("guarded full", again, want, _tols(t))
    _compare("guarded deterministic", det, want, _tols(t))


@functools.lru_cache(maxsize=None)
def _lattice_case():
    x, om, go, geo = R.make_lattice_inputs("integer", dtype=F32, seed=9, **CASES["g4_d16"])
    return (x, om, go), geo, RS.dcnv4_softmax_ref_grads(x, om, go, *geo)


def test_on_the_lattice():
    """Sampling positions on whole pixels, with the flag: the right-sided derivative of the cell floor(loc) (the
    reference's floor is detached), offset gradients of exactly zero outside the gate, and there the logit gradient -a S."""
    t, geo, want = _lattice_case()
    G, K = _gk("g4_d16")
    x, om, go = t
    assert R.min_lattice_distance(om, x.shape[1], x.shape[2], *geo[:4], geo[4], geo[6], geo[7]) == 0.0
    dt = _dev(t)
    got = _native(dt, geo, grads=tuple(torch.full_like(v, float("nan")) for v in dt[:2]), accumulate=False, deterministic=True)
    _compare("lattice", got, want, _tols(t))
    out_of_gate = ~R.gate_of(om, x.shape[1], x.shape[2], *geo[:4], G, geo[6], geo[7])
    assert out_of_gate.any()
    goff, glogit = R.unpack(got[2].cpu(), G, K)
    assert float(goff.reshape(out_of_gate.shape + (2,))[out_of_gate].abs().max()) == 0.0
    wl = R.unpack(want[2], G, K)[1].reshape(out_of_gate.shape)
    assert float(wl[out_of_gate].abs().max()) > 0
    assert_close("lattice gated-out logit gradients", glogit.reshape(out_of_gate.shape)[out_of_gate], wl[out_of_gate], 1e-4)


def test_dcnv4_module_step_under_autocast():
    """The DCNv4 module with ``softmax=True`` under torch.autocast(bfloat16) against the same module with the core swapped
    for the reference: output, input gradient and every parameter gradient."""
    from modulated_deform_conv_amd import DCNv4
    torch.manual_seed(21)
    mod = DCNv4(channels=32, kernel_size=3, group=4, offset_scale=1.0, dw_kernel_size=3, remove_center=True, softmax=True).to(DEV)
    with torch.no_grad():   # offsets away from the lattice, logits that differ
        mod.offset_mask.weight.normal_(0, 0.01)
        mod.offset_mask.bias.uniform_(0.3, 0.7)
        K = 8
        for g in range(4):
            mod.offset_mask.bias[g * 3 * K + 2 * K:(g + 1) * 3 * K].normal_(0, 1.0)
    x = torch.randn(2, 6 * 5, 32, device=DEV)
    go = torch.randn(2, 6 * 5, 32, device=DEV)
    results = []
    seen = []

    def native(*a, **k):
        from modulated_deform_conv_amd import dcnv4_core
        seen.append(k)
        return dcnv4_core(*a, **k)

    for core in (native, RS.dcnv4_softmax_ref):
        mod._core = core
        mod.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=BF16):
            y = mod(xi, shape=(6, 5))
        assert y.dtype == BF16 and y.shape == x.shape
        y.backward(go.to(y.dtype))
        torch.cuda.synchronize()
        results.append(dict(output=y.detach(), grad_x=xi.grad, **{k: p.grad for k, p in mod.named_parameters()}))
    assert seen == [dict(softmax=True)]
    native_r, ref = results
    assert all(v is not None for v in native_r.values()) and len(native_r) == 10
    for k in native_r:
        assert_close("module %s" % k, native_r[k], ref[k], TOL[BF16])


def test_dcnv3_fused_against_dcnv3():
    """DCNv3Fused, loaded from a DCNv3 state dict with non-zero offset / mask parameters, against DCNv3 in fp32: the
    output, the input gradient and every parameter gradient at 1e-4.  The core receives one packed tensor and the flag."""
    from modulated_deform_conv_amd import DCNv3, DCNv3Fused, dcnv4_core
    from modulated_deform_conv_amd.dcnv4 import offset_mask_len
    torch.manual_seed(31)
    kw = dict(channels=32, kernel_size=3, group=4, offset_scale=1.0)
    theirs = DCNv3(**kw).to(DEV)
    with torch.no_grad():   # offsets away from the lattice that depend on the pixel, logits that differ
        theirs.offset.weight.normal_(0, 0.02)
        theirs.offset.bias.uniform_(0.3, 0.7)
        theirs.mask.weight.normal_(0, 0.3)
        theirs.mask.bias.normal_(0, 1.0)
    ours = DCNv3Fused(**kw).to(DEV)
    ours.load_state_dict(theirs.state_dict())
    seen = []

    def native_core(x, om, *geo, **k):
        seen.append((x.dtype, om.dtype, tuple(om.shape), geo[-1], k))
        return dcnv4_core(x, om, *geo, **k)

    ours._core = native_core
    x = torch.randn(2, 6, 5, 32, device=DEV)
    go = torch.randn(2, 6, 5, 32, device=DEV)
    results = []
    for mod in (ours, theirs):
        xi = x.clone().requires_grad_(True)
        y = mod(xi)
        y.backward(go)
        torch.cuda.synchronize()
        results.append(dict(output=y.detach(), grad_input=xi.grad, **{k: p.grad for k, p in mod.named_parameters()}))
    assert seen == [(F32, F32, (2, 6, 5, offset_mask_len(3, 4)), False, dict(softmax=True))]
    a, b = results
    assert list(a) == list(b) and all(v is not None for v in a.values())
    assert all(float(b[k].abs().max()) > 0 for k in ("offset.weight", "offset.bias", "mask.weight", "mask.bias"))
    for k in a:
        print("fused %s: max |want| %.3e" % (k, float(b[k].abs().max())))
        assert_close("fused %s" % k, a[k], b[k], 1e-4)


def test_input_without_gradient():
    """The input needs no gradient: the backward runs with NO_GRAD_INPUT and still returns the packed gradient, in fp32
    beside fp16 values; the published 15-argument call still runs (without the softmax)."""
    from modulated_deform_conv_amd import DCNv4Function, dcnv4_core
    t, geo, want = _case("g4_d16", F16, F32)
    xs, om, go = _dev(t)
    om.requires_grad_(True)
    dcnv4_core(xs, om, *geo, softmax=True).backward(go)
    assert xs.grad is None and om.grad.dtype == F32
    assert_close("selective grad_offset_mask", om.grad, want[2], 1e-4)
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = geo[:4]
    plain = DCNv4Function.apply(xs, om.detach(), kh, kw, sh, sw, ph, pw, dh, dw, geo[4], geo[5], geo[6], 256, geo[7])
    flagged = DCNv4Function.apply(xs, om.detach(), kh, kw, sh, sw, ph, pw, dh, dw, geo[4], geo[5], geo[6], 256, geo[7], True)
    assert_close("16-argument call", flagged, want[0], TOL[F16])
    assert not torch.equal(plain, flagged)
