"""The DCNv4 operator on the GPU (include/mdconv.h, "DCNv4 operator"): output and the two gradients against
``tests.dcnv4_ref.dcnv4_ref`` evaluated in fp64 from the inputs as the kernel sees them (16-bit inputs rounded first), at the
project's tolerances by the dtype of each result -- 1e-4 for fp32, ``TOL`` of tests/test_gpu_hp.py for fp16 / bf16, the
gradient of ``offset_mask`` by the coordinate dtype -- on the smallest shapes at which each part can go wrong, plus the row
padding on both sides, and the call modes: accumulate, NO_GRAD_INPUT under a guarded workspace, determinism, graph replay,
and the module under autocast.  No element is excluded anywhere; the lattice margin is a rule for the inputs, asserted."""
import functools

import pytest
import torch

from tests import dcnv4_ref as R
from tests.test_gpu_hp import TOL as TOL16
from tests.util import assert_close, guarded_run

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(TOL16)
TOL[torch.float32] = 1e-4
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16

CASES = {
    # VL = 1; OM 32 with 5 padding columns; odd extents; border corners
    "one_lane": dict(B=1, G=1, D=4, H=5, W=7, kernel=3, pad=1),
    # the tap -> grid mapping on a non-square kernel (a swap of i and j, or of x and y, fails only here); K = 14, OM 128
    "rect_rc": dict(B=2, G=3, D=8, H=6, W=5, kernel=(5, 3), stride=2, pad=(2, 1), dilation=2, offset_scale=0.5, remove_center=True),
    # fp32: VL 4, tap rounds 4 + 4 + 1; group stride 27 inside a row of 112
    "g4_d16": dict(B=2, G=4, D=16, H=9, W=8, kernel=3, pad=1),
    # K = 8 = VL in fp32; OM 48 with no padding
    "g2_d32_rc": dict(B=1, G=2, D=32, H=5, W=4, kernel=3, pad=1, remove_center=True),
    # K = 1 < VL; OM 8
    "d64_1x1": dict(B=1, G=2, D=64, H=4, W=4, kernel=1, offset_scale=2.0),
    # three vectors per group in four lanes: an idle lane in the butterfly
    "three_vectors": dict(B=1, G=2, D=12, H=5, W=4, kernel=3, pad=1),
    # 65 vectors: 64 lanes, two rounds
    "two_rounds": dict(B=1, G=1, D=260, H=3, W=4, kernel=3, pad=1),
    "two_rounds_16bit": dict(B=1, G=1, D=520, H=3, W=4, kernel=3, pad=1),
    # one long list per corner pixel: every sample lands between input pixels (1, 1) and (2, 2)
    "crafted": dict(B=2, G=1, D=4, H=4, W=4, kernel=3, pad=1),
    "far": dict(B=1, G=2, D=4, H=8, W=8, kernel=3, pad=1),
}


def _unpacked(om, kw):
    G, K = kw["G"], R.taps(kw["kernel"], kw.get("remove_center", False))
    return R.unpack(om, G, K) + (G, K)


@functools.lru_cache(maxsize=None)
def _case(name, dtype, coord_dtype=None, variant=""):
    """CPU inputs of a case and its fp64 reference (output, grad_input, grad_offset_mask), computed once."""
    kw = dict(CASES[name])
    x, om, go, geo = R.make_inputs(dtype=dtype, coord_dtype=coord_dtype, seed=len(name) + 7, nan_padding=variant == "nan", **kw)
    if name in ("crafted", "far"):
        off, m, G, K = _unpacked(om, kw)
        if name == "crafted":
            # loc = wo + i - 1 + off_x (3x3, pad 1, scale 1): aim every tap of every pixel at (1.3, 1.4)
            loc_h, loc_w = R.positions(torch.zeros_like(off), 4, 4, *geo[:4], 1, 1.0)
            off = torch.stack([1.3 - loc_w, 1.4 - loc_h], -1).reshape(off.shape).to(om.dtype)
        else:
            shift = torch.where(torch.rand(off.shape, generator=torch.Generator().manual_seed(5)) < 0.5, -20.0, 20.0)
            off = (off + shift).to(om.dtype)
        om = R.pack(off, m, G, K)
    if name != "far":
        assert R.min_lattice_distance(om, x.shape[1], x.shape[2], *geo[:4], geo[4], geo[6], geo[7]) >= R.MARGIN
    return (x, om, go), geo, R.dcnv4_ref_grads(x, om, go, *geo)


def _native(t, geo, grads=None, need_grad_input=True, deterministic=False, accumulate=None):
    from modulated_deform_conv_amd import dcnv4
    x, om, go = t
    out = dcnv4.dcnv4_forward(x, om, *geo)
    g = dcnv4.dcnv4_backward(x, om, go, *geo, grads=grads, need_grad_input=need_grad_input, deterministic=deterministic,
                             accumulate=accumulate)
    torch.cuda.synchronize()
    return (out,) + tuple(g)


def _dev(t):
    return tuple(v.to(DEV) for v in t)


NAMES = ("output", "grad_input", "grad_offset_mask")


def _tols(t):
    """Per result: value-typed results by the value dtype, the gradient of offset_mask by the coordinate dtype."""
    return (TOL[t[0].dtype], TOL[t[0].dtype], TOL[t[1].dtype])


def _compare(tag, got, want, tols):
    for what, a, b, tol in zip(NAMES, got, want, tols):
        if a is None:
            continue
        print("%s %s: max |want| %.3e" % (tag, what, float(b.abs().max())))
        assert_close("%s %s" % (tag, what), a, b, tol)


@pytest.mark.parametrize("name, dtype, coord_dtype", [
    ("one_lane", F32, None), ("rect_rc", F32, None), ("rect_rc", F16, None), ("rect_rc", F16, F32), ("g4_d16", F32, None),
    ("g4_d16", F16, None), ("g4_d16", BF16, None), ("g4_d16", BF16, F32), ("g2_d32_rc", F32, None), ("g2_d32_rc", BF16, None),
    ("d64_1x1", BF16, None), ("d64_1x1", F16, F32), ("three_vectors", F32, None), ("g2_d32_rc", F16, F32),
    ("two_rounds", F32, None), ("two_rounds_16bit", F16, None), ("crafted", F32, None),
])
def test_against_reference(name, dtype, coord_dtype):
    t, geo, want = _case(name, dtype, coord_dtype)
    assert t[1].dtype == (coord_dtype or dtype) and float(t[1].min()) < 0 and float(t[1].max()) > 1   # no softmax assumed
    got = _native(_dev(t), geo)
    assert got[2].dtype == t[1].dtype and got[1].dtype == dtype
    _compare("%s %s/%s" % (name, dtype, coord_dtype), got, want, _tols(t))


def test_samples_wholly_outside():
    """Offsets of +-20 px: nothing is read, the output and every gradient are exactly zero, the lists are empty."""
    t, geo, want = _case("far", F32)
    assert all(float(w.abs().max()) == 0.0 for w in want)
    got = _native(_dev(t), geo)
    assert all(float(g.abs().max()) == 0.0 for g in got)


@pytest.mark.parametrize("name, dtype, coord_dtype", [("one_lane", F32, None), ("g4_d16", BF16, None), ("rect_rc", F16, F32)])
def test_nan_in_the_padding_of_offset_mask_is_never_read(name, dtype, coord_dtype):
    """The padding columns of offset_mask hold NaN: every result is finite and equals the reference (whose gradient of
    the padding is zero); the used columns are those of the plain case."""
    t, geo, want = _case(name, dtype, coord_dtype, "nan")
    used = CASES[name]["G"] * R.taps(CASES[name]["kernel"], CASES[name].get("remove_center", False)) * 3
    assert t[1].shape[-1] > used and torch.isnan(t[1][..., used:]).all() and torch.isfinite(t[1][..., :used]).all()
    got = _native(_dev(t), geo)
    assert all(torch.isfinite(g.float()).all() for g in got)
    _compare("nan padding %s" % name, got, want, _tols(t))
    got_det = _native(_dev(t), geo, deterministic=True)
    _compare("nan padding, deterministic %s" % name, got_det, want, _tols(t))


@pytest.mark.parametrize("name, dtype, coord_dtype", [("one_lane", F32, None), ("g4_d16", F16, None), ("rect_rc", BF16, F32),
                                                      ("d64_1x1", BF16, None)])
def test_padding_of_grad_offset_mask(name, dtype, coord_dtype):
    """Overwrite mode into NaN-prefilled buffers: exact zeros in the padding columns of grad_offset_mask (and no NaN left
    anywhere).  Accumulate mode: the padding columns of the caller's buffer are left bit for bit."""
    t, geo, want = _case(name, dtype, coord_dtype)
    x, om, go = _dev(t)
    used = CASES[name]["G"] * R.taps(CASES[name]["kernel"], CASES[name].get("remove_center", False)) * 3
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


def test_shape_checks_name_the_row_length():
    """A DCNv3-style row (G*K*3 = 108 elements, unpadded) is refused by name, and so is a 16-bit offset_mask of another type."""
    from modulated_deform_conv_amd import dcnv4
    t, geo, _ = _case("g4_d16", F32)
    x, om, go = _dev(t)
    with pytest.raises(ValueError, match="OM = 112"):
        dcnv4.dcnv4_forward(x, om[..., :108].contiguous(), *geo)
    with pytest.raises(ValueError, match="OM = 112"):
        dcnv4.dcnv4_backward(x, om[..., :108].contiguous(), go, *geo)
    with pytest.raises(ValueError, match="float32"):
        dcnv4.dcnv4_forward(x.to(F16), om.to(BF16), *geo)
    with pytest.raises(ValueError, match="contiguous"):
        dcnv4.dcnv4_forward(x, torch.cat([om, om], -1)[..., :112], *geo)


def test_forward_at_integer_positions():
    """Corner weights exactly 0 / 1 and the loc < size edge.  Forward only; the backward on the lattice -- the right-sided
    derivative, exact zeros outside the gate -- is tests/test_gpu_lattice.py."""
    from modulated_deform_conv_amd import dcnv4
    for name in ("one_lane", "rect_rc"):
        kw = dict(CASES[name])
        kw["offset_scale"] = 1.0 if name == "one_lane" else 2.0   # (integer positions need an integer scale)
        x, om, go, geo = R.make_inputs(dtype=F32, seed=3, integer_offsets=True, **kw)
        assert R.min_lattice_distance(om, x.shape[1], x.shape[2], *geo[:4], geo[4], geo[6], geo[7]) == 0.0
        want = R.dcnv4_ref(x.double(), om.double(), *geo)
        got = dcnv4.dcnv4_forward(x.to(DEV), om.to(DEV), *geo)
        assert_close("integer %s output" % name, got, want, 1e-4)


def test_accumulate_against_overwrite():
    """The two gradients added to non-zero buffers, fp16: buffer + gradient, rounded once."""
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
    # overwrite mode ignores what the buffers hold
    over = _native((x, om, go), geo)
    _compare("overwrite", over, want, _tols(t))


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
    """NO_GRAD_INPUT: grad_input NULL, the smaller workspace between pattern-filled margins; grad_offset_mask is bit for
    bit that of the full call.  The full and the deterministic call run guarded as well: the figure is exact."""
    t, geo, want = _case("g4_d16", dtype, coord_dtype)
    dt = _dev(t)
    full = _native(dt, geo)
    touched, calls = [], []
    _guard(monkeypatch, touched, calls)
    part = _native(dt, geo, need_grad_input=False)
    again = _native(dt, geo)
    det = _native(dt, geo, deterministic=True)
    assert touched == [], touched
    sizes = [b for name, b in calls if name == "mdconv_dcnv4_backward"]
    assert [b for name, b in calls if name == "mdconv_dcnv4_forward"] == [0, 0, 0]
    assert sizes[0] == 0 < sizes[1] <= sizes[2], sizes
    assert part[1] is None
    for i in (0, 2):
        assert torch.equal(part[i], full[i]) and torch.equal(again[i], full[i]) and torch.equal(det[i], full[i]), NAMES[i]
    _compare("guarded full", again, want, _tols(t))
    _compare("guarded deterministic", det, want, _tols(t))


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

    out = torch.empty_like(first[0])
    bufs = tuple(torch.empty_like(v) for v in (x, om))

    def step():
        dcnv4.dcnv4_forward(x, om, *geo, output=out)
        for b in bufs:   # caller-allocated buffers are added to
            b.zero_()
        dcnv4.dcnv4_backward(x, om, go, *geo, grads=bufs, deterministic=True)

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


def test_module_step_under_autocast():
    """The DCNv4 module under torch.autocast(bfloat16) against the same module with dcnv4_core swapped for dcnv4_ref: the
    Python surface and the autograd wiring (output, input gradient and every parameter gradient); then a call whose input
    needs no gradient."""
    from modulated_deform_conv_amd import DCNv4
    torch.manual_seed(21)
    mod = DCNv4(channels=32, kernel_size=3, group=4, offset_scale=1.0, dw_kernel_size=3, remove_center=True).to(DEV)
    with torch.no_grad():   # offsets away from the lattice, masks that differ
        mod.offset_mask.weight.normal_(0, 0.01)
        mod.offset_mask.bias.uniform_(0.3, 0.7)
    x = torch.randn(2, 6 * 5, 32, device=DEV)
    go = torch.randn(2, 6 * 5, 32, device=DEV)
    results = []
    for core in (None, R.dcnv4_ref):
        if core is not None:
            mod._core = core
        mod.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=BF16):
            y = mod(xi, shape=(6, 5))
        assert y.dtype == BF16 and y.shape == x.shape
        y.backward(go.to(y.dtype))
        torch.cuda.synchronize()
        results.append(dict(output=y.detach(), grad_x=xi.grad, **{k: p.grad for k, p in mod.named_parameters()}))
    native, ref = results
    assert all(v is not None for v in native.values()) and len(native) == 10
    for k in native:
        assert_close("module %s" % k, native[k], ref[k], TOL[BF16])
    # the input needs no gradient: the backward runs with NO_GRAD_INPUT and still returns the other gradient, in fp32
    # coordinates beside fp16 values
    from modulated_deform_conv_amd import dcnv4_core
    t, geo, want = _case("g4_d16", F16, F32)
    xs, om, go2 = _dev(t)
    om.requires_grad_(True)
    dcnv4_core(xs, om, *geo).backward(go2)
    assert xs.grad is None and om.grad.dtype == F32
    assert_close("selective grad_offset_mask", om.grad, want[2], 1e-4)
