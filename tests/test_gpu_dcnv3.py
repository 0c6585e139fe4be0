"""The DCNv3 core operator on the GPU (include/mdconv.h, "DCNv3 core operator"): output and the three gradients against
``tests.dcnv3_ref.dcnv3_ref`` evaluated in fp64 from the inputs as the kernel sees them (16-bit inputs rounded first), at the
project's tolerances -- 1e-4 for fp32, ``TOL`` of tests/test_gpu_hp.py for fp16 / bf16 -- on the smallest shapes at which each
part can go wrong, plus the call modes: accumulate, NO_GRAD_INPUT under a guarded workspace, determinism, graph replay, and
the module under autocast."""
import functools

import pytest
import torch

from tests import dcnv3_ref as R
from tests.test_gpu_hp import TOL as TOL16
from tests.util import assert_close, guarded_run

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(TOL16)
TOL[torch.float32] = 1e-4

CASES = {
    # one lane per (pixel, group); odd extents; border corners
    "one_lane": dict(B=1, G=1, D=4, H=5, W=7, kernel=3, pad=1),
    # width-major tap order and (x, y) offset order (a swap fails only with a non-square kernel); image stride; c_h != c_w
    "rect_5x3": dict(B=2, G=3, D=8, H=6, W=5, kernel=(5, 3), stride=2, pad=(2, 1), dilation=2, offset_scale=0.5),
    # two lanes per pair; the cross-lane sums of grad_offset / grad_mask
    "g4_d16": dict(B=2, G=4, D=16, H=9, W=8, kernel=3, pad=1),
    # eight lanes per pair; K = 1
    "d64_1x1": dict(B=1, G=2, D=64, H=4, W=4, kernel=1, offset_scale=2.0),
    # one long list per corner pixel: every sample lands between input pixels (1, 1) and (2, 2)
    "crafted": dict(B=2, G=1, D=4, H=4, W=4, kernel=3, pad=1),
    "far": dict(B=1, G=2, D=4, H=8, W=8, kernel=3, pad=1),
    # three vectors per group in four lanes (one idle lane per pair in the butterfly); 65 vectors: 64 lanes, two rounds
    "three_vectors": dict(B=1, G=2, D=12, H=5, W=4, kernel=3, pad=1),
    "two_rounds": dict(B=1, G=1, D=260, H=3, W=4, kernel=3, pad=1),
    "two_rounds_16bit": dict(B=1, G=1, D=520, H=3, W=4, kernel=3, pad=1),
}


@functools.lru_cache(maxsize=None)
def _case(name, dtype, variant=""):
    """CPU inputs of a case and its fp64 reference (output, grad_input, grad_offset, grad_mask), computed once."""
    kw = dict(CASES[name])
    if variant == "integer":
        kw["integer_offsets"] = True
    x, off, m, go, geo = R.make_inputs(dtype=dtype, seed=len(name) + 7, **kw)
    if name == "crafted":
        # loc = wo + i - 1 + off_x (3x3, pad 1, scale 1): aim every tap of every pixel at (1.3, 1.4)
        loc_h, loc_w = R.positions(torch.zeros_like(off), 4, 4, *geo[:4], 1, 1.0)
        off = torch.stack([1.3 - loc_w, 1.4 - loc_h], -1).reshape(off.shape).to(dtype)
    if name == "far":
        off = (off + torch.where(torch.rand(off.shape, generator=torch.Generator().manual_seed(5)) < 0.5, -20.0, 20.0)).to(dtype)
    if variant != "integer" and name != "far":
        assert R.min_lattice_distance(off, x.shape[1], x.shape[2], *geo[:4], geo[4], geo[6]) >= R.MARGIN
    return (x, off, m, go), geo, R.dcnv3_ref_grads(x, off, m, go, *geo)


def _native(t, geo, grads=None, need_grad_input=True, deterministic=False):
    from modulated_deform_conv_amd import dcnv3
    x, off, m, go = t
    out = dcnv3.dcnv3_forward(x, off, m, *geo)
    g = dcnv3.dcnv3_backward(x, off, m, go, *geo, grads=grads, need_grad_input=need_grad_input, deterministic=deterministic)
    torch.cuda.synchronize()
    return (out,) + tuple(g)


def _dev(t):
    return tuple(v.to(DEV) for v in t)


NAMES = ("output", "grad_input", "grad_offset", "grad_mask")


def _compare(tag, got, want, tol):
    for what, a, b in zip(NAMES, got, want):
        assert_close("%s %s" % (tag, what), a, b, tol)


@pytest.mark.parametrize("name, dtype", [
    ("one_lane", torch.float32), ("rect_5x3", torch.float32), ("g4_d16", torch.float16), ("g4_d16", torch.bfloat16),
    ("d64_1x1", torch.bfloat16), ("crafted", torch.float32), ("g4_d16", torch.float32), ("rect_5x3", torch.float16),
    ("three_vectors", torch.float32), ("two_rounds", torch.float32), ("two_rounds_16bit", torch.float16),
])
def test_against_reference(name, dtype):
    t, geo, want = _case(name, dtype)
    _compare("%s %s" % (name, dtype), _native(_dev(t), geo), want, TOL[dtype])


def test_samples_wholly_outside():
    """Offsets of +-20 px: nothing is read, the output and every gradient are zero, the lists are empty."""
    t, geo, want = _case("far", torch.float32)
    assert all(float(w.abs().max()) == 0.0 for w in want)
    got = _native(_dev(t), geo)
    _compare("far", got, want, 1e-4)
    assert all(float(g.abs().max()) == 0.0 for g in got)


def test_forward_at_integer_positions():
    """Corner weights exactly 0 / 1 and the loc < size edge.  Forward only: ``dcnv3_ref`` (``F.grid_sample``) is no reference
    for the gradients on the lattice; the backward there is tests/test_gpu_lattice.py, against ``dcnv3_direct``."""
    from modulated_deform_conv_amd import dcnv3
    for name in ("one_lane", "rect_5x3"):
        kw = dict(CASES[name])
        kw["offset_scale"] = 1.0 if name == "one_lane" else 2.0   # (integer positions need an integer scale)
        x, off, m, go, geo = R.make_inputs(dtype=torch.float32, seed=3, integer_offsets=True, **kw)
        assert R.min_lattice_distance(off, x.shape[1], x.shape[2], *geo[:4], geo[4], geo[6]) == 0.0
        want = R.dcnv3_ref(x.double(), off.double(), m.double(), *geo)
        got = dcnv3.dcnv3_forward(x.to(DEV), off.to(DEV), m.to(DEV), *geo)
        assert_close("integer %s output" % name, got, want, 1e-4)


def test_accumulate_against_overwrite():
    """The three gradients added to non-zero buffers, fp16: buffer + gradient, rounded once."""
    dtype = torch.float16
    t, geo, want = _case("g4_d16", dtype)
    x, off, m, go = _dev(t)
    gen = torch.Generator().manual_seed(9)
    base = tuple(torch.randn(v.shape, generator=gen).to(dtype) for v in (x, off, m))
    bufs = tuple(b.to(DEV) for b in base)
    got = _native((x, off, m, go), geo, grads=bufs)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got[1:], bufs))
    for what, a, b, w in zip(NAMES[1:], got[1:], base, want[1:]):
        assert_close("accumulate %s" % what, a, b.double() + w, TOL[dtype])
    # overwrite mode ignores what the buffers hold
    over = _native((x, off, m, go), geo)
    _compare("overwrite", over, want, TOL[dtype])


def _guard(monkeypatch, touched, calls):
    """tests.util.guarded_run in the place of dcnv3._run; it sizes the workspace through ``mdconv_workspace_bytes`` of the
    library handle, which for this operator's descriptor is ``mdconv_dcnv3_workspace_bytes``."""
    from modulated_deform_conv_amd import _capi, dcnv3
    real = _capi.lib()

    class Lib:
        mdconv_workspace_bytes = staticmethod(real.mdconv_dcnv3_workspace_bytes)

        def __getattr__(self, name):
            return getattr(real, name)

    proxy = Lib()
    monkeypatch.setattr(_capi, "lib", lambda: proxy)
    monkeypatch.setattr(dcnv3, "_run", guarded_run(touched, calls))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_no_grad_input_under_the_guarded_workspace(monkeypatch, dtype):
    """NO_GRAD_INPUT: grad_input NULL, the smaller workspace between pattern-filled margins; grad_offset / grad_mask are bit
    for bit those of the full call.  The full and the deterministic call run guarded as well: the figure is exact."""
    t, geo, want = _case("g4_d16", dtype)
    dt = _dev(t)
    full = _native(dt, geo)
    touched, calls = [], []
    _guard(monkeypatch, touched, calls)
    part = _native(dt, geo, need_grad_input=False)
    again = _native(dt, geo)
    det = _native(dt, geo, deterministic=True)
    assert touched == [], touched
    sizes = [b for name, b in calls if name == "mdconv_dcnv3_backward"]
    assert [b for name, b in calls if name == "mdconv_dcnv3_forward"] == [0, 0, 0]
    assert sizes[0] == 0 < sizes[1] <= sizes[2], sizes
    assert part[1] is None
    for i in (0, 2, 3):
        assert torch.equal(part[i], full[i]) and torch.equal(again[i], full[i]) and torch.equal(det[i], full[i]), NAMES[i]
    _compare("guarded full", again, want, TOL[dtype])
    _compare("guarded deterministic", det, want, TOL[dtype])


@pytest.mark.parametrize("name, dtype", [("crafted", torch.float32), ("g4_d16", torch.float32), ("g4_d16", torch.float16)])
def test_deterministic_mode(name, dtype):
    """With the flag all four results are bit-identical between two eager runs and a run replayed from a HIP graph;
    without it the output, grad_offset and grad_mask are as well."""
    from modulated_deform_conv_amd import dcnv3
    t, geo, want = _case(name, dtype)
    x, off, m, go = _dev(t)
    first = _native((x, off, m, go), geo, deterministic=True)
    second = _native((x, off, m, go), geo, deterministic=True)
    for what, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), "deterministic %s differs between two runs" % what
    plain = [_native((x, off, m, go), geo) for _ in range(2)]
    for i in (0, 2, 3):
        assert torch.equal(plain[0][i], plain[1][i]) and torch.equal(plain[0][i], first[i]), NAMES[i]
    assert_close("unflagged grad_input", plain[0][1], want[1], TOL[dtype])

    out = torch.empty_like(first[0])
    bufs = tuple(torch.empty_like(v) for v in (x, off, m))

    def step():
        dcnv3.dcnv3_forward(x, off, m, *geo, output=out)
        for b in bufs:   # caller-allocated buffers are added to
            b.zero_()
        dcnv3.dcnv3_backward(x, off, m, go, *geo, grads=bufs, deterministic=True)

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
    """The DCNv3 module under torch.autocast(bfloat16) against the same module with dcnv3_core swapped for dcnv3_ref: the
    Python surface and the autograd wiring (output, input gradient and every parameter gradient)."""
    from modulated_deform_conv_amd import DCNv3
    torch.manual_seed(21)
    mod = DCNv3(channels=32, kernel_size=3, group=4, offset_scale=1.0).to(DEV)
    with torch.no_grad():   # offsets away from the lattice, masks that differ
        mod.offset.weight.normal_(0, 0.01)
        mod.offset.bias.uniform_(0.3, 0.7)
        mod.mask.weight.normal_(0, 0.1)
    x = torch.randn(2, 6, 5, 32, device=DEV)
    go = torch.randn(2, 6, 5, 32, device=DEV)
    results = []
    for core in (None, R.dcnv3_ref):
        if core is not None:
            mod._core = core
        mod.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = mod(xi)
        assert y.dtype == torch.bfloat16
        y.backward(go.to(y.dtype))
        torch.cuda.synchronize()
        results.append(dict(output=y.detach(), grad_x=xi.grad, **{k: p.grad for k, p in mod.named_parameters()}))
    native, ref = results
    assert all(v is not None for v in native.values())
    for k in native:
        assert_close("module %s" % k, native[k], ref[k], TOL[torch.bfloat16])
    # the input needs no gradient: the backward runs with NO_GRAD_INPUT and still returns the other two
    from modulated_deform_conv_amd import dcnv3_core
    t, geo, want = _case("g4_d16", torch.float32)
    xs, off, m, go2 = _dev(t)
    off.requires_grad_(True)
    m.requires_grad_(True)
    dcnv3_core(xs, off, m, *geo).backward(go2)
    assert xs.grad is None
    assert_close("selective grad_offset", off.grad, want[2], 1e-4)
    assert_close("selective grad_mask", m.grad, want[3], 1e-4)
