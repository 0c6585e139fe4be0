"""Deformable RoI pooling on the GPU (include/mdconv.h, "Deformable RoI pooling"): output, grad_input and grad_offset against
``tests.droi_ref.droi_explicit`` evaluated in fp64 from the inputs as the kernel sees them (16-bit inputs rounded first), at
the project's tolerances -- 1e-4 for fp32, ``TOL`` of tests/test_gpu_hp.py for fp16 / bf16, by the value dtype for value-typed
results and by the coordinate dtype for grad_offset -- on the smallest shapes at which each part can go wrong, plus the call
modes: accumulate, NO_GRAD_INPUT under a guarded workspace, determinism, graph replay, the Function's layouts and the Pack
modules under autocast."""
import copy
import functools

import pytest
import torch

from tests import droi_ref as R
from tests.test_gpu_hp import TOL as TOL16
from tests.util import assert_close, guarded_run

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(TOL16)
TOL[torch.float32] = 1e-4
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
FIVE = [(F32, None), (F16, None), (BF16, None), (F16, F32), (BF16, F32)]
NAMES = ("output", "grad_input", "grad_offset")

ADAPTIVE_ROIS = [
    [0, 2.1, 3.2, 3.5, 4.8],      # bins 0.7 x 0.8: grid 1 x 1
    [1, 4.3, 1.1, 7.3, 4.5],      # bins 1.5 x 1.7: grid 2 x 2
    [0, 6.2, 5.1, 10.8, 10.3],    # bins 2.3 x 2.6: grid 3 x 3
    [1, 1.4, 0.6, 11.8, 11.6],    # bins 5.2 x 5.5: beyond the cap of 4
    [0, 5.0, 5.0, 4.5, 7.3],      # degenerate: rw < 0, no samples
    [1, -2.3, -1.7, 15.1, 13.3],  # hangs over every border of the 12 x 14 map: clamps and the gate
    [0, 3.3, 2.2, 5.1, 7.4],      # bins 0.9 x 2.6: grid 3 (y) x 1 (x)
]
INVALID_ROIS = [[0, 1.0, 1.0, 4.2, 4.4], [-1, 1.0, 1.0, 4.2, 4.4], [2, 1.0, 1.0, 4.2, 4.4], [1.5, 1.0, 1.0, 4.2, 4.4],
                [float("nan"), 1.0, 1.0, 4.2, 4.4], [1, 1.0, float("inf"), 4.2, 4.4], [1, 0.8, 1.3, 3.9, 4.6]]

CASES = {
    # one lane per bin; odd extents
    "one_lane": dict(B=1, C=4, H=5, W=7, R=3, PH=2, PW=2, sampling_ratio=2),
    # swapped x / y planes, PH against PW, idle lanes (6 vectors in 8 lanes; 3 in 4), the unordered batch index
    "rect": dict(B=2, C=24, H=6, W=9, R=5, PH=3, PW=2, sampling_ratio=3, spatial_scale=0.5, gamma=0.3),
    # 65 vectors per bin: 64 lanes, two rounds
    "two_rounds": dict(B=1, C=260, H=3, W=4, R=2, PH=2, PW=2, sampling_ratio=2),
    "two_rounds_16bit": dict(B=1, C=520, H=3, W=4, R=2, PH=2, PW=2, sampling_ratio=2),
    "adaptive": dict(B=2, C=8, H=12, W=14, rois=ADAPTIVE_ROIS, PH=2, PW=2, sampling_ratio=0, max_grid=4, gamma=0.2),
    "no_offset": dict(B=2, C=8, H=7, W=8, R=4, PH=2, PW=2, sampling_ratio=2, with_offset=False),
    "invalid_rois": dict(B=2, C=8, H=6, W=6, rois=INVALID_ROIS, PH=2, PW=2, sampling_ratio=2),
    "far": dict(B=1, C=8, H=7, W=7, R=3, PH=2, PW=2, sampling_ratio=2, off_lattice=False),
    # 64 identical RoIs on a 3 x 3 map: 4096 entries in nine lists
    "pile": dict(B=1, C=8, H=3, W=3, rois=[[0, 0.7, 0.6, 2.4, 2.3]] * 64, PH=2, PW=2, sampling_ratio=2, gamma=0.05),
}


def _geo(kw):
    return dict(output_size=(kw["PH"], kw["PW"]), spatial_scale=kw.get("spatial_scale", 1.0),
                sampling_ratio=kw.get("sampling_ratio", 0), gamma=kw.get("gamma", 0.1), max_grid=kw.get("max_grid", 8))


@functools.lru_cache(maxsize=None)
def _case(name, dtype, coord_dtype=None):
    """CPU inputs of a case, its geometry and its fp64 reference (output and the two gradients), computed once."""
    kw = CASES[name]
    inp, rois, off, go = R.make_inputs(dtype=dtype, coord_dtype=coord_dtype, seed=len(name) + 3, **kw)
    geo = _geo(kw)
    if name == "far":
        gen = torch.Generator().manual_seed(5)
        off = torch.where(torch.rand(off.shape, generator=gen) < 0.5, -64.0, 64.0).to(off.dtype)
    if name == "adaptive":   # the case is what it claims
        g = R.geometry(rois, off, kw["B"], 2, 2, 1.0, 0, geo["gamma"], 4)
        assert g["gh"].tolist() == [1, 2, 3, 4, 2, 4, 3] and g["gw"].tolist() == [1, 2, 3, 4, 0, 4, 1]
        assert float(g["bh"][3]) > 4 and float(g["bw"][4]) < 0
        beyond = clamped = False   # the overhanging RoI: samples past the gate and in the clamped zones
        for c, live, size in ((g["y"][5], g["live_y"][5], 12), (g["x"][5], g["live_x"][5], 14)):
            c = c[live.expand_as(c)]
            beyond |= bool((c < -1).any() | (c > size).any())
            clamped |= bool(((c > -1) & (c < 0)).any() | ((c > size - 1) & (c < size)).any())
        assert beyond and clamped
    return (inp, rois, off, go), geo, R.droi_explicit(inp, rois, off, grad_output=go, **geo)


def _dev(t):
    return tuple(None if v is None else v.to(DEV) for v in t)


def _native(t, geo, grads=None, need_grad_input=True, deterministic=False, accumulate=None, output=None):
    from modulated_deform_conv_amd import droi
    inp, rois, off, go = t
    out = droi.deform_roi_pool_forward(inp, rois, off, output=output, **geo)
    gi, goff = droi.deform_roi_pool_backward(inp, rois, off, go, grads=grads, need_grad_input=need_grad_input,
                                             deterministic=deterministic, accumulate=accumulate, **geo)
    torch.cuda.synchronize()
    return out, gi, goff


def _tols(t):
    """Per result: value-typed results by the value dtype, grad_offset by the coordinate dtype."""
    return (TOL[t[0].dtype], TOL[t[0].dtype], TOL[t[0].dtype if t[2] is None else t[2].dtype])


def _compare(tag, got, want, tols):
    for what, a, b, tol in zip(NAMES, got, want, tols):
        if a is None:
            assert b is None or what == "grad_input", what
            continue
        print("%s %s: max |want| %.3e" % (tag, what, float(b.abs().max())))
        assert_close("%s %s" % (tag, what), a, b, tol)


PARITY = ([("one_lane", F32, None)] + [("rect", d, c) for d, c in FIVE] + [("adaptive", d, c) for d, c in FIVE] +
          [("two_rounds" if d == F32 else "two_rounds_16bit", d, c) for d, c in FIVE] +
          [("no_offset", F32, None), ("no_offset", BF16, None), ("pile", F32, None), ("pile", F16, F32)])


@pytest.mark.parametrize("name, dtype, coord_dtype", PARITY)
def test_against_reference(name, dtype, coord_dtype):
    t, geo, want = _case(name, dtype, coord_dtype)
    got = _native(_dev(t), geo)
    assert got[0].dtype == got[1].dtype == dtype and got[0].shape == want[0].shape
    if t[2] is None:
        assert got[2] is None and want[2] is None
    else:
        assert got[2].dtype == (coord_dtype or dtype)
    assert all(float(w.abs().max()) > 0 for w in want if w is not None)
    _compare("%s %s/%s" % (name, dtype, coord_dtype), got, want, _tols(t))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_invalid_rois_under_the_guarded_workspace(monkeypatch, dtype):
    """Batch indices -1, B, 1.5 and NaN and an infinite corner: zero output rows, exact zero gradients (overwrite) or
    untouched rows (accumulate), nothing added to grad_input, nothing written outside the workspace; the valid RoIs of the
    call hold the tolerance."""
    t, geo, want = _case("invalid_rois", dtype)
    bad = [1, 2, 3, 4, 5]
    assert all(float(w[bad].abs().max()) == 0.0 for w in (want[0], want[2])) and float(want[0][[0, 6]].abs().min()) > 0
    dt = _dev(t)
    touched, calls = [], []
    _guard(monkeypatch, touched, calls)
    out = torch.full(want[0].shape, float("nan"), dtype=dtype, device=DEV)
    got = _native(dt, geo, output=out)
    assert touched == [], touched
    assert got[0].data_ptr() == out.data_ptr()
    assert float(got[0][bad].abs().max()) == 0.0 and float(got[2][bad].abs().max()) == 0.0
    _compare("invalid_rois %s" % dtype, got, want, _tols(t))
    # accumulate: the rows of the invalid RoIs keep their bits, -0.0 included
    base = torch.full(want[2].shape, -0.0, dtype=dtype)
    base[0] = 1.0
    bufs = (torch.zeros_like(dt[0]), base.to(DEV))
    acc = _native(dt, geo, grads=bufs, deterministic=True)
    assert touched == [], touched
    assert torch.equal(acc[2][bad].view(torch.int16 if dtype == BF16 else torch.int32),
                       base[bad].to(DEV).view(torch.int16 if dtype == BF16 else torch.int32))
    assert_close("invalid_rois accumulate %s grad_offset" % dtype, acc[2], base.double() + want[2], TOL[dtype])
    assert_close("invalid_rois accumulate %s grad_input" % dtype, acc[1], want[1], TOL[dtype])


def test_samples_wholly_outside():
    """Offsets of +-64 push every sample past the gate: nothing is read, the output and both gradients are exactly zero, the
    lists are empty."""
    t, geo, want = _case("far", F32)
    assert all(float(w.abs().max()) == 0.0 for w in want)
    got = _native(_dev(t), geo)
    assert all(float(g.abs().max()) == 0.0 for g in got)
    got = _native(_dev(t), geo, deterministic=True)
    assert all(float(g.abs().max()) == 0.0 for g in got)


@pytest.mark.parametrize("dtype, coord_dtype, C", [(F32, None, 4), (F16, None, 8), (BF16, F32, 8)])
def test_lattice_and_clamped_zones(dtype, coord_dtype, C):
    """Samples exactly on the lattice, in both clamped zones, on the gate's edges and beyond it (``droi_ref.lattice_inputs``:
    coordinates that are exact in every dtype) against the explicit reference, whose closed forms test_droi_cpu.py checks
    against forward differences there: the right-sided derivative, and EXACT zeros where the reference has them."""
    inp, rois, off, go, geo = R.lattice_inputs(dtype=dtype, coord_dtype=coord_dtype, C=C)
    t = (inp, rois, off, go)
    want = R.droi_explicit(inp, rois, off, grad_output=go, **geo)
    got = _native(_dev(t), geo, deterministic=True)
    _compare("lattice %s/%s" % (dtype, coord_dtype), got, want, _tols(t))
    for what, a, b in zip(NAMES, got, want):
        zero = b == 0
        assert bool(zero.any()) and float(a.cpu()[zero].abs().max()) == 0.0, what
    assert float(want[2][0, :, 1, 1].abs().max()) == 0.0 and float(want[2][0, 0, 0, 1].abs()) > 0


def test_accumulate_against_overwrite():
    """Both gradients added to non-zero buffers, fp16 values with fp32 offsets: each buffer + gradient in its own dtype,
    rounded once; overwrite mode ignores what the buffers hold, NaN included."""
    t, geo, want = _case("rect", F16, F32)
    dt = _dev(t)
    gen = torch.Generator().manual_seed(9)
    base = tuple(torch.randn(v.shape, generator=gen).to(v.dtype) for v in (t[0], t[2]))
    bufs = tuple(b.to(DEV) for b in base)
    got = _native(dt, geo, grads=bufs)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got[1:], bufs)) and (bufs[0].dtype, bufs[1].dtype) == (F16, F32)
    for what, a, b, w, tol in zip(NAMES[1:], got[1:], base, want[1:], _tols(t)[1:]):
        assert_close("accumulate %s/%s %s" % (F16, F32, what), a, b.double() + w, tol)
    nans = tuple(torch.full_like(b, float("nan")) for b in bufs)
    over = _native(dt, geo, grads=nans, accumulate=False, output=torch.full(want[0].shape, float("nan"), dtype=F16, device=DEV))
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(over[1:], nans))
    _compare("overwrite onto NaN %s/%s" % (F16, F32), over, want, _tols(t))
    fresh = _native(dt, geo)
    assert torch.equal(fresh[0], over[0]) and torch.equal(fresh[2], over[2])


def _guard(monkeypatch, touched, calls):
    """tests.util.guarded_run in the place of droi._run; it sizes the workspace through ``mdconv_workspace_bytes`` of the
    library handle, which for this operator's descriptor is ``mdconv_droi_workspace_bytes``."""
    from modulated_deform_conv_amd import _capi, droi
    real = _capi.lib()

    class Lib:
        mdconv_workspace_bytes = staticmethod(real.mdconv_droi_workspace_bytes)

        def __getattr__(self, name):
            return getattr(real, name)

    proxy = Lib()
    monkeypatch.setattr(_capi, "lib", lambda: proxy)
    monkeypatch.setattr(droi, "_run", guarded_run(touched, calls))


@pytest.mark.parametrize("name, dtype, coord_dtype", [("rect", F32, None), ("adaptive", BF16, F32)])
def test_no_grad_input_under_the_guarded_workspace(monkeypatch, name, dtype, coord_dtype):
    """NO_GRAD_INPUT: grad_input NULL, no workspace between pattern-filled margins; grad_offset is bit for bit the full
    call's.  The full and the deterministic call run guarded as well: the figure is exact."""
    t, geo, want = _case(name, dtype, coord_dtype)
    dt = _dev(t)
    full = _native(dt, geo)
    touched, calls = [], []
    _guard(monkeypatch, touched, calls)
    part = _native(dt, geo, need_grad_input=False)
    again = _native(dt, geo)
    det = _native(dt, geo, deterministic=True)
    assert touched == [], touched
    sizes = [b for n, b in calls if n == "mdconv_droi_backward"]
    assert [b for n, b in calls if n == "mdconv_droi_forward"] == [0, 0, 0]
    assert sizes[0] == 0 < sizes[1] < sizes[2], sizes
    assert part[1] is None
    for i in (0, 2):
        assert torch.equal(part[i], full[i]) and torch.equal(again[i], full[i]) and torch.equal(det[i], full[i]), NAMES[i]
    _compare("guarded full %s/%s" % (dtype, coord_dtype), again, want, _tols(t))
    _compare("guarded deterministic %s/%s" % (dtype, coord_dtype), det, want, _tols(t))


@pytest.mark.parametrize("name, dtype, coord_dtype", [("pile", F32, None), ("pile", BF16, F32), ("adaptive", F16, None)])
def test_deterministic_mode(name, dtype, coord_dtype):
    """With the flag grad_input is bit-identical over 8 runs (the pile: lists of ~450 entries) and over two replays of a HIP
    graph that holds forward + backward into caller buffers; without it output and grad_offset are bit-identical from call to
    call as well and grad_input holds the tolerance."""
    from modulated_deform_conv_amd import droi
    t, geo, want = _case(name, dtype, coord_dtype)
    inp, rois, off, go = dt = _dev(t)
    first = _native(dt, geo, deterministic=True)
    for _ in range(7):
        again = _native(dt, geo, deterministic=True)
        for what, a, b in zip(NAMES, first, again):
            assert torch.equal(a, b), "deterministic %s differs between two runs" % what
    plain = [_native(dt, geo) for _ in range(2)]
    for i in (0, 2):
        assert torch.equal(plain[0][i], plain[1][i]) and torch.equal(plain[0][i], first[i]), NAMES[i]
    assert_close("unflagged %s %s/%s grad_input" % (name, dtype, coord_dtype), plain[0][1], want[1], TOL[dtype])
    _compare("deterministic %s %s/%s" % (name, dtype, coord_dtype), first, want, _tols(t))

    out = torch.empty_like(first[0])
    bufs = (torch.empty_like(inp), torch.empty_like(off))

    def step():
        droi.deform_roi_pool_forward(inp, rois, off, output=out, **geo)
        for b in bufs:   # caller-allocated buffers are added to
            b.zero_()
        droi.deform_roi_pool_backward(inp, rois, off, go, grads=bufs, deterministic=True, **geo)

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


@pytest.mark.parametrize("dtype", [F32, F16])
def test_function_on_contiguous_and_channels_last_inputs(dtype):
    """The Function on logical NCHW tensors: a contiguous input (one layout copy) and a channels_last one (none) give equal
    results with logical shapes, in the caller's dtypes; ``offset`` None and an empty tensor mean no offset; ``input`` without
    requires_grad gets no gradient."""
    from modulated_deform_conv_amd import DeformRoIPoolFunction, deform_roi_pool
    t, geo, want = _case("rect", dtype, F32 if dtype == F16 else None)
    inp, rois, off, go = _dev(t)
    args = (geo["output_size"], geo["spatial_scale"], geo["sampling_ratio"], geo["gamma"])
    R_, C = rois.shape[0], inp.shape[3]
    results = []
    for layout in ("contiguous", "channels_last"):
        x = inp.permute(0, 3, 1, 2)   # logical NCHW over the channels-last buffer
        x = (x.contiguous() if layout == "contiguous" else x.contiguous(memory_format=torch.channels_last)).requires_grad_(True)
        assert x.is_contiguous() == (layout == "contiguous")
        o = off.clone().requires_grad_(True)
        y = DeformRoIPoolFunction.apply(x, rois, o, *args)
        assert y.shape == (R_, C, 3, 2) and y.dtype == dtype
        y.backward(go.permute(0, 3, 1, 2))
        assert x.grad.shape == x.shape and x.grad.dtype == dtype and o.grad.shape == off.shape and o.grad.dtype == off.dtype
        results.append((y.detach(), x.grad, o.grad))
    # the same bits where the operator promises them; grad_input without the deterministic flag agrees to rounding
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][2], results[1][2])
    assert_close("function %s grad_input, contiguous" % dtype, results[0][1].permute(0, 2, 3, 1), want[1], TOL[dtype])
    y, gx, goff = results[1]
    assert_close("function %s output" % dtype, y.permute(0, 2, 3, 1), want[0], TOL[dtype])
    assert_close("function %s grad_input" % dtype, gx.permute(0, 2, 3, 1), want[1], TOL[dtype])
    assert_close("function %s grad_offset" % dtype, goff, want[2], TOL[off.dtype])
    # no offset: None and an empty tensor; the input needs no gradient
    x = inp.permute(0, 3, 1, 2)
    plain = deform_roi_pool(x, rois, None, geo["output_size"], geo["spatial_scale"], geo["sampling_ratio"], geo["gamma"])
    empty = DeformRoIPoolFunction.apply(x, rois, x.new_empty(0), *args)
    ref = R.droi_explicit(t[0], t[1], None, **geo)
    assert torch.equal(plain, empty) and not plain.requires_grad
    assert_close("function %s without offset" % dtype, plain.permute(0, 2, 3, 1), ref, TOL[dtype])
    o = off.clone().requires_grad_(True)
    deform_roi_pool(x, rois, o, **geo).backward(go.permute(0, 3, 1, 2))
    assert x.grad is None and torch.equal(o.grad, goff)


PACK = dict(B=2, C=16, H=8, W=10, R=4, PH=2, PW=2, sampling_ratio=2, spatial_scale=0.5, with_offset=False)
PACK_GEO = ((2, 2), 0.5, 2, 0.1, 8)


def _settle_offsets(mod, x, rois):
    """Randomise the last layer of ``offset_fc`` and re-draw the rows of the bins (ph, pw) whose offsets -- as the fp64
    reference computes them from ``x`` -- put a sample of any RoI near the lattice, until none does (the re-draw loop of
    ``droi_ref.make_inputs`` for offsets that a layer produces; the caller asserts MARGIN on the reference's own run)."""
    gen = torch.Generator().manual_seed(7)
    last = mod.offset_fc[4]
    with torch.no_grad():
        last.weight.copy_(torch.randn(last.weight.shape, generator=gen) * 0.08)
        last.bias.copy_(torch.randn(last.bias.shape, generator=gen) * 0.3)
        pooled = R.droi_nchw(x.double(), rois, None, *PACK_GEO)
        hidden = copy.deepcopy(mod.offset_fc[:4]).double()(pooled.reshape(pooled.shape[0], -1))
        for _ in range(500):
            off = (hidden @ last.weight.double().t() + last.bias.double()).view(-1, 2, 2, 2)
            d = R.min_lattice_distance(rois, off, 2, 2, 2, *PACK_GEO[1:], per_bin=True)
            bad = (d < 1.2 * R.MARGIN).any(0).flatten()
            if not bad.any():
                return
            rows = torch.cat([bad, bad]).nonzero().flatten()
            last.weight[rows] = torch.randn(len(rows), last.weight.shape[1], generator=gen) * 0.08
            last.bias[rows] = torch.randn(len(rows), generator=gen) * 0.3
    raise AssertionError("no off-lattice offsets found")


@pytest.mark.parametrize("cls", ["DeformRoIPoolPack", "ModulatedDeformRoIPoolPack"])
@pytest.mark.parametrize("init", ["zero", "random"])
def test_pack_modules_under_autocast(cls, init):
    """The Pack modules, forward + backward under torch.autocast(bfloat16), against the same module (a deep copy, in fp64 on
    the CPU) with the core swapped for the reference composition: the Python surface and the autograd wiring -- output, the
    input's gradient and every parameter gradient.  ``offset_fc`` zero-initialised (the published start: the second pooling
    repeats the first) and randomised (offsets that depend on the input; the reference's are ASSERTED off the lattice)."""
    from modulated_deform_conv_amd import droi
    torch.manual_seed(31)
    inp, rois, _, go = R.make_inputs(dtype=F32, seed=17, **PACK)
    x = inp.permute(0, 3, 1, 2).contiguous()
    mod = getattr(droi, cls)((2, 2), 16, deform_fc_channels=32, spatial_scale=0.5, sampling_ratio=2, gamma=0.1)
    if init == "random":
        _settle_offsets(mod, x, rois)
        if cls.startswith("Modulated"):
            with torch.no_grad():
                mod.mask_fc[2].weight.normal_(0, 0.1)
    ref_mod = copy.deepcopy(mod).double()
    seen = []

    def ref_pool(input, rois, offset):
        if offset is not None:
            seen.append(offset.detach())
        return R.droi_nchw(input, rois, offset, *PACK_GEO)

    ref_mod._pool = ref_pool
    xr = x.double().requires_grad_(True)
    yr = ref_mod(xr, rois)
    yr.backward(go.permute(0, 3, 1, 2).double())
    assert len(seen) == 1 and R.min_lattice_distance(rois, seen[0], 2, 2, 2, *PACK_GEO[1:]) >= R.MARGIN
    assert (float(seen[0].abs().max()) == 0.0) == (init == "zero")

    mod = mod.to(DEV)
    xi = x.to(DEV).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = mod(xi, rois.to(DEV))
    assert y.dtype == BF16 and y.shape == (4, 16, 2, 2)
    y.backward(go.permute(0, 3, 1, 2).to(DEV).to(y.dtype))
    torch.cuda.synchronize()
    assert xi.grad.dtype == F32
    assert_close("%s %s output" % (cls, init), y.detach(), yr.detach(), TOL[BF16])
    assert_close("%s %s grad_input" % (cls, init), xi.grad, xr.grad, TOL[BF16])
    ref_grads = dict(ref_mod.named_parameters())
    for k, p in mod.named_parameters():
        if ref_grads[k].grad is None:   # (zero-initialised last layers cut the layers before them off)
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert_close("%s %s grad %s" % (cls, init, k), p.grad, ref_grads[k].grad, TOL[BF16])
