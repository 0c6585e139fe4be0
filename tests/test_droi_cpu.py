"""Deformable RoI pooling without a GPU (include/mdconv.h, "Deformable RoI pooling"): the descriptor mirror, the exports,
validation and its order, each refusal with its word, workspace sizing, the two fp64 references against each other off the
lattice, the explicit reference against fp64 forward differences on the lattice and in the clamped zones, and the Python
surface.  Host code only: no kernel is launched."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from tests import droi_ref as R
from tests.util import rel_err

EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -5
F32, F16, BF16 = 0, 1, 3
PAIRINGS = ((F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32))
FIELDS = ["dtype", "coord_dtype", "batch", "channels", "height", "width", "rois", "pooled_h", "pooled_w", "sampling_ratio",
          "max_grid", "spatial_scale", "gamma", "with_offset", "accumulate", "flags"]
NAMES = ("mdconv_droi_workspace_bytes", "mdconv_droi_forward", "mdconv_droi_backward")


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def _desc(capi, dtype=F32, coord_dtype=None, B=2, C=32, H=10, W=12, R=6, PH=3, PW=2, ratio=2, max_grid=8, scale=1.0, gamma=0.1,
          with_offset=1, accumulate=1, flags=0):
    d = capi.MdconvDroiDesc()
    d.dtype, d.coord_dtype = dtype, dtype if coord_dtype is None else coord_dtype
    d.batch, d.channels, d.height, d.width = B, C, H, W
    d.rois, d.pooled_h, d.pooled_w, d.sampling_ratio, d.max_grid = R, PH, PW, ratio, max_grid
    d.spatial_scale, d.gamma = scale, gamma
    d.with_offset, d.accumulate, d.flags = with_offset, accumulate, flags
    return d


def _fwd(capi, d, p=None, ws=None, ws_bytes=0):
    p = ctypes.c_void_p(0) if p is None else p
    return capi.lib().mdconv_droi_forward(ctypes.byref(d), p, p, p, p, ctypes.c_void_p(0) if ws is None else ws,
                                          ctypes.c_size_t(ws_bytes), ctypes.c_void_p(0))


def _bwd(capi, d, p=None, ws=None, ws_bytes=0):
    p = ctypes.c_void_p(0) if p is None else p
    return capi.lib().mdconv_droi_backward(ctypes.byref(d), p, p, p, p, p, p, ctypes.c_void_p(0) if ws is None else ws,
                                           ctypes.c_size_t(ws_bytes), ctypes.c_void_p(0))


def _ws(capi, d, backward):
    return capi.lib().mdconv_droi_workspace_bytes(ctypes.byref(d), backward)


def test_descriptor_mirror_and_exports(capi):
    assert [f[0] for f in capi.MdconvDroiDesc._fields_] == FIELDS
    assert ctypes.sizeof(capi.MdconvDroiDesc) == 16 * 4
    hdr = (Path(__file__).resolve().parent.parent / "include" / "mdconv.h").read_text()
    body = re.search(r"typedef struct mdconv_droi_desc \{(.*?)\} mdconv_droi_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for line in re.findall(r"(?:int|float)\s+([a-z_, ]+);", body) for n in re.split(r",\s*", line.strip())]
    assert declared == FIELDS
    init = re.search(r"#define MDCONV_DROI_DESC_INIT \{([^}]*)\}", hdr).group(1)
    assert [v.strip() for v in init.split(",")] == ["0"] * 10 + ["8", "1.0f", "0.1f", "1", "1", "0"]
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr)
    assert L.mdconv_abi_version() == 2 == capi.ABI_VERSION
    # the siblings' descriptors have not moved
    assert ctypes.sizeof(capi.MdconvDesc) == 132 and ctypes.sizeof(capi.MdconvDcnv3Desc) == 68


def test_valid_descriptor_stops_at_null_pointers(capi):
    for dtype, cdt in PAIRINGS:
        for call in (_fwd, _bwd):
            assert call(capi, _desc(capi, dtype=dtype, coord_dtype=cdt)) == ENULL and "NULL" in capi.last_error()
    # a descriptor outside the shape rule as well: the pointer check comes first
    assert _fwd(capi, _desc(capi, C=6)) == ENULL and _bwd(capi, _desc(capi, C=6)) == ENULL
    for flags in (0, 1, 4, 5):
        assert _fwd(capi, _desc(capi, flags=flags)) == ENULL and _bwd(capi, _desc(capi, flags=flags)) == ENULL
    # the forward ignores both flags, also without offset; the adaptive rule and both ends of the ranges are valid
    assert _fwd(capi, _desc(capi, with_offset=0, flags=4)) == ENULL
    for kw in (dict(ratio=0, max_grid=1), dict(ratio=0, max_grid=16), dict(ratio=16), dict(ratio=1, max_grid=16), dict(gamma=0.0),
               dict(scale=-0.25)):
        assert _fwd(capi, _desc(capi, **kw)) == ENULL and _bwd(capi, _desc(capi, **kw)) == ENULL, kw


@pytest.mark.parametrize("kw, word", [
    (dict(dtype=2), "dtype"), (dict(dtype=7), "dtype"), (dict(dtype=F16 | 0x10), "dtype"),
    (dict(dtype=BF16, coord_dtype=F16), "coord_dtype"), (dict(dtype=F16, coord_dtype=BF16), "coord_dtype"),
    (dict(dtype=F32, coord_dtype=F16), "coord_dtype"), (dict(dtype=F32, coord_dtype=2), "coord_dtype"),
    (dict(B=0), "positive"), (dict(C=0), "positive"), (dict(H=0), "positive"), (dict(W=-1), "positive"), (dict(R=0), "positive"),
    (dict(PH=0), "positive"), (dict(PW=-3), "positive"),
    (dict(ratio=-1), "sampling_ratio"), (dict(ratio=17), "sampling_ratio"),
    (dict(max_grid=0), "max_grid"), (dict(max_grid=17), "max_grid"), (dict(ratio=0, max_grid=-1), "max_grid"),
    (dict(scale=float("inf")), "spatial_scale"), (dict(scale=float("nan")), "spatial_scale"),
    (dict(gamma=float("-inf")), "gamma"), (dict(gamma=float("nan")), "gamma"),
    (dict(accumulate=2), "accumulate"), (dict(accumulate=-1), "accumulate"),
    (dict(flags=2), "flags"), (dict(flags=8), "flags"), (dict(flags=1 | 4 | 32), "flags"), (dict(flags=256), "flags"),
])
def test_invalid_descriptor(capi, kw, word):
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, **kw)) == EINVAL, kw
        assert word in capi.last_error(), capi.last_error()
    assert _ws(capi, _desc(capi, **kw), 0) == 0 and _ws(capi, _desc(capi, **kw), 1) == 0
    assert capi.lib().mdconv_droi_forward(None, None, None, None, None, None, ctypes.c_size_t(0), None) == EINVAL


def test_a_backward_with_nothing_to_compute_is_invalid(capi):
    d = _desc(capi, with_offset=0, flags=capi.FLAG_NO_GRAD_INPUT)
    assert _bwd(capi, d) == EINVAL and "nothing to compute" in capi.last_error()
    assert _ws(capi, d, 1) == 0 and "nothing to compute" in capi.last_error()
    assert _ws(capi, d, 0) == 0 and capi.last_error() == ""   # the forward of that descriptor is a call like any other
    # either half alone is a call: only the pointers are missing
    assert _bwd(capi, _desc(capi, with_offset=0)) == ENULL and _bwd(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT)) == ENULL


def test_shape_rule_refusals_come_before_any_launch(capi):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # non-NULL; nothing dereferences it
    for d, word in ((_desc(capi, C=6), "multiple of 16"), (_desc(capi, dtype=F16, C=4), "multiple of 16"),
                    (_desc(capi, dtype=BF16, coord_dtype=F32, C=12), "multiple of 16"),
                    (_desc(capi, B=1 << 10, C=64, H=128, W=128), "2^31 bytes"),           # input: 2^32 bytes
                    (_desc(capi, C=256, R=1 << 16, PH=7, PW=7, ratio=1), "2^31 bytes"),   # output: 3.2e9 bytes
                    (_desc(capi, C=4, R=1 << 16, PH=7, PW=7, ratio=16), "grid^2"),        # 8.2e8 samples * 4 = 3.3e9
                    (_desc(capi, C=4, R=1 << 16, PH=7, PW=7, ratio=0, max_grid=16), "grid^2")):
        for call in (_fwd, _bwd):
            assert call(capi, d, p) == EUNSUPPORTED, word
            assert word in capi.last_error() and "shape rule" in capi.last_error(), capi.last_error()
        assert _ws(capi, d, 1) == 0 and _ws(capi, d, 0) == 0
    # max_grid is not read with a fixed ratio: the same shape is inside the rule with ratio 2 (sized only, nothing launched)
    assert _ws(capi, _desc(capi, C=4, R=1 << 16, PH=7, PW=7, ratio=2, max_grid=16), 1) > 0


def test_workspace_refusal_comes_last(capi):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = _desc(capi)
    need = _ws(capi, d, 1)
    assert need > 0
    assert _bwd(capi, d, p) == EWORKSPACE and "workspace" in capi.last_error()
    assert _bwd(capi, d, p, p, need - 1) == EWORKSPACE
    misaligned = ctypes.c_void_p(p.value + 4)
    assert _bwd(capi, d, p, misaligned, need) == EWORKSPACE and "aligned" in capi.last_error()
    # outside the shape rule the same call stops earlier
    assert _bwd(capi, _desc(capi, C=6), p) == EUNSUPPORTED
    # pointer alignment: after the NULL checks, before the shape rule (include/mdconv.h, "Pointer alignment") -- 2 mod 16 is
    # below the 16-byte class of the first tensor, and the descriptor is outside the shape rule as well
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, C=6), ctypes.c_void_p((p.value | 15) - 13)) == EINVAL and "input pointer must be 16-byte aligned" in capi.last_error()
        assert call(capi, _desc(capi), ctypes.c_void_p((p.value | 15) - 13)) == EINVAL   # ... and before the workspace


def _align(n):
    return (n + 255) // 256 * 256


def test_workspace_bytes(capi):
    for dtype, cdt in PAIRINGS:
        kw = dict(dtype=dtype, coord_dtype=cdt)
        for flags in (0, 1, 4, 5):
            assert _ws(capi, _desc(capi, flags=flags, **kw), 0) == 0
        full = _ws(capi, _desc(capi, **kw), 1)
        det = _ws(capi, _desc(capi, flags=capi.FLAG_DETERMINISTIC, **kw), 1)
        none = _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **kw), 1)
        # ONE segment of B*H*W lists: counters, row pointers, R*PH*PW*G*G*4 entries of 16 bytes; the sort scratch doubles them
        rows, entries = 2 * 10 * 12, 6 * 3 * 2 * 2 * 2 * 4
        assert full == _align(rows * 4) + _align((rows + 1) * 4) + _align(entries * 16)
        assert det == full + _align(entries * 16) and none == 0
        assert _ws(capi, _desc(capi, flags=capi.FLAG_DETERMINISTIC | capi.FLAG_NO_GRAD_INPUT, **kw), 1) == 0
        assert _ws(capi, _desc(capi, accumulate=0, **kw), 1) == full
        assert _ws(capi, _desc(capi, with_offset=0, **kw), 1) == full
    # independent of the coordinate type and of the channels; the adaptive rule is sized by max_grid, a fixed ratio ignores it
    sizes = {_ws(capi, _desc(capi, dtype=dt, coord_dtype=cdt, C=C), 1) for dt, cdt in PAIRINGS for C in (32, 64)}
    assert len(sizes) == 1
    assert _ws(capi, _desc(capi, ratio=0, max_grid=4), 1) == _ws(capi, _desc(capi, ratio=4, max_grid=1), 1)
    assert _ws(capi, _desc(capi, ratio=0, max_grid=4), 1) > _ws(capi, _desc(capi, ratio=0, max_grid=3), 1)
    assert _ws(capi, _desc(capi, ratio=2, max_grid=16), 1) == _ws(capi, _desc(capi, ratio=2, max_grid=1), 1)


# ---- the references ----
OVERHANG = [[0, -1.2, -0.7, 4.1, 3.5], [1, 3.7, 2.2, 9.4, 7.9], [0, 1.1, 0.9, 6.2, 5.8], [1, 0.3, 3.3, 2.9, 7.1]]
REF_CASES = {
    # a fixed ratio, rectangular bins, interleaved images, scale and gamma away from 1
    "rect": dict(B=2, C=3, H=6, W=9, PH=3, PW=2, R=5, sampling_ratio=3, spatial_scale=0.5, gamma=0.3),
    # the adaptive rule, RoIs that hang over the borders (clamps and the gate take part), large offsets
    "adaptive": dict(B=2, C=2, H=7, W=8, PH=2, PW=3, rois=OVERHANG, sampling_ratio=0, max_grid=4, gamma=0.4, offset_std=1.5),
    "no_offset": dict(B=2, C=2, H=7, W=8, PH=2, PW=2, R=4, sampling_ratio=2, with_offset=False),
}


def _geo(kw):
    return dict(output_size=(kw["PH"], kw["PW"]), spatial_scale=kw.get("spatial_scale", 1.0),
                sampling_ratio=kw.get("sampling_ratio", 0), gamma=kw.get("gamma", 0.1), max_grid=kw.get("max_grid", 8))


@pytest.mark.parametrize("name", sorted(REF_CASES))
def test_the_two_references_agree(name):
    """The explicit gather with closed-form gradients against the hat-function composition under autograd: fp64, 1e-10,
    output and both gradients, off the lattice (asserted by the generator and again here)."""
    kw = REF_CASES[name]
    inp, rois, off, go = R.make_inputs(dtype=torch.float64, seed=11, **kw)
    geo = _geo(kw)
    assert R.min_lattice_distance(rois, off, kw["B"], kw["PH"], kw["PW"], geo["spatial_scale"], geo["sampling_ratio"],
                                  geo["gamma"], geo["max_grid"]) >= R.MARGIN
    if name == "adaptive":
        g = R.geometry(rois, off, kw["B"], kw["PH"], kw["PW"], geo["spatial_scale"], 0, geo["gamma"], geo["max_grid"])
        assert len(set(g["gh"].tolist()) | set(g["gw"].tolist())) >= 3
        live = g["live_y"][:, None, None, :]
        assert bool(((g["y"] < 0) & (g["y"] > -1) & live).any()) and bool(((g["y"] < -1) & live).any())   # clamp and gate
        assert bool(((g["y"] > 6) & (g["y"] < 7) & live).any())
    a = R.droi_explicit(inp, rois, off, grad_output=go, **geo)
    b = R.droi_autograd(inp, rois, off, grad_output=go, **geo)
    for what, x, y in zip(("output", "grad_input", "grad_offset"), a, b):
        if x is None:
            assert y is None and off is None
            continue
        assert x.shape == y.shape and float(x.abs().max()) > 0, what
        err = rel_err(x, y)
        print(name, what, "%.3e" % err)
        assert err <= 1e-10, (name, what, err)


def test_explicit_reference_against_forward_differences():
    """On the lattice and in the clamped zones the closed forms are the RIGHT-sided derivative: fp64 forward differences of
    the explicit forward, offset element by offset element.  Where an axis is clamped or gated the closed form is exactly 0."""
    inp, rois, off, go, geo = R.lattice_inputs()
    g = R.geometry(rois, off, 1, 2, 2, 1.0, 2, 0.25, 8)
    y, x = g["y"], g["x"]
    assert bool((x == x.round()).any()) and bool((y == y.round()).any())                 # on the lattice
    assert bool(((x < 0) & (x >= -1)).any()) and bool((x == -1).any())                    # clamped low, the gate's edge
    assert bool(((y >= 5) & (y <= 6)).any()) and bool((y > 6).any())                     # clamped high, gated out
    out, gi, goff = R.droi_explicit(inp, rois, off, grad_output=go, **geo)
    h = 1e-6
    fd = torch.zeros_like(goff)
    for idx in [tuple(i) for i in torch.cartesian_prod(torch.arange(2), torch.arange(2), torch.arange(2)).tolist()]:
        o2 = off.clone()
        o2[(0,) + idx] += h
        fd[(0,) + idx] = ((R.droi_explicit(inp, rois, o2, **geo) - out) * go).sum() / h
    assert rel_err(goff, fd) <= 1e-8, (goff, fd)
    # bin (1, 1): every sample beyond the gate in y -> both gradients exactly zero, and so is its output
    assert float(goff[0, :, 1, 1].abs().max()) == 0.0 and float(out[0, 1, 1].abs().max()) == 0.0
    # bin (0, 1), x: samples at 2 + {0.5, 1.5} - 3 = {-0.5, 0.5}: the clamped one adds exactly nothing to d/dx -- the value
    # with only the free sample live is the same bits
    assert float(goff[0, 0, 0, 1].abs()) > 0
    # bin (1, 0), x: samples at {0.5, 1.5} - 1.5 = {-1, 0}: -1 passes the gate and is clamped (zero), 0 is on the lattice (free)
    assert float(goff[0, 0, 1, 0].abs()) > 0
    # grad_input is the transpose of the forward: <grad_input, input> == <grad_output, output>
    assert abs(float((gi * inp).sum() - (go * out).sum())) <= 1e-10


def test_invalid_and_degenerate_rois_in_the_references():
    rois = [[0, 1.0, 1.0, 4.0, 4.0], [-1, 1.0, 1.0, 4.0, 4.0], [2, 1.0, 1.0, 4.0, 4.0], [1.5, 1.0, 1.0, 4.0, 4.0],
            [float("nan"), 1.0, 1.0, 4.0, 4.0], [0, 1.0, float("inf"), 4.0, 4.0], [1, 3.0, 3.0, 2.5, 2.0]]
    inp, rois, off, go = R.make_inputs(B=2, C=2, H=6, W=6, PH=2, PW=2, rois=rois, sampling_ratio=0, max_grid=4, seed=2,
                                       dtype=torch.float64, off_lattice=False)
    for fn in (R.droi_explicit, R.droi_autograd):
        out, gi, goff = fn(inp, rois, off, (2, 2), sampling_ratio=0, max_grid=4, grad_output=go)
        assert float(out[0].abs().max()) > 0 and float(out[1:].abs().max()) == 0.0 and float(goff[1:].abs().max()) == 0.0
        assert float(gi[1].abs().max()) == 0.0 and bool(torch.isfinite(gi).all())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.float16, torch.bfloat16])
def test_make_inputs_keeps_the_margin(dtype):
    for name, kw in sorted(REF_CASES.items()):
        inp, rois, off, go = R.make_inputs(dtype=dtype, seed=5, **kw)
        geo = _geo(kw)
        assert inp.dtype == go.dtype == dtype and rois.dtype == torch.float32 and (off is None or off.dtype == dtype)
        assert R.min_lattice_distance(rois, off, kw["B"], kw["PH"], kw["PW"], geo["spatial_scale"], geo["sampling_ratio"],
                                      geo["gamma"], geo["max_grid"]) >= R.MARGIN
    with pytest.raises(AssertionError):   # a RoI whose bins are exactly 2 px tall: the adaptive grid is on the edge of ceil
        R.make_inputs(B=1, C=2, H=8, W=8, PH=2, PW=2, rois=[[0, 0.5, 0.5, 4.5, 4.9]], sampling_ratio=0, seed=1)


def test_python_surface_without_gpu():
    import modulated_deform_conv_amd as pkg
    from modulated_deform_conv_amd import droi
    for name in ("deform_roi_pool_forward", "deform_roi_pool_backward", "DeformRoIPoolFunction", "deform_roi_pool", "DeformRoIPool",
                 "DeformRoIPoolPack", "ModulatedDeformRoIPoolPack"):
        assert getattr(pkg, name) is getattr(droi, name) and name in pkg.__all__ and name in droi.__all__
    x = torch.randn(1, 4, 6, 6)
    rois = torch.tensor([[0.0, 1.0, 1.0, 4.0, 4.0]])
    off = torch.zeros(1, 2, 2, 2)
    with pytest.raises(NotImplementedError):
        droi.deform_roi_pool(x, rois, off, (2, 2))
    with pytest.raises(NotImplementedError):
        droi.DeformRoIPoolFunction.apply(x, rois, None, (2, 2), 1.0, 0, 0.1)
    with pytest.raises(NotImplementedError):
        droi.deform_roi_pool_forward(x.permute(0, 2, 3, 1).contiguous(), rois, off, (2, 2))
    with pytest.raises(NotImplementedError):
        droi.deform_roi_pool_backward(x.permute(0, 2, 3, 1).contiguous(), rois, off, torch.zeros(1, 2, 2, 4), (2, 2))
    with pytest.raises(NotImplementedError):
        droi.DeformRoIPool((2, 2))(x, rois, off)
    m = droi.DeformRoIPoolPack((2, 3), 4, deform_fc_channels=8, spatial_scale=0.5, sampling_ratio=2, gamma=0.2)
    assert sorted(m.state_dict()) == sorted("offset_fc.%d.%s" % (i, p) for i in (0, 2, 4) for p in ("weight", "bias"))
    assert m.offset_fc[0].in_features == 2 * 3 * 4 and m.offset_fc[4].out_features == 2 * 3 * 2
    assert float(m.offset_fc[4].weight.detach().abs().max()) == 0.0 == float(m.offset_fc[4].bias.detach().abs().max())
    assert float(m.offset_fc[0].weight.detach().abs().max()) > 0
    mm = droi.ModulatedDeformRoIPoolPack(2, 4, deform_fc_channels=8)
    assert sorted(mm.state_dict()) == sorted(["offset_fc.%d.%s" % (i, p) for i in (0, 2, 4) for p in ("weight", "bias")] +
                                             ["mask_fc.%d.%s" % (i, p) for i in (0, 2) for p in ("weight", "bias")])
    assert mm.output_size == (2, 2) and isinstance(mm.mask_fc[3], torch.nn.Sigmoid)
    assert float(mm.mask_fc[2].weight.detach().abs().max()) == 0.0
    for mod in (m, mm):
        with pytest.raises(NotImplementedError):
            mod(x, rois)
        with pytest.raises(ValueError):
            mod(torch.randn(1, 5, 6, 6), rois)
