"""The DCNv4 operator without a GPU (include/mdconv.h, "DCNv4 operator"): the descriptor mirror, validation and its order,
the row length, the shape rule's refusals, workspace sizing, the Python surface, the fp64 reference against the DCNv3
reference, and the surfaces that must not have moved.  Host code only: no kernel is launched."""
import ctypes

import pytest
import torch

from tests import dcnv3_ref as R3
from tests import dcnv4_ref as R
from tests.test_dcnv3_cpu import SHAPES
from tests.util import rel_err

EINVAL, ENULL, EUNSUPPORTED = -1, -2, -5


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def _desc(capi, dtype=0, coord_dtype=None, B=2, G=4, D=16, sz=(9, 8), k=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1),
          scale=1.0, remove_center=0, accumulate=1, flags=0):
    d = capi.MdconvDcnv4Desc()
    d.dtype, d.coord_dtype = dtype, dtype if coord_dtype is None else coord_dtype
    d.batch, d.groups, d.group_channels = B, G, D
    for name, v in (("in_sz", sz), ("k_sz", k), ("stride", stride), ("pad", pad), ("dil", dil)):
        setattr(d, name, (ctypes.c_int * 2)(*v))
    d.offset_scale, d.remove_center, d.accumulate, d.flags = scale, remove_center, accumulate, flags
    return d


def _fwd(capi, d, p=None):
    p = ctypes.c_void_p(0) if p is None else p
    return capi.lib().mdconv_dcnv4_forward(ctypes.byref(d), p, p, p, ctypes.c_void_p(0), ctypes.c_size_t(0), ctypes.c_void_p(0))


def _bwd(capi, d, p=None):
    p = ctypes.c_void_p(0) if p is None else p
    return capi.lib().mdconv_dcnv4_backward(ctypes.byref(d), p, p, p, p, p, ctypes.c_void_p(0), ctypes.c_size_t(0),
                                            ctypes.c_void_p(0))


def _ws(capi, d, backward):
    return capi.lib().mdconv_dcnv4_workspace_bytes(ctypes.byref(d), backward)


def _om(capi, d):
    return capi.lib().mdconv_dcnv4_offset_mask_len(ctypes.byref(d))


def test_descriptor_mirror(capi):
    assert [f[0] for f in capi.MdconvDcnv4Desc._fields_] == [
        "dtype", "coord_dtype", "batch", "groups", "group_channels", "in_sz", "k_sz", "stride", "pad", "dil", "offset_scale",
        "remove_center", "accumulate", "flags"]
    assert ctypes.sizeof(capi.MdconvDcnv4Desc) == 19 * 4
    # the DCNv3 fields, in DCNv3's order, plus the two new ones
    v3 = [f[0] for f in capi.MdconvDcnv3Desc._fields_]
    assert [f[0] for f in capi.MdconvDcnv4Desc._fields_ if f[0] not in ("coord_dtype", "remove_center")] == v3


def test_valid_descriptor_stops_at_null_pointers(capi):
    for dtype, cdt in ((capi.F32, capi.F32), (capi.F16, capi.F16), (capi.BF16, capi.BF16), (capi.F16, capi.F32),
                       (capi.BF16, capi.F32)):
        for rc in (0, 1):
            for call in (_fwd, _bwd):
                d = _desc(capi, dtype=dtype, coord_dtype=cdt, remove_center=rc)
                assert call(capi, d) == ENULL and "NULL" in capi.last_error()
    # a descriptor outside the shape rule as well: the pointer check comes first
    assert _fwd(capi, _desc(capi, D=6)) == ENULL
    # grad_input alone may be NULL with NO_GRAD_INPUT -- the others still may not
    assert _bwd(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT)) == ENULL
    # a rectangular odd kernel may lose its centre
    assert _fwd(capi, _desc(capi, k=(5, 3), pad=(2, 1), remove_center=1)) == ENULL
    assert _fwd(capi, _desc(capi, k=(1, 3), pad=(0, 1), remove_center=1)) == ENULL


@pytest.mark.parametrize("kw", [
    dict(dtype=2), dict(dtype=7), dict(dtype=1 | 0x10), dict(B=0), dict(G=0), dict(D=0), dict(sz=(0, 8)), dict(k=(3, 0)),
    dict(stride=(0, 1)), dict(dil=(1, 0)), dict(pad=(-1, 0)), dict(flags=2), dict(flags=8), dict(flags=1 | 4 | 32), dict(flags=64),
    dict(accumulate=2), dict(sz=(2, 8), pad=(0, 0)), dict(sz=(9, 3), k=(3, 3), dil=(1, 2), pad=(0, 0)), dict(scale=float("nan")),
    # the operator's own: remove_center not 0 / 1, with an even kh or kw, with a 1x1 kernel; a coord_dtype that is neither
    dict(remove_center=2), dict(remove_center=-1), dict(remove_center=1, k=(2, 3)), dict(remove_center=1, k=(3, 4)),
    dict(remove_center=1, k=(1, 1), pad=(0, 0)), dict(dtype=0, coord_dtype=1), dict(dtype=1, coord_dtype=3),
    dict(dtype=3, coord_dtype=1), dict(dtype=3, coord_dtype=2), dict(dtype=0, coord_dtype=3),
])
def test_invalid_descriptor(capi, kw):
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, **kw)) == EINVAL, kw
        assert capi.last_error()
    assert _ws(capi, _desc(capi, **kw), 1) == 0
    assert _om(capi, _desc(capi, **kw)) == -1


def test_error_order(capi):
    """descriptor (EINVAL), then pointers (ENULL), then the shape rule (EUNSUPPORTED, named), then the workspace."""
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # non-NULL; nothing dereferences it
    bad_and_unsupported = _desc(capi, D=6, remove_center=1, k=(2, 2))
    assert _fwd(capi, bad_and_unsupported) == EINVAL and _fwd(capi, bad_and_unsupported, p) == EINVAL
    unsupported = _desc(capi, D=6)
    assert _fwd(capi, unsupported) == ENULL and _fwd(capi, unsupported, p) == EUNSUPPORTED
    # pointer alignment: after the NULL checks, before the shape rule (include/mdconv.h, "Pointer alignment") -- 2 mod 16 is
    # below the 16-byte class of the first tensor, and the descriptor is outside the shape rule as well
    for call in (_fwd, _bwd):
        assert call(capi, unsupported, ctypes.c_void_p((p.value | 15) - 13)) == EINVAL and "input pointer must be 16-byte aligned" in capi.last_error()
    # a valid backward with good pointers and no workspace stops at the workspace
    assert _bwd(capi, _desc(capi), p) == -3 and "workspace" in capi.last_error().lower()


def test_valid_flags(capi):
    for flags in (0, 1, 4, 5):
        assert _fwd(capi, _desc(capi, flags=flags)) == ENULL and _bwd(capi, _desc(capi, flags=flags)) == ENULL


@pytest.mark.parametrize("G, k, rc, K, OM", [(1, (3, 3), 0, 9, 32), (4, (3, 3), 0, 9, 112), (2, (3, 3), 1, 8, 48),
                                              (3, (5, 3), 1, 14, 128), (2, (1, 1), 0, 1, 8)])
def test_offset_mask_len(capi, G, k, rc, K, OM):
    from modulated_deform_conv_amd import dcnv4
    d = _desc(capi, G=G, k=k, pad=(k[0] // 2, k[1] // 2), remove_center=rc)
    assert R.taps(k, rc) == K
    assert _om(capi, d) == OM
    assert R.row_len(G, K) == OM and dcnv4.offset_mask_len(k, G, rc) == OM
    assert capi.lib().mdconv_dcnv4_offset_mask_len(None) == -1


def test_shape_rule_refusals_come_before_any_launch(capi):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for d, word in ((_desc(capi, D=6), "multiple of 4"), (_desc(capi, dtype=capi.F16, D=4), "multiple of 8"),
                    (_desc(capi, dtype=capi.BF16, coord_dtype=capi.F32, D=12), "multiple of 8"),
                    (_desc(capi, k=(65, 64), pad=(32, 32), sz=(64, 64)), "4096"),
                    (_desc(capi, B=1 << 16, G=1 << 10, D=64), "2^31"),
                    # offset_mask alone reaches 2^31 bytes: 16 x 1024 x 1024 pixels x OM 32 x 4 bytes (input: 2^30)
                    (_desc(capi, B=16, G=1, D=16, sz=(1024, 1024)), "2^31")):
        for call in (_fwd, _bwd):
            assert call(capi, d, p) == EUNSUPPORTED, word
            assert word in capi.last_error(), capi.last_error()
        assert _ws(capi, d, 1) == 0
    # ... and with 16-bit coordinates the same call is inside the rule (it stops at the workspace, not the shape)
    ok = _desc(capi, dtype=capi.F16, B=16, G=1, D=16, sz=(1024, 1024))
    assert _fwd(capi, ok) == ENULL and _ws(capi, ok, 1) > 0


def test_out_size(capi):
    L = capi.lib()
    d = _desc(capi, sz=(17, 12), k=(5, 3), stride=(2, 2), pad=(1, 1), dil=(2, 2))
    assert (L.mdconv_dcnv4_out_size(ctypes.byref(d), 0), L.mdconv_dcnv4_out_size(ctypes.byref(d), 1)) == (6, 5)
    assert R.out_hw(17, 12, (5, 3), 2, 1, 2) == (6, 5)
    assert L.mdconv_dcnv4_out_size(ctypes.byref(d), 2) == -1 and L.mdconv_dcnv4_out_size(None, 0) == -1


def test_workspace_bytes(capi):
    for dtype in (capi.F32, capi.F16, capi.BF16):
        for flags in (0, 1, 4, 5):
            assert _ws(capi, _desc(capi, dtype=dtype, flags=flags), 0) == 0
        full = _ws(capi, _desc(capi, dtype=dtype), 1)
        det = _ws(capi, _desc(capi, dtype=dtype, flags=capi.FLAG_DETERMINISTIC), 1)
        no_gi = _ws(capi, _desc(capi, dtype=dtype, flags=capi.FLAG_NO_GRAD_INPUT), 1)
        assert full > 0 and no_gi < full and det >= full
        # the sort scratch belongs to the grad_input stages; the write mode never changes the figure
        assert _ws(capi, _desc(capi, dtype=dtype, flags=capi.FLAG_DETERMINISTIC | capi.FLAG_NO_GRAD_INPUT), 1) == no_gi
        assert _ws(capi, _desc(capi, dtype=dtype, accumulate=0), 1) == full
        # ... and neither does the coordinate type
        assert _ws(capi, _desc(capi, dtype=dtype, coord_dtype=capi.F32), 1) == full
        assert _ws(capi, _desc(capi, dtype=dtype, coord_dtype=capi.F32, flags=capi.FLAG_DETERMINISTIC), 1) == det
    # the lists do not depend on the channels of a group, and are DCNv3's for the same taps
    assert _ws(capi, _desc(capi, D=64), 1) == _ws(capi, _desc(capi, D=16), 1)
    d3 = capi.MdconvDcnv3Desc()
    d3.dtype, d3.batch, d3.groups, d3.group_channels = 0, 2, 4, 16
    for name, v in (("in_sz", (9, 8)), ("k_sz", (3, 3)), ("stride", (1, 1)), ("pad", (1, 1)), ("dil", (1, 1))):
        setattr(d3, name, (ctypes.c_int * 2)(*v))
    d3.offset_scale, d3.accumulate = 1.0, 1
    assert _ws(capi, _desc(capi), 1) == capi.lib().mdconv_dcnv3_workspace_bytes(ctypes.byref(d3), 1)
    # one tap fewer: shorter lists
    assert _ws(capi, _desc(capi, remove_center=1), 1) < _ws(capi, _desc(capi), 1)


def _split_grads(gom, G, K):
    return R.unpack(gom, G, K)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_reference_equals_the_dcnv3_reference_on_the_full_kernel(name):
    """(a) remove_center off: dcnv4_ref(pack(offset, mask)) is dcnv3_ref(offset, mask) -- output and all gradients, the
    packed gradient unpacked; fp64, 1e-10.  Two independent statements: explicit corners here, grid_sample there."""
    x, off, m, go, geo = R3.make_inputs(dtype=torch.float64, seed=11, offset_range=2.5, **SHAPES[name])
    G, K = geo[4], R.taps(geo[0])
    want = R3.dcnv3_ref_grads(x, off, m, go, *geo)
    om = R.pack(off, m, G, K)
    assert om.shape[-1] == R.row_len(G, K) and torch.equal(torch.cat(R.unpack(om, G, K), -1), torch.cat([off, m], -1))
    out, gi, gom = R.dcnv4_ref_grads(x, om, go, *geo, False)
    assert float(gom[..., G * K * 3:].abs().max() if gom.shape[-1] > G * K * 3 else 0.0) == 0.0
    for what, a, b in zip(("output", "grad_input", "grad_offset", "grad_mask"), (out, gi) + _split_grads(gom, G, K), want):
        assert a.shape == b.shape, what
        err = rel_err(a, b)
        print(name, what, "%.3e" % err)
        assert err <= 1e-10, (name, what, err)


@pytest.mark.parametrize("kernel, pad", [((3, 3), (1, 1)), ((5, 3), (2, 1))])
def test_reference_with_remove_center_equals_a_zero_centre_mask(kernel, pad):
    """(b) remove_center on: dcnv4_ref equals dcnv3_ref over the FULL grid with an arbitrary offset and a mask of exactly 0
    on the centre tap -- output, grad_input and the gradients of the other taps; fp64, 1e-10."""
    G, D, H, W = 2, 4, 7, 6
    x, om, go, geo = R.make_inputs(B=2, G=G, D=D, H=H, W=W, kernel=kernel, pad=pad, offset_scale=0.75, remove_center=True,
                                   dtype=torch.float64, seed=5, offset_range=2.5)
    K = R.taps(kernel, True)
    full = kernel[0] * kernel[1]
    centre = (full - 1) // 2
    assert K == full - 1
    off, m = R.unpack(om, G, K)
    B, Ho, Wo = om.shape[:3]
    gen = torch.Generator().manual_seed(6)
    keep = [u for u in range(full) if u != centre]
    off_full = torch.empty(B, Ho, Wo, G, full, 2, dtype=torch.float64)
    off_full[..., keep, :] = off.reshape(B, Ho, Wo, G, K, 2)
    off_full[..., centre, :] = torch.rand(B, Ho, Wo, G, 2, generator=gen, dtype=torch.float64) * 3 - 1.37   # arbitrary
    m_full = torch.zeros(B, Ho, Wo, G, full, dtype=torch.float64)
    m_full[..., keep] = m.reshape(B, Ho, Wo, G, K)
    want = R3.dcnv3_ref_grads(x, off_full.reshape(B, Ho, Wo, -1), m_full.reshape(B, Ho, Wo, -1), go, *geo[:7])
    out, gi, gom = R.dcnv4_ref_grads(x, om, go, *geo)
    goff, gm = _split_grads(gom, G, K)
    want_goff = want[2].reshape(B, Ho, Wo, G, full, 2)[..., keep, :].reshape(goff.shape)
    want_gm = want[3].reshape(B, Ho, Wo, G, full)[..., keep].reshape(gm.shape)
    for what, a, b in (("output", out, want[0]), ("grad_input", gi, want[1]), ("grad_offset", goff, want_goff),
                       ("grad_mask", gm, want_gm)):
        err = rel_err(a, b)
        print(kernel, what, "%.3e" % err)
        assert err <= 1e-10, (kernel, what, err)


def test_nan_padding_takes_no_part_in_the_reference():
    kw = dict(B=1, G=1, D=4, H=5, W=7, kernel=3, pad=1, dtype=torch.float64, seed=2)
    x, om, go, geo = R.make_inputs(**kw)
    _, om_nan, _, _ = R.make_inputs(nan_padding=True, **kw)
    assert om.shape[-1] == 32 and torch.isnan(om_nan[..., 27:]).all() and torch.equal(om[..., :27], om_nan[..., :27])
    for a, b in zip(R.dcnv4_ref_grads(x, om, go, *geo), R.dcnv4_ref_grads(x, om_nan, go, *geo)):
        assert torch.isfinite(b).all() and torch.equal(a, b)


def test_existing_surfaces_are_untouched(capi):
    assert capi.lib().mdconv_abi_version() == 2
    assert ctypes.sizeof(capi.MdconvDesc) == 132
    assert ctypes.sizeof(capi.MdconvDcnv3Desc) == 17 * 4


def test_python_surface_without_gpu():
    import modulated_deform_conv_amd as pkg
    from modulated_deform_conv_amd import dcnv4
    for name in ("DCNv4", "dcnv4_core", "DCNv4Function", "dcnv4_forward", "dcnv4_backward"):
        assert getattr(pkg, name) is getattr(dcnv4, name) and name in pkg.__all__
    x = torch.zeros(1, 4, 4, 8)
    om = torch.zeros(1, 4, 4, dcnv4.offset_mask_len(3, 2))
    with pytest.raises(NotImplementedError):
        dcnv4.dcnv4_core(x, om, 3, 1, 1, 1, 2, 4, 1.0)
    with pytest.raises(NotImplementedError):
        dcnv4.dcnv4_forward(x, om, 3, 1, 1, 1, 2, 4, 1.0)
    with pytest.raises(NotImplementedError):
        dcnv4.dcnv4_backward(x, om, x, 3, 1, 1, 1, 2, 4, 1.0)
    with pytest.raises(NotImplementedError):   # the published positional order, im2col_step and remove_center last
        dcnv4.DCNv4Function.apply(x, om, 3, 3, 1, 1, 1, 1, 1, 1, 2, 4, 1.0, 256, False)
    m = dcnv4.DCNv4(channels=16, group=2)
    assert sorted(m.state_dict()) == sorted([
        "offset_mask.weight", "offset_mask.bias", "value_proj.weight", "value_proj.bias", "output_proj.weight",
        "output_proj.bias"])
    assert m.offset_mask.out_features == 56 and float(m.offset_mask.weight.detach().abs().max()) == 0.0
    assert float(m.offset_mask.bias.detach().abs().max()) == 0.0 and float(m.value_proj.weight.detach().abs().max()) > 0.0
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 16, 16), shape=(4, 4))
    m = dcnv4.DCNv4(channels=16, group=2, dw_kernel_size=3, remove_center=True, output_bias=False)
    assert sorted(m.state_dict()) == sorted([
        "offset_mask_dw.weight", "offset_mask_dw.bias", "offset_mask.weight", "offset_mask.bias", "value_proj.weight",
        "value_proj.bias", "output_proj.weight"])
    assert m.offset_mask.out_features == 48
    m = dcnv4.DCNv4(channels=16, group=2, without_pointwise=True)
    assert sorted(m.state_dict()) == ["offset_mask.bias", "offset_mask.weight"]
    with pytest.raises(ValueError):
        dcnv4.DCNv4(channels=18, group=4)
