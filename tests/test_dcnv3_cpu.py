"""The DCNv3 core operator without a GPU (include/mdconv.h, "DCNv3 core operator"): descriptor validation and its order,
the shape rule's refusals, output extents, workspace sizing, the two references against each other, and the surfaces
that must not have moved.  Host code only: no kernel is launched."""
import ctypes

import pytest
import torch

from tests import dcnv3_ref as R
from tests.util import rel_err

EINVAL, ENULL, EUNSUPPORTED = -1, -2, -5


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def _desc(capi, dtype=0, B=2, G=4, D=16, sz=(9, 8), k=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1), scale=1.0,
          accumulate=1, flags=0):
    d = capi.MdconvDcnv3Desc()
    d.dtype, d.batch, d.groups, d.group_channels = dtype, B, G, D
    for name, v in (("in_sz", sz), ("k_sz", k), ("stride", stride), ("pad", pad), ("dil", dil)):
        setattr(d, name, (ctypes.c_int * 2)(*v))
    d.offset_scale, d.accumulate, d.flags = scale, accumulate, flags
    return d


def _fwd(capi, d, p=None):
    p = ctypes.c_void_p(0) if p is None else p
    return capi.lib().mdconv_dcnv3_forward(ctypes.byref(d), p, p, p, p, ctypes.c_void_p(0), ctypes.c_size_t(0), ctypes.c_void_p(0))


def _bwd(capi, d, p=None):
    p = ctypes.c_void_p(0) if p is None else p
    return capi.lib().mdconv_dcnv3_backward(ctypes.byref(d), p, p, p, p, p, p, p, ctypes.c_void_p(0), ctypes.c_size_t(0),
                                            ctypes.c_void_p(0))


def _ws(capi, d, backward):
    return capi.lib().mdconv_dcnv3_workspace_bytes(ctypes.byref(d), backward)


def test_descriptor_mirror(capi):
    assert [f[0] for f in capi.MdconvDcnv3Desc._fields_] == [
        "dtype", "batch", "groups", "group_channels", "in_sz", "k_sz", "stride", "pad", "dil", "offset_scale", "accumulate",
        "flags"]
    assert ctypes.sizeof(capi.MdconvDcnv3Desc) == 17 * 4


def test_valid_descriptor_stops_at_null_pointers(capi):
    for dtype in (capi.F32, capi.F16, capi.BF16):
        for call in (_fwd, _bwd):
            assert call(capi, _desc(capi, dtype=dtype)) == ENULL and "NULL" in capi.last_error()
    # a descriptor outside the shape rule as well: the pointer check comes first
    assert _fwd(capi, _desc(capi, D=6)) == ENULL
    # grad_input alone may be NULL with NO_GRAD_INPUT -- the others still may not
    assert _bwd(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT)) == ENULL


@pytest.mark.parametrize("kw", [
    dict(dtype=2), dict(dtype=7), dict(dtype=1 | 0x10), dict(B=0), dict(G=0), dict(D=0), dict(sz=(0, 8)), dict(k=(3, 0)),
    dict(stride=(0, 1)), dict(dil=(1, 0)), dict(pad=(-1, 0)), dict(flags=2), dict(flags=8), dict(flags=1 | 4 | 32), dict(flags=64),
    dict(accumulate=2), dict(sz=(2, 8), pad=(0, 0)), dict(sz=(9, 3), k=(3, 3), dil=(1, 2), pad=(0, 0)), dict(scale=float("nan")),
])
def test_invalid_descriptor(capi, kw):
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, **kw)) == EINVAL, kw
        assert capi.last_error()
    assert _ws(capi, _desc(capi, **kw), 1) == 0


def test_valid_flags(capi):
    for flags in (0, 1, 4, 5):
        assert _fwd(capi, _desc(capi, flags=flags)) == ENULL and _bwd(capi, _desc(capi, flags=flags)) == ENULL


def test_shape_rule_refusals_come_before_any_launch(capi):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # non-NULL; nothing dereferences it
    for d, word in ((_desc(capi, D=6), "multiple of 4"), (_desc(capi, dtype=capi.F16, D=4), "multiple of 8"),
                    (_desc(capi, dtype=capi.BF16, D=12), "multiple of 8"), (_desc(capi, k=(65, 64), pad=(32, 32), sz=(64, 64)), "4096"),
                    (_desc(capi, B=1 << 16, G=1 << 10, D=64), "2^31")):
        for call in (_fwd, _bwd):
            assert call(capi, d, p) == EUNSUPPORTED, word
            assert word in capi.last_error(), capi.last_error()
            # pointer alignment: after the NULL checks, before the shape rule (include/mdconv.h, "Pointer alignment") -- 2 mod 16 is
            # below the 16-byte class of the first tensor, and the descriptor is outside the shape rule as well
            assert call(capi, d, ctypes.c_void_p((p.value | 15) - 13)) == EINVAL and "input pointer must be 16-byte aligned" in capi.last_error()
        assert _ws(capi, d, 1) == 0


def test_out_size(capi):
    L = capi.lib()
    d = _desc(capi, sz=(17, 12), k=(5, 3), stride=(2, 2), pad=(1, 1), dil=(2, 2))
    want = tuple((n + 2 * 1 - (2 * (k - 1) + 1)) // 2 + 1 for n, k in ((17, 5), (12, 3)))
    assert want == (6, 5)
    assert (L.mdconv_dcnv3_out_size(ctypes.byref(d), 0), L.mdconv_dcnv3_out_size(ctypes.byref(d), 1)) == want
    assert R.out_hw(17, 12, (5, 3), 2, 1, 2) == want
    assert L.mdconv_dcnv3_out_size(ctypes.byref(d), 2) == -1 and L.mdconv_dcnv3_out_size(None, 0) == -1


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
    # the lists do not depend on the channels of a group
    assert _ws(capi, _desc(capi, D=64), 1) == _ws(capi, _desc(capi, D=16), 1)


SHAPES = {
    "3x3": dict(B=2, G=1, D=4, H=5, W=7, kernel=3, pad=1),
    "5x3_s2_d2_g2": dict(B=2, G=2, D=4, H=9, W=8, kernel=(5, 3), stride=2, pad=(2, 1), dilation=2, offset_scale=0.5),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_reference_agrees_with_the_oracle_mapping(name):
    """Two independent statements of the contract: grid_sample on the zero-padded input, and the oracle's depthwise
    modulated 2-D operator with unit weights and remapped offsets.  fp64, 1e-10, output and the three gradients."""
    x, off, m, go, geo = R.make_inputs(dtype=torch.float64, seed=11, offset_range=2.5, **SHAPES[name])
    ref = R.dcnv3_ref_grads(x, off, m, go, *geo)
    ora = R.dcnv3_oracle(x, off, m, go, *geo)
    for what, a, b in zip(("output", "grad_input", "grad_offset", "grad_mask"), ref, ora):
        assert a.shape == b.shape, what
        err = rel_err(a, b)
        print(name, what, "%.3e" % err)
        assert err <= 1e-10, (name, what, err)


def test_existing_surfaces_are_untouched(capi):
    assert capi.lib().mdconv_abi_version() == 2
    assert ctypes.sizeof(capi.MdconvDesc) == 132


def test_python_surface_without_gpu():
    import modulated_deform_conv_amd as pkg
    from modulated_deform_conv_amd import dcnv3
    assert pkg.DCNv3 is dcnv3.DCNv3 and pkg.dcnv3_core is dcnv3.dcnv3_core and pkg.DCNv3Function is dcnv3.DCNv3Function
    x = torch.zeros(1, 4, 4, 8)
    with pytest.raises(NotImplementedError):
        dcnv3.dcnv3_core(x, torch.zeros(1, 4, 4, 2 * 9 * 2), torch.zeros(1, 4, 4, 2 * 9), 3, 1, 1, 1, 2, 4, 1.0)
    m = dcnv3.DCNv3(channels=16, group=2)
    assert sorted(m.state_dict()) == sorted([
        "dw_conv.0.weight", "dw_conv.0.bias", "dw_conv.1.1.weight", "dw_conv.1.1.bias", "offset.weight", "offset.bias",
        "mask.weight", "mask.bias", "input_proj.weight", "input_proj.bias", "output_proj.weight", "output_proj.bias"])
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 4, 4, 16))
