"""The host's match rule of the canonical-geometry instances (mdconv_common.hpp: geom_is_canon3x3, through
mdconv_geometry_is_canonical) without a GPU: a standard DCNv2 layer matches, every single deviation from it does not."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def _desc(capi, nd=2, modulated=1, B=2, C=256, O=256, sz=(9, 10), k=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1), **kw):
    d = capi.MdconvDesc()
    d.ndim, d.modulated, d.dtype, d.batch, d.c_in, d.c_out = nd | capi.DESC_V2, modulated, capi.F32, B, C, O
    d.accumulate = 1
    f = lambda v, x: tuple(v) + (x,) * (3 - nd)
    d.in_sz = (ctypes.c_int * 3)(*f(sz, 1))
    d.k_sz = (ctypes.c_int * 3)(*f(k, 1))
    d.stride = (ctypes.c_int * 3)(*f(stride, 1))
    d.pad = (ctypes.c_int * 3)(*f(pad, 0))
    d.dil = (ctypes.c_int * 3)(*f(dil, 1))
    d.groups, d.dgroups, d.in_step, d.with_bias = 1, 1, 64, 1
    for name, v in kw.items():
        setattr(d, name, v)
    return d


def _canonical(capi, d):
    return capi.lib().mdconv_geometry_is_canonical(ctypes.byref(d))


@pytest.mark.parametrize("kw", [dict(), dict(C=32, O=160, sz=(8, 37)), dict(C=48, O=24, sz=(2, 2), B=1), dict(with_bias=0)])
def test_a_standard_layer_matches(capi, kw):
    assert _canonical(capi, _desc(capi, **kw)) == 1


@pytest.mark.parametrize("kw", [
    dict(stride=(2, 2)), dict(stride=(1, 2)), dict(dil=(2, 2), pad=(2, 2)), dict(dil=(1, 2), pad=(1, 2)), dict(pad=(0, 0)),
    dict(pad=(1, 0)), dict(pad=(2, 2)), dict(k=(1, 3), pad=(0, 1)), dict(k=(3, 1), pad=(1, 0)), dict(k=(5, 5), pad=(2, 2)),
    dict(k=(1, 9), pad=(0, 4)), dict(groups=2), dict(dgroups=2), dict(modulated=0),
    dict(nd=3, sz=(5, 6, 5), k=(3, 3, 3), stride=(1, 1, 1), pad=(1, 1, 1), dil=(1, 1, 1)),
], ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()).replace(" ", ""))
def test_any_other_geometry_does_not(capi, kw):
    assert _canonical(capi, _desc(capi, **kw)) == 0


def test_an_invalid_descriptor_does_not(capi):
    assert _canonical(capi, _desc(capi, C=0)) == 0


def test_binding_names(capi):
    assert capi.last_geometry() in ("runtime", "canon3x3")
    assert "mdconv_last_geometry" in capi.EXPORTS and "mdconv_geometry_is_canonical" in capi.EXPORTS
