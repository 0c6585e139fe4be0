"""The depthwise family without a GPU (include/mdconv.h: MDCONV_PATH_DEPTHWISE = 3, MDCONV_KERNELS_DEPTHWISE = 4,
mdconv_planned_kernels): which calls the plan takes, the forced path and its refusals, the queries that answer for the route,
workspace sizing, and the names of the Python binding.  Host planning only: no kernel is launched."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def _desc(capi, nd=2, modulated=1, dtype=0, B=2, C=64, O=64, sz=(8, 8), v2=True, **kw):
    d = capi.MdconvDesc()
    d.ndim, d.modulated, d.dtype, d.batch, d.c_in, d.c_out = nd | (capi.DESC_V2 if v2 else 0), modulated, dtype, B, C, O
    d.accumulate = 1
    f = lambda v, x: tuple(v) + (x,) * (3 - nd)
    d.in_sz = (ctypes.c_int * 3)(*f(sz, 1))
    d.k_sz = (ctypes.c_int * 3)(*f((3,) * nd, 1))
    d.stride = (ctypes.c_int * 3)(1, 1, 1)
    d.pad = (ctypes.c_int * 3)(*f((1,) * nd, 0))
    d.dil = (ctypes.c_int * 3)(1, 1, 1)
    d.groups, d.dgroups, d.in_step, d.with_bias = 1, 1, 64, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _dw2d(capi, **kw):
    """fp32 MDCN2d 64 -> 64, groups = 64, 8 x 8"""
    kw.setdefault("groups", 64)
    return _desc(capi, **kw)


def _dw3d(capi, **kw):
    """fp32 DCN3d 16 -> 32, groups = 16, (5, 6, 5)"""
    kw.setdefault("groups", 16)
    return _desc(capi, nd=3, modulated=0, C=16, O=32, sz=(5, 6, 5), **kw)


DEPTHWISE = (_dw2d, _dw3d)


def _fwd_null(capi, d):
    null = ctypes.c_void_p(0)
    name = "mdconv_modulated_deform_conv2d_forward" if d.modulated else "mdconv_deform_conv3d_forward"
    args = [null] * (7 if d.modulated else 6)
    return getattr(capi.lib(), name)(ctypes.byref(d), *args, ctypes.c_size_t(0), null)


def _planned(capi, d, backward):
    return capi.lib().mdconv_planned_kernels(ctypes.byref(d), backward)


def _ws(capi, d, backward):
    return capi.lib().mdconv_workspace_bytes(ctypes.byref(d), backward)


def test_enum_values(capi):
    assert (capi.PATH_AUTO, capi.PATH_DIRECT, capi.PATH_MFMA, capi.PATH_DEPTHWISE) == (0, 1, 2, 3)
    assert capi.KERNELS[4] == "depthwise"


@pytest.mark.parametrize("make", DEPTHWISE)
def test_planned_kernels_answers_depthwise(capi, make):
    for path in (capi.PATH_AUTO, capi.PATH_DEPTHWISE):
        for backward in (0, 1):
            assert _planned(capi, make(capi, path=path), backward) == 4, (path, backward)
    assert capi.planned_kernels(make(capi), False) == "depthwise"
    assert capi.planned_kernels(make(capi), True) == "depthwise"
    # the flags never change the route; v1 descriptors route like v2 descriptors without modes
    for flags in (capi.FLAG_DETERMINISTIC, capi.FLAG_NO_GRAD_INPUT, capi.FLAG_NO_GRAD_WEIGHT, capi.FLAG_MATH_BF16, 1 | 4 | 8 | 32):
        assert _planned(capi, make(capi, flags=flags), 1) == 4, flags
    assert _planned(capi, make(capi, v2=False), 0) == 4 and _planned(capi, make(capi, v2=False), 1) == 4
    assert _planned(capi, make(capi, with_bias=1), 1) == 4


@pytest.mark.parametrize("make", DEPTHWISE)
def test_planned_kernels_of_calls_the_family_never_takes(capi, make):
    for backward in (0, 1):
        for dtype in (capi.F16, capi.BF16, capi.F64):
            assert _planned(capi, make(capi, dtype=dtype), backward) in (1, 2, 3), (dtype, backward)
        for path in (capi.PATH_MFMA, capi.PATH_DIRECT):
            assert _planned(capi, make(capi, path=path), backward) != 4, (path, backward)
    assert _planned(capi, make(capi, path=capi.PATH_DIRECT), 0) == 1


def test_planned_kernels_of_other_layers(capi):
    for backward in (0, 1):
        assert _planned(capi, _desc(capi, C=1, O=1, groups=1), backward) == 1            # the known-answer shape
        assert _planned(capi, _desc(capi, C=64, O=64, groups=32), backward) in (1, 2)    # two channels per group
        assert _planned(capi, _desc(capi, C=64, O=64, groups=1), backward) == 2
        assert _planned(capi, _desc(capi, C=64, O=64, groups=1, dtype=capi.F16), backward) == 3
        # outside the shape rule: C_in not a multiple of 4, multiplier 5, deformable groups of 2 channels, channels-last input
        assert _planned(capi, _desc(capi, C=6, O=6, groups=6), backward) != 4
        assert _planned(capi, _desc(capi, C=8, O=40, groups=8), backward) != 4
        assert _planned(capi, _desc(capi, C=8, O=8, groups=8, dgroups=4), backward) != 4
        assert _planned(capi, _dw2d(capi, input_layout=1), backward) == 0                # still refused
    assert _planned(capi, _desc(capi, C=64, O=64, groups=1, path=5), 0) == 0             # invalid descriptor
    assert _planned(capi, _desc(capi, C=64, O=64, groups=1, path=capi.PATH_DIRECT, flags=capi.FLAG_DETERMINISTIC), 1) == 0   # refused


def test_forced_path_validation_and_refusals(capi):
    for make in DEPTHWISE:
        d = make(capi, path=capi.PATH_DEPTHWISE)
        assert _fwd_null(capi, d) == -2 and "NULL" in capi.last_error()
    # not depthwise / not fp32: refused with the rule before anything is launched (the pointer check comes first in every
    # entry point, so these calls carry non-null pointers; nothing dereferences them)
    dense = _desc(capi, C=64, O=64, groups=1, path=capi.PATH_DEPTHWISE)
    half = _dw2d(capi, dtype=capi.F16, path=capi.PATH_DEPTHWISE)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for d, word in ((dense, "groups == C_in"), (half, "fp32")):
        rc = capi.lib().mdconv_modulated_deform_conv2d_forward(ctypes.byref(d), p, p, p, p, p, p, p, ctypes.c_size_t(0),
                                                               ctypes.c_void_p(0))
        assert rc == -5, rc
        err = capi.last_error()
        assert "depthwise" in err and word in err, err
        rc = capi.lib().mdconv_modulated_deform_conv2d_backward(ctypes.byref(d), *([p] * 12), ctypes.c_size_t(0), ctypes.c_void_p(0))
        assert rc == -5 and word in capi.last_error()
        assert _planned(capi, d, 0) == 0 and word in capi.last_error()
        assert _ws(capi, d, 1) == 0
    assert _fwd_null(capi, _dw2d(capi, path=5)) == -1
    assert _fwd_null(capi, _dw2d(capi, path=4)) == -1


@pytest.mark.parametrize("make", DEPTHWISE)
def test_queries_answer_for_the_route(capi, make):
    L = capi.lib()
    for path in (capi.PATH_AUTO, capi.PATH_DEPTHWISE):
        d = make(capi, path=path)
        assert L.mdconv_deterministic_supported(ctypes.byref(d), 1) == 1
        assert L.mdconv_deterministic_supported(ctypes.byref(d), 0) == 1
        for backward in (0, 1):
            assert L.mdconv_math_bf16_used(ctypes.byref(make(capi, path=path, flags=capi.FLAG_MATH_BF16)), backward) == 0
            assert L.mdconv_input_layout_supported(ctypes.byref(d), 1, backward) == 0
            assert L.mdconv_input_layout_supported(ctypes.byref(d), 0, backward) == 1


def test_workspace(capi):
    for make in DEPTHWISE:
        d = make(capi)
        weight_bytes = d.c_out * 27 * 4 if (d.ndim & 0xff) == 3 else d.c_out * 9 * 4
        assert _ws(capi, d, 0) <= weight_bytes
        full = _ws(capi, d, 1)
        assert full > 0
        no_gi = _ws(capi, make(capi, flags=capi.FLAG_NO_GRAD_INPUT), 1)
        no_gw = _ws(capi, make(capi, flags=capi.FLAG_NO_GRAD_WEIGHT), 1)
        neither = _ws(capi, make(capi, flags=capi.FLAG_NO_GRAD_INPUT | capi.FLAG_NO_GRAD_WEIGHT), 1)
        assert no_gi < full and no_gw < full and neither <= min(no_gi, no_gw)
        det = _ws(capi, make(capi, flags=capi.FLAG_DETERMINISTIC), 1)
        assert det > full
        # the sort scratch belongs to the grad_input stages
        assert _ws(capi, make(capi, flags=capi.FLAG_DETERMINISTIC | capi.FLAG_NO_GRAD_INPUT), 1) == no_gi
        assert _ws(capi, make(capi, path=capi.PATH_DEPTHWISE), 1) == full
    # what the matrix family makes of such a layer: every group padded to 16 input channels -- a workspace copy of the input
    # 16 times its size (the gap the family closes)
    big = _desc(capi, B=8, C=256, O=256, groups=256, sz=(56, 56))
    input_bytes = 8 * 256 * 56 * 56 * 4
    assert _ws(capi, _desc(capi, B=8, C=256, O=256, groups=256, sz=(56, 56), path=capi.PATH_MFMA), 0) >= 16 * input_bytes
    assert _ws(capi, big, 0) <= 256 * 9 * 4
    assert _planned(capi, big, 0) == 4 and _planned(capi, big, 1) == 4


def test_capi_names_round_trip(capi):
    prev = capi.set_path("depthwise")
    try:
        assert capi.set_path("depthwise") == "depthwise"
        # the process default reaches descriptors that name no path
        assert _planned(capi, _dw2d(capi), 0) == 4
        assert _planned(capi, _desc(capi, C=64, O=64, groups=1), 0) == 0 and "depthwise" in capi.last_error()
    finally:
        assert capi.set_path(prev) == "depthwise"
    assert capi.set_path(prev) == prev
    assert capi.KERNELS == {0: "none", 1: "direct", 2: "f32", 3: "hp", 4: "depthwise"}
    before = capi.lib().mdconv_set_path(5)   # not a path: ignored
    assert capi.lib().mdconv_set_path(before) == before


def test_size_rule_of_the_default_route(capi):
    """Several deformable groups of a multiple of 64 channels, at most 256 input channels and at least 4096 output pixels keep the
    earlier route under AUTO (measured faster there: profiles/depthwise.md); forced, the family takes them."""
    big = dict(B=8, C=256, O=256, groups=256, dgroups=4, sz=(56, 56))
    for backward in (0, 1):
        assert _planned(capi, _desc(capi, **big), backward) in (1, 2), backward
        assert _planned(capi, _desc(capi, path=capi.PATH_DEPTHWISE, **big), backward) == 4
        assert _planned(capi, _desc(capi, flags=4 | 8, **big), backward) in (1, 2)       # the flags never change the route
        assert _planned(capi, _desc(capi, **dict(big, sz=(28, 28))), backward) in (1, 2)  # 6272 pixels
        assert _planned(capi, _desc(capi, **dict(big, C=128, O=128, groups=128, dgroups=2, B=2)), backward) in (1, 2)
        # narrower groups, one deformable group, fewer pixels, more channels: taken
        for kw in (dict(dgroups=8), dict(dgroups=32), dict(dgroups=1), dict(sz=(14, 14)), dict(B=1),
                   dict(C=512, O=512, groups=512, dgroups=8), dict(C=512, O=512, groups=512, dgroups=2)):
            assert _planned(capi, _desc(capi, **dict(big, **kw)), backward) == 4, kw
