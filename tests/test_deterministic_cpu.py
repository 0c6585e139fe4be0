"""Deterministic mode without a GPU: the flag word of the descriptor (include/mdconv.h: MDCONV_FLAG_DETERMINISTIC in
``reserved[4]``), the routing query ``mdconv_deterministic_supported``, workspace sizing with the flag, and the Python
switches (``_capi.deterministic`` / ``_capi.deterministic_mode``).  Host planning only: no kernel is launched."""
import ctypes
import threading

import pytest
import torch


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


def _fwd_null(capi, d):
    null = ctypes.c_void_p(0)
    return capi.lib().mdconv_modulated_deform_conv2d_forward(ctypes.byref(d), null, null, null, null, null, null, null,
                                                             ctypes.c_size_t(0), null)


def test_flag_word_is_validated(capi):
    assert capi.FLAG_DETERMINISTIC == 1
    assert ctypes.sizeof(capi.MdconvDesc) == 132 and capi.lib().mdconv_abi_version() == 2
    d = _desc(capi)
    assert d.flags == 0 and list(d.reserved) == [0] * 5          # a fresh descriptor requests nothing
    d.flags = capi.FLAG_DETERMINISTIC
    assert list(d.reserved) == [0, 0, 0, 0, 1]                  # the flags word IS the last reserved slot
    assert _fwd_null(capi, d) == -2 and "NULL" in capi.last_error()   # passed validation, stopped at the pointers
    d.flags = 2
    assert _fwd_null(capi, d) == -1
    assert "reserved" in capi.last_error() or "flags" in capi.last_error()
    d.flags = 3
    assert _fwd_null(capi, d) == -1
    for slot in range(4):                                        # the other slots stay reserved
        r = _desc(capi, flags=1)
        r.reserved[slot] = 1
        assert _fwd_null(capi, r) == -1 and "reserved" in capi.last_error()


def test_flag_in_a_v1_descriptor_is_ignored(capi):
    L = capi.lib()
    # the tail of a v1 descriptor is not part of it: garbage there (flag bits, unknown bits) is neither read nor refused
    v1 = _desc(capi, v2=False, C=4, O=4)
    v1.reserved = (ctypes.c_int * 5)(9, 9, 9, 9, 0x7fffffff)
    assert _fwd_null(capi, v1) == -2
    plain = _desc(capi, v2=False, C=4, O=4)
    assert L.mdconv_workspace_bytes(ctypes.byref(v1), 1) == L.mdconv_workspace_bytes(ctypes.byref(plain), 1)
    # ... so a C = 4 backward (shape-generic kernels) is not refused for it: it stops at the pointers like any other call
    null = ctypes.c_void_p(0)
    rc = L.mdconv_modulated_deform_conv2d_backward(ctypes.byref(v1), *([null] * 12), ctypes.c_size_t(0), null)
    assert rc == -2 and "NULL" in capi.last_error()
    # and a 64-channel v1 backward plans exactly what it planned before
    w1 = _desc(capi, v2=False)
    w1.reserved = (ctypes.c_int * 5)(0, 0, 0, 0, 1)
    assert L.mdconv_workspace_bytes(ctypes.byref(w1), 1) == L.mdconv_workspace_bytes(ctypes.byref(_desc(capi, v2=False)), 1)


def _cases(capi):
    """(name, descriptor, deterministic backward supported)"""
    return [
        ("fp32 mdcn2d 64->64", _desc(capi, dtype=capi.F32), 1),
        ("fp16 mdcn2d 64->64", _desc(capi, dtype=capi.F16), 1),
        ("bf16 mdcn2d 64->64, fp32 sampling", _desc(capi, dtype=capi.BF16 | capi.SAMPLING_F32), 1),
        ("fp32 direct path", _desc(capi, dtype=capi.F32, path=capi.PATH_DIRECT), 0),
        ("fp16 direct path", _desc(capi, dtype=capi.F16, path=capi.PATH_DIRECT), 0),
        # BASELINE.json configs[0]: DeformConv2d 3x3, C_in = C_out = 4, 8 x 8, B = 1
        ("fp32 dcn2d c4", _desc(capi, modulated=0, dtype=capi.F32, B=1, C=4, O=4), 0),
        ("fp64 mdcn2d 64->64", _desc(capi, dtype=capi.F64), 0),
        ("fp64 dcn3d 16->16", _desc(capi, nd=3, modulated=0, dtype=capi.F64, C=16, O=16, sz=(5, 6, 5)), 0),
        ("fp32 dcn3d 16->16", _desc(capi, nd=3, modulated=0, dtype=capi.F32, C=16, O=16, sz=(5, 6, 5)), 1),
        # padded and split plans of the fp32 matrix-core backward
        ("fp32 96->64 dg4 (padded)", _desc(capi, dtype=capi.F32, C=96, O=64, dgroups=4), 1),
        ("fp32 128->128 g2 dg4 (split)", _desc(capi, dtype=capi.F32, C=128, O=128, groups=2, dgroups=4), 1),
    ]


def test_deterministic_supported_follows_the_routing(capi):
    L = capi.lib()
    for name, d, want in _cases(capi):
        for flags in (0, capi.FLAG_DETERMINISTIC):               # the query does not need the flag in the descriptor
            d.flags = flags
            assert L.mdconv_deterministic_supported(ctypes.byref(d), 1) == want, name
            if not want:
                err = capi.last_error()
                assert "deterministic" in err and "floating-point atomics" in err, (name, err)
            assert L.mdconv_deterministic_supported(ctypes.byref(d), 0) == 1, name   # every forward
    bad = _desc(capi, flags=2)
    assert L.mdconv_deterministic_supported(ctypes.byref(bad), 1) == 0               # invalid descriptor


def test_refusal_names_the_shape_rule(capi):
    L = capi.lib()
    null = ctypes.c_void_p(0)
    dummy = ctypes.c_void_p(256)   # non-NULL tensors: the refusal comes after the pointer checks, before any launch

    def bwd(d, fn):
        n = 9 if not d.modulated else 11
        return getattr(L, fn)(ctypes.byref(d), *([dummy] * n), null, ctypes.c_size_t(0), null)
    c4 = _desc(capi, modulated=0, dtype=capi.F32, B=1, C=4, O=4, flags=1)
    assert bwd(c4, "mdconv_deform_conv2d_backward") == -5          # MDCONV_EUNSUPPORTED
    err = capi.last_error()
    assert "deterministic" in err and "floating-point atomics" in err and "C_in" in err
    f64 = _desc(capi, dtype=capi.F64, flags=1)
    assert bwd(f64, "mdconv_modulated_deform_conv2d_backward") == -5 and "fp64" in capi.last_error()
    direct = _desc(capi, dtype=capi.F32, path=capi.PATH_DIRECT, flags=1)
    assert bwd(direct, "mdconv_modulated_deform_conv2d_backward") == -5 and "MDCONV_PATH_DIRECT" in capi.last_error()


def test_workspace_bytes_honours_the_flag(capi):
    L = capi.lib()
    grew = 0
    for name, d, want in _cases(capi):
        d.flags = 0
        b0, f0 = L.mdconv_workspace_bytes(ctypes.byref(d), 1), L.mdconv_workspace_bytes(ctypes.byref(d), 0)
        d.flags = capi.FLAG_DETERMINISTIC
        b1, f1 = L.mdconv_workspace_bytes(ctypes.byref(d), 1), L.mdconv_workspace_bytes(ctypes.byref(d), 0)
        assert b1 >= b0, name
        assert f1 == f0, name                                    # the forward has nothing to sort (0 stays 0)
        if not want:
            assert b1 == b0, name                                # nothing to sort on the shape-generic kernels either
        grew += b1 > b0
    assert grew >= 4   # the matrix-core backwards carry the sort's scratch
    fwd0 = _desc(capi, modulated=0, dtype=capi.F32, B=1, C=4, O=4, flags=1)
    assert L.mdconv_workspace_bytes(ctypes.byref(fwd0), 0) == 0


def test_context_manager_nests_restores_and_is_thread_local(capi):
    assert capi.deterministic_override() is None
    with capi.deterministic():
        assert capi.deterministic_mode() is True
        with capi.deterministic(False):
            assert capi.deterministic_mode() is False
            with capi.deterministic(True):
                assert capi.deterministic_mode() is True
            assert capi.deterministic_mode() is False
        assert capi.deterministic_mode() is True
        seen = []
        th = threading.Thread(target=lambda: seen.append((capi.deterministic_override(), capi.deterministic_mode())))
        th.start()
        th.join()
        assert seen == [(None, False)]                           # another thread: not inside this block
    assert capi.deterministic_override() is None and capi.deterministic_mode() is False
    with pytest.raises(ValueError):
        with capi.deterministic():
            raise ValueError("x")
    assert capi.deterministic_override() is None                 # restored on the way out of an exception


def test_mode_follows_the_torch_global(capi):
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        assert capi.deterministic_mode() is False
        torch.use_deterministic_algorithms(True)
        assert capi.deterministic_mode() is True
        seen = []
        th = threading.Thread(target=lambda: seen.append(capi.deterministic_mode()))   # e.g. an autograd worker thread
        th.start()
        th.join()
        assert seen == [True]
        with capi.deterministic(False):
            assert capi.deterministic_mode() is False            # the context manager wins
        torch.use_deterministic_algorithms(True, warn_only=True)
        assert capi.deterministic_mode() is True
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)
    assert capi.deterministic_mode() is prev
