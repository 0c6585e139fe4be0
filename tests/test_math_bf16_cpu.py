"""fp32 tensors, bf16 matrix math without a GPU: the flag of the descriptor's flags word (include/mdconv.h:
MDCONV_FLAG_MATH_BF16 = 32 in ``reserved[4]``), its validation against the dtype, the routing query
``mdconv_math_bf16_used``, workspace sizing with the flag, and the Python switch (``_capi.fp32_math`` /
``_capi.fp32_math_mode``, which follows ``torch.set_float32_matmul_precision``).  Host planning only: no kernel is launched."""
import ctypes
import threading

import pytest
import torch


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


MB16 = 32


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


def _bwd_null(capi, d):
    null = ctypes.c_void_p(0)
    return capi.lib().mdconv_modulated_deform_conv2d_backward(ctypes.byref(d), *([null] * 12), ctypes.c_size_t(0), null)


def _ws(capi, d, backward):
    return capi.lib().mdconv_workspace_bytes(ctypes.byref(d), backward)


def _used(capi, d, backward):
    return capi.lib().mdconv_math_bf16_used(ctypes.byref(d), backward)


def test_flag_value_and_abi_are_pinned(capi):
    assert capi.FLAG_MATH_BF16 == MB16
    assert ctypes.sizeof(capi.MdconvDesc) == 132 and capi.lib().mdconv_abi_version() == 2
    d = _desc(capi, flags=MB16)
    assert list(d.reserved) == [0, 0, 0, 0, 32]


def test_flag_is_validated(capi):
    for flags in (32, 33, 32 | 4 | 8):
        d = _desc(capi, dtype=capi.F32, flags=flags)
        # validation passes in both directions, the calls stop at the pointers
        assert _fwd_null(capi, d) == -2 and "NULL" in capi.last_error(), flags
        assert _bwd_null(capi, d) == -2 and "NULL" in capi.last_error(), flags
    for flags in (2, 16, 32 | 2):   # what was invalid stays invalid, alone or beside the new bit
        d = _desc(capi, dtype=capi.F32, flags=flags)
        assert _fwd_null(capi, d) == -1, flags
        err = capi.last_error()
        assert "flags" in err and "MDCONV_FLAG_NO_GRAD_INPUT" in err and "MDCONV_FLAG_NO_GRAD_WEIGHT" in err \
            and "MDCONV_FLAG_DETERMINISTIC" in err, err
        assert _bwd_null(capi, d) == -1, flags
        assert _ws(capi, d, 0) == 0 and _ws(capi, d, 1) == 0, flags


def test_flag_needs_fp32_tensors(capi):
    for dtype in (capi.F16, capi.BF16, capi.F64, capi.BF16 | capi.SAMPLING_F32 | capi.WGRAD_F32):
        d = _desc(capi, dtype=dtype, flags=MB16)
        for call in (_fwd_null, _bwd_null):
            assert call(capi, d) == -1, dtype
            assert "MDCONV_FLAG_MATH_BF16" in capi.last_error(), capi.last_error()
        assert _ws(capi, d, 0) == 0 and _ws(capi, d, 1) == 0, dtype
        assert _used(capi, d, 0) == 0 and _used(capi, d, 1) == 0, dtype


def test_flag_in_a_v1_descriptor_is_ignored(capi):
    plain = _desc(capi, v2=False, sz=(56, 56))
    v1 = _desc(capi, v2=False, sz=(56, 56))
    v1.reserved = (ctypes.c_int * 5)(0, 0, 0, 0, MB16)   # beyond the end of a v1 descriptor: not read
    assert _fwd_null(capi, v1) == -2
    for backward in (0, 1):
        assert _ws(capi, v1, backward) == _ws(capi, plain, backward)
        assert _used(capi, v1, backward) == 0
    half = _desc(capi, v2=False, dtype=capi.F16)          # ... so it is nothing to refuse a 16-bit v1 call over
    half.reserved = (ctypes.c_int * 5)(0, 0, 0, 0, MB16)
    assert _fwd_null(capi, half) == -2


def _hp_takes_bf16_backward(capi, d):
    """Whether hp_plan takes the bf16 backward of `d`'s shape (C_in a multiple of 32): only then does the backward accept
    a channels-last input."""
    twin = type(d).from_buffer_copy(d)
    twin.dtype, twin.flags = capi.BF16, 0
    return capi.lib().mdconv_input_layout_supported(ctypes.byref(twin), 1, 1)


def test_routing_table(capi):
    big = dict(dtype=capi.F32, B=2, C=64, O=64, sz=(56, 56))
    d = _desc(capi, flags=MB16, **big)
    assert _used(capi, d, 0) == 1 and _used(capi, d, 1) == 1
    d = _desc(capi, flags=0, **big)
    assert _used(capi, d, 0) == 0 and _used(capi, d, 1) == 0                      # unflagged
    d = _desc(capi, dtype=capi.F32, B=1, C=4, O=4, sz=(8, 8), flags=MB16)
    assert _used(capi, d, 0) == 0 and _used(capi, d, 1) == 0                      # fewer than 16 channels
    # the size rule (measured, profiles/math_bf16.md): fewer than 16 input or 16 output channels are declined, 16 are taken,
    # and so are narrow conv groups of a wide layer
    for C, O, want in ((8, 8, 0), (8, 64, 0), (64, 8, 0), (16, 16, 1)):
        d = _desc(capi, dtype=capi.F32, B=8, C=C, O=O, sz=(56, 56), flags=MB16)
        assert _used(capi, d, 0) == want and _used(capi, d, 1) == want, (C, O)
    d = _desc(capi, dtype=capi.F32, B=8, C=256, O=256, sz=(56, 56), groups=32, dgroups=4, flags=MB16)
    assert _used(capi, d, 0) == 1 and _used(capi, d, 1) == 1
    d = _desc(capi, flags=MB16, path=capi.PATH_DIRECT, **big)
    assert _used(capi, d, 0) == 0 and _used(capi, d, 1) == 0
    d = _desc(capi, dtype=capi.F32, B=1, C=512, O=512, sz=(7, 7), flags=MB16)
    assert _used(capi, d, 0) == 0                                                 # the few-tile rule
    assert _used(capi, d, 1) == _hp_takes_bf16_backward(capi, d)
    d = _desc(capi, dtype=capi.F64, flags=MB16, B=2, C=64, O=64, sz=(56, 56))
    assert _used(capi, d, 0) == 0 and _used(capi, d, 1) == 0                      # (an invalid descriptor)
    # the other flags travel with it and do not change the answer
    for extra in (1, 4, 8, 1 | 4 | 8):
        d = _desc(capi, flags=MB16 | extra, **big)
        assert _used(capi, d, 0) == 1 and _used(capi, d, 1) == 1, extra


def _table(capi):
    return [
        _desc(capi, dtype=capi.F32, B=2, C=64, O=64, sz=(56, 56)),
        _desc(capi, dtype=capi.F32, B=2, C=64, O=64, sz=(56, 56), with_bias=1),
        _desc(capi, dtype=capi.F32, B=1, C=4, O=4, sz=(8, 8)),
        _desc(capi, dtype=capi.F32, B=2, C=64, O=64, sz=(56, 56), path=capi.PATH_DIRECT),
        _desc(capi, dtype=capi.F32, B=1, C=512, O=512, sz=(7, 7)),
        _desc(capi, dtype=capi.F32, B=2, C=512, O=64, sz=(9, 10)),
        _desc(capi, nd=3, dtype=capi.F32, B=1, C=32, O=32, sz=(4, 9, 10)),
        _desc(capi, dtype=capi.F32, B=2, C=96, O=96, sz=(12, 12), dgroups=4),
    ]


def test_workspace_sizing(capi):
    for d in _table(capi):
        for extra in (0, 1, 4, 8, 1 | 4 | 8):
            for backward in (0, 1):
                d.flags = extra
                plain = _ws(capi, d, backward)
                d.flags = extra | MB16
                flagged = _ws(capi, d, backward)
                if not _used(capi, d, backward):
                    assert flagged == plain, (d.c_in, tuple(d.in_sz), extra, backward)   # same route, same workspace
                    continue
                twin = type(d).from_buffer_copy(d)
                twin.dtype, twin.flags = capi.BF16 | capi.SAMPLING_F32 | capi.WGRAD_F32, extra
                bf16 = _ws(capi, twin, backward)
                assert flagged >= bf16 > 0, (d.c_in, tuple(d.in_sz), extra, backward)
                # the conversions add one slot: the bf16 copy of grad_output (the forward converts inside its passes)
                go16 = d.batch * d.c_out * capi.lib().mdconv_out_size(ctypes.byref(d), 0) * \
                    capi.lib().mdconv_out_size(ctypes.byref(d), 1) * capi.lib().mdconv_out_size(ctypes.byref(d), 2) * 2
                assert flagged - bf16 == ((go16 + 255) // 256 * 256 if backward else 0)


def test_query_functions_answer_for_the_route_taken(capi):
    L = capi.lib()
    for d in _table(capi):
        d.flags = 0
        det = L.mdconv_deterministic_supported(ctypes.byref(d), 1)
        d.flags = MB16
        # (every shape the bf16 kernels take is one the fp32 matrix kernels or they can run deterministically)
        assert L.mdconv_deterministic_supported(ctypes.byref(d), 1) == (1 if _used(capi, d, 1) else det)
        assert L.mdconv_deterministic_supported(ctypes.byref(d), 0) == 1
        for backward in (0, 1):   # an fp32 channels-last input stays refused
            d.flags = 0
            cl = L.mdconv_input_layout_supported(ctypes.byref(d), 1, backward)
            d.flags = MB16
            assert L.mdconv_input_layout_supported(ctypes.byref(d), 1, backward) == cl == 0
            assert L.mdconv_input_layout_supported(ctypes.byref(d), 0, backward) == 1
        d.input_layout = 1
        assert _used(capi, d, 0) == 0 and _used(capi, d, 1) == 0
        d.input_layout = 0


def test_fp32_math_nests_restores_and_is_thread_local(capi):
    prev = torch.get_float32_matmul_precision()
    try:
        torch.set_float32_matmul_precision("highest")
        assert capi.fp32_math_override() is None and capi.fp32_math_mode() == "fp32"
        with capi.fp32_math("bf16"):
            assert capi.fp32_math_mode() == "bf16"
            with capi.fp32_math("fp32"):
                assert capi.fp32_math_mode() == "fp32"
                with capi.fp32_math():
                    assert capi.fp32_math_mode() == "bf16"
                assert capi.fp32_math_mode() == "fp32"
            assert capi.fp32_math_mode() == "bf16"
            seen = []
            th = threading.Thread(target=lambda: seen.append((capi.fp32_math_override(), capi.fp32_math_mode())))
            th.start()
            th.join()
            assert seen == [(None, "fp32")]                      # another thread: not inside this block
        assert capi.fp32_math_override() is None and capi.fp32_math_mode() == "fp32"
        with pytest.raises(ValueError):
            with capi.fp32_math("bf16"):
                raise ValueError("x")
        assert capi.fp32_math_override() is None                 # restored on the way out of an exception
        with pytest.raises(ValueError):
            capi.fp32_math("fp16")                               # bf16 only: fp16 lacks fp32's exponent range
    finally:
        torch.set_float32_matmul_precision(prev)


def test_mode_follows_float32_matmul_precision(capi):
    prev = torch.get_float32_matmul_precision()
    try:
        for precision, mode in (("medium", "bf16"), ("high", "fp32"), ("highest", "fp32")):
            torch.set_float32_matmul_precision(precision)
            assert capi.fp32_math_mode() == mode, precision
        torch.set_float32_matmul_precision("medium")
        with capi.fp32_math("fp32"):                             # an explicit choice beats the global
            assert capi.fp32_math_mode() == "fp32"
        seen = []
        th = threading.Thread(target=lambda: seen.append(capi.fp32_math_mode()))   # (autograd's worker threads see the global)
        th.start()
        th.join()
        assert seen == ["bf16"]
        torch.set_float32_matmul_precision("highest")
        with capi.fp32_math("bf16"):
            assert capi.fp32_math_mode() == "bf16"
    finally:
        torch.set_float32_matmul_precision(prev)


class _Stub:
    """What MDCONV_CUDA._desc reads of a tensor."""

    def __init__(self, dtype, *shape):
        self.dtype, self.shape, self.is_cuda = dtype, torch.Size(shape), True

    def dim(self):
        return len(self.shape)


def test_desc_sets_the_flag_for_fp32_tensors_only(capi):
    from modulated_deform_conv_amd import MDCONV_CUDA

    def flags(dtype):
        d = MDCONV_CUDA._desc(2, True, _Stub(dtype, 2, 64, 9, 10), _Stub(dtype, 64, 64, 3, 3), (3, 3), (1, 1), (1, 1), (1, 1),
                              1, 1, 64, False)
        return d.flags

    prev = torch.get_float32_matmul_precision()
    try:
        torch.set_float32_matmul_precision("highest")
        assert flags(torch.float32) == 0
        with capi.fp32_math("bf16"):
            assert flags(torch.float32) == MB16
            for dtype in (torch.float16, torch.bfloat16, torch.float64):
                assert flags(dtype) == 0, dtype
            with capi.deterministic(), capi.skip_grads(input=True):
                assert flags(torch.float32) == MB16 | 1 | 4
        torch.set_float32_matmul_precision("medium")
        assert flags(torch.float32) == MB16 and flags(torch.bfloat16) == 0
        with capi.fp32_math("fp32"):
            assert flags(torch.float32) == 0
        torch.set_float32_matmul_precision("high")
        assert flags(torch.float32) == 0
    finally:
        torch.set_float32_matmul_precision(prev)
