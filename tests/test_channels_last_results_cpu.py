"""Channels-last results without a GPU: the two flags of the descriptor's flags word (include/mdconv.h:
MDCONV_FLAG_OUTPUT_CHANNELS_LAST = 64, MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST = 128 in ``reserved[4]``), the query
``mdconv_result_layout_supported``, workspace sizing with the flags, the Python mode (``_capi.channels_last_results``), the
modules' keyword and the binding's contiguity check.  Host planning only: no kernel is launched."""
import ctypes
import threading

import pytest
import torch


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


OUT, GI = 64, 128


def _desc(capi, nd=2, modulated=1, dtype=1, B=2, C=64, O=64, sz=(8, 8), v2=True, **kw):
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


def _ws(capi, d, flags, backward=1):
    d.flags = flags
    return capi.lib().mdconv_workspace_bytes(ctypes.byref(d), backward)


def _supported(capi, d, flags, backward):
    d.flags = flags
    return capi.lib().mdconv_result_layout_supported(ctypes.byref(d), backward)


# ---------------------------------------------------------------------------------------------- flag validation
def test_flag_values_are_accepted_for_16_bit_tensors(capi):
    assert (capi.FLAG_OUTPUT_CHANNELS_LAST, capi.FLAG_GRAD_INPUT_CHANNELS_LAST) == (OUT, GI)
    for dtype in (capi.F16, capi.BF16, capi.F16 | capi.SAMPLING_F32, capi.BF16 | capi.WGRAD_F32):
        for flags in (64, 128, 192, 64 | 1, 128 | 4, 192 | 8, 192 | 1 | 4 | 8):
            d = _desc(capi, dtype=dtype, flags=flags)
            assert list(d.reserved) == [0, 0, 0, 0, flags]
            # validation passes: the calls stop at the pointers
            assert _fwd_null(capi, d) == -2 and "NULL" in capi.last_error(), (dtype, flags, capi.last_error())
            assert _bwd_null(capi, d) == -2 and "NULL" in capi.last_error(), (dtype, flags, capi.last_error())


def test_what_was_invalid_stays_invalid(capi):
    for flags in (2, 16, 64 | 2, 128 | 16, 256):
        d = _desc(capi, flags=flags)
        assert _fwd_null(capi, d) == -1 and "flags" in capi.last_error(), flags
        assert _bwd_null(capi, d) == -1, flags
        assert capi.lib().mdconv_workspace_bytes(ctypes.byref(d), 1) == 0, flags
        assert capi.lib().mdconv_result_layout_supported(ctypes.byref(d), 1) == 0, flags


def test_flags_need_16_bit_tensors(capi):
    for dtype, extra in ((capi.F32, 0), (capi.F32, capi.FLAG_MATH_BF16), (capi.F64, 0)):
        for flag, name in ((OUT, "MDCONV_FLAG_OUTPUT_CHANNELS_LAST"), (GI, "MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST")):
            d = _desc(capi, dtype=dtype, flags=flag | extra)
            for call in (_fwd_null, _bwd_null):
                assert call(capi, d) == -1, (dtype, extra, flag)
                assert name in capi.last_error(), capi.last_error()
            assert capi.lib().mdconv_workspace_bytes(ctypes.byref(d), 1) == 0
            assert capi.lib().mdconv_result_layout_supported(ctypes.byref(d), 0) == 0
        # ... and the same descriptor without them is as valid as before
        assert _fwd_null(capi, _desc(capi, dtype=dtype, flags=extra)) == -2


def test_flags_in_a_v1_descriptor_are_ignored(capi):
    L = capi.lib()
    plain = _desc(capi, v2=False)
    for bits in (64, 128, 192, 0x7fffffff):
        v1 = _desc(capi, v2=False)
        v1.reserved = (ctypes.c_int * 5)(9, 9, 9, 9, bits)   # beyond the end of a v1 descriptor: not read
        assert _fwd_null(capi, v1) == -2
        for backward in (0, 1):
            assert L.mdconv_workspace_bytes(ctypes.byref(v1), backward) == L.mdconv_workspace_bytes(ctypes.byref(plain), backward) > 0
            assert L.mdconv_result_layout_supported(ctypes.byref(v1), backward) == 1   # it requests nothing


# ---------------------------------------------------------------------------------------------- the query
def test_query_says_yes_where_the_native_kernels_take_the_call(capi):
    cases = [
        ("fp16 64->64", _desc(capi, dtype=capi.F16)),
        ("bf16 64->64", _desc(capi, dtype=capi.BF16)),
        ("fp16 96->96 in 4 deformable groups (group-padded)", _desc(capi, dtype=capi.F16, C=96, O=96, dgroups=4)),
        ("bf16 96->96 in 4 deformable groups (group-padded)", _desc(capi, dtype=capi.BF16, C=96, O=96, dgroups=4)),
        ("fp16 3-D 32->32", _desc(capi, nd=3, dtype=capi.F16, C=32, O=32, sz=(3, 4, 5))),
        ("bf16 3-D 32->32", _desc(capi, nd=3, dtype=capi.BF16, C=32, O=32, sz=(3, 4, 5))),
    ]
    for name, d in cases:
        for flags in (0, OUT, GI, OUT | GI, OUT | GI | 1, OUT | 4, GI | 8):
            for backward in (0, 1):
                assert _supported(capi, d, flags, backward) == 1, (name, flags, backward, capi.last_error())


def test_query_says_no_with_the_rule(capi):
    o36 = _desc(capi, dtype=capi.F16, C=64, O=36)
    for backward in (0, 1):
        assert _supported(capi, o36, OUT, backward) == 0
        assert "MDCONV_FLAG_OUTPUT_CHANNELS_LAST" in capi.last_error() and "multiple of 8" in capi.last_error()
        assert _supported(capi, o36, 0, backward) == 1              # an unflagged descriptor asks for nothing
    assert _supported(capi, o36, GI, 1) == 1                         # its grad_input rows are fine
    c36 = _desc(capi, dtype=capi.F16, C=36, O=64)
    assert _supported(capi, c36, GI, 1) == 0
    assert "MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST" in capi.last_error() and "multiple of 8" in capi.last_error()
    assert _supported(capi, c36, GI, 0) == 1                         # forwards accept and ignore the flag
    assert _supported(capi, c36, GI | capi.FLAG_NO_GRAD_INPUT, 1) == 1   # nothing to do
    direct = _desc(capi, dtype=capi.F16, path=capi.PATH_DIRECT)
    for flags in (OUT, GI):
        assert _supported(capi, direct, flags, 1) == 0 and "native 16-bit kernels" in capi.last_error()
    assert _supported(capi, direct, OUT, 0) == 0


def test_query_follows_the_route_of_each_direction(capi):
    # 512 input channels: the native backward does not take them (one workgroup covers all input channels), the call runs
    # through fp32 copies; the forward of a large grid is native
    wide = _desc(capi, dtype=capi.F16, C=512, O=64, sz=(56, 56))
    assert _supported(capi, wide, OUT | GI, 1) == 0 and "native 16-bit kernels" in capi.last_error()
    assert _supported(capi, wide, OUT, 0) == 1
    # ... and the forward of a few pixel tiles over many K stages runs on the fp32 kernels too
    few = _desc(capi, dtype=capi.F16, C=512, O=512, sz=(7, 7), B=16)
    assert _supported(capi, few, OUT, 0) == 0


def test_refused_calls_return_eunsupported_before_the_pointers_matter(capi):
    # (pointers are checked first, so this needs non-NULL pointers: any address will do, nothing is launched)
    d = _desc(capi, dtype=capi.F16, C=64, O=36, flags=OUT)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    L = capi.lib()
    rc = L.mdconv_modulated_deform_conv2d_forward(ctypes.byref(d), p, p, p, p, p, p, ctypes.c_void_p(0), ctypes.c_size_t(0),
                                                  ctypes.c_void_p(0))
    assert rc == -5 and "MDCONV_FLAG_OUTPUT_CHANNELS_LAST" in capi.last_error(), (rc, capi.last_error())
    rc = L.mdconv_modulated_deform_conv2d_backward(ctypes.byref(d), *([p] * 11), ctypes.c_void_p(0), ctypes.c_size_t(0),
                                                   ctypes.c_void_p(0))
    assert rc == -5 and "MDCONV_FLAG_OUTPUT_CHANNELS_LAST" in capi.last_error(), (rc, capi.last_error())


# ---------------------------------------------------------------------------------------------- workspace
def _align(n):
    return (n + 255) // 256 * 256


def _sizing_cases(capi):
    # (name, descriptor, images of the full chunk)
    return [
        ("fp16 64->64", _desc(capi, dtype=capi.F16), 2),
        ("bf16 64->40 9x7 B=3", _desc(capi, dtype=capi.BF16, O=40, B=3, sz=(9, 7)), 3),
        ("fp16 64->64 56x56 B=32 (hp_bwd3)", _desc(capi, dtype=capi.F16, B=32, sz=(56, 56)), 32),
        ("fp16 96->96 dg4 (group-padded)", _desc(capi, dtype=capi.F16, C=96, O=96, dgroups=4), 2),
        ("bf16 3-D 32->32", _desc(capi, nd=3, dtype=capi.BF16, C=32, O=32, sz=(3, 4, 5)), 2),
        # one image's channels-last input copy is 512 x 512 x 256 x 2 bytes = 128 MiB, the chunk ceiling 0x7e000000: chunks of
        # 15 images, B = 17 leaves a tail of 2 -- two chunk sizes, the slot is the full chunk's
        ("fp16 256->256 512x512 B=17 (two chunk sizes)", _desc(capi, dtype=capi.F16, C=256, O=256, B=17, sz=(512, 512)), 15),
    ]


def test_workspace_forward_unchanged_backward_grows_by_one_chunk_of_grad_output(capi):
    for name, d, bc in _sizing_cases(capi):
        for extra in (0, 1, 4, 8, 1 | 4 | 8):
            fwd = _ws(capi, d, extra, 0)
            assert fwd > 0, name
            for flags in (OUT, GI, OUT | GI):
                assert _ws(capi, d, extra | flags, 0) == fwd, (name, extra, flags)
            plain = _ws(capi, d, extra, 1)
            assert plain > 0, name
            s_o = 1
            for a in range(d.ndim & 0xff):
                s_o *= capi.lib().mdconv_out_size(ctypes.byref(d), a)
            grow = _align(bc * d.c_out * s_o * 2)
            assert _ws(capi, d, extra | OUT, 1) == plain + grow, (name, extra)
            assert _ws(capi, d, extra | GI, 1) == plain, (name, extra)
            assert _ws(capi, d, extra | OUT | GI, 1) == plain + grow, (name, extra)


def test_two_chunk_sizes_case_really_is_chunked(capi):
    # the same layer at B = 15 is one chunk: its whole grad_output is the slot; at B = 17 the slot did not grow with B
    one = _desc(capi, dtype=capi.F16, C=256, O=256, B=15, sz=(512, 512))
    two = _desc(capi, dtype=capi.F16, C=256, O=256, B=17, sz=(512, 512))
    assert _ws(capi, one, OUT) - _ws(capi, one, 0) == _ws(capi, two, OUT) - _ws(capi, two, 0) == 15 * 256 * 512 * 512 * 2


def test_sampling_and_wgrad_flags_do_not_change_the_growth(capi):
    for dtype in (capi.F16 | capi.SAMPLING_F32, capi.BF16 | capi.WGRAD_F32, capi.F16 | capi.SAMPLING_F32 | capi.WGRAD_F32):
        d = _desc(capi, dtype=dtype, B=3, sz=(9, 7))
        assert _ws(capi, d, OUT) == _ws(capi, d, 0) + _align(3 * 64 * 63 * 2)
        assert _ws(capi, d, GI) == _ws(capi, d, 0)


# ---------------------------------------------------------------------------------------------- Python
def test_mode_is_off_by_default_nests_and_is_thread_local(capi):
    assert capi.channels_last_results_mode() is False
    with capi.channels_last_results():
        assert capi.channels_last_results_mode() is True
        with capi.channels_last_results(False):
            assert capi.channels_last_results_mode() is False
            with capi.channels_last_results(True):
                assert capi.channels_last_results_mode() is True
            assert capi.channels_last_results_mode() is False
        assert capi.channels_last_results_mode() is True
        seen = []
        th = threading.Thread(target=lambda: seen.append(capi.channels_last_results_mode()))
        th.start()
        th.join()
        assert seen == [False]                                   # another thread: not inside this block
    assert capi.channels_last_results_mode() is False
    with pytest.raises(ValueError):
        with capi.channels_last_results():
            raise ValueError("x")
    assert capi.channels_last_results_mode() is False            # restored on the way out of an exception


def test_module_keyword(capi):
    from modulated_deform_conv_amd import modulated_deform_conv as pkg
    names = ("DeformConv2d", "ModulatedDeformConv2d", "DeformConv3d", "ModulatedDeformConv3d", "DeformConv2dPack",
             "ModulatedDeformConv2dPack", "DeformConv3dPack", "ModulatedDeformConv3dPack")
    for name in names:
        cls = getattr(pkg, name)
        plain = cls(8, 8, 3, padding=1)
        assert plain.channels_last_results is False
        on = cls(8, 8, 3, padding=1, channels_last_results=True)
        assert on.channels_last_results is True
        # no new parameters or buffers, the same repr
        assert [k for k, _ in on.state_dict().items()] == [k for k, _ in plain.state_dict().items()]
        assert on.extra_repr() == plain.extra_repr() and "channels_last" not in repr(on)
        for bad in (1, "yes", None, torch.channels_last):
            with pytest.raises(ValueError):
                cls(8, 8, 3, padding=1, channels_last_results=bad)
        with pytest.raises(TypeError):
            cls(8, 8, 3, 1, 1, 1, 1, 1, False, 64, None, None, True)   # keyword only


def test_check_contig_accepts_channels_last_results_inside_the_mode_only(capi):
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    cl4 = torch.empty(2, 16, 5, 6, dtype=torch.float16, device="meta").contiguous(memory_format=torch.channels_last)
    cl5 = torch.empty(2, 16, 3, 5, 6, dtype=torch.bfloat16, device="meta").contiguous(memory_format=torch.channels_last_3d)
    assert not cl4.is_contiguous() and not cl5.is_contiguous()
    for name in ("output", "grad_output", "grad_input"):
        for t in (cl4, cl5):
            with pytest.raises(RuntimeError, match="%s tensor has to be contiguous" % name):
                M._check_contig(**{name: t})
            with capi.channels_last_results():
                M._check_contig(**{name: t})
                with capi.channels_last_results(False):
                    with pytest.raises(RuntimeError, match="has to be contiguous"):
                        M._check_contig(**{name: t})
    with capi.channels_last_results():
        # every other tensor keeps its layout, fp32 results too, and a strided view is still refused
        for name in ("offset", "mask", "weight", "grad_offset", "grad_mask", "grad_weight"):
            with pytest.raises(RuntimeError, match="has to be contiguous"):
                M._check_contig(**{name: cl4})
        with pytest.raises(RuntimeError, match="has to be contiguous"):
            M._check_contig(output=cl4.float())
        with pytest.raises(RuntimeError, match="has to be contiguous"):
            M._check_contig(output=torch.empty(2, 16, 5, 12, dtype=torch.float16, device="meta")[..., ::2])
