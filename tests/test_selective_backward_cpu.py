"""Selective backward without a GPU: the two flags of the descriptor's flags word (include/mdconv.h:
MDCONV_FLAG_NO_GRAD_INPUT = 4, MDCONV_FLAG_NO_GRAD_WEIGHT = 8 in ``reserved[4]``), the pointer rule up to the pointer
check, workspace sizing with the flags, the Python switch (``_capi.skip_grads`` / ``_capi.skipped_grads``) and the fake
kernel of ``mdconv::deform_conv_backward_masked``.  Host planning only: no kernel is launched."""
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


def _bwd_null(capi, d):
    null = ctypes.c_void_p(0)
    return capi.lib().mdconv_modulated_deform_conv2d_backward(ctypes.byref(d), *([null] * 12), ctypes.c_size_t(0), null)


def test_flag_values_are_validated(capi):
    assert (capi.FLAG_DETERMINISTIC, capi.FLAG_NO_GRAD_INPUT, capi.FLAG_NO_GRAD_WEIGHT) == (1, 4, 8)
    for flags in (4, 8, 12, 1 | 4 | 8):
        d = _desc(capi, flags=flags)
        assert list(d.reserved) == [0, 0, 0, 0, flags]
        # forwards accept and ignore the flags (one descriptor serves both directions): validation passes, the call stops
        # at the pointers
        assert _fwd_null(capi, d) == -2 and "NULL" in capi.last_error(), flags
    for flags in (2, 3, 16, 6):   # 2 stays invalid, alone or beside a valid bit; 16 is unknown
        d = _desc(capi, flags=flags)
        assert _fwd_null(capi, d) == -1, flags
        err = capi.last_error()
        assert "flags" in err and "MDCONV_FLAG_NO_GRAD_INPUT" in err and "MDCONV_FLAG_NO_GRAD_WEIGHT" in err \
            and "MDCONV_FLAG_DETERMINISTIC" in err, err
        assert _bwd_null(capi, d) == -1, flags
        assert capi.lib().mdconv_workspace_bytes(ctypes.byref(d), 1) == 0, flags


def test_flags_in_a_v1_descriptor_are_ignored(capi):
    L = capi.lib()
    plain = _desc(capi, v2=False)
    for bits in (4, 8, 12, 13):
        v1 = _desc(capi, v2=False)
        v1.reserved = (ctypes.c_int * 5)(0, 0, 0, 0, bits)   # beyond the end of a v1 descriptor: not read
        assert _fwd_null(capi, v1) == -2
        for backward in (0, 1):
            assert L.mdconv_workspace_bytes(ctypes.byref(v1), backward) == L.mdconv_workspace_bytes(ctypes.byref(plain), backward)
        # the backward of a v1 descriptor requires every gradient pointer, whatever its tail holds
        assert _bwd_null(capi, v1) == -2 and "input" in capi.last_error()


def test_null_pointers_of_skipped_gradients_are_not_what_fails(capi):
    d = _desc(capi, flags=12, with_bias=1)
    assert _bwd_null(capi, d) == -2
    err = capi.last_error()
    assert "NULL" in err and "grad_input" not in err and "grad_weight" not in err and "grad_bias" not in err, err
    assert "input pointer" in err   # the first required tensor


def _ws(capi, d, flags):
    d.flags = flags
    return capi.lib().mdconv_workspace_bytes(ctypes.byref(d), 1)


def _sizing_cases(capi):
    return [
        ("fp32 64->64", _desc(capi, dtype=capi.F32)),
        ("fp16 64->64 56x56 B=32 (hp_bwd3)", _desc(capi, dtype=capi.F16, B=32, sz=(56, 56))),
        ("fp32 96->64 dg4 (padded)", _desc(capi, dtype=capi.F32, C=96, O=64, dgroups=4)),
        ("fp32 128->128 g2 dg4 (split)", _desc(capi, dtype=capi.F32, C=128, O=128, groups=2, dgroups=4)),
        ("bf16 64->64 fp32 sampling", _desc(capi, dtype=capi.BF16 | capi.SAMPLING_F32)),
        ("fp16 512->64 (fp32 copies)", _desc(capi, dtype=capi.F16, C=512, O=64, with_bias=1)),
    ]


def test_workspace_never_grows_on_the_matrix_core_routes(capi):
    for name, d in _sizing_cases(capi):
        for det in (0, capi.FLAG_DETERMINISTIC):
            full = _ws(capi, d, det)
            assert full > 0, name
            sizes = {f: _ws(capi, d, det | f) for f in (4, 8, 12)}
            for f, b in sizes.items():
                assert 0 < b <= full, (name, det, f, b, full)
            assert sizes[12] <= min(sizes[4], sizes[8]), (name, det, sizes)
            # the forward's figure does not depend on the flags
            d.flags = det
            fwd = capi.lib().mdconv_workspace_bytes(ctypes.byref(d), 0)
            d.flags = det | 12
            assert capi.lib().mdconv_workspace_bytes(ctypes.byref(d), 0) == fwd, name


def test_workspace_shrinks_where_a_stage_owns_a_slot(capi):
    hp = _desc(capi, dtype=capi.F16, B=32, sz=(56, 56))
    rows = 32 * 9 * 56 * 56 * 64 * 2                     # the column rows of hp_bwd3: B x K x S_o x C_in 16-bit values
    assert _ws(capi, hp, 0) - _ws(capi, hp, capi.FLAG_NO_GRAD_WEIGHT) >= rows
    assert _ws(capi, hp, capi.FLAG_NO_GRAD_INPUT) < _ws(capi, hp, 0)     # row pointers, entries, partial sums
    f32 = _desc(capi, dtype=capi.F32)
    det = capi.FLAG_DETERMINISTIC
    assert _ws(capi, f32, det | capi.FLAG_NO_GRAD_INPUT) < _ws(capi, f32, det)          # the sort scratch (and the lists)
    assert _ws(capi, f32, det | capi.FLAG_NO_GRAD_INPUT) == _ws(capi, f32, capi.FLAG_NO_GRAD_INPUT)   # nothing left to sort
    assert _ws(capi, f32, capi.FLAG_NO_GRAD_WEIGHT) < _ws(capi, f32, 0)                 # the split-K partials


def test_workspace_without_flags_is_unchanged_by_the_flag_word_round_trip(capi):
    for name, d in _sizing_cases(capi):
        before = _ws(capi, d, 0)
        _ws(capi, d, 12)
        twin = type(d).from_buffer_copy(d)               # differs in the flags word only
        twin.flags = 0
        assert capi.lib().mdconv_workspace_bytes(ctypes.byref(twin), 1) == before == _ws(capi, d, 0), name


def test_shape_generic_route_appends_scratch_for_an_unwanted_grad_input(capi):
    c4 = _desc(capi, modulated=0, dtype=capi.F32, B=1, C=4, O=4)
    assert _ws(capi, c4, 0) == 0
    assert _ws(capi, c4, capi.FLAG_NO_GRAD_WEIGHT) == 0
    assert _ws(capi, c4, capi.FLAG_NO_GRAD_INPUT) >= 1 * 4 * 8 * 8 * 4   # the fused data kernel scatters into it


def test_query_functions_answer_as_before(capi):
    L = capi.lib()
    for name, d in _sizing_cases(capi):
        for flags in (0, 4, 8, 12):
            d.flags = flags
            assert L.mdconv_deterministic_supported(ctypes.byref(d), 1) == 1, name
            assert L.mdconv_input_layout_supported(ctypes.byref(d), 0, 1) == 1, name
    c4 = _desc(capi, modulated=0, dtype=capi.F32, B=1, C=4, O=4, flags=12)
    assert L.mdconv_deterministic_supported(ctypes.byref(c4), 1) == 0


def test_skip_grads_nests_restores_and_is_thread_local(capi):
    assert capi.skipped_grads() == (False, False) and capi.skip_flags() == 0
    with capi.skip_grads(weight=True):
        assert capi.skipped_grads() == (False, True) and capi.skip_flags() == 8
        with capi.skip_grads(input=True):
            assert capi.skipped_grads() == (True, False) and capi.skip_flags() == 4   # the innermost block decides both
            with capi.skip_grads(input=True, weight=True):
                assert capi.skipped_grads() == (True, True) and capi.skip_flags() == 12
            with capi.skip_grads():
                assert capi.skipped_grads() == (False, False)
            assert capi.skipped_grads() == (True, False)
        assert capi.skipped_grads() == (False, True)
        seen = []
        th = threading.Thread(target=lambda: seen.append(capi.skipped_grads()))
        th.start()
        th.join()
        assert seen == [(False, False)]                          # another thread: not inside this block
    assert capi.skipped_grads() == (False, False)
    with pytest.raises(ValueError):
        with capi.skip_grads(input=True):
            raise ValueError("x")
    assert capi.skipped_grads() == (False, False)                # restored on the way out of an exception


def _meta_args(bias=True, mask=True):
    B, C, O, H, W = 2, 8, 6, 7, 9
    m = lambda *s: torch.empty(*s, device="meta")
    return dict(input=m(B, C, H, W), offset=m(B, 18, H, W), mask=m(B, 9, H, W) if mask else None, weight=m(O, C, 3, 3),
                bias=m(O) if bias else None, stride=[1, 1], padding=[1, 1], dilation=[1, 1], groups=1, deformable_groups=1,
                in_step=64)


@pytest.mark.parametrize("need_input, need_weight", [(True, True), (False, True), (True, False), (False, False)])
def test_masked_backward_fake_kernel_shapes(capi, need_input, need_weight):
    from modulated_deform_conv_amd import ops   # noqa: F401  (registers the operators)
    assert hasattr(torch.ops.mdconv, "deform_conv_backward_masked")
    for bias in (True, False):
        for mask in (True, False):
            a = _meta_args(bias, mask)
            go = torch.empty(2, 6, 7, 9, device="meta")
            gi, goff, gm, gw, gb = torch.ops.mdconv.deform_conv_backward_masked(
                go, a["input"], a["offset"], a["mask"], a["weight"], a["bias"], a["stride"], a["padding"], a["dilation"],
                a["groups"], a["deformable_groups"], a["in_step"], need_input, need_weight)
            assert gi.shape == (a["input"].shape if need_input else (0,))
            assert goff.shape == a["offset"].shape
            assert gm.shape == (a["mask"].shape if mask else (0,))
            assert gw.shape == (a["weight"].shape if need_weight else (0,))
            assert gb.shape == (a["bias"].shape if bias and need_weight else (0,))
            assert all(g.device.type == "meta" for g in (gi, goff, gm, gw, gb))
