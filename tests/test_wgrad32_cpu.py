"""fp32 weight gradients (include/mdconv.h: MDCONV_WGRAD_F32) without a GPU: descriptor validation through the C ABI, the
planning queries with the bit, and the Python plumbing (``fused_grad_buffers(dtype=)``, ``_capi.weight_grads_f32``, the
modules' keyword).  Host planning only: no kernel is launched."""
import ctypes
import threading

import pytest
import torch

from tests.test_deterministic_cpu import _cases, _desc, _fwd_null


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def test_abi_version_and_struct_unchanged(capi):
    assert capi.lib().mdconv_abi_version() == 2 == capi.ABI_VERSION
    assert ctypes.sizeof(capi.MdconvDesc) == 132
    # a bit of the dtype word beside MDCONV_SAMPLING_F32, not of the flags word (whose unknown bits stay invalid)
    assert capi.WGRAD_F32 & (capi.SAMPLING_F32 | 0xf) == 0
    d = _desc(capi, dtype=capi.F16, flags=2)
    assert _fwd_null(capi, d) == -1


@pytest.mark.parametrize("dtype", ["F16", "BF16", "F16+S32", "BF16+S32"])
def test_16bit_with_fp32_weight_gradients_passes_validation(capi, dtype):
    base, _, s32 = dtype.partition("+")
    d = _desc(capi, dtype=getattr(capi, base) | (capi.SAMPLING_F32 if s32 else 0) | capi.WGRAD_F32)
    # the forward accepts and ignores the bit (one descriptor serves both directions): stopped at the pointers
    assert _fwd_null(capi, d) == -2 and "NULL" in capi.last_error()
    null = ctypes.c_void_p(0)
    rc = capi.lib().mdconv_modulated_deform_conv2d_backward(ctypes.byref(d), *([null] * 12), ctypes.c_size_t(0), null)
    assert rc == -2 and "NULL" in capi.last_error()


@pytest.mark.parametrize("base, name", [("F32", "MDCONV_F32"), ("F64", "MDCONV_F64")])
def test_flag_is_invalid_for_wide_tensors(capi, base, name):
    assert _fwd_null(capi, _desc(capi, dtype=getattr(capi, base) | capi.WGRAD_F32)) == -1
    err = capi.last_error()
    assert "MDCONV_WGRAD_F32" in err and name in err              # a message of its own, like the sampling flag's
    assert capi.lib().mdconv_workspace_bytes(ctypes.byref(_desc(capi, dtype=getattr(capi, base) | capi.WGRAD_F32)), 1) == 0


def test_values_rejected_before_stay_rejected(capi):
    for dtype in (7, 7 | capi.WGRAD_F32, 7 | capi.SAMPLING_F32 | capi.WGRAD_F32, capi.F16 | 0x20, capi.F16 | 0x80,
                  capi.F16 | 0x04, capi.BF16 | capi.WGRAD_F32 | 0x100):
        assert _fwd_null(capi, _desc(capi, dtype=dtype)) == -1, hex(dtype)


def test_workspace_bytes_with_the_bit(capi):
    L = capi.lib()
    for base in (capi.F16, capi.BF16, capi.F16 | capi.SAMPLING_F32):
        plain, flagged = _desc(capi, dtype=base), _desc(capi, dtype=base | capi.WGRAD_F32)
        assert L.mdconv_workspace_bytes(ctypes.byref(flagged), 1) > 0                       # 64 -> 64 backward
        # the native 16-bit backward keeps its fp32 sums in the workspace either way: the same plan, the same bytes
        assert L.mdconv_workspace_bytes(ctypes.byref(flagged), 1) == L.mdconv_workspace_bytes(ctypes.byref(plain), 1)
        assert L.mdconv_workspace_bytes(ctypes.byref(flagged), 0) == L.mdconv_workspace_bytes(ctypes.byref(plain), 0)
    # the fp32 matrix family's padded plan holds grad_weight rows in the caller's element size: 2 -> 4 bytes, nothing else
    for kw in (dict(C=512, O=64, sz=(7, 6), B=1), dict(nd=3, modulated=0, C=24, O=8, sz=(4, 5, 4), groups=2, B=1)):
        plain, flagged = _desc(capi, dtype=capi.F16, **kw), _desc(capi, dtype=capi.F16 | capi.WGRAD_F32, **kw)
        b0, b1 = (L.mdconv_workspace_bytes(ctypes.byref(d), 1) for d in (plain, flagged))
        assert 0 < b0 <= b1 <= 2 * b0, (kw, b0, b1)


def test_planning_queries_do_not_depend_on_the_bit(capi):
    """The bit never changes the route: deterministic mode and the channels-last input are supported exactly where
    they are for the same call without it."""
    L = capi.lib()
    n = 0
    for name, d, want in _cases(capi):
        if d.dtype & 0xf not in (capi.F16, capi.BF16):
            continue
        n += 1
        flagged = _desc(capi)
        ctypes.memmove(ctypes.byref(flagged), ctypes.byref(d), ctypes.sizeof(d))
        flagged.dtype |= capi.WGRAD_F32
        for backward in (0, 1):
            assert L.mdconv_deterministic_supported(ctypes.byref(flagged), backward) == \
                L.mdconv_deterministic_supported(ctypes.byref(d), backward) == (want if backward else 1), name
            assert L.mdconv_input_layout_supported(ctypes.byref(flagged), 1, backward) == \
                L.mdconv_input_layout_supported(ctypes.byref(d), 1, backward), name
    assert n == 3
    # ... and on 16-bit twins of the padded / split plans of that list
    for kw in (dict(C=96, O=64, dgroups=4), dict(C=128, O=128, groups=2, dgroups=4), dict(C=4, O=4, B=1)):
        for base in (capi.F16, capi.BF16 | capi.SAMPLING_F32):
            plain, flagged = _desc(capi, dtype=base, **kw), _desc(capi, dtype=base | capi.WGRAD_F32, **kw)
            assert L.mdconv_deterministic_supported(ctypes.byref(flagged), 1) == \
                L.mdconv_deterministic_supported(ctypes.byref(plain), 1), kw
            assert (L.mdconv_workspace_bytes(ctypes.byref(flagged), 1) > 0) == \
                (L.mdconv_workspace_bytes(ctypes.byref(plain), 1) > 0), kw


def test_fused_grad_buffers_in_another_dtype():
    from modulated_deform_conv_amd.distributed import fused_grad_buffers, fused_view
    w, b = torch.zeros(6, 4, 3, 3, dtype=torch.float16), torch.zeros(6, dtype=torch.float16)
    gw, gb = fused_grad_buffers(w, b, dtype=torch.float32)
    assert gw.dtype == gb.dtype == torch.float32 and gw.shape == w.shape and gb.shape == b.shape
    flat = fused_view(gw, gb)
    assert flat is not None and flat.numel() == w.numel() + 6 and flat.dtype == torch.float32
    flat.copy_(torch.arange(flat.numel(), dtype=torch.float32))
    assert gw.view(-1)[-1].item() == w.numel() - 1 and gb[0].item() == w.numel()      # neighbours in one storage
    gw2, gb2 = fused_grad_buffers(w, None, dtype=torch.float32)
    assert gb2.numel() == 0 and fused_view(gw2, gb2).numel() == w.numel()
    # the default is unchanged: the dtype of `weight`
    gw3, gb3 = fused_grad_buffers(w, b)
    assert gw3.dtype == gb3.dtype == torch.float16 and fused_view(gw3, gb3).numel() == w.numel() + 6
    assert fused_grad_buffers(w.float(), b.float(), None)[0].dtype == torch.float32


def test_context_manager_nests_restores_and_is_thread_local(capi):
    assert capi.WGRAD_F32 == 0x40
    assert capi.weight_grads_f32_mode() is False
    with capi.weight_grads_f32():
        assert capi.weight_grads_f32_mode() is True
        with capi.weight_grads_f32(False):
            assert capi.weight_grads_f32_mode() is False
            with capi.weight_grads_f32(True):
                assert capi.weight_grads_f32_mode() is True
            assert capi.weight_grads_f32_mode() is False
        assert capi.weight_grads_f32_mode() is True
        seen = []
        th = threading.Thread(target=lambda: seen.append(capi.weight_grads_f32_mode()))
        th.start()
        th.join()
        assert seen == [False]                                   # another thread: not inside this block
        assert capi.accumulate_mode() == 1 and capi.deterministic_override() is None   # the other modes are untouched
    assert capi.weight_grads_f32_mode() is False
    with pytest.raises(ValueError):
        with capi.weight_grads_f32():
            raise ValueError("x")
    assert capi.weight_grads_f32_mode() is False                 # restored on the way out of an exception


def test_binding_sets_the_bit_from_the_gradient_dtypes(capi):
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    e = lambda dt, *s: torch.empty(*s, dtype=dt)
    for dt in (torch.float16, torch.bfloat16):
        x, gw16, gb16 = e(dt, 2, 8, 5, 5), e(dt, 8, 8, 3, 3), e(dt, 8)
        gw32, gb32 = gw16.float(), gb16.float()
        d = capi.MdconvDesc()
        d.dtype = M._DTYPES[dt]
        assert M._wgrad_f32(d, x, gw32, gb32, True) and d.dtype == M._DTYPES[dt] | capi.WGRAD_F32
        d.dtype = M._DTYPES[dt]
        assert M._wgrad_f32(d, x, gw32, e(dt, 0), False) and d.dtype & capi.WGRAD_F32   # no bias: grad_weight decides
        d.dtype = M._DTYPES[dt]
        assert not M._wgrad_f32(d, x, gw16, gb16, True) and d.dtype == M._DTYPES[dt]
        for pair in ((gw32, gb16), (gw16, gb32)):               # a mixed pair stays an error
            with pytest.raises(RuntimeError, match="fp32"):
                M._wgrad_f32(d, x, *pair, True)
    d = capi.MdconvDesc()
    d.dtype = capi.F32
    assert not M._wgrad_f32(d, e(torch.float32, 1), e(torch.float32, 1), e(torch.float32, 1), True) and d.dtype == capi.F32


def test_modules_take_weight_grad_dtype_keyword_only():
    from modulated_deform_conv_amd.modulated_deform_conv import (DeformConv3dPack, ModulatedDeformConv2d,
                                                                 ModulatedDeformConv2dPack)
    m = ModulatedDeformConv2d(8, 8, 3, padding=1, weight_grad_dtype=torch.float32)
    assert m.weight_grad_dtype == torch.float32 and m.sampling_dtype is None
    assert ModulatedDeformConv2d(8, 8, 3).weight_grad_dtype is None
    assert set(m.state_dict()) == set(ModulatedDeformConv2d(8, 8, 3).state_dict())   # checkpoints interchange
    p = ModulatedDeformConv2dPack(8, 8, 3, padding=1, sampling_dtype=torch.float32, weight_grad_dtype=torch.float32)
    assert p.weight_grad_dtype == p.sampling_dtype == torch.float32
    assert DeformConv3dPack(8, 8, 3, weight_grad_dtype=torch.float32).weight_grad_dtype == torch.float32
    for bad in (torch.float16, torch.bfloat16, torch.float64, "float32"):
        with pytest.raises(ValueError):
            ModulatedDeformConv2d(8, 8, 3, weight_grad_dtype=bad)
    with pytest.raises(TypeError):   # keyword only: the reference's positional signature is unchanged
        ModulatedDeformConv2d(8, 8, 3, 1, 0, 1, 1, 1, False, 64, None, torch.float32)
