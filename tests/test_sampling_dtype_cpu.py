"""fp32 sampling (include/mdconv.h: MDCONV_SAMPLING_F32) -- fp16 / bf16 tensors with fp32 offset, mask, grad_offset and
grad_mask: descriptor validation through the C ABI, the operator's dtype rules and its fake kernels.  No GPU needed."""
import ctypes

import pytest
import torch

import modulated_deform_conv_amd.ops as ops


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def _desc(capi, dtype, nd=2, modulated=1, c=64, o=64, size=(8, 8, 4), dgroups=1):
    d = capi.MdconvDesc()
    d.ndim, d.modulated, d.dtype, d.batch, d.c_in, d.c_out = nd | capi.DESC_V2, modulated, dtype, 2, c, o
    d.in_sz = (ctypes.c_int * 3)(*(size[:nd] + (1,) * (3 - nd)))
    d.k_sz = (ctypes.c_int * 3)(*((3,) * nd + (1,) * (3 - nd)))
    d.stride = (ctypes.c_int * 3)(1, 1, 1)
    d.pad = (ctypes.c_int * 3)(*((1,) * nd + (0,) * (3 - nd)))
    d.dil = (ctypes.c_int * 3)(1, 1, 1)
    d.groups, d.dgroups, d.in_step, d.with_bias = 1, dgroups, 64, 1
    d.accumulate, d.input_layout, d.path = 1, 0, capi.PATH_AUTO
    return d


def _forward_rc(capi, d):
    null = ctypes.c_void_p(0)
    return capi.lib().mdconv_modulated_deform_conv2d_forward(ctypes.byref(d), null, null, null, null, null, null, null,
                                                             ctypes.c_size_t(0), null)


def test_abi_version_unchanged(capi):
    assert capi.lib().mdconv_abi_version() == 2 == capi.ABI_VERSION


@pytest.mark.parametrize("base", ["F16", "BF16"])
def test_16bit_with_fp32_sampling_passes_validation(capi, base):
    d = _desc(capi, getattr(capi, base) | capi.SAMPLING_F32)
    assert _forward_rc(capi, d) == -2 and "NULL" in capi.last_error()   # valid descriptor, stopped at the pointers
    assert capi.lib().mdconv_workspace_bytes(ctypes.byref(d), 1) > 0


@pytest.mark.parametrize("base, name", [("F32", "MDCONV_F32"), ("F64", "MDCONV_F64")])
def test_fp32_sampling_flag_is_invalid_for_wide_tensors(capi, base, name):
    assert _forward_rc(capi, _desc(capi, getattr(capi, base) | capi.SAMPLING_F32)) == -1
    assert name in capi.last_error()


def test_unknown_base_dtype_stays_invalid_with_the_flag(capi):
    assert _forward_rc(capi, _desc(capi, 7 | capi.SAMPLING_F32)) == -1
    assert _forward_rc(capi, _desc(capi, capi.F16 | 0x20)) == -1


@pytest.mark.parametrize("nd, modulated", [(2, 1), (2, 0), (3, 1)])
@pytest.mark.parametrize("dgroups", [1, 2])
def test_backward_workspace_with_fp32_sampling_is_enough(capi, nd, modulated, dgroups):
    """The native 16-bit kernels read offsets / masks in place, so their plan needs at least what the 16-bit call needs."""
    L = capi.lib()
    for base in (capi.F16, capi.BF16):
        plain = _desc(capi, base, nd=nd, modulated=modulated, dgroups=dgroups)
        flagged = _desc(capi, base | capi.SAMPLING_F32, nd=nd, modulated=modulated, dgroups=dgroups)
        assert L.mdconv_workspace_bytes(ctypes.byref(flagged), 1) >= L.mdconv_workspace_bytes(ctypes.byref(plain), 1) > 0
        assert L.mdconv_input_layout_supported(ctypes.byref(flagged), 1, 1) == \
            L.mdconv_input_layout_supported(ctypes.byref(plain), 1, 1)


def test_workspace_of_the_fp32_routes_with_fp32_sampling(capi):
    """Shapes the native kernels do not take (C_in = 8: shape-generic kernels) run as fp32 calls on fp32 copies of the
    16-bit tensors: the flagged plan has room for those copies in both directions."""
    L = capi.lib()
    d = _desc(capi, capi.F16 | capi.SAMPLING_F32, c=8, o=8)
    n_x, n_w, n_o = 2 * 8 * 64, 8 * 8 * 9, 2 * 8 * 64
    assert L.mdconv_workspace_bytes(ctypes.byref(d), 0) >= 4 * (n_x + n_w + 8 + n_o)
    assert L.mdconv_workspace_bytes(ctypes.byref(d), 1) >= 4 * (2 * n_x + 2 * n_w + 16 + n_o)


def _meta_args(dtype, sdtype, mdtype=None, device="meta"):
    B, C, O, nd, K, dg = 2, 8, 6, 2, 9, 2
    osz = ops.output_size((9, 7), (3, 3), (2, 2), (1, 1), (1, 1))
    e = lambda dt, *s: torch.empty(*s, dtype=dt, device=device)
    return dict(input=e(dtype, B, C, 9, 7), offset=e(sdtype, B, dg * nd * K, *osz),
                mask=e(mdtype or sdtype, B, dg * K, *osz), weight=e(dtype, O, C // 2, 3, 3), bias=e(dtype, O),
                stride=[2, 2], padding=[1, 1], dilation=[1, 1], groups=2, deformable_groups=dg, in_step=64), osz


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_validation_accepts_16bit_tensors_with_fp32_offset_and_mask(dtype):
    a, osz = _meta_args(dtype, torch.float32)
    out = ops.deform_conv(**a)
    assert out.dtype == dtype and list(out.shape) == [2, 6] + osz
    gi, goff, gm, gw, gb = ops.deform_conv_backward(torch.empty_like(out), **a)
    assert (goff.dtype, gm.dtype) == (torch.float32, torch.float32)
    assert (gi.dtype, gw.dtype, gb.dtype) == (dtype, dtype, dtype)
    b, _ = _meta_args(dtype, torch.float32)
    b["mask"] = None
    assert ops.deform_conv(**b).dtype == dtype


@pytest.mark.parametrize("dtypes", [
    (torch.float32, torch.float16, None),      # fp32 input with a 16-bit offset
    (torch.float16, torch.float32, torch.float16),   # fp32 offset with a 16-bit mask
    (torch.float16, torch.float16, torch.float32),   # 16-bit offset with an fp32 mask
    (torch.bfloat16, torch.float64, None),     # fp64 offsets are no sampling type
    (torch.float64, torch.float32, None),
])
def test_validation_rejects_every_other_mix(dtypes):
    a, _ = _meta_args(*dtypes)
    with pytest.raises(RuntimeError, match="one dtype"):
        ops.deform_conv(**a)


def test_validation_rejects_a_16bit_weight_beside_fp32_sampling():
    a, _ = _meta_args(torch.float16, torch.float32)
    a["weight"] = a["weight"].float()
    with pytest.raises(RuntimeError, match="one dtype"):
        ops.deform_conv(**a)


def test_fake_tensor_mode_reports_the_gradient_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        a, osz = _meta_args(torch.float16, torch.float32, device="cpu")
        for n in ("input", "offset", "mask", "weight", "bias"):
            a[n].requires_grad_(True)
        out = ops.deform_conv(**a)
        assert out.dtype == torch.float16 and list(out.shape) == [2, 6] + osz
        out.sum().backward()
        assert a["offset"].grad.dtype == torch.float32 and a["mask"].grad.dtype == torch.float32
        assert a["input"].grad.dtype == torch.float16 and a["weight"].grad.dtype == torch.float16
        assert a["bias"].grad.dtype == torch.float16


def test_modules_take_sampling_dtype_keyword_only():
    from modulated_deform_conv_amd.modulated_deform_conv import (ModulatedDeformConv2d, DeformConv3dPack,
                                                                 ModulatedDeformConv2dPack)
    m = ModulatedDeformConv2d(8, 8, 3, padding=1, sampling_dtype=torch.float32)
    assert m.sampling_dtype == torch.float32
    assert ModulatedDeformConv2d(8, 8, 3).sampling_dtype is None
    # no new parameters or buffers: checkpoints interchange
    assert set(m.state_dict()) == set(ModulatedDeformConv2d(8, 8, 3).state_dict())
    p = ModulatedDeformConv2dPack(8, 8, 3, padding=1, sampling_dtype=torch.float32)
    assert set(p.state_dict()) == set(ModulatedDeformConv2dPack(8, 8, 3, padding=1).state_dict())
    assert DeformConv3dPack(8, 8, 3, sampling_dtype=torch.float32).sampling_dtype == torch.float32
    with pytest.raises(ValueError):
        ModulatedDeformConv2d(8, 8, 3, sampling_dtype=torch.float16)
    with pytest.raises(TypeError):   # keyword only: the reference's positional signature is unchanged
        ModulatedDeformConv2d(8, 8, 3, 1, 0, 1, 1, 1, False, 64, torch.float32)
