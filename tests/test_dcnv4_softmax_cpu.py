"""The DCNv4 operator's in-kernel softmax without a GPU (include/mdconv.h, MDCONV_FLAG_SOFTMAX): where the flag is valid and
where it is refused, workspace sizing against the unflagged figure, the fp64 reference against the DCNv3 reference behind a
softmax, and the Python surface -- ``softmax=`` keywords, ``DCNv3Fused`` and its row index.  Host code only: no kernel is
launched."""
import ctypes

import pytest
import torch

from tests import dcnv3_ref as R3
from tests import dcnv4_ref as R
from tests import dcnv4_softmax_ref as RS
from tests import test_dcnv3_cpu as T3
from tests import test_fda_cpu as TF
from tests import test_msda_cpu as TM
from tests.test_dcnv3_cpu import SHAPES
from tests.test_dcnv4_cpu import _bwd, _desc, _fwd, _ws
from tests.util import rel_err

EINVAL, ENULL = -1, -2
SOFTMAX = 256


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def test_flag_mirror(capi):
    assert capi.FLAG_SOFTMAX == SOFTMAX


def test_flag_is_valid_for_dcnv4(capi):
    """Alone and with DETERMINISTIC (1) and NO_GRAD_INPUT (4) a call reaches the pointer check, forward and backward."""
    for flags in (SOFTMAX, SOFTMAX | 1, SOFTMAX | 4, SOFTMAX | 5):
        for dtype, cdt in ((capi.F32, capi.F32), (capi.BF16, capi.BF16), (capi.F16, capi.F32)):
            d = _desc(capi, dtype=dtype, coord_dtype=cdt, flags=flags)
            assert _fwd(capi, d) == ENULL and "NULL" in capi.last_error()
            assert _bwd(capi, d) == ENULL and "NULL" in capi.last_error()
    assert _fwd(capi, _desc(capi, flags=SOFTMAX, remove_center=1)) == ENULL


@pytest.mark.parametrize("other", [2, 8, 16, 32, 64, 128, 512, 1 << 30])
def test_flag_with_an_unknown_bit_is_invalid(capi, other):
    for flags in (SOFTMAX | other, SOFTMAX | 1 | 4 | other):
        for call in (_fwd, _bwd):
            assert call(capi, _desc(capi, flags=flags)) == EINVAL
            assert "unknown bits" in capi.last_error()
        assert _ws(capi, _desc(capi, flags=flags), 1) == 0


def test_other_descriptors_refuse_the_flag(capi):
    for T in (T3, TM, TF):
        for flags in (SOFTMAX, SOFTMAX | 1, SOFTMAX | 4):
            d = T._desc(capi, flags=flags)
            assert T._fwd(capi, d) == EINVAL and T._bwd(capi, d) == EINVAL, T.__name__
            assert T._ws(capi, d, 1) == 0
        assert T._fwd(capi, T._desc(capi)) == ENULL
    # the flags word of the convolution descriptor as well
    from tests import test_deterministic_cpu as TD
    assert TD._fwd_null(capi, TD._desc(capi, flags=1)) == ENULL
    assert TD._fwd_null(capi, TD._desc(capi, flags=SOFTMAX)) == EINVAL
    assert TD._fwd_null(capi, TD._desc(capi, flags=SOFTMAX | 1)) == EINVAL


def _slot(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("kw", [dict(), dict(B=1, G=1, D=8, sz=(5, 7)), dict(remove_center=1), dict(B=3, G=3, sz=(6, 5), k=(5, 3), pad=(2, 1), stride=(2, 2)),
                                dict(B=1, G=2, D=64, sz=(4, 4), k=(1, 1), pad=(0, 0))])
def test_workspace_bytes(capi, kw):
    """Backward with grad_input: the unflagged figure plus 8 bytes per (output pixel, group), rounded up to a 256-byte slot.
    NO_GRAD_INPUT: 0.  Forward: 0.  The unflagged figures are those of a descriptor that never heard of the flag."""
    L = capi.lib()
    for dtype, cdt in ((capi.F32, None), (capi.F16, None), (capi.BF16, capi.F32)):
        plain = _desc(capi, dtype=dtype, coord_dtype=cdt, **kw)
        ho, wo = (L.mdconv_dcnv4_out_size(ctypes.byref(plain), a) for a in (0, 1))
        stats = _slot(8 * plain.batch * ho * wo * plain.groups)
        assert stats > 0
        for extra in (0, capi.FLAG_DETERMINISTIC):
            base = _ws(capi, _desc(capi, dtype=dtype, coord_dtype=cdt, flags=extra, **kw), 1)
            soft = _ws(capi, _desc(capi, dtype=dtype, coord_dtype=cdt, flags=extra | SOFTMAX, **kw), 1)
            assert base > 0 and soft == base + stats, (kw, extra, base, soft, stats)
            assert _ws(capi, _desc(capi, dtype=dtype, coord_dtype=cdt, flags=extra | SOFTMAX | capi.FLAG_NO_GRAD_INPUT, **kw), 1) == 0
            assert _ws(capi, _desc(capi, dtype=dtype, coord_dtype=cdt, flags=extra | SOFTMAX, **kw), 0) == 0
            assert _ws(capi, _desc(capi, dtype=dtype, coord_dtype=cdt, flags=extra | SOFTMAX, accumulate=0, **kw), 1) == soft
    # the unflagged figure itself is DCNv3's for the same taps, as before (the full kernel only)
    if not kw.get("remove_center"):
        d4 = _desc(capi, **kw)
        d3 = T3._desc(capi, **{k: v for k, v in kw.items()})
        assert _ws(capi, d4, 1) == T3._ws(capi, d3, 1)


def test_workspace_stops_a_backward_with_good_pointers(capi):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # non-NULL; nothing dereferences it
    assert _bwd(capi, _desc(capi, flags=SOFTMAX), p) == -3 and "workspace" in capi.last_error().lower()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_reference_equals_the_dcnv3_reference_behind_a_softmax(name):
    """On the full kernel dcnv4_softmax_ref(pack(offset, logits)) is dcnv3_ref(offset, softmax(logits)) -- output and all
    gradients, autograd through the softmax on the DCNv3 side; fp64, 1e-10."""
    x, off, logits, go, geo = R3.make_inputs(dtype=torch.float64, seed=13, offset_range=2.5, **SHAPES[name])
    G, K = geo[4], R.taps(geo[0])
    B, Ho, Wo, _ = logits.shape
    logits = logits * 3 - 1   # (make_inputs draws masks in [0, 1]; spread them)
    xs, o, l = (t.clone().requires_grad_(True) for t in (x, off, logits))
    m = torch.softmax(l.reshape(B, Ho, Wo, G, K), -1).reshape(B, Ho, Wo, G * K)
    out3 = R3.dcnv3_ref(xs, o, m, *geo)
    want = (out3.detach(),) + torch.autograd.grad(out3, (xs, o, l), go)
    out, gi, gom = RS.dcnv4_softmax_ref_grads(x, R.pack(off, logits, G, K), go, *geo, False)
    assert float(gom[..., G * K * 3:].abs().max() if gom.shape[-1] > G * K * 3 else 0.0) == 0.0
    for what, a, b in zip(("output", "grad_input", "grad_offset", "grad_logits"), (out, gi) + R.unpack(gom, G, K), want):
        assert a.shape == b.shape, what
        err = rel_err(a, b)
        print(name, what, "%.3e" % err)
        assert err <= 1e-10, (name, what, err)
    if K > 1:
        assert float(want[3].abs().max()) > 0


@pytest.mark.parametrize("remove_center", [False, True])
def test_reference_is_invariant_to_a_shift_of_the_logits_per_group(remove_center):
    kw = dict(B=2, G=2, D=4, H=6, W=5, kernel=3, pad=1, remove_center=remove_center, dtype=torch.float64, seed=4)
    x, om, go, geo = R.make_inputs(offset_range=2.5, **kw)
    G, K = 2, R.taps(3, remove_center)
    shift = torch.randn(om.shape[:3] + (G, 1), generator=torch.Generator().manual_seed(8), dtype=torch.float64) * 5
    a = RS.dcnv4_softmax_ref_grads(x, om, go, *geo)
    b = RS.dcnv4_softmax_ref_grads(x, RS.shift_logits(om, G, K, shift), go, *geo)
    for what, u, v in zip(("output", "grad_input", "grad_offset_mask"), a, b):
        assert rel_err(u, v) <= 1e-10, what
    # ... and the logit gradients of a (pixel, group) sum to zero
    glogit = R.unpack(a[2], G, K)[1].reshape(om.shape[:3] + (G, K))
    assert float(glogit.sum(-1).abs().max()) <= 1e-12 * float(glogit.abs().max())


def test_reference_counts_gated_out_taps_in_the_normaliser():
    """A tap pushed out of the image adds nothing to the output, still takes its share of the softmax, and its logit has
    the gradient -a S."""
    x, om, go, geo = R.make_inputs(B=1, G=1, D=4, H=5, W=7, kernel=3, pad=1, dtype=torch.float64, seed=2)
    off, m = R.unpack(om, 1, 9)
    off = off.clone()
    off[..., 0:2] = 30.0   # tap 0 of every pixel
    om = R.pack(off, m, 1, 9)
    assert not R.gate_of(om, 5, 7, *geo[:4], 1, 1.0)[..., 0].any()
    out, gi, gom = RS.dcnv4_softmax_ref_grads(x, om, go, *geo)
    a = torch.softmax(m.reshape(1, 5, 7, 9), -1)
    S = (go.double() * out).sum(-1)
    goff, glogit = R.unpack(gom, 1, 9)
    assert rel_err(glogit[..., 0], -a[..., 0] * S) <= 1e-12 and float(glogit[..., 0].abs().min()) > 0
    assert float(goff[..., 0:2].abs().max()) == 0.0


def test_python_surface_without_gpu():
    import inspect

    import modulated_deform_conv_amd as pkg
    from modulated_deform_conv_amd import dcnv3, dcnv4
    assert pkg.DCNv3Fused is dcnv3.DCNv3Fused and "DCNv3Fused" in pkg.__all__ and issubclass(dcnv3.DCNv3Fused, dcnv3.DCNv3)
    for fn in (dcnv4.dcnv4_forward, dcnv4.dcnv4_backward, dcnv4.dcnv4_core, dcnv4.DCNv4.__init__):
        assert inspect.signature(fn).parameters["softmax"].default is False
    params = list(inspect.signature(dcnv4.DCNv4Function.forward).parameters)
    assert params[-2:] == ["remove_center", "softmax"]
    x = torch.zeros(1, 4, 4, 8)
    om = torch.zeros(1, 4, 4, dcnv4.offset_mask_len(3, 2))
    with pytest.raises(NotImplementedError):
        dcnv4.dcnv4_core(x, om, 3, 1, 1, 1, 2, 4, 1.0, softmax=True)
    with pytest.raises(NotImplementedError):
        dcnv4.dcnv4_forward(x, om, 3, 1, 1, 1, 2, 4, 1.0, softmax=True)
    with pytest.raises(NotImplementedError):
        dcnv4.dcnv4_backward(x, om, x, 3, 1, 1, 1, 2, 4, 1.0, softmax=True)
    with pytest.raises(NotImplementedError):   # the published 15 arguments, and the 16th
        dcnv4.DCNv4Function.apply(x, om, 3, 3, 1, 1, 1, 1, 1, 1, 2, 4, 1.0, 256, False)
    with pytest.raises(NotImplementedError):
        dcnv4.DCNv4Function.apply(x, om, 3, 3, 1, 1, 1, 1, 1, 1, 2, 4, 1.0, 256, False, True)
    m = dcnv4.DCNv4(channels=16, group=2, softmax=True)
    assert m.softmax and "softmax=True" in m.extra_repr() and "softmax" not in dcnv4.DCNv4(channels=16, group=2).extra_repr()
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 16, 16), shape=(4, 4))
    with pytest.raises(NotImplementedError):
        dcnv3.DCNv3Fused(channels=16, group=2)(torch.zeros(1, 4, 4, 16))


@pytest.mark.parametrize("kw", [dict(channels=16, group=2), dict(channels=32, kernel_size=3, group=4, offset_scale=2.0),
                                dict(channels=8, kernel_size=5, pad=2, group=1, dw_kernel_size=3)])
def test_dcnv3_fused_has_the_state_dict_of_dcnv3(kw):
    from modulated_deform_conv_amd import DCNv3, DCNv3Fused
    theirs, ours = DCNv3(**kw), DCNv3Fused(**kw)
    assert list(ours.state_dict().keys()) == list(theirs.state_dict().keys())
    assert [k for k, _ in ours.named_parameters()] == [k for k, _ in theirs.named_parameters()]
    for k, v in theirs.state_dict().items():
        assert ours.state_dict()[k].shape == v.shape
    # the initialisation: offset and mask at zero, projections not
    assert all(float(p.detach().abs().max()) == 0.0 for lin in (ours.offset, ours.mask) for p in lin.parameters())
    assert float(ours.input_proj.weight.detach().abs().max()) > 0.0
    with torch.no_grad():
        for p in theirs.parameters():
            p.normal_()
    ours.load_state_dict(theirs.state_dict())   # strict
    for (k, a), (_, b) in zip(ours.named_parameters(), theirs.named_parameters()):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("group, kernel", [(4, 3), (1, 3), (2, 5), (3, 1)])
def test_dcnv3_fused_row_index(group, kernel):
    """The one linear layer of DCNv3Fused gives ``dcnv4_ref.pack`` of the two linears' outputs -- zeros in the padding --
    and its gradients reach both pairs of parameters."""
    from modulated_deform_conv_amd import DCNv3Fused
    from modulated_deform_conv_amd.dcnv4 import offset_mask_len
    C, K = 8 * group, kernel * kernel
    mod = DCNv3Fused(channels=C, kernel_size=kernel, pad=kernel // 2, group=group).double()
    with torch.no_grad():
        for lin in (mod.offset, mod.mask):
            lin.weight.normal_()
            lin.bias.normal_()
    OM = offset_mask_len(kernel, group)
    assert mod.pack_index.shape == (OM,) and mod.pack_index.dtype == torch.long
    x1 = torch.randn(2, 3, 4, C, dtype=torch.float64)
    w, b = mod.packed_linear()
    assert w.shape == (OM, C) and b.shape == (OM,)
    got = torch.nn.functional.linear(x1, w, b)
    want = R.pack(mod.offset(x1), mod.mask(x1), group, K)
    assert got.shape == want.shape and rel_err(got, want) <= 1e-14
    assert OM == group * K * 3 or float(got.detach()[..., group * K * 3:].abs().max()) == 0.0
    go = torch.randn(got.shape, dtype=torch.float64)
    params = (mod.offset.weight, mod.offset.bias, mod.mask.weight, mod.mask.bias)
    for a, c in zip(torch.autograd.grad(got, params, go), torch.autograd.grad(want, params, go)):
        assert rel_err(a, c) <= 1e-13
