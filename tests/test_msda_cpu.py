"""Multi-scale deformable attention without a GPU (include/mdconv.h, "Multi-scale deformable attention"): descriptor
validation and its order, the shape rule's refusals, the value length, workspace sizing, the two references against each
other, and the surfaces that must not have moved.  Host code only: no kernel is launched."""
import ctypes

import pytest
import torch

from tests import msda_ref as R
from tests.util import rel_err

EINVAL, ENULL, EUNSUPPORTED = -1, -2, -5
F32, F16, BF16 = 0, 1, 3
PAIRINGS = ((F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32))


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def _desc(capi, dtype=F32, coord_dtype=None, N=2, M=8, D=32, Lq=10, P=4, levels=((8, 8), (4, 4), (2, 2), (1, 1)), L=None,
          accumulate=1, flags=0):
    d = capi.MdconvMsdaDesc()
    d.dtype, d.coord_dtype = dtype, dtype if coord_dtype is None else coord_dtype
    d.batch, d.heads, d.head_channels, d.queries, d.points = N, M, D, Lq, P
    d.levels = len(levels) if L is None else L
    for l, (h, w) in enumerate(levels[:8]):
        d.level_sz[l][0], d.level_sz[l][1] = h, w
    d.accumulate, d.flags = accumulate, flags
    return d


def _fwd(capi, d, p=None):
    p = ctypes.c_void_p(0) if p is None else p
    return capi.lib().mdconv_msda_forward(ctypes.byref(d), p, p, p, p, ctypes.c_void_p(0), ctypes.c_size_t(0), ctypes.c_void_p(0))


def _bwd(capi, d, p=None):
    p = ctypes.c_void_p(0) if p is None else p
    return capi.lib().mdconv_msda_backward(ctypes.byref(d), p, p, p, p, p, p, p, ctypes.c_void_p(0), ctypes.c_size_t(0),
                                           ctypes.c_void_p(0))


def _ws(capi, d, backward):
    return capi.lib().mdconv_msda_workspace_bytes(ctypes.byref(d), backward)


def test_descriptor_mirror(capi):
    assert [f[0] for f in capi.MdconvMsdaDesc._fields_] == [
        "dtype", "coord_dtype", "batch", "heads", "head_channels", "queries", "levels", "points", "level_sz", "accumulate",
        "flags"]
    assert capi.MSDA_MAX_LEVELS == 8
    assert ctypes.sizeof(capi.MdconvMsdaDesc) == (8 + 8 * 2 + 2) * 4


def test_valid_descriptor_stops_at_null_pointers(capi):
    assert (capi.F32, capi.F16, capi.BF16) == (F32, F16, BF16)
    for dtype, cdt in PAIRINGS:
        for call in (_fwd, _bwd):
            assert call(capi, _desc(capi, dtype=dtype, coord_dtype=cdt)) == ENULL and "NULL" in capi.last_error()
    # a descriptor outside the shape rule as well: the pointer check comes first
    assert _fwd(capi, _desc(capi, D=6)) == ENULL
    # grad_value alone may be NULL with NO_GRAD_INPUT -- the others still may not
    assert _bwd(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT)) == ENULL
    for flags in (0, 1, 4, 5):
        assert _fwd(capi, _desc(capi, flags=flags)) == ENULL and _bwd(capi, _desc(capi, flags=flags)) == ENULL


@pytest.mark.parametrize("kw", [
    dict(dtype=2), dict(dtype=7), dict(dtype=F16 | 0x10), dict(dtype=BF16, coord_dtype=F16), dict(dtype=F16, coord_dtype=BF16),
    dict(dtype=F32, coord_dtype=F16), dict(dtype=F32, coord_dtype=2), dict(N=0), dict(M=0), dict(D=0), dict(Lq=0), dict(P=0),
    dict(P=-1), dict(L=0), dict(L=9), dict(L=-1), dict(levels=((8, 8), (0, 4))), dict(levels=((8, -1),)), dict(flags=2),
    dict(flags=8), dict(flags=1 | 4 | 32), dict(flags=64), dict(accumulate=2), dict(accumulate=-1),
])
def test_invalid_descriptor(capi, kw):
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, **kw)) == EINVAL, kw
        assert capi.last_error()
    assert _ws(capi, _desc(capi, **kw), 0) == 0 and _ws(capi, _desc(capi, **kw), 1) == 0
    assert capi.lib().mdconv_msda_value_len(ctypes.byref(_desc(capi, **kw))) == -1


def test_shape_rule_refusals_come_before_any_launch(capi):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # non-NULL; nothing dereferences it
    for d, word in ((_desc(capi, D=6), "multiple of 4"), (_desc(capi, dtype=F16, D=4), "multiple of 8"),
                    (_desc(capi, dtype=BF16, coord_dtype=F32, D=12), "multiple of 8"),
                    (_desc(capi, levels=((2, 2),) * 8, P=513), "4096"),
                    (_desc(capi, N=1 << 10, M=1 << 6, D=64, levels=((128, 128),)), "2^31"),   # value: 2^32 bytes
                    (_desc(capi, N=1, M=1, D=4, Lq=1 << 22, P=64, levels=((1, 1),)), "2^31")):   # locations: 2^31 bytes
        for call in (_fwd, _bwd):
            assert call(capi, d, p) == EUNSUPPORTED, word
            assert word in capi.last_error(), capi.last_error()
            # pointer alignment: after the NULL checks, before the shape rule (include/mdconv.h, "Pointer alignment") -- 2 mod 16 is
            # below the 16-byte class of the first tensor, and the descriptor is outside the shape rule as well
            assert call(capi, d, ctypes.c_void_p((p.value | 15) - 13)) == EINVAL and "value pointer must be 16-byte aligned" in capi.last_error()
        assert _ws(capi, d, 1) == 0
    # batch * heads above 65535: the lists of grad_value only -- the forward and the backward without grad_value take it
    big = dict(N=4096, M=17, D=4, Lq=1, P=1, levels=((1, 1),))
    assert _bwd(capi, _desc(capi, **big), p) == EUNSUPPORTED and "65535" in capi.last_error()
    assert _ws(capi, _desc(capi, **big), 1) == 0
    # (the calls that would go on to launch are only sized: a workspace query plans the same call)
    assert _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **big), 1) == 0 and not _refused(capi)
    assert _ws(capi, _desc(capi, **big), 0) == 0 and not _refused(capi)
    # (the list stride K * Lq * 4 never exceeds the bytes of sampling_locations, N * Lq * M * K * 2 elements of 2 bytes or
    # more, so the tensor rule refuses first: the largest 16-bit call of one image and one head is refused by it)
    stride = dict(dtype=F16, N=1, M=1, D=8, Lq=1 << 17, P=512, levels=((1, 1),) * 8)
    assert _bwd(capi, _desc(capi, **stride), p) == EUNSUPPORTED and "2^31" in capi.last_error()


def _refused(capi):
    return "shape rule" in capi.last_error()


def test_value_len(capi):
    L = capi.lib()
    assert L.mdconv_msda_value_len(ctypes.byref(_desc(capi))) == 64 + 16 + 4 + 1
    assert L.mdconv_msda_value_len(ctypes.byref(_desc(capi, levels=((6, 5), (3, 3), (1, 1))))) == 40
    # rows beyond `levels` are ignored
    assert L.mdconv_msda_value_len(ctypes.byref(_desc(capi, levels=((6, 5), (3, 3), (1, 1)), L=2))) == 39
    assert L.mdconv_msda_value_len(None) == -1


def test_workspace_bytes(capi):
    for dtype, cdt in PAIRINGS:
        kw = dict(dtype=dtype, coord_dtype=cdt)
        for flags in (0, 1, 4, 5):
            assert _ws(capi, _desc(capi, flags=flags, **kw), 0) == 0
        full = _ws(capi, _desc(capi, **kw), 1)
        det = _ws(capi, _desc(capi, flags=capi.FLAG_DETERMINISTIC, **kw), 1)
        no_gv = _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **kw), 1)
        assert full > 0 and no_gv == 0 < full and det >= full
        # the sort scratch belongs to the grad_value stages; the write mode never changes the figure
        assert _ws(capi, _desc(capi, flags=capi.FLAG_DETERMINISTIC | capi.FLAG_NO_GRAD_INPUT, **kw), 1) == no_gv
        assert _ws(capi, _desc(capi, accumulate=0, **kw), 1) == full
    # the lists do not depend on the channels of a head
    assert _ws(capi, _desc(capi, D=64), 1) == _ws(capi, _desc(capi, D=32), 1)
    # counters, row pointers and K * Lq * 4 entries of 16 bytes per (image, head): at least that, before alignment
    N, M, S, K, Lq = 2, 8, 85, 16, 10
    assert _ws(capi, _desc(capi), 1) >= N * M * (S * 4 + (S + 1) * 4 + K * Lq * 4 * 16)


SHAPES = {
    "rect_levels": dict(N=2, M=3, D=8, shapes=[(6, 5), (3, 3), (1, 1)], Lq=7, P=2),
    "two_levels": dict(N=1, M=2, D=4, shapes=[(16, 16), (2, 3)], Lq=5, P=3),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_two_references_agree(name):
    """Two independent statements of the contract: grid_sample per level, and the explicit four-corner gather with the
    gate.  fp64, 1e-10, output and the three gradients."""
    value, loc, attn, go = R.make_inputs(dtype=torch.float64, seed=11, **SHAPES[name])
    shapes = SHAPES[name]["shapes"]
    assert R.min_lattice_distance(loc, shapes) >= R.MARGIN
    x, y = R.pixel_positions(loc, shapes)
    assert float(x.min()) < -0.5 and float(y.min()) < -0.5   # samples beyond the border take part
    ref = R.msda_ref_grads(value, shapes, loc, attn, go)
    direct = R.msda_ref_grads(value, shapes, loc, attn, go, fn=R.msda_direct)
    for what, a, b in zip(("output", "grad_value", "grad_sampling_locations", "grad_attention_weights"), ref, direct):
        assert a.shape == b.shape, what
        assert float(a.abs().max()) > 0, what
        err = rel_err(a, b)
        print(name, what, "%.3e" % err)
        assert err <= 1e-10, (name, what, err)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.float16, torch.bfloat16])
def test_make_inputs_keeps_the_margin(dtype):
    for name in sorted(SHAPES):
        _, loc, attn, _ = R.make_inputs(dtype=dtype, seed=5, **SHAPES[name])
        assert loc.dtype == dtype and R.min_lattice_distance(loc, SHAPES[name]["shapes"]) >= R.MARGIN
        assert float((attn.double().sum((-1, -2)) - 1).abs().max()) < 2e-2


def test_existing_surfaces_are_untouched(capi):
    assert capi.lib().mdconv_abi_version() == 2 == capi.ABI_VERSION
    assert ctypes.sizeof(capi.MdconvDesc) == 132
    assert ctypes.sizeof(capi.MdconvDcnv3Desc) == 68


def test_python_surface_without_gpu():
    import modulated_deform_conv_amd as pkg
    from modulated_deform_conv_amd import msda
    for name in ("ms_deform_attn_forward", "ms_deform_attn_backward", "MSDeformAttnFunction", "ms_deform_attn", "MSDeformAttn"):
        assert getattr(pkg, name) is getattr(msda, name) and name in pkg.__all__
    shapes = [(4, 4), (2, 2)]
    value, loc, attn, go = R.make_inputs(N=1, M=2, D=4, shapes=shapes, Lq=3, P=2)
    with pytest.raises(NotImplementedError):
        msda.ms_deform_attn(value, shapes, loc, attn)
    with pytest.raises(NotImplementedError):
        msda.MSDeformAttnFunction.apply(value, torch.tensor(shapes), torch.tensor([0, 16]), loc, attn, 64)
    with pytest.raises(NotImplementedError):
        msda.ms_deform_attn_forward(value, shapes, loc, attn)
    with pytest.raises(NotImplementedError):
        msda.ms_deform_attn_backward(value, shapes, loc, attn, go)
    m = msda.MSDeformAttn(d_model=16, n_levels=2, n_heads=2, n_points=2)
    assert sorted(m.state_dict()) == sorted([
        "sampling_offsets.weight", "sampling_offsets.bias", "attention_weights.weight", "attention_weights.bias",
        "value_proj.weight", "value_proj.bias", "output_proj.weight", "output_proj.bias"])
    # the directional bias: head 0 looks along +x, point p at p + 1 steps, on every level
    bias = m.sampling_offsets.bias.detach().view(2, 2, 2, 2)
    assert torch.allclose(bias[0, :, 0], torch.tensor([1.0, 0.0])) and torch.allclose(bias[0, :, 1], torch.tensor([2.0, 0.0]))
    assert float(m.sampling_offsets.weight.detach().abs().max()) == 0.0
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 3, 16), torch.rand(1, 3, 2, 2), torch.zeros(1, 20, 16), shapes, [0, 16])
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 16), torch.rand(1, 3, 2, 2), torch.zeros(1, 21, 16), shapes, [0, 16])
