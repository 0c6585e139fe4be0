"""3-D multi-scale deformable attention without a GPU (include/mdconv.h, "3-D multi-scale deformable attention"):
descriptor validation and its order, each shape rule's refusal with its words, the value length, workspace sizing, the two
references against each other, and the Python surface.  Host code only: no kernel is launched."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from tests import msda3d_ref as R
from tests.util import rel_err

EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -5
F32, F16, BF16 = 0, 1, 3
PAIRINGS = ((F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32))
LEVELS = ((4, 4, 4), (2, 2, 2), (1, 2, 2), (1, 1, 1))


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def _desc(capi, dtype=F32, coord_dtype=None, N=2, M=8, D=32, Lq=10, P=4, levels=LEVELS, L=None, accumulate=1, flags=0):
    d = capi.MdconvMsda3dDesc()
    d.dtype, d.coord_dtype = dtype, dtype if coord_dtype is None else coord_dtype
    d.batch, d.heads, d.head_channels, d.queries, d.points = N, M, D, Lq, P
    d.levels = len(levels) if L is None else L
    for l, (t, h, w) in enumerate(levels[:8]):
        d.level_sz[l][0], d.level_sz[l][1], d.level_sz[l][2] = t, h, w
    d.accumulate, d.flags = accumulate, flags
    return d


def _null():
    return ctypes.c_void_p(0)


def _fwd(capi, d, p=None, ws=None, ws_bytes=0):
    p = _null() if p is None else p
    return capi.lib().mdconv_msda3d_forward(ctypes.byref(d), p, p, p, p, _null() if ws is None else ws,
                                            ctypes.c_size_t(ws_bytes), _null())


def _bwd(capi, d, p=None, ws=None, ws_bytes=0):
    p = _null() if p is None else p
    return capi.lib().mdconv_msda3d_backward(ctypes.byref(d), p, p, p, p, p, p, p, _null() if ws is None else ws,
                                             ctypes.c_size_t(ws_bytes), _null())


def _ws(capi, d, backward):
    return capi.lib().mdconv_msda3d_workspace_bytes(ctypes.byref(d), backward)


def _refused(capi):
    return "shape rule" in capi.last_error()


def test_descriptor_mirror_and_exports(capi):
    assert [f[0] for f in capi.MdconvMsda3dDesc._fields_] == [f[0] for f in capi.MdconvMsdaDesc._fields_]
    assert ctypes.sizeof(capi.MdconvMsda3dDesc) == (8 + 8 * 3 + 2) * 4
    assert ctypes.sizeof(capi.MdconvMsdaDesc) == (8 + 8 * 2 + 2) * 4   # the 2-D descriptor has not moved
    assert capi.lib().mdconv_abi_version() == 2 == capi.ABI_VERSION
    hdr = (Path(__file__).resolve().parent.parent / "include" / "mdconv.h").read_text()
    for name in ("mdconv_msda3d_value_len", "mdconv_msda3d_workspace_bytes", "mdconv_msda3d_forward", "mdconv_msda3d_backward"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name) and re.search(r"\b%s\s*\(" % name, hdr)
    assert "MDCONV_MSDA3D_DESC_INIT" in hdr and "level_sz[MDCONV_MSDA_MAX_LEVELS][3]" in hdr


def test_valid_descriptor_stops_at_null_pointers(capi):
    for dtype, cdt in PAIRINGS:
        for call in (_fwd, _bwd):
            assert call(capi, _desc(capi, dtype=dtype, coord_dtype=cdt)) == ENULL and "NULL" in capi.last_error()
    # grad_value alone may be NULL with NO_GRAD_INPUT -- the others still may not
    assert _bwd(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT)) == ENULL
    for flags in (0, 1, 4, 5):
        assert _fwd(capi, _desc(capi, flags=flags)) == ENULL and _bwd(capi, _desc(capi, flags=flags)) == ENULL


@pytest.mark.parametrize("kw", [
    dict(dtype=2), dict(dtype=7), dict(dtype=F16 | 0x10), dict(dtype=BF16, coord_dtype=F16), dict(dtype=F16, coord_dtype=BF16),
    dict(dtype=F32, coord_dtype=F16), dict(dtype=F32, coord_dtype=2), dict(N=0), dict(M=0), dict(D=0), dict(Lq=0), dict(P=0),
    dict(P=-1), dict(L=0), dict(L=9), dict(L=-1), dict(levels=((4, 4, 4), (0, 2, 2))), dict(levels=((4, 0, 4),)),
    dict(levels=((4, 4, 0),)), dict(levels=((2, 2, -1),)), dict(flags=2), dict(flags=8), dict(flags=1 | 4 | 32),
    dict(flags=64), dict(accumulate=2), dict(accumulate=-1),
])
def test_invalid_descriptor(capi, kw):
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, **kw)) == EINVAL, kw
        assert capi.last_error().startswith("msda3d:")
    assert _ws(capi, _desc(capi, **kw), 0) == 0 and _ws(capi, _desc(capi, **kw), 1) == 0
    assert capi.lib().mdconv_msda3d_value_len(ctypes.byref(_desc(capi, **kw))) == -1


def test_order_of_checks(capi):
    """The descriptor, then the pointers, then the shape rule, then the workspace."""
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # non-NULL; nothing dereferences it
    # invalid AND NULL pointers AND outside the shape rule: EINVAL
    assert _fwd(capi, _desc(capi, D=6, flags=2)) == EINVAL
    # outside the shape rule with NULL pointers: the pointer check comes first
    assert _fwd(capi, _desc(capi, D=6)) == ENULL and _bwd(capi, _desc(capi, D=6)) == ENULL
    # outside the shape rule with pointers and no workspace: the shape rule comes before the workspace
    assert _bwd(capi, _desc(capi, D=6), p) == EUNSUPPORTED and _refused(capi)
    # pointer alignment: after the NULL checks, before the shape rule (include/mdconv.h, "Pointer alignment") -- 2 mod 16 is
    # below the 16-byte class of the first tensor, and the descriptor is outside the shape rule as well
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, D=6), ctypes.c_void_p((p.value | 15) - 13)) == EINVAL and "value pointer must be 16-byte aligned" in capi.last_error()
    # inside the rule, pointers given, the workspace missing / too small / misaligned: EWORKSPACE, nothing launched
    need = _ws(capi, _desc(capi), 1)
    assert need > 0
    assert _bwd(capi, _desc(capi), p) == EWORKSPACE
    assert _bwd(capi, _desc(capi), p, p, need - 1) == EWORKSPACE
    assert _bwd(capi, _desc(capi), p, ctypes.c_void_p((p.value + 15) // 16 * 16 + 4), need) == EWORKSPACE


def test_shape_rule_refusals_come_before_any_launch(capi):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for d, word in ((_desc(capi, D=6), "multiple of 4"), (_desc(capi, dtype=F16, D=4), "multiple of 8"),
                    (_desc(capi, dtype=BF16, coord_dtype=F32, D=12), "multiple of 8"),
                    (_desc(capi, levels=((1, 2, 2),) * 8, P=513), "4096"),
                    (_desc(capi, N=1 << 10, M=1 << 6, D=64, levels=((16, 32, 32),)), "2^31"),   # value: 2^32 bytes
                    (_desc(capi, N=1, M=1, D=4, levels=((1 << 11, 1 << 10, 1 << 10),)), "2^31"),   # one level: 2^31 rows
                    (_desc(capi, N=1, M=1, D=4, levels=((2, 1 << 16, 1 << 16),)), "2^31"),        # its plane alone: 2^32
                    (_desc(capi, N=1, M=1, D=4, Lq=1 << 22, P=64, levels=((1, 1, 1),)), "2^31")):   # locations: 3 * 2^30 bytes
        for call in (_fwd, _bwd):
            assert call(capi, d, p) == EUNSUPPORTED, word
            assert word in capi.last_error() and _refused(capi), capi.last_error()
        assert _ws(capi, d, 1) == 0
    assert capi.lib().mdconv_msda3d_value_len(ctypes.byref(_desc(capi, levels=((2, 1 << 16, 1 << 16),)))) == -1
    # batch * heads above 65535: the lists of grad_value only -- the forward and the backward without grad_value take it
    big = dict(N=4096, M=17, D=4, Lq=1, P=1, levels=((1, 1, 1),))
    assert _bwd(capi, _desc(capi, **big), p) == EUNSUPPORTED and "65535" in capi.last_error()
    assert _ws(capi, _desc(capi, **big), 1) == 0
    # (the calls that would go on to launch are only sized: a workspace query plans the same call)
    assert _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **big), 1) == 0 and not _refused(capi)
    assert _ws(capi, _desc(capi, **big), 0) == 0 and not _refused(capi)
    # the list stride L*P*Lq*8: 2^31 here, while sampling_locations (L*P*Lq*3 elements of 2 bytes) stays below 2^31 bytes
    stride = dict(dtype=F16, N=1, M=1, D=8, Lq=1 << 16, P=512, levels=((1, 1, 1),) * 8)
    assert _bwd(capi, _desc(capi, **stride), p) == EUNSUPPORTED
    assert "list stride" in capi.last_error() and "* 8" in capi.last_error()
    assert _ws(capi, _desc(capi, **stride), 1) == 0 and _refused(capi)
    assert _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **stride), 1) == 0 and not _refused(capi)
    assert _ws(capi, _desc(capi, **stride), 0) == 0 and not _refused(capi)
    half = dict(stride, Lq=(1 << 16) - 1)
    assert _ws(capi, _desc(capi, **half), 1) > 0


def test_value_len(capi):
    L = capi.lib()
    assert L.mdconv_msda3d_value_len(ctypes.byref(_desc(capi))) == 64 + 8 + 4 + 1
    assert L.mdconv_msda3d_value_len(ctypes.byref(_desc(capi, levels=((3, 4, 5), (2, 2, 3), (1, 1, 1))))) == 73
    # rows beyond `levels` are ignored
    assert L.mdconv_msda3d_value_len(ctypes.byref(_desc(capi, levels=((3, 4, 5), (2, 2, 3), (1, 1, 1)), L=2))) == 72
    assert L.mdconv_msda3d_value_len(None) == -1


def test_workspace_bytes(capi):
    for dtype, cdt in PAIRINGS:
        kw = dict(dtype=dtype, coord_dtype=cdt)
        for flags in (0, 1, 4, 5):
            assert _ws(capi, _desc(capi, flags=flags, **kw), 0) == 0
        full = _ws(capi, _desc(capi, **kw), 1)
        det = _ws(capi, _desc(capi, flags=capi.FLAG_DETERMINISTIC, **kw), 1)
        no_gv = _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **kw), 1)
        assert no_gv == 0 < full < det
        # the sort scratch belongs to the grad_value stages; the write mode never changes the figure
        assert _ws(capi, _desc(capi, flags=capi.FLAG_DETERMINISTIC | capi.FLAG_NO_GRAD_INPUT, **kw), 1) == no_gv
        assert _ws(capi, _desc(capi, accumulate=0, **kw), 1) == full
    # the lists do not depend on the channels of a head; they grow with the queries
    assert _ws(capi, _desc(capi, D=64), 1) == _ws(capi, _desc(capi, D=32), 1)
    assert _ws(capi, _desc(capi, Lq=40), 1) > _ws(capi, _desc(capi, Lq=20), 1) > _ws(capi, _desc(capi, Lq=10), 1)
    # counters, row pointers and K * Lq * 8 entries of 16 bytes per (image, head): at least that, before alignment
    N, M, S, K, Lq = 2, 8, 77, 16, 10
    assert _ws(capi, _desc(capi), 1) >= N * M * (S * 4 + (S + 1) * 4 + K * Lq * 8 * 16)


SHAPES = {
    "three_levels": dict(N=2, M=3, D=8, shapes=[(3, 4, 5), (2, 2, 3), (1, 1, 1)], Lq=7, P=2),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_two_references_agree(name):
    """Two independent statements of the contract: grid_sample on 5-D input per level, and the explicit eight-corner
    gather with the gate.  fp64, 1e-12, output and the three gradients (measured: 8e-16)."""
    value, loc, attn, go = R.make_inputs(dtype=torch.float64, seed=11, **SHAPES[name])
    shapes = SHAPES[name]["shapes"]
    assert R.min_lattice_distance(loc, shapes) >= R.MARGIN
    x, y, z = R.pixel_positions(loc, shapes)
    assert float(x.min()) < -0.5 and float(y.min()) < -0.5 and float(z.min()) < -0.5   # samples beyond the border take part
    gate = R.gate_of(loc, shapes)
    assert bool(gate.any()) and not bool(gate.all())
    ref = R.msda3d_ref_grads(value, shapes, loc, attn, go)
    direct = R.msda3d_ref_grads(value, shapes, loc, attn, go, fn=R.msda3d_direct)
    for what, a, b in zip(("output", "grad_value", "grad_sampling_locations", "grad_attention_weights"), ref, direct):
        assert a.shape == b.shape, what
        assert float(a.abs().max()) > 0, what
        err = rel_err(a, b)
        print(name, what, "%.3e" % err)
        assert err <= 1e-12, (name, what, err)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.float16, torch.bfloat16])
def test_make_inputs_keeps_the_margin(dtype):
    for name in sorted(SHAPES):
        _, loc, attn, _ = R.make_inputs(dtype=dtype, seed=5, **SHAPES[name])
        assert loc.dtype == dtype and loc.shape[-1] == 3 and R.min_lattice_distance(loc, SHAPES[name]["shapes"]) >= R.MARGIN
        assert float((attn.double().sum((-1, -2)) - 1).abs().max()) < 2e-2


@pytest.mark.parametrize("coord_dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_lattice_inputs_assert_their_own_conditions(coord_dtype):
    shapes = [(2, 4, 2), (1, 2, 2)]
    value, loc, attn, go = R.make_lattice_inputs(1, 2, 8, shapes, P=2, dtype=coord_dtype, coord_dtype=coord_dtype)
    assert loc.dtype == coord_dtype and loc.shape[1] == go.shape[1]
    with pytest.raises(AssertionError):
        R.lattice_points(2, 3, 2)


def test_python_surface_without_gpu():
    import modulated_deform_conv_amd as pkg
    from modulated_deform_conv_amd import msda3d
    for name in ("ms_deform_attn_3d_forward", "ms_deform_attn_3d_backward", "MSDeformAttn3DFunction", "ms_deform_attn_3d",
                 "MSDeformAttn3D"):
        assert getattr(pkg, name) is getattr(msda3d, name) and name in pkg.__all__
    shapes = [(2, 4, 4), (1, 2, 2)]
    value, loc, attn, go = R.make_inputs(N=1, M=2, D=4, shapes=shapes, Lq=3, P=2)
    with pytest.raises(NotImplementedError):
        msda3d.ms_deform_attn_3d(value, shapes, loc, attn)
    with pytest.raises(NotImplementedError):
        msda3d.MSDeformAttn3DFunction.apply(value, torch.tensor(shapes), torch.tensor([0, 32]), loc, attn, 64)
    with pytest.raises(NotImplementedError):
        msda3d.ms_deform_attn_3d_forward(value, shapes, loc, attn)
    with pytest.raises(NotImplementedError):
        msda3d.ms_deform_attn_3d_backward(value, shapes, loc, attn, go)
    # a wrong level_start_index is refused before the device is looked at
    with pytest.raises(ValueError):
        msda3d.ms_deform_attn_3d(value, shapes, loc, attn, [0, 16])
    with pytest.raises(ValueError):
        msda3d.MSDeformAttn3DFunction.apply(value, torch.tensor(shapes), torch.tensor([0, 33]), loc, attn, 64)
    msda3d._check_starts(msda3d._shapes(shapes), [0, 32])
    msda3d._check_starts(msda3d._shapes(torch.tensor(shapes)), torch.tensor([0, 32]))
    with pytest.raises(ValueError):
        msda3d._check_starts(msda3d._shapes(shapes), [0, 16])
    with pytest.raises(ValueError):
        msda3d._shapes([(1, 1, 1)] * 9)
    m = msda3d.MSDeformAttn3D(d_model=16, n_levels=2, n_heads=2, n_points=2)
    assert sorted(m.state_dict()) == sorted([
        "sampling_offsets.weight", "sampling_offsets.bias", "attention_weights.weight", "attention_weights.bias",
        "value_proj.weight", "value_proj.bias", "output_proj.weight", "output_proj.bias"])
    assert m.sampling_offsets.out_features == 2 * 2 * 2 * 3 and m._core is msda3d.ms_deform_attn_3d
    # the directional bias: largest component 1 on point 0, point p at p + 1 steps, the same on every level
    bias = m.sampling_offsets.bias.detach().view(2, 2, 2, 3)
    assert torch.allclose(bias[:, :, 0].abs().max(-1)[0], torch.ones(2, 2))
    assert torch.allclose(bias[:, :, 1], 2 * bias[:, :, 0]) and torch.equal(bias[:, 0], bias[:, 1])
    assert float(m.sampling_offsets.weight.detach().abs().max()) == 0.0
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 3, 16), torch.rand(1, 3, 2, 3), torch.zeros(1, 36, 16), shapes, [0, 32])
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 16), torch.rand(1, 3, 2, 3), torch.zeros(1, 37, 16), shapes, [0, 32])
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 16), torch.rand(1, 3, 2, 2), torch.zeros(1, 36, 16), shapes, [0, 32])
