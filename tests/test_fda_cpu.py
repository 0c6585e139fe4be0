"""Packed deformable attention without a GPU (include/mdconv.h, "Packed deformable attention"): the descriptor mirror,
validation and its order, the shape rule's refusals with their words, the row length, workspace sizing against multi-scale
deformable attention, the Python packing, the two reference routes against each other, and the Python surface.  Host code
only: no kernel is launched."""
import ctypes

import pytest
import torch

from tests import fda_ref as R
from tests import msda_ref as MR
from tests.util import rel_err

EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -5
F32, F16, BF16 = 0, 1, 3
PAIRINGS = ((F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32))
LEVELS = ((8, 8), (4, 4), (2, 2), (1, 1))


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def _fill(d, dtype, coord_dtype, N, M, D, Lq, P, levels, L, accumulate, flags):
    d.dtype, d.coord_dtype = dtype, dtype if coord_dtype is None else coord_dtype
    d.batch, d.heads, d.head_channels, d.queries, d.points = N, M, D, Lq, P
    d.levels = len(levels) if L is None else L
    for l, (h, w) in enumerate(levels[:8]):
        d.level_sz[l][0], d.level_sz[l][1] = h, w
    d.accumulate, d.flags = accumulate, flags
    return d


def _desc(capi, dtype=F32, coord_dtype=None, N=2, M=8, D=32, Lq=10, P=4, levels=LEVELS, L=None, accumulate=1, flags=0,
          cls=None):
    return _fill((cls or capi.MdconvFdaDesc)(), dtype, coord_dtype, N, M, D, Lq, P, levels, L, accumulate, flags)


def _fwd(capi, d, p=None):
    p = ctypes.c_void_p(0) if p is None else p
    return capi.lib().mdconv_fda_forward(ctypes.byref(d), p, p, p, ctypes.c_void_p(0), ctypes.c_size_t(0), ctypes.c_void_p(0))


def _bwd(capi, d, p=None):
    p = ctypes.c_void_p(0) if p is None else p
    return capi.lib().mdconv_fda_backward(ctypes.byref(d), p, p, p, p, p, ctypes.c_void_p(0), ctypes.c_size_t(0),
                                          ctypes.c_void_p(0))


def _ws(capi, d, backward):
    return capi.lib().mdconv_fda_workspace_bytes(ctypes.byref(d), backward)


def _msda_ws(capi, backward=1, **kw):
    return capi.lib().mdconv_msda_workspace_bytes(ctypes.byref(_desc(capi, cls=capi.MdconvMsdaDesc, **kw)), backward)


def test_descriptor_mirror(capi):
    assert [f[0] for f in capi.MdconvFdaDesc._fields_] == [f[0] for f in capi.MdconvMsdaDesc._fields_]
    assert ctypes.sizeof(capi.MdconvFdaDesc) == ctypes.sizeof(capi.MdconvMsdaDesc) == (8 + 8 * 2 + 2) * 4
    for name in ("mdconv_fda_value_len", "mdconv_fda_loc_attn_len", "mdconv_fda_workspace_bytes", "mdconv_fda_forward",
                 "mdconv_fda_backward"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)


def test_valid_descriptor_stops_at_null_pointers(capi):
    for dtype, cdt in PAIRINGS:
        for call in (_fwd, _bwd):
            assert call(capi, _desc(capi, dtype=dtype, coord_dtype=cdt)) == ENULL and "NULL" in capi.last_error()
    # grad_value alone may be NULL with NO_GRAD_INPUT -- the others still may not
    assert _bwd(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT)) == ENULL
    for flags in (0, 1, 4, 5):   # bits 1 and 4 only
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
        assert capi.last_error().startswith("fda: ")
    assert _ws(capi, _desc(capi, **kw), 0) == 0 and _ws(capi, _desc(capi, **kw), 1) == 0
    assert capi.lib().mdconv_fda_value_len(ctypes.byref(_desc(capi, **kw))) == -1
    assert capi.lib().mdconv_fda_loc_attn_len(ctypes.byref(_desc(capi, **kw))) == -1


def test_error_order(capi):
    """descriptor (EINVAL), then pointers (ENULL), then the shape rule (EUNSUPPORTED, named), then the workspace."""
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # non-NULL; nothing dereferences it
    bad_and_unsupported = _desc(capi, D=6, flags=2)
    for call in (_fwd, _bwd):
        assert call(capi, bad_and_unsupported) == EINVAL and call(capi, bad_and_unsupported, p) == EINVAL
        unsupported = _desc(capi, D=6)
        assert call(capi, unsupported) == ENULL and call(capi, unsupported, p) == EUNSUPPORTED
        assert "fda: outside the shape rule" in capi.last_error()
        # pointer alignment: after the NULL checks, before the shape rule (include/mdconv.h, "Pointer alignment") -- 2 mod 16 is
        # below the 16-byte class of the first tensor, and the descriptor is outside the shape rule as well
        assert call(capi, unsupported, ctypes.c_void_p((p.value | 15) - 13)) == EINVAL and "value pointer must be 16-byte aligned" in capi.last_error()
    # a valid backward with good pointers and no workspace stops at the workspace; the forward needs none, and neither
    # does the backward without grad_value, so those are only sized here
    assert _bwd(capi, _desc(capi), p) == EWORKSPACE and "workspace" in capi.last_error().lower()
    assert capi.lib().mdconv_fda_forward(None, p, p, p, None, 0, None) == EINVAL


def test_shape_rule_refusals_come_before_any_launch(capi):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for d, word in ((_desc(capi, D=6), "multiple of 4"), (_desc(capi, dtype=F16, D=4), "multiple of 8"),
                    (_desc(capi, dtype=BF16, coord_dtype=F32, D=12), "multiple of 8"),
                    (_desc(capi, levels=((2, 2),) * 8, P=513), "4096"),
                    (_desc(capi, N=1 << 10, M=1 << 6, D=64, levels=((128, 128),)), "2^31"),   # value: 2^32 bytes
                    (_desc(capi, N=1, M=1, D=4, Lq=1 << 22, P=64, levels=((1, 1),)), "2^31")):   # locations alone: 2^31 bytes
        for call in (_fwd, _bwd):
            assert call(capi, d, p) == EUNSUPPORTED, word
            assert word in capi.last_error() and capi.last_error().startswith("fda: "), capi.last_error()
        assert _ws(capi, d, 1) == 0
    # the packed tensor alone: N * Lq * M * 3K * 4 = 3 * 2^18 * 3 * 256 * 4 = 2.25 * 2^30 bytes, where the locations of the
    # same shape (1.5 * 2^30) and every other tensor are inside the rule -- multi-scale deformable attention takes the shape
    packed = dict(N=1, M=1, D=4, Lq=3 << 18, P=256, levels=((1, 1),))
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, **packed), p) == EUNSUPPORTED and "2^31" in capi.last_error()
    assert _ws(capi, _desc(capi, **packed), 1) == 0 and _msda_ws(capi, **packed) > 0
    # ... and with 16-bit coordinates it is inside the rule again
    assert _ws(capi, _desc(capi, dtype=F16, **dict(packed, D=8)), 1) > 0
    # batch * heads above 65535: the lists of grad_value only -- the forward and the backward without grad_value take it
    big = dict(N=4096, M=17, D=4, Lq=1, P=1, levels=((1, 1),))
    assert _bwd(capi, _desc(capi, **big), p) == EUNSUPPORTED and "65535" in capi.last_error()
    assert _ws(capi, _desc(capi, **big), 1) == 0
    assert _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **big), 1) == 0 and "shape rule" not in capi.last_error()
    assert _ws(capi, _desc(capi, **big), 0) == 0 and "shape rule" not in capi.last_error()


def test_value_len_and_loc_attn_len(capi):
    L = capi.lib()
    assert L.mdconv_fda_value_len(ctypes.byref(_desc(capi))) == 64 + 16 + 4 + 1
    assert L.mdconv_fda_value_len(ctypes.byref(_desc(capi, levels=((6, 5), (3, 3), (1, 1)), L=2))) == 39
    assert L.mdconv_fda_value_len(None) == -1 and L.mdconv_fda_loc_attn_len(None) == -1
    for levels, P in ((LEVELS, 4), (((5, 7),), 1), (((6, 5), (3, 3), (1, 1)), 2), (((2, 2),) * 8, 512)):
        assert L.mdconv_fda_loc_attn_len(ctypes.byref(_desc(capi, levels=levels, P=P))) == 3 * len(levels) * P
    # rows beyond `levels` are ignored; the figure does not wait for the shape rule (K > 4096 is refused by a call)
    assert L.mdconv_fda_loc_attn_len(ctypes.byref(_desc(capi, L=2))) == 3 * 2 * 4
    assert L.mdconv_fda_loc_attn_len(ctypes.byref(_desc(capi, levels=((2, 2),) * 8, P=1 << 28))) == -1


def test_workspace_bytes(capi):
    """0 for the forward; a backward with grad_value takes the lists of multi-scale deformable attention for the same shape
    plus 8 bytes per (query, head), rounded up to the workspace's 256-byte slots; nothing without grad_value."""
    def stats(N, Lq, M):
        return (N * Lq * M * 8 + 255) // 256 * 256

    for dtype, cdt in PAIRINGS:
        kw = dict(dtype=dtype, coord_dtype=cdt)
        for flags in (0, 1, 4, 5):
            assert _ws(capi, _desc(capi, flags=flags, **kw), 0) == 0
        full = _ws(capi, _desc(capi, **kw), 1)
        det = _ws(capi, _desc(capi, flags=capi.FLAG_DETERMINISTIC, **kw), 1)
        no_gv = _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **kw), 1)
        assert full == _msda_ws(capi, **kw) + stats(2, 10, 8)
        assert det == _msda_ws(capi, flags=capi.FLAG_DETERMINISTIC, **kw) + stats(2, 10, 8) and det >= full
        assert no_gv == 0 < full
        assert _ws(capi, _desc(capi, flags=capi.FLAG_DETERMINISTIC | capi.FLAG_NO_GRAD_INPUT, **kw), 1) == 0
        assert _ws(capi, _desc(capi, accumulate=0, **kw), 1) == full
    odd = dict(N=1, M=3, D=8, Lq=7, P=2, levels=((6, 5), (3, 3), (1, 1)))
    assert _ws(capi, _desc(capi, **odd), 1) == _msda_ws(capi, **odd) + 256
    assert _ws(capi, _desc(capi, D=64), 1) == _ws(capi, _desc(capi, D=32), 1)


def test_python_packing_round_trip():
    from modulated_deform_conv_amd import fda
    gen = torch.Generator().manual_seed(2)
    N, Lq, M, L, P = 2, 3, 2, 3, 2
    loc = torch.rand(N, Lq, M, L, P, 2, generator=gen)
    logits = torch.randn(N, Lq, M, L, P, generator=gen)
    packed = fda.pack_loc_attn(loc, logits)
    assert packed.shape == (N, Lq, M, 3 * L * P) and packed.is_contiguous() and torch.equal(packed, R.pack(loc, logits))
    assert torch.equal(fda.pack_loc_attn(loc, logits.flatten(-2)), packed)
    # the layout of the header: tap = l * P + p; x at 2 * tap, y at 2 * tap + 1, logit at 2K + tap
    K = L * P
    for l in range(L):
        for p in range(P):
            tap = l * P + p
            assert torch.equal(packed[..., 2 * tap], loc[:, :, :, l, p, 0]) and torch.equal(packed[..., 2 * tap + 1], loc[:, :, :, l, p, 1])
            assert torch.equal(packed[..., 2 * K + tap], logits[:, :, :, l, p])
    back = fda.unpack_loc_attn(packed, L, P)
    assert torch.equal(back[0], loc) and torch.equal(back[1], logits)
    assert all(torch.equal(a, b) for a, b in zip(back, R.unpack(packed, L, P)))
    with pytest.raises(ValueError):
        fda.unpack_loc_attn(packed, L, P + 1)


SHAPES = {
    "rect_levels": dict(N=2, M=3, D=8, shapes=[(6, 5), (3, 3), (1, 1)], Lq=7, P=2),
    "two_levels": dict(N=1, M=2, D=4, shapes=[(16, 16), (2, 3)], Lq=5, P=3),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_two_reference_routes_agree(name):
    """grid_sample per level against the explicit four-corner gather, both behind the fp64 softmax: output and the two
    gradients, fp64, 1e-10; and the packed gradient is autograd's straight through unpack, softmax and the reference."""
    kw = SHAPES[name]
    shapes, P = kw["shapes"], kw["P"]
    value, loc_attn, go = R.make_inputs(dtype=torch.float64, seed=11, **kw)
    K = len(shapes) * P
    ref = R.fda_ref_grads(value, shapes, loc_attn, P, go)
    direct = R.fda_ref_grads(value, shapes, loc_attn, P, go, fn=MR.msda_direct)
    for what, a, b in zip(("output", "grad_value", "grad_sampling_loc_attn"), ref, direct):
        assert a.shape == b.shape and float(a.abs().max()) > 0, what
        assert rel_err(a, b) <= 1e-10, (name, what, rel_err(a, b))
    v, la = value.clone().requires_grad_(True), loc_attn.clone().requires_grad_(True)
    gv, gla = torch.autograd.grad(R.fda_ref(v, shapes, la, P), (v, la), go)
    assert rel_err(gv, ref[1]) <= 1e-12 and rel_err(gla, ref[2]) <= 1e-12
    # the logit gradients of a (query, head) sum to zero
    glogit = ref[2][..., 2 * K:]
    assert float(glogit.abs().max()) > 0 and float(glogit.sum(-1).abs().max()) <= 1e-12 * float(glogit.abs().max())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.float16, torch.bfloat16])
def test_make_inputs(dtype):
    for name in sorted(SHAPES):
        kw = SHAPES[name]
        L, P = len(kw["shapes"]), kw["P"]
        value, loc_attn, go = R.make_inputs(dtype=dtype, seed=5, shift=90.0, **kw)
        loc, logits = R.unpack(loc_attn, L, P)
        assert loc_attn.dtype == dtype and loc_attn.shape[-1] == 3 * L * P
        assert MR.min_lattice_distance(loc, kw["shapes"]) >= R.MARGIN
        assert 80 < float(logits.double().mean()) < 100 and float(logits.double().std()) > 1
        # the other tensors are those of the multi-scale reference's builder
        v2, loc2, _, go2 = MR.make_inputs(dtype=dtype, seed=5, **kw)
        assert torch.equal(value, v2) and torch.equal(go, go2) and torch.equal(loc, loc2)


def test_python_surface_without_gpu():
    import modulated_deform_conv_amd as pkg
    from modulated_deform_conv_amd import fda, msda
    for name in ("flash_deform_attn_forward", "flash_deform_attn_backward", "FlashDeformAttnFunction", "flash_deform_attn",
                 "FlashDeformAttn", "pack_loc_attn", "unpack_loc_attn"):
        assert getattr(pkg, name) is getattr(fda, name) and name in pkg.__all__
    shapes = [(4, 4), (2, 2)]
    value, loc_attn, go = R.make_inputs(N=1, M=2, D=4, shapes=shapes, Lq=3, P=2)
    with pytest.raises(NotImplementedError):
        fda.flash_deform_attn(value, shapes, loc_attn, 2)
    with pytest.raises(NotImplementedError):
        fda.FlashDeformAttnFunction.apply(value, torch.tensor(shapes), torch.tensor([0, 16]), loc_attn, 64, 2)
    with pytest.raises(NotImplementedError):
        fda.flash_deform_attn_forward(value, shapes, loc_attn, 2)
    with pytest.raises(NotImplementedError):
        fda.flash_deform_attn_backward(value, shapes, loc_attn, 2, go)
    # the module: MSDeformAttn's constructor, parameters and initialisation, so its checkpoints load
    torch.manual_seed(0)
    ours = fda.FlashDeformAttn(d_model=16, n_levels=2, n_heads=2, n_points=2)
    torch.manual_seed(0)
    theirs = msda.MSDeformAttn(d_model=16, n_levels=2, n_heads=2, n_points=2)
    assert sorted(ours.state_dict()) == sorted(theirs.state_dict())
    assert all(torch.equal(ours.state_dict()[k], v) for k, v in theirs.state_dict().items())
    ours.load_state_dict(theirs.state_dict())
    with pytest.raises(NotImplementedError):
        ours(torch.zeros(1, 3, 16), torch.rand(1, 3, 2, 2), torch.zeros(1, 20, 16), shapes, [0, 16])
    with pytest.raises(ValueError):
        ours(torch.zeros(1, 3, 16), torch.rand(1, 3, 2, 2), torch.zeros(1, 21, 16), shapes, [0, 16])
    # the block has no framework softmax
    import inspect
    assert "softmax" not in inspect.getsource(fda.FlashDeformAttn.forward)
