"""Packed deformable attention with a point count per level without a GPU (include/mdconv_fdap.h): the two references
against each other and, with equal counts, against tests/fda_ref.py; the header as C and as C++; descriptor validation, its
order and its messages; the shape rule with the packed tensor's size; the row length; workspace sizing against
mdconv_fda_workspace_bytes and mdconv_msdap_workspace_bytes; the Python wrappers' argument errors, the packing, and the
module's parameters.  Host code only: no kernel is launched."""
import ctypes
import os
import pathlib
import re
import shutil
import subprocess

import pytest
import torch

from tests import fda_ref as R0
from tests import fdap_ref as R
from tests import msdap_ref as MR
from tests.util import rel_err

ROOT = pathlib.Path(__file__).resolve().parents[1]
EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -5
F32, F16, BF16 = 0, 1, 3
PAIRINGS = ((F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32))
NAMES = ("output", "grad_value", "grad_sampling_loc_attn")
DFINE = dict(levels=((8, 8), (4, 4), (2, 2)), points=(3, 6, 3))


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def _desc(capi, dtype=F32, coord_dtype=None, N=2, M=8, D=32, Lq=10, levels=DFINE["levels"], points=DFINE["points"], L=None,
          accumulate=1, flags=0, cls=None):
    d = (cls or capi.MdconvFdapDesc)()
    d.dtype, d.coord_dtype = dtype, dtype if coord_dtype is None else coord_dtype
    d.batch, d.heads, d.head_channels, d.queries = N, M, D, Lq
    d.levels = len(levels) if L is None else L
    for l, (h, w) in enumerate(levels[:8]):
        d.level_sz[l][0], d.level_sz[l][1] = h, w
    for l, p in enumerate(points[:8]):
        d.points[l] = p
    d.accumulate, d.flags = accumulate, flags
    return d


def _null():
    return ctypes.c_void_p(0)


def _fwd(capi, d, p=None):
    p = _null() if p is None else p
    return capi.lib().mdconv_fdap_forward(ctypes.byref(d), p, p, p, _null(), ctypes.c_size_t(0), _null())


def _bwd(capi, d, p=None, ws=None, ws_bytes=0):
    p = _null() if p is None else p
    return capi.lib().mdconv_fdap_backward(ctypes.byref(d), p, p, p, p, p, _null() if ws is None else ws,
                                           ctypes.c_size_t(ws_bytes), _null())


def _ws(capi, d, backward):
    return capi.lib().mdconv_fdap_workspace_bytes(ctypes.byref(d), backward)


def _msdap_ws(capi, backward=1, **kw):
    return capi.lib().mdconv_msdap_workspace_bytes(ctypes.byref(_desc(capi, cls=capi.MdconvMsdapDesc, **kw)), backward)


def _refused(capi):
    return "fdap: outside the shape rule" in capi.last_error()


def _stats(N, Lq, M):
    return (N * Lq * M * 8 + 255) // 256 * 256


# ---- the references ----
REF_CASES = {
    "rect_123": dict(N=2, M=3, D=8, shapes=[(6, 5), (3, 3), (1, 1)], points=(1, 2, 3), Lq=7),
    "two_levels_41": dict(N=1, M=2, D=4, shapes=[(16, 16), (2, 3)], points=(4, 1), Lq=5),
}


@pytest.mark.parametrize("name", sorted(REF_CASES))
def test_the_two_references_agree(name):
    """The fp64 softmax in front of two independent statements of the sampling contract: grid_sample per level over the split
    tap axis, and the tap-by-tap four-corner gather with the gate.  fp64, 1e-10, output and the two gradients."""
    kw = REF_CASES[name]
    value, loc_attn, go = R.make_inputs(dtype=torch.float64, seed=11, **kw)
    shapes, points = kw["shapes"], kw["points"]
    assert loc_attn.shape[-1] == 3 * sum(points)
    ref = R.fdap_ref_grads(value, shapes, points, loc_attn, go)
    direct = R.fdap_ref_grads(value, shapes, points, loc_attn, go, fn=MR.msdap_direct)
    for what, a, b in zip(NAMES, ref, direct):
        assert a.shape == b.shape and float(a.abs().max()) > 0, what
        err = rel_err(a, b)
        print(name, what, "%.3e" % err)
        assert err <= 1e-10, (name, what, err)
    # the forward alone, differentiable, agrees with the gradient route's output
    assert rel_err(R.fdap_ref(value, shapes, points, loc_attn), ref[0]) <= 1e-12
    # per (query, head) the logit gradients of the reference sum to zero
    K = sum(points)
    assert float(ref[2][..., 2 * K:].sum(-1).abs().max()) <= 1e-12 * max(1.0, float(ref[2][..., 2 * K:].abs().max()))


@pytest.mark.parametrize("shapes, P", [([(6, 5), (3, 3), (1, 1)], 2), ([(4, 7)], 5)])
def test_equal_counts_are_the_existing_reference(shapes, P):
    """With equal counts the reference equals tests.fda_ref.fda_ref_grads on the same packed tensor, and the inputs are
    tests.fda_ref's layout: tap = l * P + p."""
    L = len(shapes)
    value, loc_attn, go = R.make_inputs(N=2, M=2, D=4, shapes=shapes, points=(P,) * L, Lq=5, dtype=torch.float64, seed=3)
    want = R0.fda_ref_grads(value, shapes, loc_attn, P, go)
    for fn in (MR.msdap_ref, MR.msdap_direct):
        got = R.fdap_ref_grads(value, shapes, (P,) * L, loc_attn, go, fn=fn)
        for what, a, b in zip(NAMES, got, want):
            assert a.shape == b.shape and rel_err(a, b) <= 1e-10, (fn.__name__, what)
    loc, logits = R.unpack(loc_attn, (P,) * L)
    loc0, logits0 = R0.unpack(loc_attn, L, P)
    assert torch.equal(loc.reshape(loc0.shape), loc0) and torch.equal(logits.reshape(logits0.shape), logits0)


def test_make_inputs_round_the_logits_to_the_coordinate_dtype():
    for dtype, cdt in ((torch.float32, None), (torch.float16, None), (torch.bfloat16, torch.float32)):
        kw = REF_CASES["rect_123"]
        value, loc_attn, go = R.make_inputs(dtype=dtype, coord_dtype=cdt, seed=5, shift=2.0, **kw)
        assert value.dtype == go.dtype == dtype and loc_attn.dtype == (cdt or dtype) and loc_attn.is_contiguous()
        loc, logits = R.unpack(loc_attn, kw["points"])
        assert MR.min_lattice_distance(loc, kw["shapes"], kw["points"]) >= R.MARGIN
        assert 1.0 < float(logits.float().mean()) < 3.0 and float(logits.float().std()) > 2.0
    shapes, points = [(8, 4), (2, 2), (1, 4)], (2, 1, 3)
    value, loc_attn, go = R.make_lattice_inputs(1, 2, 4, shapes, points)
    loc, _ = R.unpack(loc_attn, points)
    x, y = MR.pixel_positions(loc, shapes, points)
    assert float(((x - x.round()) == 0).double().mean()) > 0.9 and not bool(MR.gate_of(loc, shapes, points).all())


# ---- the C interface ----
def _header_fields():
    hdr = (ROOT / "include" / "mdconv_fdap.h").read_text()
    body = re.search(r"typedef struct mdconv_fdap_desc \{(.*?)\} mdconv_fdap_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return hdr, [re.match(r"\s*int\s+(\w+)", line).group(1) for line in body.split(";") if line.strip()]


def test_descriptor_mirror_matches_the_header(capi):
    hdr, fields = _header_fields()
    assert fields == ["dtype", "coord_dtype", "batch", "heads", "head_channels", "queries", "levels", "points", "level_sz",
                      "accumulate", "flags"]
    assert [f[0] for f in capi.MdconvFdapDesc._fields_] == fields == [f[0] for f in capi.MdconvMsdapDesc._fields_]
    assert [f[1] for f in capi.MdconvFdapDesc._fields_] == [f[1] for f in capi.MdconvMsdapDesc._fields_]
    assert "points[MDCONV_MSDA_MAX_LEVELS]" in hdr and "MDCONV_FDAP_DESC_INIT" in hdr and '#include "mdconv.h"' in hdr
    assert "UNPINNED" in hdr
    # what the header owes its reader: the logit gradient of a gated-out tap, non-finite logits, the pointer classes
    flat = " ".join(hdr.split())
    assert "-a[t] * S, not zero" in flat and "Non-finite LOGITS: the result is unspecified" in flat
    assert 'sampling_loc_attn and grad_sampling_loc_attn are "element"' in flat
    assert ctypes.sizeof(capi.MdconvFdapDesc) == ctypes.sizeof(capi.MdconvMsdapDesc) == (7 + 8 + 8 * 2 + 2) * 4
    # the existing surfaces have not moved
    assert ctypes.sizeof(capi.MdconvFdaDesc) == (8 + 8 * 2 + 2) * 4
    assert capi.lib().mdconv_abi_version() == 2 == capi.ABI_VERSION
    assert capi.SAMP_QUERIES["fdap"] == ("value_len", "loc_attn_len")


def test_exports_are_what_the_header_declares(capi):
    hdr = _header_fields()[0]
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mdconv_fdap_\w+)\s*\(", code))
    assert declared == set(capi.EXPORTS_FDAP) and len(capi.EXPORTS_FDAP) == 5
    assert not set(capi.EXPORTS_FDAP) & (set(capi.EXPORTS) | set(capi.EXPORTS_DAGG) | set(capi.EXPORTS_MSDAP))
    for name in capi.EXPORTS_FDAP:
        assert hasattr(capi.lib(), name), name
    assert "mdconv_fdap" not in (ROOT / "include" / "mdconv.h").read_text()
    assert "mdconv_fdap" not in (ROOT / "include" / "mdconv_msdap.h").read_text()
    assert "mdconv_fdap.h" in (ROOT / "modulated_deform_conv_amd" / "_build.py").read_text()   # editing it rebuilds


C_CALLER = r"""
#include <stdio.h>
#include "mdconv_fdap.h"
int main(void) {
  mdconv_fdap_desc d = MDCONV_FDAP_DESC_INIT;
  d.batch = 8; d.heads = 8; d.head_channels = 32; d.queries = 300; d.levels = 3;
  d.level_sz[0][0] = 80; d.level_sz[0][1] = 80; d.level_sz[1][0] = 40; d.level_sz[1][1] = 40;
  d.level_sz[2][0] = 20; d.level_sz[2][1] = 20;
  printf("%d %d %d %d %d\n", d.dtype, d.coord_dtype, d.accumulate, d.flags, d.points[7]);
  printf("%d\n", mdconv_fdap_loc_attn_len(&d));
  d.points[0] = 3; d.points[1] = 6; d.points[2] = 3;
  printf("%d %d\n", mdconv_fdap_value_len(&d), mdconv_fdap_loc_attn_len(&d));
  printf("%zu %d\n", mdconv_fdap_workspace_bytes(&d, 0), mdconv_fdap_workspace_bytes(&d, 1) > 0);
  printf("%d %s\n", mdconv_fdap_forward(&d, NULL, NULL, NULL, NULL, 0, NULL), mdconv_last_error());
  return 0;
}
"""


def test_a_plain_caller_builds_against_the_header(capi, tmp_path):
    """mdconv_fdap.h compiles as C11 and as C++17, MDCONV_FDAP_DESC_INIT gives fp32 / accumulate / no flags / zero counts,
    and a plain C program linked against the library gets through validation and planning without a GPU."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "caller.c"
    src.write_text(C_CALLER)
    libdir = os.path.dirname(capi.LIB_PATH)
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lmdconv_hip", "-Wl,-rpath," + libdir], check=True, capture_output=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert lines[0] == "0 0 1 0 0", lines
    assert lines[1] == "-1", lines   # the counts are still zero
    assert lines[2] == "%d 36" % (6400 + 1600 + 400), lines
    assert lines[3] == "0 1", lines
    assert lines[4].startswith("-2 ") and "value pointer is NULL" in lines[4], lines
    if shutil.which("g++"):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", str(ROOT / "include"), str(src)],
                       check=True, capture_output=True)


def test_valid_descriptor_stops_at_null_pointers(capi):
    for dtype, cdt in PAIRINGS:
        for call in (_fwd, _bwd):
            assert call(capi, _desc(capi, dtype=dtype, coord_dtype=cdt)) == ENULL and "NULL" in capi.last_error()
    assert _fwd(capi, _desc(capi, D=6)) == ENULL   # outside the shape rule as well: the pointer check comes first
    assert _bwd(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT)) == ENULL
    for flags in (0, 1, 4, 5):
        assert _fwd(capi, _desc(capi, flags=flags)) == ENULL and _bwd(capi, _desc(capi, flags=flags)) == ENULL


@pytest.mark.parametrize("kw", [
    dict(dtype=2), dict(dtype=7), dict(dtype=F16 | 0x10), dict(dtype=BF16, coord_dtype=F16), dict(dtype=F16, coord_dtype=BF16),
    dict(dtype=F32, coord_dtype=F16), dict(N=0), dict(M=0), dict(D=0), dict(Lq=0), dict(points=(3, 0, 3)), dict(points=(3, 6, -1)),
    dict(points=(0, 6, 3)), dict(L=0), dict(L=9), dict(L=-1), dict(levels=((8, 8), (0, 4), (2, 2))), dict(flags=2),
    dict(flags=8), dict(flags=1 | 4 | 32), dict(flags=256), dict(accumulate=2), dict(accumulate=-1),
])
def test_invalid_descriptor(capi, kw):
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, **kw)) == EINVAL, kw
        assert capi.last_error().startswith("fdap: ")
    assert _ws(capi, _desc(capi, **kw), 0) == 0 and _ws(capi, _desc(capi, **kw), 1) == 0
    assert capi.lib().mdconv_fdap_value_len(ctypes.byref(_desc(capi, **kw))) == -1
    assert capi.lib().mdconv_fdap_loc_attn_len(ctypes.byref(_desc(capi, **kw))) == -1


def test_point_counts_validation_and_loc_attn_len(capi):
    """A non-positive count on a level in use is EINVAL naming the level; garbage beyond `levels` is ignored;
    mdconv_fdap_loc_attn_len is 3K and mdconv_fdap_value_len is S."""
    L = capi.lib()
    assert L.mdconv_fdap_loc_attn_len(None) == -1 and L.mdconv_fdap_value_len(None) == -1
    assert L.mdconv_fdap_forward(None, _null(), _null(), _null(), None, 0, None) == EINVAL
    assert _fwd(capi, _desc(capi, points=(3, 0, 3))) == EINVAL
    assert capi.last_error() == "fdap: level 1 has a non-positive point count (0)"
    assert _bwd(capi, _desc(capi, points=(3, 6, -2))) == EINVAL and "level 2 " in capi.last_error()
    garbage = _desc(capi, points=(3, 6, 3, 0, -7, 1 << 30, 0, -1))
    assert L.mdconv_fdap_loc_attn_len(ctypes.byref(garbage)) == 36
    assert _fwd(capi, garbage) == ENULL
    assert _ws(capi, garbage, 1) == _ws(capi, _desc(capi), 1) > 0
    assert L.mdconv_fdap_value_len(ctypes.byref(_desc(capi))) == 64 + 16 + 4
    assert L.mdconv_fdap_value_len(ctypes.byref(_desc(capi, L=2))) == 64 + 16
    for levels, points in ((DFINE["levels"], (3, 6, 3)), (((5, 7),), (1,)), (((6, 5), (3, 3), (1, 1)), (1, 2, 3)),
                           (((1, 1),) * 8, (1, 3, 1, 2, 1, 1, 4, 1)), (((3, 3), (5, 4)), (1, 70)), (((2, 2),) * 8, (512,) * 8)):
        assert L.mdconv_fdap_loc_attn_len(ctypes.byref(_desc(capi, levels=levels, points=points))) == 3 * sum(points)
    # rows beyond `levels` are ignored; the figure does not wait for the shape rule (K > 4096 is refused by a call)
    assert L.mdconv_fdap_loc_attn_len(ctypes.byref(_desc(capi, L=2))) == 3 * 9
    # 3K itself out of int range: loc_attn_len says so, the calls are refused by the shape rule
    huge = _desc(capi, points=((1 << 31) - 1,) * 3)
    assert L.mdconv_fdap_loc_attn_len(ctypes.byref(huge)) == -1 and "2^31" in capi.last_error()
    assert L.mdconv_fdap_loc_attn_len(ctypes.byref(_desc(capi, points=(1 << 28, 1 << 28, 1 << 28)))) == -1
    assert _ws(capi, huge, 1) == 0 and _refused(capi) and "4096" in capi.last_error()


def test_order_of_checks(capi):
    """The descriptor (EINVAL), then the pointers -- NULL (ENULL), then alignment (EINVAL naming the argument) --, then the
    shape rule (EUNSUPPORTED), then the workspace (EWORKSPACE).  Fake non-NULL pointers: every call stops before a launch."""
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # non-NULL; nothing dereferences it
    p16 = ctypes.c_void_p((p.value + 15) // 16 * 16)
    big = dict(points=(4090, 6, 1))   # K = 4097: outside the shape rule
    assert capi.lib().mdconv_fdap_loc_attn_len(ctypes.byref(_desc(capi, **big))) == 3 * 4097
    assert _fwd(capi, _desc(capi, flags=2, **big)) == EINVAL and _fwd(capi, _desc(capi, flags=2, **big), p16) == EINVAL
    assert capi.last_error().startswith("fdap: unknown bits 0x2 in flags")
    assert _fwd(capi, _desc(capi, **big)) == ENULL and _bwd(capi, _desc(capi, **big)) == ENULL
    assert capi.last_error() == "value pointer is NULL"
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, **big), p16) == EUNSUPPORTED and _refused(capi)
        assert capi.last_error() == "fdap: outside the shape rule of the operator: the sum of points exceeds 4096"
        # a misaligned pointer fails before the shape rule: 2 mod 16 is below the 16-byte class of `value`
        assert call(capi, _desc(capi, **big), ctypes.c_void_p(p16.value + 2)) == EINVAL
        assert capi.last_error() == "value pointer must be 16-byte aligned"
    assert _ws(capi, _desc(capi, **big), 1) == 0 and _refused(capi)
    assert _ws(capi, _desc(capi, points=(4090, 5, 1)), 1) > 0
    # the packed tensor is "element": a 16-bit call takes 2 mod 4 there, an fp32-coordinate call does not
    L = capi.lib()
    q = ctypes.c_void_p(p16.value + 2)

    def fwd_packed_at(d, la):
        return L.mdconv_fdap_forward(ctypes.byref(d), p16, la, p16, _null(), ctypes.c_size_t(0), _null())

    assert fwd_packed_at(_desc(capi, dtype=F16, **big), q) == EUNSUPPORTED
    assert fwd_packed_at(_desc(capi, dtype=F16, coord_dtype=F32, **big), q) == EINVAL
    assert capi.last_error() == "sampling_loc_attn pointer must be 4-byte aligned"
    assert fwd_packed_at(_desc(capi, dtype=F16, **big), ctypes.c_void_p(p16.value + 1)) == EINVAL
    assert capi.last_error() == "sampling_loc_attn pointer must be 2-byte aligned"
    # a NULL later in the table comes before an alignment fault earlier in it
    assert L.mdconv_fdap_forward(ctypes.byref(_desc(capi, **big)), q, p16, _null(), _null(), ctypes.c_size_t(0), _null()) == ENULL
    assert capi.last_error() == "output pointer is NULL"
    # every argument of the backward in turn, by its class
    names = ("value", "sampling_loc_attn", "grad_output", "grad_value", "grad_sampling_loc_attn")
    for i, name in enumerate(names):
        sixteen = name in ("value", "grad_output", "grad_value")
        args = [p16] * 5
        args[i] = ctypes.c_void_p(p16.value + (2 if sixteen else 1))
        assert L.mdconv_fdap_backward(ctypes.byref(_desc(capi, **big)), *args, _null(), ctypes.c_size_t(0), _null()) == EINVAL
        assert capi.last_error() == "%s pointer must be %d-byte aligned" % (name, 16 if sixteen else 4), capi.last_error()
        args[i] = _null()
        assert L.mdconv_fdap_backward(ctypes.byref(_desc(capi, **big)), *args, _null(), ctypes.c_size_t(0), _null()) == ENULL
        assert capi.last_error() == "%s pointer is NULL" % name
    # a skipped grad_value is not looked at, NULL or misaligned
    for gv in (ctypes.c_void_p(p16.value + 2), _null()):
        args = [p16] * 5
        args[3] = gv
        assert L.mdconv_fdap_backward(ctypes.byref(_desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **big)), *args, _null(),
                                      ctypes.c_size_t(0), _null()) == EUNSUPPORTED
    # inside the rule, pointers given, the workspace missing / too small / misaligned: EWORKSPACE, nothing launched
    need = _ws(capi, _desc(capi), 1)
    assert need > 0
    assert _bwd(capi, _desc(capi), p16) == EWORKSPACE and capi.last_error() == "workspace too small: need %d bytes, have 0" % need
    assert _bwd(capi, _desc(capi), p16, p16, need - 1) == EWORKSPACE
    assert _bwd(capi, _desc(capi), p16, ctypes.c_void_p(p16.value + 4), need) == EWORKSPACE
    assert capi.last_error() == "workspace must be 16-byte aligned"


def test_shape_rule_refusals_come_before_any_launch(capi):
    buf = (ctypes.c_char * 64)()
    p = ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16)
    one = ((1, 1),)
    for d, word in ((_desc(capi, D=6), "multiple of 4"), (_desc(capi, dtype=F16, D=4), "multiple of 8"),
                    (_desc(capi, dtype=BF16, coord_dtype=F32, D=12), "multiple of 8"),
                    (_desc(capi, levels=((2, 2),) * 8, points=(513,) * 8), "4096"),
                    (_desc(capi, N=1 << 10, M=1 << 6, D=64, levels=((128, 128),), points=(4,)), "2^31"),   # value: 2^32 bytes
                    (_desc(capi, N=1, M=1, D=4, Lq=1 << 22, levels=one, points=(64,)), "2^31")):            # locations alone
        for call in (_fwd, _bwd):
            assert call(capi, d, p) == EUNSUPPORTED, word
            assert word in capi.last_error() and _refused(capi), capi.last_error()
        assert _ws(capi, d, 1) == 0
    # the packed tensor alone: N * Lq * M * 3K * 4 = 3 * 2^18 * 3 * 256 * 4 = 2.25 * 2^30 bytes, where the locations of the
    # same shape (1.5 * 2^30) and every other tensor are inside the rule -- the unpacked operator takes the shape
    for points in ((256,), (100, 156)):
        packed = dict(N=1, M=1, D=4, Lq=3 << 18, levels=one * len(points), points=points)
        for call in (_fwd, _bwd):
            assert call(capi, _desc(capi, **packed), p) == EUNSUPPORTED and "2^31" in capi.last_error() and _refused(capi)
        assert _ws(capi, _desc(capi, **packed), 1) == 0 and _msdap_ws(capi, **packed) > 0
        # ... and with 16-bit coordinates it is inside the rule again
        assert _ws(capi, _desc(capi, dtype=F16, **dict(packed, D=8)), 1) > 0
    # batch * heads above 65535: the lists of grad_value only -- the forward and the backward without grad_value take it
    big = dict(N=4096, M=17, D=4, Lq=1, levels=one, points=(1,))
    assert _bwd(capi, _desc(capi, **big), p) == EUNSUPPORTED and "65535" in capi.last_error()
    assert _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **big), 1) == 0 and not _refused(capi)
    assert _ws(capi, _desc(capi, **big), 0) == 0 and not _refused(capi)


@pytest.mark.parametrize("levels, P", [(((8, 8), (4, 4), (2, 2), (1, 1)), 4), (((5, 7),), 5), (((3, 2),) * 8, 1), (((6, 5), (3, 3)), 9)])
def test_workspace_equals_the_packed_operator_at_equal_counts(capi, levels, P):
    """With equal counts the figure is mdconv_fda_workspace_bytes', for every pairing, direction and flag combination."""
    for dtype, cdt in PAIRINGS:
        for flags in (0, 1, 4, 5):
            for accumulate in (0, 1):
                mine = _desc(capi, dtype=dtype, coord_dtype=cdt, Lq=7, levels=levels, points=(P,) * len(levels), flags=flags,
                             accumulate=accumulate)
                theirs = capi.MdconvFdaDesc()
                theirs.dtype, theirs.coord_dtype, theirs.batch, theirs.heads, theirs.head_channels = dtype, cdt, 2, 8, 32
                theirs.queries, theirs.levels, theirs.points, theirs.accumulate, theirs.flags = 7, len(levels), P, accumulate, flags
                for l, (h, w) in enumerate(levels):
                    theirs.level_sz[l][0], theirs.level_sz[l][1] = h, w
                for backward in (0, 1):
                    want = capi.lib().mdconv_fda_workspace_bytes(ctypes.byref(theirs), backward)
                    assert _ws(capi, mine, backward) == want, (dtype, cdt, flags, backward)
                    assert (want > 0) == (backward == 1 and not flags & 4)


def test_workspace_is_the_unpacked_operators_plus_the_statistics(capi):
    """At (3, 6, 3): mdconv_msdap_workspace_bytes for the shape plus 8 bytes per (query, head) in a 256-byte slot behind the
    lists; 0 for the forward and 0 with NO_GRAD_INPUT, whatever else is set."""
    for dtype, cdt in PAIRINGS:
        kw = dict(dtype=dtype, coord_dtype=cdt)
        for flags in (0, 1, 4, 5):
            assert _ws(capi, _desc(capi, flags=flags, **kw), 0) == 0
            assert _ws(capi, _desc(capi, flags=flags, accumulate=0, **kw), 0) == 0
        full = _ws(capi, _desc(capi, **kw), 1)
        det = _ws(capi, _desc(capi, flags=capi.FLAG_DETERMINISTIC, **kw), 1)
        assert full == _msdap_ws(capi, **kw) + _stats(2, 10, 8) and full % 256 == 0
        assert det == _msdap_ws(capi, flags=capi.FLAG_DETERMINISTIC, **kw) + _stats(2, 10, 8) and det >= full
        assert _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **kw), 1) == 0 < full
        assert _ws(capi, _desc(capi, flags=capi.FLAG_DETERMINISTIC | capi.FLAG_NO_GRAD_INPUT, **kw), 1) == 0
        assert _ws(capi, _desc(capi, accumulate=0, **kw), 1) == full
    odd = dict(N=1, M=3, D=8, Lq=7, levels=((6, 5), (3, 3), (1, 1)), points=(1, 2, 3))
    assert _stats(1, 7, 3) == 256 and _ws(capi, _desc(capi, **odd), 1) == _msdap_ws(capi, **odd) + 256
    rows = dict(N=3, M=8, D=32, Lq=300)   # 7200 pairs: 57600 bytes, a multiple of 256
    assert _ws(capi, _desc(capi, **rows), 1) == _msdap_ws(capi, **rows) + 57600
    # the figure follows K, not the split
    assert _ws(capi, _desc(capi, points=(3, 6, 3)), 1) == _ws(capi, _desc(capi, points=(4, 4, 4)), 1)
    assert _ws(capi, _desc(capi, points=(3, 6, 4)), 1) > _ws(capi, _desc(capi, points=(3, 6, 3)), 1)


# ---- the Python surface ----
def test_python_packing_round_trip():
    from modulated_deform_conv_amd import fdap
    gen = torch.Generator().manual_seed(2)
    N, Lq, M, points = 2, 3, 2, (3, 1, 2)
    K = sum(points)
    loc = torch.rand(N, Lq, M, K, 2, generator=gen)
    logits = torch.randn(N, Lq, M, K, generator=gen)
    packed = fdap.pack_loc_attn_points(loc, logits)
    assert packed.shape == (N, Lq, M, 3 * K) and packed.is_contiguous() and torch.equal(packed, R.pack(loc, logits))
    # the layout of the header: x at 2 * tap, y at 2 * tap + 1, logit at 2K + tap
    for tap in range(K):
        assert torch.equal(packed[..., 2 * tap], loc[..., tap, 0]) and torch.equal(packed[..., 2 * tap + 1], loc[..., tap, 1])
        assert torch.equal(packed[..., 2 * K + tap], logits[..., tap])
    back = fdap.unpack_loc_attn_points(packed, points)
    assert back[0].shape == loc.shape and back[1].shape == logits.shape
    assert torch.equal(back[0], loc) and torch.equal(back[1], logits)
    assert all(torch.equal(a, b) for a, b in zip(back, R.unpack(packed, points)))
    # views: writing through them writes the packed tensor
    assert all(b.untyped_storage().data_ptr() == packed.untyped_storage().data_ptr() for b in back)
    back[1][0, 0, 0, 0] = 7.0
    assert float(packed[0, 0, 0, 2 * K]) == 7.0
    assert torch.equal(fdap.unpack_loc_attn_points(packed, torch.tensor(points))[0], back[0])
    with pytest.raises(ValueError, match="fdap: a packed row"):
        fdap.unpack_loc_attn_points(packed, (3, 1, 3))


def test_python_surface_without_gpu():
    import modulated_deform_conv_amd as pkg
    from modulated_deform_conv_amd import fdap, msdap
    for name in ("flash_deform_attn_points_forward", "flash_deform_attn_points_backward", "FlashDeformAttnPointsFunction",
                 "flash_deform_attn_points", "MSDeformableAttentionFused", "pack_loc_attn_points", "unpack_loc_attn_points"):
        assert getattr(pkg, name) is getattr(fdap, name) and name in pkg.__all__ and name in fdap.__all__
    assert issubclass(fdap.MSDeformableAttentionFused, msdap.MSDeformableAttention)
    kw = REF_CASES["rect_123"]
    shapes, points = kw["shapes"], kw["points"]
    value, la, go = R.make_inputs(**kw)
    fwd, bwd = fdap.flash_deform_attn_points_forward, fdap.flash_deform_attn_points_backward
    for call in (lambda: fdap.flash_deform_attn_points(value, shapes, points, la),
                 lambda: fdap.FlashDeformAttnPointsFunction.apply(value, torch.tensor(shapes), torch.tensor(points), la),
                 lambda: fwd(value, shapes, points, la), lambda: bwd(value, shapes, points, la, go)):
        with pytest.raises(NotImplementedError):
            call()
    # the counts against the row, by name
    with pytest.raises(ValueError, match=r"num_points_list .* asks for 3 \* 7"):
        fwd(value, shapes, (1, 2, 4), la)
    with pytest.raises(ValueError, match="num_points_list has 2 entries"):
        fwd(value, shapes, (3, 3), la)
    with pytest.raises(ValueError, match="non-positive"):
        fwd(value, shapes, (6, 0, 0), la)
    # shapes, each naming the argument
    for bad, word in ((lambda: fwd(value[:, :-1], shapes, points, la), "value must be"),
                      (lambda: fwd(value, shapes, points, la[:, :, :2]), "sampling_loc_attn must be"),
                      (lambda: fwd(value, shapes, points, la, output=go[:, :-1]), "output must be"),
                      (lambda: bwd(value, shapes, points, la, go[:, :-1]), "grad_output must be"),
                      (lambda: fwd(value[0], shapes, points, la), r"value must be \[N, S, M, D\]"),
                      (lambda: fwd(value, shapes, points, la.view(2, 7, 3, 6, 3)), "sampling_loc_attn"),
                      (lambda: fwd(value, [(1, 1)] * 9, (1,) * 9, la), "levels")):
        with pytest.raises(ValueError, match=word):
            bad()
    # dtype pairing
    with pytest.raises(ValueError, match="float32"):
        fwd(value, shapes, points, la.half())
    with pytest.raises(ValueError):
        fwd(value.half(), shapes, points, la.bfloat16())
    with pytest.raises(ValueError, match="grad_output is"):
        bwd(value.half(), shapes, points, la, go)
    with pytest.raises(TypeError):
        fwd(value.double(), shapes, points, la.double())
    # density
    with pytest.raises(ValueError, match="value must be dense"):
        fwd(value.transpose(1, 2).contiguous().transpose(1, 2), shapes, points, la)
    with pytest.raises(ValueError, match="sampling_loc_attn must be dense"):
        fwd(value, shapes, points, la.transpose(1, 2).contiguous().transpose(1, 2))


def test_descriptor_of_a_call():
    from modulated_deform_conv_amd import _capi, fdap
    kw = REF_CASES["rect_123"]
    value, la, go = R.make_inputs(dtype=torch.bfloat16, coord_dtype=torch.float32, **kw)
    d = fdap._desc(value, la, tuple(kw["shapes"]), kw["points"], accumulate=0, flags=5)
    assert isinstance(d, _capi.MdconvFdapDesc)
    assert (d.dtype, d.coord_dtype, d.batch, d.heads, d.head_channels, d.queries, d.levels) == (_capi.BF16, _capi.F32, 2, 3, 8, 7, 3)
    assert list(d.points) == [1, 2, 3, 0, 0, 0, 0, 0] and [tuple(r) for r in d.level_sz][:3] == [(6, 5), (3, 3), (1, 1)]
    assert (d.accumulate, d.flags) == (0, 5)


def test_fused_module_has_the_parents_parameters_and_loads_its_checkpoint():
    from modulated_deform_conv_amd import MSDeformableAttention, MSDeformableAttentionFused, flash_deform_attn_points
    torch.manual_seed(4)
    kw = dict(embed_dim=16, num_heads=2, num_levels=3, num_points=[3, 6, 3])
    theirs, ours = MSDeformableAttention(**kw), MSDeformableAttentionFused(**kw)
    assert ours._core is flash_deform_attn_points
    sd = theirs.state_dict()
    assert list(ours.state_dict()) == list(sd)
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert torch.equal(ours.sampling_offsets.bias, theirs.sampling_offsets.bias)   # the same initialisation
    assert torch.equal(ours.num_points_scale, theirs.num_points_scale)
    with torch.no_grad():
        theirs.sampling_offsets.weight.normal_(0, 0.1)
        theirs.attention_weights.weight.normal_(0, 0.3)
        theirs.attention_weights.bias.normal_(0, 0.3)
    result = ours.load_state_dict(theirs.state_dict(), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    assert all(torch.equal(a, b) for a, b in zip(ours.state_dict().values(), theirs.state_dict().values()))
    with pytest.raises(NotImplementedError, match="discrete"):
        MSDeformableAttentionFused(embed_dim=16, num_heads=2, num_levels=2, num_points=4, method="discrete")
    shapes = [(4, 4), (2, 2), (1, 1)]
    query, flat, ref = torch.randn(1, 3, 16), torch.randn(1, 21, 16), torch.rand(1, 3, 1, 4)
    with pytest.raises(NotImplementedError):   # CPU tensors: no fallback
        ours(query, ref, flat, shapes)
    with pytest.raises(ValueError):
        ours(query, ref, torch.zeros(1, 20, 16), shapes)
    # what the two cores receive from the same parameters and inputs: the same value and locations; raw logits where the parent
    # hands over their softmax; one packed tensor [N, Lq, M, 3K]
    seen = []
    theirs._core = lambda value, shp, pts, loc, w: seen.append((value, shp, pts, loc, w)) or value.new_zeros(1, 3, 16)
    ours._core = lambda value, shp, pts, la: seen.append((value, shp, pts, la)) or value.new_zeros(1, 3, 16)
    keep = torch.ones(1, 21, dtype=torch.bool)
    keep[0, 5:9] = False
    theirs(query, ref, flat, shapes, keep)
    ours(query, ref, flat, torch.tensor(shapes), keep)
    (v0, s0, p0, loc0, w0), (v1, s1, p1, la) = seen
    assert torch.equal(v0, v1) and float(v1.detach()[0, 5:9].abs().max()) == 0.0 and s0 == s1 == tuple(shapes) and list(p0) == list(p1) == [3, 6, 3]
    assert la.shape == (1, 3, 2, 36) and la.dtype == torch.float32 and la.is_contiguous()
    assert torch.equal(la[..., :24].unflatten(-1, (12, 2)), loc0)
    logits = ours.attention_weights(query).view(1, 3, 2, 12)
    assert torch.equal(la[..., 24:], logits) and torch.allclose(torch.softmax(la[..., 24:], -1), w0, atol=1e-7)
    import inspect
    assert "softmax" not in inspect.getsource(MSDeformableAttentionFused.forward)
