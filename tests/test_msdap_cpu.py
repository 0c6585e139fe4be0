"""Multi-scale deformable attention with a point count per level without a GPU (include/mdconv_msdap.h): the two references
against each other and, with equal counts, against tests/msda_ref.py; the header as C and as C++; descriptor validation,
its order and its messages; the shape rule; workspace sizing against mdconv_msda_workspace_bytes; the Python wrappers'
argument errors and the module's parameters.  Host code only: no kernel is launched."""
import ctypes
import os
import pathlib
import re
import shutil
import subprocess

import pytest
import torch

from tests import msda_ref as R0
from tests import msdap_ref as R
from tests.util import rel_err

ROOT = pathlib.Path(__file__).resolve().parents[1]
EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -5
F32, F16, BF16 = 0, 1, 3
PAIRINGS = ((F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32))
NAMES = ("output", "grad_value", "grad_sampling_locations", "grad_attention_weights")
DFINE = dict(levels=((8, 8), (4, 4), (2, 2)), points=(3, 6, 3))


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def _desc(capi, dtype=F32, coord_dtype=None, N=2, M=8, D=32, Lq=10, levels=DFINE["levels"], points=DFINE["points"], L=None,
          accumulate=1, flags=0):
    d = capi.MdconvMsdapDesc()
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
    return capi.lib().mdconv_msdap_forward(ctypes.byref(d), p, p, p, p, _null(), ctypes.c_size_t(0), _null())


def _bwd(capi, d, p=None, ws=None, ws_bytes=0):
    p = _null() if p is None else p
    return capi.lib().mdconv_msdap_backward(ctypes.byref(d), p, p, p, p, p, p, p, _null() if ws is None else ws,
                                            ctypes.c_size_t(ws_bytes), _null())


def _ws(capi, d, backward):
    return capi.lib().mdconv_msdap_workspace_bytes(ctypes.byref(d), backward)


def _refused(capi):
    return "shape rule" in capi.last_error()


# ---- the references ----
REF_CASES = {
    "rect_123": dict(N=2, M=3, D=8, shapes=[(6, 5), (3, 3), (1, 1)], points=(1, 2, 3), Lq=7),
    "two_levels_41": dict(N=1, M=2, D=4, shapes=[(16, 16), (2, 3)], points=(4, 1), Lq=5),
}


@pytest.mark.parametrize("name", sorted(REF_CASES))
def test_the_two_references_agree(name):
    """Two independent statements of the contract: grid_sample per level over the split tap axis, and the tap-by-tap
    four-corner gather with the gate.  fp64, 1e-10, output and the three gradients."""
    kw = REF_CASES[name]
    value, loc, attn, go = R.make_inputs(dtype=torch.float64, seed=11, **kw)
    shapes, points = kw["shapes"], kw["points"]
    for l in range(len(shapes)):
        assert R.min_lattice_distance(loc, shapes, points, level=l) >= R.MARGIN
    x, y = R.pixel_positions(loc, shapes, points)
    assert float(x.min()) < -0.5 and float(y.min()) < -0.5   # samples beyond the border take part
    ref = R.msdap_ref_grads(value, shapes, points, loc, attn, go)
    direct = R.msdap_ref_grads(value, shapes, points, loc, attn, go, fn=R.msdap_direct)
    for what, a, b in zip(NAMES, ref, direct):
        assert a.shape == b.shape and float(a.abs().max()) > 0, what
        err = rel_err(a, b)
        print(name, what, "%.3e" % err)
        assert err <= 1e-10, (name, what, err)


@pytest.mark.parametrize("shapes, P", [([(6, 5), (3, 3), (1, 1)], 2), ([(4, 7)], 5)])
def test_equal_counts_are_the_existing_operator(shapes, P):
    """With equal counts both references equal tests.msda_ref.msda_ref on the reshaped tensors, output and gradients."""
    L = len(shapes)
    value, loc, attn, go = R.make_inputs(N=2, M=2, D=4, shapes=shapes, points=(P,) * L, Lq=5, dtype=torch.float64, seed=3)
    loc6, attn5 = loc.view(2, 5, 2, L, P, 2), attn.view(2, 5, 2, L, P)
    assert R0.min_lattice_distance(loc6, shapes) == R.min_lattice_distance(loc, shapes, (P,) * L) >= R.MARGIN
    want = R0.msda_ref_grads(value, shapes, loc6, attn5, go)
    for fn in (R.msdap_ref, R.msdap_direct):
        got = R.msdap_ref_grads(value, shapes, (P,) * L, loc, attn, go, fn=fn)
        for what, a, b in zip(NAMES, got, want):
            assert rel_err(a, b.reshape(a.shape)) <= 1e-10, (fn.__name__, what)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.float16, torch.bfloat16])
def test_make_inputs_keeps_the_margin(dtype):
    for name, kw in sorted(REF_CASES.items()):
        _, loc, attn, _ = R.make_inputs(dtype=dtype, seed=5, **kw)
        assert loc.dtype == dtype and loc.shape[3] == sum(kw["points"]) == attn.shape[3]
        assert R.min_lattice_distance(loc, kw["shapes"], kw["points"]) >= R.MARGIN
        assert float((attn.double().sum(-1) - 1).abs().max()) < 2e-2
    assert R.tap_levels((3, 1, 2)) == [0, 0, 0, 1, 2, 2]


def test_lattice_inputs_are_on_the_lattice():
    shapes, points = [(8, 4), (2, 2), (1, 4)], (2, 1, 3)
    for cdt in (torch.float32, torch.float16):
        value, loc, attn, go = R.make_lattice_inputs(1, 2, 4, shapes, points, coord_dtype=cdt)
        x, y = R.pixel_positions(loc, shapes, points)
        on = ((x - x.round()) == 0) & ((y - y.round()) == 0)
        assert float(on.double().mean()) > 0.9 and loc.shape[3] == 6
        # on the lattice the direct reference is the statement of the convention: finite, and zero outside the gate
        out, gv, gl, ga = R.msdap_ref_grads(value, shapes, points, loc, attn, go, fn=R.msdap_direct)
        gate = R.gate_of(loc, shapes, points)
        assert float(gl[~gate].abs().max()) == 0.0 and float(ga[~gate].abs().max()) == 0.0 and float(gl.abs().max()) > 0


# ---- the C interface ----
def _header_fields():
    hdr = (ROOT / "include" / "mdconv_msdap.h").read_text()
    body = re.search(r"typedef struct mdconv_msdap_desc \{(.*?)\} mdconv_msdap_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return hdr, [re.match(r"\s*int\s+(\w+)", line).group(1) for line in body.split(";") if line.strip()]


def test_descriptor_mirror_matches_the_header(capi):
    hdr, fields = _header_fields()
    assert fields == ["dtype", "coord_dtype", "batch", "heads", "head_channels", "queries", "levels", "points", "level_sz",
                      "accumulate", "flags"]
    assert [f[0] for f in capi.MdconvMsdapDesc._fields_] == fields == [f[0] for f in capi.MdconvMsdaDesc._fields_]
    assert "points[MDCONV_MSDA_MAX_LEVELS]" in hdr and "MDCONV_MSDAP_DESC_INIT" in hdr and '#include "mdconv.h"' in hdr
    assert "UNPINNED" in hdr
    assert ctypes.sizeof(capi.MdconvMsdapDesc) == (7 + 8 + 8 * 2 + 2) * 4
    # the existing surfaces have not moved
    assert ctypes.sizeof(capi.MdconvMsdaDesc) == (8 + 8 * 2 + 2) * 4
    assert capi.lib().mdconv_abi_version() == 2 == capi.ABI_VERSION


def test_exports_are_what_the_header_declares(capi):
    hdr = _header_fields()[0]
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mdconv_msdap_\w+)\s*\(", code))
    assert declared == set(capi.EXPORTS_MSDAP) and len(capi.EXPORTS_MSDAP) == 5
    assert not set(capi.EXPORTS_MSDAP) & (set(capi.EXPORTS) | set(capi.EXPORTS_DAGG))
    for name in capi.EXPORTS_MSDAP:
        assert hasattr(capi.lib(), name), name
    assert "mdconv_msdap" not in (ROOT / "include" / "mdconv.h").read_text()
    assert "mdconv_msdap.h" in (ROOT / "modulated_deform_conv_amd" / "_build.py").read_text()   # editing it rebuilds


C_CALLER = r"""
#include <stdio.h>
#include "mdconv_msdap.h"
int main(void) {
  mdconv_msdap_desc d = MDCONV_MSDAP_DESC_INIT;
  d.batch = 8; d.heads = 8; d.head_channels = 32; d.queries = 300; d.levels = 3;
  d.level_sz[0][0] = 80; d.level_sz[0][1] = 80; d.level_sz[1][0] = 40; d.level_sz[1][1] = 40;
  d.level_sz[2][0] = 20; d.level_sz[2][1] = 20;
  printf("%d %d %d %d %d\n", d.dtype, d.coord_dtype, d.accumulate, d.flags, d.points[7]);
  printf("%d\n", mdconv_msdap_points_len(&d));
  d.points[0] = 3; d.points[1] = 6; d.points[2] = 3;
  printf("%d %d\n", mdconv_msdap_value_len(&d), mdconv_msdap_points_len(&d));
  printf("%zu %d\n", mdconv_msdap_workspace_bytes(&d, 0), mdconv_msdap_workspace_bytes(&d, 1) > 0);
  printf("%d %s\n", mdconv_msdap_forward(&d, NULL, NULL, NULL, NULL, NULL, 0, NULL), mdconv_last_error());
  return 0;
}
"""


def test_a_plain_caller_builds_against_the_header(capi, tmp_path):
    """mdconv_msdap.h compiles as C11 and as C++17, MDCONV_MSDAP_DESC_INIT gives fp32 / accumulate / no flags / zero counts,
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
    assert lines[2] == "%d 12" % (6400 + 1600 + 400), lines
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
        assert capi.last_error().startswith("msdap:")
    assert _ws(capi, _desc(capi, **kw), 0) == 0 and _ws(capi, _desc(capi, **kw), 1) == 0
    assert capi.lib().mdconv_msdap_value_len(ctypes.byref(_desc(capi, **kw))) == -1
    assert capi.lib().mdconv_msdap_points_len(ctypes.byref(_desc(capi, **kw))) == -1


def test_point_counts_validation(capi):
    """A zero count on a level in use is EINVAL naming the level; garbage beyond `levels` is ignored."""
    L = capi.lib()
    assert L.mdconv_msdap_points_len(None) == -1 and L.mdconv_msdap_value_len(None) == -1
    assert _fwd(capi, _desc(capi, points=(3, 0, 3))) == EINVAL
    assert "level 1 has a non-positive point count (0)" in capi.last_error()
    assert _bwd(capi, _desc(capi, points=(3, 6, -2))) == EINVAL and "level 2 " in capi.last_error()
    garbage = _desc(capi, points=(3, 6, 3, 0, -7, 1 << 30, 0, -1))
    assert L.mdconv_msdap_points_len(ctypes.byref(garbage)) == 12
    assert _fwd(capi, garbage) == ENULL
    assert _ws(capi, garbage, 1) == _ws(capi, _desc(capi), 1) > 0
    assert L.mdconv_msdap_points_len(ctypes.byref(_desc(capi, points=(1, 3, 1, 2, 1, 1, 4, 1), levels=((1, 1),) * 8))) == 14
    # the sum itself out of int range: points_len says so, the calls are refused by the shape rule
    huge = _desc(capi, points=((1 << 31) - 1,) * 3)
    assert L.mdconv_msdap_points_len(ctypes.byref(huge)) == -1 and "2^31" in capi.last_error()
    assert _ws(capi, huge, 1) == 0 and _refused(capi) and "4096" in capi.last_error()


def test_order_of_checks(capi):
    """The descriptor, then the pointers (NULL, then alignment), then the shape rule, then the workspace."""
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # non-NULL; nothing dereferences it
    p16 = ctypes.c_void_p((p.value + 15) // 16 * 16)
    big = dict(points=(4090, 6, 1))   # K = 4097: outside the shape rule
    assert capi.lib().mdconv_msdap_points_len(ctypes.byref(_desc(capi, **big))) == 4097
    assert _fwd(capi, _desc(capi, flags=2, **big)) == EINVAL
    assert _fwd(capi, _desc(capi, **big)) == ENULL and _bwd(capi, _desc(capi, **big)) == ENULL
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, **big), p16) == EUNSUPPORTED and _refused(capi)
        assert "sum of points exceeds 4096" in capi.last_error()
        # a misaligned pointer fails before the shape rule: 2 mod 16 is below the 16-byte class of `value`
        assert call(capi, _desc(capi, **big), ctypes.c_void_p(p16.value + 2)) == EINVAL
        assert "value pointer must be 16-byte aligned" in capi.last_error()
    assert _ws(capi, _desc(capi, **big), 1) == 0 and _refused(capi)
    assert _ws(capi, _desc(capi, points=(4090, 5, 1)), 1) > 0
    # the coordinate tensors are "element": a 16-bit call takes 2 mod 4 there, an fp32-coordinate call does not
    L = capi.lib()
    q = ctypes.c_void_p(p16.value + 2)

    def fwd_loc_at(d, loc):
        return L.mdconv_msdap_forward(ctypes.byref(d), p16, loc, p16, p16, _null(), ctypes.c_size_t(0), _null())

    assert fwd_loc_at(_desc(capi, dtype=F16, **big), q) == EUNSUPPORTED
    assert fwd_loc_at(_desc(capi, dtype=F16, coord_dtype=F32, **big), q) == EINVAL
    assert "sampling_locations pointer must be 4-byte aligned" in capi.last_error()
    assert fwd_loc_at(_desc(capi, dtype=F16, **big), ctypes.c_void_p(p16.value + 1)) == EINVAL
    # every argument of the backward in turn, by its class
    names = ("value", "sampling_locations", "attention_weights", "grad_output", "grad_value", "grad_sampling_locations",
             "grad_attention_weights")
    for i, name in enumerate(names):
        args = [p16] * 7
        args[i] = ctypes.c_void_p(p16.value + (2 if name in ("value", "grad_output", "grad_value") else 1))
        assert L.mdconv_msdap_backward(ctypes.byref(_desc(capi, **big)), *args, _null(), ctypes.c_size_t(0), _null()) == EINVAL
        assert capi.last_error().startswith(name + " pointer must be"), capi.last_error()
    # a skipped grad_value is not looked at
    args = [p16] * 7
    args[4] = ctypes.c_void_p(p16.value + 2)
    assert L.mdconv_msdap_backward(ctypes.byref(_desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **big)), *args, _null(),
                                   ctypes.c_size_t(0), _null()) == EUNSUPPORTED
    # inside the rule, pointers given, the workspace missing / too small / misaligned: EWORKSPACE, nothing launched
    need = _ws(capi, _desc(capi), 1)
    assert need > 0
    assert _bwd(capi, _desc(capi), p16) == EWORKSPACE
    assert _bwd(capi, _desc(capi), p16, p16, need - 1) == EWORKSPACE
    assert _bwd(capi, _desc(capi), p16, ctypes.c_void_p(p16.value + 4), need) == EWORKSPACE


def test_shape_rule_refusals_come_before_any_launch(capi):
    buf = (ctypes.c_char * 64)()
    p = ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16)
    one = ((1, 1),)
    for d, word in ((_desc(capi, D=6), "multiple of 4"), (_desc(capi, dtype=F16, D=4), "multiple of 8"),
                    (_desc(capi, dtype=BF16, coord_dtype=F32, D=12), "multiple of 8"),
                    (_desc(capi, levels=((2, 2),) * 8, points=(513,) * 8), "4096"),
                    (_desc(capi, N=1 << 10, M=1 << 6, D=64, levels=((128, 128),), points=(4,)), "2^31"),   # value: 2^32 bytes
                    (_desc(capi, N=1, M=1, D=4, Lq=1 << 22, levels=one, points=(64,)), "2^31")):            # locations
        for call in (_fwd, _bwd):
            assert call(capi, d, p) == EUNSUPPORTED, word
            assert word in capi.last_error() and _refused(capi), capi.last_error()
        assert _ws(capi, d, 1) == 0
    big = dict(N=4096, M=17, D=4, Lq=1, levels=one, points=(1,))
    assert _bwd(capi, _desc(capi, **big), p) == EUNSUPPORTED and "65535" in capi.last_error()
    assert _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **big), 1) == 0 and not _refused(capi)
    assert _ws(capi, _desc(capi, **big), 0) == 0 and not _refused(capi)


@pytest.mark.parametrize("levels, P", [(((8, 8), (4, 4), (2, 2), (1, 1)), 4), (((5, 7),), 5), (((3, 2),) * 8, 1), (((6, 5), (3, 3)), 9)])
def test_workspace_equals_the_existing_operator_at_equal_counts(capi, levels, P):
    """With equal counts the figure is mdconv_msda_workspace_bytes', for every pairing, direction and flag combination."""
    for dtype, cdt in PAIRINGS:
        for flags in (0, 1, 4, 5):
            for accumulate in (0, 1):
                mine = _desc(capi, dtype=dtype, coord_dtype=cdt, Lq=7, levels=levels, points=(P,) * len(levels), flags=flags,
                             accumulate=accumulate)
                theirs = capi.MdconvMsdaDesc()
                theirs.dtype, theirs.coord_dtype, theirs.batch, theirs.heads, theirs.head_channels = dtype, cdt, 2, 8, 32
                theirs.queries, theirs.levels, theirs.points, theirs.accumulate, theirs.flags = 7, len(levels), P, accumulate, flags
                for l, (h, w) in enumerate(levels):
                    theirs.level_sz[l][0], theirs.level_sz[l][1] = h, w
                for backward in (0, 1):
                    want = capi.lib().mdconv_msda_workspace_bytes(ctypes.byref(theirs), backward)
                    assert _ws(capi, mine, backward) == want, (dtype, cdt, flags, backward)
                    assert (want > 0) == (backward == 1 and not flags & 4)
    # unequal counts: the figure follows K, not the split
    assert _ws(capi, _desc(capi, points=(3, 6, 3)), 1) == _ws(capi, _desc(capi, points=(4, 4, 4)), 1) == _ws(capi, _desc(capi, points=(10, 1, 1)), 1)
    assert _ws(capi, _desc(capi, points=(3, 6, 4)), 1) > _ws(capi, _desc(capi, points=(3, 6, 3)), 1)


# ---- the Python surface ----
def test_python_surface_without_gpu():
    import modulated_deform_conv_amd as pkg
    from modulated_deform_conv_amd import msdap
    for name in ("ms_deform_attn_points_forward", "ms_deform_attn_points_backward", "MSDeformAttnPointsFunction",
                 "ms_deform_attn_points", "MSDeformableAttention"):
        assert getattr(pkg, name) is getattr(msdap, name) and name in pkg.__all__ and name in msdap.__all__
    kw = REF_CASES["rect_123"]
    shapes, points = kw["shapes"], kw["points"]
    value, loc, attn, go = R.make_inputs(**kw)
    fwd, bwd = msdap.ms_deform_attn_points_forward, msdap.ms_deform_attn_points_backward
    for call in (lambda: msdap.ms_deform_attn_points(value, shapes, points, loc, attn),
                 lambda: msdap.MSDeformAttnPointsFunction.apply(value, torch.tensor(shapes), torch.tensor(points), loc, attn),
                 lambda: fwd(value, shapes, points, loc, attn), lambda: bwd(value, shapes, points, loc, attn, go)):
        with pytest.raises(NotImplementedError):
            call()
    # the counts against the tap axis, by name
    with pytest.raises(ValueError, match="num_points_list .* sums to 7"):
        fwd(value, shapes, (1, 2, 4), loc, attn)
    with pytest.raises(ValueError, match="num_points_list has 2 entries"):
        fwd(value, shapes, (3, 3), loc, attn)
    with pytest.raises(ValueError, match="non-positive"):
        fwd(value, shapes, (6, 0, 0), loc, attn)
    # shapes, each naming the argument
    for bad, word in ((lambda: fwd(value[:, :-1], shapes, points, loc, attn), "value must be"),
                      (lambda: fwd(value, shapes, points, loc[..., :1], attn), "sampling_locations must be"),
                      (lambda: fwd(value, shapes, points, loc, attn[:, :, :2]), "attention_weights must be"),
                      (lambda: fwd(value, shapes, points, loc, attn, output=go[:, :-1]), "output must be"),
                      (lambda: bwd(value, shapes, points, loc, attn, go[:, :-1]), "grad_output must be"),
                      (lambda: fwd(value[0], shapes, points, loc, attn), r"value must be \[N, S, M, D\]"),
                      (lambda: fwd(value, shapes, points, loc.view(2, 7, 3, 3, 2, 2), attn), "sampling_locations"),
                      (lambda: fwd(value, [(1, 1)] * 9, (1,) * 9, loc, attn), "levels")):
        with pytest.raises(ValueError, match=word):
            bad()
    # dtype pairing
    with pytest.raises(ValueError, match="float32"):
        fwd(value, shapes, points, loc.half(), attn.half())
    with pytest.raises(ValueError):
        fwd(value.half(), shapes, points, loc.bfloat16(), attn.bfloat16())
    with pytest.raises(ValueError, match="attention_weights is"):
        fwd(value.half(), shapes, points, loc, attn.half())
    with pytest.raises(ValueError, match="grad_output is"):
        bwd(value.half(), shapes, points, loc, attn, go)
    with pytest.raises(TypeError):
        fwd(value.double(), shapes, points, loc.double(), attn.double())
    # density
    with pytest.raises(ValueError, match="value must be dense"):
        fwd(value.transpose(1, 2).contiguous().transpose(1, 2), shapes, points, loc, attn)
    with pytest.raises(ValueError, match="sampling_locations must be dense"):
        fwd(value, shapes, points, loc.transpose(1, 2).contiguous().transpose(1, 2), attn)
    # host data: tensors are read
    assert msdap._points(torch.tensor(points), 3) == tuple(points) == msdap._points(list(points), 3)


def test_descriptor_of_a_call():
    from modulated_deform_conv_amd import _capi, msdap
    kw = REF_CASES["rect_123"]
    value, loc, attn, go = R.make_inputs(dtype=torch.bfloat16, coord_dtype=torch.float32, **kw)
    d = msdap._desc(value, loc, tuple(kw["shapes"]), kw["points"], accumulate=0, flags=5)
    assert (d.dtype, d.coord_dtype, d.batch, d.heads, d.head_channels, d.queries, d.levels) == (_capi.BF16, _capi.F32, 2, 3, 8, 7, 3)
    assert list(d.points) == [1, 2, 3, 0, 0, 0, 0, 0] and [tuple(r) for r in d.level_sz][:3] == [(6, 5), (3, 3), (1, 1)]
    assert (d.accumulate, d.flags) == (0, 5)


def test_module_parameters():
    from modulated_deform_conv_amd import MSDeformableAttention
    m = MSDeformableAttention(embed_dim=16, num_heads=2, num_levels=3, num_points=[3, 6, 3])
    assert sorted(m.state_dict()) == sorted([
        "num_points_scale", "sampling_offsets.weight", "sampling_offsets.bias", "attention_weights.weight",
        "attention_weights.bias", "value_proj.weight", "value_proj.bias", "output_proj.weight", "output_proj.bias"])
    assert m.sampling_offsets.weight.shape == (2 * 12 * 2, 16) and m.attention_weights.weight.shape == (2 * 12, 16)
    assert m.value_proj.weight.shape == m.output_proj.weight.shape == (16, 16)
    assert m.num_points_list == [3, 6, 3] and m.offset_scale == 0.5
    want = torch.tensor([1 / 3] * 3 + [1 / 6] * 6 + [1 / 3] * 3)
    assert m.num_points_scale.dtype == torch.float32 and torch.allclose(m.num_points_scale, want, rtol=0, atol=1e-7)
    # the directional bias repeats per level with that level's count: head 0 looks along +x, point p at p + 1 steps
    bias = m.sampling_offsets.bias.detach().view(2, 12, 2)
    steps = torch.tensor([1., 2, 3, 1, 2, 3, 4, 5, 6, 1, 2, 3])
    assert torch.allclose(bias[0, :, 0], steps) and float(bias[0, :, 1].abs().max()) < 1e-6
    assert torch.allclose(bias[1, :, 0], -steps)
    assert float(m.sampling_offsets.weight.detach().abs().max()) == 0.0
    # an int is every level's count
    u = MSDeformableAttention(embed_dim=16, num_heads=2, num_levels=2, num_points=4)
    assert u.num_points_list == [4, 4] and u.num_points_scale.tolist() == [0.25] * 8
    with pytest.raises(NotImplementedError, match="discrete"):
        MSDeformableAttention(embed_dim=16, num_heads=2, num_levels=2, num_points=4, method="discrete")
    with pytest.raises(ValueError):
        MSDeformableAttention(embed_dim=16, num_heads=2, num_levels=2, num_points=[3, 6, 3])
    with pytest.raises(ValueError):
        MSDeformableAttention(embed_dim=15, num_heads=2)
    shapes = [(4, 4), (2, 2), (1, 1)]
    query, flat = torch.zeros(1, 3, 16), torch.zeros(1, 21, 16)
    with pytest.raises(NotImplementedError):   # CPU tensors: no fallback
        m(query, torch.rand(1, 3, 1, 4), flat, shapes)
    with pytest.raises(ValueError, match="equal point counts"):
        m(query, torch.rand(1, 3, 3, 2), flat, shapes)
    with pytest.raises(ValueError):
        m(query, torch.rand(1, 3, 1, 4), torch.zeros(1, 20, 16), shapes)
    # the locations the core receives: boxes, against the formula written out
    seen = []
    m._core = lambda value, shp, pts, loc, w: seen.append((value, shp, pts, loc, w)) or value.new_zeros(1, 3, 16)
    with torch.no_grad():
        m.sampling_offsets.weight.normal_(0, 0.1)
    query = torch.randn(1, 3, 16)
    ref = torch.rand(1, 3, 1, 4)
    m(query, ref, flat, torch.tensor(shapes))
    value, shp, pts, loc, w = seen[0]
    assert value.shape == (1, 21, 2, 8) and shp == tuple(shapes) and list(pts) == [3, 6, 3]
    assert loc.shape == (1, 3, 2, 12, 2) and w.shape == (1, 3, 2, 12)
    assert torch.allclose(w.sum(-1), torch.ones(1, 3, 2))   # one softmax over all K taps of a head
    off = m.sampling_offsets(query).view(1, 3, 2, 12, 2)
    manual = ref[:, :, None, :, :2] + off * want[None, None, None, :, None] * ref[:, :, None, :, 2:] * 0.5
    assert torch.allclose(loc, manual, atol=1e-6)
    # points with equal counts: ref + offset / (W, H) of the tap's level
    seen.clear()
    u._core = m._core
    ref2 = torch.rand(1, 3, 2, 2)
    u(query, ref2, torch.zeros(1, 20, 16), [(4, 4), (2, 2)])
    loc = seen[0][3]
    off = u.sampling_offsets(query).view(1, 3, 2, 2, 4, 2)
    wh = torch.tensor([[4., 4.], [2., 2.]])
    manual = (ref2[:, :, None, :, None, :] + off / wh[None, None, None, :, None, :]).reshape(1, 3, 2, 8, 2)
    assert torch.allclose(loc, manual, atol=1e-6)
