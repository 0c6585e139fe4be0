"""Deformable aggregation without a GPU (include/mdconv_dagg.h): the two references against each other on every case of
the GPU tests, the descriptor mirror, the header in a plain C11 / C++17 caller, the exports, descriptor validation and the
order of the checks, each shape rule's refusal with its words, the feature length, workspace sizing against a formula
restated here, and the Python argument checks.  Host code only: no kernel is launched."""
import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from tests import dagg_ref as R
from tests.util import rel_err

ROOT = Path(__file__).resolve().parent.parent
EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -5
F32, F16, BF16 = 0, 1, 3
PAIRINGS = ((F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32))
LEVELS = ((4, 4), (2, 2))
NAMES = ("output", "grad_feature", "grad_sampling_location", "grad_weights")


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def _desc(capi, dtype=F32, coord_dtype=None, B=2, cams=2, levels=LEVELS, L=None, C=256, G=8, A=10, P=4, accumulate=1, flags=0):
    d = capi.MdconvDaggDesc()
    d.dtype, d.coord_dtype = dtype, dtype if coord_dtype is None else coord_dtype
    d.batch, d.cams, d.channels, d.groups, d.anchors, d.points = B, cams, C, G, A, P
    d.levels = len(levels) if L is None else L
    for l, (h, w) in enumerate(levels[:8]):
        d.level_sz[l][0], d.level_sz[l][1] = h, w
    d.accumulate, d.flags = accumulate, flags
    return d


def _null():
    return ctypes.c_void_p(0)


def _fwd(capi, d, p=None, ws=None, ws_bytes=0):
    p = _null() if p is None else p
    return capi.lib().mdconv_dagg_forward(ctypes.byref(d), p, p, p, p, _null() if ws is None else ws, ctypes.c_size_t(ws_bytes),
                                          _null())


def _bwd(capi, d, p=None, ws=None, ws_bytes=0, grad_feature=None):
    p = _null() if p is None else p
    gf = p if grad_feature is None else grad_feature
    return capi.lib().mdconv_dagg_backward(ctypes.byref(d), p, p, p, p, gf, p, p, _null() if ws is None else ws,
                                           ctypes.c_size_t(ws_bytes), _null())


def _ws(capi, d, backward):
    return capi.lib().mdconv_dagg_workspace_bytes(ctypes.byref(d), backward)


def _refused(capi):
    return "shape rule" in capi.last_error()


# ---- the references ----
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_two_references_agree(name):
    """Two independent statements of the contract: grid_sample per (camera, level) times the gate, and the explicit
    four-corner gather.  fp64, 1e-10, output and the three gradients."""
    feature, loc, weights, go = R.case_inputs(name, torch.float64)
    shapes = R.CASES[name]["shapes"]
    assert R.min_lattice_distance(loc, shapes) >= R.MARGIN
    gate = R.gate_of(loc)
    assert float(gate.double().mean()) >= 1 / 3 and not bool(gate.all())
    ref = R.dagg_ref_grads(feature, shapes, loc, weights, go)
    direct = R.dagg_ref_grads(feature, shapes, loc, weights, go, fn=R.dagg_direct)
    for what, a, b in zip(NAMES, ref, direct):
        assert a.shape == b.shape, what
        assert float(a.abs().max()) > 0, what
        err = rel_err(a, b)
        print(name, what, "%.3e" % err)
        assert err <= 1e-10, (name, what, err)
    # gated-out triples: exact zeros in both coordinate gradients
    assert float(ref[2][~gate].abs().max()) == 0.0 and float(ref[3][~gate].abs().max()) == 0.0


def _rounds_of(name, dtype):
    """(VG, VL, V, seg, per round: (first vector, one past the last)) of a case, as dagg_plan lays the anchor's row out."""
    from tests import samp_cases as SC
    kw = R.CASES[name]
    ln = SC.lanes(kw["G"] * kw["Dg"], dtype)
    VG = kw["Dg"] * SC.esize(dtype) // 16
    seg = int(VG & (VG - 1) == 0 and VG <= ln["VL"])
    return VG, ln["VL"], ln["V"], seg, [(rd * ln["VL"], min(ln["V"], (rd + 1) * ln["VL"])) for rd in range(ln["rounds"])]


def test_the_group_reduction_cases_are_what_they_claim():
    """The four group-reduction cases reach the branch of dagg_bwd_coord_kernel their comments name, from the lane geometry
    (``samp_cases.lanes``) and VG: ``seg``, the rounds, and where a round's end falls against the groups."""
    whole = lambda VG, lo, hi: [g for g in range(lo // VG, (hi - 1) // VG + 1) if g * VG >= lo and (g + 1) * VG <= hi]
    for name, (seg, rounds) in R.GROUP_CASES.items():
        dtypes = (torch.float16, torch.bfloat16) if name.endswith("16bit") else (torch.float32,)
        for dtype in dtypes:
            got = _rounds_of(name, dtype)
            assert (got[3], len(got[4])) == (seg, rounds), (name, dtype, got)
    # odd_group: three groups of three vectors in the first 9 of 16 lanes, one round
    for name, dtype in (("odd_group", torch.float32), ("odd_group_16bit", torch.float16), ("odd_group_16bit", torch.bfloat16)):
        assert _rounds_of(name, dtype)[:3] == (3, 16, 9)
    # carry_and_whole_groups: rounds 0 and 1 end inside a group and hold whole groups; rounds 1 and 2 begin with a tail
    VG, VL, V, _, rds = _rounds_of("carry_and_whole_groups", torch.float32)
    assert (VG, VL, V) == (24, 64, 192)
    for rd, (lo, hi) in enumerate(rds):
        assert whole(VG, lo, hi), rd
        assert (hi % VG != 0) == (rd < 2) and (lo % VG != 0) == (rd > 0), rd
    assert any(lo % VG and hi % VG for lo, hi in rds)   # the tail of one group, whole groups and the head of the next
    # group_fills_two_rounds: wider than a round; the group, carried over round 0, ends exactly on round 1's end
    VG, VL, V, _, rds = _rounds_of("group_fills_two_rounds", torch.float32)
    assert VG == V == 128 > VL == 64 and rds[1][1] == VG and not whole(VG, *rds[0])
    # group_per_round: a group is a whole round (VG = VL), the widest segmented butterfly
    VG, VL, V, _, rds = _rounds_of("group_per_round", torch.float32)
    assert VG == VL == 64 and V == 128 and [whole(VG, lo, hi) for lo, hi in rds] == [[0], [1]]
    # and the cases from before keep the masked butterfly at VG = 65 only
    assert _rounds_of("two_rounds", torch.float32)[:4] == (65, 64, 65, 0)


def test_the_references_at_the_gate():
    """Exactly 0.0 and 1.0 are out, one step inside both ends is in (pixel -0.5: half the weight falls outside the map), NaN,
    Inf and huge locations equal -3.0, and a NaN weight of a gated-out triple reaches nothing."""
    kw = R.CASES["cams_levels"]
    feature, loc, weights, go = R.case_inputs("cams_levels", torch.float64)
    one = torch.tensor(1.0, dtype=torch.float64)
    vals = [0.0, 1.0, torch.nextafter(torch.tensor(0.0, dtype=torch.float64), one).item(),
            torch.nextafter(one, torch.tensor(0.0, dtype=torch.float64)).item(), -0.25, 1.5]
    for i, v in enumerate(vals):
        loc[0, i, 0, 0, 0] = v
        loc[0, i, 0, 1, 1] = v
    gate = R.gate_of(loc)
    assert gate[0, :6, 0, 0].tolist() == [False, False, True, True, False, False]
    wild = loc.clone()
    weights_nan = weights.clone()
    for v, a in zip((float("nan"), float("inf"), -float("inf"), 3e38), range(4)):
        loc[1, a, 1, 2] = -3.0
        wild[1, a, 1, 2, a % 2] = v
    weights_nan[~R.gate_of(wild)] = float("nan")
    for fn in (R.dagg_ref, R.dagg_direct):
        want = R.dagg_ref_grads(feature, kw["shapes"], loc, weights, go, fn=fn)
        got = R.dagg_ref_grads(feature, kw["shapes"], wild, weights_nan, go, fn=fn)
        for what, a, b in zip(NAMES, got, want):
            assert torch.equal(a, b), what


def test_the_references_with_nothing_inside_the_gate():
    feature, loc, weights, go = R.case_inputs("cams_levels", torch.float64)
    loc = torch.where(loc < 0.5, -3.0, 4.0)
    for fn in (R.dagg_ref, R.dagg_direct):
        for t in R.dagg_ref_grads(feature, R.CASES["cams_levels"]["shapes"], loc, torch.full_like(weights, float("nan")), go, fn=fn):
            assert float(t.abs().max()) == 0.0


def test_the_trace_table_keeps_the_project_kernels_only(tmp_path):
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import bench_dagg
    csv = tmp_path / "stats.csv"
    csv.write_text('"Name","Calls","TotalDurationNs"\n'
                   '"void mdconv::(anonymous namespace)::dagg_gather_kernel<0, 0>(mdconv::DaggGeom, long)",2,3000\n'
                   '"mdconv::(anonymous namespace)::zero_words_kernel(unsigned int*, long)",2,1000\n'
                   '"void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float>>(int)",9,9000\n'
                   '"void at::native::zero_kernel(int)",9,9000\n')
    table = bench_dagg.trace_table(str(csv))
    assert len(table) == 4 and "dagg_gather_kernel<0, 0>" in table[2] and "75 %" in table[2] and "zero_words_kernel" in table[3]


def test_make_inputs_rounds_first_and_keeps_the_margin():
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        for name in ("cams_levels", "g8_d32"):
            feature, loc, weights, go = R.case_inputs(name, dtype)
            assert feature.dtype == go.dtype == loc.dtype == weights.dtype == dtype
            assert R.min_lattice_distance(loc, R.CASES[name]["shapes"]) >= R.MARGIN
    feature, loc, weights, go = R.case_inputs("g8_d32", torch.bfloat16, torch.float32)
    assert (feature.dtype, loc.dtype, weights.dtype, go.dtype) == (torch.bfloat16, torch.float32, torch.float32, torch.bfloat16)
    loc = R.case_inputs("crafted")[1]
    assert bool((loc[R.gate_of(loc)] == torch.tensor(R.CRAFTED_XY).float()).all())


# ---- the C interface ----
def _header_fields():
    hdr = (ROOT / "include" / "mdconv_dagg.h").read_text()
    body = re.search(r"typedef struct mdconv_dagg_desc \{(.*?)\} mdconv_dagg_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return hdr, [re.match(r"\s*int\s+(\w+)", line).group(1) for line in body.split(";") if line.strip()]


def test_descriptor_mirror_matches_the_header(capi):
    hdr, fields = _header_fields()
    assert fields == ["dtype", "coord_dtype", "batch", "cams", "levels", "level_sz", "channels", "groups", "anchors", "points",
                      "accumulate", "flags"]
    assert [f[0] for f in capi.MdconvDaggDesc._fields_] == fields
    assert "level_sz[MDCONV_MSDA_MAX_LEVELS][2]" in hdr and "MDCONV_DAGG_DESC_INIT" in hdr and '#include "mdconv.h"' in hdr
    assert "UNPINNED" in hdr
    assert ctypes.sizeof(capi.MdconvDaggDesc) == (5 + 8 * 2 + 6) * 4
    assert capi.lib().mdconv_abi_version() == 2 == capi.ABI_VERSION


def test_exports_are_what_the_header_declares(capi):
    hdr = _header_fields()[0]
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mdconv_dagg_\w+)\s*\(", code))
    assert declared == set(capi.EXPORTS_DAGG) and len(capi.EXPORTS_DAGG) == 4
    assert not set(capi.EXPORTS_DAGG) & set(capi.EXPORTS)
    for name in capi.EXPORTS_DAGG:
        assert hasattr(capi.lib(), name), name
    # nothing of this operator in mdconv.h: its own tests count the entry points there
    assert "mdconv_dagg" not in (ROOT / "include" / "mdconv.h").read_text()


C_CALLER = r"""
#include <stdio.h>
#include "mdconv_dagg.h"
int main(void) {
  mdconv_dagg_desc d = MDCONV_DAGG_DESC_INIT;
  d.batch = 1; d.cams = 6; d.levels = 2; d.level_sz[0][0] = 8; d.level_sz[0][1] = 22; d.level_sz[1][0] = 4; d.level_sz[1][1] = 11;
  d.channels = 256; d.groups = 8; d.anchors = 900; d.points = 13;
  printf("%d %d %d %d\n", d.dtype, d.accumulate, d.flags, mdconv_dagg_feature_len(&d));
  printf("%zu %d\n", mdconv_dagg_workspace_bytes(&d, 0), mdconv_dagg_workspace_bytes(&d, 1) > 0);
  printf("%d %s\n", mdconv_dagg_forward(&d, NULL, NULL, NULL, NULL, NULL, 0, NULL), mdconv_last_error());
  return 0;
}
"""


def test_a_plain_caller_builds_against_the_header(capi, tmp_path):
    """mdconv_dagg.h compiles as C11 and as C++17, MDCONV_DAGG_DESC_INIT gives fp32 / accumulate / no flags, and a plain C
    program linked against the library gets through validation and planning without a GPU."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "caller.c"
    src.write_text(C_CALLER)
    libdir = os.path.dirname(capi.LIB_PATH)
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lmdconv_hip", "-Wl,-rpath," + libdir], check=True, capture_output=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert lines[0] == "0 1 0 %d" % (6 * (8 * 22 + 4 * 11)), lines
    assert lines[1] == "0 1", lines
    assert lines[2].startswith("-2 ") and "feature pointer is NULL" in lines[2], lines
    if shutil.which("g++"):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", str(ROOT / "include"), str(src)],
                       check=True, capture_output=True)


def test_valid_descriptor_stops_at_null_pointers(capi):
    for dtype, cdt in PAIRINGS:
        for call in (_fwd, _bwd):
            assert call(capi, _desc(capi, dtype=dtype, coord_dtype=cdt)) == ENULL and "NULL" in capi.last_error()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # grad_feature alone may be NULL with NO_GRAD_INPUT (the call then has no workspace and would launch: it is only sized)
    assert _bwd(capi, _desc(capi), p, grad_feature=_null()) == ENULL and "grad_feature pointer is NULL" in capi.last_error()
    assert _bwd(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT)) == ENULL and "feature pointer is NULL" in capi.last_error()
    for flags in (0, 1, 4, 5):
        assert _fwd(capi, _desc(capi, flags=flags)) == ENULL and _bwd(capi, _desc(capi, flags=flags)) == ENULL


@pytest.mark.parametrize("kw", [
    dict(dtype=2), dict(dtype=7), dict(dtype=F16 | 0x10), dict(dtype=BF16, coord_dtype=F16), dict(dtype=F16, coord_dtype=BF16),
    dict(dtype=F32, coord_dtype=F16), dict(B=0), dict(cams=0), dict(C=0), dict(G=0), dict(A=0), dict(P=0), dict(P=-1),
    dict(C=256, G=7), dict(L=0), dict(L=9), dict(L=-1), dict(levels=((4, 4), (0, 2))), dict(levels=((4, -1),)), dict(flags=2),
    dict(flags=8), dict(flags=1 | 4 | 32), dict(flags=256), dict(accumulate=2), dict(accumulate=-1),
])
def test_invalid_descriptor(capi, kw):
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, **kw)) == EINVAL, kw
        assert capi.last_error().startswith("dagg:")
    assert _ws(capi, _desc(capi, **kw), 0) == 0 and _ws(capi, _desc(capi, **kw), 1) == 0
    assert capi.lib().mdconv_dagg_feature_len(ctypes.byref(_desc(capi, **kw))) == -1
    assert capi.lib().mdconv_dagg_feature_len(None) == -1


def test_order_of_checks(capi):
    """The descriptor, then the pointers (NULL, then alignment), then the shape rule, then the workspace."""
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # non-NULL; nothing dereferences it
    p16 = ctypes.c_void_p((p.value + 15) // 16 * 16)
    odd = dict(C=48, G=8)   # Dg = 6: outside the shape rule
    assert _fwd(capi, _desc(capi, flags=2, **odd)) == EINVAL
    assert _fwd(capi, _desc(capi, **odd)) == ENULL and _bwd(capi, _desc(capi, **odd)) == ENULL
    assert _bwd(capi, _desc(capi, **odd), p16) == EUNSUPPORTED and _refused(capi)
    # alignment after NULL, before the shape rule: 2 mod 16 is below the 16-byte class of `feature`
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, **odd), ctypes.c_void_p(p16.value + 2)) == EINVAL
        assert "feature pointer must be 16-byte aligned" in capi.last_error()
    # the coordinate tensors are "element": a 16-bit call takes 2 mod 4 there, an fp32-coordinate call does not
    L = capi.lib()
    q = ctypes.c_void_p(p16.value + 2)

    def fwd_loc_at(d, loc):
        return L.mdconv_dagg_forward(ctypes.byref(d), p16, loc, p16, p16, _null(), ctypes.c_size_t(0), _null())

    assert fwd_loc_at(_desc(capi, dtype=F16, **odd), q) == EUNSUPPORTED
    assert fwd_loc_at(_desc(capi, dtype=F16, coord_dtype=F32, **odd), q) == EINVAL
    assert "sampling_location pointer must be 4-byte aligned" in capi.last_error()
    assert fwd_loc_at(_desc(capi, dtype=F16, **odd), ctypes.c_void_p(p16.value + 1)) == EINVAL
    # every argument of the backward in turn, by its class
    names = ("feature", "sampling_location", "weights", "grad_output", "grad_feature", "grad_sampling_location", "grad_weights")
    for i, name in enumerate(names):
        args = [p16] * 7
        args[i] = ctypes.c_void_p(p16.value + (2 if name in ("feature", "grad_output", "grad_feature") else 1))
        assert L.mdconv_dagg_backward(ctypes.byref(_desc(capi, **odd)), *args, _null(), ctypes.c_size_t(0), _null()) == EINVAL
        assert capi.last_error().startswith(name + " pointer must be"), capi.last_error()
    # a skipped grad_feature is not looked at
    args = [p16] * 7
    args[4] = ctypes.c_void_p(p16.value + 2)
    assert L.mdconv_dagg_backward(ctypes.byref(_desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **odd)), *args, _null(),
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
    for d, word in ((_desc(capi, C=48, G=8), "multiple of 4"), (_desc(capi, dtype=F16, C=32, G=8), "multiple of 8"),
                    (_desc(capi, dtype=BF16, coord_dtype=F32, C=96, G=8), "multiple of 8"),
                    (_desc(capi, B=1 << 6, cams=1 << 4, C=1 << 10, levels=((32, 32),)), "2^31"),      # feature: 2^32 bytes
                    (_desc(capi, B=1, cams=1, C=4, G=1, levels=((1 << 16, 1 << 15),)), "2^31"),        # one map: 2^31 rows
                    (_desc(capi, B=1, cams=1 << 16, C=4, G=1, levels=((1 << 8, 1 << 7),)), "2^31"),    # cams * S_cam rows
                    (_desc(capi, B=1, C=4, G=1, A=1 << 20, P=1 << 8, cams=1, levels=one), "2^31"),     # locations: 2^31 bytes
                    (_desc(capi, B=1, C=1 << 12, G=1 << 10, A=1 << 10, P=1 << 6, cams=1 << 3, levels=one), "2^31")):   # weights
        for call in (_fwd, _bwd):
            assert call(capi, d, p) == EUNSUPPORTED, word
            assert word in capi.last_error() and _refused(capi), capi.last_error()
        assert _ws(capi, d, 1) == 0
    assert capi.lib().mdconv_dagg_feature_len(ctypes.byref(_desc(capi, cams=1 << 16, levels=((1 << 8, 1 << 7),)))) == -1
    # batch above 65535: the lists of grad_feature only -- the forward and the backward without grad_feature take it
    big = dict(B=65536, cams=1, C=4, G=1, A=1, P=1, levels=one)
    assert _bwd(capi, _desc(capi, **big), p) == EUNSUPPORTED and "65535" in capi.last_error()
    assert _ws(capi, _desc(capi, **big), 1) == 0
    # (the calls that would go on to launch are only sized: a workspace query plans the same call)
    assert _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **big), 1) == 0 and not _refused(capi)
    assert _ws(capi, _desc(capi, **big), 0) == 0 and not _refused(capi)
    # the list stride A*P*cams*L*4: 2^31 here, while weights (A*P*cams*L*G elements of 2 bytes) stay below 2^31 bytes
    stride = dict(dtype=F16, B=1, cams=1 << 3, C=8, G=1, A=1 << 16, P=1 << 7, levels=one * 8)
    assert _bwd(capi, _desc(capi, **stride), p) == EUNSUPPORTED
    assert "list stride" in capi.last_error() and "* 4" in capi.last_error()
    assert _ws(capi, _desc(capi, **stride), 1) == 0 and _refused(capi)
    assert _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **stride), 1) == 0 and not _refused(capi)
    assert _ws(capi, _desc(capi, **stride), 0) == 0 and not _refused(capi)
    assert _ws(capi, _desc(capi, **dict(stride, A=(1 << 16) - 1)), 1) > 0


def test_feature_len(capi):
    L = capi.lib()
    assert L.mdconv_dagg_feature_len(ctypes.byref(_desc(capi))) == 2 * (16 + 4)
    assert L.mdconv_dagg_feature_len(ctypes.byref(_desc(capi, cams=6, levels=((64, 176), (32, 88), (16, 44), (8, 22))))) == 89760
    # rows beyond `levels` are ignored
    assert L.mdconv_dagg_feature_len(ctypes.byref(_desc(capi, cams=3, levels=((4, 6), (2, 3), (1, 1)), L=2))) == 3 * 30


def _au(x):
    return (x + 255) // 256 * 256


def _ws_formula(B, S, A, P, cams, L, det):
    """Counters and row pointers per (image, row), A*P*cams*L*4 entries of 16 bytes per image, the sort scratch of the same
    size in deterministic mode; every slot rounded up to 256 bytes."""
    stride = A * P * cams * L * 4
    return _au(B * S * 4) + _au(B * (S + 1) * 4) + _au(B * stride * 16) + (_au(B * stride * 16) if det else 0)


def test_workspace_bytes(capi):
    for dtype, cdt in PAIRINGS:
        kw = dict(dtype=dtype, coord_dtype=cdt)
        for flags in (0, 1, 4, 5):
            assert _ws(capi, _desc(capi, flags=flags, **kw), 0) == 0
        full = _ws(capi, _desc(capi, **kw), 1)
        det = _ws(capi, _desc(capi, flags=capi.FLAG_DETERMINISTIC, **kw), 1)
        assert full == _ws_formula(2, 40, 10, 4, 2, 2, False) and det == _ws_formula(2, 40, 10, 4, 2, 2, True)
        assert _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **kw), 1) == 0
        assert _ws(capi, _desc(capi, flags=capi.FLAG_DETERMINISTIC | capi.FLAG_NO_GRAD_INPUT, **kw), 1) == 0
        assert _ws(capi, _desc(capi, accumulate=0, **kw), 1) == full
    # the lists are shared by all groups: neither the channels nor the groups change the figure
    assert _ws(capi, _desc(capi, C=512, G=4), 1) == _ws(capi, _desc(capi, C=64, G=16), 1) == _ws(capi, _desc(capi), 1)
    for name, kw in R.CASES.items():
        shapes = kw["shapes"]
        d = _desc(capi, B=kw["B"], cams=kw["cams"], levels=shapes, C=kw["G"] * kw["Dg"], G=kw["G"], A=kw["A"], P=kw["P"])
        S = kw["cams"] * sum(h * w for h, w in shapes)
        assert capi.lib().mdconv_dagg_feature_len(ctypes.byref(d)) == S
        for det in (False, True):
            d.flags = capi.FLAG_DETERMINISTIC if det else 0
            assert _ws(capi, d, 1) == _ws_formula(kw["B"], S, kw["A"], kw["P"], kw["cams"], len(shapes), det), name


# ---- the Python surface ----
def test_python_surface_without_gpu():
    import modulated_deform_conv_amd as pkg
    from modulated_deform_conv_amd import dagg
    for name in ("deformable_aggregation_forward", "deformable_aggregation_backward", "DeformableAggregationFunction",
                 "deformable_aggregation", "feature_maps_format"):
        assert getattr(pkg, name) is getattr(dagg, name) and name in pkg.__all__ and name in dagg.__all__
    assert not hasattr(dagg, "DeformableAggregation")   # no nn.Module: the published one is model code
    kw = R.CASES["cams_levels"]
    shapes = kw["shapes"]
    feature, loc, weights, go = R.case_inputs("cams_levels")
    for call in (lambda: dagg.deformable_aggregation(feature, shapes, loc, weights),
                 lambda: dagg.DeformableAggregationFunction.apply(feature, torch.tensor([shapes] * 3), None, loc, weights),
                 lambda: dagg.deformable_aggregation_forward(feature, shapes, loc, weights),
                 lambda: dagg.deformable_aggregation_backward(feature, shapes, loc, weights, go)):
        with pytest.raises(NotImplementedError):
            call()
    fwd, bwd = dagg.deformable_aggregation_forward, dagg.deformable_aggregation_backward
    # shapes
    for bad in (lambda: fwd(feature[:, :-1], shapes, loc, weights), lambda: fwd(feature, shapes[:2], loc, weights),
                lambda: fwd(feature, shapes, loc[..., :1], weights), lambda: fwd(feature, shapes, loc, weights[:, :, :1]),
                lambda: fwd(feature, shapes, loc, weights, output=go[:, :-1]), lambda: bwd(feature, shapes, loc, weights, go[:, :-1]),
                lambda: fwd(feature[0], shapes, loc, weights), lambda: fwd(feature, [(1, 1)] * 9, loc, weights)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="multiple of the groups"):
        fwd(feature, shapes, loc, torch.zeros(2, 7, 2, 3, 3, 5))
    # dtype pairing
    with pytest.raises(ValueError, match="float32"):
        fwd(feature, shapes, loc.half(), weights.half())
    with pytest.raises(ValueError):
        fwd(feature.half(), shapes, loc.bfloat16(), weights.bfloat16())
    with pytest.raises(ValueError):
        fwd(feature.half(), shapes, loc, weights.half())
    with pytest.raises(ValueError):
        bwd(feature.half(), shapes, loc, weights, go)
    with pytest.raises(TypeError):
        fwd(feature.double(), shapes, loc.double(), weights.double())
    # density
    with pytest.raises(ValueError, match="contiguous"):
        fwd(feature.transpose(1, 2).contiguous().transpose(1, 2), shapes, loc, weights)
    with pytest.raises(ValueError, match="contiguous"):
        fwd(feature, shapes, loc.flip(-1).transpose(1, 2).contiguous().transpose(1, 2), weights)
    # the published [cams, levels, 2] spatial_shape; cameras with unequal extents are refused by name
    assert dagg._shapes(torch.tensor([shapes] * 3)) == tuple(shapes) == dagg._shapes(shapes) == dagg._shapes(torch.tensor(shapes))
    with pytest.raises(ValueError, match="every camera must have the same level extents"):
        dagg._shapes([shapes, shapes, [(4, 6), (2, 3), (1, 2)]])
    with pytest.raises(ValueError, match="every camera must have the same level extents"):
        dagg.deformable_aggregation(feature, torch.tensor([shapes, shapes, [(4, 5), (2, 3), (1, 1)]]), loc, weights)
    # scale_start_index: host data is checked, before the device is looked at
    good = [[c * 31 + s for s in (0, 24, 30)] for c in range(3)]
    dagg._check_starts(tuple(shapes), 3, good)
    dagg._check_starts(tuple(shapes), 3, torch.tensor(good))
    dagg._check_starts(tuple(shapes), 3, [0, 24, 30])
    dagg._check_starts(tuple(shapes), 3, None)
    with pytest.raises(ValueError, match="cumulative"):
        dagg.deformable_aggregation(feature, shapes, loc, weights, [[0, 24, 30], [31, 55, 61], [62, 86, 93]])
    with pytest.raises(ValueError, match="cumulative"):
        dagg.DeformableAggregationFunction.apply(feature, shapes, torch.tensor([0, 24, 31]), loc, weights)


def test_feature_maps_format():
    from modulated_deform_conv_amd import dagg
    torch.manual_seed(3)
    B, cams, C = 2, 3, 8
    shapes = [(4, 6), (2, 3), (1, 1)]
    maps = [torch.randn(B, cams, C, h, w) for h, w in shapes]
    feature, spatial_shape, starts = dagg.feature_maps_format(maps)
    assert feature.shape == (B, cams * 31, C) and feature.is_contiguous()
    assert spatial_shape.tolist() == [[list(s) for s in shapes]] * cams
    assert starts.tolist() == [[c * 31 + s for s in (0, 24, 30)] for c in range(cams)]
    assert not spatial_shape.is_cuda and not starts.is_cuda
    for cam in range(cams):
        for l, (h, w) in enumerate(shapes):
            r0 = int(starts[cam, l])
            assert torch.equal(feature[:, r0:r0 + h * w].reshape(B, h, w, C).permute(0, 3, 1, 2), maps[l][:, cam])
    dagg._check_starts(dagg._shapes(spatial_shape), cams, starts)
    with pytest.raises(ValueError):
        dagg.feature_maps_format([maps[0], maps[1][:, :2]])
