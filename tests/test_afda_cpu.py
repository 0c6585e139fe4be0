"""Anchored packed deformable attention without a GPU (include/mdconv_afda.h): the reference against the reference of the
packed operator fed with ``MSDeformableAttention._locations``' tensor; the conditions ``make_inputs`` asserts, for every
case the GPU tests use; the header as C and as C++; descriptor validation, its order and its messages; the shape rule;
workspace sizing against mdconv_fdap_workspace_bytes; the Python wrappers' argument errors and the module's parameters and
fused linear.  Host code only: no kernel is launched."""
import ctypes
import os
import pathlib
import re
import shutil
import subprocess

import pytest
import torch

from tests import afda_ref as R
from tests import fdap_ref as FR
from tests import msdap_ref as MR
from tests.util import rel_err

ROOT = pathlib.Path(__file__).resolve().parents[1]
EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -5
F32, F16, BF16 = 0, 1, 3
PAIRINGS = ((F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32))
DFINE = dict(levels=((8, 8), (4, 4), (2, 2)), points=(3, 6, 3))


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def _desc(capi, dtype=F32, coord_dtype=None, N=2, M=8, D=32, Lq=10, levels=DFINE["levels"], points=DFINE["points"], L=None,
          accumulate=1, flags=0, ref_levels=1, ref_comps=4, offset_scale=0.5, grad_reference=1, cls=None):
    d = (cls or capi.MdconvAfdaDesc)()
    d.dtype, d.coord_dtype = dtype, dtype if coord_dtype is None else coord_dtype
    d.batch, d.heads, d.head_channels, d.queries = N, M, D, Lq
    d.levels = len(levels) if L is None else L
    for l, (h, w) in enumerate(levels[:8]):
        d.level_sz[l][0], d.level_sz[l][1] = h, w
    for l, p in enumerate(points[:8]):
        d.points[l] = p
    d.accumulate, d.flags = accumulate, flags
    if cls is None:
        d.ref_levels, d.ref_comps, d.offset_scale, d.grad_reference = ref_levels, ref_comps, offset_scale, grad_reference
    return d


def _null():
    return ctypes.c_void_p(0)


def _fwd(capi, d, p=None):
    p = _null() if p is None else p
    return capi.lib().mdconv_afda_forward(ctypes.byref(d), p, p, p, p, _null(), ctypes.c_size_t(0), _null())


def _bwd(capi, d, p=None, ws=None, ws_bytes=0):
    p = _null() if p is None else p
    return capi.lib().mdconv_afda_backward(ctypes.byref(d), p, p, p, p, p, p, p, _null() if ws is None else ws,
                                           ctypes.c_size_t(ws_bytes), _null())


def _ws(capi, d, backward):
    return capi.lib().mdconv_afda_workspace_bytes(ctypes.byref(d), backward)


def _fdap_ws(capi, backward=1, **kw):
    for k in ("ref_levels", "ref_comps", "offset_scale", "grad_reference"):
        kw.pop(k, None)
    return capi.lib().mdconv_fdap_workspace_bytes(ctypes.byref(_desc(capi, cls=capi.MdconvFdapDesc, **kw)), backward)


def _refused(capi):
    return "afda: outside the shape rule" in capi.last_error()


def _partials(N, Lq, M, Lr, R):
    return (N * Lq * M * Lr * R * 4 + 255) // 256 * 256


# ---- the reference ----
def _parent_locations(mod, query_shape, ref, shapes, offs):
    """``MSDeformableAttention._locations`` with the linear's output replaced by ``offs`` [N, Lq, M, K, 2]."""
    mod.__dict__["sampling_offsets"] = lambda q: offs.reshape(offs.shape[0], offs.shape[1], -1)
    try:
        return mod._locations(torch.zeros(query_shape), ref, shapes)
    finally:
        del mod.__dict__["sampling_offsets"]


@pytest.mark.parametrize("Lr, comps, points, offset_scale", [(1, 4, (3, 6, 3), 0.5), (3, 4, (3, 6, 3), 0.5), (3, 4, (1, 2, 3), 0.25),
                                                         (3, 2, (2, 2, 2), 0.5), (1, 4, (4, 4, 4), 1.5)])
def test_reference_equals_the_packed_reference_behind_the_published_locations(Lr, comps, points, offset_scale):
    """``afda_ref`` against ``fdap_ref`` fed with the tensor ``MSDeformableAttention._locations`` forms from the same
    offsets and reference, for the forms that block accepts (two-component references: equal counts only): output and the
    gradients of value and of the packed row (the offset part through the chain rule of the location formula)."""
    from modulated_deform_conv_amd.msdap import MSDeformableAttention
    shapes = [(6, 5), (3, 3), (2, 4)]
    N, M, D, Lq, K = 2, 2, 4, 5, sum(points)
    value, ref, offs_attn, go = R.make_inputs(N, M, D, shapes, points, Lq, Lr=Lr, R=comps, seed=3, offset_scale=offset_scale)
    assert ref.shape == (N, Lq, Lr, comps) and ref.dtype == torch.float32 and offs_attn.shape == (N, Lq, M, 3 * K)
    offs, logits = FR.unpack(offs_attn, points)
    mod = MSDeformableAttention(embed_dim=M * D, num_heads=M, num_levels=3, num_points=list(points), offset_scale=offset_scale)
    r = ref.clone().requires_grad_(True)
    o = offs.clone().requires_grad_(True)
    loc = _parent_locations(mod, (N, Lq, M * D), r, shapes, o)
    assert loc.shape == (N, Lq, M, K, 2) and loc.dtype == torch.float32
    assert rel_err(R.locations(ref, shapes, points, offs, offset_scale), loc) <= 1e-6   # (theirs is formed in fp32)
    want = FR.fdap_ref_grads(value, shapes, points, FR.pack(loc.detach().double(), logits.double()), go)
    got = R.afda_ref_grads(value, shapes, points, ref, offs_attn, go, offset_scale)
    assert rel_err(got[0], want[0]) <= 1e-5 and rel_err(got[1], want[1]) <= 1e-5
    # the packed gradient: the logits' as it stands, the offsets' and the reference's through their block's own autograd
    gloc, glogit = FR.unpack(want[2], points)
    gr, go_ = torch.autograd.grad(loc, (r, o), gloc.float())
    assert rel_err(FR.unpack(got[3], points)[1], glogit) <= 1e-5
    assert rel_err(FR.unpack(got[3], points)[0], go_) <= 1e-5
    assert rel_err(got[2], gr) <= 1e-5 and float(got[2].abs().max()) > 0
    direct = R.afda_ref_grads(value, shapes, points, ref, offs_attn, go, offset_scale, fn=MR.msdap_direct)
    for a, b in zip(got, direct):
        assert rel_err(a, b) <= 1e-10


def test_one_row_for_all_levels_with_two_components():
    """(Lr, R) = (1, 2), which the operator takes and the published block does not: one point for all levels."""
    shapes, points = [(4, 4), (2, 3)], (2, 1)
    value, ref, offs_attn, go = R.make_inputs(1, 2, 4, shapes, points, 5, Lr=1, R=2, seed=4)
    assert ref.shape == (1, 5, 1, 2)
    loc = R.derived(ref, shapes, points, offs_attn)
    offs = FR.unpack(offs_attn, points)[0].double()
    wh = MR._tap_wh(shapes, points)
    assert torch.equal(loc, ref.double()[:, :, None, [0, 0, 0], :] + offs * (1.0 / wh))


def _gpu_cases():
    """Every (case, form, pairing) the GPU tests draw with ``make_inputs``."""
    from tests import test_gpu_afda as G
    seen = []
    for name, (Lr, R), dtype, cdt in G.PARITY:
        seen.append((G.CASES[name], Lr, R, dtype, cdt, len(name) + 7))
    for seed in range(16):
        kw, (Lr, R), dtype, cdt = G._random_case(seed)
        seen.append((kw, Lr, R, dtype, cdt, seed))
    return seen


def test_make_inputs_conditions_hold_for_every_gpu_case():
    """``make_inputs`` asserts the margin per level and a gate that is neither all true nor all false; here for every case of
    tests/test_gpu_afda.py, on the CPU, with the offsets rounded to the case's coordinate dtype."""
    cases = _gpu_cases()
    assert len(cases) >= 30
    for kw, Lr, R_, dtype, cdt, seed in cases:
        value, ref, offs_attn, go = R.make_inputs(Lr=Lr, R=R_, dtype=dtype, coord_dtype=cdt, seed=seed, **kw)
        assert offs_attn.dtype == (cdt or dtype) and ref.dtype == torch.float32
        assert ref.shape[2:] == (1 if Lr == 1 else len(kw["shapes"]), R_)
        R.check_inputs(ref, kw["shapes"], kw["points"], offs_attn)   # (again, on the tensors as returned)
        assert float(ref[..., :2].min()) >= 0.2 and float(ref[..., :2].max()) <= 0.8
        if R_ == 4:
            assert float(ref[..., 2:].min()) >= 0.1 and float(ref[..., 2:].max()) <= 0.4


@pytest.mark.parametrize("cdt", [torch.float32, torch.float16, torch.bfloat16])
def test_lattice_inputs_are_exact(cdt):
    shapes, points = [(8, 4), (2, 2), (1, 4)], (2, 1, 3)
    value, ref, offs_attn, go = R.make_lattice_inputs(1, 2, 8, shapes, points, dtype=cdt, seed=2)
    offs = FR.unpack(offs_attn, points)[0].double()
    assert torch.equal(offs, offs.round()) and ref.shape[2:] == (3, 2)
    loc = R.derived(ref, shapes, points, offs_attn)
    pix = loc * MR._tap_wh(shapes, points) - 0.5
    assert torch.equal(pix, pix.round())
    gate = MR.gate_of(loc, shapes, points)
    assert bool(gate.any()) and not bool(gate.all())
    # fp32 arithmetic gives the same integers: reference + offset * (1 / extent), times the extent, minus a half
    wh32 = MR._tap_wh(shapes, points).float()
    levels = torch.tensor(MR.tap_levels(points))
    loc32 = ref[:, :, None, levels] + offs.float() * (1.0 / wh32)
    assert torch.equal((loc32 * wh32 - 0.5).double(), pix)


# ---- the C interface ----
def _header_fields():
    hdr = (ROOT / "include" / "mdconv_afda.h").read_text()
    body = re.search(r"typedef struct mdconv_afda_desc \{(.*?)\} mdconv_afda_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return hdr, [re.match(r"\s*(int|float)\s+(\w+)", line).groups() for line in body.split(";") if line.strip()]


def test_descriptor_mirror_matches_the_header(capi):
    hdr, fields = _header_fields()
    names = [n for _, n in fields]
    assert names == ["dtype", "coord_dtype", "batch", "heads", "head_channels", "queries", "levels", "points", "level_sz",
                     "accumulate", "flags", "ref_levels", "ref_comps", "offset_scale", "grad_reference"]
    assert [f[0] for f in capi.MdconvAfdaDesc._fields_] == names
    assert names[:11] == [f[0] for f in capi.MdconvFdapDesc._fields_]
    assert [f[1] for f in capi.MdconvAfdaDesc._fields_[:11]] == [f[1] for f in capi.MdconvFdapDesc._fields_]
    assert [t for t, n in fields if n == "offset_scale"] == ["float"] and dict(capi.MdconvAfdaDesc._fields_)["offset_scale"] is ctypes.c_float
    assert all(t == "int" for t, n in fields if n != "offset_scale")
    assert "MDCONV_AFDA_DESC_INIT" in hdr and '#include "mdconv.h"' in hdr and "UNPINNED" in hdr
    flat = " ".join(hdr.split())
    assert "-a[t] * S" in flat and "selected, not multiplied" in flat and "ALWAYS fp32" in flat
    assert 'offs_attn and grad_offs_attn (coord_dtype) are "element"' in flat
    assert ctypes.sizeof(capi.MdconvAfdaDesc) == ctypes.sizeof(capi.MdconvFdapDesc) + 16 == (7 + 8 + 8 * 2 + 2 + 4) * 4
    # the existing surfaces have not moved
    assert ctypes.sizeof(capi.MdconvFdapDesc) == (7 + 8 + 8 * 2 + 2) * 4
    assert capi.lib().mdconv_abi_version() == 2 == capi.ABI_VERSION
    assert capi.SAMP_QUERIES["afda"] == ("value_len", "offs_attn_len")


def test_exports_are_what_the_header_declares(capi):
    hdr = _header_fields()[0]
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mdconv_afda_\w+)\s*\(", code))
    assert declared == set(capi.EXPORTS_AFDA) and len(capi.EXPORTS_AFDA) == 5
    others = set(capi.EXPORTS) | set(capi.EXPORTS_DAGG) | set(capi.EXPORTS_MSDAP) | set(capi.EXPORTS_FDAP)
    assert not set(capi.EXPORTS_AFDA) & others
    for name in capi.EXPORTS_AFDA:
        assert hasattr(capi.lib(), name), name
    for other in ("mdconv.h", "mdconv_msdap.h", "mdconv_fdap.h", "mdconv_dagg.h"):
        assert "mdconv_afda" not in (ROOT / "include" / other).read_text()
    assert "mdconv_afda.h" in (ROOT / "modulated_deform_conv_amd" / "_build.py").read_text()   # editing it rebuilds


C_CALLER = r"""
#include <stdio.h>
#include "mdconv_afda.h"
int main(void) {
  mdconv_afda_desc d = MDCONV_AFDA_DESC_INIT;
  d.batch = 8; d.heads = 8; d.head_channels = 32; d.queries = 300; d.levels = 3;
  d.level_sz[0][0] = 80; d.level_sz[0][1] = 80; d.level_sz[1][0] = 40; d.level_sz[1][1] = 40;
  d.level_sz[2][0] = 20; d.level_sz[2][1] = 20;
  printf("%d %d %d %d %d %d %d %.2f %d\n", d.dtype, d.coord_dtype, d.accumulate, d.flags, d.points[7], d.ref_levels, d.ref_comps,
         d.offset_scale, d.grad_reference);
  printf("%d\n", mdconv_afda_offs_attn_len(&d));
  d.points[0] = 3; d.points[1] = 6; d.points[2] = 3;
  printf("%d %d\n", mdconv_afda_value_len(&d), mdconv_afda_offs_attn_len(&d));
  printf("%zu %d\n", mdconv_afda_workspace_bytes(&d, 0), mdconv_afda_workspace_bytes(&d, 1) > 0);
  printf("%d %s\n", mdconv_afda_forward(&d, NULL, NULL, NULL, NULL, NULL, 0, NULL), mdconv_last_error());
  return 0;
}
"""


def test_a_plain_caller_builds_against_the_header(capi, tmp_path):
    """mdconv_afda.h compiles as C11 and as C++17, MDCONV_AFDA_DESC_INIT gives fp32 / accumulate / no flags / zero counts /
    one box per query / offset_scale 0.5 / with grad_reference, and a plain C program linked against the library gets through
    validation and planning without a GPU."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "caller.c"
    src.write_text(C_CALLER)
    libdir = os.path.dirname(capi.LIB_PATH)
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lmdconv_hip", "-Wl,-rpath," + libdir], check=True, capture_output=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert lines[0] == "0 0 1 0 0 1 4 0.50 1", lines
    assert lines[1] == "-1", lines   # the counts are still zero
    assert lines[2] == "%d 36" % (6400 + 1600 + 400), lines
    assert lines[3] == "0 1", lines
    assert lines[4].startswith("-2 ") and "value pointer is NULL" in lines[4], lines
    if shutil.which("g++"):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", str(ROOT / "include"), str(src)],
                       check=True, capture_output=True)


def test_valid_descriptor_stops_at_null_pointers(capi):
    for dtype, cdt in PAIRINGS:
        for Lr, R_ in ((1, 4), (3, 4), (3, 2), (1, 2)):
            for call in (_fwd, _bwd):
                d = _desc(capi, dtype=dtype, coord_dtype=cdt, ref_levels=Lr, ref_comps=R_)
                assert call(capi, d) == ENULL and "NULL" in capi.last_error()
    assert _fwd(capi, _desc(capi, D=6)) == ENULL   # outside the shape rule as well: the pointer check comes first
    for flags in (0, 1, 4, 5):
        for gr in (0, 1):
            assert _fwd(capi, _desc(capi, flags=flags, grad_reference=gr)) == ENULL
            assert _bwd(capi, _desc(capi, flags=flags, grad_reference=gr)) == ENULL
    assert _fwd(capi, _desc(capi, ref_comps=2, offset_scale=1e30)) == ENULL   # finite; unused for R == 2


@pytest.mark.parametrize("kw, word", [
    (dict(dtype=2), "dtype"), (dict(dtype=BF16, coord_dtype=F16), "coord_dtype"), (dict(dtype=F32, coord_dtype=F16), "coord_dtype"),
    (dict(N=0), "positive"), (dict(Lq=0), "positive"), (dict(points=(3, 0, 3)), "level 1"), (dict(L=0), "levels"), (dict(L=9), "levels"),
    (dict(levels=((8, 8), (0, 4), (2, 2))), "extent"), (dict(flags=2), "flags"), (dict(flags=256), "flags"),
    (dict(accumulate=2), "accumulate"),
    (dict(ref_levels=2), "ref_levels must be 1 or levels (3), is 2"), (dict(ref_levels=0), "ref_levels"),
    (dict(ref_levels=8), "ref_levels"), (dict(ref_comps=3), "ref_comps must be 2 or 4, is 3"), (dict(ref_comps=0), "ref_comps"),
    (dict(offset_scale=float("nan")), "offset_scale is not finite"), (dict(offset_scale=float("inf")), "offset_scale is not finite"),
    (dict(ref_comps=2, offset_scale=float("-inf")), "offset_scale is not finite"),
    (dict(grad_reference=2), "grad_reference must be 0 or 1, is 2"), (dict(grad_reference=-1), "grad_reference"),
])
def test_invalid_descriptor(capi, kw, word):
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, **kw)) == EINVAL, kw
        assert capi.last_error().startswith("afda: ") and word in capi.last_error(), capi.last_error()
    assert _ws(capi, _desc(capi, **kw), 0) == 0 and _ws(capi, _desc(capi, **kw), 1) == 0
    assert capi.lib().mdconv_afda_value_len(ctypes.byref(_desc(capi, **kw))) == -1
    assert capi.lib().mdconv_afda_offs_attn_len(ctypes.byref(_desc(capi, **kw))) == -1


def test_lengths(capi):
    L = capi.lib()
    assert L.mdconv_afda_offs_attn_len(None) == -1 and L.mdconv_afda_value_len(None) == -1
    assert L.mdconv_afda_forward(None, _null(), _null(), _null(), _null(), None, 0, None) == EINVAL
    assert L.mdconv_afda_value_len(ctypes.byref(_desc(capi))) == 64 + 16 + 4
    for levels, points in ((DFINE["levels"], (3, 6, 3)), (((5, 7),), (1,)), (((3, 3), (5, 4)), (1, 70))):
        assert L.mdconv_afda_offs_attn_len(ctypes.byref(_desc(capi, levels=levels, points=points))) == 3 * sum(points)
    # one level: ref_levels 1 IS `levels`
    assert _fwd(capi, _desc(capi, levels=((5, 7),), points=(2,), ref_levels=1)) == ENULL
    huge = _desc(capi, points=((1 << 31) - 1,) * 3)
    assert L.mdconv_afda_offs_attn_len(ctypes.byref(huge)) == -1 and "2^31" in capi.last_error()


def test_order_of_checks(capi):
    """The descriptor (EINVAL) -- fdap's fields before the four of the reference --, then the pointers -- NULL (ENULL), then
    alignment (EINVAL naming the argument) --, then the shape rule (EUNSUPPORTED), then the workspace (EWORKSPACE).  Fake
    non-NULL pointers: every call stops before a launch."""
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # non-NULL; nothing dereferences it
    p16 = ctypes.c_void_p((p.value + 15) // 16 * 16)
    big = dict(points=(4090, 6, 1))   # K = 4097: outside the shape rule
    assert _fwd(capi, _desc(capi, flags=2, ref_comps=3, **big), p16) == EINVAL and "flags" in capi.last_error()
    assert _fwd(capi, _desc(capi, ref_levels=2, ref_comps=3, **big), p16) == EINVAL and "ref_levels" in capi.last_error()
    assert _fwd(capi, _desc(capi, ref_comps=3, grad_reference=5, **big)) == EINVAL and "ref_comps" in capi.last_error()
    assert _fwd(capi, _desc(capi, **big)) == ENULL and _bwd(capi, _desc(capi, **big)) == ENULL
    assert capi.last_error() == "value pointer is NULL"
    for call in (_fwd, _bwd):
        assert call(capi, _desc(capi, **big), p16) == EUNSUPPORTED and _refused(capi)
        assert capi.last_error() == "afda: outside the shape rule of the operator: the sum of points exceeds 4096"
        assert call(capi, _desc(capi, **big), ctypes.c_void_p(p16.value + 2)) == EINVAL
        assert capi.last_error() == "value pointer must be 16-byte aligned"
    assert _ws(capi, _desc(capi, **big), 1) == 0 and _refused(capi)
    L = capi.lib()
    # every argument of the forward and of the backward in turn, by its class: the reference pair is "element" of fp32 in
    # every pairing, the packed pair "element" of the coordinate dtype
    for dtype, cdt, es in ((F32, F32, 4), (F16, F16, 2), (BF16, F32, 4)):
        d = lambda **kw: _desc(capi, dtype=dtype, coord_dtype=cdt, **dict(big, **kw))   # noqa: E731
        classes = dict(value=16, reference_points=4, offs_attn=es, output=16, grad_output=16, grad_value=16,
                       grad_reference_points=4, grad_offs_attn=es)
        for fn, names in ((L.mdconv_afda_forward, ("value", "reference_points", "offs_attn", "output")),
                          (L.mdconv_afda_backward, ("value", "reference_points", "offs_attn", "grad_output", "grad_value",
                                                    "grad_reference_points", "grad_offs_attn"))):
            for i, name in enumerate(names):
                args = [p16] * len(names)
                args[i] = ctypes.c_void_p(p16.value + classes[name] // 2)
                assert fn(ctypes.byref(d()), *args, _null(), ctypes.c_size_t(0), _null()) == EINVAL, name
                assert capi.last_error() == "%s pointer must be %d-byte aligned" % (name, classes[name]), capi.last_error()
                if classes[name] < 16:   # an "element" pointer at its own alignment passes on to the shape rule
                    args[i] = ctypes.c_void_p(p16.value + classes[name])
                    assert fn(ctypes.byref(d()), *args, _null(), ctypes.c_size_t(0), _null()) == EUNSUPPORTED, name
                args[i] = _null()
                assert fn(ctypes.byref(d()), *args, _null(), ctypes.c_size_t(0), _null()) == ENULL
                assert capi.last_error() == "%s pointer is NULL" % name
    # a NULL later in the table comes before an alignment fault earlier in it
    q = ctypes.c_void_p(p16.value + 2)
    assert L.mdconv_afda_forward(ctypes.byref(_desc(capi, **big)), q, p16, p16, _null(), _null(), ctypes.c_size_t(0), _null()) == ENULL
    assert capi.last_error() == "output pointer is NULL"
    # a skipped grad_value / grad_reference_points is not looked at, NULL or misaligned
    for bad in (ctypes.c_void_p(p16.value + 2), _null()):
        args = [p16] * 7
        args[4] = bad
        assert L.mdconv_afda_backward(ctypes.byref(_desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **big)), *args, _null(),
                                      ctypes.c_size_t(0), _null()) == EUNSUPPORTED
        args = [p16] * 7
        args[5] = bad
        assert L.mdconv_afda_backward(ctypes.byref(_desc(capi, grad_reference=0, **big)), *args, _null(), ctypes.c_size_t(0),
                                      _null()) == EUNSUPPORTED
    # inside the rule, pointers given, the workspace missing / too small / misaligned: EWORKSPACE, nothing launched
    need = _ws(capi, _desc(capi), 1)
    assert need > 0
    assert _bwd(capi, _desc(capi), p16) == EWORKSPACE and capi.last_error() == "workspace too small: need %d bytes, have 0" % need
    assert _bwd(capi, _desc(capi), p16, p16, need - 1) == EWORKSPACE
    assert _bwd(capi, _desc(capi), p16, ctypes.c_void_p(p16.value + 4), need) == EWORKSPACE
    assert capi.last_error() == "workspace must be 16-byte aligned"
    # ... and with neither grad_value nor grad_reference there is none to miss: the call would launch, so it is not made


def test_shape_rule_refusals_come_before_any_launch(capi):
    buf = (ctypes.c_char * 64)()
    p = ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16)
    one = ((1, 1),)
    for d, word in ((_desc(capi, D=6), "multiple of 4"), (_desc(capi, dtype=F16, D=4), "multiple of 8"),
                    (_desc(capi, dtype=BF16, coord_dtype=F32, D=12), "multiple of 8"),
                    (_desc(capi, levels=((2, 2),) * 8, points=(513,) * 8, ref_levels=8), "4096"),
                    (_desc(capi, N=1 << 10, M=1 << 6, D=64, levels=((128, 128),), points=(4,)), "2^31"),
                    (_desc(capi, N=1, M=1, D=4, Lq=3 << 18, levels=one, points=(256,)), "2^31")):   # the packed tensor alone
        for call in (_fwd, _bwd):
            assert call(capi, d, p) == EUNSUPPORTED, word
            assert word in capi.last_error() and _refused(capi), capi.last_error()
        assert _ws(capi, d, 1) == 0
    # the partial rows of grad_reference_points alone: 2^24 pairs x 8 rows x 4 components x 4 bytes = 2^31, where the packed
    # tensor (2^24 x 8 taps x 3 x 2 bytes) and every other tensor are inside the rule -- fdap takes the shape
    rows = dict(dtype=F16, N=1, M=1 << 8, D=8, Lq=1 << 16, levels=one * 8, points=(1,) * 8, flags=capi.FLAG_NO_GRAD_INPUT)
    assert _bwd(capi, _desc(capi, ref_levels=8, **rows), p) == EUNSUPPORTED and "2^31" in capi.last_error() and _refused(capi)
    assert _bwd(capi, _desc(capi, ref_levels=8, ref_comps=2, **rows), p) == EWORKSPACE
    assert _bwd(capi, _desc(capi, ref_levels=1, **rows), p) == EWORKSPACE
    # batch * heads above 65535: the lists of grad_value only
    big = dict(N=4096, M=17, D=4, Lq=1, levels=one, points=(1,))
    assert _bwd(capi, _desc(capi, **big), p) == EUNSUPPORTED and "65535" in capi.last_error()
    assert _ws(capi, _desc(capi, **big), 0) == 0 and not _refused(capi)
    assert _ws(capi, _desc(capi, flags=capi.FLAG_NO_GRAD_INPUT, **big), 1) == _partials(4096, 1, 17, 1, 4) and not _refused(capi)


def test_workspace_is_the_packed_operators_plus_the_partial_rows(capi):
    """grad_reference == 0: mdconv_fdap_workspace_bytes for the same shape, for every pairing, form, direction and flag
    combination.  With it: that figure plus 4 * Lr * R bytes per (query, head) in a 256-byte slot -- never smaller."""
    for dtype, cdt in PAIRINGS:
        for Lr, R_ in ((1, 4), (3, 4), (3, 2), (1, 2)):
            for flags in (0, 1, 4, 5):
                for accumulate in (0, 1):
                    kw = dict(dtype=dtype, coord_dtype=cdt, flags=flags, accumulate=accumulate, ref_levels=Lr, ref_comps=R_)
                    for gr in (0, 1):
                        assert _ws(capi, _desc(capi, grad_reference=gr, **kw), 0) == 0
                    theirs = _fdap_ws(capi, 1, **kw)
                    assert (theirs > 0) == (not flags & 4)
                    assert _ws(capi, _desc(capi, grad_reference=0, **kw), 1) == theirs
                    with_ref = _ws(capi, _desc(capi, grad_reference=1, **kw), 1)
                    assert with_ref == theirs + _partials(2, 10, 8, Lr, R_) > theirs and with_ref % 256 == 0
    odd = dict(N=1, M=3, D=8, Lq=7, levels=((6, 5), (3, 3), (1, 1)), points=(1, 2, 3))
    assert _partials(1, 7, 3, 1, 2) == 256 and _partials(1, 7, 3, 3, 4) == 1024
    assert _ws(capi, _desc(capi, ref_comps=2, **odd), 1) == _fdap_ws(capi, **odd) + 256
    assert _ws(capi, _desc(capi, ref_levels=3, **odd), 1) == _fdap_ws(capi, **odd) + 1024
    # offset_scale does not enter the figure
    assert _ws(capi, _desc(capi, offset_scale=4.0), 1) == _ws(capi, _desc(capi), 1)


# ---- the Python surface ----
def test_python_surface_and_argument_errors(capi):
    import modulated_deform_conv_amd as pkg
    from modulated_deform_conv_amd import afda, fdap, msdap
    for name in ("anchored_deform_attn_forward", "anchored_deform_attn_backward", "AnchoredDeformAttnFunction",
                 "anchored_deform_attn", "MSDeformableAttentionAnchored"):
        assert getattr(pkg, name) is getattr(afda, name) and name in pkg.__all__ and name in afda.__all__
    assert issubclass(afda.MSDeformableAttentionAnchored, msdap.MSDeformableAttention)
    assert not issubclass(afda.MSDeformableAttentionAnchored, fdap.MSDeformableAttentionFused)
    shapes, points = [(6, 5), (3, 3), (1, 1)], (1, 2, 3)
    value, ref, oa, go = R.make_inputs(2, 3, 8, shapes, points, 7, Lr=1, R=4, seed=1)
    fwd, bwd = afda.anchored_deform_attn_forward, afda.anchored_deform_attn_backward
    for call in (lambda: afda.anchored_deform_attn(value, shapes, points, ref, oa),
                 lambda: afda.AnchoredDeformAttnFunction.apply(value, torch.tensor(shapes), torch.tensor(points), ref, oa, 0.5),
                 lambda: fwd(value, shapes, points, ref, oa), lambda: bwd(value, shapes, points, ref, oa, go)):
        with pytest.raises(NotImplementedError):   # CPU tensors: no fallback
            call()
    with pytest.raises(ValueError, match="afda: offs_attn has 18 elements per head"):
        fwd(value, shapes, (1, 2, 4), ref, oa)
    with pytest.raises(ValueError, match="reference_points must be"):
        fwd(value, shapes, points, ref.expand(2, 7, 2, 4).contiguous(), oa)
    with pytest.raises(ValueError, match="reference_points must be"):
        fwd(value, shapes, points, ref[..., :3].contiguous(), oa)
    with pytest.raises(ValueError, match="it must be float32"):
        fwd(value, shapes, points, ref.half(), oa)
    with pytest.raises(ValueError, match="afda: reference_points must be \\(2, 7, 1, 4\\)"):
        fwd(value, shapes, points, ref[:, :6].contiguous(), oa)
    with pytest.raises(ValueError, match="must have value's dtype or float32"):
        fwd(value.bfloat16(), shapes, points, ref, oa.half())
    with pytest.raises(ValueError, match="contiguous"):
        fwd(value, shapes, points, ref, oa.transpose(1, 2).contiguous().transpose(1, 2))
    with pytest.raises(TypeError, match="not float32, float16 or bfloat16"):
        fwd(value.double(), shapes, points, ref, oa.double())
    d = afda._desc(value, ref.expand(2, 7, 3, 4), oa, tuple(shapes), points, 0.25, accumulate=0, flags=5, grad_reference=0)
    assert isinstance(d, capi.MdconvAfdaDesc)
    assert (d.ref_levels, d.ref_comps, d.offset_scale, d.grad_reference, d.accumulate, d.flags) == (3, 4, 0.25, 0, 0, 5)
    assert list(d.points)[:3] == [1, 2, 3] and (d.batch, d.heads, d.head_channels, d.queries, d.levels) == (2, 3, 8, 7, 3)


def test_module_has_the_parents_parameters_and_its_linear_is_their_pack():
    """``MSDeformableAttentionAnchored``: the parent's ``state_dict`` keys, its checkpoint loads, ``method='discrete'`` stays
    refused, and the output of the ONE fused linear is ``pack(offsets, logits)`` of the parent's two linears -- to 1e-6 of the
    largest element: the CPU GEMMs differ in blocking."""
    from modulated_deform_conv_amd import MSDeformableAttention, MSDeformableAttentionAnchored
    torch.manual_seed(5)
    kw = dict(embed_dim=32, num_heads=4, num_levels=3, num_points=[3, 6, 3], offset_scale=0.75)
    parent = MSDeformableAttention(**kw)
    with torch.no_grad():
        parent.sampling_offsets.weight.normal_(0, 0.05)
        parent.attention_weights.weight.normal_(0, 0.2)
        parent.attention_weights.bias.normal_(0, 0.2)
    mod = MSDeformableAttentionAnchored(**kw)
    assert list(mod.state_dict()) == list(parent.state_dict())
    assert [n for n, _ in mod.named_parameters()] == [n for n, _ in parent.named_parameters()]
    assert mod.load_state_dict(parent.state_dict()).missing_keys == []
    assert mod.offset_scale == 0.75 and mod.num_points_list == [3, 6, 3]
    with pytest.raises(NotImplementedError):
        MSDeformableAttentionAnchored(method="discrete")
    N, Lq, M, K = 2, 7, 4, 12
    query = torch.randn(N, Lq, 32)
    weight, bias = mod.fused_linear()
    assert weight.shape == (M * 3 * K, 32) and bias.shape == (M * 3 * K,) and weight.requires_grad and bias.requires_grad
    row = torch.nn.functional.linear(query, weight, bias).view(N, Lq, M, 3 * K)
    want = FR.pack(parent.sampling_offsets(query).view(N, Lq, M, K, 2), parent.attention_weights(query).view(N, Lq, M, K))
    assert float((row - want).abs().max()) <= 1e-6 * float(want.abs().max())
    # the parameter gradients flow back through the weight-sized cat
    row.sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0
               for p in (mod.sampling_offsets.weight, mod.sampling_offsets.bias, mod.attention_weights.weight, mod.attention_weights.bias))
    # the forward refuses other reference forms before it reaches the core
    seen = []
    mod._core = lambda *a: seen.append(a) or torch.zeros(N, Lq, 32)
    flat = torch.randn(N, 43, 32)
    shapes = [(6, 5), (3, 3), (2, 2)]
    for form in ((1, 4), (3, 4), (3, 2)):
        mod(query, torch.rand(N, Lq, *form), flat, shapes)
    assert [tuple(a[3].shape[2:]) for a in seen] == [(1, 4), (3, 4), (3, 2)]
    assert all(a[4].shape == (N, Lq, M, 3 * K) and a[5] == 0.75 and a[2] == [3, 6, 3] for a in seen)
    for form in ((1, 2), (2, 4), (3, 3)):
        with pytest.raises(ValueError, match="reference_points must be"):
            mod(query, torch.rand(N, Lq, *form), flat, shapes)
