"""CPU-side checks of the drop-in boundary (no GPU, no compute calls):
the C-ABI library loads, exports every symbol include/mdconv.h declares, validates descriptors,
and the Python surface mirrors the reference's names / signatures / error behaviour."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def test_library_exports_every_declared_symbol(capi):
    hdr = open(os.path.join(ROOT, "include", "mdconv.h")).read()
    declared = set(re.findall(r"\b(mdconv_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == len(capi.EXPORTS) >= 20 and declared == set(capi.EXPORTS)
    L = capi.lib()
    for name in declared:
        assert getattr(L, name) is not None
    assert L.mdconv_abi_version() == 2 == capi.ABI_VERSION


def test_desc_struct_matches_header(capi):
    hdr = open(os.path.join(ROOT, "include", "mdconv.h")).read()
    body = hdr[hdr.index("typedef struct mdconv_desc {"):hdr.index("} mdconv_desc;")]
    fields = re.findall(r"^\s*int\s+([a-z_]+)(?:\[[35]\])?;", body, re.M)
    assert fields == [f[0] for f in capi.MdconvDesc._fields_]
    assert int(re.search(r"#define MDCONV_DESC_V2 (0x[0-9a-f]+)", hdr).group(1), 16) == capi.DESC_V2
    # the v1 struct is a prefix of the v2 struct: a caller built against the v1 header passes 25 ints
    assert fields.index("with_bias") == len(fields) - 5 and ctypes.sizeof(capi.MdconvDesc) == (25 + 8) * 4


def _desc(capi, **kw):
    d = capi.MdconvDesc()
    d.ndim, d.modulated, d.dtype, d.batch, d.c_in, d.c_out = 2, 1, 0, 2, 8, 8
    d.in_sz = (ctypes.c_int * 3)(8, 8, 1)
    d.k_sz = (ctypes.c_int * 3)(3, 3, 1)
    d.stride = (ctypes.c_int * 3)(1, 1, 1)
    d.pad = (ctypes.c_int * 3)(1, 1, 0)
    d.dil = (ctypes.c_int * 3)(1, 1, 1)
    d.groups, d.dgroups, d.in_step, d.with_bias = 1, 1, 64, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_descriptor_validation_without_gpu(capi):
    L = capi.lib()
    null = ctypes.c_void_p(0)

    def fwd(d):
        return L.mdconv_modulated_deform_conv2d_forward(ctypes.byref(d), null, null, null, null,
                                                        null, null, null, ctypes.c_size_t(0), null)
    assert fwd(_desc(capi, ndim=4)) == -1 and "ndim" in capi.last_error()
    assert fwd(_desc(capi, in_step=0)) == -1 and "in_step" in capi.last_error()
    assert fwd(_desc(capi, groups=3)) == -1 and "wont match" in capi.last_error()
    assert fwd(_desc(capi, dgroups=3)) == -1
    assert fwd(_desc(capi, dtype=7)) == -1
    assert fwd(_desc(capi)) == -2 and "NULL" in capi.last_error()          # pointers missing
    d3 = _desc(capi)
    assert L.mdconv_deform_conv3d_forward(ctypes.byref(d3), null, null, null, null, null, null,
                                          ctypes.c_size_t(0), null) == -1   # wrong entry point
    assert L.mdconv_out_size(ctypes.byref(_desc(capi)), 0) == 8
    big = _desc(capi)
    big.in_sz = (ctypes.c_int * 3)(56, 56, 1)
    big.stride = (ctypes.c_int * 3)(2, 2, 1)
    assert L.mdconv_out_size(ctypes.byref(big), 1) == 28


class _DescV1(ctypes.Structure):
    """``struct mdconv_desc`` as the ABI v1 header declared it: ends at with_bias."""
    _fields_ = [("ndim", ctypes.c_int), ("modulated", ctypes.c_int), ("dtype", ctypes.c_int),
                ("batch", ctypes.c_int), ("c_in", ctypes.c_int), ("c_out", ctypes.c_int),
                ("in_sz", ctypes.c_int * 3), ("k_sz", ctypes.c_int * 3), ("stride", ctypes.c_int * 3),
                ("pad", ctypes.c_int * 3), ("dil", ctypes.c_int * 3), ("groups", ctypes.c_int),
                ("dgroups", ctypes.c_int), ("in_step", ctypes.c_int), ("with_bias", ctypes.c_int)]


def test_both_descriptor_versions_without_gpu(capi):
    """ABI v1 descriptors (no MDCONV_DESC_V2 in ndim: the struct ends at with_bias, modes from the setters) and v2
    descriptors (modes in the struct) are both accepted; a v2 descriptor is validated and overrides the setters."""
    L = capi.lib()
    null = ctypes.c_void_p(0)
    # v1: a struct that really is only 25 ints long, placed at the END of a buffer so that a library reading a v2 tail
    # would read the guard ints behind it
    buf = (ctypes.c_int * (25 + 8))(*([0] * 25 + [0x5a5a5a5a] * 8))
    v1 = _DescV1.from_buffer(buf)
    v1.ndim, v1.modulated, v1.dtype, v1.batch, v1.c_in, v1.c_out = 2, 1, capi.F16, 2, 64, 64
    v1.in_sz = (ctypes.c_int * 3)(8, 8, 1)
    v1.k_sz = (ctypes.c_int * 3)(3, 3, 1)
    v1.stride = (ctypes.c_int * 3)(1, 1, 1)
    v1.pad = (ctypes.c_int * 3)(1, 1, 0)
    v1.dil = (ctypes.c_int * 3)(1, 1, 1)
    v1.groups, v1.dgroups, v1.in_step, v1.with_bias = 1, 1, 64, 0
    assert L.mdconv_out_size(ctypes.byref(v1), 0) == 8
    assert L.mdconv_workspace_bytes(ctypes.byref(v1), 1) > 0               # guard ints behind it: not read as modes
    rc = L.mdconv_modulated_deform_conv2d_forward(ctypes.byref(v1), null, null, null, null, null, null, null,
                                                  ctypes.c_size_t(0), null)
    assert rc == -2 and "NULL" in capi.last_error()                         # passed validation, stopped at the pointers
    # the v1 setters still exist and round-trip (they apply to v1 descriptors of the calling thread)
    assert L.mdconv_set_accumulate(0) == 1 and L.mdconv_set_accumulate(1) == 0
    assert L.mdconv_set_input_layout(1) == 0 and L.mdconv_set_input_layout(0) == 1
    # v2: modes are validated ...
    def fwd(d):
        return L.mdconv_modulated_deform_conv2d_forward(ctypes.byref(d), null, null, null, null, null, null, null,
                                                        ctypes.c_size_t(0), null)
    v2 = lambda **kw: _desc(capi, ndim=2 | capi.DESC_V2, accumulate=1, **kw)
    assert fwd(v2()) == -2
    assert fwd(v2(path=5)) == -1 and "call mode" in capi.last_error()
    assert fwd(v2(input_layout=3)) == -1
    bad = v2()
    bad.accumulate = 2
    assert fwd(bad) == -1
    res = v2()
    res.reserved = (ctypes.c_int * 5)(0, 0, 1, 0, 0)
    assert fwd(res) == -1 and "reserved" in capi.last_error()
    # ... and decide per call: a forced direct path in the descriptor changes the plan of THIS descriptor only
    # (fp16 backward: the shape-generic kernels need fp32 copies, the native 16-bit kernels a different workspace)
    h = lambda **kw: _plan_desc(capi, 2, capi.F16, 2, 64, 64, (8, 8), **kw)
    auto, direct = h(), h()
    direct.path = capi.PATH_DIRECT
    assert L.mdconv_workspace_bytes(ctypes.byref(auto), 1) != L.mdconv_workspace_bytes(ctypes.byref(direct), 1)
    assert L.mdconv_input_layout_supported(ctypes.byref(auto), 1, 0) == 1
    assert L.mdconv_input_layout_supported(ctypes.byref(direct), 1, 0) == 0


def test_extension_module_surface_matches_reference():
    """The 8 positional signatures of SURVEY.md section 8b."""
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    expect = {
        "deform_conv2d_forward_cuda": 17, "deform_conv2d_backward_cuda": 21,
        "modulated_deform_conv2d_forward_cuda": 17, "modulated_deform_conv2d_backward_cuda": 18,
        "deform_conv3d_forward_cuda": 21, "deform_conv3d_backward_cuda": 25,
        "modulated_deform_conv3d_forward_cuda": 22, "modulated_deform_conv3d_backward_cuda": 27,
    }
    for name, nargs in expect.items():
        assert len(inspect.signature(getattr(M, name)).parameters) == nargs, name
    # ... and the ORDER, argument by argument (the tensors, then kernel / stride / pad / dilation
    # per axis h, w[, l], then group, deformable_group, in_step, with_bias); tools/check_reference_call_sites.py compares
    # the same order with the call sites of the reference's wrapper where that tree is at hand
    tensors = {
        "deform_conv2d_forward_cuda": "input weight bias offset output",
        "deform_conv2d_backward_cuda": "input weight bias offset grad_input grad_weight grad_bias grad_offset grad_output",
        "modulated_deform_conv2d_forward_cuda": "input weight bias offset mask",
        "modulated_deform_conv2d_backward_cuda": "input weight bias offset mask grad_output",
        "deform_conv3d_forward_cuda": "input weight bias offset output",
        "deform_conv3d_backward_cuda": "input weight bias offset grad_input grad_weight grad_bias grad_offset grad_output",
        "modulated_deform_conv3d_forward_cuda": "input weight bias offset mask output",
        "modulated_deform_conv3d_backward_cuda":
            "input weight bias offset mask grad_input grad_weight grad_bias grad_offset grad_mask grad_output",
    }
    for name, t in tensors.items():
        axes = "hwl"[:3 if "3d" in name else 2]
        want = t.split() + ["%s_%s" % (p, a) for p in ("kernel", "stride", "pad", "dilation") for a in axes]
        want += ["group", "deformable_group", "in_step", "with_bias"]
        assert list(inspect.signature(getattr(M, name)).parameters) == want, name
        assert len(want) == expect[name], name


def test_python_surface_and_cpu_behaviour():
    from modulated_deform_conv_amd import modulated_deform_conv as mdc
    m = mdc.ModulatedDeformConv2d(8, 4, 3, padding=1, groups=2, deformable_groups=2)
    assert m.weight.shape == (4, 4, 3, 3) and m.bias is None and m.with_bias is False
    assert abs(m.weight.abs().max().item()) <= 1 / (8 * 9) ** 0.5
    m3 = mdc.DeformConv3d(4, 6, (3, 2, 1), bias=True)
    assert m3.weight.shape == (6, 4, 3, 2, 1) and torch.equal(m3.bias.data, torch.zeros(6))
    p = mdc.ModulatedDeformConv2dPack(4, 4, 3, padding=1, deformable_groups=2)
    assert set(p.state_dict()) == {"weight", "conv_offset.weight", "conv_offset.bias",
                                   "conv_mask.weight", "conv_mask.bias"}
    assert p.conv_offset.out_channels == 2 * 2 * 9 and p.conv_mask.out_channels == 2 * 9
    with pytest.raises(AssertionError):
        mdc.DeformConv2d(5, 4, 3, groups=2)
    # CPU tensors: NotImplementedError, exactly like the reference (no CPU fallback in the product)
    x = torch.randn(1, 8, 5, 5)
    with pytest.raises(NotImplementedError):
        m(x, torch.zeros(1, 2 * 18, 5, 5), torch.ones(1, 2 * 9, 5, 5))
    assert mdc.DeformConv2dFunction._infer_shape(
        type("C", (), dict(stride=(2, 2), padding=(1, 1), dilation=(1, 1)))(), torch.empty(2, 4, 9, 7),
        torch.empty(6, 4, 3, 3)) == (2, 6, 5, 4)


def _plan_desc(capi, nd, dtype, B, C, O, sz, G=1, DG=1, dil=1):
    d = capi.MdconvDesc()
    d.ndim, d.modulated, d.dtype, d.batch, d.c_in, d.c_out = nd | capi.DESC_V2, 1, dtype, B, C, O
    d.accumulate = 1
    f = lambda v, x: tuple(v) + (x,) * (3 - nd)
    d.in_sz = (ctypes.c_int * 3)(*f(sz, 1))
    d.k_sz = (ctypes.c_int * 3)(*f((3,) * nd, 1))
    d.stride = (ctypes.c_int * 3)(1, 1, 1)
    d.pad = (ctypes.c_int * 3)(*f((dil,) * nd, 0))
    d.dil = (ctypes.c_int * 3)(*f((dil,) * nd, 1))
    d.groups, d.dgroups, d.in_step, d.with_bias = G, DG, 64, 0
    return d


def test_workspace_plan_and_layout_query_without_gpu(capi):
    """Host planning only (no device needed): the workspace covers the buffers DESIGN.md section 3 names, and
    the per-direction channels-last query (include/mdconv.h: mdconv_input_layout_supported) separates shapes the
    native 16-bit forward takes from those its backward takes (a forward that consumed the layout
    in place must not be followed by a backward that raises)."""
    L = capi.lib()
    ws = lambda d, bwd: L.mdconv_workspace_bytes(ctypes.byref(d), bwd)
    cl = lambda d, bwd: L.mdconv_input_layout_supported(ctypes.byref(d), 1, bwd)
    cfg2 = _plan_desc(capi, 2, capi.F32, 32, 256, 256, (56, 56))
    n, K = 32 * 56 * 56, 9
    # packed weights + at most one 32 KB partial tile per resident workgroup for the tap ranges of the last dispatch
    # round (mfma_fwd.hip: 256 CUs x <= 5 workgroups): no column buffer (925 MB in the reference, mdeformable_conv.cu:159)
    assert 256 * 256 * K * 4 <= ws(cfg2, 0) <= 256 * 256 * K * 4 + 256 * 5 * 32768 + 512
    assert ws(cfg2, 1) >= n * K * 256 * 4 and ws(cfg2, 1) < 1.5 * n * K * 256 * 4   # grad_col rows + lists + tables
    assert cl(cfg2, 0) == 0 and cl(cfg2, 1) == 0                             # fp32: reference layout only
    cfg5 = _plan_desc(capi, 3, capi.F16, 8, 128, 128, (16, 64, 64), dil=2)
    rows = 8 * 27 * 16 * 64 * 64 * 128 * 2                                   # one set of 16-bit rows [b][tap][pix][c]
    assert 2 * rows < ws(cfg5, 1) < 2.5 * rows                               # grad_col rows + column rows + sums + lists
    assert cl(cfg5, 0) == 1 and cl(cfg5, 1) == 1
    wide = _plan_desc(capi, 2, capi.BF16, 2, 512, 64, (8, 8))                # 16 channel blocks: forward only
    assert cl(wide, 0) == 1 and cl(wide, 1) == 0 and ws(wide, 1) > 0          # backward: fp32 copies on the fp32 kernels
    dg16 = _plan_desc(capi, 2, capi.F16, 2, 64, 64, (8, 8), DG=4)            # 4 deformable groups of 16 channels
    assert cl(dg16, 0) == 1 and cl(dg16, 1) == 1                              # round 6: the pixel-stationary backward takes them
    dg6 = _plan_desc(capi, 2, capi.F16, 2, 96, 64, (8, 8), DG=6)              # 6 groups of 16 channels: forward only
    assert cl(dg6, 0) == 1 and cl(dg6, 1) == 0 and ws(dg6, 1) > 0             # backward: fp32 kernels / shape-generic kernels on fp32 copies
    # groups of 24 channels (round 6): group-padded on the native kernels, which need the library's own (128-wide) input copy
    pad24 = _plan_desc(capi, 2, capi.F16, 2, 96, 64, (8, 8), DG=4)
    assert cl(pad24, 0) == 0 and cl(pad24, 1) == 0
    assert ws(pad24, 0) >= 2 * 64 * 128 * 2 and ws(pad24, 1) >= 2 * 64 * 128 * 2 + 2 * 9 * 64 * 128 * 2   # xt; xt + grad_col rows
    pad24.input_layout = capi.LAYOUT_CHANNELS_LAST if hasattr(capi, "LAYOUT_CHANNELS_LAST") else 1
    assert ws(pad24, 1) >= 0                                                  # (a refused call: any answer, no crash)
    # the same in fp32: ONE padded problem (groups of 64 in the backward = 256 channels): copies of input / weight + their gradients
    f32pad = _plan_desc(capi, 2, capi.F32, 2, 96, 64, (8, 8), DG=4)
    assert ws(f32pad, 1) >= (2 * 2 * 256 * 64 + 2 * 64 * 256 * 9) * 4
    # padded plans of the fp32 kernels (host planning): output channels below 16 -> a 16-channel grad_output copy; C_in not a multiple
    # of 8 -> padded input / grad_input copies in the backward only; conv groups with 50 channels per group -> 56 per group
    o8 = _plan_desc(capi, 3, capi.F32, 1, 64, 8, (4, 12, 12))
    assert ws(o8, 1) >= (1 * 16 * 576 + 2 * 16 * 64 * 27) * 4 and ws(o8, 0) >= (1 * 16 * 576 + 16 * 64 * 27) * 4
    c100 = _plan_desc(capi, 2, capi.F32, 2, 100, 40, (18, 17))
    assert ws(c100, 1) >= 2 * 2 * 104 * 18 * 17 * 4
    g2 = _plan_desc(capi, 2, capi.F32, 2, 100, 40, (18, 17), G=2)
    assert ws(g2, 1) >= 2 * 2 * 112 * 18 * 17 * 4
    tiny = _plan_desc(capi, 2, capi.F32, 1, 4, 4, (8, 8))                      # BASELINE configs[0]: shape-generic kernels, no workspace
    assert ws(tiny, 0) == 0 and ws(tiny, 1) == 0
    assert L.mdconv_input_layout_supported(ctypes.byref(cfg5), 0, 1) == 1    # NCHW always
    assert L.mdconv_input_layout_supported(ctypes.byref(cfg5), 7, 1) == 0
    assert capi.lib().mdconv_profile_name(9) == b""


def test_16bit_plan_answers_are_stable_without_gpu(capi):
    """Host planning only: the native 16-bit family plans a call once (hp_plan.hpp: hp_plan), and the sizing query reads
    that plan's total.  For shapes its kernels take -- conv groups, 256 -> 256, 3-D, a group-padded one -- the backward
    query answers the same non-zero size every time it is asked, and covers at least the grad_col rows of the plan.  The
    3-D shape is a forward of a few pixel tiles over many K stages (7 tiles, 108 stages): it runs on the fp32 kernels from an
    NCHW input and on the native ones from a channels-last input, and the reported size is enough for either family, so
    the query answers alike for both layouts."""
    L = capi.lib()
    ws = lambda d, bwd: L.mdconv_workspace_bytes(ctypes.byref(d), bwd)
    descs = {
        "cfg3_like": (_plan_desc(capi, 2, capi.F16, 2, 256, 256, (14, 14), G=32, DG=4), 2 * 9 * 14 * 14 * 256 * 2),
        "c256": (_plan_desc(capi, 2, capi.BF16, 2, 256, 256, (14, 14)), 2 * 9 * 14 * 14 * 256 * 2),
        "3d_few_tile": (_plan_desc(capi, 3, capi.F16, 4, 256, 256, (4, 7, 7)), 4 * 27 * 4 * 7 * 7 * 256 * 2),
        "group_padded": (_plan_desc(capi, 2, capi.F16, 2, 96, 64, (8, 8), DG=4), 2 * 9 * 8 * 8 * 128 * 2),
    }
    for name, (d, gcol_rows) in descs.items():
        first = ws(d, 1)
        assert first >= gcol_rows, name
        assert ws(d, 0) > 0 and ws(d, 1) == first, name
        if name != "group_padded":   # (a padded call needs the library's own input copy: channels-last is refused)
            assert L.mdconv_input_layout_supported(ctypes.byref(d), 1, 0) == 1, name
            assert L.mdconv_input_layout_supported(ctypes.byref(d), 1, 1) == 1, name
    few = descs["3d_few_tile"][0]
    nchw = ws(few, 0)
    few.input_layout = 1   # MDCONV_LAYOUT_CHANNELS_LAST
    assert ws(few, 0) == nchw > 0


C_CALLER = r"""
#include "mdconv.h"
#include <stdio.h>
int main(void) {
  mdconv_desc d = MDCONV_DESC_INIT(2);            /* v2 descriptor: reference semantics by default */
  d.modulated = 1; d.dtype = MDCONV_F16; d.batch = 2; d.c_in = 64; d.c_out = 64;
  d.in_sz[0] = 8; d.in_sz[1] = 8; d.k_sz[0] = d.k_sz[1] = 3; d.pad[0] = d.pad[1] = 1;
  d.accumulate = 0;                                /* overwrite mode travels with the call */
  printf("%d %d %d %d %d %zu\n", mdconv_abi_version(), d.ndim == (2 | MDCONV_DESC_V2), mdconv_out_size(&d, 0),
         mdconv_out_size(&d, 1), mdconv_workspace_bytes(&d, 1) > 0, sizeof(d));
  /* NULL tensors: validation passes (descriptor accepted), the call stops at the first missing pointer */
  int rc = mdconv_modulated_deform_conv2d_backward(&d, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);
  printf("%d %s\n", rc, mdconv_last_error());
  d.reserved[1] = 7;
  printf("%d\n", mdconv_out_size(&d, 0) == 8 && mdconv_workspace_bytes(&d, 1) == 0);   /* bad v2 tail: no plan */
  return 0;
}
"""


def test_a_c_caller_builds_against_the_header_and_links_the_library(capi, tmp_path):
    """INTEGRATION.md "A C/C++ caller": include/mdconv.h compiles as C11 (and C++17), MDCONV_DESC_INIT gives a v2 descriptor
    with the reference's semantics, and a plain C program linked against libmdconv_hip.so gets through descriptor validation
    and workspace planning without a GPU."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "caller.c"
    src.write_text(C_CALLER)
    libdir = os.path.dirname(capi.LIB_PATH)
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lmdconv_hip", "-Wl,-rpath," + libdir], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, check=True)
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "2 1 8 8 1 132", lines
    assert lines[1].startswith("-2 ") and "NULL" in lines[1], lines
    assert lines[2] == "1", lines
    if shutil.which("g++"):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", os.path.join(ROOT, "include"),
                        str(src)], check=True, capture_output=True)


def test_plan_table_tool_lists_every_combination(capi):
    """tools/plan_table.py (the routing / workspace table two builds are compared by) runs without a device: one line per
    (case, dtype, direction, path, deterministic flag, layout) over tests/cases.py CASES, three integers each."""
    import subprocess
    import sys
    from tests.cases import CASES
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "plan_table.py"), "--cases-only"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(CASES) * 6 * 2 * 3 * 2 * 2
    assert len(set(ln.split(":")[0] for ln in lines)) == len(lines)
    assert all(re.fullmatch(r"\S+ \w+ (fwd|bwd) (auto|direct|mfma) det[01] cl[01]: \d+ [01] [01]", ln) for ln in lines)
