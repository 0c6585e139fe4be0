"""Pointer alignment without a GPU (include/mdconv.h and DESIGN.md, "Pointer alignment"): every tensor pointer of every
entry point has a class -- "element" or "16-byte" -- and a pointer below its class is MDCONV_EINVAL, naming the argument,
after the NULL checks and before the shape rule and the workspace check.  Fake non-NULL pointers that nothing dereferences:
every call here is made so that it must stop before a launch -- at the alignment check, at the shape rule, or at a workspace
that is needed (asserted beforehand) and not given.  The table in DESIGN.md is parsed and compared with the list below, which
also drives the calls, so table, header and library cannot drift apart."""
import ctypes
import re
from pathlib import Path

import pytest

EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -5
F32, F16, F64, BF16 = 0, 1, 2, 3
S32, WG32 = 0x10, 0x40
FLAG_OUT_CL, FLAG_GI_CL = 64, 128
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


@pytest.fixture(scope="module")
def base():
    """A 256-byte aligned address inside a live host buffer: the fake tensors.  Nothing reads or writes through it."""
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) & ~255
    assert a % 256 == 0
    yield a
    del buf


# ---- the audit, as data: entry-point group -> argument -> class -----------------------------------------------------------
# "element" / "16-byte" / "unused"; ("element", "16-byte", mode): "16-byte" in the call mode `mode`, else "element";
# ("element", N): N bytes whatever the tensors' type
CL_IN, CL_OUT, CL_GI = "MDCONV_LAYOUT_CHANNELS_LAST", "MDCONV_FLAG_OUTPUT_CHANNELS_LAST", "MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST"
AUDIT = {
    "conv.forward": dict(input=("element", "16-byte", CL_IN), weight="element", bias="element", offset="element", mask="element",
                         output=("element", "16-byte", CL_OUT)),
    "conv.backward": dict(input=("element", "16-byte", CL_IN), weight="element", bias="unused", offset="element", mask="element",
                          grad_output="element", grad_input=("element", "16-byte", CL_GI), grad_weight="element",
                          grad_bias="element", grad_offset="element", grad_mask="element"),
    "dcnv3.forward": dict(input="16-byte", offset="element", mask="element", output="16-byte"),
    "dcnv3.backward": dict(input="16-byte", offset="element", mask="element", grad_output="16-byte", grad_input="16-byte",
                           grad_offset="element", grad_mask="element"),
    "dcnv4.forward": dict(input="16-byte", offset_mask="element", output="16-byte"),
    "dcnv4.backward": dict(input="16-byte", offset_mask="element", grad_output="16-byte", grad_input="16-byte",
                           grad_offset_mask="element"),
    "fda.forward": dict(value="16-byte", sampling_loc_attn="element", output="16-byte"),
    "fda.backward": dict(value="16-byte", sampling_loc_attn="element", grad_output="16-byte", grad_value="16-byte",
                         grad_sampling_loc_attn="element"),
    "droi.forward": dict(input="16-byte", rois=("element", 4), offset="element", output="16-byte"),
    "droi.backward": dict(input="16-byte", rois=("element", 4), offset="element", grad_output="16-byte", grad_input="16-byte",
                          grad_offset="element"),
}
for _op in ("msda", "msda3d"):
    AUDIT[_op + ".forward"] = dict(value="16-byte", sampling_locations="element", attention_weights="element", output="16-byte")
    AUDIT[_op + ".backward"] = dict(value="16-byte", sampling_locations="element", attention_weights="element",
                                    grad_output="16-byte", grad_value="16-byte", grad_sampling_locations="element",
                                    grad_attention_weights="element")

# argument order of every entry point (include/mdconv.h), between the descriptor and the workspace
D_FWD = ("input", "weight", "bias", "offset", "output")
D_BWD = ("input", "weight", "bias", "offset", "grad_input", "grad_weight", "grad_bias", "grad_offset", "grad_output")
M_FWD = ("input", "weight", "bias", "offset", "mask", "output")
CONV = {   # name -> (ndim, modulated, group, arguments)
    "mdconv_deform_conv2d_forward": (2, 0, "conv.forward", D_FWD),
    "mdconv_deform_conv2d_backward": (2, 0, "conv.backward", D_BWD),
    "mdconv_modulated_deform_conv2d_forward": (2, 1, "conv.forward", M_FWD),
    "mdconv_modulated_deform_conv2d_backward": (2, 1, "conv.backward", (
        "input", "weight", "bias", "offset", "mask", "grad_output", "grad_input", "grad_offset", "grad_mask", "grad_weight",
        "grad_bias")),
    "mdconv_deform_conv3d_forward": (3, 0, "conv.forward", D_FWD),
    "mdconv_deform_conv3d_backward": (3, 0, "conv.backward", D_BWD),
    "mdconv_modulated_deform_conv3d_forward": (3, 1, "conv.forward", M_FWD),
    "mdconv_modulated_deform_conv3d_backward": (3, 1, "conv.backward", (
        "input", "weight", "bias", "offset", "mask", "grad_input", "grad_weight", "grad_bias", "grad_offset", "grad_mask",
        "grad_output")),
}
SAMP_ARGS = {
    "dcnv3.forward": ("input", "offset", "mask", "output"),
    "dcnv3.backward": ("input", "offset", "mask", "grad_output", "grad_input", "grad_offset", "grad_mask"),
    "dcnv4.forward": ("input", "offset_mask", "output"),
    "dcnv4.backward": ("input", "offset_mask", "grad_output", "grad_input", "grad_offset_mask"),
    "fda.forward": ("value", "sampling_loc_attn", "output"),
    "fda.backward": ("value", "sampling_loc_attn", "grad_output", "grad_value", "grad_sampling_loc_attn"),
    "droi.forward": ("input", "rois", "offset", "output"),
    "droi.backward": ("input", "rois", "offset", "grad_output", "grad_input", "grad_offset"),
}
for _op in ("msda", "msda3d"):
    SAMP_ARGS[_op + ".forward"] = ("value", "sampling_locations", "attention_weights", "output")
    SAMP_ARGS[_op + ".backward"] = ("value", "sampling_locations", "attention_weights", "grad_output", "grad_value",
                                    "grad_sampling_locations", "grad_attention_weights")
PAIRINGS = ((F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32))
ES = {F32: 4, F16: 2, BF16: 2, F64: 8}


def test_every_argument_of_every_entry_point_is_in_the_audit():
    hdr = (ROOT / "include" / "mdconv.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    seen = 0
    for name, params in re.findall(r"\bint (mdconv_\w+_(?:forward|backward))\s*\(([^)]*)\)", hdr):
        ptrs = tuple(re.search(r"(\w+)$", p.strip()).group(1) for p in params.split(",")
                     if "void *" in p and not re.search(r"\b(workspace|stream)$", p.strip()))
        if name in CONV:
            group, args = CONV[name][2], CONV[name][3]
        else:
            group = name[len("mdconv_"):].replace("_", ".")
            args = SAMP_ARGS[group]
        assert ptrs == args, (name, ptrs, args)
        assert set(args) <= set(AUDIT[group]), (name, set(args) - set(AUDIT[group]))
        seen += 1
    assert seen == 8 + 2 * 6   # the eight convolution entry points, six sampling operators in both directions
    assert set(AUDIT) == {CONV[n][2] for n in CONV} | set(SAMP_ARGS)


def _class_text(c):
    if isinstance(c, str):
        return c
    if isinstance(c[1], int):
        return "element (%d)" % c[1]
    return "%s; %s with %s" % c


def test_design_table_matches_the_audit():
    text = (ROOT / "DESIGN.md").read_text()
    sec = text[text.index("### 4.16 Pointer alignment"):text.index("## 5. Multi-GPU")]
    rows = [[c.strip() for c in line.strip().strip("|").split("|")] for line in sec.splitlines() if line.startswith("| ")]
    assert rows[0][:3] == ["entry points", "argument", "class"] and len(rows[0]) == 5
    table = {}
    for r in rows[1:]:
        assert len(r) == 5, r
        for ep in re.split(r",\s*", r[0]):
            assert (ep, r[1]) not in table, (ep, r[1])
            table[(ep, r[1])] = r[2]
            assert r[3], r          # the kernels and the widest access are named
            assert r[4] == "n/a" or not r[1] in ("input", "value", "weight", "bias", "offset", "mask", "rois"), r
    want = {(ep, arg): _class_text(c) for ep, args in AUDIT.items() for arg, c in args.items()}
    assert table == want, sorted(set(table.items()) ^ set(want.items()))
    # every result has a verdict on bit identity
    for r in rows[1:]:
        if r[1].startswith("grad_") and r[1] != "grad_output" or r[1] == "output":
            assert r[4] != "n/a", r
    # the header and the integration guide state the rule and the place of the check
    hdr = (ROOT / "include" / "mdconv.h").read_text()
    assert "Pointer alignment" in hdr
    assert "## Pointer alignment" in (ROOT / "INTEGRATION.md").read_text()


# ---- convolution entry points -------------------------------------------------------------------------------------------
def _conv_desc(capi, nd, modulated, dtype=F32, C=64, O=64, flags=0, input_layout=0, path=0, with_bias=1):
    d = capi.MdconvDesc()
    d.ndim, d.modulated, d.dtype, d.batch, d.c_in, d.c_out = nd | capi.DESC_V2, modulated, dtype, 2, C, O
    d.accumulate, d.input_layout, d.path = 1, input_layout, path
    f = lambda v, x: tuple(v) + (x,) * (3 - nd)
    d.in_sz = (ctypes.c_int * 3)(*f((8,) * nd if nd == 2 else (4, 4, 4), 1))
    d.k_sz = (ctypes.c_int * 3)(*f((3,) * nd, 1))
    d.stride = (ctypes.c_int * 3)(1, 1, 1)
    d.pad = (ctypes.c_int * 3)(*f((1,) * nd, 0))
    d.dil = (ctypes.c_int * 3)(1, 1, 1)
    d.groups, d.dgroups, d.in_step, d.with_bias = 1, 1, 64, with_bias
    d.flags = flags
    return d


def _conv_align(d, arg, cls):
    """(class alignment in bytes, element size) of `arg` for descriptor `d`."""
    dt = d.dtype & ~(S32 | WG32)
    es = ES[dt]
    if arg in ("offset", "mask", "grad_offset", "grad_mask") and d.dtype & S32:
        es = 4
    if arg in ("grad_weight", "grad_bias") and d.dtype & WG32:
        es = 4
    if isinstance(cls, tuple):
        on = {CL_IN: d.input_layout == 1, CL_OUT: bool(d.flags & FLAG_OUT_CL), CL_GI: bool(d.flags & FLAG_GI_CL)}[cls[2]]
        return (16 if on else es), es
    return (16 if cls == "16-byte" else es), es


def _call(capi, name, d, ptrs, ws=0, ws_bytes=0):
    return getattr(capi.lib(), name)(ctypes.byref(d), *[ctypes.c_void_p(p) for p in ptrs], ctypes.c_void_p(ws),
                                     ctypes.c_size_t(ws_bytes), ctypes.c_void_p(0))


CONV_DTYPES = (F32, F16, BF16, F16 | S32, BF16 | S32 | WG32, F64)


@pytest.mark.parametrize("name", sorted(CONV))
def test_convolution_pointers(capi, base, name):
    nd, modulated, group, args = CONV[name]
    backward = group.endswith("backward")
    L = capi.lib()
    for dtype in CONV_DTYPES:
        for mode in ({}, dict(input_layout=1), dict(flags=FLAG_OUT_CL), dict(flags=FLAG_GI_CL)):
            if mode and dtype & ~(S32 | WG32) not in (F16, BF16):
                continue
            d = _conv_desc(capi, nd, modulated, dtype=dtype, **mode)
            need = L.mdconv_workspace_bytes(ctypes.byref(d), int(backward))
            aligned = [base + 256 * i for i in range(len(args))]
            # aligned pointers go through to the last checks: the route's refusal of a layout it does not take, or the
            # workspace.  A call that neither is refused nor needs a workspace would LAUNCH: it is not made (stops_at None),
            # and only its misaligned variants are.
            refused = L.mdconv_planned_kernels(ctypes.byref(d), int(backward)) == 0
            if refused or need > 0:
                stops_at = _call(capi, name, d, aligned)
                assert stops_at == (EUNSUPPORTED if refused else EWORKSPACE), (name, dtype, mode, stops_at, capi.last_error())
            else:
                stops_at = None
            if dtype in (F32, F16, BF16 | S32 | WG32) and not mode:
                assert stops_at == EWORKSPACE, (name, dtype)   # the matrix-core routes: the pass-through half is not vacuous
            for i, arg in enumerate(args):
                cls = AUDIT[group][arg]
                align, es = _conv_align(d, arg, cls)
                for delta in (es, 1):   # one element, one byte
                    ptrs = list(aligned)
                    ptrs[i] += delta
                    passes = cls == "unused" or delta % align == 0
                    if passes and stops_at is None:
                        continue   # (would launch)
                    rc = _call(capi, name, d, ptrs)
                    err = capi.last_error()
                    if passes:
                        assert rc == stops_at, (name, dtype, mode, arg, delta, rc, err)   # passed the pointer checks, launched nothing
                    else:
                        assert rc == EINVAL and re.search(r"\b%s pointer must be %d-byte aligned" % (arg, align), err), (
                            name, dtype, mode, arg, delta, rc, err)
                # one element below a 16-byte class is below the class (the channels-last modes)
                if align == 16:
                    assert es < 16


def test_convolution_alignment_comes_after_null_and_before_the_routing_refusals(capi, base):
    name = "mdconv_modulated_deform_conv2d_backward"
    args = CONV[name][3]
    d = _conv_desc(capi, 2, 1, dtype=F16)
    ptrs = [base + 256 * i for i in range(len(args))]
    ptrs[args.index("grad_output")] += 1
    nulls = list(ptrs)
    nulls[args.index("input")] = 0
    assert _call(capi, name, d, nulls) == ENULL and "input" in capi.last_error()
    assert _call(capi, name, d, ptrs) == EINVAL and "grad_output" in capi.last_error()
    # a forced path the shape cannot take is refused AFTER the pointers: MDCONV_PATH_DEPTHWISE on a dense layer
    dd = _conv_desc(capi, 2, 1, dtype=F32, path=capi.PATH_DEPTHWISE)
    ok = [base + 256 * i for i in range(len(args))]
    assert _call(capi, name, dd, ok) == EUNSUPPORTED
    ok[args.index("grad_offset")] += 2
    assert _call(capi, name, dd, ok) == EINVAL and "grad_offset pointer must be 4-byte aligned" in capi.last_error()
    # a skipped gradient's pointers are not looked at; bias without with_bias neither
    ds = _conv_desc(capi, 2, 1, dtype=F16, flags=capi.FLAG_NO_GRAD_INPUT | capi.FLAG_NO_GRAD_WEIGHT, with_bias=0)
    odd = [base + 256 * i for i in range(len(args))]
    for a in ("grad_input", "grad_weight", "grad_bias", "bias"):
        odd[args.index(a)] += 1
    assert capi.lib().mdconv_workspace_bytes(ctypes.byref(ds), 1) > 0
    assert _call(capi, name, ds, odd) == EWORKSPACE
    assert capi.lib().mdconv_abi_version() == 2


# ---- sampling operators ----------------------------------------------------------------------------------------------------
def _samp_desc(capi, op, dtype, cdt, inside=True, flags=0):
    """A valid descriptor of `op`; `inside` false: outside the shape rule (channel rows that are no multiple of 16 bytes)."""
    D = (8 if dtype != F32 else 4) if inside else 2
    if op in ("dcnv3", "dcnv4"):
        d = capi.MdconvDcnv3Desc() if op == "dcnv3" else capi.MdconvDcnv4Desc()
        d.dtype, d.batch, d.groups, d.group_channels = dtype, 2, 2, D
        if op == "dcnv4":
            d.coord_dtype, d.remove_center = cdt, 0
        for n, v in (("in_sz", (6, 5)), ("k_sz", (3, 3)), ("stride", (1, 1)), ("pad", (1, 1)), ("dil", (1, 1))):
            setattr(d, n, (ctypes.c_int * 2)(*v))
        d.offset_scale = 1.0
    elif op in ("msda", "fda", "msda3d"):
        d = {"msda": capi.MdconvMsdaDesc, "fda": capi.MdconvFdaDesc, "msda3d": capi.MdconvMsda3dDesc}[op]()
        d.dtype, d.coord_dtype, d.batch, d.heads, d.head_channels, d.queries, d.levels, d.points = dtype, cdt, 2, 2, D, 5, 2, 3
        for l, sz in enumerate(((4, 3), (2, 2)) if op != "msda3d" else ((2, 4, 3), (1, 2, 2))):
            for a, v in enumerate(sz):
                d.level_sz[l][a] = v
    else:
        d = capi.MdconvDroiDesc()
        d.dtype, d.coord_dtype, d.batch, d.channels, d.height, d.width = dtype, cdt, 2, 2 * D if inside else D, 6, 5
        d.rois, d.pooled_h, d.pooled_w, d.sampling_ratio, d.max_grid = 3, 2, 2, 2, 8
        d.spatial_scale, d.gamma, d.with_offset = 1.0, 0.1, 1
    d.accumulate, d.flags = 1, flags
    return d


@pytest.mark.parametrize("group", sorted(SAMP_ARGS))
def test_sampling_pointers(capi, base, group):
    op, direction = group.split(".")
    backward = direction == "backward"
    name = "mdconv_%s_%s" % (op, direction)
    args = SAMP_ARGS[group]
    ws_fn = getattr(capi.lib(), "mdconv_%s_workspace_bytes" % op)
    for dtype, cdt in PAIRINGS:
        if op == "dcnv3" and cdt != dtype:
            continue   # one dtype per call
        ces = ES[cdt]
        for inside in (True, False):
            d = _samp_desc(capi, op, dtype, cdt, inside)
            need = ws_fn(ctypes.byref(d), int(backward))
            aligned = [base + 256 * i for i in range(len(args))]
            if inside and need == 0:
                # a forward: nothing stands between the pointer checks and the launch, so only refused calls are made below
                assert not backward
                stops_at = None
            else:
                if not inside:   # (asserted before the call: a descriptor inside the rule after all would launch)
                    assert need == 0 and "shape rule" in capi.last_error(), (group, dtype, cdt, capi.last_error())
                stops_at = _call(capi, name, d, aligned)
                assert stops_at == (EWORKSPACE if inside else EUNSUPPORTED), (group, dtype, cdt, inside, stops_at, capi.last_error())
            for i, arg in enumerate(args):
                cls = AUDIT[group][arg]
                es = cls[1] if isinstance(cls, tuple) else (ces if cls == "element" else ES[dtype])
                align = 16 if cls == "16-byte" else es
                for delta in (es, 1):
                    ptrs = list(aligned)
                    ptrs[i] += delta
                    if delta % align == 0:
                        if stops_at is None:
                            continue   # (would launch)
                        rc = _call(capi, name, d, ptrs)
                        assert rc == stops_at, (group, dtype, cdt, inside, arg, delta, rc, capi.last_error())
                    else:
                        rc = _call(capi, name, d, ptrs)
                        err = capi.last_error()
                        assert rc == EINVAL and re.search(r"\b%s pointer must be %d-byte aligned" % (arg, align), err), (
                            group, dtype, cdt, inside, arg, delta, rc, err)


def test_sampling_alignment_skips_the_pointers_a_call_ignores(capi, base):
    # grad_input with MDCONV_FLAG_NO_GRAD_INPUT; offset and grad_offset of deformable RoI pooling without with_offset
    args = SAMP_ARGS["dcnv3.backward"]
    d = _samp_desc(capi, "dcnv3", F16, F16, inside=False, flags=capi.FLAG_NO_GRAD_INPUT)
    ptrs = [base + 256 * i for i in range(len(args))]
    ptrs[args.index("grad_input")] += 2
    assert _call(capi, "mdconv_dcnv3_backward", d, ptrs) == EUNSUPPORTED
    d.flags = 0
    assert _call(capi, "mdconv_dcnv3_backward", d, ptrs) == EINVAL and "grad_input" in capi.last_error()
    args = SAMP_ARGS["droi.backward"]
    d = _samp_desc(capi, "droi", F32, F32, inside=False)
    d.with_offset = 0
    ptrs = [base + 256 * i for i in range(len(args))]
    ptrs[args.index("offset")] += 1
    ptrs[args.index("grad_offset")] += 1
    assert _call(capi, "mdconv_droi_backward", d, ptrs) == EUNSUPPORTED
    d.with_offset = 1
    assert _call(capi, "mdconv_droi_backward", d, ptrs) == EINVAL and "offset pointer must be 4-byte aligned" in capi.last_error()
    # NULL comes first
    ptrs[0] = 0
    assert _call(capi, "mdconv_droi_backward", d, ptrs) == ENULL


def test_python_helpers_without_gpu(capi):
    import torch
    flat = torch.arange(64, dtype=torch.float16)
    view = flat[1:33].view(4, 8)
    assert view.data_ptr() % 16 == 2
    copy = capi.aligned_input(view)
    assert copy is not view and copy.data_ptr() % 16 == 0 and torch.equal(copy, view)
    even = flat[8:40].view(4, 8)
    assert capi.aligned_input(even) is even and capi.aligned_input(None) is None
    capi.require_aligned_result("op", "output", even)
    capi.require_aligned_result("op", "output", None)
    with pytest.raises(ValueError, match="op: output must be 16-byte aligned"):
        capi.require_aligned_result("op", "output", view)
    # a channels-last view keeps its layout through the copy
    cl = torch.zeros(1 + 2 * 32 * 2 * 2, dtype=torch.float16)[1:].as_strided((2, 32, 2, 2), (128, 1, 64, 32))
    c2 = capi.aligned_input(cl)
    assert c2.data_ptr() % 16 == 0 and c2.stride() == cl.stride()
