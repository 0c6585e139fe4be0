"""Channels-last results on the GPU (include/mdconv.h: MDCONV_FLAG_OUTPUT_CHANNELS_LAST / MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST,
``_capi.channels_last_results``): the native 16-bit forwards store ``output`` as [B, spatial..., C_out], the backward takes
``grad_output`` in that layout and stores ``grad_input`` as [B, spatial..., C_in].

Contract under test: the flags change a LAYOUT and nothing else, so every comparison is against the unflagged call on the
same inputs.  ``output`` is bit for bit the unflagged output, permuted (same accumulators, one rounding); ``grad_offset``,
``grad_mask``, ``grad_weight`` and ``grad_bias`` are bit for bit (the matrix kernels read the same grad_output values from
the copy the layout pass makes); ``grad_input`` is bit for bit under MDCONV_FLAG_DETERMINISTIC (which fixes its summation
order) and meets the 16-bit tolerance of the other tests without it.  Two cases are also compared with the oracle, as a
check of the baseline.  Every call goes through ``tests.util.guarded_run``: the workspace is sized by
``mdconv_workspace_bytes`` of the FLAGGED descriptor and sits between pattern-filled margins.  Each case names the kernel it
is meant for and checks it through the profile hooks.

The switches MDCONV_CHUNK_LIMIT_BYTES and MDCONV_HP_C2I are read once per process, so the batch-chunk loop and the one-pass
gather run in child processes, like tests/test_gpu_hp_forced.py."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from tests.cases import D2, D3, M2, M3, _c, make_inputs, ndim
from tests.util import assert_close, guarded_run, run_oracle, tup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {torch.float16: 5e-3, torch.bfloat16: 3e-2}   # the 16-bit tolerances of tests/test_gpu_hp.py
OUT, GI, DET, NO_GI, NO_GW = 64, 128, 1, 4, 8
SAMP32, WGRAD32 = 0x10, 0x40
KEYS = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")
FWD = {D2: "mdconv_deform_conv2d_forward", M2: "mdconv_modulated_deform_conv2d_forward",
       D3: "mdconv_deform_conv3d_forward", M3: "mdconv_modulated_deform_conv3d_forward"}
BWD = {D2: "mdconv_deform_conv2d_backward", M2: "mdconv_modulated_deform_conv2d_backward",
       D3: "mdconv_deform_conv3d_backward", M3: "mdconv_modulated_deform_conv3d_backward"}


def _fmt(nd):
    return torch.channels_last if nd == 2 else torch.channels_last_3d


def _bits(t):
    """The tensor's values as integers in logical (NCHW) order: equality of these is equality bit for bit."""
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(_bits(got), _bits(want)):
        diff = (got.float() - want.float()).abs()
        raise AssertionError("%s: %d of %d elements differ, max |diff| %.3e" % (name, int((_bits(got) != _bits(want)).sum()),
                                                                               got.numel(), diff.max().item()))


def _inputs(case, dtype, samp32=False):
    t = make_inputs(case, dtype=dtype, device="cuda")
    if samp32:
        t["offset"] = t["offset"].float()
        t["mask"] = None if t["mask"] is None else t["mask"].float()
    return t


def _descriptor(case, t, flags, accumulate, wgrad32=False):
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    nd = ndim(case)
    k, s, p, d = (tup(case[x], nd) for x in ("k", "stride", "padding", "dilation"))
    desc = M._desc(nd, case["op"] in (M2, M3), t["input"], t["weight"], k, s, p, d, case["groups"], case["dgroups"],
                   case["in_step"], case["bias"])
    if t["offset"].dtype == torch.float32 and t["input"].dtype != torch.float32:
        desc.dtype |= SAMP32
    if wgrad32:
        desc.dtype |= WGRAD32
    desc.flags = flags          # (no mode of the calling thread: exactly these flags)
    desc.accumulate = int(accumulate)
    return desc


class Runner:
    """Calls of the C ABI through the pattern-guarded workspace helper, with the profile hooks on."""

    def __init__(self):
        from modulated_deform_conv_amd import MDCONV_CUDA as M
        from modulated_deform_conv_amd import _capi
        self.M, self.capi = M, _capi
        self.touched, self.calls = [], []
        self.run = guarded_run(self.touched, self.calls)

    def forward(self, case, t, flags, out):
        p = self.M._ptr
        b = t["bias"] if case["bias"] else t["input"].new_empty(0)
        args = [p(t["input"]), p(t["weight"]), p(b), p(t["offset"])]
        if case["op"] in (M2, M3):
            args.append(p(t["mask"]))
        args.append(p(out))
        desc = _descriptor(case, t, flags, True)
        self.capi.profile_enable(True)
        self.capi.profile_reset()
        try:
            self.run(FWD[case["op"]], desc, False, args, t["input"])
            torch.cuda.synchronize()
            name = self.capi.lib().mdconv_profile_name(0).decode()
        finally:
            self.capi.profile_enable(False)
        assert self.capi.last_kernels() == "hp", self.capi.last_kernels()
        assert not self.touched, self.touched
        return name

    def backward(self, case, t, flags, grad_output, g, accumulate=False, wgrad32=False):
        """``g``: dict of the gradient buffers (None where the call has none / leaves one out).  Returns the name of the
        backward kernel (profile slot 1)."""
        p = self.M._ptr
        op = case["op"]
        x, w, off, m = t["input"], t["weight"], t["offset"], t["mask"]
        b = t["bias"] if case["bias"] else x.new_empty(0)
        gi, goff, gm, gw, gb = (g[k] for k in KEYS)
        if op == M2:
            args = [p(x), p(w), p(b), p(off), p(m), p(grad_output), p(gi), p(goff), p(gm), p(gw), p(gb)]
        elif op == M3:
            args = [p(x), p(w), p(b), p(off), p(m), p(gi), p(gw), p(gb), p(goff), p(gm), p(grad_output)]
        else:
            args = [p(x), p(w), p(b), p(off), p(gi), p(gw), p(gb), p(goff), p(grad_output)]
        desc = _descriptor(case, t, flags, accumulate, wgrad32)
        self.capi.profile_enable(True)
        self.capi.profile_reset()
        try:
            self.run(BWD[op], desc, True, args, x)
            torch.cuda.synchronize()
            L = self.capi.lib()
            name = L.mdconv_profile_name(1).decode()
            self.launches = L.mdconv_profile_read(1, ctypes.byref(ctypes.c_double(0)))   # of the backward kernel: one per chunk
            self.gather = L.mdconv_profile_name(3).decode()
        finally:
            self.capi.profile_enable(False)
        assert self.capi.last_kernels() == "hp", self.capi.last_kernels()
        assert not self.touched, self.touched
        return name


def _grad_buffers(case, t, fill, gi_cl, wgrad32=False, skip_input=False, skip_weight=False, seed=7):
    """Gradient buffers: ``fill`` None -> NaN (overwrite mode must write every element), else reproducible random values
    scaled by ``fill`` (accumulate mode adds to them); grad_input channels-last with ``gi_cl``."""
    gen = torch.Generator().manual_seed(seed)

    def new(ref, dtype=None):
        dtype = dtype or ref.dtype
        if fill is None:
            return torch.full(ref.shape, float("nan"), dtype=dtype, device=ref.device)
        return (torch.randn(ref.shape, generator=gen) * fill).to(dtype).to(ref.device)

    wdt = torch.float32 if wgrad32 else None
    g = dict(grad_input=None if skip_input else new(t["input"]), grad_offset=new(t["offset"]),
             grad_mask=None if t["mask"] is None else new(t["mask"]),
             grad_weight=None if skip_weight else new(t["weight"], wdt),
             grad_bias=new(t["bias"], wdt) if case["bias"] and not skip_weight else None)
    if gi_cl and g["grad_input"] is not None:
        g["grad_input"] = g["grad_input"].contiguous(memory_format=_fmt(ndim(case)))
        assert not g["grad_input"].is_contiguous()
    return g


# ------------------------------------------------------------------------------------------------ forward
F = {
    # 9 x 7 image, B = 3: S_o = 63 -- the last 128-pixel tile is partial and a tile straddles two images
    "c64_o64_9x7": (_c("clr_mdcn2d_c64_o64_9x7", M2, 3, 64, 64, (9, 7), 3, seed=401), "hp_fwd2_kernel"),
    "c64_o64_9x7_nobias": (_c("clr_mdcn2d_c64_o64_9x7_nb", M2, 3, 64, 64, (9, 7), 3, bias=False, seed=402), "hp_fwd2_kernel"),
    "o32": (_c("clr_mdcn2d_c64_o32", M2, 3, 64, 32, (9, 7), 3, seed=403), "hp_fwd2_kernel"),            # one block
    "o160_rows_of_1": (_c("clr_mdcn2d_c32_o160", M2, 3, 32, 160, (9, 7), 3, seed=404), "hp_fwd2_kernel"),   # 5 single-block rows
    # 68 tiles x 2 rows: rows of 4 blocks, the last row holds one (hp_dims: MB = 4 from half a workgroup per CU on)
    "o160_rows_of_4": (_c("clr_dcn2d_c32_o160_48x60", D2, 3, 32, 160, (48, 60), 3, seed=405), "hp_fwd2_kernel"),
    "o64_rows_of_2": (_c("clr_dcn2d_c32_o64_96x88", D2, 2, 32, 64, (96, 88), 3, seed=406), "hp_fwd2_kernel"),  # 132 tiles: MB = 2
    "o40": (_c("clr_mdcn2d_c64_o40", M2, 3, 64, 40, (9, 7), 3, seed=407), "hp_fwd2_kernel"),            # a partial 32-channel block
    "g2": (_c("clr_mdcn2d_c64_o64_g2", M2, 3, 64, 64, (9, 7), 3, groups=2, seed=408), "hp_fwd2_kernel"),  # the GRP instance
    "dg4": (_c("clr_mdcn2d_c64_dg4_o64", M2, 3, 64, 64, (9, 7), 3, dgroups=4, seed=409), "hp_fwd_kernel"),
    "s2": (_c("clr_mdcn2d_c64_o96_s2", M2, 2, 64, 96, (12, 11), 3, stride=2, seed=410), "hp_fwd2_kernel"),
    "3d": (_c("clr_dcn3d_c32_o32", D3, 2, 32, 32, (3, 4, 5), 3, seed=411), "hp_fwd2_kernel"),
}
F_PARAMS = [("c64_o64_9x7", torch.float16, False, True), ("c64_o64_9x7", torch.bfloat16, False, False),
            ("c64_o64_9x7_nobias", torch.float16, False, False), ("c64_o64_9x7", torch.bfloat16, True, False),
            ("o32", torch.float16, False, False), ("o160_rows_of_1", torch.float16, False, False),
            ("o160_rows_of_4", torch.bfloat16, False, False), ("o64_rows_of_2", torch.float16, False, False),
            ("o40", torch.float16, False, False), ("o40", torch.bfloat16, False, False), ("g2", torch.float16, False, False),
            ("dg4", torch.float16, False, False), ("dg4", torch.bfloat16, False, False), ("s2", torch.bfloat16, False, False),
            ("3d", torch.float16, False, True), ("3d", torch.bfloat16, False, False)]


@pytest.mark.parametrize("name, dtype, samp32, oracle", F_PARAMS,
                         ids=["%s-%s%s" % (n, str(d)[6:], "-s32" if s else "") for n, d, s, _ in F_PARAMS])
def test_forward_output_is_the_unflagged_output_permuted(name, dtype, samp32, oracle):
    case, kernel = F[name]
    t = _inputs(case, dtype, samp32)
    r = Runner()
    ref = torch.full_like(t["grad_output"], float("nan"))
    assert r.forward(case, t, 0, ref) == kernel
    out = torch.full_like(t["grad_output"], float("nan")).contiguous(memory_format=_fmt(ndim(case)))
    assert not out.is_contiguous()
    # (the grad_input flag is for backwards: forwards accept and ignore it)
    assert r.forward(case, t, OUT | GI, out) == kernel          # the same kernel family and kernel: only the store differs
    assert r.calls[0] == r.calls[1]                             # ... and the forward's workspace is unchanged
    assert torch.isfinite(ref.float()).all()
    _same_bits("output", out, ref)
    if oracle:
        want = run_oracle(case, {k: (None if v is None else v.float()) for k, v in t.items()}, torch.float32)[0]
        assert_close("output", out.float(), want, TOL[dtype])


# ------------------------------------------------------------------------------------------------ backward
B = {
    "bwd2": (_c("clr_mdcn2d_c64_o64_9x7_b", M2, 3, 64, 64, (9, 7), 3, seed=421), "hp_bwd2_kernel"),      # S_i = 63 as well
    "bwd3": (_c("clr_mdcn2d_c64_dg4_o64_b", M2, 2, 64, 64, (9, 10), 3, dgroups=4, seed=422), "hp_bwd3_kernel"),   # groups of 16
    "bwd": (_c("clr_mdcn2d_c256_o64_dg8", M2, 2, 256, 64, (9, 8), 3, dgroups=8, seed=423), "hp_bwd_kernel"),
    "gpad": (_c("clr_mdcn2d_c96_dg4_o96", M2, 2, 96, 96, (9, 10), 3, dgroups=4, seed=424), "hp_bwd2_kernel"),  # groups of 24 as 32
    # groups of 12 channels run as 16: an octet of the kernels' rows holds 4 padding channels -- the element-wise store
    "gpad12": (_c("clr_mdcn2d_c48_dg4_o64", M2, 3, 48, 64, (8, 7), 3, dgroups=4, seed=425), "hp_bwd3_kernel"),
    # 294 tiles of 128 pixels: more than one per CU, so 96 channels run width-padded to 128 on hp_bwd3
    "wpad": (_c("clr_dcn2d_c96_o96_b12_56", D2, 12, 96, 96, (56, 56), 3, seed=426), "hp_bwd3_kernel"),
    "dg2": (_c("clr_mdcn2d_c64_dg2_o32", M2, 2, 64, 32, (9, 9), 3, dgroups=2, seed=427), None),
    "3d": (_c("clr_mdcn3d_c32_o32", M3, 2, 32, 32, (3, 4, 5), 3, seed=428), None),
    "d3d": (_c("clr_dcn3d_c64_o32_s2", D3, 2, 64, 32, (5, 6, 7), 3, stride=2, seed=429), None),
}


def _check_backward(name, dtype, flags=OUT | GI, det=True, accumulate=False, samp32=False, wgrad32=False, oracle=False):
    """The flagged backward against the unflagged one on the same inputs (and the same pre-filled buffers)."""
    case, kernel = B[name]
    nd = ndim(case)
    t = _inputs(case, dtype, samp32)
    base = DET if det else 0
    fill = 0.5 if accumulate else None
    r = Runner()
    ref = _grad_buffers(case, t, fill, False, wgrad32)
    first = r.backward(case, t, base, t["grad_output"], ref, accumulate, wgrad32)
    assert kernel is None or first == kernel, first             # (None: whichever kernel the plan picks)
    kernel = first
    got = _grad_buffers(case, t, fill, bool(flags & GI), wgrad32)
    go = t["grad_output"].contiguous(memory_format=_fmt(nd)) if flags & OUT else t["grad_output"]
    assert (not go.is_contiguous()) == bool(flags & OUT)
    assert r.backward(case, t, base | flags, go, got, accumulate, wgrad32) == kernel   # the route of the unflagged call
    # the workspace: one chunk's grad_output in 16 bits for the output side (a 256-byte slot), nothing for grad_input
    grow = (t["grad_output"].numel() * 2 + 255) // 256 * 256 if flags & OUT else 0
    assert r.calls[1][1] == r.calls[0][1] + grow, r.calls
    for key in KEYS:
        if ref[key] is None:
            assert got[key] is None
            continue
        assert torch.isfinite(ref[key].float()).all(), key
        if key == "grad_input":
            if not det:
                assert_close(key, got[key].float(), ref[key].float(), TOL[dtype])   # two 16-bit calls: to rounding
                continue
        _same_bits(key, got[key], ref[key])
    if oracle:
        want = run_oracle(case, {k: (None if v is None else v.float()) for k, v in t.items()}, torch.float32)[1]
        for key in KEYS:
            if want[key] is not None:
                assert_close(key, got[key].float(), want[key], TOL[dtype])


B_PARAMS = [("bwd2", torch.float16), ("bwd2", torch.bfloat16), ("bwd3", torch.float16), ("bwd3", torch.bfloat16),
            ("bwd", torch.float16), ("gpad", torch.float16), ("gpad", torch.bfloat16), ("gpad12", torch.float16),
            ("wpad", torch.float16), ("dg2", torch.bfloat16), ("3d", torch.float16), ("3d", torch.bfloat16), ("d3d", torch.bfloat16)]


@pytest.mark.parametrize("name, dtype", B_PARAMS, ids=["%s-%s" % (n, str(d)[6:]) for n, d in B_PARAMS])
def test_backward_with_both_flags_is_the_unflagged_backward(name, dtype):
    _check_backward(name, dtype, oracle=(name, dtype) in (("bwd2", torch.float16), ("3d", torch.float16)))


@pytest.mark.parametrize("flags", [OUT, GI], ids=["output_side_only", "grad_input_only"])
def test_each_flag_alone(flags):
    _check_backward("bwd2", torch.float16, flags=flags)
    _check_backward("gpad", torch.bfloat16, flags=flags)


@pytest.mark.parametrize("name, dtype", [("bwd2", torch.float16), ("gpad", torch.bfloat16), ("gpad12", torch.float16),
                                         ("3d", torch.bfloat16)], ids=["bwd2-fp16", "gpad-bf16", "gpad12-fp16", "3d-bf16"])
def test_accumulate_mode_adds_in_the_channels_last_layout(name, dtype):
    _check_backward(name, dtype, accumulate=True)


def test_fp32_weight_gradients_and_fp32_sampling():
    _check_backward("bwd2", torch.float16, wgrad32=True)
    _check_backward("bwd3", torch.bfloat16, wgrad32=True, accumulate=True)
    _check_backward("bwd2", torch.float16, samp32=True)


def test_without_deterministic_mode_grad_input_agrees_to_rounding():
    _check_backward("bwd2", torch.bfloat16, det=False)
    _check_backward("bwd3", torch.float16, det=False)


def test_deterministic_mode_twice_gives_the_same_bits():
    case, kernel = B["bwd3"]
    t = _inputs(case, torch.float16)
    go = t["grad_output"].contiguous(memory_format=torch.channels_last)
    r = Runner()
    runs = []
    for _ in range(2):
        g = _grad_buffers(case, t, None, True)
        assert r.backward(case, t, DET | OUT | GI, go, g) == kernel
        runs.append(g)
    for key in KEYS:
        _same_bits(key, runs[1][key], runs[0][key])


def test_selective_backward_with_the_flags():
    case, kernel = B["bwd2"]
    t = _inputs(case, torch.float16)
    go = t["grad_output"].contiguous(memory_format=torch.channels_last)
    r = Runner()
    ref = _grad_buffers(case, t, None, False)
    r.backward(case, t, DET, t["grad_output"], ref)
    # NO_GRAD_INPUT with the grad_input flag and a NULL pointer: accepted, nothing to do
    g = _grad_buffers(case, t, None, False, skip_input=True)
    assert r.backward(case, t, DET | NO_GI | GI | OUT, go, g) == kernel
    for key in ("grad_offset", "grad_mask", "grad_weight", "grad_bias"):
        _same_bits(key, g[key], ref[key])
    # NO_GRAD_WEIGHT with the output flag: grad_bias is not summed, the weight pointers may be NULL
    g = _grad_buffers(case, t, None, True, skip_weight=True)
    assert r.backward(case, t, DET | NO_GW | OUT | GI, go, g) == kernel
    for key in ("grad_input", "grad_offset", "grad_mask"):
        _same_bits(key, g[key], ref[key])


# ------------------------------------------------------------------------------------------------ unsupported shapes
O36 = _c("clr_mdcn2d_c64_o36", M2, 2, 64, 36, (9, 7), 3, seed=431)


def test_unsupported_rows_are_refused_by_the_library_before_anything_runs():
    t = _inputs(O36, torch.float16)
    r = Runner()
    out = torch.full_like(t["grad_output"], float("nan")).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match=r"\(-5\).*MDCONV_FLAG_OUTPUT_CHANNELS_LAST"):
        r.forward(O36, t, OUT, out)
    assert torch.isnan(out.float()).all()                       # nothing was launched
    g = _grad_buffers(O36, t, None, True)
    with pytest.raises(RuntimeError, match=r"\(-5\).*MDCONV_FLAG_OUTPUT_CHANNELS_LAST"):
        r.backward(O36, t, OUT | GI, t["grad_output"].contiguous(memory_format=torch.channels_last), g)
    assert all(torch.isnan(v.float()).all() for v in g.values() if v is not None)


def test_binding_falls_back_to_contiguous_temporaries_inside_the_mode(monkeypatch):
    """C_out = 36: the library does not honour the output side, grad_input (C_in = 64) it does.  The binding never raises over
    the mode: the caller's channels-last tensors hold the right values either way."""
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    from modulated_deform_conv_amd import _capi
    case, t = O36, _inputs(O36, torch.float16)
    touched, calls = [], []
    monkeypatch.setattr(M, "_run", guarded_run(touched, calls))
    x, w, b, off, m, go = (t[k] for k in ("input", "weight", "bias", "offset", "mask", "grad_output"))
    geo = (3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 64, True)
    # the reference results, outside the mode
    ref_out = M.modulated_deform_conv2d_forward_cuda(x, w, b, off, m, *geo)
    with _capi.deterministic():
        ref = M.modulated_deform_conv2d_backward_cuda(x, w, b, off, m, go, *geo)
    assert ref_out.is_contiguous() and ref[0].is_contiguous()
    out = torch.full_like(go, float("nan")).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="output tensor has to be contiguous"):
        M._forward(2, True, FWD[M2], x, w, b, off, m, out, (3, 3), (1, 1), (1, 1), (1, 1), 1, 1, 64, True)
    with _capi.channels_last_results():
        M._forward(2, True, FWD[M2], x, w, b, off, m, out, (3, 3), (1, 1), (1, 1), (1, 1), 1, 1, 64, True)
        assert out.is_contiguous(memory_format=torch.channels_last) and not out.is_contiguous()
        _same_bits("output", out, ref_out)
        # the pair that allocates its results, with a channels-last input: output stays contiguous (the query says 0),
        # grad_input is channels-last (the query says 1), a channels-last grad_output is taken through a copy
        xcl = x.contiguous(memory_format=torch.channels_last)
        out2 = M.modulated_deform_conv2d_forward_cuda(xcl, w, b, off, m, *geo)
        assert out2.is_contiguous()
        _same_bits("output", out2, ref_out)
        with _capi.deterministic():
            got = M.modulated_deform_conv2d_backward_cuda(xcl, w, b, off, m, go.contiguous(memory_format=torch.channels_last), *geo)
        assert got[0].is_contiguous(memory_format=torch.channels_last) and not got[0].is_contiguous()
        for key, a, r_ in zip(KEYS, (got[0], got[1], got[2], got[3], got[4]), (ref[0], ref[1], ref[2], ref[3], ref[4])):
            _same_bits(key, a, r_)
    assert _capi.last_kernels() == "hp" and not touched, touched


# ------------------------------------------------------------------------------------------------ modules
def _module_pair(cls, dtype, x, *args, **kw):
    torch.manual_seed(0)
    plain = cls(*args, **kw).cuda()
    on = cls(*args, channels_last_results=True, **kw).cuda()
    on.load_state_dict(plain.state_dict())
    res = []
    for mod in (plain, on):
        xi = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=dtype):
            y = mod(xi)
        # a channels-last model hands a channels-last grad_output back
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).to(y.dtype).cuda().contiguous(
            memory_format=_fmt(x.dim() - 2))
        y.backward(gy)
        res.append((y, xi.grad, {k: p.grad for k, p in mod.named_parameters()}))
    return res


@pytest.mark.parametrize("nd, dtype", [(2, torch.float16), (3, torch.bfloat16)], ids=["2d-fp16", "3d-bf16"])
def test_modules_return_channels_last_output_and_input_gradient(nd, dtype):
    from modulated_deform_conv_amd import _capi
    from modulated_deform_conv_amd import modulated_deform_conv as mdc
    gen = torch.Generator().manual_seed(3)
    if nd == 2:
        x = torch.randn(3, 64, 9, 7, generator=gen).cuda().contiguous(memory_format=torch.channels_last)
        cls, args = mdc.ModulatedDeformConv2dPack, (64, 64, 3)
    else:
        x = torch.randn(2, 32, 3, 4, 5, generator=gen).cuda().contiguous(memory_format=torch.channels_last_3d)
        cls, args = mdc.ModulatedDeformConv3dPack, (32, 32, 3)
    # (the offset / mask branch is the framework's convolution: its deterministic algorithms, so that the gradients of ITS
    # parameters -- computed from this layer's grad_offset / grad_mask -- can be compared bit for bit too)
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        (y0, gx0, gp0), (y1, gx1, gp1) = _module_pair(cls, dtype, x, *args, padding=1, bias=True)
    finally:
        torch.backends.cudnn.deterministic = prev
    assert _capi.last_kernels() == "hp"
    fmt = _fmt(nd)
    assert y0.is_contiguous()                                        # the default module: as before
    assert y1.is_contiguous(memory_format=fmt) and not y1.is_contiguous()
    assert gx1.is_contiguous(memory_format=fmt) and not gx1.is_contiguous()
    assert y1.dtype == dtype and torch.equal(y1, y0)
    # (autograd runs the backward on its own thread, outside any _capi.deterministic() of this one: grad_input sums its
    # lists in arrival order, so x.grad agrees like two 16-bit calls do; everything else is bit for bit)
    assert_close("x.grad", gx1, gx0, TOL[dtype])
    assert set(gp0) == set(gp1)
    for k in gp0:
        assert torch.equal(gp1[k], gp0[k]), k


# ------------------------------------------------------------------------------------------------ child processes
CHILD = r"""
import sys
sys.path.insert(0, %r)
import torch
from tests.cases import M2, _c
from tests import test_gpu_channels_last_results as T
from modulated_deform_conv_amd import _capi
which = sys.argv[1]
if which == "chunks":
    # tests/test_gpu_chunk_plans.py, scenario C: 9 + 9 + 2 images of 64 x 64 -- 288 tiles run hp_bwd3, the tail's 64 hp_bwd2
    case = _c("clr_chunk_mdcn2d_c64_o64", M2, 20, 64, 64, (64, 64), 3, seed=441)
    dtype, tail_kernel = torch.float16, "hp_bwd2_kernel"
else:
    # the one-pass gather (MDCONV_HP_C2I=1): hp_col2im_kernel stores grad_input itself
    case = _c("clr_c2i_mdcn2d_c64_dg2_o32", M2, 2, 64, 32, (13, 12), 3, dgroups=2, seed=442)
    dtype, tail_kernel = torch.bfloat16, None
t = T._inputs(case, dtype)
r = T.Runner()
ref_out = torch.full_like(t["grad_output"], float("nan"))
r.forward(case, t, 0, ref_out)
out = torch.full_like(t["grad_output"], float("nan")).contiguous(memory_format=torch.channels_last)
r.forward(case, t, T.OUT, out)
T._same_bits("output", out, ref_out)
for accumulate in (False, True):
    fill = 0.5 if accumulate else None
    ref = T._grad_buffers(case, t, fill, False)
    k0 = r.backward(case, t, T.DET, t["grad_output"], ref, accumulate)
    got = T._grad_buffers(case, t, fill, True)
    k1 = r.backward(case, t, T.DET | T.OUT | T.GI, t["grad_output"].contiguous(memory_format=torch.channels_last), got, accumulate)
    assert k0 == k1, (k0, k1)
    if tail_kernel:
        assert k1 == tail_kernel, k1                    # (the name of the LAST launch: the tail's kernel)
        assert r.launches == 3, r.launches              # three chunks
    for key in T.KEYS:
        T._same_bits(key, got[key], ref[key])
if which == "c2i":
    assert r.gather == "hp_col2im_kernel", r.gather
print("CLR_CHILD_OK", which)
"""


@pytest.mark.parametrize("which, env", [("chunks", {"MDCONV_CHUNK_LIMIT_BYTES": "4980736"}), ("c2i", {"MDCONV_HP_C2I": "1"})],
                         ids=["batch_chunks_tail_takes_another_plan", "one_pass_gather"])
def test_in_a_child_process(which, env):
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT, which], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=420)
    assert "CLR_CHILD_OK " + which in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
