"""Selective backward on the GPU (include/mdconv.h: MDCONV_FLAG_NO_GRAD_INPUT / MDCONV_FLAG_NO_GRAD_WEIGHT,
``_capi.skip_grads``): a backward that leaves out grad_input, the weight gradients, or both.

Contract under test: the skipped gradients' buffers are never touched (NULL or not, accumulate or overwrite); on the
matrix-core kernels every requested gradient is BIT-IDENTICAL to what the same call without the flags stores (grad_input
under deterministic mode, which fixes its summation order) -- the flags only remove stages, they never change a sum; on
the shape-generic kernels (floating-point atomics) the requested gradients meet the tolerances of the parity tests
against the oracle.  The stages are really gone (profile slots), the smaller workspace is never overrun, and the Python
layers (autograd Functions, modules, the masked torch.library operator) skip by themselves from ``needs_input_grad``.

The switches MDCONV_HP_BWD and MDCONV_CHUNK_LIMIT_BYTES are read once per process, so the hp_bwd3 variant and the
batch-chunk loop run in child processes, like tests/test_gpu_hp_forced.py."""
import contextlib
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from tests.cases import CASE_BY_NAME, D2, D3, M2, M3, _c, make_inputs, ndim
from tests.test_gpu_hp import CASE_BY_HP, FALLBACK_CASES, TOL
from tests.util import assert_close, guarded_run, run_oracle, tup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (skip grad_input, skip grad_weight + grad_bias)
FLAG_SETS = [(False, True), (True, False), (True, True)]
FLAG_IDS = ["no_weight", "no_input", "offsets_only"]
KEYS = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")


def _requested(skip):
    return [k for k in KEYS if not ((k == "grad_input" and skip[0]) or (k in ("grad_weight", "grad_bias") and skip[1]))]


def _geometry(case):
    nd = ndim(case)
    k, s, p, d = (tup(case[x], nd) for x in ("k", "stride", "padding", "dilation"))
    return k, s, p, d, (case["groups"], case["dgroups"], case["in_step"], case["bias"])


def _descriptor(case, t):
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    k, s, p, d, tail = _geometry(case)
    desc = M._desc(ndim(case), case["op"] in (M2, M3), t["input"], t["weight"], k, s, p, d, *tail)
    if M._sampling_f32(t["input"], t["offset"], t["mask"]):
        desc.dtype |= 0x10
    return desc


def _deterministic_supported(case, t):
    from modulated_deform_conv_amd import _capi
    return bool(_capi.lib().mdconv_deterministic_supported(ctypes.byref(_descriptor(case, t)), 1))


def backward(case, t, skip=(False, False), accumulate=False, fill=None):
    """One backward of ``case`` through the MDCONV_CUDA entry points with caller-allocated gradients, inside
    ``_capi.skip_grads(*skip)``.  ``fill`` None: fresh buffers, and None is passed at the skipped positions; a number: every
    gradient -- the skipped ones too -- is a real tensor pre-filled with it.  Returns the dict of what was passed."""
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    from modulated_deform_conv_amd import _capi
    op = case["op"]
    k, s, p, d, tail = _geometry(case)
    geo = k + s + p + d + tail
    x, w, off, m, go = t["input"], t["weight"], t["offset"], t["mask"], t["grad_output"]
    b = t["bias"] if case["bias"] else x.new_empty(0)
    new = (lambda ref: torch.empty_like(ref)) if fill is None else (lambda ref: torch.full_like(ref, fill))
    g = dict(grad_input=new(x), grad_offset=new(off), grad_mask=None if m is None else new(m), grad_weight=new(w),
             grad_bias=new(b) if case["bias"] else None)
    if fill is None:
        for key in KEYS:
            if key not in _requested(skip):
                g[key] = None
    gi, goff, gm, gw = g["grad_input"], g["grad_offset"], g["grad_mask"], g["grad_weight"]
    gb = g["grad_bias"] if case["bias"] or g["grad_weight"] is None else x.new_empty(0)
    mode = contextlib.nullcontext() if accumulate else _capi.overwrite_grads()
    with _capi.skip_grads(input=skip[0], weight=skip[1]), mode:
        if op == M2:   # (the export of this operator allocates its results: the helpers underneath it, with the same checks)
            desc = M._desc(2, True, x, w, k, s, p, d, *tail)
            M._check_side(desc, 2, M._prod(k), off, m, go, "grad_output", M._out_shape(desc, 2))
            pi, pw, pb = M._skipped(gi, gw, gb)
            M._backward_checks(x, w, off, m, pi, pw, pb, goff, gm, go, desc, case["bias"])
            ptr = M._ptr
            M._run("mdconv_modulated_deform_conv2d_backward", desc, True,
                   [ptr(x), ptr(w), ptr(b), ptr(off), ptr(m), ptr(go), ptr(pi), ptr(goff), ptr(gm), ptr(pw), ptr(pb)], x)
        elif op == D2:
            M.deform_conv2d_backward_cuda(x, w, b, off, gi, gw, gb, goff, go, *geo)
        elif op == D3:
            M.deform_conv3d_backward_cuda(x, w, b, off, gi, gw, gb, goff, go, *geo)
        else:
            M.modulated_deform_conv3d_backward_cuda(x, w, b, off, m, gi, gw, gb, goff, gm, go, *geo)
    torch.cuda.synchronize()
    return g


def check_contract(case, t, tol, flag_sets=FLAG_SETS):
    """Full call, then every flagged call on the same inputs in overwrite mode: bit-identical requested gradients under
    deterministic mode where the backward supports it, else each requested gradient against the oracle within ``tol``."""
    from modulated_deform_conv_amd import _capi
    det = _deterministic_supported(case, t)
    want = None
    with _capi.deterministic(det):
        full = backward(case, t)
        kernels = _capi.last_kernels()
        assert (kernels in ("f32", "hp")) == det, (case["name"], kernels, det)
        for skip in flag_sets:
            got = backward(case, t, skip)
            assert _capi.last_kernels() == kernels, (case["name"], skip)   # the route of the unflagged call
            for key in KEYS:
                if key not in _requested(skip):
                    assert got[key] is None
                elif full[key] is None:
                    assert got[key] is None, key
                elif det:
                    assert torch.equal(got[key], full[key]), (case["name"], skip, key,
                                                              (got[key].float() - full[key].float()).abs().max().item())
                else:
                    if want is None:
                        odt = torch.float64 if t["input"].dtype == torch.float64 else torch.float32
                        want = run_oracle(case, {n: (None if v is None else v.to(odt)) for n, v in t.items()}, odt)[1]
                    assert_close(key, got[key].to(want[key].dtype), want[key], tol)


F32_CASES = ["mfma_mdcn2d_c32_o48_9x10", "mfma_dcn3d_c16_o16_5x6x5", "mfma_dcn2d_g2_c32_o32", "mfma_split_mdcn2d_dg4_c128_o128",
             "mfma_pad_mdcn2d_dg4_c96_o64", "mfma_padt_mdcn2d_c32_o8_s2", "cfg1_dcn2d_c4_8x8_b1", "mdcn3d_basic"]


@pytest.mark.parametrize("name", F32_CASES)
def test_contract_fp32(name):
    case = CASE_BY_NAME[name]
    check_contract(case, make_inputs(case, dtype=torch.float32, device="cuda"), 1e-4)


def test_contract_fp64_shape_generic():
    case = CASE_BY_NAME["mdcn3d_basic"]
    check_contract(case, make_inputs(case, dtype=torch.float64, device="cuda"), 1e-4)


HALF_CASES = [CASE_BY_HP["hp_mdcn2d_c256_o256_g32_dg4"], CASE_BY_HP["hp_mdcn2d_c256_o64_dg8"], FALLBACK_CASES[0], FALLBACK_CASES[2]]
assert [c["name"] for c in HALF_CASES[2:]] == ["fb_mdcn2d_c512_o64", "fb_dcn3d_c24_o8_g2"]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", HALF_CASES, ids=lambda c: c["name"])
def test_contract_16bit(case, dtype):
    check_contract(case, make_inputs(case, dtype=dtype, device="cuda"), TOL[dtype])


def _fp32_sampling(t):
    return dict(t, offset=t["offset"].float(), mask=None if t["mask"] is None else t["mask"].float())


@pytest.mark.parametrize("name", ["hp_mdcn2d_c32_o32", "fb_mdcn2d_c512_o64"])
def test_contract_16bit_with_fp32_offsets_and_masks(name):
    case = CASE_BY_HP.get(name) or FALLBACK_CASES[0]
    t = _fp32_sampling(make_inputs(case, dtype=torch.float16, device="cuda"))
    check_contract(case, t, TOL[torch.float16])


def test_modulated_2d_export_returns_none_at_skipped_positions():
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    from modulated_deform_conv_amd import _capi
    case = CASE_BY_NAME["mfma_mdcn2d_c32_o48_9x10"]
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    k, s, p, d, tail = _geometry(case)
    args = (t["input"], t["weight"], t["bias"], t["offset"], t["mask"], t["grad_output"]) + k + s + p + d + tail
    with _capi.deterministic():
        full = M.modulated_deform_conv2d_backward_cuda(*args)
        for skip in FLAG_SETS:
            with _capi.skip_grads(input=skip[0], weight=skip[1]):
                got = M.modulated_deform_conv2d_backward_cuda(*args)
            torch.cuda.synchronize()
            for key, a, b in zip(("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias"), got, full):
                if key in _requested(skip):
                    assert torch.equal(a, b), (skip, key)
                else:
                    assert a is None, (skip, key)


@pytest.mark.parametrize("skip", FLAG_SETS, ids=FLAG_IDS)
@pytest.mark.parametrize("which", ["fp32", "fp16", "fp32_generic"])
def test_skipped_buffers_are_not_touched_in_accumulate_mode(which, skip):
    """Real, pre-filled tensors at the skipped positions: unchanged afterwards; the requested ones hold pattern + gradient
    exactly as after the unflagged accumulate call."""
    from modulated_deform_conv_amd import _capi
    case, dtype = {"fp32": (CASE_BY_NAME["mfma_dcn3d_c16_o16_5x6x5"], torch.float32),
                   "fp16": (CASE_BY_HP["hp_dcn3d_c64_o32_s2"], torch.float16),
                   "fp32_generic": (CASE_BY_NAME["mdcn3d_basic"], torch.float32)}[which]
    t = make_inputs(case, dtype=dtype, device="cuda")
    det = which != "fp32_generic"
    with _capi.deterministic(det):
        full = backward(case, t, accumulate=True, fill=0.5)
        got = backward(case, t, skip, accumulate=True, fill=0.5)
    for key in KEYS:
        if full[key] is None:
            continue
        if key not in _requested(skip):
            assert torch.equal(got[key], torch.full_like(got[key], 0.5)), key
        elif det:
            assert torch.equal(got[key], full[key]), key
        else:   # floating-point atomics: the sums agree to rounding
            assert_close(key, got[key], full[key], 1e-4)
        if key in _requested(skip):
            assert not torch.equal(got[key], torch.full_like(got[key], 0.5)), key   # (it was written)


@pytest.mark.parametrize("skip", FLAG_SETS, ids=FLAG_IDS)
def test_skipped_buffers_are_not_touched_in_overwrite_mode(skip):
    case = CASE_BY_NAME["mfma_mdcn2d_c32_o48_9x10"]
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    got = backward(case, t, skip, accumulate=False, fill=0.5)
    for key in KEYS:
        if key not in _requested(skip):
            assert torch.equal(got[key], torch.full_like(got[key], 0.5)), key


def _slot_launches():
    from modulated_deform_conv_amd import _capi
    tot = ctypes.c_double(0)
    return {which: _capi.lib().mdconv_profile_read(which, ctypes.byref(tot)) for which in (1, 2, 3)}


def profiled_slots(case, t, skip):
    """Launches per profile slot (1 = GEMM-1 / the fused 16-bit kernel, 2 = GEMM-2, 3 = the grad_input gather) and the
    kernel names of one backward."""
    from modulated_deform_conv_amd import _capi
    _capi.profile_enable(True)
    _capi.profile_reset()
    try:
        backward(case, t, skip)
        return _slot_launches(), set(_capi.profile_read())
    finally:
        _capi.profile_enable(False)


def test_the_work_is_really_gone_fp32():
    case = CASE_BY_NAME["mfma_mdcn2d_c32_o48_9x10"]
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    full, _ = profiled_slots(case, t, (False, False))
    assert full[1] >= 1 and full[2] >= 1 and full[3] >= 1, full
    now, _ = profiled_slots(case, t, (False, True))
    assert now[1] == full[1] and now[2] == 0 and now[3] == full[3], now     # no GEMM-2
    noi, _ = profiled_slots(case, t, (True, False))
    assert noi[1] == full[1] and noi[2] == full[2] and noi[3] == 0, noi     # no gather
    both, _ = profiled_slots(case, t, (True, True))
    assert both[1] == full[1] and both[2] == 0 and both[3] == 0, both


def test_weights_ready_event_after_a_call_without_weight_gradients():
    from modulated_deform_conv_amd import _capi
    case = CASE_BY_NAME["mfma_mdcn2d_c32_o48_9x10"]
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    producer, waiter = torch.cuda.Stream(), torch.cuda.Stream()
    producer.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(producer):
        backward(case, t, (False, True))
    _capi.stream_wait_weight_ready(waiter, producer)   # succeeds: the event of THIS backward, recorded before its kernels
    _capi.stream_wait_weight_ready(waiter)
    torch.cuda.synchronize()


WORKSPACE_CASES = [("fp32", CASE_BY_NAME["mfma_mdcn2d_c32_o48_9x10"], torch.float32),
                   ("fp32_padded", CASE_BY_NAME["mfma_pad_mdcn2d_dg4_c96_o64"], torch.float32),
                   ("fp16", CASE_BY_HP["hp_mdcn2d_c256_o256_g32_dg4"], torch.float16)]


@pytest.mark.parametrize("which, case, dtype", WORKSPACE_CASES, ids=[w[0] for w in WORKSPACE_CASES])
def test_nothing_is_written_outside_the_smaller_workspace(which, case, dtype, monkeypatch):
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    from modulated_deform_conv_amd import _capi
    t = make_inputs(case, dtype=dtype, device="cuda")
    touched, calls = [], []
    with _capi.deterministic():
        full = backward(case, t)
        monkeypatch.setattr(M, "_run", guarded_run(touched, calls))
        backward(case, t)
        for skip in FLAG_SETS:
            got = backward(case, t, skip)
            for key in _requested(skip):
                if full[key] is not None:
                    assert torch.equal(got[key], full[key]), (skip, key)
    assert not touched, touched
    sizes = [b for _, b in calls]
    assert len(sizes) == 4 and all(0 < b <= sizes[0] for b in sizes[1:]), sizes
    assert sizes[3] < sizes[0], sizes


# ---- child processes: the switches are read once per process -------------------------------------------------------------
BWD3_CODE = r"""
import sys
sys.path.insert(0, %r)
import torch
from tests.cases import make_inputs
from tests.test_gpu_hp import CASE_BY_HP
from tests.test_gpu_selective_backward import KEYS, _fp32_sampling, _requested, backward, profiled_slots
from modulated_deform_conv_amd import _capi
dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[sys.argv[1]]
names = ["hp_mdcn2d_c32_o32", "hp_mdcn2d_c256_o256", "hp_mdcn2d_c64_dg4_o64", "hp_dcn3d_c64_o32_s2", "hp_mdcn2d_c96_o64_wpad",
         "hp_mdcn2d_c96_dg4_o96_pad", "hp_mdcn2d_c32_o32+s32", "hp_dcn3d_c64_o32_s2+s32"]
for name in names:
    case = CASE_BY_HP[name.split("+")[0]]
    t = make_inputs(case, dtype=dtype, device="cuda")
    if name.endswith("+s32"):
        t = _fp32_sampling(t)
    with _capi.deterministic():
        full = backward(case, t)
        assert _capi.last_kernels() == "hp", (name, _capi.last_kernels())
        for skip in ((False, True), (True, True)):
            got = backward(case, t, skip)
            for key in _requested(skip):
                if full[key] is not None:
                    assert torch.equal(got[key], full[key]), (name, skip, key, (got[key].float() - full[key].float()).abs().max().item())
            slots, kernels = profiled_slots(case, t, skip)
            assert "hp_bwd3_kernel" in kernels and "hp_gemm2_kernel" not in kernels, (name, skip, kernels)
            assert slots[2] == 0 and (slots[3] == 0) == skip[0], (name, skip, slots)
        # without grad_input alone: the full kernel, GEMM-2 and the reduce run; the list build and the gather do not
        got = backward(case, t, (True, False))
        for key in ("grad_offset", "grad_mask", "grad_weight", "grad_bias"):
            if full[key] is not None:
                assert torch.equal(got[key], full[key]), (name, "no_input", key)
        slots, kernels = profiled_slots(case, t, (True, False))
        assert "hp_gemm2_kernel" in kernels and slots[3] == 0, (name, slots, kernels)
        slots, kernels = profiled_slots(case, t, (False, False))
        assert {"hp_bwd3_kernel", "hp_gemm2_kernel"} <= kernels and slots[2] >= 1 and slots[3] >= 1, (name, slots, kernels)
print("SELECTIVE_BWD3_OK")
"""


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_hp_bwd3_variant_without_column_rows(dtype):
    """MDCONV_HP_BWD=4 keeps hp_bwd3 wherever it is supported: the variant without column rows on a staged slab, with A
    fragments from global memory (16 k-steps), with deformable groups, in 3-D without a mask, width-padded, group-padded
    and with fp32 sampling -- its grad_offset / grad_mask / grad_col rows (through grad_input) bit-identical to the full
    kernel's."""
    env = dict(os.environ, MDCONV_HP_BWD="4")
    r = subprocess.run([sys.executable, "-c", BWD3_CODE % ROOT, dtype], env=env, capture_output=True, text=True, timeout=600)
    assert "SELECTIVE_BWD3_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


CHUNK_CODE = r"""
import sys
sys.path.insert(0, %r)
import torch
from tests.cases import _c, make_inputs, M2
from tests.test_gpu_selective_backward import FLAG_SETS, _requested, backward
from modulated_deform_conv_amd import _capi
case = _c("chunk_mdcn2d_c64_o64", M2, 20, 64, 64, (24, 20), 3, seed=141)   # chunks of 9, 9, 2 images
t = make_inputs(case, dtype=torch.float16, device="cuda")
with _capi.deterministic():
    full = backward(case, t)
    assert _capi.last_kernels() == "hp", _capi.last_kernels()
    for skip in FLAG_SETS:
        got = backward(case, t, skip)
        for key in _requested(skip):
            assert torch.equal(got[key], full[key]), (skip, key)
print("SELECTIVE_CHUNK_OK")
"""


def test_batch_chunk_loop():
    env = dict(os.environ, MDCONV_CHUNK_LIMIT_BYTES="600000")
    r = subprocess.run([sys.executable, "-c", CHUNK_CODE % ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert "SELECTIVE_CHUNK_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- Python layers -------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _torch_deterministic():
    prev, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=warn)


def _module_grads(mod, t, trainable):
    """.grad of (input, offset, mask, weight, bias) after one forward + backward with only ``trainable`` requiring grad."""
    leaves = {n: t[n].clone().requires_grad_(n in trainable) for n in ("input", "offset", "mask") if t[n] is not None}
    mod.weight.requires_grad_("weight" in trainable)
    mod.weight.grad = None
    if mod.bias is not None:
        mod.bias.requires_grad_("weight" in trainable)
        mod.bias.grad = None
    out = mod(*[leaves[n] for n in ("input", "offset", "mask") if n in leaves])
    out.backward(t["grad_output"])
    torch.cuda.synchronize()
    g = {n: v.grad for n, v in leaves.items()}
    g["weight"], g["bias"] = mod.weight.grad, None if mod.bias is None else mod.bias.grad
    return g


@pytest.mark.parametrize("name", ["mfma_mdcn2d_c32_o48_9x10", "mfma_dcn3d_c16_o16_5x6x5"])
def test_modules_skip_what_autograd_does_not_ask_for(name, monkeypatch):
    import modulated_deform_conv_amd.modulated_deform_conv as pkg
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    from modulated_deform_conv_amd import _capi
    case = CASE_BY_NAME[name]
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    cls = pkg.ModulatedDeformConv2d if case["op"] == M2 else pkg.DeformConv3d
    mod = cls(case["C"], case["O"], case["k"], padding=case["padding"], bias=case["bias"]).cuda()
    with torch.no_grad():
        mod.weight.copy_(t["weight"])
        if case["bias"]:
            mod.bias.copy_(t["bias"])
    flags = []
    orig = M._run
    monkeypatch.setattr(M, "_run", lambda fn, d, backward, *a: (flags.append(d.flags) if backward else None, orig(fn, d, backward, *a))[1])
    every = ("input", "offset", "mask", "weight")
    det = _capi.FLAG_DETERMINISTIC
    with _torch_deterministic():
        full = _module_grads(mod, t, every)
        frozen = _module_grads(mod, t, ("input", "offset", "mask"))
        no_input = _module_grads(mod, t, ("offset", "mask", "weight"))
        only_weight = _module_grads(mod, t, ("weight",))   # offsets and masks are always computed: nothing to skip
    assert flags == [det, det | _capi.FLAG_NO_GRAD_WEIGHT, det | _capi.FLAG_NO_GRAD_INPUT, det | _capi.FLAG_NO_GRAD_INPUT], flags
    assert frozen["weight"] is None and frozen["bias"] is None
    assert no_input["input"] is None
    for n in ("input", "offset", "mask"):
        if full.get(n) is not None:
            assert torch.equal(frozen[n], full[n]), n
    for n in ("offset", "mask", "weight", "bias"):
        if full.get(n) is not None:
            assert torch.equal(no_input[n], full[n]), n
    assert torch.equal(only_weight["weight"], full["weight"])


def _op_conf(case):
    nd = ndim(case)
    lst = lambda v: [v] * nd if isinstance(v, int) else list(v)
    return dict(stride=lst(case["stride"]), padding=lst(case["padding"]), dilation=lst(case["dilation"]), groups=case["groups"],
                deformable_groups=case["dgroups"], in_step=case["in_step"])


def test_operator_autograd_with_frozen_weights():
    import modulated_deform_conv_amd.ops as ops
    case = CASE_BY_NAME["mfma_mdcn2d_c32_o48_9x10"]
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    conf = _op_conf(case)

    def grads(trainable):
        leaves = {n: t[n].clone().requires_grad_(n in trainable) for n in ("input", "offset", "mask", "weight", "bias")}
        out = ops.deform_conv(leaves["input"], leaves["offset"], leaves["mask"], leaves["weight"], leaves["bias"], **conf)
        out.backward(t["grad_output"])
        torch.cuda.synchronize()
        return {n: v.grad for n, v in leaves.items()}
    with _torch_deterministic():
        full = grads(("input", "offset", "mask", "weight", "bias"))
        frozen = grads(("input", "offset", "mask"))
        bias_only = grads(("offset", "bias"))
    assert frozen["weight"] is None and frozen["bias"] is None
    for n in ("input", "offset", "mask"):
        assert torch.equal(frozen[n], full[n]), n
    assert bias_only["input"] is None and bias_only["weight"] is None
    assert torch.equal(bias_only["bias"], full["bias"]) and torch.equal(bias_only["offset"], full["offset"])


@pytest.mark.parametrize("need_input, need_weight", [(False, True), (True, False), (False, False)])
def test_masked_operator(need_input, need_weight):
    import modulated_deform_conv_amd.ops as ops
    case = CASE_BY_NAME["mfma_dcn3d_c16_o16_5x6x5"]
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    conf = _op_conf(case)
    args = (t["grad_output"], t["input"], t["offset"], None, t["weight"], None)
    with _torch_deterministic():
        full = ops.deform_conv_backward(*args, **conf)
        got = ops.deform_conv_backward_masked(*args, **conf, need_input=need_input, need_weight=need_weight)
    torch.cuda.synchronize()
    for key, a, b in zip(KEYS, got, full):
        if (key == "grad_input" and not need_input) or (key in ("grad_weight", "grad_bias") and not need_weight):
            assert a.numel() == 0, key
        else:
            assert torch.equal(a, b), key
    torch.library.opcheck(ops.deform_conv_backward_masked, args, dict(conf, need_input=need_input, need_weight=need_weight),
                          test_utils=("test_schema", "test_faketensor"))


def test_torch_compile_of_a_frozen_weight_layer():
    import modulated_deform_conv_amd.ops as ops
    case = CASE_BY_NAME["mdcn2d_basic"]
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    conf = _op_conf(case)
    w, b = t["weight"], t["bias"]   # frozen: no gradient asked for

    def step(x, off, m):
        y = ops.deform_conv(x, off, torch.sigmoid(m), w, b, **conf)
        return torch.relu(y).sum()

    leaves = [t[n].clone().requires_grad_(True) for n in ("input", "offset", "mask")]
    eager = step(*leaves)
    g_eager = torch.autograd.grad(eager, leaves)
    compiled = torch.compile(step, backend="aot_eager", fullgraph=True)
    out = compiled(*leaves)
    g = torch.autograd.grad(out, leaves)
    assert_close("loss", out.reshape(1), eager.reshape(1), 1e-6)
    for a, b_, n in zip(g, g_eager, ("input", "offset", "mask")):
        assert_close("grad_" + n, a, b_, 1e-6)
