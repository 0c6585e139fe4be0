"""fp32 sampling on the GPU (include/mdconv.h: MDCONV_SAMPLING_F32): fp16 / bf16 input, weight, bias and grad_output with
fp32 offset and mask.  Parity with the oracle run in fp64 on CPU copies (16-bit tensors upcast exactly, offsets / masks
as the fp32 values the kernels read), on the same kernel family as the all-16-bit call of each shape; the call modes;
the modules' `sampling_dtype`; and the case that shows the point: bf16 offsets of tens of pixels move the samples."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from tests.cases import D2, D3, M2, M3, _c, make_inputs
from tests.util import assert_close, rel_err, run_oracle, run_product

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL = {torch.float16: 5e-3, torch.bfloat16: 3e-2}   # as tests/test_gpu_hp.py
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]

PARITY_CASES = [
    _c("s32_mdcn2d_c64_o64", M2, 2, 64, 64, (9, 10), 3, seed=201),                          # hp_fwd2, tap-stationary backward
    _c("s32_dcn2d_c64_dg2_o32", D2, 2, 64, 32, (9, 9), 3, dgroups=2, seed=202, offset_scale=4.0),   # hp_fwd (32-channel groups)
    _c("s32_mdcn2d_c256_dg8_o64", M2, 2, 256, 64, (9, 8), 3, dgroups=8, seed=203),           # lane-per-pixel backward (hp_bwd)
    _c("s32_mdcn2d_c64_dg4_o64", M2, 2, 64, 64, (9, 10), 3, dgroups=4, seed=204),
    _c("s32_mdcn2d_c96_dg4_o96_pad", M2, 2, 96, 96, (9, 10), 3, dgroups=4, seed=205),        # group-padded layout
    _c("s32_mdcn2d_c128_g4_dg2_o64", M2, 2, 128, 64, (8, 9), 3, groups=4, dgroups=2, seed=206),   # conv groups
    _c("s32_dcn3d_c64_o32_s2", D3, 2, 64, 32, (5, 6, 7), 3, stride=2, seed=207),
    _c("s32_mdcn3d_c64_g2_dg2", M3, 1, 64, 64, (4, 5, 6), 3, groups=2, dgroups=2, seed=208),
    _c("s32_mdcn2d_c512_o64_f32route", M2, 1, 512, 64, (7, 6), 3, seed=209),                 # backward: fp32 matrix kernels
    _c("s32_dcn3d_c24_o8_g2", D3, 1, 24, 8, (4, 5, 4), 3, groups=2, bias=False, seed=210),   # 8 output channels
]


def _inputs(case, dtype, device="cuda"):
    """16-bit tensors, fp32 offset / mask (generated in fp64 by make_inputs, then rounded once)."""
    t = make_inputs(case, dtype=torch.float64, device=device)
    return {k: (None if v is None else v.to(torch.float32 if k in ("offset", "mask") else dtype)) for k, v in t.items()}


def _oracle(case, t):
    return run_oracle(case, {k: (None if v is None else v.double()) for k, v in t.items()}, torch.float64)


@pytest.fixture
def calls(monkeypatch):
    """(entry point, MDCONV_SAMPLING_F32 set, kernel family) of every library call."""
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    from modulated_deform_conv_amd import _capi
    seen, orig = [], M._run

    def rec(fn_name, d, backward, args, input):
        orig(fn_name, d, backward, args, input)
        seen.append((fn_name, bool(d.dtype & _capi.SAMPLING_F32), _capi.last_kernels()))

    monkeypatch.setattr(M, "_run", rec)
    return seen


def _check(case, dtype, calls, path="auto"):
    t = _inputs(case, dtype)
    run_product(case, {k: (None if v is None else v.to(dtype)) for k, v in t.items()}, path)   # all-16-bit call
    n16 = len(calls)
    out, grads, _ = run_product(case, t, path)
    torch.cuda.synchronize()
    fam16, fam32 = calls[:n16], calls[n16:]
    assert [c[1] for c in fam32] == [True] * len(fam32) and not any(c[1] for c in fam16)
    assert [c[2] for c in fam32] == [c[2] for c in fam16], (fam16, fam32)   # same kernel family
    assert out.dtype == dtype
    for k in ("grad_input", "grad_weight", "grad_bias"):
        assert grads[k] is None or grads[k].dtype == dtype, k
    for k in ("grad_offset", "grad_mask"):
        assert grads[k] is None or grads[k].dtype == torch.float32, k
    want_out, want = _oracle(case, t)
    tol = TOL[dtype]
    assert_close("output", out.float(), want_out, tol)
    for k, g in grads.items():
        if want[k] is not None:
            assert_close(k, g.float(), want[k], tol)
    return fam32


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", PARITY_CASES, ids=lambda c: c["name"])
def test_parity(case, dtype, calls):
    fams = _check(case, dtype, calls)
    if "route" in case["name"]:
        assert fams[-1][2] == "f32"
    elif "o8" not in case["name"]:
        assert [f[2] for f in fams] == ["hp", "hp"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_parity_on_the_shape_generic_path(dtype, calls):
    fams = _check(_c("s32_mdcn2d_c32_direct", M2, 2, 32, 16, (8, 9), 3, dgroups=2, seed=211), dtype, calls, "direct")
    assert [f[2] for f in fams] == ["direct", "direct"]


def test_parity_with_the_pixel_stationary_backward_forced():
    """MDCONV_HP_BWD=4 keeps hp_bwd3 wherever it is supported (read once per process: a child)."""
    env = dict(os.environ, MDCONV_HP_BWD="4")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
                        "test_parity and not forced and not direct and not f32route and not dg8"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


CHUNK_CODE = r"""
import sys
sys.path.insert(0, %r)
import torch
from tests.cases import _c, M2
from tests.test_gpu_sampling_dtype import _inputs, _oracle
from tests.util import assert_close, run_product
from modulated_deform_conv_amd import _capi
case = _c("s32_chunk_mdcn2d_c64_o64", M2, 20, 64, 64, (24, 20), 3, seed=212)
for dtype, tol in ((torch.float16, 5e-3), (torch.bfloat16, 3e-2)):
    t = _inputs(case, dtype)
    out, g, _ = run_product(case, t, "auto")
    torch.cuda.synchronize()
    assert _capi.last_kernels() == "hp", _capi.last_kernels()
    wo, w = _oracle(case, t)
    assert_close("output", out.float(), wo, tol)
    for k in g:
        if w[k] is not None:
            assert_close(k, g[k].float(), w[k], tol)
print("S32_CHUNK_OK")
"""


def test_batch_chunks():
    """Uneven batch chunks (9 + 9 + 2 images): the offset / mask pointers step by 4-byte elements."""
    env = dict(os.environ, MDCONV_CHUNK_LIMIT_BYTES="600000")
    r = subprocess.run([sys.executable, "-c", CHUNK_CODE % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert "S32_CHUNK_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_the_offsets_are_not_rounded():
    """bf16 tensors, 96 x 96, offsets uniform in +-40 px: with fp32 sampling the call is within the bf16 tolerance of the
    oracle; the all-bf16 call (offsets rounded to bf16: steps of 0.125-0.25 px there) is at least 5x further from it."""
    case = _c("s32_flow_like_mdcn2d_c32_o32", M2, 1, 32, 32, (96, 96), 3, seed=213)
    t = _inputs(case, torch.bfloat16)
    g = torch.Generator().manual_seed(213)
    t["offset"] = ((torch.rand(t["offset"].shape, generator=g, dtype=torch.float64) * 2 - 1) * 40).float().cuda()
    want_out, want = _oracle(case, t)
    out32, g32, _ = run_product(case, t, "auto")
    t16 = {k: (None if v is None else v.to(torch.bfloat16)) for k, v in t.items()}
    out16, g16, _ = run_product(case, t16, "auto")
    torch.cuda.synchronize()
    assert_close("output", out32.float(), want_out, TOL[torch.bfloat16])
    assert_close("grad_input", g32["grad_input"].float(), want["grad_input"], TOL[torch.bfloat16])
    for name, a, b, w in (("output", out32, out16, want_out), ("grad_input", g32["grad_input"], g16["grad_input"],
                                                                 want["grad_input"])):
        e32, e16 = rel_err(a.float(), w), rel_err(b.float(), w)
        assert e16 >= 5 * e32, (name, e16, e32)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("path", ["auto", "direct"])
def test_accumulate_mode_adds_to_fp32_gradients(dtype, path):
    """Caller-allocated entry point (3-D, modulated): grad_offset / grad_mask / grad_input prefilled end at prefill + gradient,
    on the native kernels and on the shape-generic ones."""
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    from modulated_deform_conv_amd import _capi
    case = _c("s32_acc_mdcn3d_c32_o32", M3, 2, 32, 32, (4, 5, 6), 3, seed=214)
    t = _inputs(case, dtype)
    gen = torch.Generator().manual_seed(7)
    pre = {k: torch.randn(t[k].shape, generator=gen).to(device="cuda", dtype=t[k].dtype)
           for k in ("input", "offset", "mask", "weight", "bias")}
    gi, goff, gm, gw, gb = (pre[k].clone() for k in ("input", "offset", "mask", "weight", "bias"))
    geo = (3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, case["groups"], 1, 64, True)
    prev = _capi.set_path(path)
    try:
        M.modulated_deform_conv3d_backward_cuda(t["input"], t["weight"], t["bias"], t["offset"], t["mask"], gi, gw, gb,
                                                goff, gm, t["grad_output"], *geo)
        torch.cuda.synchronize()
        assert _capi.last_kernels() == ("hp" if path == "auto" else "direct")
    finally:
        _capi.set_path(prev)
    _, want = _oracle(case, t)
    tol = TOL[dtype]
    for k, got in (("grad_offset", goff), ("grad_mask", gm), ("grad_input", gi), ("grad_weight", gw), ("grad_bias", gb)):
        base = k[5:]
        assert_close(k, got.double() - pre[base].double(), want[k], tol * 4 if got.dtype == dtype else tol)


def test_channels_last_input(calls):
    case = _c("s32_cl_mdcn2d_c64_o32", M2, 2, 64, 32, (9, 8), 3, seed=216)
    t = _inputs(case, torch.float16)
    t["input"] = t["input"].contiguous(memory_format=torch.channels_last)
    out, grads, _ = run_product(case, t, "auto")
    torch.cuda.synchronize()
    assert [c[2] for c in calls] == ["hp", "hp"] and all(c[1] for c in calls)
    want_out, want = _oracle(case, {k: (None if v is None else v.contiguous()) for k, v in t.items()})
    assert_close("output", out.float(), want_out, TOL[torch.float16])
    for k, g in grads.items():
        if want[k] is not None:
            assert_close(k, g.float(), want[k], TOL[torch.float16])


def test_no_call_touches_memory_outside_its_workspace(monkeypatch):
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    from modulated_deform_conv_amd import _capi
    pad, pattern, touched = 1 << 20, 0xA5, []

    def run_guarded(fn_name, d, backward, args_before_ws, input):
        L = _capi.lib()
        d.input_layout = int(not input.is_contiguous() and M._is_channels_last(input))
        ws_bytes = L.mdconv_workspace_bytes(ctypes.byref(d), int(backward))
        big = torch.full((ws_bytes + 2 * pad,), pattern, dtype=torch.uint8, device=input.device)
        rc = getattr(L, fn_name)(ctypes.byref(d), *args_before_ws, ctypes.c_void_p(big.data_ptr() + pad),
                                 ctypes.c_size_t(ws_bytes), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        for side, region in (("below", big[:pad]), ("above", big[pad + ws_bytes:])):
            if (region != pattern).any():
                touched.append((fn_name, side, ws_bytes))
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (fn_name, rc, _capi.last_error()))

    monkeypatch.setattr(M, "_run", run_guarded)
    for case in (PARITY_CASES[0], PARITY_CASES[4], PARITY_CASES[8], PARITY_CASES[9]):   # native, padded, fp32 route
        for path in ("auto", "direct"):
            run_product(case, _inputs(case, torch.bfloat16), path)
    assert not touched, touched


def test_graph_capture_and_replay():
    from modulated_deform_conv_amd.modulated_deform_conv import modulated_deform_conv2d
    case = PARITY_CASES[0]
    t = _inputs(case, torch.float16)
    leaves = {k: t[k].clone().requires_grad_() for k in ("input", "offset", "mask", "weight", "bias")}

    def step():
        for v in leaves.values():
            v.grad = None
        out = modulated_deform_conv2d(leaves["input"], leaves["offset"], leaves["mask"], leaves["weight"], leaves["bias"],
                                      1, 1, 1, 1, 1, 64)
        out.backward(t["grad_output"])
        return out

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = step().detach().clone()
        eager_g = {k: v.grad.clone() for k, v in leaves.items()}
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)
    for k, v in leaves.items():
        assert v.grad.dtype == (torch.float32 if k in ("offset", "mask") else torch.float16)
        # (the gradients' scatter sums may add in another order from one run to the next)
        assert_close(k, v.grad.double(), eager_g[k].double(), 2e-3)


def _record_entry(monkeypatch):
    """[input, weight, offset, mask] dtypes as every entry point of MDCONV_CUDA receives them (the Functions hold the entry
    points themselves, so the shared dtype check is what is wrapped)."""
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    seen, orig = [], M._check_dtypes

    def rec(d, input, offset, mask, **tensors):
        seen.append([input.dtype, tensors["weight"].dtype, offset.dtype, None if mask is None else mask.dtype])
        return orig(d, input, offset, mask, **tensors)

    monkeypatch.setattr(M, "_check_dtypes", rec)
    return seen


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_module_with_fp32_sampling_under_autocast(dtype, monkeypatch):
    from modulated_deform_conv_amd.modulated_deform_conv import ModulatedDeformConv2d
    seen = _record_entry(monkeypatch)
    case = PARITY_CASES[0]
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    mod = ModulatedDeformConv2d(64, 64, 3, padding=1, bias=True, sampling_dtype=torch.float32).cuda()
    with torch.no_grad():
        mod.weight.copy_(t["weight"]); mod.bias.copy_(t["bias"])
    x, off, m = (t[k].clone().requires_grad_() for k in ("input", "offset", "mask"))
    with torch.autocast("cuda", dtype=dtype):
        out = mod(x, off, m)
    assert out.dtype == dtype
    out.backward(t["grad_output"].to(dtype))
    assert seen == [[dtype, dtype, torch.float32, torch.float32]] * 2, seen   # forward, backward
    for v in (x, off, m, mod.weight, mod.bias):
        assert v.grad.dtype == torch.float32
    r = lambda k, v: v if k in ("offset", "mask") else v.to(dtype)
    want_out, want = _oracle(case, {k: (None if v is None else r(k, v)) for k, v in t.items()})
    tol = TOL[dtype]
    assert_close("output", out.float(), want_out, tol)
    assert_close("grad_offset", off.grad, want["grad_offset"], tol)
    assert_close("grad_mask", m.grad, want["grad_mask"], tol)
    assert_close("grad_input", x.grad, want["grad_input"], tol)


def test_default_module_still_casts_the_offsets(monkeypatch):
    from modulated_deform_conv_amd.modulated_deform_conv import ModulatedDeformConv2d
    seen = _record_entry(monkeypatch)
    t = make_inputs(PARITY_CASES[0], dtype=torch.float32, device="cuda")
    mod = ModulatedDeformConv2d(64, 64, 3, padding=1).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = mod(t["input"], t["offset"], t["mask"])
    assert out.dtype == torch.bfloat16
    assert seen == [[torch.bfloat16] * 4], seen


def test_pack_module_takes_its_offset_branch_in_fp32(monkeypatch):
    from modulated_deform_conv_amd.modulated_deform_conv import ModulatedDeformConv2dPack
    seen = _record_entry(monkeypatch)
    mod = ModulatedDeformConv2dPack(64, 64, 3, padding=1, sampling_dtype=torch.float32).cuda()
    x = torch.randn(2, 64, 9, 10, device="cuda", requires_grad=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = mod(x)
    out.float().sum().backward()
    assert out.dtype == torch.bfloat16
    assert seen == [[torch.bfloat16] * 2 + [torch.float32] * 2] * 2, seen
    assert x.grad.dtype == torch.float32 and mod.conv_offset.weight.grad.dtype == torch.float32


def test_functions_take_mixed_tensors_outside_autocast():
    import modulated_deform_conv_amd.ops as ops
    from modulated_deform_conv_amd.modulated_deform_conv import deform_conv2d
    case = _c("s32_fn_dcn2d_c32_o32", D2, 2, 32, 32, (9, 8), 3, seed=217)
    t = _inputs(case, torch.bfloat16)
    want_out, want = _oracle(case, t)
    for fn in ("function", "op"):
        leaves = {k: t[k].clone().requires_grad_() for k in ("input", "offset", "weight", "bias")}
        if fn == "function":
            out = deform_conv2d(leaves["input"], leaves["offset"], leaves["weight"], leaves["bias"], 1, 1, 1, 1, 1, 64)
        else:
            out = ops.deform_conv(leaves["input"], leaves["offset"], None, leaves["weight"], leaves["bias"], [1, 1], [1, 1],
                                  [1, 1], 1, 1, 64)
        out.backward(t["grad_output"])
        assert out.dtype == torch.bfloat16 and leaves["offset"].grad.dtype == torch.float32
        assert leaves["input"].grad.dtype == torch.bfloat16
        assert_close("output", out.float(), want_out, TOL[torch.bfloat16])
        assert_close("grad_offset", leaves["offset"].grad, want["grad_offset"], TOL[torch.bfloat16])
