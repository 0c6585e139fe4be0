"""fp32 weight gradients on the GPU (include/mdconv.h: MDCONV_WGRAD_F32): fp16 / bf16 tensors whose backward hands
grad_weight and grad_bias back as the fp32 sums it holds.  Parity with the oracle run in fp64 on exact upcasts of the
16-bit inputs, on every route and kernel of the 16-bit backward; the relation to the plain call (the mode removes the final
rounding and nothing else); the cases that show the point (no fp16 overflow, fp32 accumulation over calls); the modules'
`weight_grad_dtype`; the data-parallel exchange."""
import os
import subprocess
import sys

import pytest
import torch

from tests.cases import M2, _c, make_inputs
from tests.test_gpu_sampling_dtype import PARITY_CASES
from tests.util import assert_close, rel_err, run_oracle, run_product_into

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL = {torch.float16: 5e-3, torch.bfloat16: 3e-2}   # as tests/test_gpu_hp.py
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
DIRECT_CASE = _c("w32_mdcn2d_c32_direct", M2, 2, 32, 16, (8, 9), 3, dgroups=2, seed=211)
CASES = [(c, "auto") for c in PARITY_CASES] + [(DIRECT_CASE, "direct")]
NATIVE = PARITY_CASES[0]      # 64 -> 64, (9, 10): native 16-bit kernels, tap-stationary backward
F32ROUTE = PARITY_CASES[8]    # 512 -> 64: backward on the fp32 matrix kernels through fp32 copies


def _inputs(case, dtype, scale=1.0):
    """Every tensor 16-bit (generated in fp64 by make_inputs, then rounded once)."""
    t = make_inputs(case, dtype=torch.float64, device="cuda")
    t["grad_output"] = t["grad_output"] * scale
    return {k: (None if v is None else v.to(dtype)) for k, v in t.items()}


_ORACLE = {}


def _oracle(case, t, key):
    """fp64 oracle on exact upcasts of the 16-bit tensors; computed once per (case, dtype, variant)."""
    if key not in _ORACLE:
        _ORACLE[key] = run_oracle(case, {k: (None if v is None else v.double()) for k, v in t.items()}, torch.float64)
    return _ORACLE[key]


def _run(case, t, wdtype, accumulate=False, prefill=None, path="auto", det=False):
    """One forward + backward into caller-allocated tensors; grad_weight / grad_bias of dtype `wdtype` (fp32: the mode).
    -> (grads, kernel family of the backward)"""
    from modulated_deform_conv_amd import _capi
    dtype = t["input"].dtype
    out = torch.empty_like(t["grad_output"])
    new = torch.zeros_like if accumulate else torch.empty_like
    grads = dict(grad_input=new(t["input"]), grad_offset=new(t["offset"]),
                 grad_mask=None if t["mask"] is None else new(t["mask"]),
                 grad_weight=new(t["weight"], dtype=wdtype),
                 grad_bias=new(t["bias"], dtype=wdtype) if case["bias"] else None)
    for k, v in (prefill or {}).items():
        grads[k].copy_(v)
    with _capi.deterministic(det):
        run_product_into(case, t, out, grads, accumulate=accumulate, path=path)
    torch.cuda.synchronize()
    assert out.dtype == dtype
    return grads, _capi.last_kernels()


def _check_parity(case, dtype, path):
    t = _inputs(case, dtype)
    # the data gradients of the matrix-core kernels are bit-reproducible in deterministic mode (grad_input sums its lists
    # in arrival order otherwise); the shape-generic kernels add with floating-point atomics and refuse it
    det = path != "direct" and "o8" not in case["name"]
    g16, fam16 = _run(case, t, dtype, path=path, det=det)
    g32, fam32 = _run(case, t, torch.float32, path=path, det=det)
    assert fam32 == fam16, (fam16, fam32)                              # the bit does not change the route
    _, want = _oracle(case, t, (case["name"], dtype))
    tol = TOL[dtype]
    for k in ("grad_weight", "grad_bias"):
        if g32[k] is None:
            continue
        assert g32[k].dtype == torch.float32 and g16[k].dtype == dtype, k
        assert_close(k, g32[k], want[k], tol)
        if fam32 in ("hp", "f32"):
            # the rounding relation: those sums are reproducible from run to run, and the mode removes only the final rounding
            assert torch.equal(g32[k].to(dtype), g16[k]), "%s: fp32 result rounded != 16-bit result (max diff %g)" % (
                k, (g32[k].to(dtype).float() - g16[k].float()).abs().max().item())
    for k in ("grad_input", "grad_offset", "grad_mask"):
        if g32[k] is None:
            continue
        assert g32[k].dtype == dtype, k
        assert_close(k, g32[k].float(), want[k], tol)
        if det:
            assert torch.equal(g32[k], g16[k]), k                      # every other gradient: the same bits
    return fam32


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case, path", CASES, ids=lambda v: v["name"] if isinstance(v, dict) else v)
def test_parity(case, path, dtype):
    fam = _check_parity(case, dtype, path)
    if path == "direct":
        assert fam == "direct"
    elif "route" in case["name"]:
        assert fam == "f32"
    elif "o8" not in case["name"]:
        assert fam == "hp"


def test_parity_with_the_pixel_stationary_backward_forced():
    """MDCONV_HP_BWD=4 keeps hp_bwd3 + hp_gemm2 wherever they are supported (read once per process: a child); the native
    shapes only."""
    env = dict(os.environ, MDCONV_HP_BWD="4")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
                        "test_parity and not forced and not direct and not f32route and not dg8 and not o8"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


def _overflow_scale(case, dtype):
    """The power of two for grad_output, chosen on the CPU with the oracle: no |grad_output| above 2^15, and at least 1 % of
    the oracle's grad_weight elements above the fp16 maximum."""
    t = _inputs(case, dtype)
    _, want = _oracle(case, t, (case["name"], dtype))
    go_max = t["grad_output"].abs().max().item()
    for p in range(0, 24):
        s = 2.0 ** p
        if go_max * s > 2 ** 15:
            break
        if (want["grad_weight"].abs() * s > 65504).double().mean().item() >= 0.01:
            return s
    raise AssertionError("no power of two overflows grad_weight while grad_output stays below 2^15")


# 64 -> 64, (9, 10) with eight images: with the two images of the parity shape no power of two that keeps |grad_output| below
# 2^15 lifts 1 % of grad_weight over the fp16 maximum (2^12: 0.07 %; eight images: 6.6 %)
OVERFLOW_CASE = _c("w32_overflow_mdcn2d_c64_o64_b8", M2, 8, 64, 64, (9, 10), 3, seed=231)


def test_no_fp16_overflow():
    """The point.  A weight gradient sums B x S_o samples: with loss scaling it passes 65504 long before any grad_output
    element does.  The plain call returns inf; the fp32 sum was finite all along."""
    case, dtype = OVERFLOW_CASE, torch.float16
    s = _overflow_scale(case, dtype)
    t = _inputs(case, dtype, scale=s)
    assert t["grad_output"].abs().max().item() <= 2 ** 15 and torch.isfinite(t["grad_output"]).all()
    _, want = _oracle(case, t, (case["name"], dtype, s))
    assert (want["grad_weight"].abs() > 65504).double().mean().item() >= 0.01
    g16, fam = _run(case, t, dtype)
    assert fam == "hp"
    assert not torch.isfinite(g16["grad_weight"]).all()               # (so the case cannot go stale)
    g32, fam = _run(case, t, torch.float32)
    assert fam == "hp"
    assert torch.isfinite(g32["grad_weight"]).all() and torch.isfinite(g32["grad_bias"]).all()
    assert_close("grad_weight", g32["grad_weight"], want["grad_weight"], TOL[dtype])
    assert_close("grad_bias", g32["grad_bias"], want["grad_bias"], TOL[dtype])


def _prefill(shape, seed):
    """fp32 values of magnitude in [256, 512) that carry low mantissa bits: not representable in 16 bits."""
    g = torch.Generator().manual_seed(seed)
    p = (256 + 256 * torch.rand(shape, generator=g, dtype=torch.float64)).float()
    p = torch.where(p >= 512, torch.full_like(p, 511.99997), p)
    p = (p.view(torch.int32) | 1).view(torch.float32)                 # the last mantissa bit set
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return (p * sign).cuda()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [NATIVE, F32ROUTE], ids=["native", "f32route"])
def test_accumulate_mode_keeps_fp32(case, dtype):
    """grad = grad + sum in fp32: one fp32 add at magnitude < 512 errs by at most 2^-24 x 512 = 3e-5; a 16-bit round trip
    of the buffer's values errs by ~0.1 (fp16) / ~1 (bf16)."""
    t = _inputs(case, dtype)
    over, fam = _run(case, t, torch.float32)
    assert fam == ("hp" if case is NATIVE else "f32")
    pre = dict(grad_weight=_prefill(t["weight"].shape, 31), grad_bias=_prefill(t["bias"].shape, 32))
    assert not torch.equal(pre["grad_weight"].to(dtype).float(), pre["grad_weight"])
    acc, fam2 = _run(case, t, torch.float32, accumulate=True, prefill=pre)
    assert fam2 == fam
    for k in ("grad_weight", "grad_bias"):
        assert acc[k].dtype == torch.float32
        e = rel_err(acc[k].double() - pre[k].double(), over[k])
        print("%s %s %s: rel_err((accumulated - prefill), overwrite) = %.3e" % (case["name"], dtype, k, e))
        assert e <= 1e-4, (k, e)


MICRO_CASE = _c("w32_micro_mdcn2d_c64_o64_b4", M2, 4, 64, 64, (9, 10), 3, seed=221)


def _micro_batches(dtype, wdtype):
    """-> (grad_weight of one B = 4 call, grad_weight of two accumulate calls of two images into one zeroed buffer)"""
    case = MICRO_CASE
    t = _inputs(case, dtype)
    whole, _ = _run(case, t, wdtype)
    half = dict(case, B=2)
    acc = None
    for lo in (0, 2):
        th = {k: (v if v is None or k in ("weight", "bias") else v[lo:lo + 2].contiguous()) for k, v in t.items()}
        acc, _ = _run(half, th, wdtype, accumulate=True,
                      prefill=None if acc is None else dict(grad_weight=acc["grad_weight"], grad_bias=acc["grad_bias"]))
    return t, whole["grad_weight"], acc["grad_weight"]


def test_two_micro_batches_equal_one_batch():
    dtype = torch.float16
    t, whole32, acc32 = _micro_batches(dtype, torch.float32)
    _, whole16, acc16 = _micro_batches(dtype, dtype)
    _, want = _oracle(MICRO_CASE, t, (MICRO_CASE["name"], dtype))
    assert acc32.dtype == whole32.dtype == torch.float32
    assert_close("grad_weight (one batch)", whole32, want["grad_weight"], TOL[dtype])
    assert_close("grad_weight (two micro-batches)", acc32, want["grad_weight"], TOL[dtype])
    d32, d16 = rel_err(acc32, whole32), rel_err(acc16.float(), whole16.float())
    print("two micro-batches vs one batch, scaled max difference: fp32 weight gradients %.3e, plain fp16 %.3e" % (d32, d16))
    assert d32 < d16, (d32, d16)


def test_deterministic_mode():
    from modulated_deform_conv_amd import _capi
    t = _inputs(NATIVE, torch.bfloat16)
    a, fam = _run(NATIVE, t, torch.float32, det=True)
    b, _ = _run(NATIVE, t, torch.float32, det=True)
    assert fam == "hp" and _capi.deterministic_override() is None
    for k in a:
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), k
    assert a["grad_weight"].dtype == torch.float32


def test_a_mixed_pair_is_refused():
    t = _inputs(NATIVE, torch.float16)
    out = torch.empty_like(t["grad_output"])
    for wdt, bdt in ((torch.float32, torch.float16), (torch.float16, torch.float32)):
        grads = dict(grad_input=torch.empty_like(t["input"]), grad_offset=torch.empty_like(t["offset"]),
                     grad_mask=torch.empty_like(t["mask"]), grad_weight=torch.empty_like(t["weight"], dtype=wdt),
                     grad_bias=torch.empty_like(t["bias"], dtype=bdt))
        with pytest.raises(RuntimeError, match="fp32"):
            run_product_into(NATIVE, t, out, grads, accumulate=False)


def test_the_allocating_export_follows_the_context_manager():
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    from modulated_deform_conv_amd import _capi
    from modulated_deform_conv_amd.distributed import fused_view
    t = _inputs(NATIVE, torch.float16)
    geo = (3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 64, True)
    args = (t["input"], t["weight"], t["bias"], t["offset"], t["mask"], t["grad_output"]) + geo
    plain = M.modulated_deform_conv2d_backward_cuda(*args)
    with _capi.weight_grads_f32():
        wide = M.modulated_deform_conv2d_backward_cuda(*args)
    torch.cuda.synchronize()
    assert plain[3].dtype == plain[4].dtype == torch.float16
    assert wide[3].dtype == wide[4].dtype == torch.float32 and fused_view(wide[3], wide[4]) is not None
    assert [g.dtype for g in wide[:3]] == [torch.float16] * 3
    assert torch.equal(wide[3].half(), plain[3]) and torch.equal(wide[4].half(), plain[4])
    ref, _ = _run(NATIVE, t, torch.float32)
    assert torch.equal(wide[3], ref["grad_weight"]) and torch.equal(wide[4], ref["grad_bias"])


CHUNK_CODE = r"""
import sys
sys.path.insert(0, %r)
import torch
from tests.cases import _c, M2
from tests.test_gpu_wgrad32 import _inputs, _oracle, _run
from tests.util import assert_close
case = _c("w32_chunk_mdcn2d_c64_o64", M2, 20, 64, 64, (24, 20), 3, seed=212)
for dtype, tol in ((torch.float16, 5e-3), (torch.bfloat16, 3e-2)):
    t = _inputs(case, dtype)
    g16, fam16 = _run(case, t, dtype)
    g32, fam32 = _run(case, t, torch.float32)
    assert fam16 == fam32 == "hp", (fam16, fam32)
    _, w = _oracle(case, t, (case["name"], dtype))
    for k in g32:
        if w[k] is not None:
            assert_close(k, g32[k].float(), w[k], tol)
    for k in ("grad_weight", "grad_bias"):
        assert g32[k].dtype == torch.float32
        assert torch.equal(g32[k].to(dtype), g16[k]), k
print("W32_CHUNK_OK")
"""


def test_batch_chunks():
    """Uneven batch chunks (9 + 9 + 2 images): the running fp32 sum over the chunks is what the caller receives."""
    env = dict(os.environ, MDCONV_CHUNK_LIMIT_BYTES="600000")
    r = subprocess.run([sys.executable, "-c", CHUNK_CODE % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert "W32_CHUNK_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.fixture
def descs(monkeypatch):
    """(entry point, dtype word of the descriptor) of every library call."""
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    seen, orig = [], M._run

    def rec(fn_name, d, backward, args, input):
        orig(fn_name, d, backward, args, input)
        seen.append((fn_name, d.dtype))

    monkeypatch.setattr(M, "_run", rec)
    return seen


def _module_step(mod, t, dtype):
    x, off, m = (t[k].clone().requires_grad_() for k in ("input", "offset", "mask"))
    with torch.autocast("cuda", dtype=dtype):
        out = mod(x, off, m)
    out.backward(t["grad_output"].to(dtype))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_module_with_fp32_master_weights_under_autocast(dtype, descs):
    from modulated_deform_conv_amd import _capi
    from modulated_deform_conv_amd.modulated_deform_conv import ModulatedDeformConv2d
    t = make_inputs(NATIVE, dtype=torch.float32, device="cuda")
    mods = [ModulatedDeformConv2d(64, 64, 3, padding=1, bias=True, **kw).cuda()
            for kw in (dict(weight_grad_dtype=torch.float32), dict())]
    for mod in mods:
        with torch.no_grad():
            mod.weight.copy_(t["weight"]); mod.bias.copy_(t["bias"])
        _module_step(mod, t, dtype)
        assert mod.weight.grad.dtype == mod.bias.grad.dtype == torch.float32
    base = _capi.F16 if dtype == torch.float16 else _capi.BF16
    assert [d for _, d in descs] == [base, base | _capi.WGRAD_F32, base, base], descs   # forward, backward; forward, backward
    wide, plain = mods
    # the export's results for the same 16-bit tensors: fp32 with the mode, rounded without
    t16 = {k: (None if v is None else v.to(dtype)) for k, v in t.items()}
    ref32, _ = _run(NATIVE, t16, torch.float32)
    ref16, _ = _run(NATIVE, t16, dtype)
    assert torch.equal(wide.weight.grad, ref32["grad_weight"]) and torch.equal(wide.bias.grad, ref32["grad_bias"])
    assert torch.equal(plain.weight.grad, ref16["grad_weight"].float()) and torch.equal(plain.bias.grad, ref16["grad_bias"].float())
    assert not torch.equal(wide.weight.grad, plain.weight.grad)
    assert _capi.weight_grads_f32_mode() is False


def test_module_with_fp32_sampling_and_fp32_weight_gradients(descs):
    from modulated_deform_conv_amd import _capi
    from modulated_deform_conv_amd.modulated_deform_conv import ModulatedDeformConv2d
    t = make_inputs(NATIVE, dtype=torch.float32, device="cuda")
    mod = ModulatedDeformConv2d(64, 64, 3, padding=1, bias=True, sampling_dtype=torch.float32,
                                weight_grad_dtype=torch.float32).cuda()
    with torch.no_grad():
        mod.weight.copy_(t["weight"]); mod.bias.copy_(t["bias"])
    out = _module_step(mod, t, torch.bfloat16)
    assert out.dtype == torch.bfloat16
    both = _capi.BF16 | _capi.SAMPLING_F32 | _capi.WGRAD_F32
    assert [d for _, d in descs] == [_capi.BF16 | _capi.SAMPLING_F32, both], descs
    assert mod.weight.grad.dtype == mod.bias.grad.dtype == torch.float32
    r = lambda k, v: v if k in ("offset", "mask") else v.to(torch.bfloat16)
    _, want = run_oracle(NATIVE, {k: (None if v is None else r(k, v).double()) for k, v in t.items()}, torch.float64)
    assert_close("grad_weight", mod.weight.grad, want["grad_weight"], TOL[torch.bfloat16])
    assert_close("grad_bias", mod.bias.grad, want["grad_bias"], TOL[torch.bfloat16])


def test_16bit_parameters_keep_their_gradient_dtype(descs):
    """autograd wants the gradient in the parameter's dtype: with 16-bit parameters the mode has no effect."""
    from modulated_deform_conv_amd import _capi
    from modulated_deform_conv_amd.modulated_deform_conv import ModulatedDeformConv2d
    t = make_inputs(NATIVE, dtype=torch.float16, device="cuda")
    mod = ModulatedDeformConv2d(64, 64, 3, padding=1, bias=True, weight_grad_dtype=torch.float32).cuda().half()
    out = mod(t["input"], t["offset"], t["mask"])
    out.backward(t["grad_output"])
    assert mod.weight.grad.dtype == torch.float16 and [d for _, d in descs] == [_capi.F16, _capi.F16]


def test_deform_conv3d_pack_smoke(descs):
    from modulated_deform_conv_amd import _capi
    from modulated_deform_conv_amd.modulated_deform_conv import DeformConv3dPack
    mod = DeformConv3dPack(32, 32, 3, padding=1, bias=True, weight_grad_dtype=torch.float32).cuda()
    x = torch.randn(2, 32, 4, 5, 6, device="cuda", requires_grad=True)
    with torch.autocast("cuda", dtype=torch.float16):
        out = mod(x)
    out.float().sum().backward()
    torch.cuda.synchronize()
    assert out.dtype == torch.float16 and descs[-1] == ("mdconv_deform_conv3d_backward", _capi.F16 | _capi.WGRAD_F32)
    assert mod.weight.grad.dtype == mod.bias.grad.dtype == torch.float32
    assert torch.isfinite(mod.weight.grad).all() and torch.isfinite(x.grad).all()
    # bias.grad of a sum loss = the number of output positions per channel, exactly (an fp32 sum of ones)
    assert torch.equal(mod.bias.grad, torch.full_like(mod.bias.grad, 2 * 4 * 5 * 6))


DIST_SCRIPT = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.getcwd())
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29923")
os.environ["NCCL_DEBUG"] = "WARN"
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
from modulated_deform_conv_amd import MDCONV_CUDA as M, _capi
from modulated_deform_conv_amd.distributed import FusedGradAllReduce, fused_view
from tests.cases import CASE_BY_NAME, make_inputs
case = CASE_BY_NAME["cfg2s_mdcn2d_c64_28x28_b4"]
t = {k: (None if v is None else v.half()) for k, v in make_inputs(case, device="cuda").items()}
geo = (3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 64, True)
args = (t["input"], t["weight"], t["bias"], t["offset"], t["mask"], t["grad_output"]) + geo
sync = FusedGradAllReduce()
plain = M.modulated_deform_conv2d_backward_cuda(*args)
sync.reduce_overlapped(plain[3], plain[4])
torch.cuda.synchronize()
assert sync.last_mode == "staged"          # 16-bit gradients: reduced through the fp32 staging buffer
sync = FusedGradAllReduce()
with _capi.weight_grads_f32():
    ref = M.modulated_deform_conv2d_backward_cuda(*args)
    torch.cuda.synchronize()
    g = M.modulated_deform_conv2d_backward_cuda(*args)
sync.reduce_overlapped(g[3], g[4])
torch.cuda.synchronize()
assert g[3].dtype == g[4].dtype == torch.float32
assert sync.last_mode == "in-place" and fused_view(g[3], g[4]) is not None and sync._flat is None
assert torch.equal(g[3], ref[3]) and torch.equal(g[4], ref[4]), "all-reduce over one rank must be the identity"
assert torch.equal(g[3].half(), plain[3])
dist.destroy_process_group()
print("W32-DIST-OK")
'''


def test_exchange_reduces_the_fp32_gradients_in_place():
    r = subprocess.run([sys.executable, "-c", DIST_SCRIPT], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert "W32-DIST-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
