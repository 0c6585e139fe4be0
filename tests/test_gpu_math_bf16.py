"""fp32 tensors, bf16 matrix math (include/mdconv.h: MDCONV_FLAG_MATH_BF16; ``_capi.fp32_math``) on the GPU: an fp32 call
whose bf16 form the native 16-bit kernels take runs on those kernels -- input, weight and grad_output rounded to bf16 as
matrix operands, everything else fp32 -- and any other flagged call runs exactly as without the flag.

Tolerances: the mode has the arithmetic of a bf16 call with fp32 sampling and fp32 weight gradients, so its parity bound
against the fp32 oracle is the bf16 bound of tests/test_gpu_hp.py (3e-2); the plumbing is pinned bit for bit against that
explicit bf16 call; unflagged fp32 calls keep the fp32 bound (1e-4)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from tests.cases import CASE_BY_NAME, M2, M3, _c, make_inputs, ndim
from tests.test_gpu_hp import CASE_BY_HP, FALLBACK_CASES, TOL
from tests.util import assert_close, guarded_run, run_oracle, run_product, run_product_into, tup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_BF16, TOL_F32 = TOL[torch.bfloat16], 1e-4

NAMES = ["hp_mdcn2d_c32_o32", "hp_dcn2d_c40_o24_ragged", "hp_mdcn2d_c64_o96_s2", "hp_mdcn2d_c128_o64_g4_dg2",
         "hp_mdcn2d_c64_dg4_o64", "hp_mdcn2d_c96_dg4_o96_pad", "hp_mdcn2d_c256_o64_dg8", "hp_mdcn2d_c64_o256",
         "hp_mdcn3d_c32_o32", "hp_dcn3d_c64_o32_s2", "hp_mdcn3d_c64_dg2_o64", "hp_mdcn2d_pixels_not_mult8"]
MATH_CASES = [CASE_BY_HP[n] for n in NAMES]
ACC_CASES = [CASE_BY_HP["hp_mdcn2d_c64_dg4_o64"], CASE_BY_HP["hp_mdcn3d_c64_dg2_o64"]]
GRADS = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")


def _capi():
    from modulated_deform_conv_amd import _capi
    return _capi


def _bf16_values(t, keys):
    """`t` with the named tensors rounded to bf16 values (still fp32)"""
    return {k: (v.bfloat16().float() if v is not None and k in keys else v) for k, v in t.items()}


_ORACLE = {}


def _parity_inputs(case):
    """(fp32 device inputs with input / weight / bias holding bf16 values, the fp32 oracle's results on them): made once per
    case and shared, never written to"""
    if case["name"] not in _ORACLE:
        t = _bf16_values(make_inputs(case, dtype=torch.float32, device="cuda"), ("input", "weight", "bias"))
        _ORACLE[case["name"]] = (t, run_oracle(case, t, torch.float32))
    return _ORACLE[case["name"]]


def _buffers(t, case, fill=None, wdtype=None):
    """Caller-allocated output and gradients shaped like `t`'s tensors: NaN-filled, or random with a `fill` generator seed"""
    def like(ref, dtype=None):
        if ref is None:
            return None
        if fill is None:
            return torch.full_like(ref, float("nan"), dtype=dtype)
        g = torch.Generator(device="cuda").manual_seed(fill + ref.numel())
        return torch.randn(ref.shape, generator=g, device="cuda", dtype=torch.float32).to(dtype or ref.dtype)
    out = torch.full_like(t["grad_output"], float("nan"))
    grads = dict(grad_input=like(t["input"]), grad_offset=like(t["offset"]), grad_mask=like(t["mask"]),
                 grad_weight=like(t["weight"], wdtype), grad_bias=like(t["bias"], wdtype) if case["bias"] else None)
    return out, grads


def _guard(monkeypatch, guarded):
    """tests.util.guarded_run in place of MDCONV_CUDA._run: returns the (touched, calls) lists, or None"""
    if not guarded:
        return None
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    touched, calls = [], []
    monkeypatch.setattr(M, "_run", guarded_run(touched, calls))
    return touched, calls


def _check_guard(guard, ncalls):
    if guard is None:
        return
    touched, calls = guard
    assert not touched, touched                                    # no margin byte changed
    # (guarded_run hands over exactly mdconv_workspace_bytes: a call that needs more fails with MDCONV_EWORKSPACE)
    assert len(calls) == ncalls and all(nbytes > 0 for _, nbytes in calls), calls


# ------------------------------------------------------------------------------------------ 1 (and 7): oracle parity
@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("case", MATH_CASES, ids=lambda c: c["name"])
def test_oracle_parity(case, guarded, monkeypatch):
    capi = _capi()
    t, (want_out, want) = _parity_inputs(case)
    guard = _guard(monkeypatch, guarded)
    with capi.fp32_math("bf16"):
        out, grads, _ = run_product(case, t, "auto")
        torch.cuda.synchronize()
        assert capi.last_kernels() == "hp"
    _check_guard(guard, 2)
    assert out.dtype == torch.float32 and all(g.dtype == torch.float32 for g in grads.values() if g is not None)
    assert_close("output", out, want_out, TOL_BF16)
    for key, g in grads.items():
        if want[key] is not None:
            assert_close(key, g, want[key], TOL_BF16)
    if guarded:
        return
    # without the mode the same call is the exact fp32 call it was: the flag is what routes
    out, grads, _ = run_product(case, t, "auto")
    torch.cuda.synchronize()
    assert capi.last_kernels() != "hp"
    assert_close("output", out, want_out, TOL_F32)
    for key, g in grads.items():
        if want[key] is not None:
            assert_close(key, g, want[key], TOL_F32)


# ------------------------------------------------------------------------------------------ 2: the explicit 16-bit call
@pytest.mark.parametrize("case", MATH_CASES, ids=lambda c: c["name"])
def test_bit_for_bit_against_the_bf16_call(case):
    capi = _capi()
    t = _bf16_values(make_inputs(case, dtype=torch.float32, device="cuda"), ("input", "weight", "bias", "grad_output"))
    with capi.deterministic():
        out32, g32 = _buffers(t, case)
        with capi.fp32_math("bf16"):
            run_product_into(case, t, out32, g32, accumulate=False)
            torch.cuda.synchronize()
            assert capi.last_kernels() == "hp"
        t16 = {k: (v.bfloat16() if v is not None and k not in ("offset", "mask") else v) for k, v in t.items()}
        out16, g16 = _buffers(t16, case, wdtype=torch.float32)
        with capi.weight_grads_f32():
            run_product_into(case, t16, out16, g16, accumulate=False)
            torch.cuda.synchronize()
            assert capi.last_kernels() == "hp"
    assert out16.dtype == g16["grad_input"].dtype == torch.bfloat16
    for key in ("grad_offset", "grad_mask", "grad_weight", "grad_bias"):
        if g32[key] is not None:
            assert g32[key].dtype == g16[key].dtype == torch.float32, key
            assert torch.equal(g32[key], g16[key]), key
    assert torch.equal(out32.bfloat16(), out16)
    assert torch.equal(g32["grad_input"].bfloat16(), g16["grad_input"])


# ------------------------------------------------------------------------------------------ 3 (and 7): accumulate mode
@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("case", ACC_CASES, ids=lambda c: c["name"])
def test_accumulate_mode_adds_in_fp32(case, guarded, monkeypatch):
    capi = _capi()
    t, _ = _parity_inputs(case)
    guard = _guard(monkeypatch, guarded)
    with capi.fp32_math("bf16"):
        _, fresh = _buffers(t, case)
        out = torch.full_like(t["grad_output"], float("nan"))
        run_product_into(case, t, out, fresh, accumulate=False)
        _, pre = _buffers(t, case, fill=7)
        acc = {k: (None if v is None else v.clone()) for k, v in pre.items()}
        run_product_into(case, t, out, acc, accumulate=True)
        torch.cuda.synchronize()
        assert capi.last_kernels() == "hp"
        for key in GRADS:
            if acc[key] is not None:
                assert acc[key].dtype == torch.float32
                assert_close(key, acc[key] - pre[key], fresh[key], TOL_BF16)
        # a skipped gradient's buffer is not touched
        for skip, kept in ((dict(input=True), ("grad_input",)), (dict(weight=True), ("grad_weight", "grad_bias"))):
            acc = {k: (None if v is None else v.clone()) for k, v in pre.items()}
            with capi.skip_grads(**skip):
                run_product_into(case, t, out, acc, accumulate=True)
            torch.cuda.synchronize()
            assert capi.last_kernels() == "hp"
            for key in GRADS:
                if acc[key] is None:
                    continue
                if key in kept:
                    assert torch.equal(acc[key], pre[key]), key
                else:
                    assert_close(key, acc[key] - pre[key], fresh[key], TOL_BF16)
    _check_guard(guard, 8)


# ------------------------------------------------------------------------------------------ 4: shapes the mode does not take
def _descriptor(case, t):
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    nd = ndim(case)
    k, s, p, d = (tup(case[x], nd) for x in ("k", "stride", "padding", "dilation"))
    return M._desc(nd, case["op"] in (M2, M3), t["input"], t["weight"], k, s, p, d,
                   case["groups"], case["dgroups"], case["in_step"], case["bias"])


def _same_plan(case, t, directions):
    """used = 0 and equal workspace figures with and without the flag"""
    capi = _capi()
    L = capi.lib()
    with capi.fp32_math("fp32"):
        plain = _descriptor(case, t)
    with capi.fp32_math("bf16"):
        flagged = _descriptor(case, t)
    assert flagged.flags == plain.flags | capi.FLAG_MATH_BF16
    for backward in directions:
        assert L.mdconv_math_bf16_used(ctypes.byref(flagged), backward) == 0
        assert L.mdconv_workspace_bytes(ctypes.byref(flagged), backward) == L.mdconv_workspace_bytes(ctypes.byref(plain), backward)


WIDE_7x7 = _c("mb16_mdcn2d_c512_o512_7x7", M2, 1, 512, 512, (7, 7), 3, seed=401)


@pytest.mark.parametrize("case, det", [(CASE_BY_NAME["cfg1_dcn2d_c4_8x8_b1"], False), (FALLBACK_CASES[0], True)],
                         ids=lambda v: v["name"] if isinstance(v, dict) else "")
def test_shapes_outside_the_mode_run_as_without_the_flag(case, det):
    capi = _capi()
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    _same_plan(case, t, (0, 1))
    runs = {}
    for mode in ("fp32", "bf16"):
        with capi.deterministic(det), capi.fp32_math(mode):
            out, grads = _buffers(t, case)
            run_product_into(case, t, out, grads, accumulate=False)
            torch.cuda.synchronize()
            runs[mode] = (out, grads, capi.last_kernels())
    (out_a, g_a, fam_a), (out_b, g_b, fam_b) = runs["fp32"], runs["bf16"]
    assert fam_a == fam_b and fam_b != "hp"
    assert torch.equal(out_a, out_b)
    for key in GRADS:
        if g_a[key] is None:
            continue
        if key == "grad_input" and fam_a == "direct":   # scattered with atomics: sums in arrival order
            assert_close(key, g_b[key], g_a[key], TOL_F32)
        else:
            assert torch.equal(g_a[key], g_b[key]), key


def test_few_tile_forward_runs_as_without_the_flag():
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    capi = _capi()
    case = WIDE_7x7
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    _same_plan(case, t, (0,))
    outs, fams = [], []
    for mode in ("fp32", "bf16"):
        with capi.fp32_math(mode):
            outs.append(M.modulated_deform_conv2d_forward_cuda(t["input"], t["weight"], t["bias"], t["offset"], t["mask"],
                                                               3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 64, True))
            torch.cuda.synchronize()
            fams.append(capi.last_kernels())
    assert fams[0] == fams[1] != "hp", fams
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------ 5: Python surfaces
class _precision:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.prev = torch.get_float32_matmul_precision()
        torch.set_float32_matmul_precision(self.value)

    def __exit__(self, *exc):
        torch.set_float32_matmul_precision(self.prev)
        return False


class _torch_deterministic:
    def __enter__(self):
        self.prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
        torch.use_deterministic_algorithms(True)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.prev[0], warn_only=self.prev[1])
        return False


def _families(monkeypatch):
    """(direction, kernel family, flags word) of every call MDCONV_CUDA hands to the library, recorded on the calling thread"""
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    seen, real = [], M._run

    def spy(fn_name, d, backward, args, input):
        real(fn_name, d, backward, args, input)
        seen.append((fn_name.rsplit("_", 1)[1], _capi().last_kernels(), int(d.flags)))
    monkeypatch.setattr(M, "_run", spy)
    return seen


def _surfaces():
    """name -> (callable(leaves) -> output, parameters, inputs): the 2-D module, the 3-D module and the operator"""
    from modulated_deform_conv_amd.modulated_deform_conv import ModulatedDeformConv2d, ModulatedDeformConv3d
    import modulated_deform_conv_amd.ops  # noqa: F401  (registers mdconv::deform_conv)
    c2 = _c("mb16_mod2d", M2, 2, 64, 64, (9, 10), 3, seed=402)
    c3 = dict(CASE_BY_HP["hp_mdcn3d_c32_o32"])
    torch.manual_seed(0)
    m2 = ModulatedDeformConv2d(64, 64, 3, padding=1, bias=True).cuda()
    m3 = ModulatedDeformConv3d(32, 32, 3, padding=1, bias=True).cuda()
    with torch.no_grad():
        m2.bias.uniform_(-0.1, 0.1)
        m3.bias.uniform_(-0.1, 0.1)
    w = m2.weight.detach().clone().requires_grad_(True)
    b = m2.bias.detach().clone().requires_grad_(True)
    op = lambda x, off, m: torch.ops.mdconv.deform_conv(x, off, m, w, b, [1, 1], [1, 1], [1, 1], 1, 1, 64)
    return {"module2d": (m2, [m2.weight, m2.bias], make_inputs(c2, dtype=torch.float32, device="cuda")),
            "module3d": (m3, [m3.weight, m3.bias], make_inputs(c3, dtype=torch.float32, device="cuda")),
            "op": (op, [w, b], make_inputs(c2, dtype=torch.float32, device="cuda"))}


def _step(fn, params, t, between=None):
    """forward, `between()`, backward: [output, grad_input, grad_offset, grad_mask, parameter gradients...]"""
    lv = [t[k].clone().requires_grad_(True) for k in ("input", "offset", "mask")]
    for p in params:
        p.grad = None
    out = fn(*lv)
    if between is not None:
        between()
    out.backward(t["grad_output"])
    torch.cuda.synchronize()
    return [out.detach()] + [v.grad.clone() for v in lv] + [p.grad.clone() for p in params]


@pytest.mark.parametrize("name", ["module2d", "module3d", "op"])
def test_python_surfaces_follow_float32_matmul_precision(name, monkeypatch):
    capi = _capi()
    seen = _families(monkeypatch)
    fn, params, t = _surfaces()[name]
    with _torch_deterministic():
        with _precision("highest"):
            exact = _step(fn, params, t)
            assert seen and all(fam != "hp" and not flags & 32 for _, fam, flags in seen), seen
            del seen[:]
            with capi.fp32_math("bf16"):
                explicit = _step(fn, params, t)
            assert [d for d, _, _ in seen] == ["forward", "backward"], seen
            assert all(fam == "hp" and flags & 32 for _, fam, flags in seen), seen
        del seen[:]
        with _precision("medium"):
            medium = _step(fn, params, t)
            assert all(fam == "hp" and flags & 32 for _, fam, flags in seen) and len(seen) == 2, seen
            del seen[:]
            # the mode is recorded at forward time: a global set back before the backward does not change it
            switched = _step(fn, params, t, between=lambda: torch.set_float32_matmul_precision("highest"))
            assert all(fam == "hp" and flags & 32 for _, fam, flags in seen) and len(seen) == 2, seen
            torch.set_float32_matmul_precision("medium")   # (the step above left "highest" behind)
            with capi.fp32_math("fp32"):   # an explicit choice beats the global
                assert torch.get_float32_matmul_precision() == "medium"
                del seen[:]
                _step(fn, params, t)
                assert seen and all(fam != "hp" and not flags & 32 for _, fam, flags in seen), seen
    for got in (medium, switched):
        assert all(g.dtype == torch.float32 for g in got)
        assert all(torch.equal(a, b) for a, b in zip(got, explicit))
    assert not torch.equal(exact[0], explicit[0])                  # (bf16 operands: not the exact result)
    assert_close("output", explicit[0], exact[0], TOL_BF16)


# ------------------------------------------------------------------------------------------ 6: batch chunks
# hp_mdcn2d_pixels_not_mult8: one image's channels-last copy is 49 x 32 x 2 = 3136 bytes, its grad_col rows 9 x 49 x 32 x 2 =
# 28 224.  A limit of two copies cuts the FORWARD of B = 3 into 2 + 1; the native backward needs the limit above one image's
# grad_col rows, i.e. chunks of at least 9 images, so no limit cuts a B = 3 backward (with 6272 the bf16 backward is outside
# hp_plan and the mode leaves that direction alone).  The backward's chunks run on the same geometry with B = 10: 9 + 1.
CHUNK_SCENARIOS = {"fwd_2+1": (3, 2 * 3136, (2, None)), "bwd_9+1": (10, 28224 + 1, (2, 2))}


def _chunk_run(B, backward):
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    capi = _capi()
    case = dict(CASE_BY_HP["hp_mdcn2d_pixels_not_mult8"], B=B)
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    capi.profile_enable(True)
    capi.profile_reset()
    with capi.deterministic(), capi.fp32_math("bf16"):
        d = _descriptor(case, t)
        used = [capi.lib().mdconv_math_bf16_used(ctypes.byref(d), b) for b in (0, 1)]
        if backward:
            out, grads, _ = run_product(case, t, "auto")
        else:
            grads = {}
            out = M.modulated_deform_conv2d_forward_cuda(t["input"], t["weight"], t["bias"], t["offset"], t["mask"],
                                                         3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 64, True)
        torch.cuda.synchronize()
        assert capi.last_kernels() == "hp"
    launches = [capi.lib().mdconv_profile_read(w, ctypes.byref(ctypes.c_double(0))) for w in (0, 1)]
    capi.profile_enable(False)
    res = {k: v.cpu() for k, v in grads.items() if v is not None}
    res["output"] = out.cpu()
    return res, used, launches


def chunk_child(name, path):
    B, limit, _ = CHUNK_SCENARIOS[name]
    assert int(os.environ["MDCONV_CHUNK_LIMIT_BYTES"]) == limit
    res, used, launches = _chunk_run(B, CHUNK_SCENARIOS[name][2][1] is not None)
    torch.save(dict(res=res, used=used, launches=launches), path)
    print("MATH_BF16_CHUNKS_OK")


@pytest.mark.parametrize("name", list(CHUNK_SCENARIOS))
def test_batch_chunks_convert_per_chunk(name, tmp_path):
    B, limit, chunks = CHUNK_SCENARIOS[name]
    path = str(tmp_path / "chunked.pt")
    env = dict(os.environ, MDCONV_CHUNK_LIMIT_BYTES=str(limit))
    code = "import sys; sys.path.insert(0, %r); from tests.test_gpu_math_bf16 import chunk_child; chunk_child(%r, %r)" % (
        ROOT, name, path)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MATH_BF16_CHUNKS_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    got = torch.load(path)
    whole, used, launches = _chunk_run(B, chunks[1] is not None)
    assert used == [1, 1] and launches == [1, 1 if chunks[1] else 0], (used, launches)
    assert got["used"] == [1, 1 if chunks[1] else 0], got["used"]
    assert got["launches"][0] == chunks[0], got["launches"]          # the forward kernel ran once per chunk
    assert torch.equal(got["res"]["output"], whole["output"])
    if chunks[1] is None:
        return   # (the backward of this child is an exact fp32 call: nothing of the mode to compare)
    assert got["launches"][1] == chunks[1], got["launches"]
    for key in ("grad_input", "grad_offset", "grad_mask"):
        assert torch.equal(got["res"][key], whole[key]), key
    for key in ("grad_weight", "grad_bias"):   # partial sums split at the chunk boundary
        assert_close(key, got["res"][key], whole[key], TOL_F32)
