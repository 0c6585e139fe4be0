"""The convolution families ON the lattice: random tensors, integer sampling positions, every fast kernel family, all four
operators.  At a sampling position that is a whole pixel (d == 0) the four reference files disagree about the gradient
(``load_eps``, ``atom_eps``, ``range_gate`` of make_tap, restated per kernel family), and
tests/known_answers.py pins that on a 1-channel all-ones image, which reaches only the shape-generic kernels and cannot
tell ``v_high - v_low`` of the right pixel from that of a wrong one.  Here existing small cases of the fp32 matrix-core
kernels, the depthwise family and the native 16-bit kernels keep their ``randn`` tensors and get their offsets replaced:
all zero (a freshly initialised layer), integers in {-1, 0, 1}, or one axis integer and the others ``randn``.

Output and all five gradients against the fp32 oracle (16-bit: on the floated inputs) at the project's tolerances -- 1e-4
for fp32, ``TOL`` of tests/test_gpu_hp.py for fp16 / bf16 -- and against the shape-generic kernels.  Every test asserts
the kernel family of each library call, so a rerouted case cannot pass on the generic kernels, and that the oracle's
grad_offset is non-zero on at least a tenth of the on-lattice samples inside the image, so the case can tell the flavours
apart."""
import itertools

import pytest
import torch

from tests.cases import CASE_BY_NAME, D2, D3, M2, M3, make_inputs, ndim, out_size
from tests.test_gpu_depthwise import CASES as DW_CASES
from tests.test_gpu_hp import CASE_BY_HP, TOL as TOL16
from tests.util import assert_close, run_oracle, run_product, tup

pytestmark = pytest.mark.gpu

MODES = ("zero", "integer", "one_axis")
KEYS = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")
# the smallest case of each operator that the fp32 matrix-core kernels take (tests/cases.py)
F32_CASES = [CASE_BY_NAME[n] for n in ("mfma_dcn2d_g2_c32_o32", "mfma_mdcn2d_c32_o48_9x10", "mfma_dcn3d_c16_o16_5x6x5",
                                       "mfma_split_mdcn3d_dg2_c32_o32")]
DEPTHWISE_CASES = [DW_CASES[i] for i in (0, 2, 5, 6)]
# the smallest case of each operator of the native 16-bit kernels (tests/test_gpu_hp.py)
HP_CASES = [CASE_BY_HP[n] for n in ("hp_dcn2d_c40_o24_ragged", "hp_mdcn2d_c32_o32", "hp_dcn3d_c32_o200", "hp_mdcn3d_c32_o32")]
assert sorted(c["op"] for c in F32_CASES) == sorted(c["op"] for c in HP_CASES) == sorted([D2, M2, D3, M3])


def lattice_offsets(case, offset, mode):
    """``offset`` [B, DG * K * nd, *out] (channel = (group * K + tap) * nd + axis) with sampling positions on the lattice,
    and the mask of the elements that are.  ``one_axis``: axis tap % nd of every tap is an integer, the others keep the
    case's ``randn`` offsets."""
    nd = ndim(case)
    gen = torch.Generator().manual_seed(7000 + case["seed"])
    whole = torch.randint(-1, 2, offset.shape, generator=gen).to(offset.dtype)
    if mode == "zero":
        return torch.zeros_like(offset), torch.ones(offset.shape, dtype=torch.bool)
    if mode == "integer":
        return whole, torch.ones(offset.shape, dtype=torch.bool)
    ch = torch.arange(offset.shape[1])
    on = ((ch % nd) == ((ch // nd) % nd)).view(1, -1, *([1] * nd)).expand(offset.shape)
    return torch.where(on, whole, offset.cpu()), on


def positions(case, offset):
    """[B, DG, K, nd, *out] sampling positions in fp64: out * stride - pad + tap * dilation + offset."""
    nd = ndim(case)
    k, s, p, d = (tup(case[x], nd) for x in ("k", "stride", "padding", "dilation"))
    osz = out_size(case)
    B = offset.shape[0]
    off = offset.double().cpu().reshape(B, case["dgroups"], -1, nd, *osz)
    pos = off.clone()
    for t, tc in enumerate(itertools.product(*[range(x) for x in k])):
        for a in range(nd):
            grid = torch.arange(osz[a], dtype=torch.float64).view([-1 if i == a else 1 for i in range(nd)])
            pos[:, :, t, a] += grid * s[a] - p[a] + tc[a] * d[a]
    return pos


def _lattice_case(case, dtype, mode, sampling_dtype=None):
    """device tensors of the case with lattice offsets, and the mask [like offset] of the on-lattice coordinates of
    samples inside the image"""
    t = make_inputs(case, dtype=torch.float64, device="cpu")
    off, on = lattice_offsets(case, t["offset"], mode)
    t["offset"] = off
    sdt = sampling_dtype or dtype
    t = {k: (None if v is None else v.to(sdt if k in ("offset", "mask") else dtype).cuda()) for k, v in t.items()}
    pos = positions(case, t["offset"])
    nd = ndim(case)
    assert float((pos - pos.round()).abs().reshape(on.shape)[on].max()) == 0.0   # exact in every dtype
    size = torch.tensor(case["in_sz"], dtype=torch.float64).view(1, 1, 1, nd, *([1] * nd))
    inside = ((pos > -1) & (pos < size)).all(3, keepdim=True).expand(pos.shape).reshape(on.shape)
    return t, on & inside


@pytest.fixture
def families(monkeypatch):
    """the kernel family of every library call, in order"""
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    from modulated_deform_conv_amd import _capi
    seen, orig = [], M._run

    def rec(fn_name, d, backward, args, input):
        orig(fn_name, d, backward, args, input)
        seen.append(_capi.last_kernels())

    monkeypatch.setattr(M, "_run", rec)
    return seen


def _check(case, t, told_apart, path, families, expect, tol):
    floated = {k: (None if v is None else v.float()) for k, v in t.items()}
    want_out, want = run_oracle(case, floated, torch.float32)
    goff = want["grad_offset"].reshape(told_apart.shape)[told_apart]
    share = float((goff != 0).double().mean())
    print("%s: oracle grad_offset non-zero on %.2f of %d on-lattice elements inside" % (case["name"], share, goff.numel()))
    assert goff.numel() > 0 and share >= 0.1
    del families[:]
    out, grads, paths = run_product(case, t, path)
    torch.cuda.synchronize()
    print(case["name"], "paths", paths, "kernel families", families)
    assert len(families) == 2 and expect(families, paths), (families, paths)
    assert_close("output", out.float(), want_out, tol)
    for k in KEYS:
        if want[k] is not None:
            assert_close(k, grads[k].float(), want[k], tol)
    # ... and the shape-generic kernels
    del families[:]
    out_d, g_d, paths = run_product(case, t, "direct")
    torch.cuda.synchronize()
    assert families == ["direct", "direct"] and paths == ["direct", "direct"], (families, paths)
    assert_close("output against direct", out.float(), out_d.float().cpu(), tol)
    for k in KEYS:
        if g_d[k] is not None:
            assert_close(k + " against direct", grads[k].float(), g_d[k].float().cpu(), tol)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", F32_CASES, ids=lambda c: c["name"])
def test_lattice_fp32_matrix_core(case, mode, families):
    t, told_apart = _lattice_case(case, torch.float32, mode)
    _check(case, t, told_apart, "auto", families, lambda f, p: f == ["f32", "f32"] and p == ["mfma", "mfma"], 1e-4)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", DEPTHWISE_CASES, ids=lambda c: c["name"])
def test_lattice_depthwise(case, mode, families):
    t, told_apart = _lattice_case(case, torch.float32, mode)
    _check(case, t, told_apart, "depthwise", families,
           lambda f, p: f == ["depthwise", "depthwise"] and p == ["depthwise", "depthwise"], 1e-4)


def _native_16bit(f, p):
    """the backward on the native 16-bit kernels; the forward on them, or -- a forward of a few tiles, HpPlan::forward_preferred
    -- on the fp32 matrix-core kernels through fp32 copies: never on the shape-generic kernels"""
    return f[1] == "hp" and f[0] in ("hp", "f32")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", HP_CASES, ids=lambda c: c["name"])
def test_lattice_16bit(case, dtype, mode, families):
    t, told_apart = _lattice_case(case, dtype, mode)
    _check(case, t, told_apart, "auto", families, _native_16bit, TOL16[dtype])


@pytest.mark.parametrize("mode", MODES)
def test_lattice_16bit_with_fp32_offsets_and_masks(mode, families):
    case = CASE_BY_HP["hp_mdcn2d_c32_o32"]
    t, told_apart = _lattice_case(case, torch.bfloat16, mode, sampling_dtype=torch.float32)
    assert t["offset"].dtype == t["mask"].dtype == torch.float32 and t["input"].dtype == torch.bfloat16
    _check(case, t, told_apart, "auto", families, _native_16bit, TOL16[torch.bfloat16])
