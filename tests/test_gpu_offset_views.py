"""Tensor arguments at element-aligned addresses ("Pointer alignment").

Every other test hands the library tensors the allocator placed on 256-byte boundaries.  Here every "element"-class argument
is a dense view at an offset of 1, 2 or 4 elements inside a flat buffer (tests/offset_views.py), alone and all together, and
every result lies between two margins of 0xA5 bytes that must come back unchanged.  What is asserted, per call:
  * the path and kernel family the case is meant for (a case cannot silently run elsewhere);
  * every result against the fp64 oracle at the operator's tolerance (1e-4 fp32, 1e-2 fp16, 4e-2 bf16 and bf16 math);
  * forward outputs, and the gradients DESIGN.md's table calls bit-identical, bit for bit against the same call on
    allocator-aligned copies -- the pointer-selected variants only differ in how elements are copied or converted;
  * both margins of every result.
"16-byte"-class arguments never reach a kernel misaligned: the wrappers copy such inputs (checked by spying on the pointers
handed to the library) and refuse such result buffers with ValueError before any launch.

Which side of each pointer-selected choice a case takes (S = pixels per image):
  hp_nchw_to_nhwc (the 16-bit kernels' copy of the input, forward and backward):
      16-bit source, 8x8 (S_i = 64), C = 32: input offset 0 -> vec kernel; offset 4 elements (8 bytes) -> q4 kernel; any other
      offset -> element kernel.  C = 136 (Cp > 128): offset 0 -> q4, else element.  7x9 (S_i = 63): element kernel always.
      fp32 source (bf16 math): vec and q4 both need 16 bytes, so offset 0 -> vec (q4 for C = 136), 1 or 2 elements -> element.
  hp_bwd2 / hp_bwd3 / hp_gemm2 grad_output loads (S_o = 64): offset 0 -> buffer / 16-byte loads, else elements; 7x9: elements.
  mfma_bwd_data gout_vec (fp32, S_o = 64): grad_output offset 0 -> vector tile loads, 1 or 2 elements -> scalar; 7x9: scalar.
  hp_f32_to_bf16<VEC> (bf16 math, grad_output): offset 0 -> VEC, else the scalar variant (BF16::pack against
      bf16_operand_bits: compared bit for bit through grad_weight / grad_offset / grad_mask).
  hp_grad_bias head: grad_output offset k -> head = (8 - k) % 8 elements; the 7x9 case moves it from row to row as well.
  hp_nhwc_to_nchw (channels-last grad_output): offset 0 or 8 -> vsrc = 1, offset 1 or 2 -> vsrc = 0; S_o = 64 -> vdst = 1,
      63 -> 0.
  util_kernels word_aligned (pad_rows, pad_rows_grouped, copy_rows, unpad_rows_grouped on the caller's 16-bit tensors: the
      padded plan of the fp32 matrix family, PAD_CASES): offset 0 or 2 -> 4-byte movers, offset 1 -> halfword movers.
  widen / narrow (16-bit tensors on the fp32 matrix kernels and on the shape-generic backward): one element per access at any
      offset; the accumulating narrow next to a margin.
Not reachable from any entry point, and therefore not run here: the 16-bit compare-and-swap of mdconv_common.hpp (every 16-bit
shape-generic backward runs on fp32 copies) and the halfword side of zero_bytes (it only ever clears fp32 / fp64 tensors and
workspace)."""
import contextlib
import functools

import pytest
import torch

from tests import samp_cases as S
from tests.cases import _c, D2, D3, M2, M3, make_inputs
from tests.offset_views import at_offset
from tests.util import assert_close, run_oracle, run_product_into

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
TOL = {F32: 1e-4, F16: 1e-2, BF16: 4e-2, "f32mb": 4e-2}
INPUTS = ("input", "weight", "bias", "offset", "mask", "grad_output")
RESULTS = ("output", "grad_input", "grad_weight", "grad_bias", "grad_offset", "grad_mask")

CASES = {
    # S_i = S_o = 64: the `% 8` and `% 4` conditions hold, only the pointer decides
    "m2_c32_o32_8x8": _c("ov_m2_c32_o32_8x8", M2, 2, 32, 32, (8, 8), 3, seed=201),
    "d2_c32_o33_8x8": _c("ov_d2_c32_o33_8x8", D2, 2, 32, 33, (8, 8), 3, seed=202),
    # S = 63: the size already forces the element side
    "m2_c32_o32_7x9": _c("ov_m2_c32_o32_7x9", M2, 2, 32, 32, (7, 9), 3, seed=203),
    # Cp > 128
    "m2_c136_o32_8x8": _c("ov_m2_c136_o32_8x8", M2, 2, 136, 32, (8, 8), 3, seed=204),
    # 3-D, S = 64
    "d3_c32_o32_4x4x4": _c("ov_d3_c32_o32_4x4x4", D3, 2, 32, 32, (4, 4, 4), 3, seed=205),
    "m3_c32_o32_4x4x4": _c("ov_m3_c32_o32_4x4x4", M3, 2, 32, 32, (4, 4, 4), 3, seed=206),
}
# channels-last tensors go through the entry points that take caller-allocated results with their layouts (DCNv1)
CL_CASES = {
    "d2_c32_o32_8x8": _c("ov_cl_d2_c32_o32_8x8", D2, 2, 32, 32, (8, 8), 3, seed=208),
    "d2_c32_o32_7x9": _c("ov_cl_d2_c32_o32_7x9", D2, 2, 32, 32, (7, 9), 3, seed=209),
}
# 16-bit tensors the native kernels decline (deformable groups of 136 channels), on the fp32 matrix family as ONE padded
# problem (mfma_plans.hip, pad_plan): pad_rows / pad_rows_grouped / copy_rows / unpad_rows_grouped move the CALLER's 16-bit
# tensors and pick 4-byte or 2-byte words from the addresses (util_kernels.hip, word_aligned); every row length here is a
# multiple of 4 bytes, so only the pointer decides.  The second case pads the output channels as well (8 -> 16): bias,
# grad_output, output and grad_bias go through the movers too.
PAD_CASES = {
    "m2_c272_dg2_o32_8x8": _c("ov_pad_m2_c272_dg2_o32_8x8", M2, 2, 272, 32, (8, 8), 3, dgroups=2, seed=210),
    "m2_c272_dg2_o8_16x16": _c("ov_pad_m2_c272_dg2_o8_16x16", M2, 2, 272, 8, (16, 16), 3, dgroups=2, seed=211),
}
DEPTHWISE = _c("ov_dw_m2_c32_o32_8x8", M2, 2, 32, 32, (8, 8), 3, groups=32, seed=207)
# mode -> (tensor dtype, bf16 math, path, (path, kernels) the library must report for both directions)
MODES = {
    "f32-auto": (F32, False, "auto", ("mfma", "f32")),
    "f32-direct": (F32, False, "direct", ("direct", "direct")),
    "f16-hp": (F16, False, "mfma", ("mfma", "hp")),
    "f16-direct": (F16, False, "direct", ("direct", "direct")),
    "bf16-hp": (BF16, False, "mfma", ("mfma", "hp")),
    "bf16-direct": (BF16, False, "direct", ("direct", "direct")),
    "f32-bf16math-hp": (F32, True, "mfma", ("mfma", "hp")),
}


def _capi():
    from modulated_deform_conv_amd import _capi
    return _capi


@functools.lru_cache(maxsize=None)
def _inputs(case_name, dtype, mb16):
    """(aligned device inputs, fp64 oracle results on the values they hold): made once per (case, type), never written to."""
    case = DEPTHWISE if case_name == "depthwise" else (CASES.get(case_name) or PAD_CASES.get(case_name) or CL_CASES[case_name[3:]])
    t = make_inputs(case, dtype=dtype, device="cuda")
    if mb16:   # the operands the bf16 kernels round anyway (tests/test_gpu_math_bf16.py)
        t = {k: (v.bfloat16().float() if v is not None and k in ("input", "weight", "bias") else v) for k, v in t.items()}
    want_out, want = run_oracle(case, {k: (None if v is None else v.double()) for k, v in t.items()}, torch.float64)
    return case, t, dict(want, output=want_out)


def _offsets(t, shift=0):
    """Mixed offsets: 1, 2, 4 elements cycling over the 16-bit arguments, 1, 2 over the fp32 ones."""
    koff = {}
    for i, n in enumerate(INPUTS + RESULTS):
        ks = (1, 2, 4) if _dtype_of(n, t).itemsize == 2 else (1, 2)
        koff[n] = ks[(i + shift) % len(ks)]
    return koff


def _like(name, t):
    """The tensor a result is shaped and typed like."""
    return t[{"output": "grad_output", "grad_input": "input", "grad_weight": "weight", "grad_bias": "bias",
              "grad_offset": "offset", "grad_mask": "mask"}[name]]


def _dtype_of(name, t):
    ref = t[name] if name in INPUTS else _like(name, t)
    return (ref if ref is not None else t["input"]).dtype


@contextlib.contextmanager
def _spy_kernels(rec):
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    capi, orig = _capi(), M._run

    def run(fn_name, d, backward, args, input):
        orig(fn_name, d, backward, args, input)
        rec.append((bool(backward), capi.last_path(), capi.last_kernels(), int(d.flags)))

    M._run = run
    try:
        yield
    finally:
        M._run = orig


def _call(case, t, koff, path, expect, accumulate=False, fill=float("nan"), ctx=None):
    """Forward + backward of `case` with every tensor at element offset koff[name] (default 0) between guarded margins.
    Returns (results dict, margin checkers of the results)."""
    views, res, checks = {}, {}, {}
    for n in INPUTS:
        views[n] = None if t[n] is None else at_offset(t[n], koff.get(n, 0))[0]
    for n in RESULTS:
        ref = _like(n, t)
        if ref is None:
            res[n] = None
            continue
        res[n], checks[n] = at_offset(torch.full_like(ref, fill), koff.get(n, 0))
    grads = {k: v for k, v in res.items() if k != "output"}
    rec = []
    with _spy_kernels(rec), (ctx or contextlib.nullcontext()):
        run_product_into(case, views, res["output"], grads, accumulate=accumulate, path=path)
    torch.cuda.synchronize()
    assert [r[0] for r in rec] == [False, True], rec
    assert all(r[1:3] == expect for r in rec), (rec, expect)   # the path and the kernel family of BOTH directions
    for n, chk in checks.items():
        chk("%s %s (offsets %s)" % (case["name"], n, koff))
    return res


def _compare(tag, got, want, tol):
    for n in RESULTS:
        if got[n] is not None:
            assert_close("%s %s" % (tag, n), got[n].double(), want[n], tol)


def _bit_identical(tag, got, ctrl, kernels, dtype, mb16, koff, det=False):
    """What DESIGN.md's table promises bit for bit at any address (and no more)."""
    names = ["output"]
    if kernels != "direct":   # (the shape-generic backward sums with floating-point atomics: to rounding)
        names += ["grad_weight", "grad_offset", "grad_mask"]
        # hp_grad_bias splits a row at the 16-byte boundaries of grad_output's address: another order of the sum
        if not (kernels == "hp" and not mb16 and koff.get("grad_output", 0) % 8):
            names.append("grad_bias")
        if det:
            names.append("grad_input")
    for n in names:
        if got[n] is not None:
            assert torch.equal(got[n], ctrl[n]), "%s %s differs from the aligned call in %d elements" % (
                tag, n, int((got[n] != ctrl[n]).sum()))


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("case_name", sorted(CASES))
def test_all_arguments_at_mixed_offsets(case_name, mode):
    dtype, mb16, path, expect = MODES[mode]
    case, t, want = _inputs(case_name, dtype, mb16)
    ctx = (lambda: _capi().fp32_math("bf16")) if mb16 else (lambda: None)
    ctrl = _call(case, t, {}, path, expect, ctx=ctx())
    tol = TOL["f32mb"] if mb16 else TOL[dtype]
    _compare("%s %s aligned" % (case_name, mode), ctrl, want, tol)
    for shift in (0, 1):
        koff = _offsets(t, shift + sorted(CASES).index(case_name))
        got = _call(case, t, koff, path, expect, ctx=ctx())
        tag = "%s %s mixed%d" % (case_name, mode, shift)
        _compare(tag, got, want, tol)
        _bit_identical(tag, got, ctrl, expect[1], dtype, mb16, koff)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_each_argument_alone_at_one_element(mode):
    dtype, mb16, path, expect = MODES[mode]
    case, t, want = _inputs("m2_c32_o32_8x8", dtype, mb16)
    ctx = (lambda: _capi().fp32_math("bf16")) if mb16 else (lambda: None)
    ctrl = _call(case, t, {}, path, expect, ctx=ctx())
    tol = TOL["f32mb"] if mb16 else TOL[dtype]
    for name in INPUTS + RESULTS:
        koff = {name: 1}
        got = _call(case, t, koff, path, expect, ctx=ctx())
        _compare("%s %s+1" % (mode, name), got, want, tol)
        _bit_identical("%s %s+1" % (mode, name), got, ctrl, expect[1], dtype, mb16, koff)
    if dtype != F32:   # 8 bytes: the q4 copy of a 16-bit input (an fp32 source needs 16 bytes for q4: never by an offset)
        koff = {"input": 4, "grad_output": 4}
        got = _call(case, t, koff, path, expect, ctx=ctx())
        _compare("%s input+4" % mode, got, want, tol)
        _bit_identical("%s input+4" % mode, got, ctrl, expect[1], dtype, mb16, koff)


@pytest.mark.parametrize("case_name", sorted(PAD_CASES))
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_16bit_tensors_on_the_padded_plan_of_the_fp32_kernels(case_name, dtype):
    """The "auto" path of a 16-bit call outside the native kernels: fp32 matrix kernels through `widen` / `narrow`, behind the
    row movers of the padded plan.  Offset 1 (2 bytes) takes the halfword movers, offset 2 (4 bytes) and 0 the 4-byte ones; all
    three must give the same bits.  Overwrite and accumulate mode (which also moves the caller's grad_input and grad_weight
    INTO the padded buffers)."""
    case, t, want = _inputs(case_name, dtype, False)
    expect = ("mfma", "f32")
    tag = "%s %s" % (S._SHORT[dtype], case_name)
    for accumulate, fill in ((False, float("nan")), (True, 0.0)):
        ctrl = _call(case, t, {}, "auto", expect, accumulate=accumulate, fill=fill)
        _compare("%s aligned acc=%d" % (tag, accumulate), ctrl, want, TOL[dtype])
        for k in (1, 2):
            koff = {n: k for n in INPUTS + RESULTS}
            got = _call(case, t, koff, "auto", expect, accumulate=accumulate, fill=fill)
            _compare("%s +%d acc=%d" % (tag, k, accumulate), got, want, TOL[dtype])
            _bit_identical("%s +%d acc=%d" % (tag, k, accumulate), got, ctrl, "f32", dtype, False, koff)


def test_depthwise_at_offsets():
    case, t, want = _inputs("depthwise", F32, False)
    expect = ("depthwise", "depthwise")
    ctrl = _call(case, t, {}, "auto", expect)
    _compare("f32 depthwise aligned", ctrl, want, TOL[F32])
    for koff in [{n: 1} for n in INPUTS + RESULTS] + [_offsets(t, 0), _offsets(t, 1)]:
        got = _call(case, t, koff, "auto", expect)
        _compare("f32 depthwise %s" % koff, got, want, TOL[F32])
        _bit_identical("depthwise %s" % koff, got, ctrl, "depthwise", F32, False, koff)


@pytest.mark.parametrize("mode", ["f32-auto", "bf16-hp"])
def test_deterministic_mode_is_bit_identical_across_addresses(mode):
    """MDCONV_FLAG_DETERMINISTIC promises every output bit for bit from call to call for the same descriptor and inputs; the
    lists are sorted into a canonical order, so grad_input does not depend on the addresses either."""
    dtype, mb16, path, expect = MODES[mode]
    case, t, want = _inputs("m2_c32_o32_8x8", dtype, mb16)
    capi = _capi()
    ctrl = _call(case, t, {}, path, expect, ctx=capi.deterministic())
    koff = _offsets(t, 0)
    got = _call(case, t, koff, path, expect, ctx=capi.deterministic())
    _compare("%s deterministic" % mode, got, want, TOL[dtype])
    _bit_identical("%s deterministic" % mode, got, ctrl, expect[1], dtype, mb16, koff, det=True)


def test_fp16_direct_backward_adds_next_to_the_margins():
    """A 16-bit backward on the shape-generic path never scatters into the caller's tensors: it runs the fp32 kernels on fp32
    copies (ROUTE_DIRECT_16, f32_copies.hip) and `narrow_kernel<__half, accumulate>` adds the sums to the caller's gradients
    with one 2-byte read-modify-write per element.  (The 16-bit compare-and-swap of mdconv_common.hpp is reached from no
    entry point.)  Gradients at an offset of one element start and end in a dword shared with a margin: the margins must stay
    byte-identical, the sums right."""
    case, t, want = _inputs("m2_c32_o32_8x8", F16, False)
    koff = {n: 1 for n in RESULTS}
    for n in RESULTS:
        assert _like(n, t).numel() % 2 == 0 and _like(n, t).element_size() == 2
    got = _call(case, t, koff, "direct", ("direct", "direct"), accumulate=True, fill=0.0)
    _compare("f16 direct accumulate", got, want, TOL[F16])


@pytest.mark.parametrize("case_name", ["cl_d2_c32_o32_8x8", "cl_d2_c32_o32_7x9"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_channels_last_tensors(case_name, dtype):
    """Channels-last results mode: grad_output stays "element" (hp_nhwc_to_nchw: vsrc by the pointer, vdst by S_o % 8;
    hp_grad_bias_cl reads elements); a channels-last input, output and grad_input are "16-byte" and stay aligned."""
    capi = _capi()
    case, t, want = _inputs(case_name, dtype, False)
    cl = lambda v: v.contiguous(memory_format=torch.channels_last)
    tcl = dict(t, input=cl(t["input"]), grad_output=cl(t["grad_output"]))
    expect = ("mfma", "hp")

    def call(koff):
        views = {n: (None if tcl[n] is None else at_offset(tcl[n], koff.get(n, 0))[0]) for n in INPUTS}
        res, checks = {}, {}
        for n in RESULTS:
            ref = _like(n, t)
            if ref is None:
                res[n] = None
                continue
            ref = cl(ref) if n in ("output", "grad_input") else ref
            res[n], checks[n] = at_offset(torch.full_like(ref, float("nan")), koff.get(n, 0))
        rec = []
        with _spy_kernels(rec), capi.channels_last_results():
            run_product_into(case, views, res["output"], {k: v for k, v in res.items() if k != "output"}, accumulate=False,
                             path="mfma")
        torch.cuda.synchronize()
        assert [r[1:3] for r in rec] == [expect, expect], rec
        # the layouts were HONOURED, not replaced by the wrapper's contiguous temporaries: the forward stored a channels-last
        # output (hp_store_output_cl), the backward read a channels-last grad_output (hp_nhwc_to_nchw) and stored a
        # channels-last grad_input (hp_store_grad_input_cl)
        assert rec[0][3] & capi.FLAG_OUTPUT_CHANNELS_LAST, rec
        assert rec[1][3] & capi.FLAG_OUTPUT_CHANNELS_LAST and rec[1][3] & capi.FLAG_GRAD_INPUT_CHANNELS_LAST, rec
        for n, chk in checks.items():
            chk("%s channels-last %s" % (case_name, n))
        return res

    ctrl = call({})
    _compare("%s %s channels-last aligned" % (S._SHORT[dtype], case_name), ctrl, want, TOL[dtype])
    element_args = ("weight", "bias", "offset", "mask", "grad_weight", "grad_bias", "grad_offset", "grad_mask")
    for k_go in (1, 8, 2):   # vsrc = 0, 1, 0
        koff = dict({n: 1 for n in element_args}, grad_output=k_go, input=8, output=8, grad_input=16)
        got = call(koff)
        _compare("%s %s channels-last grad_output+%d" % (S._SHORT[dtype], case_name, k_go), got, want, TOL[dtype])
        # grad_bias is summed from the NCHW copy (one chunk): bit for bit whatever the address (include/mdconv.h)
        for n in ("output", "grad_weight", "grad_offset", "grad_bias"):
            assert torch.equal(got[n], ctrl[n]), (case_name, k_go, n)


def test_mdconv_cuda_copies_or_refuses_16_byte_class_tensors():
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    capi = _capi()
    case, t, want = _inputs("m2_c32_o32_8x8", F16, False)
    cl = lambda v: v.contiguous(memory_format=torch.channels_last)
    x_cl, _ = at_offset(cl(t["input"]), 1)
    assert x_cl.data_ptr() % 16 == 2 and M._is_channels_last(x_cl) and not x_cl.is_contiguous()
    seen = []
    orig = M._run

    def run(fn_name, d, backward, args, input):
        orig(fn_name, d, backward, args, input)
        seen.append((fn_name, d.input_layout, args[0].value))

    M._run = run
    try:
        geo = (3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 64, True)
        out = M.modulated_deform_conv2d_forward_cuda(x_cl, t["weight"], t["bias"], t["offset"], t["mask"], *geo)
        torch.cuda.synchronize()
        assert len(seen) == 1 and seen[0][1] == 1 and seen[0][2] % 16 == 0 and seen[0][2] != x_cl.data_ptr(), seen
        assert_close("f16 output from a channels-last input at an odd offset", out.double(), want["output"], TOL[F16])
        # a caller's channels-last output / grad_input below 16 bytes: ValueError naming it, nothing launched
        del seen[:]
        with capi.channels_last_results():
            out_cl, chk = at_offset(cl(torch.full_like(t["grad_output"], float("nan"))), 1)
            with pytest.raises(ValueError, match="output must be 16-byte aligned"):
                M._forward(2, True, "mdconv_modulated_deform_conv2d_forward", t["input"], t["weight"], t["bias"], t["offset"],
                           t["mask"], out_cl, (3, 3), (1, 1), (1, 1), (1, 1), 1, 1, 64, True)
            gi_cl, chk_gi = at_offset(cl(torch.zeros_like(t["input"])), 1)
            with pytest.raises(ValueError, match="grad_input must be 16-byte aligned"):   # (the DCNv1 entry point: no mask)
                M.deform_conv2d_backward_cuda(t["input"], t["weight"], t["bias"], t["offset"], gi_cl,
                                              torch.zeros_like(t["weight"]), torch.zeros_like(t["bias"]),
                                              torch.zeros_like(t["offset"]), t["grad_output"], *geo)
        assert not seen, seen
        chk("refused output")
        chk_gi("refused grad_input")
        assert bool(torch.isnan(out_cl).all())
    finally:
        M._run = orig


# ---- the sampling operators ----------------------------------------------------------------------------------------------
def _module(op_name):
    import importlib
    return importlib.import_module("modulated_deform_conv_amd." + {"dcnv4_softmax": "dcnv4"}.get(op_name, op_name))


@functools.lru_cache(maxsize=None)
def _samp_reference(op_name, dtype, cdt):
    t, geo = S.nonfinite_case(op_name, dtype, cdt)   # the fuzz-sized toy case of the operator, finite as drawn
    return t, geo, S.OPS[op_name].ref(t, geo)


def _samp_params():
    return [(name, d, c) for name in sorted(S.OPS) for d, c in S.OPS[name].pairings]


@contextlib.contextmanager
def _spy_pointers(mod, calls):
    orig = mod._run

    def run(fn_name, d, backward, args, input):
        calls.append((fn_name, [a.value for a in args]))
        orig(fn_name, d, backward, args, input)

    mod._run = run
    try:
        yield
    finally:
        mod._run = orig


@pytest.mark.parametrize("op_name, dtype, cdt", _samp_params(),
                         ids=["%s-%s" % (n, S.pairing_id(d, c)) for n, d, c in _samp_params()])
def test_sampling_operator_on_offset_views(op_name, dtype, cdt):
    op, mod = S.OPS[op_name], _module(op_name)
    t_cpu, geo, want = _samp_reference(op_name, dtype, cdt)
    t = S.dev(t_cpu)
    nt = len(t)
    ctrl = op.native(t, geo, grads=S.nan_buffers(op, t), deterministic=True, accumulate=False)
    S.compare(op, "%s %s aligned" % (S.pairing_id(dtype, cdt), op_name), ctrl, want, S.tols(op, t))
    for ks in ((1,) * nt, tuple((1, 2, 4)[i % 3] if v is not None and v.element_size() == 2 else (1, 2)[i % 2] for i, v in enumerate(t))):
        views = tuple(None if v is None else at_offset(v, k)[0] for v, k in zip(t, ks))
        bufs, checks = [], []
        for i, (g, kind) in enumerate(zip(S.nan_buffers(op, t), op.kinds[1:])):
            if g is None:
                bufs.append(g)
                continue
            # the sampled tensor's gradient is "16-byte": 8 elements (16 or 32 bytes) into the guarded buffer; a coordinate
            # gradient is "element": handed over misaligned
            v, chk = at_offset(g, 8 if kind == "v" else ks[i])
            bufs.append(v)
            checks.append(chk)
        calls = []
        with _spy_pointers(mod, calls):
            got = op.native(views, geo, grads=tuple(bufs), deterministic=True, accumulate=False)
        for chk in checks:
            chk("%s gradient" % op_name)
        assert [c[0].rsplit("_", 1)[1] for c in calls] == ["forward", "backward"], calls
        for (fn, ptrs), tensors in zip(calls, (views[:-1], views)):
            for i, v in enumerate(tensors):
                if v is None:
                    continue
                sixteen = i == 0 or i == nt - 1   # the sampled tensor and grad_output
                assert v.data_ptr() % 16 != 0, (op_name, i)
                if sixteen:
                    assert ptrs[i] % 16 == 0 and ptrs[i] != v.data_ptr(), (fn, i, "a 16-byte class input was not copied")
                else:
                    assert ptrs[i] == v.data_ptr(), (fn, i, "an element class input was copied")
        for (fn, ptrs), b in zip(calls[1:], (bufs,)):
            assert [p for p in ptrs[nt:]] == [0 if g is None else g.data_ptr() for g in b], (fn, "the gradients went elsewhere")
        S.compare(op, "%s %s offsets %s" % (S.pairing_id(dtype, cdt), op_name, ks), got, want, S.tols(op, t))
        for what, a, b in zip(op.names, got, ctrl):   # deterministic mode: every result bit for bit
            assert (a is None and b is None) or torch.equal(a, b), (op_name, ks, what)


def _forward_with_output(op_name, views, geo, out):
    m = _module(op_name)
    if op_name == "dcnv3":
        return m.dcnv3_forward(*views[:3], *geo, output=out)
    if op_name.startswith("dcnv4"):
        return m.dcnv4_forward(*views[:2], *geo, output=out, softmax=S.OPS[op_name].softmax)
    if op_name == "msda":
        return m.ms_deform_attn_forward(views[0], geo, views[1], views[2], output=out)
    if op_name == "msda3d":
        return m.ms_deform_attn_3d_forward(views[0], geo, views[1], views[2], output=out)
    if op_name == "fda":
        return m.flash_deform_attn_forward(views[0], geo[0], views[1], geo[1], output=out)
    if op_name == "dagg":
        return m.deformable_aggregation_forward(views[0], geo, views[1], views[2], output=out)
    return m.deform_roi_pool_forward(views[0], views[1], views[2], **geo, output=out)


@pytest.mark.parametrize("op_name", sorted(S.OPS))
def test_sampling_result_buffers_below_16_bytes_are_refused(op_name):
    op, mod = S.OPS[op_name], _module(op_name)
    t_cpu, geo, want = _samp_reference(op_name, F16, None)
    t = S.dev(t_cpu)
    out_shape = want[0].shape
    out_v, chk_out = at_offset(torch.full(out_shape, float("nan"), dtype=F16, device=S.DEV), 1)
    calls = []
    with _spy_pointers(mod, calls):
        with pytest.raises(ValueError, match="output must be 16-byte aligned"):
            _forward_with_output(op_name, t, geo, out_v)
        assert not calls
        # an aligned output= in the middle of a guarded buffer is written in place, margins intact
        out_a, chk_a = at_offset(torch.full(out_shape, float("nan"), dtype=F16, device=S.DEV), 8)
        assert _forward_with_output(op_name, t, geo, out_a) is out_a
        chk_a("%s output=" % op_name)
        assert_close("f16 %s output=" % op_name, out_a, want[0], S.TOL[F16])
        del calls[:]
        bufs = list(S.nan_buffers(op, t))
        bufs[0], chk_gv = at_offset(bufs[0], 1)
        with pytest.raises(ValueError, match="%s must be 16-byte aligned" % op.names[1]):
            op.native(t, geo, grads=tuple(bufs), deterministic=False, accumulate=False)
        assert [c[0].rsplit("_", 1)[1] for c in calls] == ["forward"], calls   # the backward was refused before its launch
    chk_out("%s refused output" % op_name)
    chk_gv("%s refused %s" % (op_name, op.names[1]))
    assert bool(torch.isnan(out_v).all()) and bool(torch.isnan(bufs[0]).all())


def _functional(op_name, v, geo):
    m = _module(op_name)
    if op_name == "dcnv3":
        return m.dcnv3_core(v[0], v[1], v[2], *geo)
    if op_name.startswith("dcnv4"):
        return m.dcnv4_core(v[0], v[1], *geo, softmax=S.OPS[op_name].softmax)
    if op_name == "msda":
        return m.ms_deform_attn(v[0], geo, v[1], v[2])
    if op_name == "msda3d":
        return m.ms_deform_attn_3d(v[0], geo, v[1], v[2])
    if op_name == "fda":
        return m.flash_deform_attn(v[0], geo[0], v[1], geo[1])
    if op_name == "dagg":
        return m.deformable_aggregation(v[0], geo, v[1], v[2])
    # logical NCHW in and out: permute views of the channels-last tensors, no copy
    return m.deform_roi_pool(v[0].permute(0, 3, 1, 2), v[1], v[2], **geo).permute(0, 2, 3, 1)


@pytest.mark.parametrize("op_name", sorted(S.OPS))
def test_autograd_functions_on_offset_views(op_name):
    """Function.apply with every input and the incoming gradient at an odd offset: nothing changes for the user."""
    op = S.OPS[op_name]
    t_cpu, geo, want = _samp_reference(op_name, F16, F32 if (F16, F32) in op.pairings else None)
    t = S.dev(t_cpu)
    views = [None if v is None else at_offset(v, 1)[0] for v in t]
    leaves = [v for v, like in zip(views[:-1], t[:-1]) if v is not None]
    diff = [i for i, v in enumerate(views[:-1]) if v is not None and not (op_name == "droi" and i == 1)]   # rois: no gradient
    for i in diff:
        views[i].requires_grad_(True)
    out = _functional(op_name, views[:-1], geo)
    out.backward(views[-1])   # (the incoming gradient at an odd offset as well)
    torch.cuda.synchronize()
    got = (out.detach(),) + tuple(views[i].grad for i in diff)
    assert len(leaves) >= len(diff)
    S.compare(op, "f16 %s Function.apply" % op_name, got, want, S.tols(op, t))
