"""Deterministic mode on the GPU (include/mdconv.h: MDCONV_FLAG_DETERMINISTIC; csrc/csr_sort.hip).

Every case runs its backward eight times with the flag, in overwrite mode from ``torch.empty`` result buffers, and asserts
  * all five gradients are ``torch.equal`` across the eight runs,
  * the first run matches the oracle at the tolerance of the sibling parity test (fp32 1e-4, 16-bit: TOL of test_gpu_hp.py),
  * the first run matches the same call without the flag at that tolerance.
Whether the eight flag-less runs differed is printed, not asserted: arrival order may well be stable on a small grid.
``grad_output`` and ``mask`` take values spread over six decades with mixed signs, so that any change of the summation
order of grad_input changes bits.
"""
import os
import subprocess
import sys
import warnings

import pytest
import torch

from tests.cases import CASE_BY_NAME, make_inputs, _c, M2, M3, D2, D3, ndim, out_size
from tests.util import assert_close, guarded_run, run_oracle, run_product_into

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {torch.float32: 1e-4, torch.float16: 5e-3, torch.bfloat16: 3e-2}   # tests/test_gpu_parity.py, tests/test_gpu_hp.py
RUNS = 8
KEYS = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")

BASE = _c("det_mdcn2d_c64_o64_8x8", M2, 2, 64, 64, (8, 8), 3, seed=201)


def _decades(shape, gen, top):
    """N(0, 1) x 10^U(top - 6, top): six decades, mixed signs"""
    return torch.randn(shape, generator=gen, dtype=torch.float64) * 10.0 ** (torch.rand(shape, generator=gen, dtype=torch.float64) * 6 + (top - 6))


def _inputs(case, dtype, sampling_f32=False, offsets=None):
    """make_inputs with wide-range grad_output / mask (and `offsets` in place of the case's, when given), on the GPU;
    rounded to `dtype` once, so the oracle sees what the kernels see"""
    t = make_inputs(case, dtype=torch.float64)
    gen = torch.Generator().manual_seed(7000 + case["seed"])
    # fp32: 1e-3 .. 1e3.  16-bit tensors: 1e-5 .. 10, so that mask x grad_col sums stay inside the fp16 range (65504)
    top = 3 if dtype == torch.float32 else 1
    t["grad_output"] = _decades(t["grad_output"].shape, gen, top)
    if t["mask"] is not None:
        t["mask"] = _decades(t["mask"].shape, gen, top)
    if offsets is not None:
        t["offset"] = offsets.to(torch.float64)
    out = {}
    for k, v in t.items():
        if v is None:
            out[k] = None
        else:
            dt = torch.float32 if sampling_f32 and k in ("offset", "mask") else dtype
            out[k] = v.to(dt).cuda().contiguous()
    return out


def _crafted_offsets(case, n, seed=0):
    """Image 0: exactly n samples (tap, output pixel) land on position (0.5, 0.5), every other one far outside the image;
    image 1: N(0, 2) offsets.  2-D, one deformable group."""
    gen = torch.Generator().manual_seed(4242 + seed + n)
    B, K = case["B"], 9
    Ho, Wo = out_size(case)
    off = torch.randn(B, 2 * K, Ho, Wo, generator=gen, dtype=torch.float64) * 2.0
    pick = torch.randperm(K * Ho * Wo, generator=gen)[:n]
    chosen = torch.zeros(K * Ho * Wo, dtype=torch.bool)
    chosen[pick] = True
    chosen = chosen.view(K, Ho, Wo)
    for tap in range(K):
        ti, tj = tap // 3, tap % 3
        for a, tt, coords in ((0, ti, torch.arange(Ho, dtype=torch.float64).view(Ho, 1).expand(Ho, Wo)),
                              (1, tj, torch.arange(Wo, dtype=torch.float64).view(1, Wo).expand(Ho, Wo))):
            base = coords * 1 - 1 + tt            # o * stride - pad + tap * dil
            off[0, 2 * tap + a] = torch.where(chosen[tap], 0.5 - base, -100.0 - base)
    return off


def _buffers(t, case, fill=None):
    mk = (lambda v: torch.empty_like(v, memory_format=torch.contiguous_format)) if fill is None else (lambda v: fill[id(v)].clone())
    x, w, off, m = t["input"], t["weight"], t["offset"], t["mask"]
    g = dict(grad_input=mk(x), grad_weight=mk(w), grad_offset=mk(off), grad_mask=None if m is None else mk(m),
             grad_bias=mk(t["bias"]) if case["bias"] else None)
    out = torch.empty_like(t["grad_output"])
    return out, g


def _run(case, t, det, fill=None, path=None):
    from modulated_deform_conv_amd import _capi
    out, g = _buffers(t, case, fill)
    with _capi.deterministic(det):
        run_product_into(case, t, out, g, accumulate=fill is not None, path=path)
    torch.cuda.synchronize()
    return out, g, _capi.last_kernels()


def _same(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in KEYS)


def _oracle(case, t):
    return run_oracle(case, {k: (None if v is None else v.float()) for k, v in t.items()}, torch.float32)


def _check(case, t, dtype, kernels=None, want=None, runs=RUNS):
    """the three assertions of the module docstring; returns the first deterministic run's gradients and the oracle's"""
    tol = TOL[dtype]
    first_out, first, kern = _run(case, t, True)
    if kernels is not None:
        assert kern == kernels, kern
    assert kern in ("f32", "hp"), kern
    for i in range(1, runs):
        _, g, _ = _run(case, t, True)
        for k in KEYS:
            assert (g[k] is None and first[k] is None) or torch.equal(g[k], first[k]), "%s: run %d differs from run 0" % (k, i)
    want_out, want = want or _oracle(case, t)
    plain_out, plain, _ = _run(case, t, False)
    differed = []
    for i in range(1, runs):
        again = _run(case, t, False)[1]
        differed += [k for k in KEYS if plain[k] is not None and not torch.equal(again[k], plain[k])]
    print("%s %s: flag-less runs %s" % (case["name"], dtype, "DIFFERED in " + ", ".join(sorted(set(differed))) if differed
                                        else "were bit-equal too"))
    assert_close("output", first_out.float(), want_out, tol)
    for k in KEYS:
        if want[k] is None or first[k] is None:
            continue
        assert_close(k + " vs oracle", first[k].float(), want[k], tol)
        assert_close(k + " vs flag-less", first[k].float(), plain[k].float(), tol)
    return first, (want_out, want)


# ------------------------------------------------------------------------------------------ fp32 matrix-core kernels
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_crafted_row_lengths(n):
    """Rows of exactly n entries: one wave per row up to 64 entries (its boundary at 63 / 64), the workgroup path
    beyond (65, 300).  Pair-keyed 2-D lists: the n samples at (0.5, 0.5) make two rows of n entries, anchors (0, 0) and (1, 0)."""
    t = _inputs(BASE, torch.float32, offsets=_crafted_offsets(BASE, n))
    want_out, want = _oracle(BASE, t)
    # the input does produce those lists: image 0 receives gradient in the 2 x 2 block the n samples touch and nowhere else
    gi0 = want["grad_input"][0]
    touched = gi0.abs().amax(dim=0) > 0
    assert touched[:2, :2].all() and int(touched.sum()) == 4, touched.nonzero().tolist()
    _check(BASE, t, torch.float32, kernels="f32", want=(want_out, want))


@pytest.mark.parametrize("C", [64, 128])
def test_two_deformable_groups(C):
    """Segment stride of the lists: two deformable groups (64 -> 64: groups of 32 channels, a padded or split plan of the
    fp32 backward; 128 -> 64: groups of 64, the grouped gather itself)."""
    case = _c("det_mdcn2d_c%d_dg2" % C, M2, 2, C, 64, (8, 8), 3, dgroups=2, seed=202)
    _check(case, _inputs(case, torch.float32), torch.float32, kernels="f32")


def test_fp32_3d_sample_keyed_lists():
    """The 3-D lists of mfma_csr3d.hip (two int4 per entry), at the geometry of the golden `mfma_dcn3d_c16_o16_5x6x5`, and
    with two deformable groups.
    NOTE: no 3-D shape has pair-keyed lists -- bwd_dims() sets `sample_keyed = (nd == 3)` unconditionally, so the "3-D
    where bd.sample_keyed is false" producer does not exist in this tree.  The pair-keyed format (one int4 per entry) is
    what every 2-D fp32 case of this file sorts; the second 3-D shape covers the nearest thing that does vary in 3-D, the
    segment stride of the sample-keyed lists (DG = 2)."""
    case = CASE_BY_NAME["mfma_dcn3d_c16_o16_5x6x5"]
    _check(case, _inputs(case, torch.float32), torch.float32, kernels="f32")
    case = CASE_BY_NAME["mfma_mdcn3d_g2_dg2_c128_o32"]
    _check(case, _inputs(case, torch.float32), torch.float32, kernels="f32", runs=4)


def test_accumulate_mode():
    """Buffers pre-filled with a fixed random tensor, every run from a fresh copy of it: bit-equal results."""
    t = _inputs(BASE, torch.float32)
    gen = torch.Generator().manual_seed(99)
    fill = {id(v): torch.randn(v.shape, generator=gen).cuda() for v in t.values() if v is not None}
    _, first, kern = _run(BASE, t, True, fill=fill)
    assert kern == "f32"
    for i in range(1, RUNS):
        _, g, _ = _run(BASE, t, True, fill=fill)
        assert _same(g, first), "accumulate-mode run %d differs" % i
    _, want = _oracle(BASE, t)
    for k in KEYS:
        base = {"grad_input": "input", "grad_offset": "offset", "grad_mask": "mask", "grad_weight": "weight", "grad_bias": "bias"}[k]
        assert_close(k, first[k].float(), want[k] + fill[id(t[base])].cpu(), TOL[torch.float32])


@pytest.mark.parametrize("name, C, O, G, DG", [("group_padded", 96, 64, 1, 4), ("split_backward", 128, 128, 2, 4)])
def test_padded_and_split_plans(name, C, O, G, DG):
    case = _c("det_mdcn2d_%s" % name, M2, 2, C, O, (8, 8), 3, groups=G, dgroups=DG, seed=203)
    _check(case, _inputs(case, torch.float32), torch.float32, kernels="f32")


def test_graph_replay():
    """One flagged backward captured with torch.cuda.graph: the sort is a plain kernel on the gather's stream (no host
    synchronisation, no memset node), so it captures; three replays, bit-equal among themselves and to the eager run."""
    from modulated_deform_conv_amd import _capi
    t = _inputs(BASE, torch.float32, offsets=_crafted_offsets(BASE, 300))
    _, eager, _ = _run(BASE, t, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out, g = _buffers(t, BASE)
    with torch.cuda.stream(side), _capi.deterministic():
        run_product_into(BASE, t, out, g, accumulate=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _capi.deterministic(), torch.cuda.graph(graph):
        run_product_into(BASE, t, out, g, accumulate=False)
    for i in range(3):
        for v in g.values():
            if v is not None:
                v.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(g, eager), "replay %d differs from the eager run" % i


def test_crafted_rows_under_the_guarded_workspace(monkeypatch):
    """The sort's scratch lies inside the workspace mdconv_workspace_bytes reports with the flag: long rows (300 entries,
    ranked into the scratch copy) with the workspace between pattern-filled margins."""
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    touched, calls = [], []
    monkeypatch.setattr(M, "_run", guarded_run(touched, calls))
    t = _inputs(BASE, torch.float32, offsets=_crafted_offsets(BASE, 300))
    _, a, _ = _run(BASE, t, True)
    _, b, _ = _run(BASE, t, True)
    assert not touched, touched
    assert _same(a, b)
    assert any(fn.endswith("backward") and nbytes > 0 for fn, nbytes in calls)


# ------------------------------------------------------------------------------------------ native 16-bit kernels
@pytest.mark.parametrize("name, dtype, samp32", [("fp16_short_entries", torch.float16, False),
                                                 ("bf16_long_entries", torch.bfloat16, False),
                                                 ("fp16_fp32_sampling", torch.float16, True)])
def test_native_16bit_2d(name, dtype, samp32):
    """Short entries (one int4: 2-D fp16 tensors) and long ones (two int4: bf16), with 16-bit and with fp32 offsets.
    bf16 runs the crafted rows of 65 entries (the workgroup path on two-int4 entries); the fp16 cases run the case's own
    N(0, 1) offsets: the crafted input leaves half of grad_offset exactly zero, which halves the rms the per-element
    criterion of assert_close scales its slack with -- at fp16's 5e-3 the 11-bit grad_col rows then miss it on one element
    of grad_offset (6.35e-3, scaled max error 3.1e-4), with or without the flag; nothing the list order touches."""
    offsets = _crafted_offsets(BASE, 65) if dtype == torch.bfloat16 else None
    t = _inputs(BASE, dtype, sampling_f32=samp32, offsets=offsets)
    _check(BASE, t, dtype, kernels="hp")


def test_native_16bit_3d():
    # the smallest 3-D shape tests/test_gpu_hp.py runs natively (hp_mdcn3d_c32_o32)
    case = _c("hp_mdcn3d_c32_o32", M3, 1, 32, 32, (5, 6, 5), 3, seed=111)
    _check(case, _inputs(case, torch.float16), torch.float16, kernels="hp")


# ------------------------------------------------------------------------------------------ forced multi-chunk call
CHUNK_CASE = _c("det_mdcn2d_c64_chunks_2_2_1", M2, 5, 64, 64, (8, 8), 3, seed=204)
# fp32 make_plan: the largest per-image buffer is grad_col, C K S_o 4 = 147456 bytes; twice that and a little gives chunks
# of 2 images: 2 + 2 + 1, the last one shorter (the way tests/test_gpu_chunk_plans.py forces chunks: the limit is read once
# per process, so the call runs in a child)
CHUNK_LIMIT = 2 * 64 * 9 * 64 * 4 + 4096


def chunk_child():
    assert int(os.environ["MDCONV_CHUNK_LIMIT_BYTES"]) == CHUNK_LIMIT
    _check(CHUNK_CASE, _inputs(CHUNK_CASE, torch.float32), torch.float32, kernels="f32")
    print("DET_CHUNKS_OK")


def test_forced_multi_chunk_call():
    env = dict(os.environ, MDCONV_CHUNK_LIMIT_BYTES=str(CHUNK_LIMIT), MDCONV_DEBUG_PLAN="1")
    code = "import sys; sys.path.insert(0, %r); from tests.test_gpu_deterministic import chunk_child; chunk_child()" % ROOT
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    report = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0 and "DET_CHUNKS_OK" in r.stdout, report
    # three chunks ran: GEMM-1 plan lines of 2-image chunks (128 pixels = 1 tile of 128) and of the 1-image tail differ
    assert len({ln for ln in r.stderr.splitlines() if "GEMM-1 plan" in ln}) >= 1, report


# ------------------------------------------------------------------------------------------ refusals, public surface
class _torch_deterministic:
    def __init__(self, on, warn_only=False):
        self.on, self.warn_only = on, warn_only

    def __enter__(self):
        self.prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
        torch.use_deterministic_algorithms(self.on, warn_only=self.warn_only)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.prev[0], warn_only=self.prev[1])
        return False


def _leaves(t):
    return {k: t[k].clone().requires_grad_(True) for k in ("input", "offset", "mask")}


def _flags_seen(monkeypatch):
    """flags word of every descriptor MDCONV_CUDA hands to the library"""
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    seen, real = [], M._run

    def spy(fn_name, d, backward, args, input):
        real(fn_name, d, backward, args, input)
        seen.append((fn_name.rsplit("_", 1)[1], int(d.flags)))
    monkeypatch.setattr(M, "_run", spy)
    return seen


def test_module_and_op_follow_the_torch_global(monkeypatch):
    from modulated_deform_conv_amd.modulated_deform_conv import ModulatedDeformConv2d
    import modulated_deform_conv_amd.ops  # noqa: F401  (registers mdconv::deform_conv)
    seen = _flags_seen(monkeypatch)
    t = _inputs(BASE, torch.float32, offsets=_crafted_offsets(BASE, 300))
    torch.manual_seed(0)
    mod = ModulatedDeformConv2d(64, 64, 3, padding=1).cuda()
    go = t["grad_output"]

    def module_grads():
        lv = _leaves(t)
        mod.weight.grad = None
        mod(lv["input"], lv["offset"], lv["mask"]).backward(go)   # only this library's op runs inside
        torch.cuda.synchronize()
        return [lv[k].grad.clone() for k in ("input", "offset", "mask")] + [mod.weight.grad.clone()]

    def op_grads():
        lv = _leaves(t)
        w = mod.weight.detach().clone().requires_grad_(True)
        out = torch.ops.mdconv.deform_conv(lv["input"], lv["offset"], lv["mask"], w, None, [1, 1], [1, 1], [1, 1], 1, 1, 64)
        out.backward(go)
        torch.cuda.synchronize()
        return [lv[k].grad.clone() for k in ("input", "offset", "mask")] + [w.grad.clone()]

    with _torch_deterministic(True):
        for fn in (module_grads, op_grads):
            del seen[:]
            a, b = fn(), fn()
            assert all(torch.equal(x, y) for x, y in zip(a, b)), fn.__name__
            assert seen and all(f == 1 for _, f in seen), seen      # forward and backward descriptors carry the flag
    del seen[:]
    module_grads()
    assert seen and all(f == 0 for _, f in seen), seen              # ... and none does outside


def test_context_manager_has_the_effect_of_the_global_flag(monkeypatch):
    from modulated_deform_conv_amd import _capi
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    seen = _flags_seen(monkeypatch)
    t = _inputs(BASE, torch.float32)
    geo = (3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 64, False)
    b = t["input"].new_empty(0)
    call = lambda: M.modulated_deform_conv2d_backward_cuda(t["input"], t["weight"], b, t["offset"], t["mask"], t["grad_output"], *geo)
    with _capi.deterministic():
        a = call()
        c = call()
    torch.cuda.synchronize()
    assert [f for _, f in seen] == [1, 1]
    assert all(torch.equal(x, y) for x, y in zip(a[:4], c[:4]))
    with _torch_deterministic(True):
        with _capi.deterministic(False):     # the context manager turns the mode off inside the global flag
            call()
        call()
    assert [f for _, f in seen[2:]] == [0, 1]


def _c4_module_and_inputs():
    from modulated_deform_conv_amd.modulated_deform_conv import DeformConv2d
    case = CASE_BY_NAME["cfg1_dcn2d_c4_8x8_b1"]
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    torch.manual_seed(1)
    mod = DeformConv2d(4, 4, 3, padding=1).cuda()
    with torch.no_grad():
        mod.weight.copy_(t["weight"])
    return case, t, mod


def test_c4_backward_is_refused_and_its_forward_runs():
    case, t, mod = _c4_module_and_inputs()
    x, off = t["input"].clone().requires_grad_(True), t["offset"].clone().requires_grad_(True)
    with _torch_deterministic(True):
        out = mod(x, off)                                           # the forward is deterministic anyway
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="deterministic") as ei:
            out.backward(t["grad_output"])
    assert "floating-point atomics" in str(ei.value)
    want_out, _ = run_oracle(case, t, torch.float32)
    assert_close("output", out.detach(), want_out, 1e-4)


def test_c4_backward_warns_once_with_warn_only_and_matches_the_oracle(monkeypatch):
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    monkeypatch.setattr(M, "_warned_nondeterministic", False)
    case, t, mod = _c4_module_and_inputs()
    _, want = run_oracle(case, t, torch.float32)
    with _torch_deterministic(True, warn_only=True):
        with pytest.warns(UserWarning, match="deterministic"):
            x, off = t["input"].clone().requires_grad_(True), t["offset"].clone().requires_grad_(True)
            mod(x, off).backward(t["grad_output"])
        with warnings.catch_warnings():
            warnings.simplefilter("error")                          # once per process: the second backward is silent
            x2, off2 = t["input"].clone().requires_grad_(True), t["offset"].clone().requires_grad_(True)
            mod.weight.grad = None
            mod(x2, off2).backward(t["grad_output"])
    torch.cuda.synchronize()
    assert_close("grad_input", x2.grad, want["grad_input"], 1e-4)
    assert_close("grad_offset", off2.grad, want["grad_offset"], 1e-4)
    assert_close("grad_weight", mod.weight.grad, want["grad_weight"], 1e-4)
