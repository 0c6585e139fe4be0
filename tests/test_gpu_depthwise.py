"""The depthwise family on the GPU (include/mdconv.h: MDCONV_PATH_DEPTHWISE, MDCONV_KERNELS_DEPTHWISE; csrc/dw_*.hip):
fp32 layers with groups == C_in on VALU kernels of their own, forward and backward, 2-D and 3-D, modulated and not.

Every case is forced with ``path="depthwise"`` unless it says AUTO, and checked against the fp32 oracle at the project's
fp32 tolerance (``assert_close(..., 1e-4)``) on output and all five gradients.  The shapes are the smallest that reach each
tail of the kernels: a pixel tail inside one tile, channel counts that are no multiple of 8 or 16, deformable groups of 8
channels, multipliers 2 and 4, several pixel tiles (partial rows of grad_weight from many workgroups), more taps than image
rows, even kernels and mixed strides in 3-D."""
import pytest
import torch

from tests.cases import D2, D3, M2, M3, _c, make_inputs, ndim, out_size
from tests.util import assert_close, guarded_run, run_oracle, run_product, run_product_into

pytestmark = pytest.mark.gpu

TOL = 1e-4
KEYS = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")
SOURCE = {"grad_input": "input", "grad_offset": "offset", "grad_mask": "mask", "grad_weight": "weight", "grad_bias": "bias"}

CASES = [
    _c("dw_mdcn2d_c24_dg3_11x9", M2, 2, 24, 24, (11, 9), 3, groups=24, dgroups=3, bias=True, seed=301),
    _c("dw_mdcn2d_c16_o32_s2_dil2", M2, 1, 16, 32, (13, 10), 3, stride=2, padding=2, dilation=2, groups=16, dgroups=2, seed=302),
    _c("dw_dcn2d_c20_far_offsets", D2, 3, 20, 20, (9, 12), 3, groups=20, in_step=1, bias=False, seed=303, offset_scale=3.0),
    _c("dw_mdcn2d_c8_40x37", M2, 3, 8, 8, (40, 37), 3, groups=8, seed=304),
    _c("dw_mdcn2d_c8_o32_k5_7x7", M2, 1, 8, 32, (7, 7), 5, padding=2, groups=8, seed=305),
    _c("dw_dcn3d_c16_dg2_5x6x5", D3, 2, 16, 16, (5, 6, 5), 3, groups=16, dgroups=2, seed=306),
    _c("dw_mdcn3d_c8_o16_k2_s121", M3, 1, 8, 16, (4, 7, 6), 2, padding=0, stride=(1, 2, 1), groups=8, bias=True, seed=307),
]
BY_NAME = {c["name"]: c for c in CASES}
IDS = [c["name"] for c in CASES]
CASE_2D, CASE_3D = CASES[0], CASES[5]

_cache = {}


def _fixture(case):
    """inputs on the GPU and the oracle's results, computed once per case and never written to"""
    if case["name"] not in _cache:
        t = make_inputs(case, dtype=torch.float32, device="cuda")
        _cache[case["name"]] = (t, run_oracle(case, t, torch.float32))
    return _cache[case["name"]]


def _check_parity(out, grads, want_out, want, tag=""):
    assert_close(tag + "output", out, want_out, TOL)
    for k in KEYS:
        if want[k] is None:
            continue
        assert_close(tag + k, grads[k], want[k], TOL)


def _buffers(case, t, fill):
    """caller-allocated results: ``fill`` a float (every element) or a dict name -> tensor to clone"""
    mk = (lambda name, ref: torch.full_like(ref, fill)) if not isinstance(fill, dict) else (lambda name, ref: fill[name].clone())
    g = dict(grad_input=mk("grad_input", t["input"]), grad_offset=mk("grad_offset", t["offset"]),
             grad_mask=None if t["mask"] is None else mk("grad_mask", t["mask"]), grad_weight=mk("grad_weight", t["weight"]),
             grad_bias=mk("grad_bias", t["bias"]) if case["bias"] else None)
    return torch.full_like(t["grad_output"], float("nan")), g


def _overwrite_run(case, t, path="depthwise", det=None):
    """forward + backward into NaN-filled buffers, overwrite mode"""
    from modulated_deform_conv_amd import _capi
    out, g = _buffers(case, t, float("nan"))
    if det is None:
        run_product_into(case, t, out, g, accumulate=False, path=path)
    else:
        with _capi.deterministic(det):
            run_product_into(case, t, out, g, accumulate=False, path=path)
    torch.cuda.synchronize()
    return out, g


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parity(case):
    from modulated_deform_conv_amd import _capi
    t, (want_out, want) = _fixture(case)
    out, grads, paths = run_product(case, t, "depthwise")
    assert _capi.last_kernels() == "depthwise"
    assert paths == ["depthwise", "depthwise"]
    _check_parity(out, grads, want_out, want)


def test_auto_reaches_the_family():
    from modulated_deform_conv_amd import _capi
    case = CASES[0]
    t, (want_out, want) = _fixture(case)
    out, grads, paths = run_product(case, t, "auto")
    assert paths == ["depthwise", "depthwise"] and _capi.last_kernels() == "depthwise"
    _check_parity(out, grads, want_out, want)


@pytest.mark.parametrize("case", [CASES[1], CASES[6]], ids=[IDS[1], IDS[6]])
def test_three_way(case):
    """the shape-generic kernels, the depthwise kernels and (test_parity) the oracle agree pairwise"""
    from modulated_deform_conv_amd import _capi
    t, _ = _fixture(case)
    out_d, g_d, paths = run_product(case, t, "direct")
    assert paths == ["direct", "direct"] and _capi.last_kernels() == "direct"
    out_w, g_w, paths = run_product(case, t, "depthwise")
    assert paths == ["depthwise", "depthwise"]
    assert_close("output", out_w, out_d.cpu(), TOL)
    for k in KEYS:
        if g_d[k] is not None:
            assert_close(k, g_w[k], g_d[k].cpu(), TOL)


@pytest.mark.parametrize("case", [CASE_2D, CASE_3D], ids=["2d", "3d"])
def test_accumulate_mode(case):
    from modulated_deform_conv_amd import _capi
    t, (want_out, want) = _fixture(case)
    out, plain = _overwrite_run(case, t)       # overwrite mode: on buffers prefilled with NaN
    assert _capi.last_kernels() == "depthwise"
    _check_parity(out, plain, want_out, want, "overwrite ")
    gen = torch.Generator().manual_seed(77)
    fill = {k: torch.randn(t[SOURCE[k]].shape, generator=gen).cuda() for k in KEYS if t[SOURCE[k]] is not None}
    out2, acc = _buffers(case, t, fill)
    run_product_into(case, t, out2, acc, accumulate=True, path="depthwise")
    torch.cuda.synchronize()
    assert _capi.last_kernels() == "depthwise"
    for k in KEYS:
        if plain[k] is not None:
            assert_close("accumulate " + k, acc[k], (fill[k] + plain[k]).cpu(), TOL)


@pytest.mark.parametrize("case", [CASE_2D, CASE_3D], ids=["2d", "3d"])
def test_selective_backward(case):
    """every requested gradient is bit for bit the full call's (grad_input: inside deterministic mode, which fixes the
    order of its lists); skipped gradients are passed as None"""
    from modulated_deform_conv_amd import _capi
    from tests.test_gpu_selective_backward import backward
    t, _ = _fixture(case)
    prev = _capi.set_path("depthwise")
    try:
        with _capi.deterministic():
            full = backward(case, t)
            assert _capi.last_kernels() == "depthwise"
            for skip in ((True, False), (False, True), (True, True)):
                got = backward(case, t, skip)
                assert _capi.last_kernels() == "depthwise", skip
                for k in KEYS:
                    skipped = (k == "grad_input" and skip[0]) or (k in ("grad_weight", "grad_bias") and skip[1])
                    if skipped or full[k] is None:
                        assert got[k] is None or skipped, (skip, k)
                        continue
                    assert torch.equal(got[k], full[k]), (skip, k)
    finally:
        _capi.set_path(prev)


DET_CASE = _c("dw_det_mdcn2d_c8_8x8", M2, 2, 8, 8, (8, 8), 3, groups=8, seed=308)


def _one_pixel_offsets(case, row=2.0, col=3.0):
    """image 0: every sample (tap, output pixel) lands exactly on input pixel (row, col) -- one list of K x S_o entries;
    the other images keep N(0, 2) offsets.  2-D, k 3, stride 1, pad 1, one deformable group."""
    gen = torch.Generator().manual_seed(4300)
    Ho, Wo = out_size(case)
    off = torch.randn(case["B"], 18, Ho, Wo, generator=gen, dtype=torch.float64) * 2.0
    ys = torch.arange(Ho, dtype=torch.float64).view(Ho, 1).expand(Ho, Wo)
    xs = torch.arange(Wo, dtype=torch.float64).view(1, Wo).expand(Ho, Wo)
    for tap in range(9):
        off[0, 2 * tap] = row - (ys - 1 + tap // 3)
        off[0, 2 * tap + 1] = col - (xs - 1 + tap % 3)
    return off


def _det_inputs():
    if "det" not in _cache:
        t = make_inputs(DET_CASE, dtype=torch.float32, device="cuda")
        t["offset"] = _one_pixel_offsets(DET_CASE).float().cuda()
        gen = torch.Generator().manual_seed(4301)
        # six decades, mixed signs: any change of the summation order changes bits
        shape = t["grad_output"].shape
        t["grad_output"] = (torch.randn(shape, generator=gen) * 10.0 ** (torch.rand(shape, generator=gen) * 6 - 3)).cuda()
        _cache["det"] = (t, run_oracle(DET_CASE, t, torch.float32))
    return _cache["det"]


def test_deterministic_mode_with_one_long_list():
    from modulated_deform_conv_amd import _capi
    t, (want_out, want) = _det_inputs()
    # the input does produce that list: image 0 receives gradient in one pixel and nowhere else
    touched = want["grad_input"][0].abs().amax(dim=0) > 0
    assert int(touched.sum()) == 1 and bool(touched[2, 3]), touched.nonzero().tolist()
    out_a, a = _overwrite_run(DET_CASE, t, det=True)
    assert _capi.last_kernels() == "depthwise"
    out_b, b = _overwrite_run(DET_CASE, t, det=True)
    assert torch.equal(a["grad_input"], b["grad_input"])
    _check_parity(out_a, a, want_out, want)
    # the other four gradients never depend on the mode, nor on the call
    out_c, c = _overwrite_run(DET_CASE, t, det=False)
    out_d, d = _overwrite_run(DET_CASE, t, det=False)
    assert torch.equal(out_a, out_b) and torch.equal(out_a, out_c)
    for k in ("grad_offset", "grad_mask", "grad_weight", "grad_bias"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) and torch.equal(c[k], d[k]), k
    assert_close("grad_input without the mode", c["grad_input"], want["grad_input"], TOL)


@pytest.mark.parametrize("case", [CASE_2D, CASE_3D], ids=["2d", "3d"])
def test_guarded_workspace(case, monkeypatch):
    """the workspace between pattern-filled margins, itself pattern-filled: no byte outside mdconv_workspace_bytes changes,
    and no kernel reads a slot nobody wrote"""
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    from modulated_deform_conv_amd import _capi
    touched, calls = [], []
    monkeypatch.setattr(M, "_run", guarded_run(touched, calls))
    t, (want_out, want) = _fixture(case)
    for det in (False, True):
        with _capi.deterministic(det):
            out, grads, paths = run_product(case, t, "depthwise")
        assert paths == ["depthwise", "depthwise"]
        assert not touched, touched
        _check_parity(out, grads, want_out, want)
    sizes = [nbytes for fn, nbytes in calls if fn.endswith("backward")]
    assert len(sizes) == 2 and 0 < sizes[0] < sizes[1], calls          # the sort scratch comes with the mode
    assert all(nbytes == 0 for fn, nbytes in calls if fn.endswith("forward")), calls


def test_non_finite_border_pixels_are_not_read():
    """Inf in the last input column.  1 x 1 kernel; the last two output columns sample a quarter pixel beyond the image, where
    the low and the high corner along the last axis lie outside: the reference reads nothing there, while a pair load
    clamped into the image fetches (column W - 2, column W - 1).  Every other sample stays left of the last column."""
    from modulated_deform_conv_amd import _capi
    case = _c("dw_inf_mdcn2d_c8_6x7", M2, 2, 8, 8, (6, 7), 1, padding=0, groups=8, seed=309)
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    W = 7
    t["offset"].zero_()
    t["offset"][:, 0] = 0.25
    t["offset"][:, 1] = 0.25
    for j in (W - 2, W - 1):
        t["offset"][:, 1, :, j] = W + 0.25 - j
    t["input"][:, :, :, W - 1] = float("inf")
    want_out, want = run_oracle(case, t, torch.float32)
    assert torch.isfinite(want_out).all() and all(torch.isfinite(v).all() for v in want.values() if v is not None)
    out, grads, paths = run_product(case, t, "depthwise")
    assert paths == ["depthwise", "depthwise"] and _capi.last_kernels() == "depthwise"
    _check_parity(out, grads, want_out, want)


def test_graph_replay():
    """One backward captured with torch.cuda.graph: one stream, plain kernel nodes, no memset, no host synchronisation."""
    from modulated_deform_conv_amd import _capi
    t, _ = _det_inputs()
    _, eager = _overwrite_run(DET_CASE, t, det=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out, g = _buffers(DET_CASE, t, float("nan"))
    with torch.cuda.stream(side), _capi.deterministic():
        run_product_into(DET_CASE, t, out, g, accumulate=False, path="depthwise")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    prev = _capi.set_path("depthwise")
    try:
        graph = torch.cuda.CUDAGraph()
        with _capi.deterministic(), torch.cuda.graph(graph):
            run_product_into(DET_CASE, t, out, g, accumulate=False)
    finally:
        _capi.set_path(prev)
    for i in range(2):
        for v in g.values():
            if v is not None:
                v.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert eager[k] is None or torch.equal(g[k], eager[k]), "replay %d: %s differs from the eager run" % (i, k)


def test_module_level():
    from modulated_deform_conv_amd import _capi
    from modulated_deform_conv_amd.modulated_deform_conv import ModulatedDeformConv2d
    case = _c("dw_module_mdcn2d_c32_9x10", M2, 2, 32, 32, (9, 10), 3, groups=32, bias=True, seed=310)
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    want_out, want = run_oracle(case, t, torch.float32)
    mod = ModulatedDeformConv2d(32, 32, 3, padding=1, groups=32, bias=True).cuda()
    with torch.no_grad():
        mod.weight.copy_(t["weight"])
        mod.bias.copy_(t["bias"])
    x, off, m = (t[k].clone().requires_grad_(True) for k in ("input", "offset", "mask"))
    prev = _capi.set_path("depthwise")
    try:
        out = mod(x, off, m)
        assert _capi.last_kernels() == "depthwise"
        out.backward(t["grad_output"])
        torch.cuda.synchronize()
    finally:
        _capi.set_path(prev)
    assert_close("output", out.detach(), want_out, TOL)
    for name, got in (("grad_input", x.grad), ("grad_offset", off.grad), ("grad_mask", m.grad), ("grad_weight", mod.weight.grad),
                      ("grad_bias", mod.bias.grad)):
        assert_close(name, got, want[name], TOL)
