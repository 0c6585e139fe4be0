"""The canonical-geometry instances of the fp32 forward and GEMM-1 (mdconv_common.hpp, GeomCanon3x3): a standard DCNv2
layer -- 2-D, 3x3, stride 1, pad 1, dilation 1, one conv group, one deformable group, modulated -- runs kernel instances
with that geometry compiled in, every other call the run-time instances.  Checked here: both against the CPU oracle
(tolerances of tests/test_gpu_parity.py), bit-identity between the two (MDCONV_GEOM_FIXED is read once per process, so the
run-time build of every call runs in ONE child process: this module run as a script), and the routing.

Every run is described by a (kind, key) pair that both processes turn into the same seeded inputs."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from tests.cases import M2, _c, make_inputs
from tests.util import assert_close, run_oracle, run_product, run_product_into

pytestmark = pytest.mark.gpu

TOL = 1e-4   # tests/test_gpu_parity.py, fp32

# forward: C = 32 / 48 (the unpadded / padded-K instance), O = 160 / 256 (both take the BM = 256 tile), 81 and 296 pixels per
# image (partial last 32-pixel tiles, tiles across the image boundary); offsets N(0, 3): many samples across a border or outside
FWD = {"c%d_o%d_%dx%d" % (C, O, h, w): _c("canon_fwd_c%d_o%d_%dx%d" % (C, O, h, w), M2, 2, C, O, (h, w), 3, seed=300 + i,
                                          offset_scale=3.0)
       for i, (C, O, (h, w)) in enumerate((C, O, sz) for C in (32, 48) for O in (160, 256) for sz in ((9, 9), (8, 37)))}
# GEMM-1 <2,true,4,1,true>, the instance of the headline benchmark: 9405 pixels (channels-last drain from 8192), 9405 % 32 = 29
BWD = _c("canon_bwd_c256_o256_57x55", M2, 3, 256, 256, (57, 55), 3, seed=320, offset_scale=3.0)
# geometries that must stay on the run-time instances, all at 256 channels
ROUTING = {
    "stride2": _c("canon_rt_stride2", M2, 2, 256, 256, (11, 12), 3, stride=2, seed=330, offset_scale=3.0),
    "dil2": _c("canon_rt_dil2", M2, 2, 256, 256, (9, 10), 3, padding=2, dilation=2, seed=331, offset_scale=3.0),
    "pad0": _c("canon_rt_pad0", M2, 2, 256, 256, (9, 10), 3, padding=0, seed=332, offset_scale=3.0),
    "k1x3": _c("canon_rt_k1x3", M2, 2, 256, 256, (9, 10), (1, 3), padding=(0, 1), seed=333, offset_scale=3.0),
    "g2": _c("canon_rt_g2", M2, 2, 256, 256, (9, 10), 3, groups=2, seed=334, offset_scale=3.0),
    "dg2": _c("canon_rt_dg2", M2, 2, 256, 256, (9, 10), 3, dgroups=2, seed=335, offset_scale=3.0),
}
BWD_MODES = ("plain", "det", "acc")
GRADS = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")


def plant_non_finite(case, x):
    """Inf / NaN in image 0 next to the row ends in memory -- the last pixel of a row and the first of the next -- in the
    second and the last-but-one column, the elements a half-read corner pair brings along (make_pairs_f), and in the first
    and the last element of the tensor.  Returns the 0 / 1 indicator of the planted elements."""
    h, w = case["in_sz"]
    ind = torch.zeros_like(x)
    for c, y, col, v in ((0, 2, w - 1, "inf"), (0, 3, 0, "nan"), (1, 5, w - 1, "nan"), (1, 6, 0, "inf"),
                         (2, 4, 1, "inf"), (2, 4, w - 2, "nan"), (3, 0, 1, "nan"), (3, h - 1, w - 2, "inf")):
        x[0, c, y, col] = float(v)
        ind[0, c, y, col] = 1
    x.view(-1)[0] = float("inf")
    x.view(-1)[-1] = float("nan")
    ind.view(-1)[0] = ind.view(-1)[-1] = 1
    return ind


def inputs_of(kind, key):
    case = {"fwd": FWD, "fwdnf": FWD, "route": ROUTING}.get(kind, {}).get(key, BWD)
    t = make_inputs(case, dtype=torch.float32, device="cpu")
    ind = plant_non_finite(case, t["input"]) if kind == "fwdnf" else None
    return case, t, ind


def run_on_gpu(kind, key):
    """The product's results of run (kind, key), on the CPU, and the geometry variant(s) it reported."""
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    from modulated_deform_conv_amd import _capi
    case, t, _ = inputs_of(kind, key)
    t = {n: (None if v is None else v.cuda()) for n, v in t.items()}
    if kind in ("fwd", "fwdnf"):
        prev = _capi.set_path("mfma")
        try:
            out = M.modulated_deform_conv2d_forward_cuda(t["input"], t["weight"], t["bias"], t["offset"], t["mask"],
                                                         3, 3, 1, 1, 1, 1, 1, 1, 1, 1, case["in_step"], True)
        finally:
            _capi.set_path(prev)
        return {"output": out.cpu(), "variants": [_capi.last_kernels(), _capi.last_geometry()]}
    if kind == "route":
        out, grads, paths = run_product(case, t, "mfma")
        r = {"output": out.cpu(), "variants": [_capi.last_kernels(), _capi.last_geometry()]}
        r.update({k: grads[k].cpu() for k in GRADS})
        return r
    # GEMM-1 shape: plain = fresh zero buffers; det = deterministic mode; acc = seeded non-zero buffers going in
    if key == "acc":
        g = torch.Generator().manual_seed(77)
        shapes = dict(grad_input=t["input"], grad_offset=t["offset"], grad_mask=t["mask"], grad_weight=t["weight"],
                      grad_bias=t["bias"])
        grads = {k: torch.randn(v.shape, generator=g).cuda() for k, v in shapes.items()}
        out = torch.empty_like(t["grad_output"])
        run_product_into(case, t, out, grads, accumulate=True, path="mfma")
    else:
        with _capi.deterministic(key == "det"):
            out, grads, _ = run_product(case, t, "mfma")
    r = {"output": out.cpu(), "variants": [_capi.last_kernels(), _capi.last_geometry()]}
    r.update({k: grads[k].cpu() for k in GRADS})
    return r


ALL_RUNS = ([("fwd", k) for k in FWD] + [("fwdnf", k) for k in FWD] + [("bwd", m) for m in BWD_MODES])


@pytest.fixture(scope="module")
def runtime_build():
    """Every run of ALL_RUNS with MDCONV_GEOM_FIXED=0, from one child process; its MDCONV_DEBUG_PLAN lines as 'stderr'."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "runtime.pt")
        env = dict(os.environ, MDCONV_GEOM_FIXED="0", MDCONV_DEBUG_PLAN="1")
        r = subprocess.run([sys.executable, "-m", "tests.test_gpu_canonical_instances", path], cwd=root, env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        res = torch.load(path)
    res["stderr"] = r.stderr
    return res


_oracles = {}


def oracle_of(kind, key):
    if (kind, key) not in _oracles:
        case, t, ind = inputs_of(kind, "plain" if kind == "bwd" else key)
        _oracles[(kind, key)] = run_oracle(case, t, torch.float32) + (ind,)
    return _oracles[(kind, key)]


def assert_same_bits(name, a, b):
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), \
        "%s differs between the canonical and the run-time instances" % name


@pytest.mark.parametrize("key", list(FWD))
def test_forward_matches_the_oracle_and_the_runtime_instance(key, runtime_build):
    got = run_on_gpu("fwd", key)
    assert got["variants"] == ["f32", "canon3x3"]
    assert runtime_build["fwd/" + key]["variants"] == ["f32", "runtime"]
    want_out, _, _ = oracle_of("fwd", key)
    assert_close("output", got["output"], want_out, TOL)
    assert_same_bits("output", got["output"], runtime_build["fwd/" + key]["output"])


@pytest.mark.parametrize("key", list(FWD))
def test_forward_with_non_finite_neighbours(key, runtime_build):
    """Inf / NaN beside the row ends: an element that only comes along with a half-read corner pair must not reach the
    result (0 * Inf = NaN), one that the reference reads must -- the results are the oracle's, non-finite positions included,
    from both instances."""
    case, t, ind = inputs_of("fwdnf", key)
    want_out, _, _ = oracle_of("fwdnf", key)
    # the oracle itself: finite wherever no planted element is read (read = positive total weight on the indicator image)
    import oracle
    args = (case["stride"], case["padding"], case["dilation"], case["groups"], case["dgroups"], case["in_step"])
    touched = oracle.forward(M2, ind, torch.ones_like(t["weight"]), None, t["offset"], torch.ones_like(t["mask"]), *args,
                             dtype=torch.float32)
    fin = torch.isfinite(want_out)
    assert fin[touched == 0].all() and fin.any() and not fin.all()
    for res in (run_on_gpu("fwdnf", key), runtime_build["fwdnf/" + key]):
        out = res["output"]
        assert torch.equal(torch.isfinite(out), fin), "%s: non-finite positions differ from the oracle's" % res["variants"][1]
        assert torch.equal(torch.isnan(out), torch.isnan(want_out))
        assert_close("output", torch.where(fin, out, torch.zeros_like(out)), torch.where(fin, want_out, torch.zeros_like(out)), TOL)
        assert torch.equal(out[~fin & ~torch.isnan(out)], want_out[~fin & ~torch.isnan(out)])   # the sign of an infinity
    assert_same_bits("output", torch.nan_to_num(run_on_gpu("fwdnf", key)["output"]),
                     torch.nan_to_num(runtime_build["fwdnf/" + key]["output"]))


@pytest.mark.parametrize("mode", BWD_MODES)
def test_gemm1_of_the_benchmark_instance(mode, runtime_build):
    """C = O = 256, 57x55, B = 3: GEMM-1 <2,true,4,1,true> (the child's plan line names the instance; the geometry policy is
    the only difference between the two processes).  All five gradients against the oracle; grad_offset / grad_mask /
    grad_weight / grad_bias bit-identical between the instances, grad_input bit-identical in deterministic mode and
    within the parity tolerance otherwise (the order inside its scatter lists is the atomics' arrival order)."""
    assert "GEMM-1 instance <2,1,4,1,1>, geometry: run-time" in runtime_build["stderr"]
    assert "geometry: canonical" not in runtime_build["stderr"]
    got, rt = run_on_gpu("bwd", mode), runtime_build["bwd/" + mode]
    assert got["variants"] == ["f32", "canon3x3"] and rt["variants"] == ["f32", "runtime"]
    want_out, want, _ = oracle_of("bwd", "plain")
    assert_close("output", got["output"], want_out, TOL)
    base = {}
    if mode == "acc":   # what the buffers held going in (run_on_gpu: the same seeded values)
        g = torch.Generator().manual_seed(77)
        for k in GRADS:
            base[k] = torch.randn(want[k].shape, generator=g)
    for k in GRADS:
        w = want[k] + base[k] if base else want[k]
        assert_close(k, got[k], w, TOL)
        assert_close(k + " (run-time)", rt[k], w, TOL)
        if k != "grad_input" or mode == "det":
            assert_same_bits(k, got[k], rt[k])
    assert_same_bits("output", got["output"], rt["output"])


@pytest.mark.parametrize("key", list(ROUTING))
def test_other_geometries_stay_on_the_runtime_instances(key):
    got = run_on_gpu("route", key)
    assert got["variants"] == ["f32", "runtime"]
    want_out, want, _ = oracle_of("route", key)
    assert_close("output", got["output"], want_out, TOL)
    for k in GRADS:
        assert_close(k, got[k], want[k], TOL)


if __name__ == "__main__":   # the child process of `runtime_build`
    torch.save({"%s/%s" % run: run_on_gpu(*run) for run in ALL_RUNS}, sys.argv[1])
