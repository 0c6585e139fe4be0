"""Step time (forward + backward) of fp32 depthwise layers (groups == C_in) on the depthwise kernels and on the routes such
layers took before the family existed (include/mdconv.h: MDCONV_PATH_DEPTHWISE; csrc/dw_*.hip).

    python tools/bench_depthwise.py [--reps 10] [--rounds 5] [--parent-lib PATH] [--commit TEXT] [--write profiles/depthwise.md]

Per shape four routes in one process, `rounds` interleaved measurements of `reps` steps each through tests.util.run_product
(the path a training step takes, results allocated per call): "auto" (the default route), "depthwise" (MDCONV_PATH_DEPTHWISE: the family, whatever the size rule says), "mfma" (MDCONV_PATH_MFMA: the
earlier route wherever the matrix family has a plan for the layer) and "direct" (MDCONV_PATH_DIRECT: the earlier route
elsewhere).  Which of the two the earlier route was is read from mdconv_planned_kernels under MDCONV_PATH_MFMA.  The forward of
the "auto" route is timed alone as well.  One JSON line per (shape, route) with the median and the spread over the rounds.
--parent-lib PATH measures the default route of another build of the library (the parent commit's) in a child process
beside them, which confirms the yardstick; --auto-only is that child's mode.  --write FILE writes the table as markdown."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from modulated_deform_conv_amd import _capi
from tests.cases import M2, M3, _c, make_inputs
from tests.util import run_product, tup

SPREAD = 0.05   # box spread the project quotes for same-box comparisons

SHAPES = [
    _c("mdcn2d_c256_56x56_b8", M2, 8, 256, 256, (56, 56), 3, groups=256, seed=1),
    _c("mdcn2d_c64_112x112_b8", M2, 8, 64, 64, (112, 112), 3, groups=64, seed=1),
    _c("mdcn2d_c512_14x14_b8", M2, 8, 512, 512, (14, 14), 3, groups=512, seed=1),
    _c("mdcn2d_c96_28x28_b8_k7", M2, 8, 96, 96, (28, 28), 7, padding=3, groups=96, seed=1),
    _c("mdcn2d_c128_o256_28x28_b8", M2, 8, 128, 256, (28, 28), 3, groups=128, seed=1),
    _c("mdcn2d_c256_dg4_56x56_b8", M2, 8, 256, 256, (56, 56), 3, groups=256, dgroups=4, seed=1),
    _c("mdcn3d_c64_8x28x28_b2", M3, 2, 64, 64, (8, 28, 28), 3, groups=64, seed=1),
    _c("mdcn2d_c16_8x8_b1", M2, 1, 16, 16, (8, 8), 3, groups=16, seed=1),
]
# several deformable groups: the shapes behind the size rule of the default route (plan_route, mdconv_api.hip)
SHAPES += [
    _c("rule_mdcn2d_c32_dg2_56x56_b8", M2, 8, 32, 32, (56, 56), 3, groups=32, dgroups=2, seed=1),
    _c("rule_mdcn2d_c64_dg2_56x56_b8", M2, 8, 64, 64, (56, 56), 3, groups=64, dgroups=2, seed=1),
    _c("rule_mdcn2d_c64_dg4_112x112_b8", M2, 8, 64, 64, (112, 112), 3, groups=64, dgroups=4, seed=1),
    _c("rule_mdcn2d_c128_dg4_28x28_b8", M2, 8, 128, 128, (28, 28), 3, groups=128, dgroups=4, seed=1),
    _c("rule_mdcn2d_c128_dg2_56x56_b8", M2, 8, 128, 128, (56, 56), 3, groups=128, dgroups=2, seed=1),
    _c("rule_mdcn2d_c512_dg8_14x14_b8", M2, 8, 512, 512, (14, 14), 3, groups=512, dgroups=8, seed=1),
    _c("rule_mdcn2d_c512_dg2_28x28_b8", M2, 8, 512, 512, (28, 28), 3, groups=512, dgroups=2, seed=1),
    _c("rule_mdcn3d_c64_dg4_8x28x28_b2", M3, 2, 64, 64, (8, 28, 28), 3, groups=64, dgroups=4, seed=1),
    _c("rule_mdcn2d_c256_dg4_28x28_b8", M2, 8, 256, 256, (28, 28), 3, groups=256, dgroups=4, seed=1),
    _c("rule_mdcn2d_c128_dg2_56x56_b3", M2, 3, 128, 128, (56, 56), 3, groups=128, dgroups=2, seed=1),
    _c("rule_mdcn2d_c128_dg2_56x56_b2", M2, 2, 128, 128, (56, 56), 3, groups=128, dgroups=2, seed=1),
    _c("rule_mdcn2d_c256_dg4_14x14_b8", M2, 8, 256, 256, (14, 14), 3, groups=256, dgroups=4, seed=1),
    _c("rule_mdcn2d_c512_dg2_56x56_b8", M2, 8, 512, 512, (56, 56), 3, groups=512, dgroups=2, seed=1),
    _c("rule_mdcn2d_c512_dg8_56x56_b4", M2, 4, 512, 512, (56, 56), 3, groups=512, dgroups=8, seed=1),
]


# the parts of the profile that no run of this tool measures (tools/kres.py; one rocprofv3 --kernel-trace run per shape)
NOTES = [
    "## Size rule of the default route", "",
    "`rule_*` rows: layers with several deformable groups, which the earlier route ran with the shape-generic forward and the matrix "
    "backward (dense C x C GEMMs, natively tiled where `C_in / deformable_groups` is a multiple of 64).  The `depthwise ms` column is "
    "the family forced (`MDCONV_PATH_DEPTHWISE`), `parent auto ms` the earlier route.  Forced, the family loses where the groups have "
    "a multiple of 64 channels, the layer has at most 256 channels and a few thousand pixels or more (128 channels in 2 groups at "
    "6272 / 9408 / 25088 pixels, 256 in 4 groups at 6272 / 25088); it gains or ties at 1568 pixels, with 512 channels at every size "
    "measured (8 groups of 64 at 12544 pixels: 4 % behind, inside the spread) and with narrower groups at every size.  `plan_route` "
    "therefore declines, under `MDCONV_PATH_AUTO` only: `deformable_groups > 1`, `C_in / deformable_groups` a multiple of 64, "
    "`C_in <= 256` and at least 4096 output pixels; those rows show the earlier route's family in `auto kernels`, and their "
    "`auto ms` is the re-timed step.", "",
    "## Kernel resources (`tools/kres.py dw_fwd | dw_bwd | dw_gi`)", "",
    "No kernel of the family uses scratch.  VGPRs: `dw_fwd_kernel<ND, M, CS>` 58-82 (CS = 4), 84-118 (CS = 8), no LDS; "
    "`dw_bwd_coord_kernel<ND, M>` 79-96 in 2-D with 3 KB of LDS, 135-149 in 3-D with 4 KB; `dw_list_kernel` 18-34; "
    "`dw_gather_kernel<M, CS>` 24-82; `dw_reduce_rows_kernel`, `dw_weight_table_kernel` below 32; `lists_scan_kernel` (csr_sort.hip) 44.", "",
    "## Where a step goes (one kernel trace per shape, us per launch)", "",
    "| shape | forward | coordinate / weight gradients | list count + fill | gather | small kernels (scan, table, clear, row sums) |",
    "|---|---|---|---|---|---|",
    "| mdcn2d_c256_56x56_b8 | 91 | 228 | 19 + 23 | 362 | 5 each, 8 launches |",
    "| mdcn2d_c256_dg4_56x56_b8 (forced) | 91 | 294 | 67 + 75 | 376 | 5 each, 6 launches |",
    "| mdcn3d_c64_8x28x28_b2 | 106 | 255 | 70 + 75 | 517 | 5 each, 8 launches |", "",
    "The grad_input gather is the largest kernel: per list entry a lane loads CS x M grad_output values from CS x M channel planes "
    "(4-byte gathers).  A channels-last copy of grad_output would make them 16-byte loads (DESIGN.md 4.7); not built.", "",
]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def forward_only(case, t):
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    nd = len(case["in_sz"])
    k, s, p, d = (tup(case[x], nd) for x in ("k", "stride", "padding", "dilation"))
    geo = k + s + p + d + (case["groups"], case["dgroups"], case["in_step"], case["bias"])
    if case["op"] == M2:
        return lambda: M.modulated_deform_conv2d_forward_cuda(t["input"], t["weight"], t["bias"], t["offset"], t["mask"], *geo)
    out = torch.empty_like(t["grad_output"])
    return lambda: M.modulated_deform_conv3d_forward_cuda(t["input"], t["weight"], t["bias"], t["offset"], t["mask"], out, *geo)


def measure(case, routes, reps, rounds):
    """{route: (median ms, min, max, kernel family of the backward)}; "auto_fwd": the forward of the default route alone"""
    t = make_inputs(case, dtype=torch.float32, device="cuda")
    steps = {r: (lambda r=r: run_product(case, t, r)) for r in routes}
    if "auto" in routes:
        steps["auto_fwd"] = forward_only(case, t)
    fams = {}
    for r, step in steps.items():
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        fams[r] = _capi.last_kernels()
    ms = {r: [] for r in steps}
    for _ in range(rounds):
        for r, step in steps.items():
            ms[r].append(timed(step, reps))
    return {r: (statistics.median(v), min(v), max(v), fams[r]) for r, v in ms.items()}


def earlier_route(case):
    """"mfma" where the matrix family plans both directions of the layer (the route before the depthwise family), else "direct\""""
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    nd = len(case["in_sz"])
    k, s, p, d = (tup(case[x], nd) for x in ("k", "stride", "padding", "dilation"))
    x = torch.empty((case["B"], case["C"]) + case["in_sz"], device="cuda")
    w = torch.empty((case["O"], case["C"] // case["groups"]) + k, device="cuda")
    desc = M._desc(nd, True, x, w, k, s, p, d, case["groups"], case["dgroups"], case["in_step"], case["bias"])
    desc.path = _capi.PATH_MFMA
    fams = [_capi.lib().mdconv_planned_kernels(ctypes.byref(desc), b) for b in (0, 1)]
    # (the forward and the backward of one layer fall back separately: MDCONV_PATH_MFMA refuses where MDCONV_PATH_AUTO went direct)
    return "mfma" if all(fams) else ("mixed" if any(fams) else "direct"), fams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--auto-only", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--commit", default="")
    ap.add_argument("--write")
    a = ap.parse_args()
    parent = {}
    if a.parent_lib:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--auto-only", "--reps", str(a.reps), "--rounds", str(a.rounds)],
                           env=dict(os.environ, MDCONV_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, check=True)
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                j = json.loads(ln)
                if j["route"] == "auto":
                    parent[j["shape"]] = j
                    print(json.dumps(dict(j, route="parent_auto")), flush=True)
    rows = []
    for case in SHAPES:
        earlier, fams = ("?", [0, 0]) if a.auto_only else earlier_route(case)
        routes = ["auto"] if a.auto_only else ["auto", "depthwise", "direct"] + (["mfma"] if earlier == "mfma" else [])
        res = measure(case, routes, a.reps, a.rounds)
        for k, (med, lo, hi, fam) in res.items():
            print(json.dumps(dict(shape=case["name"], route=k, lib=os.path.basename(_capi.LIB_PATH), kernels=fam, earlier=earlier,
                                  median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4))), flush=True)
        rows.append((case, earlier, res, parent.get(case["name"])))
        torch.cuda.empty_cache()
    if a.write and not a.auto_only:
        write_markdown(a.write, rows, a)


def write_markdown(path, rows, a):
    box = torch.cuda.get_device_name(0)
    out = ["# Depthwise layers (groups == C_in, fp32): step times", "",
           "Written by `tools/bench_depthwise.py --write` (forward + backward through `tests.util.run_product`, median of %d rounds "
           "of %d steps, routes interleaved in one process).  Box: %s.  Commit: %s." % (a.rounds, a.reps, box, a.commit or "(not given)"), "",
           "`earlier route`: what the layer ran on before the family existed, from `mdconv_planned_kernels` under `MDCONV_PATH_MFMA` "
           "(`mfma`: the matrix family plans both directions, every group padded to 16 channels; `direct`: it plans neither; `mixed`: "
           "it plans one, and the yardstick is `parent auto`).  "
           "`parent auto` is the default route of the parent commit's build, same box, same run: it confirms the yardstick.  "
           "`fwd` is the forward of the default route alone, `fwd GB/s` its gathered bytes (K x N x C_in corner pairs of 8 bytes x "
           "2^(nd-1)) per second.", "",
           "| shape | earlier route | auto kernels | auto ms (min - max) | depthwise ms | mfma ms | direct ms | parent auto ms | earlier / auto | fwd ms | fwd GB/s |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for case, earlier, res, par in rows:
        auto = res["auto"]
        # "mixed" (one direction on each family) cannot be forced in one build: the parent build's default route is its yardstick
        yard = res[earlier][0] if earlier in res else (par["median_ms"] if earlier == "mixed" and par else res["direct"][0])
        nd = len(case["in_sz"])
        K = 1
        for v in tup(case["k"], nd):
            K *= v
        from tests.cases import out_size
        N = case["B"]
        for v in out_size(case):
            N *= v
        gathered = K * N * case["C"] * 8 * 2 ** (nd - 1)
        fwd = res["auto_fwd"][0]
        out.append("| %s | %s | %s | %.3f (%.3f - %.3f) | %.3f | %s | %.3f | %s | %.2f | %.3f | %.0f |" % (
            case["name"], earlier, auto[3], auto[0], auto[1], auto[2], res["depthwise"][0], "%.3f" % res["mfma"][0] if "mfma" in res else "-",
            res["direct"][0], "%.3f" % par["median_ms"] if par else "-", yard / auto[0], fwd, gathered / fwd / 1e6))
        verdicts.append("%s: the default route (%s) is %s the earlier route (%s) beyond the spread: %.3f vs %.3f ms" % (
            case["name"], auto[3], "NOT SLOWER than" if auto[0] <= yard * (1 + SPREAD) else "SLOWER than", earlier, auto[0], yard))
        if par:
            verdicts.append("%s: the earlier route measured here %s the parent build within the spread (%.3f vs %.3f ms)" % (
                case["name"], "equals" if abs(yard - par["median_ms"]) <= SPREAD * par["median_ms"] else "DIFFERS from", yard, par["median_ms"]))
    out += ["", "Spread quoted by the project for same-box comparisons: %d %%." % round(SPREAD * 100), ""] + ["- " + v for v in verdicts] + [""]
    prop = torch.cuda.get_device_properties(0)
    clock_khz = getattr(prop, "clock_rate", 2400000)   # (builds of torch without the field: the MI355X's 2.4 GHz)
    peak = 57.0 * prop.multi_processor_count * clock_khz * 1e3   # bytes / s: DESIGN.md 4.4, 57 B/clk/CU for line-wide gathers
    out += ["## The forward against the gather path", "",
            "DESIGN.md 4.4 measured 57 B/clk/CU for line-wide gathers: %.1f TB/s on this box (%d CUs at %.2f GHz).  The `fwd GB/s` column "
            "counts the 8-byte corner pairs the forward asks for (lane = pixel: neighbouring lanes share lines, so it is a request rate, "
            "not line traffic); the large 2-D layers reach 8-10 TB/s, i.e. %.0f-%.0f %% of that rate, the 14 x 14 / 28 x 28 layers about a "
            "third of it (35 us kernels: launch and tail)." % (peak / 1e12, prop.multi_processor_count, clock_khz / 1e6,
                                                                8e12 / peak * 100, 10e12 / peak * 100), ""]
    out += NOTES
    with open(path, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
