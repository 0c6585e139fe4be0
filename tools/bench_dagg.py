"""Step time (forward + backward) of deformable aggregation (include/mdconv_dagg.h; csrc/dagg_*.hip) against the composed
route of plain PyTorch: one `F.grid_sample` per (camera, level), times the gate and the group weights, summed -- what a
Sparse4D-style model runs without the extension -- and its autograd backward.

    python tools/bench_dagg.py [--reps 5] [--rounds 5] [--modes float32,bfloat16,bfloat16+float32] [--shapes 0,1,2]
                               [--limit 300] [--trace-csv FILE] [--write FILE]
    python tools/bench_dagg.py --trace-steps 20 --worker-shape 0 --worker-mode float32     (under a kernel tracer)

A mode is the value dtype, `+float32` for fp32 coordinate tensors beside 16-bit values.  Per (shape, mode) the two routes
are timed interleaved in one process: `rounds` measurements of `reps` steps each, median with min and max; the spread of a
line is the larger (max - min) / median of its two routes, and a line counts as faster only beyond it.  The native forward,
the native backward without grad_feature (the coordinate-gradient kernel alone) and the full native backward are timed the
same way.  Every (shape, mode) runs in a child process of its own under a time limit of `--limit` seconds; the first child
that fails or runs out of time ends the run -- nothing more is started on the GPU after it.  `--trace-steps` runs that many
native backwards and nothing else, for a kernel trace collected in a run of its own; `--trace-csv` takes the tracer's
per-kernel statistics (columns Name, Calls, TotalDurationNs) into the markdown.  One JSON line per measurement."""
import argparse
import csv
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAMS, LEVELS, C, G, P = 6, [(64, 176), (32, 88), (16, 44), (8, 22)], 256, 8, 13
# (name, B, A)
SHAPES = [("sparse4d_B1_A900", 1, 900), ("sparse4d_B4_A900", 4, 900), ("sparse4d_B1_A300", 1, 300)]
ROUTES = ("native", "composed", "native_fwd", "native_bwd", "native_bwd_no_grad_feature")
LOC_RANGE = (-0.5, 1.5)   # uniform per axis: a quarter of the (anchor, point, camera) triples pass the gate


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def make(shape, dtype, coord_dtype):
    import torch
    _, B, A = shape
    S = CAMS * sum(h * w for h, w in LEVELS)
    L = len(LEVELS)
    gen = torch.Generator().manual_seed(1)
    feature = torch.randn(B, S, C, generator=gen).to(dtype).cuda()
    lo, hi = LOC_RANGE
    loc = (torch.rand(B, A, P, CAMS, 2, generator=gen) * (hi - lo) + lo).to(coord_dtype).cuda()
    weights = torch.softmax(torch.randn(B, A, P * CAMS * L, G, generator=gen), 2).view(B, A, P, CAMS, L, G).to(coord_dtype).cuda()
    go = torch.randn(B, A, C, generator=gen).to(dtype).cuda()
    return feature, loc, weights, go


def composed(feature, loc, weights, go):
    """The step of the pure-PyTorch fallback in the tensors' own dtypes (coordinates cast to the value dtype, as grid_sample
    needs one dtype): forward, then autograd for the three gradients."""
    import torch
    import torch.nn.functional as F
    B, S, Cc = feature.shape
    s_cam = S // CAMS
    starts, s = [], 0
    for h, w in LEVELS:
        starts.append(s)
        s += h * w

    def forward(f, lc, wt):
        gate = ((lc > 0) & (lc < 1)).all(-1)                      # [B, A, P, cams]
        grids = (2 * lc - 1).to(f.dtype)
        wt = torch.where(gate[..., None, None], wt, torch.zeros_like(wt)).to(f.dtype)
        out = 0
        for cam in range(CAMS):
            grid = grids[:, :, :, cam]
            for l, (h, w) in enumerate(LEVELS):
                r0 = cam * s_cam + starts[l]
                img = f[:, r0:r0 + h * w].transpose(1, 2).reshape(B, Cc, h, w)
                smp = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)   # [B, C, A, P]
                wg = wt[:, :, :, cam, l].permute(0, 3, 1, 2)                                                 # [B, G, A, P]
                out = out + (smp.view(B, G, Cc // G, *smp.shape[2:]) * wg[:, :, None]).sum(-1)
        return out.flatten(1, 2).transpose(1, 2).contiguous()

    def step():
        f, lc, wt = (x.detach().requires_grad_(True) for x in (feature, loc, weights))
        o = forward(f, lc, wt)
        return (o,) + torch.autograd.grad(o, (f, lc, wt), go)

    return step


def mode_dtypes(mode):
    import torch
    dtype = getattr(torch, mode.split("+")[0])
    return dtype, (getattr(torch, mode.split("+")[1]) if "+" in mode else dtype)


def worker(a):
    """One (shape, mode) in this process: JSON lines, one per route, then one with the box's name."""
    import ctypes

    import torch
    from modulated_deform_conv_amd import _capi, dagg
    shape = SHAPES[a.worker_shape]
    dtype, coord_dtype = mode_dtypes(a.worker_mode)
    feature, loc, weights, go = make(shape, dtype, coord_dtype)
    if a.trace_steps:
        for _ in range(a.trace_steps):
            dagg.deformable_aggregation_backward(feature, LEVELS, loc, weights, go)
        torch.cuda.synchronize()
        return
    steps = {
        "native": lambda: (dagg.deformable_aggregation_forward(feature, LEVELS, loc, weights),
                           dagg.deformable_aggregation_backward(feature, LEVELS, loc, weights, go)),
        "composed": composed(feature, loc, weights, go),
        "native_fwd": lambda: dagg.deformable_aggregation_forward(feature, LEVELS, loc, weights),
        "native_bwd": lambda: dagg.deformable_aggregation_backward(feature, LEVELS, loc, weights, go),
        "native_bwd_no_grad_feature": lambda: dagg.deformable_aggregation_backward(feature, LEVELS, loc, weights, go,
                                                                                 need_grad_feature=False),
    }
    for step in steps.values():
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ms = {r: [] for r in steps}
    for _ in range(a.rounds):
        for r, step in steps.items():
            ms[r].append(timed(step, a.reps))
    d = dagg._desc(feature, loc, weights, dagg._shapes(LEVELS))
    ws = int(_capi.lib().mdconv_dagg_workspace_bytes(ctypes.byref(d), 1))
    gated = float(((loc > 0) & (loc < 1)).all(-1).float().mean())
    name = "%s_%s" % (shape[0], a.worker_mode.replace("float", "f"))
    for r in ROUTES:
        v = ms[r]
        print(json.dumps(dict(shape=name, route=r, workspace_bytes=ws, gated_in=round(gated, 4),
                              median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))),
              flush=True)
    print(json.dumps(dict(box=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--modes", default="float32,bfloat16,bfloat16+float32")
    ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))))
    ap.add_argument("--limit", type=int, default=300, help="seconds each (shape, mode) may take")
    ap.add_argument("--commit", default="")
    ap.add_argument("--write")
    ap.add_argument("--trace-csv", help="per-kernel statistics of a trace of `--trace-steps` (Name, Calls, TotalDurationNs)")
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--worker-shape", type=int)
    ap.add_argument("--worker-mode")
    a = ap.parse_args()
    if a.worker_mode is not None:
        return worker(a)
    rows, box = [], "(unknown)"
    for i in (int(s) for s in a.shapes.split(",")):
        for mode in a.modes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--rounds", str(a.rounds),
                   "--worker-shape", str(i), "--worker-mode", mode]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                sys.exit("%s %s: no result within %d s; nothing more is started" % (SHAPES[i][0], mode, a.limit))
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit("%s %s: the measurement failed (exit %d); nothing more is started" % (SHAPES[i][0], mode, r.returncode))
            res, ws, name, gated = {}, 0, None, 0.0
            for line in r.stdout.splitlines():
                if not line.startswith("{"):
                    continue
                j = json.loads(line)
                if "box" in j:
                    box = j["box"]
                    continue
                print(line, flush=True)
                res[j["route"]] = (j["median_ms"], j["min_ms"], j["max_ms"])
                ws, name, gated = j["workspace_bytes"], j["shape"], j["gated_in"]
            rows.append((name, mode, res, ws, gated))
    if a.write:
        write_markdown(a.write, rows, a, box)


def trace_table(path):
    """The native backward's kernels from a tracer's per-kernel statistics: name, calls, total and per-call time."""
    with open(path, newline="") as f:
        recs = [r for r in csv.DictReader(f)]
    # the project's own kernels by name (a process under the tracer may have run framework fill kernels as well)
    own = re.compile(r"\bmdconv::(?:\(anonymous namespace\)::)?(?:dagg_\w+_kernel|lists_scan_kernel|zero_words_kernel|csr_sort_rows_kernel)\b")
    keep = [r for r in recs if own.search(r["Name"])]
    total = sum(float(r["TotalDurationNs"]) for r in keep) or 1.0
    out = ["| kernel | calls | total ms | per call us | share |", "|---|---|---|---|---|"]
    for r in sorted(keep, key=lambda r: -float(r["TotalDurationNs"])):
        t, n = float(r["TotalDurationNs"]), int(r["Calls"])
        short = re.search(r"(\w+_kernel(?:<[^>]*>)?)", r["Name"])
        out.append("| `%s` | %d | %.3f | %.1f | %.0f %% |" % (short.group(1) if short else r["Name"][:60], n, t / 1e6, t / n / 1e3,
                                                             100 * t / total))
    return out


def write_markdown(path, rows, a, box):
    lo, hi = LOC_RANGE
    out = ["# Deformable aggregation: step times against the composed route", "",
           "Written by `tools/bench_dagg.py --write` (forward + backward; median of %d rounds of %d steps, the routes "
           "interleaved in one process, one process per line).  Box: %s.  Commit: %s." % (a.rounds, a.reps, box, a.commit or "(not given)"), "",
           "Shape: the Sparse4D setup -- %d cameras, levels %s, C = %d in G = %d groups, P = %d key points; B images of A anchors.  "
           "Locations are uniform in [%.1f, %.1f] per axis, so a quarter of the (anchor, point, camera) triples are drawn to pass "
           "the gate; `gated in` is the fraction the tensors hold." % (CAMS, ", ".join("%dx%d" % s for s in LEVELS), C, G, P, lo, hi), "",
           "`composed`: the pure-PyTorch fallback -- one `F.grid_sample` per (camera, level), times the gate and the group "
           "weights, summed -- and its autograd backward, in the value dtype.  `coord` is the native backward with "
           "`MDCONV_FLAG_NO_GRAD_INPUT` (the coordinate-gradient kernel alone), `lists + gather` the full backward minus it.  "
           "`spread` is the larger (max - min) / median of the two routes of the line, measured by this run.  `f32` / `bf16` is "
           "the value dtype; `+f32`: fp32 coordinate tensors.", "",
           "| shape | gated in | native ms (min - max) | composed ms (min - max) | composed / native | spread | fwd ms | coord ms | lists + gather ms | workspace MiB |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for name, mode, res, ws, gated in rows:
        nat, comp = res["native"], res["composed"]
        spread = max((nat[2] - nat[1]) / nat[0], (comp[2] - comp[1]) / comp[0])
        out.append("| %s | %.3f | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %.1f %% | %.3f | %.3f | %.3f | %.1f |" % (
            name, gated, nat[0], nat[1], nat[2], comp[0], comp[1], comp[2], comp[0] / nat[0], 100 * spread, res["native_fwd"][0],
            res["native_bwd_no_grad_feature"][0], res["native_bwd"][0] - res["native_bwd_no_grad_feature"][0], ws / 2.0 ** 20))
        faster = nat[0] * (1 + spread) < comp[0]
        verdicts.append("%s: the native operator is %s the composed route beyond the measured spread (%.1f %%): %.3f vs %.3f ms" % (
            name, "FASTER than" if faster else "NOT FASTER than", 100 * spread, nat[0], comp[0]))
    out += [""] + ["- " + v for v in verdicts] + [""]
    if a.trace_csv:
        out += ["## Kernel trace of the native backward", "",
                "One kernel trace of `--trace-steps` backwards of %s in fp32, collected in a run of its own (the counting and the "
                "filling pass of the list build are the two instances of `dagg_list_kernel`):" % SHAPES[0][0], ""]
        out += trace_table(a.trace_csv) + [""]
    with open(path, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
