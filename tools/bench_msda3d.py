"""Step time (forward + backward) of 3-D multi-scale deformable attention (include/mdconv.h, "3-D multi-scale deformable
attention"; csrc/msda3_*.hip) against the composed route of plain PyTorch: one `F.grid_sample` on 5-D tensors per level with
the permutes around it, times the attention weights, summed -- the fallback a volumetric or video model uses without the
extension -- and its autograd backward.

    python tools/bench_msda3d.py [--reps 5] [--rounds 5] [--modes float32,bfloat16,bfloat16+float32] [--shapes 0,1,2,3]
                                 [--limit 300] [--write FILE]

A mode is the value dtype, `+float32` for fp32 coordinate tensors beside 16-bit values.  Per (shape, mode) the two routes
are timed interleaved in one process: `rounds` measurements of `reps` steps each, median with min and max.  The native
forward, the native backward without grad_value (the coordinate-gradient kernel alone) and the full native backward are
timed the same way, so the list build + gather is their difference.  Every (shape, mode) runs in a child process of its own
under a time limit of `--limit` seconds; the first child that fails or runs out of time ends the run -- nothing more is
started on the GPU after it.  One JSON line per measurement; --write FILE writes the table as markdown."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPREAD = 0.05   # box spread the project quotes for same-box comparisons
N, P = 2, 4
VOLUME = [(12, 24, 24), (6, 12, 12), (3, 6, 6)]
VIDEO = [(8, 32, 32), (8, 16, 16), (8, 8, 8)]
# (name, levels, M, D, Lq; None: one query per value row)
SHAPES = [("volume_encoder", VOLUME, 6, 64, None), ("video_encoder", VIDEO, 8, 32, None),
          ("volume_decoder", VOLUME, 6, 64, 300), ("video_decoder", VIDEO, 8, 32, 300)]
ROUTES = ("native", "composed", "native_fwd", "native_bwd", "native_bwd_no_grad_value")

NOTES = [
    "## Where the native step goes", "",
    "At the encoder shapes the forward and the coordinate-gradient kernel take 0.08-0.13 ms each; the list build and the gather of "
    "`grad_value` (`lists + gather`) take 2.0-3.4 ms, 93-95 % of the step, in every mode -- they work on 16-byte entries and do not depend "
    "on the value type.  The coarsest level holds 108 (volume) or 512 (video) of the rows and takes a third of all samples, so its lists "
    "are thousands of entries long and its counters are contended.  One kernel trace of the volume encoder in fp32 (`rocprofv3 --kernel-trace --stats`, a run of its own), per backward: `msda3_list_kernel` counting 1.13 ms and filling 1.21 ms (integer atomics on the row counters), `samp_gather_kernel` 0.97 ms, `msda3_bwd_coord_kernel` 0.127 ms, the scan and the zeroing 0.005 ms each; `msda3_fwd_kernel` 0.095 ms.  "
    "A backward with `MDCONV_FLAG_NO_GRAD_INPUT` is the `coord` column alone.", "",
    "## Kernel resources (`tools/kres.py msda3_fwd | msda3_bwd | msda3_list`)", "",
    "No kernel of the family uses scratch, AGPRs or LDS -- the level table is read through an unrolled select chain over "
    "constant indices of the kernel argument.  By (value type / coordinate type):", "",
    "| kernel | fp32 / fp32 | fp16 / fp16 | fp16 / fp32 | bf16 / bf16 | bf16 / fp32 |",
    "|---|---|---|---|---|---|",
    "| `msda3_fwd_kernel` VGPRs (waves per SIMD) | 76 (6) | 78 (6) | 78 (6) | 82 (5) | 82 (5) |",
    "| `msda3_bwd_coord_kernel` VGPRs (waves per SIMD) | 122 (4) | 126 (4) | 126 (4) | 160 (3) | 159 (3) |", "",
    "`msda3_list_kernel` (by coordinate type, fp32 / fp16 / bf16): 20 / 20 / 21 VGPRs counting, 35 / 34 / 32 filling, 8 waves "
    "per SIMD.  SGPRs: 78 - 79 (forward), 92 - 94 (coordinate backward), 36 / 40 (lists).  The gather (`samp_gather_kernel`), the "
    "scan and the sort are the sampling operators' own, unchanged.", "",
    "The tap state a pair's lanes broadcast is eight words -- three fractions, the attention weight, the byte offset of the low "
    "neighbour, the mask of the corners read and the level's two byte strides -- that is eight wave shuffles per tap where "
    "eight offsets, three fractions and the factor would be twelve; a corner's offset costs three selected adds and one select "
    "on the mask instead.  The bf16 instances carry the widening of eight corner vectors (64 values) beside the sums, which is "
    "where their registers go.", "",
    "Every existing instance of the sampling family (`samp_*` under `Dcn3Op`, `MsdaOp`, `Dcn4Op`, `FdaOp`, `Dcn4SoftOp`) and of "
    "the RoI family (`droi_*`) keeps its VGPR and SGPR counts against the parent commit: their sources (`samp_core.hpp`, "
    "`samp_gather.hip`, `csr_sort.hip`, `*_plan.hpp`, `droi_*.hip`) are untouched, and this family includes the core's header "
    "without instantiating any of its kernel templates.", "",
]


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rows_of(levels):
    return sum(t * h * w for t, h, w in levels)


def make(shape, dtype, coord_dtype):
    import torch
    _, levels, M, D, Lq = shape
    S = rows_of(levels)
    Lq = S if Lq is None else Lq
    L = len(levels)
    gen = torch.Generator().manual_seed(1)
    value = torch.randn(N, S, M, D, generator=gen).to(dtype).cuda()
    loc = (torch.rand(N, Lq, M, L, P, 3, generator=gen) * 1.1 - 0.05).to(coord_dtype).cuda()
    attn = torch.softmax(torch.randn(N, Lq, M, L * P, generator=gen), -1).view(N, Lq, M, L, P).to(coord_dtype).cuda()
    go = torch.randn(N, Lq, M * D, generator=gen).to(dtype).cuda()
    return value, loc, attn, go


def composed(value, levels, loc, attn, go):
    """The step of the pure-PyTorch fallback in the tensors' own dtypes (coordinates cast to the value dtype, as
    grid_sample needs one dtype): forward, then autograd for the three gradients."""
    import torch
    import torch.nn.functional as F
    Nn, S, Mm, Dd = value.shape
    Lq, L, Pp = loc.shape[1], loc.shape[3], loc.shape[4]
    starts, s = [], 0
    for t, h, w in levels:
        starts.append(s)
        s += t * h * w

    def forward(v, lc, at):
        grids = (2 * lc - 1).to(v.dtype)
        out = []
        for l, (t, h, w) in enumerate(levels):
            vol = v[:, starts[l]:starts[l] + t * h * w].flatten(2).transpose(1, 2).reshape(Nn * Mm, Dd, t, h, w)
            grid = grids[:, :, :, l].transpose(1, 2).flatten(0, 1)[:, None]   # [N*M, 1, Lq, P, 3]
            out.append(F.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, :, 0])
        a = at.to(v.dtype).transpose(1, 2).reshape(Nn * Mm, 1, Lq, L * Pp)
        o = (torch.stack(out, -2).flatten(-2) * a).sum(-1).view(Nn, Mm * Dd, Lq)
        return o.transpose(1, 2).contiguous()

    def step():
        v, lc, at = (x.detach().requires_grad_(True) for x in (value, loc, attn))
        o = forward(v, lc, at)
        return (o,) + torch.autograd.grad(o, (v, lc, at), go)

    return step


def mode_dtypes(mode):
    import torch
    dtype = getattr(torch, mode.split("+")[0])
    return dtype, (getattr(torch, mode.split("+")[1]) if "+" in mode else dtype)


def worker(a):
    """One (shape, mode) in this process: JSON lines, one per route, then one with the box's name."""
    import torch
    from modulated_deform_conv_amd import _capi, msda3d
    shape = SHAPES[a.worker_shape]
    dtype, coord_dtype = mode_dtypes(a.worker_mode)
    levels = shape[1]
    value, loc, attn, go = make(shape, dtype, coord_dtype)
    steps = {
        "native": lambda: (msda3d.ms_deform_attn_3d_forward(value, levels, loc, attn),
                           msda3d.ms_deform_attn_3d_backward(value, levels, loc, attn, go)),
        "composed": composed(value, levels, loc, attn, go),
        "native_fwd": lambda: msda3d.ms_deform_attn_3d_forward(value, levels, loc, attn),
        "native_bwd": lambda: msda3d.ms_deform_attn_3d_backward(value, levels, loc, attn, go),
        "native_bwd_no_grad_value": lambda: msda3d.ms_deform_attn_3d_backward(value, levels, loc, attn, go, need_grad_value=False),
    }
    for step in steps.values():
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ms = {r: [] for r in steps}
    for _ in range(a.rounds):
        for r, step in steps.items():
            ms[r].append(timed(step, a.reps))
    d = msda3d._desc(value, loc, msda3d._shapes(levels))
    ws = int(_capi.lib().mdconv_msda3d_workspace_bytes(ctypes.byref(d), 1))
    name = "%s_Lq%d_%s" % (shape[0], loc.shape[1], a.worker_mode.replace("float", "f"))
    for r in ROUTES:
        v = ms[r]
        print(json.dumps(dict(shape=name, route=r, workspace_bytes=ws, median_ms=round(statistics.median(v), 4),
                              min_ms=round(min(v), 4), max_ms=round(max(v), 4))), flush=True)
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
            res, ws, name = {}, 0, None
            for line in r.stdout.splitlines():
                if not line.startswith("{"):
                    continue
                j = json.loads(line)
                if "box" in j:
                    box = j["box"]
                    continue
                print(line, flush=True)
                res[j["route"]] = (j["median_ms"], j["min_ms"], j["max_ms"])
                ws, name = j["workspace_bytes"], j["shape"]
            rows.append((name, SHAPES[i], mode, res, ws))
    if a.write:
        write_markdown(a.write, rows, a, box)


def write_markdown(path, rows, a, box):
    out = ["# 3-D multi-scale deformable attention: step times against the composed route", "",
           "Written by `tools/bench_msda3d.py --write` (forward + backward, N = %d, P = %d; median of %d rounds of %d steps, the "
           "routes interleaved in one process, one process per line).  Box: %s.  Commit: %s." % (
               N, P, a.rounds, a.reps, box, a.commit or "(not given)"), "",
           "Shapes: `volume` = levels (12, 24, 24), (6, 12, 12), (3, 6, 6) with M = 6, D = 64; `video` = levels (8, 32, 32), "
           "(8, 16, 16), (8, 8, 8) with M = 8, D = 32; an encoder has one query per value row, a decoder 300 queries.", "",
           "`composed`: the pure-PyTorch fallback -- one 5-D `F.grid_sample` per level with the permutes around it, times the "
           "attention weights, summed -- and its autograd backward, in the value dtype.  `coord` is the native backward with "
           "`MDCONV_FLAG_NO_GRAD_INPUT` (the coordinate-gradient kernel alone), `lists + gather` the full backward minus it.  "
           "`fwd GB/s`: the 16-byte corner vectors the forward asks for (8 x L x P x N x Lq x M x D elements) per second -- a request "
           "rate, neighbouring samples share lines.  `f32` / `bf16` is the value dtype; `+f32`: fp32 coordinate tensors.", "",
           "| shape | native ms (min - max) | composed ms (min - max) | composed / native | fwd ms | coord ms | lists + gather ms | workspace MiB | fwd GB/s |",
           "|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for name, shape, mode, res, ws in rows:
        nat, comp = res["native"], res["composed"]
        _, levels, M, D, Lq = shape
        Lq = rows_of(levels) if Lq is None else Lq
        esz = 4 if mode.startswith("float32") else 2
        gathered = 8 * len(levels) * P * N * Lq * M * D * esz
        fwd = res["native_fwd"][0]
        out.append("| %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %.3f | %.3f | %.3f | %.1f | %.0f |" % (
            name, nat[0], nat[1], nat[2], comp[0], comp[1], comp[2], comp[0] / nat[0], fwd,
            res["native_bwd_no_grad_value"][0], res["native_bwd"][0] - res["native_bwd_no_grad_value"][0], ws / 2.0 ** 20,
            gathered / fwd / 1e6))
        faster = nat[0] * (1 + SPREAD) < comp[0]
        verdicts.append("%s: the native operator is %s the composed route beyond the spread: %.3f vs %.3f ms" % (
            name, "FASTER than" if faster else "NOT FASTER than", nat[0], comp[0]))
    out += ["", "Spread quoted by the project for same-box comparisons: %d %%." % round(SPREAD * 100), ""] + ["- " + v for v in verdicts] + [""]
    out += NOTES
    with open(path, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
