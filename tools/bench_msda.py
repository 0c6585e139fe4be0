"""Step time (forward + backward) of multi-scale deformable attention (include/mdconv.h, "Multi-scale deformable
attention"; csrc/msda_*.hip on csrc/samp_core.hpp) against the composed route of plain PyTorch: one `F.grid_sample` per level with the permutes
around it, times the attention weights, summed -- the fallback a model uses without the extension -- and its autograd
backward.

    python tools/bench_msda.py [--reps 5] [--rounds 5] [--modes float32,bfloat16,bfloat16+float32] [--shapes 0,1,2] [--write FILE]

A mode is the value dtype, `+float32` for fp32 coordinate tensors beside 16-bit values.  Per (shape, mode) the two routes
are timed interleaved in one process: `rounds` measurements of `reps` steps each, median with min and max.  The native
forward, the native backward without grad_value (the coordinate-gradient kernel alone) and the full native backward are
timed the same way, so the list build + gather is their difference.  One JSON line per measurement; --write FILE writes the
table as markdown."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from modulated_deform_conv_amd import _capi, msda

SPREAD = 0.05   # box spread the project quotes for same-box comparisons
N, M, D, P = 2, 8, 32, 4
PYRAMID = [(64, 64), (32, 32), (16, 16), (8, 8)]
# (name, levels, Lq; None: one query per value row)
SHAPES = [("encoder", PYRAMID, None), ("decoder", PYRAMID, 300), ("pixel_decoder", [(32, 32), (16, 16), (8, 8)], None)]

NOTES = [
    "## Kernel resources (`tools/kres.py msda_host | samp_gather | csr_sort`)", "",
    "No kernel of the family uses scratch or AGPRs -- the level table is read through an unrolled select chain over constant "
    "indices of the kernel argument -- and none but the scan uses LDS.  VGPRs (value / coordinate type: fp32 / fp32, fp16 / fp16, "
    "fp16 / fp32, bf16 / bf16, bf16 / fp32; the sampling core's kernels under `MsdaOp`): `samp_fwd_kernel` 48 / 72 / 72 / 54 / 54 (8 / 7 / 7 / 8 / 8 waves per SIMD); "
    "`samp_bwd_coord_kernel` 72 / 79 / 79 / 86 / 95 (7 / 6 / 6 / 5 / 5 waves); `samp_list_kernel` (by coordinate type, fp32 / "
    "fp16 / bf16) 14 / 13 / 13 counting, 26 filling; `samp_gather_kernel` (by value type) 28 / 40 / 36; `lists_scan_kernel` 44 "
    "with the 144 bytes of LDS of `csr_scan_chunk`.", "",
]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def make(shape, dtype, coord_dtype):
    _, levels, Lq = shape
    S = sum(h * w for h, w in levels)
    Lq = S if Lq is None else Lq
    gen = torch.Generator().manual_seed(1)
    value = torch.randn(N, S, M, D, generator=gen).to(dtype).cuda()
    loc = (torch.rand(N, Lq, M, len(levels), P, 2, generator=gen) * 1.1 - 0.05).to(coord_dtype).cuda()
    attn = torch.softmax(torch.randn(N, Lq, M, len(levels) * P, generator=gen), -1).view(N, Lq, M, len(levels), P).to(coord_dtype).cuda()
    go = torch.randn(N, Lq, M * D, generator=gen).to(dtype).cuda()
    return value, loc, attn, go


def composed(value, levels, loc, attn, go):
    """The step of the pure-PyTorch fallback in the tensors' own dtypes (coordinates cast to the value dtype, as
    grid_sample needs one dtype): forward, then autograd for the three gradients."""
    Nn, S, Mm, Dd = value.shape
    Lq, L, Pp = loc.shape[1], loc.shape[3], loc.shape[4]
    starts, s = [], 0
    for h, w in levels:
        starts.append(s)
        s += h * w

    def forward(v, lc, at):
        grids = (2 * lc - 1).to(v.dtype)
        out = []
        for l, (h, w) in enumerate(levels):
            img = v[:, starts[l]:starts[l] + h * w].flatten(2).transpose(1, 2).reshape(Nn * Mm, Dd, h, w)
            grid = grids[:, :, :, l].transpose(1, 2).flatten(0, 1)
            out.append(F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False))
        a = at.to(v.dtype).transpose(1, 2).reshape(Nn * Mm, 1, Lq, L * Pp)
        o = (torch.stack(out, -2).flatten(-2) * a).sum(-1).view(Nn, Mm * Dd, Lq)
        return o.transpose(1, 2).contiguous()

    def step():
        v, lc, at = (t.detach().requires_grad_(True) for t in (value, loc, attn))
        o = forward(v, lc, at)
        return (o,) + torch.autograd.grad(o, (v, lc, at), go)

    return step


def measure(shape, dtype, coord_dtype, reps, rounds):
    levels = shape[1]
    value, loc, attn, go = t = make(shape, dtype, coord_dtype)
    steps = {
        "native": lambda: (msda.ms_deform_attn_forward(value, levels, loc, attn),
                           msda.ms_deform_attn_backward(value, levels, loc, attn, go)),
        "composed": composed(value, levels, loc, attn, go),
        "native_fwd": lambda: msda.ms_deform_attn_forward(value, levels, loc, attn),
        "native_bwd": lambda: msda.ms_deform_attn_backward(value, levels, loc, attn, go),
        "native_bwd_no_grad_value": lambda: msda.ms_deform_attn_backward(value, levels, loc, attn, go, need_grad_value=False),
    }
    for step in steps.values():
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ms = {r: [] for r in steps}
    for _ in range(rounds):
        for r, step in steps.items():
            ms[r].append(timed(step, reps))
    d = msda._desc(value, loc, msda._shapes(levels))
    ws = int(_capi.lib().mdconv_msda_workspace_bytes(ctypes.byref(d), 1))
    return {r: (statistics.median(v), min(v), max(v)) for r, v in ms.items()}, ws, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--modes", default="float32,bfloat16,bfloat16+float32")
    ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))))
    ap.add_argument("--commit", default="")
    ap.add_argument("--write")
    a = ap.parse_args()
    rows = []
    for i in (int(s) for s in a.shapes.split(",")):
        for mode in a.modes.split(","):
            dtype = getattr(torch, mode.split("+")[0])
            coord_dtype = getattr(torch, mode.split("+")[1]) if "+" in mode else dtype
            shape = SHAPES[i]
            res, ws, t = measure(shape, dtype, coord_dtype, a.reps, a.rounds)
            name = "%s_L%d_Lq%d_%s" % (shape[0], len(shape[1]), t[1].shape[1], mode.replace("float", "f"))
            for r, (med, lo, hi) in res.items():
                print(json.dumps(dict(shape=name, route=r, workspace_bytes=ws, median_ms=round(med, 4), min_ms=round(lo, 4),
                                      max_ms=round(hi, 4))), flush=True)
            rows.append((name, shape, dtype, t[1].shape[1], res, ws))
            del t
            torch.cuda.empty_cache()
    if a.write:
        write_markdown(a.write, rows, a)


def write_markdown(path, rows, a):
    out = ["# Multi-scale deformable attention: step times against the composed route", "",
           "Written by `tools/bench_msda.py --write` (forward + backward, N = %d, M = %d, D = %d, P = %d; median of %d rounds of %d "
           "steps, the routes interleaved in one process).  Box: %s.  Commit: %s." % (
               N, M, D, P, a.rounds, a.reps, torch.cuda.get_device_name(0), a.commit or "(not given)"), "",
           "`composed`: the pure-PyTorch fallback -- one `F.grid_sample` per level with the permutes around it, times the attention "
           "weights, summed -- and its autograd backward, in the value dtype.  `coord` is the native backward with "
           "`MDCONV_FLAG_NO_GRAD_INPUT` (the coordinate-gradient kernel alone), `lists + gather` the full backward minus it.  "
           "`fwd GB/s`: the 16-byte corner vectors the forward asks for (4 x L x P x N x Lq x M x D elements) per second -- a request "
           "rate, neighbouring samples share lines.  `f32` / `bf16` is the value dtype; `+f32`: fp32 coordinate tensors.", "",
           "| shape | native ms (min - max) | composed ms (min - max) | composed / native | fwd ms | coord ms | lists + gather ms | workspace MiB | fwd GB/s |",
           "|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for name, shape, dtype, Lq, res, ws in rows:
        nat, comp = res["native"], res["composed"]
        esz = 4 if dtype == torch.float32 else 2
        gathered = 4 * len(shape[1]) * P * N * Lq * M * D * esz
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
