"""Step time (forward + backward) of the DCNv3 core operator (include/mdconv.h, "DCNv3 core operator"; csrc/dcn3_*.hip on csrc/samp_core.hpp)
against the composed route through the existing entry points of the same build: permute to NCHW, the depthwise modulated
2-D call with a weight of ones (groups = C, deformable_groups = G, weight gradients skipped), permute back.

    python tools/bench_dcnv3.py [--reps 5] [--rounds 5] [--dtypes float32,float16,bfloat16] [--shapes 0,1,...] [--write FILE]

Per (shape, dtype) the two routes are timed interleaved in one process: `rounds` measurements of `reps` steps each, median
with min and max.  The native forward, the native backward without grad_input (the coordinate-gradient kernel alone) and the
full native backward are timed the same way, so the list build + gather is their difference.  The composed route's kernel
family comes from mdconv_planned_kernels.  One JSON line per measurement; --write FILE writes the table as markdown."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from modulated_deform_conv_amd import MDCONV_CUDA as M
from modulated_deform_conv_amd import _capi, dcnv3

SPREAD = 0.05   # box spread the project quotes for same-box comparisons
B, KSZ = 8, 3
# (H = W, G, D, offset_scale)
SHAPES = [(56, 4, 16, 1.0), (28, 8, 16, 1.0), (14, 16, 16, 1.0), (7, 32, 16, 1.0), (56, 4, 16, 2.0)]

NOTES = [
    "## Kernel resources (`tools/kres.py dcn3_host | samp_gather | csr_sort`)", "",
    "No kernel of the family uses scratch or AGPRs; none but the scan uses LDS.  VGPRs (fp32 / fp16 / bf16 instance of the "
    "sampling core's kernels under `Dcn3Op`): `samp_fwd_kernel` 54 / 58 / 60 (8 waves per SIMD); `samp_bwd_coord_kernel` "
    "76 / 83 / 91 (6 / 5 / 5 waves); `samp_list_kernel` 12 / 11 / 11 counting, 24 filling; `samp_gather_kernel` 28 / 40 / 36; "
    "`lists_scan_kernel` 44 with the 144 bytes of LDS of `csr_scan_chunk`.", "",
]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def make(shape, dtype):
    hw, G, D, scale = shape
    gen = torch.Generator().manual_seed(1)
    K = KSZ * KSZ
    x = torch.randn(B, hw, hw, G * D, generator=gen).to(dtype).cuda()
    off = ((torch.rand(B, hw, hw, G * K * 2, generator=gen) * 2 - 1) * 1.5).to(dtype).cuda()
    m = torch.rand(B, hw, hw, G * K, generator=gen).to(dtype).cuda()
    go = torch.randn(B, hw, hw, G * D, generator=gen).to(dtype).cuda()
    return x, off, m, go, (KSZ, 1, 1, 1, G, D, scale)


def composed(x, off, m, go, geo):
    """The step through the existing entry points, and the descriptor of its call.  The offsets are taken as they are (the
    affine remap of tests/dcnv3_ref.dcnv3_oracle moves positions, not work); every layout change is part of the step."""
    k, s, p, d, G, D, _ = geo
    C = G * D
    w = torch.ones(C, 1, k, k, dtype=x.dtype, device=x.device)
    bias = x.new_empty(0)
    tail = (k, k, s, s, p, p, d, d, C, G, 64, False)

    def step():
        xn = x.permute(0, 3, 1, 2).contiguous()
        on = off.permute(0, 3, 1, 2).contiguous()
        mn = m.permute(0, 3, 1, 2).contiguous()
        out = M.modulated_deform_conv2d_forward_cuda(xn, w, bias, on, mn, *tail).permute(0, 2, 3, 1).contiguous()
        gon = go.permute(0, 3, 1, 2).contiguous()
        with _capi.skip_grads(weight=True):
            gi, goff, gm, _, _ = M.modulated_deform_conv2d_backward_cuda(xn, w, bias, on, mn, gon, *tail)
        return out, gi.permute(0, 2, 3, 1).contiguous(), goff.permute(0, 2, 3, 1).contiguous(), gm.permute(0, 2, 3, 1).contiguous()

    desc = M._desc(2, True, x.permute(0, 3, 1, 2).contiguous(), w, (k, k), (s, s), (p, p), (d, d), C, G, 64, False)
    fams = tuple(_capi.KERNELS[_capi.lib().mdconv_planned_kernels(ctypes.byref(desc), b)] for b in (0, 1))
    return step, fams


def measure(shape, dtype, reps, rounds):
    x, off, m, go, geo = make(shape, dtype)
    comp, fams = composed(x, off, m, go, geo)
    steps = {
        "native": lambda: (dcnv3.dcnv3_forward(x, off, m, *geo), dcnv3.dcnv3_backward(x, off, m, go, *geo)),
        "composed": comp,
        "native_fwd": lambda: dcnv3.dcnv3_forward(x, off, m, *geo),
        "native_bwd": lambda: dcnv3.dcnv3_backward(x, off, m, go, *geo),
        "native_bwd_no_grad_input": lambda: dcnv3.dcnv3_backward(x, off, m, go, *geo, need_grad_input=False),
    }
    for step in steps.values():
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ms = {r: [] for r in steps}
    for _ in range(rounds):
        for r, step in steps.items():
            ms[r].append(timed(step, reps))
    return {r: (statistics.median(v), min(v), max(v)) for r, v in ms.items()}, fams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtypes", default="float32,float16,bfloat16")
    ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))))
    ap.add_argument("--commit", default="")
    ap.add_argument("--write")
    a = ap.parse_args()
    rows = []
    for i in (int(s) for s in a.shapes.split(",")):
        for dtype in (getattr(torch, n) for n in a.dtypes.split(",")):
            shape = SHAPES[i]
            res, fams = measure(shape, dtype, a.reps, a.rounds)
            name = "%dx%dx%d_g%d_s%g_%s" % (shape[0], shape[0], shape[1] * shape[2], shape[1], shape[3], str(dtype).split(".")[1])
            for r, (med, lo, hi) in res.items():
                print(json.dumps(dict(shape=name, route=r, composed_kernels=fams, median_ms=round(med, 4), min_ms=round(lo, 4),
                                      max_ms=round(hi, 4))), flush=True)
            rows.append((name, shape, dtype, res, fams))
            torch.cuda.empty_cache()
    if a.write:
        write_markdown(a.write, rows, a)


def write_markdown(path, rows, a):
    out = ["# DCNv3 core operator: step times against the composed route", "",
           "Written by `tools/bench_dcnv3.py --write` (forward + backward, B = %d, %d x %d kernel, stride 1, pad 1; median of %d rounds of "
           "%d steps, the routes interleaved in one process).  Box: %s.  Commit: %s." % (
               B, KSZ, KSZ, a.rounds, a.reps, torch.cuda.get_device_name(0), a.commit or "(not given)"), "",
           "`composed`: permute to NCHW, the depthwise modulated 2-D call of the same build with a weight of ones and the weight "
           "gradients skipped, permute back; `composed kernels` is `mdconv_planned_kernels` of that call (forward / backward).  "
           "`coord` is the native backward with `MDCONV_FLAG_NO_GRAD_INPUT` (the coordinate-gradient kernel alone), `lists + gather` "
           "the full backward minus it.  `fwd GB/s`: the 16-byte corner vectors the forward asks for (4 x K x B x Ho x Wo x C elements) "
           "per second -- a request rate, neighbouring taps share lines.", "",
           "| shape | composed kernels | native ms (min - max) | composed ms (min - max) | composed / native | fwd ms | coord ms | lists + gather ms | fwd GB/s |",
           "|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for name, shape, dtype, res, fams in rows:
        nat, comp = res["native"], res["composed"]
        hw, G, D, _ = shape
        esz = 4 if dtype == torch.float32 else 2
        gathered = 4 * KSZ * KSZ * B * hw * hw * G * D * esz
        fwd = res["native_fwd"][0]
        out.append("| %s | %s / %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %.3f | %.3f | %.3f | %.0f |" % (
            name, fams[0], fams[1], nat[0], nat[1], nat[2], comp[0], comp[1], comp[2], comp[0] / nat[0], fwd,
            res["native_bwd_no_grad_input"][0], res["native_bwd"][0] - res["native_bwd_no_grad_input"][0], gathered / fwd / 1e6))
        faster = nat[0] * (1 + SPREAD) < comp[0]
        verdicts.append("%s: the native operator is %s the composed route beyond the spread: %.3f vs %.3f ms" % (
            name, "FASTER than" if faster else "NOT FASTER than", nat[0], comp[0]))
    out += ["", "Spread quoted by the project for same-box comparisons: %d %%." % round(SPREAD * 100), ""] + ["- " + v for v in verdicts] + [""]
    out += NOTES
    with open(path, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
