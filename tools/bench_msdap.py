"""Step time (forward + backward, through autograd) of multi-scale deformable attention with a point count per level
(include/mdconv_msdap.h; csrc/msdap_host.hip on csrc/samp_core.hpp) against the routes a user had before it: the per-level
``F.grid_sample`` composition the published code runs, and ``ms_deform_attn`` with every level padded to ``max(points)`` by
zero-weight taps (pad and slice included); on the equal-count lines also ``ms_deform_attn`` itself.

    python tools/bench_msdap.py [--reps 20] [--rounds 7] [--modes float32,bfloat16,bfloat16+float32] [--shapes 0,1,2,3,4]
                                [--commit TEXT] [--write FILE]

A mode is the value dtype, `+float32` for fp32 coordinate tensors beside 16-bit values.  Per (shape, mode) the routes are
checked against each other once and then timed interleaved in one process: `rounds` measurements of `reps` steps each, median
with min and max.  One JSON line per measurement; --write FILE writes the table as markdown."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from modulated_deform_conv_amd import msda, msdap

SPREAD = 0.05   # box spread the project quotes for same-box comparisons
N, M, D = 8, 8, 32
PYRAMID = [(80, 80), (40, 40), (20, 20)]   # a 640 x 640 input at strides 8, 16, 32
# (name, levels, points, Lq; None: one query per value row)
SHAPES = [("dfine_decoder", PYRAMID, (3, 6, 3), 300), ("dfine_decoder", PYRAMID, (3, 6, 3), 500),
          ("rtdetrv2_decoder", PYRAMID, (4, 4, 4), 300), ("rtdetrv2_decoder", PYRAMID, (4, 4, 4), 500),
          ("encoder", PYRAMID, (3, 6, 3), None)]

# VGPRs per instance (`tools/kres.py msda_host | msdap_host samp_`).  Instances are named (value type, coordinate type); the
# list kernels by the coordinate type.
RESOURCES = [
    "## Kernel resources (`tools/kres.py msda_host samp_`, `tools/kres.py msdap_host samp_`)", "",
    "`MsdapOp` is `MsdaOp` but for the level of a tap: seven compares of the tap against the prefix sums (scalars) and their "
    "sum, then `MsdaOp::level`, in place of `tap / P`.  `msda_host.hip` is unchanged and so are its instances.  VGPRs "
    "(occupancy in waves per SIMD):", "",
    "| kernel | policy | f32/f32 | f16/f16 | f16/f32 | bf16/bf16 | bf16/f32 |", "|---|---|---|---|---|---|---|",
    "| `samp_fwd_kernel` | `MsdaOp` | 48 (8) | 72 (7) | 72 (7) | 54 (8) | 54 (8) |",
    "| `samp_fwd_kernel` | `MsdapOp` (new) | 50 (8) | 70 (7) | 70 (7) | 68 (7) | 68 (7) |",
    "| `samp_bwd_coord_kernel` | `MsdaOp` | 72 (7) | 79 (6) | 79 (6) | 86 (5) | 95 (5) |",
    "| `samp_bwd_coord_kernel` | `MsdapOp` (new) | 72 (7) | 78 (6) | 78 (6) | 95 (5) | 94 (5) |", "",
    "| kernel | policy | f32 count / fill | f16 count / fill | bf16 count / fill |", "|---|---|---|---|---|",
    "| `samp_list_kernel` | `MsdaOp` | 14 / 26 | 13 / 26 | 13 / 26 |",
    "| `samp_list_kernel` | `MsdapOp` (new) | 14 / 28 | 13 / 28 | 13 / 28 |", "",
    "No new instance uses scratch, AGPRs or LDS; SGPRs 78 (forward), 92 (coordinate backward), 50 / 54 (lists) against 71-72, "
    "85-87 and 46 / 49: the eight prefix sums.  The bf16 forward instances are the ones that moved: 54 -> 68 VGPRs, 8 -> 7 "
    "waves per SIMD.  The other form of the lookup -- selecting the level's row inside the compare chain, without the sum -- "
    "was built and not kept: 48 / 70 / 70 / 68 / 68 in the forward, but 97 VGPRs and 4 waves per SIMD in the bf16/bf16 "
    "coordinate backward, and 12 / 28 in the lists.", "",
]


NOTES = [
    "## Reading the table", "",
    "The decoder steps are a handful of short kernels (0.2-0.3 ms for forward, coordinate backward, list build and gather with "
    "autograd around them), so their figures move with the box and with the host more than the 8400-query lines do; the "
    "verdicts are per line against the 5 % spread.  The padded route's pad, stack and gradient slices are framework operators "
    "on the two coordinate tensors: on the decoder lines they are most of its distance to the native operator, which is why "
    "it is behind `ms_deform_attn` even at equal counts, where it pads nothing.  On the 8400-query lines the distance is the "
    "18 taps per head walked where 12 exist in the forward and the coordinate backward; the list build and the gather of "
    "`grad_value` see no padding tap.  The equal-count lines are the measurement of the level lookup: the compare "
    "chain against the division, everything else bit-identical.  The bf16 forward instances hold 68 VGPRs against 54 (7 waves "
    "per SIMD against 8); no bf16 line shows it.", "",
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
    _, levels, points, Lq = shape
    S = sum(h * w for h, w in levels)
    Lq = S if Lq is None else Lq
    K = sum(points)
    gen = torch.Generator().manual_seed(1)
    value = torch.randn(N, S, M, D, generator=gen).to(dtype).cuda()
    loc = (torch.rand(N, Lq, M, K, 2, generator=gen) * 1.1 - 0.05).to(coord_dtype).cuda()
    attn = torch.softmax(torch.randn(N, Lq, M, K, generator=gen), -1).to(coord_dtype).cuda()
    go = torch.randn(N, Lq, M * D, generator=gen).to(dtype).cuda()
    return value, loc, attn, go


def _leaves(value, loc, attn):
    return tuple(t.detach().requires_grad_(True) for t in (value, loc, attn))


def native_step(value, levels, points, loc, attn, go):
    def step():
        v, l, a = _leaves(value, loc, attn)
        out = msdap.ms_deform_attn_points(v, levels, points, l, a)
        out.backward(go)
        return out, v.grad, l.grad, a.grad
    return step


def composed_step(value, levels, points, loc, attn, go):
    """The published core function: the tap axis split by the point counts, one ``F.grid_sample`` per level (in the value
    dtype, fp32 coordinates cast to it as autocast does), the weighted sum; gradients from autograd."""
    Nn, S, Mm, Dd = value.shape
    Lq = loc.shape[1]
    sizes = [h * w for h, w in levels]

    def step():
        v, l, a = _leaves(value, loc, attn)
        grids = (2 * l - 1).to(v.dtype).permute(0, 2, 1, 3, 4).flatten(0, 1).split(list(points), dim=2)
        sampled = []
        for (h, w), img, grid in zip(levels, v.permute(0, 2, 3, 1).flatten(0, 1).split(sizes, dim=-1), grids):
            sampled.append(F.grid_sample(img.reshape(Nn * Mm, Dd, h, w), grid, mode="bilinear", padding_mode="zeros",
                                         align_corners=False))
        w_ = a.to(v.dtype).permute(0, 2, 1, 3).reshape(Nn * Mm, 1, Lq, sum(points))
        out = (torch.cat(sampled, -1) * w_).sum(-1).reshape(Nn, Mm * Dd, Lq).permute(0, 2, 1).contiguous()
        out.backward(go)
        return out, v.grad, l.grad, a.grad
    return step


def padded_step(value, levels, points, loc, attn, go):
    """The workaround on the parent commit: every level padded to max(points) taps of weight zero, then ``ms_deform_attn``;
    the pad, the slices of the gradients (autograd's) and the two materialised tensors are in the step.  The padding taps sit
    at location -1, outside the gate, which is the cheapest place for them: they read nothing and enter no list (at a
    location inside a level they would all land on the same value rows and serialise the list build)."""
    L, P = len(levels), max(points)

    def pad(t, fill):
        return torch.stack([F.pad(p, (0, 0) * (t.dim() - 4) + (0, P - p.shape[3]), value=fill) for p in t.split(list(points), dim=3)], 3)

    def step():
        v, l, a = _leaves(value, loc, attn)
        out = msda.ms_deform_attn(v, levels, pad(l, -1.0), pad(a, 0.0))
        out.backward(go)
        return out, v.grad, l.grad, a.grad
    return step


def uniform_step(value, levels, points, loc, attn, go):
    """``ms_deform_attn`` itself on the reshaped tensors: the equal-count lines only."""
    L, P = len(levels), points[0]

    def step():
        v, l, a = _leaves(value, loc, attn)
        out = msda.ms_deform_attn(v, levels, l.view(l.shape[:3] + (L, P, 2)), a.view(a.shape[:3] + (L, P)))
        out.backward(go)
        return out, v.grad, l.grad, a.grad
    return step


def measure(shape, dtype, coord_dtype, reps, rounds):
    _, levels, points, _ = shape
    t = make(shape, dtype, coord_dtype)
    args = (t[0], levels, points, t[1], t[2], t[3])
    steps = {"native": native_step(*args), "composed": composed_step(*args), "padded": padded_step(*args)}
    if len(set(points)) == 1:
        steps["ms_deform_attn"] = uniform_step(*args)
    # the routes compute the same thing (the composition is compared in fp32 only: with 16-bit values its grids are rounded
    # to 16 bits, which moves samples across cell borders)
    want = steps["native"]()
    for r, step in steps.items():
        if r == "composed" and dtype != torch.float32:
            continue
        for u, v in zip(step(), want):
            u, v = u.detach(), v.detach()
            err = float((u.double() - v.double()).abs().max() / max(1.0, float(v.double().abs().max())))
            assert err <= (1e-4 if v.dtype == torch.float32 and dtype == torch.float32 else 3e-2), (r, err)
    for step in steps.values():
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ms = {r: [] for r in steps}
    for _ in range(rounds):
        for r, step in steps.items():
            ms[r].append(timed(step, reps))
    return {r: (statistics.median(v), min(v), max(v)) for r, v in ms.items()}, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
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
            res, t = measure(shape, dtype, coord_dtype, a.reps, a.rounds)
            name = "%s_%s_Lq%d_%s" % (shape[0], "-".join(str(p) for p in shape[2]), t[1].shape[1], mode.replace("float", "f"))
            for r, (med, lo, hi) in res.items():
                print(json.dumps(dict(shape=name, route=r, median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4))),
                      flush=True)
            rows.append((name, res))
            del t
            torch.cuda.empty_cache()
    if a.write:
        write_markdown(a.write, rows, a)


def verdict(nat, other, what):
    if nat[0] > other[0] * (1 + SPREAD):
        v = "SLOWER than %s beyond the spread" % what
    elif nat[0] * (1 + SPREAD) < other[0]:
        v = "FASTER than %s beyond the spread" % what
    else:
        v = "within the spread of %s" % what
    return "%s: %.3f vs %.3f ms" % (v, nat[0], other[0])


def write_markdown(path, rows, a):
    out = ["# Deformable attention with a point count per level: step times against the routes a user had before", "",
           "Written by `tools/bench_msdap.py --write` (forward + backward through autograd, N = %d, M = %d, D = %d, levels "
           "80x80 / 40x40 / 20x20; median of %d rounds of %d steps, the routes interleaved in one process).  Box: %s.  "
           "Commit: %s." % (N, M, D, a.rounds, a.reps, torch.cuda.get_device_name(0), a.commit or "(not given)"), "",
           "`native`: `ms_deform_attn_points`.  `composed`: the published core function -- the tap axis split by the point "
           "counts, one `F.grid_sample` per level, gradients from autograd.  `padded`: `ms_deform_attn` with every level padded "
           "to max(points) by zero-weight taps outside the gate (they read nothing and enter no list), pad and gradient "
           "slices included.  `ms_deform_attn`: the existing operator on "
           "the reshaped tensors, equal counts only.  The shape names carry the point counts and Lq (`encoder`: Lq = S = 8400); "
           "`f32` / `bf16` is the value dtype; `+f32`: fp32 coordinate tensors.", "",
           "| shape | native ms (min - max) | composed ms (min - max) | composed / native | padded ms (min - max) | padded / native | ms_deform_attn ms (min - max) |",
           "|---|---|---|---|---|---|---|"]
    verdicts = []
    for name, res in rows:
        nat, comp, pad = res["native"], res["composed"], res["padded"]
        uni = res.get("ms_deform_attn")
        out.append("| %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %.3f (%.3f - %.3f) | %.2f | %s |" % (
            (name,) + nat + comp + (comp[0] / nat[0],) + pad + (pad[0] / nat[0], "%.3f (%.3f - %.3f)" % uni if uni else "")))
        verdicts.append("%s: native is %s" % (name, verdict(nat, comp, "the composition")))
        verdicts.append("%s: native is %s" % (name, verdict(nat, pad, "the padded workaround")))
        if uni:
            verdicts.append("%s: native is %s" % (name, verdict(nat, uni, "`ms_deform_attn`")))
    out += ["", "Spread quoted by the project for same-box comparisons: %d %%." % round(SPREAD * 100), ""] + ["- " + v for v in verdicts] + [""]
    out += NOTES + RESOURCES
    with open(path, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
