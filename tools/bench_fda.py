"""Step time (forward + backward, through autograd) of packed deformable attention (include/mdconv.h, "Packed deformable
attention"; csrc/fda_*.hip on csrc/samp_core.hpp) against the route a user of this library had before it: two slices of the
packed tensor, a framework softmax over the logits, ``ms_deform_attn``, and autograd's softmax backward and concatenation of
the two gradients.

    python tools/bench_fda.py [--reps 20] [--rounds 7] [--modes float32,bfloat16,bfloat16+float32] [--shapes 0,1,2]
                              [--commit TEXT] [--write FILE]

A mode is the value dtype, `+float32` for an fp32 packed tensor beside 16-bit values.  Per (shape, mode) the two routes are
checked against each other once and then timed interleaved in one process: `rounds` measurements of `reps` steps each, median
with min and max.  The native forward, the native backward without grad_value (the coordinate-gradient kernel alone, which
here walks the taps twice) and the full native backward are timed the same way through the entry points, so the list build +
gather is their difference; `msda coord` is the coordinate-gradient kernel of ``ms_deform_attn`` on the same shape, which
walks them once.  One JSON line per measurement; --write FILE writes the table as markdown."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from modulated_deform_conv_amd import fda, msda

SPREAD = 0.05   # box spread the project quotes for same-box comparisons
N, M, D, P = 2, 8, 32, 4
PYRAMID = [(64, 64), (32, 32), (16, 16), (8, 8)]
# (name, levels, Lq; None: one query per value row) -- the shapes of tools/bench_msda.py
SHAPES = [("encoder", PYRAMID, None), ("decoder", PYRAMID, 300), ("pixel_decoder", [(32, 32), (16, 16), (8, 8)], None)]

# VGPRs per instance (`tools/kres.py dcn3_host | msda_host | dcn4_host | fda_host`, filter `samp_`), parent commit -> this
# commit, and the new instances.  Instances are named (value type, coordinate type); the list kernels by the coordinate type.
RESOURCES = [
    "## Kernel resources (`tools/kres.py dcn3_host | msda_host | dcn4_host | fda_host samp_`)", "",
    "The policy contract of the sampling core grew `begin_pair` / `kPairSum` + `factor_grad` / `list_factor`, which the three "
    "existing policies inherit as identities (`SampPlainFactor`), and `MsdaOp` now states its tap and its list item by element "
    "(`tap_state`, `list_item_at`) so that `FdaOp` can call them.  Existing instances, built from the parent commit's sources and "
    "from this commit's with the same compiler: every one of the 44 has the same VGPR and SGPR count, no scratch, no AGPRs, no "
    "LDS, the same occupancy -- the tool's lines are identical.", "",
    "| kernel | policy | f32/f32 | f16/f16 | f16/f32 | bf16/bf16 | bf16/f32 |", "|---|---|---|---|---|---|---|",
    "| `samp_fwd_kernel` | `Dcn3Op` parent -> now | 54 -> 54 | 58 -> 58 | | 60 -> 60 | |",
    "| `samp_fwd_kernel` | `MsdaOp` parent -> now | 48 -> 48 | 72 -> 72 | 72 -> 72 | 54 -> 54 | 54 -> 54 |",
    "| `samp_fwd_kernel` | `Dcn4Op` parent -> now | 56 -> 56 | 58 -> 58 | 58 -> 58 | 60 -> 60 | 60 -> 60 |",
    "| `samp_fwd_kernel` | `FdaOp` (new) | 54 | 58 | 58 | 60 | 60 |",
    "| `samp_bwd_coord_kernel` | `Dcn3Op` parent -> now | 76 -> 76 | 83 -> 83 | | 91 -> 91 | |",
    "| `samp_bwd_coord_kernel` | `MsdaOp` parent -> now | 72 -> 72 | 79 -> 79 | 79 -> 79 | 86 -> 86 | 95 -> 95 |",
    "| `samp_bwd_coord_kernel` | `Dcn4Op` parent -> now | 80 -> 80 | 88 -> 88 | 88 -> 88 | 95 -> 95 | 94 -> 94 |",
    "| `samp_bwd_coord_kernel` | `FdaOp` (new) | 78 | 84 | 84 | 90 | 89 |", "",
    "| kernel | policy | f32 count / fill | f16 count / fill | bf16 count / fill |", "|---|---|---|---|---|",
    "| `samp_list_kernel` | `Dcn3Op` parent -> now | 12 / 24 -> 12 / 24 | 11 / 24 -> 11 / 24 | 11 / 24 -> 11 / 24 |",
    "| `samp_list_kernel` | `MsdaOp` parent -> now | 14 / 26 -> 14 / 26 | 13 / 26 -> 13 / 26 | 13 / 26 -> 13 / 26 |",
    "| `samp_list_kernel` | `Dcn4Op` parent -> now | 12 / 24 -> 12 / 24 | 11 / 24 -> 11 / 24 | 11 / 24 -> 11 / 24 |",
    "| `samp_list_kernel` | `FdaOp` (new) | 14 / 26 | 13 / 26 | 13 / 26 |", "",
    "The new instances use no scratch, no AGPRs and no LDS; occupancy 8 waves per SIMD for the forward and the list kernels, 6 "
    "(f32) / 5 (16-bit values) for the coordinate backward.  `samp_gather_kernel` is not instantiated anew.  One form of the "
    "`MsdaOp` split did cost registers and was not kept: a `tap_state` that leaves the factor to its caller, which loads it after "
    "the corner offsets, takes +2 VGPRs in every `MsdaOp` forward instance (+4 for bf16 / f32) and a wave of occupancy in the two "
    "fp16 ones (72 -> 74); with the load where it was -- inside `tap_state`, by element index, as in `Dcn3Op::tap_state` -- the "
    "instances are the parent's.", "",
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
    loc = torch.rand(N, Lq, M, len(levels), P, 2, generator=gen) * 1.1 - 0.05
    logits = torch.randn(N, Lq, M, len(levels), P, generator=gen)
    loc_attn = fda.pack_loc_attn(loc, logits).to(coord_dtype).cuda()
    go = torch.randn(N, Lq, M * D, generator=gen).to(dtype).cuda()
    return value, loc_attn, go


def native_step(value, levels, loc_attn, go):
    def step():
        v, la = value.detach().requires_grad_(True), loc_attn.detach().requires_grad_(True)
        out = fda.flash_deform_attn(v, levels, la, P)
        out.backward(go)
        return out, v.grad, la.grad
    return step


def composed_step(value, levels, loc_attn, go):
    """What the block around ``ms_deform_attn`` does with the same packed tensor: two slices, the framework softmax (in the
    packed tensor's dtype: fp32 beside 16-bit values under autocast), the call, and autograd's softmax backward and
    concatenation of the two gradients."""
    L, K = len(levels), len(levels) * P
    Nn, Lq, Mm, _ = loc_attn.shape

    def step():
        v, la = value.detach().requires_grad_(True), loc_attn.detach().requires_grad_(True)
        loc = la[..., :2 * K].reshape(Nn, Lq, Mm, L, P, 2)
        attn = torch.softmax(la[..., 2 * K:], -1).reshape(Nn, Lq, Mm, L, P)
        out = msda.ms_deform_attn(v, levels, loc, attn)
        out.backward(go)
        return out, v.grad, la.grad
    return step


def measure(shape, dtype, coord_dtype, reps, rounds):
    levels = shape[1]
    value, loc_attn, go = t = make(shape, dtype, coord_dtype)
    L, K = len(levels), len(levels) * P
    Nn, Lq, Mm, _ = loc_attn.shape
    loc = loc_attn[..., :2 * K].reshape(Nn, Lq, Mm, L, P, 2).contiguous()
    attn = torch.softmax(loc_attn[..., 2 * K:].float(), -1).to(coord_dtype).reshape(Nn, Lq, Mm, L, P).contiguous()
    steps = {
        "native": native_step(value, levels, loc_attn, go),
        "composed": composed_step(value, levels, loc_attn, go),
        "native_fwd": lambda: fda.flash_deform_attn_forward(value, levels, loc_attn, P),
        "native_bwd": lambda: fda.flash_deform_attn_backward(value, levels, loc_attn, P, go),
        "native_bwd_no_grad_value": lambda: fda.flash_deform_attn_backward(value, levels, loc_attn, P, go, need_grad_value=False),
        "msda_bwd_no_grad_value": lambda: msda.ms_deform_attn_backward(value, levels, loc, attn, go, need_grad_value=False),
    }
    # the two routes compute the same thing
    for u, v in zip(steps["native"](), steps["composed"]()):
        u, v = u.detach(), v.detach()
        err = float((u.double() - v.double()).abs().max() / max(1.0, float(v.double().abs().max())))
        assert err <= (1e-4 if v.dtype == torch.float32 else 3e-2), err
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
            name = "%s_L%d_Lq%d_%s" % (shape[0], len(shape[1]), t[1].shape[1], mode.replace("float", "f"))
            for r, (med, lo, hi) in res.items():
                print(json.dumps(dict(shape=name, route=r, median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4))),
                      flush=True)
            rows.append((name, res))
            del t
            torch.cuda.empty_cache()
    if a.write:
        write_markdown(a.write, rows, a)


def write_markdown(path, rows, a):
    out = ["# Packed deformable attention: step times against the composed route through `ms_deform_attn`", "",
           "Written by `tools/bench_fda.py --write` (forward + backward through autograd, N = %d, M = %d, D = %d, P = %d; median of "
           "%d rounds of %d steps, the routes interleaved in one process).  Box: %s.  Commit: %s." % (
               N, M, D, P, a.rounds, a.reps, torch.cuda.get_device_name(0), a.commit or "(not given)"), "",
           "`native`: `flash_deform_attn` on the packed tensor.  `composed`: two slices of the packed tensor, `torch.softmax` over "
           "the logits, `ms_deform_attn`, and autograd's softmax backward and concatenation of the two gradients.  `fwd`, `coord` "
           "and `lists + gather` are the native entry points called directly: the forward, the backward with "
           "`MDCONV_FLAG_NO_GRAD_INPUT` (the coordinate-gradient kernel alone: two walks over the taps), and the full backward "
           "minus it.  `msda coord`: the coordinate-gradient kernel of `ms_deform_attn` on the same shape (one walk).  `f32` / "
           "`bf16` is the value dtype; `+f32`: an fp32 packed tensor.", "",
           "| shape | native ms (min - max) | composed ms (min - max) | composed / native | fwd ms | coord ms | msda coord ms | lists + gather ms |",
           "|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for name, res in rows:
        nat, comp = res["native"], res["composed"]
        out.append("| %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %.3f | %.3f | %.3f | %.3f |" % (
            (name,) + nat + comp + (comp[0] / nat[0], res["native_fwd"][0], res["native_bwd_no_grad_value"][0],
                                    res["msda_bwd_no_grad_value"][0], res["native_bwd"][0] - res["native_bwd_no_grad_value"][0])))
        if nat[0] > comp[0] * (1 + SPREAD):
            verdict = "SLOWER than the composed route beyond the spread"
        elif nat[0] * (1 + SPREAD) < comp[0]:
            verdict = "FASTER than the composed route beyond the spread"
        else:
            verdict = "within the spread of the composed route"
        verdicts.append("%s: the native operator is %s: %.3f vs %.3f ms" % (name, verdict, nat[0], comp[0]))
    out += ["", "Spread quoted by the project for same-box comparisons: %d %%." % round(SPREAD * 100), ""] + ["- " + v for v in verdicts] + [""]
    out += RESOURCES
    with open(path, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
