"""Step time (forward + backward, through autograd) of the DCNv4 operator (include/mdconv.h, "DCNv4 operator"; csrc/dcn4_*.hip on
csrc/samp_core.hpp) against the route a user of this library had before it: slice the packed ``offset_mask`` into contiguous
``offset`` and ``mask`` tensors, ``dcnv3_core``, and autograd's concatenation of the two gradients into the gradient of
``offset_mask``.

    python tools/bench_dcnv4.py [--reps 5] [--rounds 5] [--lines 0,1,...] [--commit TEXT] [--write FILE]

Per line the two routes are timed interleaved in one process: `rounds` measurements of `reps` steps each, median with min
and max.  The native forward, the native backward without grad_input (the coordinate-gradient kernel alone) and the full
native backward are timed the same way through the entry points, so the list build + gather is their difference.  The
composed route cannot run ``remove_center`` at all: that line reports the native time alone.  With fp32 coordinates beside
16-bit values the composed route casts its two slices to the values' dtype (DCNv3 has one dtype per call).  One JSON line
per measurement; --write FILE writes the table as markdown."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from modulated_deform_conv_amd import dcnv3, dcnv4

SPREAD = 0.05   # box spread the project quotes for same-box comparisons
B, KSZ = 8, 3
# (H = W, G, D, offset_scale): the shapes of profiles/dcnv3.md
SHAPES = [(56, 4, 16, 1.0), (28, 8, 16, 1.0), (14, 16, 16, 1.0), (7, 32, 16, 1.0), (56, 4, 16, 2.0)]
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# (shape, value dtype, coordinate dtype, remove_center): every shape in the three dtypes of profiles/dcnv3.md, then bf16 values
# with fp32 coordinates, then one remove_center line
LINES = [(s, dt, dt, False) for s in SHAPES for dt in (F32, F16, BF16)] + [(SHAPES[0], BF16, F32, False), (SHAPES[0], BF16, BF16, True)]

# VGPRs per instance (`tools/kres.py dcn3_host | msda_host | dcn4_host`, filter `samp_`), parent commit -> this commit, and
# the new instances.  Instances are named (value type, coordinate type); the list kernels by the coordinate type alone.
RESOURCES = [
    "## Kernel resources (`tools/kres.py dcn3_host | msda_host | dcn4_host samp_`)", "",
    "The policy contract of the sampling core grew `coord_index` / `factor_index` / `list_factor_index` / `finish_pair`.  Existing "
    "instances, built from the parent commit's sources and from this commit's with the same compiler: every one of the 28 has the "
    "same VGPR count, no scratch, no AGPRs, no LDS, the same occupancy.  (One SGPR count moved: `samp_list_kernel<Dcn3Op, f16, fill>` "
    "38 -> 37.)", "",
    "| kernel | policy | f32/f32 | f16/f16 | f16/f32 | bf16/bf16 | bf16/f32 |", "|---|---|---|---|---|---|---|",
    "| `samp_fwd_kernel` | `Dcn3Op` parent -> now | 54 -> 54 | 58 -> 58 | | 60 -> 60 | |",
    "| `samp_fwd_kernel` | `MsdaOp` parent -> now | 48 -> 48 | 72 -> 72 | 72 -> 72 | 54 -> 54 | 54 -> 54 |",
    "| `samp_fwd_kernel` | `Dcn4Op` (new) | 56 | 58 | 58 | 60 | 60 |",
    "| `samp_bwd_coord_kernel` | `Dcn3Op` parent -> now | 76 -> 76 | 83 -> 83 | | 91 -> 91 | |",
    "| `samp_bwd_coord_kernel` | `MsdaOp` parent -> now | 72 -> 72 | 79 -> 79 | 79 -> 79 | 86 -> 86 | 95 -> 95 |",
    "| `samp_bwd_coord_kernel` | `Dcn4Op` (new) | 80 | 88 | 88 | 95 | 94 |", "",
    "| kernel | policy | f32 count / fill | f16 count / fill | bf16 count / fill |", "|---|---|---|---|---|",
    "| `samp_list_kernel` | `Dcn3Op` parent -> now | 12 / 24 -> 12 / 24 | 11 / 24 -> 11 / 24 | 11 / 24 -> 11 / 24 |",
    "| `samp_list_kernel` | `MsdaOp` parent -> now | 14 / 26 -> 14 / 26 | 13 / 26 -> 13 / 26 | 13 / 26 -> 13 / 26 |",
    "| `samp_list_kernel` | `Dcn4Op` (new) | 12 / 24 | 11 / 24 | 11 / 24 |", "",
    "The new instances use no scratch, no AGPRs and no LDS; occupancy 8 waves per SIMD for the forward and the list kernels, 6 "
    "(f32) / 5 (16-bit values) for the coordinate backward, as under `Dcn3Op`.  Two forms of the core change did cost registers "
    "and were not kept.  Taking the two indices at the `build_tap` call (as arguments) computes them outside the `on` test, where "
    "they dominate the kernel's stores and stay live across the tap walk: +2 VGPRs in the `Dcn3Op` coordinate backward.  A "
    "`coord_index` that returns the x element with y as `+ 1` at the use costs the same +2 there (the compiler no longer forms "
    "`2 e + 1` from `e`); so the policy returns x or y by a constant selector, and `build_tap` takes its indices behind the `on` "
    "test.  Dropping `__restrict__` from the two gradient pointers costs `samp_bwd_coord_kernel<MsdaOp, bf16, bf16>` 11 VGPRs and a "
    "wave of occupancy (86 -> 97); the qualifier is still true for a packed tensor (samp_core.hpp says why) and stays.", "",
]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def make(shape, dtype, cdt, rc):
    hw, G, D, scale = shape
    gen = torch.Generator().manual_seed(1)
    K = KSZ * KSZ - int(rc)
    om_len = dcnv4.offset_mask_len(KSZ, G, rc)
    x = torch.randn(B, hw, hw, G * D, generator=gen).to(dtype).cuda()
    rows = torch.cat([(torch.rand(B, hw, hw, G, 2 * K, generator=gen) * 2 - 1) * 1.5, torch.randn(B, hw, hw, G, K, generator=gen)], -1)
    om = torch.zeros(B, hw, hw, om_len)
    om[..., :G * K * 3] = rows.reshape(B, hw, hw, G * K * 3)
    go = torch.randn(B, hw, hw, G * D, generator=gen).to(dtype).cuda()
    return x, om.to(cdt).cuda(), go, (KSZ, 1, 1, 1, G, D, scale, rc)


def native_step(x, om, go, geo):
    def step():
        xi, oi = x.detach().requires_grad_(True), om.detach().requires_grad_(True)
        out = dcnv4.dcnv4_core(xi, oi, *geo)
        out.backward(go)
        return out, xi.grad, oi.grad
    return step


def composed_step(x, om, go, geo):
    """What a DCNv4 block had to do on the DCNv3 operator: two contiguous slices (cast to the values' dtype), the call, and
    the concatenation of the two gradients that autograd performs for the slices."""
    k, s, p, d, G, D, scale, rc = geo
    K = k * k
    Bn, Ho, Wo, _ = om.shape

    def step():
        xi, oi = x.detach().requires_grad_(True), om.detach().requires_grad_(True)
        rows = oi[..., :G * K * 3].reshape(Bn, Ho, Wo, G, 3 * K)
        off = rows[..., :2 * K].reshape(Bn, Ho, Wo, G * 2 * K).to(x.dtype).contiguous()
        m = rows[..., 2 * K:].reshape(Bn, Ho, Wo, G * K).to(x.dtype).contiguous()
        out = dcnv3.dcnv3_core(xi, off, m, k, s, p, d, G, D, scale)
        out.backward(go)
        return out, xi.grad, oi.grad
    return step


def measure(line, reps, rounds):
    shape, dtype, cdt, rc = line
    x, om, go, geo = make(shape, dtype, cdt, rc)
    steps = {
        "native": native_step(x, om, go, geo),
        "native_fwd": lambda: dcnv4.dcnv4_forward(x, om, *geo),
        "native_bwd": lambda: dcnv4.dcnv4_backward(x, om, go, *geo),
        "native_bwd_no_grad_input": lambda: dcnv4.dcnv4_backward(x, om, go, *geo, need_grad_input=False),
    }
    if not rc:
        steps["composed"] = composed_step(x, om, go, geo)
        # the two routes compute the same thing (with fp32 coordinates the composed route rounds them first: not compared)
        a, b = steps["native"](), steps["composed"]()
        for u, v in zip(a, b) if cdt == dtype else ():
            err = float((u.double() - v.double()).abs().max() / max(1.0, float(v.double().abs().max())))
            assert err <= (1e-4 if v.dtype == F32 else 3e-2), err
    for step in steps.values():
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ms = {r: [] for r in steps}
    for _ in range(rounds):
        for r, step in steps.items():
            ms[r].append(timed(step, reps))
    return {r: (statistics.median(v), min(v), max(v)) for r, v in ms.items()}


def line_name(line):
    shape, dtype, cdt, rc = line
    short = lambda t: str(t).split(".")[1]
    return "%dx%dx%d_g%d_s%g_%s%s%s" % (shape[0], shape[0], shape[1] * shape[2], shape[1], shape[3], short(dtype),
                                        "" if cdt == dtype else "+" + short(cdt) + "_coords", "_remove_center" if rc else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lines", default=",".join(str(i) for i in range(len(LINES))))
    ap.add_argument("--commit", default="")
    ap.add_argument("--write")
    a = ap.parse_args()
    rows = []
    for i in (int(s) for s in a.lines.split(",")):
        res = measure(LINES[i], a.reps, a.rounds)
        name = line_name(LINES[i])
        for r, (med, lo, hi) in res.items():
            print(json.dumps(dict(line=name, route=r, median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4))), flush=True)
        rows.append((name, res))
        torch.cuda.empty_cache()
    if a.write:
        write_markdown(a.write, rows, a)


def write_markdown(path, rows, a):
    out = ["# DCNv4 operator: step times against the sliced route through the DCNv3 operator", "",
           "Written by `tools/bench_dcnv4.py --write` (forward + backward through autograd, B = %d, %d x %d kernel, stride 1, pad 1; "
           "median of %d rounds of %d steps, the routes interleaved in one process).  Box: %s.  Commit: %s." % (
               B, KSZ, KSZ, a.rounds, a.reps, torch.cuda.get_device_name(0), a.commit or "(not given)"), "",
           "`native`: `dcnv4_core` on the packed `offset_mask`.  `composed`: two contiguous slices of `offset_mask` (cast to the "
           "values' dtype where the coordinates are fp32), `dcnv3_core`, and autograd's concatenation of the two gradients; it "
           "cannot run `remove_center`, so that line has the native time alone.  `fwd`, `coord` and `lists + gather` are the "
           "native entry points called directly: the forward, the backward with `MDCONV_FLAG_NO_GRAD_INPUT` (the "
           "coordinate-gradient kernel alone), and the full backward minus it.", "",
           "| line | native ms (min - max) | composed ms (min - max) | composed / native | fwd ms | coord ms | lists + gather ms |",
           "|---|---|---|---|---|---|---|"]
    verdicts = []
    for name, res in rows:
        nat, comp = res["native"], res.get("composed")
        stages = (res["native_fwd"][0], res["native_bwd_no_grad_input"][0], res["native_bwd"][0] - res["native_bwd_no_grad_input"][0])
        if comp is None:
            out.append("| %s | %.3f (%.3f - %.3f) | cannot run | | %.3f | %.3f | %.3f |" % ((name,) + nat + stages))
            verdicts.append("%s: native alone, %.3f ms (the composed route has no remove_center)" % (name, nat[0]))
            continue
        out.append("| %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %.3f | %.3f | %.3f |" % (
            (name,) + nat + comp + (comp[0] / nat[0],) + stages))
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
