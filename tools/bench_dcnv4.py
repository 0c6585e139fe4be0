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
per measurement; --write FILE writes the table as markdown.

    python tools/bench_dcnv4.py --softmax [--reps 5] [--rounds 5] [--lines ...] [--commit TEXT] [--write profiles/dcnv4_softmax.md]

The softmax leg (MDCONV_FLAG_SOFTMAX), at the same shapes and timed the same way: ``dcnv4_core(..., softmax=True)`` on packed
logits against (a) the mask columns sliced, ``torch.softmax``, repacked, ``dcnv4_core`` without the flag, and (b) two
contiguous slices, ``F.softmax`` in fp32 and a cast as the ``DCNv3`` module runs it, ``dcnv3_core``; then one module-level
line, ``DCNv3Fused`` against ``DCNv3`` under bf16 autocast.  No route is favoured in advance: each line reports its ratios
and says "level" inside the spread, and plainly when the native call is slower."""
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


def soft_native_step(x, om, go, geo):
    def step():
        xi, oi = x.detach().requires_grad_(True), om.detach().requires_grad_(True)
        out = dcnv4.dcnv4_core(xi, oi, *geo, softmax=True)
        out.backward(go)
        return out, xi.grad, oi.grad
    return step


def soft_repacked_step(x, om, go, geo):
    """Route (a): the mask columns sliced, ``torch.softmax``, repacked, ``dcnv4_core`` without the flag."""
    k, s, p, d, G, D, scale, rc = geo
    K = k * k - int(rc)
    Bn, Ho, Wo, OM = om.shape

    def step():
        xi, oi = x.detach().requires_grad_(True), om.detach().requires_grad_(True)
        rows = oi[..., :G * K * 3].reshape(Bn, Ho, Wo, G, 3 * K)
        rows = torch.cat([rows[..., :2 * K], torch.softmax(rows[..., 2 * K:], -1)], -1).reshape(Bn, Ho, Wo, G * K * 3)
        packed = torch.cat([rows, rows.new_zeros(Bn, Ho, Wo, OM - G * K * 3)], -1) if OM > G * K * 3 else rows
        out = dcnv4.dcnv4_core(xi, packed, *geo)
        out.backward(go)
        return out, xi.grad, oi.grad
    return step


def soft_dcnv3_step(x, om, go, geo):
    """Route (b): what the ``DCNv3`` module runs behind its two linears -- ``F.softmax`` over the taps in fp32, a cast to
    the values' dtype, ``dcnv3_core`` -- on two slices of the same packed tensor."""
    k, s, p, d, G, D, scale, rc = geo
    K = k * k
    Bn, Ho, Wo, _ = om.shape

    def step():
        xi, oi = x.detach().requires_grad_(True), om.detach().requires_grad_(True)
        rows = oi[..., :G * K * 3].reshape(Bn, Ho, Wo, G, 3 * K)
        off = rows[..., :2 * K].reshape(Bn, Ho, Wo, G * 2 * K).to(x.dtype).contiguous()
        m = torch.softmax(rows[..., 2 * K:].float(), -1).reshape(Bn, Ho, Wo, G * K).to(x.dtype)
        out = dcnv3.dcnv3_core(xi, off, m, k, s, p, d, G, D, scale)
        out.backward(go)
        return out, xi.grad, oi.grad
    return step


def interleaved(steps, reps, rounds):
    for step in steps.values():
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ms = {r: [] for r in steps}
    for _ in range(rounds):
        for r, step in steps.items():
            ms[r].append(timed(step, reps))
    return {r: (statistics.median(v), min(v), max(v)) for r, v in ms.items()}


def measure_softmax(line, reps, rounds):
    shape, dtype, cdt, rc = line
    x, om, go, geo = make(shape, dtype, cdt, rc)
    steps = {"native": soft_native_step(x, om, go, geo), "repacked": soft_repacked_step(x, om, go, geo)}
    if not rc:
        steps["dcnv3"] = soft_dcnv3_step(x, om, go, geo)
    # the routes compute the same thing (with fp32 coordinates route (b) rounds them first: not compared)
    a = steps["native"]()
    for r in ("repacked", "dcnv3"):
        if r in steps and (r == "repacked" or cdt == dtype):
            for u, v in zip(a, steps[r]()):
                u, v = u.detach(), v.detach()
                err = float((u.double() - v.double()).abs().max() / max(1.0, float(v.double().abs().max())))
                assert err <= (1e-4 if v.dtype == F32 else 3e-2), (r, err)
    return interleaved(steps, reps, rounds)


def measure_modules(reps, rounds, hw=56, C=64, G=4):
    """``DCNv3Fused`` against ``DCNv3`` with the same parameters, one training step under bf16 autocast."""
    torch.manual_seed(3)
    theirs = dcnv3.DCNv3(channels=C, kernel_size=KSZ, group=G).cuda()
    with torch.no_grad():
        theirs.offset.weight.normal_(0, 0.02)
        theirs.offset.bias.uniform_(-1, 1)
        theirs.mask.weight.normal_(0, 0.3)
    ours = dcnv3.DCNv3Fused(channels=C, kernel_size=KSZ, group=G).cuda()
    ours.load_state_dict(theirs.state_dict())
    x = torch.randn(B, hw, hw, C, device="cuda")
    go = torch.randn(B, hw, hw, C, device="cuda").bfloat16()

    def step_of(mod):
        def step():
            mod.zero_grad(set_to_none=True)
            xi = x.detach().requires_grad_(True)
            with torch.autocast("cuda", dtype=BF16):
                y = mod(xi)
            y.backward(go)
            return y
        return step
    return "module_%dx%dx%d_g%d_bf16_autocast" % (hw, hw, C, G), interleaved(dict(native=step_of(ours), dcnv3=step_of(theirs)), reps, rounds)


def verdict_of(nat, other):
    if nat > other * (1 + SPREAD):
        return "SLOWER"
    if nat * (1 + SPREAD) < other:
        return "faster"
    return "level"


SOFT_RESOURCES = [
    "## Kernel resources (`tools/kres.py dcn4_host samp_`)", "",
    "`Dcn4SoftOp` is a policy type of its own, so no existing instance is compiled differently: `dcn4_host.hip` built from the "
    "parent commit's sources and from this commit's with the same compiler gives every `Dcn4Op` instance the same VGPR count, SGPR "
    "count, occupancy and zero scratch (table below, `VGPRs / SGPRs / waves per SIMD`), and `tools/kres.py dcn3_host | msda_host | "
    "fda_host samp_` print the same 12 + 16 + 16 lines for both trees: the instances of `Dcn3Op`, `MsdaOp` and `FdaOp` keep every "
    "figure (`FdaOp` is used as it stands: `fda_weight` is shared, nothing was factored out of it).  The new instances use no "
    "scratch, no AGPRs and no LDS.", "",
    "| kernel | policy | f32/f32 | f16/f16 | f16/f32 | bf16/bf16 | bf16/f32 |", "|---|---|---|---|---|---|---|",
    "| `samp_fwd_kernel` | `Dcn4Op` parent | 56 / 56 / 8 | 58 / 56 / 8 | 58 / 56 / 8 | 60 / 56 / 8 | 60 / 56 / 8 |",
    "| `samp_fwd_kernel` | `Dcn4Op` now | 56 / 56 / 8 | 58 / 56 / 8 | 58 / 56 / 8 | 60 / 56 / 8 | 60 / 56 / 8 |",
    "| `samp_fwd_kernel` | `Dcn4SoftOp` (new) | 58 / 57 / 8 | 64 / 57 / 8 | 64 / 57 / 8 | 66 / 59 / 7 | 66 / 59 / 7 |",
    "| `samp_bwd_coord_kernel` | `Dcn4Op` parent | 80 / 74 / 6 | 88 / 74 / 5 | 88 / 74 / 5 | 95 / 76 / 5 | 94 / 74 / 5 |",
    "| `samp_bwd_coord_kernel` | `Dcn4Op` now | 80 / 74 / 6 | 88 / 74 / 5 | 88 / 74 / 5 | 95 / 76 / 5 | 94 / 74 / 5 |",
    "| `samp_bwd_coord_kernel` | `Dcn4SoftOp` (new) | 84 / 79 / 5 | 91 / 79 / 5 | 91 / 79 / 5 | 108 / 79 / 4 | 96 / 79 / 5 |", "",
    "| kernel | policy | f32 count / fill | f16 count / fill | bf16 count / fill |", "|---|---|---|---|---|",
    "| `samp_list_kernel` | `Dcn4Op` parent | 12 / 32 / 8, 24 / 38 / 8 | 11 / 32 / 8, 24 / 43 / 8 | 11 / 34 / 8, 24 / 38 / 8 |",
    "| `samp_list_kernel` | `Dcn4Op` now | 12 / 32 / 8, 24 / 38 / 8 | 11 / 32 / 8, 24 / 43 / 8 | 11 / 34 / 8, 24 / 38 / 8 |",
    "| `samp_list_kernel` | `Dcn4SoftOp` (new) | 12 / 32 / 8, 24 / 41 / 8 | 11 / 32 / 8, 24 / 41 / 8 | 11 / 34 / 8, 24 / 41 / 8 |", "",
    "`samp_gather_kernel` is shared and unchanged.", "",
]


def write_softmax_markdown(path, rows, a):
    out = ["# DCNv4 operator with the softmax inside (MDCONV_FLAG_SOFTMAX): step times against the composed routes", "",
           "Written by `tools/bench_dcnv4.py --softmax --write` (forward + backward through autograd, B = %d, %d x %d kernel, stride 1, "
           "pad 1; median of %d rounds of %d steps, the routes interleaved in one process).  Box: %s.  Commit: %s." % (
               B, KSZ, KSZ, a.rounds, a.reps, torch.cuda.get_device_name(0), a.commit or "(not given)"), "",
           "`native`: `dcnv4_core(..., softmax=True)` on the packed logits.  `repacked` (a): the mask columns sliced, `torch.softmax`, "
           "repacked, `dcnv4_core` without the flag.  `dcnv3` (b): two contiguous slices, `F.softmax` in fp32 and a cast as the `DCNv3` "
           "module runs it, `dcnv3_core`; it cannot run `remove_center`.  The `module_` line is one training step of `DCNv3Fused` "
           "(native) against `DCNv3` (dcnv3) with the same parameters under bf16 autocast.  A ratio above 1 means the native call is "
           "faster; \"level\" is inside the %d %% spread the project quotes for same-box comparisons." % round(SPREAD * 100), "",
           "| line | native ms (min - max) | repacked ms (min - max) | repacked / native | dcnv3 ms (min - max) | dcnv3 / native |",
           "|---|---|---|---|---|---|"]
    verdicts = []
    for name, res in rows:
        nat = res["native"]
        cells, said = [], []
        for r in ("repacked", "dcnv3"):
            if r in res:
                cells += ["%.3f (%.3f - %.3f)" % res[r], "%.2f" % (res[r][0] / nat[0])]
                said.append("%s against %s (%.3f vs %.3f ms)" % (verdict_of(nat[0], res[r][0]), r, nat[0], res[r][0]))
            else:
                cells += ["cannot run" if r == "dcnv3" else "", ""]
        out.append("| %s | %.3f (%.3f - %.3f) | %s |" % ((name,) + nat + (" | ".join(cells),)))
        verdicts.append("%s: the native call is %s" % (name, ", ".join(said)))
    out += [""] + ["- " + v for v in verdicts] + [""] + SOFT_RESOURCES
    with open(path, "w") as f:
        f.write("\n".join(out))


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
    ap.add_argument("--softmax", action="store_true", help="the MDCONV_FLAG_SOFTMAX leg (module docstring)")
    a = ap.parse_args()
    rows = []
    if a.softmax:
        todo = [(line_name(LINES[i]), lambda i=i: measure_softmax(LINES[i], a.reps, a.rounds)) for i in (int(s) for s in a.lines.split(","))]
        for name, run in todo + [(None, lambda: measure_modules(a.reps, a.rounds))]:
            res = run()
            if name is None:
                name, res = res
            for r, (med, lo, hi) in res.items():
                print(json.dumps(dict(line=name, leg="softmax", route=r, median_ms=round(med, 4), min_ms=round(lo, 4),
                                      max_ms=round(hi, 4))), flush=True)
            rows.append((name, res))
            torch.cuda.empty_cache()
        if a.write:
            write_softmax_markdown(a.write, rows, a)
        return
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
