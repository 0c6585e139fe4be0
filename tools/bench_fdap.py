"""Step time (forward + backward, through autograd) of packed deformable attention with a point count per level
(include/mdconv_fdap.h; csrc/fdap_host.hip on csrc/samp_core.hpp) against the route a user had before it: two slices of the
same packed tensor, ``torch.softmax``, ``ms_deform_attn_points`` and autograd's concatenation of the two gradients; on the
equal-count lines also ``flash_deform_attn``; and one whole-block line, ``MSDeformableAttentionFused`` against
``MSDeformableAttention`` under bf16 autocast.

    python tools/bench_fdap.py [--reps 20] [--rounds 7] [--modes float32,bfloat16,bfloat16+float32] [--shapes 0,1,2,3,4]
                               [--no-block] [--commit TEXT] [--write FILE]

A mode is the value dtype, `+float32` for an fp32 packed tensor beside 16-bit values.  Per (shape, mode) the routes are
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

from modulated_deform_conv_amd import fda, fdap, msdap

SPREAD = 0.05   # box spread the project quotes for same-box comparisons
N, M, D = 8, 8, 32
PYRAMID = [(80, 80), (40, 40), (20, 20)]   # a 640 x 640 input at strides 8, 16, 32
# (name, levels, points, Lq; None: one query per value row)
SHAPES = [("dfine_decoder", PYRAMID, (3, 6, 3), 300), ("dfine_decoder", PYRAMID, (3, 6, 3), 500),
          ("encoder", PYRAMID, (3, 6, 3), None),
          ("rtdetrv2_decoder", PYRAMID, (4, 4, 4), 300), ("rtdetrv2_decoder", PYRAMID, (4, 4, 4), 500)]
BLOCK_LQ = 300

# VGPRs / SGPRs per instance (`tools/kres.py fda_host | msdap_host | fdap_host samp_`).  Instances are named (value type,
# coordinate type); the list kernels by the coordinate type.
RESOURCES = [
    "## Kernel resources (`tools/kres.py fda_host samp_`, `tools/kres.py msdap_host samp_`, `tools/kres.py fdap_host samp_`)", "",
    "`FdapOp` is `FdaOp` with `MsdapOp::tap_state` / `list_item_at` in the place of `MsdaOp`'s: the packed addressing, the "
    "pair statistics and `fda_weight` of the one, the prefix-sum level lookup of the other.  `fda_host.hip` and "
    "`msdap_host.hip` are unchanged and so are their instances.  VGPRs (occupancy in waves per SIMD):", "",
    "    kernel                  policy           f32/f32   f16/f16   f16/f32   bf16/bf16   bf16/f32",
    "    samp_fwd_kernel         FdaOp            54 (8)    58 (8)    58 (8)    60 (8)      60 (8)",
    "    samp_fwd_kernel         MsdapOp          50 (8)    70 (7)    70 (7)    68 (7)      68 (7)",
    "    samp_fwd_kernel         FdapOp (new)     52 (8)    58 (8)    58 (8)    60 (8)      60 (8)",
    "    samp_bwd_coord_kernel   FdaOp            78 (6)    84 (5)    84 (5)    90 (5)      89 (5)",
    "    samp_bwd_coord_kernel   MsdapOp          72 (7)    78 (6)    78 (6)    95 (5)      94 (5)",
    "    samp_bwd_coord_kernel   FdapOp (new)     76 (6)    83 (5)    83 (5)    89 (5)      88 (5)", "",
    "    kernel             policy           f32 count / fill   f16 count / fill   bf16 count / fill",
    "    samp_list_kernel   FdaOp            14 / 26            13 / 26            13 / 26",
    "    samp_list_kernel   MsdapOp          14 / 28            13 / 28            13 / 28",
    "    samp_list_kernel   FdapOp (new)     14 / 28            13 / 28            13 / 28", "",
    "No new instance uses scratch, AGPRs or LDS.  SGPRs: 76-78 (forward), 94 (coordinate backward), 50 / 54 (lists), against "
    "71-73, 90 and 47 / 50 of `FdaOp` and 78, 92 and 50 / 54 of `MsdapOp`: the level table and the eight prefix sums are read "
    "with constant indices only and stay in scalar registers.  Every new instance has the occupancy of its `FdaOp` "
    "counterpart.", "",
]

NOTES = [
    "## Reading the table", "",
    "The decoder steps are a handful of short kernels with autograd around them, so their figures move with the box and with "
    "the host more than the 8400-query lines do; the verdicts are per line against the 5 % spread.  What the native route "
    "leaves out of the composed one is framework work on the packed tensor: two slice copies, the softmax, its backward and "
    "the concatenation of the two gradients.  What it adds is the second walk over the taps in the coordinate backward "
    "(`samp_pair_sum`), which loads the corners twice.  On the 8400-query lines the list build and the gather of `grad_value` "
    "dominate either route.  The equal-count lines measure the level lookup against `flash_deform_attn`: the compare chain "
    "against the division, everything else bit-identical.  The block line carries, on either route, the four projections, the "
    "location arithmetic and every parameter gradient, which are most of its step; there the fused block trades the framework "
    "softmax and its backward for one `cat` into a 3K-wide row and the two slice copies of that `cat`'s backward.  The "
    "operator is on request; nothing routes to it.  A caution on the fp32 300-query lines: the composed route there has been "
    "seen at two levels on one build, about 0.23 ms and about 0.31 ms (its many short framework launches are host-bound), "
    "so a ratio near 1.36x on such a line is the upper of the two readings; the bf16 lines of the same shape, which did not "
    "move, are the figure to plan with.", "",
]


def outcome(rows):
    """One paragraph from the verdicts: how many operator lines are faster / level / slower than the composed route."""
    def side(nat, other):
        return "slower" if nat[0] > other[0] * (1 + SPREAD) else "faster" if nat[0] * (1 + SPREAD) < other[0] else "level"

    ops = [(name, res) for name, res in rows if not name.startswith("block")]
    tally = {"faster": [], "level": [], "slower": []}
    for name, res in ops:
        tally[side(res["native"], res["composed"])].append(res["composed"][0] / res["native"][0])
    text = "Outcome against the composed route, %d operator lines: " % len(ops) + "; ".join(
        "%d %s (%.2fx - %.2fx)" % (len(v), k, min(v), max(v)) for k, v in tally.items() if v) + "."
    uni = [res["flash_deform_attn"][0] / res["native"][0] for _, res in ops if "flash_deform_attn" in res]
    if uni:
        text += "  Against `flash_deform_attn` at equal counts: %.2fx - %.2fx on %d lines." % (min(uni), max(uni), len(uni))
    for name, res in rows:
        if name.startswith("block"):
            how = {"faster": "faster than", "slower": "slower than", "level": "level with"}[side(res["native"], res["composed"])]
            text += "  The whole block is %s `MSDeformableAttention`: %.3f against %.3f ms (%.2fx)." % (
                how, res["native"][0], res["composed"][0], res["composed"][0] / res["native"][0])
    return text


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
    loc = torch.rand(N, Lq, M, K, 2, generator=gen) * 1.1 - 0.05
    logits = torch.randn(N, Lq, M, K, generator=gen)
    loc_attn = fdap.pack_loc_attn_points(loc, logits).to(coord_dtype).cuda()
    go = torch.randn(N, Lq, M * D, generator=gen).to(dtype).cuda()
    return value, loc_attn, go


def _leaves(value, loc_attn):
    return tuple(t.detach().requires_grad_(True) for t in (value, loc_attn))


def native_step(value, levels, points, loc_attn, go):
    def step():
        v, la = _leaves(value, loc_attn)
        out = fdap.flash_deform_attn_points(v, levels, points, la)
        out.backward(go)
        return out, v.grad, la.grad
    return step


def composed_step(value, levels, points, loc_attn, go):
    """What a user has on the parent commit: two slices of the same packed tensor, ``torch.softmax``,
    ``ms_deform_attn_points``; autograd runs the softmax's backward and concatenates the two gradients."""
    K = sum(points)

    def step():
        v, la = _leaves(value, loc_attn)
        loc = la[..., :2 * K].unflatten(-1, (K, 2))
        attn = torch.softmax(la[..., 2 * K:], -1)
        out = msdap.ms_deform_attn_points(v, levels, points, loc, attn)
        out.backward(go)
        return out, v.grad, la.grad
    return step


def uniform_step(value, levels, points, loc_attn, go):
    """``flash_deform_attn`` itself on the same memory: the equal-count lines only."""
    P = points[0]

    def step():
        v, la = _leaves(value, loc_attn)
        out = fda.flash_deform_attn(v, levels, la, P)
        out.backward(go)
        return out, v.grad, la.grad
    return step


def _interleaved(steps, reps, rounds):
    for _ in range(2):   # warm-up, interleaved like the measurement: allocator, kernel loads, clocks
        for step in steps.values():
            timed(step, reps)
    ms = {r: [] for r in steps}
    for _ in range(rounds):
        for r, step in steps.items():
            ms[r].append(timed(step, reps))
    return {r: (statistics.median(v), min(v), max(v)) for r, v in ms.items()}


def measure(shape, dtype, coord_dtype, reps, rounds):
    _, levels, points, _ = shape
    t = make(shape, dtype, coord_dtype)
    args = (t[0], levels, points, t[1], t[2])
    steps = {"native": native_step(*args), "composed": composed_step(*args)}
    if len(set(points)) == 1:
        steps["flash_deform_attn"] = uniform_step(*args)
    want = steps["native"]()
    for r, step in steps.items():   # the routes compute the same thing
        for u, v in zip(step(), want):
            u, v = u.detach(), v.detach()
            err = float((u.double() - v.double()).abs().max() / max(1.0, float(v.double().abs().max())))
            assert err <= (1e-4 if v.dtype == torch.float32 and dtype == torch.float32 else 3e-2), (r, err)
    return _interleaved(steps, reps, rounds), t


def measure_block(reps, rounds):
    """``MSDeformableAttentionFused`` against ``MSDeformableAttention`` with the same parameters: one decoder-layer step under
    bf16 autocast, forward + backward with every parameter gradient."""
    levels, points = PYRAMID, [3, 6, 3]
    S, C = sum(h * w for h, w in levels), M * D
    torch.manual_seed(3)
    theirs = msdap.MSDeformableAttention(embed_dim=C, num_heads=M, num_levels=3, num_points=points).cuda()
    with torch.no_grad():
        theirs.sampling_offsets.weight.normal_(0, 0.02)
        theirs.attention_weights.weight.normal_(0, 0.2)
    ours = fdap.MSDeformableAttentionFused(embed_dim=C, num_heads=M, num_levels=3, num_points=points).cuda()
    ours.load_state_dict(theirs.state_dict())
    query = torch.randn(N, BLOCK_LQ, C, device="cuda")
    flat = torch.randn(N, S, C, device="cuda")
    boxes = torch.cat([torch.rand(N, BLOCK_LQ, 1, 2, device="cuda") * 0.8 + 0.1, torch.rand(N, BLOCK_LQ, 1, 2, device="cuda") * 0.3 + 0.05], -1)
    go = torch.randn(N, BLOCK_LQ, C, device="cuda").bfloat16()

    def step_of(mod):
        def step():
            mod.zero_grad(set_to_none=True)
            q, f = query.detach().requires_grad_(True), flat.detach().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = mod(q, boxes, f, levels)
            y.backward(go)
            return y, q.grad, f.grad
        return step

    steps = {"native": step_of(ours), "composed": step_of(theirs)}
    for u, v in zip(steps["native"](), steps["composed"]()):
        u, v = u.detach(), v.detach()
        err = float((u.double() - v.double()).abs().max() / max(1.0, float(v.double().abs().max())))
        assert err <= 3e-2, err
    return _interleaved(steps, reps, rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--modes", default="float32,bfloat16,bfloat16+float32")
    ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))))
    ap.add_argument("--no-block", action="store_true")
    ap.add_argument("--commit", default="")
    ap.add_argument("--write")
    a = ap.parse_args()
    rows = []
    for i in (int(s) for s in a.shapes.split(",") if s):
        for mode in a.modes.split(","):
            dtype = getattr(torch, mode.split("+")[0])
            coord_dtype = getattr(torch, mode.split("+")[1]) if "+" in mode else dtype
            shape = SHAPES[i]
            res, t = measure(shape, dtype, coord_dtype, a.reps, a.rounds)
            name = "%s_%s_Lq%d_%s" % (shape[0], "-".join(str(p) for p in shape[2]), t[1].shape[1], mode.replace("float", "f"))
            rows.append((name, res))
            del t
            torch.cuda.empty_cache()
    if not a.no_block:
        rows.append(("block_3-6-3_Lq%d_autocast_bf16" % BLOCK_LQ, measure_block(a.reps, a.rounds)))
    for name, res in rows:
        for r, (med, lo, hi) in res.items():
            print(json.dumps(dict(shape=name, route=r, median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4))),
                  flush=True)
    if a.write:
        write_markdown(a.write, rows, a)


def verdict(nat, other, what):
    if nat[0] > other[0] * (1 + SPREAD):
        v = "SLOWER than %s beyond the spread" % what
    elif nat[0] * (1 + SPREAD) < other[0]:
        v = "FASTER than %s beyond the spread" % what
    else:
        v = "within the spread of %s (level)" % what
    return "%s: %.3f vs %.3f ms, %.2fx" % (v, nat[0], other[0], other[0] / nat[0])


def write_markdown(path, rows, a):
    out = ["# Packed deformable attention with a point count per level: step times against the route a user had before", "",
           "Written by `tools/bench_fdap.py --write` (forward + backward through autograd, N = %d, M = %d, D = %d, levels "
           "80x80 / 40x40 / 20x20; median of %d rounds of %d steps, the routes interleaved in one process).  Box: %s.  "
           "Parent commit: %s." % (N, M, D, a.rounds, a.reps, torch.cuda.get_device_name(0), a.commit or "(not given)"), "",
           "`native`: `flash_deform_attn_points`.  `composed`: two slices of the same packed tensor, `torch.softmax`, "
           "`ms_deform_attn_points`, autograd's softmax backward and concatenation of the two gradients.  `flash_deform_attn`: "
           "the existing packed operator on the same memory, equal counts only.  The shape names carry the point counts and Lq "
           "(`encoder`: Lq = S = 8400); `f32` / `bf16` is the value dtype; `+f32`: an fp32 packed tensor.  The `block` line is "
           "`MSDeformableAttentionFused` (native) against `MSDeformableAttention` (composed) with the same parameters under "
           "bf16 autocast: projections, location arithmetic and every parameter gradient included.", "",
           "| shape | native ms (min - max) | composed ms (min - max) | composed / native | flash_deform_attn ms (min - max) |",
           "|---|---|---|---|---|"]
    verdicts = []
    for name, res in rows:
        nat, comp = res["native"], res["composed"]
        uni = res.get("flash_deform_attn")
        out.append("| %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %s |" % (
            (name,) + nat + comp + (comp[0] / nat[0], "%.3f (%.3f - %.3f)" % uni if uni else "")))
        verdicts.append("%s: native is %s" % (name, verdict(nat, comp, "the composed route")))
        if uni:
            verdicts.append("%s: native is %s" % (name, verdict(nat, uni, "`flash_deform_attn`")))
    out += ["", "Spread quoted by the project for same-box comparisons: %d %%.  %s" % (round(SPREAD * 100), outcome(rows)), ""]
    out += ["- " + v for v in verdicts] + [""]
    out += NOTES + RESOURCES
    with open(path, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
