"""Step time (forward + backward, through autograd) of anchored packed deformable attention (include/mdconv_afda.h;
csrc/afda_host.hip on csrc/samp_core.hpp) against the route a user has without it: ``MSDeformableAttention._locations``-style
framework arithmetic on the same raw offsets and boxes, ``pack_loc_attn_points`` and ``flash_deform_attn_points``; and
whole-block lines, ``MSDeformableAttentionAnchored`` against ``MSDeformableAttentionFused`` and ``MSDeformableAttention``.

    python tools/bench_afda.py [--reps 20] [--rounds 7] [--modes float32,bfloat16,bfloat16+float32] [--shapes 0,1,2,3,4,5]
                               [--no-block] [--commit TEXT] [--write FILE]

A mode is the value dtype, `+float32` for an fp32 packed row beside 16-bit values.  Per (shape, mode) the routes are checked
against each other once and then timed interleaved in one process: `rounds` measurements of `reps` steps each, median with
min and max.  One JSON line per measurement; --write FILE writes the table as markdown."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from modulated_deform_conv_amd import afda, fdap, msdap

SPREAD = 0.05   # box spread the project quotes for same-box comparisons
N, M, D = 8, 8, 32
PYRAMID = [(80, 80), (40, 40), (20, 20)]   # a 640 x 640 input at strides 8, 16, 32
OFFSET_SCALE = 0.5
# (name, levels, points, Lq; None: one query per value row)
SHAPES = [("dfine_decoder", PYRAMID, (3, 6, 3), 300), ("dfine_decoder", PYRAMID, (3, 6, 3), 500),
          ("encoder", PYRAMID, (3, 6, 3), None),
          ("rtdetrv2_decoder", PYRAMID, (4, 4, 4), 300), ("rtdetrv2_decoder", PYRAMID, (4, 4, 4), 500),
          ("encoder", PYRAMID, (4, 4, 4), None)]
BLOCK_LQ = 300

# VGPRs per instance (`tools/kres.py fda_host | msdap_host | fdap_host | afda_host`).  Instances are named (value type,
# coordinate type); the list kernels by the coordinate type.
RESOURCES = [
    "## Kernel resources (`tools/kres.py fda_host`, `msdap_host`, `fdap_host`, `afda_host`)", "",
    "The shared coordinate backward gained one hook (`SampTapGrads`, `Op::tap_grads`), discarded at compile time for every "
    "policy without `kTapGrads`.  The `tools/kres.py` lines of `fda_host`, `msdap_host` and `fdap_host` (VGPRs, AGPRs, SGPRs, "
    "scratch, occupancy, LDS of every instance) were taken before and after the change and compare equal byte for byte; "
    "they are the `FdaOp`, `MsdapOp` and `FdapOp` rows below.  `AfdaOp` has `FdapOp`'s instance count (5 + 5 + 6): `Lr`, `R` "
    "and `offset_scale` are run-time data of the geometry.  VGPRs (occupancy in waves per SIMD):", "",
    "    kernel                  policy           f32/f32   f16/f16   f16/f32   bf16/bf16   bf16/f32",
    "    samp_fwd_kernel         FdaOp            54 (8)    58 (8)    58 (8)    60 (8)      60 (8)",
    "    samp_fwd_kernel         MsdapOp          50 (8)    70 (7)    70 (7)    68 (7)      68 (7)",
    "    samp_fwd_kernel         FdapOp           52 (8)    58 (8)    58 (8)    60 (8)      60 (8)",
    "    samp_fwd_kernel         AfdaOp (new)     59 (7)    81 (5)    81 (5)    77 (6)      77 (6)",
    "    samp_bwd_coord_kernel   FdaOp            78 (6)    84 (5)    84 (5)    90 (5)      89 (5)",
    "    samp_bwd_coord_kernel   MsdapOp          72 (7)    78 (6)    78 (6)    95 (5)      94 (5)",
    "    samp_bwd_coord_kernel   FdapOp           76 (6)    83 (5)    83 (5)    89 (5)      88 (5)",
    "    samp_bwd_coord_kernel   AfdaOp (new)     106 (4)   112 (4)   112 (4)   129 (3)     128 (4)", "",
    "    kernel             policy           f32 count / fill   f16 count / fill   bf16 count / fill",
    "    samp_list_kernel   FdaOp            14 / 26            13 / 26            13 / 26",
    "    samp_list_kernel   MsdapOp          14 / 28            13 / 28            13 / 28",
    "    samp_list_kernel   FdapOp           14 / 28            13 / 28            13 / 28",
    "    samp_list_kernel   AfdaOp (new)     21 / 28            20 / 28            20 / 28", "",
    "    afda_ref_reduce_kernel (new)         8 VGPRs, 16 SGPRs, occupancy 8", "",
    "No new instance uses scratch, AGPRs or LDS.  SGPRs of `AfdaOp`: 106 (forward and coordinate backward: the allocation's "
    "ceiling), 66 / 70 (lists), against 76-78, 94 and 50 / 54 of `FdapOp`: the geometry carries three more per-level tables "
    "(`inv_points`, `invW`, `invH`) beside the level table and the prefix sums, all read with constant indices.  The new "
    "instances pay for the reference row in the pair context (4 VGPRs), the running sums of grad_reference_points (4) and the "
    "location arithmetic with registers: the coordinate backward runs at 3-4 waves per SIMD where `FdapOp` runs at 5-6, the "
    "16-bit forwards at 5-6 where it runs at 8.  That is the known cost of this version; the step times above are measured "
    "with it.", "",
]

NOTES = [
    "## Reading the table", "",
    "The decoder steps are a handful of short kernels with autograd around them, so their figures move with the box and with "
    "the host more than the 8400-query lines do; the verdicts are per line against the 5 % spread.  `composed` is what a user "
    "has without the operator: the reference arithmetic of `MSDeformableAttention._locations` in framework operators on the "
    "same raw offsets and boxes (fp32, as that method does it; its backward included), one `cat` with the logits, "
    "`flash_deform_attn_points`, and the slice copies of the `cat`'s backward.  Under the `bf16` mode the composed route "
    "therefore hands the operator an fp32 packed tensor, exactly as the existing blocks do, while the native route reads the "
    "bf16 row as it is.  The reference needs no gradient on these lines (the decoders detach it); the `+gref` lines give it "
    "one on both routes.  The block lines carry, on every route, the projections and every parameter gradient; the anchored "
    "block replaces two linears, the location arithmetic, the `cat` and their backward by one linear on a weight-sized `cat`.  "
    "The operator is on request; nothing routes to it.", "",
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
    boxes = torch.cat([torch.rand(N, Lq, 1, 2, generator=gen) * 0.8 + 0.1, torch.rand(N, Lq, 1, 2, generator=gen) * 0.3 + 0.05], -1).cuda()
    offs = torch.randn(N, Lq, M, 2 * K, generator=gen) * 3     # offsets of a few units, as the linear produces them
    logits = torch.randn(N, Lq, M, K, generator=gen)
    offs_attn = torch.cat([offs, logits], -1).to(coord_dtype).cuda()
    go = torch.randn(N, Lq, M * D, generator=gen).to(dtype).cuda()
    return value, boxes, offs_attn, go


def _leaves(gref, value, boxes, offs_attn):
    return (value.detach().requires_grad_(True), boxes.detach().requires_grad_(gref), offs_attn.detach().requires_grad_(True))


def native_step(value, levels, points, boxes, offs_attn, go, gref):
    def step():
        v, b, oa = _leaves(gref, value, boxes, offs_attn)
        out = afda.anchored_deform_attn(v, levels, points, b, oa, OFFSET_SCALE)
        out.backward(go)
        return out, v.grad, oa.grad, b.grad
    return step


def composed_step(value, levels, points, boxes, offs_attn, go, gref):
    """What a user has on the parent commit: ``_locations``' arithmetic in framework operators (fp32), one ``cat``,
    ``flash_deform_attn_points``."""
    K = sum(points)
    scale = torch.tensor([1.0 / n for n in points for _ in range(n)], dtype=torch.float32, device="cuda")[None, None, None, :, None]

    def step():
        v, b, oa = _leaves(gref, value, boxes, offs_attn)
        Nn, Lq = oa.shape[:2]
        offsets = oa[..., :2 * K].float().view(Nn, Lq, M, K, 2)
        ref = b.float()
        loc = ref[:, :, None, :, :2] + offsets * scale * ref[:, :, None, :, 2:] * OFFSET_SCALE
        out = fdap.flash_deform_attn_points(v, levels, points, fdap.pack_loc_attn_points(loc, oa[..., 2 * K:].float()))
        out.backward(go)
        return out, v.grad, oa.grad, b.grad
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


def _same(tag, got, want, tol):
    for what, u, v in zip(("output", "grad_value", "grad_packed", "grad_reference"), got, want):
        if u is None and v is None:
            continue
        u, v = u.detach(), v.detach()
        err = (u.double() - v.double()).abs() / max(1.0, float(v.double().abs().max()))
        # (the routes round the location differently, by an ulp: of some 10^5 unguarded random samples a few sit that close
        # to the lattice, change their cell and with it their gradient -- so a few elements in 10^4 may differ)
        assert float((err > tol).double().mean()) <= 1e-4, (tag, what, float(err.max()), float((err > tol).double().mean()))


def measure(shape, dtype, coord_dtype, reps, rounds, gref=False):
    _, levels, points, _ = shape
    t = make(shape, dtype, coord_dtype)
    args = (t[0], levels, points, t[1], t[2], t[3], gref)
    steps = {"native": native_step(*args), "composed": composed_step(*args)}
    _same("composed", steps["composed"](), steps["native"](), 1e-4 if dtype == coord_dtype == torch.float32 else 3e-2)
    return _interleaved(steps, reps, rounds), t


def measure_block(reps, rounds, autocast):
    """``MSDeformableAttentionAnchored`` against ``MSDeformableAttentionFused`` and ``MSDeformableAttention`` with the same
    parameters: one decoder-layer step, forward + backward with every parameter gradient, fp32 or under bf16 autocast."""
    levels, points = PYRAMID, [3, 6, 3]
    S, C = sum(h * w for h, w in levels), M * D
    torch.manual_seed(3)
    theirs = msdap.MSDeformableAttention(embed_dim=C, num_heads=M, num_levels=3, num_points=points).cuda()
    with torch.no_grad():
        theirs.sampling_offsets.weight.normal_(0, 0.02)
        theirs.attention_weights.weight.normal_(0, 0.2)
    fused = fdap.MSDeformableAttentionFused(embed_dim=C, num_heads=M, num_levels=3, num_points=points).cuda()
    ours = afda.MSDeformableAttentionAnchored(embed_dim=C, num_heads=M, num_levels=3, num_points=points).cuda()
    fused.load_state_dict(theirs.state_dict())
    ours.load_state_dict(theirs.state_dict())
    query = torch.randn(N, BLOCK_LQ, C, device="cuda")
    flat = torch.randn(N, S, C, device="cuda")
    boxes = torch.cat([torch.rand(N, BLOCK_LQ, 1, 2, device="cuda") * 0.8 + 0.1, torch.rand(N, BLOCK_LQ, 1, 2, device="cuda") * 0.3 + 0.05], -1)
    go = torch.randn(N, BLOCK_LQ, C, device="cuda")
    go = go.bfloat16() if autocast else go

    def step_of(mod):
        def step():
            mod.zero_grad(set_to_none=True)
            q, f = query.detach().requires_grad_(True), flat.detach().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                y = mod(q, boxes, f, levels)
            y.backward(go)
            return y, q.grad, f.grad
        return step

    steps = {"native": step_of(ours), "fused": step_of(fused), "composed": step_of(theirs)}
    want = steps["composed"]()
    for r in ("native", "fused"):
        _same(r, steps[r](), want, 3e-2 if autocast else 1e-4)
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
    measure(SHAPES[0], torch.float32, torch.float32, a.reps, 2)   # (discarded: the box's clocks, the allocator, first loads)
    for i in (int(s) for s in a.shapes.split(",") if s):
        for mode in a.modes.split(","):
            dtype = getattr(torch, mode.split("+")[0])
            coord_dtype = getattr(torch, mode.split("+")[1]) if "+" in mode else dtype
            shape = SHAPES[i]
            for gref in (False, True) if shape[3] == 300 else (False,):   # (the 300-query shapes also with grad_reference)
                res, t = measure(shape, dtype, coord_dtype, a.reps, a.rounds, gref)
                name = "%s_%s_Lq%d_%s%s" % (shape[0], "-".join(str(p) for p in shape[2]), t[2].shape[1], mode.replace("float", "f"),
                                            "+gref" if gref else "")
                rows.append((name, res))
                del t
                torch.cuda.empty_cache()
    if not a.no_block:
        rows.append(("block_3-6-3_Lq%d_autocast_bf16" % BLOCK_LQ, measure_block(a.reps, a.rounds, True)))
        rows.append(("block_3-6-3_Lq%d_f32" % BLOCK_LQ, measure_block(a.reps, a.rounds, False)))
    for name, res in rows:
        for r, (med, lo, hi) in res.items():
            print(json.dumps(dict(shape=name, route=r, median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4))),
                  flush=True)
    if a.write:
        write_markdown(a.write, rows, a)


def side(nat, other):
    return "slower" if nat[0] > other[0] * (1 + SPREAD) else "faster" if nat[0] * (1 + SPREAD) < other[0] else "level"


def verdict(nat, other, what):
    v = {"slower": "SLOWER than %s beyond the spread", "faster": "FASTER than %s beyond the spread",
         "level": "within the spread of %s (level)"}[side(nat, other)] % what
    return "%s: %.3f vs %.3f ms, %.2fx" % (v, nat[0], other[0], other[0] / nat[0])


def outcome(rows):
    """One paragraph from the verdicts."""
    ops = [(name, res) for name, res in rows if not name.startswith("block")]
    tally = {"faster": [], "level": [], "slower": []}
    for name, res in ops:
        tally[side(res["native"], res["composed"])].append(res["composed"][0] / res["native"][0])
    text = "Outcome against the composed route, %d operator lines: " % len(ops) + "; ".join(
        "%d %s (%.2fx - %.2fx)" % (len(v), k, min(v), max(v)) for k, v in tally.items() if v) + "."
    for name, res in rows:
        if name.startswith("block"):
            text += "  %s: `MSDeformableAttentionAnchored` is %s `MSDeformableAttentionFused` (%.3f against %.3f ms, %.2fx) and %s "\
                    "`MSDeformableAttention` (%.3f ms, %.2fx)." % (
                        name, {"faster": "faster than", "slower": "slower than", "level": "level with"}[side(res["native"], res["fused"])],
                        res["native"][0], res["fused"][0], res["fused"][0] / res["native"][0],
                        {"faster": "faster than", "slower": "slower than", "level": "level with"}[side(res["native"], res["composed"])],
                        res["composed"][0], res["composed"][0] / res["native"][0])
    return text


def write_markdown(path, rows, a):
    out = ["# Anchored packed deformable attention: step times against the route a user has without it", "",
           "Written by `tools/bench_afda.py --write` (forward + backward through autograd, N = %d, M = %d, D = %d, levels "
           "80x80 / 40x40 / 20x20, one box per query, offset_scale %.1f; median of %d rounds of %d steps, the routes "
           "interleaved in one process).  Box: %s.  Parent commit: %s." % (
               N, M, D, OFFSET_SCALE, a.rounds, a.reps, torch.cuda.get_device_name(0), a.commit or "(not given)"), "",
           "`native`: `anchored_deform_attn` on the raw packed row and the boxes.  `composed`: `_locations`-style framework "
           "arithmetic on the same offsets and boxes, `pack_loc_attn_points`, `flash_deform_attn_points`.  The shape names "
           "carry the point counts and Lq (`encoder`: Lq = S = 8400); `f32` / `bf16` is the value dtype and the packed row's; "
           "`+f32`: an fp32 packed row beside bf16 values; `+gref`: the boxes need a gradient.  The `block` lines are "
           "`MSDeformableAttentionAnchored` (native) against `MSDeformableAttentionFused` (fused) and `MSDeformableAttention` "
           "(composed) with the same parameters.", "",
           "| shape | native ms (min - max) | composed ms (min - max) | composed / native | fused block ms (min - max) |",
           "|---|---|---|---|---|"]
    verdicts = []
    for name, res in rows:
        nat, comp = res["native"], res["composed"]
        fused = res.get("fused")
        out.append("| %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %s |" % (
            (name,) + nat + comp + (comp[0] / nat[0], "%.3f (%.3f - %.3f)" % fused if fused else "")))
        if fused:
            verdicts.append("%s: native is %s" % (name, verdict(nat, fused, "`MSDeformableAttentionFused`")))
            verdicts.append("%s: native is %s" % (name, verdict(nat, comp, "`MSDeformableAttention`")))
        else:
            verdicts.append("%s: native is %s" % (name, verdict(nat, comp, "the composed route")))
    out += ["", "Spread quoted by the project for same-box comparisons: %d %%.  %s" % (round(SPREAD * 100), outcome(rows)), ""]
    out += ["- " + v for v in verdicts] + [""]
    out += NOTES + RESOURCES
    with open(path, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
