"""Step time (forward + backward) of deformable RoI pooling (include/mdconv.h, "Deformable RoI pooling"; csrc/droi_*.hip)
against a composition of plain PyTorch -- what a detector head uses without the extension -- and its autograd backward.  Two
compositions are timed and the FASTER one is the yardstick of a line:

    gather       an explicit four-corner gather, vectorised over the RoIs (in chunks that bound its memory), the grid padded
                 to the largest grid of the call
    grid_sample  one `F.grid_sample` (border padding, align_corners) and one mean per RoI; RoIAlign's clamp without its gate,
                 so a sample more than one pixel outside the map is clamped where the operator drops it

    python tools/bench_droi.py [--reps 5] [--rounds 5] [--modes float32,bfloat16,bfloat16+float32] [--shapes 0,1,..] [--write FILE]

A mode is the value dtype, `+float32` for fp32 offsets beside 16-bit values.  Shapes are detector-like: 256 channels, 7 x 7
bins, 512 and 1024 RoIs over a 200 x 304 and a 50 x 76 map, sampling_ratio 2 and adaptive (max_grid 8).  The slower
composition is found with one warm step each; the native step and the faster composition are then timed interleaved in one
process: `rounds` measurements of `reps` steps each, median with min and max.  The native forward, the native backward without
grad_input (the offset-gradient kernel alone) and the full native backward are timed the same way, so the list build + gather
is their difference.  One JSON line per measurement; --write FILE writes the table as markdown."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from modulated_deform_conv_amd import _capi, droi

SPREAD = 0.05   # box spread the project quotes for same-box comparisons
B, C, PH, PW, GAMMA, MAX_GRID = 2, 256, 7, 7, 0.1, 8
# (map H, W, RoIs, sampling_ratio)
SHAPES = [(H, W, R, ratio) for H, W in ((200, 304), (50, 76)) for R in (512, 1024) for ratio in (2, 0)]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def make(shape, dtype, coord_dtype):
    """RoIs in feature-map coordinates (spatial_scale 1) of 1/16 to 1/3 of the map's height, inside the map."""
    H, W, R, _ = shape
    gen = torch.Generator().manual_seed(1)
    inp = torch.randn(B, H, W, C, generator=gen).to(dtype).cuda()
    h = (1 / 16 + torch.rand(R, generator=gen) * (1 / 3 - 1 / 16)) * H
    w = h * (0.5 + torch.rand(R, generator=gen))
    x1 = torch.rand(R, generator=gen) * (W - w)
    y1 = torch.rand(R, generator=gen) * (H - h)
    b = torch.randint(0, B, (R,), generator=gen).float()
    rois = torch.stack([b, x1 + 0.5, y1 + 0.5, x1 + w + 0.5, y1 + h + 0.5], 1).cuda()
    off = (torch.randn(R, 2, PH, PW, generator=gen) * 0.5).to(coord_dtype).cuda()
    go = torch.randn(R, PH, PW, C, generator=gen).to(dtype).cuda()
    return inp, rois, off, go


def positions(rois, off, ratio):
    """fp32 sample coordinates y, x [R, PH, PW, G], the grids gh, gw [R] and G, the largest grid of the call."""
    x1s, y1s, x2s, y2s = (rois[:, i] - 0.5 for i in (1, 2, 3, 4))
    rw, rh = x2s - x1s, y2s - y1s
    bw, bh = rw / PW, rh / PH
    if ratio > 0:
        gh = gw = torch.full_like(rw, ratio).long()
    else:
        gh, gw = bh.ceil().clamp(0, MAX_GRID).long(), bw.ceil().clamp(0, MAX_GRID).long()
    G = int(max(gh.max(), gw.max()))   # (a host synchronisation: part of what the composition costs)
    idx = torch.arange(G, device=rois.device)
    half = (idx.float() + 0.5)[None, None, None, :]
    ph = torch.arange(PH, device=rois.device).float()[None, :, None, None]
    pw = torch.arange(PW, device=rois.device).float()[None, None, :, None]
    o = off.float()
    y = (y1s[:, None, None] + GAMMA * rh[:, None, None] * o[:, 1])[..., None] + ph * bh[:, None, None, None] + \
        half * (bh / gh.clamp(min=1))[:, None, None, None]
    x = (x1s[:, None, None] + GAMMA * rw[:, None, None] * o[:, 0])[..., None] + pw * bw[:, None, None, None] + \
        half * (bw / gw.clamp(min=1))[:, None, None, None]
    return y, x, gh, gw, G, idx


def _axis(loc, size, live):
    gate = ((loc >= -1) & (loc <= size) & live).float()
    c = loc.clamp(min=0)
    lo = c.floor().clamp(max=size - 1)
    frac = torch.where(lo >= size - 1, torch.zeros_like(c), c - lo)
    hi = (lo + 1).clamp(max=size - 1)
    return lo.long(), hi.long(), (1 - frac) * gate, frac * gate


def gather_forward(inp, rois, off, ratio):
    H, W = inp.shape[1], inp.shape[2]
    y, x, gh, gw, G, idx = positions(rois, off, ratio)
    ylo, yhi, wy0, wy1 = _axis(y, H, (idx[None] < gh[:, None])[:, None, None, :])
    xlo, xhi, wx0, wx1 = _axis(x, W, (idx[None] < gw[:, None])[:, None, None, :])
    inv = 1.0 / (gh * gw).clamp(min=1).float()
    chunk = max(1, (1 << 26) // (PH * PW * G * G * C))   # at most 2^26 gathered elements per corner and chunk
    outs = []
    for r0 in range(0, rois.shape[0], chunk):
        s = slice(r0, r0 + chunk)
        bb = rois[s, 0].long()[:, None, None, None, None]
        acc = 0
        for yi, wy in ((ylo, wy0), (yhi, wy1)):
            for xi, wx in ((xlo, wx0), (xhi, wx1)):
                v = inp[bb, yi[s][..., :, None], xi[s][..., None, :]]   # [r, PH, PW, G, G, C]
                wgt = (wy[s][..., :, None] * wx[s][..., None, :] * inv[s, None, None, None, None]).to(inp.dtype)
                acc = acc + torch.einsum("rpqyx,rpqyxc->rpqc", wgt, v)
        outs.append(acc)
    return torch.cat(outs)


def grid_sample_forward(inp, rois, off, ratio):
    H, W = inp.shape[1], inp.shape[2]
    img = inp.permute(0, 3, 1, 2)
    y, x, gh, gw, G, idx = positions(rois, off, ratio)
    gy, gx = (2 * y / (H - 1) - 1).to(inp.dtype), (2 * x / (W - 1) - 1).to(inp.dtype)
    bs, ghs, gws = rois[:, 0].long().tolist(), gh.tolist(), gw.tolist()
    outs = []
    for r in range(rois.shape[0]):
        a, c = max(ghs[r], 1), max(gws[r], 1)
        yy = gy[r, :, :, :a].permute(0, 2, 1)[:, :, :, None].expand(PH, a, PW, c)
        xx = gx[r, :, :, :c][:, None, :, :].expand(PH, a, PW, c)
        grid = torch.stack([xx, yy], -1).reshape(1, PH * a, PW * c, 2)
        s = F.grid_sample(img[bs[r]:bs[r] + 1], grid, mode="bilinear", padding_mode="border", align_corners=True)
        outs.append(s.view(C, PH, a, PW, c).mean((2, 4)))
    return torch.stack(outs).permute(0, 2, 3, 1)


def composed(forward, inp, rois, off, go, ratio):
    def step():
        i, o = inp.detach().requires_grad_(True), off.detach().requires_grad_(True)
        out = forward(i, rois, o, ratio)
        return (out,) + torch.autograd.grad(out, (i, o), go)
    return step


def measure(shape, dtype, coord_dtype, reps, rounds):
    ratio = shape[3]
    inp, rois, off, go = t = make(shape, dtype, coord_dtype)
    geo = dict(output_size=(PH, PW), spatial_scale=1.0, sampling_ratio=ratio, gamma=GAMMA, max_grid=MAX_GRID)
    routes = {"gather": composed(gather_forward, inp, rois, off, go, ratio),
              "grid_sample": composed(grid_sample_forward, inp, rois, off, go, ratio)}
    once = {}
    for name, step in routes.items():   # one warm step each decides which composition is the yardstick
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        once[name] = (time.perf_counter() - t0) * 1e3
    best = min(once, key=once.get)
    steps = {
        "native": lambda: (droi.deform_roi_pool_forward(inp, rois, off, **geo),
                           droi.deform_roi_pool_backward(inp, rois, off, go, **geo)),
        "composed": routes[best],
        "native_fwd": lambda: droi.deform_roi_pool_forward(inp, rois, off, **geo),
        "native_bwd": lambda: droi.deform_roi_pool_backward(inp, rois, off, go, **geo),
        "native_bwd_no_grad_input": lambda: droi.deform_roi_pool_backward(inp, rois, off, go, need_grad_input=False, **geo),
    }
    for step in steps.values():
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    ms = {r: [] for r in steps}
    for _ in range(rounds):
        for r, step in steps.items():
            ms[r].append(timed(step, reps))
    d = droi._desc(inp, rois, off, (PH, PW), 1.0, ratio, GAMMA, MAX_GRID)
    ws = int(_capi.lib().mdconv_droi_workspace_bytes(ctypes.byref(d), 1))
    # the compositions follow RoIAlign's clamp too (`gather` its gate as well): the outputs agree, which keeps the comparison honest
    err = float((steps["native_fwd"]().float() - routes[best]()[0].float()).abs().max())
    return {r: (statistics.median(v), min(v), max(v)) for r, v in ms.items()}, ws, best, once, err


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
            H, W, R, ratio = shape = SHAPES[i]
            res, ws, best, once, err = measure(shape, dtype, coord_dtype, a.reps, a.rounds)
            name = "%dx%d_R%d_%s_%s" % (H, W, R, "ratio%d" % ratio if ratio else "adaptive", mode.replace("float", "f"))
            for r, (med, lo, hi) in res.items():
                print(json.dumps(dict(shape=name, route=r, composition=best, workspace_bytes=ws, median_ms=round(med, 4),
                                      min_ms=round(lo, 4), max_ms=round(hi, 4), one_step_ms={k: round(v, 2) for k, v in once.items()},
                                      max_abs_diff=err)), flush=True)
            rows.append((name, res, ws, best, once, err))
            torch.cuda.empty_cache()
    if a.write:
        write_markdown(a.write, rows, a)


def write_markdown(path, rows, a):
    out = ["## Step times against the composed route", "",
           "Written by `tools/bench_droi.py --write` (forward + backward, B = %d, C = %d, %d x %d bins, gamma = %g, max_grid = %d; "
           "median of %d rounds of %d steps, the routes interleaved in one process).  Box: %s.  Commit: %s." % (
               B, C, PH, PW, GAMMA, MAX_GRID, a.rounds, a.reps, torch.cuda.get_device_name(0), a.commit or "(not given)"), "",
           "`composed`: the faster of two pure-PyTorch compositions with their autograd backward, in the value dtype -- `gather` (an "
           "explicit four-corner gather over all RoIs) and `grid_sample` (one `F.grid_sample` per RoI); `one step ms` is the single "
           "warm step of each that picked it.  `offset` is the native backward with `MDCONV_FLAG_NO_GRAD_INPUT` (the offset-gradient "
           "kernel alone), `lists + gather` the full backward minus it.  `max diff`: largest absolute difference of the two "
           "forward outputs.  `f32` / `bf16` is the value dtype; `+f32`: fp32 offsets.", "",
           "| shape | native ms (min - max) | composed ms (min - max) | composed / native | composition (one step ms: gather, grid_sample) | fwd ms | offset ms | lists + gather ms | workspace MiB | max diff |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for name, res, ws, best, once, err in rows:
        nat, comp = res["native"], res["composed"]
        out.append("| %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %s (%.1f, %.1f) | %.3f | %.3f | %.3f | %.1f | %.1e |" % (
            name, nat[0], nat[1], nat[2], comp[0], comp[1], comp[2], comp[0] / nat[0], best, once["gather"], once["grid_sample"],
            res["native_fwd"][0], res["native_bwd_no_grad_input"][0], res["native_bwd"][0] - res["native_bwd_no_grad_input"][0],
            ws / 2.0 ** 20, err))
        faster = nat[0] * (1 + SPREAD) < comp[0]
        verdicts.append("%s: the native operator is %s the composed route beyond the spread: %.3f vs %.3f ms" % (
            name, "FASTER than" if faster else "NOT FASTER than", nat[0], comp[0]))
    out += ["", "Spread quoted by the project for same-box comparisons: %d %%." % round(SPREAD * 100), ""] + ["- " + v for v in verdicts] + [""]
    with open(path, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
