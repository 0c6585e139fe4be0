#!/usr/bin/env python3
"""Forward + backward time of fp32 sampling (include/mdconv.h: MDCONV_SAMPLING_F32) against the same layer with every
tensor 16-bit and with every tensor fp32, one GPU, default kernel path, captured steps replayed (no host latency).

    python tools/sampling_dtype_bench.py [headline|cfg3|cfg5|flow|small3d] ...

Target: fp32 sampling <= 1.10x the all-16-bit step.  Offsets / masks are read and their gradients written in fp32, so the
16-bit kernels move twice the sampling bytes; the line to watch is `flow` (DG = 8 with 64 channels: 216 offset / mask
values per pixel against 64 input channels)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modulated_deform_conv_amd import MDCONV_CUDA as M  # noqa: E402
from modulated_deform_conv_amd import _capi  # noqa: E402

# (nd, B, C, O, spatial, groups, deformable groups, dilation, 16-bit dtype)
LAYERS = {
    "headline": (2, 8, 256, 256, (56, 56), 1, 1, 1, torch.float16),   # fp16 twin of the headline layer, B = 8
    "cfg3": (2, 32, 256, 256, (56, 56), 32, 4, 1, torch.float16),      # bench.py cfg3 shard
    "cfg5": (3, 8, 128, 128, (16, 64, 64), 1, 1, 2, torch.float16),    # bench.py cfg5 shard
    "flow": (2, 16, 64, 64, (64, 64), 1, 8, 1, torch.bfloat16),        # flow-guided alignment-like layer
    "small3d": (3, 2, 64, 64, (8, 16, 16), 1, 1, 1, torch.bfloat16),
}


def timeit(fn, n):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def step_fn(name, dtype, sdtype):
    nd, B, C, O, sp, G, DG, dil, _ = LAYERS[name]
    K = 3 ** nd
    osz = sp   # stride 1, padding = dilation
    g = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s, dt=dtype: torch.randn(*s, device="cuda", generator=g).to(dt)
    x, w, b = rn(B, C, *sp), rn(O, C // G, *(3,) * nd) * 0.05, rn(O)
    off, m = rn(B, DG * nd * K, *osz, dt=sdtype) * 2, torch.sigmoid(rn(B, DG * K, *osz, dt=sdtype))
    go = rn(B, O, *osz)
    geo = (3,) * nd + (1,) * nd + (dil,) * nd + (dil,) * nd + (G, DG, 64, True)
    if nd == 2:
        def step():
            M.modulated_deform_conv2d_forward_cuda(x, w, b, off, m, *geo)
            M.modulated_deform_conv2d_backward_cuda(x, w, b, off, m, go, *geo)
    else:
        out = torch.empty(B, O, *osz, device="cuda", dtype=dtype)
        gi, gw, gb, goff, gm = (torch.zeros_like(t) for t in (x, w, b, off, m))

        def step():
            M.modulated_deform_conv3d_forward_cuda(x, w, b, off, m, out, *geo)
            M.modulated_deform_conv3d_backward_cuda(x, w, b, off, m, gi, gw, gb, goff, gm, go, *geo)
    return step


def graph_time(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(); step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    fam = _capi.last_kernels()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return timeit(graph.replay, 20), fam


def run(name):
    dt = LAYERS[name][-1]
    t16, f16 = graph_time(step_fn(name, dt, dt))
    ts, fs = graph_time(step_fn(name, dt, torch.float32))
    t32, f32 = graph_time(step_fn(name, torch.float32, torch.float32))
    print("%-9s %s  all-16-bit %.3f ms (%s)  fp32 sampling %.3f ms (%s)  all-fp32 %.3f ms (%s)  ratio %.3f" % (
        name, str(dt).replace("torch.", ""), t16, f16, ts, fs, t32, f32, ts / t16), flush=True)
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for n in (sys.argv[1:] or list(LAYERS)):
        run(n)
