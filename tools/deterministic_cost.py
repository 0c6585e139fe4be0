#!/usr/bin/env python3
"""Cost of deterministic mode (include/mdconv.h: MDCONV_FLAG_DETERMINISTIC): forward + backward of the bench.py
workloads with and without the flag, and one collision-heavy call (every offset of a 3x3, 56 x 56 layer pointing at one
pixel: two scatter lists of K * S_o entries per image).  Timing as tools/bench_configs.py; profiles/deterministic.md
holds the table.

    python tools/deterministic_cost.py [cfg2 cfg2_f16 cfg3 cfg4 cfg5 collide]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from modulated_deform_conv_amd import _capi  # noqa: E402
from tools.bench_configs import timeit  # noqa: E402

bench.WORKLOADS["cfg2_f16"] = dict(bench.WORKLOADS["cfg2"], dtype="f16",
                                   what="ModulatedDeformConv2d 3x3, C_in=C_out=256, 56x56, fp16 (twin of the headline shape)")
bench.WORKLOADS["collide"] = dict(bench.WORKLOADS["cfg2"], B=8,
                                  what="headline layer, B=8, every sample of an image at position (20.5, 20.5)")


def workload(name):
    wl = bench.Workload("collide" if name == "collide" else name, "cuda")
    if name == "collide":
        H, W = wl.cfg["sp"]
        oy = torch.arange(H, dtype=torch.float32).view(H, 1).expand(H, W)
        ox = torch.arange(W, dtype=torch.float32).view(1, W).expand(H, W)
        off = torch.empty_like(wl.off)
        for tap in range(9):
            off[:, 2 * tap] = (20.5 - (oy - 1 + tap // 3)).to(off)
            off[:, 2 * tap + 1] = (20.5 - (ox - 1 + tap % 3)).to(off)
        wl.off = off
    return wl


def main():
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["cfg2", "cfg2_f16", "cfg3", "cfg4", "cfg5", "collide"]
    print("| workload | B | kernels | fwd ms | bwd ms | bwd ms, deterministic | bwd cost | step cost |")
    print("|---|---|---|---|---|---|---|---|")
    for name in names:
        wl = workload(name)
        n = 3 if name == "collide" else 10
        with _capi.deterministic(False):
            tf = timeit(wl.forward, n)
            tb = timeit(wl.backward, n)
        kern = _capi.last_kernels()
        with _capi.deterministic(True):
            td = timeit(wl.backward, n)
        print("| %s | %d | %s | %.3f | %.3f | %.3f | %+.1f %% | %+.1f %% |"
              % (name, wl.B, kern, tf, tb, td, (td / tb - 1) * 100, ((tf + td) / (tf + tb) - 1) * 100), flush=True)
        del wl
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
