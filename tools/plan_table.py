#!/usr/bin/env python3
"""Developer aid: the library's routing and workspace answers for a fixed table of descriptors, one line each --
``mdconv_workspace_bytes``, ``mdconv_deterministic_supported`` and ``mdconv_input_layout_supported`` (channels-last).
Host only: needs no device (without one the library plans for 256 CUs and an occupancy of 4).  Two builds whose tables
are byte-identical route and size every listed call alike; load another build with MDCONV_LIB=<path>.

Descriptors: shapes x dtypes (fp32, fp16, bf16, fp16 / bf16 with fp32 sampling, fp64) x forward / backward x path
(auto, direct, mfma) x deterministic flag x input layout.  Shapes: tests/cases.py (CASES, EXTREME_F32, EXTREME_HP), the
shapes of tools/realistic_sweep.py, and the seeded generators of tests/cases.py and tools/fuzz_more.py.

usage: python tools/plan_table.py [--cases-only] [--seeds N] [-o FILE]"""
import argparse
import ctypes
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from modulated_deform_conv_amd import _capi  # noqa: E402
from tests import cases as C  # noqa: E402

DTYPES = (("f32", _capi.F32), ("f16", _capi.F16), ("bf16", _capi.BF16), ("f16s", _capi.F16 | _capi.SAMPLING_F32),
          ("bf16s", _capi.BF16 | _capi.SAMPLING_F32), ("f64", _capi.F64))
PATHS = (("auto", _capi.PATH_AUTO), ("direct", _capi.PATH_DIRECT), ("mfma", _capi.PATH_MFMA))
LAYOUT_CHANNELS_LAST = 1
COMBOS = len(DTYPES) * 2 * len(PATHS) * 2 * 2   # lines per shape


def shapes(cases_only=False, seeds=300):
    out = list(C.CASES)
    if cases_only:
        return out
    out += list(C.EXTREME_F32) + list(C.EXTREME_HP)
    import tools.realistic_sweep as rs
    for i, (name, op, B, ci, co, sz, dg) in enumerate(rs.SHAPES + rs.MORE):
        out.append(C._c("sweep%d_%s" % (i, name), op, B, ci, co, sz, 3, dgroups=dg))
    import tools.fuzz_more as fm
    for gen in (C.case_f32_wide, C.case_hp_wide, fm.case_f32, fm.case_hp, fm.case_hp_dg, fm.case_hp_pad):
        out += [gen(seed) for seed in range(seeds)]
    return out


def descriptor(case, dtype, path, det, layout):
    nd = C.ndim(case)
    d = _capi.MdconvDesc()
    d.ndim = nd | _capi.DESC_V2
    d.modulated = 1 if case["op"] in (C.M2, C.M3) else 0
    d.dtype = dtype
    d.batch, d.c_in, d.c_out = case["B"], case["C"], case["O"]
    for name, key in (("in_sz", "in_sz"), ("k_sz", "k"), ("stride", "stride"), ("pad", "padding"), ("dil", "dilation")):
        v = C._tup(case[key], nd)
        for a in range(3):
            getattr(d, name)[a] = v[a] if a < nd else (0 if name == "pad" else 1)
    d.groups, d.dgroups, d.in_step = case["groups"], case["dgroups"], case["in_step"]
    d.with_bias = 1 if case["bias"] else 0
    d.accumulate, d.input_layout, d.path = 1, layout, path
    d.flags = _capi.FLAG_DETERMINISTIC if det else 0
    return d


def rows(case_list):
    L = _capi.lib()
    for case in case_list:
        for (dn, dt), bwd, (pn, path), det, layout in itertools.product(DTYPES, (0, 1), PATHS, (0, 1), (0, 1)):
            d = descriptor(case, dt, path, det, layout)
            p = ctypes.byref(d)
            yield "%s %s %s %s det%d cl%d: %d %d %d" % (
                case["name"], dn, "bwd" if bwd else "fwd", pn, det, layout, L.mdconv_workspace_bytes(p, bwd),
                L.mdconv_deterministic_supported(p, bwd), L.mdconv_input_layout_supported(p, LAYOUT_CHANNELS_LAST, bwd))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases-only", action="store_true", help="tests/cases.py CASES only")
    ap.add_argument("--seeds", type=int, default=300, help="seeds per generator")
    ap.add_argument("-o", "--output", help="write the table here instead of stdout")
    a = ap.parse_args()
    out = open(a.output, "w") if a.output else sys.stdout
    for line in rows(shapes(a.cases_only, a.seeds)):
        out.write(line + "\n")
    if a.output:
        out.close()


if __name__ == "__main__":
    main()
