"""Seeded random shapes for the seven channels-last sampling operators (DCNv4 with and without ``softmax=``: eight entries of
tests/samp_cases.py), 24 seeds each, the dtype pairings rotating over the seeds: output and every gradient against the fp64
reference evaluated from the inputs as the kernel sees them, at the project's tolerances (1e-4 fp32, ``TOL`` of
tests/test_gpu_hp.py for 16-bit; value-typed results by the value dtype, coordinate and factor gradients by the coordinate
dtype).  The draws cover the operators' whole parameter space at extents of at most 24 (tests/samp_cases.py states the
drawing rule; tests/test_samp_cases_cpu.py checks every draw without a GPU).  Every third seed also runs the backward onto
random buffers (buffer + gradient, rounded once) and with ``deterministic=True`` (two runs bit-identical)."""
import functools

import pytest
import torch

from tests import samp_cases as SC
from tests.util import assert_close

pytestmark = pytest.mark.gpu

_DRAWN = {}   # operator -> {seed: structure} of the seeds that ran in this session


@functools.lru_cache(maxsize=None)
def _reference(op_name, seed):
    t, geo, _, _ = SC.fuzz_case(op_name, seed)
    return SC.OPS[op_name].ref(t, geo)


@pytest.mark.parametrize("seed", range(SC.FUZZ_SEEDS))
@pytest.mark.parametrize("op_name", sorted(SC.OPS))
def test_random_shape(op_name, seed):
    op = SC.OPS[op_name]
    t, geo, spec, _ = SC.fuzz_case(op_name, seed)
    dtype, coord_dtype = SC.fuzz_pairing(op_name, seed)
    want = _reference(op_name, seed)
    tol = SC.tols(op, t)
    tag = "fuzz %s %s %d" % (SC.pairing_id(dtype, coord_dtype), op_name, seed)
    print(tag, spec)
    dt = SC.dev(t)
    got = op.native(dt, geo)
    for g, kind in zip(got, op.kinds):
        assert g is None or g.dtype == (dtype if kind == "v" else (coord_dtype or dtype))
    SC.compare(op, tag, got, want, tol)
    _DRAWN.setdefault(op_name, {})[seed] = op.structure(t, geo)
    if seed % 3:
        return
    # accumulate: each buffer + gradient in the buffer's dtype, rounded once
    gen = torch.Generator().manual_seed(seed + 9)
    base = tuple(None if v is None else torch.randn(v.shape, generator=gen).to(v.dtype) for v in op.grad_like(t))
    bufs = SC.dev(base)
    acc = op.native(dt, geo, grads=bufs, accumulate=True)
    for what, a, buf, b, w, e in zip(op.names[1:], acc[1:], bufs, base, want[1:], tol[1:]):
        if b is None:
            assert a is None and w is None, what
            continue
        assert a.data_ptr() == buf.data_ptr(), what
        assert_close("%s accumulate %s" % (tag, what), a, b.double() + w, e)
    # deterministic: bit-identical over two runs, and within tolerance
    first = op.native(dt, geo, deterministic=True)
    second = op.native(dt, geo, deterministic=True)
    for what, a, b in zip(op.names, first, second):
        assert (a is None and b is None) or torch.equal(a, b), "%s: deterministic %s differs between two runs" % (tag, what)
    SC.compare(op, tag + " deterministic", first, want, tol)


def test_fuzz_reaches_the_lane_geometry():
    """From the draws that ran: the seeds of each operator reach three distinct VL, a K below VL and a K that is no multiple
    of VL (the RoI pooling has no tap batches: three VL, both grid rules); the aggregation's also both group reductions of
    its coordinate backward (``seg``), a row of more than one round and five levels or more.  Needs the seeds of this module
    in the same session."""
    if any(len(_DRAWN.get(op_name, {})) < SC.FUZZ_SEEDS for op_name in SC.OPS):
        pytest.skip("needs the %d random cases per operator of this module in the same session" % SC.FUZZ_SEEDS)
    for op_name, drawn in sorted(_DRAWN.items()):
        st = list(drawn.values())
        assert len({s["VL"] for s in st}) >= 3, op_name
        if op_name == "droi":
            assert any(len(s["grids"]) > 1 for s in st), "no seed with RoIs of different adaptive grids"
            continue
        assert any(s["K"] < s["VL"] for s in st), op_name
        assert any(s["K"] % s["VL"] for s in st), op_name
        if op_name == "dagg":
            assert {s["seg"] for s in st} == {0, 1}
            assert any(s["rounds"] > 1 for s in st) and any(s["L"] >= 5 for s in st)
