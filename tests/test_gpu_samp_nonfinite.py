"""NaN, infinite and overflowing coordinates on the seven channels-last sampling operators.  The contract (include/mdconv.h): a
sample contributes iff it passes the gate on every axis, so a NaN or infinite coordinate -- or a finite one that overflows once
scaled by the extent or by ``offset_scale`` -- contributes nothing and has gradient exactly zero.  A fresh layer whose offset
branch diverges produces exactly such inputs.

A fuzz-sized case per operator (tests/samp_cases.py) has a fixed tenth of its coordinate tuples overwritten with NaN, +Inf,
-Inf, +-3e38 (fp32 coordinates) or 65504 (fp16 coordinates), on x alone, on y alone (z alone in 3-D) and on all axes; for the
RoI pooling the overwritten tensor is ``offset``.  The expected value is the operator's own result with every such coordinate
replaced by a finite one far outside the gate: under ``deterministic=True`` bit for bit, for the output and every gradient;
and that result meets the fp64 reference of the replaced inputs at the project's tolerance.  Over NaN-filled buffers in
overwrite mode the coordinate gradients of the overwritten samples are exactly zero, and so are their factor gradients for the
operators whose factor is a stored element; for the two softmax policies the factor gradient of a gated-out tap is the
normaliser's, ``-a * S`` -- what the reference's autograd gives, compared within tolerance and bit for bit against the
replaced run.  Nothing in any result is non-finite.  The factors themselves stay finite here: a non-finite factor on a
gated-out tap is 0 x NaN in the reference as well."""
import functools

import pytest
import torch

from tests import samp_cases as SC

pytestmark = pytest.mark.gpu

PARAMS = [(op_name, d, c, axes) for op_name in sorted(SC.OPS) for d, c in SC.NONFINITE_PAIRINGS
          for axes in SC.nonfinite_axes(op_name)]
IDS = ["%s-%s-%s" % (o, SC.pairing_id(d, c), "".join("xyz"[a] for a in axes)) for o, d, c, axes in PARAMS]


def _run(op, t, geo):
    dt = SC.dev(t)
    return op.native(dt, geo, grads=SC.nan_buffers(op, dt), accumulate=False, deterministic=True)


@functools.lru_cache(maxsize=None)
def _replaced_run(op_name, dtype, coord_dtype, axes):
    t, geo, _ = SC.replaced_case(op_name, dtype, coord_dtype, axes)
    return tuple(None if g is None else g.cpu() for g in _run(SC.OPS[op_name], t, geo))


@pytest.mark.parametrize("op_name, dtype, coord_dtype, axes", PARAMS, ids=IDS)
def test_nonfinite_coordinates_are_gated_out(op_name, dtype, coord_dtype, axes):
    op = SC.OPS[op_name]
    t2, geo, want = SC.replaced_case(op_name, dtype, coord_dtype, axes)
    tag = "nonfinite %s %s %s" % (SC.pairing_id(dtype, coord_dtype), op_name, "".join("xyz"[a] for a in axes))
    base = _replaced_run(op_name, dtype, coord_dtype, axes)
    SC.compare(op, tag, base, want, SC.tols(op, t2))
    sel = SC.overwritten(op_name, dtype, coord_dtype)
    for value in SC.NONFINITE_VALUES[coord_dtype or dtype]:
        t3, _ = SC.overwrite(op_name, dtype, coord_dtype, axes, value)
        got = tuple(None if g is None else g.cpu() for g in _run(op, t3, geo))
        for what, a, b in zip(op.names, got, base):
            if b is None:
                assert a is None, what
                continue
            assert bool(torch.isfinite(a.float()).all()), "%s, %r: %s has non-finite values" % (tag, value, what)
            assert torch.equal(a, b), "%s, %r: %s differs from the run with the coordinate far outside (%d elements)" % (
                tag, value, what, int((a != b).sum()))
        gcoord, gfactor = op.unpack_grads(got, t3, geo)
        assert float(gcoord[sel].float().abs().max()) == 0.0, "%s, %r: coordinate gradient of a gated-out sample" % (tag, value)
        if op.plain_factor and gfactor is not None:
            assert float(gfactor[sel].float().abs().max()) == 0.0, "%s, %r: factor gradient of a gated-out sample" % (tag, value)
