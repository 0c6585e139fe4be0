"""The cases of tests/samp_cases.py are what they claim, from the reference geometry alone (no GPU): the generators' own
conditions (``MARGIN``; ``GRID_MARGIN`` for the RoI pooling), the structural property each case exists for -- rows per
segment, segments, the longest list, pairs, bytes of the sampled tensor, computed from the reference's corner rows --, the
operator's shape rule (the library sizes the backward's workspace: a refused call has none), and the two references against
each other at 1e-10 where the module has two.  The GPU modules draw from the same table, so they cannot run a stale case."""
import ctypes

import pytest
import torch

from tests import droi_ref as RD
from tests import samp_cases as SC
from tests.dcnv3_ref import MARGIN
from tests.util import rel_err

F32, F16 = SC.F32, SC.F16
REDRAWS = {}


@pytest.fixture(scope="module")
def capi():
    from modulated_deform_conv_amd import _build, _capi
    _build.build()
    return _capi


def _meta(t):
    return tuple(None if v is None else torch.empty(v.shape, dtype=v.dtype, device="meta") for v in t)


def _workspace_bytes(capi, op_name, t, geo):
    """Bytes of the full backward's workspace by the library's own plan: 0 for a call outside the shape rule."""
    from modulated_deform_conv_amd import dagg, dcnv3, dcnv4, droi, fda, msda, msda3d
    L = capi.lib()
    if op_name == "dagg":
        d, fn = dagg._desc(t[0], t[1], t[2], geo), L.mdconv_dagg_workspace_bytes
    elif op_name == "dcnv3":
        d, fn = dcnv3._desc(t[0], *geo), L.mdconv_dcnv3_workspace_bytes
    elif op_name.startswith("dcnv4"):
        d, fn = dcnv4._desc(t[0], t[1], *geo), L.mdconv_dcnv4_workspace_bytes
    elif op_name == "msda":
        d, fn = msda._desc(t[0], t[1], geo), L.mdconv_msda_workspace_bytes
    elif op_name == "msda3d":
        d, fn = msda3d._desc(t[0], t[1], geo), L.mdconv_msda3d_workspace_bytes
    elif op_name == "fda":
        d, fn = fda._desc(t[0], t[1], geo[0], geo[1]), L.mdconv_fda_workspace_bytes
    else:
        d, fn = droi._desc(t[0], t[1], t[2], **geo), L.mdconv_droi_workspace_bytes
    return int(fn(ctypes.byref(d), 1))


def _conditions(op, t, geo):
    """The generator's own conditions, measured again on the tensors the GPU test will use."""
    assert op.min_lattice_distance(t, geo) >= MARGIN
    if op.name == "droi" and geo["sampling_ratio"] == 0:
        PH, PW = geo["output_size"]
        assert RD.min_grid_distance(t[1], t[0].shape[0], PH, PW, geo["spatial_scale"], geo["max_grid"]) >= RD.GRID_MARGIN


def _references_agree(tag, op, t, geo, want=None):
    if op.direct is None:
        return
    want = op.ref(t, geo) if want is None else want
    other = op.direct(t, geo)
    for what, a, b in zip(op.names, want, other):
        if a is None:
            assert b is None, what
            continue
        err = rel_err(a, b)
        assert err <= 1e-10, (tag, what, err)


def _extents(op_name, spec):
    if "shapes" in spec:
        return max(max(s) for s in spec["shapes"])
    return max(spec["H"], spec["W"])


@pytest.mark.parametrize("seed", range(SC.FUZZ_SEEDS))
@pytest.mark.parametrize("op_name", sorted(SC.OPS))
def test_fuzz_draw(capi, op_name, seed):
    """Every seed has a valid draw (no seed is skipped), inside the drawing rule and the operator's shape rule."""
    op = SC.OPS[op_name]
    t, geo, spec, redraws = SC.fuzz_case(op_name, seed)
    REDRAWS.setdefault(op_name, []).append(redraws)
    dtype, coord_dtype = SC.fuzz_pairing(op_name, seed)
    assert t[0].dtype == dtype
    like = [g for g, k in zip(op.grad_like(t), op.kinds[1:]) if k == "c" and g is not None]
    assert all(g.dtype == (coord_dtype or dtype) for g in like)
    assert _extents(op_name, spec) <= (24 if (coord_dtype or dtype) == F32 else 8)
    _conditions(op, t, geo)
    s = op.structure(t, geo)
    assert s["V"] in op.fuzz_V and s["K"] >= 1 and s["entries"] > 0
    assert s["bytes"] < SC.LIMIT and s["segments"] <= SC.MAX_SEGMENTS
    assert _workspace_bytes(capi, op_name, t, geo) > 0, capi.last_error()
    _references_agree("%s seed %d" % (op_name, seed), op, t, geo)


def test_fuzz_redraws_and_coverage(capi):
    """How many redraws each operator took (printed), and what the 24 seeds of each operator reach: three distinct VL, a K
    below VL and a K that is no multiple of VL (the RoI pooling walks a bin's samples lane by lane, without tap batches: its
    seeds reach three VL, both grid rules, and calls with and without offset).  The aggregation's seeds also reach both
    group reductions of its coordinate backward (``seg``), a row of more than one round, and five levels or more."""
    for op_name in sorted(SC.OPS):
        op = SC.OPS[op_name]
        draws = [SC.fuzz_case(op_name, seed) for seed in range(SC.FUZZ_SEEDS)]
        print("%-14s redraws per seed: %s (total %d)" % (op_name, [d[3] for d in draws], sum(d[3] for d in draws)))
        st = [op.structure(d[0], d[1]) for d in draws]
        assert len({s["VL"] for s in st}) >= 3, op_name
        if op_name == "droi":
            assert {d[2]["sampling_ratio"] == 0 for d in draws} == {True, False}
            assert {d[2]["with_offset"] for d in draws} == {True, False}
            assert any(len(s["grids"]) > 1 for s in st)
        else:
            assert any(s["K"] < s["VL"] for s in st), op_name
            assert any(s["K"] % s["VL"] for s in st), op_name
        if op_name == "dagg":
            assert {s["seg"] for s in st} == {0, 1}
            assert any(s["rounds"] > 1 for s in st) and any(s["L"] >= 5 for s in st)


@pytest.mark.parametrize("name, dtype, coord_dtype", SC.fixed_params(SC.FIXED_CASES), ids=SC.fixed_ids(SC.FIXED_CASES))
def test_fixed_case(capi, name, dtype, coord_dtype):
    """A case of the scan, list and segment tables has the structure it exists for."""
    case = SC.FIXED_CASES[name]
    op = SC.OPS[case["op"]]
    t, geo = SC.fixed_case(name, dtype, coord_dtype)
    _conditions(op, t, geo)
    s = op.structure(t, geo)
    claim = case["claim"]
    print(name, {k: v for k, v in s.items()})
    for key in ("rows", "segments", "longest"):
        if key in claim:
            assert s[key] == claim[key], (key, s[key], claim[key])
    if "chunks" in claim:
        assert -(-s["rows"] // SC.K_SCAN_CHUNK) == claim["chunks"]
        assert s["segments"] > 1 or case["op"] == "droi"   # (the RoI pooling has one segment by construction)
        if claim["chunks"] >= 3:   # the `pre` loop takes its second iteration from lo = 4096 on
            assert s["rows"] > 4096 and s["rows"] % SC.K_SORT_ROWS and s["rows"] % SC.K_SCAN_CHUNK
    if claim.get("chunks", 1) > 1:   # the rows of a segment's last chunk take entries: a wrong `pre` sum moves real lists
        assert s["last_chunk_entries"] > 0
    if claim.get("straddle"):
        assert s["segments"] > 1 and s["rows"] % SC.K_SORT_ROWS
    if claim.get("tail"):
        assert s["pairs"] > s["pairs_per_block"] and s["pairs"] % s["pairs_per_block"]
    if "longest" in claim:
        assert claim["longest"] >= SC.K_KEY_BLOCK
    assert s["entries"] > 0 and s["bytes"] < SC.LIMIT and s["segments"] <= SC.MAX_SEGMENTS
    assert _workspace_bytes(capi, case["op"], t, geo) > 0, capi.last_error()
    if dtype == F32:
        _references_agree(name, op, t, geo, SC.fixed_reference(name, dtype, coord_dtype))


def test_wide_image_rule_is_the_fp32_positions():
    """The input rule of the 2049-row cases (tests/samp_cases.py): on the 3 x 683 image with free fp32 offsets the fp64
    reference ITSELF moves by more than the fp32 tolerance once its positions are formed in fp32 -- 1.1e-4 per element on the
    output, 2.1e-4 on grad_offset, 2.0e-4 on grad_mask, scaled maximum 2e-5 to 4e-5 -- which is what the kernels measured
    against the fp64 reference on such inputs.  On the binary grid of the 2049-row cases fp32 forms every position exactly."""
    from tests import dcnv3_ref as R3
    from tests.util import elem_err
    t, geo, want, rounded = SC.wide_free_case()
    per_element = {}
    for what, a, b in zip(SC.Dcnv3.names, rounded, want):
        per_element[what] = elem_err(a, b)
        print("%-12s scaled %.3e per-element %.3e" % (what, rel_err(a, b), per_element[what]))
        assert rel_err(a, b) <= 1e-4, what
    assert max(per_element.values()) > 1e-4 and per_element["output"] > 1e-4
    assert max(per_element.values()) <= SC.WIDE_FREE_ELEM_TOL
    t, geo = SC.fixed_case("dcnv3_2049")
    args = (t[1], t[0].shape[1], t[0].shape[2]) + tuple(geo[:4]) + (geo[4], geo[6])
    assert all(torch.equal(a, b) for a, b in zip(R3.positions(*args), R3.positions(*args, position_dtype=F32)))


def test_the_tables_cover_what_the_issue_names():
    scan = {SC.FIXED_CASES[n]["op"] for n in SC.SCAN_CASES}
    assert {"dcnv3", "msda", "msda3d", "droi", "dagg"} <= scan
    for op_name in ("dcnv3", "msda", "msda3d", "droi", "dagg"):
        rows = sorted(c["claim"]["rows"] for c in SC.SCAN_CASES.values() if c["op"] == op_name)
        assert rows[0] == 2048 and rows[1] == 2049 and rows[2] > 4096, (op_name, rows)
    assert sorted(c["claim"]["longest"] for c in SC.LIST_CASES.values() if c["op"] == "msda") == [2048, 2049, 2100]
    assert sorted(c["claim"]["longest"] for c in SC.LIST_CASES.values() if c["op"] == "dagg") == [2048, 2049, 2100]
    assert {c["op"] for c in SC.SEGMENT_CASES.values()} == {"dcnv3", "dcnv4", "dcnv4_softmax", "msda", "fda", "msda3d", "dagg"}
    assert set(SC.TOP_CASES) == set(SC.OPS) == set(SC.NONFINITE_CASES)


def test_dagg_batch_limit(capi):
    """One image more than ``dagg_65535``: the full backward has no plan, for the reason dagg_plan states for the lists of
    grad_feature; the backward without grad_feature, which builds no lists, and the forward are inside the shape rule."""
    from modulated_deform_conv_amd import dagg
    t, geo = SC.fixed_case("dagg_65535")
    assert t[0].shape[0] == SC.MAX_SEGMENTS
    more = tuple(torch.empty((SC.MAX_SEGMENTS + 1,) + v.shape[1:], dtype=v.dtype, device="meta") for v in t)
    fn = capi.lib().mdconv_dagg_workspace_bytes
    assert int(fn(ctypes.byref(dagg._desc(more[0], more[1], more[2], geo)), 1)) == 0
    assert "shape rule" in capi.last_error() and "batch exceeds 65535" in capi.last_error()
    skip = dagg._desc(more[0], more[1], more[2], geo, flags=capi.FLAG_NO_GRAD_INPUT)
    assert int(fn(ctypes.byref(skip), 1)) == 0 and "shape rule" not in capi.last_error()   # accepted: a call without workspace
    assert int(fn(ctypes.byref(dagg._desc(more[0], more[1], more[2], geo)), 0)) == 0 and "shape rule" not in capi.last_error()


@pytest.mark.parametrize("op_name", sorted(SC.TOP_CASES))
def test_top_case(capi, op_name):
    """The sampled tensor ends less than 2 MiB below 2^31 bytes, each image stays small, and the shape rule takes the call."""
    spec = SC.TOP_CASES[op_name]
    nbytes = SC.top_bytes(op_name)
    assert SC.LIMIT - (2 << 20) < nbytes < SC.LIMIT
    images = spec.get("N", spec.get("B"))
    assert max(SC.TOP_IMAGES) < images and nbytes // images <= 1 << 20
    # the descriptor of the call, from tensors without storage: a small draw of the same geometry, stretched to the batch
    op = SC.OPS[op_name]
    small = dict(spec)
    small["N" if "N" in spec else "B"] = 3
    t, geo = op.draw(small, F32, None, 0)
    lead = lambda v: None if v is None else torch.empty((images,) + v.shape[1:], dtype=v.dtype, device="meta")
    if op_name == "droi":
        big = (lead(t[0]),) + _meta(t[1:])
    else:
        big = tuple(lead(v) for v in t)
    assert big[0].numel() * 4 == nbytes
    assert _workspace_bytes(capi, op_name, big, geo) > 0, capi.last_error()
    one_more = (torch.empty((images + 1,) + t[0].shape[1:], dtype=F32, device="meta"),) + tuple(big[1:])
    assert _workspace_bytes(capi, op_name, one_more, geo) == 0   # one image more reaches 2^31 bytes: refused


@pytest.mark.parametrize("op_name", sorted(SC.NONFINITE_CASES))
def test_nonfinite_case(op_name):
    """The overwritten tenth is a tenth, in and out of the gate before it is overwritten; the replaced inputs put every such
    sample outside the gate; the non-finite inputs really are non-finite where meant and nowhere else."""
    op = SC.OPS[op_name]
    for dtype, coord_dtype in SC.NONFINITE_PAIRINGS:
        t, geo = SC.nonfinite_case(op_name, dtype, coord_dtype)
        _conditions(op, t, geo)
        sel = SC.overwritten(op_name, dtype, coord_dtype)
        assert 0.08 <= float(sel.double().mean()) <= 0.12 and int(sel.sum()) >= 3
        coords, _ = op.unpack(t, geo)
        assert torch.isfinite(coords.float()).all() and coords.shape[-1] == op.naxes
        for axes in SC.nonfinite_axes(op_name):
            t2, _, want = SC.replaced_case(op_name, dtype, coord_dtype, axes)
            if op.gate is not None:
                gate = op.gate(t, geo)
                assert gate.shape == sel.shape and bool(gate[sel].any())   # samples that DID contribute are overwritten
                assert not bool(op.gate(t2, geo)[sel].any())
                assert torch.equal(op.gate(t2, geo)[~sel], gate[~sel])
            assert all(torch.isfinite(w).all() for w in want if w is not None)
            for value in SC.NONFINITE_VALUES[coord_dtype or dtype]:
                t3, _ = SC.overwrite(op_name, dtype, coord_dtype, axes, value)
                c3, _ = op.unpack(t3, geo)
                for a in range(op.naxes):
                    col = c3[..., a].float()
                    if a in axes:
                        hit = col[sel]
                        assert bool(torch.isnan(hit).all()) if value != value else bool((hit == value).all())
                    else:
                        assert torch.equal(col[sel], coords[..., a].float()[sel])
                    assert torch.equal(col[~sel], coords[..., a].float()[~sel])
                assert torch.equal(t3[0], t[0]) and torch.equal(t3[-1], t[-1])   # values and grad_output are untouched
