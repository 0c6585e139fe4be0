"""The shared list builder, scan, sort and gather of the channels-last sampling operators past one unit of work, and the top
MiB below 2^31 bytes (the cases are tests/samp_cases.py's; tests/test_samp_cases_cpu.py asserts their structure without a GPU):

  * segments of 2048, 2049 and more than 4096 rows -- one, two and three chunks of ``csr_scan_chunk`` (kScanChunk = 2048), the
    ``pre`` loop and its second iteration --, more than one segment (a 64-row sort chunk straddles two), many workgroups with a
    partly filled last one; one depthwise case, whose family builds its lists with the same ``scatter_lists_build``; the
    aggregation's segment is an image of cams * S_cam rows, with camera boundaries inside a chunk (its own list kernel and gather);
  * lists of exactly 2048, 2049 and 2100 entries: the second pass over the key blocks of ``sort_row_block`` (kKeyBlock = 2048),
    its last partial block and the padding keys;
  * 65535 segments, the scan's ``grid.y`` at the limit the shape rules allow;
  * a sampled tensor that ends 1 MiB below 2^31 bytes, where a sign or carry mistake in a 32-bit byte offset would show.

Every case is compared against the fp64 reference in plain and in deterministic mode, and the deterministic mode is
bit-identical over two runs.  Tolerances are the project's: 1e-4 for fp32, ``TOL`` of tests/test_gpu_hp.py for 16-bit.  The
2049-row cases of DCNv3 and the RoI pooling need a 3 x 683 image, where fp32 resolves a position to 6e-5 px only: their
coordinates lie on a binary grid on which fp32 forms every position exactly (tests/samp_cases.py states the rule), and
``test_wide_image_misses_are_the_fp32_positions`` pins what free offsets cost there."""
import pytest
import torch

from tests import samp_cases as SC
from tests.cases import M2, _c, make_inputs
from tests.util import assert_close, run_oracle, run_product

pytestmark = pytest.mark.gpu

DEV = SC.DEV
F32 = SC.F32


def _plain_and_deterministic(table, name, dtype, coord_dtype):
    op = SC.OPS[table[name]["op"]]
    t, geo = SC.fixed_case(name, dtype, coord_dtype)
    want = SC.fixed_reference(name, dtype, coord_dtype)
    tol = SC.tols(op, t)
    tag = "scale %s %s" % (SC.pairing_id(dtype, coord_dtype), name)
    dt = SC.dev(t)
    SC.compare(op, tag, op.native(dt, geo), want, tol)
    first = op.native(dt, geo, deterministic=True)
    second = op.native(dt, geo, deterministic=True)
    for what, a, b in zip(op.names, first, second):
        assert (a is None and b is None) or torch.equal(a, b), "%s: deterministic %s differs between two runs" % (tag, what)
    SC.compare(op, tag + " deterministic", first, want, tol)
    return op, t, geo, first


@pytest.mark.parametrize("name, dtype, coord_dtype", SC.fixed_params(SC.SCAN_CASES), ids=SC.fixed_ids(SC.SCAN_CASES))
def test_several_scan_chunks(name, dtype, coord_dtype):
    _plain_and_deterministic(SC.SCAN_CASES, name, dtype, coord_dtype)


def test_wide_image_misses_are_the_fp32_positions():
    """The 3 x 683 image with FREE fp32 offsets (the 2049-row cases keep theirs on a binary grid, tests/samp_cases.py): against
    the fp64 reference evaluated at the positions fp32 arithmetic forms -- the kernel's one rounding applied to the reference
    -- every result holds the project's 1e-4 on both criteria; against the all-fp64 reference the scaled maximum holds 1e-4
    and the per-element error stays within 2.5e-4, the reference's own movement under that rounding (2.15e-4, measured in
    tests/test_samp_cases_cpu.py) with a margin, which pins the size of the deviation."""
    op = SC.Dcnv3
    t, geo, want, rounded = SC.wide_free_case()
    got = op.native(SC.dev(t), geo)
    SC.compare(op, "wide f32-same dcnv3 fp32-positions", got, rounded, SC.tols(op, t))
    for what, a, b in zip(op.names, got, want):
        assert_close("widefree f32-same dcnv3 %s" % what, a, b, 1e-4, elem_tol=SC.WIDE_FREE_ELEM_TOL)


def test_depthwise_lists_over_several_scan_chunks():
    """50 x 45 = 2250 input pixels per segment: two scan chunks through the depthwise family's ``scatter_lists_build``."""
    from modulated_deform_conv_amd import _capi
    case = _c("dw_mdcn2d_c8_50x45", M2, 2, 8, 8, (50, 45), 3, groups=8, seed=311)
    assert 50 * 45 > SC.K_SCAN_CHUNK
    t = make_inputs(case, dtype=F32, device="cuda")
    want_out, want = run_oracle(case, t, F32)
    for det in (False, True):
        with _capi.deterministic(det):
            out, grads, paths = run_product(case, t, "depthwise")
        assert _capi.last_kernels() == "depthwise" and paths == ["depthwise", "depthwise"]
        assert_close("scale f32-same depthwise output", out, want_out, 1e-4)
        for k, v in grads.items():
            if v is not None and want[k] is not None:
                assert_close("scale f32-same depthwise %s" % k, v, want[k], 1e-4)


@pytest.mark.parametrize("name, dtype, coord_dtype", SC.fixed_params(SC.LIST_CASES), ids=SC.fixed_ids(SC.LIST_CASES))
def test_long_lists(name, dtype, coord_dtype):
    """A lost or doubled entry among 2100 random terms moves grad_value by about 2 % of its rms, far above 1e-4."""
    _plain_and_deterministic(SC.LIST_CASES, name, dtype, coord_dtype)


@pytest.mark.parametrize("name, dtype, coord_dtype", SC.fixed_params(SC.SEGMENT_CASES), ids=SC.fixed_ids(SC.SEGMENT_CASES))
def test_the_segment_limit(name, dtype, coord_dtype):
    _plain_and_deterministic(SC.SEGMENT_CASES, name, dtype, coord_dtype)


# ---- the top MiB below 2^31 bytes ----
def _top_inputs(op_name):
    """The tensors of the top case on the GPU and their host counterparts for TOP_IMAGES.  The sampled tensor and grad_output
    are drawn on the GPU; the coordinates and factors of every image are those of a three-image draw of the generator (so the
    MARGIN rule holds), image n taking draw n % 3 and TOP_IMAGES[k] draw k.  For the attention operators the locations of
    all other images are -3: no query samples them."""
    op = SC.OPS[op_name]
    spec = dict(SC.TOP_CASES[op_name])
    key = "N" if "N" in spec else "B"
    images = spec[key]
    spec[key] = len(SC.TOP_IMAGES)
    small, geo = op.draw(spec, F32, None, 77)
    gen = torch.Generator(device=DEV).manual_seed(78)
    pick = torch.tensor(SC.TOP_IMAGES, device=DEV)
    sampled = torch.randn((images,) + small[0].shape[1:], device=DEV, generator=gen)
    assert sampled.numel() * 4 == SC.top_bytes(op_name)
    if op_name == "droi":
        rois = small[1].clone()
        rois[:, 0] = torch.tensor(SC.TOP_IMAGES, dtype=torch.float32)[small[1][:, 0].long()]
        big = (sampled, rois.to(DEV), small[2].to(DEV), small[3].to(DEV))
        host = (sampled[pick].cpu(),) + tuple(small[1:])
        return op, geo, big, host, images
    idx = torch.arange(images, device=DEV) % len(SC.TOP_IMAGES)
    idx[pick] = torch.arange(len(SC.TOP_IMAGES), device=DEV)
    go = torch.randn((images,) + small[-1].shape[1:], device=DEV, generator=gen)
    big = (sampled,) + tuple(v.to(DEV)[idx] for v in small[1:-1]) + (go,)
    if "shapes" in spec:
        coords, _ = op.unpack(big, geo)
        coords = coords.clone()
        others = torch.ones(images, dtype=torch.bool, device=DEV)
        others[pick] = False
        coords[others] = -3.0
        big = op.repack(big, geo, coords)
    host = (sampled[pick].cpu(),) + tuple(small[1:-1]) + (go[pick].cpu(),)
    return op, geo, big, host, images


def _check_top(op, tag, got, want, images, zero_elsewhere):
    pick = torch.tensor(SC.TOP_IMAGES, device=DEV)
    for what, a, b, kind in zip(op.names, got, want, op.kinds):
        if op.name == "droi" and what != "grad_input":
            assert_close("%s %s" % (tag, what), a, b, 1e-4)   # per RoI: the whole tensor
            continue
        assert_close("%s %s" % (tag, what), a[pick], b, 1e-4)
    g = got[1]
    lo, hi = g.flatten(1).aminmax(dim=1)   # (a NaN anywhere in an image makes both NaN)
    assert bool(torch.isfinite(lo).all()) and bool(torch.isfinite(hi).all()), "%s: %s is not finite everywhere" % (tag, op.names[1])
    if zero_elsewhere:
        others = torch.ones(images, dtype=torch.bool, device=DEV)
        others[pick] = False
        assert float(lo[others].abs().max()) == 0.0 and float(hi[others].abs().max()) == 0.0, \
            "%s: %s is not zero on the images nothing samples" % (tag, op.names[1])
        assert float(hi[pick].min()) > 0.0


@pytest.mark.parametrize("op_name", sorted(SC.TOP_CASES))
def test_top_mib_below_2_31_bytes(op_name):
    """Images 0, 1023 and 2046 of 2047 against the fp64 reference of those images alone (the operators are independent per
    image); the gradient of the sampled tensor is finite everywhere and, where only those images are sampled (the attention
    operators, the RoI pooling), exactly zero on every other image.  Full backward, plain and deterministic."""
    op, geo, big, host, images = _top_inputs(op_name)
    try:
        want = op.ref(host, geo)
        zero_elsewhere = "shapes" in SC.TOP_CASES[op_name] or op_name == "droi"
        for det in (False, True):
            got = op.native(big, geo, deterministic=det)
            _check_top(op, "top f32-same %s%s" % (op_name, " deterministic" if det else ""), got, want, images, zero_elsewhere)
            del got
            torch.cuda.empty_cache()
    finally:
        del big
        torch.cuda.empty_cache()
