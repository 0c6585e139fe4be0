"""The fp32 grad_input gather (csrc/mfma_col2im.hip) at the list shapes that can break it: one anchor that owns every
sample, lists that are empty or sit at the ends of an image row whose length is no multiple of the 32-pixel tile, channel
counts that leave a 256-channel block partly filled or start a second one, accumulation onto a prefilled grad_input,
deterministic mode, and the grouped kernel.

All cases are fp32 2-D modulated.  Each runs the default kernel selection -- asserted to be the matrix-core family -- against
the shape-generic kernels and the CPU oracle at 1e-4 (the tolerance of tests/test_gpu_extremes.py).

List lengths of the hot anchor: 15 x 15 output pixels x 9 taps = 2025 samples at (7.5, 7.5), i.e. two lists (rows 7 and 8
of column 7) of 2025 entries = 126 steps of 16 entries + 8 + 1: the full step and the exact steps behind it.  C = 64 runs the
narrow kernel (16 entries per fetch); C = 256 puts the same lists through col2im_gather_kernel.
"""
import pytest
import torch

from tests.cases import M2, _c, make_inputs, out_size
from tests.util import assert_close, run_oracle, run_product, run_product_into

pytestmark = pytest.mark.gpu

TOL = 1e-4
KEYS = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")
FAR = -100.0   # a coordinate far outside every image of this file


def _tap_base(case, axis):
    """o * stride - pad + tap * dilation along `axis` (0 = rows, 1 = columns) as a [9, Ho, Wo] tensor (3 x 3, stride 1,
    pad 1, dilation 1: every case of this file)"""
    Ho, Wo = out_size(case)
    o = (torch.arange(Ho, dtype=torch.float32).view(1, Ho, 1) if axis == 0 else
         torch.arange(Wo, dtype=torch.float32).view(1, 1, Wo)).expand(9, Ho, Wo)
    tap = torch.arange(9).view(9, 1, 1)
    return o - 1 + (tap // 3 if axis == 0 else tap % 3).float()


def _place(case, t, axis, pos):
    """Overwrite the offsets along `axis` so that sample (b, tap, pixel) lies at coordinate pos[b, tap, h, w] (one
    deformable group); dyadic positions keep `base + offset` exact in fp32."""
    off = t["offset"].clone()
    off[:, axis::2] = pos - _tap_base(case, axis)
    t["offset"] = off.contiguous()


def _hot_case(C):
    case = _c("gl_hot_anchor_c%d" % C, M2, 1, C, C, (15, 15), 3, seed=301)
    t = make_inputs(case)
    for axis in (0, 1):
        _place(case, t, axis, torch.full((1, 9, 15, 15), 7.5))
    return case, t


def _row_ends_case():
    """5 x 33 image (S_i = 165 = 5 tiles of 32 + 5): half the samples far outside, the others on column 0 alone (x = -0.5) or
    column 32 alone (x = 32.5); rows stay where make_inputs put them.  Every anchor of columns 1..30 has an empty list."""
    case = _c("gl_row_ends_5x33", M2, 2, 256, 64, (5, 33), 3, seed=302)
    t = make_inputs(case)
    gen = torch.Generator().manual_seed(3020)
    kind = torch.randint(0, 4, (2, 9, 5, 33), generator=gen)
    pos = torch.where(kind < 2, torch.tensor(FAR), torch.where(kind == 2, torch.tensor(-0.5), torch.tensor(32.5)))
    _place(case, t, 1, pos)
    return case, t


def _plain_case(name, C, O=64, dgroups=1, seed=303):
    case = _c(name, M2, 2, C, O, (8, 8), 3, dgroups=dgroups, seed=seed)
    return case, make_inputs(case)


_BUILDERS = {
    "hot_anchor_c64": lambda: _hot_case(64),
    "hot_anchor_c256": lambda: _hot_case(256),
    "row_ends_5x33": _row_ends_case,
    "channels_72": lambda: _plain_case("gl_c72", 72),
    "channels_320": lambda: _plain_case("gl_c320", 320),
    "grouped_dg2_c64": lambda: _plain_case("gl_dg2_c64", 64, dgroups=2, seed=304),
    "grouped_dg2_c128": lambda: _plain_case("gl_dg2_c128", 128, dgroups=2, seed=305),
}
_cache = {}


def _get(name):
    """(case, device tensors, oracle output, oracle gradients), built once per process and never modified"""
    if name not in _cache:
        case, t = _BUILDERS[name]()
        want_out, want = run_oracle(case, t, torch.float32)
        _cache[name] = (case, {k: (None if v is None else v.cuda()) for k, v in t.items()}, want_out, want)
    return _cache[name]


def _matrix_path_ran(paths=None):
    from modulated_deform_conv_amd import _capi
    assert _capi.last_path() == "mfma" and _capi.last_kernels() == "f32", (_capi.last_path(), _capi.last_kernels())
    if paths is not None:
        assert paths == ["mfma", "mfma"], paths


@pytest.mark.parametrize("name", list(_BUILDERS))
def test_gather_lists(name):
    case, t, want_out, want = _get(name)
    out_a, g_a, paths = run_product(case, t, "auto")
    _matrix_path_ran(paths)
    out_d, g_d, _ = run_product(case, t, "direct")
    assert_close("output", out_a, out_d, TOL)
    assert_close("output/oracle", out_a, want_out, TOL)
    for k in KEYS:
        assert_close(k, g_a[k], g_d[k], TOL)
        assert_close(k + "/oracle", g_a[k], want[k], TOL)


def test_hot_anchor_really_is_one_point():
    """the crafted offsets do what the docstring says: grad_input is non-zero in the 2 x 2 block around (7.5, 7.5) only"""
    _, _, _, want = _get("hot_anchor_c256")
    touched = want["grad_input"][0].abs().amax(dim=0) > 0
    assert touched[7:9, 7:9].all() and int(touched.sum()) == 4, touched.nonzero().tolist()


def _buffers(case, t, fill=None):
    mk = (lambda v: torch.empty_like(v)) if fill is None else (lambda v: fill[id(v)].clone())
    g = dict(grad_input=mk(t["input"]), grad_weight=mk(t["weight"]), grad_offset=mk(t["offset"]), grad_mask=mk(t["mask"]),
             grad_bias=mk(t["bias"]))
    return torch.empty_like(t["grad_output"]), g


@pytest.mark.parametrize("name", ["channels_72", "row_ends_5x33"])
def test_accumulate_mode(name):
    case, t, _, want = _get(name)
    gen = torch.Generator().manual_seed(99)
    fill = {id(t[k]): torch.randn(t[k].shape, generator=gen).cuda() for k in ("input", "weight", "offset", "mask", "bias")}
    out, g = _buffers(case, t, fill)
    run_product_into(case, t, out, g, accumulate=True, path="auto")
    torch.cuda.synchronize()
    _matrix_path_ran()
    for k, src in zip(KEYS, ("input", "offset", "mask", "weight", "bias")):
        assert_close(k, g[k], want[k] + fill[id(t[src])].cpu(), TOL)


@pytest.mark.parametrize("name", ["hot_anchor_c64", "hot_anchor_c256"])
def test_deterministic_mode_is_bit_equal(name):
    from modulated_deform_conv_amd import _capi
    case, t, _, want = _get(name)
    runs = []
    for _ in range(2):
        out, g = _buffers(case, t)
        with _capi.deterministic():
            run_product_into(case, t, out, g, accumulate=False, path="auto")
        torch.cuda.synchronize()
        _matrix_path_ran()
        runs.append(g)
    assert torch.equal(runs[0]["grad_input"], runs[1]["grad_input"])
    assert_close("grad_input/oracle", runs[0]["grad_input"], want["grad_input"], TOL)
