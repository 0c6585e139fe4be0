"""Batch-chunked calls whose LAST chunk takes a different plan than the full chunks of the same call.

Both kernel families cut a call into batch chunks when a tensor would pass the 32-bit buffer range (hp_host.hip:
chunk_batch / hp_plan, run by hp_forward / hp_backward; mfma_kernels.hip: make_plan / native_forward / native_backward), and many plan
decisions follow the pixel count of the chunk being launched: the forward row width of the 16-bit kernels (hp_dims: MB),
hp_fwd2 or hp_fwd, hp_bwd3 or hp_bwd2 (use_bwd3), the channels-last fp32 forward and GEMM-2 (fwd_channels_last /
bwd_channels_last), the N % 32 instance and split-K count of GEMM-2 (bwd_dims).  Weights, tables and the workspace layout
are prepared once per call.  The other chunk tests use shapes so small that every chunk picks the same plan; here
MDCONV_CHUNK_LIMIT_BYTES is chosen so that the plan FLIPS on the tail.

Every scenario, in a child process (the switches are read once per process), one child after the other:
  * derives the chunk sizes and the plan of the full chunk and of the tail from the library's rules, mirrored below, with
    the device's CU count, and asserts that they differ -- on another CU count, or after a rule change, the case fails
    instead of testing nothing;
  * where the kernels have different names, proves the flip through the profile hooks: the slot's launch count is the
    chunk count, a call of Bc images names the full chunk's kernel, a call of the tail's size the tail's;
  * runs with the workspace in the middle of a pattern-filled allocation (tests.util.guarded_run: margins AND workspace
    carry the pattern, so a table row nobody wrote reads as garbage) and checks both margins;
  * compares the output and all five gradients with the CPU oracle in fp32: 1e-4 (fp32), 5e-3 (fp16), 3e-2 (bf16), the
    tolerances of the other chunk tests.  The output buffer starts as NaN, so a block that is skipped cannot pass by
    holding an earlier call's values.
Modes: "zeros" accumulates into zeroed gradient buffers; "prefill" accumulates into buffers that hold +s / -s/2 in turn
(s = the oracle gradient's rms, so that the sum's 16-bit rounding stays in proportion) and must give prefill + gradient;
"nan" runs in overwrite mode into NaN-filled buffers and must write every element.

Regressions covered: fwd_mb and fwd_k2 for a tail that took narrower forward rows than the row table was filled for
(hp_plan now takes the row width once per call; the numbers, the NaN-filled output and the pattern-filled table are
the evidence -- both chunk sizes run the same kernel, so there is no proof by name); f32_bwd_cl and f32_padn_3+2 for a
tail whose fp32 backward workspace is larger than a full chunk's (make_plan now sizes it for the larger need).

Scenarios that share a chunk limit and environment run in ONE child (the switches are per process, and the interpreter
start would otherwise dominate the module's time), so a fault in a group's first scenario hides the group's others;
orderly failures do not: the child runs every scenario and reports each failed check."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20


# ------------------------------------------------------------------ the library's planning rules, mirrored
def _ceil(x, m):
    return -(-x // m) * m


def _pow2_ceil(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def _prod(v):
    p = 1
    for x in v:
        p *= x
    return p


def _chunks(B, bc):
    return [min(bc, B - b0) for b0 in range(0, B, bc)]


def _geo(case):
    """(nd, K, S_i, S_o) of a stride-1 case whose padding keeps the size (k = 3, padding 1)."""
    nd = len(case["in_sz"])
    assert case["k"] == 3 and case["stride"] == 1 and case["padding"] == 1 and case["dilation"] == 1
    return nd, 3 ** nd, _prod(case["in_sz"]), _prod(case["in_sz"])


def hp_width(case):
    """Channels the 16-bit BACKWARD runs on: one deformable group of 96 / 160 / 192 / 224 padded channels is widened to
    128 / 256 where the full chunk takes hp_bwd3 (hp_host.hip: width_padded, a step of hp_plan).  A partial mirror: it does not test that
    the full chunk takes hp_bwd3; a case where it does not fails the kernel-name check of slot 1."""
    Cp = _ceil(case["C"], 32)
    if case["groups"] == 1 and case["dgroups"] == 1 and 64 < Cp < 256 and _pow2_ceil(Cp) != Cp:
        return _pow2_ceil(Cp)
    return case["C"]


def hp_chunk_batch(case, C, limit, backward):
    """hp_host.hip: chunk_batch -- the channels-last input copy (or the output rows) of a chunk, and one image's grad_col
    rows, stay below the limit."""
    nd, K, S_i, S_o = _geo(case)
    Cp, Op = _ceil(C, 32), _ceil(case["O"], 32)
    per = max(S_i * Cp * 2, S_o * (Op if backward else case["O"]) * 2)
    assert per < limit and (not backward or K * S_o * Cp * 2 < limit), "the limit refuses the native 16-bit kernels"
    return min(case["B"], limit // per)


def hp_fwd_plan(case, images, cus):
    """hp_host.hip: hp_dims (MB, oranges) and hp_plan's forward kernel choice (hp_fwd2 unless a 64-channel stage would straddle deformable groups
    or, with deformable groups, a second workgroup row exists), one conv group."""
    nd, K, S_i, S_o = _geo(case)
    oblks = _ceil(case["O"], 32) // 32
    MB = 4 if oblks >= 3 else oblks
    tiles = -(-images * S_o // 128)
    if tiles * (-(-oblks // MB)) * 2 < cus:
        MB = 1
    oranges = -(-oblks // MB)
    DG = case["dgroups"]
    fwd2 = DG == 1 or ((case["C"] // DG) % 64 == 0 and oranges == 1)
    return dict(tiles=tiles, MB=MB, rows=oranges, kernel="hp_fwd2_kernel" if fwd2 else "hp_fwd_kernel")


def hp_bwd_plan(case, C, images, cus):
    """hp_host.hip: use_bwd3, asked by hp_plan for each chunk size -- the pixel-stationary hp_bwd3 beyond one 128-pixel tile per CU (earlier for the instances of
    hp_bwd2 that spill), the tap-stationary hp_bwd2 below; one conv group.  A partial mirror: the library's further
    conditions (hp_bwd3_supported, the LDS and deformable-group limits of hp_bwd2) are left to the kernel-name and
    launch-count checks, which fail where they bite."""
    nd, K, S_i, S_o = _geo(case)
    Cp = _ceil(C, 32)
    MB2 = _pow2_ceil(_ceil(case["O"], 32) // 32)
    nks, waves = 2 * MB2, _pow2_ceil(Cp // 32)
    spills = nks >= 16 or (waves >= 8 and nks >= 8)
    limit = cus * (36 if nd == 3 else 16) // Cp if spills else cus
    tiles = -(-images * S_o // 128)
    return dict(tiles=tiles, kernel="hp_bwd3_kernel" if tiles > limit else "hp_bwd2_kernel")


def f32_bwd_cl(case, images):
    """mfma_fwd_cl.hip: bwd_channels_last."""
    nd, K, S_i, S_o = _geo(case)
    C, DG = case["C"], case["dgroups"]
    if C % 64 or (DG != 1 and (C // DG) % 64):
        return False
    return nd == 3 or case["groups"] >= 8 or images * S_o >= 8192


def f32_fwd_cl(case, images):
    """mfma_fwd_cl.hip: fwd_channels_last."""
    nd, K, S_i, S_o = _geo(case)
    if case["dgroups"] != 1 or (case["C"] // case["groups"]) % 64:
        return False
    return nd == 3 or (images * S_o >= 16384 and case["C"] <= 128 and case["O"] <= 128)


def f32_chunk_batch(case, limit, backward):
    """mfma_kernels.hip: make_plan -- every per-chunk tensor and workspace buffer addressed with 32-bit offsets (fp32
    elements, also for 16-bit tensors, which run through fp32 copies)."""
    nd, K, S_i, S_o = _geo(case)
    C, O, DG = case["C"], case["O"], case["dgroups"]
    per = max(C * S_i * 4, O * S_o * 4)
    if backward:
        rm = (64 if O <= 64 else (128 if O <= 128 else 256)) if f32_bwd_cl(case, 1) else 256
        per = max(per, C * K * S_o * 4, S_o * _ceil(O, rm) * 4, DG * K * S_o * 2 * (1 << nd) * 4, DG * K * S_o * 32)
    assert per < limit
    return min(case["B"], limit // per)


def f32_fwd_plan(case, images):
    return dict(kernel="mfma_fwd_cl_kernel" if f32_fwd_cl(case, images) else "mfma_fwd_kernel")


def f32_bwd_plan(case, images):
    """GEMM-2 of the fp32 backward: layout, and the N % 32 instance whose occupancy sets the split-K count (bwd_dims)."""
    nd, K, S_i, S_o = _geo(case)
    cl = f32_bwd_cl(case, images)
    return dict(kernel="mfma_bwd_weight_cl_kernel" if cl else "mfma_bwd_weight_kernel", padn=(images * S_o) % 32 != 0)


# ------------------------------------------------------------------ scenarios
def _scenarios():
    from tests.cases import D2, D3, M2, M3, _c
    s = {}

    def add(group, name, case, dtype, limit, kind, path="auto", samp32=False, mode="zeros", env=None):
        s.setdefault(group, dict(limit=limit, env=env or {}, scen=[]))
        assert s[group]["limit"] == limit and s[group]["env"] == (env or {})
        s[group]["scen"].append(dict(name=name, case=case, dtype=dtype, kind=kind, path=path, samp32=samp32, mode=mode))

    # A: 5 + 5 + 1 images of 64 x 64: 160 tiles x 1 row of 4 blocks -> 32 tiles, which hp_dims alone gives 4 single-block rows
    a = _c("chunk_a_mdcn2d_c64_dg2_o128", M2, 11, 64, 128, (64, 64), 3, dgroups=2, seed=301)
    add("fwd_mb", "A_fp16", a, "float16", 5 * MiB + MiB // 2, "hp_fwd")
    add("fwd_mb", "A_fp16_s32", a, "float16", 5 * MiB + MiB // 2, "hp_fwd", samp32=True)
    # B: groups of 64 channels run hp_fwd2 on one row; hp_dims alone gives a 1-image tail 4 rows, and those mean hp_fwd.
    # The limit must exceed one image's grad_col rows (9 * 4096 * 128 * 2 = 9 437 184 B): 10 + 1 images
    b = _c("chunk_b_mdcn2d_c128_dg2_o128", M2, 11, 128, 128, (64, 64), 3, dgroups=2, seed=302)
    add("fwd_k2", "B_fp16", b, "float16", 10 * MiB, "hp_fwd")
    # C: 9 + 9 + 2 images (the limit exceeds one image's grad_col rows, 9 * 4096 * 64 * 2 = 4 718 592 B): 288 -> 64 tiles
    c = _c("chunk_c_mdcn2d_c64_o64", M2, 20, 64, 64, (64, 64), 3, seed=303)
    add("bwd3_2d", "C_fp16", c, "float16", 4980736, "hp_bwd")
    add("bwd3_2d", "C_bf16", c, "bfloat16", 4980736, "hp_bwd")
    add("bwd3_2d", "C_fp16_s32", c, "float16", 4980736, "hp_bwd", samp32=True)
    add("bwd3_2d", "C_fp16_prefill", c, "float16", 4980736, "hp_bwd", mode="prefill")
    add("bwd3_2d", "C_fp16_nan", c, "float16", 4980736, "hp_bwd", mode="nan")
    # D: 96 channels run width-padded to 128 because the full chunk (9 images, 288 tiles) takes hp_bwd3; the 2-image tail
    # runs hp_bwd2 on the padded width.  One image's padded grad_col rows: 9 * 4096 * 128 * 2 = 9 437 184 B
    d = _c("chunk_d_dcn2d_c96_o96", D2, 11, 96, 96, (64, 64), 3, seed=304)
    add("bwd3_pad", "D_fp16", d, "float16", 9 * MiB + MiB // 2, "hp_bwd")
    # E: 3-D, 28 + 2 images of 8 x 16 x 16 (131 072 B each): 448 -> 32 tiles
    e = _c("chunk_e_mdcn3d_c32_o32", M3, 30, 32, 32, (8, 16, 16), 3, seed=305)
    add("bwd3_3d", "E_fp16", e, "float16", 28 * 131072, "hp_bwd")
    # F: fp32 forward, 16 + 4 images of 32 x 32: 16 384 pixels run channels-last, 4096 do not
    f = _c("chunk_f_mdcn2d_c64_o64", M2, 20, 64, 64, (32, 32), 3, seed=306)
    add("f32_fwd_cl", "F_fp32", f, "float32", 4 * MiB, "f32_fwd", path="mfma")
    # fp32 backward, 8 + 5 images of 32 x 32: 8192 pixels run GEMM-2 channels-last on 64-row tiles, 5120 pixels on 256-row
    # tiles whose split-K partials are larger than everything the full chunk needs (mfma_kernels.hip, make_plan).  Before
    # the workspace was sized for the larger chunk need this case would have written megabytes past its workspace, so it
    # was never run against that code.
    i = _c("chunk_i_mdcn2d_c64_o64", M2, 13, 64, 64, (32, 32), 3, seed=307)
    add("f32_bwd_cl", "I_fp32", i, "float32", 19 * MiB, "f32_bwd", path="mfma")
    # G: 256 -> 256 channels with bias, images of 144 / 48 pixels (per image 256 * K * S_o * 4 = 1 327 104 B of grad_col in
    # 2-D and 3-D alike): 3 + 2 images = N % 32 != 0 then == 0, 4 + 3 images the other way round
    g2 = _c("chunk_g_dcn2d_c256_o256", D2, 5, 256, 256, (12, 12), 3, seed=308)
    g3 = _c("chunk_g_dcn3d_c256_o256", D3, 5, 256, 256, (3, 4, 4), 3, seed=309)
    dbg = {"MDCONV_DEBUG_PLAN": "1"}
    for lim_images, B, tag in ((3, 5, "3+2"), (4, 7, "4+3")):
        grp = "f32_padn_" + tag
        add(grp, "G_dcn2d_" + tag, dict(g2, B=B), "float32", lim_images * 1327104, "f32_padn", path="mfma", env=dbg)
        add(grp, "G_dcn3d_" + tag, dict(g3, B=B), "float32", lim_images * 1327104, "f32_padn", path="mfma", env=dbg)
    add("f32_padn_3+2", "G_dcn2d_3+2_prefill", dict(g2, B=5), "float32", 3 * 1327104, "f32_padn", path="mfma", mode="prefill", env=dbg)
    add("f32_padn_3+2", "G_dcn2d_3+2_nan", dict(g2, B=5), "float32", 3 * 1327104, "f32_padn", path="mfma", mode="nan", env=dbg)
    # H: 512 input channels: the native 16-bit backward refuses (more than 8 channel blocks) and so does the forward (few
    # tiles, many K stages), so both run the fp32 kernels through fp32 copies, chunk by chunk: forward 18 + 1 images,
    # backward 9 x 2 + 1 (one image's grad_col: 512 * 9 * 42 * 4 = 774 144 B)
    h = _c("chunk_h_mdcn2d_c512_o64", M2, 19, 512, 64, (7, 6), 3, seed=310)
    add("half_io", "H_fp16_prefill", h, "float16", 1600000, "half_io", mode="prefill")
    add("half_io", "H_bf16_s32_nan", h, "bfloat16", 1600000, "half_io", samp32=True, mode="nan")
    add("half_io", "H_bf16", h, "bfloat16", 1600000, "half_io")
    return s


GROUPS = list(_scenarios())
TOL = {"float32": 1e-4, "float16": 5e-3, "bfloat16": 3e-2}


# ------------------------------------------------------------------ the child
def _plans(sc, limit, cus):
    """((forward chunks, backward chunks), {slot: (full chunk's plan, tail's plan)}, what must differ) from the mirrored
    rules.  Slots are the profile slots: 0 forward, 1 the 16-bit backward kernel, 2 GEMM-2 of the fp32 backward."""
    case, kind = sc["case"], sc["kind"]
    B = case["B"]
    if kind in ("hp_fwd", "hp_bwd"):
        Cb = hp_width(case)
        fc = _chunks(B, hp_chunk_batch(case, case["C"], limit, False))
        bc = _chunks(B, hp_chunk_batch(case, Cb, limit, True))
        plans = {0: (hp_fwd_plan(case, fc[0], cus), hp_fwd_plan(case, fc[-1], cus)),
                 1: (hp_bwd_plan(case, Cb, bc[0], cus), hp_bwd_plan(case, Cb, bc[-1], cus))}
        flip = 0 if kind == "hp_fwd" else 1
    else:
        fc = _chunks(B, f32_chunk_batch(case, limit, False))
        bc = _chunks(B, f32_chunk_batch(case, limit, True))
        plans = {0: (f32_fwd_plan(case, fc[0]), f32_fwd_plan(case, fc[-1])),
                 2: (f32_bwd_plan(case, bc[0]), f32_bwd_plan(case, bc[-1]))}
        flip = {"f32_fwd": 0, "f32_bwd": 2, "f32_padn": 2, "half_io": None}[kind]
    return (fc, bc), plans, flip


def _buffers(t, case, want, mode):
    """(out, grads, expected grads) for a mode."""
    import torch
    refs = dict(grad_input=t["input"], grad_weight=t["weight"], grad_offset=t["offset"], grad_mask=t["mask"],
                grad_bias=t["bias"] if case["bias"] else None)
    grads, expect = {}, {}
    for k, ref in refs.items():
        if ref is None:
            grads[k] = expect[k] = None
            continue
        w = want[k].to(torch.float32)
        if mode == "zeros":
            grads[k], expect[k] = torch.zeros_like(ref), w
        elif mode == "nan":
            grads[k], expect[k] = torch.full_like(ref, float("nan")), w
        else:
            s = w.pow(2).mean().sqrt().item()
            pre = torch.full(ref.shape, s, dtype=torch.float32)
            pre.view(-1)[1::2] = -s / 2
            grads[k] = pre.to(ref.dtype).to(ref.device)
            expect[k] = grads[k].float().cpu() + w
    return grads, expect


def _call(sc, t, B, path):
    """One guarded forward + backward of the first B images into fresh buffers; returns (out, grads)."""
    import torch
    from tests.util import run_product_into
    case = dict(sc["case"], B=B)
    tt = {k: (None if v is None else (v if k in ("weight", "bias") else v[:B].contiguous())) for k, v in t.items()}
    out = torch.full_like(tt["grad_output"], float("nan"))
    grads = dict(grad_input=torch.zeros_like(tt["input"]), grad_weight=torch.zeros_like(tt["weight"]),
                 grad_offset=torch.zeros_like(tt["offset"]),
                 grad_mask=None if tt["mask"] is None else torch.zeros_like(tt["mask"]),
                 grad_bias=torch.zeros_like(tt["bias"]) if case["bias"] else None)
    run_product_into(case, tt, out, grads, True, path)
    return out, grads


def _names(slots):
    """{slot: (kernel name of the last launch, launches since the last reset)}"""
    import ctypes
    from modulated_deform_conv_amd import _capi
    L = _capi.lib()
    return {w: (L.mdconv_profile_name(w).decode(), L.mdconv_profile_read(w, ctypes.byref(ctypes.c_double(0)))) for w in slots}


def _scenario(sc, limit, cus, oracle_cache):
    import torch
    from modulated_deform_conv_amd import MDCONV_CUDA as M
    from modulated_deform_conv_amd import _capi
    from tests.cases import make_inputs
    from tests.util import assert_close, guarded_run, run_oracle, run_product_into
    errors = []

    def check(ok, msg):
        print("    %s %s" % ("ok  " if ok else "FAIL", msg), flush=True)
        if not ok:
            errors.append(msg)

    case, dtype, path, mode = sc["case"], getattr(torch, sc["dtype"]), sc["path"], sc["mode"]
    (fc, bc), plans, flip = _plans(sc, limit, cus)
    print("  %s: %d CUs, forward chunks %s, backward chunks %s, plans %s" % (sc["name"], cus, fc, bc, plans), flush=True)
    # ---- the precondition: the rules give the tail another plan than the full chunk
    if flip is None:
        check(len(fc) > 1 and fc[-1] < fc[0] and len(bc) > 2 and bc[-1] < bc[0], "uneven chunks, forward and backward")
    else:
        chunks = fc if flip == 0 else bc
        check(len(chunks) > 1 and chunks[-1] < chunks[0], "a shorter last chunk")
        check(plans[flip][0] != plans[flip][1], "slot %d: the tail's plan %s differs from the full chunk's %s"
              % (flip, plans[flip][1], plans[flip][0]))
    if errors:
        return errors

    key = (case["name"], case["B"], sc["dtype"], sc["samp32"])
    t = make_inputs(case, dtype=torch.float64, device="cuda")
    t = {k: (None if v is None else v.to(torch.float32 if sc["samp32"] and k in ("offset", "mask") else dtype))
         for k, v in t.items()}
    if key not in oracle_cache:
        oracle_cache[key] = run_oracle(case, {k: (None if v is None else v.float().contiguous()) for k, v in t.items()},
                                       torch.float32)
    want_out, want = oracle_cache[key]

    touched, calls = [], []
    M._run = guarded_run(touched, calls)
    _capi.profile_enable(True)
    _capi.profile_reset()
    out = torch.full_like(t["grad_output"], float("nan"))
    grads, expect = _buffers(t, case, want, mode)
    run_product_into(case, t, out, grads, mode != "nan", path)
    torch.cuda.synchronize()
    fam = _capi.last_kernels()
    check(fam == ("f32" if sc["kind"].startswith(("f32", "half")) else "hp"), "kernel family %s" % fam)
    check(all(ws > 0 for _, ws in calls) and len(calls) == 2, "two calls with a workspace: %s" % calls)
    check(not touched, "both margins of the workspace untouched %s" % touched)
    slots = sorted(plans)
    got = _names(slots)
    # ---- the flip, through the profile hooks
    check(got[0][1] == len(fc), "forward launches %d = chunks %d" % (got[0][1], len(fc)))
    check(got[slots[1]][1] == len(bc), "backward launches %d = chunks %d" % (got[slots[1]][1], len(bc)))
    for slot in slots:
        full, tail = plans[slot]
        chunks = fc if slot == 0 else bc
        # the forward row width of the 16-bit kernels is taken once per call: every chunk runs the full chunk's kernel
        per_call = sc["kind"].startswith("hp") and slot == 0
        check(got[slot][0] == (full if per_call else tail)["kernel"], "slot %d after the chunked call: %s" % (slot, got[slot][0]))
        if full["kernel"] != tail["kernel"]:
            for images, plan in ((chunks[0], full), (chunks[-1], tail)):
                _capi.profile_reset()
                _call(sc, t, images, path)
                torch.cuda.synchronize()
                n = _names([slot])[slot]
                check(n == (plan["kernel"], 1), "slot %d after a call of %d images: %s" % (slot, images, n))
    check(not touched, "both margins untouched in the single-chunk calls %s" % touched)
    _capi.profile_enable(False)

    tol = TOL[sc["dtype"]]
    for name, g, w in [("output", out, want_out)] + [(k, grads[k], expect[k]) for k in grads]:
        if w is None:
            continue
        try:
            assert_close(name, g.float(), w, tol)
            check(True, name)
        except AssertionError as e:
            check(False, "%s" % e)
    return errors


def child(group):
    import torch
    g = _scenarios()[group]
    assert int(os.environ["MDCONV_CHUNK_LIMIT_BYTES"]) == g["limit"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    failed, cache = {}, {}
    for sc in g["scen"]:
        errors = _scenario(sc, g["limit"], cus, cache)
        if errors:
            failed[sc["name"]] = errors
    for name, errors in failed.items():
        print("FAILED %s: %s" % (name, "; ".join(errors)))
    if failed:
        sys.exit(1)
    print("CHUNK_PLANS_OK %s (%d scenarios)" % (group, len(g["scen"])))


@pytest.mark.parametrize("group", GROUPS)
def test_last_chunk_with_another_plan(group):
    g = _scenarios()[group]
    env = dict(os.environ, MDCONV_CHUNK_LIMIT_BYTES=str(g["limit"]), **g["env"])
    code = "import sys; sys.path.insert(0, %r); from tests.test_gpu_chunk_plans import child; child(%r)" % (ROOT, group)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=420)
    plan_lines = sorted({ln for ln in r.stderr.splitlines() if "GEMM-2 plan" in ln})
    report = r.stdout[-6000:] + "\n".join(plan_lines[:40]) + "\n" + "\n".join(
        ln for ln in r.stderr.splitlines() if "GEMM-2 plan" not in ln and "forward plan" not in ln)[-3000:]
    print(report)
    assert r.returncode == 0, report
    assert "CHUNK_PLANS_OK %s" % group in r.stdout, report
