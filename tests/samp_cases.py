"""One table of the seven channels-last sampling operators -- DCNv3, DCNv4 (plain and ``softmax=``), multi-scale deformable
attention, packed attention, 3-D attention, deformable RoI pooling and deformable aggregation -- adapted to a common shape,
and the case lists of tests/test_gpu_samp_fuzz.py, tests/test_gpu_samp_scale.py and tests/test_gpu_samp_nonfinite.py.
Importable without a GPU: tests/test_samp_cases_cpu.py checks, from the reference geometry alone, that every case is what it
claims.

An operator entry (``OPS[name]``) holds: ``draw(spec, dtype, coord_dtype, seed)`` -> ``(t, geo)`` -- the CPU tensors of a call,
``grad_output`` last, and the call's static arguments --, ``native(t, geo, ...)`` (the forward and backward entry points,
imported lazily), ``ref(t, geo)`` and, where the reference module has a second statement of the contract, ``direct(t, geo)``
(both: output and every gradient in fp64 from the values the tensors hold), ``gate(t, geo)`` where the module has ``gate_of``,
``kinds`` (per result ``v``: value-typed, ``c``: coordinate-typed), ``structure(t, geo)`` (segments, rows per segment, the
longest list and the entry total from the reference's corner rows, pairs, bytes of the sampled tensor, lane geometry), and
``unpack`` / ``repack`` / ``unpack_grads`` (the coordinate tuples and factors of a call as tensors [..., axes] and [...])."""
import functools
import random

import torch

from tests import dagg_ref as RG
from tests import dcnv3_ref as R3
from tests import dcnv4_ref as R4
from tests import dcnv4_softmax_ref as R4S
from tests import droi_ref as RD
from tests import fda_ref as RF
from tests import msda3d_ref as RA3
from tests import msda_ref as RA
from tests.test_gpu_hp import TOL as _TOL16

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
TOL = dict(_TOL16)
TOL[F32] = 1e-4
PAIRINGS = ((F32, None), (F16, None), (BF16, None), (F16, F32), (BF16, F32))
SAME_TYPE = ((F32, None), (F16, None), (BF16, None))   # DCNv3: the coordinates have the values' type
K_SCAN_CHUNK = 2048   # kScanChunk (mdconv_common.hpp)
K_SORT_ROWS = 64      # kRowsPerChunk (csr_sort.hip)
K_KEY_BLOCK = 2048    # kKeyBlock (csr_sort.hip)
MAX_SEGMENTS = 65535  # the grid.y limit of the scan, the operators' shape rule
LIMIT = 1 << 31       # "every tensor is below 2^31 bytes"
FUZZ_V = (1, 2, 3, 4, 5, 8, 16)   # vectors per head of a random shape: V = 1, odd V, V = 5 in eight lanes, VL = 16


def esize(dtype):
    return 4 if dtype == F32 else 2


def lanes(D, dtype):
    """samp_lanes (samp_core.hpp): vectors per head V, lanes per pair VL, rounds; pairs per workgroup of 256 lanes."""
    V = D * esize(dtype) // 16
    lg = 0
    while (1 << lg) < V and lg < 6:
        lg += 1
    VL = 1 << lg
    return dict(V=V, VL=VL, rounds=-(-V // VL), pairs_per_block=4 * (64 // VL))


def _corner_counts(seg, nseg, rows, start, axes):
    """Entries per list, [nseg * rows] int64, from the reference geometry: a sample at ``axes`` = [(position, size), ...]
    (slowest axis first; fp64 positions and sizes broadcastable to the shape of ``seg``) passes the gate -1 < p < size on
    every axis and then reads each of its 2^n neighbours that lies inside; ``start`` is the first row of the sample's level."""
    gate = torch.ones(seg.shape, dtype=torch.bool)
    for p, size in axes:
        gate = gate & (p > -1) & (p < size)
    lo = [torch.where(gate, p, torch.zeros_like(p)).floor().long() for p, _ in axes]
    counts = torch.zeros(nseg * rows, dtype=torch.int64)
    for corner in range(1 << len(axes)):
        read, lin = gate.clone(), torch.zeros_like(lo[0])
        for a, (_, size) in enumerate(axes):
            i = lo[a] + ((corner >> a) & 1)
            sz = torch.as_tensor(size).long()
            read = read & (i >= 0) & (i < sz)
            lin = lin * sz + i.clamp(min=0)
        row = (seg * rows + start + lin)[read]
        counts += torch.bincount(row, minlength=nseg * rows)
    return counts


def _summary(counts, nseg, rows, pairs, sampled, D, K):
    last_chunk = (rows - 1) // K_SCAN_CHUNK * K_SCAN_CHUNK   # first row of a segment's last scan chunk
    return dict(segments=nseg, rows=rows, longest=int(counts.max()), entries=int(counts.sum()), pairs=pairs,
                last_chunk_entries=int(counts.view(nseg, rows)[:, last_chunk:].sum()),
                bytes=sampled.numel() * sampled.element_size(), K=K, **lanes(D, sampled.dtype))


def _call_kw(grads, deterministic, accumulate):
    kw = dict(grads=grads, deterministic=deterministic)
    if grads is not None:
        kw["accumulate"] = bool(accumulate)
    return kw


class Dcnv3:
    name, kinds, pairings, plain_factor, naxes = "dcnv3", "vvcc", SAME_TYPE, True, 2
    names = ("output", "grad_input", "grad_offset", "grad_mask")
    fuzz_V = FUZZ_V   # the V a random shape of the operator may have (test_fuzz_draw)
    far = -1e4   # px

    @staticmethod
    def draw(spec, dtype, coord_dtype, seed):
        assert coord_dtype in (None, dtype), "DCNv3 has one dtype per call"
        x, off, m, go, geo = R3.make_inputs(dtype=dtype, seed=seed, **spec)
        return (x, off, m, go), geo

    @staticmethod
    def native(t, geo, grads=None, deterministic=False, accumulate=True):
        from modulated_deform_conv_amd import dcnv3
        x, off, m, go = t
        out = dcnv3.dcnv3_forward(x, off, m, *geo)
        g = dcnv3.dcnv3_backward(x, off, m, go, *geo, **_call_kw(grads, deterministic, accumulate))
        torch.cuda.synchronize()
        return (out,) + tuple(g)

    @staticmethod
    def ref(t, geo):
        return R3.dcnv3_ref_grads(*t, *geo)

    @staticmethod
    def direct(t, geo):
        return R3.dcnv3_direct_grads(*t, *geo)

    @staticmethod
    def grad_like(t):
        return t[:3]

    @staticmethod
    def _positions(t, geo):
        return R3.positions(t[1], t[0].shape[1], t[0].shape[2], *geo[:4], geo[4], geo[6])

    @classmethod
    def gate(cls, t, geo):
        return R3.gate_of(t[1], t[0].shape[1], t[0].shape[2], *geo[:4], geo[4], geo[6]).flatten(3)

    @classmethod
    def min_lattice_distance(cls, t, geo):
        d = torch.stack(cls._positions(t, geo))
        return float((d - d.round()).abs().min())

    @classmethod
    def structure(cls, t, geo):
        B, H, W, _ = t[0].shape
        G, D = geo[4], geo[5]
        loc_h, loc_w = cls._positions(t, geo)   # [B, Ho, Wo, G, K]
        K = loc_h.shape[-1]
        seg = (torch.arange(B).view(B, 1, 1, 1, 1) * G + torch.arange(G).view(1, 1, 1, G, 1)).expand(loc_h.shape)
        counts = _corner_counts(seg, B * G, H * W, 0, [(loc_h, float(H)), (loc_w, float(W))])
        return _summary(counts, B * G, H * W, loc_h.numel() // K, t[0], D, K)

    @staticmethod
    def unpack(t, geo):
        off, m = t[1], t[2]
        return off.reshape(off.shape[:3] + (-1, 2)), m

    @staticmethod
    def repack(t, geo, coords):
        return (t[0], coords.reshape(t[1].shape).contiguous(), t[2], t[3])

    @staticmethod
    def unpack_grads(got, t, geo):
        return got[2].reshape(got[2].shape[:3] + (-1, 2)), got[3]

    @staticmethod
    def far_value(t, geo):
        return Dcnv3.far / geo[6]


class Dcnv4:
    name, kinds, pairings, plain_factor, naxes, softmax = "dcnv4", "vvc", PAIRINGS, True, 2, False
    names = ("output", "grad_input", "grad_offset_mask")
    fuzz_V = FUZZ_V

    @staticmethod
    def draw(spec, dtype, coord_dtype, seed):
        x, om, go, geo = R4.make_inputs(dtype=dtype, coord_dtype=coord_dtype, seed=seed, **spec)
        return (x, om, go), geo

    @classmethod
    def native(cls, t, geo, grads=None, deterministic=False, accumulate=True):
        from modulated_deform_conv_amd import dcnv4
        x, om, go = t
        out = dcnv4.dcnv4_forward(x, om, *geo, softmax=cls.softmax)
        g = dcnv4.dcnv4_backward(x, om, go, *geo, softmax=cls.softmax, **_call_kw(grads, deterministic, accumulate))
        torch.cuda.synchronize()
        return (out,) + tuple(g)

    @classmethod
    def ref(cls, t, geo):
        return (R4S.dcnv4_softmax_ref_grads if cls.softmax else R4.dcnv4_ref_grads)(*t, *geo)

    direct = None

    @staticmethod
    def grad_like(t):
        return t[:2]

    @staticmethod
    def _positions(t, geo):
        G, K = geo[4], R4.taps(geo[0], geo[7])
        off, _ = R4.unpack(t[1], G, K)
        return R4.positions(off, t[0].shape[1], t[0].shape[2], *geo[:4], G, geo[6], geo[7])

    @classmethod
    def gate(cls, t, geo):
        return R4.gate_of(t[1], t[0].shape[1], t[0].shape[2], *geo[:4], geo[4], geo[6], geo[7]).flatten(3)

    @classmethod
    def min_lattice_distance(cls, t, geo):
        return R4.min_lattice_distance(t[1], t[0].shape[1], t[0].shape[2], *geo[:4], geo[4], geo[6], geo[7])

    structure = classmethod(Dcnv3.structure.__func__)

    @staticmethod
    def unpack(t, geo):
        G, K = geo[4], R4.taps(geo[0], geo[7])
        off, m = R4.unpack(t[1], G, K)
        return off.reshape(off.shape[:3] + (-1, 2)), m

    @staticmethod
    def repack(t, geo, coords):
        G, K = geo[4], R4.taps(geo[0], geo[7])
        off, m = R4.unpack(t[1], G, K)
        return (t[0], R4.pack(coords.reshape(off.shape), m, G, K).contiguous(), t[2])

    @staticmethod
    def unpack_grads(got, t, geo):
        G, K = geo[4], R4.taps(geo[0], geo[7])
        off, m = R4.unpack(got[2], G, K)
        return off.reshape(off.shape[:3] + (-1, 2)), m

    far_value = staticmethod(Dcnv3.far_value)


class Dcnv4Softmax(Dcnv4):
    name, plain_factor, softmax = "dcnv4_softmax", False, True


class Msda:
    name, kinds, pairings, plain_factor, naxes = "msda", "vvcc", PAIRINGS, True, 2
    names = ("output", "grad_value", "grad_sampling_locations", "grad_attention_weights")
    fuzz_V = FUZZ_V
    R = RA

    @classmethod
    def draw(cls, spec, dtype, coord_dtype, seed):
        spec = dict(spec)
        shapes = tuple(tuple(s) for s in spec.pop("shapes"))
        return cls.R.make_inputs(shapes=list(shapes), dtype=dtype, coord_dtype=coord_dtype, seed=seed, **spec), shapes

    @staticmethod
    def native(t, geo, grads=None, deterministic=False, accumulate=True):
        from modulated_deform_conv_amd import msda
        value, loc, attn, go = t
        out = msda.ms_deform_attn_forward(value, geo, loc, attn)
        g = msda.ms_deform_attn_backward(value, geo, loc, attn, go, **_call_kw(grads, deterministic, accumulate))
        torch.cuda.synchronize()
        return (out,) + tuple(g)

    @staticmethod
    def ref(t, geo):
        return RA.msda_ref_grads(t[0], geo, t[1], t[2], t[3])

    @staticmethod
    def direct(t, geo):
        return RA.msda_ref_grads(t[0], geo, t[1], t[2], t[3], fn=RA.msda_direct)

    @staticmethod
    def grad_like(t):
        return t[:3]

    @classmethod
    def _loc(cls, t, geo):
        return t[1]

    @classmethod
    def _shapes(cls, geo):
        return geo

    @classmethod
    def gate(cls, t, geo):
        return cls.R.gate_of(cls._loc(t, geo), list(cls._shapes(geo)))

    @classmethod
    def min_lattice_distance(cls, t, geo):
        return cls.R.min_lattice_distance(cls._loc(t, geo), list(cls._shapes(geo)))

    @classmethod
    def structure(cls, t, geo):
        shapes = cls._shapes(geo)
        loc = cls._loc(t, geo)
        N, S, M, D = t[0].shape
        Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
        pos = cls.R.pixel_positions(loc, list(shapes))   # fastest axis first: (x, y[, z]), each [N, Lq, M, L, P]
        seg = (torch.arange(N).view(N, 1, 1, 1, 1) * M + torch.arange(M).view(1, 1, M, 1, 1)).expand(pos[0].shape)
        starts, total = cls.R.level_starts(list(shapes))
        assert total == S
        start = torch.tensor(starts).view(1, 1, 1, L, 1)
        axes = []
        for a in range(len(pos) - 1, -1, -1):   # slowest first; a shape row is (slowest, ..., fastest)
            size = torch.tensor([float(s[len(pos) - 1 - a]) for s in shapes], dtype=torch.float64).view(1, 1, 1, L, 1)
            axes.append((pos[a], size.expand(pos[a].shape)))
        counts = _corner_counts(seg, N * M, S, start, axes)
        return _summary(counts, N * M, S, N * Lq * M, t[0], D, L * P)

    @staticmethod
    def unpack(t, geo):
        return t[1], t[2]

    @staticmethod
    def repack(t, geo, coords):
        return (t[0], coords.contiguous(), t[2], t[3])

    @staticmethod
    def unpack_grads(got, t, geo):
        return got[2], got[3]

    @staticmethod
    def far_value(t, geo):
        return -3.0


class Msda3d(Msda):
    name, naxes = "msda3d", 3
    R = RA3

    @staticmethod
    def native(t, geo, grads=None, deterministic=False, accumulate=True):
        from modulated_deform_conv_amd import msda3d
        value, loc, attn, go = t
        out = msda3d.ms_deform_attn_3d_forward(value, geo, loc, attn)
        g = msda3d.ms_deform_attn_3d_backward(value, geo, loc, attn, go, **_call_kw(grads, deterministic, accumulate))
        torch.cuda.synchronize()
        return (out,) + tuple(g)

    @staticmethod
    def ref(t, geo):
        return RA3.msda3d_ref_grads(t[0], geo, t[1], t[2], t[3])

    @staticmethod
    def direct(t, geo):
        return RA3.msda3d_ref_grads(t[0], geo, t[1], t[2], t[3], fn=RA3.msda3d_direct)


class Fda(Msda):
    name, kinds, plain_factor = "fda", "vvc", False
    names = ("output", "grad_value", "grad_sampling_loc_attn")

    @staticmethod
    def draw(spec, dtype, coord_dtype, seed):
        spec = dict(spec)
        shapes = tuple(tuple(s) for s in spec.pop("shapes"))
        t = RF.make_inputs(shapes=list(shapes), dtype=dtype, coord_dtype=coord_dtype, seed=seed, **spec)
        return t, (shapes, spec["P"])

    @staticmethod
    def native(t, geo, grads=None, deterministic=False, accumulate=True):
        from modulated_deform_conv_amd import fda
        value, la, go = t
        shapes, P = geo
        out = fda.flash_deform_attn_forward(value, shapes, la, P)
        g = fda.flash_deform_attn_backward(value, shapes, la, P, go, **_call_kw(grads, deterministic, accumulate))
        torch.cuda.synchronize()
        return (out,) + tuple(g)

    @staticmethod
    def ref(t, geo):
        return RF.fda_ref_grads(t[0], list(geo[0]), t[1], geo[1], t[2])

    @staticmethod
    def direct(t, geo):
        return RF.fda_ref_grads(t[0], list(geo[0]), t[1], geo[1], t[2], fn=RA.msda_direct)

    @staticmethod
    def grad_like(t):
        return t[:2]

    @classmethod
    def _loc(cls, t, geo):
        return RF.unpack(t[1], len(geo[0]), geo[1])[0]

    @classmethod
    def _shapes(cls, geo):
        return geo[0]

    @staticmethod
    def unpack(t, geo):
        return RF.unpack(t[1], len(geo[0]), geo[1])

    @staticmethod
    def repack(t, geo, coords):
        _, logits = RF.unpack(t[1], len(geo[0]), geo[1])
        return (t[0], RF.pack(coords, logits), t[2])

    @staticmethod
    def unpack_grads(got, t, geo):
        return RF.unpack(got[2], len(geo[0]), geo[1])


class Droi:
    name, kinds, pairings, plain_factor, naxes = "droi", "vvc", PAIRINGS, True, 2
    names = ("output", "grad_input", "grad_offset")
    fuzz_V = FUZZ_V
    gate = None   # the reference module has no gate_of: RoIAlign's gate is closed, -1 <= loc <= size, inside droi_explicit

    @staticmethod
    def geo_of(spec):
        return dict(output_size=(spec["PH"], spec["PW"]), spatial_scale=spec.get("spatial_scale", 1.0),
                    sampling_ratio=spec.get("sampling_ratio", 0), gamma=spec.get("gamma", 0.1), max_grid=spec.get("max_grid", 8))

    @staticmethod
    def draw(spec, dtype, coord_dtype, seed):
        return RD.make_inputs(dtype=dtype, coord_dtype=coord_dtype, seed=seed, **spec), Droi.geo_of(spec)

    @staticmethod
    def native(t, geo, grads=None, deterministic=False, accumulate=True):
        from modulated_deform_conv_amd import droi
        inp, rois, off, go = t
        out = droi.deform_roi_pool_forward(inp, rois, off, **geo)
        g = droi.deform_roi_pool_backward(inp, rois, off, go, **geo, **_call_kw(grads, deterministic, accumulate))
        torch.cuda.synchronize()
        return (out,) + tuple(g)

    @staticmethod
    def ref(t, geo):
        return RD.droi_explicit(t[0], t[1], t[2], grad_output=t[3], **geo)

    @staticmethod
    def direct(t, geo):
        return RD.droi_autograd(t[0], t[1], t[2], grad_output=t[3], **geo)

    @staticmethod
    def grad_like(t):
        return (t[0], t[2])

    @staticmethod
    def _args(t, geo):
        PH, PW = geo["output_size"]
        return (t[0].shape[0], PH, PW, geo["spatial_scale"], geo["sampling_ratio"], geo["gamma"], geo["max_grid"])

    @classmethod
    def min_lattice_distance(cls, t, geo):
        return RD.min_lattice_distance(t[1], t[2], *cls._args(t, geo))

    @classmethod
    def structure(cls, t, geo):
        B, H, W, C = t[0].shape
        g = RD.geometry(t[1], t[2], *cls._args(t, geo))
        R, PH, PW, G = g["y"].shape
        iny, ylo, _, _, _ = RD._axis(g["y"], H)
        inx, xlo, _, _, _ = RD._axis(g["x"], W)
        m = g["live_y"][:, None, None, :, None] & g["live_x"][:, None, None, None, :] & iny[..., :, None] & inx[..., None, :]
        b = g["b"][:, None, None, None, None].expand(m.shape)
        counts = torch.zeros(B * H * W, dtype=torch.int64)
        for cy in (0, 1):
            for cx in (0, 1):
                yy, xx = (ylo + cy)[..., :, None].expand(m.shape), (xlo + cx)[..., None, :].expand(m.shape)
                read = m & (yy < H) & (xx < W)
                counts += torch.bincount(((b * H + yy.clamp(max=H - 1)) * W + xx.clamp(max=W - 1))[read], minlength=B * H * W)
        s = _summary(counts, 1, B * H * W, R * PH * PW, t[0], C, G * G)
        s["grids"] = sorted(set(zip(g["gh"].tolist(), g["gw"].tolist())))
        return s

    @staticmethod
    def unpack(t, geo):
        return t[2].permute(0, 2, 3, 1), None

    @staticmethod
    def repack(t, geo, coords):
        return (t[0], t[1], coords.permute(0, 3, 1, 2).contiguous(), t[3])

    @staticmethod
    def unpack_grads(got, t, geo):
        return got[2].permute(0, 2, 3, 1), None

    @staticmethod
    def far_value(t, geo):
        return -1e4   # times gamma * (RoI extent >= 1.5 px): hundreds of pixels outside


DAGG_G = (1, 2, 3, 4, 8)                 # groups of a random shape
DAGG_VG = (1, 2, 3, 4, 5, 6, 8, 33)      # vectors per group: VG = 33 with G >= 2 takes two rounds and carries a group


class Dagg:
    """Deformable aggregation: the anchor's whole row is the head (D = C), a unit (point, camera) the tap (K = U), and one
    segment per image of S = cams * S_cam rows; ``seg`` and ``rounds`` tell which reduction of dagg_bwd_coord_kernel runs."""
    name, kinds, pairings, plain_factor, naxes = "dagg", "vvcc", PAIRINGS, True, 2
    names = ("output", "grad_feature", "grad_sampling_location", "grad_weights")
    fuzz_V = tuple(sorted({g * vg for g in DAGG_G for vg in DAGG_VG}))

    @staticmethod
    def draw(spec, dtype, coord_dtype, seed):
        spec = dict(spec)
        shapes = tuple(tuple(s) for s in spec.pop("shapes"))
        return RG.make_inputs(shapes=list(shapes), dtype=dtype, coord_dtype=coord_dtype, seed=seed, **spec), shapes

    @staticmethod
    def native(t, geo, grads=None, deterministic=False, accumulate=True):
        from modulated_deform_conv_amd import dagg
        feature, loc, weights, go = t
        out = dagg.deformable_aggregation_forward(feature, geo, loc, weights)
        g = dagg.deformable_aggregation_backward(feature, geo, loc, weights, go, **_call_kw(grads, deterministic, accumulate))
        torch.cuda.synchronize()
        return (out,) + tuple(g)

    @staticmethod
    def ref(t, geo):
        return RG.dagg_ref_grads(t[0], geo, t[1], t[2], t[3])

    @staticmethod
    def direct(t, geo):
        return RG.dagg_ref_grads(t[0], geo, t[1], t[2], t[3], fn=RG.dagg_direct)

    @staticmethod
    def grad_like(t):
        return t[:3]

    @staticmethod
    def gate(t, geo):
        return RG.gate_of(t[1])   # [B, A, P, cams]

    @staticmethod
    def min_lattice_distance(t, geo):
        return RG.min_lattice_distance(t[1], list(geo))

    @staticmethod
    def structure(t, geo):
        feature, loc, weights = t[:3]
        B, S, C = feature.shape
        A, P, cams = loc.shape[1:4]
        L, G = weights.shape[4:]
        starts, s_cam = RG.level_starts(list(geo))
        assert S == cams * s_cam and L == len(geo)
        pos = RG.pixel_positions(loc, list(geo))   # [B, A, P, cams, L, 2], (x, y)
        # the operator's own gate, 0 < x < 1 and 0 < y < 1 on the stored location: a unit outside it reads no level
        gate = RG.gate_of(loc)[..., None].expand(pos.shape[:-1])
        x, y = (torch.where(gate, pos[..., a], torch.full_like(pos[..., a], -2.0)) for a in (0, 1))
        seg = torch.arange(B).view(B, 1, 1, 1, 1).expand(x.shape)
        start = torch.arange(cams).view(1, 1, 1, cams, 1) * s_cam + torch.tensor(starts).view(1, 1, 1, 1, L)
        hs, ws = (torch.tensor([float(s[a]) for s in geo], dtype=torch.float64).view(1, 1, 1, 1, L).expand(x.shape) for a in (0, 1))
        counts = _corner_counts(seg, B, S, start, [(y, hs), (x, ws)])
        s = _summary(counts, B, S, B * A, feature, C, P * cams)
        VG = C // G * esize(feature.dtype) // 16
        # DaggGeom.seg (dagg_host.hip): a group is an aligned power-of-two run of lanes inside one round
        s.update(VG=VG, seg=int(VG & (VG - 1) == 0 and VG <= s["VL"]), L=L)
        return s

    @staticmethod
    def unpack(t, geo):
        return t[1], t[2]

    @staticmethod
    def repack(t, geo, coords):
        return (t[0], coords.contiguous(), t[2], t[3])

    @staticmethod
    def unpack_grads(got, t, geo):
        return got[2], got[3]

    @staticmethod
    def far_value(t, geo):
        return -3.0


OPS = {op.name: op for op in (Dcnv3, Dcnv4, Dcnv4Softmax, Msda, Fda, Msda3d, Droi, Dagg)}


def tols(op, t):
    """Per result: value-typed results by the value dtype, coordinate and factor gradients by the coordinate dtype."""
    like = op.grad_like(t)
    cdt = next((g.dtype for g, k in zip(like, op.kinds[1:]) if k == "c" and g is not None), t[0].dtype)
    return tuple(TOL[t[0].dtype] if k == "v" else TOL[cdt] for k in op.kinds)


DEV = "cuda:0"
_SHORT = {F32: "f32", F16: "f16", BF16: "bf16", None: "same"}


def pairing_id(dtype, coord_dtype):
    return "%s-%s" % (_SHORT[dtype], _SHORT[coord_dtype])


def dev(t):
    return tuple(None if v is None else v.to(DEV) for v in t)


def nan_buffers(op, t):
    """Caller-allocated gradient buffers full of NaN, for the overwrite mode."""
    return tuple(None if v is None else torch.full_like(v, NAN) for v in op.grad_like(t))


def compare(op, tag, got, want, tol):
    """Every result against the fp64 reference with ``tests.util.assert_close`` (both criteria), at the tolerances ``tol``."""
    from tests.util import assert_close
    assert len(got) == len(want) == len(op.names)
    for what, a, b, e in zip(op.names, got, want, tol):
        if a is None or b is None:
            assert a is None and b is None, (tag, what)
            continue
        assert_close("%s %s" % (tag, what), a, b, e)


# ---- part 2: seeded random shapes ------------------------------------------------------------------------------------
FUZZ_SEEDS = 24
FUZZ_ATTEMPTS = 8
_V = FUZZ_V


def _head_channels(r, dtype):
    return (4 if dtype == F32 else 8) * r.choice(_V)


def _max_extent(dtype, coord_dtype, wide=24):
    """Extents above 16 need fp32 coordinates; same-type 16-bit coordinates stay at extents of 8 or less (a 16-bit location
    cannot keep MARGIN from the lattice of a wide level)."""
    return wide if (coord_dtype or dtype) == F32 else 8


def _draw_dcn(r, dtype, coord_dtype, v4):
    ext = _max_extent(dtype, coord_dtype)
    kernel = (r.randint(1, 5), r.randint(1, 5))
    spec = dict(B=r.randint(1, 3), G=r.choice((1, 2, 3, 4)), D=_head_channels(r, dtype), H=r.randint(1, ext), W=r.randint(1, ext),
                kernel=kernel, stride=(r.randint(1, 3), r.randint(1, 3)), pad=(r.randint(0, 2), r.randint(0, 2)),
                dilation=(r.randint(1, 2), r.randint(1, 2)), offset_scale=r.choice((0.5, 1.0, 2.0)))
    if v4:   # an odd kernel with a tap left (1 x 1 would leave K = 0)
        spec["remove_center"] = kernel[0] % 2 == 1 and kernel[1] % 2 == 1 and kernel != (1, 1) and r.random() < 0.5
    Ho, Wo = R3.out_hw(spec["H"], spec["W"], kernel, spec["stride"], spec["pad"], spec["dilation"])
    if Ho < 1 or Wo < 1:
        raise ValueError("shape rule: the output extent is below 1")
    return spec


def _draw_levels(r, ext, L, dims, depth=5):
    shapes = []
    for _ in range(L):
        if r.random() < 0.2:
            shapes.append((1,) * dims)
        else:
            shapes.append(tuple(r.randint(1, depth if dims == 3 and a == 0 else ext) for a in range(dims)))
    return tuple(shapes)


def _draw_attn(r, dtype, coord_dtype, dims):
    ext = _max_extent(dtype, coord_dtype, 24 if dims == 2 else 12)
    L = r.randint(1, 8)
    return dict(N=r.randint(1, 2), M=r.choice((1, 2, 3, 4, 8)), D=_head_channels(r, dtype), shapes=_draw_levels(r, ext, L, dims),
                Lq=r.randint(1, 40), P=r.randint(1, 5))


def _draw_droi(r, dtype, coord_dtype):
    ext = _max_extent(dtype, coord_dtype)
    return dict(B=r.randint(1, 3), C=_head_channels(r, dtype), H=r.randint(4, ext), W=r.randint(4, ext), R=r.randint(1, 6),
                PH=r.randint(1, 4), PW=r.randint(1, 4), spatial_scale=r.choice((1.0, 0.5, 0.25)), sampling_ratio=r.randint(0, 3),
                gamma=r.choice((0.05, 0.1, 0.3)), max_grid=r.choice((2, 4, 8)), with_offset=r.random() < 0.7)


def _draw_dagg(r, dtype, coord_dtype):
    """U = P * cams against VL, G and VG independently (V = G * VG: no power of two, a group across a round's end, V = 66
    and more in two or more rounds), one to eight levels shared by up to six cameras."""
    ext = _max_extent(dtype, coord_dtype)
    L = r.randint(1, 8)
    return dict(B=r.randint(1, 3), A=r.randint(1, 40), P=r.randint(1, 5), cams=r.randint(1, 6), shapes=_draw_levels(r, ext, L, 2),
                G=r.choice(DAGG_G), Dg=r.choice(DAGG_VG) * (4 if dtype == F32 else 8))


_DRAW = {"dcnv3": lambda r, d, c: _draw_dcn(r, d, c, False), "dcnv4": lambda r, d, c: _draw_dcn(r, d, c, True), "dagg": _draw_dagg,
         "dcnv4_softmax": lambda r, d, c: _draw_dcn(r, d, c, True), "msda": lambda r, d, c: _draw_attn(r, d, c, 2),
         "fda": lambda r, d, c: _draw_attn(r, d, c, 2), "msda3d": lambda r, d, c: _draw_attn(r, d, c, 3), "droi": _draw_droi}


def fuzz_pairing(op_name, seed):
    pairings = OPS[op_name].pairings
    return pairings[seed % len(pairings)]


@functools.lru_cache(maxsize=None)
def fuzz_case(op_name, seed):
    """(t, geo, spec, redraws) of seed ``seed`` of an operator: the spec is drawn from (operator, seed, attempt); a draw that
    fails an assertion of the generator or falls outside the operator's shape rule is drawn again, FUZZ_ATTEMPTS at most.  No
    seed is skipped: without a valid draw this raises."""
    op = OPS[op_name]
    dtype, coord_dtype = fuzz_pairing(op_name, seed)
    why = []
    for attempt in range(FUZZ_ATTEMPTS):
        r = random.Random("%s/%d/%d" % (op_name, seed, attempt))
        try:
            spec = _DRAW[op_name](r, dtype, coord_dtype)
            t, geo = op.draw(spec, dtype, coord_dtype, 1000 * seed + attempt)
        except (AssertionError, ValueError) as e:
            why.append("%d: %s" % (attempt, str(e)[:80]))
            continue
        return t, geo, spec, attempt
    raise RuntimeError("%s seed %d: no valid draw in %d attempts (%s)" % (op_name, seed, FUZZ_ATTEMPTS, "; ".join(why)))


# ---- parts 3 and 5: fixed cases ---------------------------------------------------------------------------------------
# name -> dict(op, spec, pairings, craft, claim).  ``claim``: what the case exists for, asserted by test_samp_cases_cpu.py
# against ``structure()``: rows / segments / longest / bytes are exact figures, ``chunks`` the scan chunks per segment,
# ``straddle`` a 64-row sort chunk that covers two segments, ``tail`` a partly filled last workgroup after at least one full.
def _crafted_attn(t, geo):
    """Every level-0 sample at x = 1.3, y = 1.4 of the 4 x 4 level: four lists take them all."""
    loc = t[1]
    loc[:, :, :, 0, :, 0] = (1.3 + 0.5) / 4
    loc[:, :, :, 0, :, 1] = (1.4 + 0.5) / 4
    return t


def _crafted_dcnv3(t, geo):
    """Every tap of every output pixel aimed at (1.3, 1.4): four lists take them all."""
    x, off, m, go = t
    loc_h, loc_w = R3.positions(torch.zeros_like(off), x.shape[1], x.shape[2], *geo[:4], geo[4], geo[6])
    off = torch.stack([1.3 - loc_w, 1.4 - loc_h], -1).reshape(off.shape).to(off.dtype)
    return (x, off, m, go)


# Input rule of the wide images.  2049 rows in one image are 3 x 683 pixels (683 is prime), and fp32 resolves a coordinate
# near 683 to 6.1e-5 px: a position the kernel forms in fp32 is up to 3e-5 px away from the fp64 position of the same stored
# offset, which moves a bilinear sample by 3e-5 x the difference of two neighbours.  With free fp32 offsets the output's
# per-element error against the fp64 reference measured 1.7e-4 (DCNv4, softmax) and 2.0e-4 (RoI pooling) on the MI355X, scaled
# maximum 3e-5 to 8e-5, and the reference itself moves by as much when its positions are rounded to fp32
# (tests/test_samp_cases_cpu.py, tests/test_gpu_samp_scale.py: WIDE_FREE).  The 2049-row cases therefore keep their
# coordinates on a binary grid on which every fp32 position sum is exact -- 10 bits before and at most 13 after the point --
# and the fp64 reference sees the positions the kernel sees.
def _dyadic_dcnv3(t, geo):
    """Offsets on multiples of 2^-10 (offset_scale 1): tap + offset + base is exact in fp32 below 1024."""
    x, off, m, go = t
    assert geo[6] == 1.0 and max(x.shape[1], x.shape[2]) < 1024
    return (x, (off.double() * 1024).round().div(1024).to(off.dtype), m, go)


def _dyadic_rois(R, H, W, seed):
    """RoIs of one image on multiples of 1/16, the last one over the image's last pixel."""
    gen = torch.Generator().manual_seed(seed)
    q = lambda v: (v * 16).floor() / 16
    x1 = q(torch.rand(R, generator=gen) * (W - 4.5))
    y1 = q(torch.rand(R, generator=gen) * (H - 2.5))
    w = 2 + q(torch.rand(R, generator=gen) * 2)
    h = 1.5 + q(torch.rand(R, generator=gen) * (H - 2.5))
    x1[-1], w[-1], y1[-1], h[-1] = W - 3.0, 2.5, H - 2.5, 2.0
    box = torch.stack([x1, y1, x1 + w, y1 + h], 1) + 0.5
    return [[0.0] + row for row in box.tolist()]


def _dyadic_droi(t, geo):
    """Offsets on multiples of 2^-6 beside RoIs on multiples of 2^-4, 2 x 2 bins of 2 x 2 samples, gamma = 2^-3 and
    spatial_scale 1: every term of a sample coordinate is a multiple of 2^-13 and every sum is exact in fp32 below 1024."""
    inp, rois, off, go = t
    assert geo["gamma"] == 0.125 and geo["spatial_scale"] == 1.0 and geo["output_size"] == (2, 2) and geo["sampling_ratio"] == 2
    assert torch.equal((rois * 16).round() / 16, rois) and max(inp.shape[1], inp.shape[2]) < 1024
    return (inp, rois, (off.double() * 64).round().div(64).to(off.dtype), go)


def _crafted_dagg(t, geo):
    """Every location at pixel (1.3, 1.4) of the 4 x 4 level, (0.4, 0.45) of the 2 x 2 one: every unit passes the gate, and
    four rows of each level take one entry per unit."""
    feature, loc, weights, go = t
    loc = torch.tensor(RG.CRAFTED_XY, dtype=torch.float64).to(loc.dtype).expand(loc.shape).contiguous()
    return (feature, loc, weights, go)


CRAFT = {"attn": _crafted_attn, "dcnv3": _crafted_dcnv3, "dyadic_dcnv3": _dyadic_dcnv3, "dyadic_droi": _dyadic_droi,
         "dagg": _crafted_dagg}
# the 3 x 683 image with free fp32 offsets: what the input rule above is measured on
WIDE_FREE = dict(op="dcnv3", spec=dict(B=2, G=2, D=4, H=3, W=683, kernel=3, pad=1), seed=17)
# per-element bound of WIDE_FREE against the fp64 reference: the reference's own movement under fp32 positions, 2.15e-4
# (grad_offset), with a margin; the scaled maximum stays at the project's 1e-4
WIDE_FREE_ELEM_TOL = 2.5e-4

_ATTN_BIG = ((70, 67), (33, 35), (9, 9), (1, 1))   # 5927 rows: a multiple of neither 64 nor 2048, three scan chunks
SCAN_CASES = {
    # rows per segment of 2048 (one full chunk), 2049 (the last chunk holds one row), and above 4096 (the `pre` loop takes a
    # second iteration from lo = 4096 on); more than one segment; many workgroups with a partly filled last one
    "msda_2048": dict(op="msda", spec=dict(N=2, M=2, D=4, shapes=((32, 64),), Lq=67, P=2), claim=dict(rows=2048, chunks=1)),
    "msda_2049": dict(op="msda", spec=dict(N=2, M=2, D=4, shapes=((32, 64), (1, 1)), Lq=67, P=2),
                      claim=dict(rows=2049, chunks=2, straddle=True, tail=True)),
    "msda_5927": dict(op="msda", spec=dict(N=2, M=3, D=8, shapes=_ATTN_BIG, Lq=301, P=2), pairings=((F32, None), (F16, F32)),
                      claim=dict(rows=5927, chunks=3, straddle=True, tail=True)),
    "fda_5927": dict(op="fda", spec=dict(N=2, M=3, D=8, shapes=_ATTN_BIG, Lq=301, P=2), pairings=((F16, F32),),
                     claim=dict(rows=5927, chunks=3, straddle=True, tail=True)),
    "dcnv3_2048": dict(op="dcnv3", spec=dict(B=2, G=2, D=4, H=32, W=64, kernel=3, pad=1), claim=dict(rows=2048, chunks=1)),
    "dcnv3_2049": dict(op="dcnv3", spec=dict(B=2, G=2, D=4, H=3, W=683, kernel=3, pad=1), craft="dyadic_dcnv3",
                       claim=dict(rows=2049, chunks=2, straddle=True, tail=True)),
    "dcnv3_4690": dict(op="dcnv3", spec=dict(B=2, G=3, D=8, H=67, W=70, kernel=3, pad=1),
                       claim=dict(rows=4690, chunks=3, straddle=True, tail=True)),
    "dcnv4_4690": dict(op="dcnv4", spec=dict(B=2, G=3, D=8, H=67, W=70, kernel=3, pad=1), pairings=((F16, F32),),
                       claim=dict(rows=4690, chunks=3, straddle=True, tail=True)),
    "dcnv4_softmax_2050": dict(op="dcnv4_softmax", spec=dict(B=2, G=2, D=4, H=41, W=50, kernel=3, pad=1, remove_center=True),
                               claim=dict(rows=2050, chunks=2, straddle=True, tail=True)),
    "msda3d_2048": dict(op="msda3d", spec=dict(N=2, M=2, D=4, shapes=((2, 32, 32),), Lq=67, P=2), claim=dict(rows=2048, chunks=1)),
    "msda3d_2049": dict(op="msda3d", spec=dict(N=2, M=2, D=4, shapes=((2, 32, 32), (1, 1, 1)), Lq=67, P=2),
                        claim=dict(rows=2049, chunks=2, straddle=True, tail=True)),
    "msda3d_4786": dict(op="msda3d", spec=dict(N=2, M=2, D=8, shapes=((5, 33, 29), (1, 1, 1)), Lq=150, P=2),
                        pairings=((F32, None), (F16, F32)), claim=dict(rows=4786, chunks=3, straddle=True, tail=True)),
    # the RoI pooling has ONE segment of B * H * W rows: chunks and workgroups, no second segment
    "droi_2048": dict(op="droi", spec=dict(B=2, C=4, H=32, W=32, R=37, PH=3, PW=3, sampling_ratio=2), claim=dict(rows=2048, chunks=1)),
    "droi_2049": dict(op="droi", spec=dict(B=1, C=4, H=3, W=683, rois=_dyadic_rois(80, 3, 683, 5), PH=2, PW=2, sampling_ratio=2,
                                           gamma=0.125), craft="dyadic_droi",
                      claim=dict(rows=2049, chunks=2, tail=True)),
    "droi_4794": dict(op="droi", spec=dict(B=2, C=8, H=47, W=51, R=41, PH=3, PW=3, sampling_ratio=0, max_grid=4),
                      pairings=((F32, None), (F16, F32)), claim=dict(rows=4794, chunks=3, tail=True)),
    # deformable aggregation: one segment per IMAGE of cams * S_cam rows, its own list kernel and gather.  2049 rows: the last
    # chunk holds the one-pixel level's row, which every gated-in unit samples.  4680 = 3 cameras x 1560 rows: the camera
    # boundaries at rows 1560 and 3120 fall inside scan chunks
    "dagg_2048": dict(op="dagg", spec=dict(B=2, A=67, P=2, cams=2, shapes=((32, 32),), G=1, Dg=4), claim=dict(rows=2048, chunks=1)),
    "dagg_2049": dict(op="dagg", spec=dict(B=2, A=135, P=2, cams=1, shapes=((32, 64), (1, 1)), G=1, Dg=4),
                      claim=dict(rows=2049, chunks=2, straddle=True, tail=True)),
    "dagg_4680": dict(op="dagg", spec=dict(B=2, A=101, P=2, cams=3, shapes=((37, 41), (6, 7), (1, 1)), G=3, Dg=8),
                      pairings=((F32, None), (F16, F32)), claim=dict(rows=4680, chunks=3, straddle=True, tail=True)),
}

LIST_CASES = {
    # lists of exactly 2048 (one key block), 2049 (a second pass of one key; the padding keys) and 2100 entries
    "msda_list_2048": dict(op="msda", spec=dict(N=1, M=1, D=4, shapes=((4, 4), (2, 2)), Lq=2048, P=1), craft="attn",
                           claim=dict(longest=2048)),
    "msda_list_2049": dict(op="msda", spec=dict(N=1, M=1, D=4, shapes=((4, 4), (2, 2)), Lq=2049, P=1), craft="attn",
                           claim=dict(longest=2049)),
    "msda_list_2100": dict(op="msda", spec=dict(N=1, M=1, D=4, shapes=((4, 4), (2, 2)), Lq=700, P=3), craft="attn",
                           claim=dict(longest=2100)),
    # K * output pixels = 3 * 28 * 25
    "dcnv3_list_2100": dict(op="dcnv3", spec=dict(B=1, G=1, D=4, H=28, W=25, kernel=(3, 1), pad=(1, 0)), craft="dcnv3",
                            claim=dict(longest=2100)),
    # an entry per sample, shared by all groups (the gather multiplies by weights[id * G + grp]): A * P units at one location
    "dagg_list_2048": dict(op="dagg", spec=dict(B=1, A=2048, P=1, cams=1, shapes=((4, 4), (2, 2)), G=1, Dg=4), craft="dagg",
                           claim=dict(longest=2048)),
    "dagg_list_2049": dict(op="dagg", spec=dict(B=1, A=2049, P=1, cams=1, shapes=((4, 4), (2, 2)), G=1, Dg=4), craft="dagg",
                           claim=dict(longest=2049)),
    "dagg_list_2100": dict(op="dagg", spec=dict(B=1, A=700, P=3, cams=1, shapes=((4, 4), (2, 2)), G=1, Dg=4), craft="dagg",
                           claim=dict(longest=2100)),
}

SEGMENT_CASES = {
    # 65535 segments on tiny tensors: the scan's grid.y at HIP's limit; every operator whose host code states the rule
    "msda_65535": dict(op="msda", spec=dict(N=65535, M=1, D=4, shapes=((1, 2),), Lq=1, P=1), claim=dict(segments=65535)),
    "fda_65535": dict(op="fda", spec=dict(N=21845, M=3, D=4, shapes=((1, 2),), Lq=1, P=1), claim=dict(segments=65535)),
    "msda3d_65535": dict(op="msda3d", spec=dict(N=65535, M=1, D=4, shapes=((1, 1, 2),), Lq=1, P=1), claim=dict(segments=65535)),
    "dcnv3_65535": dict(op="dcnv3", spec=dict(B=21845, G=3, D=4, H=2, W=2, kernel=1), claim=dict(segments=65535)),
    "dcnv4_65535": dict(op="dcnv4", spec=dict(B=21845, G=3, D=4, H=2, W=2, kernel=1), claim=dict(segments=65535)),
    "dcnv4_softmax_65535": dict(op="dcnv4_softmax", spec=dict(B=13107, G=5, D=4, H=2, W=2, kernel=(1, 3), pad=(0, 1)),
                                claim=dict(segments=65535)),
    # one segment per image: batch = 65535, the limit dagg_plan states for the lists
    "dagg_65535": dict(op="dagg", spec=dict(B=65535, A=1, P=1, cams=1, shapes=((1, 2),), G=1, Dg=4), claim=dict(segments=65535)),
}

FIXED_CASES = dict(SCAN_CASES, **LIST_CASES, **SEGMENT_CASES)


def fixed_params(table):
    """(name, dtype, coord_dtype) of every case of ``table`` (default pairing: fp32)."""
    return [(name, d, c) for name, case in table.items() for d, c in case.get("pairings", ((F32, None),))]


@functools.lru_cache(maxsize=None)
def wide_free_case():
    """(t, geo, fp64 reference, fp64 reference at positions formed in fp32) of WIDE_FREE."""
    t, geo = Dcnv3.draw(dict(WIDE_FREE["spec"]), F32, None, WIDE_FREE["seed"])
    return t, geo, Dcnv3.ref(t, geo), R3.dcnv3_ref_grads(*t, *geo, position_dtype=F32)


def fixed_ids(table):
    return ["%s-%s" % (name, pairing_id(d, c)) for name, d, c in fixed_params(table)]


@functools.lru_cache(maxsize=None)
def fixed_case(name, dtype=F32, coord_dtype=None):
    """(t, geo) of a fixed case: CPU tensors, computed once and left unchanged."""
    case = FIXED_CASES[name]
    op = OPS[case["op"]]
    t, geo = op.draw(dict(case["spec"]), dtype, coord_dtype, len(name) + 7)
    if case.get("craft"):
        t = CRAFT[case["craft"]](t, geo)
        assert op.min_lattice_distance(t, geo) >= R3.MARGIN
    return t, geo


@functools.lru_cache(maxsize=None)
def fixed_reference(name, dtype=F32, coord_dtype=None):
    t, geo = fixed_case(name, dtype, coord_dtype)
    return OPS[FIXED_CASES[name]["op"]].ref(t, geo)


# ---- part 4: the top MiB below 2^31 bytes -----------------------------------------------------------------------------
# fp32; the sampled tensor ends less than 2 MiB below 2^31 bytes while each image stays small.  Drawn on the GPU by
# tests/test_gpu_samp_scale.py; here the shapes only.  ``images``: the images compared against the reference.
TOP_IMAGES = (0, 1023, 2046)
TOP_CASES = {
    "msda": dict(N=2047, M=8, D=32, shapes=((32, 32),), Lq=5, P=2),
    "fda": dict(N=2047, M=8, D=32, shapes=((32, 32),), Lq=5, P=2),
    "msda3d": dict(N=2047, M=8, D=32, shapes=((4, 16, 16),), Lq=5, P=2),
    "dcnv3": dict(B=2047, G=8, D=32, H=32, W=32, kernel=1, stride=2),
    "dcnv4": dict(B=2047, G=8, D=32, H=32, W=32, kernel=1, stride=2),
    "dcnv4_softmax": dict(B=2047, G=8, D=32, H=32, W=32, kernel=(1, 3), stride=2, pad=(0, 1)),
    "droi": dict(B=2047, C=256, H=32, W=32, R=6, PH=2, PW=2, sampling_ratio=2),
    "dagg": dict(B=2047, A=5, P=2, cams=2, shapes=((16, 32),), G=8, Dg=32),
}


def top_bytes(op_name):
    s = TOP_CASES[op_name]
    if op_name == "dagg":
        return s["B"] * s["cams"] * sum(h * w for h, w in s["shapes"]) * s["G"] * s["Dg"] * 4
    if "shapes" in s:
        rows = sum(functools.reduce(lambda a, b: a * b, sh) for sh in s["shapes"])
        return s["N"] * rows * s["M"] * s["D"] * 4
    if op_name == "droi":
        return s["B"] * s["H"] * s["W"] * s["C"] * 4
    return s["B"] * s["H"] * s["W"] * s["G"] * s["D"] * 4


# ---- part 5: non-finite coordinates -----------------------------------------------------------------------------------
# One fuzz-sized case per operator; offset_scale = 2 so that a finite +-3e38 offset overflows once scaled, extents of at
# least 2 so that a +-3e38 location does.
NONFINITE_CASES = {
    "dcnv3": dict(B=2, G=2, D=8, H=7, W=6, kernel=3, pad=1, offset_scale=2.0),
    "dcnv4": dict(B=2, G=2, D=8, H=7, W=6, kernel=3, pad=1, offset_scale=2.0, remove_center=True),
    "dcnv4_softmax": dict(B=2, G=3, D=8, H=7, W=6, kernel=(3, 1), pad=(1, 0), offset_scale=2.0),
    "msda": dict(N=2, M=3, D=8, shapes=((6, 5), (3, 4), (2, 2)), Lq=9, P=2),
    "fda": dict(N=2, M=3, D=8, shapes=((6, 5), (3, 4), (2, 2)), Lq=9, P=2),
    "msda3d": dict(N=2, M=2, D=8, shapes=((3, 5, 4), (2, 2, 3)), Lq=9, P=2),
    "droi": dict(B=2, C=8, H=8, W=7, R=5, PH=3, PW=2, sampling_ratio=2, gamma=0.2),
    "dagg": dict(B=2, A=9, P=2, cams=3, shapes=((6, 5), (3, 4), (2, 2)), G=3, Dg=8),
}
NONFINITE_PAIRINGS = ((F32, None), (F16, None))
NAN, INF = float("nan"), float("inf")
NONFINITE_VALUES = {F32: (NAN, INF, -INF, 3e38, -3e38), F16: (NAN, INF, -INF, 65504.0)}


def nonfinite_axes(op_name):
    n = OPS[op_name].naxes
    return [(a,) for a in range(n)] + [tuple(range(n))]


@functools.lru_cache(maxsize=None)
def nonfinite_case(op_name, dtype, coord_dtype=None):
    op = OPS[op_name]
    return op.draw(dict(NONFINITE_CASES[op_name]), dtype, coord_dtype, 41)


def overwritten(op_name, dtype, coord_dtype=None):
    """[...] bool over the coordinate tuples of the case: a fixed tenth of them (every tenth, from the third on)."""
    t, geo = nonfinite_case(op_name, dtype, coord_dtype)
    coords, _ = OPS[op_name].unpack(t, geo)
    lead = coords.shape[:-1]
    n = 1
    for s in lead:
        n *= s
    return (torch.arange(n) % 10 == 2).view(lead)


def overwrite(op_name, dtype, coord_dtype, axes, value):
    """The tensors of the non-finite case with ``value`` written to the ``axes`` of the overwritten coordinate tuples."""
    op = OPS[op_name]
    t, geo = nonfinite_case(op_name, dtype, coord_dtype)
    coords, _ = op.unpack(t, geo)
    coords = coords.clone()
    sel = overwritten(op_name, dtype, coord_dtype)
    for a in axes:
        coords[..., a] = torch.where(sel, torch.full_like(coords[..., a], value), coords[..., a])
    return op.repack(t, geo, coords), geo


@functools.lru_cache(maxsize=None)
def replaced_case(op_name, dtype, coord_dtype, axes):
    """The same inputs with every such coordinate replaced by a finite one far outside the gate (normalised -3 for the
    attention operators and the aggregation, -1e4 px for the DCN operators, an offset of -1e4 RoI fractions for the RoI pooling), and the fp64
    reference of those inputs."""
    op = OPS[op_name]
    t, geo = nonfinite_case(op_name, dtype, coord_dtype)
    t2, _ = overwrite(op_name, dtype, coord_dtype, axes, op.far_value(t, geo))
    return t2, geo, op.ref(t2, geo)
