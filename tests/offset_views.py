"""Tensors at element-aligned addresses, with guarded margins ("Pointer alignment").

PyTorch's allocator hands out blocks on 256-byte (or coarser) boundaries, so a suite that allocates its tensors one by one
only ever shows a kernel pointers of that alignment.  ``at_offset`` copies a tensor into the middle of a flat buffer at a
chosen ELEMENT offset -- what a slice of a flat parameter buffer or a piece of ``torch.split`` looks like -- and fills the
buffer's two margins with the byte 0xA5; the checker it returns asserts that both margins are byte-identical afterwards.
``tests.util.guarded_run`` is the model: that one guards the workspace, this one the tensors.  No GPU is needed to import
or to use this module."""
import torch

GUARD_BYTES = 256
GUARD_PATTERN = 0xA5


def _extent(t):
    """Elements of storage a dense (possibly permuted) tensor spans: 1 + sum (size - 1) * stride."""
    return 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride())) if t.numel() else 0


def at_offset(t, k, guard=GUARD_BYTES, mod16=None):
    """Copy ``t`` into a flat buffer of its dtype at element offset ``guard_elems + k`` (``guard_elems`` = ``guard`` bytes
    in elements; the buffer's own address is a multiple of 256, so the view's is ``k * element_size`` modulo 16 for
    ``k * element_size < 16``).  Both margins -- ``guard`` bytes in front, at least ``guard`` bytes behind -- hold the byte
    0xA5.  Returns ``(view, check)``: ``view`` has ``t``'s shape AND strides (``as_strided``: a channels-last ``t`` gives a
    channels-last view) and ``t``'s values; ``check(what="")`` asserts that both margins are unchanged and names the first
    changed byte otherwise.  ``mod16``: the value ``view.data_ptr() % 16`` must have -- asserted here, so that a change of
    the allocator cannot make a test vacuous (default: ``k * element_size % 16``)."""
    assert t.numel() > 0 and k >= 0
    es = t.element_size()
    assert guard % es == 0 and guard % 16 == 0
    n = _extent(t)
    assert n == t.numel(), "at_offset takes dense tensors (any permutation of a contiguous one)"
    g = guard // es
    tail = g + (-(k + n)) % (16 // es if es < 16 else 1)   # the buffer ends on a 16-byte boundary
    flat = torch.empty(g + k + n + tail, dtype=t.dtype, device=t.device)
    raw = flat.view(torch.uint8)
    raw.fill_(GUARD_PATTERN)
    view = flat.as_strided(t.shape, t.stride(), g + k)
    view.copy_(t)
    want = (k * es) % 16 if mod16 is None else mod16
    assert flat.data_ptr() % 16 == 0, "the allocator no longer aligns to 16 bytes"
    assert view.data_ptr() == flat.data_ptr() + (g + k) * es and view.data_ptr() % 16 == want, (view.data_ptr() % 16, want)
    lo, hi = (g + k) * es, (g + k + n) * es   # the tensor's bytes inside `raw`

    def check(what=""):
        if raw.is_cuda:
            torch.cuda.synchronize(raw.device)
        for side, region, base in (("in front of", raw[:lo], -lo), ("behind", raw[hi:], 0)):
            bad = (region != GUARD_PATTERN).nonzero()
            assert bad.numel() == 0, "%s: %d bytes changed %s the tensor, first at byte %+d (now 0x%02x)" % (
                what or "at_offset", bad.numel(), side, int(bad[0]) + base, int(region[int(bad[0])]))

    return view, check

