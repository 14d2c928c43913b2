"""The scaffold the single-op GPU tests of test_backbone_gpu.py and test_plan_ops_gpu.py share: a weight blob and an arena laid out by
hand, a plan of n ops created, run once and destroyed, activations stored and read back.  WHAT an op is -- its smap_op fields, its
operands, its reference -- stays with each test.

POISONED ARENAS.  The executor's contract (csrc/plan_check.h, for_each_span of csrc/plan_check.cpp): an op reads its declared operands
and its window's zero page, and writes its declared outputs (split K: its partial tiles and tickets too); smap_plan_run clears the zero
pages, the ticket slices and the status words.  So every byte of a test arena that is NOT a stored tensor -- alignment gaps, output
regions, split-K partials, tickets, the guards around every tensor, the zero page itself -- holds a FILL byte, the plan runs once per
fill of FILLS on the same operands (run_filled), and
  * what the op may write must come out byte-identical under both fills (a read that leaves its operand and is used, or an output
    element that is never written, differs);
  * every other byte must be as it was (assert_only_written).
Guards (guard_bytes) keep an over-read off the neighbouring operand, which holds the same bytes under both fills."""
import ctypes as C

import torch

DEV = "cuda:0"
FILLS = (0xFF, 0x7B)    # 0xFF..: NaN as fp16 and fp32, 0xFFFFFFFF as a ticket; 0x7B7B..: large and FINITE (a ReLU's max turns NaN into 0)
ZERO_PAGE_RANGE = (0, 16384)  # csrc/plan_check.h SMAP_ZERO_PAGE of window 0: cleared by smap_plan_run, hence one of the ranges a run may write


def _al(n):
    return (n + 255) // 256 * 256


def raw8(t):
    return t.contiguous().view(torch.uint8).reshape(-1)


def stored(v, planes=2):
    """fp32 [..., C] -> its storage: fp16 [..., C], or fp16 [..., hi(C) | lo(C)] (split precision, csrc/conv.hip X3)."""
    hi = v.to(torch.float16)
    return hi if planes == 1 else torch.cat([hi, (v - hi.float()).to(torch.float16)], -1)


def guard_bytes(pixel_bytes, W=0):
    """The guard in front of and behind an arena tensor of `pixel_bytes` per pixel and W pixels per row: max(256, W + 2) pixels (256: the
    largest M tile; W + 2: the reach of a 3x3 tap off the image), rounded up to 256 bytes."""
    return _al(max(256, W + 2) * pixel_bytes)


def weight_blob(chunks, fill=0, guard=0):
    """Tensors -> (uint8 blob holding each on a 256-byte boundary, in order, `guard` bytes (a multiple of 256: one packed K tile of all
    rows) behind each, everything that is not a tensor = `fill`; their offsets)."""
    offs, cur = [], 0
    for c in chunks:
        offs.append(cur)
        cur += _al(c.numel() * c.element_size()) + _al(guard)
    blob = torch.full((cur,), fill, dtype=torch.uint8)
    for c, o in zip(chunks, offs):
        blob[o:o + c.numel() * c.element_size()] = raw8(c)
    return blob, offs


def arena_offsets(sizes, guards=None):
    """Byte sizes (None: absent, offset -1), 256-aligned one behind the other behind the zero page, guards[i] bytes (a multiple of 256)
    in front of and behind entry i -> (their offsets, the arena's bytes)."""
    from smap_amd.engine import ZERO_PAGE
    offs, cur = [], ZERO_PAGE
    for i, n in enumerate(sizes):
        gd = guards[i] if guards is not None and n is not None else 0
        assert gd % 256 == 0
        offs.append(-1 if n is None else cur + gd)
        cur += _al(n or 0) + (2 * gd if n is not None else 0)
    return offs, cur + 256


def arena_of(tensors, *regions, fill=0, guards=None):
    """Stored tensors (None: absent, offset -1), then regions of `regions` bytes, laid out by arena_offsets with `guards` (one per tensor
    and region) -> (uint8 host arena, the offsets of all of them).  Every byte that is not a stored tensor = `fill`: regions, gaps,
    guards, the zero page."""
    offs, total = arena_offsets([None if t is None else t.numel() * t.element_size() for t in tensors] + list(regions), guards)
    arena = torch.full((total,), fill, dtype=torch.uint8)
    for t, o in zip(tensors, offs):
        if t is not None:
            arena[o:o + t.numel() * t.element_size()] = raw8(t)
    return arena, offs


def run_plan(ops, n, arena, blob, out=None, inp=None):
    """A plan of the n smap_op in `ops` (one op or an array): create, run once on the current stream over arena / blob (copied to the device
    unless they are there) [, the output buffer `out` and the device images `inp` of a stem], synchronise, destroy.  Returns the device
    arena."""
    from smap_amd import lib as L
    lib = L.load()
    h = C.c_void_p()
    L.check(lib.smap_plan_create(ops if isinstance(ops, C.Array) else C.byref(ops), n, C.byref(h)), "smap_plan_create")
    arena, blob = arena.to(DEV), blob.to(DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        L.check(lib.smap_plan_run(h, C.c_void_p(inp.data_ptr()) if inp is not None else None, C.c_void_p(arena.data_ptr()),
                                  C.c_void_p(blob.data_ptr()), C.c_void_p(out.data_ptr()) if out is not None else None, st), "run")
        torch.cuda.synchronize()
    finally:
        lib.smap_plan_destroy(h)
    return arena


# -- the poisoned-arena property
def region_name(off, regions):
    """Which of `regions` [(name, lo, hi)] byte `off` falls in -- or the guard / gap behind which of them."""
    for name, lo, hi in regions:
        if lo <= off < hi:
            return name
    behind = [r for r in regions if r[2] <= off]
    return "the guard or gap behind %s" % max(behind, key=lambda r: r[2])[0] if behind else "the guard or gap in front of every region"


def _first_difference(a, b, base=0):
    """Offset (+ base) of the first byte at which the uint8 tensors differ, or None."""
    if torch.equal(a, b):
        return None
    return base + int((a != b).nonzero()[0])


def assert_only_written(before, after, written, regions=(), what="arena"):
    """`before`, `after`: one buffer (uint8, same device) in front of and behind a run; `written`: the byte ranges [(lo, hi)] the run may
    write, from the test's own layout as for_each_span states them.  Every other byte must be bit-identical; the failure names the first
    offset that is not and the region of `regions` [(name, lo, hi)] it falls in."""
    assert before.dtype == after.dtype == torch.uint8 and before.shape == after.shape
    n, cur = before.numel(), 0
    for lo, hi in sorted(written) + [(n, n)]:
        assert 0 <= lo <= hi <= n, (lo, hi, n)
        if lo > cur:
            off = _first_difference(before[cur:lo], after[cur:lo], cur)
            if off is not None:
                raise AssertionError("%s byte %d, in %s, changed outside the ranges the run may write: 0x%02x -> 0x%02x"
                                     % (what, off, region_name(off, regions), int(before[off]), int(after[off])))
        cur = max(cur, hi)


def assert_same_across_fills(a, b, written, regions=(), what="arena"):
    """The ranges a run may write, out of two runs on the same operands under two fills: byte-identical, or the failure names the first
    offset that differs -- a value that depends on bytes the op does not own, or an element that was never written."""
    for lo, hi in sorted(written):
        off = _first_difference(a[lo:hi], b[lo:hi], lo)
        if off is not None:
            raise AssertionError("%s byte %d, in %s, differs between fills: 0x%02x / 0x%02x -- it depends on bytes the op does not own, or "
                                 "was never written" % (what, off, region_name(off, regions), int(a[off]), int(b[off])))


def run_filled(ops, n, arena_for, blob_for, written, regions=(), out_for=None, out_written=(), inp=None, fills=FILLS):
    """The double run.  arena_for(fill) / blob_for(fill) [/ out_for(fill)]: the host (or device) arena, weight blob [and fp32 output buffer]
    of the SAME operands with every other byte = fill.  Runs the plan once per fill; after each run nothing but `written` of the arena
    [`out_written` of the output buffer] has changed and the weight blob is as it was; across the runs `written` [`out_written`] is
    byte-identical, ticket slices and zero page included (both end at zero).  Returns ([device arena per fill], [output buffer per fill])."""
    arenas, outs = [], []
    for fill in fills:
        before, blob0 = arena_for(fill).to(DEV), blob_for(fill).to(DEV)
        out0 = out_for(fill).to(DEV) if out_for is not None else None
        arena, blob, out = before.clone(), blob0.clone(), (out0.clone() if out0 is not None else None)
        run_plan(ops, n, arena, blob, out, inp)
        assert_only_written(before, arena, written, regions)
        assert _first_difference(blob0, blob) is None, "weight blob byte %d was written" % _first_difference(blob0, blob)
        if out is not None:
            assert_only_written(raw8(out0), raw8(out), out_written, what="output buffer")
        arenas.append(arena)
        outs.append(out)
    for k in range(1, len(fills)):
        assert_same_across_fills(arenas[0], arenas[k], written, regions)
        if out_for is not None:
            assert_same_across_fills(raw8(outs[0]), raw8(outs[k]), out_written, what="output buffer")
    return arenas, outs


class FilledLaunch:
    """One hand-made plan on poisoned arenas.  operands: [(name, stored tensor or None (absent: offset -1), bytes per pixel, W)];
    outputs: [(name, bytes, bytes per pixel, W)] -- every range the plan may write besides the zero page (outputs, segment outputs,
    split-K partials, tickets; 0 bytes: absent); chunks: the weight blob's tensors, `blob_guard` bytes behind each.  short_in: the LAST
    short_in bytes of the first operand are left to the fill (the negative control: real operand bytes then differ between the runs).
    .offs: arena offsets of operands, then outputs; .woffs: the chunks' offsets in the blob."""

    def __init__(self, operands, outputs, chunks=(), blob_guard=0, short_in=0):
        self.tensors = [t for _, t, _, _ in operands]
        if short_in:
            self.tensors[0] = raw8(self.tensors[0])[:-short_in]
        self.out_bytes = [n for _, n, _, _ in outputs]
        self.guards = [guard_bytes(p, w) for _, _, p, w in list(operands) + list(outputs)]
        sizes = [None if t is None else t.numel() * t.element_size() for t in self.tensors] + self.out_bytes
        self.offs, self.total = arena_offsets(sizes, self.guards)
        names = [o[0] for o in operands] + [o[0] for o in outputs]
        self.regions = [("the zero page",) + ZERO_PAGE_RANGE] + [(nm, o, o + n) for nm, o, n in zip(names, self.offs, sizes) if n]
        self.chunks, self.blob_guard = list(chunks) or [torch.zeros(64, dtype=torch.float32)], blob_guard
        self.woffs = weight_blob(self.chunks, 0, blob_guard)[1]

    def arena(self, fill):
        return arena_of(self.tensors, *self.out_bytes, fill=fill, guards=self.guards)[0]

    def blob(self, fill):
        return weight_blob(self.chunks, fill, self.blob_guard)[0]

    def written(self, short_out=0):
        """The zero page and every output; short_out: the first output declared that many bytes short (the negative control)."""
        w = [(o, o + n) for o, n in zip(self.offs[len(self.tensors):], self.out_bytes) if n]
        if short_out:
            w[0] = (w[0][0], w[0][1] - short_out)
        return [ZERO_PAGE_RANGE] + w

    def run(self, ops, n=1, short_out=0, out_for=None, out_written=(), inp=None):
        """run_filled -> the device arena of the first fill (FILLS[0]: a stray fill is a NaN there); .arenas / .outs keep both runs."""
        self.arenas, self.outs = run_filled(ops, n, self.arena, self.blob, self.written(short_out), self.regions, out_for, out_written, inp)
        return self.arenas[0]


def read_act(arena, off, shape, planes=1, dtype=torch.float16, to=torch.float32):
    """The NHWC activation of `shape` at byte `off` of the arena as `to` values: fp16 / fp32 (dtype) as stored, or hi + lo of split precision."""
    B, H, W, Cs = shape
    raw = arena[off:off + B * H * W * Cs * planes * dtype.itemsize].cpu().view(dtype)
    if planes == 1:
        return raw.view(B, H, W, Cs).to(to)
    v = raw.view(B, H, W, 2, Cs).to(to)
    return v[..., 0, :] + v[..., 1, :]


# -- ops that go through Graph(build=False): tensors are engine.Tensor, values travel as NCHW f64
class GraphArena:
    """The arena of a hand-appended schedule whose `inputs` nobody produces, laid out BY HAND: every tensor (split-K scratch and tickets
    included) one behind the other behind the zero page with guard_bytes of its own pixel stride in front of and behind it.  Values are
    `put` once; host(fill) is the arena with those values and every other byte = fill."""

    def __init__(self, g, *inputs):
        for t in inputs:
            t.first = 0
        g.allocate(reuse=False)                                     # liveness and the checks of the packer; the offsets are replaced
        self.g, self.values = g, []
        every = g.tensors + g.scratch_tensors + ([g.kcount] if g.kcount is not None else [])
        acts = {id(t) for t in g.tensors}
        guards = [guard_bytes(t.C * t.esize * t.planes if id(t) in acts else 256, t.W) for t in every]
        offs, g.arena_bytes = arena_offsets([t.nbytes for t in every], guards)
        for t, o in zip(every, offs):
            t.off = o
        self.regions = [(t.name, t.off, t.off + t.nbytes) for t in every]
        self.produced = [t for t in every if not any(t is u for u in inputs)]

    def put(self, t, v):
        """NCHW fp32 -> the storage of tensor t; returns what was stored, NCHW f64."""
        s = stored(v.permute(0, 2, 3, 1).contiguous(), t.planes)
        self.values.append((t.off, raw8(s)))
        return s.double().view(t.B, t.H, t.W, t.planes, -1).sum(3).permute(0, 3, 1, 2)

    def host(self, fill):
        arena = torch.full((self.g.arena_bytes,), fill, dtype=torch.uint8)
        for off, raw in self.values:
            arena[off:off + raw.numel()] = raw
        return arena

    def blob(self, fill):
        """Graph.weight_blob with the alignment gaps and one guard of 64 KiB behind the last chunk = fill."""
        blob = torch.full((_al(self.g.woff) + 65536,), fill, dtype=torch.uint8)
        for off, raw in self.g.wchunks:
            blob[off:off + raw.numel()] = raw
        return blob

    def written(self):
        """What the schedule's ops may write: every tensor somebody produces (outputs, segment outputs, partial tiles, tickets), the zero page."""
        return [ZERO_PAGE_RANGE] + [(t.off, t.off + t.nbytes) for t in self.produced]

    def run(self, ops, n, out_for=None, out_written=()):
        """run_filled over this arena -> (the device arena of the first fill, its output buffer)."""
        arenas, outs = run_filled(ops, n, self.host, self.blob, self.written(), self.regions, out_for, out_written)
        return arenas[0], outs[0]


def get(arena, t):
    """Tensor t out of the device arena, NCHW f64."""
    return read_act(arena, t.off, (t.B, t.H, t.W, t.C), t.planes, torch.float16 if t.esize == 2 else torch.float32, torch.float64).permute(0, 3, 1, 2)
