"""The scaffold the single-op GPU tests of test_backbone_gpu.py share: a weight blob and an arena laid out by hand, a plan of n ops created,
run once and destroyed, activations stored and read back.  WHAT an op is -- its smap_op fields, its operands, its reference -- stays with
each test."""
import ctypes as C

import torch

DEV = "cuda:0"


def _al(n):
    return (n + 255) // 256 * 256


def raw8(t):
    return t.contiguous().view(torch.uint8).reshape(-1)


def stored(v, planes=2):
    """fp32 [..., C] -> its storage: fp16 [..., C], or fp16 [..., hi(C) | lo(C)] (split precision, csrc/conv.hip X3)."""
    hi = v.to(torch.float16)
    return hi if planes == 1 else torch.cat([hi, (v - hi.float()).to(torch.float16)], -1)


def weight_blob(chunks):
    """Tensors -> (uint8 blob holding each on a 256-byte boundary, in order; their offsets)."""
    offs, cur = [], 0
    for c in chunks:
        offs.append(cur)
        cur += _al(c.numel() * c.element_size())
    blob = torch.zeros(cur, dtype=torch.uint8)
    for c, o in zip(chunks, offs):
        blob[o:o + c.numel() * c.element_size()] = raw8(c)
    return blob, offs


def arena_offsets(sizes):
    """Byte sizes (None: absent, offset -1), 256-aligned one behind the other behind the zero page -> (their offsets, the arena's bytes)."""
    from smap_amd.engine import ZERO_PAGE
    offs, cur = [], ZERO_PAGE
    for n in sizes:
        offs.append(-1 if n is None else cur)
        cur += _al(n or 0)
    return offs, cur + 256


def arena_of(tensors, *regions):
    """Stored tensors (None: absent, offset -1), then zeroed regions of `regions` bytes, laid out by arena_offsets -> (uint8 host arena,
    the offsets of all of them)."""
    offs, total = arena_offsets([None if t is None else t.numel() * t.element_size() for t in tensors] + list(regions))
    arena = torch.zeros(total, dtype=torch.uint8)
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


def read_act(arena, off, shape, planes=1, dtype=torch.float16, to=torch.float32):
    """The NHWC activation of `shape` at byte `off` of the arena as `to` values: fp16 / fp32 (dtype) as stored, or hi + lo of split precision."""
    B, H, W, Cs = shape
    raw = arena[off:off + B * H * W * Cs * planes * dtype.itemsize].cpu().view(dtype)
    if planes == 1:
        return raw.view(B, H, W, Cs).to(to)
    v = raw.view(B, H, W, 2, Cs).to(to)
    return v[..., 0, :] + v[..., 1, :]


# -- ops that go through Graph(build=False): tensors are engine.Tensor, values travel as NCHW f64
def graph_arena(g, *inputs):
    """The zeroed device arena of a hand-appended schedule whose `inputs` nobody produces."""
    for t in inputs:
        t.first = 0
    g.allocate(reuse=False)
    return torch.zeros(g.arena_bytes, dtype=torch.uint8, device=DEV)


def put(arena, t, v):
    """NCHW fp32 -> the storage of tensor t in the device arena; returns what was stored, NCHW f64."""
    s = stored(v.permute(0, 2, 3, 1).contiguous(), t.planes)
    arena[t.off:t.off + t.nbytes].view(torch.float16).copy_(s.reshape(-1).to(DEV))
    return s.double().view(t.B, t.H, t.W, t.planes, -1).sum(3).permute(0, 3, 1, 2)


def get(arena, t):
    """Tensor t out of the device arena, NCHW f64."""
    return read_act(arena, t.off, (t.B, t.H, t.W, t.C), t.planes, torch.float16 if t.esize == 2 else torch.float32, torch.float64).permute(0, 3, 1, 2)
