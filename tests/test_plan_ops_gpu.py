"""stem_kernel, stem_pool_kernel, maxpool_kernel, upadd_kernel and headsum_kernel of csrc/plan.hip one op per plan, against float64 on
the CPU from the operands as stored, at the shapes where their edge code runs: ragged tiles, odd extents, extents of 1, the second trip
of the grid-stride loops, non-finite pixels, every number of head sources.  Shapes, op builders and references: tests/plan_ops.py (the
checker's side of the same ops: test_plan_ops_cpu.py).  Every test prints its worst error as a fraction of its bound.

Every plan runs once per fill on poisoned arenas with guards around each tensor (single_op.FilledLaunch / run_filled): what the op may
write -- its output, the zero page and, in the fp32 output buffer, the maps and the status words smap_plan_run clears -- is byte-identical
under both fills, and no other byte of the arena, the output buffer or the weight blob changes."""
import pytest
import torch
import torch.nn.functional as F

import plan_ops as P
from single_op import DEV, ZERO_PAGE_RANGE, FilledLaunch, arena_offsets, guard_bytes, read_act, run_filled, stored

pytestmark = pytest.mark.gpu

PRECISIONS = [False, True]
P_IDS = ["f16", "x3"]


def conv_tolerance(ref, x3):
    """The single-conv bounds of test_backbone_gpu.py."""
    m = float(ref[torch.isfinite(ref)].abs().max()) if torch.isfinite(ref).any() else 0.0
    return (3e-6 * m + 1e-6) if x3 else (2e-3 * m + 1e-3)


def report(what, err, bound):
    """Worst |err| / bound over the elements (bound: a number or a tensor)."""
    frac = float((err / bound).max()) if err.numel() else 0.0
    print("%s: worst error %.3g of its bound" % (what, frac))
    return frac


def same_bits(a, b):
    """fp16 tensors equal bit for bit, a NaN equal to any NaN."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a.view(torch.int16)[~na], b.view(torch.int16)[~nb])


# ------------------------------------------------------------------------------------------------------------------- stem
def stem_operands(B, H, W, x3, flip_from=0, nan=False, dead_channels=False, seed=0):
    from smap_amd.engine import pack_stem_weights
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(flip_from or B, 3, H, W, generator=g)
    if nan:                                     # column 4 j + 2: the eighth, zero-weight column of output pixel 2 j - 1's K granules (K = kh, c, kw 7 -> 8)
        x[0, 1, H // 2, W // 4 * 2 | 2] = float("nan")
    w = torch.randn(64, 3, 7, 7, generator=g, dtype=torch.float64) * (1.0 / 147) ** 0.5
    bias = torch.randn(64, generator=g)
    if dead_channels:
        bias[::3] = -100.0                      # relu(conv + bias) is 0 at every pixel of these channels
    wk, acc_scale = pack_stem_weights(w, x3)
    return x, w, bias, [wk, bias], acc_scale


def run_stem(ops_of, outputs, x, chunks):
    """ops_of(arena offsets, w_off, bias_off) -> the ops; outputs: (byte sizes, bytes per pixel, pixels per row) of the tensors they write.
    Returns the device arena of the first fill and the offsets."""
    launch = FilledLaunch([], [("output %d" % i, n, p, w) for i, (n, p, w) in enumerate(zip(*outputs))], chunks, blob_guard=4096)
    ops = ops_of(launch.offs, *launch.woffs)
    from smap_amd import lib as L
    arr = (L.SmapOp * len(ops))(*ops)
    return launch.run(arr, len(ops), inp=x.to(DEV)), launch.offs


STEM_CASES = [(s, 0) for s in P.STEM_SHAPES] + [(P.STEM_FLIP[:3], P.STEM_FLIP[3])]
STEM_IDS = ["%dx%dx%d%s" % (*s, " flip" if f else "") for s, f in STEM_CASES]


@pytest.mark.parametrize("x3", PRECISIONS, ids=P_IDS)
@pytest.mark.parametrize("case", STEM_CASES, ids=STEM_IDS)
def test_stem_vs_float64_conv(case, x3):
    """SMAP_OP_STEM against relu(F.conv2d(stride 2, padding 3) + bias) in float64 of the stored image and weights, under the single-conv
    bounds (f16: 2e-3 max|ref| + 1e-3; x3: 3e-6 max|ref| + 1e-6), at output sizes that are no multiple of the 16 x 16 tile, odd H and W
    (an incomplete last patch row / column) and images smaller than one patch; with flip_from the second half of the batch is the stem
    of the mirrored images.  Nothing but [B, Ho, Wo, planes * 64] and the zero page of the poisoned arena is written (run_stem)."""
    (B, H, W), flip_from = case
    x, w, bias, chunks, acc_scale = stem_operands(B, H, W, x3, flip_from)
    Ho, Wo, pl = P.conv_out(H), P.conv_out(W), 1 + x3
    arena_d, offs = run_stem(lambda o, w_off, bias_off: [P.stem_op(B, H, W, x3, o[0], w_off, bias_off, acc_scale, flip_from)],
                             P.stem_sizes(B, H, W, x3), x, chunks)
    got = read_act(arena_d, offs[0], (B, Ho, Wo, 64), pl, to=torch.float64)
    ref = P.stem_reference(x, w, bias, x3, flip_from)
    assert report("stem", (got - ref).abs().max().view(1), conv_tolerance(ref, x3)) <= 1.0


POOLED_CASES = [(c, "") for c in STEM_CASES] + [(((1, 37, 61), 0), "nan"), (((2, 32, 70), 0), "dead")]
POOLED_IDS = STEM_IDS + ["1x37x61 one NaN pixel", "2x32x70 channels at zero"]


@pytest.mark.parametrize("x3", PRECISIONS, ids=P_IDS)
@pytest.mark.parametrize("case", POOLED_CASES, ids=POOLED_IDS)
def test_stem_pool_vs_float64_and_vs_the_two_kernels(case, x3):
    """SMAP_OP_STEMPOOL against F.max_pool2d(3, 2, 1) of the float64 stem under the same bounds, and bit for bit against SMAP_OP_STEM
    followed by SMAP_OP_MAXPOOL.  One NaN pixel in the image: the NaN mask of both routes is torch's (max_pool2d propagates NaN).  A bias
    of -100 on every third channel: those channels are 0 at every pixel, the value the fused kernel pads its LDS tile with."""
    ((B, H, W), flip_from), special = case
    x, w, bias, chunks, acc_scale = stem_operands(B, H, W, x3, flip_from, nan=special == "nan", dead_channels=special == "dead")
    Hs, Ws, pl = P.conv_out(H), P.conv_out(W), 1 + x3
    Ho, Wo = P.conv_out(Hs), P.conv_out(Ws)
    stem_bytes, pool_bytes = B * Hs * Ws * 64 * 2 * pl, B * Ho * Wo * 64 * 2 * pl
    fused_d, fo = run_stem(lambda o, w_off, bias_off: [P.stem_op(B, H, W, x3, o[0], w_off, bias_off, acc_scale, flip_from, pool=True)],
                           P.stem_sizes(B, H, W, x3, pool=True), x, chunks)
    two_d, to = run_stem(lambda o, w_off, bias_off: [P.stem_op(B, H, W, x3, o[0], w_off, bias_off, acc_scale, flip_from),
                                                     P.maxpool_op(B, Hs, Ws, 64, x3, o[0], o[1])],
                         ([stem_bytes, pool_bytes], [128 * pl] * 2, [Ws, Wo]), x, chunks)
    ref = P.maxpool_reference(P.stem_reference(x, w, bias, x3, flip_from))
    if special == "dead":
        assert not ref[..., ::3].any() and ref[..., 1::3].any()
    nan = torch.isnan(ref)
    assert bool(nan.any()) == (special == "nan") and not nan.all()
    for name, arena_d, off in (("stem+pool", fused_d, fo[0]), ("stem, pool", two_d, to[1])):
        got = read_act(arena_d, off, (B, Ho, Wo, 64), pl, to=torch.float64)
        assert torch.equal(torch.isnan(got), nan), name
        assert report(name, (got - ref)[~nan].abs().max().view(1), conv_tolerance(ref, x3)) <= 1.0
    raw = lambda a, off: a[off:off + pool_bytes].cpu().view(torch.float16)
    assert same_bits(raw(fused_d, fo[0]), raw(two_d, to[1]))


# --------------------------------------------------------------------------------------------------------------- max-pool
def pool_input(B, H, W, Cc, kind, x3):
    """fp32 NHWC: all negative (a zero padding would win every border window), or with NaN / +inf / -inf in channels 0 / 1 / 2 of an
    interior, an edge and a corner pixel.  Split precision: one pixel whose pair is (hi, lo = +half an ulp of an ODD hi) -- hi + lo
    rounds to the EVEN neighbour of hi, so re-splitting the sum does not give the pair back."""
    g = torch.Generator().manual_seed(5)
    v = torch.randn(B, H, W, Cc, generator=g)
    tie = 1 + 2.0 ** -10 + 2.0 ** -11 - 2.0 ** -23
    if kind == "negative":
        v = -v.abs() - 0.5
        tie = -tie / 4
    else:
        for y, xx in ((H // 2, W // 2), (H // 2, 0), (H - 1, W - 1)):
            v[B - 1, y, xx, 0], v[B - 1, y, xx, 1], v[B - 1, y, xx, 2] = float("nan"), float("inf"), float("-inf")
        tie = tie * 8
    if x3:
        v[0, H // 3, W // 3, Cc - 1] = tie
    return v


@pytest.mark.parametrize("kind", ["negative", "nonfinite"])
@pytest.mark.parametrize("x3", PRECISIONS, ids=P_IDS)
@pytest.mark.parametrize("shape", P.POOL_SHAPES, ids=["%dx%dx%dx%d" % s for s in P.POOL_SHAPES])
def test_maxpool_is_exact(shape, x3, kind):
    """SMAP_OP_MAXPOOL equals F.max_pool2d(3, 2, 1) in float64 of the stored values (fp16, or hi + lo) exactly, NaN for NaN, at odd
    sizes, a single pixel and a channel count that is no multiple of 64.  Split precision: the output pair is the winning pixel's own
    (hi, lo), for every finite winner (an infinite value has lo = inf - inf = NaN in storage: it is a NaN to every reader, pool included)."""
    B, H, W, Cc = shape
    Ho, Wo, pl = P.conv_out(H), P.conv_out(W), 1 + x3
    s = stored(pool_input(B, H, W, Cc, kind, x3), pl)
    launch = FilledLaunch([("in", s, Cc * 2 * pl, W)], [("out", B * Ho * Wo * Cc * 2 * pl, Cc * 2 * pl, Wo)])
    in_off, out_off = launch.offs
    arena_d = launch.run(P.maxpool_op(B, H, W, Cc, x3, in_off, out_off))
    val = s.double().view(B, H, W, pl, Cc).sum(3)
    ref, win = P.maxpool_reference(val, return_indices=True)
    got = read_act(arena_d, out_off, (B, Ho, Wo, Cc), pl, to=torch.float64)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan], ref[~nan])
    if kind == "negative":
        assert bool((ref < 0).all())
    else:
        assert bool(nan.any()) and (x3 or (bool((ref == float("inf")).any()) and (H > 1 or bool((ref == float("-inf")).any()))))
    if x3:
        pairs_in = s.view(B, H * W, 2, Cc)
        pairs_out = arena_d[out_off:out_off + B * Ho * Wo * Cc * 4].cpu().view(torch.float16).view(B, Ho, Wo, 2, Cc)
        idx = win.view(B, Ho * Wo, Cc)
        fin = torch.isfinite(ref)
        for plane in (0, 1):
            want = torch.gather(pairs_in[:, :, plane], 1, idx).view(B, Ho, Wo, Cc)
            assert torch.equal(pairs_out[..., plane, :].view(torch.int16)[fin], want.view(torch.int16)[fin]), ("hi", "lo")[plane]


def test_maxpool_beyond_the_grid_cap():
    """More groups of eight channels than the 8192 x 256 threads grid_for launches: the second trip of maxpool_kernel's grid-stride loop,
    against torch's own fp16 max-pool on the device (exact, and not the code under test)."""
    B, H, W, Cc = P.POOL_OVER_THE_CAP
    Ho, Wo = P.conv_out(H), P.conv_out(W)
    in_bytes, out_bytes = B * H * W * Cc * 2, B * Ho * Wo * Cc * 2
    (in_off, out_off), total = arena_offsets([in_bytes, out_bytes], [guard_bytes(Cc * 2, W), guard_bytes(Cc * 2, Wo)])
    x = torch.randn(B, H, W, Cc, device=DEV, generator=torch.Generator(DEV).manual_seed(6)).half()

    def arena_for(fill):                       # (built on the device: 138 MB of input)
        a = torch.full((total,), fill, dtype=torch.uint8, device=DEV)
        a[in_off:in_off + in_bytes].view(torch.float16).copy_(x.view(-1))
        return a
    (arena_d, _), _ = run_filled(P.maxpool_op(B, H, W, Cc, False, in_off, out_off), 1, arena_for, lambda fill: torch.full((256,), fill, dtype=torch.uint8),
                                 [ZERO_PAGE_RANGE, (out_off, out_off + out_bytes)], [("in", in_off, in_off + in_bytes), ("out", out_off, out_off + out_bytes)])
    got = arena_d[out_off:out_off + out_bytes].view(torch.float16).view(B, Ho, Wo, Cc)
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(got, want)


# ----------------------------------------------------------------------------------------------------------- bilinear add
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", P.UPADD_SHAPES + [P.UPADD_OVER_THE_CAP], ids=["%dx%dx%dx%d<-%dx%d" % s for s in P.UPADD_SHAPES] + ["over the grid cap"])
def test_upadd_vs_float64(shape, relu):
    """SMAP_OP_UPADD against relu(a + the bilinear map of t) with lerp_index's float32 taps (plan_ops.lerp_taps, anchored to torch in
    test_plan_ops_cpu.py) evaluated in float64, per element within 2^-11 |ref| + 2^-24 + 8 * 2^-24 (|a| + sum of weight * |tap|) + the
    weights' slack: odd ratios, x2, equal sizes (identity), a 1 x 1 source, output extents of 1, and the second trip of the grid-stride
    loop.  (Without the slack term -- plan_ops.lerp_slack: `scale * dst - i0` is one fma on the device, its product unrounded -- the
    device is at up to 15.6 times the first three terms where (in - 1) / (out - 1) is inexact, 65 -> 130; with it, at 0.998.)"""
    B, Ho, Wo, Cc, h, w = shape
    g = torch.Generator().manual_seed(7)
    a, t = torch.randn(B, Ho, Wo, Cc, generator=g).half(), torch.randn(B, h, w, Cc, generator=g).half()
    launch = FilledLaunch([("a", a, Cc * 2, Wo), ("t", t, Cc * 2, w)], [("out", a.numel() * 2, Cc * 2, Wo)])
    a_off, t_off, out_off = launch.offs
    arena_d = launch.run(P.upadd_op(B, Ho, Wo, Cc, h, w, relu, a_off, t_off, out_off))          # (the operands and the guards are as they were)
    got = read_act(arena_d, out_off, (B, Ho, Wo, Cc), to=torch.float64)
    ref, mag, slack = P.upadd_reference(a, t, relu)
    assert bool((a.double() + P.bilinear(t.double(), Ho, Wo) < 0).any())          # negative sums are present
    assert report("upadd", (got - ref).abs(), P.upadd_bound(ref, mag, slack)) <= 1.0
    assert bool((got >= 0).all()) == bool(relu)


# --------------------------------------------------------------------------------------------------------------- head sum
HEAD_RUNS = [(i, False, min(15, c[3]), scale) for i, c in enumerate(P.HEAD_CASES) for scale in (False, True)] + \
            [(i, True, n_kpt, scale) for i in (0, 1) for n_kpt in (15, 0) for scale in (False, True)]


@pytest.mark.parametrize("run", HEAD_RUNS, ids=["case %d%s n_kpt %d%s" % (i, " flip" if f else "", k, " scaled" if s else "") for i, f, k, s in HEAD_RUNS])
def test_headsum_vs_float64(run):
    """SMAP_OP_HEADSUM against ((s0 + up(s1)) + up(s2)) with the float32 taps in float64 [merged with the mirrored frames b + B through a
    pair table that is no involution] [divided by 255 / 127], per element within 12 * 2^-24 * sum of |tap| * weight + the weights' slack
    (plan_ops.lerp_slack; without it the device is at up to 7.3 times the first term, with it at 0.70): one, two and three
    sources, the first one up-sampled, odd ratios, a second 32-pixel segment of one pixel, Cout = 1 and Cout = 48, and large finite
    garbage in the sources' padding channels Cout .. Cin - 1.  One source at the output's size, unmerged and unscaled, is a transposition:
    bit for bit.  Arena and output buffer [maps | status words | 64 words nobody owns] are poisoned: the status words end at 0 (smap_plan_run
    clears them), nothing behind them and nothing in the arena but the zero page is written."""
    i, flip, n_kpt, scale = run
    B, Ho, Wo, Cout, Cin, sizes = P.HEAD_CASES[i]
    g = torch.Generator().manual_seed(11 + i)
    frames = 2 * B if flip else B
    srcs = []
    for h, w in sizes:
        s = torch.randn(frames, h, w, Cin, generator=g) * 50
        s[..., Cout:] = 1e30 * torch.sign(torch.randn(frames, h, w, Cin - Cout, generator=g))
        srcs.append(s)
    pair = P.odd_pair_table(Cout) if flip else None
    launch = FilledLaunch([("source %d" % k, s, Cin * 4, s.shape[2]) for k, s in enumerate(srcs)], [],
                          [torch.tensor(pair if flip else [0], dtype=torch.int32)], blob_guard=256)
    n_map, n_status = B * Cout * Ho * Wo, (B + 30) // 31
    op = P.headsum_op(B, Ho, Wo, Cout, Cin, sizes, launch.offs, 0, 4 * n_map, flip, n_kpt, launch.woffs[0], scale)
    launch.run(op, out_for=lambda fill: torch.full((4 * (n_map + n_status + 64),), fill, dtype=torch.uint8).view(torch.float32),
               out_written=[(0, 4 * (n_map + n_status))])
    out = launch.outs[0]
    got = out[:n_map].cpu().view(B, Cout, Ho, Wo)
    ref, mag, slack = P.headsum_reference(srcs, Ho, Wo, Cout, B, flip, pair, n_kpt, scale)
    assert report("headsum", (got.double() - ref).abs(), P.headsum_bound(mag, slack).clamp_min(1e-300)) <= 1.0
    if len(sizes) == 1 and not flip and not scale:
        assert sizes[0] == (Ho, Wo) and torch.equal(got, srcs[0][..., :Cout].permute(0, 3, 1, 2))
    assert not bool(out[n_map:n_map + n_status].view(torch.int32).any())
