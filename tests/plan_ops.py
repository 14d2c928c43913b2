"""What test_plan_ops_gpu.py and test_plan_ops_cpu.py share about the five non-conv ops of csrc/plan.hip (STEM, STEMPOOL, MAXPOOL, UPADD,
HEADSUM): the shapes, one hand-made smap_op per kind, and the float64 references on the CPU.  Nothing here touches the GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from single_op import arena_offsets, guard_bytes

OP_STEM, OP_MAXPOOL, OP_UPADD, OP_HEADSUM, OP_STEMPOOL = 1, 2, 3, 4, 5      # include/smap_hip.h smap_op_kind

# ---------------------------------------------------------------------------------------------------------------- shapes
STEM_SHAPES = [(1, 37, 61), (2, 32, 70), (1, 7, 9), (1, 1, 1), (1, 33, 32)]                              # B, H, W
STEM_FLIP = (2, 37, 61, 1)                                                                                # B, H, W, flip_from
POOL_SHAPES = [(2, 19, 31, 64), (1, 1, 1, 8), (1, 2, 3, 8), (3, 16, 24, 72)]                              # B, H, W, C
POOL_OVER_THE_CAP = (1, 184, 184, 2048)        # 92 * 92 * 256 = 2 166 784 groups of eight channels > 8192 workgroups of 256
UPADD_SHAPES = [(2, 13, 21, 64, 7, 11), (1, 16, 24, 256, 8, 12), (1, 16, 24, 8, 16, 24), (1, 9, 9, 16, 1, 1), (1, 1, 5, 8, 3, 2),
                (1, 5, 1, 8, 2, 3)]                                                                       # B, Ho, Wo, C, h, w
UPADD_OVER_THE_CAP = (1, 130, 130, 1024, 65, 65)       # 130 * 130 * 128 = 2 163 200
HEAD_CASES = [      # B, Ho, Wo, Cout, Cin, sources (h, w)
    (2, 16, 24, 43, 48, [(16, 24), (8, 12), (4, 6)]),
    (1, 13, 33, 43, 48, [(13, 33), (7, 17), (4, 9)]),
    (1, 5, 70, 14, 16, [(5, 70)]),
    (2, 9, 31, 1, 8, [(9, 31)]),
    (1, 16, 40, 43, 48, [(16, 40), (8, 20)]),
    (1, 8, 32, 48, 48, [(4, 16), (8, 32), (2, 8)]),
]
GRID_CAP_ITEMS = 8192 * 256     # work items one trip of a grid-stride loop covers (grid_for, csrc/plan.hip)


def conv_out(n):
    """Output extent of the 7x7 s2 p3 conv -- and of the 3x3 s2 p1 pool."""
    return (n - 1) // 2 + 1


# ---------------------------------------------------------------------------------------------------------------- ops
def _op(kind, B, H, W, Cin, Ho, Wo, Cout):
    from smap_amd import lib as L
    o = L.SmapOp()
    o.kind, o.B, o.H, o.W, o.Cin, o.Ho, o.Wo, o.Cout = kind, B, H, W, Cin, Ho, Wo, Cout
    o.res_off = o.add1_off = o.add2_off = o.ext_off = -1
    for k in range(3):
        o.aux_off[k] = -1
    return o


def stem_op(B, H, W, x3, out_off, w_off, bias_off, acc_scale=1.0, flip_from=0, pool=False):
    Ho, Wo = conv_out(H), conv_out(W)
    if pool:
        Ho, Wo = conv_out(Ho), conv_out(Wo)
    o = _op(OP_STEMPOOL if pool else OP_STEM, B, H, W, 3, Ho, Wo, 64)
    o.ksize, o.stride, o.pad, o.relu = 7, 2, 3, 1
    o.out_off, o.w_off, o.bias_off, o.precision, o.acc_scale, o.flip_from = out_off, w_off, bias_off, int(x3), acc_scale, flip_from
    return o


def maxpool_op(B, H, W, Cc, x3, in_off, out_off):
    o = _op(OP_MAXPOOL, B, H, W, Cc, conv_out(H), conv_out(W), Cc)
    o.ksize, o.stride, o.pad = 3, 2, 1
    o.in_off, o.out_off, o.precision = in_off, out_off, int(x3)
    return o


def upadd_op(B, Ho, Wo, Cc, h, w, relu, a_off, t_off, out_off):
    o = _op(OP_UPADD, B, Ho, Wo, Cc, Ho, Wo, Cc)
    o.relu, o.in_off, o.out_off = int(relu), a_off, out_off
    o.aux_off[0], o.aux_h[0], o.aux_w[0] = t_off, h, w
    return o


def headsum_op(B, Ho, Wo, Cout, Cin, srcs, src_offs, ext_off, status_off, flip=False, n_kpt=0, pair_off=0, scale=False):
    """B OUTPUT frames; with flip the sources hold 2 B and flip_from = B."""
    o = _op(OP_HEADSUM, B, srcs[0][0], srcs[0][1], Cin, Ho, Wo, Cout)
    o.n_aux = len(srcs)
    for k, ((h, w), off) in enumerate(zip(srcs, src_offs)):
        o.aux_off[k], o.aux_h[k], o.aux_w[k] = off, h, w
    o.ext_off, o.status_off, o.scale_hms = ext_off, status_off, int(scale)
    if flip:
        o.flip_from, o.w_off = B, pair_off
    if flip or scale:
        o.in_c_off = n_kpt
    return o


# Each kind's arena: its tensors one behind the other, the output last, each between two guards of its own pixel stride
# (single_op.arena_offsets, guard_bytes) -> (byte sizes, bytes per pixel, pixels per row), one entry per tensor.
def stem_sizes(B, H, W, x3, pool=False):
    Ho, Wo = conv_out(H), conv_out(W)
    if pool:
        Ho, Wo = conv_out(Ho), conv_out(Wo)
    return [B * Ho * Wo * 64 * 2 * (1 + x3)], [64 * 2 * (1 + x3)], [Wo]


def maxpool_sizes(B, H, W, Cc, x3):
    pix = Cc * 2 * (1 + x3)
    return [B * H * W * pix, B * conv_out(H) * conv_out(W) * pix], [pix, pix], [W, conv_out(W)]


def upadd_sizes(B, Ho, Wo, Cc, h, w):
    return [B * Ho * Wo * Cc * 2, B * h * w * Cc * 2, B * Ho * Wo * Cc * 2], [Cc * 2] * 3, [Wo, w, Wo]


def headsum_sizes(B, Cin, srcs, flip=False):
    return [(2 if flip else 1) * B * h * w * Cin * 4 for h, w in srcs], [Cin * 4] * len(srcs), [w for _, w in srcs]


def laid_out(sizes, pix, rows):
    """The arena offsets of one kind's tensors, as the GPU tests lay them out."""
    return arena_offsets(sizes, [guard_bytes(p, w) for p, w in zip(pix, rows)])[0]


def laid_out_stem(B, H, W, x3, flip_from=0, pool=False):
    offs = laid_out(*stem_sizes(B, H, W, x3, pool))
    return stem_op(B, H, W, x3, offs[0], 0, 64 * 176 * 2 * (1 + x3), 1.0, flip_from, pool)      # (the bias behind the weights: a multiple of 256)


def laid_out_maxpool(B, H, W, Cc, x3):
    offs = laid_out(*maxpool_sizes(B, H, W, Cc, x3))
    return maxpool_op(B, H, W, Cc, x3, offs[0], offs[1])


def laid_out_upadd(B, Ho, Wo, Cc, h, w, relu=1):
    offs = laid_out(*upadd_sizes(B, Ho, Wo, Cc, h, w))
    return upadd_op(B, Ho, Wo, Cc, h, w, relu, offs[0], offs[1], offs[2])


def laid_out_headsum(B, Ho, Wo, Cout, Cin, srcs, flip=False, n_kpt=0, scale=False):
    offs = laid_out(*headsum_sizes(B, Cin, srcs, flip))
    return headsum_op(B, Ho, Wo, Cout, Cin, srcs, offs, 0, B * Cout * Ho * Wo * 4, flip, n_kpt, 0, scale)


# ---------------------------------------------------------------------------------------------------------------- references
def as_stored(v, planes):
    """fp32 values -> what their storage holds, in float64: fp16(v), or hi + lo of split precision."""
    hi = v.to(torch.float16)
    return hi.double() if planes == 1 else hi.double() + (v - hi.float()).to(torch.float16).double()


def stem_weights_as_stored(w, x3):
    """The stem's f64 weights as the kernel multiplies them: fp16(w), or (hi + lo) * 2^-s of split precision."""
    from smap_amd.engine import split_f16
    if not x3:
        return w.to(torch.float16).double()
    hi, lo, scale = split_f16(w)
    return (hi.double() + lo.double()) * scale


def stem_reference(x, w, bias, x3, flip_from=0):
    """x fp32 [frames, 3, H, W] (frames = flip_from when > 0) -> relu(conv 7x7 s2 p3 + bias) of the stored operands, f64 NHWC
    [B, Ho, Wo, 64]; with flip_from the second half of the batch is the stem of the mirrored images."""
    xs = as_stored(x, 1 + x3)
    if flip_from:
        xs = torch.cat([xs, torch.flip(xs, [-1])])
    y = F.conv2d(xs, stem_weights_as_stored(w, x3), bias.double(), stride=2, padding=3)
    return F.relu(y).permute(0, 2, 3, 1).contiguous()


def maxpool_reference(v, return_indices=False):
    """f64 NHWC -> MaxPool2d(3, 2, 1) of it, NHWC [, the winners' flat pixel indices y * W + x, NHWC]."""
    r = F.max_pool2d(v.permute(0, 3, 1, 2), 3, 2, 1, return_indices=return_indices)
    if not return_indices:
        return r.permute(0, 2, 3, 1).contiguous()
    return r[0].permute(0, 2, 3, 1).contiguous(), r[1].permute(0, 2, 3, 1).contiguous()


def _lerp_src(in_size, out_size):
    scale = np.float32(in_size - 1) / np.float32(out_size - 1) if out_size > 1 else np.float32(0)
    return (scale * np.arange(out_size, dtype=np.int64).astype(np.float32)).astype(np.float32)


def lerp_taps(in_size, out_size):
    """lerp_index of csrc/plan.h for every dst in 0 .. out_size - 1, in numpy float32 -> (i0, i1 int64; l0, l1 float32)."""
    dst = np.arange(out_size, dtype=np.int64)
    if in_size == out_size:
        return dst, dst.copy(), np.ones(out_size, np.float32), np.zeros(out_size, np.float32)
    src = _lerp_src(in_size, out_size)
    i0 = src.astype(np.int64)                                      # (int)src: truncation, src >= 0
    i1 = i0 + (i0 < in_size - 1)
    l1 = np.clip((src - i0.astype(np.float32)).astype(np.float32), np.float32(0), np.float32(1))
    return i0, i1, (np.float32(1) - l1).astype(np.float32), l1


def lerp_slack(in_size, out_size):
    """How far the device's l1 (and l0) may lie from lerp_taps', per dst, float64.  `src - (float)i0` with src = scale * (float)dst is one
    fused multiply-add where the compiler contracts it: the product then enters unrounded, half an ulp of src away from the float32 src the
    restatement subtracts from (both are lerp_index; which one a kernel holds is the compiler's choice per inlined copy).  l0 = 1 - l1 moves
    by the same amount and one rounding of its own (2^-24).  Equal sizes: the weights are the constants 1 and 0."""
    if in_size == out_size:
        return np.zeros(out_size)
    return np.spacing(_lerp_src(in_size, out_size)).astype(np.float64) / 2 + 2.0 ** -24


def _interp(v, ty, tx):
    """wy0 (wx0 v00 + wx1 v01) + wy1 (wx0 v10 + wx1 v11) of f64 NHWC v for taps (i0, i1, w0, w1) per output row / column, in float64."""
    (y0, y1, wy0, wy1), (x0, x1, wx0, wx1) = ty, tx
    cy = lambda l: torch.from_numpy(np.asarray(l, dtype=np.float64)).view(1, -1, 1, 1)
    cx = lambda l: torch.from_numpy(np.asarray(l, dtype=np.float64)).view(1, 1, -1, 1)
    row = lambda r: cx(wx0) * r[:, :, x0] + cx(wx1) * r[:, :, x1]
    return cy(wy0) * row(v[:, y0]) + cy(wy1) * row(v[:, y1])


def bilinear(v, Ho, Wo, taps=lerp_taps):
    """f64 NHWC [B, h, w, C] -> ly0 (lx0 v00 + lx1 v01) + ly1 (lx0 v10 + lx1 v11) at [B, Ho, Wo, C] with the float32 weights of `taps`,
    evaluated in float64."""
    return _interp(v, taps(v.shape[1], Ho), taps(v.shape[2], Wo))


def bilinear_slack(av, Ho, Wo):
    """What lerp_slack of the weights is worth in the interpolated value, from av = |v|: the row weights moved by dy against the
    column-interpolated rows, plus the column weights moved by dx inside each row."""
    ty, tx = lerp_taps(av.shape[1], Ho), lerp_taps(av.shape[2], Wo)
    dy, dx = lerp_slack(av.shape[1], Ho), lerp_slack(av.shape[2], Wo)
    return _interp(av, (ty[0], ty[1], dy, dy), tx) + _interp(av, ty, (tx[0], tx[1], dx, dx))


def upadd_reference(a, t, relu):
    """fp16 NHWC a [B, Ho, Wo, C], t [B, h, w, C] -> (relu(a + up(t)) in f64, |a| + sum of weight * |tap|, the slack of the weights)."""
    a, t = a.double(), t.double()
    ref = a + bilinear(t, a.shape[1], a.shape[2])
    return (F.relu(ref) if relu else ref), a.abs() + bilinear(t.abs(), a.shape[1], a.shape[2]), bilinear_slack(t.abs(), a.shape[1], a.shape[2])


def upadd_bound(ref, mag, slack):
    """One fp16 rounding of the result, the fp16 subnormal floor, eight fp32 roundings of the expression the kernel evaluates -- and the
    weights' own slack (lerp_slack), which the first three do not count."""
    return 2.0 ** -11 * ref.abs() + 2.0 ** -24 + 8 * 2.0 ** -24 * mag + slack


def headsum_reference(srcs, Ho, Wo, Cout, B, flip=False, pair=None, n_kpt=0, scale=False):
    """fp32 NHWC sources [frames, h, w, Cin] -> (((s0 + up(s1)) + up(s2)) [merged with the mirrored frames] [scaled], f64 NCHW
    [B, Cout, Ho, Wo]; the sum of |tap| * its weight over the taps that enter each value; the slack of the weights, carried the same way)."""
    val = mag = slack = None
    for s in srcs:
        s = s[..., :Cout].double()
        u, m, e = bilinear(s, Ho, Wo), bilinear(s.abs(), Ho, Wo), bilinear_slack(s.abs(), Ho, Wo)
        val, mag, slack = (u, m, e) if val is None else (val + u, mag + m, slack + e)
    val, mag, slack = val.permute(0, 3, 1, 2), mag.permute(0, 3, 1, 2), slack.permute(0, 3, 1, 2)
    if flip:
        pair = torch.as_tensor(pair, dtype=torch.long)
        sign = torch.tensor([-1.0 if c >= n_kpt and (c - n_kpt) % 2 == 0 else 1.0 for c in range(Cout)], dtype=torch.float64).view(1, -1, 1, 1)
        half = torch.tensor([0.5 if c >= n_kpt else 1.0 for c in range(Cout)], dtype=torch.float64).view(1, -1, 1, 1)
        val = (val[:B] + sign * val[B:, pair].flip(-1)) * half
        mag = (mag[:B] + mag[B:, pair].flip(-1)) * half
        slack = (slack[:B] + slack[B:, pair].flip(-1)) * half
    if scale:
        div = torch.tensor([255.0 if c < n_kpt else 127.0 for c in range(Cout)], dtype=torch.float64).view(1, -1, 1, 1)
        val, mag, slack = val / div, mag / div, slack / div
    return val.contiguous(), mag.contiguous(), slack.contiguous()


def headsum_bound(mag, slack):
    """Twelve fp32 roundings of the sum the kernel evaluates, and the weights' own slack (lerp_slack)."""
    return 12 * 2.0 ** -24 * mag + slack


def odd_pair_table(n):
    """A permutation of n channels that is not an involution (a pair[c] read on the wrong side shows)."""
    pair = np.random.default_rng(4).permutation(n).tolist()
    assert any(pair[pair[c]] != c for c in range(n)) and sorted(pair) == list(range(n))
    return pair
