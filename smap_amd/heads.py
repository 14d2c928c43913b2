"""The three head arms of one Upsample_unit in fp32, forward and backward, for training the heads on a frozen backbone
(reference: model/smap.py:190-229, res*_conv1 1x1 + BN + ReLU, res*_conv2 3x3 + BN; csrc/heads.hip).

With BN in eval mode an arm is  Y_a = conv3x3(relu(X W1_a^T + b1_a), W2_a) + b2_a  over the unit's `out` tensor X, with the folded
weights of gemm_f32.fold_bn.  `forward` / `backward` are the two C calls on raw tensors; `UnitHeads` is the pair as one autograd.Function, so
that fold_bn -- written in differentiable torch ops -- carries the gradients on to conv.weight, conv.bias, bn.weight and bn.bias,
the running statistics staying frozen.  The backward pass recomputes M = relu(Z) into its workspace (the reference's efficient=True
checkpointing) and is the exact gradient of the fp32 forward.  No CPU path and no fallback: the tensors live on the GPU.

X is a [B, h, w, chl] tensor (NHWC): fp32, fp16, or fp16 [B, h, w, 2, chl] hi|lo planes whose sum is the value.  A channel-padded
pixel is a view whose last stride is 1 (x[..., :chl] of a wider tensor).  Heads come and go as dense [B, C_a, h, w] in `UnitHeads`;
`forward` / `backward` take any HeadSource tuple (ptr, h, w, c, pix_stride, ch_stride, frame_stride), as smap_amd/loss.py does.
Training the arms' parameters (the keys, the losses, the tuners) is smap_amd/finetune.py.
"""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import lib as L
from .gemm_f32 import dense_fp32, folded, new_workspace, round64, slice_len, slices, x_descriptor

MAX_ARM_C = 64      # csrc/heads.hip


def workspace_layout(B, h, w, chl, backward):
    """Offsets in floats of M [P][3 chl], gZ [P][3 chl], part [slices][chl * max(3 chl, 576)], colpart [slices][3 chl] and the total
    (csrc/heads.hip layout_of); the forward pass has M alone."""
    P = B * h * w
    n = slices(P)
    lay = {"P": P, "slices": n, "slice_len": slice_len(P), "m": 0}
    at = round64(P * 3 * chl)
    if backward:
        lay["gz"] = at
        at += round64(P * 3 * chl)
        lay["part"] = at
        at += round64(n * chl * max(3 * chl, 9 * MAX_ARM_C))
        lay["colpart"] = at
        at += round64(n * 3 * chl)
    lay["floats"] = at
    return lay


def workspace_bytes(B, h, w, chl, backward):
    n = L.load().smap_heads_ws_bytes(B, h, w, chl, int(backward))
    if n < 0:
        raise L.SmapError("smap_heads_ws_bytes: argument error (B %d, %d x %d, chl %d)" % (B, h, w, chl))
    return n


def workspace_views(ws, B, h, w, chl, backward=True):
    """M and gZ as [B, h, w, 3, chl] views of a workspace a call has filled (arm a: [..., a, :])."""
    lay = workspace_layout(B, h, w, chl, backward)
    f = ws.view(torch.float32)
    n = lay["P"] * 3 * chl
    out = {"m": f[lay["m"]:lay["m"] + n].view(B, h, w, 3, chl)}
    if backward:
        out["gz"] = f[lay["gz"]:lay["gz"] + n].view(B, h, w, 3, chl)
    return out


def nchw_source(t):
    """HeadSource tuple of a dense [B, c, h, w] fp32 tensor."""
    _, c, h, w = t.shape
    return (t.data_ptr(), h, w, c, 1, h * w, c * h * w)


def _sources(srcs):
    arr = (L.HeadSrc * 3)()
    for a, (ptr, h, w, c, pix, ch, frame) in enumerate(srcs):
        arr[a] = L.HeadSrc(int(ptr) if ptr else None, int(h), int(w), int(c), int(pix), int(ch), 0, int(frame))
    return arr


def _ptrs(tensors):
    return (C.c_void_p * 3)(*[t.data_ptr() for t in tensors])


def _check_weights(chl, w1cat, b1cat, w2, b2, cs):
    dense_fp32(w1cat, (3 * chl, chl), "w1cat")
    dense_fp32(b1cat, (3 * chl,), "b1cat")
    for a in range(3):
        dense_fp32(w2[a], (cs[a], chl, 3, 3), "w2[%d]" % a)
        if b2 is not None:
            dense_fp32(b2[a], (cs[a],), "b2[%d]" % a)


def forward(x, w1cat, b1cat, w2, b2, y_sources, ws=None):
    """smap_heads_forward on the current stream: writes Y_a through the three HeadSource tuples `y_sources`; returns the workspace
    (M = relu(Z) lies in it, workspace_views)."""
    xd, B, h, w, chl = x_descriptor(x)
    _check_weights(chl, w1cat, b1cat, w2, b2, [s[3] for s in y_sources])
    dev = x.device
    if ws is None:
        ws = new_workspace(workspace_bytes(B, h, w, chl, False), dev)
    with torch.cuda.device(dev):
        L.check(L.load().smap_heads_forward(C.byref(xd), w1cat.data_ptr(), b1cat.data_ptr(), _ptrs(w2), _ptrs(b2), _sources(y_sources), B, h, w,
                                            chl, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream), "smap_heads_forward")
    return ws


def backward(x, w1cat, b1cat, w2, g_sources, want_gx=True, ws=None):
    """smap_heads_backward on the current stream: the gradients of sum_a <G_a, Y_a> at the folded weights and at X.  Returns
    (gw1cat, gb1cat, [gw2_a], [gb2_a], gx [B, h, w, chl] fp32 or None, ws); M and gZ lie in ws (workspace_views)."""
    xd, B, h, w, chl = x_descriptor(x)
    cs = [s[3] for s in g_sources]
    _check_weights(chl, w1cat, b1cat, w2, None, cs)
    dev = x.device
    if ws is None:
        ws = new_workspace(workspace_bytes(B, h, w, chl, True), dev)
    f32 = dict(dtype=torch.float32, device=dev)
    gw1, gb1 = torch.empty((3 * chl, chl), **f32), torch.empty((3 * chl,), **f32)
    gw2 = [torch.empty((c, chl, 3, 3), **f32) for c in cs]
    gb2 = [torch.empty((c,), **f32) for c in cs]
    gx = torch.empty((B, h, w, chl), **f32) if want_gx else None
    with torch.cuda.device(dev):
        L.check(L.load().smap_heads_backward(C.byref(xd), w1cat.data_ptr(), b1cat.data_ptr(), _ptrs(w2), _sources(g_sources), B, h, w, chl,
                                             gw1.data_ptr(), gb1.data_ptr(), _ptrs(gw2), _ptrs(gb2), gx.data_ptr() if want_gx else None, chl,
                                             ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream), "smap_heads_backward")
    return gw1, gb1, gw2, gb2, gx, ws


class UnitHeads(torch.autograd.Function):
    """(Y_0, Y_1, Y_2), dense [B, C_a, h, w] fp32, of X and the folded weights w1cat [3 chl, chl], b1cat [3 chl], w2_a [C_a, chl, 3, 3],
    b2_a [C_a].  Gradients: the folded weights, and X where it is fp32 (an fp16 X is the frozen engine's and autograd gives it none).
    sink: None, or a dict -- the backward pass then also leaves the gradient at X there as sink["gx"] ([B, h, w, chl] fp32), whatever
    X's layout: the seam a backward pass through the rest of the unit starts from -- and the upstream gradients it received as sink["g"]."""

    @staticmethod
    def forward(ctx, x, w1cat, b1cat, w2_0, b2_0, w2_1, b2_1, w2_2, b2_2, sink=None):
        ctx.sink = sink
        w2, b2 = [w2_0, w2_1, w2_2], [b2_0, b2_1, b2_2]
        B, h, w = x.shape[:3]
        ys = [torch.empty((B, t.shape[0], h, w), dtype=torch.float32, device=x.device) for t in w2]
        forward(x, w1cat, b1cat, w2, b2, [nchw_source(y) for y in ys])
        ctx.save_for_backward(x, w1cat, b1cat, *w2)
        return tuple(ys)

    @staticmethod
    @once_differentiable
    def backward(ctx, g0, g1, g2):
        x, w1cat, b1cat, *w2 = ctx.saved_tensors
        gs = [g.contiguous() for g in (g0, g1, g2)]
        to_x = ctx.needs_input_grad[0] and x.dtype == torch.float32
        gw1, gb1, gw2, gb2, gx, _ = backward(x, w1cat, b1cat, w2, [nchw_source(g) for g in gs], want_gx=to_x or ctx.sink is not None)
        if ctx.sink is not None:
            ctx.sink["gx"], ctx.sink["g"] = gx, gs
        return (gx if to_x else None), gw1, gb1, gw2[0], gb2[0], gw2[1], gb2[1], gw2[2], gb2[2], None


def folded_unit_weights(params, arms, eps=1e-5):
    """w1cat, b1cat, [w2_a], [b2_a] of the three (conv1, conv2) prefixes `arms` from `params` (state_dict keys -> fp32 tensors, leaves
    where a gradient is wanted), folded with gemm_f32.fold_bn."""
    w1, b1, w2, b2 = [], [], [], []
    for c1, c2 in arms:
        w, b = folded(params, c1, eps)
        w1.append(w.flatten(1))
        b1.append(b)
        w, b = folded(params, c2, eps)
        w2.append(w.contiguous())
        b2.append(b.contiguous())
    return torch.cat(w1).contiguous(), torch.cat(b1).contiguous(), w2, b2


def unit_heads(x, params, arms, eps=1e-5, sink=None):
    """The three head tensors of a unit from its `out` tensor X and the unfolded parameters: fold_bn, then UnitHeads."""
    w1cat, b1cat, w2, b2 = folded_unit_weights(params, arms, eps)
    return UnitHeads.apply(x, w1cat, b1cat, w2[0], b2[0], w2[1], b2[1], w2[2], b2[2], sink)
