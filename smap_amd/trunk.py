"""The trunk of one Upsample_unit in fp32, forward and backward, for training the last stage's decoder on a frozen ResNet
(reference: model/smap.py:210-217, out = relu(u_skip(x) + up_conv(interpolate(out_prev))); csrc/trunk.hip).

With BN in eval mode and folded by gemm_f32.fold_bn a trunk is  O = relu(X Wu^T + I(O_prev Wc^T) + b),  b = bu + bc, I the bilinear
align_corners interpolation to the unit's resolution.  `forward` / `backward` are the two C calls on raw tensors; `UnitTrunk` is the
pair as one autograd.Function, so that fold_bn carries the gradients on to conv.weight, conv.bias, bn.weight and bn.bias of u_skip and
up_conv, and O_prev's gradient on to the coarser unit.  No CPU path and no fallback: the tensors live on the GPU.

X and O_prev are [B, h, w, C] tensors in any layout gemm_f32.x_descriptor reads; O is dense fp32 [B, h, w, chl].
Training the trunk's parameters (the keys, the decoder loss, the tuner) is smap_amd/finetune.py.
"""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import gemm_f32 as G
from . import lib as L


def workspace_layout(B, h, w, hp, wp, cin, chl, backward):
    """Offsets in floats (csrc/trunk.hip layout_of): forward S [P][chl] | U [P'][chl]; backward gPre | gU | part | colpart | colsum.
    hp = wp = 0: no up path, P' = 0."""
    P, Pl = B * h * w, B * hp * wp
    n, nl = G.slices(P), G.slices(Pl)
    lay = {"P": P, "Pl": Pl, "slices": n, "slices_lo": nl, "s": 0}
    at = G.round64(P * chl)
    lay["u"] = at
    at += G.round64(Pl * chl)
    if backward:
        lay["part"] = at
        at += G.round64(max(n * chl * cin, nl * chl * chl))
        lay["colpart"] = at
        at += G.round64(max(n, nl) * chl)
        lay["colsum"] = at
        at += G.round64(chl)
    lay["floats"] = at
    return lay


def workspace_bytes(B, h, w, hp, wp, cin, chl, backward):
    n = L.load().smap_trunk_ws_bytes(B, h, w, hp, wp, cin, chl, int(backward))
    if n < 0:
        raise L.SmapError("smap_trunk_ws_bytes: argument error (B %d, %d x %d from %d x %d, cin %d, chl %d)" % (B, h, w, hp, wp, cin, chl))
    return n


def workspace_views(ws, B, h, w, hp, wp, cin, chl, backward):
    """S and U (forward) or gPre and gU (backward) as [B, h, w, chl] and [B, hp, wp, chl] views of a workspace a call has filled."""
    lay = workspace_layout(B, h, w, hp, wp, cin, chl, backward)
    f = ws.view(torch.float32)
    names = ("gpre", "gu") if backward else ("s", "u")
    out = {names[0]: f[:lay["P"] * chl].view(B, h, w, chl)}
    if lay["Pl"]:
        out[names[1]] = f[lay["u"]:lay["u"] + lay["Pl"] * chl].view(B, hp, wp, chl)
    return out


def _operands(x, o_prev, wu, wc):
    xd, B, h, w, cin = G.x_descriptor(x)
    chl = wu.shape[0]
    G.dense_fp32(wu, (chl, cin), "wu")
    pd, hp, wp = None, 0, 0
    if o_prev is not None:
        pd, Bp, hp, wp, cp = G.x_descriptor(o_prev)
        if Bp != B or cp != chl:
            raise ValueError("O_prev %s does not go with X %s and chl %d" % (tuple(o_prev.shape), tuple(x.shape), chl))
        G.dense_fp32(wc, (chl, chl), "wc")
    elif wc is not None:
        raise ValueError("wc without O_prev: the coarsest unit has no up_conv")
    return xd, pd, (B, h, w, hp, wp, cin, chl)


def forward(x, o_prev, wu, wc, b, ws=None):
    """smap_trunk_forward on the current stream.  Returns (O [B, h, w, chl] fp32, ws); S and U lie in ws where there is an up path."""
    xd, pd, dims = _operands(x, o_prev, wu, wc)
    B, h, w, hp, wp, cin, chl = dims
    G.dense_fp32(b, (chl,), "b")
    up = pd is not None
    dev = x.device
    if ws is None:
        ws = G.new_workspace(workspace_bytes(*dims, False), dev)
    o = torch.empty((B, h, w, chl), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().smap_trunk_forward(C.byref(xd), C.byref(pd) if up else None, wu.data_ptr(), wc.data_ptr() if up else None, b.data_ptr(),
                                            o.data_ptr(), *dims, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream),
                "smap_trunk_forward")
    return o, ws


def backward(x, o_prev, o, wu, wc, g_o, want_gx=False, ws=None):
    """smap_trunk_backward on the current stream: the gradients of <G, O>.  Returns (gwu, gwc, gb, g_o_prev, gx, ws); gwc and g_o_prev are
    None without an up path, gx [B, h, w, cin] fp32 is None unless wanted.  gPre and gU lie in ws (workspace_views)."""
    xd, pd, dims = _operands(x, o_prev, wu, wc)
    B, h, w, hp, wp, cin, chl = dims
    G.dense_fp32(o, (B, h, w, chl), "o")
    G.dense_fp32(g_o, (B, h, w, chl), "g_o")
    up = pd is not None
    dev = x.device
    if ws is None:
        ws = G.new_workspace(workspace_bytes(*dims, True), dev)
    f32 = dict(dtype=torch.float32, device=dev)
    gwu, gb = torch.empty((chl, cin), **f32), torch.empty((chl,), **f32)
    gwc = torch.empty((chl, chl), **f32) if up else None
    gprev = torch.empty((B, hp, wp, chl), **f32) if up else None
    gx = torch.empty((B, h, w, cin), **f32) if want_gx else None
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        L.check(L.load().smap_trunk_backward(C.byref(xd), C.byref(pd) if up else None, o.data_ptr(), wu.data_ptr(), ptr(wc) if up else None,
                                             g_o.data_ptr(), gwu.data_ptr(), ptr(gwc), gb.data_ptr(), ptr(gprev), ptr(gx), cin, *dims,
                                             ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream), "smap_trunk_backward")
    return gwu, gwc, gb, gprev, gx, ws


class UnitTrunk(torch.autograd.Function):
    """O [B, h, w, chl] fp32 of X, O_prev (None for the coarsest unit) and the folded wu [chl, cin], wc [chl, chl] (None without O_prev),
    b [chl] = bu + bc.  Gradients: wu, wc, b, and O_prev where it is fp32; X is the frozen engine's and autograd gives it none.
    sink: None, or a dict -- the backward pass then also leaves the gradient at X there as sink["gx"] ([B, h, w, cin] fp32): the seam a
    downsample backward starts from."""

    @staticmethod
    def forward(ctx, x, o_prev, wu, wc, b, sink=None):
        ctx.sink, ctx.up = sink, o_prev is not None
        o, _ = forward(x, o_prev, wu, wc, b)
        ctx.save_for_backward(x, o, wu, *([o_prev, wc] if ctx.up else []))
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, o, wu, *rest = ctx.saved_tensors
        o_prev, wc = rest if ctx.up else (None, None)
        gwu, gwc, gb, gprev, gx, _ = backward(x, o_prev, o, wu, wc, g.contiguous(), want_gx=ctx.sink is not None)
        if ctx.sink is not None:
            ctx.sink["gx"] = gx
        to_prev = ctx.up and ctx.needs_input_grad[1] and o_prev.dtype == torch.float32
        return None, (gprev if to_prev else None), gwu, gwc, gb, None


def folded_trunk_weights(params, unit, ind, eps=1e-5):
    """wu [chl, cin], wc [chl, chl] or None, b = bu + bc of Upsample_unit `unit` from `params` (state_dict keys -> fp32 tensors), folded
    with gemm_f32.fold_bn.  The one sum b is what gives both biases the same gradient tensor."""
    def one(p):
        w, b = G.folded(params, p, eps)
        return w.flatten(1).contiguous(), b
    wu, b = one(unit + ".u_skip")
    wc = None
    if ind > 0:
        wc, bc = one(unit + ".up_conv")
        b = b + bc
    return wu, wc, b.contiguous()


def unit_trunk(x, o_prev, params, unit, ind, eps=1e-5, sink=None):
    """A unit's `out` from its input X, the coarser unit's out and the unfolded parameters: fold_bn, then UnitTrunk."""
    wu, wc, b = folded_trunk_weights(params, unit, ind, eps)
    return UnitTrunk.apply(x, o_prev, wu, wc, b, sink)
