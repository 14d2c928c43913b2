"""The trunk of one Upsample_unit in fp32, forward and backward, for training the last stage's decoder on a frozen ResNet
(reference: model/smap.py:210-217, out = relu(u_skip(x) + up_conv(interpolate(out_prev))); csrc/trunk.hip).

With BN in eval mode and folded by heads.fold_bn a trunk is  O = relu(X Wu^T + I(O_prev Wc^T) + b),  b = bu + bc, I the bilinear
align_corners interpolation to the unit's resolution.  `forward` / `backward` are the two C calls on raw tensors; `UnitTrunk` is the
pair as one autograd.Function, so that fold_bn carries the gradients on to conv.weight, conv.bias, bn.weight and bn.bias of u_skip and
up_conv, and O_prev's gradient on to the coarser unit.  No CPU path and no fallback: the tensors live on the GPU.

X and O_prev are [B, h, w, C] tensors in any layout heads.x_descriptor reads; O is dense fp32 [B, h, w, chl].
"""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import heads as H
from . import lib as L


def workspace_layout(B, h, w, hp, wp, cin, chl, backward):
    """Offsets in floats (csrc/trunk.hip layout_of): forward S [P][chl] | U [P'][chl]; backward gPre | gU | part | colpart | colsum.
    hp = wp = 0: no up path, P' = 0."""
    P, Pl = B * h * w, B * hp * wp
    n, nl = -(-P // H.slice_len(P)), (-(-Pl // H.slice_len(Pl)) if Pl else 0)
    lay = {"P": P, "Pl": Pl, "slices": n, "slices_lo": nl, "s": 0}
    at = H._round64(P * chl)
    lay["u"] = at
    at += H._round64(Pl * chl)
    if backward:
        lay["part"] = at
        at += H._round64(max(n * chl * cin, nl * chl * chl))
        lay["colpart"] = at
        at += H._round64(max(n, nl) * chl)
        lay["colsum"] = at
        at += H._round64(chl)
    lay["floats"] = at
    return lay


def workspace_bytes(B, h, w, hp, wp, cin, chl, backward):
    n = L.load().smap_trunk_ws_bytes(B, h, w, hp, wp, cin, chl, int(backward))
    if n < 0:
        raise L.SmapError("smap_trunk_ws_bytes: argument error (B %d, %d x %d from %d x %d, cin %d, chl %d)" % (B, h, w, hp, wp, cin, chl))
    return n


def new_workspace(B, h, w, hp, wp, cin, chl, backward, device):
    return torch.empty((workspace_bytes(B, h, w, hp, wp, cin, chl, backward),), dtype=torch.uint8, device=device)


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
    xd, B, h, w, cin = H.x_descriptor(x)
    chl = wu.shape[0]
    H._dense_fp32(wu, (chl, cin), "wu")
    pd, hp, wp = None, 0, 0
    if o_prev is not None:
        pd, Bp, hp, wp, cp = H.x_descriptor(o_prev)
        if Bp != B or cp != chl:
            raise ValueError("O_prev %s does not go with X %s and chl %d" % (tuple(o_prev.shape), tuple(x.shape), chl))
        H._dense_fp32(wc, (chl, chl), "wc")
    elif wc is not None:
        raise ValueError("wc without O_prev: the coarsest unit has no up_conv")
    return xd, pd, (B, h, w, hp, wp, cin, chl)


def forward(x, o_prev, wu, wc, b, ws=None):
    """smap_trunk_forward on the current stream.  Returns (O [B, h, w, chl] fp32, ws); S and U lie in ws where there is an up path."""
    xd, pd, dims = _operands(x, o_prev, wu, wc)
    B, h, w, hp, wp, cin, chl = dims
    H._dense_fp32(b, (chl,), "b")
    up = pd is not None
    dev = x.device
    if ws is None:
        ws = new_workspace(*dims, False, dev)
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
    H._dense_fp32(o, (B, h, w, chl), "o")
    H._dense_fp32(g_o, (B, h, w, chl), "g_o")
    up = pd is not None
    dev = x.device
    if ws is None:
        ws = new_workspace(*dims, True, dev)
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


def trunk_prefixes(unit, ind):
    """The module prefixes of a unit's trunk convs: u_skip, and up_conv from the second unit on."""
    return [unit + ".u_skip"] + ([unit + ".up_conv"] if ind > 0 else [])


def folded_trunk_weights(params, unit, ind, eps=1e-5):
    """wu [chl, cin], wc [chl, chl] or None, b = bu + bc of Upsample_unit `unit` from `params` (state_dict keys -> fp32 tensors), folded
    with heads.fold_bn.  The one sum b is what gives both biases the same gradient tensor."""
    def one(p):
        w, b = H.fold_bn(params[p + ".conv.weight"], params.get(p + ".conv.bias"), params[p + ".bn.weight"], params[p + ".bn.bias"],
                         params[p + ".bn.running_mean"], params[p + ".bn.running_var"], eps)
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


def trunk_parameter_keys(stage):
    """The 28 state_dict keys of the trunks of `stage`'s four units: u_skip x 4 and up_conv x 3, times the four trained kinds."""
    return ["%s.%s" % (m, k) for ind in range(4) for m in trunk_prefixes(H.unit_name(stage, ind), ind) for k in H.TRAINED]


def decoder_parameter_keys(stage_num):
    """What decoder training changes: the head parameters of every stage (288 keys at three stages) and the 28 trunk parameters of the
    LAST stage.  The last stage has neither skips nor cross_conv, so its `out` tensors feed its heads and the next finer unit alone and
    these gradients are exact; the trunks of the stages before it also feed the next stage's ResNet, whose backward pass is not here."""
    return H.head_parameter_keys(stage_num) + trunk_parameter_keys(stage_num - 1)


def decoder_loss(model, leaves, frozen, imgs, valids, labels, rdepth, sinks=None):
    """The training loss of the network as a function of `leaves` (decoder_parameter_keys), the ResNets frozen: ONE engine forward
    (all heads, the units' out and input tensors kept); the heads of stages 0 .. n - 2 in fp32 on the engine's `out`, exactly as
    heads.heads_loss runs them; for the last stage a UnitTrunk chain up1 -> up4 in fp32 from the engine's frozen x4 .. x1, its heads on
    that fp32 O; SMAPLossNative.  The engine is built once: the trunk's weights move, the engine's inputs to it do not.
    sinks: None, or a dict that receives {unit: {"gx": gradient at the last stage's input of that unit}} during backward().  Returns the
    loss dict (total_loss carries the graph)."""
    H.check_trainable(model, imgs, "decoder")
    B, _, Hh, W = imgs.shape
    eng = model.engine(B, Hh, W, imgs.device, all_heads=True, keep_unit_out=True, keep_unit_in=True)
    eng.run(imgs.float(), out=eng.new_output())
    outs, ins = eng.unit_out_sources(), eng.unit_in_sources()
    params = {**frozen, **leaves}
    last = model.stage_num - 1
    chain = []                                   # the last stage's fp32 O, coarsest first

    def unit_x(s, ind):
        if s != last:
            return outs[(s, ind)]
        assert ind == len(chain)                 # schedule order: up1 .. up4
        sink = None if sinks is None else sinks.setdefault(ind, {})
        chain.append(unit_trunk(ins[(s, ind)], chain[-1] if chain else None, params, H.unit_name(s, ind), ind, sink=sink))
        return chain[-1]
    return H.units_loss(model, params, unit_x, valids, labels, rdepth)


def decoder_parameter_gradients(model, imgs, valids, labels, rdepth):
    """(losses, {state_dict key: gradient of total_loss} for the 316 decoder parameters, [the gradients at the last stage's x4, x3, x2,
    x1, [B, h, w, Cin] fp32]).  The last is the seam a backward pass through the last ResNet would start from: nothing here consumes it."""
    leaves, frozen = H.parameter_leaves(model, decoder_parameter_keys(model.stage_num), imgs.device)
    sinks = {}
    losses = decoder_loss(model, leaves, frozen, imgs, valids, labels, rdepth, sinks)
    losses["total_loss"].backward()
    return ({k: v.detach() for k, v in losses.items()}, {k: v.grad for k, v in leaves.items()}, [sinks[ind]["gx"] for ind in range(4)])


class DecoderFineTuner(H.FrozenBackboneTuner):
    """Adam on the whole decoder of the LAST stage -- its four trunks (u_skip, up_conv) and its heads -- and on the heads of the stages
    before it, the ResNets frozen.  HeadFineTuner's contract over decoder_parameter_keys: the same reference Adam built from
    cfg.SOLVER, loss / step / commit, the engine built once and never between steps (the trunk runs forward in fp32 from the engine's
    frozen x4 .. x1; UnitTrunk), commit() writing the leaves back and invalidating the model's engines once.

        tuner = DecoderFineTuner(model.eval(), cfg, lr=1e-4, weight_decay=0.0)
        for imgs, valids, labels, rdepth in batches:
            losses = tuner.step(imgs, valids, labels, rdepth)
        tuner.commit()"""

    def __init__(self, model, cfg, lr=None, weight_decay=None, num_gpu=1, device=None):
        super().__init__(model, cfg, decoder_parameter_keys(model.stage_num), decoder_loss, lr, weight_decay, num_gpu, device)
