"""The three head arms of one Upsample_unit in fp32, forward and backward, for training the heads on a frozen backbone
(reference: model/smap.py:190-229, res*_conv1 1x1 + BN + ReLU, res*_conv2 3x3 + BN; csrc/heads.hip).

With BN in eval mode an arm is  Y_a = conv3x3(relu(X W1_a^T + b1_a), W2_a) + b2_a  over the unit's `out` tensor X, with the folded
weights of `fold_bn`.  `forward` / `backward` are the two C calls on raw tensors; `UnitHeads` is the pair as one autograd.Function, so
that `fold_bn` -- written in differentiable torch ops -- carries the gradients on to conv.weight, conv.bias, bn.weight and bn.bias,
the running statistics staying frozen.  The backward pass recomputes M = relu(Z) into its workspace (the reference's efficient=True
checkpointing) and is the exact gradient of the fp32 forward.  No CPU path and no fallback: the tensors live on the GPU.

X is a [B, h, w, chl] tensor (NHWC): fp32, fp16, or fp16 [B, h, w, 2, chl] hi|lo planes whose sum is the value.  A channel-padded
pixel is a view whose last stride is 1 (x[..., :chl] of a wider tensor).  Heads come and go as dense [B, C_a, h, w] in `UnitHeads`;
`forward` / `backward` take any HeadSource tuple (ptr, h, w, c, pix_stride, ch_stride, frame_stride), as smap_amd/loss.py does.
"""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import lib as L

MAX_ARM_C, SLICE_MIN, SLICE_MAX_N, BK = 64, 256, 64, 16      # csrc/heads.hip


def _round64(n):
    return (n + 63) // 64 * 64


def slice_len(P):
    """Pixels per reduction slice (csrc/heads.hip slice_len_of)."""
    if P <= SLICE_MIN * SLICE_MAX_N:
        return SLICE_MIN
    per = (P + SLICE_MAX_N - 1) // SLICE_MAX_N
    return (per + BK - 1) // BK * BK


def workspace_layout(B, h, w, chl, backward):
    """Offsets in floats of M [P][3 chl], gZ [P][3 chl], part [slices][chl * max(3 chl, 576)], colpart [slices][3 chl] and the total
    (csrc/heads.hip layout_of); the forward pass has M alone."""
    P = B * h * w
    n = -(-P // slice_len(P))
    lay = {"P": P, "slices": n, "slice_len": slice_len(P), "m": 0}
    at = _round64(P * 3 * chl)
    if backward:
        lay["gz"] = at
        at += _round64(P * 3 * chl)
        lay["part"] = at
        at += _round64(n * chl * max(3 * chl, 9 * MAX_ARM_C))
        lay["colpart"] = at
        at += _round64(n * 3 * chl)
    lay["floats"] = at
    return lay


def workspace_bytes(B, h, w, chl, backward):
    n = L.load().smap_heads_ws_bytes(B, h, w, chl, int(backward))
    if n < 0:
        raise L.SmapError("smap_heads_ws_bytes: argument error (B %d, %d x %d, chl %d)" % (B, h, w, chl))
    return n


def new_workspace(B, h, w, chl, backward, device):
    """A workspace tensor (uint8; torch's allocator aligns it to 512 bytes)."""
    return torch.empty((workspace_bytes(B, h, w, chl, backward),), dtype=torch.uint8, device=device)


def workspace_views(ws, B, h, w, chl, backward=True):
    """M and gZ as [B, h, w, 3, chl] views of a workspace a call has filled (arm a: [..., a, :])."""
    lay = workspace_layout(B, h, w, chl, backward)
    f = ws.view(torch.float32)
    n = lay["P"] * 3 * chl
    out = {"m": f[lay["m"]:lay["m"] + n].view(B, h, w, 3, chl)}
    if backward:
        out["gz"] = f[lay["gz"]:lay["gz"] + n].view(B, h, w, 3, chl)
    return out


def x_descriptor(x):
    """(smap_heads_x, B, h, w, chl) of X: [B, h, w, chl] fp32 or fp16, or [B, h, w, 2, chl] fp16 hi|lo; frames and pixels back to back."""
    if not x.is_cuda:
        raise ValueError("X must live on the GPU")
    if x.dim() == 5 and x.dtype == torch.float16 and x.shape[3] == 2:
        B, h, w, _, chl = x.shape
        layout, pix = L.HEADS_X_F16_HILO, x.stride(2)
        ok = x.stride(4) == 1 and x.stride(3) == chl
    elif x.dim() == 4 and x.dtype in (torch.float32, torch.float16):
        B, h, w, chl = x.shape
        layout, pix = (L.HEADS_X_F32 if x.dtype == torch.float32 else L.HEADS_X_F16), x.stride(2)
        ok = x.stride(3) == 1
    else:
        raise ValueError("X: [B, h, w, chl] fp32 / fp16 or [B, h, w, 2, chl] fp16, not %s %s" % (tuple(x.shape), x.dtype))
    if not ok or x.stride(1) != w * pix or x.stride(0) != h * w * pix:
        raise ValueError("X: channels, pixels and frames must lie back to back (strides %s)" % (x.stride(),))
    return L.HeadsX(x.data_ptr(), layout, pix), B, h, w, chl


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


def _dense_fp32(t, shape, what):
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError("%s: dense fp32 %s expected, got %s %s" % (what, tuple(shape), tuple(t.shape), t.dtype))
    return t


def _check_weights(chl, w1cat, b1cat, w2, b2, cs):
    _dense_fp32(w1cat, (3 * chl, chl), "w1cat")
    _dense_fp32(b1cat, (3 * chl,), "b1cat")
    for a in range(3):
        _dense_fp32(w2[a], (cs[a], chl, 3, 3), "w2[%d]" % a)
        if b2 is not None:
            _dense_fp32(b2[a], (cs[a],), "b2[%d]" % a)


def forward(x, w1cat, b1cat, w2, b2, y_sources, ws=None):
    """smap_heads_forward on the current stream: writes Y_a through the three HeadSource tuples `y_sources`; returns the workspace
    (M = relu(Z) lies in it, workspace_views)."""
    xd, B, h, w, chl = x_descriptor(x)
    _check_weights(chl, w1cat, b1cat, w2, b2, [s[3] for s in y_sources])
    dev = x.device
    if ws is None:
        ws = new_workspace(B, h, w, chl, False, dev)
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
        ws = new_workspace(B, h, w, chl, True, dev)
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


def fold_bn(weight, bias, gamma, beta, mean, var, eps=1e-5):
    """Eval-mode BN folded into the conv before it: w' = w g / sqrt(var + eps), b' = (b - mean) g / sqrt(var + eps) + beta.  Plain
    differentiable torch ops: autograd carries d / d w' and d / d b' on to weight, bias (may be None), gamma and beta."""
    scale = gamma / torch.sqrt(var + eps)
    b = -mean if bias is None else bias - mean
    return weight * scale.view(-1, *([1] * (weight.dim() - 1))), b * scale + beta


ARMS = ("res", "res_d", "res_rd")          # heatmap_2d | det_d | root_d: <unit>.<arm>_conv1, <unit>.<arm>_conv2 (model/smap.py)


def arm_prefixes(unit):
    """The (conv1, conv2) module prefixes of the three arms of Upsample_unit `unit` (e.g. "stage0.upsample.up1")."""
    return [("%s.%s_conv1" % (unit, a), "%s.%s_conv2" % (unit, a)) for a in ARMS]


def folded_unit_weights(params, arms, eps=1e-5):
    """w1cat, b1cat, [w2_a], [b2_a] of the three (conv1, conv2) prefixes `arms` from `params` (state_dict keys -> fp32 tensors, leaves
    where a gradient is wanted), folded with fold_bn."""
    def one(p):
        return fold_bn(params[p + ".conv.weight"], params.get(p + ".conv.bias"), params[p + ".bn.weight"], params[p + ".bn.bias"],
                       params[p + ".bn.running_mean"], params[p + ".bn.running_var"], eps)
    w1, b1, w2, b2 = [], [], [], []
    for c1, c2 in arms:
        w, b = one(c1)
        w1.append(w.flatten(1))
        b1.append(b)
        w, b = one(c2)
        w2.append(w.contiguous())
        b2.append(b.contiguous())
    return torch.cat(w1).contiguous(), torch.cat(b1).contiguous(), w2, b2


def unit_heads(x, params, arms, eps=1e-5, sink=None):
    """The three head tensors of a unit from its `out` tensor X and the unfolded parameters: fold_bn, then UnitHeads."""
    w1cat, b1cat, w2, b2 = folded_unit_weights(params, arms, eps)
    return UnitHeads.apply(x, w1cat, b1cat, w2[0], b2[0], w2[1], b2[1], w2[2], b2[2], sink)


TRAINED = ("conv.weight", "conv.bias", "bn.weight", "bn.bias")
FROZEN = ("bn.running_mean", "bn.running_var")
HEAD_KEYS = ("heatmap_2d", "det_d", "root_d")


def unit_name(stage, ind):
    return "stage%d.upsample.up%d" % (stage, ind + 1)


def head_parameter_keys(stage_num):
    """The state_dict keys of what head training changes: conv.weight, conv.bias, bn.weight, bn.bias of the 6 head convs of each of
    the 4 * stage_num units (72 convs, 288 keys at three stages), in schedule order."""
    return ["%s.%s" % (m, k) for s in range(stage_num) for ind in range(4) for pair in arm_prefixes(unit_name(s, ind)) for m in pair for k in TRAINED]


def parameter_leaves(model, keys, device=None):
    """(leaves, frozen): fp32 copies of the model's parameters `keys` as autograd leaves, and of their BNs' running statistics."""
    sd = model.state_dict()
    mv = lambda t: t.detach().to(device=device or t.device, dtype=torch.float32).clone()
    leaves = {k: mv(sd[k]).requires_grad_(True) for k in keys}
    frozen = {k[:-len("conv.weight")] + f: mv(sd[k[:-len("conv.weight")] + f]) for k in keys if k.endswith("conv.weight") for f in FROZEN}
    return leaves, frozen


def head_leaves(model, device=None):
    """parameter_leaves of the model's head parameters."""
    return parameter_leaves(model, head_parameter_keys(model.stage_num), device)


def check_trainable(model, imgs, what):
    if model.training:
        raise RuntimeError("%s training runs on a frozen backbone with BatchNorm in eval mode: call model.eval() first" % what)
    if not imgs.is_cuda:
        raise NotImplementedError("%s training runs on a ROCm GPU only: images on %s, there is no CPU fallback" % (what, imgs.device))


def units_loss(model, params, unit_x, valids, labels, rdepth, sinks=None):
    """UnitHeads in fp32 on unit_x(stage, unit) -- each unit's `out` -- for all 4 * stage_num units in schedule order, then SMAPLossNative.
    sinks: None, or a dict that receives {(stage, unit): {"gx": gradient at out}} during backward().  Returns the loss dict."""
    from .loss import SMAPLossNative
    outputs = {k: [[None] * 4 for _ in range(model.stage_num)] for k in HEAD_KEYS}
    for s in range(model.stage_num):
        for ind in range(4):
            sink = None
            if sinks is not None:
                sink = sinks.setdefault((s, ind), {})
            ys = unit_heads(unit_x(s, ind), params, arm_prefixes(unit_name(s, ind)), sink=sink)
            for k, y in zip(HEAD_KEYS, ys):
                outputs[k][s][ind] = y
    crit = SMAPLossNative(model.stage_num, model.ohkm, model.topk, model.ctf)
    return crit(outputs, valids, labels, rdepth)


def heads_loss(model, leaves, frozen, imgs, valids, labels, rdepth, sinks=None):
    """The training loss of the network as a function of the head parameters `leaves`, the backbone frozen: the all-heads engine forward
    (keep_unit_out), UnitHeads in fp32 on each of the kept `out` tensors, SMAPLossNative.  Eval mode, the current stream, no host
    synchronisation.  sinks: None, or a dict that receives {(stage, unit): {"gx": gradient at out}} during backward().  Returns the
    loss dict (total_loss carries the graph)."""
    check_trainable(model, imgs, "head")
    B, _, H, W = imgs.shape
    eng = model.engine(B, H, W, imgs.device, all_heads=True, keep_unit_out=True)       # built once: `out` does not depend on the heads
    eng.run(imgs.float(), out=eng.new_output())
    outs = eng.unit_out_sources()
    return units_loss(model, {**frozen, **leaves}, lambda s, ind: outs[(s, ind)], valids, labels, rdepth, sinks)


def head_parameter_gradients(model, imgs, valids, labels, rdepth):
    """(losses, {state_dict key: gradient of total_loss} for the 288 head parameters, {(stage, unit): gradient at the unit's out,
    [B, h, w, chl] fp32}).  The last is produced, not consumed: the backward pass through the rest of the unit is not here."""
    leaves, frozen = head_leaves(model, imgs.device)
    sinks = {}
    losses = heads_loss(model, leaves, frozen, imgs, valids, labels, rdepth, sinks)
    losses["total_loss"].backward()
    return ({k: v.detach() for k, v in losses.items()}, {k: v.grad for k, v in leaves.items()}, {k: d["gx"] for k, d in sinks.items()})


class FrozenBackboneTuner:
    """What HeadFineTuner and trunk.DecoderFineTuner share: the reference's Adam (lib/utils/solver.py make_optimizer) over fp32 leaves of
    the model's parameters `keys`, and loss / step / commit around `loss_fn(model, leaves, frozen, imgs, valids, labels, rdepth)`."""

    def __init__(self, model, cfg, keys, loss_fn, lr=None, weight_decay=None, num_gpu=1, device=None):
        solver = getattr(cfg, "SOLVER", None)
        base, decay = getattr(solver, "BASE_LR", None), getattr(solver, "WEIGHT_DECAY", None)
        if (lr is None and base is None) or (weight_decay is None and decay is None):
            raise ValueError("cfg.SOLVER has no BASE_LR / WEIGHT_DECAY (this repository's inference config leaves the optimiser's entries out): "
                             "give lr and weight_decay")
        lr = base * num_gpu if lr is None else lr
        weight_decay = decay if weight_decay is None else weight_decay
        self.model, self.loss_fn = model, loss_fn
        self.leaves, self.frozen = parameter_leaves(model, keys, device)
        self.optimizer = torch.optim.Adam(list(self.leaves.values()), lr=lr, betas=(0.9, 0.999), eps=1e-08, weight_decay=weight_decay)

    def loss(self, imgs, valids, labels, rdepth):
        """The loss dict at the tuner's current parameters (no graph)."""
        with torch.no_grad():
            return self.loss_fn(self.model, self.leaves, self.frozen, imgs, valids, labels, rdepth)

    def step(self, imgs, valids, labels, rdepth):
        """One optimizer step; returns the loss dict BEFORE the step (detached device scalars, no synchronisation)."""
        self.optimizer.zero_grad(set_to_none=True)
        losses = self.loss_fn(self.model, self.leaves, self.frozen, imgs, valids, labels, rdepth)
        losses["total_loss"].backward()
        self.optimizer.step()
        return {k: v.detach() for k, v in losses.items()}

    def commit(self):
        own = dict(self.model.named_parameters())
        with torch.no_grad():
            for k, v in self.leaves.items():
                own[k].copy_(v)
        self.model.invalidate_engine()


class HeadFineTuner(FrozenBackboneTuner):
    """Adam on the head parameters of `model`, the backbone frozen (the common way to adapt the key-point, relative-depth and
    root-depth heads to a new camera or data set).  The optimizer is configured as the reference's lib/utils/solver.py make_optimizer
    configures it from the experiment's cfg: Adam(lr = cfg.SOLVER.BASE_LR * num_gpu, betas (0.9, 0.999), eps 1e-8,
    weight_decay = cfg.SOLVER.WEIGHT_DECAY) -- over the head parameters alone.  lr / weight_decay, where given, replace the cfg's values
    (fine-tuning usually wants a smaller rate than training from scratch); a cfg without those two entries (this repository's own config.py) needs both.

        tuner = HeadFineTuner(model.eval(), cfg)
        for imgs, valids, labels, rdepth in batches:
            losses = tuner.step(imgs, valids, labels, rdepth)
        tuner.commit()

    The engine is built once and never between steps: the frozen backbone's `out` tensors do not depend on the heads, and the heads
    themselves run in fp32 from the tuner's own leaves (UnitHeads).  commit() writes the leaves back into the model's parameters and
    calls model.invalidate_engine() once, so the next model(...) rebuilds its schedules from the trained weights."""

    def __init__(self, model, cfg, lr=None, weight_decay=None, num_gpu=1, device=None):
        super().__init__(model, cfg, head_parameter_keys(model.stage_num), heads_loss, lr, weight_decay, num_gpu, device)
