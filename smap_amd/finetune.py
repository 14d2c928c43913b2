"""Training on a frozen backbone: which parameters move, the loss as a function of them, their gradients, and the Adam tuners
(DESIGN.md sections 18 and 19).  The fp32 arithmetic is heads.py (UnitHeads: the three head arms of a unit) and trunk.py (UnitTrunk:
u_skip, up_conv and the bilinear add); here the engine's kept tensors are wired through them into SMAPLossNative.

    head training     the 6 head convs of each of the 4 * stage_num units, on the engine's `out` tensors (HeadFineTuner)
    decoder training  those, and the trunks of the LAST stage's four units, from the engine's x4 .. x1 (DecoderFineTuner)
"""
import torch

from . import heads as H
from . import trunk as T
from .loss import SMAPLossNative

TRAINED = ("conv.weight", "conv.bias", "bn.weight", "bn.bias")
FROZEN = ("bn.running_mean", "bn.running_var")
HEAD_KEYS = ("heatmap_2d", "det_d", "root_d")
ARMS = ("res", "res_d", "res_rd")          # heatmap_2d | det_d | root_d: <unit>.<arm>_conv1, <unit>.<arm>_conv2 (model/smap.py)


def unit_name(stage, ind):
    return "stage%d.upsample.up%d" % (stage, ind + 1)


def arm_prefixes(unit):
    """The (conv1, conv2) module prefixes of the three arms of Upsample_unit `unit` (e.g. "stage0.upsample.up1")."""
    return [("%s.%s_conv1" % (unit, a), "%s.%s_conv2" % (unit, a)) for a in ARMS]


def trunk_prefixes(unit, ind):
    """The module prefixes of a unit's trunk convs: u_skip, and up_conv from the second unit on."""
    return [unit + ".u_skip"] + ([unit + ".up_conv"] if ind > 0 else [])


def head_parameter_keys(stage_num):
    """The state_dict keys of what head training changes: conv.weight, conv.bias, bn.weight, bn.bias of the 6 head convs of each of
    the 4 * stage_num units (72 convs, 288 keys at three stages), in schedule order."""
    return ["%s.%s" % (m, k) for s in range(stage_num) for ind in range(4) for pair in arm_prefixes(unit_name(s, ind)) for m in pair for k in TRAINED]


def trunk_parameter_keys(stage):
    """The 28 state_dict keys of the trunks of `stage`'s four units: u_skip x 4 and up_conv x 3, times the four trained kinds."""
    return ["%s.%s" % (m, k) for ind in range(4) for m in trunk_prefixes(unit_name(stage, ind), ind) for k in TRAINED]


def decoder_parameter_keys(stage_num):
    """What decoder training changes: the head parameters of every stage (288 keys at three stages) and the 28 trunk parameters of the
    LAST stage.  The last stage has neither skips nor cross_conv, so its `out` tensors feed its heads and the next finer unit alone and
    these gradients are exact; the trunks of the stages before it also feed the next stage's ResNet, whose backward pass is not here."""
    return head_parameter_keys(stage_num) + trunk_parameter_keys(stage_num - 1)


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
    outputs = {k: [[None] * 4 for _ in range(model.stage_num)] for k in HEAD_KEYS}
    for s in range(model.stage_num):
        for ind in range(4):
            sink = None
            if sinks is not None:
                sink = sinks.setdefault((s, ind), {})
            ys = H.unit_heads(unit_x(s, ind), params, arm_prefixes(unit_name(s, ind)), sink=sink)
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
    B, _, Hh, W = imgs.shape
    eng = model.engine(B, Hh, W, imgs.device, all_heads=True, keep_unit_out=True)       # built once: `out` does not depend on the heads
    eng.run(imgs.float(), out=eng.new_output())
    outs = eng.unit_out_sources()
    return units_loss(model, {**frozen, **leaves}, lambda s, ind: outs[(s, ind)], valids, labels, rdepth, sinks)


def decoder_loss(model, leaves, frozen, imgs, valids, labels, rdepth, sinks=None):
    """The training loss of the network as a function of `leaves` (decoder_parameter_keys), the ResNets frozen: ONE engine forward
    (all heads, the units' out and input tensors kept); the heads of stages 0 .. n - 2 in fp32 on the engine's `out`, exactly as
    heads_loss runs them; for the last stage a UnitTrunk chain up1 -> up4 in fp32 from the engine's frozen x4 .. x1, its heads on
    that fp32 O; SMAPLossNative.  The engine is built once: the trunk's weights move, the engine's inputs to it do not.
    sinks: None, or a dict that receives {unit: {"gx": gradient at the last stage's input of that unit}} during backward().  Returns the
    loss dict (total_loss carries the graph)."""
    check_trainable(model, imgs, "decoder")
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
        chain.append(T.unit_trunk(ins[(s, ind)], chain[-1] if chain else None, params, unit_name(s, ind), ind, sink=sink))
        return chain[-1]
    return units_loss(model, params, unit_x, valids, labels, rdepth)


def _parameter_gradients(model, keys, loss_fn, imgs, valids, labels, rdepth):
    """(detached losses, {key: gradient of total_loss}, the sinks loss_fn filled) after one backward pass from fresh leaves."""
    leaves, frozen = parameter_leaves(model, keys, imgs.device)
    sinks = {}
    losses = loss_fn(model, leaves, frozen, imgs, valids, labels, rdepth, sinks)
    losses["total_loss"].backward()
    return {k: v.detach() for k, v in losses.items()}, {k: v.grad for k, v in leaves.items()}, sinks


def head_parameter_gradients(model, imgs, valids, labels, rdepth):
    """(losses, {state_dict key: gradient of total_loss} for the 288 head parameters, {(stage, unit): gradient at the unit's out,
    [B, h, w, chl] fp32}).  The last is produced, not consumed: the backward pass through the rest of the unit is not here."""
    losses, grads, sinks = _parameter_gradients(model, head_parameter_keys(model.stage_num), heads_loss, imgs, valids, labels, rdepth)
    return losses, grads, {k: d["gx"] for k, d in sinks.items()}


def decoder_parameter_gradients(model, imgs, valids, labels, rdepth):
    """(losses, {state_dict key: gradient of total_loss} for the 316 decoder parameters, [the gradients at the last stage's x4, x3, x2,
    x1, [B, h, w, Cin] fp32]).  The last is the seam a backward pass through the last ResNet would start from: nothing here consumes it."""
    losses, grads, sinks = _parameter_gradients(model, decoder_parameter_keys(model.stage_num), decoder_loss, imgs, valids, labels, rdepth)
    return losses, grads, [sinks[ind]["gx"] for ind in range(4)]


class FrozenBackboneTuner:
    """What HeadFineTuner and DecoderFineTuner share: the reference's Adam (lib/utils/solver.py make_optimizer) over fp32 leaves of
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


class DecoderFineTuner(FrozenBackboneTuner):
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
