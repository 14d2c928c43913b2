"""What the tests of the fp32 training path share (test_{heads,trunk}_{cpu,gpu}.py, test_{heads,trunk}_train_gpu.py): the bound check,
guarded buffers, the operand layouts, the small network and its inputs, the walk of a golden gradient file, the carried bound of the
unfolded gradients, the fine-tuners' contract, and the fake-pointer setters of the argument-check tests."""
import types

import numpy as np
import pytest
import torch

import heads_restate as HR
import heads_scenes as HS
import valloss_inputs as VI
from helpers import make_cfg
from recipe import recipe_state_dict
from smap_amd import finetune as F

DEV = "cuda:0"
U = HR.U


def held(what, got, want, bound, worst=None):
    """got within bound of want on every element.  Without `worst` the largest measured / bound ratio (0 / 0 counts as 0) is printed and
    returned; with it, it is recorded there instead, as the largest per kind of tensor (the last two parts of `what`)."""
    err = (got.double().cpu() - want).abs()
    inf, zero = torch.full_like(err, float("inf")), torch.zeros_like(err)
    ratio = float(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, inf, zero)).max())
    if worst is None:
        print("  %-22s max err %.3e  measured / bound %.4f" % (what, float(err.max()), ratio))
    else:
        kind = ".".join(what.rsplit(".", 2)[-2:])
        worst[kind] = max(worst.get(kind, 0.0), ratio)
    assert ratio <= 1.0, (what, ratio)
    return ratio


def unfolded_held(m, params, grad_of, gw, gb, ew, eb, eps, worst=None):
    """The four gradients grad_of("<m>.<kind>") at the unfolded parameters of module `m` against the restatement's chain rule from the
    folded (gw, gb).  Bound: the folded gradients' bounds (ew, eb) carried through the fold's Jacobian on magnitudes, plus torch's own
    fp32 fold arithmetic: (n + 8) * 2^-24 on the magnitudes of its terms, n = the terms of bn.weight's sum (the conv's fan-in + 1)."""
    p = {k: params["%s.%s" % (m, k)].detach().double().cpu() for k in F.TRAINED + F.FROZEN}
    n = p["conv.weight"][0].numel() + 1
    ref = HR.unfold_grads(p, gw, gb, eps)
    carried = HR.unfold_grads(p, ew, eb, eps, magnitudes=True)
    mags = HR.unfold_grads(p, gw.abs() + ew, gb.abs() + eb, eps, magnitudes=True)
    name = m.rsplit(".", 1)[-1] if worst is None else m
    for kind in F.TRAINED:
        held("%s.%s" % (name, kind), grad_of("%s.%s" % (m, kind)), ref[kind], carried[kind] + (n + 8) * U * mags[kind], worst)


GUARD = 64           # floats, 256 bytes: the payload keeps the buffer's alignment


def guarded(n, byte):
    buf = torch.full((4 * (n + 2 * GUARD),), byte, dtype=torch.uint8, device=DEV)
    return buf, buf.view(torch.float32)[GUARD:GUARD + n]


def layouts(t):
    """The same fp16-representable values in every layout smap_heads_x describes."""
    t16 = t.half()
    return {"f32": t16.float(), "f32 padded pixel": torch.cat([t16.float(), torch.full_like(t16, float("nan"), dtype=torch.float32)], -1)[..., :t16.shape[-1]],
            "f16": t16, "hi|lo, lo = 0": torch.stack([t16, torch.zeros_like(t16)], dim=3)}


def small_net(sd=None, precision="x3"):
    """(the small network on the device, its state dict): recipe weights, or `sd`; precision None leaves the model's default."""
    from smap_amd.model.smap import SMAP
    torch.manual_seed(0)
    net = SMAP(make_cfg((16, 24))).eval()
    sd = recipe_state_dict(net.state_dict()) if sd is None else sd
    net.load_state_dict(sd)
    net = net.to(DEV)
    if precision is not None:
        net.precision = precision
    return net, sd


def inputs(case):
    return {k: torch.from_numpy(v).to(DEV) for k, v in VI.inputs(case).items()}


def value(t):
    """fp32 values of a unit tensor in either engine layout."""
    return t[..., 0, :].float() + t[..., 1, :].float() if t.dim() == 5 else t.float()


def source_tensor(eng, s, out):
    """[frames, c, h, w] view of a head source through its descriptor: what the loss reads."""
    base = eng.arena if eng.arena.data_ptr() <= s.ptr < eng.arena.data_ptr() + eng.arena.numel() else out.view(torch.uint8)
    off = (s.ptr - base.data_ptr()) // 4
    return torch.as_strided(base.view(torch.float32), (eng.B, s.c, s.h, s.w), (s.frame_stride, s.ch_stride, s.w * s.pix_stride, s.pix_stride), off)


def relative_l2(key, got, want_digest=None, want_whole=None):
    """Relative L2 of a tensor against the golden file: over the whole tensor, or over the digest's seeded samples, whose sum and three
    seeded projections are held too, relative to the sum of magnitudes (times the projection's largest weight)."""
    if want_whole is not None:
        return float(np.linalg.norm(got - want_whole) / np.linalg.norm(want_whole))
    first = 2 + HS.N_PROJ
    d, scale = HS.digest(key, got, want_digest.size - first)
    rel = np.linalg.norm(d[first:] - want_digest[first:]) / np.linalg.norm(want_digest[first:])
    return float(max(rel, (np.abs(d[:first] - want_digest[:first]) / scale[:first]).max()))


def golden_distances(keys, grads, whole, digests):
    """{key: relative_l2 of grads[key]} against a golden gradient file, in the order of `keys`: conv.weight against the next row of
    `digests`, every other tensor against the next values of `whole`; both arrays are consumed exactly."""
    at, row, out = 0, 0, {}
    for k in keys:
        got = grads[k].double().cpu().numpy()
        if k.endswith("conv.weight"):
            out[k] = relative_l2(k, got, want_digest=digests[row])
            row += 1
        else:
            out[k] = relative_l2(k, got, want_whole=whole[at:at + got.size].reshape(got.shape))
            at += got.size
    assert at == whole.size and row == digests.shape[0]
    return out


def largest_per_kind(distances):
    """{kind: (the largest distance, its key)} of golden_distances' result, kind = the last two parts of the key."""
    worst = {}
    for k, rel in distances.items():
        kind = ".".join(k.rsplit(".", 2)[-2:])
        if rel > worst.get(kind, (0.0, ""))[0]:
            worst[kind] = (rel, k)
    return worst


def tuner_contract(cls, keys, engine_flags, sd, x, monkeypatch, built_tuner=None, before_commit=None):
    """What HeadFineTuner and DecoderFineTuner both promise, on a model of their own with the state dict `sd`: the optimizer configured
    from cfg.SOLVER as make_optimizer does; five Adam steps at a small learning rate strictly lower total_loss; the engine is built
    exactly once, with `engine_flags`, before commit(); nothing is written before it; commit() moves `keys` and nothing else and bumps
    weights_generation once; the model's own validation loss then rebuilds its engine without engine_flags[0].  A test may check more in
    built_tuner(net, cfg, tuner), right after the tuner is built, and in before_commit(tuner, before), after the steps.  Returns (the
    model's loss dict, the tuner's loss dict at the same weights)."""
    import smap_amd.model.smap as M
    net, _ = small_net(sd)                                       # its own model: commit() changes it
    inp = inputs("ones")
    built = []
    real = M.BackboneEngine
    monkeypatch.setattr(M, "BackboneEngine", lambda *a, **k: (built.append(k), real(*a, **k))[1])
    cfg = make_cfg((16, 24))
    cfg.SOLVER = types.SimpleNamespace(BASE_LR=2e-4, WEIGHT_DECAY=8e-6)             # the reference's config.py:51,54
    assert cls(net, cfg, num_gpu=2).optimizer.defaults["lr"] == 4e-4 and \
        cls(net, cfg).optimizer.defaults["weight_decay"] == 8e-6                     # as make_optimizer configures it
    with pytest.raises(ValueError, match="BASE_LR"):
        cls(net, make_cfg((16, 24)))
    tuner = cls(net, cfg, lr=1e-5)
    if built_tuner is not None:
        built_tuner(net, cfg, tuner)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    seen = [float(tuner.step(x, inp["valids"], inp["labels"], inp["rdepth"])["total_loss"]) for _ in range(5)]
    final = tuner.loss(x, inp["valids"], inp["labels"], inp["rdepth"])
    seen.append(float(final["total_loss"]))
    print("total_loss per step", seen)
    assert all(b < a for a, b in zip(seen, seen[1:])), seen
    assert len(built) == 1 and all(built[0].get(f) for f in engine_flags)
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())      # nothing written before commit
    if before_commit is not None:
        before_commit(tuner, before)
    gen = net.weights_generation
    tuner.commit()
    assert net.weights_generation == gen + 1
    keys = set(keys)
    after = net.state_dict()
    assert all(torch.equal(after[k], before[k]) == (k not in keys) for k in after)   # the named parameters moved, nothing else did
    own = net(x, inp["valids"], inp["labels"], inp["rdepth"])
    assert len(built) == 2 and not built[1].get(engine_flags[0])
    return own, final


FAKE = 0x7F0000000000            # never dereferenced: the argument-check tests' calls are refused before any HIP call


def set_attr(name, value):
    return lambda a: setattr(a, name, value)


def set_fields(which, **kw):
    """Sets fields of the struct (or attributes of the object) a.<which>."""
    def f(a):
        for k, v in kw.items():
            setattr(getattr(a, which), k, v)
    return f
