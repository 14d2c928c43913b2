"""Decoder training on a frozen ResNet, on the GPU, small network, both valloss_inputs cases: the engine seam
(BackboneEngine(keep_unit_in=True).unit_in_sources), SMAP.decoder_parameter_gradients against the reference's whole network in float64
(tests/golden/trunk_small.npz, heads_small.npz), and DecoderFineTuner.

The x3 backbone's x4 .. x1 lie within 2e-5 of their maxima of float64's (the figure the project holds x3 head tensors to) and no bound is
derived for what that does to a gradient: the 28 trunk gradients and the four gradients at x4 .. x1 are MEASURED distances against the
float64 reference -- relative L2 per tensor, the measure the 288 head gradients are held to -- recorded in profiles/trunk_parity.json and
asserted at 4 x, the project's margin for a recorded distance."""
import numpy as np
import pytest
import torch

import heads_scenes as HS
import valloss_inputs as VI
from smap_amd import finetune as F
from smap_amd import gemm_f32 as G
from smap_amd import trunk as T
from train_kit import DEV, golden_distances, inputs, largest_per_kind, relative_l2, small_net, source_tensor, tuner_contract, value

pytestmark = pytest.mark.gpu
LOSSES = ("total_loss", "loss_2d", "loss_bone", "loss_root")
LAST = 2
X_TOLERANCE = 2e-5                  # of each tensor's maximum: what the x3 schedule's tensors are held to against float64
# profiles/trunk_parity.json, the largest over both cases: end_to_end_trunk_gradient_relative_l2 (over the 28 trunk tensors and the
# four gradients at x4 .. x1)
TRUNK_GRADIENT_DISTANCE = 1.01e-6
# profiles/heads_parity.json: what tests/test_heads_train_gpu.py holds the 288 head gradients and the losses to -- the losses against
# the reference's, and the x3 schedule's loss after commit() against the tuner's fp32 loss
HEAD_GRADIENT_DISTANCE = 3.6e-6
FORWARD_DISTANCE = 5.9e-7
MARGIN = 4


@pytest.fixture(scope="module")
def small():
    return small_net()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(f"{golden_dir}/trunk_small.npz")


@pytest.fixture(scope="module")
def golden_heads(golden_dir):
    return np.load(f"{golden_dir}/heads_small.npz")


@pytest.fixture(scope="module")
def golden_losses(golden_dir):
    return np.load(f"{golden_dir}/valloss_small.npz")


@pytest.fixture(scope="module")
def x(golden_dir):
    return torch.from_numpy(np.load(f"{golden_dir}/backbone_small.npz")["x"]).to(DEV)


@pytest.fixture(scope="module")
def gradients(small, x):
    """SMAP.decoder_parameter_gradients of both cases, computed once."""
    net, _ = small
    out = {}
    for case in VI.CASES:
        inp = inputs(case)
        out[case] = net.decoder_parameter_gradients(x, inp["valids"], inp["labels"], inp["rdepth"])
    return out


@pytest.mark.parametrize("precision", ["x3", "f16"])
def test_keeping_unit_in_changes_no_output(small, golden, x, precision):
    """An engine built with keep_unit_in runs the same ops in the same order and returns output buffers and the 36 head tensors byte-equal
    to one built without it; unit_in_sources is read_tensor of the units' inputs in a layout the trunk takes, and the last stage's
    x4 .. x1 of the x3 engine lie within 2e-5 of their maxima of the reference's float64 values (the golden file's 1024 samples each)."""
    from smap_amd.engine import BackboneEngine, plan_cache_key
    _, sd = small
    plain = BackboneEngine(sd, 2, 64, 96, DEV, precision=precision, all_heads=True, keep_unit_out=True)
    kept = BackboneEngine(sd, 2, 64, 96, DEV, precision=precision, all_heads=True, keep_unit_out=True, keep_unit_in=True)
    ops = lambda e: [(o.kind, o.out.name if o.out else None) for o in e.graph.ops]
    assert kept.n_ops == plain.n_ops and ops(kept) == ops(plain)
    with pytest.raises(RuntimeError, match="keep_unit_in"):
        plain.unit_in_sources()
    with pytest.raises(ValueError, match="all_heads"):
        BackboneEngine(sd, 2, 64, 96, DEV, precision=precision, keep_unit_in=True)
    args = (sd, 2, 64, 96, 3, 256, 43, 14, precision, None, False)
    assert plan_cache_key(*args, True, None, True) == plan_cache_key(*args, True, None, True, False) != plan_cache_key(*args, True, None, True, True)
    outs = []
    for eng in (plain, kept):
        out = eng.new_output()
        eng.run(x, out=out)
        outs.append((out, [source_tensor(eng, s, out).clone() for d in eng.head_sources(out) for s in d.values()],
                     [t.clone() for t in eng.unit_out_sources().values()]))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert len(outs[0][1]) == 36 and all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    assert all(torch.equal(a, b) for a, b in zip(outs[0][2], outs[1][2]))
    srcs = kept.unit_in_sources()
    assert sorted(srcs) == [(s, i) for s in range(3) for i in range(4)]
    for (s, ind), t in srcs.items():
        h, w, c = 2 << ind, 3 << ind, 2048 >> ind
        assert t.dtype == torch.float16 and tuple(t.shape) == ((2, h, w, 2, c) if precision == "x3" else (2, h, w, c))
        want = kept.read_tensor(kept.graph.unit_in[(s, ind)].name)[:2]
        assert torch.equal(value(t), want.float()), (s, ind)
        assert float(want.min()) >= 0 and float(want.max()) > 0                      # post-ReLU, and alive
        G.x_descriptor(t)
    if precision == "x3":
        first = 2 + HS.N_PROJ
        for ind in range(4):
            want = golden["x_digests"][ind]
            got, _ = HS.digest("x%d" % (4 - ind), value(srcs[(LAST, ind)]).double().cpu().numpy(), want.size - first)
            top = np.abs(want[first:]).max()
            err = np.abs(got[first:] - want[first:]).max()
            print("x%d  max |x3 - float64| over the samples %.3e  = %.3e of the largest sample" % (4 - ind, err, err / top))
            assert err <= X_TOLERANCE * top, (ind, err, top)


def test_fp32_chain_at_untrained_weights_is_the_engines_out(small, x):
    """The UnitTrunk chain up1 -> up4 of the last stage from unit_in_sources, at the model's own weights, against the engine's kept `out`
    (the x3 schedule's trunk on the same inputs): within 2e-5 of each tensor's maximum."""
    net, _ = small
    eng = net.engine(2, 64, 96, x.device, all_heads=True, keep_unit_out=True, keep_unit_in=True)
    eng.run(x, out=eng.new_output())
    outs, ins = eng.unit_out_sources(), eng.unit_in_sources()
    leaves, frozen = F.parameter_leaves(net, F.trunk_parameter_keys(LAST))
    params = {**frozen, **{k: v.detach() for k, v in leaves.items()}}
    o = None
    for ind in range(4):
        o = T.unit_trunk(ins[(LAST, ind)], o, params, F.unit_name(LAST, ind), ind)
        want = value(outs[(LAST, ind)])
        err, top = float((o - want).abs().max()), float(want.max())
        print("up%d  max |fp32 chain - x3 out| %.3e  = %.3e of the maximum" % (ind + 1, err, err / top))
        assert tuple(o.shape) == (2, 2 << ind, 3 << ind, 256) and err <= X_TOLERANCE * top, (ind, err, top)


@pytest.mark.parametrize("case", VI.CASES)
def test_trunk_gradients_against_the_reference(small, golden, golden_losses, gradients, case):
    """Each of the 28 trunk gradients and of the four gradients at x4 .. x1 against the reference's own (its whole network in float64):
    relative L2 per tensor at most MARGIN * TRUNK_GRADIENT_DISTANCE; the losses within MARGIN * FORWARD_DISTANCE of the reference's."""
    net, _ = small
    losses, grads, gxs = gradients[case]
    assert len(grads) == 316 and sorted(grads) == sorted(F.decoder_parameter_keys(3)) and len(gxs) == 4
    sd = net.state_dict()
    assert all(grads[k].shape == sd[k].shape and grads[k].dtype == torch.float32 for k in grads)
    whole, digests = golden[case + "_whole"], golden[case + "_digests"]
    assert int(golden["seed"]) == VI.SEED and digests.shape[0] == 7
    worst = largest_per_kind(golden_distances(F.trunk_parameter_keys(LAST), grads, whole, digests))
    for ind, g in enumerate(gxs):
        assert tuple(g.shape) == (2, 2 << ind, 3 << ind, 2048 >> ind) and g.dtype == torch.float32
        worst["gx%d" % (4 - ind)] = (relative_l2("gx%d" % (4 - ind), g.double().cpu().numpy(), want_digest=golden[case + "_gx_digests"][ind]), "")
    print(case, "end-to-end trunk relative L2 against the reference, largest per kind", worst)
    largest = max(v[0] for v in worst.values())
    print(case, "end-to-end trunk relative L2 against the reference, largest", largest)
    assert largest <= MARGIN * TRUNK_GRADIENT_DISTANCE, (case, worst)
    for n, k in enumerate(LOSSES):
        assert losses[k].grad_fn is None
        rel = abs(float(losses[k]) - golden_losses[case + "_losses"][n]) / abs(golden_losses[case + "_losses"][n])
        print(case, k, "forward distance, relative", rel)
        assert rel <= MARGIN * FORWARD_DISTANCE, (case, k, rel)


@pytest.mark.parametrize("case", VI.CASES)
def test_head_gradients_still_meet_the_reference(golden_heads, gradients, case):
    """The 288 head gradients out of decoder_parameter_gradients -- the last stage's now on the fp32 O -- against heads_small.npz at the
    figure tests/test_heads_train_gpu.py holds head_parameter_gradients to."""
    _, grads, _ = gradients[case]
    whole, digests = golden_heads[case + "_whole"], golden_heads[case + "_digests"]
    assert digests.shape[0] == 72
    largest = max([(0.0, "")] + [(rel, k) for k, rel in golden_distances(F.head_parameter_keys(3), grads, whole, digests).items()])
    print(case, "head gradients from the decoder pass, largest relative L2", largest)
    assert largest[0] <= MARGIN * HEAD_GRADIENT_DISTANCE, (case, largest)


def test_decoder_tuner_lowers_the_loss_and_commits_once(small, x, monkeypatch):
    """Five Adam steps at a small learning rate strictly lower total_loss and move the trunk leaves; the engine is built exactly once
    before commit(); after it the model's own validation loss (the x3 all-heads schedule rebuilt from the committed weights) agrees with
    the tuner's fp32 loss at those weights within MARGIN * FORWARD_DISTANCE, relative: the recorded loss distance HeadFineTuner's commit is
    held to, although here the trunk too runs in x3 on one side and in fp32 on the other."""
    def built_tuner(net, cfg, tuner):
        assert isinstance(tuner, F.FrozenBackboneTuner) and isinstance(F.HeadFineTuner(net, cfg), F.FrozenBackboneTuner)      # one shared tuner
        assert len(tuner.leaves) == 316 and tuner.optimizer.defaults["betas"] == (0.9, 0.999) and tuner.optimizer.defaults["eps"] == 1e-8

    def before_commit(tuner, before):
        assert all(not torch.equal(tuner.leaves[k].detach(), before[k]) for k in F.trunk_parameter_keys(LAST))  # every trunk leaf moved
    own, final = tuner_contract(F.DecoderFineTuner, F.decoder_parameter_keys(3), ("keep_unit_in", "keep_unit_out", "all_heads"), small[1], x,
                                monkeypatch, built_tuner, before_commit)
    for k in LOSSES:
        rel = abs(float(own[k]) - float(final[k])) / abs(float(final[k]))
        print(k, "x3 schedule", float(own[k]), "fp32 decoder", float(final[k]), "committed loss distance, relative", rel)
        assert rel <= MARGIN * FORWARD_DISTANCE, (k, rel)
