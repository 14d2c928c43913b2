"""Head training on a frozen backbone, on the GPU: the engine seam (BackboneEngine(keep_unit_out=True).unit_out_sources),
SMAP.head_parameter_gradients and HeadFineTuner on the small network (2 x 3 x 64 x 96, recipe weights, the inputs of valloss_inputs.py).

The head arms themselves are pinned by tests/test_heads_gpu.py; here the chain around them is: the loss value against the REFERENCE's
float64 loss (tests/golden/valloss_small.npz) with test_valloss_gpu.py's bound -- 1.5 * 2e-5 * S, S the fixture's first-order
sensitivity to a relative perturbation of the native head tensors, 2e-5 the x3 engine's bound on them: the fp32 arms read the engine's
x3 `out`, so their head tensors carry that error and the arms' own (1e-6) on top, inside the half-again; a head wired to the wrong
unit, arm or label scale misses it by orders of magnitude -- and every parameter gradient against the float64 restatement
(tests/heads_restate.py) of the arms' backward on the engine's own `out` and the upstream gradients the loss handed over, within the
composed fp32 bounds of test_heads_gpu.py (the loss gradient itself is tests/test_lossgrad_gpu.py's).

End to end against the REFERENCE (tests/golden/heads_small.npz, gen_golden_heads_small.py: the reference's whole small network in float64,
every head through its own F.interpolate and SMAP._calculate_loss, total_loss.backward()): the relative L2 distance of each of the 288
parameter gradients, and the relative distance of the four losses.  These two are MEASURED distances -- the engine's x3 backbone differs
from float64 by a few 1e-6 and no bound is derived for what that does to a gradient -- recorded in profiles/heads_parity.json and
asserted at 4 times the largest recorded value (the results are bit-reproducible: the margin absorbs a toolchain change):
GRADIENT_DISTANCE and FORWARD_DISTANCE below."""
import numpy as np
import pytest
import torch

import heads_restate as R
import heads_scenes as HS
import valloss_inputs as VI
from smap_amd import finetune as F
from smap_amd import gemm_f32 as G
from smap_amd import heads as H
from train_kit import DEV, golden_distances, held, inputs, largest_per_kind, small_net, source_tensor, tuner_contract, unfolded_held, value

pytestmark = pytest.mark.gpu
LOSSES = ("total_loss", "loss_2d", "loss_bone", "loss_root")
# profiles/heads_parity.json, the largest over both cases: end_to_end_gradient_relative_l2 (over the 288 tensors) and
# forward_distance_relative (over the four losses, |value - reference| / reference)
GRADIENT_DISTANCE = 3.6e-6
FORWARD_DISTANCE = 5.9e-7
MARGIN = 4


@pytest.fixture(scope="module")
def small():
    return small_net()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(f"{golden_dir}/valloss_small.npz")


@pytest.fixture(scope="module")
def golden_gradients(golden_dir):
    return np.load(f"{golden_dir}/heads_small.npz")


@pytest.fixture(scope="module")
def x(golden_dir):
    return torch.from_numpy(np.load(f"{golden_dir}/backbone_small.npz")["x"]).to(DEV)


@pytest.mark.parametrize("precision", ["x3", "f16"])
def test_keeping_unit_out_changes_no_output(small, x, precision):
    """An engine built with keep_unit_out returns maps and head tensors byte-equal to one built without it; unit_out_sources is
    read_tensor of the same `out` (hi + lo in fp32 for the planes), in a layout the head arms take."""
    from smap_amd.engine import BackboneEngine
    _, sd = small
    plain = BackboneEngine(sd, 2, 64, 96, DEV, precision=precision, all_heads=True)
    kept = BackboneEngine(sd, 2, 64, 96, DEV, precision=precision, all_heads=True, keep_unit_out=True)
    assert kept.n_ops == plain.n_ops and [(o.kind, o.out.name if o.out else None) for o in kept.graph.ops] == \
        [(o.kind, o.out.name if o.out else None) for o in plain.graph.ops]
    with pytest.raises(RuntimeError, match="keep_unit_out"):
        plain.unit_out_sources()
    with pytest.raises(ValueError, match="all_heads"):
        BackboneEngine(sd, 2, 64, 96, DEV, precision=precision, keep_unit_out=True)
    outs = []
    for eng in (plain, kept):
        out = eng.new_output()
        eng.run(x, out=out)
        outs.append((out, [source_tensor(eng, s, out).clone() for d in eng.head_sources(out) for s in d.values()]))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert len(outs[0][1]) == 36 and all(torch.equal(a, b) for a, b in zip(*[o[1] for o in outs]))
    srcs = kept.unit_out_sources()
    assert sorted(srcs) == [(s, i) for s in range(3) for i in range(4)]
    for (s, ind), t in srcs.items():
        h, w = 2 << ind, 3 << ind
        assert t.dtype == torch.float16 and tuple(t.shape) == ((2, h, w, 2, 256) if precision == "x3" else (2, h, w, 256))
        want = kept.read_tensor(F.unit_name(s, ind) + ".out")[:2]
        got = value(t) if precision == "x3" else t
        assert torch.equal(got, want), (s, ind)
        assert float(want.min()) >= 0 and float(want.max()) > 0                      # post-ReLU, and alive
        G.x_descriptor(t)


@pytest.mark.parametrize("case", VI.CASES)
def test_head_parameter_gradients(small, golden, x, case):
    net, _ = small
    inp = inputs(case)
    losses, grads, gouts = net.head_parameter_gradients(x, inp["valids"], inp["labels"], inp["rdepth"])
    n_engines = len(net._engines)
    # the same bits from the pieces, which also hand over what the restatement needs: G at every head, the engine's own `out`
    leaves, frozen = F.head_leaves(net)
    sinks = {}
    again = F.heads_loss(net, leaves, frozen, x, inp["valids"], inp["labels"], inp["rdepth"], sinks)
    again["total_loss"].backward()
    assert len(net._engines) == n_engines
    assert sorted(grads) == sorted(F.head_parameter_keys(3)) and len(grads) == 288 and sorted(gouts) == sorted(sinks) and len(gouts) == 12
    sd = net.state_dict()
    for k, g in grads.items():
        assert g.shape == sd[k].shape and g.dtype == torch.float32 and torch.equal(g, leaves[k].grad), k
    for n, k in enumerate(LOSSES):
        assert torch.equal(losses[k], again[k].detach()) and losses[k].grad_fn is None
        err, allowed = abs(float(losses[k]) - golden[case + "_losses"][n]), 1.5 * 2e-5 * golden[case + "_S"][n]
        print(case, k, "value", float(losses[k]), "error against the reference", err, "allowed", allowed)
        assert err <= allowed, (case, k, err, allowed)
        rel = err / abs(golden[case + "_losses"][n])
        print(case, k, "forward distance, relative", rel)
        assert rel <= MARGIN * FORWARD_DISTANCE, (case, k, rel)
    eng = net.engine(2, 64, 96, x.device, all_heads=True, keep_unit_out=True)
    outs = eng.unit_out_sources()                                   # of the last run: the same images
    d = lambda t: t.detach().double().cpu()
    worst = {}
    for (s, ind), sink in sinks.items():
        assert torch.equal(gouts[(s, ind)], sink["gx"]) and tuple(sink["gx"].shape) == (2, 2 << ind, 3 << ind, 256)
        arms = F.arm_prefixes(F.unit_name(s, ind))
        params = {**frozen, **{k: v.detach() for k, v in leaves.items()}}
        w1cat, b1cat, w2, b2 = (H.folded_unit_weights(params, arms))
        t = outs[(s, ind)]
        xs = d(value(t))
        f = dict(w1cat=d(w1cat), b1cat=d(b1cat), w2=[d(v) for v in w2], b2=[d(v) for v in b2], g=[d(v) for v in sink["g"]])
        z, _ = R.forward(xs, f["w1cat"], f["b1cat"], f["w2"], f["b2"])
        e_m, _ = R.forward_bounds(xs, f["w1cat"], f["b1cat"], f["w2"], f["b2"], z)
        tie, _ = HS.ties(None, xs, f["w1cat"], f["b1cat"])
        assert float(tie.double().mean()) <= HS.TIE_CAP
        # at a tie the kernel's own mask: M again from the workspace of a forward call on the same operands
        ys = [torch.empty((2, c, 2 << ind, 3 << ind), dtype=torch.float32, device=DEV) for c in HS.ARM_C]
        ws = H.forward(t, w1cat, b1cat, w2, b2, [H.nchw_source(y) for y in ys])
        m_k = d(H.workspace_views(ws, 2, 2 << ind, 3 << ind, 256, backward=False)["m"]).flatten(3)
        mask = torch.where(tie, m_k > 0, z > 0)
        want = R.backward(xs, f["w1cat"], f["w2"], f["g"], z, mask)
        e = R.backward_bounds(xs, f["w1cat"], f["w2"], f["g"], z, mask, e_m)
        held("gx", sink["gx"], want["gx"], e["gx"], worst)
        for a, (c1, c2) in enumerate(arms):
            sl = slice(a * 256, (a + 1) * 256)
            for m, gw, gb, ew, eb in ((c1, want["gw1"][sl], want["gb1"][sl], e["gw1"][sl], e["gb1"][sl]),
                                      (c2, want["gw2"][a], want["gb2"][a], e["gw2"][a], e["gb2"][a])):
                unfolded_held(m, params, grads.get, gw, gb, ew, eb, HS.EPS, worst)
    print(case, "largest measured / bound", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("case", VI.CASES)
def test_parameter_gradients_against_the_reference(small, golden_gradients, x, case):
    """Each of the 288 gradients of SMAP.head_parameter_gradients against the reference's own (its whole network, interpolation, loss
    and autograd in float64): relative L2 per tensor -- over the whole tensor for conv.bias, bn.weight, bn.bias; over the golden file's 64
    seeded samples for conv.weight, whose sum and three seeded projections are held too, relative to the sum of magnitudes (times the
    projection's largest weight) -- at most MARGIN * GRADIENT_DISTANCE."""
    net, _ = small
    inp = inputs(case)
    _, grads, _ = net.head_parameter_gradients(x, inp["valids"], inp["labels"], inp["rdepth"])
    whole, digests = golden_gradients[case + "_whole"], golden_gradients[case + "_digests"]
    assert int(golden_gradients["seed"]) == VI.SEED and digests.shape[0] == 72
    worst = largest_per_kind(golden_distances(F.head_parameter_keys(3), grads, whole, digests))
    print(case, "end-to-end relative L2 against the reference, largest per kind", worst)
    largest = max(v[0] for v in worst.values())
    print(case, "end-to-end relative L2 against the reference, largest", largest)
    assert largest <= MARGIN * GRADIENT_DISTANCE, (case, worst)


def test_fine_tuner_lowers_the_loss_and_commits_once(small, golden, x, monkeypatch):
    """Five Adam steps at a small learning rate strictly lower total_loss; the engine is built exactly once before commit(); after it
    the model's own validation loss (SMAP.forward with labels: the x3 all-heads schedule, rebuilt from the committed weights) agrees
    with the tuner's fp32-arm loss at those weights within the recorded forward distance (FORWARD_DISTANCE, relative, times MARGIN):
    the two paths share the engine's `out` and differ in the head arms' arithmetic alone, x3 against fp32."""
    own, final = tuner_contract(F.HeadFineTuner, F.head_parameter_keys(3), ("keep_unit_out", "all_heads"), small[1], x, monkeypatch)
    for n, k in enumerate(LOSSES):
        err, allowed = abs(float(own[k]) - float(final[k])), MARGIN * FORWARD_DISTANCE * abs(float(final[k]))
        print(k, "x3 schedule", float(own[k]), "fp32 arms", float(final[k]), "difference", err, "allowed", allowed)
        assert err <= allowed, (k, err, allowed)
