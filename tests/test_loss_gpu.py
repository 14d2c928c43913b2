"""GPU: the training loss (csrc/loss.hip smap_loss_forward / smap_loss_backward, smap_amd/loss.py, lib/utils/loss_h.py) against
tests/golden/loss.npz -- the reference's SMAP._calculate_loss executed in float64 on the same fp32 inputs, and autograd through it
(tests/golden/gen_golden_loss.py).

Tolerances, from the arithmetic alone:
  losses     5e-7 relative.  Every term carries at most 2^-24 from the fp32 subtraction, doubled by the square; everything after is
             double; one final fp32 rounding adds 2^-24.  All terms are non-negative, so nothing cancels: < 2^-22 ~ 2.4e-7, and a
             factor 2 for the divisions' orders.
  gradients  5e-7 relative, elementwise, of coef * upstream * (out - label) in float64: the fp32 subtraction, the fp32 factor, its
             product with the upstream gradient and the final product round once each.  Where the reference is 0 the result is 0."""
import os

import numpy as np
import pytest
import torch

import loss_scenes as LS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NC, N2D, NDD = 57, 43, 14
RTOL = 5e-7


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "loss.npz"))


def criterion(s, **kw):
    from smap_amd.loss import SMAPLoss
    return SMAPLoss(stage_num=s["stage_num"], ohkm=s["ohkm"], topk=s["topk"], ctf=s["ctf"], **kw)


def to_device(name, requires_grad=True):
    """The scene's inputs on the device: (outputs dict of leaves, valids [B, 57, 1], labels, rdepth, the flat list of leaves)."""
    s, x = LS.SCENES[name], LS.inputs(name)
    leaf = lambda a: torch.from_numpy(a).to(DEV).requires_grad_(requires_grad)
    nest = lambda ts: [ts[4 * i:4 * i + 4] for i in range(s["stage_num"])]
    hm, dd, rd = [leaf(a) for a in x["hm"]], [leaf(a) for a in x["dd"]], [leaf(a) for a in x["rd"]]
    outputs = dict(heatmap_2d=nest(hm), det_d=nest(dd), root_d=nest(rd))
    dev = lambda a: torch.from_numpy(a).to(DEV)
    return outputs, dev(x["valids"])[:, :, None], dev(x["labels"]), dev(x["rdepth"]), (hm, dd, rd)


def run(name):
    """Forward and backward (through total_loss * upstream) once: (losses [4] fp32, per head the gradients as numpy)."""
    s = LS.SCENES[name]
    outputs, valids, labels, rdepth, (hm, dd, rd) = to_device(name)
    got = criterion(s)(outputs, valids, labels, rdepth)
    assert set(got) == {"total_loss", "loss_2d", "loss_bone", "loss_root"}
    assert got["total_loss"].requires_grad and not any(got[k].requires_grad for k in ("loss_2d", "loss_bone", "loss_root"))
    (got["total_loss"] * s["upstream"]).backward()
    losses = np.array([got[k].item() for k in ("total_loss", "loss_2d", "loss_bone", "loss_root")], np.float32)
    grads = [[t.grad.cpu().numpy() for t in ts] for ts in (hm, dd, rd)]
    return losses, grads


_runs = {}


def first_run(name):
    if name not in _runs:
        _runs[name] = run(name)
    return _runs[name]


@pytest.mark.parametrize("name", list(LS.SCENES))
def test_losses_and_gradients_equal_the_reference(name, golden):
    s, x = LS.SCENES[name], LS.inputs(name)
    losses, (ghm, gdd, grd) = first_run(name)
    want = golden[name + "_losses"]
    err = np.abs(losses.astype(np.float64) - want) / np.where(want == 0, 1, np.abs(want))
    print(name, "losses", losses, "reference", want, "relative error", err)
    assert (err <= RTOL).all(), (losses, want)
    # dense gradients: coef (upstream folded in) * the exact difference
    d = LS.differences(name, x)
    worst = 0.0
    for h in range(4 * s["stage_num"]):
        ref = golden[name + "_coef"][h][:, :, None, None] * d[h]
        got = np.concatenate([ghm[h], gdd[h]], axis=1).astype(np.float64)
        assert (got[ref == 0] == 0).all(), h
        live = ref != 0
        e = np.abs(got[live] - ref[live]) / np.abs(ref[live])
        worst = max(worst, float(e.max()) if e.size else 0.0)
    print(name, "dense gradients: worst relative error", worst)
    assert worst <= RTOL
    # root_d: the fixture's entries, exactly 0 elsewhere
    ref = np.zeros((4 * s["stage_num"], s["B"], 1, s["H"], s["W"]))
    for (h, b, y, xx), v in zip(golden[name + "_rd_idx"], golden[name + "_rd_val"]):
        ref[h, b, 0, y, xx] = v
    got = np.stack(grd).astype(np.float64)
    assert (got[ref == 0] == 0).all()
    e = np.abs(got - ref)[ref != 0] / np.abs(ref[ref != 0])
    print(name, "root_d gradients: entries", int((ref != 0).sum()), "worst relative error", float(e.max()) if e.size else 0.0)
    assert (e <= RTOL).all()


@pytest.mark.parametrize("name", ["scalar", "vector"])
def test_two_runs_give_the_same_bits(name):
    a, b = first_run(name), run(name)
    assert a[0].tobytes() == b[0].tobytes()
    for ga, gb in zip(a[1], b[1]):
        for ta, tb in zip(ga, gb):
            assert ta.tobytes() == tb.tobytes()


@pytest.mark.parametrize("name", ["scalar", "vector"])
def test_a_batch_is_its_frames_alone(name):
    """sums [n_heads, B, 57] of the batch = the sums of every frame run alone, bit for bit: a plane's sum depends on the plane only."""
    from smap_amd import loss as K
    s = LS.SCENES[name]
    outputs, valids, labels, rdepth, (hm, dd, rd) = to_device(name, requires_grad=False)
    n_heads, B, R = 4 * s["stage_num"], s["B"], rdepth.shape[1]
    flat = [t for h in range(n_heads) for t in (hm[h], dd[h], rd[h])]

    def sums(tensors, labels, valids, rdepth):
        cfg = K._Config(s["stage_num"], s["ohkm"], s["topk"], s["ctf"], 0, labels.shape[0], labels.shape[1], R, s["H"], s["W"])
        _, ws = K.forward_raw(cfg, tensors, labels, valids, rdepth)
        return K.workspace_views(ws, n_heads, labels.shape[0], R)["sums"].cpu().numpy()

    whole = sums(flat, labels, valids[:, :, 0].contiguous(), rdepth)
    assert whole.shape == (n_heads, B, NC) and (whole > 0).all()
    for b in range(B):
        alone = sums([t[b:b + 1] for t in flat], labels[b:b + 1], valids[b:b + 1, :, 0].contiguous(), rdepth[b:b + 1])
        assert alone.tobytes() == np.ascontiguousarray(whole[:, b:b + 1]).tobytes(), b
    # and they are the float64 sums of the fp32 differences, up to the order of the additions
    want = LS.host_sums(name, LS.inputs(name), np.float32)
    assert (np.abs(whole - want) <= 1e-12 * want).all()


def test_strided_inputs_equal_their_contiguous_copies():
    name = "vector"
    s = LS.SCENES[name]
    outputs, valids, labels, rdepth, (hm, dd, rd) = to_device(name)
    wide = torch.zeros((s["B"], N2D, s["H"], 2 * s["W"]), device=DEV)
    wide[..., ::2] = hm[7].detach()
    strided = wide[..., ::2].requires_grad_(True)
    assert not strided.is_contiguous()
    outputs["heatmap_2d"][1][3] = strided
    tall = torch.zeros((s["B"], 2 * s["S"], NC, s["H"], s["W"]), device=DEV)
    tall[:, ::2] = labels
    got = criterion(s)(outputs, valids, tall[:, ::2], rdepth)
    got["total_loss"].backward()
    losses, (ghm, _, _) = first_run(name)
    assert got["total_loss"].item() == losses[0] and got["loss_2d"].item() == losses[1]
    assert strided.grad.cpu().numpy().tobytes() == ghm[7].tobytes()


def test_single_head_modules_of_the_reference_import_path(golden):
    """JointsL2Loss / DepthLoss of lib.utils.loss_h on head 11 of the first scene: what the reference's own calls returned."""
    from lib.utils.loss_h import DepthLoss, JointsL2Loss
    name, h = "scalar", 11
    s, x = LS.SCENES[name], LS.inputs(name)
    want = golden[name + "_per_head"][h]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    lab = x["labels"][:, LS.head_scale(s, h)][:, LS.LABEL_CHANNEL]
    valid = dev(x["valids"])[:, :, None]
    hm, dd, rd = dev(x["hm"][h]).requires_grad_(True), dev(x["dd"][h]).requires_grad_(True), dev(x["rd"][h]).requires_grad_(True)
    l2d = JointsL2Loss(has_ohkm=True, topk=s["topk"], paf_num=14)(hm, valid[:, :N2D], dev(lab[:, :N2D]))
    l3d = JointsL2Loss(has_ohkm=True, topk=s["topk"], paf_num=0)(dd, valid[:, N2D:], dev(lab[:, N2D:]))
    lrd = DepthLoss()(rd, dev(x["rdepth"]))
    got = np.array([l2d.item(), l3d.item(), lrd.item()], np.float64)
    print("head", h, got, "reference", want)
    assert (np.abs(got - want) <= RTOL * np.abs(want)).all()
    # their gradients are the network loss's with its weights (0.1, 5, 10; head 11 is a finest head) taken out
    (l2d + l3d + lrd).backward()
    d = LS.differences(name, x)[h]
    coef = golden[name + "_coef"][h] / np.r_[np.full(N2D, 0.1), np.full(NDD, 5.0)]
    ref = coef[:, :, None, None] * d
    got = np.concatenate([hm.grad.cpu().numpy(), dd.grad.cpu().numpy()], axis=1).astype(np.float64)
    assert (got[ref == 0] == 0).all() and (np.abs(got - ref)[ref != 0] <= RTOL * np.abs(ref[ref != 0])).all()
    ref = np.zeros((s["B"], 1, s["H"], s["W"]))
    for (hh, b, y, xx), v in zip(golden[name + "_rd_idx"], golden[name + "_rd_val"]):
        if hh == h:
            ref[b, 0, y, xx] = v / 10.0
    got = rd.grad.cpu().numpy().astype(np.float64)
    assert (got[ref == 0] == 0).all() and (np.abs(got - ref)[ref != 0] <= RTOL * np.abs(ref[ref != 0])).all()
    # plain means (no OHKM) of the same head, against numpy on the fp32 differences
    plain = JointsL2Loss()(hm.detach(), valid[:, :N2D], dev(lab[:, :N2D])).item()
    m = (LS.differences(name, x, np.float32)[h].astype(np.float64) ** 2).mean(axis=(2, 3))[:, :N2D]
    assert abs(plain - m.mean()) <= RTOL * m.mean()


def test_rendered_labels_as_outputs_give_zero(golden_dir):
    """render_labels feeds SMAPLoss; outputs equal to the labels' own channels at every head's supervising scale: total 0, gradients 0."""
    from labels_restate import KERNELS, LIMBS
    from smap_amd.labels import LabelSpec, render_labels
    z = np.load(os.path.join(golden_dir, "labels.npz"))
    name = next(str(n) for n in z["names"] if tuple(z[str(n) + "_shape"]) == (17, 23) and len(z[str(n) + "_bodys"]) >= 2)
    bodys = z[name + "_bodys"]
    spec = LabelSpec(tuple(KERNELS), tuple(LIMBS), 1, 4, (17, 23), 2, 20)
    labels = render_labels([bodys, bodys[:0]], spec, device=DEV)
    assert tuple(labels.shape) == (2, 5, NC, 17, 23) and float(labels.abs().max()) > 1
    s = LS.SCENES["scalar"]
    index = torch.tensor(LS.LABEL_CHANNEL, device=DEV)
    hm, dd, rd = [], [], []
    for h in range(12):
        own = labels[:, LS.head_scale(s, h)].index_select(1, index)
        hm.append(own[:, :N2D].clone().requires_grad_(True))
        dd.append(own[:, N2D:].clone().requires_grad_(True))
        rd.append(torch.full((2, 1, 17, 23), 1.5, device=DEV).requires_grad_(True))
    nest = lambda ts: [ts[4 * i:4 * i + 4] for i in range(3)]
    rdepth = torch.zeros((2, 20, 3), device=DEV)
    rdepth[0, 0] = torch.tensor([4.25, 7.5, 1.5])
    got = criterion(s, strict=True)(dict(heatmap_2d=nest(hm), det_d=nest(dd), root_d=nest(rd)), torch.ones((2, NC, 1), device=DEV), labels, rdepth)
    got["total_loss"].backward()
    assert all(got[k].item() == 0 for k in got)
    assert all(float(t.grad.abs().max()) == 0 for ts in (hm, dd, rd) for t in ts)


def test_no_host_synchronisation():
    """Forward and backward under torch's synchronisation debug mode: any blocking call raises."""
    assert hasattr(torch.cuda, "set_sync_debug_mode")
    name = "vector"
    s = LS.SCENES[name]
    outputs, valids, labels, rdepth, (hm, dd, rd) = to_device(name)
    crit = criterion(s)
    up = torch.tensor(1.0, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = crit(outputs, valids, labels, rdepth)
        (got["total_loss"] * up).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    losses, (ghm, _, _) = first_run(name)
    assert got["total_loss"].item() == losses[0] and hm[0].grad.cpu().numpy().tobytes() == ghm[0].tobytes()


def test_a_row_outside_the_map():
    """Never dereferenced: total NaN, the other terms and the gradients of the maps as before; strict=True raises instead."""
    name = "scalar"
    s = LS.SCENES[name]
    outputs, valids, labels, rdepth, (hm, dd, rd) = to_device(name)
    rdepth[1, 2] = torch.tensor([3.0e9, 4.0, 1.0])
    got = criterion(s)(outputs, valids, labels, rdepth)
    got["total_loss"].backward()
    losses, (ghm, _, grd) = first_run(name)
    assert np.isnan(got["total_loss"].item()) and got["loss_2d"].item() == losses[1] and got["loss_bone"].item() == losses[2]
    assert hm[3].grad.cpu().numpy().tobytes() == ghm[3].tobytes()
    assert np.isfinite(rd[3].grad.cpu().numpy()).all() and (rd[3].grad[1] == 0).all()
    with pytest.raises(ValueError, match="outside"):
        criterion(s, strict=True)(outputs, valids, labels, rdepth)


def test_input_rules_on_the_device():
    """A wrong shape names the head; a missing head is named too; the gradient is once differentiable."""
    name = "squeeze"
    s = LS.SCENES[name]
    crit = criterion(s)
    outputs, valids, labels, rdepth, (hm, dd, rd) = to_device(name)
    good = outputs["det_d"][0][2]
    outputs["det_d"][0][2] = torch.zeros((s["B"], NDD, s["H"], s["W"] + 1), device=DEV)
    with pytest.raises(ValueError, match=r"outputs\['det_d'\]\[0\]\[2\].*shape"):
        crit(outputs, valids, labels, rdepth)
    outputs["det_d"][0][2] = good[:, :13]
    with pytest.raises(ValueError, match=r"outputs\['det_d'\]\[0\]\[2\]"):
        crit(outputs, valids, labels, rdepth)
    outputs["det_d"][0][2] = good
    del outputs["root_d"][0][3]
    with pytest.raises(ValueError, match=r"outputs\['root_d'\]\[0\]\[3\] is missing"):
        crit(outputs, valids, labels, rdepth)
    outputs["root_d"][0].append(rd[3])
    with pytest.raises(ValueError, match="rdepth"):
        crit(outputs, valids, labels, rdepth[:, :, :2])
    with pytest.raises(ValueError, match="valids"):
        crit(outputs, valids[:, :56], labels, rdepth)
    with pytest.raises(ValueError, match="labels"):
        crit(outputs, valids, labels[:, :3], rdepth)
    with pytest.raises(TypeError, match=r"outputs\['heatmap_2d'\]\[0\]\[1\].*float32"):
        crit(dict(outputs, heatmap_2d=[[hm[0], hm[1].double(), hm[2], hm[3]]]), valids, labels, rdepth)
    total = crit(outputs, valids, labels, rdepth)["total_loss"]
    (g,) = torch.autograd.grad(total, hm[0], create_graph=True)
    assert not g.requires_grad                                # once differentiable: no graph hangs on the gradient ...
    with pytest.raises(RuntimeError):                        # ... so a second derivative is refused, not silently taken as zero
        g.sum().backward()
