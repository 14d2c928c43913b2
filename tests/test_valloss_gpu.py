"""GPU suite of the validation loss: smap_loss_forward_src alone on synthetic sources, the all-heads engine against the native head
tensors of the imported reference (tests/golden/valloss_small.npz), SMAP.forward(imgs, valids, labels, rdepth) against the reference's
float64 loss, and test.py --eval_loss 1."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_scenes as LS
import valloss_inputs as VI
from helpers import make_cfg
from recipe import recipe_state_dict
from train_kit import small_net, source_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("heatmap_2d", "det_d", "root_d")
CHANNELS = (43, 14, 1)
LOSSES = ("total_loss", "loss_2d", "loss_bone", "loss_root")
U = 2.0 ** -24


# ---- the reduction alone ---------------------------------------------------------------------------------------------------------
# scene of loss_scenes.py (labels, masks, rows), source sizes of heads j = 0..3, and which tensors are NCHW instead of padded NHWC
CASES = {"A": dict(scene="vector", sizes=[(2, 3), (4, 6), (8, 12), (16, 24)], nchw={(5, 0), (6, 1), (2, 2), (11, 2)}),
         "B": dict(scene="scalar", sizes=[(1, 1), (1, 3), (3, 2), (9, 11)], nchw={(3, 0), (3, 2)})}


class Sources:
    """Random native head tensors of a case on the device, their descriptors, and torch's own upsampling of them."""

    def __init__(self, case):
        from smap_amd.engine import HeadSource
        spec = CASES[case]
        s = self.scene = LS.SCENES[spec["scene"]]
        x = LS.inputs(spec["scene"])
        self.B, self.H, self.W, self.n_heads = s["B"], s["H"], s["W"], 4 * s["stage_num"]
        rng = np.random.RandomState(909 + ord(case))
        self.hold, self.desc, self.nchw, self.up = [], [], [], []
        for h in range(self.n_heads):
            sh, sw = spec["sizes"][h % 4]
            d, ups = {}, []
            for k, (key, c) in enumerate(zip(KEYS, CHANNELS)):
                v = torch.from_numpy((rng.standard_normal((self.B, c, sh, sw)) * (1 + 0.1 * h)).astype(np.float32)).to(DEV)
                if (h, k) in spec["nchw"]:
                    t = v.contiguous()
                    d[key] = HeadSource(t.data_ptr(), sh, sw, c, 1, sh * sw, c * sh * sw)
                else:                                    # NHWC, the pixel padded to a multiple of 8 channels with junk behind the last one
                    pad = (c + 7) // 8 * 8
                    t = torch.full((self.B, sh, sw, pad), 1e30, dtype=torch.float32, device=DEV)
                    t[..., :c] = v.permute(0, 2, 3, 1)
                    d[key] = HeadSource(t.data_ptr(), sh, sw, c, pad, 1, sh * sw * pad)
                self.hold.append(t)
                ups.append(F.interpolate(v, size=(self.H, self.W), mode="bilinear", align_corners=True) if (sh, sw) != (self.H, self.W) else v)
                self.nchw.append(v)
            self.desc.append(d)
            self.up.append(ups)
        self.labels, self.valids, self.rdepth = (torch.from_numpy(x[k]).to(DEV) for k in ("labels", "valids", "rdepth"))
        self.R = self.rdepth.shape[1]

    def cfg(self, B=None):
        from smap_amd.loss import _Config
        s = self.scene
        return _Config(s["stage_num"], s["ohkm"], s["topk"], s["ctf"], 0, self.B if B is None else B, s["S"], self.R, self.H, self.W)

    def run(self):
        from smap_amd.loss import forward_from_sources, workspace_views
        result, ws = forward_from_sources(self.cfg(), self.desc, self.labels, self.valids, self.rdepth)
        return result, workspace_views(ws, self.n_heads, self.B, self.R)


@pytest.fixture(scope="module", params=["A", "B"])
def sources(request):
    return Sources(request.param)


def test_reduce_from_sources_matches_torch_upsampling_within_the_rounding_bound(sources):
    """sums [n_heads][B][57] against numpy float64 over d = fp32(v) - label (the fp32 subtraction the kernels do), v torch's fp32
    F.interpolate(align_corners=True) of the same source on the device.  Bound per channel, computed here: sum over the pixels of
    2 |d| eps + eps^2 with eps = 4 * 2^-24 * max |source| -- four fp32 roundings of the six-multiply tap expression, any contraction.
    root_d at the rows' cells within eps.  The losses against SMAPLoss on the upsampled maps: 5e-7 relative (DESIGN section 13's figure)
    plus the same bounds carried through the finish, which is linear in the sums once the selection is fixed."""
    from smap_amd.loss import SMAPLoss, forward_raw, workspace_views
    S = sources
    result, v = S.run()
    sums = v["sums"].cpu().numpy()
    want, bound = np.zeros_like(sums), np.zeros_like(sums)
    for h in range(S.n_heads):
        lab = S.labels[:, LS.head_scale(S.scene, h)][:, LS.LABEL_CHANNEL].cpu().numpy()
        up = torch.cat(S.up[h][:2], 1).cpu().numpy()
        d = (up - lab).astype(np.float64)                                        # fp32 subtraction, as the kernels round it
        want[h] = (d * d).sum(axis=(2, 3))
        eps = np.concatenate([np.full(c, 4 * U * float(S.nchw[3 * h + k].abs().max())) for k, c in enumerate(CHANNELS[:2])])[None, :, None, None]
        bound[h] = (2 * np.abs(d) * eps + eps * eps).sum(axis=(2, 3))
    print("sums: worst error / bound", float((np.abs(sums - want) / bound).max()))
    assert (np.abs(sums - want) <= bound).all()
    # root_d at the rows' cells
    rd_at, cells = v["rd_at"].cpu().numpy(), v["root_cell"].cpu().numpy()
    rows, eps_root, counted = S.rdepth.cpu().numpy(), np.zeros(S.n_heads), 0
    for h in range(S.n_heads):
        up = S.up[h][2].cpu().numpy()
        eps_root[h] = 4 * U * float(S.nchw[3 * h + 2].abs().max())
        for b in range(S.B):
            for r in range(S.R):
                y, x, z = rows[b, r]
                if z > 0:
                    assert cells[h, b, r] == int(y) * S.W + int(x)
                    assert abs(float(rd_at[h, b, r]) - float(up[b, 0, int(y), int(x)])) <= eps_root[h]
                    counted += 1
                else:
                    assert cells[h, b, r] == -1 and rd_at[h, b, r] == 0
    assert counted >= S.n_heads
    # the four values against SMAPLoss on the upsampled maps
    nest = lambda k: [[S.up[4 * i + j][k].contiguous() for j in range(4)] for i in range(S.scene["stage_num"])]
    crit = SMAPLoss(S.scene["stage_num"], S.scene["ohkm"], S.scene["topk"], S.scene["ctf"])
    cfg, tensors, labels, valids, rdepth = crit._check(dict(heatmap_2d=nest(0), det_d=nest(1), root_d=nest(2)), S.valids, S.labels, S.rdepth)
    ref, ws = forward_raw(cfg, tensors, labels, valids, rdepth)
    rv = workspace_views(ws, S.n_heads, S.B, S.R)
    assert torch.equal(rv["sel"], v["sel"]), "the same channels are mined"
    half = rv["coef"].cpu().numpy().astype(np.float64) / 2                       # d total / d sums
    fine = np.array([h % 4 == 3 for h in range(S.n_heads)])
    w_head = np.where(fine, 1.0, 0.25)
    carried = np.array([(half * bound).sum() + 10 * (w_head * eps_root).sum(),
                        (half[fine, :, :43] * bound[fine, :, :43]).sum() / 0.1, (half[fine, :, 43:] * bound[fine, :, 43:]).sum() / 5,
                        eps_root[fine].sum()])
    got, ref = result.cpu().numpy().astype(np.float64), ref.cpu().numpy().astype(np.float64)
    print("losses", got[:4], "reference", ref[:4], "allowed", 5e-7 * np.abs(ref[:4]) + carried)
    assert (np.abs(got[:4] - ref[:4]) <= 5e-7 * np.abs(ref[:4]) + carried).all() and got[4] == ref[4] == 0


def test_reduce_from_sources_same_bits_and_frame_independent(sources):
    """Two runs give the same bits (fixed-order folds, no atomics); a frame's sums and root reads in the batch are those of the frame
    run alone (pointers moved to it); one run under torch's synchronisation debug mode: the entry point never waits for the device."""
    from smap_amd.engine import HeadSource
    from smap_amd.loss import forward_from_sources, workspace_views
    S = sources
    r0, v0 = S.run()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r1, v1 = S.run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(r0.view(torch.int32), r1.view(torch.int32))
    for k in ("sums", "rd_at", "root_cell", "m", "sel"):
        assert torch.equal(v0[k], v1[k]), k
    for b in range(S.B):
        desc = [{key: HeadSource(s.ptr + 4 * b * s.frame_stride, *s[1:]) for key, s in d.items()} for d in S.desc]
        _, ws = forward_from_sources(S.cfg(1), desc, S.labels[b:b + 1].contiguous(), S.valids[b:b + 1].contiguous(), S.rdepth[b:b + 1].contiguous())
        v = workspace_views(ws, S.n_heads, 1, S.R)
        assert torch.equal(v["sums"][:, 0], v0["sums"][:, b]) and torch.equal(v["rd_at"][:, 0], v0["rd_at"][:, b]), b


def test_forward_src_argument_errors(sources):
    from smap_amd import lib as L
    from smap_amd.loss import source_workspace_bytes
    S = sources
    lib = L.load()
    n = 3 * S.n_heads
    bytes_ = source_workspace_bytes(S.n_heads, S.B, S.R, S.H, S.W)
    assert lib.smap_loss_src_workspace_bytes(S.n_heads, S.B, S.R, S.H, S.W) == bytes_
    assert lib.smap_loss_src_workspace_bytes(17, S.B, S.R, S.H, S.W) == -1 and lib.smap_loss_src_workspace_bytes(12, S.B, S.R, 0, S.W) == -1
    ws = torch.zeros(bytes_, dtype=torch.uint8, device=DEV)
    res = torch.zeros(8, dtype=torch.float32, device=DEV)

    def call(edit=None, labels=S.labels, valids=S.valids, rdepth=S.rdepth, srcs=True, wsp=ws.data_ptr(), wsb=bytes_, result=res.data_ptr(),
             S_=S.scene["S"], H=S.H, W=S.W):
        arr = (L.HeadSrc * n)()
        for h, d in enumerate(S.desc):
            for k, key in enumerate(KEYS):
                s = d[key]
                arr[3 * h + k] = L.HeadSrc(s.ptr, s.h, s.w, s.c, s.pix_stride, s.ch_stride, 0, s.frame_stride)
        if edit:
            edit(arr)
        sc = S.scene
        ptr = lambda t: None if t is None else t.data_ptr()
        return lib.smap_loss_forward_src(arr if srcs else None, ptr(labels), ptr(valids), ptr(rdepth), sc["stage_num"], int(sc["ohkm"]), sc["topk"],
                                         int(sc["ctf"]), S.B, S_, S.R, H, W, wsp, wsb, result, torch.cuda.current_stream().cuda_stream)

    def setter(i, **kw):
        def edit(arr):
            for k, val in kw.items():
                setattr(arr[i], k, val)
        return edit

    assert call() == 0
    bad = [dict(srcs=False), dict(labels=None), dict(valids=None), dict(rdepth=None), dict(wsp=None), dict(result=None), dict(wsb=bytes_ - 8),
           dict(wsp=ws.data_ptr() + 4), dict(S_=4), dict(edit=setter(0, ptr=None)), dict(edit=setter(4, ptr=S.desc[1]["det_d"].ptr + 2)),
           dict(edit=setter(0, h=0)), dict(edit=setter(1, w=-1)), dict(edit=setter(9, h=S.H + 1)), dict(edit=setter(9, w=S.W + 1)),
           dict(edit=setter(0, c=42)), dict(edit=setter(1, c=43)), dict(edit=setter(2, c=0)), dict(edit=setter(0, pix_stride=0)),
           dict(edit=setter(0, ch_stride=0)), dict(edit=setter(0, frame_stride=0)), dict(edit=setter(0, pix_stride=42, ch_stride=1)),
           dict(edit=setter(0, pix_stride=2, ch_stride=3)), dict(H=S.H - 1) if S.H > 1 else dict(H=0)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()


# ---- the all-heads engine --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return small_net(precision=None)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(f"{golden_dir}/valloss_small.npz")


@pytest.fixture(scope="module")
def x(golden_dir):
    return torch.from_numpy(np.load(f"{golden_dir}/backbone_small.npz")["x"]).to(DEV)


@pytest.mark.parametrize("taphead", ["1", "0"], ids=["tapdot_root", "plain_root"])
def test_all_heads_engine_native_heads_match_the_reference(small, golden, x, monkeypatch, taphead):
    """precision x3, 2 x 64 x 96, an arena that reuses nothing: each of the 36 native head tensors of frame 1 within 2e-5 * max of the
    reference's (test_small_schedule_split_precision_every_tensor's bound), frame 0 through its sum and abs-sum within 2e-5 of the
    abs-sum.  With a reusing arena the loss is the same bits: no head tensor was handed to a later op."""
    from smap_amd.engine import BackboneEngine
    from smap_amd.loss import EngineLoss
    monkeypatch.setenv("SMAP_TAPHEAD", taphead)
    _, sd = small
    inp = {k: torch.from_numpy(v).to(DEV) for k, v in VI.inputs("coco").items()}
    results = {}
    for reuse in (False, True):
        eng = BackboneEngine(sd, 2, 64, 96, DEV, reuse=reuse, precision="x3", all_heads=True)
        out = eng.new_output()
        eng.run(x, out=out)
        src = eng.head_sources(out)
        results[reuse], _ = EngineLoss().raw(src, inp["valids"], inp["labels"], inp["rdepth"])
        if reuse:
            continue
        worst = 0.0
        for h, d in enumerate(src):
            for k, key in enumerate(KEYS):
                t = eng.graph.head_tensors[(h // 4, h % 4)][key]
                got = source_tensor(eng, d[key], out)
                if t is not None:
                    assert torch.equal(got, eng.read_tensor(t.name).permute(0, 3, 1, 2)[:, :CHANNELS[k]]), "the descriptor addresses the tensor"
                got = got.double().cpu().numpy()
                want = golden["h%d_%d" % (h, k)].astype(np.float64)
                worst = max(worst, np.abs(got[1] - want).max() / np.abs(want).max())
                assert np.abs(got[1] - want).max() <= 2e-5 * np.abs(want).max(), (h, key)
                i = 3 * h + k
                assert abs(got[0].sum() - golden["sum0"][i]) <= 2e-5 * golden["abs0"][i], (h, key)
                assert abs(np.abs(got[0]).sum() - golden["abs0"][i]) <= 2e-5 * golden["abs0"][i], (h, key)
        print("native heads: worst relative error", worst)
    assert torch.isfinite(results[True][:4]).all() and torch.equal(results[True].view(torch.int32), results[False].view(torch.int32))


@pytest.mark.parametrize("kw", [dict(), dict(scaled_hms=True), dict(flip_pair=True)], ids=["plain", "scaled_hms", "flip_pair"])
def test_all_heads_engine_leaves_the_inference_outputs_bit_equal(small, x, kw):
    from exps.stage3_root2.config import cfg                                    # (the configuration's flip order)
    from smap_amd.engine import BackboneEngine
    _, sd = small
    if kw.get("flip_pair"):
        kw = dict(flip_pair=list(cfg.DATASET.KEYPOINT.FLIP_ORDER) + [cfg.DATASET.KEYPOINT.NUM + c for c in cfg.DATASET.PAF.FLIP_CHANNEL])
    outs = []
    for all_heads in (False, True):
        eng = BackboneEngine(sd, 2, 64, 96, DEV, precision="x3", all_heads=all_heads, **kw)
        buf = eng.new_output()
        eng.run(x, out=buf)
        outs.append(buf)
        if all_heads and "flip_pair" in kw:
            assert all(t.B == 4 for d in eng.graph.head_tensors.values() for t in d.values() if t is not None)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "hms | det_d | root_d | status words"
    assert outs[0][:eng.out_floats].abs().max() > 0


# ---- SMAP.forward ----------------------------------------------------------------------------------------------------------------
def test_forward_with_labels_matches_the_reference_loss(small, golden, x):
    """Each of the four values within 1.5 * 2e-5 * S of the reference's float64 loss -- S the fixture's first-order sensitivity to a
    relative perturbation of the native head tensors (2e-5: the engine's bound on them), half again for the second-order term; both
    cases.  The same bits twice, forward(x) unchanged afterwards, training mode raises, f16 runs and is finite."""
    net, _ = small
    net.precision = "x3"
    before = [t.clone() for t in net(x)]
    for case in VI.CASES:
        inp = {k: torch.from_numpy(v).to(DEV) for k, v in VI.inputs(case).items()}
        got = net(x, inp["valids"][:, :, None], inp["labels"], inp["rdepth"])
        again = net(x, inp["valids"], inp["labels"], inp["rdepth"])
        assert list(got) == list(LOSSES)
        for n, k in enumerate(LOSSES):
            assert got[k].dim() == 0 and got[k].is_cuda and got[k].grad_fn is None and not got[k].requires_grad
            assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), k
            err, allowed = abs(float(got[k]) - golden[case + "_losses"][n]), 1.5 * 2e-5 * golden[case + "_S"][n]
            print(case, k, "value", float(got[k]), "error", err, "allowed", allowed)
            assert err <= allowed, (case, k, err, allowed)
    after = net(x)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    inp = {k: torch.from_numpy(v).to(DEV) for k, v in VI.inputs("ones").items()}
    with pytest.raises(RuntimeError, match="batch statistics"):
        net.train()(x, inp["valids"], inp["labels"], inp["rdepth"])
    net.eval()
    with pytest.raises(ValueError, match="labels must be"):
        net(x, inp["valids"], inp["labels"][:, :, :, :8].contiguous(), inp["rdepth"])
    net.precision = "f16"
    try:
        f16 = net(x, inp["valids"], inp["labels"], inp["rdepth"])
        vals = [float(f16[k]) for k in LOSSES]
        print("f16 relative deviation", [abs(v - g) / g for v, g in zip(vals, golden["ones_losses"])])
        assert all(np.isfinite(vals))
    finally:
        net.precision = "x3"


# ---- command line -----------------------------------------------------------------------------------------------------------------
def test_cli_eval_loss_on_both_loaders(tmp_path, monkeypatch):
    """`test.py -t generate_result --eval_loss 1` on the three annotated frames of the existing CLI tests, batch 2 (a ragged last
    batch): error['loss'] counts 3 frames in 2 batches, its values are the frame-weighted means of a direct SMAP.forward over the same
    batches, the device loader writes the same, and the records are those of a run without the flag."""
    from model.smap import SMAP
    from smap_amd.loss import ValidationLoss
    from test_entry_gpu import _annotated_set
    monkeypatch.setenv("SMAP_NO_TILE_TABLE", "1")
    torch.manual_seed(0)
    net = SMAP(make_cfg((128, 208))).eval()
    sd = recipe_state_dict(net.state_dict())
    for k in list(sd):
        if k.endswith("up4.res_conv2.bn.bias"):
            sd[k] = sd[k] + 40.0
    net.load_state_dict(sd)
    net = net.to(DEV)
    torch.save({"model": sd}, tmp_path / "SMAP.pth")
    from exps.stage3_root2.config import cfg
    keep = (cfg.TEST.ROOT_PATH, cfg.TEST.JSON_PATH, cfg.TEST.IMG_PER_GPU)
    try:
        root = _annotated_set(tmp_path, net, DEV, [(512, 832), (480, 640), (1080, 1920), (2048, 2048), (600, 800)], seed=11)
        from lib.utils.dataloader import get_test_loader
        cfg.TEST.IMG_PER_GPU = 2
        direct = ValidationLoss(net, cfg, DEV)
        for imgs, meta_data, _, scales in get_test_loader(cfg, num_gpu=1, local_rank=0, stage="test"):
            direct.update(imgs.to(DEV).float().contiguous(), meta_data, scales)
        want = direct.result_entry()["loss"]
    finally:
        cfg.TEST.ROOT_PATH, cfg.TEST.JSON_PATH, cfg.TEST.IMG_PER_GPU = keep
    del net
    assert want["frames"] == 3 and want["batches"] == 2 and all(np.isfinite(want[k]) and want[k] > 0 for k in LOSSES)
    env = dict(os.environ, PROJECT_HOME=str(tmp_path), SMAP_TEST_ROOT=str(root), SMAP_NO_TILE_TABLE="1", SMAP_DECODE_THREADS="3",
               SMAP_PLAN_CACHE=str(tmp_path / "plan_cache"), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, os.path.join(ROOT, "exps", "stage3_root2", "test.py"), "-p", str(tmp_path / "SMAP.pth"),
           "-t", "generate_result", "-d", "test", "--batch_size", "2"]
    docs = {}
    for tag, flags in (("loss", ["--eval_loss", "1"]), ("dev", ["--eval_loss", "1", "--eval_3d", "1", "--device_preprocess", "1"]), ("plain", [])):
        r = subprocess.run(cmd + ["--json_name", tag] + flags, capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        docs[tag] = json.loads((tmp_path / "model_logs" / "stage3_root2" / "result" / f"stage3_root2_generate_result_test_{tag}.json").read_text())
        assert ("validation loss over 3 frames in 2 batches" in r.stderr) == (tag != "plain")
    assert list(docs["loss"]["error"]) == ["loss"] and list(docs["loss"]["error"]["loss"]) == list(LOSSES) + ["frames", "batches"]
    assert docs["loss"]["error"]["loss"] == want
    assert list(docs["dev"]["error"])[-1] == "loss"
    # the device loader resizes with the GPU's arithmetic: its frames differ in the last bits, so does the loss
    for k in LOSSES:
        assert abs(docs["dev"]["error"]["loss"][k] - want[k]) <= 1e-3 * want[k], k
    assert docs["dev"]["error"]["loss"]["frames"] == 3 and docs["dev"]["error"]["loss"]["batches"] == 2
    assert "error" not in docs["plain"] and len(docs["plain"]["3d_pairs"]) >= 1
    assert docs["loss"]["3d_pairs"] == docs["plain"]["3d_pairs"]
