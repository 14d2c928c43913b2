"""GPU: the MuPoTS-3D scorer (csrc/mupots.hip, smap_amd/mupots.py) against the restatement tests/mupots_restate.py on the constructed
scenes of tests/mupots_scenes.py (their docstring lists the edges) -- matching index, considered flag, errors, accumulators and tables
bit for bit, NaN by position -- and `test.py -t generate_result --eval_mupots ROOT` against `python -m smap_amd.evaluate --mupots`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mupots_restate as R
import mupots_scenes as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NJ = 15


@pytest.fixture(scope="module")
def scene():
    return S.build()


@pytest.fixture(scope="module")
def annotations(scene):
    from smap_amd.mupots import Annotations
    return Annotations([1, 2, 3], scene["seq_offset"], scene["gt_count"], scene["gt2d"], scene["gt3d"], scene["occ"])


@pytest.mark.parametrize("config", list(S.CONFIGS))
def test_constructed_scenes_equal_the_restatement(scene, annotations, config):
    """3 sequences of 1, 5 and 12 frames in one launch, in every mode."""
    from smap_amd.mupots import MuPoTSScorer
    relative, use_skel, matched_only = S.CONFIGS[config]
    rows, accs = R.score(scene["seq_offset"], scene["gt_count"], scene["gt2d"], scene["gt3d"], scene["occ"], S.restate_preds(scene),
                         relative, use_skel, matched_only)
    F, G = scene["gt2d"].shape[:2]
    w_match, w_considered, w_err, w_rootz = S.rows_arrays(rows, F, G)
    pose2d, pose3d = S.pose_dicts(scene)
    scorer = MuPoTSScorer(annotations, relative, use_skel, matched_only, device=DEV)
    res = scorer.score(pose2d, pose3d)                                        # f17 has no entry and no valid person: never looked up
    assert (res.match == w_match).all(), np.argwhere(res.match != w_match)
    assert (res.considered == w_considered).all()
    assert (np.isnan(res.errors) == np.isnan(w_err)).all() and S.same_bits(res.errors, w_err)
    assert S.same_bits(res.rootz, w_rootz)
    assert S.same_bits(res.acc, np.asarray(accs)), np.argwhere(res.acc != np.asarray(accs))[:10]
    want = R.tables(accs)

    def same(a, b, where):
        if isinstance(b, dict):
            for k in b:
                same(a[k], b[k], where + (k,))
        else:
            assert S.same_bits(np.asarray(a, np.float64), np.asarray(b, np.float64)), where
    same(res.tables, want, ())
    for f, m in scene["expect_match"].items():                                # the hand-known outcomes, on the device's own rows
        assert res.match[f, :len(m)].tolist() == m, f
    again = scorer.score(pose2d, pose3d)
    assert (again.match == res.match).all() and S.same_bits(again.errors, res.errors) and S.same_bits(again.acc, res.acc)
    if config == "absolute":
        assert np.isnan(res.tables["ordinal_rate"][0]) and np.isnan(res.tables["mean_ordinal_rate"])
        assert res.acc[1, 3:5].tolist() == [5.0, 6.0]
    if config == "no_skel":
        assert res.errors[10, 0, :14].tolist() == [150.0] * 14
    if config == "default":
        assert np.isnan(res.errors[9, 0]).nonzero()[0].tolist() == [3, 4] and res.acc[1, :3].tolist() == [9.0, 9.0, 3.0]


def test_scorer_through_the_loader_and_the_limits(tmp_path, scene, annotations):
    """The same scenes read from TS<k>/annot.mat + occlusion.mat give the same result; 16 valid persons are scored, 17 are refused on the
    host, and so is a frame that the predictions lack."""
    from smap_amd import mupots as M
    S.write_root(str(tmp_path), scene)
    pose2d, pose3d = S.pose_dicts(scene, ext=".png")
    a = M.MuPoTSScorer(M.load_annotations(str(tmp_path)), device=DEV).score(pose2d, pose3d)
    b = M.MuPoTSScorer(annotations, device=DEV).score(pose2d, pose3d)
    assert (a.match == b.match).all() and S.same_bits(a.errors, b.errors) and S.same_bits(a.acc, b.acc)
    assert b.match[15, :16].tolist() == list(range(15, -1, -1)) and b.considered[15].all()
    with pytest.raises(ValueError, match="at most 16"):
        M.MuPoTSScorer(M.Annotations([1], [0, 1], [17], np.zeros((1, 17, NJ, 2)), np.zeros((1, 17, NJ, 3)), np.zeros((1, 17, NJ))), device=DEV)
    del pose2d["TS2/img_000003.png"]
    with pytest.raises(ValueError, match="TS2/img_000003"):
        M.MuPoTSScorer(annotations, device=DEV).score(pose2d, pose3d)


def test_cli_eval_mupots_writes_the_summary_and_leaves_the_rest_alone(tmp_path, monkeypatch):
    """`test.py -t generate_result --eval_mupots ROOT` on the tiny annotated set of the other CLI tests, with a synthetic annotation
    root laid next to what the run predicts: error["mupots"] equals `python -m smap_amd.evaluate RESULT.json --mupots ROOT` on the file
    it wrote, and without that key the file is the file of a run without the flag, byte for byte."""
    from helpers import make_cfg
    from lib.eval.convert import convert_records
    from model.refinenet import RefineNet
    from model.smap import SMAP
    from recipe import recipe_state_dict
    from test_entry_gpu import _annotated_set
    import scipy.io as scio
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
    torch.save(recipe_state_dict(RefineNet().eval().state_dict()), tmp_path / "RefineNet.pth")
    root = _annotated_set(tmp_path, net, DEV, [(512, 832), (480, 640), (600, 800)], seed=11)
    del net
    env = dict(os.environ, PROJECT_HOME=str(tmp_path), SMAP_TEST_ROOT=str(root), SMAP_NO_TILE_TABLE="1",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, os.path.join(ROOT, "exps", "stage3_root2", "test.py"), "-p", str(tmp_path / "SMAP.pth"),
           "-rp", str(tmp_path / "RefineNet.pth"), "-t", "generate_result", "-d", "test", "--batch_size", "2"]
    out = lambda tag: tmp_path / "model_logs" / "stage3_root2" / "result" / f"stage3_root2_generate_result_test_{tag}.json"
    r = subprocess.run(cmd + ["--json_name", "plain"], capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    # the annotation root: frame TS<k>/img_<i> of the fixture is frame i of sequence k; its valid persons are the run's own predictions,
    # moved a little, plus one person nobody predicted; the frames in front of it hold no valid person
    pose3d, pose2d, _ = convert_records(json.loads(out("plain").read_text())["3d_pairs"])
    assert len(pose3d) >= 1
    order = np.asarray(R.SMAP_ORDER) - 1
    rng = np.random.default_rng(3)
    mroot = tmp_path / "mupots_root"
    for k in (1, 2, 3):
        name = "TS%d/img_%06d.npy" % (k, k - 1)
        p2 = np.asarray(pose2d.get(name, np.zeros((0, NJ, 4))))[:, order, :2]
        p3 = np.asarray(pose3d.get(name, np.zeros((0, NJ, 4))))[:, order, :3]
        n = min(len(p2), 3) if name in pose2d else 0
        K = n + 1 if name in pose2d else 1
        ann, occ = np.empty((k, K), dtype=object), np.empty((k, K), dtype=object)
        for i in range(k):
            for g in range(K):
                valid = i == k - 1 and name in pose2d
                a2, u3 = rng.normal(3000, 50, (2, 17)), rng.normal(0, 500, (3, 17)) + np.array([[0.0], [0.0], [3000.0]])
                if valid and g < n:
                    a2[:, :NJ], u3[:, :NJ] = p2[g].T + rng.normal(0, 3, (2, NJ)), p3[g].T + rng.normal(0, 40, (3, NJ))
                ann[i, g] = {"annot2": a2, "annot3": u3, "univ_annot3": u3, "isValidFrame": float(valid)}
                occ[i, g] = (rng.random((1, 17)) < 0.3).astype(np.float64)
        (mroot / ("TS%d" % k)).mkdir(parents=True)
        scio.savemat(mroot / ("TS%d" % k) / "annot.mat", {"annotations": ann})
        scio.savemat(mroot / ("TS%d" % k) / "occlusion.mat", {"occlusion_labels": occ})
    r = subprocess.run(cmd + ["--json_name", "mupots", "--eval_mupots", str(mroot)], capture_output=True, text=True, timeout=900, env=env,
                       cwd=str(tmp_path))
    assert r.returncode == 0 and "MuPoTS-3D: 3DPCK" in r.stderr, r.stderr[-3000:]
    doc = json.loads(out("mupots").read_text())
    assert list(doc["error"]) == ["mupots"] and doc["error"]["mupots"]["sequences"] == [1, 2, 3]
    assert sum(doc["error"]["mupots"]["annotated"]) >= 1
    r = subprocess.run([sys.executable, "-m", "smap_amd.evaluate", str(out("mupots")), "--mupots", str(mroot), "--out", str(tmp_path / "csv")],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and json.dumps(json.loads(r.stdout)) == json.dumps(doc["error"]["mupots"]), r.stderr[-2000:]
    assert len(os.listdir(tmp_path / "csv")) == 3
    del doc["error"]
    assert json.dumps(doc).encode() == out("plain").read_bytes()
