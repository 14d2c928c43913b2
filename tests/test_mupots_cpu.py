"""CPU: the MuPoTS-3D protocol (smap_amd/mupots.py, csrc/mupots_core.h) without a GPU -- the restatement pinned by cases that can be
worked out by hand, the annotation loader on files in the MuPoTS layout, the host twin of the kernels under sanitizers against the
restatement bit for bit, the table assembly, and the refusals of the two command lines."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import mupots_restate as R
import mupots_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NJ = 15


@pytest.fixture(scope="module")
def scene():
    return S.build()


@pytest.fixture(scope="module")
def restated(scene):
    """config name -> (rows, accs) of the restatement on the constructed scenes; computed once."""
    return {name: R.score(scene["seq_offset"], scene["gt_count"], scene["gt2d"], scene["gt3d"], scene["occ"], S.restate_preds(scene), *cfg)
            for name, cfg in S.CONFIGS.items()}


def _one_person(pred3_of, relative=True, use_skel=True):
    """One sequence, one frame, one person with integer coordinates and one prediction pred3_of(gt3) at the same pixels."""
    g2, g3 = S.person((800, 500), (300, -200, 3200))
    p3 = np.zeros((1, NJ, 4))
    p3[0, :, :3] = S.to_smap(pred3_of(g3))
    rows, accs = R.score([0, 1], [1], g2[None, None], g3[None, None], np.zeros((1, 1, NJ)), [(S.to_smap(g2)[None], p3)], relative, use_skel, False)
    return g3, rows[0][0], accs, R.tables(accs)


def test_restatement_prediction_equals_ground_truth():
    _, (match, considered, err, _), accs, t = _one_person(lambda g3: g3.copy())
    assert match == 0 and considered == 1 and err == [0.0] * NJ
    assert t["pck"][0] == [100.0] * 9 and t["mpjpe"][0] == [0.0] * 15
    assert t["auc"][0] == pytest.approx([100 * 30 / 31] * 9, rel=1e-15)           # threshold 0 is strict: 30 of the 31 thresholds hit
    assert accs[0][:5] == [1.0, 1.0, 0.0, 0.0, 0.0] and t["PCK15"] == [1.0] * NJ
    assert math.isnan(t["ordinal_rate"][0]) and math.isnan(t["mean_ordinal_rate"])


def test_restatement_scaled_prediction_with_and_without_bone_mapping():
    scaled = lambda g3: g3[14] + 2.0 * (g3 - g3[14])
    g3, (_, _, err, _), _, _ = _one_person(scaled, use_skel=True)
    assert max(err) < 1e-9                                                     # the bone directions are the ground truth's: lengths restored
    g3, (_, _, err, _), _, _ = _one_person(scaled, use_skel=False)
    rel = g3 - g3[14]
    want = [math.sqrt(((x * x) + (y * y)) + (z * z)) for x, y, z in rel.tolist()]   # |2 P_j - P_j| = |P_j|
    assert err == want and err[14] == 0.0


def test_restatement_error_of_exactly_150():
    def shifted(g3):
        p = g3.copy()
        p[:14] += np.array([90.0, 120.0, 0.0])
        return p
    _, (_, _, err, _), accs, t = _one_person(shifted, use_skel=False)
    assert err[:14] == [150.0] * 14 and err[14] == 0.0
    assert t["pck"][0] == [0.0] * 9                                            # < 150: a miss
    assert t["PCK15"] == [1.0] * NJ                                            # <= 150: a hit
    for j in range(14):
        assert accs[0][5 + 33 * j + 31] == 0.0 and accs[0][5 + 33 * j + 32] == 1.0
        assert accs[0][500 + 3 * j + 2] == 0.0 and accs[0][545 + 3 * j + 2] == 0.0     # not > 150 in either masked table
    assert t["visible"]["pck"][0][:15] == pytest.approx([1.0] * 15) and t["visible"]["pck"][0][15] == 14.0


def test_restatement_on_the_constructed_scenes(scene, restated):
    """What the scenes were built to show, read off the restatement's rows."""
    rows, accs = restated["default"]
    for f, want in scene["expect_match"].items():
        assert [r[0] for r in rows[f]] == want, f
    assert rows[1] == [] and rows[17] == []
    assert rows[5][1][2] != [100000.0] * NJ and all(e > 99000 for e in rows[5][1][2])      # the loser of the competition
    nan_at = [j for j, e in enumerate(rows[9][0][2]) if e != e]
    assert nan_at == [3, 4]                                                    # elbow (zero bone) and wrist (its descendant)
    assert accs[1][:3] == [9.0, 9.0, 3.0] and accs[0][:3] == [1.0, 1.0, 0.0]
    assert accs[2][545 + 3 * 3 + 2] >= 1.0 and accs[2][500 + 3 * 4 + 2] >= 1.0   # NaN -> 160 > 150: occluded elbow, visible wrist
    rows, accs = restated["matched_only"]
    assert accs[1][:3] == [6.0, 9.0, 3.0] and rows[5][1][1] == 0
    rows, accs = restated["no_skel"]
    assert rows[10][0][2][:14] == [150.0] * 14 and all(e == e for e in rows[9][0][2])
    rows, accs = restated["absolute"]
    t = R.tables(accs)
    # seq 1: f2 (two unmatched: pd difference 0, gt gap 1600 -> wrong), f3, f4 (3 pairs), f5 (one unmatched: 100000 is farther, and so is the gt)
    assert accs[1][3:5] == [5.0, 6.0] and accs[0][3:5] == [0.0, 0.0]
    per_frame = []
    for f in (11, 12, 13, 14):
        a = R.new_acc()
        R.fold_frame(a, rows[f], scene["occ"][f][:2].tolist(), False)
        per_frame.append(a[3:5])
    assert per_frame == [[1.0, 1.0], [1.0, 1.0], [0.0, 1.0], [0.0, 1.0]]
    assert math.isnan(t["ordinal_rate"][0]) and math.isnan(t["mean_ordinal_rate"]) and t["total_ordinal"][2] == 4 + 120 + 3


def test_loader_cuts_columns_drops_invalid_persons_and_keeps_order(tmp_path, scene):
    from smap_amd import mupots as M
    S.write_root(str(tmp_path), scene, sequences=(3, 11, 20))
    ann = M.load_annotations(str(tmp_path))
    assert ann.sequences == [3, 11, 20] and ann.seq_offset.tolist() == scene["seq_offset"].tolist()
    assert ann.gt_count.tolist() == scene["gt_count"].tolist() and ann.gt2d.shape == (18, 16, NJ, 2)
    for key in ("gt2d", "gt3d", "occ"):
        assert S.same_bits(getattr(ann, key), scene[key]), key
    assert ann.frame_names()[:3] == ["TS3/img_000000", "TS11/img_000000", "TS11/img_000001"]
    only = M.load_annotations(str(tmp_path), sequences=[11])
    assert only.sequences == [11] and only.frames == 5 and S.same_bits(only.gt3d, scene["gt3d"][1:6, :3])
    with pytest.raises(ValueError, match="no such directory"):
        M.load_annotations(str(tmp_path / "nowhere"))
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no TS"):
        M.load_annotations(str(tmp_path / "empty"))


@pytest.fixture(scope="module")
def host_twin(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mupots_twin") / "mupots_main"
    r = subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "smap_amd", "csrc"), os.path.join(ROOT, "tests", "c", "mupots_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("config", list(S.CONFIGS))
def test_host_twin_under_sanitizers_equals_the_restatement(tmp_path, scene, restated, host_twin, config):
    """csrc/mupots_core.h in serial loops (tests/c/mupots_main.cpp, -fsanitize=address,undefined, run as a program): rows and
    accumulators bit for bit the restatement's, NaN where it has NaN, and no sanitizer report."""
    S.write_scene_bin(tmp_path / "scene.bin", scene, S.CONFIGS[config])
    r = subprocess.run([str(host_twin), str(tmp_path / "scene.bin"), str(tmp_path / "rows.bin")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    F, G = scene["gt2d"].shape[:2]
    match, considered, err, rootz, acc = S.read_rows_bin(tmp_path / "rows.bin", F, G, 3)
    rows, accs = restated[config]
    w_match, w_considered, w_err, w_rootz = S.rows_arrays(rows, F, G)
    assert (match == w_match).all() and (considered == w_considered).all()
    assert S.same_bits(err, w_err) and (np.isnan(err) == np.isnan(w_err)).all() and S.same_bits(rootz, w_rootz)
    assert S.same_bits(acc, np.asarray(accs))


@pytest.mark.parametrize("config", list(S.CONFIGS))
def test_table_assembly_equals_the_restatement(restated, config):
    from smap_amd.mupots import tables_from_acc
    _, accs = restated[config]
    got, want = tables_from_acc(np.asarray(accs)), R.tables(accs)
    assert set(got) == set(want)

    def same(a, b, where):
        if isinstance(b, dict):
            for k in b:
                same(a[k], b[k], where + (k,))
        else:
            assert S.same_bits(np.asarray(a, np.float64), np.asarray(b, np.float64)), where
    same(got, want, ())


def test_write_csv_uses_the_reference_file_names(tmp_path, scene, restated):
    from smap_amd import mupots as M
    ann = M.Annotations([1, 2, 3], scene["seq_offset"], scene["gt_count"], scene["gt2d"], scene["gt3d"], scene["occ"])
    rows, accs = restated["matched_only"]
    F, G = scene["gt2d"].shape[:2]
    res = M.MuPoTSResult(ann, True, *S.rows_arrays(rows, F, G), np.asarray(accs))
    paths = res.write_csv(str(tmp_path / "eval_result"))
    assert [os.path.basename(p) for p in paths] == ["only_matched_annotations_multiperson_3dhp_evaluation_sequencewise.csv",
                                                    "only_matched_annotations_visible_joints_multiperson_3dhp_evaluation_sequencewise.csv",
                                                    "only_matched_annotations_occluded_joints_multiperson_3dhp_evaluation_sequencewise.csv"]
    lines = open(paths[0]).read().splitlines()
    assert len(lines) == 3 * 4 and lines[0].endswith("left_ankle,Average") and lines[4].startswith("PCK,Head,") and lines[8].startswith("AUC,")
    assert len(open(paths[1]).read().splitlines()) == 6
    assert res.sequence_errors(1).shape == (NJ, 6) and json.dumps(res.summary())


def test_pose_mats_of_convert_pack_like_the_dicts(tmp_path, scene):
    """`--pose3d pose3d.mat --pose2d pose2d.mat`: the two files as lib/eval/convert.py writes them (frames of 0, 1 and many persons) are
    read back into the dicts they were written from, so the scorer is handed the same arrays."""
    import scipy.io as scio
    from smap_amd import mupots as M
    pose2d, pose3d = S.pose_dicts(scene)
    scio.savemat(tmp_path / "pose3d.mat", {"preds_3d_kpt": pose3d})
    scio.savemat(tmp_path / "pose2d.mat", {"preds_2d_kpt": pose2d})
    got2, got3 = M.load_pose_mats(str(tmp_path / "pose3d.mat"), str(tmp_path / "pose2d.mat"))
    assert sorted(got2) == sorted(pose2d) and sorted(got3) == sorted(pose3d)
    ann = M.Annotations([1, 2, 3], scene["seq_offset"], scene["gt_count"], scene["gt2d"], scene["gt3d"], scene["occ"])
    for a, b in zip(M.pack_predictions(ann, got2, got3), M.pack_predictions(ann, pose2d, pose3d)):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all()
    with pytest.raises(ValueError, match="preds_2d_kpt"):
        M.load_pose_mats(str(tmp_path / "pose3d.mat"), str(tmp_path / "pose3d.mat"))


# ---- refusals: none of them needs a GPU -------------------------------------------------------------------------------------------
def _cli(args, cwd=ROOT):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "smap_amd.evaluate"] + args, capture_output=True, text=True, timeout=300, env=env, cwd=cwd)


def _result_json(path, frames):
    """A result file whose records convert_records accepts: frames = [(image_path, persons)]."""
    pairs = []
    for name, persons in frames:
        gt = np.zeros((1, NJ, 11))
        gt[0, 0, 4:7] = [1500.0, 1024.0, 1024.0]
        pairs.append({"image_path": name, "pred_3d": np.ones((persons, NJ, 4)).tolist(), "pred_2d": np.ones((persons, NJ, 4)).tolist(),
                      "gt_3d": gt.tolist(), "gt_2d": gt.tolist()})
    path.write_text(json.dumps({"model_pattern": "MIX", "3d_pairs": pairs}))
    return str(path)


def test_cli_refusals_and_exit_codes(tmp_path, scene):
    from smap_amd import mupots as M
    root = tmp_path / "root"
    S.write_root(str(root), scene)
    every = [("x/TS%d/img_%06d.jpg" % (k, i), 1) for k, n in zip((1, 2, 3), S.SEQ_FRAMES) for i in range(n)]
    good = _result_json(tmp_path / "good.json", every)
    r = _cli([good, "--mupots", str(tmp_path / "nowhere")])
    assert r.returncode == 2 and "no such directory" in r.stderr and r.stdout == ""
    (tmp_path / "other.json").write_text(json.dumps({"pairs": []}))
    r = _cli([str(tmp_path / "other.json"), "--mupots", str(root)])
    assert r.returncode == 2 and "3d_pairs" in r.stderr
    crowd = _result_json(tmp_path / "crowd.json", [(n, 128 if n.endswith("TS2/img_000002.jpg") else 1) for n, _ in every])
    r = _cli([crowd, "--mupots", str(root)])
    assert r.returncode == 2 and "TS2/img_000002" in r.stderr and "128 predictions" in r.stderr
    short = _result_json(tmp_path / "short.json", [e for e in every if not e[0].endswith("TS3/img_000004.jpg")])
    r = _cli([short, "--mupots", str(root)])
    assert r.returncode == 2 and "TS3/img_000004" in r.stderr
    r = _cli(["--mupots", str(root)])
    assert r.returncode == 2 and "either a result JSON or" in r.stderr
    r = _cli([good, "--mupots", str(root), "--pose3d", "pose3d.mat"])
    assert r.returncode == 2 and "come together" in r.stderr
    # the same refusals through the module; missing="empty" accepts the short file; a frame without valid persons needs no entry
    from lib.eval.convert import convert_records
    ann = M.load_annotations(str(root))
    pose3d, pose2d, _ = convert_records(json.load(open(short))["3d_pairs"])
    with pytest.raises(ValueError, match="TS3/img_000004"):
        M.pack_predictions(ann, pose2d, pose3d)
    p2, p3, off = M.pack_predictions(ann, pose2d, pose3d, missing="empty")
    assert off[-1] == len(p2) == len(p3) == 15 and off[10] == off[11]            # 16 frames with persons, one of them missing
    for name in ("TS2/img_000000.jpg", "TS3/img_000011.jpg"):                  # the two frames without valid persons
        pose2d.pop(name), pose3d.pop(name)
    assert M.pack_predictions(ann, pose2d, pose3d, missing="empty")[2].tolist() == off.tolist()
    # 17 valid persons: refused where the annotations are packed, with the frame's name
    big = dict(scene, gt_count=scene["gt_count"].copy(), gt2d=np.zeros((18, 17, NJ, 2)), gt3d=np.zeros((18, 17, NJ, 3)), occ=np.zeros((18, 17, NJ)))
    big["gt_count"][7] = 17
    S.write_root(str(tmp_path / "big"), big)
    with pytest.raises(ValueError, match=r"TS3/img_000001: 17 valid persons"):
        M.load_annotations(str(tmp_path / "big"))
    r = _cli([good, "--mupots", str(tmp_path / "big")])
    assert r.returncode == 2 and "17 valid persons" in r.stderr
    with pytest.raises(ValueError, match="cuda"):
        M.MuPoTSScorer(ann, device="cpu")


def test_test_py_parser_rules_for_eval_mupots():
    script = os.path.join(ROOT, "exps", "stage3_root2", "test.py")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for extra, message in ((["-t", "run_inference", "--eval_mupots", "somewhere"], "--eval_mupots requires -t generate_result"),
                           (["-t", "generate_train", "--eval_mupots", "somewhere"], "--eval_mupots requires -t generate_result"),
                           (["-t", "generate_result", "--dry_run", "1", "--eval_mupots", "somewhere"], "not available with --dry_run 1")):
        r = subprocess.run([sys.executable, script] + extra, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert r.returncode == 2 and message in r.stderr, (extra, r.stderr[-1000:])
