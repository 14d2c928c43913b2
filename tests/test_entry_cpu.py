"""CPU suite for the host-side orchestration: dataset letter-boxing, flip-TTA merge, camera
defaults, contiguous frame sharding and the 2-rank gloo gather of result records."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_custom_dataset_letterbox(tmp_path):
    from dataset.custom_dataset import CustomDataset
    from exps.stage3_root2.config import cfg
    rng = np.random.default_rng(0)
    np.save(tmp_path / "wide.npy", rng.integers(0, 255, (300, 1000, 3), dtype=np.uint8))
    np.save(tmp_path / "tall.npy", rng.integers(0, 255, (900, 400, 3), dtype=np.uint8))
    from PIL import Image
    Image.fromarray(rng.integers(0, 255, (512, 832, 3), dtype=np.uint8)).save(tmp_path / "exact.png")
    ds = CustomDataset(cfg, str(tmp_path))
    assert len(ds) == 3
    for i in range(3):
        img, name, scale = ds[i]
        assert img.shape == (3, 512, 832) and img.dtype == torch.float32
        assert scale["net_width"] == 832 and scale["net_height"] == 512
        assert abs(scale["scale"] - min(832 / scale["img_width"], 512 / scale["img_height"])) < 1e-12
        pad = (torch.tensor(128 / 255.0) - ds.mean) / ds.std              # 128-grey padding, normalised
        if "wide" in name:
            assert torch.allclose(img[:, 0, 0], pad.view(3)) and torch.allclose(img[:, -1, -1], pad.view(3))
        if "tall" in name:
            assert torch.allclose(img[:, 0, 0], pad.view(3)) and torch.allclose(img[:, 256, -1], pad.view(3))


def test_merge_flip_matches_reference_loop():
    from exps.stage3_root2.config import cfg
    from exps.stage3_root2.test_util import merge_flip
    g = torch.Generator().manual_seed(0)
    a = torch.randn(2, 43, 8, 12, generator=g)
    b = torch.randn(2, 43, 8, 12, generator=g)
    want = a.clone()
    fl = torch.flip(b, dims=[-1])                                           # test.py:58
    kpt = 15
    pair = cfg.DATASET.KEYPOINT.FLIP_ORDER + [x + kpt for x in cfg.DATASET.PAF.FLIP_CHANNEL]
    for i in range(len(pair)):                                              # test.py:65-69
        if i >= kpt and (i - kpt) % 2 == 0:
            want[:, i] += fl[:, pair[i]] * -1
        else:
            want[:, i] += fl[:, pair[i]]
    want[:, kpt:] *= 0.5
    got = merge_flip(a.clone(), b, cfg)
    assert torch.equal(got, want)


def test_default_cams():
    from exps.stage3_root2.test_util import default_cams
    scales = {"scale": torch.tensor([0.5, 0.25]), "img_width": torch.tensor([1664, 3328]),
              "img_height": torch.tensor([1024, 1000]), "net_width": torch.tensor([832, 832]),
              "net_height": torch.tensor([512, 512])}
    c = default_cams(scales, 2)
    assert c.shape == (2, 9) and c.dtype == np.float64
    assert list(c[1]) == [0.25, 3328, 1000, 832, 512, 3328, 3328, 1664, 500]


def test_shard_range_is_a_contiguous_partition():
    from smap_amd.dist import shard_range
    for n in (0, 1, 7, 8, 9, 64, 1000):
        for world in (1, 2, 3, 8):
            spans = [shard_range(n, world, r) for r in range(world)]
            flat = [i for s, e in spans for i in range(s, e)]
            assert flat == list(range(n))
            assert max(e - s for s, e in spans) <= -(-n // world)


_WORKER = r"""
import os, sys, json
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from smap_amd.dist import gather_bytes, gather_records, shard_range
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
st, ed = shard_range(11, world, rank)
recs = [{"image_path": f"img{i}", "pred_3d": [[float(i), 0.5 * rank]], "root_d": [1.0 / (i + 1)]} for i in range(st, ed)]
parts = gather_records(recs)
flat = [r for p in parts for r in p]
from lib.utils import comm
assert comm.get_world_size() == world and comm.get_rank() == rank and comm.is_main_process() == (rank == 0)
comm.synchronize()
assert comm.all_gather({"r": rank}) == [{"r": r} for r in range(world)]
raw = gather_bytes(b"x" * (3 * rank))            # ragged payloads, an empty one included
assert raw == [b"x" * (3 * r) for r in range(world)], raw
assert [r["image_path"] for r in flat] == [f"img{i}" for i in range(11)], flat
assert flat[7]["root_d"][0] == 1.0 / 8
if rank == 0:
    print("GATHER_OK", len(flat))
dist.destroy_process_group()
"""


def test_two_rank_gloo_gather(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29541", str(script), ROOT],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "GATHER_OK 11" in r.stdout


def test_host_resize_is_opencv_fixed_point_linear():
    """resize_linear_u8 restates OpenCV's 8-bit INTER_LINEAR (11-bit fixed-point coefficients, integer vertical pass).  Checked
    here against (a) a scalar transcription of the published per-pixel formula on random positions, (b) the float bilinear of
    the same sampling rule (F.interpolate, align_corners=False): the fixed-point result stays within 1 LSB of it, (c) the
    identities OpenCV guarantees: same size = copy, exact 2x shrink = 2x2 box mean."""
    import math
    import torch.nn.functional as F
    from smap_amd.preprocess import resize_linear_u8
    rng = np.random.default_rng(2)
    for (h, w), f in [((300, 1000), 0.832), ((900, 400), 512 / 900), ((37, 53), 512 / 37), ((480, 640), 1.3), ((1080, 1920), 832 / 1920)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        nh, nw = int(round(h * f)), int(round(w * f))
        got = resize_linear_u8(img, nh, nw, fx=f, fy=f).astype(np.int32)
        assert got.shape == (nh, nw, 3)
        for _ in range(300):                                   # (a) the formula, pixel by pixel
            dy, dx, c = int(rng.integers(nh)), int(rng.integers(nw)), int(rng.integers(3))
            def tap(d, n):
                v = np.float32((d + 0.5) * (1.0 / f) - 0.5)
                s = math.floor(v)
                v = np.float32(v - np.float32(s))
                if s < 0: s, v = 0, np.float32(0)
                if s >= n - 1: s, v = n - 1, np.float32(0)
                return s, min(s + 1, n - 1), int(np.rint((np.float32(1) - v) * np.float32(2048))), int(np.rint(v * np.float32(2048)))
            y0, y1, b0, b1 = tap(dy, h)
            x0, x1, a0, a1 = tap(dx, w)
            h0 = int(img[y0, x0, c]) * a0 + int(img[y0, x1, c]) * a1
            h1 = int(img[y1, x0, c]) * a0 + int(img[y1, x1, c]) * a1
            assert got[dy, dx, c] == (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
        t = torch.from_numpy(img).permute(2, 0, 1)[None].float()    # (b) float bilinear of the same sampling rule
        ref = F.interpolate(t, size=(nh, nw), mode="bilinear", align_corners=False, antialias=False)[0].permute(1, 2, 0).numpy()
        if abs(nh / h - f) < 1e-3 and abs(nw / w - f) < 1e-3:      # (torch derives its scale from the sizes, OpenCV takes fx)
            assert np.abs(got - ref).max() <= 1.0 + 0.02 * 255 * abs(nw / w - f) * w / 2
    img = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    assert np.array_equal(resize_linear_u8(img, 64, 96, fx=1.0, fy=1.0), img)                       # (c)
    box = (img.astype(np.int32).reshape(32, 2, 48, 2, 3).sum((1, 3)) + 2) >> 2
    assert np.array_equal(resize_linear_u8(img, 32, 48, fx=0.5, fy=0.5), box.astype(np.uint8))


def test_derived_skeleton_tables_equal_reference_constants():
    """dataset/data_settings.py derives limbs and mirror tables from the skeleton tree; the values are
    the reference's (dataset/data_settings.py:22,28-34)."""
    from dataset.data_settings import MIX
    assert MIX.KEYPOINT.FLIP_ORDER == [0, 1, 2, 9, 10, 11, 12, 13, 14, 3, 4, 5, 6, 7, 8]
    assert MIX.PAF.VECTOR == [[0, 1], [0, 2], [0, 9], [9, 10], [10, 11], [0, 3], [3, 4], [4, 5],
                              [2, 12], [12, 13], [13, 14], [2, 6], [6, 7], [7, 8]]
    assert MIX.PAF.FLIP_CHANNEL == [0, 1, 2, 3, 10, 11, 12, 13, 14, 15, 4, 5, 6, 7, 8, 9,
                                    22, 23, 24, 25, 26, 27, 16, 17, 18, 19, 20, 21]
    assert (MIX.INPUT_SHAPE, MIX.OUTPUT_SHAPE, MIX.STRIDE, MIX.ROOT_IDX) == ((512, 832), (128, 208), 4, 2)


def test_record_builders_reproduce_reference_json(golden_dir):
    """frame_record / train_records (test_util.py:134-158) on the golden arrays give the reference's JSON."""
    from smap_amd.records import annotation_camera, frame_record, kept_annotations, train_records
    z = np.load(f"{golden_dir}/lift_gt.npz")
    seen = 0
    for c in range(int(z["n_cases"])):
        p = f"c{c}_"
        ann = z[p + "ann"]
        gt = kept_annotations(ann)
        if int(z[p + "empty"]):
            continue
        assert np.array_equal(gt, z[p + "gt"])
        want_r = json.loads(bytes(z[p + "json_result"]).decode())["3d_pairs"]
        want_t = json.loads(bytes(z[p + "json_train"]).decode())["3d_pairs"]
        got_r = frame_record(z[p + "matched"], z[p + "refined"], z[p + "root_z"], want_r[0]["image_path"], gt)
        assert [got_r] == want_r
        assert train_records(z[p + "matched"], z[p + "refined"], z[p + "root_z"], gt) == want_t
        s, w, h = z[p + "scale"]
        cam = annotation_camera(gt, {"scale": s, "img_width": w, "img_height": h, "net_width": 832, "net_height": 512})
        assert np.array_equal(cam, z[p + "cam"])
        seen += len(want_t)
    assert seen > 0
    # annotations without intrinsics columns: f from column 7, principal point at the image centre (test.py:84-88)
    short = np.zeros((1, 15, 8), np.float32)
    short[0, :, 7] = 1234.5
    cam = annotation_camera(short, {"scale": 0.5, "img_width": 640, "img_height": 480, "net_width": 832, "net_height": 512})
    assert cam.tolist() == [0.5, 640, 480, 832, 512, 1234.5, 1234.5, 320, 240]


def test_p2p_dataset_matches_reference_golden(golden_dir, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))                # a test-support reader now: the RefineNet TRAINING data set is out of scope
    from p2p_dataset import P2PDataset
    z = np.load(f"{golden_dir}/p2p.npz")
    path = tmp_path / "train.json"
    path.write_text(bytes(z["json"]).decode())
    ds = P2PDataset(dataset_path=str(path))
    assert len(ds) == len(z["inp"])
    for i in range(len(ds)):
        a, b = ds[i]
        assert a.dtype == torch.float32 and np.array_equal(a.numpy(), z["inp"][i]) and np.array_equal(b.numpy(), z["gt"][i])


def test_joint_dataset_croppad_and_loader(tmp_path):
    """The no-augmentation aug_croppad (ImageAugmentation.py:54-111): geometry, annotation transform, the
    off-canvas rule, the isValidation split and the contiguous per-rank split of get_test_loader."""
    from exps.stage3_root2.config import cfg
    from dataset.base_dataset import JointDataset, croppad_geometry
    from lib.utils.dataloader import get_test_loader
    # 1920x1080: scale 832/1920, resized 832x468, pasted 22 rows down; 2048x2048: scale 0.25, 512x512, 160 columns in
    s, (nh, nw), (left, top) = croppad_geometry(1920, 1080, 832, 512)
    assert (nh, nw, left, top) == (468, 832, 0, 22) and s == 832 / 1920
    s, (nh, nw), (left, top) = croppad_geometry(2048, 2048, 832, 512)
    assert (nh, nw, left, top, s) == (512, 512, 160, 0, 0.25)
    # a frame larger than the canvas in one direction after scaling cannot happen (scale = min ratio); odd sizes:
    s, (nh, nw), (left, top) = croppad_geometry(641, 479, 832, 512)
    assert nw <= 832 and nh <= 512 and left == int(416 - int(320 * s)) and top == int(256 - int(239 * s))
    root = tmp_path / "set"
    root.mkdir()
    rng = np.random.default_rng(0)
    entries = []
    for i, (h, w) in enumerate([(1080, 1920), (2048, 2048), (480, 640), (512, 832), (300, 400)]):
        np.save(root / f"f{i}.npy", rng.integers(0, 255, (h, w, 3), dtype=np.uint8))
        bodys = np.zeros((2, 15, 11))
        bodys[0, :, 0], bodys[0, :, 1], bodys[0, :, 3] = w / 2, h / 2, 2          # image centre
        bodys[1, :, 0], bodys[1, :, 1], bodys[1, :, 3] = -5.0, h / 2, 2          # left of the image
        bodys[:, :, 7:] = [1000, 1001, w / 2, h / 2]
        entries.append({"dataset": "muco", "img_paths": f"f{i}.npy", "img_width": w, "img_height": h,
                        "isValidation": int(i != 4), "bodys": bodys.tolist()})
    (root / "gt.json").write_text(json.dumps({"root": entries}))
    cfg.TEST.ROOT_PATH, cfg.TEST.JSON_PATH = str(root), str(root / "gt.json")
    ds = JointDataset(cfg, "test")
    assert len(ds) == 4
    img, meta, path, scale = ds[0]
    assert img.shape == (3, 512, 832) and meta.shape == (cfg.DATASET.MAX_PEOPLE, 15, 11) and meta.dtype == torch.float32
    assert path == "f0.npy" and scale == {"scale": 832 / 1920, "img_width": 1920, "img_height": 1080,
                                          "net_width": 832, "net_height": 512}
    assert torch.allclose(meta[0, :, :2], torch.tensor([416.0, 256.0]).expand(15, 2))     # centre -> canvas centre
    assert (meta[0, :, 3] == 2).all() and (meta[1, :, 3] == 0).all()                       # off-canvas joints: score 0
    assert not meta[2:].any()
    grey = (128 / 255 - torch.tensor(cfg.INPUT.MEANS)) / torch.tensor(cfg.INPUT.STDS)
    assert torch.allclose(img[:, :22].amax((1, 2)), grey) and torch.allclose(img[:, 490:].amin((1, 2)), grey)   # 128-grey bands
    img1, meta1, _, _ = ds[1]
    assert torch.allclose(img1[:, :, :160].amax((1, 2)), grey) and torch.allclose(meta1[0, 0, :2], torch.tensor([416.0, 256.0]))
    with pytest.raises(NotImplementedError):
        JointDataset(cfg, "train")
    cfg.TEST.IMG_PER_GPU = 2
    parts = [[p for b in get_test_loader(cfg, 2, r, "test") for p in b[2]] for r in range(2)]
    assert parts == [["f0.npy", "f1.npy"], ["f2.npy", "f3.npy"]]
    b = next(iter(get_test_loader(cfg, 1, 0, "test")))
    assert b[0].shape == (2, 3, 512, 832) and b[1].shape == (2, cfg.DATASET.MAX_PEOPLE, 15, 11) and len(b[3]) == 2


def test_bench_control_flow_two_ranks_gloo():
    """bench.py --dry-run under torch.distributed.run with 2 ranks: every rank issues the same collectives (ONE end-of-run
    gather of the pickled records of all timed steps, barrier, MAX all-reduce) and rank 0 alone prints the one JSON line."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29533", os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--steps", "5", "--warmup", "2", "--dry-run"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 5 and d["config"]["ranks_in_gather"] == 2
    # the gather carries every record of the 5 timed batches of each rank (8 frames each; batches 2..6 after 2 warm-ups)
    assert d["config"]["records_per_rank"] == [40, 40]
    assert d["config"]["first_paths"] == ["r0/b2/f0", "r1/b2/f0"] and d["config"]["last_paths"] == ["r0/b6/f7", "r1/b6/f7"]


def test_bench_gpus_flag_spawns_its_own_ranks_and_rejects_a_wrong_world():
    """`python bench.py --gpus 2` WITHOUT a launcher re-executes itself under torch.distributed.run with two ranks (round 3
    printed an n_gpus: 1 line for it); a launcher whose world size disagrees with --gpus is an error, not a silent line."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["ranks_in_gather"] == 2 and d["config"]["records_per_rank"] == [24, 24]
    # world 2 from the launcher, --gpus left at its default of 1: refuse
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29535", os.path.join(ROOT, "bench.py"),
                        "--steps", "3", "--warmup", "1", "--dry-run"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_bench_control_flow_eight_ranks_gloo():
    """The driver's 8-GPU launch line (`torch.distributed.run --nproc-per-node 8 bench.py --gpus 8`) with --dry-run: all eight
    ranks reach the one end-of-run gather, rank order == frame order, every rank's host CPU per step is reported."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8",
                        "--master-addr", "127.0.0.1", "--master-port", "29547", os.path.join(ROOT, "bench.py"),
                        "--gpus", "8", "--steps", "5", "--warmup", "2", "--dry-run"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["config"]["ranks_in_gather"] == 8
    assert d["config"]["records_per_rank"] == [40] * 8
    assert d["config"]["first_paths"] == [f"r{k}/b2/f0" for k in range(8)]
    assert d["config"]["last_paths"] == [f"r{k}/b6/f7" for k in range(8)]
    assert len(d["config"]["host_ms_per_step"]["process_cpu_per_rank"]) == 8
    # one record is enough to diagnose a scaling run: every rank's own rate and the slowest / fastest step time (the headline uses the MAX)
    pr = d["config"]["per_rank"]
    assert len(pr["frames_per_sec"]) == 8 and all(f > 0 for f in pr["frames_per_sec"])
    assert pr["ms_per_step_min"] <= pr["ms_per_step_max"] <= d["ms_per_step"] * 1.0001


def test_bench_dump_outputs_writes_the_last_steps_records(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the records of the LAST timed step (batch j, scene set K) of every rank as float32 / float64 .npy
    files, persons concatenated in frame order; a frame without a record counts 0 persons, an earlier step's record of the same
    frame is superseded by the last one; beyond the size cap a fixed seeded sample of the frames, named in frames.npy."""
    import bench
    rng = np.random.default_rng(5)

    def rec(path, P):
        return {"pred_2d": rng.normal(size=(P, 15, 4)).astype(np.float32), "pred_3d": rng.normal(size=(P, 15, 4)),
                "root_d": rng.normal(size=P), "image_path": path, "gt_3d": [], "gt_2d": []}
    r0 = [rec("r0/b1/f0", 2), rec("r0/b0/f1", 3), rec("r0/b1/f0", 1), rec("r0/b1/f2", 4), rec("synthK8/r0/b1/f1", 8),
          rec("synthK2/r0/b1/f1", 2)]
    r1 = [rec("r1/b1/f1", 5)]
    bench.dump_records(str(tmp_path / "d"), [r0, r1], 3, 1, 8)
    ld = lambda n: np.load(tmp_path / "d" / f"{n}.npy")
    assert ld("persons").dtype == np.float64 and ld("persons").tolist() == [1, 0, 4, 0, 5, 0]
    p2 = ld("pred_2d")
    assert p2.dtype == np.float32 and p2.shape == (10, 15, 4)
    assert np.array_equal(p2, np.concatenate([r0[2]["pred_2d"], r0[3]["pred_2d"], r1[0]["pred_2d"]]))
    assert ld("pred_3d").dtype == np.float64 and np.array_equal(ld("pred_3d")[1:5], r0[3]["pred_3d"])
    assert np.array_equal(ld("root_d"), np.concatenate([r0[2]["root_d"], r0[3]["root_d"], r1[0]["root_d"]]))
    assert ld("synth_persons").tolist() == [0, 8, 0, 0, 0, 0] and np.array_equal(ld("synth_pred_2d"), r0[4]["pred_2d"])
    assert not (tmp_path / "d" / "frames.npy").exists()
    # over the cap: a sample of whole frames that fits, the same one every time
    many = [rec(f"r0/b0/f{i}", 20) for i in range(64)]
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", (1 << 20) + 64 * 1024)
    for d in ("s1", "s2"):
        bench.dump_records(str(tmp_path / d), [many], 64, 0, 0)
    files = sorted(os.listdir(tmp_path / "s1"))
    assert "frames.npy" in files and sum(os.path.getsize(tmp_path / "s1" / f) for f in files) <= bench.DUMP_CAP_BYTES
    kept = np.load(tmp_path / "s1" / "frames.npy").astype(int)
    assert 0 < len(kept) < 64 and np.array_equal(kept, np.load(tmp_path / "s2" / "frames.npy"))
    assert np.array_equal(np.load(tmp_path / "s1" / "pred_3d.npy"), np.concatenate([many[i]["pred_3d"] for i in kept]))


def test_test_py_dry_run_eight_ranks(tmp_path):
    """exps/stage3_root2/test.py --dry_run 1 under an 8-rank launch: 37 images (not a multiple of ranks x batch) are split in
    contiguous blocks of ceil(37/8) = 5 (lib/utils/dataloader.py:80-85), ragged last batches are padded and their padding
    dropped, the gather keeps rank order == image order, rank 0 writes one record per image."""
    imgs = tmp_path / "images"
    imgs.mkdir()
    rng = np.random.default_rng(0)
    names = [f"im{k:03d}.npy" for k in range(37)]
    for n in names:
        np.save(imgs / n, rng.integers(0, 256, (24, 40, 3), dtype=np.uint8))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PROJECT_HOME=str(tmp_path), OMP_NUM_THREADS="1",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8",
                        "--master-addr", "127.0.0.1", "--master-port", "29549",
                        os.path.join(ROOT, "exps", "stage3_root2", "test.py"), "-t", "run_inference", "-d", "test",
                        "--batch_size", "2", "--dataset_path", str(imgs), "--json_name", "dry", "--dry_run", "1"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = list(tmp_path.rglob("*run_inference_test_dry.json"))
    assert len(out) == 1, (list(tmp_path.rglob("*.json")), r.stderr[-1000:])
    res = json.load(open(out[0]))
    got = [rec["image_path"] for rec in res["3d_pairs"]]
    assert got == names                                     # every image once, in listing order
    assert all(len(rec["pred_3d"]) == 1 and len(rec["pred_3d"][0]) == 15 for rec in res["3d_pairs"])


def test_coalesced_pipeline_protocol_without_a_gpu(monkeypatch):
    """smap_amd/pipeline.py::CoalescedPipeline on CPU, the device pipeline replaced by a recorder: `group` submitted batches reach
    the inner pipeline as ONE batch (cameras, tags, per-frame prefixes of the extra maps and annotations concatenated in
    submission order; images and extra maps as LISTS of the callers' tensors -- nothing is copied), records come back in order, an incomplete trailing group goes through a batch-sized pipeline at
    flush(), and make_pipeline picks the group size from the frames per launch (x2 with flip-TTA)."""
    import smap_amd.pipeline as P

    class Recorder:
        built = []

        def __init__(self, model, cfg, batch, H, W, device, **kw):
            self.B, self.kw, self.calls, self.q = batch, kw, [], []
            self.chunk = self.frames_per_launch = batch
            self.engine = self.depth = self.s_comm = None
            self.bb_events, self.post_events = [], []
            Recorder.built.append(self)

        def submit(self, imgs, cams, tags, extra=(), time_backbone=False, annotations=None):
            ident = [id(t) for t in imgs] if isinstance(imgs, list) else None           # the callers' own tensors, not copies
            cat = lambda t: torch.cat(list(t)) if isinstance(t, (list, tuple)) else t
            imgs = cat(imgs)
            assert len(imgs) == len(cams) == len(tags) == self.B
            self.calls.append((imgs.clone(), np.asarray(cams).copy(), list(tags), [(t, cat(h).clone(), cat(r).clone(), d) for t, h, r, d in extra],
                               time_backbone, annotations, ident))
            self.q.append([{"image_path": t, "v": float(imgs[i].sum())} for i, t in enumerate(tags)])
            return self.q.pop(0) if len(self.q) > 1 else None

        def flush(self):
            out = [r for b in self.q for r in b]
            self.q = []
            return out or None

    monkeypatch.setattr(P, "PosePipeline", Recorder)
    B = 2
    pipe = P.make_pipeline(None, None, B, 8, 8, "cpu", launch_frames=6, depth=2)
    assert isinstance(pipe, P.CoalescedPipeline) and pipe.group == 3 and pipe.B == B and pipe.frames_per_launch == 6
    got, sent = [], []
    for i in range(8):                                   # 8 batches = 2 full groups + 2 left over
        imgs = torch.full((B, 3, 8, 8), float(i))
        sent.append(imgs)
        cams = np.full((B, 9), float(i))
        ex = [(f"K{i % 2}", torch.full((B, 43, 2, 2), 10.0 + i), torch.full((B, 1, 2, 2), 20.0 + i), None)]
        got += pipe.submit(imgs, cams, [f"b{i}/{j}" for j in range(B)], extra=ex, time_backbone=(i == 4)) or []
    got += pipe.flush() or []
    assert [r["image_path"] for r in got] == [f"b{i}/{j}" for i in range(8) for j in range(B)]       # every frame once, in order
    assert [r["v"] for r in got] == [float(i) * 3 * 64 for i in range(8) for _ in range(B)]
    big, small = Recorder.built[0], Recorder.built[1]
    assert big.B == 6 and small.B == 2 and len(big.calls) == 2 and len(small.calls) == 2
    imgs, cams, tags, extra, timed, ann, ident = big.calls[1]                                        # batches 3, 4, 5
    assert ident == [id(sent[3]), id(sent[4]), id(sent[5])]                                          # handed down as they are: no gather copy
    assert imgs[:, 0, 0, 0].tolist() == [3, 3, 4, 4, 5, 5] and cams[:, 0].tolist() == [3, 3, 4, 4, 5, 5] and timed and ann is None
    assert tags == [f"b{i}/{j}" for i in (3, 4, 5) for j in range(B)]
    assert extra[0][0] == ["K1", "K1", "K0", "K0", "K1", "K1"] and extra[0][1][:, 0, 0, 0].tolist() == [13, 13, 14, 14, 15, 15]
    assert extra[0][2][:, 0, 0, 0].tolist() == [23, 23, 24, 24, 25, 25] and extra[0][3] is None
    assert not big.calls[0][4]                                                                       # no timed batch in group 0
    # group size from the launch size; flip-TTA doubles the frames of a batch; ground-truth modes and large batches are not coalesced
    assert P.make_pipeline(None, None, 8, 8, 8, "cpu", launch_frames=16).group == 2
    assert P.make_pipeline(None, None, 4, 8, 8, "cpu", launch_frames=16, do_flip=True).group == 2
    for kw in (dict(launch_frames=0), dict(launch_frames=16, do_flip=True), dict(launch_frames=16, record_mode="generate_result")):
        assert isinstance(P.make_pipeline(None, None, 8, 8, 8, "cpu", **kw), Recorder), kw


def test_clock_sampler_reads_hwmon_files_and_survives_their_absence(tmp_path, monkeypatch):
    """benchkit/clocks.py: the bench line's `roofline.clocks` (shader clock and package power held in the timed region).  With hwmon files:
    means over the samples inside [t0, t1]; without: None, and the bench goes on."""
    import time
    from benchkit import clocks
    (tmp_path / "freq1_input").write_text("1990000000\n")
    (tmp_path / "power1_average").write_text("1380000000\n")
    monkeypatch.setattr(clocks, "_hwmon_dir", lambda i=0: str(tmp_path))
    t0 = time.perf_counter()
    with clocks.ClockSampler(0, period_s=0.005) as s:
        time.sleep(0.06)
    got = s.summary(t0, time.perf_counter())
    assert got["samples"] >= 3 and abs(got["sclk_mhz"] - 1990.0) < 1e-6 and abs(got["power_w"] - 1380.0) < 1e-6
    assert abs(got["clock_share_of_max"] - 1990.0 / 2400.0) < 1e-9
    assert s.summary(t0 - 10, t0 - 5) is None
    monkeypatch.setattr(clocks, "_hwmon_dir", lambda i=0: None)
    with clocks.ClockSampler(0) as s2:
        pass
    assert s2.summary() is None


def test_process_decoders_hand_over_the_frames_the_in_thread_decoder_reads(tmp_path):
    """smap_amd/loaders.py::DevicePreprocLoader with SMAP_DECODE_PROCS (process_decoders): worker processes (dataset/decode.py: numpy + PIL only) decode into
    one shared-memory block, the loader's pool threads copy their slot out.  Same bytes as the in-thread decoder for PNG, JPEG (EXIF
    orientation applied) and .npy files; a frame larger than a slot is decoded in-thread; a broken file raises in the consumer; the block
    is unlinked when the iteration ends."""
    import contextlib
    import importlib.util
    import types
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from dataset.decode import read_bgr
    spec = importlib.util.spec_from_file_location("smap_cli_test", os.path.join(ROOT, "exps", "stage3_root2", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    rng = np.random.default_rng(5)
    paths = []
    for i, (h, w, ext) in enumerate([(40, 60, "png"), (64, 48, "jpg"), (30, 30, "npy"), (200, 300, "png"), (50, 70, "jpg")]):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p = str(tmp_path / f"f{i}.{ext}")
        if ext == "npy":
            np.save(p, a)
        elif i == 4:
            ex = Image.Exif()
            ex[0x0112] = 6                                   # "rotated 90 degrees": cv2.imread applies it
            Image.fromarray(a).save(p, quality=95, exif=ex)
        else:
            Image.fromarray(a).save(p)
        paths.append(p)
    from smap_amd.loaders import process_decoders
    assert cli.DevicePreprocLoader.__module__ == "smap_amd.loaders"
    ds = types.SimpleNamespace(path=lambda i: paths[i], name=lambda i: os.path.basename(paths[i]))
    shm_dir = "/dev/shm"
    before = set(os.listdir(shm_dir)) if os.path.isdir(shm_dir) else set()
    with contextlib.ExitStack() as stack:
        decode = process_decoders(stack, ds, 2, 64 * 1024, lambda img: np.array(img))     # 64 KiB slots: the 200x300 frame (180 kB) does not fit
        during = (set(os.listdir(shm_dir)) if os.path.isdir(shm_dir) else set()) - before
        with ThreadPoolExecutor(2) as ex:
            got = list(ex.map(decode, range(len(paths))))
        for i, (img, name) in enumerate(got):
            assert name == os.path.basename(paths[i])
            assert np.array_equal(img, read_bgr(paths[i])), i
        assert got[4][0].shape == (70, 50, 3)                 # the EXIF rotation happened in the worker too
        bad = str(tmp_path / "broken.png")
        with open(bad, "wb") as f:
            f.write(b"not a png")
        paths.append(bad)
        with pytest.raises(RuntimeError):
            decode(len(paths) - 1)
    if os.path.isdir(shm_dir):
        assert during and not (during & set(os.listdir(shm_dir)))       # the block existed while the loader ran and is gone now


def _cli():
    """exps/stage3_root2/test.py as a module (its file name is not importable by pytest's rules: loaded by path)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("smap_cli_test", os.path.join(ROOT, "exps", "stage3_root2", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def _gt_batch(with_frames):
    """A collate_test batch of 3 frames, B = 4 to come: 2, 0 and 1 kept persons (frame 0 carries a third whose root score is 1: dropped)."""
    ann = torch.zeros((3, 6, 15, 11))
    for f, p, x in ((0, 0, 10.0), (0, 1, 20.0), (2, 0, 30.0)):
        ann[f, p, :, 0], ann[f, p, :, 3] = x, 2.0
        ann[f, p, :, 7:] = torch.tensor([1000.0 + x, 1001.0, 416.0, 256.0])
    ann[0, 2, :, 0], ann[0, 2, :, 3] = 40.0, 1.0
    metas = tuple({"scale": 0.5 * (k + 1), "img_width": 1664, "img_height": 1024, "net_width": 832, "net_height": 512} for k in range(3))
    imgs = torch.arange(3.0).view(3, 1, 1, 1).expand(3, 3, 4, 6).contiguous() if with_frames else None
    return imgs, ann, ("a", "b", "c"), metas


def test_shape_batch_and_pad_to():
    """shape_batch turns a loader batch into what submit takes, pad_to(B) pads every per-frame member alike: the last entry repeated,
    tag None, cams a float64 row; a full batch is not copied."""
    from smap_amd.records import kept_annotations
    cli = _cli()
    cpu = torch.device("cpu")
    # an inference batch of 3 frames
    cli.cfg.TEST_MODE = "run_inference"                     # (what main() sets from -t)
    frames = torch.arange(3.0).view(3, 1, 1, 1).expand(3, 3, 4, 6).contiguous()
    scales = {"scale": torch.tensor([1.0, 2.0, 3.0]), "img_width": torch.tensor([832] * 3), "img_height": torch.tensor([512] * 3),
              "net_width": torch.tensor([832] * 3), "net_height": torch.tensor([512] * 3)}
    b = cli.pad_to(cli.shape_batch((frames, ["a", "b", "c"], scales), cli.cfg, cpu), 4)
    assert b.imgs.shape == (4, 3, 4, 6) and [float(f.mean()) for f in b.imgs] == [0.0, 1.0, 2.0, 2.0]
    assert b.tags == ["a", "b", "c", None] and b.annotations is None and b.map_inputs is None
    assert isinstance(b.cams, np.ndarray) and b.cams.dtype == np.float64 and b.cams.shape == (4, 9)
    assert b.cams[:, 0].tolist() == [1.0, 2.0, 3.0, 3.0] and np.array_equal(b.cams[2], b.cams[3])
    # a full batch of 4: the very same tensor, nothing copied
    full = torch.zeros((4, 3, 4, 6))
    sc4 = {k: torch.cat([v, v[-1:]]) for k, v in scales.items()}
    b4 = cli.shape_batch((full, ["a", "b", "c", "d"], sc4), cli.cfg, cpu)
    assert cli.pad_to(b4, 4) is b4 and b4.imgs is full
    # a ground-truth batch of 3 frames with 2, 0 and 1 kept persons
    cli.cfg.TEST_MODE = "generate_result"
    batch = _gt_batch(True)
    b = cli.pad_to(cli.shape_batch(batch, cli.cfg, cpu), 4)
    assert [len(a) for a in b.annotations] == [2, 0, 1, 1] and len(b.annotations) == 4
    for a, m in zip(b.annotations[:3], batch[1]):
        assert np.array_equal(a, kept_annotations(m.numpy(), cli.cfg.DATASET.ROOT_IDX))
    assert b.annotations[0][:, 0, 0].tolist() == [10.0, 20.0]               # the person with root score 1 is gone
    assert np.array_equal(b.annotations[3], b.annotations[2])
    assert list(b.cams[1]) == [1.0] * 9 and b.cams.dtype == np.float64 and b.cams.shape == (4, 9) and np.array_equal(b.cams[2], b.cams[3])
    assert list(b.cams[0]) == [0.5, 1664, 1024, 832, 512, 1010.0, 1001.0, 416.0, 256.0]
    assert b.tags == ["a", "b", "c", None] and b.imgs.shape == (4, 3, 4, 6) and torch.equal(b.imgs[3], b.imgs[2]) and b.map_inputs is None
    # the same without frames (--maps_from_gt 1)
    batch = _gt_batch(False)
    b = cli.pad_to(cli.shape_batch(batch, cli.cfg, cpu, maps_from_gt=True), 4)
    H, W = cli.cfg.dataset.INPUT_SHAPE
    assert tuple(b.imgs.shape) == (4, 3, H, W) and len(b.imgs) == 4
    anns, scs = b.map_inputs
    assert len(anns) == 4 and len(scs) == 4 and all(isinstance(a, torch.Tensor) for a in anns)
    assert all(torch.equal(a, m) for a, m in zip(anns[:3], batch[1])) and torch.equal(anns[3], anns[2])
    assert list(scs[:3]) == list(batch[3]) and scs[3] == scs[2]
    assert [len(a) for a in b.annotations] == [2, 0, 1, 1] and b.tags == ["a", "b", "c", None] and list(b.cams[1]) == [1.0] * 9


_REFUSALS = [
    ("--eval_mupots X -t run_inference", "--eval_mupots requires -t generate_result"),
    ("--eval_mupots X -t generate_result --dry_run 1", "--eval_mupots scores on the GPU: not available with --dry_run 1"),
    ("--eval_loss 1 -t generate_train", "--eval_loss 1 requires -t generate_result"),
    ("--eval_loss 1 -t generate_result --dry_run 1", "--eval_loss 1 runs on the GPU: not available with --dry_run 1"),
    ("--eval_loss 1 -t generate_result --maps_from_gt 1", "--eval_loss 1 needs the network's heads: not available with --maps_from_gt 1"),
    ("--maps_from_gt 1", "--maps_from_gt 1 renders the maps from annotations: -t run_inference has none (use -t generate_result or generate_train)"),
    ("--maps_from_gt 1 -t generate_train --dry_run 1", "--maps_from_gt 1 renders on the GPU: not available with --dry_run 1"),
    ("--device_decode 3 --device_preprocess 1", "--device_decode is 0, 1 or 2"),
    ("--device_decode 2", "--device_decode 2 requires --device_preprocess 1"),
    ("--eval_3d 1", "--eval_3d 1 requires -t generate_result"),
    ("--eval_3d 1 -t generate_result --dry_run 1", "--eval_3d 1 scores on the GPU: not available with --dry_run 1"),
    ("--eval_maps 1 -t generate_train", "--eval_maps 1 requires -t generate_result"),
    ("--eval_maps 1 -t generate_result --dry_run 1", "--eval_maps 1 scores on the GPU: not available with --dry_run 1"),
    # two rules apply: the earlier check wins
    ("--eval_mupots X -t run_inference --dry_run 1", "--eval_mupots requires -t generate_result"),
    ("--eval_loss 1 -t generate_result --dry_run 1 --maps_from_gt 1", "--eval_loss 1 runs on the GPU: not available with --dry_run 1"),
]


@pytest.mark.parametrize("k", range(len(_REFUSALS)))
def test_flag_rules_refuse_with_their_message(k, capsys):
    """Every rule of FLAG_RULES through parse_args: argparse's refusal (exit status 2) with the message on stderr; rule k of the table is
    case k here, and it is the FIRST rule that applies to that command line."""
    cli = _cli()
    line, message = _REFUSALS[k]
    assert len(cli.FLAG_RULES) == 13
    with pytest.raises(SystemExit) as exc:
        cli.parse_args(line.split())
    assert exc.value.code == 2
    err = capsys.readouterr().err
    assert err.rstrip("\n").endswith("error: " + message), err
    if k < 13:
        assert cli.FLAG_RULES[k][1].format(device_decode=2) == message


@pytest.mark.parametrize("line", ["-t run_inference --dataset_path x --device_preprocess 1 --device_decode 2 --dry_run 1",
                                  "-t generate_result --eval_3d 1 --eval_maps 1 --eval_loss 1 --eval_mupots ROOT --device_preprocess 1 --device_decode 1",
                                  "-t generate_train -d generation --maps_from_gt 1"])
def test_parse_args_accepts_one_line_per_mode(line):
    args = _cli().parse_args(line.split())
    assert args.test_mode == line.split()[1] and args.batch_size == 1 and args.SMAP_path == "log/SMAP.pth"


def test_validation_loss_log_lines_on_the_host():
    """ValidationLoss.log_lines(raw): the one line the entry script logs; result_entry of the same raw as before."""
    from exps.stage3_root2.config import cfg
    from smap_amd.loss import ValidationLoss
    raw = [6.0, 3.0, 1.5, 0.75, 3.0, 2.0]
    vl = ValidationLoss(None, cfg, "cpu")
    assert vl.log_lines(raw) == ["validation loss over 3 frames in 2 batches: total 2  2d 1  bone 0.5  root 0.25"]
    assert vl.result_entry(raw) == {"loss": {"total_loss": 2.0, "loss_2d": 1.0, "loss_bone": 0.5, "loss_root": 0.25, "frames": 3, "batches": 2}}


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_loader_variants_without_a_device(mode, threads, tmp_path, monkeypatch):
    """DevicePreprocLoader with its device calls replaced by recorders (jpeg.reconstruct, jpeg.decode_coefficients_device -- status 0
    exactly where the host decoder decodes the file, the device decoder's contract -- and preprocess_batch; page-locking needs a GPU and
    is replaced by a copy): five files, batch 2, in the consumer's thread and on a pool of 3, for --device_decode 0, 1 and 2.  The
    "truncated" JPEG is cut inside its scan with the end-of-image marker kept: the native decoders refuse it and PIL decodes it.  (A file
    cut short at its end makes PIL raise, and so the run: tests/test_jpeg_huff_gpu.py.)"""
    import io
    import threading
    from PIL import Image
    from exps.stage3_root2.config import cfg
    from dataset.custom_dataset import CustomDataset
    from dataset.decode import read_bgr
    try:
        from smap_amd import jpeg as J, lib as L
        L.load()
    except Exception as e:                                    # a checkout without the built library: the parser is not faked
        pytest.skip(f"smap_amd.jpeg's host side needs the built library: {e!r}")
    import smap_amd.loaders as LD
    rng = np.random.default_rng(3)
    pics = [rng.integers(0, 256, (40 + 8 * k, 56, 3), dtype=np.uint8) for k in range(5)]
    for k in (0, 1):
        Image.fromarray(pics[k]).save(tmp_path / f"f{k}.jpg", quality=90)
    Image.fromarray(pics[2]).save(tmp_path / "f2.png")
    np.save(tmp_path / "f3.npy", pics[3])
    b = io.BytesIO()
    Image.fromarray(pics[4]).save(b, "JPEG", quality=90)
    whole = b.getvalue()
    (tmp_path / "f4.jpg").write_bytes(whole[:(J.probe(whole).scan_offset + len(whole)) // 2] + b"\xff\xd9")
    seen = []

    def fake_reconstruct(coeffs, info, device):
        assert coeffs is not None
        return ("reconstructed", J.output_shape(info))

    def fake_device_decode(frame, info, scan, device):
        co = J.decode_coefficients(J.frame_bytes(frame), info)
        return co, torch.tensor([0 if co is not None else 1], dtype=torch.int32)

    def fake_preprocess(raws, means, stds, device, **kw):
        assert not kw                                         # an image folder: the letter-box
        seen.append(list(raws))
        return torch.zeros((len(raws), 3, 2, 2)), {"scale": [1.0] * len(raws)}
    monkeypatch.setattr(J, "reconstruct", fake_reconstruct)
    monkeypatch.setattr(J, "decode_coefficients_device", fake_device_decode)
    monkeypatch.setattr(LD, "preprocess_batch", fake_preprocess)
    monkeypatch.setattr(LD, "pinned", lambda img: torch.from_numpy(np.array(img)))
    monkeypatch.setenv("SMAP_DECODE_THREADS", str(threads))
    monkeypatch.delenv("SMAP_DECODE_PROCS", raising=False)
    ds = CustomDataset(cfg, str(tmp_path))
    names = [ds.name(i) for i in range(len(ds))]             # the listing's order: the file order of the run
    assert sorted(names) == ["f0.jpg", "f1.jpg", "f2.png", "f3.npy", "f4.jpg"]
    loader = LD.DevicePreprocLoader(ds, range(len(ds)), 2, cfg, torch.device("cpu"), device_decode=mode)
    assert len(loader) == 3
    before, during, got = threading.active_count(), [], []
    for imgs, batch_names, scales in loader:
        during.append(threading.active_count())
        got.append((len(imgs), list(batch_names)))
    assert got == [(2, names[0:2]), (2, names[2:4]), (1, names[4:5])]               # file order, a ragged last batch of one frame
    if threads == 1:
        assert max(during) <= before                          # nothing was started
    raws = dict(zip(names, [r for batch in seen for r in batch]))
    for n in ("f2.png", "f3.npy", "f4.jpg"):                  # the PNG, the .npy and the truncated JPEG arrive as frames decoded on the host
        assert np.array_equal(np.asarray(raws[n]), read_bgr(str(tmp_path / n))), n
    for k, n in enumerate(("f0.jpg", "f1.jpg")):
        if mode:
            assert raws[n] == ("reconstructed", pics[k].shape[:2])
        else:
            assert np.array_equal(np.asarray(raws[n]), read_bgr(str(tmp_path / n)))
    # the parent's rules: PIL frames are counted under --device_decode only, .npy frames never; mode 2 redoes on the host what the device refuses
    assert (loader.pil_frames, loader.host_frames) == {0: (0, 0), 1: (2, 0), 2: (2, 1)}[mode]
