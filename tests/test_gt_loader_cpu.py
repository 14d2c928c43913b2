"""CPU suite of the ground-truth modes' device loader: what JointDataset hands the loader (raw / path / name / geometry / extras), the
per-rank split of test.py's main(), the facts about croppad_geometry the clipped pre-processing window rests on, and the export of
smap_preprocess_batch."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_set(root, sizes, stored=None, seed=3):
    """`sizes`: (h, w) the JSON states per frame; `stored`: (h, w) of the .npy file where it differs."""
    rng = np.random.default_rng(seed)
    entries = []
    for i, (h, w) in enumerate(sizes):
        sh, sw = (stored or {}).get(i, (h, w))
        os.makedirs(os.path.join(root, f"TS{i + 1}"), exist_ok=True)
        np.save(os.path.join(root, f"TS{i + 1}", f"img_{i:06d}.npy"), rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8))
        bodys = np.zeros((1 + i % 3, 15, 11))
        bodys[:, :, 0] = rng.uniform(-20, w + 20, bodys.shape[:2])                 # some joints leave the canvas: score 0
        bodys[:, :, 1] = rng.uniform(-20, h + 20, bodys.shape[:2])
        bodys[:, :, 2] = rng.uniform(200, 500, bodys.shape[:2])
        bodys[:, :, 3] = 2
        bodys[:, :, 7:11] = [1500.0, 1490.0, w / 2, h / 2]
        entries.append({"dataset": "MUCO", "img_paths": f"TS{i + 1}/img_{i:06d}.npy", "img_width": w, "img_height": h,
                        "isValidation": 1, "bodys": bodys.tolist()})
    with open(os.path.join(root, "M3E_gt.json"), "w") as f:
        json.dump({"root": entries}, f)
    return entries


@pytest.fixture
def gt_cfg(tmp_path, monkeypatch):
    from exps.stage3_root2.config import cfg
    monkeypatch.setitem(cfg.TEST, "ROOT_PATH", str(tmp_path))
    monkeypatch.setitem(cfg.TEST, "JSON_PATH", str(tmp_path / "M3E_gt.json"))
    return cfg


def test_raw_is_getitem_without_the_preprocessing(tmp_path, gt_cfg):
    from dataset.base_dataset import JointDataset, croppad_geometry
    sizes = [(75, 100), (60, 97), (33, 67), (64, 104)]
    _write_set(str(tmp_path), sizes, stored={2: (32, 66)})                           # entry 2: the JSON is off by one from the file
    ds = JointDataset(gt_cfg, "test")
    assert len(ds) == len(sizes)
    for i, (h, w) in enumerate(sizes):
        _, ann, path, meta = ds[i]
        frame, r_ann, r_path, r_meta, geometry = ds.raw(i)
        assert frame.dtype == np.uint8 and np.array_equal(frame, np.load(ds.path(i)))           # the decoded frame as it is
        assert frame.shape[:2] == ((32, 66) if i == 2 else (h, w))
        assert r_ann.dtype == torch.float32 and torch.equal(r_ann, ann)
        assert r_path == path == ds.name(i) and ds.path(i) == os.path.join(str(tmp_path), path)
        assert r_meta == meta and set(meta) == {"scale", "img_width", "img_height", "net_width", "net_height"}
        scale, (nh, nw), (left, top) = croppad_geometry(w, h, 832, 512)              # from the ANNOTATION's size, also for entry 2
        assert geometry == (meta, (nh, nw, top, left), scale, scale) == ds.geometry(i)
        e_ann, e_meta = ds.extras(i)
        assert torch.equal(e_ann, ann) and e_meta == meta


def test_custom_dataset_answers_the_same_protocol(tmp_path):
    from dataset.custom_dataset import CustomDataset
    from exps.stage3_root2.config import cfg
    (tmp_path / "sub").mkdir()
    np.save(tmp_path / "sub" / "a.npy", np.zeros((4, 5, 3), np.uint8))
    ds = CustomDataset(cfg, str(tmp_path))
    assert ds.path(0) == str(tmp_path / "sub" / "a.npy") and ds.name(0) == "sub/a.npy" == ds.raw(0)[1] == ds[0][1]
    assert ds.geometry(0) is None and ds.extras(0) is None and ds.raw(0)[0].shape == (4, 5, 3)


@pytest.mark.parametrize("n", [1, 7, 10])
def test_rank_split_is_get_test_loaders(tmp_path, gt_cfg, n):
    from lib.utils.dataloader import get_test_loader, rank_block
    entries = [{"dataset": "MUCO", "img_paths": f"f{i}.npy", "img_width": 8, "img_height": 8, "isValidation": 1,
                "bodys": np.zeros((1, 15, 11)).tolist()} for i in range(n)]
    (tmp_path / "M3E_gt.json").write_text(json.dumps({"root": entries}))
    for world in (1, 4, 8):
        seen = []
        for rank in range(world):
            want = list(get_test_loader(gt_cfg, world, rank, "test").dataset.indices)
            st, ed = rank_block(n, world, rank)
            assert list(range(st, ed)) == want, (n, world, rank)
            assert 0 <= st <= ed <= n
            seen += want
        assert seen == list(range(n))                                                # every frame once, in order
        if n < world:
            assert rank_block(n, world, world - 1)[0] == rank_block(n, world, world - 1)[1]      # empty tail ranks


def test_croppad_window_never_starts_before_the_canvas_and_may_overhang():
    from dataset.base_dataset import croppad_geometry
    overhang = 0
    for w in range(1, 2100, 7):
        for h in range(1, 2100, 11):
            _, (nh, nw), (left, top) = croppad_geometry(w, h, 832, 512)
            assert left >= 0 and top >= 0, (w, h)
            overhang += left + nw > 832 or top + nh > 512
    assert overhang == 32131
    _, (nh, nw), (left, top) = croppad_geometry(1921, 1080, 832, 512)
    assert (left, nw) == (1, 832) and left + nw == 833                                # one column clipped
    _, (nh, nw), (left, top) = croppad_geometry(100, 75, 832, 512)
    assert (top, nh) == (4, 512) and top + nh == 516                                  # four rows clipped
    _, (nh, nw), (left, top) = croppad_geometry(1, 1, 832, 512)
    assert (left, top, nh, nw) == (416, 256, 512, 512)


def test_library_exports_and_binds_preprocess_batch():
    from smap_amd import lib as L
    assert "smap_preprocess_batch" in L.SYMBOLS
    so = ctypes.CDLL(L.SO_PATH)
    assert hasattr(so, "smap_preprocess_batch")
    lib = L.load()
    assert lib.smap_preprocess_batch.argtypes is not None and len(lib.smap_preprocess_batch.argtypes) == 8
    assert lib.smap_sizeof_prep_frame() == ctypes.sizeof(L.PrepFrame) == 48
    hdr = open(os.path.join(ROOT, "include", "smap_hip.h")).read()
    assert "#define SMAP_PREP_MAX_FRAMES %d\n" % L.PREP_MAX_FRAMES in hdr
    # argument errors are decided on the host, before anything touches a device
    mean, std = (ctypes.c_float * 3)(0.4, 0.4, 0.4), (ctypes.c_float * 3)(0.2, 0.2, 0.2)
    ok = L.PrepFrame(0x1000, 4, 4, 4, 4, 0, 0, 1.0, 1.0)
    one = (L.PrepFrame * 1)(ok)
    dst = ctypes.c_void_p(0x2000)
    assert lib.smap_preprocess_batch(one, 0, dst, 8, 8, mean, std, None) == -1
    assert lib.smap_preprocess_batch(one, 1, None, 8, 8, mean, std, None) == -1
    assert lib.smap_preprocess_batch(None, 1, dst, 8, 8, mean, std, None) == -1
    assert lib.smap_preprocess_batch(one, 1, dst, 0, 8, mean, std, None) == -1
    assert lib.smap_preprocess_batch(one, 1, dst, 8, 8, None, std, None) == -1
    for field, bad in (("src", None), ("h", 0), ("w", -1), ("nh", 0), ("nw", 0), ("fx", 0.0), ("fy", float("nan"))):
        f = L.PrepFrame(0x1000, 4, 4, 4, 4, 0, 0, 1.0, 1.0)
        setattr(f, field, bad)
        assert lib.smap_preprocess_batch((L.PrepFrame * 2)(ok, f), 2, dst, 8, 8, mean, std, None) == -1, field
