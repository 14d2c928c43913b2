"""GPU suite of the ground-truth modes' device loader: smap_preprocess_batch against the host path (resize_linear_u8, the clipped paste
of JointDataset.__getitem__, float().div(255), (t - mean) / std on the CPU), DevicePreprocLoader on an annotated set against
get_test_loader, and `test.py -t generate_result|generate_train --device_preprocess 1 [--device_decode 1|2]` against the same command
without the flags.  Every comparison is torch.equal / == : there is no tolerance in this file."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_ref as R
from helpers import make_cfg
from recipe import recipe_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
MEANS, STDS = [0.406, 0.456, 0.485], [0.225, 0.224, 0.229]
SENTINEL = -777.0


# ------------------------------------------------------------------------------------------------------------------ kernel
def _host(img, window, fx, fy, net_h, net_w):
    """The host path of dataset/base_dataset.py::JointDataset.__getitem__ for one frame."""
    from smap_amd.preprocess import resize_linear_u8
    nh, nw, top, left = window
    r = resize_linear_u8(img, nh, nw, fx=fx, fy=fy)
    canvas = np.full((net_h, net_w, 3), 128, np.uint8)
    x0, y0 = max(left, 0), max(top, 0)
    x1, y1 = min(left + nw, net_w), min(top + nh, net_h)
    if x1 > x0 and y1 > y0:
        canvas[y0:y1, x0:x1] = r[y0 - top:y1 - top, x0 - left:x1 - left]
    t = torch.from_numpy(canvas).permute(2, 0, 1).float().div(255.0)
    return (t - torch.tensor(MEANS).view(3, 1, 1)) / torch.tensor(STDS).view(3, 1, 1)


def _croppad(h, w, net_h, net_w, seed, stored=None):
    """(frame, window, fx, fy) of an h x w annotation entry in crop-and-pad geometry; `stored`: the file's own size where it differs."""
    from dataset.base_dataset import croppad_geometry
    scale, (nh, nw), (left, top) = croppad_geometry(w, h, net_w, net_h)
    sh, sw = stored or (h, w)
    return np.random.default_rng(seed).integers(0, 256, (sh, sw, 3), dtype=np.uint8), (nh, nw, top, left), scale, scale


def _device(frames, net_h, net_w, misalign=0):
    """smap_preprocess_batch on `frames` = [(frame, window, fx, fy)], each from its own device buffer -> [B,3,net_h,net_w] on the CPU.
    The output is allocated with one more frame (and `misalign` floats in front) of a sentinel that must come back untouched."""
    from smap_amd import lib as L
    lib = L.load()
    B, n = len(frames), 3 * net_h * net_w
    buf = torch.full((misalign + (B + 1) * n,), SENTINEL, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[misalign:]
    srcs = [torch.from_numpy(np.ascontiguousarray(f[0])).to(DEV) for f in frames]
    table = (L.PrepFrame * B)(*[L.PrepFrame(s.data_ptr(), f[0].shape[0], f[0].shape[1], *[int(v) for v in f[1]], float(f[2]), float(f[3]))
                                for s, f in zip(srcs, frames)])
    rc = lib.smap_preprocess_batch(table, B, C.c_void_p(out.data_ptr()), net_h, net_w, (C.c_float * 3)(*MEANS), (C.c_float * 3)(*STDS),
                                   C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.all(got[:misalign] == SENTINEL) and torch.all(got[misalign + B * n:] == SENTINEL), "wrote outside its frames"
    return got[misalign:misalign + B * n].view(B, 3, net_h, net_w)


def _check(frames, net_h, net_w, misalign=0):
    got = _device(frames, net_h, net_w, misalign)
    for b, (img, window, fx, fy) in enumerate(frames):
        want = _host(img, window, fx, fy, net_h, net_w)
        assert torch.equal(got[b], want), (b, img.shape, window, (got[b] - want).abs().max().item(),
                                           torch.nonzero(got[b] != want)[:4].tolist())


SIX = [(64, 96), (40, 97), (5, 7), (1, 1), (32, 48), (67, 33)]           # exact 2x | left = 1, one column clipped | upscale x6.4 |
#                                                                          window at (24, 16), 32 x 32 | identity | tall


def _six(net_h=32, net_w=48):
    return [_croppad(h, w, net_h, net_w, seed=10 + i) for i, (h, w) in enumerate(SIX)]


def _constructed(net_h=32, net_w=48):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (20, 31, 3), dtype=np.uint8)
    return [(img, (30, 46, -3, -5), 46 / 31, 30 / 20),                                      # negative offsets: clipped top and left
            (img, (30, 46, net_h - 2, net_w - 3), 46 / 31, 30 / 20),                        # overhangs bottom and right by most of itself
            (img, (10, 12, net_h, 4), 12 / 31, 10 / 20),                                    # wholly below the canvas: all padding
            (img, (10, 12, 3, -12), 12 / 31, 10 / 20),                                      # wholly left of it
            (img, (10, 12, -10, net_w + 7), 12 / 31, 10 / 20),                              # above and right of it
            _croppad(41, 98, net_h, net_w, seed=6, stored=(40, 97)),                        # h, w one less than the geometry assumed
            _croppad(64, 96, net_h, net_w, seed=7, stored=(63, 95))]                        # ... on the 2x box-mean path


def test_crop_pad_geometry_of_the_six_sources_is_what_the_cases_are_named_for():
    f = _six()
    assert f[0][1] == (32, 48, 0, 0) and f[0][2] == 0.5
    assert f[1][1][1:] == (48, 7, 1) and f[1][1][3] + f[1][1][1] == 49                      # one column clipped
    assert f[3][1] == (32, 32, 16, 24)
    assert f[4][1] == (32, 48, 0, 0) and f[4][2] == 1.0


@pytest.mark.parametrize("k", range(len(SIX)))
def test_batch_of_one(k):
    _check([_six()[k]], 32, 48)


def test_six_sizes_in_one_launch():
    _check(_six(), 32, 48)


def test_constructed_windows_clip_like_the_host_paste():
    frames = _constructed()
    _check(frames, 32, 48)
    got = _device(frames[2:5], 32, 48)
    pad = _host(frames[2][0], (1, 1, 99, 99), 1.0, 1.0, 32, 48)
    assert all(torch.equal(g, pad) for g in got)                                            # a window off the canvas: a frame of padding


def test_seventeen_frames_take_two_launches():
    pool = _six() + _constructed()
    _check([pool[i % len(pool)] for i in range(17)], 32, 48)


def test_scalar_path_canvas_width_not_a_multiple_of_four():
    _check([_croppad(h, w, 32, 50, seed=30 + i) for i, (h, w) in enumerate(SIX + [(64, 100), (41, 101)])], 32, 50)


def test_scalar_path_destination_off_16_byte_alignment():
    _check(_six() + _constructed(), 32, 48, misalign=1)


def test_full_canvas_from_a_1080_by_1921_frame():
    f = _croppad(1080, 1921, 512, 832, seed=40)
    assert f[1] == (468, 832, 23, 1)                                                       # left = 1, nw = 832: one column clipped
    _check([f, _croppad(75, 100, 512, 832, seed=41)], 512, 832)                             # + top = 4, nh = 512: four rows clipped


def test_letterbox_geometry_equals_calls_of_smap_preprocess():
    from smap_amd import lib as L
    from smap_amd.preprocess import letterbox_geometry
    lib = L.load()
    frames = []
    for i, (h, w) in enumerate(SIX + [(30, 100), (100, 30)]):
        scale, window = letterbox_geometry(w, h, 48, 32)
        frames.append((np.random.default_rng(50 + i).integers(0, 256, (h, w, 3), dtype=np.uint8), window, scale["scale"], scale["scale"]))
    got = _device(frames, 32, 48)
    one = torch.empty((len(frames), 3, 32, 48), dtype=torch.float32, device=DEV)
    for b, (img, (nh, nw, top, left), fx, fy) in enumerate(frames):
        src = torch.from_numpy(img).to(DEV)
        rc = lib.smap_preprocess(C.c_void_p(src.data_ptr()), img.shape[0], img.shape[1], nh, nw, top, left, C.c_void_p(one[b].data_ptr()), 32, 48,
                                 (C.c_float * 3)(*MEANS), (C.c_float * 3)(*STDS), fx, fy, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
    assert torch.equal(got, one.cpu())
    for b, f in enumerate(frames):                                                          # and both are the host path
        assert torch.equal(got[b], _host(*f, 32, 48))


def test_preprocess_batch_with_geometries_and_an_empty_window():
    """smap_amd.preprocess.preprocess_batch(geometries=...): the crop-and-pad windows, and a 1 x 1024 strip whose resized width rounds to
    0 -- the host path pastes nothing and leaves a frame of padding, and so does this one."""
    from dataset.base_dataset import croppad_geometry
    from smap_amd.preprocess import preprocess_batch
    frames = [_croppad(h, w, 512, 832, seed=70 + i) for i, (h, w) in enumerate([(60, 97), (1024, 1)])]
    assert frames[1][1][:2] == (512, 0) and croppad_geometry(1, 1024, 832, 512)[1] == (512, 0)
    metas = [dict(scale=f[2], img_width=f[0].shape[1], img_height=f[0].shape[0], net_width=832, net_height=512) for f in frames]
    got, scales = preprocess_batch([f[0] for f in frames], MEANS, STDS, DEV, geometries=[(m, f[1], f[2], f[3]) for m, f in zip(metas, frames)])
    torch.cuda.synchronize()
    for b, f in enumerate(frames):
        assert torch.equal(got[b].cpu(), _host(*f, 512, 832)), b
    assert scales["img_width"] == [97, 1] and scales["scale"] == [frames[0][2], frames[1][2]]
    assert len(torch.unique(got[1, 0])) == 1                                                # the strip: padding everywhere


def test_argument_errors():
    from smap_amd import lib as L
    lib = L.load()
    src = torch.zeros((4, 4, 3), dtype=torch.uint8, device=DEV)
    dst = torch.full((2, 3, 8, 8), SENTINEL, dtype=torch.float32, device=DEV)
    mean, std, st = (C.c_float * 3)(*MEANS), (C.c_float * 3)(*STDS), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def frame(**kw):
        f = L.PrepFrame(src.data_ptr(), 4, 4, 4, 4, 0, 0, 1.0, 1.0)
        for k, v in kw.items():
            setattr(f, k, v)
        return f
    ok = frame()
    d = C.c_void_p(dst.data_ptr())
    E_ARG = -1
    assert lib.smap_preprocess_batch((L.PrepFrame * 1)(ok), 0, d, 8, 8, mean, std, st) == E_ARG
    assert lib.smap_preprocess_batch((L.PrepFrame * 1)(ok), -1, d, 8, 8, mean, std, st) == E_ARG
    assert lib.smap_preprocess_batch(None, 1, d, 8, 8, mean, std, st) == E_ARG
    assert lib.smap_preprocess_batch((L.PrepFrame * 1)(ok), 1, None, 8, 8, mean, std, st) == E_ARG
    assert lib.smap_preprocess_batch((L.PrepFrame * 1)(ok), 1, d, 8, 8, None, std, st) == E_ARG
    assert lib.smap_preprocess_batch((L.PrepFrame * 1)(ok), 1, d, 8, 8, mean, None, st) == E_ARG
    assert lib.smap_preprocess_batch((L.PrepFrame * 1)(ok), 1, d, 0, 8, mean, std, st) == E_ARG
    assert lib.smap_preprocess_batch((L.PrepFrame * 1)(ok), 1, d, 8, -8, mean, std, st) == E_ARG
    for kw in (dict(src=None), dict(h=0), dict(w=0), dict(h=-4), dict(nh=0), dict(nw=0), dict(nh=-1), dict(nw=-1)):
        assert lib.smap_preprocess_batch((L.PrepFrame * 2)(ok, frame(**kw)), 2, d, 8, 8, mean, std, st) == E_ARG, kw
    torch.cuda.synchronize()
    assert torch.all(dst == SENTINEL)                                                       # a refused batch launches nothing
    assert lib.smap_preprocess_batch((L.PrepFrame * 2)(ok, ok), 2, d, 8, 8, mean, std, st) == 0
    torch.cuda.synchronize()
    assert not torch.any(dst == SENTINEL)


# ------------------------------------------------------------------------------------------------------------------ loader
LOADER_SIZES = [(60, 97), (75, 100), (1024, 1664), (128, 208), (33, 67)]     # odd width | four rows clipped | exact 2x | x4 | tall-ish, odd
OFF_BY_ONE = 3                                                               # this entry's JSON says one more than its file holds


def _write_loader_set(root, ext):
    rng = np.random.default_rng(21)
    entries = []
    for i, (h, w) in enumerate(LOADER_SIZES):
        os.makedirs(os.path.join(root, f"TS{i + 1}"), exist_ok=True)
        rel = f"TS{i + 1}/img_{i:06d}.{ext}"
        if ext == "npy":
            np.save(os.path.join(root, rel), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        else:
            with open(os.path.join(root, rel), "wb") as f:
                f.write(R.encode(R.content("noise" if i % 2 else "smooth", h, w, i), 90, ("4:2:0", "4:4:4", "4:2:2")[i % 3]))
        jh, jw = (h + 1, w + 1) if i == OFF_BY_ONE else (h, w)
        bodys = np.zeros((1 + i % 3, 15, 11))
        bodys[:, :, 0] = rng.uniform(0, w, bodys.shape[:2])
        bodys[:, :, 1] = rng.uniform(0, h, bodys.shape[:2])
        bodys[:, :, 2] = rng.uniform(200, 500, bodys.shape[:2])
        bodys[:, :, 3] = 2
        bodys[:, :, 7:11] = [1500.0, 1490.0, w / 2, h / 2]
        entries.append({"dataset": "MUCO", "img_paths": rel, "img_width": jw, "img_height": jh, "isValidation": 1, "bodys": bodys.tolist()})
    with open(os.path.join(root, "M3E_gt.json"), "w") as f:
        json.dump({"root": entries}, f)


@pytest.fixture(scope="module")
def loader_sets(tmp_path_factory):
    """{ext: (folder, the host loader's batches)}: the same five frames as .npy and as baseline JPEG, batch 2 (a ragged tail)."""
    from exps.stage3_root2.config import cfg
    from lib.utils.dataloader import get_test_loader
    base = tmp_path_factory.mktemp("gt_sets")
    keep = (cfg.TEST.ROOT_PATH, cfg.TEST.JSON_PATH, cfg.TEST.IMG_PER_GPU)
    out = {}
    try:
        for ext in ("npy", "jpg"):
            root = str(base / ext)
            _write_loader_set(root, ext)
            cfg.TEST.ROOT_PATH, cfg.TEST.JSON_PATH, cfg.TEST.IMG_PER_GPU = root, os.path.join(root, "M3E_gt.json"), 2
            out[ext] = (root, list(get_test_loader(cfg, 1, 0, "test")))
    finally:
        cfg.TEST.ROOT_PATH, cfg.TEST.JSON_PATH, cfg.TEST.IMG_PER_GPU = keep
    return out


@pytest.mark.parametrize("ext,env,device_decode,relative", [
    ("npy", {"SMAP_DECODE_THREADS": "1"}, 0, False), ("npy", {"SMAP_DECODE_THREADS": "4"}, 0, False),
    ("npy", {"SMAP_DECODE_PROCS": "2"}, 0, True),
    ("jpg", {"SMAP_DECODE_THREADS": "4"}, 0, False), ("jpg", {"SMAP_DECODE_PROCS": "2"}, 0, True),
    ("jpg", {"SMAP_DECODE_THREADS": "4"}, 1, False), ("jpg", {"SMAP_DECODE_THREADS": "1"}, 1, False),
    ("jpg", {"SMAP_DECODE_THREADS": "4"}, 2, False), ("jpg", {"SMAP_DECODE_THREADS": "1"}, 2, False)])
def test_device_loader_equals_host_loader(loader_sets, monkeypatch, ext, env, device_decode, relative):
    from dataset.base_dataset import JointDataset
    from exps.stage3_root2.config import cfg
    from exps.stage3_root2.test import DevicePreprocLoader
    root, host = loader_sets[ext]
    for k in ("SMAP_DECODE_THREADS", "SMAP_DECODE_PROCS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if relative:                                   # a relative root, from a directory that is not the repository's: the workers run elsewhere
        monkeypatch.chdir(os.path.dirname(root))
        assert os.getcwd() != ROOT
        root = os.path.basename(root)
    monkeypatch.setitem(cfg.TEST, "ROOT_PATH", root)
    monkeypatch.setitem(cfg.TEST, "JSON_PATH", os.path.join(root, "M3E_gt.json"))
    ds = JointDataset(cfg, "test")
    assert ds.geometry(OFF_BY_ONE)[0]["img_width"] == LOADER_SIZES[OFF_BY_ONE][1] + 1
    loader = DevicePreprocLoader(ds, range(len(ds)), 2, cfg, DEV, device_decode=device_decode)
    assert len(loader) == len(host) == 3
    got = list(loader)
    torch.cuda.synchronize()
    assert len(got) == len(host)
    for (g_img, g_ann, g_path, g_meta), (h_img, h_ann, h_path, h_meta) in zip(got, host):
        assert g_img.device.type == "cuda" and g_img.dtype == torch.float32 and g_img.shape == h_img.shape
        assert torch.equal(g_img.cpu(), h_img), (g_path, (g_img.cpu() - h_img).abs().max().item())
        assert g_ann.dtype == torch.float32 and torch.equal(g_ann, h_ann)
        assert isinstance(g_path, tuple) and g_path == h_path
        assert isinstance(g_meta, tuple) and g_meta == h_meta
    assert len(got[-1][0]) == 1                                                             # the ragged tail
    if device_decode:
        assert loader.pil_frames == 0                                                       # every frame is a baseline JPEG: none left to PIL


# --------------------------------------------------------------------------------------------------------------------- CLI
@pytest.mark.parametrize("mode,data_mode,extra", [("generate_result", "test", ["--eval_3d", "1"]), ("generate_result", "test", []),
                                                  ("generate_train", "generation", [])])
def test_cli_ground_truth_modes_on_the_device_loader(tmp_path, mode, data_mode, extra):
    """The flags act in the ground-truth modes and change nothing in the result file: an annotated set of .npy, baseline JPEG and one
    progressive JPEG frames (odd widths among them), batch 2."""
    from PIL import Image
    from model.smap import SMAP
    from model.refinenet import RefineNet
    from test_entry_gpu import _annotated_set
    torch.manual_seed(0)
    net = SMAP(make_cfg((128, 208))).eval()
    sd = recipe_state_dict(net.state_dict())
    for k in list(sd):
        if k.endswith("up4.res_conv2.bn.bias"):
            sd[k] = sd[k] + 40.0
    net.load_state_dict(sd)
    rsd = recipe_state_dict(RefineNet().state_dict())
    torch.save({"model": sd}, tmp_path / "SMAP.pth")
    torch.save(rsd, tmp_path / "RefineNet.pth")
    from exps.stage3_root2.config import cfg
    keep = (cfg.TEST.ROOT_PATH, cfg.TEST.JSON_PATH)
    try:
        root = _annotated_set(tmp_path, net.to(DEV), "cuda:0", [(512, 833), (480, 641), (300, 400), (601, 800), (256, 417), (600, 801), (511, 832)], seed=11)
    finally:
        cfg.TEST.ROOT_PATH, cfg.TEST.JSON_PATH = keep
    # frames 2 and 3 stay .npy, the others become JPEGs (4:4:4, quality 98: the network sees nearly the frame the annotations were placed on),
    # frame 4 a progressive one: the device decoders hand it to PIL.  isValidation (i % 3 != 0) puts 1, 2, 4, 5 into `test`, 0, 3, 6 into `generation`
    muco = tmp_path / "data" / "MuCo"
    for js, top in ((root / "M3E_gt.json", root), (muco / "annotations" / "MuCo.json", muco)):
        entries = json.loads(js.read_text())["root"]
        for i, e in enumerate(entries):
            if i in (2, 3):
                continue
            rgb = np.ascontiguousarray(np.load(top / e["img_paths"])[:, :, ::-1])
            os.remove(top / e["img_paths"])
            e["img_paths"] = e["img_paths"][:-4] + ".jpg"
            if i == 4:
                Image.fromarray(rgb).save(top / e["img_paths"], "JPEG", progressive=True, quality=85)    # (4:2:0: Pillow cannot write
                #                                                                                    progressive 4:4:4 noise at high quality)
            else:
                (top / e["img_paths"]).write_bytes(R.encode(rgb, 98, "4:4:4"))
        js.write_text(json.dumps({"root": entries}))
    n_frames, n_pil = (4, 1) if data_mode == "test" else (3, 0)
    res, logs = {}, {}
    for tag, flags in (("host", []), ("dev", ["--device_preprocess", "1"]), ("dec1", ["--device_preprocess", "1", "--device_decode", "1"]),
                       ("dec2", ["--device_preprocess", "1", "--device_decode", "2"])):
        env = dict(os.environ, PROJECT_HOME=str(tmp_path), SMAP_TEST_ROOT=str(root), SMAP_DECODE_THREADS="3",
                   SMAP_PLAN_CACHE=str(tmp_path / "plan_cache"),                            # the first run builds the schedule, the others load it
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "exps", "stage3_root2", "test.py"), "-p", str(tmp_path / "SMAP.pth"),
                            "-rp", str(tmp_path / "RefineNet.pth"), "-t", mode, "-d", data_mode, "--batch_size", "2", "--json_name", tag]
                           + extra + flags, capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        logs[tag] = r.stderr
        res[tag] = json.loads((tmp_path / "model_logs" / "stage3_root2" / "result" / f"stage3_root2_{mode}_{data_mode}_{tag}.json").read_text())
    assert len(res["host"]["3d_pairs"]) >= 1, "the set-up must produce records"
    assert ("error" in res["host"]) == bool(extra)
    for tag in ("dev", "dec1", "dec2"):
        assert res[tag] == res["host"], tag                                                 # the whole file, the `error` dict included
    assert "device decode:" not in logs["host"] and "device decode:" not in logs["dev"]
    assert "device decode: {} of {} frames fell back to PIL".format(n_pil, n_frames) in logs["dec1"]
    assert re.search(r"device decode: \d+ of {} frames were redone on the host, {} fell back to PIL".format(n_frames, n_pil), logs["dec2"])
