"""CPU suite of the training-sample path (smap_amd/augment.py, csrc/cubic_table.cpp, the argument checks of csrc/augment.hip,
dataset/ImageAugmentation.py, lib/utils/dataloader.py::get_train_loader): no GPU is touched.

tests/golden/augment.npz (tests/golden/gen_golden_augment.py) pins the control flow, the annotation arithmetic and the crop geometry by
EXECUTING the reference's functions; the pixel arithmetic of warpAffine / resize inside its canvases is restated from OpenCV's published
algorithm, not executed (cv2 is not installed)."""
import copy
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest
import torch

from smap_amd import augment as A
from smap_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "augment.npz"))
NAMES = [str(n) for n in GOLD["names"]]
MEANS, STDS = [0.406, 0.456, 0.485], [0.225, 0.224, 0.229]


def scene(name):
    """(entry, image, draws, params, with_augmentation, canvas shape) of a fixture scene."""
    crop_y, crop_x = (int(v) for v in GOLD[name + "_canvas_shape"])
    img = GOLD[str(GOLD[name + "_image_key"])]
    entry = {"dataset": str(GOLD[name + "_dataset"]), "img_height": img.shape[0], "img_width": img.shape[1], "isValidation": 0,
             "img_paths": name + ".npy", "bodys": GOLD[name + "_in_bodys"].tolist()}
    params = A.AugParams(crop_x, crop_y, 40, 10, 0.5, 0.8, 1.1, tuple(int(k) for k in GOLD["flip_order"]))
    return entry, img, tuple(float(d) for d in GOLD[name + "_draws"]), params, bool(GOLD[name + "_with_aug"]), (crop_y, crop_x)


def test_fixture_holds_the_scenes_the_kernel_can_go_wrong_on():
    assert len(NAMES) >= 12 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "augment.npz")) < 400 * 1024
    shapes = {tuple(int(v) for v in GOLD[n + "_canvas_shape"]) for n in NAMES}
    assert shapes == {(64, 96), (37, 50)}                # the vector path (width % 4 == 0) and the scalar path
    assert not GOLD["rotate_off_with_aug"] and (GOLD["invisible_bodys"][:, :, 3] == 0).all()
    assert 0 < (GOLD["joints_leave_bodys"][:, :, 3] > 0).sum() < 30


def _c_table():
    out = np.empty(1024 * 16, np.int16)
    assert L.load().smap_cubic_table(C.c_void_p(out.ctypes.data)) == 0
    return out.reshape(1024, 16)


def test_cubic_table_of_the_library_equals_the_restatement_bit_for_bit():
    tab = _c_table()
    assert np.array_equal(tab, A.cubic_table())
    assert (tab.astype(np.int64).sum(1) == 32768).all()
    # entry 0: the identity tap.  2^15 does not fit int16: saturate_cast leaves 32767 on the second row, and the sum fix-up puts the
    # missing 1 on the first entry it scans, [2][2] -- (32767 p + q + 2^14) >> 15 == p for any two 8-bit values
    assert tab[0].reshape(4, 4).tolist() == [[0, 0, 0, 0], [0, 32767, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]
    assert L.load().smap_cubic_table(None) == -1


def test_cubic_table_rows_without_a_vertical_offset():
    """fy = 0: the weights sit on the second row; the third holds at most the sum fix-up, the first and the last nothing."""
    t = A.cubic_table().astype(np.int64).reshape(32, 32, 4, 4)
    assert np.array_equal(t[0, :, 1, :].sum(1) + t[0, :, 2, :].sum(1), np.full(32, 32768))
    assert (t[0, :, 0, :] == 0).all() and (t[0, :, 3, :] == 0).all() and np.abs(t[0, :, 2, :]).max() <= 8


@pytest.mark.parametrize("name", NAMES)
def test_plan_sample_reproduces_the_reference(name):
    entry, img, draws, params, with_aug, _ = scene(name)
    bodys, meta, fields = A.plan_sample(entry, draws, params, with_aug)
    want = GOLD[name + "_bodys"]
    assert bodys.shape == want.shape
    assert np.abs(bodys[:, :, :2] - want[:, :, :2]).max() < 1e-9
    assert np.array_equal(bodys[:, :, 2:], want[:, :, 2:])                   # visibilities, depths, cameras: exactly
    assert meta["scale"] == float(GOLD[name + "_scale"])
    assert np.array_equal(np.asarray(meta["center"]), GOLD[name + "_center"])
    assert fields["rotate"] == int(with_aug) and fields["flip"] == int(with_aug and draws[4] <= 0.5)
    assert all(isinstance(fields[k], int) for k in ("rotate", "rh", "rw", "nh", "nw", "top", "left", "flip"))
    if str(GOLD[name + "_dataset"]) != "COCO" or not with_aug:               # the multiplier is for COCO entries only
        assert meta["scale"] == min(params.crop_x / float(fields["rw"]), params.crop_y / float(fields["rh"]))


@pytest.mark.parametrize("name", NAMES)
def test_staged_restatement_reproduces_the_recorded_canvas(name):
    entry, img, draws, params, with_aug, (crop_y, crop_x) = scene(name)
    _, _, fields = A.plan_sample(entry, draws, params, with_aug)
    assert np.array_equal(A.staged_canvas(img, fields, crop_y, crop_x), GOLD[name + "_canvas"])


def test_plan_without_augmentation_is_croppad_geometry():
    from dataset.base_dataset import croppad_geometry
    for w, h in ((1920, 1080), (640, 480), (641, 479), (2048, 2048)):
        entry = {"dataset": "MUCO", "img_width": w, "img_height": h, "bodys": np.zeros((1, 15, 11)).tolist()}
        _, meta, f = A.plan_sample(entry, (0.1, 0.9, 0.05, 0.7, 0.1), A.AugParams(832, 512, 40, 10, 0.5, 0.8, 1.1, tuple(range(15))), False)
        scale, (nh, nw), (left, top) = croppad_geometry(w, h, 832, 512)
        assert (meta["scale"], f["nh"], f["nw"], f["left"], f["top"], f["rotate"], f["flip"]) == (scale, nh, nw, left, top, 0, 0)


def test_plan_refuses_a_crop_that_leaves_the_padded_image():
    """A 40 px shift on the 37-row canvas: the reference's slice would end beyond the padded image (numpy truncates it to 36 rows) or
    start below 0 (numpy wraps)."""
    entry, img, draws, params, with_aug, _ = scene("shift_plus40")
    for dice_y in (1.0, 0.0):
        with pytest.raises(ValueError, match="padded image"):
            A.plan_sample(entry, (draws[0], draws[1], dice_y, draws[3], draws[4]), params, True)


def test_draw_takes_five_values_in_the_reference_order():
    a, b = random.Random(7), random.Random(7)
    assert A.draw(a) == tuple(b.random() for _ in range(5))


def smooth(h, w, seed=3):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 55 * np.sin(rng.uniform(0.03, 0.07) * x + rng.uniform(0.03, 0.07) * y + c) + 45 * np.cos(rng.uniform(0.02, 0.06) * x - 0.04 * y)
                    for c in range(3)], -1)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def test_warp_at_degree_zero_on_an_even_source_is_the_identity():
    img = smooth(40, 58)
    M, nW, nH = A.rotate_bound_matrix(40, 58, 0.0)
    assert (nW, nH) == (58, 40)
    assert np.array_equal(A.warp_affine_cubic_u8(img, M, (nW, nH)), img)
    M, nW, nH = A.rotate_bound_matrix(41, 57, 0.0)           # odd: shifted by half a pixel (nW / 2 - w // 2 = 0.5), not the identity
    assert (M[0, 2], M[1, 2]) == (0.5, 0.5)
    assert not np.array_equal(A.warp_affine_cubic_u8(smooth(41, 57), M, (nW, nH)), smooth(41, 57))


def _keys(t, k):
    """Keys' cubic (A = -0.75), weight of tap k in {-1, 0, 1, 2} at fraction t, float64."""
    a = -0.75
    d = np.abs(t - k)
    return np.where(d <= 1, ((a + 2) * d - (a + 3)) * d * d + 1, ((a * d - 5 * a) * d + 8 * a) * d - 4 * a)


def test_warp_against_a_float64_cubic_at_the_unquantised_coordinate():
    """The restated fixed-point warp against real arithmetic (DESIGN.md section 16 has the derivation).  On an image whose neighbouring
    pixels differ by at most g grey levels, with C1 = max_t sum_k |k| |w_k'(t)| and L1 = max_t sum_k |w_k(t)| of the Keys kernel:
      coordinate grid   each axis is off by at most 1/64 + 1/1024 px (nearest 1/32 of a sum of two values rounded at 1/1024)
                        -> 2 * (1/64 + 1/1024) * g * C1 * L1
      weight rounding   16 weights rounded at 2^-15 (<= 0.51 each with the float32 products) plus the sum fix-up (<= their total),
                        against differences of at most 4 g inside the footprint -> 2 * 16 * 0.51 * 4 g / 32768
      final rounding    0.5
    Measured on the restatement, here on the CPU, never on the kernel."""
    img = smooth(70, 90, seed=11)
    i64 = img.astype(np.float64)
    g = max(np.abs(np.diff(i64, axis=0)).max(), np.abs(np.diff(i64, axis=1)).max())
    assert 2 <= g <= 8
    t = np.linspace(0, 1, 20001)
    w = np.stack([_keys(t, k) for k in (-1, 0, 1, 2)])
    L1 = np.abs(w).sum(0).max()
    C1 = (np.abs(np.gradient(w, t, axis=1)) * np.abs(np.array([-1, 0, 1, 2]))[:, None]).sum(0).max() * 1.001
    bound = 2 * (1 / 64 + 1 / 1024) * g * C1 * L1 + 2 * 16 * 0.51 * 4 * g / 32768 + 0.5
    worst = 0.0
    for degree in (-10.0, 3.3, 10.0):
        M, nW, nH = A.rotate_bound_matrix(70, 90, degree)
        got = A.warp_affine_cubic_u8(img, M, (nW, nH)).astype(np.float64)
        m = A.invert_affine(M)
        yy, xx = np.mgrid[0:nH, 0:nW].astype(np.float64)
        u, v = m[0] * xx + m[1] * yy + m[2], m[3] * xx + m[4] * yy + m[5]
        inside = (u >= 2) & (u <= 90 - 4) & (v >= 2) & (v <= 70 - 4)          # the footprint, and its quantised twin, inside the image
        assert inside.sum() > 3000
        iu, iv = np.floor(u).astype(int), np.floor(v).astype(int)
        fu, fv = u - iu, v - iv
        ref = np.zeros((nH, nW, 3))
        for a in (-1, 0, 1, 2):
            for b in (-1, 0, 1, 2):
                px = i64[np.clip(iv + a, 0, 69), np.clip(iu + b, 0, 89)]
                ref += px * (_keys(fv, a) * _keys(fu, b))[..., None]
        err = np.abs(got - np.clip(ref, 0, 255))[inside].max()
        worst = max(worst, err)
    print("warp vs float64 cubic: max |error| %.4f grey levels, bound %.4f (g = %g, C1 = %.4f, L1 = %.4f)" % (worst, bound, g, C1, L1))
    assert worst <= bound


def test_augment_batch_refuses_bad_arguments_without_a_gpu():
    lib = L.load()
    mean, std = (C.c_float * 3)(*MEANS), (C.c_float * 3)(*STDS)
    src, dst, tab = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(16384)    # never dereferenced: every call is refused before a launch
    ident = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)

    def frame(**kw):
        f = dict(rotate=1, rh=20, rw=24, m=ident, nh=8, nw=8, top=0, left=0, fx=0.5, fy=0.5, flip=0)
        f.update({k: v for k, v in kw.items() if k not in ("src", "h", "w")})
        return A.aug_frame(kw.get("src", 4096), kw.get("h", 16), kw.get("w", 16), f)
    ok = frame()
    one = (L.AugFrame * 1)(ok)
    call = lambda frames, B, d=dst, nh=8, nw=8, mn=mean, sd=std, t=tab: lib.smap_augment_batch(frames, B, d, nh, nw, mn, sd, t, None)
    assert call(None, 1) == -1 and call(one, 0) == -1 and call(one, -3) == -1
    assert call(one, 1, d=None) == -1 and call(one, 1, mn=None) == -1 and call(one, 1, sd=None) == -1
    assert call(one, 1, nh=0) == -1 and call(one, 1, nw=-8) == -1
    assert call(one, 1, t=None) == -1                                        # a rotating frame needs the table ...
    assert call(one, 1, t=C.c_void_p(16384 + 2)) == -1                       # ... 16-byte aligned
    bad = [dict(src=None), dict(h=0), dict(w=-1), dict(rh=0), dict(rw=0), dict(fx=0.0), dict(fy=-1.0), dict(fx=float("nan")),
           dict(h=16385), dict(w=16385), dict(rh=16385), dict(rw=16385), dict(m=(1.0, 0.0, float("inf"), 0.0, 1.0, 0.0))]
    for kw in bad:
        assert call((L.AugFrame * 2)(ok, frame(**kw)), 2) == -1, kw
    for kw in (dict(nh=0), dict(nw=-2)):                                     # (aug_frame itself moves an empty window off the canvas)
        f = frame()
        for k, v in kw.items():
            setattr(f, k, v)
        assert call((L.AugFrame * 2)(ok, f), 2) == -1, kw
    assert lib.smap_sizeof_aug_frame() == C.sizeof(L.AugFrame) == 112


def test_reference_api_on_key_points(monkeypatch):
    from dataset import ImageAugmentation as IA
    rng = np.random.default_rng(5)
    bodys = rng.uniform(0, 90, (2, 15, 11))
    order = [0, 1, 2, 9, 10, 11, 12, 13, 14, 3, 4, 5, 6, 7, 8]
    params = {"flip_prob": 0.5, "flip_order": order, "crop_size_x": 96, "crop_size_y": 64}
    monkeypatch.setattr(IA.random, "random", lambda: 0.5)                    # dice <= flip_prob: flips
    meta, img = IA.aug_flip({"bodys": bodys.copy()}, None, params)
    assert img is None
    want = bodys.copy()
    want[:, :, 0] = 96 - 1 - want[:, :, 0]
    assert np.array_equal(meta["bodys"], want[:, order])
    monkeypatch.setattr(IA.random, "random", lambda: 0.75)
    assert np.array_equal(IA.aug_flip({"bodys": bodys.copy()}, None, params)[0]["bodys"], bodys)
    M, _, _ = A.rotate_bound_matrix(64, 96, 7.5)
    p = IA.rotate_skel2d(bodys[0][:, :2], M)
    assert p.shape == (15, 2) and np.allclose(p, bodys[0][:, :2] @ M[:, :2].T + M[:, 2], atol=1e-12)
    c = np.array([[96 // 2, 64 // 2]], np.float64)                           # the centre goes to the centre of the enlarged box
    _, nW, nH = A.rotate_bound_matrix(64, 96, 7.5)
    assert np.allclose(IA.rotate_skel2d(c, M), [[nW / 2, nH / 2]], atol=1e-12)
    for fn in ("aug_rotate", "aug_croppad", "aug_flip", "rotate_bound", "rotate_skel2d"):
        assert callable(getattr(IA, fn))


class StubSet:
    """What get_train_loader needs of a set before the first batch: a length."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_train_loader_index_stream():
    from exps.stage3_root2.config import cfg as base
    from lib.utils.dataloader import get_train_loader, train_batches
    cfg = copy.deepcopy(base)
    cfg.SOLVER.MAX_ITER, cfg.SOLVER.IMG_PER_GPU = 23, 2
    assert base.SOLVER.IMG_PER_GPU == 2 and base.SOLVER.MAX_ITER == 192000
    n = 11
    loaders = [get_train_loader(cfg, 2, is_dist=True, start_iter=3, dataset=StubSet(n), rank=r, device="cuda:0") for r in range(2)]
    for ld in loaders:
        assert len(ld) == 23 - 3 and ld.bs == 2 and len(ld.idx) == 40
    per_epoch = [{}, {}]
    for r, ld in enumerate(loaders):
        for epoch, index in ld.idx:
            per_epoch[r].setdefault(epoch, []).append(index)
    epochs = sorted(set(per_epoch[0]) & set(per_epoch[1]))
    assert len(epochs) >= 4
    full = [e for e in epochs if len(per_epoch[0][e]) == 6 and len(per_epoch[1][e]) == 5]
    assert len(full) >= 3
    for e in full:
        a, b = per_epoch[0][e], per_epoch[1][e]
        assert not set(a) & set(b) and sorted(a + b) == list(range(n))       # disjoint across the ranks, together the whole set
    assert len({tuple(per_epoch[0][e]) for e in full}) == len(full)          # reshuffled per epoch
    # a resumed run continues the stream; without shuffle the order is the file's; one process sees everything
    assert train_batches(n, 2, 0, 2, 23, 3) == train_batches(n, 2, 0, 2, 23, 0)[3:]
    assert train_batches(5, 1, 0, 2, 3, shuffle=False) == [[(0, 0), (0, 1)], [(0, 2), (0, 3)], [(0, 4), (1, 0)]]
    single = get_train_loader(cfg, 2, is_dist=False, is_shuffle=False, dataset=StubSet(n), device="cuda:0")
    assert [k for k in single.idx[:n]] == [(0, i) for i in range(n)] and len(single) == 23
    assert loaders[0].idx == get_train_loader(cfg, 2, start_iter=3, dataset=StubSet(n), rank=0, device="cuda:0").idx


def test_train_set_reads_the_reference_split_and_plans_by_key(tmp_path):
    from exps.stage3_root2.config import cfg as base
    from smap_amd.loaders import TrainSet
    import json
    cfg = copy.deepcopy(base)
    person = np.zeros((1, 15, 11))
    person[:, :, :2], person[:, :, 2], person[:, :, 3], person[:, :, 7:] = 200.0, 400.0, 2, (1400.0, 1400.0, 320.0, 240.0)
    rec = lambda ds, name, val: {"dataset": ds, "img_paths": name, "img_width": 640, "img_height": 480, "isValidation": val, "bodys": person.tolist()}
    coco, muco = tmp_path / "coco.json", tmp_path / "muco.json"
    coco.write_text(json.dumps({"root": [rec("COCO", "c0.jpg", 0), rec("COCO", "c1.jpg", 1), rec("COCO", "c2.jpg", 0)]}))
    muco.write_text(json.dumps({"root": [rec("MUCO", "m0.jpg", 0), rec("MUCO", "m1.jpg", 0)]}))
    cfg.dataset.COCO_JSON_PATH, cfg.dataset.MUCO_JSON_PATH, cfg.dataset.USED_3D_DATASETS = str(coco), str(muco), ["MUCO"]
    ts = TrainSet(cfg, seed=4)
    assert [ts.name(i) for i in range(len(ts))] == ["m0.jpg", "m1.jpg", "c0.jpg", "c2.jpg"]      # 3D sets in front, isValidation == 0
    assert ts.path(2) == os.path.join(cfg.dataset.COCO_ROOT_PATH, "c0.jpg") and ts.path(0) == os.path.join(cfg.dataset.MUCO_ROOT_PATH, "m0.jpg")
    assert ts.geometry((3, 2)) == ts.geometry((3, 2)) and ts.geometry((3, 2)) != ts.geometry((4, 2)) and ts.geometry(2) == ts.geometry((0, 2))
    bodys, valid, meta = ts.extras((1, 2))
    assert bodys.shape == (1, 15, 11) and valid.shape == (57, 1) and valid[1, 0] == 0 and meta["dataset"] == "COCO"
    assert ts.extras((1, 0))[1].all()
    want = A.plan_sample(ts.data[2], A.draw(random.Random("4:1:2")), ts.params, True)
    assert np.array_equal(bodys, want[0]) and ts.geometry((1, 2)) == want[2]
    from dataset.base_dataset import JointDataset
    with pytest.raises(NotImplementedError, match="TrainSet"):
        JointDataset(cfg, "train")


def test_cubic_table_under_sanitizers(tmp_path):
    """tests/c/cubic_table_main.cpp + csrc/cubic_table.cpp built for the CPU with -fsanitize=address,undefined: no report, every entry
    sums to 32768, and the bytes are the restatement's."""
    csrc = os.path.join(ROOT, "smap_amd", "csrc")
    exe = tmp_path / "cubic_table"
    r = subprocess.run(["g++", "-g", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "cubic_table_main.cpp"),
                        os.path.join(csrc, "cubic_table.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    digest = 1469598103934665603
    for v in A.cubic_table().reshape(-1).astype(np.uint16).tolist():
        digest = ((digest ^ v) * 1099511628211) & (2 ** 64 - 1)
    assert p.stdout.splitlines() == ["entries with a wrong sum: 0", "digest %d" % digest]
