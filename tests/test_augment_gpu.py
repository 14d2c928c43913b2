"""GPU suite of the training-sample path: smap_augment_batch (csrc/augment.hip) against the staged restatement (bicubic warp rounded to
uint8, linear resize, pad / crop, flip, ToTensor + Normalize with torch's own ops), bit for bit on the fp32 output; and TrainLoader.
Shapes are small: canvases of 64 x 96 (four pixels and one 16-byte store per thread) and 37 x 50 (the scalar path)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from smap_amd import augment as A
from smap_amd import lib as L
from test_augment_cpu import GOLD, MEANS, NAMES, STDS, scene, smooth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def staged(frames, canvas):
    return torch.stack([A.staged_sample(img, f, canvas[0], canvas[1], MEANS, STDS) for img, f in frames])


def device(frames, canvas):
    out = A.augment_batch([img for img, _ in frames], [f for _, f in frames], MEANS, STDS, DEV, net_w=canvas[1], net_h=canvas[0])
    assert out.dtype == torch.float32 and out.device == DEV and tuple(out.shape) == (len(frames), 3, canvas[0], canvas[1])
    return out.cpu()


def hand(h, w, degree, scale, top, left, flip=0, M=None, size=None):
    """Fields of a rotating frame built by hand: rotate_bound's matrix for `degree` (or M with size = (nW, nH)), resized by `scale`."""
    if M is None:
        M, nW, nH = A.rotate_bound_matrix(h, w, degree)
    else:
        nW, nH = size
    return dict(rotate=1, rh=nH, rw=nW, m=tuple(float(v) for v in np.asarray(M).reshape(-1)), nh=int(round(nH * scale)), nw=int(round(nW * scale)),
                top=top, left=left, fx=scale, fy=scale, flip=flip)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_scene_equals_the_staged_restatement(name):
    entry, img, draws, params, with_aug, canvas = scene(name)
    _, _, fields = A.plan_sample(entry, draws, params, with_aug)
    got = device([(img, fields)], canvas)
    assert same(got, staged([(img, fields)], canvas))
    # ... and through the recorded canvas: the reference's own pad / crop / flip around the restated pixels
    t = torch.from_numpy(GOLD[name + "_canvas"]).permute(2, 0, 1).float().div(255.0)
    want = (t - torch.tensor(MEANS).view(3, 1, 1)) / torch.tensor(STDS).view(3, 1, 1)
    assert same(got[0], want)


@pytest.mark.parametrize("canvas", [(64, 96), (37, 50)])
def test_without_rotation_and_flip_it_is_preprocess_batch(canvas):
    from smap_amd.preprocess import preprocess_batch
    params = A.AugParams(canvas[1], canvas[0], 40, 10, 0.5, 0.8, 1.1, tuple(range(15)))
    frames, geoms = [], []
    for k, (h, w) in enumerate(((89, 120), (120, 90), (33, 201), (128, 192))):     # (the last one: the exact 2x shrink on the large canvas)
        entry = {"dataset": "MUCO", "img_width": w, "img_height": h, "bodys": []}
        _, meta, f = A.plan_sample(entry, (0.5,) * 5, params, False)
        assert f["rotate"] == 0 and f["flip"] == 0
        frames.append((smooth(h, w, seed=k), f))
        geoms.append((meta, (f["nh"], f["nw"], f["top"], f["left"]), f["fx"], f["fy"]))
    # a window that overhangs the canvas on every side
    f = dict(rotate=0, rh=70, rw=110, m=IDENT, nh=91, nw=143, top=-20, left=-30, fx=1.3, fy=1.3, flip=0)
    frames.append((smooth(70, 110, seed=9), f))
    geoms.append((geoms[0][0], (91, 143, -20, -30), 1.3, 1.3))
    got = device(frames, canvas)
    want, _ = preprocess_batch([img for img, _ in frames], MEANS, STDS, DEV, net_w=canvas[1], net_h=canvas[0], geometries=geoms)
    assert same(got, want.cpu())
    assert same(got, staged(frames, canvas))


def test_footprints_on_the_border():
    """A 4 x 4 and a 1 x 1 source at +-10 degrees: every 4 x 4 footprint touches the border (or lies wholly outside); and a quarter turn
    built by hand on a 45 x 61 source, where the warp is an exact permutation of the pixels."""
    canvas = (37, 50)
    frames = []
    for (h, w), degree, scale in (((4, 4), 10.0, 6.0), ((4, 4), -10.0, 6.0), ((1, 1), 10.0, 9.0), ((1, 1), -10.0, 9.0), ((5, 3), 10.0, 4.0)):
        img = np.random.default_rng(h * 10 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
        frames.append((img, hand(h, w, degree, scale, 3, 7)))
    assert same(device(frames, canvas), staged(frames, canvas))
    img = smooth(45, 61, seed=2)
    M = np.array([[0.0, -1.0, 44.0], [1.0, 0.0, 0.0]])                        # x' = 44 - y, y' = x: a quarter turn clockwise
    assert np.array_equal(A.warp_affine_cubic_u8(img, M, (45, 61)), np.rot90(img, -1))
    for canvas, top, left in (((64, 48), 1, 2), ((67, 49), 3, 1)):
        f = hand(45, 61, None, 1.0, top, left, M=M, size=(45, 61))
        got = device([(img, f)], canvas)
        assert same(got, staged([(img, f)], canvas))
        turned = torch.from_numpy(np.ascontiguousarray(np.rot90(img, -1))).permute(2, 0, 1).float().div(255.0)
        want = (turned - torch.tensor(MEANS).view(3, 1, 1)) / torch.tensor(STDS).view(3, 1, 1)
        assert same(got[0][:, top:top + 61, left:left + 45], want)


@pytest.mark.parametrize("canvas", [(64, 96), (37, 50)])
def test_exact_two_times_shrink_over_a_rotated_source(canvas):
    """fx = fy = 0.5: cv2.resize turns INTER_LINEAR into the 2 x 2 box mean; here over the rotated image, whose four pixels are warped."""
    frames = []
    for k, ((h, w), degree, flip) in enumerate((((90, 120), 7.0, 0), ((91, 121), -10.0, 1), ((60, 70), 3.0, 0))):
        f = hand(h, w, degree, 0.5, 2 - k, 5 * k - 3, flip=flip)
        assert 1.0 / f["fx"] == 2.0
        frames.append((smooth(h, w, seed=20 + k), f))
    assert same(device(frames, canvas), staged(frames, canvas))


def test_seventeen_frames_take_two_launches_and_equal_their_single_results():
    canvas = (37, 52)
    rng = np.random.default_rng(17)
    frames = []
    for k in range(17):
        h, w = int(rng.integers(20, 70)), int(rng.integers(20, 90))
        if k % 5 == 4:
            f = dict(rotate=0, rh=h, rw=w, m=IDENT, nh=int(round(h * 0.7)), nw=int(round(w * 0.7)), top=k - 8, left=2 * k - 10, fx=0.7, fy=0.7, flip=k % 2)
        else:
            f = hand(h, w, float(rng.uniform(-10, 10)), float(rng.uniform(0.5, 1.4)), int(rng.integers(-10, 10)), int(rng.integers(-15, 15)), flip=k % 2)
        frames.append((smooth(h, w, seed=40 + k), f))
    assert len(frames) > L.PREP_MAX_FRAMES
    got = device(frames, canvas)
    for k, fr in enumerate(frames):
        assert same(got[k:k + 1], device([fr], canvas)), k
    assert same(got[[0, 4, 16]], staged([frames[0], frames[4], frames[16]], canvas))


def _launch(srcs, fields, out, canvas):
    """smap_augment_batch on frames that already lie on the device (views into larger allocations), into `out`."""
    table = (L.AugFrame * len(srcs))(*[A.aug_frame(s.data_ptr(), s.shape[0], s.shape[1], f) for s, f in zip(srcs, fields)])
    tab = A.device_cubic_table(DEV)
    with torch.cuda.device(DEV):
        st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        L.check(L.load().smap_augment_batch(table, len(srcs), C.c_void_p(out.data_ptr()), canvas[0], canvas[1], (C.c_float * 3)(*MEANS),
                                            (C.c_float * 3)(*STDS), C.c_void_p(tab.data_ptr()), st), "smap_augment_batch")
    torch.cuda.synchronize(DEV)


@pytest.mark.parametrize("canvas", [(64, 96), (37, 50)])
def test_a_launch_touches_only_its_operands(canvas):
    """Every source lies inside a larger allocation whose guard bytes are 0x00, then 0xFF; dst lies inside a larger allocation filled
    with a NaN pattern.  The outputs are byte-identical under both fills, hold no NaN, equal the restatement, and the NaN guard around
    dst is untouched.  All extents stay inside the allocations: nothing here can fault."""
    GUARD = 4096
    specs = [((4, 4), hand(4, 4, 10.0, 6.0, 3, 7)), ((45, 61), hand(45, 61, -10.0, 0.9, -5, -9, flip=1)),
             ((50, 66), dict(rotate=0, rh=50, rw=66, m=IDENT, nh=75, nw=99, top=-4, left=-2, fx=1.5, fy=1.5, flip=0)),
             ((40, 50), hand(40, 50, 5.0, 0.5, 1, 1))]
    imgs = [smooth(h, w, seed=60 + k) for k, ((h, w), _) in enumerate(specs)]
    fields = [f for _, f in specs]
    n_out = len(specs) * 3 * canvas[0] * canvas[1]
    outs = []
    for fill in (0x00, 0xFF):
        srcs = []
        for img in imgs:
            buf = torch.full((GUARD + img.size + GUARD,), fill, dtype=torch.uint8, device=DEV)
            buf[GUARD:GUARD + img.size] = torch.from_numpy(img.reshape(-1)).to(DEV)
            srcs.append(buf[GUARD:GUARD + img.size].view(img.shape))
        big = torch.full((1024 + n_out + 1024,), float("nan"), dtype=torch.float32, device=DEV)
        big.view(torch.int32).fill_(0x7FC0BEEF)
        out = big[1024:1024 + n_out].view(len(specs), 3, canvas[0], canvas[1])
        assert out.data_ptr() % 16 == 0
        _launch(srcs, fields, out, canvas)
        assert not torch.isnan(out).any()
        guard = torch.cat([big[:1024], big[1024 + n_out:]]).view(torch.int32)
        assert bool((guard == 0x7FC0BEEF).all())
        outs.append(out.cpu())
    assert same(outs[0], outs[1])
    assert same(outs[0], staged(list(zip(imgs, fields)), canvas))
    # negative control, on the restatement: a frame read with a width one too large walks into the guard bytes behind it, and the
    # two fills then DO give different outputs -- the comparison above would notice a read outside the operands
    h, w = specs[2][0]
    wrong = []
    for fill in (0x00, 0xFF):
        host = np.full(GUARD + imgs[2].size + GUARD, fill, np.uint8)
        host[GUARD:GUARD + imgs[2].size] = imgs[2].reshape(-1)
        view = host[GUARD:GUARD + h * (w + 1) * 3].reshape(h, w + 1, 3)        # the last h * 3 bytes are guard bytes
        bottom = dict(fields[2], top=canvas[0] - fields[2]["nh"], left=canvas[1] - fields[2]["nw"])     # the window's last rows on the canvas
        wrong.append(A.staged_sample(view, bottom, canvas[0], canvas[1], MEANS, STDS))
    assert not same(wrong[0], wrong[1])


def _records(folder, sizes):
    rng = np.random.default_rng(23)
    recs = []
    for k, (h, w) in enumerate(sizes):
        np.save(os.path.join(folder, "f%d.npy" % k), smooth(h, w, seed=80 + k))
        bodys = np.zeros((2, 15, 11))
        bodys[:, :, 0], bodys[:, :, 1] = rng.uniform(0.2 * w, 0.8 * w, (2, 15)), rng.uniform(0.2 * h, 0.8 * h, (2, 15))
        bodys[:, :, 2], bodys[:, :, 3] = rng.uniform(300, 600, (2, 1)), rng.choice([0, 1, 2], (2, 15), p=[0.1, 0.3, 0.6])
        bodys[:, :, 6], bodys[:, :, 7:] = bodys[:, :, 2], (1400.0, 1400.0, w / 2, h / 2)
        recs.append({"dataset": "COCO" if k % 2 else "MUCO", "img_paths": "f%d.npy" % k, "img_width": w, "img_height": h, "isValidation": 0,
                     "bodys": bodys.tolist()})
    return recs


def test_train_loader_batches(tmp_path, monkeypatch):
    """get_train_loader on a folder of 5 .npy frames, IMG_PER_GPU = 2: the reference's BatchCollator shapes on the device, every part
    equal to its own function on the planned sample, the same bytes with 1 and with 4 decode threads, and SMAPLoss takes the batch."""
    from exps.stage3_root2.config import cfg as base
    from lib.utils.dataloader import get_train_loader
    from smap_amd.labels import label_spec, render_labels, root_depth_labels, valid_vector
    from smap_amd.loaders import TrainLoader, TrainSet
    from smap_amd.loss import SMAPLoss
    cfg = copy.deepcopy(base)
    cfg.SOLVER.MAX_ITER = 4
    cfg.dataset.COCO_ROOT_PATH = cfg.dataset.MUCO_ROOT_PATH = str(tmp_path)
    ts = TrainSet(cfg, seed=1, data=_records(str(tmp_path), ((240, 320), (241, 319), (200, 420), (480, 640), (130, 150))))
    spec = label_spec(cfg)
    runs = []
    for threads in ("1", "4"):
        monkeypatch.setenv("SMAP_DECODE_THREADS", threads)
        loader = get_train_loader(cfg, 1, is_dist=False, dataset=ts, device=DEV)
        assert isinstance(loader, TrainLoader) and len(loader) == 4 and loader.threads == int(threads)
        batches = list(loader)
        assert all(t.dtype == torch.float32 and t.device == DEV for batch in batches for t in batch)
        runs.append([tuple(t.cpu() for t in batch) for batch in batches])
        keys = loader.idx
    assert len(runs[0]) == len(runs[1]) == 4
    for a, b in zip(*runs):
        assert all(same(x, y) for x, y in zip(a, b))
    assert len({k for k in keys}) == 8 and {k[0] for k in keys} == {0, 1}         # 8 samples of a 5-frame set: into the second epoch
    for n, (imgs, valids, labels, rdepth) in enumerate(runs[0]):
        assert tuple(imgs.shape) == (2, 3, 512, 832) and tuple(valids.shape) == (2, 57, 1)
        assert tuple(labels.shape) == (2, 5, 57, 128, 208) and tuple(rdepth.shape) == (2, cfg.DATASET.MAX_PEOPLE, 3)
        for j, key in enumerate(keys[2 * n:2 * n + 2]):
            bodys, meta, fields = ts.plan(key)
            frame = np.load(ts.path(key))
            assert same(imgs[j:j + 1], A.augment_batch([frame], [fields], cfg.INPUT.MEANS, cfg.INPUT.STDS, DEV))
            assert same(labels[j:j + 1], render_labels([bodys], spec, False, DEV))
            assert same(valids[j], torch.from_numpy(valid_vector(meta["dataset"]).astype(np.float32)))
            assert same(rdepth[j], torch.from_numpy(root_depth_labels(bodys, meta["scale"], spec)))
    imgs, valids, labels, rdepth = (t.to(DEV) for t in runs[0][0])
    g = torch.Generator(device="cpu").manual_seed(3)
    heads = {k: [[(torch.rand((2, c, 128, 208), generator=g) * 0.1).to(DEV).requires_grad_(True) for _ in range(4)] for _ in range(3)]
             for k, c in (("heatmap_2d", 43), ("det_d", 14), ("root_d", 1))}
    losses = SMAPLoss.from_cfg(cfg, strict=True)(heads, valids, labels, rdepth)
    assert all(bool(torch.isfinite(v)) for v in losses.values()) and float(losses["total_loss"].detach()) > 0
    losses["total_loss"].backward()
    assert heads["heatmap_2d"][2][3].grad is not None


def test_reference_api_rotates_crops_and_flips_on_the_device(monkeypatch):
    """dataset/ImageAugmentation.py over a numpy frame: the three calls in the reference's order give the fixture's canvas and key points."""
    from dataset import ImageAugmentation as IA
    name = "flip_on"
    entry, img, draws, params, with_aug, (crop_y, crop_x) = scene(name)
    replay = list(draws)
    monkeypatch.setattr(IA.random, "random", lambda: replay.pop(0))
    meta = {"dataset": "MUCO", "bodys": np.asarray(entry["bodys"], np.float64), "center": np.array([img.shape[1] // 2, img.shape[0] // 2])}
    p = params.as_dict()
    meta, out = IA.aug_rotate(meta, img, p)
    meta, out = IA.aug_croppad(meta, out, p, False)
    meta, out = IA.aug_flip(meta, out, p)
    assert not replay and out.dtype == np.uint8 and np.array_equal(out, GOLD[name + "_canvas"])
    assert np.abs(meta["bodys"][:, :, :2] - GOLD[name + "_bodys"][:, :, :2]).max() < 1e-9
    assert meta["scale"] == float(GOLD[name + "_scale"]) and np.array_equal(meta["center"], GOLD[name + "_center"])
