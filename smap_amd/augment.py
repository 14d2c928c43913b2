"""Training samples on the GPU (reference: dataset/ImageAugmentation.py aug_rotate / aug_croppad / aug_flip + ToTensor + Normalize,
as dataset/base_dataset.py stage `train` chains them).

The split: the HOST does the annotation arithmetic of one sample (`plan_sample`: float64, operation by operation as the reference does
it -- the rotation matrix and its fix-up, the key points, the crop geometry, the visibilities, the flip) and hands the image work out as
one descriptor; the GPU does all of the image work of a batch in ONE launch (`augment_batch` -> smap_augment_batch, csrc/augment.hip):
bicubic rotate, linear resize, crop / pad, flip and normalise straight from the uploaded uint8 frames; the rotated image is never written.

What is pinned how: the control flow, the annotation arithmetic and the crop geometry are pinned by EXECUTING the
reference's functions (tests/golden/gen_golden_augment.py); the pixel arithmetic of cv2.warpAffine and cv2.resize is RESTATED from
OpenCV's published algorithm (`warp_affine_cubic_u8`, `cubic_table` here, `resize_linear_u8` in smap_amd/preprocess.py) -- cv2 is not
installed, parity with it is not pinned by execution."""
import ctypes as C
import math
import threading
import warnings
from typing import NamedTuple, Tuple

import numpy as np
import torch

from . import lib as _L
from .preprocess import resize_linear_u8

BORDER = 128


class AugParams(NamedTuple):
    """base_dataset.py:78-87 params_transform, the entries the augmentation reads."""
    crop_x: int
    crop_y: int
    center_perterb_max: float
    max_rotate_degree: float
    flip_prob: float
    scale_min: float
    scale_max: float
    flip_order: Tuple[int, ...]

    @classmethod
    def from_cfg(cls, cfg):
        ds = cfg.dataset
        t = ds.TRAIN
        return cls(int(ds.INPUT_SHAPE[1]), int(ds.INPUT_SHAPE[0]), t.CENTER_TRANS_MAX, t.ROTATE_MAX, t.FLIP_PROB, t.SCALE_MIN, t.SCALE_MAX,
                   tuple(int(k) for k in ds.KEYPOINT.FLIP_ORDER))

    def as_dict(self):
        """The reference's params_transform dict."""
        return {"crop_size_x": self.crop_x, "crop_size_y": self.crop_y, "center_perterb_max": self.center_perterb_max,
                "max_rotate_degree": self.max_rotate_degree, "flip_prob": self.flip_prob, "flip_order": list(self.flip_order),
                "scale_max": self.scale_max, "scale_min": self.scale_min}


def draw(rng):
    """The five random.random() values one sample consumes, in the reference's order: aug_rotate's dice; aug_croppad's dice_x, dice_y,
    scale_random (always drawn, whether used or not); aug_flip's dice.  rng: a random.Random."""
    return tuple(rng.random() for _ in range(5))


def get_rotation_matrix_2d(center, angle, scale):
    """cv2.getRotationMatrix2D: [2, 3] float64."""
    a = angle * math.pi / 180.0
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = float(center[0]), float(center[1])
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], np.float64)


def rotate_bound_matrix(h, w, angle):
    """rotate_bound (ImageAugmentation.py:143-170) without its warpAffine: (M [2,3], nW, nH)."""
    cX, cY = w // 2, h // 2
    M = get_rotation_matrix_2d((cX, cY), -angle, 1.0)
    cos, sin = np.abs(M[0, 0]), np.abs(M[0, 1])
    nW, nH = int((h * sin) + (w * cos)), int((h * cos) + (w * sin))
    M[0, 2] += (nW / 2) - cX
    M[1, 2] += (nH / 2) - cY
    return M, nW, nH


def rotate_skel2d(p2d, R):
    """ImageAugmentation.py:173-176."""
    aug_p2d = np.concatenate((p2d, np.ones((p2d.shape[0], 1))), axis=1)
    return (R @ aug_p2d.T).T[:, :2]


def _clear_outside(bodys, crop_x, crop_y):
    out = (bodys[:, :, 0] >= crop_x) | (bodys[:, :, 0] < 0) | (bodys[:, :, 1] >= crop_y) | (bodys[:, :, 1] < 0)
    bodys[:, :, 3][out] = 0


def plan_sample(entry, draws, params, with_augmentation=True):
    """One training sample of base_dataset.py stage `train` without its pixels: -> (bodys [P,15,C] float64 in network pixels, meta,
    fields).  entry: one annotation record (dataset, img_width, img_height, bodys); draws: draw(rng).
    meta: scale (aug_croppad's resize factor), center (the reference's meta['center'] after aug_croppad: the UN-ROTATED frame's centre
    plus the window offset -- aug_rotate does not update it), dataset, img_width, img_height, net_width, net_height.
    fields: what smap_aug_frame takes beside the frame: rotate, rh, rw, m (forward matrix, 6 floats), nh, nw, top, left, fx, fy, flip.
    The image window (top, left) is where the reference's slice of the padded image puts the resized image; the key-point offset is
    int(crop / 2 - centre).  The two agree for even crop sizes and differ by one pixel for odd ones, as in the reference.
    ValueError: the reference's slice would start below 0 or end beyond the padded image (numpy wraps or truncates there: no
    fixed-size sample exists)."""
    d_rot, dice_x, dice_y, scale_random, d_flip = draws
    dataset = str(entry["dataset"]).upper()
    w, h = int(entry["img_width"]), int(entry["img_height"])
    bodys = np.array(entry["bodys"], dtype=np.float64)
    if bodys.ndim != 3:
        bodys = np.zeros((0, 15, 11), np.float64)
    center0 = np.array([w // 2, h // 2])
    crop_x, crop_y = int(params.crop_x), int(params.crop_y)
    fields = dict(rotate=0, rh=h, rw=w, m=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0), flip=0)
    nW, nH = w, h
    if with_augmentation:                                                   # aug_rotate
        degree = (d_rot - 0.5) * 2 * params.max_rotate_degree
        M, nW, nH = rotate_bound_matrix(h, w, degree)
        for i in range(len(bodys)):
            bodys[i][:, :2] = rotate_skel2d(bodys[i][:, :2], M)
        fields.update(rotate=1, rh=nH, rw=nW, m=tuple(float(v) for v in M.reshape(-1)))
    # aug_croppad (with_augmentation only for COCO entries: base_dataset.py:141-144)
    scale_multiplier = (params.scale_max - params.scale_min) * scale_random + params.scale_min
    scale = min(crop_x / float(nW), crop_y / float(nH))
    if with_augmentation and dataset == "COCO":
        scale *= scale_multiplier
    bodys[:, :, :2] *= scale
    perterb = params.center_perterb_max if with_augmentation else 0         # (base_dataset.py:139)
    x_offset = int((dice_x - 0.5) * 2 * perterb)
    y_offset = int((dice_y - 0.5) * 2 * perterb)
    center = (center0 * scale + np.array([x_offset, y_offset])).astype(int)
    nw, nh = int(round(nW * scale)), int(round(nH * scale))                 # cv2.resize(fx, fy): dsize = cvRound(src * f)
    y0, y1 = int(center[1] + crop_y / 2), int(center[1] + crop_y / 2 + crop_y)
    x0, x1 = int(center[0] + crop_x / 2), int(center[0] + crop_x / 2 + crop_x)
    if y0 < 0 or x0 < 0 or y1 > nh + 2 * crop_y or x1 > nw + 2 * crop_x or y1 - y0 != crop_y or x1 - x0 != crop_x:
        raise ValueError("the crop slice [%d:%d, %d:%d] leaves the padded image (%d x %d): no %d x %d sample exists" % (
            y0, y1, x0, x1, nh + 2 * crop_y, nw + 2 * crop_x, crop_y, crop_x))
    offset = np.array([crop_x / 2 - center[0], crop_y / 2 - center[1]]).astype(int)
    bodys[:, :, :2] += offset
    _clear_outside(bodys, crop_x, crop_y)
    fields.update(nh=nh, nw=nw, top=crop_y - y0, left=crop_x - x0, fx=float(scale), fy=float(scale))
    if with_augmentation and d_flip <= params.flip_prob:                    # aug_flip
        bodys[:, :, 0] = crop_x - 1 - bodys[:, :, 0]
        bodys = bodys[:, list(params.flip_order), :]
        fields["flip"] = 1
    _clear_outside(bodys, crop_x, crop_y)                                   # remove_illegal_joint
    meta = {"scale": scale, "center": center0 + offset, "dataset": dataset, "img_width": w, "img_height": h,
            "net_width": crop_x, "net_height": crop_y}
    return bodys, meta, fields


# ---- restatements (numpy): for the tests, the fixture generator and the reference-shaped entry points ----
_cubic = None


def cubic_table():
    """[1024, 16] int16: smap_cubic_table restated in numpy float32, operation by operation (OpenCV imgwarp.cpp interpolateCubic,
    initInterTab1D, initInterTab2D with INTER_BITS = 5, INTER_REMAP_COEF_BITS = 15)."""
    global _cubic
    if _cubic is not None:
        return _cubic
    f = np.float32
    A, one = f(-0.75), f(1)
    x = np.arange(32, dtype=f) * f(1.0 / 32)
    c0 = ((A * (x + one) - f(5) * A) * (x + one) + f(8) * A) * (x + one) - f(4) * A
    c1 = ((A + f(2)) * x - (A + f(3))) * x * x + one
    c2 = ((A + f(2)) * (one - x) - (A + f(3))) * (one - x) * (one - x) + one
    c3 = one - c0 - c1 - c2
    t = np.stack([c0, c1, c2, c3], 1).astype(f)                              # [32, 4]
    v = (t[:, None, :, None] * t[None, :, None, :]).astype(f)                # [i (y), j (x), k1, k2] = vy * vx
    tab = np.clip(np.rint(v * f(32768)), -32768, 32767).astype(np.int64).reshape(1024, 4, 4)
    for e in tab:
        diff = int(e.sum()) - 32768
        if diff == 0:
            continue
        # initInterTab2D scans rows / columns ksize / 2 and ksize / 2 + 1 (2 and 3 of the 4 x 4), ties to the first met
        M = m = (2, 2)
        for k1 in (2, 3):
            for k2 in (2, 3):
                if e[k1, k2] < e[m]:
                    m = (k1, k2)
                elif e[k1, k2] > e[M]:
                    M = (k1, k2)
        if diff < 0:
            e[M] -= diff
        else:
            e[m] -= diff
    _cubic = tab.reshape(1024, 16).astype(np.int16)
    _cubic.setflags(write=False)
    return _cubic


def invert_affine(M):
    """cv::warpAffine's inversion of the forward matrix, in float64, operation by operation -> 6 floats."""
    m = [float(v) for v in np.asarray(M, np.float64).reshape(-1)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def warp_affine_cubic_u8(img, M, dsize, border=BORDER):
    """cv2.warpAffine(img, M, dsize, flags=INTER_CUBIC, borderMode=BORDER_CONSTANT, borderValue=(border,) * 3) on an 8-bit image,
    restated from OpenCV's generic path (no IPP, no OpenCL): the inverted matrix in double, the map in 10 + 5 fractional bits
    (X0 = cvRound((M1*y + M2) * 1024) + 16, adelta = cvRound(M0 * x * 1024), X = (X0 + adelta) >> 5), the 4 x 4 fixed-point weights of
    cubic_table() at source column (X >> 5) - 1, saturate_u8((sum + 2^14) >> 15); a tap outside the image contributes `border`.
    dsize = (nW, nH)."""
    img = np.ascontiguousarray(img)
    h, w = img.shape[:2]
    nW, nH = int(dsize[0]), int(dsize[1])
    m = invert_affine(M)
    x = np.arange(nW, dtype=np.float64)
    y = np.arange(nH, dtype=np.float64)
    adelta = np.rint(m[0] * x * 1024.0).astype(np.int64)
    bdelta = np.rint(m[3] * x * 1024.0).astype(np.int64)
    X0 = np.rint((m[1] * y + m[2]) * 1024.0).astype(np.int64) + 16
    Y0 = np.rint((m[4] * y + m[5]) * 1024.0).astype(np.int64) + 16
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    sx = np.clip(X >> 5, -32768, 32767) - 1
    sy = np.clip(Y >> 5, -32768, 32767) - 1
    wt = cubic_table().astype(np.int64)[(Y & 31) * 32 + (X & 31)]           # [nH, nW, 16]
    src = img.astype(np.int64)
    acc = np.zeros((nH, nW, 3), np.int64)
    for i in range(4):
        yy = sy + i
        for j in range(4):
            xx = sx + j
            inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            px = np.where(inside[..., None], src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], border)
            acc += px * wt[..., i * 4 + j, None]
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def staged_canvas(img, fields, net_h, net_w):
    """The staged pipeline of one sample up to the uint8 canvas [net_h, net_w, 3]: warp (when fields['rotate']), resize_linear_u8,
    paste at (top, left) of the 128-grey canvas clipped to it (= the reference's pad and slice), flip."""
    if fields["rotate"]:
        img = warp_affine_cubic_u8(img, np.asarray(fields["m"], np.float64).reshape(2, 3), (fields["rw"], fields["rh"]))
    nh, nw, top, left = fields["nh"], fields["nw"], fields["top"], fields["left"]
    canvas = np.full((net_h, net_w, 3), BORDER, np.uint8)
    if nh > 0 and nw > 0:
        r = resize_linear_u8(img, nh, nw, fx=fields["fx"], fy=fields["fy"])
        x0, y0 = max(left, 0), max(top, 0)
        x1, y1 = min(left + nw, net_w), min(top + nh, net_h)
        if x1 > x0 and y1 > y0:
            canvas[y0:y1, x0:x1] = r[y0 - top:y1 - top, x0 - left:x1 - left]
    if fields["flip"]:
        canvas = np.ascontiguousarray(canvas[:, ::-1])
    return canvas


def staged_sample(img, fields, net_h, net_w, means, stds):
    """staged_canvas, then ToTensor + Normalize with torch's own ops in that order -> [3, net_h, net_w] fp32 (CPU)."""
    t = torch.from_numpy(staged_canvas(img, fields, net_h, net_w)).permute(2, 0, 1).float().div(255.0)
    mean = torch.tensor(means, dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor(stds, dtype=torch.float32).view(3, 1, 1)
    return (t - mean) / std


# ---- the device half ----
_tables, _tables_lock = {}, threading.Lock()


def device_cubic_table(device):
    """smap_cubic_table's output on `device`, uploaded once per device."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    with _tables_lock:
        if key not in _tables:
            host = np.empty(1024 * 16, np.int16)
            _L.check(_L.load().smap_cubic_table(C.c_void_p(host.ctypes.data)), "smap_cubic_table")
            _tables[key] = torch.from_numpy(host).to(device)
        return _tables[key]


def aug_frame(ptr, h, w, fields):
    """struct smap_aug_frame of a frame at device address `ptr` and its plan_sample fields.  An empty resize window (nh or nw == 0)
    becomes a 1 x 1 window off the canvas: a frame of padding, as in preprocess_batch."""
    nh, nw, top, left = int(fields["nh"]), int(fields["nw"]), int(fields["top"]), int(fields["left"])
    if nh <= 0 or nw <= 0:
        nh, nw, top, left = 1, 1, 1 << 30, 1 << 30
    return _L.AugFrame(ptr, int(h), int(w), int(bool(fields["rotate"])), int(fields["rh"]), int(fields["rw"]), nh, nw, top, left,
                       int(bool(fields["flip"])), (C.c_double * 6)(*[float(v) for v in fields["m"]]), float(fields["fx"]), float(fields["fy"]))


def augment_batch(images, plans, means, stds, device, net_w=832, net_h=512):
    """images: list of uint8 HxWx3 BGR arrays / tensors (host or device); plans: the `fields` of plan_sample, one per image.  Returns
    imgs [B,3,net_h,net_w] fp32 on `device`: every frame is uploaded from where it lies and the whole batch is written by
    smap_augment_batch (one launch per 16 frames), on the current stream."""
    lib = _L.load()
    B = len(images)
    if len(plans) != B:
        raise ValueError("one plan per image")
    device = torch.device(device)
    out = torch.empty((B, 3, net_h, net_w), dtype=torch.float32, device=device)
    if not B:
        return out
    mean, std = (C.c_float * 3)(*means), (C.c_float * 3)(*stds)
    keep, table = [], (_L.AugFrame * B)()
    with torch.cuda.device(device):
        st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        tab = device_cubic_table(device) if any(p["rotate"] for p in plans) else None
        for i, (im, plan) in enumerate(zip(images, plans)):
            if isinstance(im, torch.Tensor):
                t = im.contiguous()
            else:
                with warnings.catch_warnings():          # the decoder's frames are read-only views of its bytes: they are only read here
                    warnings.simplefilter("ignore", UserWarning)
                    t = torch.as_tensor(np.ascontiguousarray(im))
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise ValueError("images must be uint8 HxWx3 (BGR)")
            d = t.to(device, non_blocking=True)
            keep.append(d)
            table[i] = aug_frame(d.data_ptr(), t.shape[0], t.shape[1], plan)
        _L.check(lib.smap_augment_batch(table, B, C.c_void_p(out.data_ptr()), net_h, net_w, mean, std,
                                        C.c_void_p(tab.data_ptr() if tab is not None else None), st), "smap_augment_batch")
    return out
