"""The reference's augmentation entry points (dataset/ImageAugmentation.py:54-176) over numpy frames, with the image work on the GPU.

Same signatures, same module-level `random` draws in the same order, same in-place updates of `meta` ('bodys', 'scale', 'center').
The key-point arithmetic is host float64, as in smap_amd/augment.py::plan_sample; every image operation is one smap_augment_batch launch
of a single frame (smap_amd/augment.py, csrc/augment.hip) whose 8-bit result is read back -- as dataset/representation.py does for the
label maps.  The training loader does not go through these functions: it plans a whole sample on the host and runs ONE fused launch per
batch (smap_amd/loaders.py::TrainLoader); these exist for code written against the reference's API.  aug_scale (unused by the
reference's datasets) is not provided."""
import random

import numpy as np

from smap_amd import augment as _A


def _device_u8(img, fields, out_h, out_w):
    """One frame through smap_augment_batch with mean 0 / std 1, read back as uint8 [out_h, out_w, 3]."""
    import torch
    out = _A.augment_batch([np.ascontiguousarray(img)], [fields], (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), torch.device("cuda", torch.cuda.current_device()),
                           net_w=out_w, net_h=out_h)
    return np.ascontiguousarray(torch.round(out[0] * 255.0).to(torch.uint8).permute(1, 2, 0).cpu().numpy())


def _identity(h, w, **kw):
    return dict(dict(rotate=0, rh=h, rw=w, m=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0), nh=h, nw=w, top=0, left=0, fx=1.0, fy=1.0, flip=0), **kw)


def rotate_skel2d(p2d, R):
    return _A.rotate_skel2d(np.asarray(p2d), R)


def rotate_bound(image, angle, bordervalue):
    """(rotated image, M): the frame turned clockwise by `angle` degrees inside its enlarged bounding box (bicubic, constant border)."""
    if tuple(int(v) for v in bordervalue) != (_A.BORDER,) * 3:
        raise NotImplementedError("rotate_bound: the device warp pads with %d only" % _A.BORDER)
    h, w = image.shape[:2]
    M, nW, nH = _A.rotate_bound_matrix(h, w, float(angle))
    return _device_u8(image, _identity(nH, nW, rotate=1, m=tuple(float(v) for v in M.reshape(-1))), nH, nW), M


def aug_rotate(meta, img, params_transform):
    dice = random.random()
    degree = (dice - 0.5) * 2 * params_transform['max_rotate_degree']
    img_rot, R = rotate_bound(img, degree, (128, 128, 128))
    for i in range(len(meta['bodys'])):
        meta['bodys'][i][:, :2] = rotate_skel2d(meta['bodys'][i][:, :2], R)
    return meta, img_rot


def aug_croppad(meta, img, params_transform, with_augmentation=True):
    dice_x, dice_y, scale_random = random.random(), random.random(), random.random()
    crop_x, crop_y = int(params_transform['crop_size_x']), int(params_transform['crop_size_y'])
    h, w = img.shape[:2]
    scale = min(params_transform['crop_size_x'] / float(w), params_transform['crop_size_y'] / float(h))
    if with_augmentation:
        scale *= (params_transform['scale_max'] - params_transform['scale_min']) * scale_random + params_transform['scale_min']
    meta['scale'] = scale
    meta['bodys'][:, :, :2] *= scale
    shift = np.array([int((dice_x - 0.5) * 2 * params_transform['center_perterb_max']),
                      int((dice_y - 0.5) * 2 * params_transform['center_perterb_max'])])
    center = (meta['center'] * scale + shift).astype(int)
    nw, nh = int(round(w * scale)), int(round(h * scale))
    y0, x0 = int(center[1] + crop_y / 2), int(center[0] + crop_x / 2)
    if y0 < 0 or x0 < 0 or int(center[1] + crop_y / 2 + crop_y) > nh + 2 * crop_y or int(center[0] + crop_x / 2 + crop_x) > nw + 2 * crop_x:
        raise ValueError("aug_croppad: the crop leaves the padded image, no %d x %d sample exists" % (crop_y, crop_x))
    img = _device_u8(img, _identity(h, w, nh=nh, nw=nw, top=crop_y - y0, left=crop_x - x0, fx=scale, fy=scale), crop_y, crop_x)
    offset = np.array([crop_x / 2 - center[0], crop_y / 2 - center[1]]).astype(int)
    meta['center'] += offset
    for i in range(len(meta['bodys'])):
        b = meta['bodys'][i]
        b[:, :2] += offset
        b[(b[:, 0] >= crop_x) | (b[:, 0] < 0) | (b[:, 1] >= crop_y) | (b[:, 1] < 0), 3] = 0
    return meta, img


def aug_flip(meta, img, params_transform):
    """img may be None: the key points alone are mirrored, in a frame crop_size_x wide."""
    dice = random.random()
    if dice <= params_transform['flip_prob']:
        if img is None:
            w = int(params_transform['crop_size_x'])
        else:
            h, w = img.shape[:2]
            img = _device_u8(img, _identity(h, w, flip=1), h, w)
        for i in range(len(meta['bodys'])):
            meta['bodys'][i][:, 0] = w - 1 - meta['bodys'][i][:, 0]
            meta['bodys'][i][:, :] = meta['bodys'][i][params_transform['flip_order'], :]
    return meta, img
