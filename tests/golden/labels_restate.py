"""numpy restatements of the label renderer's arithmetic (smap_amd/csrc/labels.hip), shared by the fixture generator
(gen_golden_labels.py), the tests and tools/bench_labels.py.  Nothing here imports the product.

  * `gaussian_blur` / `heatmaps`: cv2.GaussianBlur(map, ksize, 0) on an fp32 map as DESIGN.md "Label maps" states it -- fixed taps up
    to size 7, computed taps beyond, a row pass then a column pass, each an fp32 sum over the taps in ascending order starting from
    0.0f, BORDER_REFLECT_101.  OpenCV is not installed where this project is built: stated, not executed.
  * `pafs`: generate_paf / putVecMaps3D (dataset/representation.py:36-113) in per-pixel form -- what one device thread does.  The
    generator asserts it equal, bit for bit, to the reference's own function on every scene, line width and flag before it writes.
"""
import numpy as np

LIMBS = [(0, 1), (0, 2), (0, 9), (9, 10), (10, 11), (0, 3), (3, 4), (4, 5), (2, 12), (12, 13), (13, 14), (2, 6), (6, 7), (7, 8)]
KERNELS = [(15, 15), (11, 11), (9, 9), (7, 7), (5, 5)]
NJ = 15


def taps(n):
    if n == 5:
        return (np.asarray([1, 4, 6, 4, 1], np.float64) / 16).astype(np.float32)
    if n == 7:
        return np.asarray([0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125], np.float32)
    if n == 3:
        return np.asarray([0.25, 0.5, 0.25], np.float32)
    if n == 1:
        return np.asarray([1.0], np.float32)
    sigma = 0.3 * ((n - 1) * 0.5 - 1) + 0.8
    c = [np.float32(np.exp(-0.5 / (sigma * sigma) * (i - (n - 1) * 0.5) * (i - (n - 1) * 0.5))) for i in range(n)]
    total = 0.0
    for v in c:
        total += float(v)
    return np.asarray([np.float32(float(v) / total) for v in c], np.float32)


def _reflect101(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _pass(src, k, axis):
    n, r = len(k), len(k) // 2
    size = src.shape[axis]
    assert r <= size - 1
    acc = np.zeros_like(src, dtype=np.float32)
    for i in range(n):                                           # taps in ascending order, fp32 throughout
        idx = _reflect101(np.arange(size) + i - r, size)
        acc = acc + np.float32(k[i]) * np.take(src, idx, axis=axis)
    return acc


def gaussian_blur(src, ksize, sigma=0):
    """ksize = (width, height), as cv2 takes it."""
    assert sigma == 0 and src.dtype == np.float32 and src.ndim == 2
    return _pass(_pass(src, taps(int(ksize[0])), 1), taps(int(ksize[1])), 0)


def heatmaps(bodys, shape, stride, kernel):
    """generate_heatmap (:5-21) on top of gaussian_blur."""
    out = np.zeros((NJ,) + tuple(shape), np.float32)
    for i in range(NJ):
        for j in range(len(bodys)):
            if bodys[j][i][3] < 1:
                continue
            out[i, int(bodys[j][i][1] / stride), int(bodys[j][i][0] / stride)] = 1
        out[i] = gaussian_blur(out[i], kernel, 0)
        maxi = np.amax(out[i])
        if maxi <= 1e-8:
            continue
        out[i] /= maxi / 255
    return out


def pafs(bodys, shape, stride, thre, with_mds, limbs=LIMBS):
    """[42, H, W] fp32: every pixel walks the persons in order; acc *= cnt, acc += vec, cnt += (vec_x != 0 or vec_y != 0),
    acc /= max(cnt, 1) in fp32, the mask in float64."""
    H, W = shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.zeros((len(limbs) * 3, H, W), np.float32)
    for l, (a, b) in enumerate(limbs):
        acc = np.zeros((3, H, W), np.float32)
        cnt = np.zeros((H, W), np.float32)
        for body in bodys:
            need = 2 if (thre > 1 and with_mds) else 1
            if body[a][3] < need or body[b][3] < need:
                continue
            ca = np.array(body[a][:3], dtype=int).astype(float)
            cb = np.array(body[b][:3], dtype=int).astype(float)
            limb_z = cb[2] - ca[2]
            ca, cb = ca[:2] / stride, cb[:2] / stride
            vec = cb - ca
            norm = np.linalg.norm(vec)
            if norm < 1.0:
                continue
            u = vec / norm
            x0 = max(int(round(min(ca[0], cb[0]) - thre)), 0)
            x1 = int(min(int(round(max(ca[0], cb[0]) + thre)), float(W)))
            y0 = max(int(round(min(ca[1], cb[1]) - thre)), 0)
            y1 = int(min(int(round(max(ca[1], cb[1]) + thre)), float(H)))
            inside = (xx >= x0) & (xx < x1) & (yy >= y0) & (yy < y1)
            width = np.abs((xx - ca[0]) * u[1] - (yy - ca[1]) * u[0])
            m = (inside & (width < thre)).astype(np.float64)
            v = np.stack([(m * u[0]).astype(np.float32), (m * u[1]).astype(np.float32), (m * limb_z).astype(np.float32)])
            acc = acc * cnt
            acc = acc + v
            cnt = cnt + ((v[0] != 0) | (v[1] != 0)).astype(np.float32)
            acc = acc / np.where(cnt == 0, np.float32(1), cnt)
        out[3 * l:3 * l + 3] = acc
    out[0::3] *= 127
    out[1::3] *= 127
    return out


def labels(bodys, shape, stride, line_width=1, with_mds=False, kernels=KERNELS):
    """[S, 57, H, W] fp32: a sample's labels (base_dataset.py:177-185)."""
    out = np.zeros((len(kernels), NJ + 42) + tuple(shape), np.float32)
    for i, k in enumerate(kernels):
        out[i, :NJ] = heatmaps(bodys, shape, stride, k)
        out[i, NJ:] = pafs(bodys, shape, stride, max(1, 3 - i) * line_width, with_mds)
    return out
