"""Ground-truth label maps on the GPU (reference: dataset/representation.py, dataset/base_dataset.py:167-187).

`render_labels` renders, for a batch of annotated frames, what JointDataset.__getitem__ renders for one training sample: per label
scale 15 Gaussian heat-maps (x 255) and 14 x (x, y, z) part-affinity / relative-depth fields (x 127 on x and y) --
labels [B, S, 57, H, W] fp32.  The split (csrc/labels.hip, DESIGN.md "Label maps"):

  host   everything per (frame, scale, limb, person) in float64 with the reference's own expressions (`pack_table`): validity with
         `with_mds`, the int truncation, / stride, np.linalg.norm on the 2-vector (a BLAS dot: not vectorised here, a rewrite need not
         round alike), the unit vector, limb_z, the int(round()) box; per (frame, joint) the set of impulse cells; the blur taps.
  device every per-pixel operation: two launches per batch (smap_render_labels), no allocation, the caller's stream.

The fields are bit for bit the reference's (tests/golden/labels.npz was written by running it).  The heat-maps follow OpenCV's
GaussianBlur as DESIGN.md states it; OpenCV is not part of this image, so that half is argued, not executed.

`gt_maps` turns labels into the three tensors the backbone returns, at its raw scale -- what a perfectly trained network would emit --
for `test.py --maps_from_gt 1` and PosePipeline(maps_source=...).  `root_depth_labels` and `valid_vector` are the two small host-side
pieces of a training sample (generate_rdepth, the `valid` mask)."""
import ctypes as C
from typing import NamedTuple, Tuple

import numpy as np
import torch

from . import lib as L

NJ, NL, NC = 15, 14, L.LABEL_C
MAX_HW = 32768


class LabelSpec(NamedTuple):
    """What the renderer reads of a configuration (label_spec(cfg))."""
    kernels: Tuple[Tuple[int, int], ...]     # DATASET.TRAIN.GAUSSIAN_KERNELS: (width, height) of every label scale's blur
    paf_vector: Tuple[Tuple[int, int], ...]  # DATASET.PAF.VECTOR
    line_width: float                        # DATASET.PAF.LINE_WIDTH_THRE
    stride: int
    shape: Tuple[int, int]                   # (H, W) of the maps
    root_idx: int
    max_people: int

    @property
    def thres(self):
        """Line width of every label scale (base_dataset.py:185)."""
        return tuple(max(1, 3 - i) * self.line_width for i in range(len(self.kernels)))


def label_spec(cfg, shape=None, kernels=None):
    ds = cfg.dataset
    kernels = ds.TRAIN.GAUSSIAN_KERNELS if kernels is None else kernels
    return LabelSpec(tuple((int(k[0]), int(k[1])) for k in kernels), tuple((int(a), int(b)) for a, b in ds.PAF.VECTOR),
                     ds.PAF.LINE_WIDTH_THRE, int(ds.STRIDE), tuple(int(v) for v in (ds.OUTPUT_SHAPE if shape is None else shape)),
                     int(ds.ROOT_IDX), int(cfg.DATASET.MAX_PEOPLE))


# ---- the blur taps -----------------------------------------------------------------------------------------------------------
_SMALL_TAPS = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
               7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def gaussian_taps(n):
    """fp32 taps of cv2.getGaussianKernel(n, 0): the fixed tables up to 7, beyond them sigma = 0.3 * ((n - 1) * 0.5 - 1) + 0.8,
    c_i = fp32(exp(-0.5 / sigma^2 * (i - (n - 1) / 2)^2)), k_i = fp32(c_i / sum c_i), the sum in float64 in ascending order."""
    n = int(n)
    if n < 1 or n >= L.LABEL_MAX_TAPS or n % 2 == 0:
        raise ValueError("a blur size is odd and below %d, got %d" % (L.LABEL_MAX_TAPS, n))
    if n in _SMALL_TAPS:
        return np.asarray(_SMALL_TAPS[n], np.float32)
    sigma = 0.3 * ((n - 1) * 0.5 - 1) + 0.8
    scale2x = -0.5 / (sigma * sigma)
    c = np.zeros(n, np.float32)
    total = 0.0
    for i in range(n):
        x = i - (n - 1) * 0.5
        c[i] = np.float32(np.exp(scale2x * x * x))
        total += float(c[i])
    return np.asarray([np.float32(float(v) / total) for v in c], np.float32)


# ---- the descriptor table ----------------------------------------------------------------------------------------------------
def table_layout(B, S, P):
    """Byte offsets of the table's sections and its size (csrc/labels.hip table_layout)."""
    a8 = lambda v: (v + 7) // 8 * 8
    groups = B * S * NL
    t = {"limb_f": 0}
    t["limb_box"] = t["limb_f"] + groups * P * 6 * 8
    t["limb_n"] = t["limb_box"] + groups * P * 4 * 4
    t["imp"] = a8(t["limb_n"] + groups * 4)
    t["imp_n"] = t["imp"] + B * NJ * P * 4
    t["taps"] = a8(t["imp_n"] + B * NJ * 4)
    t["bytes"] = a8(t["taps"] + S * 2 * L.LABEL_MAX_TAPS * 4)
    return t


def table_views(buf, B, S, P):
    """dict of typed numpy views of a table buffer (uint8 [bytes])."""
    t = table_layout(B, S, P)
    groups = B * S * NL
    v = lambda key, dtype, shape: buf[t[key]:t[key] + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)
    return dict(limb_f=v("limb_f", np.float64, (B, S, NL, P, 6)), limb_box=v("limb_box", np.int32, (B, S, NL, P, 4)),
                limb_n=v("limb_n", np.int32, (B, S, NL)), imp=v("imp", np.int32, (B, NJ, P)), imp_n=v("imp_n", np.int32, (B, NJ)),
                taps=v("taps", np.float32, (S, 2, L.LABEL_MAX_TAPS)))


def limb_geometry(bodys, a, b, stride):
    """(centerA / stride [2], unit vector [2], limb_z) of one person's limb a -> b, or None when it is shorter than one cell:
    representation.py:46-47,56-77, expression by expression."""
    centerA = np.array(bodys[a][:3], dtype=int)
    centerB = np.array(bodys[b][:3], dtype=int)
    centerA = centerA.astype(float)
    centerB = centerB.astype(float)
    z_A = centerA[2]
    z_B = centerB[2]
    centerA = centerA[:2]
    centerB = centerB[:2]
    centerB = centerB / stride
    centerA = centerA / stride
    limb_vec = centerB - centerA
    limb_z = z_B - z_A
    norm = np.linalg.norm(limb_vec)
    if norm < 1.0:
        return None
    return centerA, centerB, limb_vec / norm, limb_z


def limb_box(centerA, centerB, thre, grid_x, grid_y):
    """(min_x, max_x, min_y, max_y) of representation.py:80-83 as ints.  The float64 scalars are taken as Python floats first: the same
    IEEE subtraction and the same round-half-even, without numpy's scalar dispatch (four fifths of the packer's time otherwise)."""
    ax, ay, bx, by = float(centerA[0]), float(centerA[1]), float(centerB[0]), float(centerB[1])
    min_x = max(int(round(min(ax, bx) - thre)), 0)
    max_x = min(int(round(max(ax, bx) + thre)), grid_x)
    min_y = max(int(round(min(ay, by) - thre)), 0)
    max_y = min(int(round(max(ay, by) + thre)), grid_y)
    return int(min_x), int(max_x), int(min_y), int(max_y)


def _checked(annotations, need_columns=4):
    out = []
    for i, a in enumerate(annotations):
        a = np.asarray(a, np.float64)
        if a.ndim != 3 or a.shape[1] != NJ or a.shape[2] < need_columns:
            raise ValueError("annotations[%d]: expected [P, 15, C >= %d], got %s" % (i, need_columns, a.shape))
        if len(a) > L.LABEL_MAX_PERSONS:
            raise ValueError("annotations[%d]: at most %d persons per frame, got %d" % (i, L.LABEL_MAX_PERSONS, len(a)))
        if not np.isfinite(a[:, :, :4]).all():
            raise ValueError("annotations[%d]: x, y, Z and the visibility must be finite" % i)
        out.append(a)
    return out


def pack_table(annotations, kernels, thres, paf_vector, stride, shape, with_mds=False):
    """The host half of the renderer: annotations (list of [P_i, 15, C] in network pixels) -> (table uint8 [bytes], ksizes int32 [S, 2], P).
    kernels: S blur sizes (width, height); thres: S line widths."""
    H, W = int(shape[0]), int(shape[1])
    if H < 8 or W < 8 or H * W > MAX_HW:
        raise ValueError("maps are at least 8 x 8 and at most %d cells, got %d x %d" % (MAX_HW, H, W))
    S, B = len(kernels), len(annotations)
    if not 1 <= S <= L.LABEL_MAX_SCALES or len(thres) != S:
        raise ValueError("1 to %d label scales, one line width each" % L.LABEL_MAX_SCALES)
    if B < 1 or B * S > 65535:
        raise ValueError("a batch holds 1 to 65535 // S frames")
    if len(paf_vector) != NL:
        raise ValueError("the skeleton has %d limbs" % NL)
    annotations = _checked(annotations)
    P = max(1, max(len(a) for a in annotations))
    buf = np.zeros(table_layout(B, S, P)["bytes"], np.uint8)
    v = table_views(buf, B, S, P)
    ksizes = np.asarray([[int(k[0]), int(k[1])] for k in kernels], np.int32).reshape(S, 2)
    for s in range(S):
        for d in range(2):
            k = gaussian_taps(ksizes[s, d])
            v["taps"][s, d, :len(k)] = k
    grid_y, grid_x = (H * stride) / stride, (W * stride) / stride          # crop_size / stride (:66-67)
    for f, bodys in enumerate(annotations):
        for j in range(NJ):
            cells = []
            for p in np.flatnonzero(~(bodys[:, j, 3] < 1)) if len(bodys) else ():
                target_y = bodys[p][j][1] / stride
                target_x = bodys[p][j][0] / stride
                y, x = int(target_y), int(target_x)
                if not (0 <= y < H and 0 <= x < W) or target_y < 0 or target_x < 0:
                    raise ValueError("frame %d, person %d, joint %d: (%g, %g) is outside the %d x %d map; the reference indexes "
                                     "out of range here (base_dataset.py:109-119 clears the visibility first)" % (f, p, j, target_x, target_y, H, W))
                if y * W + x not in cells:
                    cells.append(y * W + x)
            v["imp"][f, j, :len(cells)] = cells
            v["imp_n"][f, j] = len(cells)
        for l, (a, b) in enumerate(paf_vector):
            geo = [None] * len(bodys)
            for p in range(len(bodys)):
                if bodys[p][a][3] >= 1 and bodys[p][b][3] >= 1:
                    geo[p] = limb_geometry(bodys[p], a, b, stride)
            boxes = {}                                          # (person, line width) -> box: scales that share a width share it
            for s, thre in enumerate(thres):
                rows_f, rows_box = [], []
                for p in range(len(bodys)):
                    if geo[p] is None:
                        continue
                    if thre > 1 and with_mds and (bodys[p][a][3] < 2 or bodys[p][b][3] < 2):           # :41-45
                        continue
                    centerA, centerB, unit, limb_z = geo[p]
                    rows_f.append((centerA[0], centerA[1], unit[0], unit[1], limb_z, thre))
                    if (p, thre) not in boxes:
                        boxes[p, thre] = limb_box(centerA, centerB, thre, grid_x, grid_y)
                    rows_box.append(boxes[p, thre])
                if rows_f:
                    v["limb_f"][f, s, l, :len(rows_f)] = rows_f
                    v["limb_box"][f, s, l, :len(rows_f)] = rows_box
                v["limb_n"][f, s, l] = len(rows_f)
    return buf, ksizes, P


# ---- the launches ------------------------------------------------------------------------------------------------------------
def launch_table(buf, ksizes, P, B, S, shape, device, out=None):
    """The device half: one page-locked upload of a packed table (pack_table) and the two launches, on the current stream."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("label maps are rendered on the GPU (smap_amd has no CPU path), got device %s" % device)
    H, W = shape
    if out is None:
        out = torch.empty((B, S, NC, H, W), dtype=torch.float32, device=device)
    elif (tuple(out.shape) != (B, S, NC, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device.type != "cuda"
          or (device.index is not None and out.device != device)):
        raise ValueError("out= is a contiguous fp32 tensor [%d, %d, %d, %d, %d] on %s" % (B, S, NC, H, W, device))
    host = torch.empty((len(buf),), dtype=torch.uint8).pin_memory()
    host.numpy()[:] = buf
    with torch.cuda.device(out.device):
        table = host.to(out.device, non_blocking=True)
        ks = (C.c_int32 * (2 * S))(*[int(k) for k in ksizes.reshape(-1)])
        L.check(L.load().smap_render_labels(table.data_ptr(), len(buf), ks, B, S, P, H, W, out.data_ptr(),
                                            torch.cuda.current_stream(out.device).cuda_stream), "smap_render_labels")
    return out


def _render(annotations, kernels, thres, paf_vector, stride, shape, with_mds, device, out=None):
    if torch.device(device).type != "cuda":
        raise ValueError("label maps are rendered on the GPU (smap_amd has no CPU path), got device %s" % device)
    buf, ksizes, P = pack_table(annotations, kernels, thres, paf_vector, stride, shape, with_mds)
    return launch_table(buf, ksizes, P, len(annotations), len(kernels), (int(shape[0]), int(shape[1])), device, out)


def render_labels(annotations, spec, with_mds=False, device="cuda", out=None):
    """annotations: list of B arrays [P_i, 15, C >= 4] (x, y, Z, visibility, ...) in network pixels, P_i may be 0 -> labels
    [B, S, 57, H, W] fp32 on `device` (or `out`), rendered on the current stream.  A joint with visibility >= 1 outside the map is a
    ValueError (JointDataset.remove_illegal_joint clears such visibilities before the reference renders)."""
    return _render(annotations, spec.kernels, spec.thres, spec.paf_vector, spec.stride, spec.shape, with_mds, device, out)


# ---- the host-side pieces of a sample ----------------------------------------------------------------------------------------
def root_depth_labels(bodys, scale, spec):
    """generate_rdepth (:23-34): [MAX_PEOPLE, 3] fp32 rows (y / stride, x / stride, Z / f_x / scale) of the visible roots, sorted far
    to near with the reference's own numpy calls (zero rows sort by their place).  bodys [P, 15, C >= 8]."""
    bodys = _checked([bodys], 8)[0]
    stride, root_idx, max_people = spec.stride, spec.root_idx, spec.max_people
    rdepth = np.zeros((max_people, 3), dtype='float32')
    for j in range(len(bodys)):
        if bodys[j][root_idx, 3] < 1 or j >= max_people:
            continue
        rdepth[j, 0] = bodys[j][root_idx, 1] / stride
        rdepth[j, 1] = bodys[j][root_idx, 0] / stride
        rdepth[j, 2] = bodys[j][root_idx, 2] / bodys[j][root_idx, 7] / scale
    rdepth = rdepth[np.argsort(-rdepth[:, 2])]
    return rdepth


def valid_vector(dataset_name):
    """The [57, 1] channel mask of a sample (base_dataset.py:167-175): COCO has no head top and no depth."""
    valid = np.ones((NJ + NL * 3, 1), np.float64)
    if str(dataset_name).upper() == "COCO":
        valid[1, 0] = 0
        valid[NJ, 0] = 0
        valid[NJ + 1, 0] = 0
        valid[NJ + NL * 2:, 0] = 0
    return valid


ROOT_PATCH = 7          # gt_maps paints the root depth on ROOT_PATCH x ROOT_PATCH cells around a root


def root_depth_map(annotations, metas, spec):
    """[B, 1, H, W] fp32 (host): zero, except Z / f_x / scale (generate_rdepth's value) on the 7 x 7 cells, clipped to the map, around
    every root with visibility >= 1; persons painted far to near, so the nearer one wins an overlap.  This map is this project's own
    construction: the reference supervises root depth at the root points only (lib/utils/loss_h.py:19-23) and has no such map."""
    H, W = spec.shape
    annotations = _checked(annotations, 8)
    out = np.zeros((len(annotations), 1, H, W), np.float32)
    r = ROOT_PATCH // 2
    for f, (bodys, meta) in enumerate(zip(annotations, metas)):
        scale = float(meta["scale"] if isinstance(meta, dict) else meta)
        roots = []
        for p in range(len(bodys)):
            row = bodys[p][spec.root_idx]
            if row[3] < 1:
                continue
            y, x = int(row[1] / spec.stride), int(row[0] / spec.stride)
            roots.append((np.float32(row[2] / row[7] / scale), y, x))
        for d, y, x in sorted(roots, key=lambda t: -float(t[0])):             # stable: equal depths keep the annotation order
            out[f, 0, max(0, y - r):max(0, min(H, y + r + 1)), max(0, x - r):max(0, min(W, x + r + 1))] = d
    return out


def gt_maps(labels, annotations, metas, spec):
    """(hms [B, 43, H, W], det_d [B, 14, H, W], root_d [B, 1, H, W]) at the network's RAW scale (before test.py's / 255 | / 127), from
    labels = render_labels(annotations, spec).  The 2D channels are the sum of the label scales that supervise the three outputs
    SMAP.forward adds (model/smap.py:368-370,418 with COARSE_TO_FINE: the last three scales, last first); det_d is the z channels of
    the last scale; root_d is root_depth_map (metas: one dict with 'scale', or one number, per frame)."""
    B, S = labels.shape[:2]
    if S < 3 or tuple(labels.shape[2:]) != (NC,) + tuple(spec.shape) or len(annotations) != B or len(metas) != B:
        raise ValueError("labels [B, S >= 3, 57, H, W] of these annotations and one meta per frame")
    idx2d = list(range(NJ)) + [NJ + c for c in range(3 * NL) if c % 3 != 2]
    idx2d = torch.tensor(idx2d, dtype=torch.long, device=labels.device)
    hms = labels[:, S - 1].index_select(1, idx2d)
    hms += labels[:, S - 2].index_select(1, idx2d)
    hms += labels[:, S - 3].index_select(1, idx2d)
    det_d = labels[:, S - 1, NJ + 2::3].contiguous()
    root = torch.from_numpy(root_depth_map(annotations, metas, spec)).pin_memory().to(labels.device, non_blocking=True)
    return hms, det_d, root


class GtMapsSource:
    """PosePipeline(maps_source=GtMapsSource(spec)): a batch's maps rendered from ALL its annotations.  Called with
    (annotations, metas): annotations a list / tensor of B arrays [P, 15, C >= 8] in network pixels (zero rows = padding), metas one
    dict with 'scale' per frame.  Visibilities of joints that lie outside the map AS HELD (fp32 annotations can round onto the far
    border) are cleared first, as JointDataset.remove_illegal_joint does."""

    def __init__(self, spec, device="cuda", with_mds=False):
        self.spec, self.device, self.with_mds = spec, device, bool(with_mds)

    def __call__(self, inputs):
        annotations, metas = inputs
        H, W = self.spec.shape
        frames = []
        for a in annotations:
            a = np.array(a.numpy() if isinstance(a, torch.Tensor) else a, np.float64)
            off = (a[:, :, 0] >= W * self.spec.stride) | (a[:, :, 0] < 0) | (a[:, :, 1] >= H * self.spec.stride) | (a[:, :, 1] < 0)
            a[:, :, 3][off] = 0
            frames.append(a)
        labels = render_labels(frames, self.spec, self.with_mds, self.device)
        return gt_maps(labels, frames, metas, self.spec)
