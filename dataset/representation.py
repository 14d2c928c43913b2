"""Label rendering under the reference's import path (reference: dataset/representation.py:5-53).

The three functions keep the reference's signatures, take and return numpy arrays and handle one frame at one label scale per call;
the maps are rendered on the GPU by smap_amd.labels (csrc/labels.hip), the root depths on the host.  A caller that renders whole
samples or batches uses smap_amd.labels.render_labels: one upload and two launches for every frame and scale together.
The part-affinity fields and the root depths are bit for bit the reference's; the heat-maps follow cv2.GaussianBlur as DESIGN.md
"Label maps" states it (OpenCV is not part of this image)."""
import numpy as np

from smap_amd import labels as _labels

_ONE_LIMB_WIDTH = (1,)


def _device():
    import torch
    return "cuda:%d" % torch.cuda.current_device()


def _bodys(bodys):
    return np.asarray(bodys, np.float64).reshape(-1, _labels.NJ, np.shape(bodys)[-1] if len(bodys) else 4)


def generate_heatmap(bodys, output_shape, stride, keypoint_num, kernel=(7, 7)):
    if keypoint_num != _labels.NJ:
        raise ValueError("the skeleton has %d key points" % _labels.NJ)
    limbs = tuple(map(tuple, _default_limbs()))
    out = _labels._render([_bodys(bodys)], (tuple(kernel),), _ONE_LIMB_WIDTH, limbs, stride, tuple(output_shape), False, _device())
    return out[0, 0, :keypoint_num].cpu().numpy()


def generate_rdepth(meta, stride, root_idx, max_people):
    spec = _labels.LabelSpec((), (), 1, stride, (0, 0), root_idx, max_people)
    return _labels.root_depth_labels(_bodys(meta['bodys']), meta['scale'], spec)


def generate_paf(bodys, output_shape, params_transform, paf_num, paf_vector, paf_thre, with_mds):
    if paf_num != _labels.NL or len(paf_vector) != paf_num:
        raise ValueError("the skeleton has %d limbs" % _labels.NL)
    stride = params_transform['stride']
    grid = (params_transform['crop_size_y'] / stride, params_transform['crop_size_x'] / stride)
    if tuple(grid) != tuple(output_shape):
        raise ValueError("crop_size / stride %s is not the map shape %s" % (grid, tuple(output_shape)))
    out = _labels._render([_bodys(bodys)], ((1, 1),), (paf_thre,), tuple((int(a), int(b)) for a, b in paf_vector), stride,
                          tuple(int(v) for v in output_shape), bool(with_mds), _device())
    return out[0, 0, _labels.NJ:].cpu().numpy()


def _default_limbs():
    from dataset.data_settings import MIX
    return MIX.PAF.VECTOR
