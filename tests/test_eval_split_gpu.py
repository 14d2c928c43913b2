"""GPU: both scorers of csrc/eval.hip at the split between their two launch paths -- (B, G) = (16, 64), 1024 person rows, the last
shape of the fused launch, and (17, 64), the first shape of terms-then-fold -- against the sequential numpy restatements that
tests/test_eval_cpu.py and tests/test_eval_maps_cpu.py pin to the reference's fixtures.  The library is called directly, so that
the term rows can be handed over full of NaN; counts holds 0, 1, G, a value above G and a negative one, which the library clamps,
and every input row at or beyond the clamped count is NaN: a row read or written out of turn shows in the sums or in the rows."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_eval_gpu import new_acc, restate_eval_3d
from test_eval_gpu import same_bits as same_bits_nan_aware
from test_eval_maps_gpu import O_DD, O_DE, assert_close_to_reference, restate_maps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NJ, NL, MAXP, G, B_MAX = 15, 14, 127, 64, 17
COUNTS = np.asarray([0, 1, G, G + 6, -3, 37, 64, 9, 50, 2, 63, 21, 64, 33, 5, 48, 12], np.int32)
CLAMPED = np.clip(COUNTS, 0, G)
ROOT_ERROR_OF_THE_ROOT = 15 + 2        # |(gt_2 - gt_2) - (pred_2 - pred_2)|: zero whatever the inputs


def inputs_3d():
    """-> pred [17,127,15,4], gt [17,64,15,4]: errors on both sides of 15, missing joints, persons and roots, hidden ground-truth roots,
    depth orders that agree and that do not; NaN from each frame's clamped count on."""
    rng = np.random.default_rng(1664)
    gt = np.zeros((B_MAX, G, NJ, 4))
    gt[..., :3] = rng.uniform(-80, 80, (B_MAX, G, NJ, 3))
    gt[:, :, 2, 2] = rng.uniform(200, 500, (B_MAX, G))
    gt[..., 3] = np.where(rng.random((B_MAX, G, NJ)) < 0.1, 1.0, 2.0)
    pred = np.zeros((B_MAX, MAXP, NJ, 4))
    pred[:, :G, :, :3] = gt[..., :3] + rng.normal(0, 9, (B_MAX, G, NJ, 3))
    pred[:, :G, 2, 2] = rng.uniform(200, 500, (B_MAX, G))
    pred[:, :G, :, 3] = np.where(rng.random((B_MAX, G, NJ)) < 0.1, 0.0, rng.uniform(0.3, 1.0, (B_MAX, G, NJ)))
    pred[:, :G][rng.random((B_MAX, G)) < 0.05] = 0.0
    for b, n in enumerate(CLAMPED):
        pred[b, n:], gt[b, n:] = np.nan, np.nan
    return pred, gt


def inputs_maps():
    """-> pred_2d [17,127,15,4], depth_v [17,127,14], bone_mask [17,127], gt_2d [17,64,15,4]: keypoints inside and outside the head
    size, unmatched rows, hidden joints, limbs sampled and not, depth products on both sides of -1; NaN (mask: all ones) from each
    frame's clamped count on."""
    rng = np.random.default_rng(1088)
    gt = np.zeros((B_MAX, G, NJ, 4))
    gt[..., :2] = rng.uniform(100, 700, (B_MAX, G, 1, 2)) + rng.normal(0, 40, (B_MAX, G, NJ, 2))
    gt[..., 2] = rng.uniform(200, 500, (B_MAX, G, NJ))
    gt[..., 3] = np.where(rng.random((B_MAX, G, NJ)) < 0.1, 1.0, 2.0)
    pred = np.zeros((B_MAX, MAXP, NJ, 4))
    pred[:, :G, :, :2] = gt[..., :2] + rng.normal(0, 10, (B_MAX, G, NJ, 2))
    pred[:, :G, :, 2:] = rng.uniform(0.3, 1.0, (B_MAX, G, NJ, 2))
    pred[:, :G][rng.random((B_MAX, G)) < 0.05] = 0.0
    depth_v = np.zeros((B_MAX, MAXP, NL))
    depth_v[:, :G] = rng.normal(0, 60, (B_MAX, G, NL))
    mask = np.zeros((B_MAX, MAXP), np.int32)
    mask[:, :G] = rng.integers(0, 1 << NL, (B_MAX, G))
    for b, n in enumerate(CLAMPED):
        pred[b, n:], depth_v[b, n:], mask[b, n:], gt[b, n:] = np.nan, np.nan, -1, np.nan
    return pred, depth_v, mask, gt


def expected_3d(pred, gt):
    """-> the restatement's accumulators after 16 and after 17 frames, on the clamped counts."""
    acc, out = new_acc(), {}
    for b, n in enumerate(CLAMPED):
        restate_eval_3d(pred[b, :n], gt[b, :n], acc)
        out[b + 1] = acc.copy()
    return out


def expected_maps(pred, depth_v, mask, gt):
    acc, out = np.zeros(87), {}
    for b, n in enumerate(CLAMPED):
        restate_maps(pred[b, :n], gt[b, :n], depth_v[b, :n], mask[b, :n], acc)
        out[b + 1] = acc.copy()
    return out


def means_something(want, but=()):
    """Finite, and every field but `but` non-zero: equality with these sums is no equality of zeros."""
    return np.isfinite(want).all() and (np.delete(want, list(but)) != 0).all()


@pytest.fixture(scope="module")
def cases():
    i3, im = inputs_3d(), inputs_maps()
    return {"3d": (i3, expected_3d(*i3)), "maps": (im, expected_maps(*im))}


def _call(lib, scorer, B, arrays):
    """acc_init, then one update of the first B frames with the term rows full of NaN -> (acc [NF], terms [B,G,NF], device inputs)."""
    nf = 80 if scorer == "3d" else 87
    dev = [torch.from_numpy(np.ascontiguousarray(a[:B])).to(DEV) for a in arrays]
    counts = torch.from_numpy(COUNTS[:B].copy()).to(DEV)
    terms = torch.full((B, G, nf), float("nan"), dtype=torch.float64, device=DEV)
    acc = torch.empty(nf, dtype=torch.float64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if scorer == "3d":
        assert lib.smap_eval3d_acc_init(p(acc), st) == 0
        assert lib.smap_eval3d_update(p(dev[0]), p(counts), p(dev[1]), B, G, p(terms), p(acc), st) == 0
    else:
        assert lib.smap_evalmaps_acc_init(p(acc), st) == 0
        assert lib.smap_evalmaps_update(p(dev[0]), p(dev[1]), p(dev[2]), p(counts), p(dev[3]), B, G, p(terms), p(acc), st) == 0
    return acc.cpu().numpy(), terms.cpu().numpy(), dev, counts


@pytest.mark.parametrize("B", [16, 17])
@pytest.mark.parametrize("scorer", ["3d", "maps"])
def test_both_sides_of_the_launch_split_equal_the_restatement(cases, scorer, B):
    from smap_amd import lib as L
    lib = L.load()
    assert (B * G > 1024) == (B == 17) and {0, 1, G}.issubset(COUNTS[:B].tolist()) and COUNTS[:B].max() > G and COUNTS[:B].min() < 0
    arrays, expected = cases[scorer]
    want = expected[B]
    assert means_something(want, but=[ROOT_ERROR_OF_THE_ROOT] if scorer == "3d" else [])
    got, rows, dev, counts = _call(lib, scorer, B, arrays)
    if scorer == "3d":
        assert same_bits_nan_aware(got, want) and not np.isnan(got).any()
    else:                                                        # distance_e under its derived bound, every other field bit for bit
        assert_close_to_reference(got, want, int(CLAMPED[:B].sum()), B, f"B = {B}")
        assert (got[O_DE:O_DD] > 0).all()
    for b, n in enumerate(CLAMPED[:B]):                          # a person's row is written whole, the rows beyond the count not at all
        assert np.isnan(rows[b, n:]).all() and not np.isnan(rows[b, :n]).any()
    if scorer == "3d":                                           # the two exported halves, one after the other: the same bits
        p = lambda t: C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        terms = torch.full((B, G, 80), float("nan"), dtype=torch.float64, device=DEV)
        acc = torch.empty(80, dtype=torch.float64, device=DEV)
        assert lib.smap_eval3d_acc_init(p(acc), st) == 0
        assert lib.smap_eval3d_terms(p(dev[0]), p(counts), p(dev[1]), B, G, p(terms), st) == 0
        assert lib.smap_eval3d_fold(p(terms), p(counts), B, G, p(acc), st) == 0
        assert acc.cpu().numpy().tobytes() == got.tobytes()
