"""The inputs of tests/golden/valloss_small.npz: gen_golden_valloss.py and the validation-loss tests regenerate them from the seed, as
loss_scenes.py does for loss.npz (the fixture stores the seed and the reference's results only).

Network, weights and images are those of backbone_small.npz: x [2, 3, 64, 96], maps 16 x 24, head levels 2x3 / 4x6 / 8x12 / 16x24.
Labels [2, 5, 57, 16, 24] with per-channel amplitudes as loss_scenes.inputs draws them; root rows: frame 0 on cells (0, 0) and
(H - 1, W - 1) with fractional coordinates, and a Z <= 0 row; frame 1 one row.
  ones   every channel valid
  coco   frame 1 carries the COCO channel mask (its 14 depth channels weigh zero)
"""
import numpy as np

from loss_scenes import coco_valid

SEED = 5505
CASES = ("ones", "coco")
B, S, NC, H, W = 2, 5, 57, 16, 24
ROWS = [[(0.0, 0.0, 1.2), (15.9, 23.5, 0.7), (3.0, 3.0, -1.0)], [(5.5, 6.5, 2.0)]]


def inputs(case):
    """dict(labels [2, 5, 57, 16, 24], valids [2, 57], rdepth [2, 3, 3]), fp32."""
    assert case in CASES
    rng = np.random.RandomState(SEED)
    labels = rng.standard_normal((B, S, NC, H, W)).astype(np.float32) * (0.5 + rng.uniform(0, 3, (1, 1, NC, 1, 1))).astype(np.float32)
    valids = np.ones((B, NC), np.float32)
    if case == "coco":
        valids[1] = coco_valid()
    rdepth = np.zeros((B, max(len(r) for r in ROWS), 3), np.float32)
    for b, rows in enumerate(ROWS):
        for r, row in enumerate(rows):
            rdepth[b, r] = row
    return dict(labels=labels, valids=valids, rdepth=rdepth)
