"""The scenes of tests/golden/lossgrad.npz: gen_golden_lossgrad.py and the tests of the loss gradient at native resolution regenerate
the same inputs from a seed (only the seeds and the reference's results are stored).  `sizes` are the source sizes of heads j = 0..3 of
every stage; every head gets its own random tensors and every label channel its own amplitude.

  small     the small schedule's geometry: 16 x 24 output, sources 2x3, 4x6, 8x12, 16x24, B = 2, 3 stages, OHKM, coarse-to-fine,
            upstream 0.37.  Frame 1 carries the COCO mask (14 zero-weight depth channels).  Root rows of frame 0: two persons on one
            cell, one row on each corner cell -- (15, 23) lies in the last source row and column, i0 == i1 -- and a Z <= 0 row between
            counted rows.
  odd       13 x 9 (H * W % 4 != 0), sources 1x1, 3x2, 7x5, 13x9, B = 1, no mining.
  ratios    degenerate and non-integer ratios: 16 x 24 with sources 1x5, 4x1, 5x7, 16x24, B = 2, 1 stage.
"""
import numpy as np

NC, N2D, NDD = 57, 43, 14
CHANNELS = (N2D, NDD, 1)

SCENES = {
    "small": dict(seed=5105, B=2, H=16, W=24, sizes=[(2, 3), (4, 6), (8, 12), (16, 24)], stage_num=3, ohkm=True, topk=8, ctf=True, S=5,
                  upstream=0.37, coco_frames=[1],
                  rows=[[(2.3, 4.7, 1.5), (2.9, 4.1, 0.8), (0.0, 0.0, 1.2), (3.0, 3.0, -1.0), (0.2, 23.0, 0.9), (15.0, 0.5, 1.1),
                         (15.9, 23.5, 0.7)], [(5.5, 6.5, 2.0), (0, 0, 0), (9.0, 17.0, 0.6)]]),
    "odd": dict(seed=6206, B=1, H=13, W=9, sizes=[(1, 1), (3, 2), (7, 5), (13, 9)], stage_num=2, ohkm=False, topk=8, ctf=False, S=4,
                upstream=1.0, rows=[[(6.2, 4.4, 1.0), (12.0, 8.0, 2.5)]]),
    "ratios": dict(seed=7307, B=2, H=16, W=24, sizes=[(1, 5), (4, 1), (5, 7), (16, 24)], stage_num=1, ohkm=True, topk=5, ctf=True, S=5,
                   upstream=2.0, zero_valids={0: [3, 20, 50]}, rows=[[(1.5, 2.5, 0.7)], [(9.0, 13.0, 1.9), (4.0, 4.0, 0.0), (15.5, 23.5, 0.4)]]),
}


def coco_valid():
    """smap_amd.labels.valid_vector('COCO'), flat."""
    v = np.ones(NC, np.float32)
    v[[1, 15, 16]] = 0
    v[N2D:] = 0
    return v


def head_scale(s, h):
    """Label scale of head h = 4 * stage + j: j, plus 1 on the last stage with coarse-to-fine."""
    return h % 4 + (1 if h // 4 == s["stage_num"] - 1 and s["ctf"] else 0)


# not in the fixture (the kernels against the restatement only): ONE head group at the real geometry, ratios 127 / 15 and 207 / 25
REAL = dict(seed=8408, B=1, H=128, W=208, sizes=[(16, 26), (32, 52), (64, 104), (128, 208)], stage_num=1, ohkm=True, topk=8, ctf=True, S=5,
            upstream=0.5, rows=[[(127.0, 207.0, 1.0), (40.3, 99.9, 2.0), (0.0, 100.0, 0.0), (63.5, 103.5, 0.8)]])


def inputs(name):
    """dict(src: n_heads lists of three fp32 arrays [B, 43 | 14 | 1, h, w]; labels [B, S, 57, H, W]; valids [B, 57]; rdepth [B, R, 3])
    of a scene of SCENES by name, or of a dict like them."""
    s = SCENES[name] if isinstance(name, str) else name
    rng = np.random.RandomState(s["seed"])
    B, H, W, S = s["B"], s["H"], s["W"], s["S"]
    draw = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    labels = draw(B, S, NC, H, W) * (0.5 + rng.uniform(0, 3, (1, 1, NC, 1, 1))).astype(np.float32)
    src = []
    for h in range(4 * s["stage_num"]):
        sh, sw = s["sizes"][h % 4]
        src.append([draw(B, c, sh, sw) * np.float32(1 + 0.1 * h) for c in CHANNELS])
    valids = np.ones((B, NC), np.float32)
    for b in s.get("coco_frames", []):
        valids[b] = coco_valid()
    for b, channels in s.get("zero_valids", {}).items():
        valids[b, channels] = 0
    R = max(1, max(len(r) for r in s["rows"]))
    rdepth = np.zeros((B, R, 3), np.float32)
    for b, rows in enumerate(s["rows"]):
        for r, row in enumerate(rows):
            rdepth[b, r] = row
    return dict(src=src, labels=labels, valids=valids, rdepth=rdepth)
