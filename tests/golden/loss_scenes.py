"""The scenes of tests/golden/loss.npz: gen_golden_loss.py and the loss tests regenerate the same inputs from a seed (only the seeds
and the reference's results are stored).  Every head gets its own random outputs, so a swapped pointer or label scale shows.

  scalar    B = 2, 9 x 11 (odd area: the 4-byte path), 3 stages, OHKM, coarse-to-fine, S = 5, every channel valid; three roots in frame
            0, two of them on one cell with fractional coordinates; frame 1 has none.
  vector    B = 3, 16 x 24 (more pixels than threads in a workgroup: the 16-byte path); frame 1 carries the COCO channel mask (all 14
            depth channels weigh zero: top-k over 14 zeros); a Z <= 0 row between positive rows; roots on cells (0, 0) and
            (H - 1, W - 1); one root whose y in (-1, 0) truncates to row 0.
  squeeze   B = 1 (the reference's valid.squeeze() changes rank there), 8 x 8, 1 stage, no OHKM, no coarse-to-fine, S = 4, no root.
  upstream  B = 2, 12 x 20, 2 stages, topk = 3, backward through total_loss * 0.37; a few zero-weight channels.
"""
import numpy as np

NC, N2D, NDD = 57, 43, 14

SCENES = {
    "scalar": dict(seed=1101, B=2, H=9, W=11, stage_num=3, ohkm=True, topk=8, ctf=True, S=5, upstream=1.0,
                   rows=[[(2.3, 4.7, 1.5), (2.9, 4.1, 0.8), (7.0, 10.0, 2.2), (0, 0, 0)], []]),
    "vector": dict(seed=2202, B=3, H=16, W=24, stage_num=3, ohkm=True, topk=8, ctf=True, S=5, upstream=1.0,
                   rows=[[(0.0, 0.0, 1.2), (0, 0, 0), (15.9, 23.5, 0.7), (3.0, 3.0, -1.0), (8.0, 9.0, 0.4)], [(5.5, 6.5, 2.0)],
                         [(-0.5, 3.2, 0.9)]]),
    "squeeze": dict(seed=3303, B=1, H=8, W=8, stage_num=1, ohkm=False, topk=8, ctf=False, S=4, upstream=1.0, rows=[[]]),
    "upstream": dict(seed=4404, B=2, H=12, W=20, stage_num=2, ohkm=True, topk=3, ctf=True, S=5, upstream=0.37,
                     rows=[[(1.2, 2.2, 1.1)], [(11.0, 19.0, 0.6), (4.5, 4.5, 3.0)]]),
}


def coco_valid():
    """smap_amd.labels.valid_vector('COCO'), flat."""
    v = np.ones(NC, np.float32)
    v[[1, 15, 16]] = 0
    v[N2D:] = 0
    return v


def inputs(name):
    """dict(hm, dd, rd: lists of n_heads fp32 arrays; labels [B, S, 57, H, W]; valids [B, 57]; rdepth [B, R, 3]) of a scene."""
    s = SCENES[name]
    rng = np.random.RandomState(s["seed"])
    B, H, W, S = s["B"], s["H"], s["W"], s["S"]
    n_heads = 4 * s["stage_num"]
    draw = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    # every channel its own amplitude, so that the per-channel losses are spread out (the generator asserts: no near tie in a top-k)
    labels = draw(B, S, NC, H, W) * (0.5 + rng.uniform(0, 3, (1, 1, NC, 1, 1))).astype(np.float32)
    hm = [draw(B, N2D, H, W) * np.float32(1 + 0.1 * h) for h in range(n_heads)]
    dd = [draw(B, NDD, H, W) * np.float32(1 + 0.1 * h) for h in range(n_heads)]
    rd = [draw(B, 1, H, W) for h in range(n_heads)]
    valids = np.ones((B, NC), np.float32)
    if name == "vector":
        valids[1] = coco_valid()
    if name == "upstream":
        valids[0, [3, 20, 50]] = 0
        valids[1, [0, 44]] = 0
    R = max(1, max(len(r) for r in s["rows"]))
    rdepth = np.zeros((B, R, 3), np.float32)
    for b, rows in enumerate(s["rows"]):
        for r, row in enumerate(rows):
            rdepth[b, r] = row
    return dict(hm=hm, dd=dd, rd=rd, labels=labels, valids=valids, rdepth=rdepth)


# ---- what the tests derive from a scene's inputs (plain numpy) ---------------------------------------------------------------------
LABEL_CHANNEL = list(range(15)) + [15 + 3 * (c // 2) + c % 2 for c in range(28)] + [15 + 3 * c + 2 for c in range(NDD)]


def head_scale(s, h):
    """Label scale of head h = 4 * stage + j: j, plus 1 on the last stage with coarse-to-fine."""
    return h % 4 + (1 if h // 4 == s["stage_num"] - 1 and s["ctf"] else 0)


def differences(name, x, dtype=np.float64):
    """Per head the differences out - label, [B, 57, H, W] in OUTPUT order (43 2D channels, then the 14 depth channels): in float64
    the exact ones the reference works on, in float32 the rounded ones the kernels work on."""
    s = SCENES[name]
    out = []
    for h in range(4 * s["stage_num"]):
        lab = x["labels"][:, head_scale(s, h)][:, LABEL_CHANNEL]
        out.append(np.concatenate([x["hm"][h], x["dd"][h]], axis=1).astype(dtype) - lab.astype(dtype))
    return out


def host_sums(name, x, dtype=np.float64):
    """float64 [n_heads, B, 57]: the sum over a plane of double(d) * double(d)."""
    return np.stack([(d.astype(np.float64) ** 2).sum(axis=(2, 3)) for d in differences(name, x, dtype)])


def rd_at_rows(name, x):
    """fp32 [n_heads, B, R]: root_d at the cell of every counted row that lies on the map, 0 elsewhere."""
    s = SCENES[name]
    rdepth = x["rdepth"]
    out = np.zeros((4 * s["stage_num"],) + rdepth.shape[:2], np.float32)
    for h in range(len(out)):
        for b in range(rdepth.shape[0]):
            for r in range(rdepth.shape[1]):
                y, xx, z = rdepth[b, r]
                if z > 0 and -1 < y < s["H"] and -1 < xx < s["W"]:
                    out[h, b, r] = x["rd"][h][b, 0, int(y), int(xx)]
    return out
