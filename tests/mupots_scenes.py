"""Constructed MuPoTS-3D scenes for tests/test_mupots_cpu.py and tests/test_mupots_gpu.py: three sequences of 1, 5 and 12 frames that
hold every edge the protocol has (the list is in `build`), the binary scene file of tests/c/mupots_main.cpp, and a writer of the
MuPoTS annotation layout (TS<k>/annot.mat, TS<k>/occlusion.mat).  Plain numpy; imports nothing of the package under test."""
import os

import numpy as np

from mupots_restate import SMAP_ORDER

NJ = 15
ORDER0 = np.asarray(SMAP_ORDER) - 1
# a standing skeleton in the protocol's joint order, millimetres from the pelvis (y down)
TEMPLATE = np.array([[0, -700, 0], [0, -500, 0], [-180, -480, 0], [-250, -250, 20], [-260, -20, 40], [180, -480, 0], [250, -250, 20],
                     [260, -20, 40], [-100, 0, 0], [-110, 400, 10], [-115, 800, 20], [100, 0, 0], [110, 400, 10], [115, 800, 20],
                     [0, 0, 0]], np.float64)
CONFIGS = {"default": (1, 1, 0), "matched_only": (1, 1, 1), "no_skel": (1, 0, 0), "absolute": (0, 1, 0), "absolute_matched": (0, 0, 1)}
SEQ_FRAMES = (1, 5, 12)


def to_smap(a):
    """[15,C] in the protocol's order -> SMAP's order (what pose2d.mat / pose3d.mat hold)."""
    out = np.zeros_like(a)
    out[ORDER0] = a
    return out


def person(c2, pelvis, scale=1.0, wobble=None):
    """-> gt2 [15,2] pixels, gt3 [15,3] mm."""
    t = TEMPLATE * scale + (0 if wobble is None else wobble)
    t[14] = 0
    return np.asarray(c2, np.float64) + TEMPLATE[:, :2] * 0.25, np.asarray(pelvis, np.float64) + t


def pred_like(gt2, gt3, d2=(1.0, -1.0), scale=1.1, off=(10.0, -5.0, 30.0), wobble=None):
    """A prediction near a ground-truth person, protocol order -> p2 [15,2], p3 [15,3]."""
    rel = (gt3 - gt3[14]) * scale + (0 if wobble is None else wobble)
    rel[14] = 0                                                    # the pelvis stays where `off` puts it
    return gt2 + np.asarray(d2, np.float64), gt3[14] + np.asarray(off, np.float64) + rel


def far(i, rng):
    """A prediction far from everybody."""
    return np.array([6000.0 + 60 * i, 5000.0]) + TEMPLATE[:, :2] * 0.25, np.array([0.0, 0.0, 9000.0]) + TEMPLATE + rng.normal(0, 20, (NJ, 3))


def build():
    """-> scene dict: seq_offset [4], gt_count [18], gt2d [18,16,15,2], gt3d [18,16,15,3], occ [18,16,15]; preds: per frame
    (p2 [P,15,2], p3 [P,15,4]) in SMAP order or None (no entry); expect_match: {frame: matching}.

    seq 0   f0  one person, P = 1, prediction == ground truth; no ordinal pair in the sequence (rate NaN, mean NaN)
    seq 1   f1  no valid person (predictions present)
            f2  two persons, an entry without predictions: both unmatched (100000), an ordinal pair of two unmatched persons
            f3  P = 65: person 0 matches prediction 64, person 1 prediction 5
            f4  P = 127: predictions 3 and 70 tie for person 0 (3 wins), 10 and 20 tie for person 1 (10 wins), person 2 matches 126;
                prediction 90 is a worse candidate for person 0
            f5  two persons compete for one prediction: the second stays unmatched; an ordinal pair with an unmatched person
    seq 2   f6  |dx| exactly 40 on every matching joint: no match
            f7  |dx| 40 on all but one joint (39.75): matched with score 1
            f8  ground truth near the origin; prediction 0 all at exactly (0, 0) (score 0), prediction 1 has five joints at (0, 0): matched
            f9  shoulder and elbow missing (zeros): a zero bone, NaN at the elbow and the wrist; elbow occluded, wrist visible
            f10 integer coordinates, prediction = ground truth + (90, 120, 0) about the pelvis: error exactly 150 without use_skel
            f11 ordinal: product > 0                     f12 ordinal: both differences < 300 (product < 0)
            f13 ordinal: product exactly 0, ground-truth gap 400    f14 ordinal: reversed
            f15 16 valid persons, 16 predictions         f16 three persons, six predictions, noise
            f17 no valid person, no entry
    """
    rng = np.random.default_rng(5)
    frames = []                                                    # (persons [(gt2, gt3, occ)], preds [(p2, p3)] or None)
    expect = {}
    occ_rng = lambda: (rng.random(NJ) < 0.3).astype(np.float64)
    wob = lambda s: rng.normal(0, s, (NJ, 3))

    def frame(persons, preds, match=None):
        if match is not None:
            expect[len(frames)] = match
        frames.append((persons, preds))

    # f0
    g2, g3 = person((500, 400), (100, 50, 3000), wobble=wob(10))
    frame([(g2, g3, occ_rng())], [(g2.copy(), g3.copy())], [0])
    # f1
    frame([], [far(0, rng)])
    # f2
    a, b = person((300, 300), (-500, 0, 2500), wobble=wob(10)), person((900, 300), (600, 0, 4100), wobble=wob(10))
    frame([(*a, occ_rng()), (*b, occ_rng())], [], [-1, -1])
    # f3
    a, b = person((300, 300), (-500, 0, 2500), wobble=wob(10)), person((900, 300), (600, 0, 4100), wobble=wob(10))
    preds = [far(i, rng) for i in range(65)]
    preds[64] = pred_like(*a, wobble=wob(15))
    preds[5] = pred_like(*b, wobble=wob(15))
    frame([(*a, occ_rng()), (*b, occ_rng())], preds, [64, 5])
    # f4
    a, b, c = (person((300, 300), (-500, 0, 2500), wobble=wob(10)), person((900, 300), (600, 0, 4100), wobble=wob(10)),
               person((1500, 300), (1500, 100, 3300), wobble=wob(10)))
    preds = [far(i, rng) for i in range(127)]
    preds[3] = pred_like(*a, wobble=wob(15))
    preds[70] = (preds[3][0].copy(), pred_like(*a, scale=0.9, wobble=wob(40))[1])           # the same 2D: the same score
    worse = pred_like(*a, wobble=wob(15))
    worse[0][2:6] += 50.0
    preds[90] = worse
    preds[10] = pred_like(*b, wobble=wob(15))
    preds[20] = (preds[10][0].copy(), pred_like(*b, scale=1.3, wobble=wob(40))[1])
    preds[126] = pred_like(*c, wobble=wob(15))
    frame([(*a, occ_rng()), (*b, occ_rng()), (*c, occ_rng())], preds, [3, 10, 126])
    # f5
    a = person((600, 400), (0, 0, 3000), wobble=wob(10))
    b = person((605, 403), (50, 0, 3600), wobble=wob(10))
    frame([(*a, occ_rng()), (*b, occ_rng())], [pred_like(*a, wobble=wob(15))], [0, -1])
    # f6: integer pixels, dx = exactly 40 on every joint
    a = person((400, 400), (0, 0, 3000))
    p = pred_like(*a, d2=(40.0, 0.0))
    frame([(*a, occ_rng())], [p], [-1])
    # f7: one joint at 39.75
    p = pred_like(*a, d2=(40.0, 0.0))
    p[0][7, 0] -= 0.25
    frame([(*a, occ_rng())], [p], [0])
    # f8: the ground truth within 40 px of the origin
    a = person((0, 0), (0, 0, 3000), wobble=wob(10))
    a = (a[0] * 0.2, a[1])
    p0 = pred_like(*a)
    p0 = (np.zeros((NJ, 2)), p0[1])
    p1 = pred_like(*a, wobble=wob(15))
    p1[0][[2, 4, 6, 8, 10]] = 0.0
    frame([(*a, occ_rng())], [p0, p1], [1])
    # f9: right shoulder (2) and right elbow (3) missing -> zero bone at the elbow, NaN at elbow (3) and wrist (4)
    a = person((700, 300), (200, -100, 2800), wobble=wob(10))
    p = pred_like(*a, wobble=wob(15))
    p[0][[2, 3]] = 0.0
    p[1][[2, 3]] = 0.0
    o = np.zeros(NJ)
    o[3] = 1.0
    frame([(*a, o)], [p], [0])
    # f10: exactly 150
    a = person((800, 500), (300, -200, 3200))
    p = pred_like(*a, scale=1.0, off=(7.0, -3.0, 64.0))
    p[1][:14] += np.array([90.0, 120.0, 0.0])
    frame([(*a, occ_rng())], [p], [0])

    def pair(gz, pz):
        a_ = person((300, 300), (-500, 0, gz[0]), wobble=wob(10))
        b_ = person((900, 300), (600, 0, gz[1]), wobble=wob(10))
        pa = pred_like(*a_, off=(10.0, -5.0, pz[0] - gz[0]), wobble=wob(15))
        pb = pred_like(*b_, off=(10.0, -5.0, pz[1] - gz[1]), wobble=wob(15))
        frame([(*a_, occ_rng()), (*b_, occ_rng())], [pb, pa], [1, 0])

    pair((3000.0, 3500.0), (2900.0, 3600.0))                       # f11
    pair((3000.0, 3100.0), (3050.0, 3040.0))                       # f12
    pair((3000.0, 3400.0), (3200.0, 3200.0))                       # f13
    pair((3000.0, 3500.0), (3500.0, 3000.0))                       # f14
    # f15
    persons, preds = [], []
    for g in range(16):
        a = person((200 + 300 * (g % 8), 300 + 500 * (g // 8)), (-2000 + 300 * g, 0, 2500 + 170 * ((7 * g) % 16)), wobble=wob(10))
        persons.append((*a, occ_rng()))
        preds.append(pred_like(*a, off=(10.0, -5.0, float(rng.normal(0, 250))), wobble=wob(15)))
    preds = preds[::-1]
    frame(persons, preds, list(range(15, -1, -1)))
    # f16
    persons, preds = [], [far(i, rng) for i in range(6)]
    for g in range(3):
        a = person((300 + 400 * g, 350), (-700 + 700 * g, 0, 3000 + 200 * g), wobble=wob(10))
        persons.append((*a, occ_rng()))
        preds[2 * g] = pred_like(*a, off=(10.0, -5.0, float(rng.normal(0, 100))), wobble=wob(30))
    frame(persons, preds, [0, 2, 4])
    # f17
    frame([], None)

    F, G = len(frames), 16
    assert F == sum(SEQ_FRAMES)
    scene = {"seq_offset": np.concatenate([[0], np.cumsum(SEQ_FRAMES)]).astype(np.int32), "gt_count": np.zeros(F, np.int32),
             "gt2d": np.zeros((F, G, NJ, 2)), "gt3d": np.zeros((F, G, NJ, 3)), "occ": np.zeros((F, G, NJ)), "preds": [], "expect_match": expect}
    for f, (persons, preds) in enumerate(frames):
        scene["gt_count"][f] = len(persons)
        for g, (g2, g3, o) in enumerate(persons):
            scene["gt2d"][f, g], scene["gt3d"][f, g], scene["occ"][f, g] = g2, g3, o
        if preds is None:
            scene["preds"].append(None)
        else:
            p2 = np.zeros((len(preds), NJ, 2))
            p3 = np.zeros((len(preds), NJ, 4))
            for i, (a2, a3) in enumerate(preds):
                p2[i], p3[i, :, :3], p3[i, :, 3] = to_smap(a2), to_smap(a3), 1.0
            scene["preds"].append((p2, p3))
    return scene


def restate_preds(scene):
    """The per-frame predictions as mupots_restate.score takes them: a frame with valid persons and no entry would be an error there."""
    return [p if p is not None else (np.zeros((0, NJ, 2)), np.zeros((0, NJ, 4))) for p in scene["preds"]]


def packed(scene):
    """-> pred2d [sumP,15,2], pred3d [sumP,15,4], pred_offset [F+1]."""
    p2 = [p[0] for p in scene["preds"] if p is not None and len(p[0])]
    p3 = [p[1] for p in scene["preds"] if p is not None and len(p[0])]
    off = np.concatenate([[0], np.cumsum([0 if p is None else len(p[0]) for p in scene["preds"]])]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate(p2)), np.ascontiguousarray(np.concatenate(p3)), off


def pose_dicts(scene, sequences=(1, 2, 3), ext=".jpg"):
    """-> (pose2d, pose3d) keyed like lib.eval.convert.convert_records' output."""
    pose2d, pose3d, f = {}, {}, 0
    for k, n in zip(sequences, SEQ_FRAMES):
        for i in range(n):
            if scene["preds"][f] is not None:
                name = "TS%d/img_%06d%s" % (k, i, ext)
                pose2d[name] = np.concatenate([scene["preds"][f][0], np.ones((len(scene["preds"][f][0]), NJ, 2))], 2)
                pose3d[name] = scene["preds"][f][1]
            f += 1
    return pose2d, pose3d


def write_scene_bin(path, scene, config):
    """The input of tests/c/mupots_main.cpp."""
    p2, p3, off = packed(scene)
    F, G = scene["gt2d"].shape[:2]
    with open(path, "wb") as f:
        np.asarray([F, G, len(scene["seq_offset"]) - 1, len(p2), *config, 0], np.int32).tofile(f)
        for a in (scene["gt2d"], scene["gt3d"], scene["occ"]):
            np.ascontiguousarray(a, np.float64).tofile(f)
        for a in (scene["gt_count"], scene["seq_offset"], off):
            np.ascontiguousarray(a, np.int32).tofile(f)
        p2.tofile(f)
        p3.tofile(f)


def read_rows_bin(path, F, G, S, acc_doubles=590):
    """The output of tests/c/mupots_main.cpp -> match, considered, err, rootz, acc."""
    with open(path, "rb") as f:
        match = np.fromfile(f, np.int32, F * G).reshape(F, G)
        considered = np.fromfile(f, np.int32, F * G).reshape(F, G)
        err = np.fromfile(f, np.float64, F * G * NJ).reshape(F, G, NJ)
        rootz = np.fromfile(f, np.float64, F * G * 2).reshape(F, G, 2)
        acc = np.fromfile(f, np.float64, S * acc_doubles).reshape(S, acc_doubles)
        assert f.read() == b""
    return match, considered, err, rootz, acc


def rows_arrays(rows, F, G):
    """mupots_restate.score's rows -> the arrays the device writes (zero beyond a frame's persons)."""
    match, considered = np.zeros((F, G), np.int32), np.zeros((F, G), np.int32)
    err, rootz = np.zeros((F, G, NJ)), np.zeros((F, G, 2))
    for f, frame in enumerate(rows):
        for g, (m, c, e, z) in enumerate(frame):
            match[f, g], considered[f, g], err[f, g], rootz[f, g] = m, c, e, z
    return match, considered, err, rootz


def same_bits(a, b):
    """Equal bit patterns, or NaN in both, element for element."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def write_root(root, scene, sequences=(1, 2, 3), invalid_first=True):
    """The scene's ground truth in the MuPoTS layout: TS<k>/annot.mat {annotations: frames x persons cell of structs (annot2 [2,17],
    annot3 [3,17], univ_annot3 [3,17], isValidFrame)} and TS<k>/occlusion.mat {occlusion_labels: the same cell of [1,17]}.  Invalid
    persons (isValidFrame 0, with junk) are put in front of the valid ones in odd frames and behind them everywhere."""
    import scipy.io as scio
    rng = np.random.default_rng(9)
    f = 0
    for k, n in zip(sequences, SEQ_FRAMES):
        counts = scene["gt_count"][f:f + n]
        K = int(counts.max()) + 2
        ann, occ = np.empty((n, K), dtype=object), np.empty((n, K), dtype=object)
        for i in range(n):
            lead = 1 if (invalid_first and i % 2 == 1) else 0
            for p in range(K):
                g = p - lead
                valid = 0 <= g < counts[i]
                a2, u3, o = rng.normal(500, 100, (2, 17)), rng.normal(0, 1000, (3, 17)), (rng.random((1, 17)) < 0.5).astype(np.float64)
                if valid:
                    a2[:, :NJ], u3[:, :NJ], o[0, :NJ] = scene["gt2d"][f + i, g].T, scene["gt3d"][f + i, g].T, scene["occ"][f + i, g]
                ann[i, p] = {"annot2": a2, "annot3": u3 * 0.9, "univ_annot3": u3, "isValidFrame": float(valid)}
                occ[i, p] = o
        os.makedirs(os.path.join(root, "TS%d" % k), exist_ok=True)
        scio.savemat(os.path.join(root, "TS%d" % k, "annot.mat"), {"annotations": ann})
        scio.savemat(os.path.join(root, "TS%d" % k, "occlusion.mat"), {"occlusion_labels": occ})
        f += n
