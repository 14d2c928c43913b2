"""The MuPoTS-3D protocol in plain float64 Python: the yardstick of tests/test_mupots_*.py and tools/bench_mupots.py.

Written from zju3dv/SMAP lib/eval/mupots_smap.m and lib/eval/util_smap/*.m, statement by statement, with explicit expressions: Python
floats are IEEE doubles, every operator rounds once, math.sqrt is correctly rounded, and every sum is a loop in the order stated.
No numpy reduction is used; numpy only carries the data.  Imports nothing of the package under test.

Indices are 1-based in the comments (the .m files) and 0-based in the code.

Where MATLAB leaves an order unspecified (its `norm`, the association of its `sum` / `mean`) this file fixes one:
  norm([x y z]) = sqrt((x*x + y*y) + z*z); sum(A, 3) and mean(A, 3) add the persons in the order they were appended; sums over
  joints, joint groups, thresholds and sequences run in index order.
"""
import math

import numpy as np

NJ = 15
NAN = float("nan")
SMAP_ORDER = [2, 1, 10, 11, 12, 4, 5, 6, 13, 14, 15, 7, 8, 9, 3]              # mupots_smap.m:122-123
O1 = [2, 15, 2, 3, 4, 2, 6, 7, 15, 9, 10, 15, 12, 13, 15]                   # :15-17
TRAVERSAL = [2, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14]                 # safe_traversal_order(2:end), :29,183
MATCHING_JOINTS = list(range(2, 15))                                        # :98
EVAL_JOINTS = list(range(1, 15))                                            # :99
JOINT_NAMES = ["head_top", "neck", "right_shoulder", "right_elbow", "right_wrist", "left_shoulder", "left_elbow", "left_wrist",
               "right_hip", "right_knee", "right_ankle", "left_hip", "left_knee", "left_ankle", "pelvis"]
JOINT_GROUPS = [("Head", [1]), ("Neck", [2]), ("Shou", [3, 6]), ("Elbow", [4, 7]), ("Wrist", [5, 8]), ("Hip", [9, 12]),
                ("Knee", [10, 13]), ("Ankle", [11, 14])]                    # mpii_get_pck_auc_joint_groups.m
THRESH = [5 * t for t in range(31)]                                         # mpii_compute_3d_pck.m:20
ACC = 590                                                                   # include/smap_hip.h SMAP_MUPOTS_ACC_DOUBLES


def div(a, b):
    """MATLAB's a / b on doubles: x / 0 is +-Inf, 0 / 0 and NaN / x are NaN."""
    a, b = float(a), float(b)
    if b == 0.0:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def norm3(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def match_frame(gt2, pred2):
    """mpii_multiperson_get_identity_matching.m with threshold 40.  gt2: per person [15][2]; pred2: per prediction [15][2] in the
    protocol's joint order.  -> matching (0-based prediction index or -1 per ground-truth person)."""
    matched = [False] * len(pred2)
    matching = []
    for g in gt2:
        best, best_score = -1, 0
        for i, p in enumerate(pred2):
            if matched[i]:
                continue                                                     # :9-11 (its score stays 0)
            score = 0
            for j in MATCHING_JOINTS:
                px, py = p[j - 1][0], p[j - 1][1]
                near = abs(g[j - 1][0] - px) < 40 and abs(g[j - 1][1] - py) < 40          # :12-13
                visible = not (px == 0 and py == 0)                                        # mupots_smap.m:143
                if near and visible:
                    score += 1
            if score > best_score:                                           # max(): the FIRST maximum, :17
                best, best_score = i, score
        if best_score > 0:                                                   # :18-21
            matched[best] = True
        matching.append(best if best_score > 0 else -1)
    return matching


def map_bones(pred, gt):
    """mpii_map_to_gt_bone_lengths.m.  pred, gt: [15][3] -> mapped [15][3]."""
    mapped = [list(p) for p in pred]
    for idx in TRAVERSAL:
        i, pa = idx - 1, O1[idx - 1] - 1
        gt_len = norm3([gt[i][c] - gt[pa][c] for c in range(3)])
        v = [pred[i][c] - pred[pa][c] for c in range(3)]
        n = norm3(v)
        v = [div(v[c] * gt_len, n) for c in range(3)]
        mapped[i] = [mapped[pa][c] + v[c] for c in range(3)]
    return mapped


def cal_ordinal(pd1, pd2, gt1, gt2, thres=300):
    """cal_ordinal.m:52-60."""
    if (gt1 - gt2) * (pd1 - pd2) > 0:
        return 1
    if abs(gt1 - gt2) < thres and abs(pd1 - pd2) < thres:
        return 0
    return -1


def score_frame(gt2, gt3, pred2_smap, pred3_smap, relative, use_skel, matched_only):
    """One frame with >= 1 valid person (mupots_smap.m:118-221).  gt2 [G][15][2], gt3 [G][15][3]; pred2_smap [P][15][>=2],
    pred3_smap [P][15][>=3] in SMAP order.  -> per person (match, considered, err[15], (pred root z, gt root z))."""
    order = [k - 1 for k in SMAP_ORDER]
    pred2 = [[[float(p[k][0]), float(p[k][1])] for k in order] for p in pred2_smap]
    pred3 = []
    for p in pred3_smap:
        q = [[float(p[k][0]), float(p[k][1]), float(p[k][2])] for k in order]
        if relative:                                                         # :153-154
            q = [[q[j][c] - q[14][c] for c in range(3)] for j in range(NJ)]
        pred3.append(q)
    matching = match_frame(gt2, pred2)
    rows = []
    for k, g in enumerate(gt3):
        g = [[float(g[j][c]) for c in range(3)] for j in range(NJ)]
        P = [[g[j][c] - g[14][c] for c in range(3)] for j in range(NJ)] if relative else g          # :172-176
        if matching[k] >= 0:
            pred_p = pred3[matching[k]]
            if use_skel:
                pred_p = map_bones(pred_p, P)
            considered = 1
        else:
            pred_p = [[100000.0] * 3 for _ in range(NJ)]                     # :188
            considered = 0 if matched_only else 1
        err = []
        for j in range(NJ):                                                  # :199-200
            dx, dy, dz = pred_p[j][0] - P[j][0], pred_p[j][1] - P[j][1], pred_p[j][2] - P[j][2]
            err.append(math.sqrt(((dx * dx) + (dy * dy)) + (dz * dz)))
        rows.append((matching[k], considered, err, (pred_p[14][2], P[14][2])))
    return rows


def new_acc():
    return [0.0] * ACC


def fold_frame(acc, rows, occ, relative):
    """Add one frame's rows to a sequence's accumulator (list of ACC floats): the counters and sums the tables are built from."""
    acc[1] += len(rows)                                                      # annotated_people, :86
    for match, considered, err, _ in rows:
        if match < 0:
            acc[2] += 1                                                      # undetected_people, :167
    kept = [(r, o) for r, o in zip(rows, occ) if r[1]]
    for (match, considered, err, rz), o in kept:
        acc[0] += 1
        for j in range(NJ):
            e = err[j]
            base = 5 + 33 * j
            acc[base] = acc[base] + e
            for t in range(31):
                if e < THRESH[t]:
                    acc[base + 1 + t] += 1
            if e <= 150:
                acc[base + 32] += 1
            for m in range(2):                                               # 0: visibility = 1 - occlusion (:108), 1: occlusion
                mask = float(o[j]) if m else 1.0 - float(o[j])
                me = (160.0 if e != e else e) * mask                         # ..._visibility_mask.m:15-16
                b = 500 + 45 * m + 3 * j
                acc[b] = acc[b] + mask
                acc[b + 1] = acc[b + 1] + me
                if me > 150:
                    acc[b + 2] += 1
    if not relative:                                                         # :195-198,210-221
        z = [r[3] for r, _ in kept]
        for a in range(len(z) - 1):
            for b in range(a + 1, len(z)):
                if cal_ordinal(z[b][0], z[a][0], z[b][1], z[a][1], 300) >= 0:
                    acc[3] += 1
                acc[4] += 1


def score(seq_offset, gt_count, gt2d, gt3d, occ, preds, relative=True, use_skel=True, matched_only=False):
    """The frames of S sequences: seq_offset [S+1], gt_count [F], gt2d [F,G,15,2], gt3d [F,G,15,3], occ [F,G,15]; preds: per frame
    (pred2 [P,15,>=2], pred3 [P,15,>=3]) in SMAP joint order, or None for a frame without valid persons.
    -> rows: per frame the list score_frame returns ([] for an empty frame); accs: per sequence ACC floats."""
    rows, accs = [], []
    for s in range(len(seq_offset) - 1):
        acc = new_acc()
        for f in range(int(seq_offset[s]), int(seq_offset[s + 1])):
            n = int(gt_count[f])
            if n == 0:                                                       # :88-90
                rows.append([])
                continue
            p2, p3 = preds[f]
            r = score_frame(np.asarray(gt2d[f][:n]).tolist(), np.asarray(gt3d[f][:n]).tolist(), np.asarray(p2).tolist(), np.asarray(p3).tolist(),
                            relative, use_skel, matched_only)
            fold_frame(acc, r, np.asarray(occ[f][:n]).tolist(), relative)
            rows.append(r)
        accs.append(acc)
    return rows, accs


def tables(accs):
    """The tables of mpii_evaluate_multiperson_errors.m / mpii_compute_3d_pck.m (eval_joints = 1:14), the two tables of
    mpii_evaluate_multiperson_errors_visibility_mask.m, PCK15 (mupots_smap.m:245-256) and the ordinal rates (:229,232), from the
    per-sequence accumulators."""
    out = {"mpjpe": [], "pck": [], "auc": [], "visible": {"mpjpe": [], "pck": []}, "occluded": {"mpjpe": [], "pck": []},
           "ordinal_rate": [], "total_ordinal": [], "undetected": [], "annotated": [], "considered": []}
    nt = len(THRESH)
    for acc in accs:
        nf = acc[0]
        mpjpe = [div(acc[5 + 33 * (j - 1)], nf) for j in EVAL_JOINTS]                       # mean(..., 3), ...errors.m:27
        total = 0.0
        for v in mpjpe:
            total = total + v
        out["mpjpe"].append(mpjpe + [total / len(mpjpe)])                                    # mean(mpjpe(:)), :29
        pck_row, auc_row = [], []
        pck_total, curve_total, joint_count = None, None, 0
        for _, joints in JOINT_GROUPS:                                                       # mpii_compute_3d_pck.m:27-46
            n = len(joints)
            curve = []
            for t in range(nt):
                cnt = 0.0
                for j in joints:
                    cnt = cnt + acc[5 + 33 * (j - 1) + 1 + t]
                curve.append(div(cnt, n * nf))                                               # :30
            joint_count += n
            curve_total = [c * n for c in curve] if curve_total is None else [a + c * n for a, c in zip(curve_total, curve)]   # :34-38
            s = 0.0
            for c in curve:
                s = s + c
            auc_row.append(100 * s / nt)                                                     # :39
            cnt = 0.0
            for j in joints:
                cnt = cnt + acc[5 + 33 * (j - 1) + 1 + 30]                                   # < 150 is the last threshold
            pck = div(100 * cnt, n * nf)                                                     # :40
            pck_row.append(pck)
            pck_total = pck * n if pck_total is None else pck_total + pck * n                # :41-45
        pck_row.append(pck_total / joint_count)                                              # :47
        curve_total = [c / joint_count for c in curve_total]                                 # :48
        s = 0.0
        for c in curve_total:
            s = s + c
        auc_row.append(100 * s / nt)                                                         # :49
        out["pck"].append(pck_row)
        out["auc"].append(auc_row)
        for m, name in enumerate(("visible", "occluded")):                                   # ..._visibility_mask.m:18-23
            b = 500 + 45 * m
            mp, pk = [], []
            s_err = s_mask = s_cnt = 0.0
            for j in EVAL_JOINTS:
                jm, me, cnt = acc[b + 3 * (j - 1)], acc[b + 3 * (j - 1) + 1], acc[b + 3 * (j - 1) + 2]
                mp.append(me / (jm + 0.0000000000000000000000000001))
                pk.append(1 - cnt / (jm + 0.0000000000000000000000001))
                s_err, s_mask, s_cnt = s_err + me, s_mask + jm, s_cnt + cnt
            mp.append(div(s_err, s_mask))
            pk.append(1 - div(s_cnt, s_mask))
            out[name]["mpjpe"].append(mp + [0.0])                                            # zeros(., 16): the 16th column stays 0
            out[name]["pck"].append(pk + [s_mask])
        out["ordinal_rate"].append(div(acc[3], acc[4]))                                      # mupots_smap.m:229
        out["total_ordinal"].append(acc[4])
        out["undetected"].append(acc[2])
        out["annotated"].append(acc[1])
        out["considered"].append(acc[0])
    s = 0.0
    for r in out["ordinal_rate"]:
        s = s + r
    out["mean_ordinal_rate"] = div(s, len(accs))                                             # :232
    count = 0.0
    per_joint = [0.0] * NJ
    for acc in accs:                                                                         # :245-256
        for j in range(NJ):
            per_joint[j] = per_joint[j] + acc[5 + 33 * j + 32]
        count = count + acc[0]
    out["PCK15"] = [div(v, count) for v in per_joint]
    return out
