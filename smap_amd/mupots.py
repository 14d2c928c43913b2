"""MuPoTS-3D scoring on the GPU: 3DPCK (root-relative or absolute), AUC, MPJPE and the ordinal rate of root depths.

Reference: lib/eval/mupots_smap.m with the helpers under lib/eval/util_smap/ -- the MATLAB step behind lib/eval/convert.py.  The
per-frame work (greedy 2D matching, bone-length mapping, per-joint errors) and the ordered per-sequence sums run in the HIP kernels of
csrc/mupots.hip, in float64 without contraction; the tables are built here from the per-sequence accumulators (error sums and integer
counts) with sequential Python sums, in the .m files' order of operations.

    ann = load_annotations("MultiPersonTestSet")            # TS<k>/annot.mat + TS<k>/occlusion.mat
    pose3d, pose2d, _ = lib.eval.convert.convert_records(result["3d_pairs"])
    res = MuPoTSScorer(ann, device="cuda:0").score(pose2d, pose3d)
    res.summary(); res.write_csv("eval_result")

What is NOT claimed: bit equality with MATLAB itself.  MATLAB specifies neither its `norm` nor the association of `sum` / `mean`; this
module fixes both (sqrt((x*x + y*y) + z*z); persons, joints, thresholds and sequences in index order).  DESIGN.md has the bound.

A frame's predictions are looked up as `TS<k>/img_<i:06d>` (i counts from 0, mupots_smap.m:119-120) whatever the key's extension.
"""
import csv
import ctypes as C
import os
import re

import numpy as np

NJ, MAXG, MAXP, NT = 15, 16, 127, 31                    # SMAP_MUPOTS_MAXG, SMAP_MUPOTS_MAXP; thresholds 0:5:150
ACC_DOUBLES = 590                                       # SMAP_MUPOTS_ACC_DOUBLES
F_CONSIDERED, F_ANNOTATED, F_UNDETECTED, F_ORD_CORRECT, F_ORD_TOTAL, F_JOINT, JOINT_W, F_MASK, MASK_W = 0, 1, 2, 3, 4, 5, 33, 500, 3
JOINT_NAMES = ("head_top", "neck", "right_shoulder", "right_elbow", "right_wrist", "left_shoulder", "left_elbow", "left_wrist",
               "right_hip", "right_knee", "right_ankle", "left_hip", "left_knee", "left_ankle", "pelvis")
# mpii_get_pck_auc_joint_groups.m, 1-based as written there
JOINT_GROUPS = (("Head", (1,)), ("Neck", (2,)), ("Shou", (3, 6)), ("Elbow", (4, 7)), ("Wrist", (5, 8)), ("Hip", (9, 12)),
                ("Knee", (10, 13)), ("Ankle", (11, 14)))
EVAL_JOINTS = tuple(range(1, 15))                       # mupots_smap.m:99
_NAN = float("nan")


class Annotations:
    """The ground truth of S sequences, packed for the device: frames of all sequences one after the other.

    sequences [S] ints (the k of TS<k>), seq_offset [S+1], gt_count [F] int32 = valid persons of the frame, gt2d [F,G,15,2],
    gt3d [F,G,15,3] (univ_annot3), occ [F,G,15] float64, G = the largest count (at least 1)."""

    def __init__(self, sequences, seq_offset, gt_count, gt2d, gt3d, occ):
        self.sequences = [int(s) for s in sequences]
        self.seq_offset = np.ascontiguousarray(seq_offset, np.int32)
        self.gt_count = np.ascontiguousarray(gt_count, np.int32)
        self.gt2d = np.ascontiguousarray(gt2d, np.float64)
        self.gt3d = np.ascontiguousarray(gt3d, np.float64)
        self.occ = np.ascontiguousarray(occ, np.float64)
        F, G = self.gt_count.shape[0], self.gt2d.shape[1] if self.gt2d.ndim == 4 else 0
        if self.gt2d.shape != (F, G, NJ, 2) or self.gt3d.shape != (F, G, NJ, 3) or self.occ.shape != (F, G, NJ) or F < 1 or G < 1:
            raise ValueError("annotations: gt2d [F,G,15,2], gt3d [F,G,15,3], occ [F,G,15] and gt_count [F] with F, G >= 1")
        if self.seq_offset.shape != (len(self.sequences) + 1,) or self.seq_offset[0] != 0 or self.seq_offset[-1] != F or \
                (np.diff(self.seq_offset) < 0).any():
            raise ValueError("annotations: seq_offset must run from 0 to the number of frames")
        if (self.gt_count < 0).any() or (self.gt_count > G).any():
            raise ValueError("annotations: gt_count outside 0..G")

    @property
    def frames(self):
        return int(self.gt_count.shape[0])

    def frame_names(self):
        """`TS<k>/img_<i:06d>` of every frame, the key its predictions are looked up by."""
        return [frame_key(k, i) for s, k in enumerate(self.sequences) for i in range(int(self.seq_offset[s + 1] - self.seq_offset[s]))]


def frame_key(sequence, index):
    return "TS%d/img_%06d" % (sequence, index)


def pack_persons(sequences, frames_of):
    """sequences: the ids; frames_of(k) -> per frame a list of VALID persons (annot2 [2,>=15], univ_annot3 [3,>=15], occlusion [>=15]) in
    annotation order -> Annotations.  More than 16 valid persons in a frame: ValueError naming the frame."""
    per_seq = [list(frames_of(k)) for k in sequences]
    counts = [len(fr) for frs in per_seq for fr in frs]
    for k, frs in zip(sequences, per_seq):
        for i, fr in enumerate(frs):
            if len(fr) > MAXG:
                raise ValueError(f"{frame_key(k, i)}: {len(fr)} valid persons, at most {MAXG} are scored per frame")
    F, G = len(counts), max(1, max(counts, default=1))
    if F < 1:
        raise ValueError("annotations without frames")
    gt2d, gt3d, occ = np.zeros((F, G, NJ, 2)), np.zeros((F, G, NJ, 3)), np.zeros((F, G, NJ))
    f = 0
    offsets = [0]
    for frs in per_seq:
        for fr in frs:
            for g, (a2, u3, oc) in enumerate(fr):
                gt2d[f, g] = np.asarray(a2, np.float64)[:, :NJ].T                       # mupots_smap.m:53,104
                gt3d[f, g] = np.asarray(u3, np.float64)[:, :NJ].T                       # :55,105
                occ[f, g] = np.asarray(oc, np.float64).reshape(-1)[:NJ]                 # :60,107
            f += 1
        offsets.append(f)
    return Annotations(sequences, offsets, counts, gt2d, gt3d, occ)


def _field(cell, name):
    v = cell[name]
    while isinstance(v, np.ndarray) and v.dtype == object:
        v = v.reshape(-1)[0]
    return np.asarray(v)


def load_annotations(root, sequences=None):
    """TS<k>/annot.mat (`annotations`, a frames x persons cell of structs with annot2 [2,17], univ_annot3 [3,17], isValidFrame) and
    TS<k>/occlusion.mat (`occlusion_labels`, the same cell of [1,17]) of every sequence -> Annotations.  17 columns are cut to 15, invalid
    persons are dropped, the order is kept (mupots_smap.m:49-62,80-111).  sequences: the k to read; default: every TS<k> under root."""
    import scipy.io as scio
    if not os.path.isdir(root):
        raise ValueError(f"{root}: no such directory")
    if sequences is None:
        sequences = sorted(int(m.group(1)) for m in (re.fullmatch(r"TS(\d+)", d) for d in os.listdir(root))
                           if m and os.path.exists(os.path.join(root, m.group(0), "annot.mat")))
    sequences = [int(k) for k in sequences]
    if not sequences:
        raise ValueError(f"{root}: no TS<k>/annot.mat found")

    def frames_of(k):
        base = os.path.join(root, "TS%d" % k)
        try:
            ann = scio.loadmat(os.path.join(base, "annot.mat"))["annotations"]
            occ = scio.loadmat(os.path.join(base, "occlusion.mat"))["occlusion_labels"]
        except (OSError, KeyError) as exc:
            raise ValueError(f"{base}: cannot read annot.mat / occlusion.mat ({exc})")
        if ann.ndim != 2 or occ.shape != ann.shape:
            raise ValueError(f"{base}: annotations {ann.shape} and occlusion_labels {occ.shape} must be the same frames x persons cell")
        for i in range(ann.shape[0]):
            frame = []
            for p in range(ann.shape[1]):
                cell = ann[i, p]
                if float(_field(cell, "isValidFrame").reshape(-1)[0]) != 0:
                    frame.append((_field(cell, "annot2"), _field(cell, "univ_annot3"), np.asarray(occ[i, p])))
            yield frame

    return pack_persons(sequences, frames_of)


def _stem_keys(d):
    return {os.path.splitext(str(k))[0]: v for k, v in d.items() if not str(k).startswith("__")}


def pack_predictions(ann, pose2d, pose3d, missing="error"):
    """The dicts of lib.eval.convert.convert_records ({image: [P,15,>=2] px}, {image: [P,15,>=3] mm}, SMAP joint order) -> pred2d
    [sumP,15,2], pred3d [sumP,15,4], pred_offset [F+1] in the annotations' frame order.  ValueError naming the frame: a frame with valid
    persons that has no predictions entry (unless missing="empty": it then counts as no predictions; the MATLAB script would stop there),
    more than 127 predictions."""
    if missing not in ("error", "empty"):
        raise ValueError('missing must be "error" or "empty"')
    p2s, p3s = _stem_keys(pose2d), _stem_keys(pose3d)
    rows2, rows3, offsets = [], [], [0]
    for f, name in enumerate(ann.frame_names()):
        n = 0
        if ann.gt_count[f] > 0:                                                        # a frame without valid persons is never looked up (:88-90)
            if name not in p2s or name not in p3s:
                if missing == "error":
                    raise ValueError(f"{name}: the annotations have this frame, the predictions do not (missing=\"empty\" scores it as no prediction)")
            else:
                a2, a3 = np.asarray(p2s[name], np.float64), np.asarray(p3s[name], np.float64)
                if a2.size == 0 and a3.size == 0:
                    a2, a3 = np.zeros((0, NJ, 2)), np.zeros((0, NJ, 3))
                if a2.ndim != 3 or a3.ndim != 3 or a2.shape[1] != NJ or a3.shape[1] != NJ or a2.shape[2] < 2 or a3.shape[2] < 3 or len(a2) != len(a3):
                    raise ValueError(f"{name}: predictions must be [P,15,>=2] pixels and [P,15,>=3] millimetres, got {a2.shape} and {a3.shape}")
                if len(a2) > MAXP:
                    raise ValueError(f"{name}: {len(a2)} predictions, at most {MAXP} are matched per frame")
                n = len(a2)
                rows2.append(a2[:, :, :2])
                p4 = np.zeros((n, NJ, 4))
                p4[:, :, :3] = a3[:, :, :3]
                rows3.append(p4)
        offsets.append(offsets[-1] + n)
    pred2d = np.concatenate(rows2) if rows2 else np.zeros((0, NJ, 2))
    pred3d = np.concatenate(rows3) if rows3 else np.zeros((0, NJ, 4))
    return np.ascontiguousarray(pred2d), np.ascontiguousarray(pred3d), np.asarray(offsets, np.int32)


def _div(a, b):
    """MATLAB's a / b: x / 0 = +-Inf, 0 / 0 = NaN."""
    a, b = float(a), float(b)
    if b == 0.0:
        return _NAN if (a != a or a == 0.0) else float(np.copysign(np.inf, a) * np.copysign(1.0, b))
    return a / b


def _seq_sum(values):
    s = 0.0
    for v in values:
        s = s + v
    return s


def tables_from_acc(acc):
    """[S, 590] per-sequence accumulators -> the tables, with the .m files' order of operations and sequential sums:
    mpjpe [S][15] (joints 1..14, Average), pck / auc [S][9] (8 joint groups, Total)      mpii_evaluate_multiperson_errors.m, mpii_compute_3d_pck.m
    visible / occluded {mpjpe [S][16], pck [S][16]}                                     mpii_evaluate_multiperson_errors_visibility_mask.m
    PCK15 [15], ordinal_rate [S], mean_ordinal_rate, total_ordinal / undetected / annotated / considered [S]   mupots_smap.m:224-256"""
    acc = np.asarray(acc, np.float64).reshape(-1, ACC_DOUBLES)
    out = {"mpjpe": [], "pck": [], "auc": [], "visible": {"mpjpe": [], "pck": []}, "occluded": {"mpjpe": [], "pck": []},
           "ordinal_rate": [], "total_ordinal": [], "undetected": [], "annotated": [], "considered": []}
    for a in acc.tolist():
        nf = a[F_CONSIDERED]
        jf = lambda j, k: a[F_JOINT + JOINT_W * (j - 1) + k]                                 # j 1-based
        mpjpe = [_div(jf(j, 0), nf) for j in EVAL_JOINTS]                                    # ...errors.m:27
        out["mpjpe"].append(mpjpe + [_seq_sum(mpjpe) / len(mpjpe)])                          # :29
        pck_row, auc_row, pck_total, curve_total, joint_count = [], [], None, None, 0
        for _, joints in JOINT_GROUPS:                                                       # mpii_compute_3d_pck.m:27-46
            n = len(joints)
            curve = [_div(_seq_sum(jf(j, 1 + t) for j in joints), n * nf) for t in range(NT)]     # :30
            joint_count += n
            curve_total = [c * n for c in curve] if curve_total is None else [x + c * n for x, c in zip(curve_total, curve)]
            auc_row.append(100 * _seq_sum(curve) / NT)                                       # :39
            pck = _div(100 * _seq_sum(jf(j, NT) for j in joints), n * nf)                    # :40, < 150 = the last threshold
            pck_row.append(pck)
            pck_total = pck * n if pck_total is None else pck_total + pck * n
        pck_row.append(pck_total / joint_count)                                              # :47
        auc_row.append(100 * _seq_sum(c / joint_count for c in curve_total) / NT)            # :48-49
        out["pck"].append(pck_row)
        out["auc"].append(auc_row)
        for m, name in enumerate(("visible", "occluded")):                                   # ..._visibility_mask.m:18-23
            mf = lambda j, k: a[F_MASK + NJ * MASK_W * m + MASK_W * (j - 1) + k]
            mp = [mf(j, 1) / (mf(j, 0) + 0.0000000000000000000000000001) for j in EVAL_JOINTS]
            pk = [1 - mf(j, 2) / (mf(j, 0) + 0.0000000000000000000000001) for j in EVAL_JOINTS]
            s_mask = _seq_sum(mf(j, 0) for j in EVAL_JOINTS)
            mp.append(_div(_seq_sum(mf(j, 1) for j in EVAL_JOINTS), s_mask))
            pk.append(1 - _div(_seq_sum(mf(j, 2) for j in EVAL_JOINTS), s_mask))
            out[name]["mpjpe"].append(mp + [0.0])
            out[name]["pck"].append(pk + [s_mask])
        out["ordinal_rate"].append(_div(a[F_ORD_CORRECT], a[F_ORD_TOTAL]))                   # mupots_smap.m:229
        for key, f in (("total_ordinal", F_ORD_TOTAL), ("undetected", F_UNDETECTED), ("annotated", F_ANNOTATED), ("considered", F_CONSIDERED)):
            out[key].append(a[f])
    out["mean_ordinal_rate"] = _div(_seq_sum(out["ordinal_rate"]), len(out["ordinal_rate"]))    # :232
    count = _seq_sum(a[F_CONSIDERED] for a in acc.tolist())
    out["PCK15"] = [_div(_seq_sum(a[F_JOINT + JOINT_W * j + 1 + NT] for a in acc.tolist()), count) for j in range(NJ)]     # :245-256
    return out


class MuPoTSResult:
    """rows: match [F,G] (index of the matched prediction inside its frame, -1 = none), considered [F,G], errors [F,G,15] (what
    mupots_smap.m saves as sequencewise_per_joint_error, for g < gt_count[f] where considered), rootz [F,G,2]; acc [S,590]; tables."""

    def __init__(self, ann, matched_only, match, considered, errors, rootz, acc):
        self.annotations, self.matched_only = ann, bool(matched_only)
        self.match, self.considered, self.errors, self.rootz, self.acc = match, considered, errors, rootz, acc
        self.tables = tables_from_acc(acc)

    def sequence_errors(self, s):
        """[15, n] errors of sequence s: one column per considered person, frames then persons in order (per_joint_error)."""
        f0, f1 = int(self.annotations.seq_offset[s]), int(self.annotations.seq_offset[s + 1])
        cols = [self.errors[f, g] for f in range(f0, f1) for g in range(int(self.annotations.gt_count[f])) if self.considered[f, g]]
        return np.stack(cols, 1) if cols else np.zeros((NJ, 0))

    def summary(self):
        """What a checkpoint is compared by, JSON-able: the Total 3DPCK and AUC and the average MPJPE per sequence and their means over
        the sequences, PCK15, the ordinal rates, the person counts."""
        t = self.tables
        mean = lambda v: _div(_seq_sum(v), len(v))
        return {"mode": "only_matched_annotations" if self.matched_only else "all_annotated",
                "sequences": list(self.annotations.sequences),
                "pck": [r[-1] for r in t["pck"]], "auc": [r[-1] for r in t["auc"]], "mpjpe": [r[-1] for r in t["mpjpe"]],
                "mean_pck": mean([r[-1] for r in t["pck"]]), "mean_auc": mean([r[-1] for r in t["auc"]]),
                "mean_mpjpe": mean([r[-1] for r in t["mpjpe"]]),
                "PCK15": list(t["PCK15"]), "ordinal_rate": list(t["ordinal_rate"]), "mean_ordinal_rate": t["mean_ordinal_rate"],
                "total_ordinal": [int(v) for v in t["total_ordinal"]], "undetected": [int(v) for v in t["undetected"]],
                "annotated": [int(v) for v in t["annotated"]], "considered": [int(v) for v in t["considered"]]}

    def write_csv(self, out_dir):
        """The three tables under the reference's file names (mupots_smap.m:234-269).  The cell layout is the .m files'; the number
        formatting is Python's repr, not writetable's."""
        os.makedirs(out_dir, exist_ok=True)
        prefix = "only_matched_annotations_" if self.matched_only else "all_annotated_"
        t, names = self.tables, ["TestSeq%d" % (i + 1) for i in range(len(self.tables["mpjpe"]))]
        groups = [g for g, _ in JOINT_GROUPS] + ["Total"]
        rows = [[""] + [JOINT_NAMES[j - 1] for j in EVAL_JOINTS] + ["Average"]] + [[n] + r for n, r in zip(names, t["mpjpe"])]
        for title, key in (("PCK", "pck"), ("AUC", "auc")):
            rows += [[title] + groups] + [[n] + r for n, r in zip(names, t[key])]
        paths = []

        def write(name, table):
            paths.append(os.path.join(out_dir, name))
            with open(paths[-1], "w", newline="") as f:
                csv.writer(f).writerows([["" if v is None else (repr(v) if isinstance(v, float) else v) for v in r] for r in table])

        write(prefix + "multiperson_3dhp_evaluation_sequencewise.csv", rows)
        for key in ("visible", "occluded"):
            write(prefix + key + "_joints_multiperson_3dhp_evaluation_sequencewise.csv", t[key]["mpjpe"] + t[key]["pck"])
        return paths


class MuPoTSScorer:
    """mupots_smap.m on `device`: relative = is_relative, use_skel = use_skel, matched_only = EVALUATION_MODE 1."""

    def __init__(self, annotations, relative=True, use_skel=True, matched_only=False, device="cuda:0"):
        import torch
        if not isinstance(annotations, Annotations):
            raise ValueError("annotations: what load_annotations returns")
        if annotations.gt2d.shape[1] > MAXG:
            raise ValueError(f"at most {MAXG} valid persons per frame")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("MuPoTSScorer scores on the GPU: device must be a cuda device (there is no host scorer)")
        from . import lib as _L
        self._L, self._lib = _L, _L.load()
        self.annotations = annotations
        self.relative, self.use_skel, self.matched_only = bool(relative), bool(use_skel), bool(matched_only)
        self._gt = None                                            # uploaded by the first launch: refusals need no GPU

    def _uploaded(self):
        import torch
        if self._gt is None:
            self._gt = {k: torch.from_numpy(getattr(self.annotations, k)).to(self.device)
                        for k in ("gt2d", "gt3d", "occ", "gt_count", "seq_offset")}
        return self._gt

    def launch(self, pred2d, pred3d, pred_offset, out=None):
        """The two launches on the current stream, device tensors in and out (pred2d [sumP,15,2], pred3d [sumP,15,4] float64, pred_offset
        [F+1] int32) -> (match, considered, errors, rootz, acc) on the device."""
        import torch
        a, g = self.annotations, self._uploaded()
        F, G, S = a.frames, a.gt2d.shape[1], len(a.sequences)
        sumP = int(pred2d.shape[0])
        if pred2d.dtype != torch.float64 or pred3d.dtype != torch.float64 or tuple(pred2d.shape[1:]) != (NJ, 2) or \
                tuple(pred3d.shape) != (sumP, NJ, 4) or pred_offset.dtype != torch.int32 or tuple(pred_offset.shape) != (F + 1,):
            raise ValueError("pred2d float64 [sumP,15,2], pred3d float64 [sumP,15,4], pred_offset int32 [F+1]")
        if sumP == 0:                                              # the library takes no null pointer: one row nobody owns
            pred2d, pred3d = torch.zeros((1, NJ, 2), dtype=torch.float64, device=self.device), torch.zeros((1, NJ, 4), dtype=torch.float64, device=self.device)
        if out is None:
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)
            out = (z((F, G), torch.int32), z((F, G), torch.int32), z((F, G, NJ), torch.float64), z((F, G, 2), torch.float64),
                   z((S, ACC_DOUBLES), torch.float64))
        match, considered, err, rootz, acc = out
        p = lambda t: C.c_void_p(t.data_ptr())
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            self._L.check(self._lib.smap_mupots_frames(p(g["gt2d"]), p(g["gt3d"]), p(g["gt_count"]), p(pred2d), p(pred3d), p(pred_offset), F, G,
                                                       sumP, int(self.relative), int(self.use_skel), int(self.matched_only), p(match),
                                                       p(considered), p(err), p(rootz), stream), "smap_mupots_frames")
            self._L.check(self._lib.smap_mupots_fold(p(g["seq_offset"]), S, p(g["gt_count"]), F, G, p(match), p(considered), p(err), p(rootz),
                                                     p(g["occ"]), int(self.relative), p(acc), stream), "smap_mupots_fold")
        return out

    def score(self, pose2d, pose3d, missing="error"):
        """The dicts of lib.eval.convert.convert_records -> MuPoTSResult."""
        import torch
        pred2d, pred3d, offsets = pack_predictions(self.annotations, pose2d, pose3d, missing)       # refusals first
        up = lambda a: torch.from_numpy(a).to(self.device)
        out = self.launch(up(pred2d), up(pred3d), up(offsets))
        match, considered, err, rootz, acc = (t.cpu().numpy() for t in out)
        return MuPoTSResult(self.annotations, self.matched_only, match, considered, err, rootz, acc)


def load_pose_mats(pose3d_path, pose2d_path):
    """pose3d.mat / pose2d.mat as lib.eval.convert.convert writes them -> the two dicts (pose2d, pose3d)."""
    import scipy.io as scio

    def read(path, var):
        try:
            m = scio.loadmat(path)
        except (OSError, ValueError) as exc:
            raise ValueError(f"{path}: cannot read ({exc})")
        if var not in m:
            raise ValueError(f"{path}: no `{var}`")
        s = m[var]
        if s.dtype.names is None:
            raise ValueError(f"{path}: `{var}` is not a struct of frames")
        out = {}
        for name in s.dtype.names:
            v = np.asarray(s[name].reshape(-1)[0], np.float64)
            out[name] = v.reshape(-1, NJ, v.shape[-1]) if v.size else np.zeros((0, NJ, 4))
        return out

    return read(pose2d_path, "preds_2d_kpt"), read(pose3d_path, "preds_3d_kpt")
