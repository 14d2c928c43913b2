"""MPJPE / PCK / ordinal scoring of `generate_result` runs, on the GPU.

Reference: lib/eval/test_util_panoptic.py -- `eval_3d` (:273-307), `initialization` (:332-355) and the generate_result
branch of `calculate_and_log` (:379-408), which puts an `error` dict into the result file.  The reference scores one
person at a time with ~20 numpy calls on the host; here the persons of a batch are scored by the HIP kernels of
csrc/eval.hip next to the float64 tensors the ground-truth modes already keep on the device (smap_lift_gt /
smap_refine_gt), on the stream the caller is on, and nothing comes back to the host before `raw()` / `summary()`.

The 80 float64 accumulators (include/smap_hip.h, SMAP_EVAL_ACC_DOUBLES) live on the device across `update` calls and are
the reference's running sums bit for bit: every person's terms are added one `+=` per field, frames then persons in
order.

`EvalMaps` scores the network's MAPS the same way -- the `eval` branch of that module: `eval_one_image` (:88-113, head-size-normalised
2D keypoint error and keypoint recall), the `eval` part of `generate_rootZ` (:145-156, per limb |sampled relative depth - annotated
relative depth| and a count of sign reversals) and the `eval` branch of `calculate_and_log` (:359-378).  Its 87 float64
(SMAP_EVALMAPS_ACC_DOUBLES) are fed by `lift_batch(..., gt_mode=True, bones=True)`: the per-limb depth exists only inside the lifting
kernel.  Those two functions sum a frame's persons into a zero vector first and add that to the running total; the device fold
associates the same way, so the six counters and `distance_d` are the reference's bit for bit.  `distance_e` is not: the reference's
`distance()` squares and roots with `**`, i.e. libm `pow`, which differs from multiply / correctly rounded `sqrt` in the last place
for ~1 % of inputs (DESIGN section 10 has the bound).  Limb 0 is (0, 1) = cfg.DATASET.PAF.VECTOR, the table the lifting samples with;
the panoptic module's own table has (1, 0) there.  Annotation depths are subtracted in float64 as they stand, where the reference,
handed a float32 annotation array, would subtract in fp32.  The MuPoTS-3D protocol (lib/eval/mupots_smap.m: 3DPCK, AUC, MPJPE,
ordinal rate) is scored by smap_amd/mupots.py; `--mupots ROOT` below runs it.

    python -m smap_amd.evaluate RESULT.json [--refine 0|1] [--maps 0|1] [--device cuda:0]
    python -m smap_amd.evaluate RESULT.json --mupots ROOT [--relative 0|1] [--matched_only 0|1] [--use_skel 0|1] [--out DIR]
    python -m smap_amd.evaluate --pose3d pose3d.mat --pose2d pose2d.mat --mupots ROOT ...

scores an existing result file -- this project's or one written by the reference's test.py -- and prints the summary as
JSON.  Annotations are fp32 (dataset/base_dataset.py), so a file holds exactly the ground truth the run saw; where the
reference is handed a float32 annotation array it subtracts the ground-truth root in fp32, here every operation is float64
on the values as they stand in the file."""
import ctypes as C
import json
import sys

import numpy as np
import torch

from . import lib as _L

NJ, MAXP, MAXG = 15, 127, 64
ACC_DOUBLES = TERM_DOUBLES = 80
VECTORS = ("real_error", "root_error", "count_point", "real_PCK", "root_PCK")                       # 15 doubles each, in this order
SCALARS = ("count_people", "total_people_gt", "total_pair_count", "reverse_pair_count", "less_15")  # then these five
_INT_SCALARS = ("count_people", "total_people_gt")                                                  # Python ints in the reference
PAIR_COUNT_0 = 1e-8                                                                                  # initialization, :351
# the order of the reference's error dict (initialization :346-355)
_KEY_ORDER = ("real_error", "root_error", "count_people", "total_people_gt", "count_point", "total_pair_count", "reverse_pair_count",
              "less_15", "root_PCK", "real_PCK")


def _key(name, refine):
    """`initialization` (:333-336): every key but total_people_gt carries `_after_refine` when RefineNet ran."""
    return name if name == "total_people_gt" or not refine else name + "_after_refine"


def unpack(acc, refine=False):
    """[80] float64 in accumulator order -> the reference's error dict before the final divisions (its keys, order and types)."""
    acc = np.asarray(acc, np.float64).reshape(ACC_DOUBLES)
    vals = {k: acc[15 * i:15 * i + 15].copy() for i, k in enumerate(VECTORS)}
    for i, k in enumerate(SCALARS):
        v = acc[75 + i]
        vals[k] = int(v) if k in _INT_SCALARS else float(v)
    return {_key(k, refine): vals[k] for k in _KEY_ORDER}


def pack(raw, refine=False):
    """The inverse of `unpack`."""
    return np.concatenate([np.asarray(raw[_key(k, refine)], np.float64).reshape(15) for k in VECTORS] +
                          [np.asarray([float(raw[_key(k, refine)]) for k in SCALARS], np.float64)])


def _is_refine(raw):
    return "count_people_after_refine" in raw


def summarize(raw):
    """The generate_result branch of calculate_and_log (:384-387,402-406) on a `raw()` dict: real_error and root_error divided by
    count_point, the two PCK vectors by count_people, arrays as lists.  A zero divisor gives nan / inf, as numpy's division does."""
    refine = _is_refine(raw)
    k = lambda name: _key(name, refine)
    out = {key: (v.copy() if isinstance(v, np.ndarray) else v) for key, v in raw.items()}
    with np.errstate(divide="ignore", invalid="ignore"):
        out[k("real_error")] = out[k("real_error")] / out[k("count_point")]
        out[k("root_error")] = out[k("root_error")] / out[k("count_point")]
        out[k("root_PCK")] = out[k("root_PCK")] / np.float64(out[k("count_people")])
        out[k("real_PCK")] = out[k("real_PCK")] / np.float64(out[k("count_people")])
    for name in VECTORS:
        out[k(name)] = out[k(name)].tolist()
    return out


def log_values(raw):
    """What the last four log lines of calculate_and_log print (:392-400): recall of points [15], reverse rate, less-than-15 rate,
    person recall.  numpy division: a zero divisor gives nan / inf where the reference's Python scalars would raise."""
    refine = _is_refine(raw)
    k = lambda name: np.asarray(raw[_key(name, refine)], np.float64)[()]          # ndarray stays, int / float -> np.float64
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"point_recall": k("count_point") / k("count_people"), "reverse_rate": k("reverse_pair_count") / k("total_pair_count"),
                "less_15_rate": k("less_15") / k("total_people_gt"), "people_recall": k("count_people") / k("total_people_gt")}


def log_lines(raw):
    """The six log lines of calculate_and_log's generate_result branch (:388-400), same wording."""
    refine = _is_refine(raw)
    s, v = summarize(raw), log_values(raw)
    k = lambda name: _key(name, refine)
    a = lambda name: np.asarray(s[k(name)])
    return ["Real error is {}, root error is {}".format(a("real_error"), a("root_error")),
            "Real PCK_25 is {}, root PCK_15 is {}. ".format(a("real_PCK"), a("root_PCK")),
            "Recall of points is {}".format(v["point_recall"]),
            "Reverse rate is {}".format(v["reverse_rate"]),
            "Less than 25 rate is {}".format(v["less_15_rate"]),
            "find {} people, total is {}, recall is {}".format(raw[k("count_people")], raw["total_people_gt"], v["people_recall"])]


def merge(raws):
    """Per-rank `raw()` dicts, in rank order -> the accumulators of the whole run.

    The counters (count_point, the PCK sums, the people / pair / less_15 counts) are sums of ones: exact in any order.
    total_pair_count is replayed as the one-rank run would have built it: 1e-8, then one `+= 1` per counted pair.
    real_error and root_error are float64 sums of non-negative terms that a one-rank run adds person by person; adding
    per-rank subtotals re-associates them.  Each of the two sums is within (n - 1) * 2^-53 of the exact value, relatively, so
    they differ from each other by at most n * 2^-52 relative, n = the number of terms (count_point of that joint).  Derived,
    not measured; tests/test_eval_cpu.py asserts it."""
    raws = list(raws)
    if not raws:
        raise ValueError("merge() needs at least one accumulator")
    refine = _is_refine(raws[0])
    if any(_is_refine(r) != refine for r in raws):
        raise ValueError("merge(): accumulators with and without RefineNet keys")
    acc = np.zeros(ACC_DOUBLES)
    pairs = 0
    for r in raws:                                              # rank order
        p = pack(r, refine)
        pairs += int(round(p[77] - PAIR_COUNT_0))
        p[77] = 0.0
        acc = acc + p
    acc[77] = np.cumsum(np.concatenate([[PAIR_COUNT_0], np.ones(pairs)]))[-1]     # sequential: ((1e-8 + 1) + 1) + ...
    return unpack(acc, refine)


# ---- the maps' scores: eval_one_image + generate_rootZ('eval') + calculate_and_log('eval') ----
NL = 14
MAPS_ACC_DOUBLES = MAPS_TERM_DOUBLES = 87
# (key, length, integer in the reference) in accumulator order == the order of `initialization` (:338-343)
MAPS_FIELDS = (("count_gt", NJ, True), ("count_pred", NJ, True), ("distance_e", NJ, False),
               ("distance_d", NL, False), ("reverse_count", NL, False), ("count_pred_bone", NL, True))
MAPS_KEYS = tuple(k for k, _, _ in MAPS_FIELDS)
MAPS_2D_KEYS = MAPS_KEYS[:3]


def unpack_maps(acc):
    """[87] float64 in accumulator order -> the six `eval` keys of the reference's error dict with its dtypes: int64 arrays for
    count_gt, count_pred and count_pred_bone, float64 for distance_e, distance_d and reverse_count."""
    acc = np.asarray(acc, np.float64).reshape(MAPS_ACC_DOUBLES)
    out, o = {}, 0
    for key, n, is_int in MAPS_FIELDS:
        out[key] = acc[o:o + n].astype(np.int64) if is_int else acc[o:o + n].copy()
        o += n
    return out


def pack_maps(raw):
    """The inverse of `unpack_maps`."""
    return np.concatenate([np.asarray(raw[key], np.float64).reshape(n) for key, n, _ in MAPS_FIELDS])


def summarize_maps(raw):
    """The `eval` branch of calculate_and_log (:360-372) on a `raw()` dict: error_point = distance_e / count_pred, recall =
    count_pred / count_gt, depth_e and depth_reverse_count over count_pred_bone, each where the divisor is > 0 and 0 elsewhere;
    avg_error / avg_recall = np.average over the entries with a divisor (nan when there is none, as np.average of nothing is)."""
    c_gt, c_pred, c_bone = (np.asarray(raw[k]) for k in ("count_gt", "count_pred", "count_pred_bone"))
    d_e, d_d, rev = (np.asarray(raw[k], np.float64) for k in ("distance_e", "distance_d", "reverse_count"))
    error_point, recall = np.zeros(NJ), np.zeros(NJ)
    depth_e, depth_reverse_count = np.zeros(NL), np.zeros(NL)
    mask, mask_bone = c_pred > 0, c_bone > 0
    error_point[mask] = d_e[mask] / c_pred[mask]
    depth_e[mask_bone] = d_d[mask_bone] / c_bone[mask_bone]
    depth_reverse_count[mask_bone] = rev[mask_bone] / c_bone[mask_bone]
    avg_error = np.average(error_point[mask]) if mask.any() else np.float64("nan")
    mask = c_gt > 0
    recall[mask] = c_pred[mask] / c_gt[mask]
    avg_recall = np.average(recall[mask]) if mask.any() else np.float64("nan")
    return {"error_point": error_point, "recall": recall, "depth_e": depth_e, "depth_reverse_count": depth_reverse_count,
            "avg_error": avg_error, "avg_recall": avg_recall}


def log_lines_maps(raw):
    """The five result lines of calculate_and_log's `eval` branch (:374-378), same wording."""
    s = summarize_maps(raw)
    return ["keypoints error of validation dataset is {}".format(s["error_point"]),
            "Keypoints recall of validation dataset is {}".format(s["recall"]),
            "Bones depth distance is {}".format(s["depth_e"]),
            "Bones reverse count is {}".format(s["depth_reverse_count"]),
            "Average error is {}, average recall is {}".format(s["avg_error"], s["avg_recall"])]


def merge_maps(raws):
    """Per-rank `EvalMaps.raw()` dicts, in rank order -> the accumulators of the whole run.

    The four counters are sums of ones: exact in any order.  distance_e and distance_d are float64 sums of non-negative terms; a
    one-rank run adds one per-frame partial after the other, here per-rank subtotals are added, which re-associates them at the rank
    boundaries.  As in `merge`: each way of summing n non-negative terms is within (n - 1) * 2^-53 of the exact sum, relatively, so
    the two differ by at most n * 2^-52 relative, n = count_pred (count_pred_bone) of that field.  tests/test_eval_maps_cpu.py."""
    raws = list(raws)
    if not raws:
        raise ValueError("merge_maps() needs at least one accumulator")
    acc = np.zeros(MAPS_ACC_DOUBLES)
    for r in raws:                                              # rank order; the counters are integers in float64: exact below 2^53
        acc = acc + pack_maps(r)
    return unpack_maps(acc)


def _padded(annotations, gmax, columns):
    """B arrays [G_i,15,C] -> ([B,G,15,4] float64 = columns(a), row for row, zero padded; counts [B])."""
    rows = [np.asarray(a, np.float64) for a in annotations]
    rows = [a if a.size else np.zeros((0, NJ, 4)) for a in rows]                 # an empty list arrives as a 1-D array
    G = max(1, max((len(a) for a in rows), default=1)) if gmax is None else int(gmax)
    if G > MAXG or any(len(a) > G for a in rows):
        raise ValueError("at most %d annotations per frame" % MAXG)
    gt = np.zeros((len(rows), G, NJ, 4), np.float64)
    for i, a in enumerate(rows):
        if len(a):
            gt[i, :len(a)] = columns(a)
    return gt, np.asarray([len(a) for a in rows], np.int32)


def gt2d_rows(annotations, gmax=None):
    """B arrays [G_i,15,>=4] of KEPT annotations -> gt_2d [B,G,15,4] float64 = columns 0:4 (x, y, Z, score: network pixels and the
    annotated depth), row for row, zero padded."""
    return _padded(annotations, gmax, lambda a: a[:, :, 0:4])[0]


def gt_rows(annotations, gmax=None):
    """B annotation arrays [G_i,15,>=7] -> (gt [B,G,15,4] float64 = (X,Y,Z,score) = columns 4:7 and 3, row for row, zero padded;
    counts [B]).  No row is dropped: row g stays the annotation the registration kernel calls g."""
    return _padded(annotations, gmax, lambda a: a[:, :, (4, 5, 6, 3)])


def _kept(annotations, root_idx):
    """The pipeline's filter (records.kept_annotations, test.py:76-80) on each frame: the annotations whose root score is > 1."""
    from .records import kept_annotations
    rows = [np.asarray(a, np.float64) for a in annotations]
    return [kept_annotations(a, root_idx) if a.size else a for a in rows]


def gt_from_annotations(annotations, root_idx=2):
    """gt_rows of the annotations whose root score is > 1 -- the pipeline's filter (records.kept_annotations, test.py:76-80)."""
    return gt_rows(_kept(annotations, root_idx))


def _check_tensors(named):
    """Every (name, t): a contiguous torch.Tensor on a GPU, or ValueError."""
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch.Tensor")
        if not t.is_cuda:
            raise ValueError(f"{name} must live on the GPU (there is no host scorer)")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")


def _check_one_device(named):
    if len({t.device for _, t in named}) != 1:
        names = [name for name, _ in named]
        raise ValueError("%s and %s must be on one device" % (", ".join(names[:-1]), names[-1]))


_PRED_SHAPE, _GT_SHAPE = f"float64 [B,{MAXP},{NJ},4]", f"float64 [B,G,{NJ},4] with 1 <= G <= {MAXG}"


def _need(ok, name, t, what):
    """`ok` -- t has the dtype and the shape -- or ValueError: name must be what, got ..."""
    if not ok:
        raise ValueError(f"{name} must be {what}, got {t.dtype} {tuple(t.shape)}")


def _need_gt_counts(B, name, gt, counts):
    _need(gt.dtype == torch.float64 and gt.dim() == 4 and gt.shape[0] == B and 1 <= gt.shape[1] <= MAXG and tuple(gt.shape[2:]) == (NJ, 4),
          name, gt, _GT_SHAPE)
    _need(counts.dtype == torch.int32 and tuple(counts.shape) == (B,), "counts", counts, "int32 [B]")


def check_maps_args(pred_2d, depth_v, bone_mask, counts, gt_2d):
    """-> (B, G).  ValueError for anything smap_evalmaps_update must not be handed."""
    named = (("pred_2d", pred_2d), ("depth_v", depth_v), ("bone_mask", bone_mask), ("counts", counts), ("gt_2d", gt_2d))
    _check_tensors(named)
    _need(pred_2d.dtype == torch.float64 and pred_2d.dim() == 4 and tuple(pred_2d.shape[1:]) == (MAXP, NJ, 4), "pred_2d", pred_2d,
          _PRED_SHAPE + " (lift_batch(gt_mode=True))")
    B = pred_2d.shape[0]
    if B < 1:
        raise ValueError("an empty batch")
    _need(depth_v.dtype == torch.float64 and tuple(depth_v.shape) == (B, MAXP, NL), "depth_v", depth_v, f"float64 [B,{MAXP},{NL}]")
    _need(bone_mask.dtype == torch.int32 and tuple(bone_mask.shape) == (B, MAXP), "bone_mask", bone_mask, f"int32 [B,{MAXP}]")
    _need_gt_counts(B, "gt_2d", gt_2d, counts)
    _check_one_device(named)
    return B, gt_2d.shape[1]


def check_update_args(pred_3d, counts, gt):
    """-> (B, G).  ValueError for anything smap_eval3d_update must not be handed."""
    named = (("pred_3d", pred_3d), ("counts", counts), ("gt", gt))
    _check_tensors(named)
    _need(pred_3d.dtype == torch.float64 and pred_3d.dim() == 4 and tuple(pred_3d.shape[1:]) == (MAXP, NJ, 4), "pred_3d", pred_3d, _PRED_SHAPE)
    B = pred_3d.shape[0]
    _need_gt_counts(B, "gt", gt, counts)
    if B < 1:
        raise ValueError("an empty batch")
    _check_one_device(named)
    return B, gt.shape[1]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _DeviceAccumulator:
    """WIDTH float64 on `device`, updated in order by the library's INIT and UPDATE entry points.

    update() runs on the caller's current stream and returns at once; calls are ordered after one another on the device
    whatever streams they come from (an event chain, no host wait), because the sums are ordered.  raw() / summary() read the
    accumulators back -- the only host synchronisation.  A metric set supplies WIDTH, INIT, UPDATE, _check (the inputs of update()
    -> (B, G) or ValueError), _unpack (the accumulators on the host -> the raw() dict), _summarize, and merge_raws / log_lines /
    result_entry, with which test.py treats every evaluator alike."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} scores on the GPU: device must be a cuda device (there is no host scorer)")
        self._lib = _L.load()
        self.acc = torch.empty((self.WIDTH,), dtype=torch.float64, device=self.device)
        self._ev = torch.cuda.Event()
        self._launch = getattr(self._lib, self.UPDATE)
        with torch.cuda.device(self.device):
            _L.check(getattr(self._lib, self.INIT)(_p(self.acc), _stream(self.device)), self.INIT)
            self._ev.record()

    def _update(self, *tensors):
        """The inputs in the order UPDATE takes them."""
        B, G = self._check(*tensors)
        if tensors[0].device != self.device:
            raise ValueError(f"this evaluator lives on {self.device}, the tensors on {tensors[0].device}")
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(self._ev)                            # after the previous update (or the initialisation), on whatever stream it ran
            terms = torch.empty((B, G, self.WIDTH), dtype=torch.float64, device=self.device)
            _L.check(self._launch(*map(_p, tensors), B, G, _p(terms), _p(self.acc), _stream(self.device)), self.UPDATE)
            self._ev.record()

    def raw(self):
        """The reference's error dict BEFORE calculate_and_log's divisions, with its keys and types (unpack / unpack_maps)."""
        with torch.cuda.device(self.device):
            torch.cuda.current_stream(self.device).wait_event(self._ev)
            host = self.acc.cpu().numpy()
        return self._unpack(host)

    def summary(self):
        """What calculate_and_log makes of raw() (summarize / summarize_maps)."""
        return self._summarize(self.raw())


class Eval3D(_DeviceAccumulator):
    """The reference's `error` dict of a generate_result run as 80 float64 on `device`: its keys carry `_after_refine` when refine is
    set.  summary() is what the reference's calculate_and_log leaves in result['error'] in generate_result mode."""
    WIDTH, INIT, UPDATE = ACC_DOUBLES, "smap_eval3d_acc_init", "smap_eval3d_update"
    _check, _summarize = staticmethod(check_update_args), staticmethod(summarize)
    # the module's functions under the names test.py calls on every evaluator (the right-hand `log_lines` is the module's)
    merge_raws, log_lines, result_entry = staticmethod(merge), staticmethod(log_lines), staticmethod(summarize)

    def __init__(self, device, refine=False):
        self.refine = bool(refine)
        super().__init__(device)

    def _unpack(self, host):
        return unpack(host, self.refine)

    def update(self, pred_3d, counts, gt):
        """pred_3d [B,127,15,4] f64 (lift_batch(gt_mode=True) / refine_batch), counts [B] int32 (persons = kept annotations of each
        frame, register_gt_batch's matched_counts), gt [B,G,15,4] f64 (X,Y,Z,score): device tensors.  Rows >= counts[b] are not read."""
        self._update(pred_3d, counts, gt)

    def update_from_annotations(self, pred_3d, counts, annotations, root_idx=2):
        """update() with the ground truth built from B annotation arrays [G_i,15,11] (rows with root score > 1 are kept, as the
        pipeline does) and uploaded on the current stream."""
        gt, _ = gt_from_annotations(annotations, root_idx)
        self.update(pred_3d, counts, torch.from_numpy(gt).to(self.device, non_blocking=True))


class EvalMaps(_DeviceAccumulator):
    """The six `eval` accumulators of the reference's error dict (count_gt, count_pred, distance_e, distance_d, reverse_count,
    count_pred_bone) as 87 float64 on `device`.  summary(): error_point, recall, depth_e, depth_reverse_count, avg_error, avg_recall."""
    WIDTH, INIT, UPDATE = MAPS_ACC_DOUBLES, "smap_evalmaps_acc_init", "smap_evalmaps_update"
    _check, _unpack, _summarize = staticmethod(check_maps_args), staticmethod(unpack_maps), staticmethod(summarize_maps)
    merge_raws, log_lines = staticmethod(merge_maps), staticmethod(log_lines_maps)

    @staticmethod
    def result_entry(raw):
        return {k: raw[k].tolist() for k in MAPS_KEYS}

    def update(self, pred_2d, depth_v, bone_mask, counts, gt_2d):
        """pred_2d [B,127,15,4] f64, depth_v [B,127,14] f64, bone_mask [B,127] int32: lift_batch(gt_mode=True, bones=True) on the rows
        register_gt_batch matched; counts [B] int32 = its matched_counts; gt_2d [B,G,15,4] f64 = columns 0:4 of the kept annotations
        (gt2d_rows).  Device tensors; rows >= counts[b] are not read."""
        self._update(pred_2d, depth_v, bone_mask, counts, gt_2d)

    def update_from_annotations(self, pred_2d, depth_v, bone_mask, counts, annotations, root_idx=2):
        """update() with gt_2d built from B annotation arrays [G_i,15,>=4] (rows with root score > 1 are kept, as the pipeline does)
        and uploaded on the current stream."""
        gt_2d = gt2d_rows(_kept(annotations, root_idx))
        self.update(pred_2d, depth_v, bone_mask, counts, torch.from_numpy(gt_2d).to(self.device, non_blocking=True))


BONES_REFUSAL = ("the bone depth error cannot be scored from a result file: the per-limb depth `depth_v` is not in it (it exists only "
                 "inside the lifting kernel); score it while the run runs, `test.py -t generate_result --eval_maps 1`")


def _frame_preds(records, path, key):
    """What both parsers refuse first -> (n, record n, its `key` as [P,15,4]) of every record."""
    if not records:
        raise ValueError(f"{path}: no records to score")
    for n, r in enumerate(records):
        if not isinstance(r, dict) or key not in r:
            raise ValueError(f"{path}: record {n} has no {key}: not a result file of test.py")
        pred = np.asarray(r[key], np.float64)
        if pred.ndim != 3 or pred.shape[1:] != (NJ, 4):
            raise ValueError(f"{path}: record {n} holds one person, not a frame: a generate_train file cannot be scored")
        yield n, r, pred


def _refuse_crowd(path, n, pred):
    if len(pred) > MAXG:
        raise ValueError(f"{path}: record {n} has {len(pred)} persons, at most {MAXG} are scored per frame")


def _parse_records_maps(records, path):
    """Frame records -> [(pred_2d [P,15,4], gt_2d [P,15,4])]; ValueError for anything whose 2D part cannot be scored."""
    frames = []
    for n, r, pred in _frame_preds(records, path, "pred_2d"):
        if "gt_2d" not in r or len(r["gt_2d"]) == 0:
            raise ValueError(f"{path}: record {n} has no gt_2d (a run_inference file?): score a `-t generate_result` run")
        g2 = np.asarray(r["gt_2d"], np.float64)
        if g2.ndim != 3 or g2.shape[:2] != (len(pred), NJ) or g2.shape[2] < 4:
            raise ValueError(f"{path}: record {n}: gt_2d does not match the {len(pred)} persons of pred_2d")
        _refuse_crowd(path, n, pred)
        frames.append((pred, g2[:, :, 0:4]))
    return frames


def _parse_records(records, path):
    """Frame records -> [(pred [P,15,4], gt xyz [P,15,3], gt score [P,15])]; ValueError for anything that cannot be scored."""
    frames = []
    for n, r, pred in _frame_preds(records, path, "pred_3d"):
        if "gt_3d" not in r or "gt_2d" not in r:
            raise ValueError(f"{path}: record {n} has no gt_3d / gt_2d: not a generate_result file")
        if len(r["gt_3d"]) == 0 or len(r["gt_2d"]) == 0:
            raise ValueError(f"{path}: record {n} has no ground truth (a run_inference file?): score a `-t generate_result` run")
        g3, g2 = np.asarray(r["gt_3d"], np.float64), np.asarray(r["gt_2d"], np.float64)
        if g3.ndim != 3 or g2.ndim != 3 or g3.shape[:2] != (len(pred), NJ) or g2.shape[:2] != (len(pred), NJ) or g3.shape[2] < 3 or g2.shape[2] < 4:
            raise ValueError(f"{path}: record {n}: gt_3d / gt_2d do not match the {len(pred)} persons of pred_3d")
        _refuse_crowd(path, n, pred)
        frames.append((pred, g3[:, :, 0:3], g2[:, :, 3]))
    return frames


def _pred_batches(frames, frames_per_call):
    """Parsed frames (the prediction first) -> (the frames of a call, pred [B,127,15,4], counts [B]) of at most frames_per_call frames
    each, in order."""
    for s in range(0, len(frames), frames_per_call):
        part = frames[s:s + frames_per_call]
        pred = np.zeros((len(part), MAXP, NJ, 4), np.float64)
        for i, fr in enumerate(part):
            pred[i, :len(fr[0])] = fr[0]
        yield part, pred, np.asarray([len(fr[0]) for fr in part], np.int32)


def _batches(frames, frames_per_call):
    """-> (pred [B,127,15,4], counts [B], gt [B,G,15,4]) of at most frames_per_call frames each, in order."""
    for part, pred, counts in _pred_batches(frames, frames_per_call):
        gt = np.zeros((len(part), counts.max(), NJ, 4), np.float64)
        for i, (p, xyz, score) in enumerate(part):
            gt[i, :len(p), :, :3] = xyz
            gt[i, :len(p), :, 3] = score
        yield pred, counts, gt


def score_records_maps(records, device, path="<records>", frames_per_call=256):
    """The 2D part (count_gt, count_pred, distance_e) of `3d_pairs` frame records (pred_2d, gt_2d per frame) -> EvalMaps, frames in
    order.  The bone part stays zero: BONES_REFUSAL."""
    frames = _parse_records_maps(records, path)                # refusals first: they need no GPU
    ev = EvalMaps(device)
    up = lambda a: torch.from_numpy(a).to(ev.device)
    for part, pred, counts in _pred_batches(frames, frames_per_call):
        ev.update(up(pred), torch.zeros((len(part), MAXP, NL), dtype=torch.float64, device=ev.device),
                  torch.zeros((len(part), MAXP), dtype=torch.int32, device=ev.device), up(counts), up(gt2d_rows([g for _, g in part])))
    return ev


def score_records(records, device, refine=False, path="<records>", frames_per_call=256):
    """`3d_pairs` frame records (pred_3d, gt_3d, gt_2d per frame) -> Eval3D holding their score, frames in order."""
    frames = _parse_records(records, path)                     # refusals first: they need no GPU
    ev = Eval3D(device, refine)
    for pred, counts, gt in _batches(frames, frames_per_call):
        ev.update(torch.from_numpy(pred).to(ev.device), torch.from_numpy(counts).to(ev.device), torch.from_numpy(gt).to(ev.device))
    return ev


def _load_pairs(path):
    """The `3d_pairs` list of a result file, or ValueError."""
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or "3d_pairs" not in doc:
        raise ValueError(f"{path}: no `3d_pairs` list: not a result file of test.py")
    return doc["3d_pairs"]


def score_file_maps(path, device="cuda:0", frames_per_call=256):
    """Score the 2D part of a generate_result file on the GPU -> the three 2D keys of `EvalMaps.raw()`."""
    raw = score_records_maps(_load_pairs(path), device, path=path, frames_per_call=frames_per_call).raw()
    return {k: raw[k] for k in MAPS_2D_KEYS}


def score_file(path, device="cuda:0", refine=False, frames_per_call=256):
    """Score a generate_result file on the GPU -> the `raw()` dict.  Reads pred_3d, gt_3d[:, :, 0:3] and gt_2d[:, :, 3] per record.
    A file without ground truth (run_inference) or with per-person records (generate_train) is refused with ValueError."""
    return score_records(_load_pairs(path), device, refine, path=path, frames_per_call=frames_per_call).raw()


def _main_mupots(ap, args):
    """`--mupots ROOT`: convert (or read the two .mat files), score, print the summary as JSON.  Refusals: exit status 2."""
    from . import mupots as M
    if (args.pose3d is None) != (args.pose2d is None):
        ap.error("--pose3d and --pose2d come together")
    if (args.result is None) == (args.pose3d is None):
        ap.error("--mupots scores either a result JSON or --pose3d / --pose2d")
    try:
        ann = M.load_annotations(args.mupots)
        if args.result is not None:
            from lib.eval.convert import convert_records
            pose3d, pose2d, _ = convert_records(_load_pairs(args.result))
        else:
            pose2d, pose3d = M.load_pose_mats(args.pose3d, args.pose2d)
        res = M.MuPoTSScorer(ann, bool(args.relative), bool(args.use_skel), bool(args.matched_only), args.device).score(pose2d, pose3d)
        if args.out:
            res.write_csv(args.out)
    except (ValueError, OSError, KeyError, NotImplementedError) as exc:
        print(f"smap_amd.evaluate: {exc}", file=sys.stderr)
        return 2
    print(json.dumps(res.summary()))
    return 0


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m smap_amd.evaluate", description="Score a `test.py -t generate_result` file on the GPU.")
    ap.add_argument("result", nargs="?", help="result JSON (`3d_pairs` with pred_3d, gt_3d, gt_2d per frame)")
    ap.add_argument("--refine", type=int, default=0, choices=[0, 1], help="1: the run used RefineNet (keys carry _after_refine)")
    ap.add_argument("--maps", type=int, default=0, choices=[0, 1],
                    help="1: score the 2D part of the maps' metrics instead (keypoint error / recall from pred_2d and gt_2d)")
    ap.add_argument("--bones", type=int, default=0, choices=[0, 1], help="refused: " + BONES_REFUSAL)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--mupots", metavar="ROOT", default=None,
                    help="score the MuPoTS-3D protocol instead (lib/eval/mupots_smap.m): ROOT holds TS<k>/annot.mat and TS<k>/occlusion.mat")
    ap.add_argument("--relative", type=int, default=1, choices=[0, 1], help="with --mupots: 1 root-relative (is_relative), 0 absolute + ordinal rate")
    ap.add_argument("--matched_only", type=int, default=0, choices=[0, 1], help="with --mupots: EVALUATION_MODE, 1 = only matched annotations")
    ap.add_argument("--use_skel", type=int, default=1, choices=[0, 1], help="with --mupots: map the predicted bones to the ground truth's lengths")
    ap.add_argument("--out", metavar="DIR", default=None, help="with --mupots: also write the three sequence-wise CSV tables there")
    ap.add_argument("--pose3d", default=None, help="with --mupots: pose3d.mat of lib/eval/convert.py in place of the result JSON")
    ap.add_argument("--pose2d", default=None, help="with --mupots: pose2d.mat of lib/eval/convert.py")
    args = ap.parse_args(argv)
    if args.mupots is not None:
        return _main_mupots(ap, args)
    if args.result is None:
        ap.error("the following arguments are required: result")
    if args.bones:
        print(f"smap_amd.evaluate: {BONES_REFUSAL}", file=sys.stderr)
        return 2
    try:
        if args.maps:
            raw = score_file_maps(args.result, args.device)
            s = summarize_maps(dict(raw, distance_d=np.zeros(NL), reverse_count=np.zeros(NL), count_pred_bone=np.zeros(NL, np.int64)))
            out = {k: np.asarray(v).tolist() for k, v in raw.items()}
            out.update({k: np.asarray(s[k]).tolist() for k in ("error_point", "recall", "avg_error", "avg_recall")})
            print(f"smap_amd.evaluate: {BONES_REFUSAL}", file=sys.stderr)
            print(json.dumps(out))
            return 0
        raw = score_file(args.result, args.device, bool(args.refine))
    except (ValueError, OSError) as exc:
        print(f"smap_amd.evaluate: {exc}", file=sys.stderr)
        return 2
    print(json.dumps(summarize(raw)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
