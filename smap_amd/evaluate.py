"""MPJPE / PCK / ordinal scoring of `generate_result` runs, on the GPU.

Reference: lib/eval/test_util_panoptic.py -- `eval_3d` (:273-307), `initialization` (:332-355) and the generate_result
branch of `calculate_and_log` (:379-408), which puts an `error` dict into the result file.  The reference scores one
person at a time with ~20 numpy calls on the host; here the persons of a batch are scored by the HIP kernels of
csrc/eval.hip next to the float64 tensors the ground-truth modes already keep on the device (smap_lift_gt /
smap_refine_gt), on the stream the caller is on, and nothing comes back to the host before `raw()` / `summary()`.

The 80 float64 accumulators (include/smap_hip.h, SMAP_EVAL_ACC_DOUBLES) live on the device across `update` calls and are
the reference's running sums bit for bit: every person's terms are added one `+=` per field, frames then persons in
order.  Not scored (out of scope): the 2D error / recall of `eval_one_image` and the per-bone depth error.

    python -m smap_amd.evaluate RESULT.json [--refine 0|1] [--device cuda:0]

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


def gt_rows(annotations, gmax=None):
    """B annotation arrays [G_i,15,>=7] -> (gt [B,G,15,4] float64 = (X,Y,Z,score) = columns 4:7 and 3, row for row, zero padded;
    counts [B]).  No row is dropped: row g stays the annotation the registration kernel calls g."""
    rows = [np.asarray(a, np.float64) for a in annotations]
    rows = [a if a.size else np.zeros((0, NJ, 11)) for a in rows]
    G = max(1, max((len(a) for a in rows), default=1)) if gmax is None else int(gmax)
    if G > MAXG or any(len(a) > G for a in rows):
        raise ValueError("at most %d annotations per frame" % MAXG)
    gt = np.zeros((len(rows), G, NJ, 4), np.float64)
    for i, a in enumerate(rows):
        if len(a):
            gt[i, :len(a), :, :3] = a[:, :, 4:7]
            gt[i, :len(a), :, 3] = a[:, :, 3]
    return gt, np.asarray([len(a) for a in rows], np.int32)


def gt_from_annotations(annotations, root_idx=2):
    """gt_rows of the annotations whose root score is > 1 -- the pipeline's filter (records.kept_annotations, test.py:76-80)."""
    kept = []
    for a in annotations:
        a = np.asarray(a, np.float64)
        kept.append(a[a[:, root_idx, 3] > 1] if a.size else a)
    return gt_rows(kept)


def check_update_args(pred_3d, counts, gt):
    """-> (B, G).  ValueError for anything smap_eval3d_update must not be handed."""
    for name, t in (("pred_3d", pred_3d), ("counts", counts), ("gt", gt)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch.Tensor")
        if not t.is_cuda:
            raise ValueError(f"{name} must live on the GPU (there is no host scorer)")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if pred_3d.dim() != 4 or tuple(pred_3d.shape[1:]) != (MAXP, NJ, 4) or pred_3d.dtype != torch.float64:
        raise ValueError(f"pred_3d must be float64 [B,{MAXP},{NJ},4], got {pred_3d.dtype} {tuple(pred_3d.shape)}")
    B = pred_3d.shape[0]
    if gt.dim() != 4 or gt.shape[0] != B or tuple(gt.shape[2:]) != (NJ, 4) or gt.dtype != torch.float64 or not 1 <= gt.shape[1] <= MAXG:
        raise ValueError(f"gt must be float64 [B,G,{NJ},4] with 1 <= G <= {MAXG}, got {gt.dtype} {tuple(gt.shape)}")
    if tuple(counts.shape) != (B,) or counts.dtype != torch.int32:
        raise ValueError(f"counts must be int32 [B], got {counts.dtype} {tuple(counts.shape)}")
    if B < 1:
        raise ValueError("an empty batch")
    if not (pred_3d.device == counts.device == gt.device):
        raise ValueError("pred_3d, counts and gt must be on one device")
    return B, gt.shape[1]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Eval3D:
    """The reference's `error` dict of a generate_result run as 80 float64 on `device`.

    update() runs on the caller's current stream and returns at once; calls are ordered after one another on the device
    whatever streams they come from (an event chain, no host wait), because the sums are ordered.  raw() / summary() read the
    accumulators back -- the only host synchronisation."""

    def __init__(self, device, refine=False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("Eval3D scores on the GPU: device must be a cuda device (there is no host scorer)")
        self.refine = bool(refine)
        self._lib = _L.load()
        self.acc = torch.empty((ACC_DOUBLES,), dtype=torch.float64, device=self.device)
        self._ev = torch.cuda.Event()
        with torch.cuda.device(self.device):
            _L.check(self._lib.smap_eval3d_acc_init(_p(self.acc), _stream(self.device)), "smap_eval3d_acc_init")
            self._ev.record()

    def update(self, pred_3d, counts, gt):
        """pred_3d [B,127,15,4] f64 (lift_batch(gt_mode=True) / refine_batch), counts [B] int32 (persons = kept annotations of each
        frame, register_gt_batch's matched_counts), gt [B,G,15,4] f64 (X,Y,Z,score): device tensors.  Rows >= counts[b] are not read."""
        B, G = check_update_args(pred_3d, counts, gt)
        if pred_3d.device != self.device:
            raise ValueError(f"this evaluator lives on {self.device}, the tensors on {pred_3d.device}")
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(self._ev)                            # after the previous update (or the initialisation), on whatever stream it ran
            terms = torch.empty((B, G, TERM_DOUBLES), dtype=torch.float64, device=self.device)
            _L.check(self._lib.smap_eval3d_update(_p(pred_3d), _p(counts), _p(gt), B, G, _p(terms), _p(self.acc), _stream(self.device)),
                     "smap_eval3d_update")
            self._ev.record()

    def update_from_annotations(self, pred_3d, counts, annotations, root_idx=2):
        """update() with the ground truth built from B annotation arrays [G_i,15,11] (rows with root score > 1 are kept, as the
        pipeline does) and uploaded on the current stream."""
        gt, _ = gt_from_annotations(annotations, root_idx)
        self.update(pred_3d, counts, torch.from_numpy(gt).to(self.device, non_blocking=True))

    def raw(self):
        """The reference's error dict BEFORE calculate_and_log's divisions: its keys (with `_after_refine` when refine is set), ndarray
        float64 [15] / int / float values."""
        with torch.cuda.device(self.device):
            torch.cuda.current_stream(self.device).wait_event(self._ev)
            host = self.acc.cpu().numpy()
        return unpack(host, self.refine)

    def summary(self):
        """What the reference's calculate_and_log leaves in result['error'] in generate_result mode."""
        return summarize(self.raw())


def _parse_records(records, path):
    """Frame records -> [(pred [P,15,4], gt xyz [P,15,3], gt score [P,15])]; ValueError for anything that cannot be scored."""
    if not records:
        raise ValueError(f"{path}: no records to score")
    frames = []
    for n, r in enumerate(records):
        if not isinstance(r, dict) or "pred_3d" not in r:
            raise ValueError(f"{path}: record {n} has no pred_3d: not a result file of test.py")
        pred = np.asarray(r["pred_3d"], np.float64)
        if pred.ndim != 3 or pred.shape[1:] != (NJ, 4):
            raise ValueError(f"{path}: record {n} holds one person, not a frame: a generate_train file cannot be scored")
        if "gt_3d" not in r or "gt_2d" not in r:
            raise ValueError(f"{path}: record {n} has no gt_3d / gt_2d: not a generate_result file")
        if len(r["gt_3d"]) == 0 or len(r["gt_2d"]) == 0:
            raise ValueError(f"{path}: record {n} has no ground truth (a run_inference file?): score a `-t generate_result` run")
        g3, g2 = np.asarray(r["gt_3d"], np.float64), np.asarray(r["gt_2d"], np.float64)
        if g3.ndim != 3 or g2.ndim != 3 or g3.shape[:2] != (len(pred), NJ) or g2.shape[:2] != (len(pred), NJ) or g3.shape[2] < 3 or g2.shape[2] < 4:
            raise ValueError(f"{path}: record {n}: gt_3d / gt_2d do not match the {len(pred)} persons of pred_3d")
        if len(pred) > MAXG:
            raise ValueError(f"{path}: record {n} has {len(pred)} persons, at most {MAXG} are scored per frame")
        frames.append((pred, g3[:, :, 0:3], g2[:, :, 3]))
    return frames


def _batches(frames, frames_per_call):
    """-> (pred [B,127,15,4], counts [B], gt [B,G,15,4]) of at most frames_per_call frames each, in order."""
    for s in range(0, len(frames), frames_per_call):
        part = frames[s:s + frames_per_call]
        G = max(len(p) for p, _, _ in part)
        pred = np.zeros((len(part), MAXP, NJ, 4), np.float64)
        gt = np.zeros((len(part), G, NJ, 4), np.float64)
        for i, (p, xyz, score) in enumerate(part):
            pred[i, :len(p)] = p
            gt[i, :len(p), :, :3] = xyz
            gt[i, :len(p), :, 3] = score
        yield pred, np.asarray([len(p) for p, _, _ in part], np.int32), gt


def score_records(records, device, refine=False, path="<records>", frames_per_call=256):
    """`3d_pairs` frame records (pred_3d, gt_3d, gt_2d per frame) -> Eval3D holding their score, frames in order."""
    frames = _parse_records(records, path)                     # refusals first: they need no GPU
    ev = Eval3D(device, refine)
    for pred, counts, gt in _batches(frames, frames_per_call):
        ev.update(torch.from_numpy(pred).to(ev.device), torch.from_numpy(counts).to(ev.device), torch.from_numpy(gt).to(ev.device))
    return ev


def score_file(path, device="cuda:0", refine=False, frames_per_call=256):
    """Score a generate_result file on the GPU -> the `raw()` dict.  Reads pred_3d, gt_3d[:, :, 0:3] and gt_2d[:, :, 3] per record.
    A file without ground truth (run_inference) or with per-person records (generate_train) is refused with ValueError."""
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or "3d_pairs" not in doc:
        raise ValueError(f"{path}: no `3d_pairs` list: not a result file of test.py")
    return score_records(doc["3d_pairs"], device, refine, path=path, frames_per_call=frames_per_call).raw()


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m smap_amd.evaluate", description="Score a `test.py -t generate_result` file on the GPU.")
    ap.add_argument("result", help="result JSON (`3d_pairs` with pred_3d, gt_3d, gt_2d per frame)")
    ap.add_argument("--refine", type=int, default=0, choices=[0, 1], help="1: the run used RefineNet (keys carry _after_refine)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    try:
        raw = score_file(args.result, args.device, bool(args.refine))
    except (ValueError, OSError) as exc:
        print(f"smap_amd.evaluate: {exc}", file=sys.stderr)
        return 2
    print(json.dumps(summarize(raw)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
