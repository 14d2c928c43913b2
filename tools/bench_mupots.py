#!/usr/bin/env python3
"""The MuPoTS-3D scorer on the GPU (smap_amd/mupots.py, csrc/mupots.hip) against its restatement on the same box's host.

    python tools/bench_mupots.py [--reps 20] [--out profiles/mupots_bench.json]

A synthetic set the size of the real one: 20 sequences, 8370 frames, 3 valid persons and 6 predictions per frame (three of them near a
person, three far away).  Device time per scoring from HIP events over `--reps` runs (upload of the predictions + the two launches;
the ground truth is resident, warmed up first), the host's time for tests/mupots_restate.score on the same set (one core, plain
Python floats) -- after checking that rows and accumulators agree bit for bit.  The workload is small; nothing here asserts a time."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import mupots_restate as R  # noqa: E402
import mupots_scenes as S  # noqa: E402

SEQUENCES, FRAMES, PERSONS, PREDICTIONS, NJ = 20, 8370, 3, 6, 15


def synthetic(seed=1):
    rng = np.random.default_rng(seed)
    per_seq = [FRAMES // SEQUENCES + (1 if s < FRAMES % SEQUENCES else 0) for s in range(SEQUENCES)]
    seq_offset = np.concatenate([[0], np.cumsum(per_seq)]).astype(np.int32)
    F, G, P = FRAMES, PERSONS, PREDICTIONS
    pelvis = np.stack([rng.uniform(-1500, 1500, (F, G)), rng.uniform(-300, 300, (F, G)), rng.uniform(2000, 6000, (F, G))], -1)
    gt3d = pelvis[:, :, None, :] + S.TEMPLATE + rng.normal(0, 15, (F, G, NJ, 3))
    centre = np.stack([300.0 + 500 * np.arange(G)[None, :] + rng.uniform(-80, 80, (F, G)), rng.uniform(300, 700, (F, G))], -1)
    gt2d = centre[:, :, None, :] + S.TEMPLATE[:, :2] * 0.25
    occ = (rng.random((F, G, NJ)) < 0.2).astype(np.float64)
    order = np.asarray(R.SMAP_ORDER) - 1
    p2 = np.zeros((F, P, NJ, 2))
    p3 = np.zeros((F, P, NJ, 4))
    near2 = gt2d + rng.normal(0, 8, (F, G, NJ, 2))
    near3 = gt3d + rng.normal(0, 60, (F, G, NJ, 3)) + rng.normal(0, 150, (F, G, 1, 3))
    far2 = np.array([6000.0, 5000.0]) + rng.normal(0, 50, (F, P - G, NJ, 2))
    far3 = np.array([0.0, 0.0, 9000.0]) + S.TEMPLATE + rng.normal(0, 20, (F, P - G, NJ, 3))
    slots = np.stack([rng.permutation(P) for _ in range(F)])                      # where the near predictions sit in the frame
    proto2 = np.concatenate([near2, far2], 1)
    proto3 = np.concatenate([near3, far3], 1)
    idx = np.arange(F)[:, None]
    tmp2, tmp3 = np.zeros_like(proto2), np.zeros_like(proto3)
    tmp2[idx, slots], tmp3[idx, slots] = proto2, proto3
    p2[:, :, order], p3[:, :, order, :3] = tmp2, tmp3
    p3[..., 3] = 1.0
    return seq_offset, np.full(F, G, np.int32), gt2d, gt3d, occ, p2, p3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mupots_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mupots.py measures on the GPU; none found")
    from smap_amd.mupots import Annotations, MuPoTSScorer
    dev = "cuda:0"
    seq_offset, counts, gt2d, gt3d, occ, p2, p3 = synthetic()
    F = len(counts)
    ann = Annotations(list(range(1, SEQUENCES + 1)), seq_offset, counts, gt2d, gt3d, occ)
    scorer = MuPoTSScorer(ann, device=dev)
    pred2d, pred3d = np.ascontiguousarray(p2.reshape(-1, NJ, 2)), np.ascontiguousarray(p3.reshape(-1, NJ, 4))
    offsets = (np.arange(F + 1) * PREDICTIONS).astype(np.int32)
    pinned = [torch.from_numpy(a).pin_memory() for a in (pred2d, pred3d, offsets)]

    def once(out=None):
        return scorer.launch(*(t.to(dev, non_blocking=True) for t in pinned), out=out)

    out = once()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        once(out)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    match, considered, err, rootz, acc = (t.cpu().numpy() for t in out)

    t0 = time.perf_counter()
    rows, accs = R.score(seq_offset, counts, gt2d, gt3d, occ, [(p2[f], p3[f]) for f in range(F)], True, True, False)
    host_s = time.perf_counter() - t0
    w_match, w_considered, w_err, w_rootz = S.rows_arrays(rows, F, PERSONS)
    equal = bool((match == w_match).all() and (considered == w_considered).all() and S.same_bits(err, w_err) and
                 S.same_bits(rootz, w_rootz) and S.same_bits(acc, np.asarray(accs)))
    t = R.tables(accs)
    result = {"gpu": torch.cuda.get_device_name(0), "sequences": SEQUENCES, "frames": F, "persons_per_frame": PERSONS,
              "predictions_per_frame": PREDICTIONS, "reps": args.reps,
              "what": "device_ms: HIP events around one scoring = upload of the predictions (pinned, %d bytes) + smap_mupots_frames + "
                      "smap_mupots_fold, ground truth resident; restatement_s: tests/mupots_restate.score on one core"
                      % sum(a.nbytes for a in (pred2d, pred3d, offsets)),
              "device_ms_median": float(np.median(times)), "device_ms_min": float(np.min(times)), "device_ms_max": float(np.max(times)),
              "restatement_s": host_s, "equal_to_the_restatement_bit_for_bit": equal,
              "mean_pck": float(np.mean([r[-1] for r in t["pck"]])), "mean_auc": float(np.mean([r[-1] for r in t["auc"]])),
              "matched": int((match >= 0).sum())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
