#!/usr/bin/env python3
"""Label rendering on the GPU (smap_amd/labels.py, csrc/labels.hip) against its numpy restatement on the same box's host.

    python tools/bench_labels.py [--batches 200] [--frames 8] [--out profiles/labels_bench.json] [--cli 1]

Per person count (2, 8, 20 per frame, 128 x 208 maps, five label scales): device time per batch from HIP events over `--batches`
renders of one packed table (upload + the two launches; warmed up first), the host's time to pack that table, and the host's time for
tests/golden/labels_restate.labels on the same batch (one core, numpy) -- after checking that the two agree bit for bit.
`--cli 1` also runs `test.py -t generate_result --maps_from_gt 1 --eval_3d 1 --eval_maps 1` on the annotation file of the CLI test
(tests/test_labels_gpu.py) and records its `error` summary: the error that remains with perfect maps.  Nothing here asserts a time."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import labels_restate as R  # noqa: E402

SHAPE, STRIDE = (128, 208), 4


def scene(frames, persons, seed):
    """`frames` arrays [persons, 15, 8]: joints scattered over a person-sized window, visibility 1 or 2."""
    rng = np.random.default_rng(seed)
    H, W = SHAPE[0] * STRIDE, SHAPE[1] * STRIDE
    out = []
    for _ in range(frames):
        b = np.zeros((persons, 15, 8))
        centre = np.stack([rng.uniform(60, W - 60, persons), rng.uniform(130, H - 130, persons)], 1)
        b[:, :, :2] = centre[:, None, :] + rng.normal(0, 1, (persons, 15, 2)) * (35, 70)
        b[:, :, 0] = np.clip(b[:, :, 0], 0, W - 0.01)
        b[:, :, 1] = np.clip(b[:, :, 1], 0, H - 0.01)
        b[:, :, 2] = rng.uniform(200, 700, (persons, 1)) + rng.normal(0, 12, (persons, 15))
        b[:, :, 3] = rng.choice([1, 2], (persons, 15))
        b[:, :, 7] = 1400.0
        out.append(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "labels_bench.json"))
    ap.add_argument("--cli", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_labels.py measures on the GPU; none found")
    from exps.stage3_root2.config import cfg
    from smap_amd.labels import label_spec, launch_table, pack_table
    dev = "cuda:0"
    spec = label_spec(cfg)
    doc = {"gpu": torch.cuda.get_device_name(0), "frames_per_batch": args.frames, "batches": args.batches, "map": list(SHAPE),
           "label_scales": len(spec.kernels), "output_mb_per_batch": args.frames * len(spec.kernels) * 57 * SHAPE[0] * SHAPE[1] * 4 / 1e6,
           "what": "device_ms_per_batch: HIP events around --batches renders (table upload + 2 launches each) / batches; "
                   "host_pack_ms: smap_amd.labels.pack_table; numpy_ms_per_batch: labels_restate.labels over the batch, one core",
           "cases": []}
    for persons in (2, 8, 20):
        frames = scene(args.frames, persons, 100 + persons)
        t0 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            buf, ksizes, P = pack_table(frames, spec.kernels, spec.thres, spec.paf_vector, spec.stride, spec.shape)
        pack_ms = (time.perf_counter() - t0) / reps * 1e3
        out = torch.empty((args.frames, len(spec.kernels), 57) + SHAPE, dtype=torch.float32, device=dev)
        render = lambda: launch_table(buf, ksizes, P, args.frames, len(spec.kernels), spec.shape, dev, out)
        for _ in range(10):
            render()
        torch.cuda.synchronize()
        per = []
        for _ in range(args.batches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            render()
            e1.record()
            per.append((e0, e1))
        torch.cuda.synchronize()
        ms = np.asarray([a.elapsed_time(b) for a, b in per])
        t0 = time.perf_counter()
        want = np.stack([R.labels(f, SHAPE, STRIDE) for f in frames])
        numpy_ms = (time.perf_counter() - t0) * 1e3
        got = out.cpu().numpy()
        same = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
        case = {"persons_per_frame": persons, "device_ms_per_batch": float(ms.mean()), "device_ms_per_batch_median": float(np.median(ms)),
                "device_ms_per_batch_min": float(ms.min()), "device_ms_per_batch_max": float(ms.max()),
                "host_pack_ms_per_batch": pack_ms, "numpy_ms_per_batch": numpy_ms, "table_bytes": int(len(buf)),
                "equal_to_the_restatement_bit_for_bit": same}
        print(json.dumps(case), flush=True)
        doc["cases"].append(case)
    if args.cli:
        import test_labels_gpu as T
        with tempfile.TemporaryDirectory() as tmp:
            from pathlib import Path
            tmp = Path(tmp)
            z = np.load(os.path.join(ROOT, "tests", "golden", "labels.npz"))
            root = T.write_annotations(tmp, z)
            env = dict(os.environ, PROJECT_HOME=str(tmp), SMAP_TEST_ROOT=str(root), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
            r = subprocess.run([sys.executable, os.path.join(ROOT, "exps", "stage3_root2", "test.py"), "-t", "generate_result", "-d", "test",
                                "--batch_size", "2", "--maps_from_gt", "1", "--eval_3d", "1", "--eval_maps", "1", "--json_name", "ceiling"],
                               capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp))
            cli = {"command": "test.py -t generate_result -d test --batch_size 2 --maps_from_gt 1 --eval_3d 1 --eval_maps 1",
                   "annotations": "tests/test_labels_gpu.py write_annotations: 3 frames of 3, 2 and 1 persons (the `pipe` scene), no image files",
                   "returncode": r.returncode}
            if r.returncode == 0:
                res = json.loads((tmp / "model_logs" / "stage3_root2" / "result" / "stage3_root2_generate_result_test_ceiling.json").read_text())
                cli["records"] = len(res["3d_pairs"])
                cli["error"] = res["error"]
                cli["log"] = [l for l in r.stderr.splitlines() if " INFO " in l and "Pairs writed" not in l][-12:]
            else:
                cli["stderr"] = r.stderr[-2000:]
            doc["perfect_maps_ceiling"] = cli
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
