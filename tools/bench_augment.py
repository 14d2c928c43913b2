#!/usr/bin/env python3
"""Training-sample augmentation on the GPU (smap_amd/augment.py, csrc/augment.hip) against its floor and its numpy restatement.

    python tools/bench_augment.py [--batches 200] [--frames 8] [--out profiles/augment_bench.json]

Per source size (1920 x 1080, and 640 x 480: the COCO case, which is upscaled), `--frames` frames resident on the device into the
512 x 832 network frame, device time per batch from HIP events around each of `--batches` launches (warmed up first; median, min - max,
and the mean over one event pair around the whole window):
  fused_rotate      smap_augment_batch with rotation on (the plans of plan_sample under seeded draws: degrees in +-10, flips, shifts)
  fused_no_rotate   smap_augment_batch with rotate = 0, flip = 0
  preprocess_batch  smap_preprocess_batch on the same frames and windows: the floor -- the same output bytes written, no warp
  numpy_one_core    the staged restatement (warp_affine_cubic_u8 + resize_linear_u8 + paste + normalise) of ONE frame on one core,
                    times `--frames` (the whole batch would take minutes)
The fused outputs are checked against the restatement (one frame per case) and against preprocess_batch (rotation off) bit for bit
before anything is timed.  Nothing here asserts a time."""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NET_H, NET_W = 512, 832


def timed(fn, batches, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0.record()
    for _ in range(batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        per.append((e0, e1))
    w1.record()
    torch.cuda.synchronize()
    us = np.asarray([a.elapsed_time(b) for a, b in per]) * 1e3
    return {"median_us": float(np.median(us)), "min_us": float(us.min()), "max_us": float(us.max()),
            "window_mean_us": float(w0.elapsed_time(w1) * 1e3 / batches)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py measures on the GPU; none found")
    from exps.stage3_root2.config import cfg
    from smap_amd import augment as A
    from smap_amd import lib as L
    lib, dev = L.load(), torch.device("cuda:0")
    params = A.AugParams.from_cfg(cfg)
    mean, std = (C.c_float * 3)(*cfg.INPUT.MEANS), (C.c_float * 3)(*cfg.INPUT.STDS)
    tab = A.device_cubic_table(dev)
    out = torch.empty((args.frames, 3, NET_H, NET_W), dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    doc = {"gpu": torch.cuda.get_device_name(0), "frames_per_batch": args.frames, "batches": args.batches, "net": [NET_H, NET_W],
           "output_mb_per_batch": args.frames * 3 * NET_H * NET_W * 4 / 1e6,
           "what": "device time per batch of frames already on the device: HIP events around each launch (median, min, max) and around "
                   "the whole window (window_mean_us); numpy_one_core_ms_per_batch = one frame's staged restatement x frames", "cases": []}
    for h, w, dataset in ((1080, 1920, "MUCO"), (480, 640, "COCO")):
        rng = np.random.default_rng(h)
        y, x = np.mgrid[0:h, 0:w].astype(np.float32)
        host = [np.clip(128 + 70 * np.sin(0.01 * (k + 2) * x + 0.013 * y)[..., None] + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
                for k in range(args.frames)]
        frames = [torch.from_numpy(f).to(dev) for f in host]
        entry = {"dataset": dataset, "img_width": w, "img_height": h, "bodys": []}
        plans = {True: [A.plan_sample(entry, A.draw(random.Random("bench:%d:%d" % (h, k))), params, True)[2] for k in range(args.frames)],
                 False: [A.plan_sample(entry, (0.5,) * 5, params, False)[2] for _ in range(args.frames)]}
        tables = {k: (L.AugFrame * args.frames)(*[A.aug_frame(f.data_ptr(), h, w, p) for f, p in zip(frames, v)]) for k, v in plans.items()}
        prep = (L.PrepFrame * args.frames)(*[L.PrepFrame(f.data_ptr(), h, w, p["nh"], p["nw"], p["top"], p["left"], p["fx"], p["fy"])
                                             for f, p in zip(frames, plans[False])])
        fused = lambda key: L.check(lib.smap_augment_batch(tables[key], args.frames, C.c_void_p(out.data_ptr()), NET_H, NET_W, mean, std,
                                                           C.c_void_p(tab.data_ptr()), st), "smap_augment_batch")
        floor = lambda: L.check(lib.smap_preprocess_batch(prep, args.frames, C.c_void_p(out.data_ptr()), NET_H, NET_W, mean, std, st),
                                "smap_preprocess_batch")
        bits = lambda t: t.cpu().contiguous().view(torch.int32)
        # correctness first: rotation on against the restatement (frame 0, timed: the one-core figure), rotation off against the floor
        fused(True)
        got = bits(out[0])
        t0 = time.perf_counter()
        want = A.staged_sample(host[0], plans[True][0], NET_H, NET_W, cfg.INPUT.MEANS, cfg.INPUT.STDS)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        same_rot = bool(torch.equal(got, bits(want)))
        fused(False)
        got = bits(out)
        floor()
        same_floor = bool(torch.equal(got, bits(out)))
        case = {"source": [h, w], "dataset": dataset, "degrees": [round(math_degree(p), 3) for p in plans[True]],
                "fused_rotate": timed(lambda: fused(True), args.batches), "fused_no_rotate": timed(lambda: fused(False), args.batches),
                "preprocess_batch": timed(floor, args.batches), "numpy_one_core_ms_per_batch": numpy_ms * args.frames,
                "numpy_one_core_ms_one_frame": numpy_ms, "rotate_equal_to_the_restatement_bit_for_bit": same_rot,
                "no_rotate_equal_to_preprocess_batch_bit_for_bit": same_floor}
        print(json.dumps(case), flush=True)
        doc["cases"].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


def math_degree(plan):
    """The clockwise angle of a plan's matrix, in degrees."""
    import math
    return math.degrees(math.atan2(-plan["m"][1], plan["m"][0]))


if __name__ == "__main__":
    main()
