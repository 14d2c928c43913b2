#!/usr/bin/env python3
"""End-to-end rate of the SHIPPED command line on a folder of images:

    python exps/stage3_root2/test.py -t run_inference -d test --batch_size 8 --dataset_path <folder> [--device_preprocess 1]

decode -> [host resize | H2D of the uint8 image + GPU pre-processing] -> backbone -> association -> lifting -> records -> JSON, timed
inside the CLI's own loop (SMAP_CLI_TIMING) and around the whole process.  The folder is generated here: N images of two source
resolutions -- the bench's 8 frames as 832x512 PNGs and as 1664x1024 JPEGs (every pixel doubled: the pre-processing's 2x shrink gives
the frame back) -- so that the network sees the workload the bench line is quoted on (~20 skeletons per frame: association, lifting
and record building do real work); a second folder holds the same pictures as .npy (no decoder).

    python tools/cli_e2e.py [--images 256] [--out profiles/r5_cli_e2e.json] [--only jpeg | --only huffman [--pairs 3] | --only gt [--pairs 3]]

A third folder holds only the 1664x1024 JPEGs: there the PIL decoders (16 threads, 16 processes) run against `--device_decode 1`
(Huffman decode on the host, the rest of the decode on the GPU) and the .npy frames.  --only jpeg runs those four legs alone.  --only huffman runs, on that folder, `--device_decode 1` against
`--device_decode 2` (the Huffman decode on the GPU as well) alternating, `--pairs` times each at SMAP_DECODE_THREADS = 16 and = 2 after one
uncounted run that builds the plan cache, and adds a summary with the mean and the spread (min .. max) of every leg.
--only gt measures the GROUND-TRUTH modes: an annotated folder (M3E_gt.json + the 1664x1024 JPEGs) run as
`-t generate_result --eval_3d 1` on the host loader (lib/utils/dataloader.py), with `--device_preprocess 1`, and with `--device_decode 1` / `2`
on top, `--pairs` times each, interleaved, after one uncounted run; and the pre-processing of 8 1080p frames alone, by device events over
200 batches: 8 launches of smap_preprocess against one of smap_preprocess_batch.
--only maps measures what `--eval_maps 1` costs: on the same annotated folder, `-t generate_result --eval_3d 1 --device_preprocess 1
--device_decode 1` without and with `--eval_maps 1`, `--pairs` times each, interleaved, after one uncounted run -- and, with `--parent DIR` (a
built checkout of the parent commit), that checkout's run of the command without the flag as a third interleaved leg; then the device-event
time of smap_evalmaps_update alone, back to back, at a step's shapes.
--only scorers measures that time for both scorers, smap_eval3d_update and smap_evalmaps_update, and with `--parent DIR` on that
checkout's library as well: one process per tree and repeat, alternating, `--pairs` repeats each.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def bench_frames_as_images(cfg_means, cfg_stds):
    """The bench's 8 input frames (randn, seed 1234: the frames the workload's heads were calibrated on, ~20 skeletons each) as uint8
    BGR images of the network size: pixel = (x * std + mean) * 255, rounded and clipped -- what a decoder hands the pre-processing."""
    x = torch.randn(8, 3, 512, 832, generator=torch.Generator().manual_seed(1234))
    mean = torch.tensor(cfg_means).view(1, 3, 1, 1)
    std = torch.tensor(cfg_stds).view(1, 3, 1, 1)
    return ((x * std + mean) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()     # [8,512,832,3]


def preprocess_launch_ab(batches=200, frames=8, h=1080, w=1920):
    """Per-batch device time of the pre-processing of `frames` h x w frames (crop-and-pad geometry, separate source buffers, one fp32
    batch): `frames` launches of smap_preprocess against one launch of smap_preprocess_batch, by events around `batches` batches,
    three times each, alternating."""
    import ctypes as C
    from dataset.base_dataset import croppad_geometry
    from exps.stage3_root2.config import cfg as run_cfg
    from smap_amd import lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    scale, (nh, nw), (left, top) = croppad_geometry(w, h, 832, 512)
    srcs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(i)).to(dev) for i in range(frames)]
    out = torch.empty((frames, 3, 512, 832), dtype=torch.float32, device=dev)
    mean, std = (C.c_float * 3)(*run_cfg.INPUT.MEANS), (C.c_float * 3)(*run_cfg.INPUT.STDS)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    table = (L.PrepFrame * frames)(*[L.PrepFrame(s.data_ptr(), h, w, nh, nw, top, left, scale, scale) for s in srcs])

    def single():
        for i, s in enumerate(srcs):
            L.check(lib.smap_preprocess(C.c_void_p(s.data_ptr()), h, w, nh, nw, top, left, C.c_void_p(out[i].data_ptr()), 512, 832, mean, std,
                                        scale, scale, st), "smap_preprocess")

    def batched():
        L.check(lib.smap_preprocess_batch(table, frames, C.c_void_p(out.data_ptr()), 512, 832, mean, std, st), "smap_preprocess_batch")

    def timed(fn):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(batches):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / batches                  # us per batch
    res = {"single_launches_us_per_batch": [], "batched_launch_us_per_batch": []}
    for _ in range(3):
        res["single_launches_us_per_batch"].append(timed(single))
        res["batched_launch_us_per_batch"].append(timed(batched))
    single()
    ref = out.clone()
    out.zero_()
    batched()
    res.update(frames=frames, source=f"{w}x{h}", batches=batches, same_bits=bool(torch.equal(ref, out)))
    return res


def update_us(evaluator="maps", shapes=((8, 4), (8, 20), (16, 20), (8, 64), (17, 64)), iters=200):
    """Device-event time of one scorer's update alone ("maps": smap_evalmaps_update, "3d": smap_eval3d_update), back to back, per
    call, for (B, G): every annotation matched to a full person."""
    from smap_amd.evaluate import Eval3D, EvalMaps
    dev = torch.device("cuda:0")
    out = {}
    for B, G in shapes:
        g = torch.Generator().manual_seed(B * 100 + G)
        p2 = torch.zeros((B, 127, 15, 4), dtype=torch.float64)
        p2[:, :G] = torch.rand((B, G, 15, 4), generator=g, dtype=torch.float64) * 400 + 1
        gt = p2[:, :G].clone() + torch.randn((B, G, 15, 4), generator=g, dtype=torch.float64) * 3
        gt[..., 3] = 2
        dv = torch.randn((B, 127, 14), generator=g, dtype=torch.float64)
        counts = torch.full((B,), G, dtype=torch.int32, device=dev)
        if evaluator == "maps":
            ev, a = EvalMaps(dev), [p2.to(dev), dv.to(dev), torch.full((B, 127), (1 << 14) - 1, dtype=torch.int32, device=dev), counts,
                                    gt.contiguous().to(dev)]
        else:
            ev, a = Eval3D(dev), [p2.to(dev), counts, gt.contiguous().to(dev)]
        for _ in range(10):
            ev.update(*a)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(iters):
            ev.update(*a)
        t1.record()
        torch.cuda.synchronize()
        out[f"B={B},G={G}"] = {"us_per_update": t0.elapsed_time(t1) * 1e3 / iters, "launches": 2 if B * G > 1024 else 1}
    return out


def scorers_leg(args):
    """--only scorers: update_us of both scorers on this tree and, with --parent, on that checkout's package: one process per tree and
    repeat, alternating, `--pairs` repeats each.  A shape passes when this tree's median is at most the parent's median plus the
    parent's own spread (max - min) over its repeats."""
    trees = ([("parent", os.path.abspath(args.parent))] if args.parent else []) + [("this", ROOT)]
    runs = {name: [] for name, _ in trees}
    for _ in range(args.pairs):
        for name, tree in trees:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--scorers_child", tree], capture_output=True, text=True, timeout=600)
            if r.returncode:
                sys.exit(f"{name}: update_us failed ({r.returncode}): {r.stderr[-1500:]}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"what": "Eval3D.update / EvalMaps.update alone, back to back, by device events: tools/cli_e2e.py --only scorers --pairs N --parent DIR",
           "gpu": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "repeats_alternating": args.pairs,
           "rule": "this tree's median <= the parent's median + (the parent's max - min)", "shapes": {}}
    for scorer in ("3d", "maps"):
        for shape in runs["this"][0][scorer]:
            us = {name: [rep[scorer][shape]["us_per_update"] for rep in reps] for name, reps in runs.items()}
            rec = {f"{name}_us": v for name, v in us.items()}
            rec.update({f"{name}_median_us": float(np.median(v)) for name, v in us.items()})
            if args.parent:
                rec["parent_spread_us"] = max(us["parent"]) - min(us["parent"])
                rec["passes"] = bool(rec["this_median_us"] <= rec["parent_median_us"] + rec["parent_spread_us"])
            out["shapes"][f"{scorer} {shape}"] = rec
    if args.parent:
        out["shapes_passing"], out["shapes_measured"] = sum(v["passes"] for v in out["shapes"].values()), len(out["shapes"])
    print(json.dumps(out["shapes"], indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


def gt_leg(args, tmp, jpg):
    """--only gt and --only maps: see the module's docstring."""
    rng = np.random.default_rng(7)
    root = os.path.join(tmp, "MultiPersonTestSet")
    os.makedirs(os.path.join(root, "TS1"))
    entries = []
    for i in range(args.images):                                  # the 1664x1024 JPEGs of the JPEG-only folder, annotated: 4 persons per frame
        rel = f"TS1/img_{i:06d}.jpg"
        os.symlink(os.path.realpath(os.path.join(jpg, f"im{i:05d}.jpg")), os.path.join(root, rel))
        bodys = np.zeros((4, 15, 11))
        bodys[:, :, 0] = rng.uniform(0, 1664, (4, 1)) + rng.normal(0, 60, (4, 15))
        bodys[:, :, 1] = rng.uniform(0, 1024, (4, 1)) + rng.normal(0, 60, (4, 15))
        bodys[:, :, 2] = rng.uniform(200, 500, (4, 15))
        bodys[:, :, 3] = 2
        bodys[:, :, 4:7] = rng.normal(0, 60, (4, 15, 3)) + np.array([0, 0, 300])
        bodys[:, :, 7:11] = [1500.0, 1490.0, 832.0, 512.0]
        entries.append({"dataset": "MUCO", "img_paths": rel, "img_width": 1664, "img_height": 1024, "isValidation": 1, "bodys": bodys.tolist()})
    with open(os.path.join(root, "M3E_gt.json"), "w") as f:
        json.dump({"root": entries}, f)
    dp = ["--device_preprocess", "1"]
    legs = [("host loader (get_test_loader: PIL + numpy resize in the consumer's thread, fp32 upload)", []),
            ("--device_preprocess 1", dp), ("--device_preprocess 1 --device_decode 1", dp + ["--device_decode", "1"]),
            ("--device_preprocess 1 --device_decode 2", dp + ["--device_decode", "2"])]
    cases = [("warm-up (builds the plan cache; not counted)", dp)] + [leg for _ in range(args.pairs) for leg in legs]
    trees = {}
    if args.only == "maps":
        dd = dp + ["--device_decode", "1"]
        legs = [("--eval_3d 1", dd), ("--eval_3d 1 --eval_maps 1", dd + ["--eval_maps", "1"])]
        if args.parent:
            legs.append(("parent commit, --eval_3d 1", dd))
            trees["parent commit, --eval_3d 1"] = os.path.abspath(args.parent)
        cases = [("warm-up (builds the plan cache; not counted)", dd)] + [leg for _ in range(args.pairs) for leg in legs]
    runs, first = [], None
    for name, extra in cases:
        tree = trees.get(name, ROOT)
        timing = os.path.join(tmp, "timing.json")
        env = dict(os.environ, PROJECT_HOME=tmp, PYTHONPATH=tree + os.pathsep + os.environ.get("PYTHONPATH", ""), SMAP_CLI_TIMING=timing,
                   SMAP_PLAN_CACHE=os.path.join(tmp, "plan_cache"), SMAP_TEST_ROOT=root)
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, os.path.join(tree, "exps", "stage3_root2", "test.py"), "-p", os.path.join(tmp, "SMAP.pth"),
                            "-t", "generate_result", "-d", "test", "--eval_3d", "1", "--batch_size", str(args.batch), "--json_name", "gt"] + extra,
                           capture_output=True, text=True, env=env, cwd=tmp, timeout=1500)
        rec = {"case": name, "returncode": r.returncode, "process_wall_s": time.perf_counter() - t0}
        if r.returncode == 0 and os.path.exists(timing):
            rec.update(json.load(open(timing)))
            os.remove(timing)
            res = json.load(open(os.path.join(tmp, "model_logs", "stage3_root2", "result", "stage3_root2_generate_result_test_gt.json")))
            rec["records_in_result_file"] = len(res["3d_pairs"])
            rec["error_keys"] = len(res.get("error", {}))
            for k in ("count_gt", "count_pred", "distance_e", "distance_d", "reverse_count", "count_pred_bone"):
                res.get("error", {}).pop(k, None)                 # (--only maps: the flag adds these six keys and nothing else)
            if first is None:
                first = res
            rec["same_result_file_as_first_run"] = res == first
        else:
            rec["stderr_tail"] = r.stderr[-1500:]
        runs.append(rec)
        print(json.dumps(rec), flush=True)
    summary = {}
    for rec in runs[1:]:
        if rec.get("frames_per_s_after_engine_build"):
            summary.setdefault(rec["case"], []).append(rec["frames_per_s_after_engine_build"])
    if args.only == "maps":
        out = {"images": args.images, "batch_size": args.batch, "mode": "-t generate_result -d test --eval_3d 1 --device_preprocess 1 --device_decode 1",
               "sources": "the bench's 8 frames as 1664x1024 JPEG q98 4:4:4 (pixel-doubled), annotated with 4 persons each",
               "host_cpus_allowed": len(os.sched_getaffinity(0)), "gpu": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
               "repetitions_interleaved": args.pairs, "runs": runs,
               "summary_frames_per_s_after_engine_build": {k: {"mean": float(np.mean(v)), "min": min(v), "max": max(v), "runs": v}
                                                           for k, v in summary.items()},
               "smap_evalmaps_update_device_events": update_us("maps")}
        print(json.dumps(out["summary_frames_per_s_after_engine_build"], indent=1))
        print(json.dumps(out["smap_evalmaps_update_device_events"], indent=1))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)
        print("wrote", args.out)
        return
    out = {"images": args.images, "batch_size": args.batch, "mode": "-t generate_result -d test --eval_3d 1",
           "sources": "the bench's 8 frames as 1664x1024 JPEG q98 4:4:4 (pixel-doubled), annotated with 4 persons each",
           "host_cpus_allowed": len(os.sched_getaffinity(0)), "gpu": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
           "repetitions_interleaved": args.pairs, "runs": runs,
           "summary_frames_per_s_after_engine_build": {k: {"mean": float(np.mean(v)), "min": min(v), "max": max(v), "runs": v}
                                                       for k, v in summary.items()},
           "preprocess_8_frames_1080p": preprocess_launch_ab()}
    print(json.dumps(out["summary_frames_per_s_after_engine_build"], indent=1))
    print(json.dumps(out["preprocess_8_frames_1080p"], indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "cli_e2e.json"))
    ap.add_argument("--only", choices=["", "jpeg", "huffman", "gt", "maps", "scorers"], default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--parent", default="", help="--only maps / scorers: a built checkout of the parent commit, run as a further leg")
    ap.add_argument("--scorers_child", default="", help=argparse.SUPPRESS)       # one repeat of --only scorers on the package of that tree
    args = ap.parse_args()
    if args.scorers_child:
        sys.path.insert(0, args.scorers_child)
        import smap_amd
        assert os.path.realpath(os.path.dirname(os.path.dirname(smap_amd.__file__))) == os.path.realpath(args.scorers_child)
        print(json.dumps({"3d": update_us("3d"), "maps": update_us("maps")}))
        return
    if args.only == "scorers":
        return scorers_leg(args)
    from PIL import Image
    from benchkit.workload import make_cfg, people_state_dict
    from smap_amd.model.smap import SMAP
    tmp = tempfile.mkdtemp(prefix="smap_cli_e2e_")
    enc, raw, jpg = os.path.join(tmp, "encoded"), os.path.join(tmp, "npy"), os.path.join(tmp, "jpg")
    os.makedirs(enc), os.makedirs(raw), os.makedirs(jpg)
    from exps.stage3_root2.config import cfg as run_cfg
    t0 = time.perf_counter()
    base = bench_frames_as_images(list(run_cfg.INPUT.MEANS), list(run_cfg.INPUT.STDS))
    sizes = []
    # two source resolutions: 832x512 (no resize) as PNG, and 1664x1024 = every pixel doubled (the 2x shrink of the pre-processing is the
    # 2x2 box mean: it returns the original frame) as JPEG quality 98 (4:4:4); 8 + 8 files are written, the rest of the folder links to them
    written = {}
    for i in range(args.images):
        f, big = i % 8, (i // 8) % 2
        ext = "jpg" if big else "png"
        if (f, big) not in written:
            img = base[f] if not big else np.repeat(np.repeat(base[f], 2, axis=0), 2, axis=1)
            path = os.path.join(enc, f"src_{f}_{big}.{ext}.data")
            if big:
                Image.fromarray(img[:, :, ::-1]).save(path, format="JPEG", quality=98, subsampling=0)      # 4:4:4: the frame comes back within 0.6 grey levels
            else:
                Image.fromarray(img[:, :, ::-1]).save(path, format="PNG", compress_level=1)
            npy = os.path.join(tmp, f"src_{f}_{big}.npy")          # (outside the folder: the loader lists every *.npy below it)
            np.save(npy, img)
            written[(f, big)] = (path, npy)
            sizes.append(os.path.getsize(path))
        os.symlink(written[(f, big)][0], os.path.join(enc, f"im{i:05d}.{ext}"))
        os.symlink(written[(f, big)][1], os.path.join(raw, f"im{i:05d}.npy"))
    for i in range(args.images):                                    # the JPEG-only folder: the 8 1664x1024 JPEGs, round robin
        os.symlink(written[(i % 8, 1)][0], os.path.join(jpg, f"im{i:05d}.jpg"))
    gen_s = time.perf_counter() - t0
    torch.manual_seed(0)
    net = SMAP(make_cfg((128, 208))).eval()
    sd = people_state_dict(net.state_dict(), "smooth")
    torch.save({"model": sd}, os.path.join(tmp, "SMAP.pth"))
    if args.only in ("gt", "maps"):
        return gt_leg(args, tmp, jpg)
    runs = []
    cases = [("encoded jpg/png, GPU pre-processing, 16 decode threads (default)", enc, ["--device_preprocess", "1"], {}),
             ("encoded jpg/png, GPU pre-processing, 8 decode threads", enc, ["--device_preprocess", "1"], {"SMAP_DECODE_THREADS": "8"}),
             ("encoded jpg/png, GPU pre-processing, 32 decode threads", enc, ["--device_preprocess", "1"], {"SMAP_DECODE_THREADS": "32"}),
             ("encoded jpg/png, GPU pre-processing, 16 decode PROCESSES (SMAP_DECODE_PROCS)", enc, ["--device_preprocess", "1"], {"SMAP_DECODE_PROCS": "16"}),
             ("encoded jpg/png, GPU pre-processing, 32 decode PROCESSES", enc, ["--device_preprocess", "1"], {"SMAP_DECODE_PROCS": "32"}),
             ("encoded jpg/png, GPU pre-processing, ONE decode thread (round-4 loader)", enc, ["--device_preprocess", "1"], {"SMAP_DECODE_THREADS": "1"}),
             (".npy frames (no decoder), GPU pre-processing", raw, ["--device_preprocess", "1"], {}),
             ("encoded jpg/png, host pre-processing (the reference's DataLoader path), first 128 images", enc + "_few", [], {})]
    dd = ["--device_preprocess", "1", "--device_decode", "1"]
    jpeg_cases = [("1664x1024 JPEG only, PIL, 16 decode threads", jpg, ["--device_preprocess", "1"], {"SMAP_DECODE_THREADS": "16"}),
                  ("1664x1024 JPEG only, PIL, 16 decode PROCESSES (SMAP_DECODE_PROCS)", jpg, ["--device_preprocess", "1"], {"SMAP_DECODE_PROCS": "16"}),
                  ("1664x1024 JPEG only, --device_decode 1 (host Huffman decode, default threads; IDCT / colour on the GPU)", jpg, dd, {}),
                  (".npy frames (no decoder), GPU pre-processing", raw, ["--device_preprocess", "1"], {})]
    cases = jpeg_cases if args.only == "jpeg" else cases + jpeg_cases[:3]
    if args.only == "huffman":
        cases = [("warm-up (builds the plan cache; not counted)", jpg, dd, {"SMAP_DECODE_THREADS": "16"})]
        for threads in ("16", "2"):
            for _ in range(args.pairs):
                for mode in ("1", "2"):
                    cases.append((f"1664x1024 JPEG only, --device_decode {mode}, {threads} decode threads", jpg,
                                  ["--device_preprocess", "1", "--device_decode", mode], {"SMAP_DECODE_THREADS": threads}))
    os.makedirs(enc + "_few")
    for n in sorted(os.listdir(enc)):
        if n.startswith("im") and int(n[2:7]) < 128:
            os.symlink(os.path.realpath(os.path.join(enc, n)), os.path.join(enc + "_few", n))
    for name, folder, extra, env_extra in cases:
        timing = os.path.join(tmp, "timing.json")
        # the plan cache of this run lives in the temporary folder: the FIRST case builds the schedules (first_submit_s = seconds of weight
        # packing), every later case is a "second start" that loads them through smap_plan_create_from_blob
        env = dict(os.environ, PROJECT_HOME=tmp, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), SMAP_CLI_TIMING=timing,
                   SMAP_PLAN_CACHE=os.path.join(tmp, "plan_cache"), **env_extra)
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "exps", "stage3_root2", "test.py"), "-p", os.path.join(tmp, "SMAP.pth"),
                            "-t", "run_inference", "-d", "test", "--batch_size", str(args.batch), "--dataset_path", folder, "--json_name", "e2e"] + extra,
                           capture_output=True, text=True, env=env, cwd=tmp, timeout=1500)
        wall = time.perf_counter() - t0
        rec = {"case": name, "returncode": r.returncode, "process_wall_s": wall, "plan_cache": "cold (schedules built and stored)" if not runs else "warm (second start)"}
        if r.returncode == 0 and os.path.exists(timing):
            rec.update(json.load(open(timing)))
            out = os.path.join(tmp, "model_logs", "stage3_root2", "result", "stage3_root2_run_inference_test_e2e.json")
            res = json.load(open(out))
            rec["records_in_result_file"] = len(res["3d_pairs"])
            rec["result_file_MB"] = os.path.getsize(out) / 1e6
        else:
            rec["stderr_tail"] = r.stderr[-1500:]
        runs.append(rec)
        print(json.dumps(rec), flush=True)
    out = {"images": args.images, "batch_size": args.batch, "sources": "the bench's 8 frames: 832x512 PNG and 1664x1024 JPEG q98 4:4:4 (pixel-doubled), alternating in groups of 8",
           "mean_file_KB": float(np.mean(sizes)) / 1e3, "generation_s": gen_s, "host_cpus_allowed": len(os.sched_getaffinity(0)),
           "gpu": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "runs": runs}
    if args.only == "huffman":
        legs = {}
        for rec in runs[1:]:
            if rec.get("frames_per_s_after_engine_build"):
                legs.setdefault(rec["case"], []).append(rec["frames_per_s_after_engine_build"])
        out["summary_frames_per_s"] = {k: {"mean": float(np.mean(v)), "min": min(v), "max": max(v), "runs": v} for k, v in legs.items()}
        print(json.dumps(out["summary_frames_per_s"], indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
