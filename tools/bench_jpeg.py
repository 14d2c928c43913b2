#!/usr/bin/env python3
"""Host cost of a 1664x1024 JPEG frame, CPU only: PIL's whole decode + BGR pack (dataset.decode.read_bgr, what the loader runs today)
against the host half of `--device_decode 1` (smap_amd/jpeg.py: native marker parse + Huffman decode into int16 coefficients; the
IDCT, upsampling and colour conversion then run on the GPU).  One thread, and 16 threads over the same frames (ms per frame of wall time).

Two sets: the 8 JPEGs tools/cli_e2e.py writes (the bench's frames pixel-doubled, quality 98, 4:4:4) and a photo-like set (smooth
gradients with mild noise, quality 90, 4:2:0).

    python tools/bench_jpeg.py [--reps 5] [--threads 16] [--out file.json]

`--device_huffman 1` (needs the GPU) measures `--device_decode 2` on the same two sets instead: the host's share per frame (marker parse
+ smap_jpeg_scan_tables + the copy into one page-locked buffer, process time of one thread), the bytes a frame uploads in either mode,
and the GPU time per frame of smap_jpeg_decode_coefficients_device between two stream events for every `--subseq` x `--rounds` asked
for, with the status words (a configuration that does not converge on every frame says so).  `--trace_only 1` only runs the shipped
defaults once per frame after a warm-up: the run to put under `rocprofv3 --kernel-trace --stats` for per-kernel times.
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402


def cli_e2e_frames():
    from PIL import Image
    from cli_e2e import bench_frames_as_images
    from exps.stage3_root2.config import cfg
    out = []
    for img in bench_frames_as_images(list(cfg.INPUT.MEANS), list(cfg.INPUT.STDS)):
        big = np.repeat(np.repeat(img, 2, axis=0), 2, axis=1)
        b = io.BytesIO()
        Image.fromarray(big[:, :, ::-1]).save(b, format="JPEG", quality=98, subsampling=0)
        out.append(b.getvalue())
    return out


def photo_like_frames(n=8):
    from PIL import Image
    out = []
    yy, xx = np.mgrid[0:1024, 0:1664].astype(np.float64)
    for i in range(n):
        rng = np.random.default_rng(i)
        ch = [127.5 + 100 * np.sin(xx / (150 + 40 * k + 10 * i) + yy / (230 - 30 * k) + i) for k in range(3)]
        img = np.stack(ch, -1) + rng.normal(0, 4, (1024, 1664, 3))
        b = io.BytesIO()
        Image.fromarray(np.clip(img, 0, 255).round().astype(np.uint8)).save(b, format="JPEG", quality=90)
        out.append(b.getvalue())
    return out


def timed(fn, frames, reps, threads):
    """ms of wall time per frame: `reps` passes over the frames, one thread or a pool of `threads`."""
    fn(frames[0])
    work = frames * reps
    t0 = time.perf_counter()
    if threads == 1:
        for f in work:
            fn(f)
    else:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(fn, work))
    return 1e3 * (time.perf_counter() - t0) / len(work)


def device_huffman(args, sets):
    import torch
    from smap_amd import jpeg as J
    dev = torch.device("cuda:0")
    res = {"subseq": args.subseq, "rounds": args.rounds, "reps": args.reps, "sets": {}}
    for name, frames in sets:
        infos = [J.probe(f) for f in frames]
        t0 = time.process_time()
        for _ in range(args.reps):
            packed = [J.pack_frame(f, i) for f, i in zip(frames, infos)]
        r = {"mean_file_KB": float(np.mean([len(f) for f in frames])) / 1e3,
             "host_probe_tables_pack_ms": 1e3 * (time.process_time() - t0) / (args.reps * len(frames)) + 1e3 * _probe_s(J, frames),
             "h2d_bytes_mode1": float(np.mean([i.coef_bytes for i in infos])),
             "h2d_bytes_mode2": float(np.mean([p.numel() for p in packed])), "runs": []}
        want = [J.decode_coefficients(f, i, pin=False) for f, i in zip(frames, infos)]
        if args.trace_only:
            for _ in range(2):
                for p, i in zip(packed, infos):
                    J.decode_coefficients_device(p, i, None, dev)
                torch.cuda.synchronize()
            res["sets"][name] = r
            continue
        for subseq in args.subseq:
            for rounds in args.rounds:
                outs = [J.decode_coefficients_device(p, i, None, dev, subseq, rounds) for p, i in zip(packed, infos)]    # warm-up + check
                status = [int(st.item()) for _, st in outs]
                equal = all(torch.equal(co.cpu(), w) for (co, _), w, st in zip(outs, want, status) if st == 0)
                ups = [p.to(dev) for p in packed]
                torch.cuda.synchronize()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                for _ in range(args.reps):
                    for p, i in zip(ups, infos):                                  # (already on the device: the launches alone)
                        J.decode_coefficients_device(p, i, None, dev, subseq, rounds)
                ev[1].record()
                torch.cuda.synchronize()
                run = {"subseq_bytes": subseq, "rounds": rounds, "status": status, "equal_where_status_0": bool(equal),
                       "gpu_ms_per_frame": ev[0].elapsed_time(ev[1]) / (args.reps * len(frames))}
                r["runs"].append(run)
                print(name, json.dumps(run), flush=True)
        res["sets"][name] = r
        print(name, json.dumps({k: v for k, v in r.items() if k != "runs"}), flush=True)
    return res


def _probe_s(J, frames):
    t0 = time.process_time()
    for f in frames:
        J.probe(f)
    return (time.process_time() - t0) / len(frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device_huffman", type=int, default=0)
    ap.add_argument("--trace_only", type=int, default=0)
    ap.add_argument("--subseq", type=int, nargs="+", default=[0])
    ap.add_argument("--rounds", type=int, nargs="+", default=[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from dataset.decode import read_bgr
    from smap_amd import jpeg as J
    if args.device_huffman:
        res = device_huffman(args, (("cli_e2e 1664x1024 q98 4:4:4", cli_e2e_frames()), ("photo-like 1664x1024 q90 4:2:0", photo_like_frames())))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(res, open(args.out, "w"), indent=1)
        return

    def pil(data):
        return read_bgr(io.BytesIO(data))

    def native(data):
        info = J.probe(data)
        return J.decode_coefficients(data, info, pin=False)
    res = {"threads": args.threads, "reps": args.reps, "cpus_allowed": len(os.sched_getaffinity(0)), "sets": {}}
    for name, frames in (("cli_e2e 1664x1024 q98 4:4:4", cli_e2e_frames()), ("photo-like 1664x1024 q90 4:2:0", photo_like_frames())):
        assert all(J.probe(f) is not None for f in frames)
        r = {"mean_file_KB": float(np.mean([len(f) for f in frames])) / 1e3}
        for t in (1, args.threads):
            r[f"pil_decode_bgr_ms_{t}t"] = timed(pil, frames, args.reps, t)
            r[f"native_entropy_decode_ms_{t}t"] = timed(native, frames, args.reps, t)
        r["native_over_pil_1t"] = r["native_entropy_decode_ms_1t"] / r["pil_decode_bgr_ms_1t"]
        res["sets"][name] = r
        print(name, json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
