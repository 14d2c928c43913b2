#!/usr/bin/env python3
"""Host cost of a 1664x1024 JPEG frame, CPU only: PIL's whole decode + BGR pack (dataset.decode.read_bgr, what the loader runs today)
against the host half of `--device_decode 1` (smap_amd/jpeg.py: native marker parse + Huffman decode into int16 coefficients; the
IDCT, upsampling and colour conversion then run on the GPU).  One thread, and 16 threads over the same frames (ms per frame of wall time).

Two sets: the 8 JPEGs tools/cli_e2e.py writes (the bench's frames pixel-doubled, quality 98, 4:4:4) and a photo-like set (smooth
gradients with mild noise, quality 90, 4:2:0).

    python tools/bench_jpeg.py [--reps 5] [--threads 16] [--out file.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from dataset.decode import read_bgr
    from smap_amd import jpeg as J

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
