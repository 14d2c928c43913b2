#!/usr/bin/env python3
"""Time the training loss from native-resolution heads (smap_amd/loss.py SMAPLossNative: smap_loss_forward_src + smap_loss_backward_src)
against the same job on the upsampled route: 36 F.interpolate calls on the device, SMAPLoss forward + backward, autograd's interpolate
backward.

    python tools/bench_lossgrad.py [--iters 200] [--warmup 20] [--out profiles/lossgrad_bench.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_lossgrad.py --native-only --iters 50 --warmup 5
    python tools/bench_lossgrad.py --reduce-trace DIR/.../*_kernel_trace.csv [--trace-out profiles/lossgrad_kernel_trace.json]

Cases: B = 2 and B = 8 at 128 x 208 maps, heads of 16x26, 32x52, 64x104 and 128x208 per stage, 3 stages, OHKM (topk 8), coarse-to-fine, 5
label scales, 20 root-depth rows per frame of which 6 are persons.  Both routes start from the same 36 native leaves and end with their
36 .grad tensors; per route forward + backward:
  device_ms   HIP events around every iteration (median, min, max, mean over --iters after --warmup);
  wall_ms     time.perf_counter around the whole loop with one synchronisation at its end, / iters.
The bytes the two new launches move BY DESIGN are stated over the launches' own median durations from a kernel
trace, in a run of its own: `--native-only` times the native route alone, `--reduce-trace` (no GPU needed) reduces the trace's CSV."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_common import stats, time_loop  # noqa: E402
from smap_amd import loss as K  # noqa: E402

DEV = "cuda:0"
H, W, S, R, STAGES, TOPK = 128, 208, 5, 20, 3, 8
SIZES = ((16, 26), (32, 52), (64, 104), (128, 208))
KEYS = (("heatmap_2d", K.N2D), ("det_d", K.NDD), ("root_d", 1))


def design_bytes(B):
    """(part, fold): bytes the two launches of smap_loss_backward_src move by design.  Channels with a factor: all 57 of a head below the
    finest, 4 * topk of a finest head.  part reads those channels' label planes once and their source planes once, writes four partial
    sums per interval of a source below H x W, and for a source of H x W every gradient plane; root_d planes are zeroed.  fold reads the
    partial sums and writes every gradient plane of the sources below H x W."""
    part = fold = 0
    for h in range(4 * STAGES):
        sh, sw = SIZES[h % 4]
        live = 4 * TOPK if h % 4 == 3 else K.NC
        part += B * live * H * W * 4 + B * live * sh * sw * 4 + B * sh * sw * 4
        if (sh, sw) == (H, W):
            part += B * K.NC * H * W * 4
        else:
            part += B * live * sh * sw * 16
            fold += B * live * sh * sw * 16 + B * K.NC * sh * sw * 4
    return part, fold


def reduce_trace(path, out_path):
    """rocprofv3's *_kernel_trace.csv of a `--native-only` run -> per new launch and batch size its durations and bytes by design / s."""
    import csv
    durations = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        kind = "part" if "loss_backward_src_part" in name else "fold" if "loss_backward_src_fold" in name else None
        if kind is None:
            continue
        B = int(r["Grid_Size_Y"]) // max(1, int(r["Workgroup_Size_Y"]))
        durations.setdefault((kind, B), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = dict(what="rocprofv3 --kernel-trace over `python tools/bench_lossgrad.py --native-only` (a run of its own), reduced by "
                    "`tools/bench_lossgrad.py --reduce-trace`: duration of the two launches of smap_loss_backward_src per batch size, and "
                    "the bytes a launch moves by design over its median duration", map=[H, W], kernels={})
    for (kind, B), ns in sorted(durations.items()):
        need = design_bytes(B)[0 if kind == "part" else 1]
        med = float(np.median(ns)) / 1e3
        out["kernels"]["%s_B%d" % (kind, B)] = dict(calls=len(ns), median_us=med, min_us=min(ns) / 1e3, max_us=max(ns) / 1e3, bytes=need,
                                                    gb_per_s=need / (med * 1e-6) / 1e9)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


def make_inputs(B, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rand = lambda *shape: torch.randn(shape, generator=g, device=DEV)
    labels = rand(B, S, K.NC, H, W)
    native = {key: [[rand(B, ch, *SIZES[j]).requires_grad_(True) for j in range(4)] for _ in range(STAGES)] for key, ch in KEYS}
    rdepth = torch.zeros((B, R, 3), device=DEV)
    rows = np.random.RandomState(seed)
    for b in range(B):
        for r in range(6):
            rdepth[b, r] = torch.tensor([rows.uniform(0, H - 1), rows.uniform(0, W - 1), rows.uniform(0.5, 5)])
    return native, torch.ones((B, K.NC, 1), device=DEV), labels, rdepth


def leaves(outputs):
    return [t for key in outputs for stage in outputs[key] for t in stage]


def upsampled(native):
    """What the reference's Upsample_unit does to every head before the loss."""
    up = lambda t: t if tuple(t.shape[2:]) == (H, W) else F.interpolate(t, size=(H, W), mode="bilinear", align_corners=True)
    return {key: [[up(t) for t in stage] for stage in native[key]] for key in native}


def bench_case(B, iters, warmup, native_only=False):
    native, valids, labels, rdepth = make_inputs(B)
    new, old = K.SMAPLossNative(STAGES, True, TOPK, True), K.SMAPLoss(STAGES, True, TOPK, True)

    def clear():
        for t in leaves(native):
            t.grad = None

    def native_step():
        clear()
        new(native, valids, labels, rdepth)["total_loss"].backward()

    def upsampled_step():
        clear()
        old(upsampled(native), valids, labels, rdepth)["total_loss"].backward()

    case = dict(B=B)
    case["native_forward_backward"] = stats(*time_loop(native_step, iters, warmup))
    if native_only:
        return case
    case["upsampled_forward_backward"] = stats(*time_loop(upsampled_step, iters, warmup))
    native_step()
    a = [t.grad.clone() for t in leaves(native)]
    upsampled_step()
    case["max_gradient_difference_relative"] = max(float((x - t.grad).abs().max() / t.grad.abs().max().clamp_min(1e-30))
                                                   for x, t in zip(a, leaves(native)))
    part, fold = design_bytes(B)
    case["part_bytes_by_design"], case["fold_bytes_by_design"] = part, fold
    for k in ("device_ms_median", "wall_ms"):
        case["speedup_" + k] = case["upsampled_forward_backward"][k] / case["native_forward_backward"][k]
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--native-only", action="store_true", help="time the native route alone (for a kernel trace); writes no file without --out")
    ap.add_argument("--out", default=None, help="default: profiles/lossgrad_bench.json (none with --native-only)")
    ap.add_argument("--reduce-trace", metavar="CSV", help="reduce a rocprofv3 kernel trace of a --native-only run; no GPU needed")
    ap.add_argument("--trace-out", default=os.path.join(ROOT, "profiles", "lossgrad_kernel_trace.json"))
    args = ap.parse_args()
    if args.reduce_trace:
        return reduce_trace(args.reduce_trace, args.trace_out)
    if args.out is None and not args.native_only:
        args.out = os.path.join(ROOT, "profiles", "lossgrad_bench.json")
    out = dict(gpu=torch.cuda.get_device_name(0), map=[H, W], head_sizes=SIZES, stages=STAGES, ohkm=True, topk=TOPK, coarse_to_fine=True,
               label_scales=S, rows_per_frame=R, persons_per_frame=6, iters=args.iters, warmup=args.warmup,
               what="forward + backward from the same 36 native leaves to their .grad.  native: SMAPLossNative (smap_loss_forward_src, "
                    "smap_loss_backward_src).  upsampled: 36 F.interpolate(bilinear, align_corners), SMAPLoss, autograd's interpolate "
                    "backward.  device_ms: HIP events around each iteration; wall_ms: perf_counter around the loop, one synchronisation "
                    "at its end",
               cases=[bench_case(B, args.iters, args.warmup, args.native_only) for B in (2, 8)])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
