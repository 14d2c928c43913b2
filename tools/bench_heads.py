#!/usr/bin/env python3
"""Time the head arms of one Upsample_unit in fp32 (smap_amd/heads.py: smap_heads_forward, smap_heads_backward) against the same unit
in plain torch fp32 on the device (F.conv2d + autograd: the comparison path), and a whole HeadFineTuner.step.

    python tools/bench_heads.py [--iters 50] [--warmup 5] [--out profiles/heads_bench.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_heads.py --calls-only --iters 20 --warmup 3
    python tools/bench_heads.py --reduce-trace DIR/.../*_kernel_trace.csv --iters 20 --warmup 3 [--out profiles/heads_bench.json]

Cases: the four levels of the full network (16x26 ... 128x208) at B = 2 and B = 8, chl = 256, C = (43, 14, 1), X as the x3 engine
leaves it (fp16 hi|lo planes), heads dense NCHW.
  device_ms   HIP events around every iteration (median, min, max over --iters after --warmup), workspaces allocated outside.
  tflops      the multiply-adds the call needs by its shapes (2 flops each, below) over the median; beside it the 122 TF/s that
              cdna_hip_programming.md quotes for an untuned LDS-tiled 4096^3 GEMM on the same instruction.
  launches    (--reduce-trace, a run of its own under rocprofv3) per launch of a call its median duration and rate.  The trace lists
              kernels in start order; a --calls-only run issues, per case, (warmup + iters) forward calls of 4 launches and then as many
              backward calls of 13, so the k-th launch of every call is known by position.
  step        HeadFineTuner.step on the full network (512 x 832 images): the all-heads x3 engine, twelve units' arms forward and
              backward, the loss, Adam -- wall time per step with one synchronisation at the end of the loop.
Recorded, not gated."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_common import DEV, full_network_batch, read_json, reduce_positional_trace, stats, time_loop, write_merged  # noqa: E402
from smap_amd import finetune as FT  # noqa: E402
from smap_amd import gemm_f32 as G  # noqa: E402
from smap_amd import heads as H  # noqa: E402

CHL, ARM_C = 256, (43, 14, 1)
LEVELS = ((16, 26), (32, 52), (64, 104), (128, 208))
BATCHES = (2, 8)
GUIDE_TFLOPS = 122.0
FORWARD_LAUNCHES = ["Z|M"] + ["Y_%d" % a for a in range(3)]
BACKWARD_LAUNCHES = ["Z|M"] + [n % a for a in range(3) for n in ("gW2_%d part", "gW2_%d fold", "gZ_%d")] + ["gW1 part", "gW1 fold", "gX"]
KERNELS = ("conv_gemm_kernel", "reduce_gemm_kernel", "reduce_fold_kernel")


def launch_flops(B, h, w):
    """Multiply-adds * 2 of every launch by its shapes (a fold launch adds `slices` numbers per output: counted as that)."""
    P, c = B * h * w, CHL
    slices = H.workspace_layout(B, h, w, c, True)["slices"]
    f = {"Z|M": 2 * P * c * 3 * c, "gW1 part": 2 * P * 3 * c * c, "gX": 2 * P * 3 * c * c, "gW1 fold": slices * 3 * c * c}
    for a, ca in enumerate(ARM_C):
        f["Y_%d" % a] = f["gZ_%d" % a] = f["gW2_%d part" % a] = 2 * P * 9 * c * ca
        f["gW2_%d fold" % a] = slices * 9 * c * ca
    return f


def make_unit(B, h, w, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rand = lambda *shape: torch.randn(shape, generator=g, device=DEV)
    x = torch.relu(rand(B, h, w, CHL))
    hi = x.half()
    planes = torch.stack([hi, (x - hi.float()).half()], dim=3).contiguous()
    w1cat, b1cat = rand(3 * CHL, CHL) * (2.0 / CHL) ** 0.5, rand(3 * CHL) * 0.1
    w2 = [rand(c, CHL, 3, 3) * (2.0 / (9 * CHL)) ** 0.5 for c in ARM_C]
    b2 = [rand(c) * 0.1 for c in ARM_C]
    gs = [rand(B, c, h, w) * 1e-6 for c in ARM_C]
    return planes, w1cat, b1cat, w2, b2, gs


def bench_case(B, h, w, iters, warmup, calls_only):
    print("case B %d level %d x %d" % (B, h, w), file=sys.stderr, flush=True)
    planes, w1cat, b1cat, w2, b2, gs = make_unit(B, h, w)
    ys = [torch.empty((B, c, h, w), dtype=torch.float32, device=DEV) for c in ARM_C]
    ws_f, ws_b = (G.new_workspace(H.workspace_bytes(B, h, w, CHL, backward), DEV) for backward in (False, True))
    ysrc, gsrc = [H.nchw_source(y) for y in ys], [H.nchw_source(g) for g in gs]
    fl = launch_flops(B, h, w)
    case = dict(B=B, level=[h, w], pixels=B * h * w)
    fwd, _ = time_loop(lambda: H.forward(planes, w1cat, b1cat, w2, b2, ysrc, ws=ws_f), iters, warmup)
    bwd, _ = time_loop(lambda: H.backward(planes, w1cat, b1cat, w2, gsrc, ws=ws_b), iters, warmup)
    case["smap_heads_forward"] = stats(fwd, flops=sum(fl[k] for k in FORWARD_LAUNCHES), guide_tflops=GUIDE_TFLOPS)
    case["smap_heads_backward"] = stats(bwd, flops=sum(fl[k] for k in BACKWARD_LAUNCHES), guide_tflops=GUIDE_TFLOPS)
    if calls_only:
        return case
    # the comparison path: the same unit in torch fp32, NCHW, conv2d + autograd (forward alone; forward + backward to all gradients)
    xt = (planes[..., 0, :].float() + planes[..., 1, :].float()).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    leaves = [xt, w1cat.view(3 * CHL, CHL, 1, 1).clone().requires_grad_(True), b1cat.clone().requires_grad_(True)]
    leaves += [t.clone().requires_grad_(True) for t in w2 + b2]

    def torch_forward():
        m = torch.relu(F.conv2d(leaves[0], leaves[1], leaves[2]))
        return [F.conv2d(m[:, a * CHL:(a + 1) * CHL], leaves[3 + a], leaves[6 + a], padding=1) for a in range(3)]

    def torch_forward_only():
        with torch.no_grad():
            torch_forward()

    def torch_both():
        for t in leaves:
            t.grad = None
        torch.autograd.backward(torch_forward(), gs)
    case["torch_forward"] = stats(time_loop(torch_forward_only, iters, warmup)[0])
    case["torch_forward_backward"] = stats(time_loop(torch_both, iters, warmup)[0])
    case["ours_forward_backward_ms"] = case["smap_heads_forward"]["device_ms_median"] + case["smap_heads_backward"]["device_ms_median"]
    got = H.backward(planes, w1cat, b1cat, w2, gsrc, ws=ws_b)
    torch_both()
    # relative L2 per tensor, and beside it the count of Z elements on whose SIGN the two fp32 evaluation orders disagree (ours: M > 0 in the
    # workspace): each such element switches an element of gZ on or off in one of the two, which no rounding argument covers
    with torch.no_grad():
        theirs = torch.relu(F.conv2d(leaves[0], leaves[1], leaves[2])).permute(0, 2, 3, 1) > 0
    ours = H.workspace_views(ws_b, B, h, w, CHL)["m"].flatten(3) > 0
    case["relu_sign_disagreements_with_torch"] = int((ours != theirs).sum())
    case["z_elements"] = int(ours.numel())
    rel = lambda a, b: float((a - b).double().norm() / b.double().norm().clamp_min(1e-300))
    case["max_gradient_relative_l2_difference_to_torch"] = max(
        [rel(got[0], leaves[1].grad.view(3 * CHL, CHL)), rel(got[1], leaves[2].grad), rel(got[4], leaves[0].grad.permute(0, 2, 3, 1))]
        + [rel(got[2][a], leaves[3 + a].grad) for a in range(3)] + [rel(got[3][a], leaves[6 + a].grad) for a in range(3)])
    return case


def bench_step(B, iters, warmup):
    print("step B %d" % B, file=sys.stderr, flush=True)
    net, cfg, batch = full_network_batch(B)
    tuner = FT.HeadFineTuner(net, cfg, lr=1e-6, weight_decay=8e-6)
    step = lambda: tuner.step(*batch)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return dict(B=B, images=[512, 832], iters=iters, wall_ms_per_step=(time.perf_counter() - t0) * 1e3 / iters,
                peak_memory_gib=torch.cuda.max_memory_allocated() / 2 ** 30)


def reduce_trace(path, iters, warmup):
    """Per case the median duration and rate of every launch, from a kernel trace of a --calls-only run with the same --iters / --warmup."""
    def case(B, h, w):
        fl = launch_flops(B, h, w)
        rate = lambda name, med: dict(flops=int(fl[name]), tflops=fl[name] / (med * 1e-6) / 1e12,
                                      share_of_guide_untuned_gemm=fl[name] / (med * 1e-6) / 1e12 / GUIDE_TFLOPS)
        return dict(B=B, level=[h, w]), [("smap_heads_forward", FORWARD_LAUNCHES, 0), ("smap_heads_backward", BACKWARD_LAUNCHES, 0)], rate
    return reduce_positional_trace(path, KERNELS, [case(B, h, w) for B in BATCHES for h, w in LEVELS], iters + warmup, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--calls-only", action="store_true", help="time the two C calls alone (for a kernel trace); writes no file without --out")
    ap.add_argument("--reduce-trace", metavar="CSV", help="add per-launch figures from a rocprofv3 kernel trace of a --calls-only run to --out")
    ap.add_argument("--out", default=None, help="default: profiles/heads_bench.json (none with --calls-only)")
    args = ap.parse_args()
    default = os.path.join(ROOT, "profiles", "heads_bench.json")
    if args.reduce_trace:
        path = args.out or default
        out = read_json(path)
        out["launches"] = dict(what="rocprofv3 --kernel-trace over `tools/bench_heads.py --calls-only` (a run of its own), reduced by --reduce-trace",
                               iters=args.iters, warmup=args.warmup, cases=reduce_trace(args.reduce_trace, args.iters, args.warmup))
        json.dump(out, open(path, "w"), indent=1)
        return print(json.dumps(out["launches"], indent=1))
    if args.out is None and not args.calls_only:
        args.out = default
    out = dict(gpu=torch.cuda.get_device_name(0), chl=CHL, arm_channels=ARM_C, x_layout="fp16 hi|lo planes", iters=args.iters, warmup=args.warmup,
               guide_untuned_f32_mfma_gemm_tflops=GUIDE_TFLOPS,
               what="device_ms: HIP events around each iteration of one call.  tflops: flops by shape over the median.  torch_*: the same unit "
                    "as F.conv2d + autograd in fp32 on the device (the comparison path).  step: HeadFineTuner.step on the full network, wall time",
               cases=[bench_case(B, h, w, args.iters, args.warmup, args.calls_only) for B in BATCHES for h, w in LEVELS])
    if not args.calls_only:
        out["step"] = [bench_step(B, args.step_iters, 2) for B in BATCHES]
    if args.out:
        write_merged(out, args.out)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
