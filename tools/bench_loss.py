#!/usr/bin/env python3
"""Time the fused training loss (smap_amd/loss.py) against the same loss written with plain torch operations on the device.

    python tools/bench_loss.py [--iters 200] [--warmup 20] [--out profiles/loss_bench.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_loss.py --fused-only --iters 50 --warmup 5
    python tools/bench_loss.py --reduce-trace DIR/.../*_kernel_trace.csv [--trace-out profiles/loss_kernel_trace.json]

Cases: B = 2 and B = 8 at 128 x 208 maps, 3 stages, OHKM (topk 8), coarse-to-fine, 5 label scales, 20 root-depth rows per frame of
which 6 are persons.  Per case and path, forward alone and forward + backward:
  device_ms   HIP events around every iteration (median, min, max, mean over --iters after --warmup);
  wall_ms     time.perf_counter around the whole loop with one synchronisation at its end, / iters -- this includes what the host
              waits for inside an iteration (the baseline's per-row `if z > 0` reads a device value on the host).
The baseline (`torch_loss`) is the arithmetic of DESIGN.md section 13 in torch calls: index_select for the label channels, mse_loss
without reduction, mean, topk, and a Python loop over the root-depth rows with one device read per row.
The fused path's achieved bytes/s are stated against the bytes each launch MUST move: forward reads every output and label plane
once (its time includes the one-workgroup finish); backward reads both planes of every channel whose factor is not zero and writes
every gradient once.  Clocks and power are sampled while the fused loops run (benchkit/clocks.py).
Events around an iteration cannot tell the launches apart, and at B = 2 the host, not the device, sets the pace.  The achieved bytes/s
of the reduction and of the backward launch THEMSELVES therefore come from a kernel trace: `--fused-only` times the fused path alone
(under rocprofv3, in a run of its own; it writes no file unless --out is given), and `--reduce-trace` (no GPU needed) reduces the
trace's CSV to per-launch durations per batch size and bytes / median duration.  A finish launch belongs to the batch size of the
reduction launch before it."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_common import stats, time_loop  # noqa: E402
from benchkit.clocks import ClockSampler  # noqa: E402
from smap_amd import loss as K  # noqa: E402

DEV = "cuda:0"
H, W, S, R, STAGES, TOPK = 128, 208, 5, 20, 3, 8


def torch_loss(outputs, valids, labels, rdepth, stage_num=STAGES, ohkm=True, topk=TOPK, ctf=True):
    """The loss with plain torch operations (the comparison; not used by the package)."""
    index = torch.tensor(K.LABEL_CHANNEL, device=labels.device)
    weight = (valids.reshape(valids.shape[0], -1) > 0).float()

    def joints(out, lab, w, hard, groups):
        per_channel = torch.nn.functional.mse_loss(out, lab, reduction="none").mean(dim=(2, 3)) * w
        if not hard:
            return per_channel.mean()
        return sum(torch.topk(per_channel[:, a:b], k=k, dim=1, sorted=False)[0].mean() for a, b, k in groups)

    def root(out):
        total, count = 0.0, 0
        for b in range(rdepth.shape[0]):
            for r in range(rdepth.shape[1]):
                if rdepth[b, r, 2] > 0:                                   # a device value read on the host, per row
                    total = total + torch.abs(out[b, 0, int(rdepth[b, r, 0]), int(rdepth[b, r, 1])] - rdepth[b, r, 2])
                    count += 1
        return total / count if count else out.sum() * 0

    total = l2 = l3 = lr = 0.0
    for i in range(stage_num):
        for j in range(4):
            lab = labels[:, j + (1 if i == stage_num - 1 and ctf else 0)].index_select(1, index)
            hard = ohkm and j == 3
            a = joints(outputs["heatmap_2d"][i][j], lab[:, :K.N2D], weight[:, :K.N2D], hard, ((0, 15, topk), (15, 43, 2 * topk)))
            b = joints(outputs["det_d"][i][j], lab[:, K.N2D:], weight[:, K.N2D:], hard, ((0, 14, topk),))
            c = root(outputs["root_d"][i][j])
            t = 0.1 * a + 5 * b + 10 * c
            if j == 3:
                l2, l3, lr = l2 + a, l3 + b, lr + c
            else:
                t = t / 4
            total = total + t
    return dict(total_loss=total, loss_2d=l2, loss_bone=l3, loss_root=lr)


def forward_bytes(B):
    """Bytes the reduction must read: every output plane of the 2D and depth heads and its label plane, once."""
    return 4 * STAGES * B * K.NC * H * W * 4 * 2


def backward_bytes(B):
    """Bytes the backward launch must move: per channel with a factor two planes read and one written, else one written; root_d written."""
    selected = [K.NC if h % 4 != 3 else 4 * TOPK for h in range(4 * STAGES)]
    return sum(B * H * W * 4 * (3 * s + (K.NC - s) + 1) for s in selected)


def reduce_trace(path, out_path):
    """rocprofv3's *_kernel_trace.csv of a `--fused-only` run -> per kernel and batch size the launches' durations and achieved bytes/s."""
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "loss_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    durations, B = {}, None
    for r in rows:
        name = r["Kernel_Name"]
        kind = "reduce" if "loss_reduce" in name else "finish" if "loss_finish" in name else "backward" if "loss_backward" in name else None
        if kind is None:
            continue
        if kind != "finish":                                   # grid (58, B, n_heads) workgroups of (256, 1, 1) threads
            B = int(r["Grid_Size_Y"]) // max(1, int(r["Workgroup_Size_Y"]))
        if B is None:
            continue
        durations.setdefault((kind, B), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = dict(what="rocprofv3 --kernel-trace over `python tools/bench_loss.py --fused-only` (a run of its own), reduced by "
                    "`tools/bench_loss.py --reduce-trace`: duration of the loss kernels per launch and batch size, and the bytes a launch "
                    "must move over its median duration; a finish launch is counted with the reduction launch before it",
               map=[H, W], kernels={})
    for (kind, B), ns in sorted(durations.items()):
        entry = dict(calls=len(ns), median_us=float(np.median(ns)) / 1e3, min_us=min(ns) / 1e3, max_us=max(ns) / 1e3)
        need = forward_bytes(B) if kind == "reduce" else backward_bytes(B) if kind == "backward" else None
        if need:
            entry["bytes"] = need
            entry["gb_per_s"] = need / (entry["median_us"] * 1e-6) / 1e9
        out["kernels"]["%s_B%d" % (kind, B)] = entry
    for B in sorted({b for _, b in durations}):
        k = out["kernels"]
        if all(n + "_B%d" % B in k for n in ("reduce", "finish")):
            k["finish_B%d" % B]["share_of_forward_kernels"] = k["finish_B%d" % B]["median_us"] / (k["finish_B%d" % B]["median_us"] + k["reduce_B%d" % B]["median_us"])
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


def make_inputs(B, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rand = lambda *shape: torch.randn(shape, generator=g, device=DEV)
    labels = rand(B, S, K.NC, H, W)
    nest = lambda ch: [[rand(B, ch, H, W).requires_grad_(True) for _ in range(4)] for _ in range(STAGES)]
    outputs = dict(heatmap_2d=nest(K.N2D), det_d=nest(K.NDD), root_d=nest(1))
    rdepth = torch.zeros((B, R, 3), device=DEV)
    rows = np.random.RandomState(seed)
    for b in range(B):
        for r in range(6):
            rdepth[b, r] = torch.tensor([rows.uniform(0, H - 1), rows.uniform(0, W - 1), rows.uniform(0.5, 5)])
    return outputs, torch.ones((B, K.NC, 1), device=DEV), labels, rdepth


def leaves(outputs):
    return [t for key in outputs for stage in outputs[key] for t in stage]


def bench_case(B, iters, warmup, fused_only=False):
    outputs, valids, labels, rdepth = make_inputs(B)
    crit = K.SMAPLoss(STAGES, True, TOPK, True)

    def clear():
        for t in leaves(outputs):
            t.grad = None

    def fwd(fn):
        def step():
            with torch.no_grad():
                fn(outputs, valids, labels, rdepth)["total_loss"]
        return step

    def fwd_bwd(fn):
        def step():
            clear()
            fn(outputs, valids, labels, rdepth)["total_loss"].backward()
        return step

    case = dict(B=B)
    with ClockSampler(0) as clocks:
        case["fused_forward"] = stats(*time_loop(fwd(crit), iters, warmup))
        case["fused_forward_backward"] = stats(*time_loop(fwd_bwd(crit), iters, warmup))
    case["clocks_during_fused"] = clocks.summary()
    if fused_only:
        return case
    # the baseline synchronises per row: fewer iterations keep the tool short, the per-iteration figures are comparable
    n = max(10, iters // 10)
    case["torch_forward"] = dict(stats(*time_loop(fwd(torch_loss), n, 3)), iters=n)
    case["torch_forward_backward"] = dict(stats(*time_loop(fwd_bwd(torch_loss), n, 3)), iters=n)
    # agreement of the two paths on these inputs
    clear()
    a = crit(outputs, valids, labels, rdepth)
    a["total_loss"].backward()
    ga = [t.grad.clone() for t in leaves(outputs)]
    clear()
    b = torch_loss(outputs, valids, labels, rdepth)
    b["total_loss"].backward()
    case["total_fused"], case["total_torch"] = a["total_loss"].item(), b["total_loss"].item()
    case["max_gradient_difference_relative"] = max(float((x - t.grad).abs().max() / t.grad.abs().max().clamp_min(1e-30))
                                                   for x, t in zip(ga, leaves(outputs)))
    # bytes the launches must move; over event times these are lower bounds of the launches' own rates (see --reduce-trace)
    case["forward_bytes"], case["backward_bytes"] = forward_bytes(B), backward_bytes(B)
    case["forward_gb_per_s"] = case["forward_bytes"] / (case["fused_forward"]["device_ms_median"] * 1e-3) / 1e9
    bwd_ms = case["fused_forward_backward"]["device_ms_median"] - case["fused_forward"]["device_ms_median"]
    case["backward_ms_by_difference"] = bwd_ms
    case["backward_gb_per_s"] = case["backward_bytes"] / (bwd_ms * 1e-3) / 1e9 if bwd_ms > 0 else None
    for k in ("forward", "forward_backward"):
        case["speedup_device_" + k] = case["torch_" + k]["device_ms_median"] / case["fused_" + k]["device_ms_median"]
        case["speedup_wall_" + k] = case["torch_" + k]["wall_ms"] / case["fused_" + k]["wall_ms"]
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--fused-only", action="store_true", help="time the fused path alone (for a kernel trace); writes no file without --out")
    ap.add_argument("--out", default=None, help="default: profiles/loss_bench.json (none with --fused-only)")
    ap.add_argument("--reduce-trace", metavar="CSV", help="reduce a rocprofv3 kernel trace of a --fused-only run; no GPU needed")
    ap.add_argument("--trace-out", default=os.path.join(ROOT, "profiles", "loss_kernel_trace.json"))
    args = ap.parse_args()
    if args.reduce_trace:
        return reduce_trace(args.reduce_trace, args.trace_out)
    if args.out is None and not args.fused_only:
        args.out = os.path.join(ROOT, "profiles", "loss_bench.json")
    out = dict(gpu=torch.cuda.get_device_name(0), map=[H, W], stages=STAGES, ohkm=True, topk=TOPK, coarse_to_fine=True, label_scales=S,
               rows_per_frame=R, persons_per_frame=6, iters=args.iters, warmup=args.warmup,
               what="device_ms: HIP events around each iteration; wall_ms: perf_counter around the loop, one synchronisation at its end; "
                    "torch_*: tools/bench_loss.py torch_loss (mse_loss, mean, topk, a per-row indexing loop with one host read per row); "
                    "backward_ms_by_difference includes autograd's own small kernels",
               cases=[bench_case(B, args.iters, args.warmup, args.fused_only) for B in (2, 8)])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
