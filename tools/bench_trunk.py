#!/usr/bin/env python3
"""Time the trunk of one Upsample_unit in fp32 (smap_amd/trunk.py: smap_trunk_forward, smap_trunk_backward) against the same unit in
plain torch fp32 on the device (F.conv2d + F.interpolate + autograd: the comparison path), and a whole DecoderFineTuner.step beside a
HeadFineTuner.step of the same run.

    python tools/bench_trunk.py [--iters 50] [--warmup 5] [--out profiles/trunk_bench.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_trunk.py --calls-only --iters 20 --warmup 3
    python tools/bench_trunk.py --reduce-trace DIR/.../*_kernel_trace.csv --iters 20 --warmup 3 [--out profiles/trunk_bench.json]

Cases: the four levels of the full network -- up1 16x26 Cin 2048 (no up path), up2 32x52 Cin 1024, up3 64x104 Cin 512, up4 128x208
Cin 256 -- at B = 2 and B = 8, chl = 256, X as the x3 engine leaves it (fp16 hi|lo planes), O_prev dense fp32 (the chain's own).
  device_ms   HIP events around every iteration (median, min, max over --iters after --warmup), workspaces allocated outside.
  tflops      the multiply-adds of the call's GEMMs by their shapes (2 flops each) over the median.
  launches    (--reduce-trace, a run of its own under rocprofv3) per launch of a call its median duration; GEMMs with their rate, the
              three elementwise kernels with the bytes they move by shape and the resulting GB/s.  A --calls-only run issues, per case,
              (warmup + iters) forward calls and then as many backward calls (with gX), so the k-th launch of every call is known by position.
  step        DecoderFineTuner.step and HeadFineTuner.step on the full network (512 x 832 images), wall time per step with one
              synchronisation at the end of the loop, one after the other in the same process.
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
from smap_amd import trunk as T  # noqa: E402

CHL = 256
LEVELS = ((16, 26, 2048), (32, 52, 1024), (64, 104, 512), (128, 208, 256))       # h, w, Cin of up1 .. up4
BATCHES = (2, 8)
KERNELS = ("conv_gemm_kernel", "reduce_gemm_kernel", "reduce_fold_kernel", "upadd_forward_kernel", "relu_mask_kernel", "upadd_adjoint_kernel")


def launches(ind):
    fwd = ["O"] if ind == 0 else ["S", "U", "upadd_forward"]
    bwd = ["relu_mask", "gWu part", "gWu fold", "gX"] + ([] if ind == 0 else ["upadd_adjoint", "gWc part", "gWc fold", "gO_prev"])
    return fwd, bwd


def launch_work(B, ind):
    """name -> (flops, bytes) by shape: multiply-adds * 2 of a GEMM (a fold adds `slices` numbers per output); bytes read + written of
    an elementwise kernel, every tensor counted once (upadd_forward's four taps per pixel of U are cache hits after the first)."""
    h, w, cin = LEVELS[ind]
    hp, wp = (LEVELS[ind - 1][:2] if ind else (0, 0))
    P, Pl, c = B * h * w, B * hp * wp, CHL
    lay = T.workspace_layout(B, h, w, hp, wp, cin, c, True)
    f = {"O": (2 * P * cin * c, 0), "S": (2 * P * cin * c, 0), "U": (2 * Pl * c * c, 0), "upadd_forward": (0, 4 * c * (2 * P + Pl)),
         "relu_mask": (0, 4 * c * 3 * P), "gWu part": (2 * P * c * cin, 0), "gWu fold": (lay["slices"] * c * cin, 0), "gX": (2 * P * c * cin, 0),
         "upadd_adjoint": (0, 4 * c * (P + Pl)), "gWc part": (2 * Pl * c * c, 0), "gWc fold": (lay["slices_lo"] * c * c, 0),
         "gO_prev": (2 * Pl * c * c, 0)}
    return f


def make_unit(B, ind, seed=0):
    h, w, cin = LEVELS[ind]
    g = torch.Generator(device=DEV).manual_seed(seed)
    rand = lambda *shape: torch.randn(shape, generator=g, device=DEV)
    x = torch.relu(rand(B, h, w, cin))
    hi = x.half()
    planes = torch.stack([hi, (x - hi.float()).half()], dim=3).contiguous()
    o_prev = torch.relu(rand(B, *LEVELS[ind - 1][:2], CHL)) if ind else None
    wu, b = rand(CHL, cin) * (2.0 / cin) ** 0.5, rand(CHL) * 0.1
    wc = rand(CHL, CHL) * (2.0 / CHL) ** 0.5 if ind else None
    return planes, o_prev, wu, wc, b, rand(B, h, w, CHL) * 1e-6


def bench_case(B, ind, iters, warmup, calls_only):
    h, w, cin = LEVELS[ind]
    hp, wp = (LEVELS[ind - 1][:2] if ind else (0, 0))
    print("case B %d up%d %d x %d Cin %d" % (B, ind + 1, h, w, cin), file=sys.stderr, flush=True)
    planes, o_prev, wu, wc, b, g = make_unit(B, ind)
    dims = (B, h, w, hp, wp, cin, CHL)
    ws_f, ws_b = (G.new_workspace(T.workspace_bytes(*dims, backward), DEV) for backward in (False, True))
    work = launch_work(B, ind)
    fwd_names, bwd_names = launches(ind)
    case = dict(B=B, unit="up%d" % (ind + 1), level=[h, w], cin=cin, pixels=B * h * w)
    o, _ = T.forward(planes, o_prev, wu, wc, b, ws=ws_f)
    fwd, _ = time_loop(lambda: T.forward(planes, o_prev, wu, wc, b, ws=ws_f), iters, warmup)
    bwd, _ = time_loop(lambda: T.backward(planes, o_prev, o, wu, wc, g, want_gx=True, ws=ws_b), iters, warmup)
    case["smap_trunk_forward"] = stats(fwd, flops=sum(work[k][0] for k in fwd_names))
    case["smap_trunk_backward"] = stats(bwd, flops=sum(work[k][0] for k in bwd_names))
    if calls_only:
        return case
    # the comparison path: the same unit in torch fp32, NCHW, conv2d + interpolate + autograd (forward alone; forward + backward to all gradients)
    xt = (planes[..., 0, :].float() + planes[..., 1, :].float()).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    leaves = [xt, wu.view(CHL, cin, 1, 1).clone().requires_grad_(True), b.clone().requires_grad_(True)]
    if ind:
        leaves += [o_prev.permute(0, 3, 1, 2).contiguous().requires_grad_(True), wc.view(CHL, CHL, 1, 1).clone().requires_grad_(True)]
    gt = g.permute(0, 3, 1, 2).contiguous()

    def torch_forward():
        out = F.conv2d(leaves[0], leaves[1], leaves[2])
        if ind:                                       # the reference's order: interpolate, then the 1x1 at the HIGH resolution
            out = out + F.conv2d(F.interpolate(leaves[3], size=(h, w), mode="bilinear", align_corners=True), leaves[4])
        return torch.relu(out)

    def torch_forward_only():
        with torch.no_grad():
            torch_forward()

    def torch_both():
        for t in leaves:
            t.grad = None
        torch.autograd.backward([torch_forward()], [gt])
    case["torch_forward"] = stats(time_loop(torch_forward_only, iters, warmup)[0])
    case["torch_forward_backward"] = stats(time_loop(torch_both, iters, warmup)[0])
    case["ours_forward_backward_ms"] = case["smap_trunk_forward"]["device_ms_median"] + case["smap_trunk_backward"]["device_ms_median"]
    gwu, gwc, gb, gprev, gx, _ = T.backward(planes, o_prev, o, wu, wc, g, want_gx=True, ws=ws_b)
    torch_both()
    with torch.no_grad():
        theirs = torch_forward().permute(0, 2, 3, 1) > 0
    case["relu_sign_disagreements_with_torch"] = int(((o > 0) != theirs).sum())
    case["o_elements"] = int(o.numel())
    rel = lambda a, b: float((a - b).double().norm() / b.double().norm().clamp_min(1e-300))
    diffs = [rel(gwu, leaves[1].grad.view(CHL, cin)), rel(gb, leaves[2].grad), rel(gx, leaves[0].grad.permute(0, 2, 3, 1))]
    if ind:
        diffs += [rel(gprev, leaves[3].grad.permute(0, 2, 3, 1)), rel(gwc, leaves[4].grad.view(CHL, CHL))]
    case["max_gradient_relative_l2_difference_to_torch"] = max(diffs)
    return case


def bench_step(B, iters, warmup):
    print("step B %d" % B, file=sys.stderr, flush=True)
    net, cfg, batch = full_network_batch(B)
    out = dict(B=B, images=[512, 832], iters=iters)
    for name, cls in (("HeadFineTuner", FT.HeadFineTuner), ("DecoderFineTuner", FT.DecoderFineTuner)):
        tuner = cls(net, cfg, lr=1e-6, weight_decay=8e-6)
        step = lambda: tuner.step(*batch)
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        out[name] = dict(wall_ms_per_step=(time.perf_counter() - t0) * 1e3 / iters, peak_memory_gib=torch.cuda.max_memory_allocated() / 2 ** 30)
    return out


def reduce_trace(path, iters, warmup):
    """Per case the median duration of every launch, from a kernel trace of a --calls-only run with the same --iters / --warmup."""
    def case(B, ind):
        h, w, cin = LEVELS[ind]
        work = launch_work(B, ind)
        fwd_names, bwd_names = launches(ind)

        def rate(name, med):
            flops, nbytes = work[name]
            return dict(flops=int(flops), tflops=flops / (med * 1e-6) / 1e12) if flops else dict(bytes=int(nbytes), gb_per_s=nbytes / (med * 1e-6) / 1e9)
        # bench_case runs one forward call before its timed loops (it makes O): that call's launches come first
        return (dict(B=B, unit="up%d" % (ind + 1), level=[h, w], cin=cin),
                [("smap_trunk_forward", fwd_names, 1), ("smap_trunk_backward", bwd_names, 0)], rate)
    return reduce_positional_trace(path, KERNELS, [case(B, ind) for B in BATCHES for ind in range(4)], iters + warmup, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--calls-only", action="store_true", help="time the two C calls alone (for a kernel trace); writes no file without --out")
    ap.add_argument("--reduce-trace", metavar="CSV", help="add per-launch figures from a rocprofv3 kernel trace of a --calls-only run to --out")
    ap.add_argument("--out", default=None, help="default: profiles/trunk_bench.json (none with --calls-only)")
    args = ap.parse_args()
    default = os.path.join(ROOT, "profiles", "trunk_bench.json")
    if args.reduce_trace:
        path = args.out or default
        out = read_json(path)
        out["launches"] = dict(what="rocprofv3 --kernel-trace over `tools/bench_trunk.py --calls-only` (a run of its own), reduced by --reduce-trace",
                               iters=args.iters, warmup=args.warmup, cases=reduce_trace(args.reduce_trace, args.iters, args.warmup))
        json.dump(out, open(path, "w"), indent=1)
        return print(json.dumps(out["launches"], indent=1))
    if args.out is None and not args.calls_only:
        args.out = default
    out = dict(gpu=torch.cuda.get_device_name(0), chl=CHL, x_layout="fp16 hi|lo planes", o_prev_layout="fp32", iters=args.iters, warmup=args.warmup,
               what="device_ms: HIP events around each iteration of one call (backward with gX).  tflops: the GEMMs' flops by shape over the median.  "
                    "torch_*: the same unit as F.conv2d + F.interpolate + autograd in fp32 on the device (the comparison path).  step: "
                    "DecoderFineTuner.step and HeadFineTuner.step on the full network, wall time, the same process",
               cases=[bench_case(B, ind, args.iters, args.warmup, args.calls_only) for B in BATCHES for ind in range(4)])
    if not args.calls_only:
        out["step"] = [bench_step(B, args.step_iters, 2) for B in BATCHES]
    if args.out:
        write_merged(out, args.out)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
