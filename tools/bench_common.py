"""What tools/bench_heads.py, bench_trunk.py, bench_loss.py and bench_lossgrad.py share: the timed loop and its summary, the full-network
training batch of the two `step` benchmarks, the positional reducer of a rocprofv3 kernel trace, and the writer that keeps a reduced
trace in the JSON a later timing run rewrites.  A sibling import: the tools run as `python tools/bench_*.py`."""
import csv
import json
import os
import re
import time

import numpy as np
import torch

DEV = "cuda:0"


def time_loop(step, iters, warmup):
    """(per-iteration device ms [iters], wall ms per iteration): HIP events around every iteration after `warmup` untimed ones,
    time.perf_counter around the whole loop with one synchronisation at its end."""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    t0 = time.perf_counter()
    for a, b in ev:
        a.record()
        step()
        b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / iters
    return np.array([a.elapsed_time(b) for a, b in ev]), wall


def stats(ms, wall=None, flops=None, guide_tflops=None):
    """Median, min and max of time_loop's device ms; with `wall` the mean and the wall time too; with `flops` the rate over the median,
    and its share of `guide_tflops` where given."""
    out = dict(device_ms_median=float(np.median(ms)), device_ms_min=float(ms.min()), device_ms_max=float(ms.max()))
    if wall is not None:
        out.update(device_ms_mean=float(ms.mean()), wall_ms=float(wall))
    if flops is not None:
        out["flops"] = int(flops)
        out["tflops"] = flops / (out["device_ms_median"] * 1e-3) / 1e12
        if guide_tflops is not None:
            out["share_of_guide_untuned_gemm"] = out["tflops"] / guide_tflops
    return out


def full_network_batch(B):
    """(the full network on the device in x3 with recipe weights, its cfg, (imgs, valids, labels, rdepth) of B 512 x 832 frames)."""
    from benchkit.recipe import recipe_state_dict
    from benchkit.workload import make_cfg
    from smap_amd.model.smap import SMAP
    torch.manual_seed(0)
    net = SMAP(make_cfg((128, 208))).eval()
    net.load_state_dict(recipe_state_dict(net.state_dict()))
    net = net.to(DEV)
    net.precision = "x3"
    g = torch.Generator(device=DEV).manual_seed(1)
    imgs = torch.randn((B, 3, 512, 832), generator=g, device=DEV)
    labels = torch.randn((B, 5, 57, 128, 208), generator=g, device=DEV)
    valids = torch.ones((B, 57, 1), device=DEV)
    rdepth = torch.zeros((B, 8, 3), device=DEV)
    rdepth[:, :4] = torch.tensor([[10.5, 20.5, 2.0], [100.2, 50.7, 3.0], [64.0, 104.0, 1.5], [127.0, 207.0, 4.0]], device=DEV)
    return net, make_cfg((128, 208)), (imgs, valids, labels, rdepth)


def reduce_positional_trace(path, kernels, cases, calls, warmup):
    """Per case and call the median duration of every launch, from a kernel trace of a --calls-only run.  The trace lists kernels in
    start order and a run issues, per case and call, `extra` untimed calls and then `calls` = warmup + iters more, so the k-th launch of
    every call is known by position.  cases: (case dict, [(call name, launch names, extra)], describe) in the run's order, where
    describe(launch name, median us) gives what stands beside "kernel" and "median_us".  Returns the case dicts, filled."""
    rows = [r for r in csv.DictReader(open(path)) if any(k in r["Kernel_Name"] for k in kernels)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    at, out = 0, []
    for case, blocks, describe in cases:
        for what, names, extra in blocks:
            block = rows[at:at + (calls + extra) * len(names)]
            assert len(block) == (calls + extra) * len(names), (at, len(rows))
            at += len(block)
            per = {}
            for k, name in enumerate(names):
                ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in block[(warmup + extra) * len(names) + k::len(names)]]
                med = float(np.median(ns)) / 1e3
                per[name] = dict(kernel=re.search(r"(%s)(<[^>]*>)?" % "|".join(kernels), block[k]["Kernel_Name"]).group(0), median_us=med,
                                 **describe(name, med))
            case[what] = per
        out.append(case)
    assert at == len(rows), (at, len(rows))
    return out


def read_json(path):
    return json.load(open(path)) if os.path.exists(path) else {}


def write_merged(out, path, keep=("launches",)):
    """Writes `out` to `path`; the entries `keep` of a file already there stay."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    prev = read_json(path)
    out.update({k: prev[k] for k in keep if k in prev})
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
