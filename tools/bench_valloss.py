#!/usr/bin/env python3
"""Time the validation loss on the flagship shape: B x 3 x 512 x 832, precision x3.

    python tools/bench_valloss.py [--steps 100] [--warmup 10] [--batches 8 2] [--out profiles/valloss_bench.json]

Per batch size, medians of HIP events around each step:
  forward_default_ms     the inference schedule (BackboneEngine.run)
  forward_all_heads_ms   the schedule with the 62 training-only head convs (all_heads=True), same weights and frames
  loss_src_ms            smap_loss_forward_src on the 36 head tensors at their own resolutions (three launches)
  loss_upsampled_ms      the alternative it replaces: one single-source HEADSUM launch per head tensor (36: a plan of its own over copies
                         of the same tensors, bilinear to 128 x 208, NCHW) followed by smap_loss_forward on the upsampled maps
  validation_step_ms     SMAP.forward(imgs, valids, labels, rdepth): all-heads forward + loss, as one step
Both loss paths read the same 36 NHWC tensors (the all-heads engine's, copied into the comparison plan's arena; the tap-dot route's finest
root-depth map is copied from the output buffer), and their values are compared.  Labels are random; 6 root rows per frame."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from benchkit.workload import make_cfg  # noqa: E402
from benchkit.recipe import recipe_state_dict  # noqa: E402
from smap_amd import lib as L  # noqa: E402
from smap_amd import loss as K  # noqa: E402
from smap_amd.engine import OP_HEADSUM, Graph, HeadSource, Op  # noqa: E402
from smap_amd.model.smap import SMAP  # noqa: E402

DEV = "cuda:0"
H, W, S, R = 128, 208, 5, 20
KEYS = ("heatmap_2d", "det_d", "root_d")


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        step()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()))


class UpsamplePlan:
    """36 single-source HEADSUM ops over NHWC copies of the head tensors -> 36 NCHW maps [B, c, 128, 208] in one output buffer."""

    def __init__(self, eng, out):
        B = eng.B
        g = Graph(None, B, 512, 832, precision="x3", build=False)
        g.out_h, g.out_w = H, W
        self.items, off = [], 0
        for h, d in enumerate(eng.head_sources(out)):
            for key in KEYS:
                s = d[key]
                t = g.tensor("h%d.%s" % (h, key), s.h, s.w, (s.c + 7) // 8 * 8, 4)
                t.first = 0                                        # an input of this plan: no op writes it, it is there from the start
                self.items.append((h, key, s, t, off))
                off += B * s.c * H * W * 4
        g.out_bytes = g.status_off = off
        g.status_words = (B + 30) // 31
        for _, _, s, t, ext in self.items:
            g.ops.append(Op(OP_HEADSUM, aux=[t], p=dict(Cout=s.c, ext_off=ext)))
        g.allocate(reuse=False)
        self.g, self.lib = g, L.load()
        self.arena = torch.zeros((g.arena_bytes,), dtype=torch.uint8, device=DEV)
        self.out = torch.zeros((off // 4 + g.status_words,), dtype=torch.float32, device=DEV)
        self.weights = g.weight_blob().to(DEV)
        self.handle = C.c_void_p()
        L.check(self.lib.smap_plan_create(g.emit(), len(g.ops), C.byref(self.handle)), "smap_plan_create")
        flat = self.arena.view(torch.float32)
        self.desc = [dict() for _ in range(len(self.items) // 3)]
        for h, key, s, t, _ in self.items:                         # copy the engine's tensor (through its descriptor) into this arena, NHWC
            base = eng.arena if eng.arena.data_ptr() <= s.ptr < eng.arena.data_ptr() + eng.arena.numel() else out.view(torch.uint8)
            src = torch.as_strided(base.view(torch.float32), (B, s.h, s.w, s.c), (s.frame_stride, s.w * s.pix_stride, s.pix_stride, s.ch_stride),
                                   (s.ptr - base.data_ptr()) // 4)
            dst = flat[t.off // 4:t.off // 4 + B * t.H * t.W * t.C].view(B, t.H, t.W, t.C)
            dst[..., :s.c] = src
            self.desc[h][key] = HeadSource(self.arena.data_ptr() + t.off, t.H, t.W, s.c, t.C, 1, t.H * t.W * t.C)
        self.maps = [self.out[ext // 4:ext // 4 + B * s.c * H * W].view(B, s.c, H, W) for _, _, s, _, ext in self.items]

    def run(self):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(self.lib.smap_plan_run_range(self.handle, 0, len(self.g.ops), None, C.c_void_p(self.arena.data_ptr()),
                                             C.c_void_p(self.weights.data_ptr()), C.c_void_p(self.out.data_ptr()), st), "smap_plan_run")

    def close(self):
        self.lib.smap_plan_destroy(self.handle)


def bench(B, steps, warmup, net):
    g = torch.Generator(device=DEV).manual_seed(B)
    imgs = torch.randn((B, 3, 512, 832), generator=g, device=DEV)
    labels = torch.randn((B, S, K.NC, H, W), generator=g, device=DEV)
    valids = torch.ones((B, K.NC), device=DEV)
    rdepth = torch.zeros((B, R, 3), device=DEV)
    rows = np.random.RandomState(B)
    for b in range(B):
        for r in range(6):
            rdepth[b, r] = torch.tensor([rows.uniform(0, H - 1), rows.uniform(0, W - 1), rows.uniform(0.5, 5)])
    case = dict(B=B)
    eng0 = net.engine(B, 512, 832, torch.device(DEV))
    case["forward_default"] = timed(lambda: eng0.run(imgs), steps, warmup)
    eng = net.engine(B, 512, 832, torch.device(DEV), all_heads=True)
    out = eng.new_output()
    case["forward_all_heads"] = timed(lambda: eng.run(imgs, out=out), steps, warmup)
    case["ops"] = dict(default=eng0.n_ops, all_heads=eng.n_ops)
    case["arena_bytes"] = dict(default=eng0.arena.numel(), all_heads=eng.arena.numel())
    crit = K.EngineLoss(3, True, 8, True)
    cfg, labels_c, valids_c, rdepth_c = crit.check(valids, labels, rdepth)
    up = UpsamplePlan(eng, out)
    case["loss_src"] = timed(lambda: K.forward_from_sources(cfg, up.desc, labels_c, valids_c, rdepth_c), steps, warmup)
    full = K.SMAPLoss(3, True, 8, True)
    nest = lambda k: [[up.maps[3 * (4 * i + j) + k] for j in range(4)] for i in range(3)]
    outputs = dict(heatmap_2d=nest(0), det_d=nest(1), root_d=nest(2))
    c2, tensors, l2, v2, r2 = full._check(outputs, valids, labels, rdepth)

    def upsampled():
        up.run()
        return K.forward_raw(c2, tensors, l2, v2, r2)
    case["loss_upsampled"] = timed(upsampled, steps, warmup)
    case["loss_upsampled_headsum_only"] = timed(up.run, steps, warmup)
    a = K.forward_from_sources(cfg, up.desc, labels_c, valids_c, rdepth_c)[0].cpu().numpy()
    b = upsampled()[0].cpu().numpy()
    case["values_src"], case["values_upsampled"] = a[:4].tolist(), b[:4].tolist()
    case["max_relative_difference"] = float(np.max(np.abs(a[:4] - b[:4]) / np.abs(b[:4])))
    case["validation_step"] = timed(lambda: net(imgs, valids, labels, rdepth), steps, warmup)
    case["upsampled_bytes_written_and_read"] = 2 * up.out.numel() * 4
    up.close()
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 2])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "valloss_bench.json"))
    args = ap.parse_args()
    torch.manual_seed(0)
    net = SMAP(make_cfg((H, W))).eval()
    net.load_state_dict(recipe_state_dict(net.state_dict()))
    net = net.to(DEV)
    net.precision = "x3"
    out = dict(gpu=torch.cuda.get_device_name(0), input=[3, 512, 832], precision="x3", steps=args.steps, warmup=args.warmup,
               what="medians of HIP events around each step; tools/bench_valloss.py says what each row runs",
               cases=[bench(B, args.steps, args.warmup, net) for B in args.batches])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
