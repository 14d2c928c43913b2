"""Whole schedules on poisoned arenas.  The schedule executor rests on one contract (csrc/plan_check.h, for_each_span of
csrc/plan_check.cpp): an op reads its declared operands and its window's zero page and writes its declared outputs, and smap_plan_run
clears the zero pages, the split-K tickets and the status words.  The arena packer's liveness reuse, the plan cache and the resident
batches bench.py rotates all lean on it -- and every other whole-schedule test starts from a zeroed arena, or from the previous run of
the SAME input.  Here the reusing engine (reuse=True: what the product runs) runs three times on the same images: on its own zeroed
arena, after arena, output buffer and the weight blob's alignment gaps were filled with 0xFF (NaN in fp16 and fp32, 0xFFFFFFFF in a
ticket), and after they were filled with 0x7B (large and finite: a ReLU's max turns a NaN into 0).  The output maps and the status words
must be byte-identical.  No buffer that a kernel reads as an index or a count is filled: the tickets are fetch-add counters that
smap_plan_run zeroes, not spin locks, so a fill cannot make a launch wait or address memory from data.

On a failure the schedule is rebuilt with reuse=False and every tensor is compared across the fills in schedule order: the message names
the first one that differs.  The single launches have the same property, with guards, in test_backbone_gpu.py / test_plan_ops_gpu.py."""
import pytest
import torch

from helpers import make_cfg
from recipe import recipe_state_dict
from single_op import DEV, FILLS

pytestmark = pytest.mark.gpu

ROUND6_SWITCHES = ("SMAP_CAT", "SMAP_SKIPSUM", "SMAP_TAPHEAD")
LAYER_BY_LAYER = {"SMAP_BLOCK": "", "SMAP_BLOCK_FIRST": ""}       # (as the tests of these flavours in test_backbone_gpu.py set them)

# name: (environment, engine keywords, batch, precisions)
FLAVOURS = {
    "default": ({}, {}, 2, ("x3", "f16")),
    "flip_tta": ({}, {"flip": True}, 2, ("x3", "f16")),
    "all_heads": ({}, {"all_heads": True}, 2, ("x3",)),
    "whole_bottlenecks": ({"SMAP_BLOCK": "64:91,128:94", "SMAP_BLOCK_FIRST": "64:93"}, {}, 2, ("x3",)),
    "fused_tails": ({"SMAP_TAIL": "64:81,128:82", **LAYER_BY_LAYER}, {}, 2, ("x3",)),
    "halo16": ({"SMAP_HALO3": "16"}, {}, 2, ("x3",)),
    "halo32deep": ({"SMAP_HALO3": "32", "SMAP_HALO3_DEEP": "1"}, {}, 2, ("x3",)),
    "split_k_3": ({"SMAP_SPLITK": "3", **LAYER_BY_LAYER}, {}, 2, ("x3",)),
    "split_k_16": ({"SMAP_SPLITK": "16", "SMAP_X3_TILE": "20", "SMAP_DEEP_TILE": "0", **LAYER_BY_LAYER}, {}, 2, ("x3",)),
    "merge_0": ({"SMAP_MERGE_1X1": "0", "SMAP_SKIPSUM": "0"}, {}, 2, ("x3",)),
    "merge_2": ({"SMAP_MERGE_1X1": "2", "SMAP_SKIPSUM": "0"}, {}, 2, ("x3",)),
    "lanes": ({"SMAP_LANES": "1"}, {}, 2, ("x3",)),
    "batch_1": ({k: None for k in ROUND6_SWITCHES}, {}, 1, ("x3",)),      # the batch-1 schedule as the product builds it: split K by the rule
    "graph_replay": ({}, {"replay": True}, 2, ("x3",)),
}
RUNS = [(name, p) for name, f in FLAVOURS.items() for p in f[3]]


@pytest.fixture(scope="module")
def small_sd():
    from smap_amd.model.smap import SMAP
    torch.manual_seed(0)
    return recipe_state_dict(SMAP(make_cfg((16, 24))).state_dict())


def flip_pair():
    from exps.stage3_root2.config import cfg
    return list(cfg.DATASET.KEYPOINT.FLIP_ORDER) + [cfg.DATASET.KEYPOINT.NUM + c for c in cfg.DATASET.PAF.FLIP_CHANNEL]


def build(sd, B, precision, kw, reuse):
    from smap_amd.engine import BackboneEngine
    return BackboneEngine(sd, B, 64, 96, DEV, reuse=reuse, precision=precision, flip_pair=flip_pair() if kw.get("flip") else None,
                          all_heads=bool(kw.get("all_heads")))


def poison(eng, out, fill):
    """Arena, output buffer (maps and status words) and the weight blob's alignment gaps = fill, in place: captured graphs keep the pointers."""
    eng.arena.fill_(fill)
    out.view(torch.uint8).fill_(fill)
    blob = torch.full((eng.weights.numel(),), fill, dtype=torch.uint8)
    for off, raw in eng.graph.wchunks:
        blob[off:off + raw.numel()] = raw
    eng.weights.copy_(blob.to(DEV))


def first_differing_tensor(sd, B, precision, kw, x):
    """The schedule without reuse, once per fill: the first tensor in schedule order whose bytes differ between the fills."""
    eng = build(sd, B, precision, kw, reuse=False)
    out, seen = eng.new_output(), []
    for fill in FILLS:
        poison(eng, out, fill)
        eng.run(x, out=out)
        torch.cuda.synchronize()
        seen.append({t.name: eng.arena[t.off:t.off + t.nbytes].clone() for t in eng.graph.tensors})
    for t in sorted(eng.graph.tensors, key=lambda t: t.first):
        if not torch.equal(seen[0][t.name], seen[1][t.name]):
            off = int((seen[0][t.name] != seen[1][t.name]).nonzero()[0])
            return "first tensor that differs between the fills without reuse: %s (op %d), byte %d of %d" % (t.name, t.first, off, t.nbytes)
    return "no tensor differs between the fills without reuse: the dependency needs the reusing arena's layout"


@pytest.mark.parametrize("flavour,precision", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_schedule_outputs_do_not_depend_on_what_the_arena_held(small_sd, monkeypatch, flavour, precision):
    """Zeroed arena, 0xFF everywhere, 0x7B everywhere: the same maps and status words, bit for bit -- for the default schedule in both
    precisions and for every launch flavour the small schedules can be switched to (whole-Bottleneck launches, fused tails, halo kernels,
    forced split K, merged and unmerged 1x1s, lanes, flip-TTA, all heads, the batch-1 schedule, graph replay, whose capture must hold
    smap_plan_run's memsets of zero pages, tickets and status words)."""
    env, kw, B, _ = FLAVOURS[flavour]
    for k, v in env.items():
        monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)
    eng = build(small_sd, B, precision, kw, reuse=True)
    ops = eng.graph.ops
    if flavour.startswith("split_k") or flavour == "batch_1":
        n_split = sum(1 for op in ops if op.p.get("ksplit", 1) > 1)
        assert n_split >= (1 if flavour == "batch_1" else 30), n_split
    if flavour == "whole_bottlenecks":
        assert sum(1 for op in ops if op.kind == 0 and "head" in op.p) == 18
    if flavour == "fused_tails":
        assert sum(1 for op in ops if op.kind == 0 and "tail" in op.p) == 18
    if flavour.startswith("halo"):
        assert any(30 <= op.p["tile"] < 50 for op in ops if op.kind == 0)
    if flavour.startswith("merge"):
        assert sum(len(op.outs) for op in ops) == {"merge_2": 18, "merge_0": 0}[flavour]
    if flavour == "lanes":
        assert eng.graph.lanes and len({op.lane for op in ops}) == 3
    x = torch.randn(B, 3, 64, 96, generator=torch.Generator().manual_seed(31)).to(DEV)
    out = eng.new_output()
    if kw.get("replay"):
        replay = eng.capture(out)
        run = lambda: replay(x)
    else:
        run = lambda: eng.run(x, out=out)
    kept = eng.graph.keep if kw.get("all_heads") else []            # all heads: the loss reads these out of the arena behind the schedule
    assert not kw.get("all_heads") or len(kept) >= 30
    results = []
    for fill in (None,) + FILLS:
        if fill is not None:
            poison(eng, out, fill)
        run()
        torch.cuda.synchronize()
        results.append((out.view(torch.int32).clone(), [eng.arena[t.off:t.off + t.nbytes].clone() for t in kept]))
    maps = results[0][0][:eng.out_floats].view(torch.float32)
    assert bool(torch.isfinite(maps).all()) and float(maps.abs().max()) > 1e-3
    assert not bool(results[0][0][eng.out_floats:].any())           # status words: no non-finite value reached the maps
    for (bits, heads), fill in zip(results[1:], FILLS):
        same = torch.equal(bits, results[0][0]) and all(torch.equal(a, b) for a, b in zip(heads, results[0][1]))
        if not same:
            n = int((bits != results[0][0]).sum())
            pytest.fail("fill 0x%02X: %d of %d output words (maps | status) differ from the run on the zeroed arena; %s"
                        % (fill, n, bits.numel(), first_differing_tensor(small_sd, B, precision, kw, x)))
