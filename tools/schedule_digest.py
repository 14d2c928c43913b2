#!/usr/bin/env python3
"""blake2b of Graph.blob() -- every launch descriptor, every packed weight, the arena size, the output layout -- and of every tensor's
(name, first, last, off, nbytes), split-K scratch and the ticket region included, for a fixed list of schedules and SMAP_* switch settings,
one line per case: two versions of the schedule builder (smap_amd/engine.py) that claim to build the same schedules print the same lines.
CPU only (the library is not loaded).  Weights: recipe_state_dict of a seed-0 SMAP, as tests/test_host_cpu.py's small_sd.  A case the
builder refuses prints the exception's type in place of the digests.
    python tools/schedule_digest.py [--only SUBSTRING]"""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from benchkit.recipe import recipe_state_dict  # noqa: E402
from benchkit.workload import make_cfg  # noqa: E402
from exps.stage3_root2.config import cfg  # noqa: E402
from smap_amd.engine import Graph  # noqa: E402
from smap_amd.model.smap import SMAP  # noqa: E402

# every variable the schedule builder listens to: removed from the environment before each case, then the case's own are set
SWITCHES = ("BLOCK", "BLOCK_FIRST", "TAIL", "CAT", "SKIPSUM", "TAPHEAD", "MERGE_1X1", "SPLITK", "SPLITK_MINK", "DEEP_TILE", "LANES", "WPAIRS",
            "X3_TILE", "CAT_TILE", "RELUSUM_TILE", "HALO3", "HALO3_DEEP", "TILE_REMAP", "TILE_POLICY", "STEMPOOL", "NO_UPADD_FUSION",
            "TILE_TABLE", "TILE_TABLE_X3", "NO_TILE_TABLE")
CONFTEST = dict(CAT="1", SKIPSUM="1", TAPHEAD="1")        # what tests/conftest.py sets for every test
BOTH = ("f16", "x3")


SMALL, ONE, EIGHT = (2, 64, 96), (1, 512, 832), (8, 512, 832)


def flip_pair():
    return list(cfg.DATASET.KEYPOINT.FLIP_ORDER) + [cfg.DATASET.KEYPOINT.NUM + c for c in cfg.DATASET.PAF.FLIP_CHANNEL]


def small_cases():
    """(label, precision, Graph keyword arguments, switches) of the cases at 2x64x96 -- the smallest shape the builder accepts with all
    five levels present -- in a fixed order (tests/test_host_cpu.py walks the same list)."""
    flip = flip_pair()
    for prec in BOTH:
        yield "default", prec, {}, {}
        yield "conftest", prec, {}, CONFTEST
    # every switch in turn, on top of the conftest setting, in the precision its tests use
    for prec, sw in (("x3", dict(MERGE_1X1="0")), ("f16", dict(MERGE_1X1="0")), ("x3", dict(MERGE_1X1="2")), ("f16", dict(MERGE_1X1="2")),
                     ("x3", dict(SKIPSUM="0")), ("f16", dict(SKIPSUM="0")), ("x3", dict(CAT="0")), ("f16", dict(CAT="0")),
                     ("x3", dict(TAPHEAD="0")), ("f16", dict(TAPHEAD="0")),
                     ("x3", dict(SPLITK="0")), ("x3", dict(SPLITK="3")), ("f16", dict(SPLITK="3")), ("x3", dict(SPLITK="t384")),
                     ("x3", dict(X3_TILE="2", DEEP_TILE="0")),
                     ("x3", dict(BLOCK="", BLOCK_FIRST="")),
                     ("x3", dict(TAIL="64:80,128:82", BLOCK="")), ("f16", dict(TAIL="64:80,128:82", BLOCK="")),
                     ("x3", dict(HALO3="16")), ("f16", dict(HALO3="16")), ("x3", dict(HALO3="32", HALO3_DEEP="1")),
                     ("x3", dict(LANES="1")), ("f16", dict(LANES="1")),
                     ("x3", dict(STEMPOOL="1")), ("f16", dict(STEMPOOL="1")),
                     ("f16", dict(NO_UPADD_FUSION="1", MERGE_1X1="0")),
                     ("x3", dict(WPAIRS="0")), ("x3", dict(WPAIRS="1")), ("f16", dict(WPAIRS="0")),
                     ("x3", dict(TILE_REMAP="2:7")), ("f16", dict(TILE_REMAP="2:7")),
                     ("x3", dict(NO_TILE_TABLE="1")), ("f16", dict(NO_TILE_TABLE="1")),
                     ("f16", dict(TILE_POLICY="traffic")),        # (refused: the policy cannot read a merged launch's key)
                     ("f16", dict(TILE_POLICY="traffic", MERGE_1X1="0")),
                     ("x3", dict(CAT_TILE="20")), ("x3", dict(RELUSUM_TILE="53"))):
        yield "switch", prec, {}, {**CONFTEST, **sw}
    # the Upsample_unit in every merge mode: alone, with lanes, with every head chain, with the flip pair
    for prec in BOTH:
        for m in "02":
            yield "switch", prec, {}, dict(MERGE_1X1=m)                                   # (without the conftest switches)
        for m in "02":
            yield "switch", prec, {}, {**CONFTEST, "LANES": "1", "MERGE_1X1": m}           # (mode 1 with lanes: above)
        for m in "012":
            yield "all_heads", prec, dict(all_heads=True), {**CONFTEST, "MERGE_1X1": m}
        yield "all_heads+flip_pair", prec, dict(all_heads=True, flip_pair=flip), CONFTEST
        yield "all_heads", prec, dict(all_heads=True), {**CONFTEST, "LANES": "1"}
        yield "flip_pair", prec, dict(flip_pair=flip), {**CONFTEST, "MERGE_1X1": "0"}
        yield "stage_num=2", prec, dict(stage_num=2), CONFTEST
        yield "switch", prec, {}, {**CONFTEST, "STEMPOOL": "1", "MERGE_1X1": "0"}
    yield "switch", "f16", {}, {**CONFTEST, "NO_UPADD_FUSION": "1"}          # honoured with MERGE_1X1=0 only: the conftest case's digest


def cases():
    """(label, precision, (B, H, W), Graph keyword arguments, switches, allocate's reuse) in a fixed order."""
    flip = flip_pair()
    for prec in BOTH:                                     # the default environment at full size
        for shape in (ONE, EIGHT):
            yield "default", prec, shape, {}, {}, True
        yield "flip_pair", prec, EIGHT, dict(flip_pair=flip), {}, True
        yield "all_heads", prec, EIGHT, dict(all_heads=True), {}, True
        yield "scaled_hms", prec, EIGHT, dict(scaled_hms=True), {}, True
    yield "default", "x3", (16, 512, 832), {}, {}, True
    # the real batch-1 rules (no conftest switches)
    yield "switch", "x3", ONE, {}, dict(SPLITK_MINK="1024"), True
    yield "switch", "x3", ONE, {}, dict(BLOCK="64:91,128:94"), True
    for reuse in (True, False):                           # reuse=False: the arena that keeps every tensor (read_tensor)
        for label, prec, kw, sw in small_cases():
            yield label, prec, SMALL, kw, sw, reuse


def set_switches(sw):
    for k in SWITCHES:
        os.environ.pop("SMAP_" + k, None)
    for k, v in sw.items():
        os.environ["SMAP_" + k] = v


def every_tensor(g):
    """Everything the arena holds: the activation tensors, the split-K scratch and the ticket region."""
    return g.tensors + g.scratch_tensors + ([g.kcount] if g.kcount is not None else [])


def digest(sd, prec, shape, kw, sw, reuse=True):
    set_switches(sw)
    try:
        g = Graph(sd, *shape, precision=prec, **kw)
        g.allocate(reuse=reuse)
        life = repr([(t.name, t.first, t.last, t.off, t.nbytes) for t in every_tensor(g)]).encode()
        return "%s tensors %s n_ops %d lanes %d flops %d alg_bytes %d arena_bytes %d" % (
            hashlib.blake2b(g.blob(), digest_size=16).hexdigest(), hashlib.blake2b(life, digest_size=16).hexdigest(),
            len(g.ops), int(g.lanes), g.flops, g.alg_bytes, g.arena_bytes)
    except Exception as exc:                              # noqa: BLE001  (a refused case is a result too)
        return type(exc).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="run the cases whose line contains this text")
    args = ap.parse_args()
    torch.manual_seed(0)
    sd = recipe_state_dict(SMAP(make_cfg((16, 24))).state_dict())
    for label, prec, shape, kw, sw, reuse in cases():
        head = "%-10s %-3s %2dx%dx%d %s%s" % (label, prec, *shape, " ".join(f"{k}={v!r}" for k, v in sw.items()) or "-", "" if reuse else " reuse=False")
        if args.only in head:
            print(head, digest(sd, prec, shape, kw, sw, reuse), flush=True)


if __name__ == "__main__":
    main()
