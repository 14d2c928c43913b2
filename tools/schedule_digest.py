#!/usr/bin/env python3
"""blake2b of Graph.blob() -- every launch descriptor, every packed weight, the arena size, the output layout -- for a fixed list of
schedules and SMAP_* switch settings, one line per case: two versions of the schedule builder (smap_amd/engine.py) that claim to build
the same schedules print the same lines.  CPU only (the library is not loaded).  Weights: recipe_state_dict of a seed-0 SMAP, as
tests/test_host_cpu.py's small_sd.  A case the builder refuses prints the exception's type in place of the digest.
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


def cases():
    """(label, precision, (B, H, W), Graph keyword arguments, switches) in a fixed order."""
    flip = list(cfg.DATASET.KEYPOINT.FLIP_ORDER) + [cfg.DATASET.KEYPOINT.NUM + c for c in cfg.DATASET.PAF.FLIP_CHANNEL]
    small, one, eight = (2, 64, 96), (1, 512, 832), (8, 512, 832)
    for prec in BOTH:                                     # the default environment
        for shape in (small, one, eight):
            yield "default", prec, shape, {}, {}
        yield "flip_pair", prec, eight, dict(flip_pair=flip), {}
        yield "all_heads", prec, eight, dict(all_heads=True), {}
        yield "scaled_hms", prec, eight, dict(scaled_hms=True), {}
        yield "conftest", prec, small, {}, CONFTEST
    yield "default", "x3", (16, 512, 832), {}, {}
    # every switch in turn on the small schedule, on top of the conftest setting, in the precision its tests use
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
        yield "switch", prec, small, {}, {**CONFTEST, **sw}
    # the real batch-1 rules (no conftest switches)
    yield "switch", "x3", one, {}, dict(SPLITK_MINK="1024")
    yield "switch", "x3", one, {}, dict(BLOCK="64:91,128:94")


def digest(sd, prec, shape, kw, sw):
    for k in SWITCHES:
        os.environ.pop("SMAP_" + k, None)
    for k, v in sw.items():
        os.environ["SMAP_" + k] = v
    try:
        g = Graph(sd, *shape, precision=prec, **kw)
        g.allocate()
        return "%s n_ops %d lanes %d flops %d alg_bytes %d arena_bytes %d" % (
            hashlib.blake2b(g.blob(), digest_size=16).hexdigest(), len(g.ops), int(g.lanes), g.flops, g.alg_bytes, g.arena_bytes)
    except Exception as exc:                              # noqa: BLE001  (a refused case is a result too)
        return type(exc).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="run the cases whose line contains this text")
    args = ap.parse_args()
    torch.manual_seed(0)
    sd = recipe_state_dict(SMAP(make_cfg((16, 24))).state_dict())
    for label, prec, shape, kw, sw in cases():
        head = "%-10s %-3s %2dx%dx%d %s" % (label, prec, *shape, " ".join(f"{k}={v!r}" for k, v in sw.items()) or "-")
        if args.only in head:
            print(head, digest(sd, prec, shape, kw, sw), flush=True)


if __name__ == "__main__":
    main()
