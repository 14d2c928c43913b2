"""Host side of the SMAP backbone on MI355X: folds the checkpoint, lays the static
inference schedule out as an array of `smap_op` (include/smap_hip.h) and runs it
through libsmap_hip.so.  Python only DESCRIBES the schedule; every kernel launch
happens inside smap_plan_run (csrc/plan.hip).

Reference being replaced: model/smap.py SMAP.forward, inference branch (:403-419).

What the schedule does differently from a layer-by-layer replay (all exact up to
floating-point rounding):
  * eval-mode BatchNorm is folded into the conv weights / bias (smap.py:13-45);
  * heads that the inference branch never returns are not computed (smap.py:417-419 uses
    only stage-2 res2..4, res_d4, res_rd4): 62 of the 268 convs -- unless the schedule is built with all_heads=True (the validation
    loss), which adds them and keeps all 36 head tensors;
  * `up_conv(bilinear_up(x))` (smap.py:214-215) is evaluated as `bilinear_up(up_conv(x))`:
    a 1x1 conv + per-channel affine commutes with the (convex, per-channel) bilinear
    resampling, which moves the 256->256 GEMM to the 4x smaller grid;
  * the three 1x1 head convs of stage-2/up4 share their input and run as one N=768 GEMM;
  * the 1x1 convs of an Upsample_unit that read the same tensor (smap.py:210-241: skip2 | cross_conv / res_conv1 | the next unit's
    up_conv on `out`; u_skip | skip1 on x where u_skip has no bilinear add) run as ONE launch with one output tensor each (conv_seg);
  * layer1's Bottlenecks and layer2's identity Bottlenecks run as one launch each (conv_block*, csrc/convb.hip / convc.hip);
  * small schedules (batch 1): the long-K launches split their K loop over several workgroups per output tile (split_k);
  * residual add, ReLU and the inter-stage skip adds (smap.py:142-153) run in the
    epilogue of the producing conv.
Activations are NHWC fp16, accumulation fp32, head outputs fp32 (precision "f16"), or -- precision "x3", the mode
whose results meet the reference's fp32 arithmetic -- every activation and weight as an fp16 hi/lo PAIR (22 significant
bits) with three MFMAs per K step (csrc/conv.hip, template X3): ~1e-6 relative error through the whole graph instead of
~1e-3, at 3x the matrix work and 2x the bytes.
"""
import ctypes as C
import os
from collections import namedtuple
from dataclasses import dataclass, field, fields

import torch

from . import lib as _L

OP_CONV, OP_STEM, OP_MAXPOOL, OP_UPADD, OP_HEADSUM, OP_STEMPOOL, OP_TAPSUM = range(7)

# ----------------------------------------------------------------------------- tile ids
# What every conv tile id (smap_op.tile) means, written down ONCE for the Python side; the C side keeps the same rows in csrc/tiles.h
# (per-row notes on LDS size / waves / why a variant exists live there), tests/test_host_cpu.py compares the two fact by fact.
#   family: "igemm" (csrc/conv.hip), "halo" (csrc/conv3.hip: plain 3x3 stride-1), "persist" (csrc/convp.hip: persistent workgroups, register
#           epilogue), "tail" (csrc/convf.hip: a Bottleneck's 3x3 with the following 1x1 fused in), "block" (csrc/convb.hip / convc.hip: a
#           whole Bottleneck per launch)
#   bm, bn: output tile, pixels x channels;  bk16, bkx3: halves per staged K tile in fp16 / split precision
#   prec:   the precisions the id has an instance in ("f16 x3" unless said)
#   caps:   further instances of the conv.hip kernel: "splitk", "dual" (second input along K), "relusum" (relu(conv) + relu(conv)),
#           "regepi" (register epilogue INSTEAD of the LDS-staged one), "tapdot"
#   tail_bn: output channels per chunk of the fused 1x1 tail;  planes, first: the Bottleneck a "block" tile runs (first = with a shortcut conv)
Tile = namedtuple("Tile", "family bm bn bk16 bkx3 caps tail_bn planes first prec", defaults=("", 0, 0, False, "f16 x3"))
TILE_TABLE = {
    # 0..4: two-stage pipelines of 64-half K tiles; 5..9: the same tiles with deeper LDS-DMA pipelines
    0: Tile("igemm", 128, 128, 64, 64), 1: Tile("igemm", 128, 64, 64, 64), 2: Tile("igemm", 64, 64, 64, 64, "splitk"),
    3: Tile("igemm", 128, 32, 64, 64), 4: Tile("igemm", 64, 128, 64, 64),
    5: Tile("igemm", 128, 128, 64, 32, prec="f16"), 6: Tile("igemm", 128, 64, 64, 32, prec="f16"), 7: Tile("igemm", 64, 64, 64, 64, "splitk"),
    8: Tile("igemm", 128, 32, 64, 32, prec="f16"), 9: Tile("igemm", 64, 128, 64, 32, prec="f16"),
    # (ids 10..18 belonged to a register-epilogue GEMM that no measured table entry selected: tools/experiments/, outside the product build)
    # 20..27: BK = 32 staging (LDS-staged epilogue kept)
    20: Tile("igemm", 128, 128, 32, 32, "splitk dual"), 21: Tile("igemm", 128, 64, 32, 32), 22: Tile("igemm", 64, 64, 32, 32, "splitk"),
    23: Tile("igemm", 64, 128, 32, 32), 24: Tile("igemm", 128, 128, 32, 32), 25: Tile("igemm", 128, 64, 32, 32),
    26: Tile("igemm", 64, 64, 32, 32), 27: Tile("igemm", 64, 128, 32, 32),
    # 30..39: halo-tiled 3x3, BM = 128 output pixels as an 8x16 / 4x32 patch (34..37: deeper weight pipeline; 38, 39: Cout <= 32 heads)
    30: Tile("halo", 128, 64, 64, 32), 31: Tile("halo", 128, 128, 64, 32), 32: Tile("halo", 128, 64, 64, 32), 33: Tile("halo", 128, 128, 64, 32),
    34: Tile("halo", 128, 64, 64, 32), 35: Tile("halo", 128, 128, 64, 32), 36: Tile("halo", 128, 64, 64, 32), 37: Tile("halo", 128, 128, 64, 32),
    38: Tile("halo", 128, 32, 64, 32), 39: Tile("halo", 128, 32, 64, 32),
    # 40..45: the same kernel with EIGHT waves: 8x16 pixels (two workgroups per CU), 16x16 / 16x16 x 64 channels / 8x32 (one); 44, 45 = 41, 43
    # with the two waves of a SIMD half an iteration apart
    40: Tile("halo", 128, 128, 64, 32), 41: Tile("halo", 256, 128, 64, 32), 42: Tile("halo", 256, 64, 64, 32), 43: Tile("halo", 256, 128, 64, 32),
    44: Tile("halo", 256, 128, 64, 32), 45: Tile("halo", 256, 128, 64, 32),
    # 50..55: conv.hip with EIGHT waves per workgroup (the low-resolution layers); 55: 4-stage pipeline (bytes in flight for the streaming layers)
    50: Tile("igemm", 128, 128, 32, 32, "dual relusum"), 51: Tile("igemm", 128, 128, 32, 32, "dual relusum"), 52: Tile("igemm", 128, 128, 64, 64),
    53: Tile("igemm", 256, 128, 32, 32, "dual relusum"), 54: Tile("igemm", 128, 256, 32, 32, "dual relusum tapdot"), 55: Tile("igemm", 128, 128, 32, 32),
    # 56: 256 x 256, half the L2 -> LDS bytes per MFMA of the 128 x 128 tiles.  Split precision, fp16 outputs, residual + ReLU only
    56: Tile("igemm", 256, 256, 64, 32, "regepi", prec="x3"),
    # 60..65: persistent workgroups with loader waves (no fused bilinear add, no fp32 out)
    60: Tile("persist", 128, 256, 32, 32), 61: Tile("persist", 256, 128, 32, 32), 62: Tile("persist", 128, 128, 32, 32),
    63: Tile("persist", 128, 64, 32, 32), 64: Tile("persist", 128, 64, 32, 32), 65: Tile("persist", 128, 64, 32, 32),
    # 80..82: a Bottleneck's 3x3 (BN = all of its planes) with the following 1x1 fused in
    80: Tile("tail", 128, 64, 64, 32, tail_bn=64), 81: Tile("tail", 128, 64, 64, 32, tail_bn=128), 82: Tile("tail", 128, 128, 64, 32, tail_bn=64),
    # 90, 91: a whole identity Bottleneck of 64 planes (1x1 -> 3x3 -> 1x1 + residual) per 4x16 / 8x16 pixel tile; 92, 93: the same for the FIRST
    # block of layer1 (64 input channels, 1x1 shortcut conv instead of the identity residual); 94: 128 planes / 512 channels (layer2), eight waves
    90: Tile("block", 64, 64, 64, 32, tail_bn=64, planes=64, prec="x3"), 91: Tile("block", 128, 64, 64, 32, tail_bn=64, planes=64, prec="x3"),
    92: Tile("block", 64, 64, 64, 32, tail_bn=64, planes=64, first=True, prec="x3"), 93: Tile("block", 128, 64, 64, 32, tail_bn=64, planes=64, first=True, prec="x3"),
    94: Tile("block", 128, 128, 64, 32, tail_bn=128, planes=128, prec="x3")}


def tile_family(tile):
    return TILE_TABLE[tile].family


def tile_bk(tile, x3):
    """Halves per K chunk of the LDS rows a tile id stages = the packing unit of its weights.  The halo
    kernels' rows are always 128 bytes: 64 channels, or [hi32 | lo32] of 32 channels in split precision."""
    return TILE_TABLE[tile].bkx3 if x3 else TILE_TABLE[tile].bk16


def tile_has(tile, cap=None, x3=False):
    """Does tile id `tile` have an instance in this precision -- and, with `cap`, that further instance of it?"""
    row = TILE_TABLE.get(tile)
    return row is not None and ("x3" if x3 else "f16") in row.prec.split() and (cap is None or cap in row.caps.split())


def tile_ids(family=None, cap=None, x3=None):
    """Tile ids, ascending: of these families (one name or several), with this capability, with an instance in this precision (None: any)."""
    fams = None if family is None else (family,) if isinstance(family, str) else tuple(family)
    return tuple(t for t, r in sorted(TILE_TABLE.items()) if (fams is None or r.family in fams)
                 and (tile_has(t, cap, x3) if x3 is not None else tile_has(t, cap, False) or tile_has(t, cap, True)))


# names older call sites import: one-line views of the table
TILES = {t: (r.bm, r.bn) for t, r in TILE_TABLE.items()}                      # tile id -> (BM, BN)
TAIL_BN = {t: r.tail_bn for t, r in TILE_TABLE.items() if r.tail_bn}          # tile id -> output channels per chunk of the fused 1x1
HALO_ROWS = ("halo", "tail", "block")     # families whose 3x3 weights are packed as 128-byte halo rows (pack_halo_rows)
TAIL_DEFAULT = {}                          # Bottleneck planes -> fused tile id (empty: every block runs c2 and c3 as two launches)
# Bottleneck planes -> tile id of the WHOLE-block launch (csrc/convb.hip) for stride-1 identity blocks in split precision; {} = off.
# BLOCK_FIRST_DEFAULT: the same for the first block of layer1 (the one with a shortcut conv; 64 input channels).
# Measured in situ (profiles/r4_v4_ab_whole_block_first.log, same box, interleaved): 781 -> 800 (identity blocks, 8 x 16 tiles) -> 821
# frames/s (+ first blocks); 4 x 16 tiles: 816.
BLOCK_DEFAULT = {64: 91, 128: 94}       # layer1 (csrc/convb.hip) and layer2 (csrc/convc.hip) identity blocks
BLOCK_FIRST_DEFAULT = {64: 93}


# ----------------------------------------------------------------------------- schedule switches
_HERE = os.path.dirname(os.path.abspath(__file__))
_TABLE_FILES = {}       # (path, mtime, size) -> parsed tile table: SchedulePolicy.from_env runs once per Graph, hundreds of times in the tests


def _load_table(path):
    """A measured tile table (json: shape key -> tile id or ranked list of ids) by path; {} when there is no such file."""
    if not os.path.exists(path):
        return {}
    st = os.stat(path)
    key = (path, st.st_mtime_ns, st.st_size)
    if key not in _TABLE_FILES:
        import json
        _TABLE_FILES[key] = json.load(open(path))
    return _TABLE_FILES[key]


@dataclass(frozen=True)
class SchedulePolicy:
    """Every switch that changes what Graph builds, as one value: read from the SMAP_* environment variables ONCE (from_env, the only
    place this file reads them), kept by the Graph built under it (Graph.policy) and hashed into the plan cache key (cache_token).  All
    of them are A/B hooks and test handles; the defaults are the shipped schedule."""
    block: tuple = None
    """SMAP_BLOCK="64:91,128:94": (Bottleneck planes, tile id) of the whole-block launches; () = none; None (unset) = the rule of Graph.block_tile."""
    block_first: tuple = None
    """SMAP_BLOCK_FIRST="64:93": the same for layer1's first block; None (unset) = BLOCK_FIRST_DEFAULT, 92 for 93 in small schedules."""
    tail: tuple = None
    """SMAP_TAIL="64:80,128:82": (planes, tile id) pairs of the fused 3x3 + 1x1 launches (Graph.conv_tail); None (unset) = TAIL_DEFAULT."""
    cat: bool = None
    """SMAP_CAT=0|1: a Bottleneck's last 1x1 and its shortcut conv as one launch (Graph.conv_cat) never / in small schedules too; None = in all but those."""
    skipsum: bool = None
    """SMAP_SKIPSUM=0|1: skip1 + skip2 of an Upsample_unit as one launch and one tensor (Graph.conv_relusum), the same way."""
    taphead: bool = None
    """SMAP_TAPHEAD=0|1: the root-depth head as tap-dot launch + stencil (Graph.conv_tapdot / tapsum), the same way."""
    merge_1x1: int = 1
    """SMAP_MERGE_1X1: shared-input 1x1s of an Upsample_unit as one launch (Graph.conv_seg): 1 = the merges that pay, 2 = all of them, 0 = one launch per conv."""
    splitk: str = ""
    """SMAP_SPLITK: "" (unset or "1") = the measured rule of Graph.split_k, "0" = off, "<n>" = n parts wherever a launch qualifies, "t<n>" = aim at n workgroups."""
    splitk_mink: int = 2048
    """SMAP_SPLITK_MINK: shortest K loop the measured split-K rule shares out (re-measured with the release / acquire ticket: EXPERIMENTS R6.5)."""
    deep_tile: bool = True
    """SMAP_DEEP_TILE=0 switches Graph.deep_pipeline_tile (tile 2 -> 7 for launches of <= 256 workgroups, profiles/r5_v9_*) off."""
    lanes: bool = False
    """SMAP_LANES=1: the independent head chains on forked streams (Graph.lanes; profiles/r5_v3_ab_b1.log)."""
    wpairs: int = None
    """SMAP_WPAIRS=0|1 forces one layout of the packed 32-half weight tiles; None = pairs in small schedules (Graph.w_pairs; profiles/r3_ab_wpairs*.log)."""
    x3_tile: int = None
    """SMAP_X3_TILE: one split-precision tile id put before the table's candidates wherever it fits (Graph._pick)."""
    cat_tile: int = None
    """SMAP_CAT_TILE: tile id of every Graph.conv_cat launch."""
    relusum_tile: int = None
    """SMAP_RELUSUM_TILE: tile id of every Graph.conv_relusum launch (profiles/r6_v14_ab_two_input_tiles.log)."""
    halo3: tuple = None
    """SMAP_HALO3="16" | "32" [":64" | ":128"]: (pixel-tile width, BN or None) -- every plain 3x3 with Cout > 32 on that halo tile (csrc/conv3.hip)."""
    halo3_deep: bool = False
    """SMAP_HALO3_DEEP: ... on its variant with the deeper weight pipeline (tile id + 4)."""
    tile_remap: tuple = ()
    """SMAP_TILE_REMAP="0:5,1:6": (tile id, tile id) pairs that swap variants of one tile shape (other pipeline depth) without touching the schedule."""
    tile_policy: str = ""
    """SMAP_TILE_POLICY="traffic[:min blocks]": experiment of pick_tile -- fewest L2 -> LDS bytes subject to a minimum block count (fp16)."""
    stempool: bool = False
    """SMAP_STEMPOOL: ResNet_top as one kernel that writes the pooled tensor only (bit-identical, no faster inside the two-batch pipeline)."""
    no_upadd_fusion: bool = False
    """SMAP_NO_UPADD_FUSION: fp16 with SMAP_MERGE_1X1=0 -- the bilinear add as a launch of its own (SMAP_OP_UPADD) instead of the u_skip conv's epilogue."""
    tile_table: dict = field(default_factory=dict, repr=False)
    """The measured fp16 table (pick_tile): SMAP_TILE_TABLE=<json>, default smap_amd/tile_table.json; {} under SMAP_NO_TILE_TABLE."""
    tile_table_x3: dict = field(default_factory=dict, repr=False)
    """The measured split-precision table (pick_tile_x3): SMAP_TILE_TABLE_X3=<json>, default smap_amd/tile_table_x3.json; {} under SMAP_NO_TILE_TABLE."""

    @classmethod
    def from_env(cls, environ=os.environ):
        """The policy that the SMAP_* variables of `environ` describe."""
        get = lambda name, default="": environ.get("SMAP_" + name, default)
        pairs = lambda spec: None if spec is None else tuple((int(a), int(b)) for a, b in (kv.split(":") for kv in spec.split(",") if ":" in kv))
        tri = lambda name: {"0": False, "1": True}.get(get(name))
        num = lambda name: int(get(name)) if get(name) else None
        remap = pairs(get("TILE_REMAP"))
        assert all(TILES[a] == TILES[b] for a, b in remap), "remap must keep the tile shape"
        tw, _, bn = get("HALO3").partition(":")
        table = lambda name, shipped: {} if get("NO_TILE_TABLE") else _load_table(get(name) or os.path.join(_HERE, shipped))
        return cls(block=pairs(get("BLOCK", None)), block_first=pairs(get("BLOCK_FIRST", None)), tail=pairs(get("TAIL", None)),
                   cat=tri("CAT"), skipsum=tri("SKIPSUM"), taphead=tri("TAPHEAD"), merge_1x1={"0": 0, "2": 2}.get(get("MERGE_1X1"), 1),
                   splitk="" if get("SPLITK") == "1" else get("SPLITK"), splitk_mink=int(get("SPLITK_MINK", "2048")),
                   deep_tile=get("DEEP_TILE") != "0", lanes=get("LANES") == "1", wpairs={"0": 0, "1": 1}.get(get("WPAIRS")),
                   x3_tile=num("X3_TILE"), cat_tile=num("CAT_TILE"), relusum_tile=num("RELUSUM_TILE"),
                   halo3=(int(tw), int(bn) if bn else None) if tw else None, halo3_deep=bool(get("HALO3_DEEP")), tile_remap=remap,
                   tile_policy=get("TILE_POLICY"), stempool=bool(get("STEMPOOL")), no_upadd_fusion=bool(get("NO_UPADD_FUSION")),
                   tile_table=table("TILE_TABLE", "tile_table.json"), tile_table_x3=table("TILE_TABLE_X3", "tile_table_x3.json"))

    def cache_token(self):
        """What the plan cache key hashes: every field in declaration order, the two tables as a digest of their parsed content."""
        import hashlib
        import json
        digest = lambda t: hashlib.blake2b(json.dumps(t, sort_keys=True).encode(), digest_size=16).hexdigest()
        return tuple((f.name, digest(v) if isinstance(v, dict) else v) for f in fields(self) for v in (getattr(self, f.name),))


LAYERS = (3, 4, 6, 3)            # smap.py:299  resnet-50
PLANES = (64, 128, 256, 512)
ALIGN = 256
ZERO_PAGE = 16384             # csrc/plan.hip SMAP_ZERO_PAGE
WINDOW = 1 << 32              # csrc/plan.hip SMAP_WINDOW: bytes [k * WINDOW, k * WINDOW + ZERO_PAGE) of the arena are reserved
PRECISIONS = ("f16", "x3")


def split_f16(w, scaled=True):
    """f64 tensor -> (hi, lo fp16 tensors of w * 2^s, 2^-s): hi = fp16(w 2^s), lo = fp16(w 2^s - hi).  s puts max |w| in
    [2^13, 2^14) so that the lo parts of all but vanishing weights are normal fp16 numbers."""
    import math
    m = float(w.abs().max())
    s = (13 - math.frexp(m)[1] + 1) if (scaled and m > 0) else 0          # frexp: m = f * 2^e, f in [0.5, 1)
    ws = w.double() * (2.0 ** s)
    hi = ws.to(torch.float16)
    lo = (ws - hi.double()).to(torch.float16)
    assert torch.isfinite(hi).all()
    return hi, lo, 2.0 ** -s


def pack_stem_weights(w, x3):
    """The stem's [64, 3, 7, 7] f64 weights -> (what SMAP_OP_STEM / STEMPOOL read at w_off, acc_scale): fp16 [64][22][8], K = (kh, c, kw
    7->8) + one zero granule; split precision: the hi and the lo matrix of w * 2^s one behind the other, acc_scale = 2^-s."""
    if x3:
        hi, lo, scale = split_f16(w.permute(0, 2, 1, 3).reshape(64, 21, 7))
        wk = torch.zeros((2, 64, 22, 8), dtype=torch.float16)
        wk[0, :, :21, :7], wk[1, :, :21, :7] = hi, lo
        return wk.reshape(2, 64, 176), scale
    wk = torch.zeros((64, 22, 8), dtype=torch.float16)
    wk[:, :21, :7] = w.permute(0, 2, 1, 3).reshape(64, 21, 7).to(torch.float16)
    return wk.reshape(64, 176), 1.0


def _table_entry(v):
    """A table value is one tile id or a ranked list of them (best first): the specialised kernels do not take every op of
    a shape (conv3.hip: plain 3x3 only; convp.hip: no fused bilinear add, no fp32 output), Graph.conv picks the first
    entry that is legal for the op at hand."""
    return [int(t) for t in v] if isinstance(v, (list, tuple)) else [int(v)]


def tile_legal(tile, *, cout, cout_pad=None, plain3=True, up=False, out_fp32=False, adds=False, x3=True):
    """Can tile id `tile` run an op with these properties?  Mirrors csrc/plan.hip::validate."""
    fam = tile_family(tile)
    if tile_has(tile, "regepi", True):
        return x3 and not up and not out_fp32 and not adds and cout % 8 == 0
    if fam == "halo":
        return plain3
    if fam in ("tail", "block"):
        return False                     # only Graph.conv_tail / Graph.conv_block build these
    if fam == "persist":
        cp = cout_pad if cout_pad is not None else _rup(cout, TILES[tile][1])
        return not up and not out_fp32 and cout % 8 == 0 and cp <= 2048
    return True


def pick_tile_x3(M, cout, key=None, policy=None):
    """Split precision: candidates in order of preference -- the measured table (tools/autotune.py --precision x3 ->
    smap_amd/tile_table_x3.json) when the shape is in it, then the largest BK = 32 tile that still gives >= 512
    workgroups / the one with most workgroups.  policy: whose table (None: the environment's)."""
    table = (policy or SchedulePolicy.from_env()).tile_table_x3
    keys = [key] if isinstance(key, str) else list(key or [])          # several keys: most specific first
    # a batch size the table was not tuned for borrows the entries of the nearest tuned one (same layer shape, M within 2x-4x):
    # closer to the optimum than the block-count heuristic (tuned tables: +8 % at batch 8, +7 % at 16, +19 % at 1)
    tuned = sorted({int(k.split(",")[0]) for k in table})
    if keys and tuned:
        f = int(keys[0].split(",")[0])
        if f not in tuned:
            import math
            near = min(tuned, key=lambda b: abs(math.log(b / f)))
            keys = keys + [",".join([str(near)] + k.split(",")[1:]) for k in keys]
    cands = [t for k in keys if k in table for t in _table_entry(table[k])]
    if cout <= 32:
        return cands + [3]
    best, best_blocks = None, -1
    for t in ((21, 22) if cout <= 64 else (20, 23, 21, 22)):
        bm, bn = TILES[t]
        blocks = -(-M // bm) * (-(-cout // bn))
        if blocks >= 512:
            return cands + [t]
        if blocks > best_blocks:
            best, best_blocks = t, blocks
    return cands + [best]


def pack_conv_weights(w2, tile, x3, ksize, cin, pairs=True):
    """fp16 [planes][cout_pad][K] (K = (kh, kw, cin), planes = hi | lo in split precision) -> the byte image the conv kernels'
    LDS-DMA reads, as ONE CONTIGUOUS BLOCK PER STAGED WEIGHT TILE: [n tile][K tile][plane][row][16-byte slot], the slot
    order already carrying the kernels' XOR swizzle -- a weight tile is then BN x row-bytes of consecutive addresses, i.e.
    every wave-wide global_load_lds reads one contiguous KiB.  (Strided 64-byte row segments out of a [cout][K] matrix
    stream from L2 at half the rate: profiles/r3_v3_ubench_lds_dma_rows.log; weight tiles are re-streamed by every M tile
    and were the larger half of the L2 -> LDS traffic.)
      igemm / persist (csrc/conv.hip, convp.hip): K tile = BK halves in (kh, kw, cin) order; slot s of row r holds granule
        s ^ ((r >> 1) & 7) (BK = 64) or s ^ ((r >> 2) & 3) (BK = 32); 32-half tiles come in pairs [n tile][pair][plane][row]
        [tile 2p | tile 2p+1]: 128-byte rows again, the second half of every fetched cache line is the next K tile;
      halo (csrc/conv3.hip): tiles ordered [channel chunk][tap]; 128-byte rows of 64 channels, or in split precision of
        32 channels as logical granules 0..3 = hi, 4..7 = lo; slot s of row r holds logical granule s ^ ((r >> 1) & 7)."""
    planes, cout_pad, K = w2.shape
    assert planes == (2 if x3 else 1) and K == ksize * ksize * cin
    bn = TILES[tile][1]
    nt = cout_pad // bn
    assert nt * bn == cout_pad
    r = torch.arange(bn)
    if tile_family(tile) in HALO_ROWS:
        assert ksize == 3
        return pack_halo_rows(w2, bn, 9, cin, x3)
    bk = tile_bk(tile, x3)
    spr = bk // 8
    kt = K // bk
    assert kt * bk == K
    rows = w2.reshape(planes, nt, bn, kt, spr, 8).permute(1, 3, 0, 2, 4, 5)          # [nt][kt][plane][row][granule][8]
    swz = ((r >> 1) & 7) if bk == 64 else ((r >> 2) & 3)
    idx = torch.arange(spr)[None, :] ^ swz[:, None]
    tiles = rows[:, :, :, r[:, None], idx, :]                                        # slot order of the LDS image
    if bk == 32 and pairs:
        # 32-half K tiles are stored in PAIRS: a 128-byte row = [K tile 2p (64 B) | K tile 2p+1 (64 B)], so that the cache line
        # a K tile's load brings in also serves the next K tile (small launches are latency-bound: the L1 hit matters there)
        assert kt % 2 == 0
        tiles = tiles.reshape(nt, kt // 2, 2, planes, bn, spr, 8).permute(0, 1, 3, 4, 2, 5, 6)   # [nt][pair][plane][row][half][4][8]
    return tiles.contiguous()


def pack_halo_rows(w2, bn, taps, cin, x3):
    """[planes][cout_pad][K = (tap, cin)] -> blocks [n tile][channel chunk][tap][bn rows][8 slots][8 halves] of 128-byte rows
    (csrc/conv3.hip; taps = 1: the fused 1x1 of csrc/convf.hip, bn = its chunk of output channels)."""
    planes, cout_pad, K = w2.shape
    assert K == taps * cin and cout_pad % bn == 0
    nt = cout_pad // bn
    ch = 32 if x3 else 64
    cch = cin // ch
    assert cch * ch == cin
    r = torch.arange(bn)
    w = w2.reshape(planes, nt, bn, taps, cch, ch // 8, 8)
    if x3:       # logical granule = plane * 4 + g
        rows = w.permute(1, 4, 3, 2, 0, 5, 6).reshape(nt, cch, taps, bn, 8, 8)
    else:
        rows = w[0].permute(0, 3, 2, 1, 4, 5)
    idx = torch.arange(8)[None, :] ^ ((r[:, None] >> 1) & 7)
    return rows[:, :, :, r[:, None], idx, :].contiguous()


def pack_rows16(w2):
    """[2 planes][rows][K] (hi | lo) -> [K / 16][rows][4 slots][8 halves]: the 16-channel stages of csrc/convb.hip's leading 1x1 --
    64-byte rows [hi16 | lo16], logical granule = plane * 2 + g (g = which 8 of the 16 channels), slot s of row r holds
    granule s ^ ((r >> 2) & 3)."""
    planes, rows, K = w2.shape
    assert planes == 2 and K % 16 == 0
    w = w2.reshape(2, rows, K // 16, 2, 8).permute(2, 1, 0, 3, 4).reshape(K // 16, rows, 4, 8)
    r = torch.arange(rows)
    idx = torch.arange(4)[None, :] ^ ((r[:, None] >> 2) & 3)
    return w[:, r[:, None], idx, :].contiguous()


def unpack_halo_rows(packed, bn, taps, cin, cout_pad, x3):
    planes, K = (2 if x3 else 1), taps * cin
    perm = pack_halo_rows(torch.arange(planes * cout_pad * K, dtype=torch.int64).reshape(planes, cout_pad, K), bn, taps, cin, x3).reshape(-1)
    out = torch.empty(planes * cout_pad * K, dtype=packed.dtype)
    out[perm] = packed.reshape(-1)
    return out.reshape(planes, cout_pad, K)


def unpack_conv_weights(packed, tile, x3, ksize, cin, cout_pad, pairs=True):
    """Inverse of pack_conv_weights: the flat fp16 image -> [planes][cout_pad][K] (oracle/graph_interp.py, tests)."""
    planes, K = (2 if x3 else 1), ksize * ksize * cin
    perm = pack_conv_weights(torch.arange(planes * cout_pad * K, dtype=torch.int64).reshape(planes, cout_pad, K),
                             tile, x3, ksize, cin, pairs=pairs).reshape(-1)
    out = torch.empty(planes * cout_pad * K, dtype=packed.dtype)
    out[perm] = packed.reshape(-1)
    return out.reshape(planes, cout_pad, K)


def _rup(x, m):
    return (x + m - 1) // m * m


# ----------------------------------------------------------------------------- folding
def fold_conv_bn(sd, prefix, eps=1e-5):
    """conv_bn_relu (smap.py:13-45) in eval mode -> (w [Cout,Cin,kh,kw] f64, b [Cout] f64)."""
    w = sd[prefix + ".conv.weight"].double()
    b = sd[prefix + ".conv.bias"].double()
    g = sd[prefix + ".bn.weight"].double()
    beta = sd[prefix + ".bn.bias"].double()
    mu = sd[prefix + ".bn.running_mean"].double()
    var = sd[prefix + ".bn.running_var"].double()
    s = g / torch.sqrt(var + eps)
    return w * s[:, None, None, None], (b - mu) * s + beta


# ----------------------------------------------------------------------------- graph IR
@dataclass
class Tensor:
    name: str
    B: int
    H: int
    W: int
    C: int                 # channel stride of a pixel
    esize: int = 2         # bytes per element (2 = fp16, 4 = fp32)
    planes: int = 1        # 2 = split precision: a pixel is [hi(C) | lo(C)] fp16
    first: int = -1
    last: int = -1
    off: int = -1

    @property
    def nbytes(self):
        return self.B * self.H * self.W * self.C * self.esize * self.planes


@dataclass
class Op:
    kind: int
    out: Tensor = None
    inp: Tensor = None
    res: Tensor = None
    add1: Tensor = None
    add2: Tensor = None
    aux: list = field(default_factory=list)
    p: dict = field(default_factory=dict)
    lane: int = 0                                 # stream lane (smap_op.lane): 0 = the caller's stream
    outs: list = field(default_factory=list)      # further output tensors (N segments 1, 2 of a merged 1x1 launch)
    aux2: Tensor = None                           # second input, concatenated along K (Graph.conv_cat)
    scratch: list = field(default_factory=list)   # arena scratch that lives for this op only (split K: the partial tiles)

    # Every Tensor field above is named in exactly ONE of reads() / writes() / scratch: what Graph.allocate and Graph.emit enumerate.
    def reads(self):
        return [t for t in [self.inp, self.res, self.add1, self.add2, self.aux2] + list(self.aux) if t is not None]

    def writes(self):
        return ([self.out] if self.out is not None else []) + list(self.outs)


def pick_tile_heuristic(M, cout):
    """Largest tile that still gives >= 2 waves of workgroups on 256 CUs."""
    if cout <= 32:
        return 3
    cands = [1, 2] if cout <= 64 else [0, 1, 2]
    best, best_blocks = None, -1
    for t in cands:
        bm, bn = TILES[t]
        blocks = -(-M // bm) * (-(-cout // bn))
        if blocks >= 512:
            return t
        if blocks > best_blocks:
            best, best_blocks = t, blocks
    return best


def pick_tile(M, cout, key=None, policy=None):
    """Measured table (tools/autotune.py -> smap_amd/tile_table.json, keyed "B,H,W,Cin,Cout,k,s")
    when the shape is in it, else the block-count heuristic.  policy: whose table and tile_policy (None: the environment's)."""
    policy = policy or SchedulePolicy.from_env()
    pol = policy.tile_policy
    if pol.startswith("traffic"):       # experiment: minimise L2->LDS bytes subject to a minimum block count
        min_blocks = int(pol.split(":")[1]) if ":" in pol else 256
        K = 1
        if key is not None:
            _, _, _, cin, _, ks, _ = map(int, key.split(","))
            K = ks * ks * cin
        best, best_cost = None, None
        for t in ([3] if cout <= 32 else [0, 1, 2, 4]):
            bm, bn = TILES[t]
            if cout <= 64 and bn > 64:
                continue
            mt, nt = -(-M // bm), -(-cout // bn)
            cost = (mt * bm * nt + nt * bn * mt) * K
            if mt * nt < min_blocks:
                cost *= 4
            if best is None or cost < best_cost:
                best, best_cost = t, cost
        return best
    if key is not None and key in policy.tile_table:
        return _table_entry(policy.tile_table[key])[0]
    return pick_tile_heuristic(M, cout)


class ArenaTooLarge(ValueError):
    """The schedule does not fit: ONE activation tensor exceeds a 4 GiB window (the conv kernels address their input with 32-bit
    byte offsets from a 4 GiB-aligned base, csrc/plan.hip: 52 frames of the widest split-precision tensor), or the whole arena
    exceeds the memory budget (BackboneEngine: SMAP_MAX_ARENA_BYTES, default 90 % of the device's memory / 4 arenas -- a pipeline keeps
    one arena per backbone in flight and per schedule size).  Either way: run the frames in smaller launches
    (PosePipeline splits by itself)."""


ARENAS_PER_DEVICE = 4       # what a pipeline keeps: `depth` (2) backbones in flight x (the coalesced schedule + the batch-sized one for trailing groups)


def arena_budget(device):
    """Bytes ONE activation arena may take on `device`: SMAP_MAX_ARENA_BYTES, else 90 % of the device's TOTAL memory shared out over the
    arenas a pipeline keeps (SMAP_ARENAS_PER_DEVICE, default 4).  (Round 5 took 45 % of what happened to be FREE when the engine was built:
    the chunking of a pipeline -- hence its throughput -- then depended on the allocator's state and on which engine was built first.)"""
    env = os.environ.get("SMAP_MAX_ARENA_BYTES", "")
    if env:
        return int(float(env))
    _, total = torch.cuda.mem_get_info(device)
    return int(0.9 * total / max(1, int(os.environ.get("SMAP_ARENAS_PER_DEVICE", ARENAS_PER_DEVICE))))


class _FreeList:
    """The free byte ranges of the arena, as Graph._place uses them."""
    def __init__(self):
        self.blocks = []                 # (off, size); sorted and merged by give(), remainders of take() at the end

    def take(self, need):
        """Best fit: the offset of `need` bytes at the head of the smallest block that holds them (the first such in list order), or None."""
        pick = None
        for k, (_, sz) in enumerate(self.blocks):
            if sz >= need and (pick is None or sz < self.blocks[pick][1]):
                pick = k
        if pick is None:
            return None
        off, sz = self.blocks.pop(pick)
        if sz > need:
            self.blocks.append((off + need, sz - need))
        return off

    def give(self, off, size):
        """Hand a range back and merge neighbours (blocks on either side of a zero page are never adjacent)."""
        merged = []
        for o, sz in sorted(self.blocks + [(off, size)]):
            if merged and merged[-1][0] + merged[-1][1] == o:
                merged[-1] = (merged[-1][0], merged[-1][1] + sz)
            else:
                merged.append((o, sz))
        self.blocks = merged


class Graph:
    def __init__(self, sd, B, H, W, stage_num=3, chl=256, kpt_paf=43, paf=14, keep_ref=False, precision="f16",
                 flip_pair=None, build=True, scaled_hms=False, all_heads=False, policy=None, keep_unit_out=False, keep_unit_in=False):
        """policy: the SchedulePolicy to build under (None: the environment's, read here) -- also what the emitters below consult when a
        harness calls them.
        build=False: an EMPTY schedule with all the book-keeping in place (single-op harnesses of tests / tools append to it with
        Graph.tensor / conv / conv_seg and then allocate() / emit()).
        flip_pair (43 ints: KEYPOINT.FLIP_ORDER + [15 + c for c in PAF.FLIP_CHANNEL]) switches the flip-TTA of
        test.py:55-70 on INSIDE the schedule: B input frames run as a 2B batch whose second half the stem reads mirrored,
        and the head sum merges the mirrored maps back (no flipped copy of the images, no separate merge pass); the
        depth heads, which the reference takes from the un-mirrored pass only, run on the first B frames.
        all_heads: every Upsample_unit of every stage also runs its three head chains (smap.py:221-229: res_conv1 -> res_conv2,
        res_d_conv1 -> res_d_conv2, res_rd_conv1 -> res_rd_conv2) -- the 62 convs the inference schedule leaves out -- and keeps the 36
        results as fp32 tensors at the unit's own resolution to the end of the schedule (Graph.head_tensors: what the validation loss
        reads).  The launches the inference outputs come from are the default schedule's, unchanged.
        keep_unit_out (with all_heads): the twelve `out` tensors of the units stay allocated to the end of the schedule as well
        (Graph.unit_out: what the head arms' fp32 forward and backward read, smap_amd/heads.py).  Nothing else changes: the same ops in
        the same order, the arena alone grows.
        keep_unit_in (with all_heads): the twelve INPUT tensors of the units (x4 .. x1 of every stage) stay allocated as well
        (Graph.unit_in: what the trunk's fp32 forward and backward read, smap_amd/trunk.py).  Again the arena alone grows."""
        assert precision in PRECISIONS, precision
        self.precision, self.x3 = precision, precision == "x3"
        self.policy = policy or SchedulePolicy.from_env()
        self.keep_ref = keep_ref
        self.flip_pair = list(flip_pair) if flip_pair is not None else None
        # scaled_hms: the head sum stores hms / 255 (key points) and / 127 (PAFs), i.e. the maps as test.py:111-112 hands them to the
        # association (smap_op.scale_hms) -- what the pipelines ask for; SMAP.forward keeps the raw maps of smap.py:417-419
        self.scaled_hms = bool(scaled_hms)
        self.all_heads = bool(all_heads)
        self.keep_unit_out = bool(keep_unit_out)
        if self.keep_unit_out and not self.all_heads:
            raise ValueError("keep_unit_out needs all_heads=True")
        self.unit_out = {}                    # keep_unit_out: (stage, unit) -> the unit's `out` Tensor
        self.keep_unit_in = bool(keep_unit_in)
        if self.keep_unit_in and not self.all_heads:
            raise ValueError("keep_unit_in needs all_heads=True")
        self.unit_in = {}                     # keep_unit_in: (stage, unit) -> the unit's input Tensor
        self.convs = []                       # state-dict prefix of every conv of the reference the schedule computes, in build order
        self.head_tensors = {}                # all_heads: (stage, unit) -> {"heatmap_2d" | "det_d" | "root_d": Tensor, or None = the output buffer's map}
        self.keep = []                        # tensors that stay allocated to the end of the schedule whoever reads them (allocate)
        self.frames = B                       # frames of the input / output
        if self.flip_pair is not None:
            assert len(self.flip_pair) == kpt_paf
            if sorted(self.flip_pair) != list(range(kpt_paf)):      # the head sum indexes LDS with these values
                raise ValueError("flip_pair must be a permutation of the %d output channels (cfg FLIP_ORDER / PAF.FLIP_CHANNEL)" % kpt_paf)
            B = 2 * B                         # frames of every activation tensor
        assert not build or (H % 32 == 0 and W % 32 == 0), "input must be a multiple of 32 (5 stride-2 levels)"
        self.sd, self.B, self.H, self.W = sd, B, H, W
        # 32-half K tiles of the packed weights are stored in PAIRS (128-byte rows [tile 2p | tile 2p+1]) for SMALL schedules (<= 2 frames of
        # 512x832 worth of pixels): every launch of those is latency-bound and lives on the L1 hit the second half of each fetched line
        # gives the next K tile (batch 1: 226 vs 195 frames/s); larger schedules are bandwidth-bound and prefer one contiguous block
        # per K tile (batch 8: 751 vs 738).  A per-launch rule (pairs for <= 512 workgroups) sits in between on both (226 / 745):
        # profiles/r3_ab_wpairs*.log.  SchedulePolicy.wpairs forces one layout for the whole schedule.
        self.w_pairs = int(self.small) if self.policy.wpairs is None else self.policy.wpairs
        # Forked streams for the independent head chains (smap_op.lane; BackboneEngine switches the plan's lanes on).  OFF by default: measured
        # at batch 1 (profiles/r5_v3_ab_b1.log) the forward is SLOWER with them, launched kernel by kernel (3.619 -> 3.706 ms) and replayed from
        # a graph (3.129 -> 3.436 ms): the head chains are 6 of 170 launches, and every fork / join costs an event round trip on the critical
        # path.  The mechanism stays tested: tests/test_backbone_gpu.py::test_lanes_fork_the_head_chains_and_change_nothing.
        self.lanes = int(self.policy.lanes)
        self.cur_lane = 0                                    # lane of the ops being appended (Graph.on_lane)
        self.ops, self.tensors = [], []
        self.scratch_tensors, self.kcount, self.kcount_tiles = [], None, 0      # split K: partial-tile scratch per op, one ticket region per schedule
        self.wchunks, self.woff = [], 0
        self.stage_num, self.chl, self.kpt_paf, self.paf = stage_num, chl, kpt_paf, paf
        self.flops = 0
        self.alg_bytes = 0                    # unfused per-launch traffic: input + output + weights + residual / skip adds / taps
        if build:
            self._build()

    # -- helpers
    def _fold(self, prefix):
        self.convs.append(prefix)
        return fold_conv_bn(self.sd, prefix)

    def tensor(self, name, H, W, C, esize=2):
        t = Tensor(name, self.B, H, W, C, esize, 2 if (self.x3 and esize == 2) else 1)
        self.tensors.append(t)
        return t

    def deep_pipeline_tile(self, tile, M, cout_pad, K):
        """Tile 2 (64x64, two LDS stages of 64-half K tiles, 64 KiB) -> tile 7 (the same tile with FOUR stages: three K tiles in flight,
        128 KiB) for launches of at most 256 workgroups.  Such a launch leaves every CU to one workgroup anyway, so the second
        workgroup's worth of LDS buys prefetch depth instead: the K loops of these launches are bound by the latency of the ONE tile a
        two-stage pipeline keeps in flight (~1 us per K tile at batch 1).  Measured at batch 1 per shape (profiles/r5_v9_*): -6 .. -21 %
        on launches of <= 256 workgroups, +31 .. +41 % on launches of 416 (one workgroup per CU instead of two).  SchedulePolicy.deep_tile."""
        if not self.x3 or tile != 2 or not self.policy.deep_tile:
            return tile
        bm, bn = TILES[2]
        wgs = -(-M // bm) * (cout_pad // bn) * self.split_k(2, M, cout_pad, K)
        return 7 if wgs <= 256 else 2

    def on_lane(self, lane):
        """Context manager: ops appended inside run on stream lane `lane` (0 when the schedule has no lanes)."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            prev, self.cur_lane = self.cur_lane, (lane if self.lanes else 0)
            n0 = len(self.ops)
            try:
                yield
            finally:
                for op in self.ops[n0:]:
                    op.lane = self.cur_lane
                self.cur_lane = prev
        return cm()

    def split_k(self, tile, M, cout_pad, K):
        """K parts per output tile for a conv.hip launch of this shape (include/smap_hip.h smap_op.ksplit), or 1.  Small schedules only
        (batch 1: configs[1]): a launch with fewer output tiles than half the CUs whose K loop is long enough to share out -- the 32x52
        and 16x26 levels run 26-104 workgroups of 16-72 K tiles each there.  SchedulePolicy.splitk: "0" switches it off, "<n>" forces n
        parts wherever the tile allows."""
        env = self.policy.splitk
        if env == "0" or not tile_has(tile, "splitk", self.x3):
            return 1
        bm, bn = TILES[tile]
        tiles = -(-M // bm) * (cout_pad // bn)
        n_k = K // tile_bk(tile, self.x3)
        if tiles >= 128 or n_k < 8:                      # the launch fills half the chip by itself, or has no K loop to share out
            return 1
        if env.startswith("t"):                          # "t384": aim at that many workgroups per launch, any K (A/B hook)
            s = min(8, int(env[1:]) // tiles, n_k // 4)
        elif env:                                        # "3": that many parts wherever a launch qualifies (tests)
            s = min(int(env), 16, n_k)
        else:
            # Measured at batch 1 (profiles/r5_v3_*): a part costs ~9 us (partial tile to memory and back, ticket, late epilogue), so
            # only long K loops gain: K = 4608 with 4 parts 57.6 -> 33.0 us, K = 2304 with 2 parts 30.2 -> 25.1, K = 2048 with 4
            # parts 27.9 -> 25.8; K = 1024 with 2 parts LOSES (17.0 -> 19.0), and aiming at 384 / 512 workgroups instead of 256 loses too
            if K < self.policy.splitk_mink:
                return 1
            s = min(4, 256 // tiles, n_k // 8)
        return s if s >= 2 else 1

    def _split_k_fields(self, name, tile, M, cout_pad, ks):
        """Scratch tensor + ticket slice of a split-K op -> (dict for Op.p, [scratch tensor])."""
        if ks <= 1:
            return {}, []
        bm, bn = TILES[tile]
        tiles = -(-M // bm) * (cout_pad // bn)
        part = Tensor(name + ".kpart", 1, 1, 1, tiles * ks * bm * bn, 4, 1)
        self.scratch_tensors.append(part)
        if self.kcount is None:
            self.kcount = Tensor("split_k.tickets", 1, 1, 1, 0, 4, 1)
        first_ticket = self.kcount_tiles
        self.kcount_tiles += tiles
        self.kcount.C = self.kcount_tiles
        return dict(ksplit=ks, kcount_first=first_ticket), [part]

    def _add_w(self, t):
        t = t.contiguous()
        raw = t.view(torch.uint8).reshape(-1) if t.dtype != torch.uint8 else t.reshape(-1)
        off = self.woff
        self.wchunks.append((off, raw))
        self.woff = _rup(off + raw.numel(), ALIGN)
        return off

    # -- what every conv emitter below shares
    @property
    def small(self):
        """A SMALL schedule: at most 2 frames of 512x832 worth of pixels (batch 1).  Its launches are latency-bound: split K, the deep-pipeline
        64 x 64 tile and paired weight tiles instead of the two-input launches and the widest whole-block tiles."""
        return self.B * self.H * self.W <= 2 * 512 * 832

    @property
    def one_window(self):
        """Does the reusing arena fit ONE 4 GiB window?  Both inputs of a two-input launch are addressed from one base (allocate)."""
        return self.B * self.H * self.W <= 20 * 512 * 832

    def _weights(self, name, rows, cout_pad=None):
        """[cout][K] folded rows -> (wk [planes][cout_pad][K] fp16 with zero rows behind cout, acc_scale).  Split precision: hi | lo of
        rows * 2^s and 2^-s (split_f16: ONE scale per call, and its assertion that they are finite); fp16: the cast and 1.0, weights beyond
        fp16's range are an error of op `name`."""
        cout, K = rows.shape
        wk = torch.zeros((2 if self.x3 else 1, cout_pad or cout, K), dtype=torch.float16)
        acc_scale = 1.0
        if self.x3:
            wk[0, :cout], wk[1, :cout], acc_scale = split_f16(rows)
        else:
            wk[0, :cout] = rows.to(torch.float16)
            self._check_fp16(name, wk, rows)
        return wk, acc_scale

    def _check_fp16(self, name, wk, *folded):
        if not torch.isfinite(wk).all():
            raise ValueError(f"{name}: folded weights exceed the fp16 range (max |w| = {max(float(w.abs().max()) for w in folded):.3g})")

    def _bias(self, b, cout_pad=None):
        bk = torch.zeros((cout_pad or b.numel(),), dtype=torch.float32)
        bk[:b.numel()] = b.to(torch.float32)
        return bk

    def _ref(self, **folded):
        """w_ref / b_ref of an op's p (sub-)dict: the folded f64 parameters under keep_ref (oracle/graph_interp.py, tests), else None."""
        return {k + "_ref": v if self.keep_ref else None for k, v in folded.items()}

    def _forced_or_first(self, forced, cands, cap):
        """Tile of a two-input launch: the one an A/B hook of the policy names, else the first candidate with an instance of `cap` in this precision."""
        return forced if forced is not None else next(t for t in cands if tile_has(t, cap, self.x3))

    def _pick(self, keys, legal, M, cout, K, *, key16, deep_pad, remap, remap16, x3_tile_fits=lambda t: True, tile=None):
        """Tile id of a conv.hip-style launch of M x cout x K.  Split precision: the first legal(t) among SchedulePolicy.x3_tile (where
        x3_tile_fits), the measured table's entries under `keys` (most specific first) and the block-count rule.  fp16: the table's entry
        under key16 -- the table is keyed by shape only, so the block-count heuristic stands in for an entry that is not legal(t).  Then
        `remap` (fp16: before the legality check, and only with remap16) and the deep-pipeline rule for the 64 x 64 tile, whose N extent is
        deep_pad.  tile: the caller names it -- it must be legal, the deep-pipeline rule still applies."""
        pol = self.policy
        if tile is not None:
            assert legal(tile), tile
        elif self.x3:
            cands = pick_tile_x3(M, cout, keys, pol)
            if pol.x3_tile is not None and x3_tile_fits(pol.x3_tile):
                cands = [pol.x3_tile] + cands
            tile = next(t for t in cands if legal(t))
            tile = remap.get(tile, tile)
        else:
            tile = pick_tile(M, cout, key16, pol)
            if remap16:
                tile = remap.get(tile, tile)
            if not legal(tile):
                tile = pick_tile_heuristic(M, cout)
        return self.deep_pipeline_tile(tile, M, deep_pad, K)

    def _conv_op(self, out, x, wk, bias, *, flops, alg_bytes, kinds, Cin, Cout, cout_pad, tile, acc_scale, ref, relu=1, ksize=1, stride=1,
                 in_c_off=0, out_fp32=0, frames=None, w_pairs=None, split_k=None, sub=None, **tensors):
        """Append ONE conv launch writing `out` from `x`: the accounting, the p keys every launch has (a 1x1 stride-1 ReLU conv on all frames
        unless said) and the main weights / bias in the weight section.  split_k = (M, K): the launch may split its K loop.  sub(): the emitter's
        own sub-dicts -- called AFTER the main weights are placed, the weight section is laid out in call order.  tensors: further Op fields."""
        self.flops += flops
        self.alg_bytes += alg_bytes
        skf, scratch = {}, []
        if split_k:
            M, K = split_k
            skf, scratch = self._split_k_fields(out.name, tile, M, cout_pad, self.split_k(tile, M, cout_pad, K))
        p = dict(flops=flops, alg_bytes=alg_bytes, kinds=kinds, **skf,
                 Cin=Cin, in_c_off=in_c_off, Cout=Cout, ksize=ksize, stride=stride, pad=ksize // 2, relu=int(relu),
                 cout_pad=cout_pad, tile=tile, out_fp32=int(out_fp32), w_off=self._add_w(wk), bias_off=self._add_w(bias),
                 acc_scale=acc_scale, frames=self.B if frames is None else frames, w_pairs=self.w_pairs if w_pairs is None else w_pairs)
        p.update(sub() if sub else {}, **ref)
        self.ops.append(Op(OP_CONV, out=out, inp=x, scratch=scratch, p=p, **tensors))
        return out

    def conv(self, name, prefixes, x, ksize=1, stride=1, relu=True, res=None, add1=None, add2=None,
             in_c_off=0, cin=None, out_fp32=False, up=None, frames=None):
        """One conv launch; `prefixes` (list) are concatenated along Cout (shared input).  frames: run on the first
        `frames` frames of the batch only (flip-TTA: heads whose mirrored half nobody reads)."""
        ws, bs = zip(*[self._fold(p) for p in prefixes])
        w, b = torch.cat(ws, 0), torch.cat(bs, 0)
        cout, cin_w = w.shape[0], w.shape[1]
        cin = cin or x.C
        assert cin_w == cin and w.shape[2] == ksize, (name, w.shape, cin, ksize)
        pad = ksize // 2
        Ho = (x.H + 2 * pad - ksize) // stride + 1
        Wo = (x.W + 2 * pad - ksize) // stride + 1
        nfr = self.B if frames is None else frames
        M, K = nfr * Ho * Wo, ksize * ksize * cin
        key = f"{nfr},{x.H},{x.W},{cin},{cout},{ksize},{stride}"
        plain3 = ksize == 3 and stride == 1 and res is None and add1 is None and add2 is None and up is None
        legal = lambda t: tile_legal(t, cout=cout, plain3=plain3, up=up is not None, out_fp32=out_fp32,
                                     adds=add1 is not None or add2 is not None, x3=self.x3)
        # ops with the fused bilinear add have their own table entries (the tap loads of the epilogue favour wider tiles)
        tile = self._pick([key + ",up", key] if up is not None else [key], legal, M, cout, K, key16=key, deep_pad=_rup(cout, 64),
                          remap=dict(self.policy.tile_remap), remap16=True, x3_tile_fits=lambda t: cout > 32 and not (cout <= 64 and TILES[t][1] > 64))
        if self.policy.halo3 and plain3 and cout > 32:      # (a halo tile is never the 64 x 64 one: the deep-pipeline rule above has nothing to say)
            tw, hbn = self.policy.halo3
            hbn = hbn or min(TILES[tile][1], 128 if cout > 64 else 64)
            tile = {(16, 64): 30, (16, 128): 31, (32, 64): 32, (32, 128): 33}[(tw, max(hbn, 64))] + (4 if self.policy.halo3_deep else 0)
        cout_pad = _rup(cout, TILES[tile][1])
        wk, acc_scale = self._weights(name, w.permute(0, 2, 3, 1).reshape(cout, K), cout_pad)
        wk = pack_conv_weights(wk, tile, self.x3, ksize, cin, pairs=self.w_pairs)   # one contiguous block per staged weight tile (pair)
        out = self.tensor(name, Ho, Wo, _rup(cout, 8), 4 if out_fp32 else 2)
        by = (nfr * x.H * x.W * cin * 2 * x.planes + nfr * Ho * Wo * out.C * out.esize * out.planes
              + wk.numel() * 2 + sum(t.nbytes * nfr // self.B for t in (res, add1, add2, up) if t is not None))
        return self._conv_op(out, x, wk, self._bias(b, cout_pad), flops=2 * M * cout * K, alg_bytes=by, kinds="1x1" if ksize == 1 else "3x3",
                             Cin=cin, Cout=cout, cout_pad=cout_pad, tile=tile, acc_scale=acc_scale, ref=self._ref(w=w, b=b), relu=relu,
                             ksize=ksize, stride=stride, in_c_off=in_c_off, out_fp32=out_fp32, frames=nfr, split_k=(M, K),
                             res=res, add1=add1, add2=add2, aux=[up] if up is not None else [])

    def conv_relusum(self, name, pre1, x, pre2, x2, tile=None):
        """relu(conv1(x)) + relu(conv2(x2)) as ONE launch and ONE tensor (include/smap_hip.h smap_op.in2_mode = 1): the two inter-stage skips of an
        Upsample_unit, skip1 on the unit's input and skip2 on its output (smap.py:218-241), which the next stage only ever ADDS to its feature map
        (smap.py:142-153).  One write and one read of an in_planes-wide tensor less per level; each conv keeps its own power-of-two scale."""
        (w1, b1), (w2, b2) = self._fold(pre1), self._fold(pre2)
        cout, c1, c2 = w1.shape[0], w1.shape[1], w2.shape[1]
        assert w2.shape[0] == cout and w1.shape[2] == 1 == w2.shape[2] and c1 == x.C and c2 == x2.C and cout % 8 == 0 and (x.H, x.W) == (x2.H, x2.W)
        M, K = self.B * x.H * x.W, c1 + c2
        if tile is None:
            key = f"{self.B},{x.H},{x.W},{c1}+{c2}relusum,{cout},1,1"
            # measured in situ (profiles/r6_v14_ab_two_input_tiles.log): the 128 x 256 tile (both inputs' rows staged once per launch instead of once
            # per 128-channel N tile) 860-864 frames/s against 847 with the 128 x 128 tiles; the K-concatenated launches (conv_cat) do not care
            tile = self._forced_or_first(self.policy.relusum_tile, (pick_tile_x3(M, cout, key, self.policy) if self.x3 else []) + [54, 53, 50, 51], "relusum")
        assert tile_has(tile, "relusum", self.x3), tile
        cout_pad = _rup(cout, TILES[tile][1])
        wk1, sc1 = self._weights(name, w1.reshape(cout, c1), cout_pad)
        wk2, sc2 = self._weights(name, w2.reshape(cout, c2), cout_pad)
        wk = pack_conv_weights(torch.cat([wk1, wk2], 2), tile, self.x3, 1, K, pairs=self.w_pairs)
        out = self.tensor(name, x.H, x.W, cout)
        return self._conv_op(out, x, wk, self._bias(b1, cout_pad), flops=2 * M * cout * K, alg_bytes=x.nbytes + x2.nbytes + out.nbytes + wk.numel() * 2,
                             kinds="1x1", Cin=c1, Cout=cout, cout_pad=cout_pad, tile=tile, acc_scale=sc1, ref=self._ref(w=w1, b=b1), relu=0, aux2=x2,
                             sub=lambda: dict(cat=dict(cin=c2, stride=1, relusum=True, acc_scale=sc2, bias_off=self._add_w(self._bias(b2, cout_pad)),
                                                       **self._ref(w=w2, b=b2))))

    def conv_tapdot(self, name, pre1, pre3, x, frames=None):
        """A 1x1 conv + ReLU (prefix pre1, 256 -> 256) whose ONLY consumer is a 3x3 conv with one output channel (prefix pre3) -- smap.py:227-229,
        res_rd_conv1 -> res_rd_conv2 -- with the per-pixel half of that 3x3 inside its epilogue (include/smap_hip.h smap_op.tap_n): the launch
        stores t[m][k] = <w3[k], y[m]>, nine fp32 numbers per pixel, instead of the 256-channel activation; Graph.tapsum finishes the conv.
        Returns (t tensor, bias of the 3x3)."""
        w1, b1 = self._fold(pre1)
        w3, b3 = self._fold(pre3)
        cout, cin = w1.shape[0], w1.shape[1]
        assert cout == 256 == w3.shape[1] and w3.shape[0] == 1 and w3.shape[2] == 3 and cin == x.C and w1.shape[2] == 1
        tile = tile_ids(cap="tapdot", x3=self.x3)[0]
        nfr = self.B if frames is None else frames
        M = nfr * x.H * x.W
        wk, acc_scale = self._weights(name, w1.reshape(cout, cin))
        wk = pack_conv_weights(wk, tile, self.x3, 1, cin, pairs=self.w_pairs)
        # the 3x3's weights as B fragments of v_mfma_f32_16x16x32_f16 (include/smap_hip.h smap_op.tap_n): [K step][hi, lo][lane][8 halves],
        # lane l = tap l % 16 (9..15: zeros), channels 32 step + 8 (l / 16) .. +7; pre-scaled by a power of two like every split weight matrix
        tw = torch.zeros((16, cout), dtype=torch.float64)
        tw[:9] = w3[0].permute(1, 2, 0).reshape(9, cout)                                   # [kh*3+kw][channel]
        thi, tlo, tap_scale = split_f16(tw)
        lane = torch.arange(64)
        kidx = (torch.arange(cout // 32)[:, None, None] * 32 + (lane // 16)[None, :, None] * 8 + torch.arange(8)[None, None, :])     # [step][lane][8]
        tapw = torch.stack([thi[(lane % 16)[None, :, None], kidx], tlo[(lane % 16)[None, :, None], kidx]], 1).contiguous()              # [step][2][64][8]
        t = Tensor(name, self.B, x.H, x.W, 16, 4, 1)
        self.tensors.append(t)
        by = nfr * x.H * x.W * cin * 2 * x.planes + nfr * x.H * x.W * 16 * 4 + wk.numel() * 2
        self._conv_op(t, x, wk, self._bias(b1), flops=2 * M * cout * cin + 2 * M * 9 * cout, alg_bytes=by, kinds="1x1", Cin=cin, Cout=cout,
                      cout_pad=cout, tile=tile, acc_scale=acc_scale, ref=self._ref(w=w1, b=b1), out_fp32=1, frames=nfr,
                      sub=lambda: dict(tap=dict(w_off=self._add_w(tapw), scale=tap_scale, **self._ref(w=w3))))
        return t, b3

    def tapsum(self, t, b3, ext_off):
        """The stencil half of conv_tapdot's 3x3: out[b,0,y,x] = b3 + sum over taps of t[b, y+kh-1, x+kw-1][3 kh + kw] -> the fp32 NCHW map at
        ext_off of the output buffer (SMAP_OP_TAPSUM; stands where the head sum of that map stood)."""
        self.ops.append(Op(OP_TAPSUM, aux=[t], p=dict(Cout=1, ext_off=ext_off, bias_off=self._add_w(b3.to(torch.float32).reshape(1)),
                                                       **self._ref(b=b3))))

    def conv_cat(self, name, pre1, x, pre2, x2, stride2, relu=True, tile=None):
        """The last 1x1 of a Bottleneck (prefix pre1, on x) TOGETHER with the block's 1x1 shortcut conv (prefix pre2, on x2 sampled with spatial
        stride `stride2`) as ONE launch: out = act(W1 x + W2 x2 + b1 + b2) -- smap.py:60-77 adds the shortcut's output before the ReLU, no
        activation in between, so the two GEMMs share their accumulators when K is the concatenation of both inputs' channels
        (include/smap_hip.h smap_op.in2_*).  The shortcut tensor is never written or read back and its launch disappears."""
        (w1, b1), (w2, b2) = self._fold(pre1), self._fold(pre2)
        cout, c1, c2 = w1.shape[0], w1.shape[1], w2.shape[1]
        assert w2.shape[0] == cout and w1.shape[2] == 1 == w2.shape[2] and c1 == x.C and c2 == x2.C and cout % 8 == 0
        Ho, Wo = x.H, x.W
        assert (x2.H - 1) // stride2 + 1 == Ho and (x2.W - 1) // stride2 + 1 == Wo
        M, K = self.B * Ho * Wo, c1 + c2
        if tile is None:
            key = f"{self.B},{Ho},{Wo},{c1}+{c2}cat,{cout},1,1"
            tile = self._forced_or_first(self.policy.cat_tile, (pick_tile_x3(M, cout, key, self.policy) if self.x3 else []) + [50, 51, 20], "dual")
        assert tile_has(tile, "dual", self.x3), tile
        cout_pad = _rup(cout, TILES[tile][1])
        # [cout][K = (x channels | x2 channels)] with ONE power-of-two scale: the two matrices share the accumulators
        wk, acc_scale = self._weights(name, torch.cat([w1.reshape(cout, c1), w2.reshape(cout, c2)], 1), cout_pad)
        wk = pack_conv_weights(wk, tile, self.x3, 1, K, pairs=self.w_pairs)
        out = self.tensor(name, Ho, Wo, cout)
        by = x.nbytes + self.B * Ho * Wo * c2 * 2 * x2.planes + out.nbytes + wk.numel() * 2      # (the strided shortcut touches the sampled pixels only)
        return self._conv_op(out, x, wk, self._bias(b1 + b2, cout_pad), flops=2 * M * cout * K, alg_bytes=by, kinds="1x1", Cin=c1, Cout=cout,
                             cout_pad=cout_pad, tile=tile, acc_scale=acc_scale, ref=self._ref(w=w1, b=b1), relu=relu, aux2=x2,
                             sub=lambda: dict(cat=dict(cin=c2, stride=stride2, **self._ref(w=w2, b=b2))))

    def conv_seg(self, segs, x, up=None, tile=None):
        """Several 1x1 stride-1 convs that read the SAME input as ONE launch with one output tensor per conv (include/smap_hip.h
        smap_op.seg_*; Upsample_unit, smap.py:210-241: u_skip | skip1 on x; skip2 | cross_conv | the next unit's up_conv on
        `out`).  segs: [(tensor name, prefix, relu)], up to three; `up` (the fused bilinear add) belongs to the first.  The weight
        matrix is the concatenation of the convs' rows, each segment starting on a multiple of the tile's N extent and carrying
        its own power-of-two scale in split precision, so every conv computes exactly what its own launch would.  Returns the
        output tensors in order."""
        assert 2 <= len(segs) <= 3
        folded = [self._fold(pre) for _, pre, _ in segs]
        cin = x.C
        couts = [w.shape[0] for w, _ in folded]
        assert all(w.shape[1] == cin and w.shape[2] == 1 for w, _ in folded) and all(c % 8 == 0 for c in couts)
        M = self.B * x.H * x.W
        # table keys: the merged shape "B,H,W,Cin,c0+c1[+c2],1,1" (tools/autotune_seg.py), then -- a launch nobody tuned -- the entry of its
        # widest conv alone (same input, same K: the nearest measured relative)
        key = f"{self.B},{x.H},{x.W},{cin},{'+'.join(map(str, couts))},1,1"
        wide = f"{self.B},{x.H},{x.W},{cin},{max(couts)},1,1"
        legal = lambda t: (tile_family(t) == "igemm" and tile_has(t, None, self.x3) and TILES[t][1] >= 64       # (not the Cout <= 32 tiles)
                           and (not tile_has(t, "regepi", True) or (self.x3 and up is None)))
        keys = ([key + ",up"] if up is not None else []) + [key] + ([wide + ",up"] if up is not None else []) + [wide]
        # (this emitter's own: every segment counts padded to 64 in the deep-pipeline rule; the remap does not apply in fp16, and never TO tile 0)
        tile = self._pick(keys, legal, M, sum(couts), cin, key16=key, deep_pad=sum(_rup(c, 64) for c in couts),
                          remap={a: b for a, b in self.policy.tile_remap if b}, remap16=False, tile=tile)
        bn = TILES[tile][1]
        starts, n = [], 0
        for c in couts:
            starts.append(n)
            n = _rup(n + c, bn)
        cout_pad = n
        wk = torch.zeros((2 if self.x3 else 1, cout_pad, cin), dtype=torch.float16)
        bk = torch.zeros((cout_pad,), dtype=torch.float32)
        scales = []
        for (w, b), st, c in zip(folded, starts, couts):
            wk[:, st:st + c], sc = self._weights(segs[0][0], w.reshape(c, cin))
            bk[st:st + c] = b.to(torch.float32)
            scales.append(sc)
        self._check_fp16(segs[0][0], wk, *[w for w, _ in folded])       # (in both precisions, as this emitter always did)
        wk = pack_conv_weights(wk, tile, self.x3, 1, cin, pairs=self.w_pairs)
        outs = [self.tensor(nm, x.H, x.W, c) for (nm, _, _), c in zip(segs, couts)]
        by = x.nbytes + sum(t.nbytes for t in outs) + wk.numel() * 2 + (up.nbytes if up is not None else 0)
        self._conv_op(outs[0], x, wk, bk, flops=2 * M * sum(couts) * cin, alg_bytes=by, kinds="1x1", Cin=cin, Cout=couts[0], cout_pad=cout_pad,
                      tile=tile, acc_scale=scales[0], ref=self._ref(w=folded[0][0], b=folded[0][1]), relu=segs[0][2], split_k=(M, cin),
                      aux=[up] if up is not None else [], outs=outs[1:],
                      sub=lambda: dict(segs=[dict(n0=st, cout=c, relu=int(r), acc_scale=sc, **self._ref(w=w, b=b))
                                             for st, c, (_, _, r), sc, (w, b) in list(zip(starts, couts, segs, scales, folded))[1:]]))
        return outs

    def conv_tail(self, name, pre3, pre1, x, tile, res=None, add1=None, add2=None):
        """A Bottleneck's 3x3 stride-1 conv (prefix pre3, bias + ReLU) and the 1x1 behind it (prefix pre1, + res, ReLU, + add1,
        + add2) as ONE launch (csrc/convf.hip, the "tail" tile ids): the 3x3's output never leaves the CU."""
        w3, b3 = self._fold(pre3)
        w1, b1 = self._fold(pre1)
        P, cin = w3.shape[0], w3.shape[1]
        cout = w1.shape[0]
        bn2 = TAIL_BN[tile]
        assert TILES[tile][1] == P == w1.shape[1] and cin == x.C and w3.shape[2] == 3 and w1.shape[2] == 1 and cout % 8 == 0
        cout_pad = _rup(cout, bn2)
        M = self.B * x.H * x.W
        K3 = 9 * cin
        wk3, sc3 = self._weights(name, w3.permute(0, 2, 3, 1).reshape(P, K3))
        wk1, sc1 = self._weights(name, w1.reshape(cout, P), cout_pad)
        wk3 = pack_halo_rows(wk3, P, 9, cin, self.x3)
        wk1 = pack_halo_rows(wk1, bn2, 1, P, self.x3)
        out = self.tensor(name, x.H, x.W, cout)
        by = (x.nbytes + out.nbytes + (wk3.numel() + wk1.numel()) * 2
              + sum(t.nbytes for t in (res, add1, add2) if t is not None))
        return self._conv_op(out, x, wk3, self._bias(b3), flops=2 * M * (P * K3 + cout * P), alg_bytes=by, kinds="3x3+1x1", Cin=cin, Cout=P, cout_pad=P,
                             tile=tile, acc_scale=sc3, ref=self._ref(w=w3, b=b3), ksize=3, w_pairs=0, res=res, add1=add1, add2=add2,
                             sub=lambda: dict(tail=dict(cout=cout, cout_pad=cout_pad, w_off=self._add_w(wk1), bias_off=self._add_w(self._bias(b1, cout_pad)),
                                                        acc_scale=sc1, **self._ref(w=w1, b=b1))))

    def conv_block_first(self, name, pre, x, tile):
        """The FIRST Bottleneck of layer1 (smap.py:48-77 with the 1x1 shortcut conv of :124-129; 64 input channels, stride 1) as ONE
        launch (csrc/convb.hip, the "block" tile ids with first = True): relu(c3(c2(c1(x))) + downsample(x)); x is read once."""
        assert self.x3
        w1, b1 = self._fold(pre + ".conv_bn_relu1")
        w3, b3 = self._fold(pre + ".conv_bn_relu2")
        wt, bt = self._fold(pre + ".conv_bn_relu3")
        wd, bd = self._fold(pre + ".downsample")
        P, Cin = w1.shape[0], w1.shape[1]
        C = wt.shape[0]
        assert P == 64 == Cin == x.C and C == 256 and tuple(wd.shape[:2]) == (C, Cin) and wd.shape[2] == 1 and w3.shape[2] == 3
        M = self.B * x.H * x.W
        wk1, sc1 = self._weights(name, w1.reshape(P, Cin))
        wk1 = pack_halo_rows(wk1, P, 1, Cin, True)                                    # [1][2 chunks][1][64 rows][128 B]
        wk3, sc3 = self._weights(name, w3.permute(0, 2, 3, 1).reshape(P, 9 * P))
        wk3 = pack_halo_rows(wk3, P, 9, P, True)
        wkt, sct = self._weights(name, wt.reshape(C, P))
        wkt = pack_halo_rows(wkt, 64, 1, P, True)
        wkd, scd = self._weights(name, wd.reshape(C, Cin))
        wkd = pack_halo_rows(wkd, 64, 1, Cin, True)                                   # [4 n chunks][2 k chunks][1][64 rows][128 B]
        out = self.tensor(name, x.H, x.W, C)
        by = x.nbytes + out.nbytes + (wk1.numel() + wk3.numel() + wkt.numel() + wkd.numel()) * 2
        return self._conv_op(out, x, wk3, self._bias(b3), flops=2 * M * (P * Cin + P * 9 * P + C * P + C * Cin), alg_bytes=by, kinds="block", Cin=P,
                             Cout=P, cout_pad=P, tile=tile, acc_scale=sc3, ref=self._ref(w=w3, b=b3), ksize=3, w_pairs=0,
                             sub=lambda: dict(
                                 head=dict(cin=Cin, w_off=self._add_w(wk1), bias_off=self._add_w(self._bias(b1)), acc_scale=sc1, **self._ref(w=w1, b=b1)),
                                 tail=dict(cout=C, cout_pad=C, w_off=self._add_w(wkt), bias_off=self._add_w(self._bias(bt + bd)), acc_scale=sct,
                                           **self._ref(w=wt, b=bt)),
                                 short=dict(w_off=self._add_w(wkd), acc_scale=scd, **self._ref(w=wd, b=bd))))

    def conv_block(self, name, pre, x, tile, add1=None, add2=None):
        """A whole stride-1 identity Bottleneck (smap.py:48-77: conv_bn_relu1 1x1 -> conv_bn_relu2 3x3 -> conv_bn_relu3 1x1, + x,
        ReLU, + add1, + add2) as ONE launch (csrc/convb.hip / convc.hip, the "block" tile ids, split precision): x is read once, the two
        intermediates and the residual never leave the CU."""
        assert self.x3, "the whole-block kernel has a split-precision instance only"
        w1, b1 = self._fold(pre + ".conv_bn_relu1")
        w3, b3 = self._fold(pre + ".conv_bn_relu2")
        wt, bt = self._fold(pre + ".conv_bn_relu3")
        P, C = w1.shape[0], w1.shape[1]
        bn2 = TAIL_BN[tile]
        assert P == TILES[tile][1] and C == 4 * P == x.C == wt.shape[0] and w3.shape[:2] == (P, P) and w3.shape[2] == 3 and wt.shape[1] == P
        assert tile_family(tile) == "block" and not TILE_TABLE[tile].first and P == TILE_TABLE[tile].planes
        M = self.B * x.H * x.W
        wk1, sc1 = self._weights(name, w1.reshape(P, C))
        if P == 64:
            wk1 = pack_rows16(wk1)                                                    # [C/16 stages][P rows][64 B]
        else:
            wk1 = pack_halo_rows(wk1, P, 1, C, True)                                  # csrc/convc.hip: [1][C/32 chunks][1][P rows][128 B]
        wk3, sc3 = self._weights(name, w3.permute(0, 2, 3, 1).reshape(P, 9 * P))
        wk3 = pack_halo_rows(wk3, P, 9, P, True)                                      # [1][P/32][9 taps][P rows][128 B]
        wkt, sct = self._weights(name, wt.reshape(C, P))
        wkt = pack_halo_rows(wkt, bn2, 1, P, True)                                    # [C/64][P/32][1][64 rows][128 B]
        out = self.tensor(name, x.H, x.W, C)
        by = (x.nbytes + out.nbytes + (wk1.numel() + wk3.numel() + wkt.numel()) * 2
              + sum(t.nbytes for t in (add1, add2) if t is not None))
        return self._conv_op(out, x, wk3, self._bias(b3), flops=2 * M * (P * C + P * 9 * P + C * P), alg_bytes=by, kinds="block", Cin=P, Cout=P,
                             cout_pad=P, tile=tile, acc_scale=sc3, ref=self._ref(w=w3, b=b3), ksize=3, w_pairs=0, res=x, add1=add1, add2=add2,
                             sub=lambda: dict(
                                 head=dict(cin=C, w_off=self._add_w(wk1), bias_off=self._add_w(self._bias(b1)), acc_scale=sc1, **self._ref(w=w1, b=b1)),
                                 tail=dict(cout=C, cout_pad=C, w_off=self._add_w(wkt), bias_off=self._add_w(self._bias(bt)), acc_scale=sct,
                                           **self._ref(w=wt, b=bt))))

    def block_tile(self, planes, stride, has_ds):
        """Tile id of the whole-block launch for this Bottleneck, or None.  Identity blocks (no shortcut conv) of stride 1 in
        split precision only; SchedulePolicy.block chooses per width, default BLOCK_DEFAULT -- in small schedules (<= 2 frames of
        512x832) without layer2's entry (at batch 1 the 64x104 level has 52 tiles of the eight-wave kernel for 256 CUs, 55-57 us per block
        where the three launches take ~42: profiles/r5_v2_x3_layers_batch1.txt) and with layer1's on 4 x 16 pixel tiles (twice the
        workgroups: profiles/r5_v11_ab_b1_whole_block_tiles.log)."""
        if stride != 1 or has_ds or not self.x3:
            return None
        if self.policy.block is None and self.small:
            return {64: 90}.get(planes)  # 4 x 16 pixel tiles: 416 workgroups of half the work at batch 1 (2.91 -> 2.84 ms per frame)
        return dict(BLOCK_DEFAULT if self.policy.block is None else self.policy.block).get(planes)

    # -- the network (smap.py:313-353 structure, :403-419 data flow)
    def _build(self):
        B, H, W, sd = self.B, self.H, self.W, self.sd
        # ResNet_top (smap.py:80-92)
        w, b = self._fold("top.conv")
        wk, stem_scale = pack_stem_weights(w, self.x3)
        H2, W2 = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
        H4, W4 = (H2 + 2 - 3) // 2 + 1, (W2 + 2 - 3) // 2 + 1
        self.flops += 2 * B * H2 * W2 * 64 * 147
        stem_p = dict(w_off=self._add_w(wk), bias_off=self._add_w(b.to(torch.float32)), w_ref=w, b_ref=b, acc_scale=stem_scale)
        if not self.policy.stempool:                    # default: conv and max-pool as two kernels (the fused kernel below is
            t = self.tensor("top.conv", H2, W2, 64)     # bit-identical but no faster inside the two-batch pipeline)
            self.ops.append(Op(OP_STEM, out=t, p=stem_p))
            x = self.tensor("top.pool", H4, W4, 64)
            self.ops.append(Op(OP_MAXPOOL, out=x, inp=t))
        else:                                           # ResNet_top in one kernel, only the pooled tensor is written
            x = self.tensor("top.pool", H4, W4, 64)
            self.ops.append(Op(OP_STEMPOOL, out=x, p=stem_p))
        self.out_h, self.out_w = H4, W4
        skip1 = skip2 = None
        for s in range(self.stage_num):
            last = s == self.stage_num - 1
            x, skip1, skip2 = self._stage(s, x, skip1, skip2, gen_skip=not last, heads=last)

    def _bottleneck(self, pre, x, planes, stride, has_ds, add1=None, add2=None):
        # Bottleneck (smap.py:48-77): stride on the 3x3, shortcut 1x1 stride-s when shape changes
        blk = self.block_tile(planes, stride, has_ds)
        if blk is not None:         # c1 + c2 + c3 + residual in one launch (csrc/convb.hip)
            return self.conv_block(pre + ".c3", pre, x, blk, add1=add1, add2=add2)
        first = dict(BLOCK_FIRST_DEFAULT if self.policy.block_first is None else self.policy.block_first).get(planes)
        if self.policy.block_first is None and first == 93 and self.small:
            first = 92                   # small schedules: the 4 x 16 tiles here too
        if first is not None and self.x3 and has_ds and stride == 1 and x.C == 64 and planes == 64 and add1 is None and add2 is None:
            return self.conv_block_first(pre + ".c3", pre, x, first)
        # A block with a shortcut conv (the first of layer2 / 3 / 4; layer1's runs as a whole-block launch above): its last 1x1 and the shortcut
        # as ONE GEMM over K = (planes | in_planes) -- the shortcut tensor is never stored (conv_cat).  SchedulePolicy.cat = False: two launches, as round 5 ran.
        # (Not for arenas beyond one 4 GiB window: both inputs are addressed from one base.)
        # (Not in small schedules -- <= 2 frames of 512x832 --: their launches live on split K and the deep-pipeline 64 x 64 tile, which the
        #  two-input instances do not have: batch 1 measured 3.4 ms per frame with them against 2.9 without, profiles/r6_final_*.)
        cat = (has_ds and add1 is None and add2 is None and self.policy.cat is not False and self.tail_tile(planes, stride) is None
               and self.one_window and (self.policy.cat or not self.small))
        idn = x if (not has_ds or cat) else self.conv(pre + ".downsample", [pre + ".downsample"], x, 1, stride, relu=False)
        y = self.conv(pre + ".c1", [pre + ".conv_bn_relu1"], x, 1, 1, relu=True)
        if cat:
            y = self.conv(pre + ".c2", [pre + ".conv_bn_relu2"], y, 3, stride, relu=True)
            return self.conv_cat(pre + ".c3", pre + ".conv_bn_relu3", y, pre + ".downsample", x, stride, relu=True)
        tail = self.tail_tile(planes, stride)
        if tail is not None:        # c2 + c3 in one launch (csrc/convf.hip)
            return self.conv_tail(pre + ".c3", pre + ".conv_bn_relu2", pre + ".conv_bn_relu3", y, tail, res=idn, add1=add1, add2=add2)
        y = self.conv(pre + ".c2", [pre + ".conv_bn_relu2"], y, 3, stride, relu=True)
        return self.conv(pre + ".c3", [pre + ".conv_bn_relu3"], y, 1, 1, relu=True, res=idn, add1=add1, add2=add2)

    def tail_tile(self, planes, stride):
        """Tile id of the fused 3x3 + 1x1 launch for a Bottleneck of this width, or None = two launches.
        SchedulePolicy.tail chooses per width; default: see TAIL_DEFAULT."""
        if stride != 1:
            return None
        return dict(TAIL_DEFAULT if self.policy.tail is None else self.policy.tail).get(planes)

    def _stage(self, s, x, skip1, skip2, gen_skip, heads):
        """Stage s on x: the ResNet layers (+ the previous stage's skips), Upsample_module (smap.py:244-286: up1 on x4 ... up4 on x1) and, behind
        the last stage (heads), the output buffer.  Returns (cross_conv, skip1 list, skip2 list) for the next stage; the lists are fine -> coarse
        (smap.py:283-284)."""
        x1, x2, x3, x4 = self._layers(s, x, skip1, skip2)
        out, tl, s1, s2, cross, head_t = None, None, [None] * 4, [None] * 4, None, {}
        for ind, xin in enumerate((x4, x3, x2, x1)):
            out, tl, s1[3 - ind], s2[3 - ind], cross = self._unit(s, ind, xin, out, tl, gen_skip, heads, head_t)
        if heads:
            self._outputs(head_t)
        return cross, (s1 if gen_skip else None), (s2 if gen_skip else None)

    def _layers(self, s, x, skip1, skip2):
        """layer1..4 of stage s -> [x1, x2, x3, x4]; the last block of layer li adds skip1[li] + skip2[li] of the previous stage (smap.py:142-153)."""
        feats = []
        inpl = 64
        for li, (planes, nblk) in enumerate(zip(PLANES, LAYERS)):
            stride = 1 if li == 0 else 2
            for j in range(nblk):
                lastb = j == nblk - 1
                a1 = skip1[li] if (skip1 is not None and lastb) else None
                a2 = skip2[li] if (skip2 is not None and lastb) else None
                has_ds = j == 0 and (stride != 1 or inpl != planes * 4)
                x = self._bottleneck(f"stage{s}.downsample.layer{li + 1}.{j}", x, planes, stride if j == 0 else 1, has_ds, a1, a2)
                inpl = planes * 4
            feats.append(x)
        return feats

    def _shared_input(self, convs, x, merge, up=None):
        """1x1 convs [(tensor name, prefix, relu)] that all read x -> {tensor name: tensor}: ONE launch with one output per conv (conv_seg)
        where `merge` says so and there are at least two of them, else one launch each, in order.  up (the fused bilinear add) belongs to the first."""
        if merge and len(convs) >= 2:
            outs = self.conv_seg(convs, x, up=up)
        else:
            outs = [self.conv(nm, [pre], x, relu=relu, up=up if k == 0 else None) for k, (nm, pre, relu) in enumerate(convs)]
        return dict(zip([nm for nm, _, _ in convs], outs))

    def _unit(self, s, ind, xin, below, tl, gen_skip, heads, head_t):
        """Upsample_unit up{ind + 1} of stage s on xin (smap.py:210-241).  below: the previous unit's `out`; tl: this unit's up_conv@low
        (up_conv commuted with the upsample: evaluated on `below`) where the previous unit's launch on `out` has made it already.  heads: the
        inference heads of the last stage, into head_t.  Returns (out, the next unit's up_conv@low or None, skip1, skip2, cross_conv) -- None for
        what this unit does not make.

        Shared-input 1x1s as ONE launch with one output per conv (conv_seg).  Measured (profiles/r5_v1_*): the launches on `out` (skip2 |
        cross_conv | res_conv1 | the next unit's up_conv) are 3-33 % faster merged than one by one at every level; u_skip | skip1 on x is faster
        merged where u_skip has no fused bilinear add (up1: 228 vs 244 us at 16 frames) and SLOWER where it has one (128x208: 712 vs 610 us;
        32x52: 277 vs 256): one tile shape must then serve the bilinear epilogue (which wants the 256-wide tile) and the plain skip1 (which
        wants the eight-wave 128x128 one).  SchedulePolicy.merge_1x1: 1 (default) = the merges that pay, 2 = all of them, 0 = one launch per
        conv -- the baseline the merged schedules are compared against: nothing merged, no two-input or tap-dot launch, no side lane, and this
        unit's up_conv@low at the top of the unit."""
        mode, pol = self.policy.merge_1x1, self.policy
        u = f"stage{s}.upsample.up{ind + 1}"
        un = f"stage{s}.upsample.up{ind + 2}"                    # the next unit: its up_conv reads this unit's `out`
        side = lambda lane: self.on_lane(lane if mode else 0)
        if ind and not mode:
            tl = self.conv(u + ".up_conv@low", [u + ".up_conv"], below, relu=False)
        # The inter-stage skips as ONE tensor per level: skip1(x) + skip2(out) in one launch (conv_relusum); the next stage adds that one tensor.
        # SchedulePolicy.skipsum = False: round 5's two tensors (skip1 beside u_skip, skip2 as a segment of the launch on `out`).  Not beyond one
        # 4 GiB window; small schedules: as conv_cat.
        skipsum = gen_skip and mode != 0 and pol.skipsum is not False and self.one_window and (pol.skipsum or not self.small)
        # on the unit's input:  out = relu(u_skip(x) [+ bilinear(up_conv@low)])  |  skip1 = relu(skip1(x))
        on_x = [(u + ".out", u + ".u_skip", True)] + ([(u + ".skip1", u + ".skip1", True)] if gen_skip and not skipsum else [])
        if tl is not None and not mode and pol.no_upadd_fusion and not self.x3:      # the bilinear add as a launch of its own, not the conv's epilogue
            a = self.conv(u + ".u_skip", [u + ".u_skip"], xin, relu=False)
            out = self.tensor(u + ".out", a.H, a.W, a.C)
            self.ops.append(Op(OP_UPADD, out=out, inp=a, aux=[tl], p=dict(relu=1)))
            got = self._shared_input(on_x[1:], xin, False)
        else:
            got = self._shared_input(on_x, xin, mode == 2 or (mode == 1 and tl is None), up=tl)
            out = got[u + ".out"]
        if skipsum:
            got[u + ".skip1"] = self.conv_relusum(u + ".skipsum", u + ".skip1", xin, u + ".skip2", out)
        # on `out`: skip2 | cross_conv (stages with skips), res_conv1 (last stage), the next unit's up_conv@low
        on_out = [(u + ".skip2", u + ".skip2", True)] if gen_skip and not skipsum else []
        if gen_skip and ind == 3:
            on_out.append((u + ".cross_conv", u + ".cross_conv", True))
        if heads and 1 <= ind < 3:
            on_out.append((u + ".res1", u + ".res_conv1", True))
        if ind < 3 and mode:
            on_out.append((un + ".up_conv@low", un + ".up_conv", False))
        got.update(self._shared_input(on_out, out, mode != 0))
        if heads and ind == 3:
            # The root-depth head (res_rd_conv1 -> res_rd_conv2, a 3x3 with ONE output channel) as a 1x1 launch whose epilogue
            # keeps nine dot products per pixel instead of the 256-channel activation, + a nine-term stencil (conv_tapdot / tapsum):
            # 0.87 GB per 16 frames and the N = 1 MFMA launch (8.9 TFLOP/s) gone.  SchedulePolicy.taphead = False: round 5's three-way 1x1 + 3x3.
            tap = mode != 0 and self.chl == 256 and pol.taphead is not False and (pol.taphead or not self.small)
            m = self.conv(u + ".heads1x1", [u + ".res_conv1", u + ".res_d_conv1"] + ([] if tap else [u + ".res_rd_conv1"]), out, relu=True)
            c = self.chl
            head_t["res4"] = self.conv(u + ".res", [u + ".res_conv2"], m, 3, relu=False, in_c_off=0, cin=c, out_fp32=True)
            with side(1):     # the three 3x3 heads read disjoint channel slices of m: side by side
                head_t["res_d"] = self.conv(u + ".res_d", [u + ".res_d_conv2"], m, 3, relu=False, in_c_off=c, cin=c, out_fp32=True, frames=self.frames)
            with side(2):
                if tap:
                    head_t["res_rd_tap"] = self.conv_tapdot(u + ".res_rd_t", u + ".res_rd_conv1", u + ".res_rd_conv2", out, frames=self.frames)
                else:
                    head_t["res_rd"] = self.conv(u + ".res_rd", [u + ".res_rd_conv2"], m, 3, relu=False, in_c_off=2 * c, cin=c,
                                                 out_fp32=True, frames=self.frames)
        elif heads and ind >= 1:
            with side(1):     # the 3x3 head of this unit runs beside the next unit's launches
                head_t[f"res{ind + 1}"] = self.conv(u + ".res", [u + ".res_conv2"], got[u + ".res1"], 3, relu=False, out_fp32=True)
        if self.keep_unit_in:
            self.unit_in[(s, ind)] = xin
            self.keep.append(xin)
        self._train_heads(s, ind, u, out, head_t if heads else {})
        return out, got.get(un + ".up_conv@low"), got.get(u + ".skip1"), got.get(u + ".skip2"), got.get(u + ".cross_conv")

    def _outputs(self, head_t):
        """The output buffer: its layout (out_layout, the status words behind the maps) and the ops that write it from the last stage's heads."""
        B, h, w = self.frames, self.out_h, self.out_w
        n_hms, n_d = self.kpt_paf, self.paf
        flip_p = {}
        if self.flip_pair is not None:         # pair table of the in-schedule flip-TTA merge lives in the weight blob
            flip_p = dict(flip_from=self.frames, n_kpt=n_hms - 2 * n_d, w_off=self._add_w(torch.tensor(self.flip_pair, dtype=torch.int32)))
        self.out_layout = dict(hms=(0, n_hms), det_d=(B * n_hms * h * w * 4, n_d), root_d=(B * (n_hms + n_d) * h * w * 4, 1))
        self.out_bytes = B * (n_hms + n_d + 1) * h * w * 4
        self.status_off = self.out_bytes                 # int32 status words behind the maps (include/smap_hip.h)
        self.status_words = (B + 30) // 31               # SMAP_STATUS_WORDS: frame f = word f // 31, bit 1 + f % 31
        # outputs_2d = res4 + res3 + res2 (smap.py:417)
        self.ops.append(Op(OP_HEADSUM, aux=[head_t["res4"], head_t["res3"], head_t["res2"]],
                           p={**dict(Cout=n_hms, ext_off=self.out_layout["hms"][0], n_kpt=n_hms - 2 * n_d, scale_hms=int(self.scaled_hms)), **flip_p}))
        with self.on_lane(1):
            self.ops.append(Op(OP_HEADSUM, aux=[head_t["res_d"]], p=dict(Cout=n_d, ext_off=self.out_layout["det_d"][0])))
        with self.on_lane(2):
            if "res_rd_tap" in head_t:
                self.tapsum(*head_t["res_rd_tap"], self.out_layout["root_d"][0])
            else:
                self.ops.append(Op(OP_HEADSUM, aux=[head_t["res_rd"]], p=dict(Cout=1, ext_off=self.out_layout["root_d"][0])))

    def _train_heads(self, s, ind, u, out, head_t):
        """all_heads: the head chains of unit `u` (stage s, up{ind + 1}) that the inference schedule does not run, on `out`, with the launches
        the inference heads use: ONE 1x1 launch for the missing res_conv1 | res_d_conv1 | res_rd_conv1 (shared input, concatenated along
        Cout), then a 3x3 per head on its channel slice, fp32 out at the unit's resolution.  head_t: what the unit has already (the last
        stage's inference heads).  Flip-TTA: the first `frames` frames only, the loss never reads the mirrored half."""
        if not self.all_heads:
            return
        if self.keep_unit_out:
            self.unit_out[(s, ind)] = out
            self.keep.append(out)
        have = {"heatmap_2d": head_t.get(f"res{ind + 1}"), "det_d": head_t.get("res_d") if ind == 3 else None,
                "root_d": head_t.get("res_rd") if ind == 3 else None}
        rd_in_output = ind == 3 and "res_rd_tap" in head_t       # tap-dot route: the map exists as the output buffer's NCHW block only
        todo = [(key, nm) for key, nm in (("heatmap_2d", "res"), ("det_d", "res_d"), ("root_d", "res_rd"))
                if have[key] is None and not (key == "root_d" and rd_in_output)]
        if todo:
            c = self.chl
            m = self.conv(u + ".heads1x1", [f"{u}.{nm}_conv1" for _, nm in todo], out, relu=True, frames=self.frames)
            for k, (key, nm) in enumerate(todo):
                have[key] = self.conv(f"{u}.{nm}", [f"{u}.{nm}_conv2"], m, 3, relu=False, in_c_off=k * c, cin=c, out_fp32=True,
                                      frames=self.frames)
        self.head_tensors[(s, ind)] = have
        self.keep += [t for t in have.values() if t is not None]

    # -- arena: liveness-based first-fit allocation
    def _producers(self):
        """id(tensor) -> index of the op that writes it."""
        return {id(t): i for i, op in enumerate(self.ops) for t in op.writes()}

    def allocate(self, reuse=True):
        """Offsets for every tensor; reuse=False: no two tensors share a byte (read_tensor).  Returns the arena's size."""
        self._liveness()
        return self._place(reuse)

    def _liveness(self):
        """first / last of every tensor = the ops between which its bytes are its own."""
        for i, op in enumerate(self.ops):
            for t in op.reads():
                t.last = i
            for t in op.writes():
                t.first = i
                t.last = max(t.last, i)
            for t in op.scratch:
                t.first = t.last = i
        # Lanes: an op on a side lane may start as soon as its producers are done and end as late as the schedule does.  What it WRITES is
        # therefore live from the op after its last producer, what it READS stays live to the end of the schedule (smap_op.lane's contract).
        producer = self._producers()
        n_last = len(self.ops) - 1
        for op in self.ops:
            if not op.lane:
                continue
            start = 1 + max([producer.get(id(t), -1) for t in op.reads()] + [-1])
            for t in op.writes() + op.scratch:
                t.first = min(t.first, start)
            for t in op.reads() + op.scratch:
                t.last = n_last
        if self.kcount is not None:                                # the tickets of every split-K op: one region, alive for the whole schedule
            self.kcount.first, self.kcount.last = 0, n_last
        for t in self.keep:                                        # (all_heads: the loss reads the head tensors behind the schedule)
            t.last = n_last

    def _place(self, reuse):
        """Window-aware first fit in order of `first`: a tensor takes the smallest free block that holds it, else the top of the arena."""
        every = self.tensors + self.scratch_tensors + ([self.kcount] if self.kcount is not None else [])
        # arena[k * WINDOW : k * WINDOW + ZERO_PAGE] are the conv kernels' zero pages (csrc/plan.hip): never allocated, so no
        # tensor crosses a window boundary and every conv input is within 32 bits of its window's base
        for t in every:
            if _rup(t.nbytes, ALIGN) > WINDOW - ZERO_PAGE:
                raise ArenaTooLarge(f"{t.name}: {t.nbytes / 2 ** 30:.2f} GiB ({self.B} frames, precision {self.precision}) does not fit a "
                                    "4 GiB addressing window of the conv kernels -- use a smaller batch (PosePipeline splits by itself)")
        by_first, expiring = {}, {}
        for t in every:
            by_first.setdefault(t.first, []).append(t)
            expiring.setdefault(t.last, []).append(t)
        # Both inputs of a two-input launch (conv_cat / conv_relusum) are addressed from one 64-bit base: they must share a window.  The
        # builder makes such launches only where the reusing arena fits one window; an arena that keeps every tensor (reuse=False, for
        # read_tensor) does not, and there the two are placed side by side when the first of them is.
        group = {}
        if not reuse:
            for op in self.ops:
                if op.kind == OP_CONV and "cat" in op.p:
                    g = list({id(t): t for t in group.get(id(op.inp), [op.inp]) + group.get(id(op.aux2), [op.aux2])}.values())
                    for t in g:
                        group[id(t)] = g
                        t.off = -1
        free, top = _FreeList(), ZERO_PAGE
        for i in range(len(self.ops)):
            for t in by_first.get(i, []):
                if t.off >= 0 and id(t) in group:                  # (placed with its partner)
                    continue
                off = free.take(_rup(t.nbytes, ALIGN)) if reuse else None
                if off is not None:
                    t.off = off
                    continue
                members = [m for m in group.get(id(t), [t]) if m is t or m.off < 0]
                need = sum(_rup(m.nbytes, ALIGN) for m in members)
                nxt = (top // WINDOW + 1) * WINDOW                 # start of the next window = its zero page
                if top + need > nxt:                               # would run into it: leave the rest of this window free
                    if reuse and nxt > top:
                        free.blocks.append((top, nxt - top))
                    top = nxt + ZERO_PAGE
                for m in members:
                    m.off = top
                    top += _rup(m.nbytes, ALIGN)
            for t in expiring.get(i, []):
                if reuse and t.off >= 0:
                    free.give(t.off, _rup(t.nbytes, ALIGN))
        self.arena_bytes = max(top, ALIGN)
        for t in every:
            if t.off >= 0:
                assert t.off % WINDOW >= ZERO_PAGE and t.off // WINDOW == (t.off + t.nbytes - 1) // WINDOW, t.name
        return self.arena_bytes

    def emit(self):
        arr = (_L.SmapOp * len(self.ops))()
        producer = self._producers()
        for i, op in enumerate(self.ops):
            o = arr[i]
            C.memset(C.byref(o), 0, C.sizeof(o))
            # lanes: wait for the latest producer on every OTHER lane (ops of one lane are ordered by their stream)
            o.lane = op.lane
            waits = {}
            for pi in (producer[id(t)] for t in op.reads() if id(t) in producer):
                ln = self.ops[pi].lane
                if ln != op.lane:
                    waits[ln] = max(waits.get(ln, -1), pi)
            for k in range(4):
                o.wait_op[k] = -1
            for k, pi in enumerate(sorted(waits.values())):
                o.wait_op[k] = pi
            o.n_wait = len(waits)
            o.kind = op.kind
            o.B = self.B
            o.res_off = o.add1_off = o.add2_off = -1
            for k in range(3):
                o.aux_off[k] = -1
            o.in_off = o.out_off = o.w_off = o.bias_off = o.ext_off = -1
            o.precision, o.acc_scale = int(self.x3), 1.0
            p = op.p
            if op.kind == OP_CONV:
                self._emit_conv(o, op)
            elif op.kind in (OP_STEM, OP_STEMPOOL):
                y = op.out
                o.H, o.W, o.Cin, o.Ho, o.Wo, o.Cout = self.H, self.W, 3, y.H, y.W, 64
                o.ksize, o.stride, o.pad, o.relu = 7, 2, 3, 1
                o.out_off, o.w_off, o.bias_off = y.off, p["w_off"], p["bias_off"]
                o.acc_scale = p["acc_scale"]
                o.flip_from = self.frames if self.flip_pair is not None else 0
            elif op.kind == OP_MAXPOOL:
                x, y = op.inp, op.out
                o.H, o.W, o.Cin, o.Ho, o.Wo, o.Cout = x.H, x.W, x.C, y.H, y.W, y.C
                o.ksize, o.stride, o.pad = 3, 2, 1
                o.in_off, o.out_off = x.off, y.off
            elif op.kind == OP_UPADD:
                x, y, t = op.inp, op.out, op.aux[0]
                o.H, o.W, o.Cin, o.Ho, o.Wo, o.Cout = x.H, x.W, x.C, y.H, y.W, y.C
                o.relu = p["relu"]
                o.in_off, o.out_off = x.off, y.off
                o.aux_off[0], o.aux_h[0], o.aux_w[0] = t.off, t.H, t.W
            elif op.kind == OP_TAPSUM:
                t = op.aux[0]
                o.H, o.W, o.Cin, o.Ho, o.Wo, o.Cout = t.H, t.W, t.C, self.out_h, self.out_w, 1
                o.aux_off[0], o.aux_h[0], o.aux_w[0] = t.off, t.H, t.W
                o.ext_off, o.bias_off = p["ext_off"], p["bias_off"]
                o.B = self.frames
                o.status_off = self.status_off
            elif op.kind == OP_HEADSUM:
                s0 = op.aux[0]
                assert all(t.C == s0.C and t.esize == 4 for t in op.aux)
                o.H, o.W, o.Cin, o.Ho, o.Wo, o.Cout = s0.H, s0.W, s0.C, self.out_h, self.out_w, p["Cout"]
                o.n_aux = len(op.aux)
                for k, t in enumerate(op.aux):
                    o.aux_off[k], o.aux_h[k], o.aux_w[k] = t.off, t.H, t.W
                o.ext_off = p["ext_off"]
                o.B = self.frames                          # output frames (flip-TTA: the mirrored half is merged in)
                o.status_off = self.status_off
                if p.get("flip_from"):
                    o.flip_from, o.in_c_off, o.w_off = p["flip_from"], p["n_kpt"], p["w_off"]
                if p.get("scale_hms"):
                    o.scale_hms, o.in_c_off = 1, p["n_kpt"]
        return arr

    def _emit_conv(self, o, op):
        """The smap_op fields of a conv launch (every Graph.conv* emitter), behind the defaults emit() has set."""
        p, x, y = op.p, op.inp, op.out
        o.B = p["frames"]
        o.H, o.W, o.Cin, o.in_stride_c, o.in_c_off = x.H, x.W, p["Cin"], x.C * x.planes, p["in_c_off"]
        o.Ho, o.Wo, o.Cout = y.H, y.W, p["Cout"]
        o.ksize, o.stride, o.pad, o.relu = p["ksize"], p["stride"], p["pad"], p["relu"]
        o.cout_pad, o.out_stride_c, o.out_c_off = p["cout_pad"], y.C * y.planes, 0
        o.acc_scale = p["acc_scale"]
        o.w_pairs = p["w_pairs"]
        o.out_fp32, o.tile = p["out_fp32"], p["tile"]
        if "tail" in p:
            tl = p["tail"]
            o.tail_cout, o.tail_cout_pad, o.tail_acc_scale = tl["cout"], tl["cout_pad"], tl["acc_scale"]
            o.tail_w_off, o.tail_bias_off = tl["w_off"], tl["bias_off"]
        if "head" in p:
            hd = p["head"]
            o.head_cin, o.head_acc_scale, o.head_w_off, o.head_bias_off = hd["cin"], hd["acc_scale"], hd["w_off"], hd["bias_off"]
        if "short" in p:
            o.short_w_off, o.short_acc_scale = p["short"]["w_off"], p["short"]["acc_scale"]
        o.in_off, o.out_off, o.w_off, o.bias_off = x.off, y.off, p["w_off"], p["bias_off"]
        for nm in ("res", "add1", "add2"):
            t = getattr(op, nm)
            if t is not None:
                assert (t.H, t.W, t.C) == (y.H, y.W, y.C) and t.esize == 2, (y.name, nm)
                setattr(o, nm + "_off", t.off)
        if op.aux:
            t = op.aux[0]
            assert t.C == y.C and t.esize == 2
            o.aux_off[0], o.aux_h[0], o.aux_w[0] = t.off, t.H, t.W
        if "tap" in p:
            o.tap_n, o.tap_w_off, o.tap_scale = 9, p["tap"]["w_off"], p["tap"]["scale"]
            o.out_stride_c = 16
        if "cat" in p:
            t = op.aux2
            assert t.off // WINDOW == x.off // WINDOW, (y.name, "both inputs of a conv_cat launch must lie in one 4 GiB window")
            o.in2_off, o.in2_H, o.in2_W, o.in2_C, o.in2_stride_c, o.in2_stride = t.off, t.H, t.W, p["cat"]["cin"], t.C * t.planes, p["cat"]["stride"]
            if p["cat"].get("relusum"):
                o.in2_mode, o.in2_acc_scale, o.in2_bias_off = 1, p["cat"]["acc_scale"], p["cat"]["bias_off"]
        if p.get("ksplit", 1) > 1:
            o.ksplit, o.kpart_off, o.kcount_off = p["ksplit"], op.scratch[0].off, self.kcount.off + 4 * p["kcount_first"]
        for j, (sg, t) in enumerate(zip(p.get("segs", []), op.outs)):
            assert (t.H, t.W, t.C) == (y.H, y.W, sg["cout"]) and t.esize == 2
            o.seg_n[j], o.seg_cout[j], o.seg_relu[j], o.seg_acc_scale[j] = sg["n0"], sg["cout"], sg["relu"], sg["acc_scale"]
            o.seg_out_stride_c[j], o.seg_out_off[j] = t.C * t.planes, t.off

    def blob(self):
        """The allocated schedule as one relocatable byte image (include/smap_hip.h "plan blob": smap_blob_header | smap_op[n]
        | weight section), little-endian: smap_plan_create_from_blob validates it and hands back the buffer sizes and the
        output layout, so that a host with nothing but the header can run SMAP.forward (tests/c/blob_runner.c)."""
        ops = self.emit()
        n_ops = len(self.ops)
        hdr = _L.BlobHeader()
        ops_off = _rup(C.sizeof(hdr), ALIGN)
        ops_bytes = C.sizeof(_L.SmapOp) * n_ops
        w_off = _rup(ops_off + ops_bytes, ALIGN)
        wblob = self.weight_blob().numpy().tobytes()
        hdr.magic, hdr.version, hdr.sizeof_op, hdr.header_bytes = b"SMAPPLN1", _L.BLOB_VERSION, C.sizeof(_L.SmapOp), C.sizeof(hdr)
        hdr.n_ops, hdr.ops_offset = n_ops, ops_off
        hdr.weights_offset, hdr.weights_bytes = w_off, len(wblob)
        hdr.arena_bytes, hdr.out_bytes = self.arena_bytes, self.out_bytes + 4 * self.status_words
        i = hdr.info
        i.frames, i.H, i.W, i.out_h, i.out_w = self.frames, self.H, self.W, self.out_h, self.out_w
        i.n_hms, i.n_det, i.n_root, i.precision = self.kpt_paf, self.paf, 1, int(self.x3)
        i.arena_bytes, i.out_bytes, i.weights_offset, i.weights_bytes = hdr.arena_bytes, hdr.out_bytes, w_off, len(wblob)
        i.hms_off, i.det_off, i.root_off = self.out_layout["hms"][0], self.out_layout["det_d"][0], self.out_layout["root_d"][0]
        i.status_off = self.status_off
        out = bytearray(w_off + len(wblob))
        out[:C.sizeof(hdr)] = bytes(hdr)
        out[ops_off:ops_off + ops_bytes] = bytes(ops)
        out[w_off:] = wblob
        return bytes(out)

    def weight_blob(self):
        blob = torch.zeros((max(self.woff, ALIGN),), dtype=torch.uint8)
        for off, raw in self.wchunks:
            blob[off:off + raw.numel()] = raw
        return blob


# ----------------------------------------------------------------------------- plan cache
# Building a schedule is 2.5-10 s of Python (BN folding in f64, hi/lo splits, weight packing for ~150 launches); its result -- Graph.blob():
# ops + packed weights -- depends only on the checkpoint, the shape, the arithmetic, the tile tables and this file.  With SMAP_PLAN_CACHE=<dir>
# (exps/stage3_root2/test.py defaults it to ~/.cache/smap_amd) BackboneEngine stores the blob there and the next process loads it through
# smap_plan_create_from_blob: < 1 s from the page cache instead of the build.  At most PLAN_CACHE_KEEP blobs are kept (oldest out).
PLAN_CACHE_KEEP = 6


def plan_cache_dir():
    d = os.environ.get("SMAP_PLAN_CACHE", "")
    return None if d in ("", "0") else os.path.expanduser(d)


def state_hash(sd):
    """Content hash of a state dict (keys, shapes, dtypes, bytes): xxh3 when the module is there (~10 GB/s), else blake2b."""
    try:
        import xxhash
        h = xxhash.xxh3_128()
    except ImportError:                                     # pragma: no cover
        import hashlib
        h = hashlib.blake2b(digest_size=16)
    for k in sorted(sd):
        t = sd[k].detach().cpu().contiguous()
        h.update(f"{k}|{tuple(t.shape)}|{t.dtype}|".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().data if t.numel() else b"")
    return h.hexdigest()


# The schedule builder's source, hashed into the key: EVERY module the builder imports schedule logic from belongs in this tuple.
BUILDER_SOURCES = ("engine.py",)


def plan_cache_key(sd, B, H, W, stage_num, chl, kpt_paf, paf, precision, flip_pair, scaled_hms, all_heads=False, policy=None, keep_unit_out=False,
                   keep_unit_in=False):
    import hashlib
    policy = policy or SchedulePolicy.from_env()
    h = hashlib.blake2b(digest_size=16)
    h.update(repr((state_hash(sd), B, H, W, stage_num, chl, kpt_paf, paf, precision, tuple(flip_pair) if flip_pair is not None else None,
                   bool(scaled_hms), _L.BLOB_VERSION, C.sizeof(_L.SmapOp), _L.version(), policy.cache_token(), bool(all_heads))
                  + ((True,) if keep_unit_out else ()) + (("in",) if keep_unit_in else ())).encode())        # (the tuple grows only where a flag is set)
    for f in BUILDER_SOURCES:
        h.update(open(os.path.join(_HERE, f), "rb").read())
    return h.hexdigest()


HeadSource = namedtuple("HeadSource", "ptr h w c pix_stride ch_stride frame_stride")
HEAD_KEYS = (("heatmap_2d", "kpt_paf"), ("det_d", "paf"), ("root_d", None))


def graph_head_sources(g, arena_ptr=0, out_ptr=0):
    """BackboneEngine.head_sources of an allocated all_heads Graph whose arena and output buffer start at these addresses."""
    res = []
    for s in range(g.stage_num):
        for ind in range(4):
            d = {}
            for key, attr in HEAD_KEYS:
                t, c = g.head_tensors[(s, ind)][key], (getattr(g, attr) if attr else 1)
                if t is not None:            # fp32 NHWC in the arena
                    assert t.esize == 4 and t.off >= 0 and t.C >= c
                    d[key] = HeadSource(arena_ptr + t.off, t.H, t.W, c, t.C, 1, t.H * t.W * t.C)
                else:                        # the [frames, 1, h, w] block of the output buffer
                    hw = g.out_h * g.out_w
                    d[key] = HeadSource(out_ptr + g.out_layout[key][0], g.out_h, g.out_w, c, 1, hw, c * hw)
            res.append(d)
    return res


# ----------------------------------------------------------------------------- engine
class BackboneEngine:
    """Device-resident schedule for one (B, H, W): weights, arena, output buffer, plan."""

    def __init__(self, state_dict, B, H, W, device, stage_num=3, chl=256, kpt_paf=43, paf=14, reuse=True,
                 precision="f16", flip_pair=None, scaled_hms=False, all_heads=False, keep_unit_out=False, keep_unit_in=False):
        self.lib = _L.load()          # fails loudly when libsmap_hip.so is missing
        self.precision = precision
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("BackboneEngine needs a ROCm GPU device (no CPU path in smap_amd)")
        sd = {k: v.detach().cpu() for k, v in state_dict.items()}
        self.policy = SchedulePolicy.from_env()            # what the plan is made under: the cache key, and engine.graph whenever it is built
        self._graph_args = (sd, B, H, W, stage_num, chl, kpt_paf, paf, precision, flip_pair, scaled_hms, reuse, bool(all_heads), self.policy,
                            bool(keep_unit_out), bool(keep_unit_in))
        if keep_unit_out and not all_heads:
            raise ValueError("keep_unit_out needs all_heads=True")
        if keep_unit_in and not all_heads:
            raise ValueError("keep_unit_in needs all_heads=True")
        self.all_heads, self.stage_num, self.keep_unit_out, self.keep_unit_in = bool(all_heads), stage_num, bool(keep_unit_out), bool(keep_unit_in)
        self._graph = None
        self.B, self.H, self.W = B, H, W
        self.kpt_paf, self.paf = kpt_paf, paf
        self.from_cache = False
        cdir = plan_cache_dir() if reuse else None         # (reuse=False: debugging layouts, never cached)
        meta = None
        if cdir is not None:
            self.cache_key = plan_cache_key(sd, B, H, W, stage_num, chl, kpt_paf, paf, precision, flip_pair, scaled_hms, all_heads, self.policy,
                                            keep_unit_out, keep_unit_in)
            meta = self._load_cached(cdir)
        if meta is None:
            g = self.graph                                 # builds and allocates the schedule
            meta = dict(arena_bytes=g.arena_bytes, out_h=g.out_h, out_w=g.out_w, out_bytes=g.out_bytes, status_words=g.status_words,
                        lanes=int(g.lanes), flops=g.flops, alg_bytes=g.alg_bytes, n_ops=len(g.ops))
        budget = arena_budget(self.device)
        if meta["arena_bytes"] > budget:
            raise ArenaTooLarge(f"the activation arena of a {B}-frame schedule ({precision}{', flip-TTA' if flip_pair is not None else ''}) takes "
                                f"{meta['arena_bytes'] / 2 ** 30:.2f} GiB, the budget is {budget / 2 ** 30:.2f} GiB (SMAP_MAX_ARENA_BYTES / 90 % of the "
                                "device memory shared by 4 arenas): use smaller launches")
        self.h, self.w = meta["out_h"], meta["out_w"]
        self.n_ops = meta["n_ops"]
        if not self.from_cache:
            g = self.graph
            self.ops = g.emit()
            self.weights = g.weight_blob().to(self.device)
            handle = C.c_void_p()
            with torch.cuda.device(self.device):
                _L.check(self.lib.smap_plan_create(self.ops, self.n_ops, C.byref(handle)), "smap_plan_create")
            self.handle = handle
            if cdir is not None:
                self._store_cached(cdir, meta)
        self.arena = torch.zeros((meta["arena_bytes"],), dtype=torch.uint8, device=self.device)
        if meta["lanes"]:
            _L.check(self.lib.smap_plan_set_lanes(self.handle, 1), "smap_plan_set_lanes")
        self.out_floats = meta["out_bytes"] // 4
        self.status_words = meta["status_words"]
        self.out = self.new_output()                      # default output buffer
        self.hms, self.det_d, self.root_d = self.views(self.out)
        self.flops_per_batch = meta["flops"]
        self.alg_bytes_per_batch = meta["alg_bytes"]      # conv launches only (stem / pool / head sums are < 3 % more)

    @property
    def graph(self):
        """The schedule as Python objects (ops, tensors, weight chunks).  An engine loaded from the plan cache builds it only when somebody
        asks (profiling tools, tests, blob()): the launches themselves need the plan handle alone."""
        if self._graph is None:
            sd, B, H, W, stage_num, chl, kpt_paf, paf, precision, flip_pair, scaled_hms, reuse, all_heads, policy, keep_unit_out, keep_unit_in = self._graph_args
            g = Graph(sd, B, H, W, stage_num, chl, kpt_paf, paf, precision=precision, flip_pair=flip_pair, scaled_hms=scaled_hms,
                      all_heads=all_heads, policy=policy, keep_unit_out=keep_unit_out, keep_unit_in=keep_unit_in)
            g.allocate(reuse=reuse)
            self._graph = g
        return self._graph

    def _load_cached(self, cdir):
        """Plan + weights from <cdir>/<key>.smapplan through smap_plan_create_from_blob, or None (absent / refused: rebuilt and rewritten)."""
        import json
        path = os.path.join(cdir, self.cache_key + ".smapplan")
        if not (os.path.exists(path) and os.path.exists(path + ".json")):
            return None
        try:
            meta = json.load(open(path + ".json"))
            raw = torch.from_file(path, shared=False, size=os.path.getsize(path), dtype=torch.uint8)
            handle, info = C.c_void_p(), _L.BlobInfo()
            with torch.cuda.device(self.device):
                rc = self.lib.smap_plan_create_from_blob(C.c_void_p(raw.data_ptr()), raw.numel(), C.byref(handle), C.byref(info))
            if rc != 0 or info.arena_bytes != meta["arena_bytes"] or info.frames != self.B:
                return None
            self.weights = raw[info.weights_offset:info.weights_offset + info.weights_bytes].to(self.device)
            self.handle, self.ops, self.from_cache = handle, None, True
            os.utime(path)                                  # most recently used
            return meta
        except Exception:                                   # a damaged cache entry is not an error: build the schedule
            return None

    def _store_cached(self, cdir, meta):
        import json
        try:
            os.makedirs(cdir, exist_ok=True)
            path = os.path.join(cdir, self.cache_key + ".smapplan")
            tmp = f"{path}.{os.getpid()}.tmp"
            with open(tmp, "wb") as f:
                f.write(self.graph.blob())
            os.replace(tmp, path)
            json.dump(meta, open(path + ".json", "w"))
            old = sorted((p for p in (os.path.join(cdir, n) for n in os.listdir(cdir)) if p.endswith(".smapplan")), key=os.path.getmtime)
            for p_ in old[:-PLAN_CACHE_KEEP]:
                for q in (p_, p_ + ".json"):
                    if os.path.exists(q):
                        os.remove(q)
        except OSError:                                     # read-only home, full disk: the cache is an optimisation
            pass

    def sibling(self):
        """A second executor of the same schedule with its own arena (weights and plan shared), so that
        two batches can be in flight on two streams."""
        import copy
        e = copy.copy(self)                # (shares _graph / _graph_args too)
        e.arena = torch.zeros_like(self.arena)
        e.out = e.new_output()
        e.hms, e.det_d, e.root_d = e.views(e.out)
        e._is_sibling = True
        e._parent = self               # the shared plan handle lives as long as any executor of it
        return e

    def new_output(self):
        """A fresh fp32 output buffer (hms | det_d | root_d | status words); pass it to run(out=...) to double-buffer.
        Zero-filled: a partial run(first, count) (debug / trace tools) must not hand back uninitialised memory."""
        return torch.zeros((self.out_floats + self.status_words,), dtype=torch.float32, device=self.device)

    def status(self, out=None):
        """The status word of the last run into `out` (synchronises): bit 0 = a non-finite value reached the output
        maps, i.e. an activation left the fp16 range on the way (split precision has fp16's range, not fp32's)."""
        buf = self.out if out is None else out
        return int(buf[self.out_floats:self.out_floats + 1].view(torch.int32).item())

    def bad_frames(self, out=None):
        """Output frames of the last run into `out` whose maps hold a non-finite value (synchronises): frame f is bit 1 + f % 31 of
        status word f // 31."""
        buf = self.out if out is None else out
        words = buf[self.out_floats:self.out_floats + self.status_words].view(torch.int32).tolist()
        return [f for f in range(self.B) if (words[f // 31] >> (1 + f % 31)) & 1]

    def raise_if_nonfinite(self, out=None):
        if self.status(out) & 1:
            raise RuntimeError("SMAP backbone produced non-finite outputs: an activation exceeded the fp16 range (65504) of the "
                               f"'{self.precision}' arithmetic; see INTEGRATION.md section 5")

    def views(self, out):
        B, n = self.B, self.B * self.h * self.w
        k, p = self.kpt_paf, self.paf
        return (out[:n * k].view(B, k, self.h, self.w), out[n * k:n * (k + p)].view(B, p, self.h, self.w),
                out[n * (k + p):n * (k + p + 1)].view(B, 1, self.h, self.w))

    def __del__(self):
        try:
            if getattr(self, "_is_sibling", False):
                return
            if getattr(self, "handle", None):
                self.lib.smap_plan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def run(self, imgs, first=0, count=None, out=None):
        """imgs: [B,3,H,W] fp32 contiguous on the device -- or a list / tuple of n (1..8, a divisor of B) such tensors of B / n
        frames each, read where they are (smap_plan_run_inputs: no gather copy in front of the stem).  Returns (hms, det_d,
        root_d) views of the output buffer `out` (default: the engine's own, overwritten by the next run)."""
        parts = list(imgs) if isinstance(imgs, (list, tuple)) else [imgs]
        n = len(parts)
        if not 1 <= n <= _L.MAX_INPUTS or self.B % n:
            raise ValueError(f"{n} input buffers for a schedule of {self.B} frames (1..{_L.MAX_INPUTS} buffers, a divisor of the batch)")
        for t in parts:
            if tuple(t.shape) != (self.B // n, 3, self.H, self.W) or t.dtype != torch.float32 or not t.is_cuda:
                raise ValueError(f"imgs must be float32 GPU tensor(s) [{self.B // n},3,{self.H},{self.W}], got "
                                 f"{tuple(t.shape)} {t.dtype} {t.device}")
        parts = [t.contiguous() for t in parts]
        dev0 = parts[0].device
        if out is not None and (out.dtype != torch.float32 or out.device != dev0 or not out.is_contiguous()
                                or out.numel() < self.out_floats + self.status_words):
            # the maps are followed by the status words: a buffer of the pre-round-3 size would be written past its end
            raise ValueError(f"out must be a contiguous float32 tensor of >= {self.out_floats + self.status_words} elements on {dev0} "
                             f"(BackboneEngine.new_output()), got {out.dtype} x {out.numel()} on {out.device}")
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        outp = C.c_void_p((self.out if out is None else out).data_ptr())
        with torch.cuda.device(self.device):
            if n == 1 or first != 0 or count is not None:
                if n != 1:
                    raise ValueError("partial runs (first / count) take one input buffer")
                count = self.n_ops - first if count is None else count
                _L.check(self.lib.smap_plan_run_range(self.handle, first, count, C.c_void_p(parts[0].data_ptr()),
                                                      C.c_void_p(self.arena.data_ptr()), C.c_void_p(self.weights.data_ptr()), outp, st),
                         "smap_plan_run")
            else:
                ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in parts])
                _L.check(self.lib.smap_plan_run_inputs(self.handle, ptrs, n, C.c_void_p(self.arena.data_ptr()),
                                                       C.c_void_p(self.weights.data_ptr()), outp, st), "smap_plan_run_inputs")
        return (self.hms, self.det_d, self.root_d) if out is None else self.views(out)

    def head_sources(self, out=None):
        """all_heads engines: where the loss reads the 36 head tensors of the last run into `out` (default: the engine's own buffer).
        A list over heads h = 4 * stage + j (j = 0: up1, the coarsest) of {"heatmap_2d" | "det_d" | "root_d": HeadSource}: device pointer,
        source height and width, channels, and the pixel, channel and frame strides in floats.  The heads are fp32 NHWC with the padded
        channel stride the convs leave (48 | 16 | 8); the last stage's finest root-depth map of the tap-dot route is the NCHW block of
        the output buffer (never scaled).  Flip-TTA: 2B frames lie behind each pointer, the first B are the unmirrored ones."""
        if not self.all_heads:
            raise RuntimeError("head_sources() needs an engine built with all_heads=True")
        return graph_head_sources(self.graph, self.arena.data_ptr(), (self.out if out is None else out).data_ptr())

    def unit_out_sources(self):
        """keep_unit_out engines: {(stage, unit): the unit's `out` of the last run}, unit 0 = up1 (the coarsest), as views of the arena
        in the layouts smap_amd/heads.py reads: fp16 [B, h, w, 2, chl] hi|lo planes ("x3") or fp16 [B, h, w, chl] ("f16").  Flip-TTA: the
        first B (unmirrored) frames.  Views, not copies: the next run overwrites them."""
        if not self.keep_unit_out:
            raise RuntimeError("unit_out_sources() needs an engine built with all_heads=True, keep_unit_out=True")
        return self._unit_views(self.graph.unit_out)

    def unit_in_sources(self):
        """keep_unit_in engines: {(stage, unit): the unit's INPUT of the last run} -- x4 for unit 0 (up1) .. x1 for unit 3 -- as views of
        the arena in the layouts gemm_f32.x_descriptor reads, like unit_out_sources."""
        if not self.keep_unit_in:
            raise RuntimeError("unit_in_sources() needs an engine built with all_heads=True, keep_unit_in=True")
        return self._unit_views(self.graph.unit_in)

    def _unit_views(self, tensors):
        res = {}
        for key, t in tensors.items():
            assert t.esize == 2 and t.off >= 0
            raw = self.arena[t.off:t.off + t.nbytes].view(torch.float16)
            res[key] = (raw.view(t.B, t.H, t.W, 2, t.C) if t.planes == 2 else raw.view(t.B, t.H, t.W, t.C))[:self.B]
        return res

    def blob(self):
        """The whole schedule as one relocatable byte image (Graph.blob): what a host without this Python builder loads with
        smap_plan_create_from_blob.  Returns bytes."""
        return self.graph.blob()

    def capture(self, out=None):
        """Record the whole schedule (the ~208 launches of smap_plan_run) into a HIP graph.  Returns
        replay(imgs) -> (hms, det_d, root_d): copies `imgs` into the graph's static input buffer and launches the graph
        on the current stream -- one graph launch instead of ~208 kernel launches, which is what bounds small batches
        (B = 1: 2.9 ms per forward launch by launch).  Arena, weights and `out` are baked into the graph."""
        dev = self.device
        out_t = self.out if out is None else out
        static_in = torch.empty((self.B, 3, self.H, self.W), dtype=torch.float32, device=dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self.run(static_in, out=out_t)                 # warm-up outside the capture (module load, lazy init)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            self.run(static_in, out=out_t)
        views = (self.hms, self.det_d, self.root_d) if out is None else self.views(out_t)

        def replay(imgs):
            static_in.copy_(imgs, non_blocking=True)
            graph.replay()
            return views
        replay.graph, replay.static_in = graph, static_in      # keep them alive with the closure
        return replay

    def read_tensor(self, name):
        """Debug/test helper: NHWC activation `name` from the arena (valid with reuse=False)."""
        t = next(t for t in self.graph.tensors if t.name == name)
        dt = torch.float16 if t.esize == 2 else torch.float32
        raw = self.arena[t.off:t.off + t.nbytes].view(dt)
        if t.planes == 2:              # split precision: hi + lo as fp32
            raw = raw.view(t.B, t.H, t.W, 2, t.C).float()
            return raw[..., 0, :] + raw[..., 1, :]
        return raw.view(t.B, t.H, t.W, t.C)
