"""CPU tests of the host logic added in round 2: split-precision weight packing and schedule emission, the in-schedule
flip-TTA op list, tile tables, lazy result records, the end-to-end parity checker on synthetic inputs."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import make_cfg
from recipe import recipe_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def small_sd():
    from smap_amd.model.smap import SMAP
    torch.manual_seed(0)
    return recipe_state_dict(SMAP(make_cfg((16, 24))).state_dict())


def test_split_f16_reconstructs_to_22_bits():
    from smap_amd.engine import split_f16
    g = torch.Generator().manual_seed(0)
    w = torch.randn(64, 576, generator=g, dtype=torch.float64) * 0.03
    w[0, 0], w[0, 1] = 0.0, 1e-7                                   # vanishing weights survive too
    hi, lo, inv = split_f16(w)
    assert hi.dtype == lo.dtype == torch.float16 and torch.isfinite(hi).all() and torch.isfinite(lo).all()
    s = 1.0 / inv
    assert 2 ** 13 <= w.abs().max().item() * s < 2 ** 14 and float(np.log2(s)).is_integer()
    back = (hi.double() + lo.double()) * inv
    assert ((back - w).abs() <= w.abs() * 2.0 ** -21 + 2.0 ** -24 * inv).all()
    # plain fp16 is three orders of magnitude coarser on the same data
    assert (w.half().double() - w).abs().max() > 100 * (back - w).abs().max()
    z = split_f16(torch.zeros(4, 8, dtype=torch.float64))
    assert z[2] == 1.0 and not z[0].any() and not z[1].any()


@pytest.mark.parametrize("blocks", [False, True], ids=["layer_by_layer", "whole_blocks"])
def test_x3_graph_emits_split_strides_and_weights(small_sd, monkeypatch, blocks):
    from smap_amd.engine import Graph, OP_CONV, OP_HEADSUM, OP_MAXPOOL, OP_STEM, ZERO_PAGE, tile_ids
    if not blocks:                      # the layer-by-layer schedule: op for op the fp16 one (the default fuses layer1's Bottlenecks)
        monkeypatch.setenv("SMAP_BLOCK", "")
        monkeypatch.setenv("SMAP_BLOCK_FIRST", "")
    else:                               # (named explicitly: a schedule this small drops layer2's whole-block launches by default)
        monkeypatch.setenv("SMAP_BLOCK", "64:91,128:94")
    monkeypatch.setenv("SMAP_SPLITK", "0")          # (this test is about the split-precision STORAGE: no split-K scratch, no lanes, whose
    monkeypatch.setenv("SMAP_LANES", "0")           #  extended lifetimes would blur the arena comparison at the end)
    g16 = Graph(small_sd, 2, 64, 96)
    g = Graph(small_sd, 2, 64, 96, precision="x3")
    g.allocate()
    ops = g.emit()
    n_blk = sum(1 for op in g.ops if "head" in op.p)
    assert n_blk == (18 if blocks else 0)                 # 3 stages x (first block + two identity blocks of layer1 + three identity blocks of layer2)
    # (a first block is 3 launches layer by layer since round 6 -- c1, c2, c3 with the shortcut conv inside, Graph.conv_cat -- and 1 as a whole block)
    assert len(g.ops) == len(g16.ops) - (3 * 2 + 2 * 6 + 2 * 9 if blocks else 0) and g.flops == g16.flops
    ncat = lambda gr: sum(1 for op in gr.ops if "cat" in op.p and not op.p["cat"].get("relusum"))
    assert ncat(g) == (9 if blocks else 12) and ncat(g16) == 12
    # ... and the eight skip pairs of stages 0 / 1 (skip1 on the unit's input + skip2 on its output) are one launch, one tensor each (Graph.conv_relusum)
    assert sum(1 for op in g.ops if "cat" in op.p and op.p["cat"].get("relusum")) == 8 and not any(t.name.endswith((".skip1", ".skip2")) for t in g.tensors)
    assert not any(op.out is not None and op.out.name.endswith(".downsample") for op in g.ops)
    assert g.weight_blob().numel() > 1.9 * g16.weight_blob().numel()
    for op, o in zip(g.ops, ops):
        assert o.precision == 1
        if op.kind == OP_CONV:
            x, y = op.inp, op.out
            assert x.planes == 2 and o.in_stride_c == 2 * x.C and o.in_c_off + o.Cin <= x.C
            assert o.tile in tile_ids(("igemm", "halo", "persist", "block"), x3=True) and o.acc_scale > 0
            assert (y.planes, o.out_stride_c) == ((1, y.C) if o.out_fp32 else (2, 2 * y.C))
            assert o.in_off >= ZERO_PAGE and o.Cin * 2 + o.in_stride_c + 16 <= ZERO_PAGE
            for t in (op.res, op.add1, op.add2):
                assert t is None or t.planes == 2
        elif op.kind == OP_STEM:
            assert o.acc_scale > 0 and op.out.planes == 2
        elif op.kind == OP_MAXPOOL:
            assert op.inp.planes == op.out.planes == 2
        elif op.kind == OP_HEADSUM:
            assert all(t.esize == 4 and t.planes == 1 for t in op.aux)
    # arena: split tensors take twice the bytes (fewer of them are alive at once when layer1's intermediates stay on chip)
    g16.allocate()
    assert g.arena_bytes > (1.6 if blocks else 1.8) * g16.arena_bytes


def test_flip_graph_runs_two_B_frames_and_merges_in_the_head_sum(small_sd):
    from smap_amd.engine import Graph, OP_CONV, OP_HEADSUM, OP_STEM, OP_TAPSUM
    pair = list(range(43))[::-1]
    g = Graph(small_sd, 3, 64, 96, flip_pair=pair)
    g.allocate()
    ops = g.emit()
    assert g.B == 6 and g.frames == 3 and g.out_bytes == 3 * 58 * 16 * 24 * 4
    kinds = [op.kind for op in g.ops]
    stem = ops[kinds.index(OP_STEM)]
    assert stem.B == 6 and stem.flip_from == 3
    heads = [o for o in ops if o.kind in (OP_HEADSUM, OP_TAPSUM)]      # hms, det_d: head sums; root_d: the stencil half of its 3x3 (Graph.tapsum)
    assert [h.kind for h in heads] == [OP_HEADSUM, OP_HEADSUM, OP_TAPSUM]
    assert [h.B for h in heads] == [3, 3, 3] and [h.flip_from for h in heads] == [3, 0, 0]
    assert heads[0].in_c_off == 15 and heads[0].w_off >= 0
    blob = g.weight_blob()
    tab = blob[heads[0].w_off:heads[0].w_off + 43 * 4].view(torch.int32).tolist()
    assert tab == pair
    convs = {op.out.name: o for op, o in zip(g.ops, ops) if op.kind == OP_CONV}
    depth = [n for n in convs if n.endswith(".res_d") or n.endswith(".res_rd_t")]
    assert len(depth) == 2 and all(convs[n].B == 3 for n in depth)          # mirrored half of the depth heads: never read
    assert all(o.B == 6 for n, o in convs.items() if n not in depth)
    with pytest.raises(AssertionError):
        Graph(small_sd, 3, 64, 96, flip_pair=[0, 1, 2])


def test_shipped_launcher_settings_are_plannable():
    """exps/stage3_root2/test.sh runs --batch_size 16 --do_flip 1 in the default split precision: 32 frames of activations, a
    5.6 GiB arena.  Until round 3 the conv kernels addressed the whole arena with 32-bit offsets (4 GiB) and the batch ran as
    2 x 8; now a launch addresses its input from the input's 4 GiB WINDOW, the arena reserves a zero page at the start of every
    window, and the shipped setting plans as ONE schedule.  The limit that remains is one tensor per window (64 frames of
    the 768-channel head tensor do not fit), and the graph says so in words."""
    from types import SimpleNamespace as NS
    from smap_amd.engine import ArenaTooLarge, Graph, WINDOW, ZERO_PAGE, OP_CONV
    from smap_amd.model.smap import SMAP
    sh = open(os.path.join(ROOT, "exps", "stage3_root2", "test.sh")).read()
    assert "--batch_size 16" in sh and "--do_flip 1" in sh
    cfg = NS(MODEL=NS(STAGE_NUM=3, UPSAMPLE_CHANNEL_NUM=256), DATASET=NS(KEYPOINT=NS(NUM=15), PAF=NS(NUM=14)),
             OUTPUT_SHAPE=(128, 208), LOSS=NS(OHKM=True, TOPK=8, COARSE_TO_FINE=True))
    torch.manual_seed(0)
    sd = SMAP(cfg).state_dict()
    g = Graph(sd, 16, 512, 832, precision="x3", flip_pair=list(range(43)))
    assert g.allocate() > (1 << 32)                                         # beyond what 32-bit arena offsets could address
    windows = set()
    for t in g.tensors:                                                     # no tensor on a zero page, none across a window boundary
        assert t.off % WINDOW >= ZERO_PAGE and t.off // WINDOW == (t.off + t.nbytes - 1) // WINDOW, t.name
    for op, o in zip(g.ops, g.emit()):
        if op.kind == OP_CONV:
            windows.add(o.in_off // WINDOW)
            assert o.in_off % WINDOW + op.inp.nbytes <= (1 << 32)
    assert len(windows) >= 2, "the test must exercise a launch whose input lies beyond the first window"
    live = sorted((t.first, t.last, t.off, t.off + t.nbytes) for t in g.tensors)
    for i, a in enumerate(live):                                            # live ranges never share bytes
        for b in live[i + 1:]:
            if b[0] > a[1]:
                break
            assert a[3] <= b[2] or b[3] <= a[2] or a[1] < b[0]
    # the LIBRARY agrees with the allocator's idea of windows and zero pages (smap_plan_create runs without a GPU): a library
    # built with another window size than engine.WINDOW refuses these ops -- round 4 lost a GPU visit to exactly that
    import ctypes as C
    from smap_amd import lib as L
    h = C.c_void_p()
    assert L.load().smap_plan_create(g.emit(), len(g.ops), C.byref(h)) == 0
    L.load().smap_plan_destroy(h)
    # (the widest tensor is the 512-channel head tensor since round 6 -- the root-depth head no longer stores its 256 channels --: 78 frames per window)
    Graph(sd, 32, 512, 832, precision="x3", flip_pair=list(range(43))).allocate()
    with pytest.raises(ArenaTooLarge, match="smaller batch"):
        Graph(sd, 40, 512, 832, precision="x3", flip_pair=list(range(43))).allocate()
    with pytest.raises(ValueError):
        Graph(sd, 1, 64, 96, flip_pair=[0] * 43)             # not a permutation


def test_tile_tables_name_existing_tiles():
    from smap_amd.engine import TILES, _table_entry, tile_family, tile_has, tile_ids
    t16 = json.load(open(os.path.join(ROOT, "smap_amd", "tile_table.json")))
    tx3 = json.load(open(os.path.join(ROOT, "smap_amd", "tile_table_x3.json")))
    assert t16 and all(t in TILES for v in t16.values() for t in _table_entry(v))
    assert tx3 and all(t in tile_ids(("igemm", "halo", "persist"), x3=True) for v in tx3.values() for t in _table_entry(v))
    for key, v in tx3.items():
        f = key.split(",")                                                   # optional 8th field: "up" (ops with a fused bilinear add)
        merged = "+" in f[4]                                                 # "c0+c1[+c2]": a merged 1x1 launch (Graph.conv_seg, tools/autotune_seg.py)
        B, H, W, cin, k, s = map(int, f[:4] + f[5:7])
        cout = sum(map(int, f[4].split("+")))
        assert f[7:] in ([], ["up"])
        assert not merged or (k == 1 and s == 1 and all(tile_family(t) == "igemm" for t in _table_entry(v)))
        for t in _table_entry(v):
            assert B in (1, 8, 16) and (tile_family(t) != "halo" or (k == 3 and s == 1))   # (1 = configs[1], 16 = the flip-TTA schedule of batch 8); halo tiles: plain 3x3 stride 1 only
            assert cout > 32 or (TILES[t][1] == 32 and tile_has(t, None, True))      # the Cout <= 32 tiles: 3, 38, 39
        assert tile_family(_table_entry(v)[-1]) != "persist"                         # a ranked list ends on a tile that takes every op


def test_tile_geometry_tables_agree_with_the_library():
    """engine.py packs the weight blob per tile (BN rows x BK halves blocks); the kernels' template arguments (csrc/tiles.h) are the truth."""
    import ctypes as C
    from smap_amd import lib as L
    from smap_amd.engine import TILES, tile_bk
    lib = L.load()
    from smap_amd.engine import TAIL_BN
    for t in range(0, 100):
        assert lib.smap_conv_tile_tail_bn(t) == TAIL_BN.get(t, 0), t
        bm, bn = C.c_int(), C.c_int()
        rc = lib.smap_conv_tile_dims(t, C.byref(bm), C.byref(bn))
        assert (rc == 0) == (t in TILES), t
        if rc == 0:
            assert (bm.value, bn.value) == TILES[t], t
            for prec in (0, 1):
                assert lib.smap_conv_tile_bk(t, prec) == tile_bk(t, bool(prec)), (t, prec)
        else:
            assert lib.smap_conv_tile_bk(t, 0) == 0


def _capability_probe(tile, x3, variant):
    """The smallest CONV op that csrc/plan_check.cpp::validate can only refuse for what tile id `tile` is: laid out from the PYTHON table's row
    (unknown ids: as a 1x1 on a 128 x 64 tile), 1 frame of 8 x 8 pixels, every tensor a MiB apart inside the first window.
    variant: "plain", "fp32out", "splitk" (ksplit = 2), "dual" (in2_C), "relusum" (in2_mode = 1), "segments" (two N segments), "tapdot"."""
    from smap_amd import lib as L
    from smap_amd.engine import TILE_TABLE, Tile
    row = TILE_TABLE.get(tile, Tile("igemm", 128, 64, 64, 64))
    MiB, pl = 1 << 20, 2 if x3 else 1
    o = L.SmapOp()
    o.kind, o.B, o.H, o.W, o.Ho, o.Wo, o.tile, o.precision, o.acc_scale, o.relu = 0, 1, 8, 8, 8, 8, tile, int(x3), 1.0, 1
    o.in_off, o.out_off, o.w_off, o.bias_off, o.res_off, o.add1_off, o.add2_off, o.ext_off = 1 * MiB, 2 * MiB, 0, 0, -1, -1, -1, -1
    for i in range(3):
        o.aux_off[i] = -1
    if row.family in ("igemm", "persist"):                 # a 1x1, 256 -> 256 channels (every N extent divides 256; four K tiles of 64 halves)
        o.ksize, o.stride, o.pad, o.Cin, o.Cout, o.cout_pad = 1, 1, 0, 256, 256, 256
    else:                                                  # a plain 3x3 on 64 channels, one N tile
        o.ksize, o.stride, o.pad, o.Cin, o.Cout, o.cout_pad = 3, 1, 1, max(64, row.planes), row.bn, row.bn
    o.in_stride_c, o.out_stride_c = o.Cin * pl, o.Cout * pl
    if row.tail_bn:                                        # "tail" / "block": the fused 1x1 behind the 3x3, 4 x its planes
        o.tail_cout = o.tail_cout_pad = 4 * row.bn
        o.tail_w_off, o.tail_bias_off, o.tail_acc_scale, o.out_stride_c = 0, 0, 1.0, 4 * row.bn * pl
    if row.family == "block":                              # (split precision only: the layout is the split one in both probes)
        o.head_cin = row.planes if row.first else 4 * row.planes
        o.in_stride_c, o.out_stride_c, o.head_w_off, o.head_bias_off, o.head_acc_scale = 2 * o.head_cin, 8 * row.planes, 0, 0, 1.0
        if row.first:
            o.short_w_off, o.short_acc_scale = 0, 1.0
        else:
            o.res_off = o.in_off
    if variant == "fp32out":
        o.out_fp32, o.out_stride_c = 1, o.out_stride_c // pl
    elif variant == "splitk":
        o.ksplit, o.kpart_off, o.kcount_off = 2, 32 * MiB, 48 * MiB
    elif variant in ("dual", "relusum"):
        o.in2_C, o.in2_stride, o.in2_H, o.in2_W, o.in2_stride_c, o.in2_off = 64, 1, 8, 8, 64 * pl, 3 * MiB
        if variant == "relusum":
            o.in2_mode, o.relu, o.in2_bias_off, o.in2_acc_scale = 1, 0, 0, 1.0
    elif variant == "segments":                            # two N tiles, one segment each
        o.Cout, o.cout_pad, o.out_stride_c = row.bn, 2 * row.bn, row.bn * pl
        o.seg_n[0], o.seg_cout[0], o.seg_out_stride_c[0], o.seg_acc_scale[0], o.seg_out_off[0] = row.bn, row.bn, row.bn * pl, 1.0, 4 * MiB
    elif variant == "tapdot":
        o.tap_n, o.out_fp32, o.out_stride_c, o.tap_w_off, o.tap_scale = 9, 1, 16, 0, 1.0
    else:
        assert variant == "plain"
    return o


def test_tile_capabilities_agree_with_what_the_plan_accepts():
    """The facts of a tile id that no ABI function exports -- which precisions it has an instance in, its kernel family, split K, second
    input, relu-sum, register epilogue, tap-dot, the planes / first-block flag of a whole-block tile -- compared through
    csrc/plan_check.cpp::validate: for every id 0..99 and both precisions, smap_plan_create accepts a minimal op that needs the fact exactly
    when the Python table (smap_amd/engine.py TILE_TABLE) says the id has it.  Plan creation touches no GPU."""
    import ctypes as C
    from smap_amd import lib as L
    from smap_amd.engine import TILE_TABLE, tile_family, tile_has
    lib = L.load()
    want = {"plain": lambda t, x3: True,
            "fp32out": lambda t, x3: tile_family(t) in ("igemm", "halo") and not tile_has(t, "regepi", x3),
            "splitk": lambda t, x3: tile_has(t, "splitk", x3),
            "dual": lambda t, x3: tile_has(t, "dual", x3),
            "relusum": lambda t, x3: tile_has(t, "relusum", x3),
            "segments": lambda t, x3: tile_family(t) == "igemm",
            "tapdot": lambda t, x3: tile_has(t, "tapdot", x3)}
    accepted = 0
    for t in range(100):
        for x3 in (False, True):
            for variant, rule in want.items():
                o, h = _capability_probe(t, x3, variant), C.c_void_p()
                rc = lib.smap_plan_create(C.byref(o), 1, C.byref(h))
                if rc == 0:
                    lib.smap_plan_destroy(h)
                assert (rc == 0) == (tile_has(t, None, x3) and rule(t, x3)), (t, "x3" if x3 else "f16", variant, rc)
                accepted += rc == 0
    assert accepted > 2 * len(TILE_TABLE)                  # (the probes are legal ops: most ids take the plain one in both precisions)


def test_weight_packing_is_a_permutation_and_inverts():
    from smap_amd.engine import TILES, pack_conv_weights, unpack_conv_weights
    for tile, x3, k, cin, cout_pad in ((0, False, 3, 128, 256), (20, True, 1, 64, 128), (31, True, 3, 64, 256), (36, False, 3, 64, 64),
                                       (52, True, 1, 128, 256), (60, True, 3, 64, 512), (3, True, 3, 64, 32)):
        planes, K = (2 if x3 else 1), k * k * cin
        w = torch.randn(planes, cout_pad, K).half()
        p = pack_conv_weights(w, tile, x3, k, cin)
        assert p.numel() == w.numel() and torch.equal(p.reshape(-1).sort().values, w.reshape(-1).sort().values)
        assert torch.equal(unpack_conv_weights(p.reshape(-1), tile, x3, k, cin, cout_pad), w)


def test_weight_packing_matches_the_kernels_address_arithmetic():
    """pack_conv_weights against the byte addresses the kernels compute (csrc/conv.hip issue_b, conv3.hip, convp.hip): element
    (plane, n, k) must sit where lane (row, slot) of the LDS-DMA that stages its K tile reads it."""
    import random
    from smap_amd.engine import TILES, pack_conv_weights, tile_bk, tile_family
    random.seed(0)
    for tile, x3, ks, cin, cout_pad in ((0, False, 3, 128, 256), (0, True, 1, 256, 256), (20, True, 3, 64, 128), (22, True, 1, 256, 256),
                                        (52, True, 1, 128, 256), (31, True, 3, 128, 256), (31, False, 3, 128, 256), (36, True, 3, 64, 64),
                                        (38, False, 3, 256, 32), (60, True, 1, 64, 512), (62, False, 3, 64, 256), (64, True, 1, 128, 64)):
        planes, K, bn = (2 if x3 else 1), ks * ks * cin, TILES[tile][1]
        w2 = torch.arange(planes * cout_pad * K, dtype=torch.float32).reshape(planes, cout_pad, K)
        for pairs in (True, False):
          P = pack_conv_weights(w2, tile, x3, ks, cin, pairs=pairs).reshape(-1)
          for _ in range(300):
              n = random.randrange(cout_pad)
              nt, r = n // bn, n % bn
              if tile_family(tile) == "halo":
                  ch = 32 if x3 else 64
                  cch = cin // ch
                  cc, tap, s, e = random.randrange(cch), random.randrange(9), random.randrange(8), random.randrange(8)
                  gl = s ^ ((r >> 1) & 7)
                  pl, g = ((gl >> 2), (gl & 3)) if x3 else (0, gl)
                  k = tap * cin + cc * ch + g * 8 + e
                  off = ((((nt * cch + cc) * 9 + tap) * bn + r) * 8 + s) * 8 + e
              else:
                  bk = tile_bk(tile, x3)
                  spr, KT = bk // 8, K // bk
                  it, pl, s, e = random.randrange(KT), random.randrange(planes), random.randrange(spr), random.randrange(8)
                  g = s ^ (((r >> 1) & 7) if bk == 64 else ((r >> 2) & 3))
                  k = it * bk + g * 8 + e
                  if bk == 64 or not pairs:        # byte = (nt*KT + it)*WBLK + (pl*BN + r)*ROWB + s*16
                      off = ((((nt * KT + it) * planes + pl) * bn + r) * spr + s) * 8 + e
                  else:               # pairs: byte = (nt*KT/2 + it/2)*WBLK + (it&1)*64 + (pl*BN + r)*128 + s*16
                      off = (((((nt * (KT // 2) + it // 2) * planes + pl) * bn + r) * 2 + (it & 1)) * 4 + s) * 8 + e
              assert P[off] == w2[pl, n, k], (tile, x3, off)


def test_fused_bottleneck_tail_schedule_on_cpu(small_sd, monkeypatch):
    """SMAP_TAIL routes stride-1 Bottlenecks to the one-launch 3x3 + 1x1 op (csrc/convf.hip): the op list shrinks by one launch
    per such block, the torch interpretation of the fused schedule equals the unfused one bit for bit in both its modes (the
    quantised mode reads the weights back out of the packed blob: the 1x1's chunk blocks invert), the plan accepts the ops
    and rejects inconsistent ones."""
    import ctypes as C
    from oracle.graph_interp import run_graph
    from smap_amd import lib as L
    from smap_amd.engine import Graph, OP_CONV, TAIL_BN, pack_halo_rows, unpack_halo_rows
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(3))
    monkeypatch.setenv("SMAP_CAT", "0")                  # (this test compares ROUNDINGS op for op: the shortcut tensors stay stored on both sides)
    g0 = Graph(small_sd, 2, 64, 96, keep_ref=True)
    want, want_q = run_graph(g0, x.double(), quantize=False), run_graph(g0, x, quantize=True)
    monkeypatch.setenv("SMAP_TAIL", "64:80,128:82")
    monkeypatch.setenv("SMAP_BLOCK", "")                 # (the whole-block launches would take layer1's blocks in split precision)
    monkeypatch.setenv("SMAP_BLOCK_FIRST", "")
    for prec in ("f16", "x3"):
        g = Graph(small_sd, 2, 64, 96, keep_ref=True, precision=prec)
        tails = [op for op in g.ops if op.kind == OP_CONV and "tail" in op.p]
        assert len(tails) == 18 and len(g.ops) == len(g0.ops) - 18            # layer1: 3 blocks, layer2: 3 stride-1 blocks, x 3 stages
        assert all(op.res is not None and op.p["Cout"] * 4 == op.p["tail"]["cout"] for op in tails)
        assert all(torch.equal(a, b) for a, b in zip(run_graph(g, x.double(), quantize=False), want))
        if prec == "f16":
            assert all(torch.equal(a, b) for a, b in zip(run_graph(g, x, quantize=True), want_q))
        g.allocate()
        ops = g.emit()
        h = C.c_void_p()
        assert L.load().smap_plan_create(ops, len(g.ops), C.byref(h)) == 0
        L.load().smap_plan_destroy(h)
        i = next(k for k, op in enumerate(g.ops) if op.kind == OP_CONV and "tail" in op.p)
        for field, bad in (("tail_cout", 0), ("tail_cout", 100), ("tail_cout_pad", 32), ("stride", 2), ("tile", 36), ("tail_w_off", -1)):
            keep = getattr(ops[i], field)
            setattr(ops[i], field, bad)
            assert L.load().smap_plan_create(ops, len(g.ops), C.byref(h)) != 0, field
            setattr(ops[i], field, keep)
    for x3 in (False, True):
        w = torch.randn(2 if x3 else 1, 256, 64).half()
        p = pack_halo_rows(w, TAIL_BN[80], 1, 64, x3)
        assert p.shape[:3] == (4, 2 if x3 else 1, 1) and torch.equal(unpack_halo_rows(p.reshape(-1), 64, 1, 64, 256, x3), w)


def test_lazy_records_equal_eager_records():
    from smap_amd.records import frame_record, to_jsonable, train_records
    rng = np.random.default_rng(0)
    p2, p3, rz = rng.normal(size=(3, 15, 4)).astype(np.float32), rng.normal(size=(3, 15, 4)), rng.normal(size=3)
    gt = rng.normal(size=(3, 15, 11))
    for g in (None, gt):
        eager = frame_record(p2, p3, rz, "a.jpg", g)
        lazy = frame_record(p2, p3, rz, "a.jpg", g, as_lists=False)
        p2_before = p2.copy()
        assert isinstance(lazy["pred_2d"], np.ndarray) and lazy["pred_2d"] is not p2
        assert to_jsonable([lazy]) == [eager] and json.dumps(to_jsonable([lazy])) == json.dumps([eager])
        assert np.array_equal(p2, p2_before)
    assert to_jsonable(train_records(p2, p3, rz, gt, as_lists=False)) == train_records(p2, p3, rz, gt)


def test_parity_compare_counts_what_it_says():
    from benchkit import parity

    def frame(shift=0.0, drop_person=False, z_err=0.0):
        peaks = np.zeros((15, 128, 3), np.float32)
        for c in range(15):
            peaks[c, 0, 0] = 4
            peaks[c, 1:5, :2] = np.array([[10, 10], [50, 20], [90, 60], [150, 100]]) + c + shift
            peaks[c, 1:5, 2] = 0.9
        bodys = np.zeros((2, 15, 4), np.float32)
        bodys[:, :, :2] = np.arange(60).reshape(2, 15, 2) + shift
        bodys[:, :, 3] = 1.0
        p3 = np.zeros((2, 15, 4))
        p3[:, :, :3] = np.arange(90).reshape(2, 15, 3) + z_err
        p3[:, :, 3] = 1.0
        n = 1 if drop_person else 2
        maps = {k: np.ones((2, 4, 4), np.float32) for k in ("hms", "det_d", "root_d")}
        return dict(peaks=peaks, bodys=bodys[:n], p2=bodys[:n] * 4, p3=p3[:n], rz=np.array([300.0, 310.0])[:n] + z_err, **maps)

    same = parity.compare([frame()], [frame()])
    assert same["peak_match"] == same["person_match"] == same["limb_match"] == 1.0 and same["max_joint_err_cm"] == 0.0
    assert same["peaks_differing"] == 0 and same["peaks_clear_mismatch"] == 0
    assert same["peaks_ref"] == 60 and same["persons_ref"] == 2 and same["joints_compared"] == 30
    sub = parity.compare([frame(shift=0.2, z_err=0.05)], [frame()])           # sub-pixel shift: still the same peaks
    assert sub["peak_match"] == 1.0 and sub["limb_match"] == 1.0
    assert abs(sub["max_joint_err_cm"] - 0.05 * 3 ** 0.5) < 1e-9 and abs(sub["root_z_max_err_cm"] - 0.05) < 1e-9
    moved = parity.compare([frame(shift=1.0)], [frame()])                     # one pixel away: different peaks
    assert moved["peak_match"] < 0.5 and moved["person_match"] == 0.0
    lost = parity.compare([frame(drop_person=True)], [frame()])
    assert lost["person_match"] == 0.5 and lost["peak_match"] == 1.0


def test_lifter_ties_are_told_from_real_joint_errors():
    """generate_relZ samples the depth maps at ROUNDED positions (test_util.py:66,74-79): a coordinate 1e-6 px from an index
    step puts one sample on the neighbouring depth pixel -- a joint error of centimetres from a 1e-6 px input difference.
    benchkit/parity.py must call that a lifter tie, and must NOT excuse the same error when the coordinates differ by more."""
    from benchkit import parity
    from oracle import oracle_lib as O
    rng = np.random.default_rng(3)
    H, W = 32, 48
    det_d = rng.normal(0, 30, (14, H, W)).astype(np.float32)          # rough depth maps: a moved sample is visible
    root_d = rng.uniform(0.5, 1.0, (H, W)).astype(np.float32)
    cam = np.asarray([1.0, 4 * W, 4 * H, 4 * W, 4 * H, 1000.0, 1000.0, 2 * W, 2 * H], np.float64)
    body = np.zeros((1, 15, 4), np.float32)
    body[0, :, 0] = rng.uniform(8, W - 8, 15)
    body[0, :, 1] = rng.uniform(8, H - 8, 15)
    body[0, :, 3] = 1.0
    body[0, 0, :2] = (20.25, 10.25)                                   # pelvis and neck well inside a depth pixel
    body[0, 2, :2] = (24.25, 14.25)

    def frame(bd):
        p2, p3, rz = O.lift(bd, det_d, root_d, cam)
        peaks = np.zeros((15, 128, 3), np.float32)
        return dict(peaks=peaks, bodys=bd, p2=p2, p3=p3, rz=rz, det_d=det_d, root_d=root_d, hms=np.ones((43, H, W), np.float32))

    # limb 8 = (2, 12): put joint 12 so that its x4 coordinate sits on the step between two depth pixels: round(x) = 4m - 0.5
    step = np.float32((4 * 30 - 0.5) / 4)                             # x4 -> 119.5 exactly: np.round goes to 120 (even) = pixel 30
    a, b = body.copy(), body.copy()
    a[0, 12, 0] = step
    b[0, 12, 0] = np.nextafter(step, np.float32(0))                   # one ulp below: rounds to 119 = pixel 29
    assert parity.lift_sample_pixels(a[0])[2][8][0][-1, 1] != parity.lift_sample_pixels(b[0])[2][8][0][-1, 1]
    m = parity.compare([frame(a)], [frame(b)])
    assert m["person_match"] == 1.0 and m["limb_match"] == 1.0
    assert m["max_joint_err_cm"] > 0.1, "the moved sample must matter in this scene"
    assert m["joints_over_0.1cm_unexplained"] == 0 and m["lifter_ties"] >= 1, m
    assert m["lifter_tie_max_coord_diff_px"] < 5e-4
    # the same sample moved by a coordinate that differs by 0.2 px (still 'the same peak' for the 0.5 px pairing): not a tie
    c = body.copy()
    c[0, 12, 0] = step - np.float32(0.05)                              # 0.2 network px away: far beyond LIFT_TIE_PX
    m2 = parity.compare([frame(a)], [frame(c)])
    assert m2["limb_match"] == 1.0 and m2["max_joint_err_cm"] > 0.1
    assert m2["joints_over_0.1cm_unexplained"] >= 1 and m2["lifter_ties"] == 0, m2


def test_peak_ties_are_told_from_real_mismatches():
    """A candidate that clears the threshold by 1e-7 of the map scale in one path and misses it in the other is a floating-
    point tie; one that differs by 1e-2 is a mismatch."""
    from benchkit import parity
    rng = np.random.default_rng(5)
    base = rng.uniform(0.0, 0.1, (43, 32, 48)).astype(np.float32)
    base[3, 10, 20], base[7, 20, 30] = 0.9, 0.5                     # two clear peaks (scale = 0.9)

    def frame(hms):
        peaks = np.zeros((15, 128, 3), np.float32)
        return dict(peaks=peaks, bodys=np.zeros((0, 15, 4), np.float32), p2=np.zeros((0, 15, 4)), p3=np.zeros((0, 15, 4)),
                    rz=np.zeros((0,)), hms=hms, det_d=np.ones((1, 2, 2), np.float32), root_d=np.ones((2, 2), np.float32))

    assert parity.peak_pixels(base[:15]) == {(3, 10, 20), (7, 20, 30)}
    tie_ref, tie_hip = base.copy(), base.copy()
    tie_ref[5, 8, 8], tie_hip[5, 8, 8] = 0.2 + 2e-7, 0.2 - 2e-7      # just above / just below the 0.2 threshold
    m = parity.compare([frame(tie_hip)], [frame(tie_ref)])
    assert m["peaks_differing"] == 1 and m["peaks_clear_mismatch"] == 0 and m["peaks_differing_max_margin"] < 1e-6
    bad_hip = base.copy()
    bad_hip[7, 20, 30] = 0.1                                          # a clear peak lost
    m = parity.compare([frame(bad_hip)], [frame(base)])
    assert m["peaks_differing"] == 1 and m["peaks_clear_mismatch"] == 1 and m["peaks_differing_max_margin"] > 0.1
    # more than 127 candidates in a channel: a tie near the top of the raster also moves the cap at its end -- one decision
    # differs (the tie), one perfectly clear peak is swapped in / out as a CONSEQUENCE (counted apart, not a mismatch)
    crowd = base.copy()
    ys, xs = np.meshgrid(np.arange(4, 30, 2), np.arange(2, 46, 2), indexing="ij")
    crowd[9, ys.ravel()[:130], xs.ravel()[:130]] = 0.9                 # 130 isolated clear peaks in channel 9 (rows 4..)
    c_ref, c_hip = crowd.copy(), crowd.copy()
    c_ref[9, 1, 8], c_hip[9, 1, 8] = 0.2 + 2e-7, 0.2 - 2e-7           # a tie above them all in raster order
    m = parity.compare([frame(c_hip)], [frame(c_ref)])
    assert m["peaks_differing"] == 1 and m["peaks_clear_mismatch"] == 0 and m["peaks_cap_shifted"] == 1


def test_people_weights_are_calibrated_data_not_weights():
    from benchkit.workload import HEAD_KINDS, people_state_dict
    cal = json.load(open(os.path.join(ROOT, "benchkit", "head_calibration.json")))
    assert set(cal) == set(HEAD_KINDS) and all(len(cal[k]["kpt_bias"]) == 15 for k in cal)
    from smap_amd.model.smap import SMAP
    torch.manual_seed(0)
    base = SMAP(make_cfg((16, 24))).state_dict()
    a, b = recipe_state_dict(base), people_state_dict(base, "smooth")
    changed = sorted(k for k in a if not torch.equal(a[k], b[k]))
    assert changed == ["stage2.upsample.up4.res_conv2.bn.bias", "stage2.upsample.up4.res_conv2.bn.weight",
                       "stage2.upsample.up4.res_rd_conv2.bn.bias", "stage2.upsample.up4.res_rd_conv2.bn.weight"]


# ------------------------------------------------------------------ round 5: merged launches, split K, small-schedule rules, lanes
def _full_size_sd():
    from types import SimpleNamespace as NS
    from smap_amd.model.smap import SMAP
    cfg = NS(MODEL=NS(STAGE_NUM=3, UPSAMPLE_CHANNEL_NUM=256), DATASET=NS(KEYPOINT=NS(NUM=15), PAF=NS(NUM=14)),
             OUTPUT_SHAPE=(128, 208), LOSS=NS(OHKM=True, TOPK=8, COARSE_TO_FINE=True))
    torch.manual_seed(0)
    return SMAP(cfg).state_dict()


def test_batch_1_schedule_rules_and_arena(monkeypatch):
    """What the batch-1 schedule (BASELINE configs[1]) is made of, without a GPU: split K only on the long-K launches of the coarse
    levels (K >= 2048, <= 4 parts, workgroups x parts <= 256 there), the four-stage 64x64 tile exactly on the launches of <= 256
    workgroups, layer1's whole blocks on 4x16 tiles, layer2's as three launches; every split op has its own scratch and ticket slice,
    scratch and tickets never share bytes with a live tensor; the library accepts the plan; with lanes on, every wait names an earlier
    op of another lane and nothing a side-lane op touches is reused before the end of the schedule."""
    import ctypes as C
    from smap_amd import lib as L
    from smap_amd.engine import Graph, OP_CONV, TILES, tile_bk, tile_family
    sd = _full_size_sd()
    for k in ("SMAP_CAT", "SMAP_SKIPSUM", "SMAP_TAPHEAD"):          # (conftest forces round 6's launches on for the small TEST schedules; this is the real batch-1 rule)
        monkeypatch.delenv(k, raising=False)
    for lanes in ("0", "1"):
        monkeypatch.setenv("SMAP_LANES", lanes)
        g = Graph(sd, 1, 512, 832, precision="x3")
        g.allocate()
        ops = g.emit()
        convs = [(op, o) for op, o in zip(g.ops, ops) if op.kind == OP_CONV]
        assert sorted({op.p["tile"] for op, _ in convs if tile_family(op.p["tile"]) in ("tail", "block")}) == [90, 92]              # layer1: 4 x 16 tiles; no tile 94
        split = [(op, o) for op, o in convs if o.ksplit > 1]
        assert 30 <= len(split) <= 40
        tickets = set()
        for op, o in split:
            K = o.ksize * o.ksize * o.Cin
            bm, bn = TILES[o.tile]
            tiles = -(-(o.B * o.Ho * o.Wo) // bm) * (o.cout_pad // bn)
            assert K >= 2048 and 2 <= o.ksplit <= 4 and tiles * o.ksplit <= 256 and o.ksplit <= K // tile_bk(o.tile, True)
            assert o.kpart_off == op.scratch[0].off and op.scratch[0].nbytes == tiles * o.ksplit * bm * bn * 4
            lo = o.kcount_off
            assert g.kcount.off <= lo and lo + 4 * tiles <= g.kcount.off + g.kcount.nbytes
            assert not tickets & set(range(lo, lo + 4 * tiles, 4))
            tickets |= set(range(lo, lo + 4 * tiles, 4))
        for op, o in convs:                                        # the deep-pipeline rule
            if o.tile in (2, 7):
                wgs = -(-(o.B * o.Ho * o.Wo) // 64) * (o.cout_pad // 64) * max(1, o.ksplit)
                assert (o.tile == 7) == (wgs <= 256), (op.out.name, wgs)
        every = g.tensors + g.scratch_tensors + [g.kcount]
        live = sorted((t.first, t.last, t.off, t.off + t.nbytes, t.name) for t in every)
        for i, a in enumerate(live):
            for b in live[i + 1:]:
                if b[0] > a[1]:
                    break
                assert a[3] <= b[2] or b[3] <= a[2], (a[4], b[4])
        n = len(g.ops)
        if lanes == "1":
            assert sorted({op.lane for op in g.ops}) == [0, 1, 2]
            for i, (op, o) in enumerate(zip(g.ops, ops)):
                for k in range(o.n_wait):
                    assert 0 <= o.wait_op[k] < i and ops[o.wait_op[k]].lane != o.lane
                if op.lane:
                    for t in [op.inp, op.res, op.add1, op.add2] + list(op.aux):
                        assert t is None or t.last == n - 1
        else:
            assert all(o.lane == 0 and o.n_wait == 0 for o in ops)
        h = C.c_void_p()
        assert L.load().smap_plan_create(ops, n, C.byref(h)) == 0
        rc = L.load().smap_plan_set_lanes(h, int(lanes))          # lanes on: creates the side streams IN this call (include/smap_hip.h) --
        assert rc == 0 or (lanes == "1" and not torch.cuda.is_available() and rc <= -1000), rc     # a hipError_t on a host without a GPU
        if rc == 0:
            assert L.load().smap_plan_set_lanes(h, 0) == 0
        L.load().smap_plan_destroy(h)


def test_merged_launch_descriptors_and_validation(small_sd, monkeypatch):
    """Graph.conv_seg -> smap_op.seg_*: segment starts are multiples of the tile's N extent and in order, every segment has its own
    output tensor / scale, the plan validates -- and refuses a segment that is mis-aligned, overlaps the next one, or sits on a tile
    family without the per-segment epilogue."""
    import ctypes as C
    from smap_amd import lib as L
    from smap_amd.engine import Graph, OP_CONV, TILES
    monkeypatch.setenv("SMAP_SKIPSUM", "0")              # (the skip convs as segments: with the default skip1 + skip2 launches only stage 2's two merged launches remain)
    for merge, n in (("2", 18), ("1", 12), ("0", 0)):
        monkeypatch.setenv("SMAP_MERGE_1X1", merge)
        g = Graph(small_sd, 2, 64, 96, precision="x3")
        g.allocate()
        ops = g.emit()
        segd = [(op, o) for op, o in zip(g.ops, ops) if op.kind == OP_CONV and o.seg_n[0] > 0]
        assert len(segd) == n
        for op, o in segd:
            bn = TILES[o.tile][1]
            starts = [s for s in o.seg_n if s > 0]
            assert starts == sorted(starts) and all(s % bn == 0 for s in starts) and o.Cout <= starts[0] and o.ksize == 1
            for j, t in enumerate(op.outs):
                assert o.seg_out_off[j] == t.off and o.seg_cout[j] == t.C and o.seg_out_stride_c[j] == 2 * t.C and o.seg_acc_scale[j] > 0
            assert len({op.out.off} | {t.off for t in op.outs}) == 1 + len(op.outs)
        h = C.c_void_p()
        assert L.load().smap_plan_create(ops, len(g.ops), C.byref(h)) == 0
        L.load().smap_plan_destroy(h)
        if segd:
            i = next(k for k, op in enumerate(g.ops) if op.outs)
            for field, val in (("seg_n", ops[i].seg_n[0] + 8), ("seg_cout", ops[i].seg_cout[0] + 4), ("tile", 60), ("ksize", 3)):
                bad = (L.SmapOp * len(g.ops))()
                C.memmove(bad, ops, C.sizeof(bad))
                if field in ("seg_n", "seg_cout"):
                    getattr(bad[i], field)[0] = val
                else:
                    setattr(bad[i], field, val)
                assert L.load().smap_plan_create(bad, len(g.ops), C.byref(h)) != 0, field


# -- launch inventory: every conv launch the shipped schedules run has a unit case in tests/test_backbone_gpu.py --------------------------

SHIPPED_SCHEDULES = [   # frames, precision, flip-TTA: BASELINE configs[1] (batch 1), one 8-frame step, the 16-frame launch bench.py times
    (1, "x3", False), (8, "x3", False), (16, "x3", False), (1, "f16", False), (8, "f16", False), (16, "f16", False),
    (8, "x3", True),                                   # 8-frame steps with flip-TTA (16 frames per launch)
    (16, "x3", True),                                  # exps/stage3_root2/test.sh: --batch_size 16 --do_flip 1
]
SIG_FIELDS = ("precision", "tile", "ksize", "stride", "relu", "res", "adds", "bilinear", "out_fp32", "split_k", "w_pairs", "segments",
              "in2", "tap", "fused")


def _signature(precision, tile, ksize, stride, relu, res, adds, up, out_fp32, ksplit, w_pairs, segments=0, in2="", tap=False, fused=""):
    """What decides which code a conv launch runs.  w_pairs only changes the layout of 32-half K tiles (smap_op.w_pairs): 0 elsewhere."""
    from smap_amd.engine import tile_bk, tile_family
    x3 = precision == "x3"
    wp = int(bool(w_pairs)) if (tile_family(tile) in ("igemm", "persist") and tile_bk(tile, x3) == 32) else 0
    return (precision, int(tile), int(ksize), int(stride), int(bool(relu)), bool(res), bool(adds), bool(up), int(bool(out_fp32)),
            ksplit > 1, wp, int(segments), in2, bool(tap), fused)


def launch_signature(g, op):
    p = op.p
    fused = ("block_first" if "short" in p else "block") if "head" in p else "tail" if "tail" in p else ""
    in2 = ("relusum" if p["cat"].get("relusum") else "cat") if "cat" in p else ""
    return _signature(g.precision, p["tile"], p["ksize"], p["stride"], p["relu"], op.res is not None,
                      op.add1 is not None or op.add2 is not None, bool(op.aux), p["out_fp32"], p.get("ksplit", 1), p["w_pairs"],
                      len(p.get("segs", [])), in2, "tap" in p, fused)


def unit_case_signatures(T):
    """The signatures the unit cases of tests/test_backbone_gpu.py (module T) run, derived from its case lists as its tests run them."""
    from smap_amd.engine import TILE_TABLE, tile_has, tile_ids
    cov = set()
    for cases, prec in ((T.CASES, "f16"), (T.X3_CASES, "x3")):      # _run_single_conv(*case, seed=hash(case) % 1000): w_pairs = seed % 2
        for c in cases:
            _, _, _, _, _, k, s, tile, relu, res, adds = c
            cov.add(_signature(prec, tile, k, s, relu, res, adds, None, 0, 1, hash(c) % 1000 % 2))
    for c in getattr(T, "EDGE_CASES", []):
        prec, _, _, _, _, _, k, s, tile, relu, res, adds, up, out_fp32, ksplit, w_pairs = c
        for pr in (("f16", "x3") if prec == "both" else (prec,)):
            cov.add(_signature(pr, tile, k, s, relu, res, adds, up, out_fp32, ksplit, w_pairs))
    for c in T.TAIL_CASES:
        _, _, _, _, _, _, tile, relu, res, adds = c
        for pr in ("f16", "x3"):
            cov.add(_signature(pr, tile, 3, 1, relu, res, adds, None, 0, 1, 0, fused="tail"))
    for _, _, _, tile, adds in T.BLOCK_CASES:                       # split precision only; the first block's shortcut replaces the residual
        first = TILE_TABLE[tile].first
        cov.add(_signature("x3", tile, 3, 1, 1, not first, adds, None, 0, 1, 0, fused="block_first" if first else "block"))
    for c in T.SEG_CASES:
        _, _, _, _, couts, relus, up, tile, w_pairs = (c + (1,))[:9]
        for pr in ("f16", "x3"):
            if pr == "x3" or not tile_has(tile, "regepi", True):
                cov.add(_signature(pr, tile, 1, 1, relus[0], False, False, up, 0, 1, w_pairs, segments=len(couts) - 1))
    for c in T.CAT_CASES:                                             # w_pairs = (B == 1) in these harnesses
        for pr in ("f16", "x3"):
            cov.add(_signature(pr, c[7], 1, 1, 1, False, False, None, 0, 1, c[0] == 1, in2="cat"))
    for c in getattr(T, "RELUSUM_CASES", []):
        for pr in ("f16", "x3"):
            cov.add(_signature(pr, c[6], 1, 1, 0, False, False, None, 0, 1, c[0] == 1, in2="relusum"))
    for B, _, _ in getattr(T, "TAP_SHAPES", []):
        for pr in ("f16", "x3"):
            cov.add(_signature(pr, tile_ids(cap="tapdot")[0], 1, 1, 1, False, False, None, 1, 1, B == 1, tap=True))
    return cov


def test_launch_inventory_every_shipped_conv_has_a_unit_case(monkeypatch):
    """The schedules the product builds at 512x832 (round 6's switches as the product sets them, not as conftest forces them for the
    small test schedules) reduced to one signature per conv launch: tile, taps, stride, every epilogue input, split K, weight layout,
    segments, second input, tap head, fused block.  Each must be run by a unit case of tests/test_backbone_gpu.py against an f64
    reference: a kernel path that only a full-size schedule reaches is otherwise checked only through the end-to-end outputs."""
    import test_backbone_gpu as T
    from smap_amd.engine import Graph, OP_CONV
    for k in ("SMAP_CAT", "SMAP_SKIPSUM", "SMAP_TAPHEAD"):
        monkeypatch.delenv(k, raising=False)
    sd = _full_size_sd()
    shipped = {}
    for B, prec, flip in SHIPPED_SCHEDULES:
        g = Graph(sd, B, 512, 832, precision=prec, flip_pair=list(range(43)) if flip else None)
        for op in g.ops:
            if op.kind == OP_CONV:
                shipped.setdefault(launch_signature(g, op), f"{B}{'xflip' if flip else ''} {prec}: {op.out.name}")
    assert len(shipped) > 100
    missing = sorted(set(shipped) - unit_case_signatures(T))
    assert not missing, "conv launches of the shipped schedules without a unit case:\n" + "\n".join(
        f"  {dict(zip(SIG_FIELDS, s))}  (e.g. {shipped[s]})" for s in missing)


@pytest.mark.parametrize("B", [8, 16])
def test_arena_without_reuse_keeps_two_input_launches_in_one_window(monkeypatch, B):
    """reuse=False (every tensor kept, for BackboneEngine.read_tensor) makes an 8-frame x3 arena of 8 GiB: both inputs of every conv_cat /
    conv_relusum launch must still share a 4 GiB window (one base address per launch), and the library must accept the plan.  The
    reusing arena -- what the product runs -- keeps its layout."""
    import ctypes as C
    from smap_amd import lib as L
    from smap_amd.engine import Graph, OP_CONV, WINDOW
    for k in ("SMAP_CAT", "SMAP_SKIPSUM", "SMAP_TAPHEAD"):
        monkeypatch.delenv(k, raising=False)
    g = Graph(_full_size_sd(), B, 512, 832, precision="x3")
    assert g.allocate(reuse=False) > 2 * WINDOW
    two = [op for op in g.ops if op.kind == OP_CONV and "cat" in op.p]
    assert len(two) >= 10 and all(op.inp.off // WINDOW == op.aux2.off // WINDOW for op in two)
    spans = sorted((t.off, t.off + t.nbytes) for t in g.tensors + g.scratch_tensors + [g.kcount] if t is not None and t.off >= 0)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))          # nothing shares bytes
    h = C.c_void_p()
    assert L.load().smap_plan_create(g.emit(), len(g.ops), C.byref(h)) == 0
    L.load().smap_plan_destroy(h)


# -- the host-side guard (csrc/plan_check.cpp): one rule for every arena range of every op kind ---------------------------------------------

def _one_op_plan_rc(o, alter=None):
    """smap_plan_create on a copy of `o` alone (lane 0, no waits), after alter(copy)."""
    import ctypes as C
    from smap_amd import lib as L
    one = (L.SmapOp * 1)(o)
    one[0].lane = one[0].n_wait = 0
    if alter:
        alter(one[0])
    h = C.c_void_p()
    rc = L.load().smap_plan_create(one, 1, C.byref(h))
    if rc == 0:
        L.load().smap_plan_destroy(h)
    return rc


BAD_ARENA_OFFSETS = (-1, 0, 16384 - 16, 2 ** 32 - 16)      # absent; on the zero page; its last 16 bytes; crossing into the next window's zero page


@pytest.fixture(scope="module")
def guard_schedules(small_sd):
    """Two emitted 2x64x96 schedules that between them hold every op kind: split precision with split K forced on and round 6's launches
    (second input, tap-dot + TAPSUM); fp16 with one launch per conv, the unfused UPADD and the fused stem + pool."""
    from smap_amd.engine import Graph
    out = {}
    for name, precision, env in (("x3", "x3", dict(SMAP_SPLITK="2", SMAP_CAT="1", SMAP_SKIPSUM="1", SMAP_TAPHEAD="1")),
                                 ("f16", "f16", dict(SMAP_MERGE_1X1="0", SMAP_NO_UPADD_FUSION="1", SMAP_STEMPOOL="1"))):
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            g = Graph(small_sd, 2, 64, 96, precision=precision)
            g.allocate()
            out[name] = g.emit()
    return out


def test_every_required_arena_offset_of_every_op_kind_is_checked(guard_schedules):
    """One op of each kind out of emitted 2x64x96 schedules, as a one-op plan: accepted as emitted, refused with any REQUIRED arena offset
    absent (-1), on a reserved zero page (0, SMAP_ZERO_PAGE - 16) or crossing into the next window (2^32 - 16).  (Before the ranges of
    every kind went through one walk, the MAXPOOL, UPADD, STEM, STEMPOOL and HEADSUM rows were accepted.)"""
    from smap_amd.engine import OP_CONV, OP_HEADSUM, OP_MAXPOOL, OP_STEM, OP_STEMPOOL, OP_TAPSUM, OP_UPADD
    x3, f16 = guard_schedules["x3"], guard_schedules["f16"]
    first = lambda ops, pred: next(o for o in ops if pred(o))
    rows = [     # kind, the op, its required arena offsets as (field, index or None)
        ("CONV", first(x3, lambda o: o.kind == OP_CONV and o.head_cin == 0 and o.ksplit <= 1), [("in_off", None), ("out_off", None)]),
        ("CONV split K", first(x3, lambda o: o.kind == OP_CONV and o.ksplit > 1), [("kpart_off", None), ("kcount_off", None)]),
        ("CONV second input", first(x3, lambda o: o.kind == OP_CONV and o.in2_C > 0), [("in2_off", None)]),
        ("CONV segments", first(x3, lambda o: o.kind == OP_CONV and o.seg_n[0] > 0), [("seg_out_off", 0)]),
        ("STEM", first(x3, lambda o: o.kind == OP_STEM), [("out_off", None)]),
        ("STEMPOOL", first(f16, lambda o: o.kind == OP_STEMPOOL), [("out_off", None)]),
        ("MAXPOOL", first(x3, lambda o: o.kind == OP_MAXPOOL), [("in_off", None), ("out_off", None)]),
        ("UPADD", first(f16, lambda o: o.kind == OP_UPADD), [("in_off", None), ("out_off", None), ("aux_off", 0)]),
        ("HEADSUM", first(x3, lambda o: o.kind == OP_HEADSUM and o.n_aux == 3), [("aux_off", 0), ("aux_off", 1), ("aux_off", 2)]),
        ("TAPSUM", first(x3, lambda o: o.kind == OP_TAPSUM), [("aux_off", 0)]),
    ]
    for kind, o, fields in rows:
        assert _one_op_plan_rc(o) == 0, kind
        for field, idx in fields:
            for val in BAD_ARENA_OFFSETS:
                def alter(c, field=field, idx=idx, val=val):
                    if idx is None:
                        setattr(c, field, val)
                    else:
                        getattr(c, field)[idx] = val
                assert _one_op_plan_rc(o, alter) != 0, (kind, field, idx, val)


def test_split_k_tickets_may_not_lie_on_a_head_sum_or_tap_sum_source(guard_schedules):
    """A ticket slice overlaps no arena range of any op: the fp32 sources of HEADSUM and TAPSUM included."""
    import ctypes as C
    from smap_amd import lib as L
    from smap_amd.engine import OP_CONV, OP_HEADSUM, OP_TAPSUM
    ops = guard_schedules["x3"]
    n, h = len(ops), C.c_void_p()
    assert L.load().smap_plan_create(ops, n, C.byref(h)) == 0
    L.load().smap_plan_destroy(h)
    i = next(k for k in range(n) if ops[k].kind == OP_CONV and ops[k].ksplit > 1)
    for kind in (OP_HEADSUM, OP_TAPSUM):
        src = next(o for o in ops if o.kind == kind)
        bad = (L.SmapOp * n)()
        C.memmove(bad, ops, C.sizeof(bad))
        bad[i].kcount_off = src.aux_off[0]
        assert L.load().smap_plan_create(bad, n, C.byref(h)) != 0, kind


def test_sizes_beyond_int64_are_refused(guard_schedules):
    """B = H = W = in_stride_c = INT32_MAX on an otherwise valid CONV: the byte count of its input does not fit int64."""
    from smap_amd.engine import OP_CONV
    o = next(o for o in guard_schedules["x3"] if o.kind == OP_CONV and o.head_cin == 0)

    def huge(c):
        c.B = c.H = c.W = c.in_stride_c = 2 ** 31 - 1
    assert _one_op_plan_rc(o) == 0 and _one_op_plan_rc(o, huge) != 0


# smap_workspace_bytes (arena, output) of the library built from the parent of the commit that introduced csrc/plan_check.cpp
WORKSPACE_BEFORE_THE_SPLIT = {("x3", 2): (4735232, 178180), ("f16 flip", 2): (5718784, 178180),
                              ("x3", 8): (1308639232, 49414148), ("x3", 16): (2617262080, 98828292)}


def test_workspace_bytes_did_not_drift(small_sd):
    import ctypes as C
    from smap_amd import lib as L
    from smap_amd.engine import Graph
    lib = L.load()
    full = _full_size_sd()
    for (name, B), want in WORKSPACE_BEFORE_THE_SPLIT.items():
        g = Graph(small_sd, 2, 64, 96, precision=name[:3].strip(), flip_pair=list(range(43)) if "flip" in name else None) if B == 2 else \
            Graph(full, B, 512, 832, precision="x3")
        g.allocate()
        h, ar, ob = C.c_void_p(), C.c_int64(), C.c_int64()
        assert lib.smap_plan_create(g.emit(), len(g.ops), C.byref(h)) == 0
        assert lib.smap_workspace_bytes(h, C.byref(ar), C.byref(ob)) == 0
        lib.smap_plan_destroy(h)
        assert (ar.value, ob.value) == want, (name, B)


# -- SchedulePolicy (smap_amd/engine.py): the SMAP_* schedule switches as one value
# one setting per SchedulePolicy field that differs from what the tests run under (tests/conftest.py: CAT / SKIPSUM / TAPHEAD = 1); TABLE = a file
POLICY_SETTINGS = {
    "block": {"SMAP_BLOCK": ""}, "block_first": {"SMAP_BLOCK_FIRST": ""}, "tail": {"SMAP_TAIL": "64:80,128:82"},
    "cat": {"SMAP_CAT": "0"}, "skipsum": {"SMAP_SKIPSUM": "0"}, "taphead": {"SMAP_TAPHEAD": "0"}, "merge_1x1": {"SMAP_MERGE_1X1": "0"},
    "splitk": {"SMAP_SPLITK": "3"}, "splitk_mink": {"SMAP_SPLITK_MINK": "1024"}, "deep_tile": {"SMAP_DEEP_TILE": "0"},
    "lanes": {"SMAP_LANES": "1"}, "wpairs": {"SMAP_WPAIRS": "0"}, "x3_tile": {"SMAP_X3_TILE": "2"}, "cat_tile": {"SMAP_CAT_TILE": "20"},
    "relusum_tile": {"SMAP_RELUSUM_TILE": "53"}, "halo3": {"SMAP_HALO3": "16"}, "halo3_deep": {"SMAP_HALO3_DEEP": "1"},
    "tile_remap": {"SMAP_TILE_REMAP": "2:7"}, "tile_policy": {"SMAP_TILE_POLICY": "traffic"}, "stempool": {"SMAP_STEMPOOL": "1"},
    "no_upadd_fusion": {"SMAP_NO_UPADD_FUSION": "1"}, "tile_table": {"SMAP_TILE_TABLE": "TABLE"}, "tile_table_x3": {"SMAP_TILE_TABLE_X3": "TABLE"}}


def _cache_key():
    from smap_amd.engine import plan_cache_key
    return plan_cache_key({"w": torch.arange(4.0)}, 2, 64, 96, 3, 256, 43, 14, "x3", None, False)


def test_plan_cache_key_covers_every_policy_field_and_nothing_else(monkeypatch, tmp_path):
    import dataclasses
    from smap_amd.engine import SchedulePolicy
    fields = [f.name for f in dataclasses.fields(SchedulePolicy)]
    assert sorted(fields) == sorted(POLICY_SETTINGS), "a new SchedulePolicy field needs a setting in POLICY_SETTINGS"
    table = tmp_path / "table.json"
    table.write_text(json.dumps({"2,16,24,64,64,1,1": 21}))
    base = _cache_key()
    assert base == _cache_key()
    for name in fields:
        with monkeypatch.context() as mp:
            for k, v in POLICY_SETTINGS[name].items():
                mp.setenv(k, str(table) if v == "TABLE" else v)
            assert getattr(SchedulePolicy.from_env(), name) != getattr(SchedulePolicy.from_env({"SMAP_CAT": "1", "SMAP_SKIPSUM": "1", "SMAP_TAPHEAD": "1"}), name), name
            assert _cache_key() != base, name
        assert _cache_key() == base, name
    for k in ("SMAP_DECODE_THREADS", "SMAP_LAUNCH_FRAMES", "SMAP_TRACE_PTR", "SMAP_ARENAS_PER_DEVICE"):       # not schedule switches
        monkeypatch.setenv(k, "3")
    assert _cache_key() == base


def test_plan_cache_key_covers_both_tile_tables(monkeypatch, tmp_path):
    t16, tx3 = tmp_path / "t16.json", tmp_path / "tx3.json"
    for t in (t16, tx3):
        t.write_text(json.dumps({"2,16,24,64,64,1,1": 21}))
    monkeypatch.setenv("SMAP_TILE_TABLE", str(t16))
    monkeypatch.setenv("SMAP_TILE_TABLE_X3", str(tx3))
    keys = [_cache_key()]
    for t in (t16, tx3):
        t.write_text(json.dumps({"2,16,24,64,64,1,1": 21, "2,16,24,64,256,1,1": 20}))
        keys.append(_cache_key())
    assert len(set(keys)) == 3, keys
    monkeypatch.setenv("SMAP_NO_TILE_TABLE", "1")         # both tables empty, whatever the files say
    assert _cache_key() not in keys


def _plain_1x1(g):
    """The first launch of Graph g that Graph.conv built from one 1x1 conv of 64 output channels: (op, its key in the tile tables)."""
    from smap_amd.engine import OP_CONV
    op = next(op for op in g.ops if op.kind == OP_CONV and op.p["ksize"] == 1 and op.p["Cout"] == 64 and op.p["kinds"] == "1x1"
              and not ({"segs", "cat", "tap"} & set(op.p)) and not op.aux)
    return op, f"{op.p['frames']},{op.inp.H},{op.inp.W},{op.p['Cin']},64,1,{op.p['stride']}"


def test_every_graph_is_built_under_its_own_policy(small_sd, monkeypatch, tmp_path):
    from smap_amd.engine import Graph, SchedulePolicy
    monkeypatch.setenv("SMAP_BLOCK", "")                  # (layer by layer: layer1's 1x1 convs are launches of their own)
    monkeypatch.setenv("SMAP_BLOCK_FIRST", "")
    monkeypatch.setenv("SMAP_NO_TILE_TABLE", "1")
    g1 = Graph(small_sd, 2, 64, 96, precision="x3")
    op1, key = _plain_1x1(g1)
    other = 21 if op1.p["tile"] != 21 else 22             # the two 32-half K tiles a 64-channel launch may run on
    table = tmp_path / "tx3.json"
    table.write_text(json.dumps({key: other}))
    monkeypatch.setenv("SMAP_TILE_TABLE_X3", str(table))
    assert _plain_1x1(Graph(small_sd, 2, 64, 96, precision="x3"))[0].p["tile"] == op1.p["tile"]       # SMAP_NO_TILE_TABLE still set
    monkeypatch.delenv("SMAP_NO_TILE_TABLE")
    g2 = Graph(small_sd, 2, 64, 96, precision="x3")       # same process, other table: honoured
    assert g2.policy.tile_table_x3 == {key: other} and g1.policy.tile_table_x3 == {}
    assert _plain_1x1(g2)[0].p["tile"] == other
    g3 = Graph(small_sd, 2, 64, 96, precision="x3", policy=g1.policy)          # an explicit policy: the environment is not consulted
    assert g3.policy is g1.policy and [op.p.get("tile") for op in g3.ops] == [op.p.get("tile") for op in g1.ops]
    assert SchedulePolicy.from_env({"SMAP_NO_TILE_TABLE": "1", "SMAP_BLOCK": "", "SMAP_BLOCK_FIRST": "", "SMAP_CAT": "1", "SMAP_SKIPSUM": "1",
                                    "SMAP_TAPHEAD": "1"}) == g1.policy


def test_schedule_switches_are_read_in_from_env_only(small_sd, monkeypatch, tmp_path):
    """Built twice under ONE policy object, with every switch variable of the environment changed in between: the same blob."""
    from smap_amd.engine import Graph, SchedulePolicy
    policy = SchedulePolicy.from_env()

    def blob():
        g = Graph(small_sd, 2, 64, 96, precision="x3", policy=policy)
        g.allocate()
        return g.blob()
    want = blob()
    table = tmp_path / "table.json"
    table.write_text(json.dumps({"2,16,24,64,64,1,1": 21}))
    for setting in POLICY_SETTINGS.values():
        for k, v in setting.items():
            monkeypatch.setenv(k, str(table) if v == "TABLE" else v)
    monkeypatch.setenv("SMAP_NO_TILE_TABLE", "1")
    assert SchedulePolicy.from_env() != policy
    assert blob() == want


# -- the poisoned-arena harness of the single-op GPU tests (tests/single_op.py) ---------------------------------------------------------------

def test_poisoned_arena_comparator_on_synthetic_buffers():
    """assert_only_written / assert_same_across_fills on hand-made before / after buffers laid out as the GPU tests lay theirs out (zero page,
    guard, input, guard, guard, output, guard): a change inside a written range is accepted; ONE changed byte in a guard, in an input and in
    the zero page's neighbour is refused, with its offset and the region it falls in; a written byte that differs between the fills is
    refused too."""
    import single_op as S
    x = torch.arange(300, dtype=torch.float16)
    guards = [S.guard_bytes(16, 5), S.guard_bytes(32, 5)]
    assert guards == [4096, 8192]                                   # 256 pixels of each tensor's own stride
    before, (in_off, out_off) = S.arena_of([x], 1000, fill=0xFF, guards=guards)
    assert in_off == 16384 + 4096 and out_off == in_off + 768 + 4096 + 8192 and before.numel() == out_off + 1024 + 8192 + 256
    assert bool((before[:in_off] == 0xFF).all()) and bool((before[in_off + 600:] == 0xFF).all())        # zero page, guards, gaps, output
    assert torch.equal(before[in_off:in_off + 600], S.raw8(x))
    other = S.arena_of([x], 1000, fill=0x7B, guards=guards)[0]
    assert torch.equal(other[in_off:in_off + 600], S.raw8(x)) and bool((other[out_off:] == 0x7B).all())
    written = [S.ZERO_PAGE_RANGE, (out_off, out_off + 1000)]
    regions = [("the zero page",) + S.ZERO_PAGE_RANGE, ("x", in_off, in_off + 600), ("out", out_off, out_off + 1000)]
    after = before.clone()
    after[:16384] = 0
    after[out_off:out_off + 1000] = 7
    S.assert_only_written(before, after, written, regions)          # every written byte changed: accepted
    S.assert_only_written(before, before.clone(), written, regions)
    for off, where in ((16384, "the guard or gap behind the zero page"), (in_off - 1, "the guard or gap behind the zero page"),
                       (in_off + 599, "in x,"), (in_off + 600, "the guard or gap behind x"), (out_off - 1, "the guard or gap behind x"),
                       (out_off + 1000, "the guard or gap behind out"), (before.numel() - 1, "the guard or gap behind out")):
        bad = after.clone()
        bad[off] ^= 1
        with pytest.raises(AssertionError, match=r"arena byte %d, .*%s.* changed outside" % (off, where)):
            S.assert_only_written(before, bad, written, regions)
    with pytest.raises(AssertionError, match="byte %d, in out, changed outside" % (out_off + 999)):     # the written range declared one byte short
        S.assert_only_written(before, after, [S.ZERO_PAGE_RANGE, (out_off, out_off + 999)], regions)
    after2 = after.clone()
    S.assert_same_across_fills(after, after2, written, regions)
    after2[in_off - 1] ^= 1                                          # outside the written ranges: not this check's business
    S.assert_same_across_fills(after, after2, written, regions)
    after2[out_off + 17] = 0x7B
    with pytest.raises(AssertionError, match="arena byte %d, in out, differs between fills: 0x07 / 0x7b" % (out_off + 17)):
        S.assert_same_across_fills(after, after2, written, regions)
    # the layout of a launch: operands, outputs, weight chunks with their guards; an absent operand has offset -1 and no bytes
    la = S.FilledLaunch([("x", x, 16, 5), ("res", None, 16, 5)], [("out", 1000, 32, 5), ("tickets", 0, 4, 0)], [torch.ones(100), torch.ones(3)],
                        blob_guard=512)
    assert la.offs[:3] == [in_off, -1, out_off] and la.woffs == [0, 512 + 512] and la.written() == written
    assert la.written(short_out=16) == [S.ZERO_PAGE_RANGE, (out_off, out_off + 984)]
    blob = la.blob(0x7B)
    assert blob.numel() == 1024 + 256 + 512 and bool((blob[400:1024] == 0x7B).all()) and bool((blob[1024 + 12:] == 0x7B).all())
    assert torch.equal(la.arena(0xFF)[:before.numel()], before) and la.total == before.numel() + 2 * S.guard_bytes(4)      # (the absent tickets' guards)
    short = S.FilledLaunch([("x", x, 16, 5)], [("out", 1000, 32, 5)], short_in=16)
    assert short.offs == [in_off, out_off] and bool((short.arena(0x7B)[in_off + 584:in_off + 600] == 0x7B).all())


# -- what the schedule builder enumerates: an op's operands, the arena's lifetimes, the convs of an Upsample_unit ------------------------------

def _digest_tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("schedule_digest", os.path.join(ROOT, "tools", "schedule_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def small_schedules(small_sd):
    """Every 2x64x96 case of tools/schedule_digest.py (the smallest shape the builder accepts with all five levels present), built and
    allocated with reuse=True ONCE: [(case, ops, every tensor of the arena)].  The weights go with the Graph; ops and tensors are small."""
    from smap_amd.engine import Graph
    T = _digest_tool()
    out, refused = [], []
    with pytest.MonkeyPatch.context() as mp:
        for label, prec, kw, sw in T.small_cases():
            for k in T.SWITCHES:
                mp.delenv("SMAP_" + k, raising=False)
            for k, v in sw.items():
                mp.setenv("SMAP_" + k, v)
            case = "%s %s %s" % (label, prec, sw)
            try:
                g = Graph(small_sd, *T.SMALL, precision=prec, **kw)
            except ValueError:
                refused.append(case)
                continue
            g.allocate(reuse=True)
            out.append((case, g.ops, T.every_tensor(g)))
    assert len(refused) == 1 and "TILE_POLICY" in refused[0] and "MERGE_1X1" not in refused[0], refused      # (the tool's list says why)
    assert len(out) >= 60
    return out


def _tensor_fields(op):
    """(field name, the Tensors in it) of every dataclass field of `op` that holds a Tensor or a list of them."""
    import dataclasses
    from smap_amd.engine import Tensor
    for f in dataclasses.fields(op):
        v = getattr(op, f.name)
        ts = [v] if isinstance(v, Tensor) else [t for t in v if isinstance(t, Tensor)] if isinstance(v, (list, tuple)) else []
        if ts:
            yield f.name, ts


def test_every_tensor_field_of_an_op_is_a_read_a_write_or_scratch(small_schedules):
    """Graph.allocate and Graph.emit enumerate an op's tensors through Op.reads(), Op.writes() and Op.scratch only: every dataclass field of
    Op that holds a Tensor (or a list of them) must be covered by one of the three -- over every op of the small schedules, and on a probe op
    with a tensor of its own in EVERY field that can hold one (found from dataclasses.fields: a field added later and classified by nobody
    fails here before a schedule uses it).  A field left out gives its tensor too short a lifetime: the packer then hands its bytes on while
    they are still read, and nothing else fails."""
    import dataclasses
    from smap_amd.engine import Op, Tensor
    seen = set()
    for case, ops, _ in small_schedules:
        for i, op in enumerate(ops):
            covered = {id(t) for t in op.reads() + op.writes() + list(op.scratch)}
            for name, ts in _tensor_fields(op):
                seen.add(name)
                assert all(id(t) in covered for t in ts), (case, i, name)
    assert seen == {"out", "inp", "res", "add1", "add2", "aux", "outs", "aux2", "scratch"}       # (the schedules use every field there is)
    can_hold = [f for f in dataclasses.fields(Op) if f.type in (Tensor, list)]
    probe = Op(0, **{f.name: Tensor(f.name, 1, 1, 1, 8) if f.type is Tensor else [Tensor(f.name, 1, 1, 1, 8)] for f in can_hold})
    assert {f.name for f in can_hold} == {name for name, _ in _tensor_fields(probe)} >= seen
    covered = {id(t) for t in probe.reads() + probe.writes() + list(probe.scratch)}
    assert all(id(t) in covered for _, ts in _tensor_fields(probe) for t in ts)
    assert not {id(t) for t in probe.reads()} & {id(t) for t in probe.writes()} and Op(0).reads() == Op(0).writes() == []


def test_small_schedules_have_no_live_overlap_and_keep_off_the_zero_pages(small_schedules):
    """reuse=True: no two arena tensors (split-K scratch and the ticket region included) whose [first, last] intervals intersect share a
    byte, every tensor is placed, and none touches a zero page or crosses a window -- in every small schedule, the all-heads and lanes ones
    (whose side-lane operands live to the end of the schedule) included."""
    from smap_amd.engine import WINDOW, ZERO_PAGE
    for case, ops, every in small_schedules:
        assert all(0 <= t.first <= t.last < len(ops) for t in every), case
        for t in every:
            assert t.off >= 0 and t.off % WINDOW >= ZERO_PAGE and t.off // WINDOW == (t.off + t.nbytes - 1) // WINDOW, (case, t.name)
        live = sorted((t.first, t.last, t.off, t.off + t.nbytes, t.name) for t in every)
        for i, a in enumerate(live):
            for b in live[i + 1:]:
                if b[0] > a[1]:
                    break
                assert a[3] <= b[2] or b[3] <= a[2], (case, a[4], b[4])


@pytest.mark.parametrize("all_heads", [False, True], ids=["inference", "all_heads"])
def test_merge_modes_compute_the_same_convs(small_sd, all_heads):
    """SMAP_MERGE_1X1 = 0, 1 and 2 change how an Upsample_unit's 1x1 convs are LAUNCHED, never which convs of the reference run: the
    sorted state-dict prefixes are the same list, with and without every head chain (policy: no skip1 + skip2 launch, no K-concatenated
    shortcut, no tap-dot head -- mode 0 never has them)."""
    from dataclasses import replace
    from smap_amd.engine import Graph, SchedulePolicy
    base = SchedulePolicy.from_env({"SMAP_CAT": "0", "SMAP_SKIPSUM": "0", "SMAP_TAPHEAD": "0"})
    convs = [sorted(Graph(small_sd, 2, 64, 96, all_heads=all_heads, policy=replace(base, merge_1x1=m)).convs) for m in (0, 1, 2)]
    assert convs[0] == convs[1] == convs[2] and len(convs[0]) == len(set(convs[0])) == (268 if all_heads else 206)
