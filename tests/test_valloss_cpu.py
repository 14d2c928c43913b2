"""CPU suite of the validation loss: the all-heads schedule (smap_amd/engine.py Graph(all_heads=True)) against the native head tensors
of the imported reference (tests/golden/valloss_small.npz, gen_golden_valloss.py), what it must leave unchanged, its arena, the source
descriptors the loss reads, and test.py's --eval_loss argument rules.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import make_cfg
from recipe import recipe_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("heatmap_2d", "det_d", "root_d")
CHANNELS = (43, 14, 1)
LEVELS = ((2, 3), (4, 6), (8, 12), (16, 24))
TOL = 2e-5          # tests/test_oracle_cpu.py's bound for this interpreter against the reference's golden outputs


@pytest.fixture(scope="module")
def sd():
    from smap_amd.model.smap import SMAP
    torch.manual_seed(0)
    return recipe_state_dict(SMAP(make_cfg((16, 24))).state_dict())


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(f"{golden_dir}/valloss_small.npz")


def all_heads_graph(sd, **kw):
    from smap_amd.engine import Graph
    g = Graph(sd, 2, 64, 96, all_heads=True, **kw)
    g.allocate()
    return g


@pytest.mark.parametrize("taphead", ["1", "0"], ids=["tapdot_root", "plain_root"])
def test_all_heads_schedule_interpreted_matches_reference_native_heads(sd, golden, golden_dir, monkeypatch, taphead):
    """Graph(all_heads=True) through oracle/graph_interp.py (fp32, un-rounded folded weights): the 36 head tensors of frame 1 within
    2e-5 * max |tensor| of the reference's; frame 0 through its sum and abs-sum, within 2e-5 of the abs-sum (a relative error of 2e-5
    in every element moves either sum by no more).  The last stage's finest root-depth map is the output's own on the tap-dot route."""
    from oracle.graph_interp import run_graph
    monkeypatch.setenv("SMAP_TAPHEAD", taphead)
    g = all_heads_graph(sd, keep_ref=True)
    x = torch.from_numpy(np.load(f"{golden_dir}/backbone_small.npz")["x"])
    with torch.no_grad():
        hms, det_d, root_d, T = run_graph(g, x, quantize=False, keep=True)
    assert (g.head_tensors[(2, 3)]["root_d"] is None) == (taphead == "1")
    for s in range(3):
        for j in range(4):
            for k, (key, c) in enumerate(zip(KEYS, CHANNELS)):
                t = g.head_tensors[(s, j)][key]
                got = (T[t.name] if t is not None else root_d).double().numpy()
                assert got.shape == (2, c) + LEVELS[j], (s, j, key, got.shape)
                want = golden["h%d_%d" % (4 * s + j, k)].astype(np.float64)
                assert np.abs(got[1] - want).max() <= TOL * np.abs(want).max(), (s, j, key)
                i = 3 * (4 * s + j) + k
                assert abs(got[0].sum() - golden["sum0"][i]) <= TOL * golden["abs0"][i], (s, j, key)
                assert abs(np.abs(got[0]).sum() - golden["abs0"][i]) <= TOL * golden["abs0"][i], (s, j, key)
    z = np.load(f"{golden_dir}/backbone_small.npz")          # ... and the inference outputs are still the reference's
    for a, k in zip((hms, det_d, root_d), ("hms", "det_d", "root_d")):
        assert np.abs(a.numpy() - z[k]).max() <= TOL * np.abs(z[k]).max(), k


@pytest.mark.parametrize("kw", [dict(), dict(precision="x3", scaled_hms=True), dict(precision="x3", flip_pair=list(range(43)))],
                         ids=["f16", "x3_scaled", "x3_flip"])
def test_all_heads_false_is_the_schedule_built_without_the_argument(sd, kw):
    from smap_amd.engine import Graph
    a, b = Graph(sd, 2, 64, 96, **kw), Graph(sd, 2, 64, 96, all_heads=False, **kw)
    a.allocate()
    b.allocate()
    assert len(a.ops) == len(b.ops) and bytes(a.emit()) == bytes(b.emit())
    assert a.out_layout == b.out_layout and a.arena_bytes == b.arena_bytes and a.blob() == b.blob()
    assert b.head_tensors == {} and b.keep == []


@pytest.mark.parametrize("kw", [dict(precision="x3"), dict(precision="x3", flip_pair=list(range(43)), scaled_hms=True)], ids=["plain", "flip_scaled"])
def test_all_heads_adds_the_62_training_convs_and_keeps_the_inference_launches(sd, kw):
    """Counted by name: the 206 convs of the inference schedule, plus res_conv1/2, res_d_conv1/2 and res_rd_conv1/2 of every unit but
    those the inference outputs need already -- 268, every conv of the checkpoint.  The default schedule's ops are all still there,
    field for field but for the arena offsets and split-K tickets, in their order."""
    import re
    from smap_amd.engine import Graph
    d, g = Graph(sd, 2, 64, 96, **kw), Graph(sd, 2, 64, 96, all_heads=True, **kw)
    assert len(d.convs) == len(set(d.convs)) == 206 and len(g.convs) == len(set(g.convs)) == 268
    more = set(g.convs) - set(d.convs)
    assert len(more) == 62 and set(d.convs) <= set(g.convs)
    assert all(re.fullmatch(r"stage[0-2]\.upsample\.up[1-4]\.res_(d_|rd_)?conv[12]", n) for n in more)
    assert set(g.convs) == {n[:-len(".conv.weight")] for n in sd if n.endswith(".conv.weight")}
    names = lambda graph: [(op.kind, op.out.name if op.out is not None else None, op.p.get("tile"), op.p.get("w_pairs"), op.p.get("frames"),
                            op.p.get("ext_off")) for op in graph.ops]
    it = iter(names(g))
    assert all(n in it for n in names(d)), "the default schedule's launches, in order, are a subsequence of the all-heads schedule's"
    assert g.out_layout == d.out_layout and g.out_bytes == d.out_bytes and g.status_off == d.status_off


@pytest.mark.parametrize("reuse", [True, False])
def test_head_tensors_stay_allocated_to_the_end(sd, reuse, monkeypatch):
    """No head tensor shares a byte with a tensor (or split-K scratch) that is written after it: the loss reads all 36 behind the
    last op.  Both routes of the finest root-depth head."""
    from smap_amd.engine import Graph
    for tap in ("1", "0"):
        monkeypatch.setenv("SMAP_TAPHEAD", tap)
        g = Graph(sd, 2, 64, 96, precision="x3", all_heads=True)
        g.allocate(reuse=reuse)
        heads = [t for d in g.head_tensors.values() for t in d.values() if t is not None]
        assert len(heads) == (35 if tap == "1" else 36) and len({id(t) for t in heads}) == len(heads)
        n_last = len(g.ops) - 1
        every = g.tensors + g.scratch_tensors
        for h in heads:
            assert h.esize == 4 and h.off >= 0 and h.last == n_last
            for t in every:
                if t is h or t.off < 0 or t.first < h.first:
                    continue
                assert t.off + t.nbytes <= h.off or h.off + h.nbytes <= t.off, (h.name, t.name)
        assert max(t.off + t.nbytes for t in every) <= g.arena_bytes


def test_head_sources_describe_the_native_heads(sd, monkeypatch):
    from smap_amd.engine import graph_head_sources
    for tap in ("1", "0"):
        monkeypatch.setenv("SMAP_TAPHEAD", tap)
        for flip in (None, list(range(43))):
            g = all_heads_graph(sd, precision="x3", flip_pair=flip)
            src = graph_head_sources(g, arena_ptr=1 << 20, out_ptr=1 << 40)
            assert len(src) == 12
            for h, d in enumerate(src):
                hh, ww = LEVELS[h % 4]
                for key, c, pad in zip(KEYS, CHANNELS, (48, 16, 8)):
                    s = d[key]
                    if h == 11 and key == "root_d" and tap == "1":       # the NCHW block of the output buffer
                        assert s == ((1 << 40) + g.out_layout["root_d"][0], 16, 24, 1, 1, 16 * 24, 16 * 24)
                        continue
                    t = g.head_tensors[(h // 4, h % 4)][key]
                    assert s == ((1 << 20) + t.off, hh, ww, c, pad, 1, hh * ww * pad) and t.B == (4 if flip else 2)
                    assert s.ptr % 16 == 0
            assert len({d[k].ptr for d in src for k in KEYS}) == 36


def test_plan_cache_key_tells_the_two_schedules_apart(sd):
    from smap_amd.engine import plan_cache_key
    args = (sd, 2, 64, 96, 3, 256, 43, 14, "x3", None, False)
    assert plan_cache_key(*args) == plan_cache_key(*args, all_heads=False) != plan_cache_key(*args, all_heads=True)


def test_forward_with_labels_needs_eval_mode_and_a_gpu(sd):
    from smap_amd.model.smap import SMAP
    net = SMAP(make_cfg((16, 24)))
    x, v, lab, rd = torch.zeros(2, 3, 64, 96), torch.ones(2, 57, 1), torch.zeros(2, 5, 57, 16, 24), torch.zeros(2, 3, 3)
    with pytest.raises(RuntimeError, match="batch statistics.*backward pass"):
        net.train()(x, v, lab, rd)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        net.eval()(x, v, lab, rd)


def test_eval_loss_argument_rules():
    test_py = os.path.join(ROOT, "exps", "stage3_root2", "test.py")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = lambda *a: subprocess.run([sys.executable, test_py, *a], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    for mode in ("run_inference", "generate_train"):
        r = run("-t", mode, "--eval_loss", "1")
        assert r.returncode == 2 and "--eval_loss 1 requires -t generate_result" in r.stderr, r.stderr
    r = run("-t", "generate_result", "--eval_loss", "1", "--dry_run", "1")
    assert r.returncode == 2 and "--eval_loss 1 runs on the GPU: not available with --dry_run 1" in r.stderr, r.stderr
    r = run("-t", "generate_result", "--eval_loss", "1", "--maps_from_gt", "1")
    assert r.returncode == 2 and "--eval_loss 1 needs the network's heads: not available with --maps_from_gt 1" in r.stderr, r.stderr
    r = run("-t", "generate_result", "--eval_loss", "2")
    assert r.returncode == 2
