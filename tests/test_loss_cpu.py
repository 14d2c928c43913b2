"""CPU suite of the training loss: everything behind the reduction (csrc/loss_core.h through smap_loss_finish_host and, alone under
sanitizers, tests/c/loss_finish_main.cpp) against tests/golden/loss.npz -- the reference's own losses, tables and gradient factors,
recorded by executing it in float64 (tests/golden/gen_golden_loss.py) -- plus the argument rules of the C ABI and of the Python side.

The sums fed in are numpy's float64 sums of the EXACT differences of the regenerated fp32 inputs, so both sides are double arithmetic
on the same numbers and differ by operation order alone: 1e-12 relative."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import loss_scenes as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC, N2D, NDD = 57, 43, 14
RTOL = 1e-12


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "loss.npz"))


_scene_cache = {}


def scene_inputs(name):
    """(inputs, float64 sums of the exact differences, root_d at the rows): computed once per scene, never modified."""
    if name not in _scene_cache:
        x = LS.inputs(name)
        _scene_cache[name] = (x, LS.host_sums(name, x), LS.rd_at_rows(name, x))
    return _scene_cache[name]


def finish_host(s, sums, valids, rdepth, rd_at, single=0):
    """smap_loss_finish_host -> (rc, dict of its outputs)."""
    from smap_amd import lib as L
    n_heads = 1 if single else 4 * s["stage_num"]
    B, R = valids.shape[0], rdepth.shape[1]
    f64 = lambda a: np.ascontiguousarray(a, np.float64)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    sums, valids, rdepth, rd_at = f64(sums), f32(valids), f32(rdepth), f32(rd_at)
    out = dict(result=np.full(8, -7.0), m=np.zeros((n_heads, B, NC)), sel=np.zeros((n_heads, B, NC)), coef=np.zeros((n_heads, B, NC)),
               root_cell=np.zeros((n_heads, B, R), np.int32), root_fac=np.zeros((n_heads, B, R)), part=np.zeros((n_heads, B, 6)))
    ptr = lambda a: a.ctypes.data
    rc = L.load().smap_loss_finish_host(ptr(sums), ptr(valids), ptr(rdepth), ptr(rd_at), s["stage_num"], int(s["ohkm"]), s["topk"],
                                        int(s["ctf"]), single, B, R, s["H"], s["W"], ptr(out["result"]), ptr(out["m"]), ptr(out["sel"]),
                                        ptr(out["coef"]), ptr(out["root_cell"]), ptr(out["root_fac"]), ptr(out["part"]))
    return rc, out


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= rtol * np.abs(b)).all())


def root_gradient(s, x, out, n_heads):
    """The dense root_d gradient [n_heads, B, H, W] the root table stands for (rows added in order)."""
    g = np.zeros((n_heads, s["B"], s["H"] * s["W"]))
    for h in range(n_heads):
        for b in range(s["B"]):
            for r in range(x["rdepth"].shape[1]):
                if out["root_cell"][h, b, r] >= 0:
                    g[h, b, out["root_cell"][h, b, r]] += out["root_fac"][h, b, r]
    return g.reshape(n_heads, s["B"], s["H"], s["W"])


def check_against_fixture(name, golden, out):
    s, (x, sums, rd_at) = LS.SCENES[name], scene_inputs(name)
    n_heads = 4 * s["stage_num"]
    assert close(out["result"][:4], golden[name + "_losses"]), (out["result"][:4], golden[name + "_losses"])
    assert (out["result"][4:] == 0).all()
    # the per-channel tables are the reference's tmp_loss
    assert close(out["m"][:, :, :N2D], golden[name + "_tmp2d"]) and close(out["m"][:, :, N2D:], golden[name + "_tmp3d"])
    # coef: the reference's gradient factor (the fixture folds the upstream gradient in)
    want = golden[name + "_coef"]
    assert close(out["coef"] * s["upstream"], want)
    # the selection is where the reference's gradient flows; where m is 0 any choice is right (zero-weight ties)
    live = out["m"] > 0
    assert ((out["sel"] != 0) == (want != 0))[live].all() and set(np.unique(out["sel"])) <= {0.0, 1.0}
    if s["ohkm"]:
        for h in range(3, n_heads, 4):
            assert (out["sel"][h, :, :15].sum(1) == s["topk"]).all() and (out["sel"][h, :, 15:N2D].sum(1) == 2 * s["topk"]).all()
            assert (out["sel"][h, :, N2D:].sum(1) == s["topk"]).all()
    assert (out["sel"][[h for h in range(n_heads) if h % 4 != 3 or not s["ohkm"]]] == 1).all()
    # the root table is the reference's root_d gradient
    g = root_gradient(s, x, out, n_heads) * s["upstream"]
    want_g = np.zeros_like(g)
    for (h, b, y, xx), v in zip(golden[name + "_rd_idx"], golden[name + "_rd_val"]):
        want_g[h, b, y, xx] = v
    assert close(g, want_g)


@pytest.mark.parametrize("name", list(LS.SCENES))
def test_finish_host_equals_the_reference(name, golden):
    s, (x, sums, rd_at) = LS.SCENES[name], scene_inputs(name)
    assert int(golden[name + "_seed"]) == s["seed"] and float(golden[name + "_upstream"]) == s["upstream"]
    rc, out = finish_host(s, sums, x["valids"], x["rdepth"], rd_at)
    assert rc == 0
    check_against_fixture(name, golden, out)


def test_ties_go_to_the_lower_channel():
    """Two identical channels across the cut of every top-k: the lower index is kept, whatever order the values come in."""
    s = dict(stage_num=1, ohkm=True, topk=2, ctf=False, H=4, W=4)
    sums = np.zeros((4, 1, NC))
    sums[3, 0, :15] = np.arange(15, 0, -1)                   # key points: 15, 14, 13 ... -> top-2 = channels 0, 1
    sums[3, 0, 1] = sums[3, 0, 2] = 14.0                      # channels 1 and 2 tie for the second place
    sums[3, 0, 15:N2D] = np.arange(1, 29)                     # PAF: ascending -> top-4 = the last four
    sums[3, 0, 15 + 24] = sums[3, 0, 15 + 20] = 25.5          # channels 20 and 24 of the group tie for the fourth place
    sums[3, 0, N2D:] = 3.0                                    # depth: all equal -> channels 0, 1
    rc, out = finish_host(s, sums, np.ones((1, NC)), np.zeros((1, 1, 3)), np.zeros((4, 1, 1)))
    assert rc == 0
    assert np.flatnonzero(out["sel"][3, 0, :15]).tolist() == [0, 1]
    assert np.flatnonzero(out["sel"][3, 0, 15:N2D]).tolist() == [20, 25, 26, 27]
    assert np.flatnonzero(out["sel"][3, 0, N2D:]).tolist() == [0, 1]
    assert (out["coef"][3, 0][out["sel"][3, 0] == 0] == 0).all() and (out["coef"][3, 0][out["sel"][3, 0] == 1] > 0).all()
    assert (out["sel"][:3] == 1).all()
    # mean over (B, topk) + mean over (B, 2 * topk); depth: mean over (B, topk)
    assert close(out["result"][1], ((15 + 14) / 2 + (25.5 + 26 + 27 + 28) / 4) / 16) and close(out["result"][2], 3.0 / 16)


def test_a_row_outside_the_map_is_counted_and_poisons_the_total():
    s, (x, sums, rd_at) = LS.SCENES["scalar"], scene_inputs("scalar")
    for row in ((9.0, 3.0, 1.0), (3.0, 11.0, 1.0), (-1.0, 3.0, 1.0), (3.0, -2.5, 1.0), (float("nan"), 3.0, 1.0), (3e9, 3.0, 1.0)):
        rdepth = x["rdepth"].copy()
        rdepth[1, 2] = row
        rc, out = finish_host(s, sums, x["valids"], rdepth, rd_at)
        assert rc == 0 and out["result"][4] == 1 and np.isnan(out["result"][0]), row
        assert (out["root_cell"][:, 1, 2] == -2).all() and (out["root_fac"][:, 1, 2] == 0).all()
        assert np.isfinite(out["result"][1:4]).all()
    rdepth = x["rdepth"].copy()
    rdepth[1, 2] = (9.0, 3.0, 0.0)                           # Z <= 0: not a row at all
    rc, out = finish_host(s, sums, x["valids"], rdepth, rd_at)
    assert rc == 0 and out["result"][4] == 0 and np.isfinite(out["result"][0])


def test_argument_errors():
    """Every SMAP_E_ARG case, before any launch (none of these calls reaches the GPU)."""
    from smap_amd import lib as L
    lib = L.load()
    good = dict(stage_num=3, ohkm=1, topk=8, ctf=1, single=0, B=2, S=5, R=4, H=9, W=11)
    buf = np.zeros(1 << 16, np.uint8)
    p = buf.ctypes.data                                       # a non-null HOST address: an accepted call would launch, so none may be
    heads = (C.c_void_p * 48)(*([p] * 48))

    def forward(heads=heads, labels=p, valids=p, rdepth=p, ws=p, ws_bytes=1 << 16, result=p, **kw):
        a = dict(good, **kw)
        return lib.smap_loss_forward(heads, labels, valids, rdepth, a["stage_num"], a["ohkm"], a["topk"], a["ctf"], a["single"], a["B"],
                                     a["S"], a["R"], a["H"], a["W"], ws, ws_bytes, result, None)

    def backward(heads=heads, labels=p, ws=p, ws_bytes=1 << 16, upstream=p, grad=p, **kw):
        a = dict(good, **kw)
        return lib.smap_loss_backward(heads, labels, a["stage_num"], a["ohkm"], a["topk"], a["ctf"], a["single"], a["B"], a["S"], a["R"],
                                      a["H"], a["W"], ws, ws_bytes, upstream, grad, None)

    bad = [dict(stage_num=0), dict(stage_num=5), dict(S=4), dict(S=3, ctf=0), dict(topk=0), dict(topk=15), dict(H=0), dict(W=0),
           dict(H=4097, W=4096), dict(B=0), dict(B=65536), dict(R=0), dict(R=65536), dict(single=1), dict(single=1, stage_num=1, ctf=1)]
    for kw in bad:
        assert forward(**kw) == -1 and backward(**kw) == -1, kw
    for name in ("heads", "labels", "valids", "rdepth", "ws", "result"):
        assert forward(**{name: None}) == -1, name
    for name in ("heads", "labels", "ws", "upstream", "grad"):
        assert backward(**{name: None}) == -1, name
    one_null = (C.c_void_p * 48)(*([p] * 17 + [None] + [p] * 30))
    assert forward(heads=one_null) == -1 and backward(heads=one_null) == -1
    need = lib.smap_loss_workspace_bytes(12, 2, 4)
    from smap_amd.loss import workspace_layout
    assert need == workspace_layout(12, 2, 4)["bytes"] and need % 8 == 0
    assert forward(ws_bytes=need - 8) == -1 and backward(ws_bytes=need - 8) == -1 and forward(ws=p + 4) == -1
    for args in ((0, 2, 4), (17, 2, 4), (12, 0, 4), (12, 65536, 4), (12, 2, 0), (12, 2, 65536)):
        assert lib.smap_loss_workspace_bytes(*args) == -1
    assert forward(topk=0, ohkm=0, S=4, ctf=0, stage_num=1, B=1, R=1, H=1 << 12, W=1 << 12, ws_bytes=0) == -1   # legal up to the workspace
    # the host finish refuses the same parameters
    s = dict(LS.SCENES["squeeze"])
    x, sums, rd_at = scene_inputs("squeeze")
    for kw in (dict(stage_num=0), dict(stage_num=5), dict(ohkm=True, topk=0), dict(ohkm=True, topk=15), dict(H=0), dict(H=1 << 13, W=1 << 12)):
        assert finish_host(dict(s, **kw), np.zeros((16, 1, NC)), x["valids"], x["rdepth"], np.zeros((16, 1, 1)))[0] == -1, kw
    assert lib.smap_loss_finish_host(None, None, None, None, 1, 0, 8, 0, 0, 1, 1, 8, 8, None, None, None, None, None, None, None) == -1


def test_python_argument_errors():
    from smap_amd.loss import SMAPLoss
    B, H, W = 1, 8, 8
    outputs = dict(heatmap_2d=[[torch.zeros(B, 43, H, W)] * 4], det_d=[[torch.zeros(B, 14, H, W)] * 4], root_d=[[torch.zeros(B, 1, H, W)] * 4])
    labels, valids, rdepth = torch.zeros(B, 4, NC, H, W), torch.ones(B, NC, 1), torch.zeros(B, 2, 3)
    crit = SMAPLoss(stage_num=1, ohkm=False, ctf=False)
    with pytest.raises(ValueError, match="no CPU path"):
        crit(outputs, valids, labels, rdepth)
    with pytest.raises(TypeError, match="float32"):
        crit(outputs, valids, labels.double(), rdepth)
    with pytest.raises(TypeError, match="Tensor"):
        crit(outputs, valids, labels.numpy(), rdepth)
    with pytest.raises(ValueError, match="stage_num"):
        SMAPLoss(stage_num=5)
    with pytest.raises(ValueError, match="topk"):
        SMAPLoss(topk=15)
    SMAPLoss(topk=99, ohkm=False)
    cfg = type("NS", (), {})()
    cfg.MODEL, cfg.LOSS = type("NS", (), dict(STAGE_NUM=2)), type("NS", (), dict(OHKM=True, TOPK=5, COARSE_TO_FINE=False))
    crit = SMAPLoss.from_cfg(cfg)
    assert (crit.stage_num, crit.ohkm, crit.topk, crit.ctf, crit.strict) == (2, True, 5, False, False)


def test_reference_import_path():
    import lib.utils.loss_h as loss_h
    assert os.path.abspath(loss_h.__file__).startswith(ROOT)
    loss_h.DepthLoss()
    loss_h.JointsL2Loss()
    m = loss_h.JointsL2Loss(has_ohkm=True, topk=8, paf_num=14)
    assert (m.has_ohkm, m.topk, m.paf_num, m.thres) == (True, 8, 14, 0)
    with pytest.raises(NotImplementedError, match="thres"):
        loss_h.JointsL2Loss(thres=0.5)
    with pytest.raises(ValueError, match="no CPU path"):
        loss_h.DepthLoss()(torch.zeros(1, 1, 8, 8), torch.zeros(1, 2, 3))
    with pytest.raises(ValueError, match="no CPU path"):
        loss_h.JointsL2Loss()(torch.zeros(1, 14, 8, 8), torch.ones(1, 14, 1), torch.zeros(1, 14, 8, 8))
    with pytest.raises(ValueError, match="channels"):
        loss_h.JointsL2Loss()(torch.zeros(1, 13, 8, 8), torch.ones(1, 13, 1), torch.zeros(1, 13, 8, 8))


def test_finish_alone_under_sanitizers(tmp_path, golden):
    """tests/c/loss_finish_main.cpp over csrc/loss_core.h, built for the CPU with -fsanitize=address,undefined: scenes 1 to 3 give the
    fixture's numbers, an all-NaN table of sums runs through; no report either way."""
    csrc = os.path.join(ROOT, "smap_amd", "csrc")
    exe = tmp_path / "loss_finish"
    r = subprocess.run(["g++", "-g", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                        os.path.join(ROOT, "tests", "c", "loss_finish_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    for name in ("scalar", "vector", "squeeze"):
        s, (x, sums, rd_at) = LS.SCENES[name], scene_inputs(name)
        n_heads, B, R = 4 * s["stage_num"], s["B"], x["rdepth"].shape[1]
        path = tmp_path / (name + ".bin")
        hdr = np.array([s["stage_num"], s["ohkm"], s["topk"], s["ctf"], 0, B, R, s["H"], s["W"]], np.int32)
        path.write_bytes(hdr.tobytes() + sums.astype(np.float64).tobytes() + x["valids"].tobytes() + x["rdepth"].tobytes() + rd_at.tobytes())
        for extra in ((), ("nan",)):
            r = subprocess.run([str(exe), str(path)] + list(extra), capture_output=True, text=True, env=env, timeout=120)
            assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (name, extra, r.stderr[-3000:])
            cols = {}
            for line in r.stdout.splitlines():
                key, *rest = line.split()
                cols.setdefault(key, []).append(float(rest[-1]))
            n = n_heads * B * NC
            assert [len(cols[k]) for k in ("result", "coef", "sel", "m", "cell", "fac")] == [8, n, n, n, n_heads * B * R, n_heads * B * R]
            if extra:
                assert np.isnan(cols["result"][0]) and np.isnan(cols["m"]).all() and cols["result"][4] == 0
                continue
            shape = (n_heads, B, NC)
            out = dict(result=np.array(cols["result"]), coef=np.array(cols["coef"]).reshape(shape), sel=np.array(cols["sel"]).reshape(shape),
                       m=np.array(cols["m"]).reshape(shape), root_cell=np.array(cols["cell"], np.int64).reshape(n_heads, B, R),
                       root_fac=np.array(cols["fac"]).reshape(n_heads, B, R))
            check_against_fixture(name, golden, out)
