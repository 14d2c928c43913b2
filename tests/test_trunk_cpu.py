"""Upsample_unit trunk without a GPU: the float64 restatement (tests/trunk_restate.py) against the reference's recorded results
(tests/golden/trunk.npz, gen_golden_trunk.py), the sign-tie condition of the scenes, the workspace layout, and the argument checks of
smap_trunk_ws_bytes / smap_trunk_forward / smap_trunk_backward -- which all happen before any HIP call, so fake pointers serve."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import trunk_restate as R
import trunk_scenes as TS
import smap_amd.lib as L
from smap_amd import finetune as F
from smap_amd import gemm_f32 as G
from smap_amd import trunk as T
from train_kit import FAKE, set_attr as _set, set_fields as _d

RTOL = 1e-12           # of the tensor's largest magnitude: both sides are float64 and differ in summation order only


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "trunk.npz")))


def restate(name):
    """The restatement's O, gX, gO_prev and the gradients at the unfolded parameters of a scene, float64, with float64's interpolation weights."""
    s = TS.SCENES[name]
    x, o_prev, g, params = R.scene_operands(name)
    mods = TS.module_names(name)
    wu, bu = R.fold(params[mods[0]], TS.EPS, matrix=True)
    wc, b, it = None, bu, None
    if s["ind"] > 0:
        wc, bc = R.fold(params[mods[1]], TS.EPS, matrix=True)
        b, it = bu + bc, R.Interp(s["hp"], s["wp"], s["h"], s["w"], fp32=False)
    pre, _, _ = R.forward(x, o_prev, wu, wc, b, it)
    gr = R.backward(x, o_prev, wu, wc, g, pre > 0, it)
    unfolded = {mods[0]: R.unfold_grads(params[mods[0]], gr["gwu"], gr["gb"], TS.EPS)}
    if s["ind"] > 0:
        unfolded[mods[1]] = R.unfold_grads(params[mods[1]], gr["gwc"], gr["gb"], TS.EPS)
    return dict(o=torch.relu(pre), gx=gr["gx"], gprev=gr.get("gprev"), unfolded=unfolded)


def test_scene_fold_matches_restatement():
    for name in TS.SCENES:
        _, _, _, params = R.scene_operands(name)
        mods = TS.module_names(name)
        wu, wc, b = TS.folded64(name)
        fw, fb = R.fold(params[mods[0]], TS.EPS, matrix=True)
        assert torch.equal(fw, wu)
        if wc is not None:
            cw, cb = R.fold(params[mods[1]], TS.EPS, matrix=True)
            assert torch.equal(cw, wc)
            fb = fb + cb
        assert torch.equal(fb, b)


@pytest.mark.parametrize("name", list(TS.SCENES))
def test_restatement_against_reference(name, golden):
    r = restate(name)
    seen = set()

    def whole(key, got):
        want = golden[key]
        got = got.numpy().reshape(want.shape)
        assert np.abs(got - want).max() <= RTOL * np.abs(want).max(), key
        seen.add(key)

    def digested(key, got):
        d, scale = TS.digest(key, got.contiguous().numpy())
        want = golden[key + "_digest"]
        assert (np.abs(d - want) <= RTOL * scale).all(), (key, np.abs((d - want) / scale).max())
        seen.add(key + "_digest")

    digested(name + "/o", r["o"])
    if name in TS.FULL_O:
        whole(name + "/o", r["o"])
    digested(name + "/gx", r["gx"])
    if r["gprev"] is not None:
        digested(name + "/gprev", r["gprev"])
    for m in TS.module_names(name):
        for kind in TS.PARAM_KINDS:
            key = "%s/%s.%s" % (name, m, kind)
            (digested if kind == "conv.weight" else whole)(key, r["unfolded"][m][kind])
    stored = {k for k in golden if k.startswith(name + "/") and not k.endswith(("/seed", "/ties"))}
    assert seen == stored, stored ^ seen                       # every stored value was held against
    assert int(golden[name + "/seed"]) == TS.SCENES[name]["seed"]


@pytest.mark.parametrize("name", list(TS.SCENES))
def test_sign_ties_are_rare(name, golden):
    assert TS.check_ties(name) <= 1e-2
    assert float(golden[name + "/ties"]) <= 1e-2              # and among the reference's own float64 values, as the generator recorded


def test_fp32_interpolation_rule_is_the_float64_rule_rounded():
    """The two weight tables of trunk_scenes.lerp_table name the same taps at every scene's sizes and differ by fp32 rounding of the
    source coordinate: at most 2^-23 * the largest source index, absolute."""
    for s in TS.SCENES.values():
        for lo, hi in ((s["hp"], s["h"]), (s["wp"], s["w"])):
            if lo == 0:
                continue
            a, b = TS.lerp_table(lo, hi, True), TS.lerp_table(lo, hi, False)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
            assert np.abs(a[3] - b[3]).max() <= 2.0 ** -23 * max(lo - 1, 1) and np.abs(a[2] - b[2]).max() <= 2.0 ** -23 * max(lo - 1, 1)
            assert (np.abs(a[2] + a[3] - 1) <= 2.0 ** -24).all()


def test_scene_pixels_span_ragged_slices():
    s = TS.SCENES["f"]
    lay = T.workspace_layout(TS.B, s["h"], s["w"], s["hp"], s["wp"], s["cin"], s["chl"], True)
    assert lay["slices"] == 11 and lay["P"] % 256 != 0 and lay["slices_lo"] == 3 and lay["Pl"] % 256 != 0
    s = TS.SCENES["e"]
    assert T.workspace_layout(TS.B, s["h"], s["w"], 0, 0, s["cin"], s["chl"], True)["slices"] == 1
    # g: long slices at high resolution (61 of 272, the last of 242, its last k-step of 16 ragged), slices of 256 at low resolution
    s = TS.SCENES["g"]
    lay = T.workspace_layout(TS.B, s["h"], s["w"], s["hp"], s["wp"], s["cin"], s["chl"], True)
    n = G.slice_len(lay["P"])
    assert lay["P"] > 16384 and n == 272 and lay["slices"] == 61 and lay["P"] % n == 242 and 242 % 16 != 0
    assert lay["slices_lo"] >= 2 and G.slice_len(lay["Pl"]) == 256 and lay["Pl"] % 256 != 0
    assert R.K_red(lay["P"]) == 333 and R.red_chain(lay["Pl"]) == 256 + lay["slices_lo"]
    # h: identity interpolation, and a quad count that is no power of two
    s = TS.SCENES["h"]
    assert s["hp"] == s["h"] and s["wp"] == s["w"] and (s["chl"] // 4) & (s["chl"] // 4 - 1) != 0
    # i: both ratios above 2, so a cell's range holds pixels whose two taps both lie strictly inside it
    s = TS.SCENES["i"]
    assert (s["h"] - 1) / (s["hp"] - 1) > 2 and (s["w"] - 1) / (s["wp"] - 1) > 2


DIMS = [(2, 2, 3, 0, 0, 64, 64), (2, 5, 7, 3, 4, 128, 64), (2, 33, 41, 17, 21, 64, 64), (1, 1, 1, 1, 1, 64, 128), (8, 128, 208, 64, 104, 256, 256),
        (8, 16, 26, 0, 0, 2048, 256), (3, 100, 171, 50, 86, 512, 192), (2, 4, 4, 16, 16, 4096, 1024),
        (2, 91, 91, 46, 46, 64, 64), (2, 4, 6, 4, 6, 192, 320), (2, 7, 10, 2, 3, 64, 64)]


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("backward", [0, 1])
def test_ws_bytes_matches_python_layout(dims, backward):
    lay = T.workspace_layout(*dims, backward)
    assert L.load().smap_trunk_ws_bytes(*dims, backward) == 4 * lay["floats"]
    assert all(lay[k] % 64 == 0 for k in lay if k in ("s", "u", "part", "colpart", "colsum", "floats"))
    if backward:
        B, h, w, hp, wp, cin, chl = dims
        assert lay["colpart"] - lay["part"] >= max(lay["slices"] * chl * cin, lay["slices_lo"] * chl * chl)      # room for chl x Cin per slice
        assert lay["slices"] <= 64 and lay["slices_lo"] <= 64


@pytest.mark.parametrize("dims", [(0, 2, 3, 0, 0, 64, 64), (70000, 2, 3, 0, 0, 64, 64), (2, 0, 3, 0, 0, 64, 64), (2, 3, 0, 0, 0, 64, 64),
                                  (2, 4097, 4097, 0, 0, 64, 64), (64, 1024, 2048, 0, 0, 64, 64), (2, 2, 3, 0, 0, 64, 0), (2, 2, 3, 0, 0, 64, 32),
                                  (2, 2, 3, 0, 0, 64, 96), (2, 2, 3, 0, 0, 64, 1088), (2, 2, 3, 0, 0, 0, 64), (2, 2, 3, 0, 0, 32, 64),
                                  (2, 2, 3, 0, 0, 100, 64), (2, 2, 3, 0, 0, 4160, 64), (2, 2, 3, 1, 0, 64, 64), (2, 2, 3, 0, 2, 64, 64),
                                  (2, 2, 3, -1, -1, 64, 64), (2, 2, 3, 4097, 4097, 64, 64), (64, 2, 3, 1024, 2048, 64, 64)])
def test_ws_bytes_rejects(dims):
    assert L.load().smap_trunk_ws_bytes(*dims, 1) == -1


VALID = (2, 5, 7, 3, 4, 128, 64)


class Args:
    """A valid argument set of both calls on fake pointers, with or without an up path; one field is broken per case."""

    def __init__(self, up=True):
        self.B, self.h, self.w, self.hp, self.wp, self.cin, self.chl = VALID if up else (2, 5, 7, 0, 0, 128, 64)
        self.valid = (self.B, self.h, self.w, self.hp, self.wp, self.cin, self.chl)
        self.x = L.HeadsX(FAKE, L.HEADS_X_F32, 128)
        self.o_prev = L.HeadsX(FAKE + 0x100000, L.HEADS_X_F32, 64) if up else None
        self.wu, self.b, self.o = FAKE + 0x200000, FAKE + 0x400000, FAKE + 0x500000
        self.wc = FAKE + 0x300000 if up else None
        self.g_o, self.gwu, self.gb = FAKE + 0x600000, FAKE + 0x700000, FAKE + 0x900000
        self.gwc, self.g_o_prev = (FAKE + 0x800000, FAKE + 0xA00000) if up else (None, None)
        self.gx, self.gx_stride = FAKE + 0xB00000, 128
        self.ws = FAKE + 0x1000000
        self.ws_bytes = None
        self.x_null = False

    def call(self, backward):
        lib = L.load()
        x = None if self.x_null else C.byref(self.x)
        prev = None if self.o_prev is None else C.byref(self.o_prev)
        need = lib.smap_trunk_ws_bytes(*self.valid, backward)              # of the VALID sizes: a broken size must be refused on its own
        ws_bytes = need if self.ws_bytes is None else self.ws_bytes(need)
        dims = (self.B, self.h, self.w, self.hp, self.wp, self.cin, self.chl)
        if backward:
            return lib.smap_trunk_backward(x, prev, self.o, self.wu, self.wc, self.g_o, self.gwu, self.gwc, self.gb, self.g_o_prev, self.gx,
                                           self.gx_stride, *dims, self.ws, ws_bytes, None)
        return lib.smap_trunk_forward(x, prev, self.wu, self.wc, self.b, self.o, *dims, self.ws, ws_bytes, None)


def _dims(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


BOTH = {
    "x null": _set("x_null", True), "x ptr null": _d("x", ptr=None), "x misaligned": _d("x", ptr=FAKE + 8), "x layout": _d("x", layout=3),
    "x stride below cin": _d("x", pix_stride=124), "x stride not 4n": _d("x", pix_stride=130),
    "x f16 misaligned": _d("x", ptr=FAKE + 4, layout=L.HEADS_X_F16), "x hilo stride below 2 cin": _d("x", layout=L.HEADS_X_F16_HILO, pix_stride=128),
    "o_prev ptr null": _d("o_prev", ptr=None), "o_prev misaligned": _d("o_prev", ptr=FAKE + 0x100008), "o_prev layout": _d("o_prev", layout=-1),
    "o_prev stride below chl": _d("o_prev", pix_stride=60), "o_prev hilo stride below 2 chl": _d("o_prev", layout=L.HEADS_X_F16_HILO, pix_stride=64),
    "o_prev null with wc": _set("o_prev", None), "o_prev without wc": _set("wc", None), "o_prev without hp wp": _dims(hp=0, wp=0),
    "wu null": _set("wu", None), "wu misaligned": _set("wu", FAKE + 2), "wc misaligned": _set("wc", FAKE + 0x300001),
    "o null": _set("o", None), "o misaligned": _set("o", FAKE + 0x500004),
    "B 0": _dims(B=0), "h 0": _dims(h=0), "w negative": _dims(w=-7), "hp 0": _dims(hp=0), "wp negative": _dims(wp=-4),
    "chl 0": _dims(chl=0), "chl 96": _dims(chl=96), "chl 32": _dims(chl=32), "chl 2048": _dims(chl=2048),
    "cin 0": _dims(cin=0), "cin 96": _dims(cin=96), "cin 32": _dims(cin=32), "cin 8192": _dims(cin=8192),
    "P above 2^26": _dims(B=65, h=1024, w=1024), "P' above 2^26": _dims(B=65, hp=1024, wp=1024),
    "ws null": _set("ws", None), "ws misaligned": _set("ws", FAKE + 0x1000000 + 128), "ws small": _set("ws_bytes", lambda n: n - 1),
    "ws negative": _set("ws_bytes", lambda n: -n),
}
FORWARD = {"b null": _set("b", None), "b misaligned": _set("b", FAKE + 0x400004)}
BACKWARD = {
    "g_o null": _set("g_o", None), "g_o misaligned": _set("g_o", FAKE + 0x600008), "gwu null": _set("gwu", None),
    "gwu misaligned": _set("gwu", FAKE + 0x700002), "gb null": _set("gb", None), "gb misaligned": _set("gb", FAKE + 0x900001),
    "gwc null": _set("gwc", None), "gwc misaligned": _set("gwc", FAKE + 0x800002), "g_o_prev null": _set("g_o_prev", None),
    "g_o_prev misaligned": _set("g_o_prev", FAKE + 0xA00003), "gx misaligned": _set("gx", FAKE + 0xB00002), "gx stride below cin": _set("gx_stride", 127),
    "ws of the forward size": _set("ws_bytes", lambda n: L.load().smap_trunk_ws_bytes(*VALID, 0)),
}
# the coarsest unit: nothing of the up path may be given
NO_UP_BOTH = {"wc given": _set("wc", FAKE + 0x300000), "hp wp given": _dims(hp=3, wp=4)}
NO_UP_BACKWARD = {"gwc given": _set("gwc", FAKE + 0x800000), "g_o_prev given": _set("g_o_prev", FAKE + 0xA00000)}


def test_valid_sizes_are_accepted_by_ws_bytes():
    """The cases above break ONE thing each: the unbroken sets are in range."""
    assert L.load().smap_trunk_ws_bytes(*VALID, 1) > L.load().smap_trunk_ws_bytes(*VALID, 0) > 0
    assert L.load().smap_trunk_ws_bytes(2, 5, 7, 0, 0, 128, 64, 1) > 0


@pytest.mark.parametrize("case", list(BOTH) + list(FORWARD))
def test_forward_rejects(case):
    a = Args()
    (BOTH.get(case) or FORWARD[case])(a)
    assert a.call(0) == -1


@pytest.mark.parametrize("case", list(BOTH) + list(BACKWARD))
def test_backward_rejects(case):
    a = Args()
    (BOTH.get(case) or BACKWARD[case])(a)
    assert a.call(1) == -1


@pytest.mark.parametrize("case", list(NO_UP_BOTH))
@pytest.mark.parametrize("backward", [0, 1])
def test_no_up_path_rejects_up_arguments(case, backward):
    a = Args(up=False)
    NO_UP_BOTH[case](a)
    assert a.call(backward) == -1


@pytest.mark.parametrize("case", list(NO_UP_BACKWARD))
def test_no_up_path_backward_rejects_up_gradients(case):
    a = Args(up=False)
    NO_UP_BACKWARD[case](a)
    assert a.call(1) == -1


def test_parameter_keys():
    keys = F.trunk_parameter_keys(2)
    assert len(keys) == 28 and len(set(keys)) == 28
    assert keys[0] == "stage2.upsample.up1.u_skip.conv.weight" and "stage2.upsample.up1.up_conv.conv.weight" not in keys
    assert "stage2.upsample.up4.up_conv.bn.bias" in keys
