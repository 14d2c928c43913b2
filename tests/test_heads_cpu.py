"""Head arms without a GPU: the float64 restatement (tests/heads_restate.py) against the reference's recorded results
(tests/golden/heads.npz, gen_golden_heads.py), the sign-tie condition of the scenes, the workspace layout, and the argument checks of
smap_heads_ws_bytes / smap_heads_forward / smap_heads_backward -- which all happen before any HIP call, so fake pointers serve."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import heads_restate as R
import heads_scenes as HS
import smap_amd.lib as L
from smap_amd import gemm_f32 as G
from smap_amd import heads as H
from train_kit import FAKE, set_attr as _set, set_fields as _d

RTOL = 1e-12           # of the tensor's largest magnitude: both sides are float64 and differ in summation order only


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "heads.npz")))


@pytest.fixture(scope="module")
def restated():
    """Per scene: the restatement's Y_a, gX and the gradients at the unfolded parameters, float64, computed once."""
    out = {}
    for name in HS.SCENES:
        x_np, g_np = HS.inputs(name)
        x, g = torch.from_numpy(x_np).double(), [torch.from_numpy(a).double() for a in g_np]
        sd = {k: v.double() for k, v in HS.weights(name).items()}
        mods = HS.module_names(name)
        params = {m: {k: sd["%s.%s" % (m, k)] for k in HS.PARAM_KINDS + ("bn.running_mean", "bn.running_var")} for pair in mods for m in pair}
        folded = {m: R.fold(p, HS.EPS) for m, p in params.items()}
        w1cat = torch.cat([folded[c1][0].flatten(1) for c1, _ in mods])
        b1cat = torch.cat([folded[c1][1] for c1, _ in mods])
        w2, b2 = [folded[c2][0] for _, c2 in mods], [folded[c2][1] for _, c2 in mods]
        z, ys = R.forward(x, w1cat, b1cat, w2, b2)
        gr = R.backward(x, w1cat, w2, g, z)
        chl = x.shape[-1]
        unfolded = {}
        for a, (c1, c2) in enumerate(mods):
            unfolded[c1] = R.unfold_grads(params[c1], gr["gw1"][a * chl:(a + 1) * chl], gr["gb1"][a * chl:(a + 1) * chl], HS.EPS)
            unfolded[c2] = R.unfold_grads(params[c2], gr["gw2"][a], gr["gb2"][a], HS.EPS)
        out[name] = dict(y=ys, gx=gr["gx"], unfolded=unfolded)
    return out


def test_scene_fold_matches_restatement():
    for name in HS.SCENES:
        sd = {k: v.double() for k, v in HS.weights(name).items()}
        w1cat, b1cat, w2, b2 = HS.folded64(name)
        for a, (c1, c2) in enumerate(HS.module_names(name)):
            chl = HS.SCENES[name]["chl"]
            for m, w, b in ((c1, w1cat[a * chl:(a + 1) * chl], b1cat[a * chl:(a + 1) * chl]), (c2, w2[a], b2[a])):
                p = {k: sd["%s.%s" % (m, k)] for k in HS.PARAM_KINDS + ("bn.running_mean", "bn.running_var")}
                fw, fb = R.fold(p, HS.EPS)
                assert torch.equal(fw.flatten(1), w.flatten(1)) and torch.equal(fb, b)


@pytest.mark.parametrize("name", list(HS.SCENES))
def test_restatement_against_reference(name, golden, restated):
    r = restated[name]
    seen = set()

    def whole(key, got):
        want = golden[key]
        got = got.numpy().reshape(want.shape)
        assert np.abs(got - want).max() <= RTOL * np.abs(want).max(), key
        seen.add(key)

    def digested(key, got):
        d, scale = HS.digest(key, got.contiguous().numpy())
        want = golden[key + "_digest"]
        assert (np.abs(d - want) <= RTOL * scale).all(), (key, np.abs((d - want) / scale).max())
        seen.add(key + "_digest")

    for a in range(3):
        digested("%s/y%d" % (name, a), r["y"][a])
        if name in HS.FULL_Y:
            whole("%s/y%d" % (name, a), r["y"][a])
    digested(name + "/gx", r["gx"])
    for pair in HS.module_names(name):
        for m in pair:
            for kind in HS.PARAM_KINDS:
                key = "%s/%s.%s" % (name, m, kind)
                (digested if kind == "conv.weight" else whole)(key, r["unfolded"][m][kind])
    stored = {k for k in golden if k.startswith(name + "/") and not k.endswith("/seed")}
    assert seen == stored, stored ^ seen                       # every stored value was held against
    assert int(golden[name + "/seed"]) == HS.SCENES[name]["seed"]


@pytest.mark.parametrize("name", list(HS.SCENES))
def test_sign_ties_are_rare(name):
    assert HS.check_ties(name) <= 1e-3


def test_scene_pixels_span_ragged_slices():
    s = HS.SCENES["s33x41"]
    P = HS.B * s["h"] * s["w"]
    lay = H.workspace_layout(HS.B, s["h"], s["w"], s["chl"], True)
    assert lay["slices"] >= 3 and P % lay["slice_len"] != 0 and P % 128 != 0 and P % 256 != 0
    # l91x91: above the 16384 pixels up to which a slice has 256 -- 61 slices of 272, the last of 242, whose last k-step of 16 is ragged
    s = HS.SCENES["l91x91"]
    P = HS.B * s["h"] * s["w"]
    lay = H.workspace_layout(HS.B, s["h"], s["w"], s["chl"], True)
    assert P > 16384 and lay["slice_len"] == 272 and lay["slices"] == 61 and P % lay["slice_len"] == 242 and 242 % 16 != 0 and P % 128 != 0
    assert R.K_red(P) == 272 + 61 and R.red_chain(P) == 333 and R.red_chain(70) == 70 and R.red_chain(2706) == 256 + 11
    # w9x15: more than one 256-wide column tile beside the nine taps of gW2, and more than one slice
    s = HS.SCENES["w9x15"]
    assert s["chl"] > 256 and H.workspace_layout(HS.B, s["h"], s["w"], s["chl"], True)["slices"] >= 2


@pytest.mark.parametrize("dims", [(2, 2, 3, 64), (2, 5, 7, 256), (2, 33, 41, 64), (1, 1, 1, 128), (8, 128, 208, 256), (3, 100, 171, 192),
                                  (2, 91, 91, 64), (2, 9, 15, 320)])
@pytest.mark.parametrize("backward", [0, 1])
def test_ws_bytes_matches_python_layout(dims, backward):
    B, h, w, chl = dims
    lay = H.workspace_layout(B, h, w, chl, backward)
    assert L.load().smap_heads_ws_bytes(B, h, w, chl, backward) == 4 * lay["floats"]
    assert lay["slices"] * lay["slice_len"] >= lay["P"] > (lay["slices"] - 1) * lay["slice_len"] and lay["slices"] <= 64
    assert all(lay[k] % 64 == 0 for k in lay if k in ("m", "gz", "part", "colpart", "floats"))


@pytest.mark.parametrize("dims", [(0, 2, 3, 64), (70000, 2, 3, 64), (2, 0, 3, 64), (2, 3, 0, 64), (2, 4097, 4097, 64), (64, 1024, 2048, 64),
                                  (2, 2, 3, 0), (2, 2, 3, 32), (2, 2, 3, 96), (2, 2, 3, 65), (2, 2, 3, 1088)])
def test_ws_bytes_rejects(dims):
    assert L.load().smap_heads_ws_bytes(*dims, 1) == -1


class Args:
    """A valid argument set of both calls on fake pointers; one field is broken per case."""

    def __init__(self):
        self.B, self.h, self.w, self.chl = 2, 5, 7, 64
        self.x = L.HeadsX(FAKE, L.HEADS_X_F32, 64)
        self.w1, self.b1 = FAKE + 0x100000, FAKE + 0x200000
        self.w2 = [FAKE + 0x300000 + 0x10000 * a for a in range(3)]
        self.b2 = [FAKE + 0x400000 + 0x10000 * a for a in range(3)]
        px = self.h * self.w
        self.heads = [[FAKE + 0x500000 + 0x100000 * a, self.h, self.w, c, 1, px, c * px] for a, c in enumerate(HS.ARM_C)]
        self.gw1, self.gb1 = FAKE + 0x900000, FAKE + 0xA00000
        self.gw2 = [FAKE + 0xB00000 + 0x10000 * a for a in range(3)]
        self.gb2 = [FAKE + 0xC00000 + 0x10000 * a for a in range(3)]
        self.gx, self.gx_stride = FAKE + 0xD00000, 64
        self.ws = FAKE + 0x1000000
        self.ws_bytes = None
        self.null = set()                    # names of the pointer arrays / structs passed as null

    def ptrs(self, name):
        return None if name in self.null else (C.c_void_p * 3)(*getattr(self, name))

    def call(self, backward):
        lib = L.load()
        heads = None if "heads" in self.null else (L.HeadSrc * 3)(*[L.HeadSrc(p, h, w, c, pix, ch, 0, fr) for p, h, w, c, pix, ch, fr in self.heads])
        x = None if "x" in self.null else C.byref(self.x)
        need = lib.smap_heads_ws_bytes(2, 5, 7, 64, backward)            # of the VALID sizes: a broken size must be refused on its own
        ws_bytes = need if self.ws_bytes is None else self.ws_bytes(need)
        if backward:
            return lib.smap_heads_backward(x, self.w1, self.b1, self.ptrs("w2"), heads, self.B, self.h, self.w, self.chl, self.gw1, self.gb1,
                                           self.ptrs("gw2"), self.ptrs("gb2"), self.gx, self.gx_stride, self.ws, ws_bytes, None)
        return lib.smap_heads_forward(x, self.w1, self.b1, self.ptrs("w2"), self.ptrs("b2"), heads, self.B, self.h, self.w, self.chl, self.ws,
                                      ws_bytes, None)


def _item(name, i, value):
    return lambda a: getattr(a, name).__setitem__(i, value)


def _head(i, field, value):
    return lambda a: a.heads[i].__setitem__(field, value)


BOTH = {
    "x null": lambda a: a.null.add("x"), "x ptr null": _d("x", ptr=None), "x misaligned": _d("x", ptr=FAKE + 8), "x layout": _d("x", layout=3),
    "x stride below chl": _d("x", pix_stride=60), "x stride not 4n": _d("x", pix_stride=66),
    "x f16 misaligned": _d("x", ptr=FAKE + 4, layout=L.HEADS_X_F16), "x hilo stride below 2 chl": _d("x", layout=L.HEADS_X_F16_HILO, pix_stride=64),
    "w1 null": _set("w1", None), "w1 misaligned": _set("w1", FAKE + 2), "b1 null": _set("b1", None),
    "w2 null": lambda a: a.null.add("w2"), "w2[1] null": _item("w2", 1, None), "w2[2] misaligned": _item("w2", 2, FAKE + 1),
    "heads null": lambda a: a.null.add("heads"), "head ptr null": _head(0, 0, None), "head misaligned": _head(1, 0, FAKE + 2),
    "head h": _head(0, 1, 4), "head w": _head(2, 2, 8), "head c 0": _head(2, 3, 0), "head c 65": _head(0, 3, 65),
    "head pix stride 0": _head(0, 4, 0), "head ch stride below pixels": _head(0, 5, 34), "head frame stride": _head(1, 6, 14 * 35 - 1),
    "head nhwc stride below c": lambda a: a.heads.__setitem__(0, [FAKE + 0x500000, 5, 7, 43, 40, 1, 35 * 40]),
    "B 0": _set("B", 0), "h 0": _set("h", 0), "w negative": _set("w", -7), "chl 0": _set("chl", 0), "chl 96": _set("chl", 96),
    "chl 32": _set("chl", 32), "chl 2048": _set("chl", 2048),
    "ws null": _set("ws", None), "ws misaligned": _set("ws", FAKE + 0x1000000 + 128), "ws small": _set("ws_bytes", lambda n: n - 1),
    "ws negative": _set("ws_bytes", lambda n: -n),
}
FORWARD = {"b2 null": lambda a: a.null.add("b2"), "b2[0] null": _item("b2", 0, None), "b2[1] misaligned": _item("b2", 1, FAKE + 3)}
BACKWARD = {
    "gw1 null": _set("gw1", None), "gb1 null": _set("gb1", None), "gb1 misaligned": _set("gb1", FAKE + 1),
    "gw2 null": lambda a: a.null.add("gw2"), "gw2[0] null": _item("gw2", 0, None), "gb2 null": lambda a: a.null.add("gb2"),
    "gb2[2] null": _item("gb2", 2, None), "gx misaligned": _set("gx", FAKE + 2), "gx stride below chl": _set("gx_stride", 63),
    "ws of the forward size": _set("ws_bytes", lambda n: L.load().smap_heads_ws_bytes(2, 5, 7, 64, 0)),
}


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


def test_fold_bn_is_the_restatement_fold_and_differentiable():
    name = "o5x7"
    sd = {k: v.double() for k, v in HS.weights(name).items()}
    m = HS.module_names(name)[1][1]
    p = {k: sd["%s.%s" % (m, k)].clone().requires_grad_(k in HS.PARAM_KINDS) for k in HS.PARAM_KINDS + ("bn.running_mean", "bn.running_var")}
    w, b = G.fold_bn(p["conv.weight"], p["conv.bias"], p["bn.weight"], p["bn.bias"], p["bn.running_mean"], p["bn.running_var"], HS.EPS)
    rw, rb = R.fold({k: v.detach() for k, v in p.items()}, HS.EPS)
    assert torch.allclose(w, rw, rtol=1e-15, atol=0) and torch.allclose(b, rb, rtol=1e-15, atol=0)
    gen = torch.Generator().manual_seed(5)
    gw, gb = torch.randn(w.shape, generator=gen, dtype=torch.float64), torch.randn(b.shape, generator=gen, dtype=torch.float64)
    ((w * gw).sum() + (b * gb).sum()).backward()
    want = R.unfold_grads({k: v.detach() for k, v in p.items()}, gw, gb, HS.EPS)
    for kind in HS.PARAM_KINDS:
        assert torch.allclose(p[kind].grad, want[kind], rtol=1e-12, atol=1e-14), kind
    assert p["bn.running_mean"].grad is None and p["bn.running_var"].grad is None
