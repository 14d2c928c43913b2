"""Scenes of the Upsample_unit trunk tests (smap_amd/trunk.py, csrc/trunk.hip): one unit's input X, the coarser unit's out O_prev, the
unit's u_skip and up_conv with recipe weights BY KEY, and an upstream gradient G at the unit's out.  Shared by gen_golden_trunk.py
(which runs the reference's module on them) and the tests, so it imports neither the reference nor this repository's package: numpy,
torch and the weight recipe only.

    scene  ind  low -> high          Cin   chl   what it exercises
    a      0    2x3                   64    64   no up path; every pixel a border
    b      1    3x4 -> 5x7           128    64   non-integer ratio, ragged tiles
    c      2    1x5 -> 2x9            64    64   a height-1 source
    d      3    8x12 -> 16x24        256   256   the small network's up4
    e      0    2x3                 2048   256   longest K, widest N, one slice
    f      2    17x21 -> 33x41        64    64   eleven reduction slices, the last ragged
    g      3    46x46 -> 91x91        64    64   16562 pixels: 61 slices of 272 (the last of 242) on gWu and gb; 17 of 256 on gWc
    h      1    4x6 -> 4x6           192   320   identity interpolation; 80 channel quads, no power of two; ragged 128-wide column tiles
    i      2    2x3 -> 7x10           64    64   ratios 3.5 and 3.33: many pixels inside one cell's range, one-sided ranges at the border

X and O_prev are drawn post-ReLU: relu(N(0, 1)).  G ~ N(0, 1) * 3e-7, as loss gradients are.

ReLU sign ties: an element of the pre-activation pre = S + I(U) + b whose float64 value lies within
    (Cin + chl + 6) * 2^-24 * (sum |x||wu| + I(sum |o_prev||wc|) + |b|)
of zero; there the fp32 mask O > 0 may differ from float64's.  CONDITION on every committed seed, asserted by check_ties() and, on the
reference's own float64 values, by the generator: ties are at most 1 % of the scene's elements.  A seed that fails is replaced; the cap
is not loosened.
"""
import numpy as np
import torch

from heads_scenes import digest  # noqa: F401  (the golden file's digests are heads_scenes.digest)
from recipe import recipe_state_dict

B = 2
EPS = 1e-5
G_SCALE = 3e-7
TIE_CAP = 1e-2
U = 2.0 ** -24

SCENES = {
    "a": dict(ind=0, h=2, w=3, hp=0, wp=0, cin=64, chl=64, unit="stage2.upsample.up1", seed=201),
    "b": dict(ind=1, h=5, w=7, hp=3, wp=4, cin=128, chl=64, unit="stage2.upsample.up2", seed=202),
    "c": dict(ind=2, h=2, w=9, hp=1, wp=5, cin=64, chl=64, unit="stage2.upsample.up3", seed=203),
    "d": dict(ind=3, h=16, w=24, hp=8, wp=12, cin=256, chl=256, unit="stage2.upsample.up4", seed=204),
    "e": dict(ind=0, h=2, w=3, hp=0, wp=0, cin=2048, chl=256, unit="stage2.upsample.up1", seed=205),
    "f": dict(ind=2, h=33, w=41, hp=17, wp=21, cin=64, chl=64, unit="stage2.upsample.up3", seed=206),
    "g": dict(ind=3, h=91, w=91, hp=46, wp=46, cin=64, chl=64, unit="stage2.upsample.up4", seed=207),
    "h": dict(ind=1, h=4, w=6, hp=4, wp=6, cin=192, chl=320, unit="stage2.upsample.up2", seed=208),
    "i": dict(ind=2, h=7, w=10, hp=2, wp=3, cin=64, chl=64, unit="stage2.upsample.up3", seed=209),
}
FULL_O = ("a", "b", "c")                     # scenes whose out tensor the golden file keeps whole
PARAM_KINDS = ("conv.weight", "conv.bias", "bn.weight", "bn.bias")
STATS = ("bn.running_mean", "bn.running_var")


def module_names(name):
    """The scene's trunk modules: u_skip, and up_conv where there is an up path."""
    s = SCENES[name]
    return [s["unit"] + ".u_skip"] + ([s["unit"] + ".up_conv"] if s["ind"] > 0 else [])


def weights(name):
    """state_dict key -> fp32 tensor of the trunk modules, from the recipe (seeded by key, shaped as the reference's modules are)."""
    s = SCENES[name]
    shapes = {}
    for m, cin in zip(module_names(name), (s["cin"], s["chl"])):
        shapes[m + ".conv.weight"] = torch.empty((s["chl"], cin, 1, 1))
        for k in ("conv.bias", "bn.weight", "bn.bias") + STATS:
            shapes["%s.%s" % (m, k)] = torch.empty(s["chl"])
    return recipe_state_dict(shapes)


def inputs(name):
    """X [B, h, w, cin], O_prev [B, hp, wp, chl] or None, G [B, h, w, chl]: fp32 numpy."""
    s = SCENES[name]
    rng = np.random.default_rng(s["seed"])
    x = np.maximum(rng.standard_normal((B, s["h"], s["w"], s["cin"])), 0.0).astype(np.float32)
    o_prev = None
    if s["ind"] > 0:
        o_prev = np.maximum(rng.standard_normal((B, s["hp"], s["wp"], s["chl"])), 0.0).astype(np.float32)
    g = (rng.standard_normal((B, s["h"], s["w"], s["chl"])) * G_SCALE).astype(np.float32)
    return x, o_prev, g


def folded64(name):
    """wu [chl, cin], wc [chl, chl] or None, b = bu + bc in float64: eval-mode BN folded into the conv before it."""
    sd = {k: v.double() for k, v in weights(name).items()}

    def one(p):
        s = sd[p + ".bn.weight"] / torch.sqrt(sd[p + ".bn.running_var"] + EPS)
        return (sd[p + ".conv.weight"] * s.view(-1, 1, 1, 1)).flatten(1), (sd[p + ".conv.bias"] - sd[p + ".bn.running_mean"]) * s + sd[p + ".bn.bias"]
    mods = module_names(name)
    wu, b = one(mods[0])
    wc = None
    if len(mods) > 1:
        wc, bc = one(mods[1])
        b = b + bc
    return wu, wc, b


def lerp_table(in_size, out_size, fp32):
    """ATen's bilinear align_corners index and weight rule per output index: (i0, i1, l0, l1), the weights as float64 values.
    fp32: computed as the fp32 kernels compute them (csrc/plan.h lerp_index), each operation rounded to fp32; else in float64, as
    F.interpolate computes them on a float64 tensor."""
    f = np.float32 if fp32 else np.float64
    dst = np.arange(out_size)
    if in_size == out_size:
        return dst, dst.copy(), np.ones(out_size), np.zeros(out_size)
    scale = f(in_size - 1) / f(out_size - 1) if out_size > 1 else f(0)
    src = (scale * dst.astype(f)).astype(f)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < in_size - 1)
    l1 = np.clip((src - i0.astype(f)).astype(f), f(0), f(1))
    l0 = (f(1) - l1).astype(f)
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def lerp_matrix(in_size, out_size, fp32):
    """[out_size, in_size] float64: row d holds l0 at i0 and l1 at i1 (added where the two name the same index)."""
    i0, i1, l0, l1 = lerp_table(in_size, out_size, fp32)
    m = np.zeros((out_size, in_size))
    np.add.at(m, (np.arange(out_size), i0), l0)
    np.add.at(m, (np.arange(out_size), i1), l1)
    return torch.from_numpy(m)


def interp(u, h, w, fp32):
    """I(u): [B, hp, wp, c] float64 -> [B, h, w, c]."""
    my, mx = lerp_matrix(u.shape[1], h, fp32), lerp_matrix(u.shape[2], w, fp32)
    return torch.einsum("yi,xj,bijc->byxc", my, mx, u)


def ties(name, x=None, o_prev=None, wu=None, wc=None, b=None, fp32=True):
    """(tie mask [B, h, w, chl], pre float64) of the scene -- or of the given fp32-valued operands."""
    s = SCENES[name]
    if x is None:
        x_np, p_np, _ = inputs(name)
        x, o_prev = torch.from_numpy(x_np), (None if p_np is None else torch.from_numpy(p_np))
    if wu is None:
        wu, wc, b = (None if t is None else t.float() for t in folded64(name))     # the kernel's operands: the fp32 roundings of the folded weights
    x, wu, b = x.double(), wu.double(), b.double()
    pre, mag = x @ wu.T + b, x.abs() @ wu.abs().T + b.abs()
    if o_prev is not None:
        o_prev, wc = o_prev.double(), wc.double()
        pre = pre + interp(o_prev @ wc.T, s["h"], s["w"], fp32)
        mag = mag + interp(o_prev.abs() @ wc.abs().T, s["h"], s["w"], fp32)
    return pre.abs() <= (s["cin"] + s["chl"] + 6) * U * mag, pre


def check_ties(name):
    """The condition of this file's docstring; returns the scene's tie fraction."""
    tie, _ = ties(name)
    frac = float(tie.double().mean())
    assert frac <= TIE_CAP, (name, frac)
    return frac


if __name__ == "__main__":
    for n in SCENES:
        print(n, "tie fraction %.5f %%" % (100 * check_ties(n)))
