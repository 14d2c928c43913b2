"""Scenes of the head-arm tests (smap_amd/heads.py, csrc/heads.hip): one Upsample_unit's `out` tensor X, the unit's six head convs with
recipe weights BY KEY, and upstream gradients G_a.  Shared by gen_golden_heads.py (which runs the reference's modules on them) and the
tests, so it imports neither the reference nor this repository's package: numpy, torch and the weight recipe only.

Shapes are the smallest at which each thing can still go wrong: 2x3 (every pixel is border), 5x7 (odd, 70 pixels: a ragged tile in both
kernels), 16x24 (the small network's finest level, 768 pixels: three reduction slices), 33x41 (2706 pixels: eleven slices of 256, the
last of 146), 91x91 (16562 pixels, above the 16384 up to which a slice has 256: 61 slices of 272, the last of 242, whose last k-step
of 16 holds 2), 9x15 at chl 320 (two column tiles of 256 times nine taps in gW2; ragged 128-wide tiles at N = 960 and 320).  chl 64, 256
and 320; C = (43, 14, 1); B = 2.

X is drawn post-ReLU: relu(N(0, 1)), about half of it zero.  G_a ~ N(0, 1) * g_scale with g_scale = 3e-7: most of it below fp16's
smallest normal number (6.1e-5) and a good part below its smallest subnormal (6e-8), as loss gradients are.

ReLU sign ties: an element of Z whose float64 value lies within the fp32 forward's own error bound of zero,
|Z| <= (chl + 2) * 2^-24 * (sum |x||w| + |b|); there the kernel's mask may differ from float64's.  CONDITION on every committed seed,
asserted by check_ties() (tests/test_heads_cpu.py runs it): ties are at most 0.1 % of the scene's Z elements.  A seed that fails is
replaced; the cap is not loosened.
"""
import zlib

import numpy as np
import torch

from recipe import recipe_state_dict

B = 2
ARM_C = (43, 14, 1)
ARMS = ("res", "res_d", "res_rd")
EPS = 1e-5                                 # nn.BatchNorm2d's default, what the reference's conv_bn_relu uses
G_SCALE = 3e-7
TIE_CAP = 1e-3
U = 2.0 ** -24

SCENES = {
    "b2x3": dict(h=2, w=3, chl=64, unit="stage0.upsample.up1", seed=101),
    "o5x7": dict(h=5, w=7, chl=64, unit="stage1.upsample.up2", seed=102),
    "o5x7w": dict(h=5, w=7, chl=256, unit="stage2.upsample.up1", seed=103),
    "f16x24": dict(h=16, w=24, chl=256, unit="stage2.upsample.up4", seed=104),
    "s33x41": dict(h=33, w=41, chl=64, unit="stage0.upsample.up3", seed=105),
    "l91x91": dict(h=91, w=91, chl=64, unit="stage1.upsample.up4", seed=106),
    "w9x15": dict(h=9, w=15, chl=320, unit="stage2.upsample.up2", seed=107),
}
FULL_Y = ("b2x3", "o5x7", "o5x7w")           # scenes whose head tensors the golden file keeps whole
PARAM_KINDS = ("conv.weight", "conv.bias", "bn.weight", "bn.bias")       # what is trained; the running statistics stay frozen


def module_names(name):
    """The six conv_bn_relu modules of the scene's unit, arm after arm: conv1, conv2."""
    u = SCENES[name]["unit"]
    return [("%s.%s_conv1" % (u, a), "%s.%s_conv2" % (u, a)) for a in ARMS]


def weights(name):
    """state_dict key -> fp32 tensor for the six modules, from the recipe (seeded by key, shaped as the reference's modules are)."""
    chl = SCENES[name]["chl"]
    shapes = {}
    for (c1, c2), c in zip(module_names(name), ARM_C):
        for p, shape in ((c1, (chl, chl, 1, 1)), (c2, (c, chl, 3, 3))):
            shapes[p + ".conv.weight"] = torch.empty(shape)
            for k in ("conv.bias", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var"):
                shapes["%s.%s" % (p, k)] = torch.empty(shape[0])
    return recipe_state_dict(shapes)


def inputs(name):
    """X [B, h, w, chl] and G_a [B, C_a, h, w], fp32 numpy."""
    s = SCENES[name]
    rng = np.random.default_rng(s["seed"])
    x = np.maximum(rng.standard_normal((B, s["h"], s["w"], s["chl"])), 0.0).astype(np.float32)
    g = [(rng.standard_normal((B, c, s["h"], s["w"])) * G_SCALE).astype(np.float32) for c in ARM_C]
    return x, g


def folded64(name):
    """w1cat [3 chl, chl], b1cat, [w2_a], [b2_a] in float64: eval-mode BN folded into the conv before it."""
    sd = {k: v.double() for k, v in weights(name).items()}

    def one(p):
        s = sd[p + ".bn.weight"] / torch.sqrt(sd[p + ".bn.running_var"] + EPS)
        return sd[p + ".conv.weight"] * s.view(-1, 1, 1, 1), (sd[p + ".conv.bias"] - sd[p + ".bn.running_mean"]) * s + sd[p + ".bn.bias"]
    w1, b1, w2, b2 = [], [], [], []
    for c1, c2 in module_names(name):
        w, b = one(c1)
        w1.append(w.flatten(1)), b1.append(b)
        w, b = one(c2)
        w2.append(w), b2.append(b)
    return torch.cat(w1), torch.cat(b1), w2, b2


def ties(name, x=None, w1cat=None, b1cat=None):
    """(tie mask [B, h, w, 3 chl], Z float64) of the scene -- or of the given fp32-valued X and folded 1x1 weights."""
    if x is None:
        x = torch.from_numpy(inputs(name)[0])
    if w1cat is None:
        w1cat, b1cat = (t.float() for t in folded64(name)[:2])       # the kernel's operands are the fp32 roundings of the folded weights
    x, w, b = x.double(), w1cat.double(), b1cat.double()
    z = x @ w.T + b
    mag = x.abs() @ w.abs().T + b.abs()
    return z.abs() <= (x.shape[-1] + 2) * U * mag, z


def check_ties(name):
    """The condition of this file's docstring; returns the scene's tie fraction."""
    tie, _ = ties(name)
    frac = float(tie.double().mean())
    assert frac <= TIE_CAP, (name, frac)
    return frac


N_SAMPLES, N_PROJ = 256, 3


def digest(key, a, n_samples=N_SAMPLES):
    """What the golden file keeps of a large float64 tensor: its sum, the sum of its magnitudes, N_PROJ seeded Gaussian projections and
    n_samples seeded sample positions -- as (digest [2 + N_PROJ + n_samples], scale [same], the tolerance unit of every entry: max |a|
    for a sample, sum |a| for the sum, sum |a| * max |v| for a projection).  The samples are digest[2 + N_PROJ:]."""
    a = np.asarray(a, np.float64).ravel()
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    proj = rng.standard_normal((N_PROJ, a.size))
    pos = rng.integers(0, a.size, n_samples)
    mag = np.abs(a).sum()
    d = np.concatenate([[a.sum(), mag], proj @ a, a[pos]])
    scale = np.concatenate([[mag, mag], mag * np.abs(proj).max(axis=1), np.full(n_samples, np.abs(a).max())])
    return d, scale


if __name__ == "__main__":
    for n in SCENES:
        print(n, "tie fraction %.5f %%" % (100 * check_ties(n)))
