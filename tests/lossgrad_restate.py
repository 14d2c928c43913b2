"""A numpy restatement of the loss gradient at the heads' native resolution (include/smap_hip.h smap_loss_backward_src): float64
arithmetic on the fp32 inputs, the align-corners index rule in float32 exactly as csrc/plan.h lerp_index writes it.  No product code is
imported.  The loss tests compare the kernels with this, and this with the reference's autograd (tests/golden/lossgrad.npz).

    up       = Wy @ source @ Wx^T             Wy [H, h]: row y holds l0(y) at i0(y) plus l1(y) at i1(y) (both at the last source row)
    e        = (up - label) * f               f = coef * upstream
    gradient = Wy^T @ e @ Wx

`variant` names a deliberately wrong restatement (the negative controls of tests/test_lossgrad_cpu.py)."""
import numpy as np

NKP, NPAF, N2D, NDD, NC = 15, 28, 43, 14, 57
LABEL_CHANNEL = list(range(NKP)) + [NKP + 3 * (c // 2) + c % 2 for c in range(NPAF)] + [NKP + 3 * c + 2 for c in range(NDD)]
F32 = np.float32


def lerp_index(n_in, n_out):
    """(i0, i1 int arrays, l0, l1 float32 arrays) over dst = 0 .. n_out - 1: lerp_index of csrc/plan.h, operation by operation."""
    dst = np.arange(n_out)
    if n_in == n_out:
        return dst, dst.copy(), np.ones(n_out, F32), np.zeros(n_out, F32)
    scale = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    src = (scale * dst.astype(F32)).astype(F32)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = np.clip((src - i0.astype(F32)).astype(F32), F32(0), F32(1))
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0, l1


def weights(n_in, n_out, variant=None):
    """float64 [n_out, n_in]: the weight of output index y on source index i."""
    i0, i1, l0, l1 = lerp_index(n_in, n_out)
    w = np.zeros((n_out, n_in))
    for y in range(n_out):
        w[y, i0[y]] += float(l0[y])
        if variant == "drop_l1_at_last" and i0[y] == i1[y]:
            continue
        if variant == "drop_l1_into_last" and i1[y] == n_in - 1 and n_in not in (1, n_out):
            continue
        w[y, i1[y]] += float(l0[y] if variant == "l0_both" else l1[y])
    return w


def upsample(src, H, W):
    """[..., h, w] -> [..., H, W] in float64."""
    return weights(src.shape[-2], H) @ src.astype(np.float64) @ weights(src.shape[-1], W).T


def head_scale(s, h):
    return h % 4 + (1 if h // 4 == s["stage_num"] - 1 and s["ctf"] else 0)


def forward(s, x):
    """The loss of scene parameters s on inputs x (lossgrad_scenes.inputs): dict(losses [4], coef [n_heads, B, 57] with d total / d up =
    coef * (up - label), diff: per head up - label [B, 57, H, W], root: per head the list of (b, y, x, factor) with d total / d up_root
    [b, y, x] += factor, abs_up: per head sum over the taps of |weight * source| [B, 57, H, W])."""
    n_heads, B, H, W = 4 * s["stage_num"], s["B"], s["H"], s["W"]
    valid = (x["valids"] > 0).astype(np.float64)
    coef = np.zeros((n_heads, B, NC))
    diffs, roots, abs_ups = [], [], []
    total = l2d = l3d = lroot = 0.0
    for h in range(n_heads):
        fine = h % 4 == 3
        factor = 1.0 if fine else 0.25
        src = np.concatenate(x["src"][h][:2], axis=1)
        up = upsample(src, H, W)
        wy, wx = weights(src.shape[-2], H), weights(src.shape[-1], W)
        abs_ups.append(wy @ np.abs(src.astype(np.float64)) @ wx.T)
        lab = x["labels"][:, head_scale(s, h)][:, LABEL_CHANNEL].astype(np.float64)
        d = up - lab
        diffs.append(d)
        m = (d * d).mean(axis=(2, 3)) * valid
        hard = s["ohkm"] and fine
        groups = [(0, NKP, s["topk"]), (NKP, NPAF, 2 * s["topk"]), (N2D, NDD, s["topk"])] if hard else [(0, N2D, N2D), (N2D, NDD, NDD)]
        vals = []
        for first, n, keep in groups:
            part = 0.1 if first < N2D else 5.0
            sel = np.zeros((B, n))
            for b in range(B):
                order = np.argsort(-m[b, first:first + n], kind="stable")      # larger first, ties to the lower channel
                sel[b, order[:keep]] = 1
            vals.append((m[:, first:first + n] * sel).sum() / (B * keep))
            coef[h, :, first:first + n] = factor * part * 2.0 / (H * W * B * keep) * valid[:, first:first + n] * sel
        loss2d, loss3d = sum(vals[:-1]), vals[-1]
        # DepthLoss: the rows with Z > 0, their cell by truncation
        up_root = upsample(x["src"][h][2], H, W)
        rows = []
        for b in range(B):
            for y, xx, z in x["rdepth"][b]:
                if z > 0:
                    assert -1 < y < H and -1 < xx < W
                    rows.append((b, int(y), int(xx), float(up_root[b, 0, int(y), int(xx)]) - float(z)))
        root = sum(abs(r[3]) for r in rows) / len(rows) if rows else 0.0
        roots.append([(b, y, xx, 10.0 * factor * np.sign(dz) / len(rows)) for b, y, xx, dz in rows])
        total += factor * (0.1 * loss2d + 5.0 * loss3d + 10.0 * root)
        if fine:
            l2d, l3d, lroot = l2d + loss2d, l3d + loss3d, lroot + root
    return dict(losses=np.array([total, l2d, l3d, lroot]), coef=coef, diff=diffs, root=roots, abs_up=abs_ups)


def gradients(s, x, coef=None, variant=None, fwd=None):
    """Per head [g heatmap_2d, g det_d, g root_d], float64 arrays shaped like the sources.  coef: None -- the restated factor in
    float64, f = coef * upstream; or the kernel's own fp32 table [n_heads, B, 57], f = fp32(coef * fp32(upstream)) as the kernel
    rounds it."""
    fwd = forward(s, x) if fwd is None else fwd
    H, W = s["H"], s["W"]
    upstream = 1.0 if variant == "ignore_upstream" else s["upstream"]
    if coef is None:
        f = fwd["coef"] * upstream
    else:
        f = (coef.astype(F32) * F32(upstream)).astype(F32).astype(np.float64)
    out = []
    for h in range(len(x["src"])):
        sh, sw = x["src"][h][0].shape[2:]
        wy, wx = weights(sh, H, variant), weights(sw, W, variant)
        e = fwd["diff"][h] * f[h][:, :, None, None]
        g = wy.T @ e @ wx
        rh, rw = x["src"][h][2].shape[2:]
        ry, rx = weights(rh, H, variant), weights(rw, W, variant)
        groot = np.zeros(x["src"][h][2].shape)
        for b, y, xx, fac in fwd["root"][h]:
            groot[b, 0] += fac * upstream * np.outer(ry[y], rx[xx])
        out.append([g[:, :N2D], g[:, N2D:], groot])
    return out
