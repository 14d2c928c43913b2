"""Float64 restatement of the head arms of one Upsample_unit (smap_amd/heads.py, csrc/heads.hip), launch by launch, in plain torch.

    forward   Z_a = X W1_a^T + b1_a        M_a = relu(Z_a)        Y_a = conv3x3(M_a, W2_a, pad 1) + b2_a
    backward  gb2_a = sum_p G_a            gW2_a[c, ci, t] = sum_p G_a[p, c] M_a[p + t, ci]   (inside the image)
              gM_a = conv3x3^T(G_a, W2_a)  gZ_a = gM_a * [Z_a > 0]
              gb1_a = sum_p gZ_a           gW1_a = gZ_a^T X       gX = sum_a gZ_a W1_a

Every function is one launch of the library and takes that launch's inputs; called on magnitudes (absolute values, no bias sign) the
same function gives sum |a * b|, the quantity the fp32 chain bound  |err| <= (K + 2) * 2^-24 * sum |a * b|  is stated in (K: the
launch's reduction length; K fused multiply-adds and one bias addition, each within 2^-24 relative).  A reduction over the P pixels
is not one chain of P terms: it is sliced, and its K is red_chain(P).
Layouts: X, Z, M, gZ, gX are [B, h, w, channels]; heads and their gradients [B, C_a, h, w]; weights as torch keeps them.
"""
import torch
import torch.nn.functional as F

from smap_amd.gemm_f32 import slice_len

U = 2.0 ** -24
TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]


def K_red(P):
    """slice_len(P) + slices(P): the chain length of a reduction over P pixels (reduce_gemm + reduce_fold; gW and the column sums gb
    alike).  Within a slice every output is ONE fmaf chain of at most slice_len terms, k ascending -- rows beyond the slice's end add
    exact zeros -- and reduce_fold then adds the `slices` parts in order: K_red roundings on any term, so
    |err| <= gamma_K sum |a * b| <= (K_red + 2) * 2^-24 * sum |a * b|  while  K_red^2 * 2^-24 <= 2, which is asserted here: it holds up
    to about 3.7e5 pixels (K_red = 5792), not for every P the library admits, and not for K = P itself from P = 5793 on."""
    n = slice_len(P)
    k = n + -(-P // n)
    assert k * k * U <= 2, (P, k)
    return k


def red_chain(P):
    """The K of a reduction's bound: min(P, K_red(P)).  Up to slice_len pixels the one slice is a chain of P terms and the fold adds
    it to zero exactly, and in any order of summation no term of a sum of P products is rounded more than P times; P is the smaller
    of the two only below 260 pixels.  Never larger than the P the bounds used before."""
    return min(P, K_red(P))


def z_launch(x, w1cat, b1cat):
    """Z [B, h, w, 3 chl] of the three arms side by side; K = chl."""
    return x @ w1cat.T + b1cat


def y_launch(m_a, w2, b2):
    """Y_a [B, C_a, h, w] from M_a [B, h, w, chl]; K = 9 chl."""
    return F.conv2d(m_a.permute(0, 3, 1, 2), w2, b2, padding=1)


def gm_launch(g, w2):
    """gM_a [B, h, w, chl] from G_a [B, C_a, h, w]: the adjoint of y_launch in M; K = 9 C_a."""
    return F.conv_transpose2d(g, w2, padding=1).permute(0, 2, 3, 1)


def gw2_launch(g, m_a):
    """gW2_a [C_a, chl, 3, 3] and gb2_a [C_a]; K = B h w."""
    Bn, h, w, chl = m_a.shape
    mp = F.pad(m_a.permute(0, 3, 1, 2), (1, 1, 1, 1))
    gw = torch.stack([torch.einsum("bcyx,biyx->ci", g, mp[:, :, ky:ky + h, kx:kx + w]) for ky, kx in TAPS], dim=2)
    return gw.view(g.shape[1], chl, 3, 3), g.sum(dim=(0, 2, 3))


def gw1_launch(gz, x):
    """gW1cat [3 chl, chl] and gb1cat [3 chl]; K = B h w."""
    return torch.einsum("bhwn,bhwc->nc", gz, x), gz.sum(dim=(0, 1, 2))


def gx_launch(gz, w1cat):
    """gX [B, h, w, chl]; K = 3 chl."""
    return gz @ w1cat


def arms(t, chl):
    """The three arms' [B, h, w, chl] slices of a [B, h, w, 3 chl] tensor."""
    return [t[..., a * chl:(a + 1) * chl] for a in range(3)]


def forward(x, w1cat, b1cat, w2, b2):
    """Z [B, h, w, 3 chl] and [Y_a]."""
    z = z_launch(x, w1cat, b1cat)
    return z, [y_launch(m_a, w2[a], b2[a]) for a, m_a in enumerate(arms(torch.relu(z), x.shape[-1]))]


def backward(x, w1cat, w2, g, z, mask=None):
    """The gradients of sum_a <G_a, Y_a>: dict gw1, gb1, gw2 [3], gb2 [3], gx, gz.  mask [B, h, w, 3 chl] (bool): used in place of Z > 0."""
    chl = x.shape[-1]
    mask = (z > 0) if mask is None else mask
    m = arms(torch.relu(z), chl)
    out = {"gw2": [], "gb2": []}
    gz = []
    for a in range(3):
        gw, gb = gw2_launch(g[a], m[a])
        out["gw2"].append(gw), out["gb2"].append(gb)
        gz.append(gm_launch(g[a], w2[a]))
    out["gz"] = torch.cat(gz, dim=-1) * mask
    out["gw1"], out["gb1"] = gw1_launch(out["gz"], x)
    out["gx"] = gx_launch(out["gz"], w1cat)
    return out


def forward_bounds(x, w1cat, b1cat, w2, b2, z):
    """Bounds on |kernel - restatement| of M [B, h, w, 3 chl] and of every Y_a, for the composed fp32 forward on the same fp32 operands:
    e_M = (chl + 2) u mag(Z)  (relu is 1-Lipschitz);  e_Y = (9 chl + 2) u (conv(|M| + e_M, |W2|) + |b2|) + conv(e_M, |W2|):
    the chain bound on the kernel's own M, which lies within e_M of the restatement's, plus what e_M itself carries through the conv."""
    chl = x.shape[-1]
    e_m = (chl + 2) * U * z_launch(x.abs(), w1cat.abs(), b1cat.abs())
    m = torch.relu(z)
    e_y = [(9 * chl + 2) * U * y_launch(ma + ea, w2[a].abs(), b2[a].abs()) + y_launch(ea, w2[a].abs(), None)
           for a, (ma, ea) in enumerate(zip(arms(m, chl), arms(e_m, chl)))]
    return e_m, e_y


def backward_bounds(x, w1cat, w2, g, z, mask, e_m):
    """Bounds for the composed backward given the mask both sides use and e_M of forward_bounds, each launch's chain bound on its own
    (perturbed) inputs plus the perturbation carried through: dict like backward's."""
    chl, K = x.shape[-1], red_chain(x.shape[0] * x.shape[1] * x.shape[2])
    m, em = arms(torch.relu(z), chl), arms(e_m, chl)
    out = {"gw2": [], "gb2": []}
    gz_mag, e_gz = [], []
    for a in range(3):
        ga = g[a].abs()
        gw_mag, gb_mag = gw2_launch(ga, m[a] + em[a])
        out["gw2"].append((K + 2) * U * gw_mag + gw2_launch(ga, em[a])[0])
        out["gb2"].append((K + 2) * U * gb_mag)
        mag = gm_launch(ga, w2[a].abs())
        gz_mag.append(mag)
        e_gz.append((9 * g[a].shape[1] + 2) * U * mag)
    gz_mag, e_gz = torch.cat(gz_mag, dim=-1) * mask, torch.cat(e_gz, dim=-1) * mask
    out["gz"] = e_gz
    w_mag, b_mag = gw1_launch(gz_mag + e_gz, x.abs())
    w_e, b_e = gw1_launch(e_gz, x.abs())
    out["gw1"], out["gb1"] = (K + 2) * U * w_mag + w_e, (K + 2) * U * b_mag + b_e
    out["gx"] = (3 * chl + 2) * U * gx_launch(gz_mag + e_gz, w1cat.abs()) + gx_launch(e_gz, w1cat.abs())
    return out


def fold(p, eps=1e-5, matrix=False):
    """Folded (w', b') of one conv_bn_relu: p = dict of conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var.
    matrix: w' as [out, in * taps] (what the trunk's 1x1 GEMMs take)."""
    s = p["bn.weight"] / torch.sqrt(p["bn.running_var"] + eps)
    w = p["conv.weight"] * s.view(-1, 1, 1, 1)
    return (w.flatten(1) if matrix else w), (p["conv.bias"] - p["bn.running_mean"]) * s + p["bn.bias"]


def unfold_grads(p, gw, gb, eps=1e-5, magnitudes=False):
    """The chain rule of fold with frozen statistics: gradients at conv.weight, conv.bias, bn.weight, bn.bias from those at (w', b').
    magnitudes: every term's absolute value instead (gw, gb then are magnitudes or bounds)."""
    a = (lambda t: t.abs()) if magnitudes else (lambda t: t)
    r = 1.0 / torch.sqrt(p["bn.running_var"] + eps)
    s = a(p["bn.weight"]) * r
    gw = gw.view_as(p["conv.weight"])
    return {"conv.weight": gw * s.view(-1, 1, 1, 1), "conv.bias": gb * s, "bn.bias": gb,
            "bn.weight": ((gw * a(p["conv.weight"])).sum(dim=(1, 2, 3)) + gb * a(p["conv.bias"] - p["bn.running_mean"])) * r}
