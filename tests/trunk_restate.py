"""Float64 restatement of the trunk of one Upsample_unit (smap_amd/trunk.py, csrc/trunk.hip), launch by launch, in plain torch.

    forward   S = X Wu^T        U = O_prev Wc^T (at LOW resolution)       O = relu(S + I(U) + b)
    backward  gPre = gO * [O > 0]      gb = sum_p gPre      gWu = gPre^T X      gX = gPre Wu
              gU = I^T gPre            gWc = gU^T O_prev    gO_prev = gU Wc

Every function is one launch of the library and takes that launch's inputs; called on magnitudes the same function gives sum |a * b|,
the quantity the fp32 chain bound  |err| <= (K + 2) * 2^-24 * sum |a * b|  is stated in.  The interpolation I is a pair of matrices
(trunk_scenes.lerp_matrix): with fp32 = False they hold the weights F.interpolate computes on a float64 tensor (what the golden file
was made with), with fp32 = True the weights the fp32 kernels compute, exactly, as float64 numbers -- the GPU is held to those: its
weights ARE ATen's fp32 rule, and the distance between the two rules is not an arithmetic error of the kernel.
Layouts: [B, h, w, channels] throughout; weights [out, in].
"""
import torch

import heads_restate as HR
import trunk_scenes as TS

U = 2.0 ** -24
K_red, red_chain = HR.K_red, HR.red_chain          # the chain length of a reduction over the pixels: sliced here as in the head arms


class Interp:
    """I and I^T between hp x wp and h x w, and the number of (pixel, tap) pairs that name each low-resolution cell."""

    def __init__(self, hp, wp, h, w, fp32):
        self.my, self.mx = TS.lerp_matrix(hp, h, fp32), TS.lerp_matrix(wp, w, fp32)
        ny, nx = self._names(hp, h), self._names(wp, w)
        self.taps = (ny[:, None] * nx[None, :]).double()            # [hp, wp]

    @staticmethod
    def _names(in_size, out_size):
        i0, i1, _, _ = TS.lerp_table(in_size, out_size, True)
        n = torch.zeros(in_size, dtype=torch.int64)
        for i in (i0, i1):
            n += torch.bincount(torch.from_numpy(i), minlength=in_size)
        return n

    def up(self, u):
        return torch.einsum("yi,xj,bijc->byxc", self.my, self.mx, u)

    def down(self, g):
        return torch.einsum("yi,xj,byxc->bijc", self.my, self.mx, g)


def mm_launch(a, w):
    """[.., K] x [N, K]^T: S, U (K = the input channels)."""
    return a @ w.T


def upadd_launch(s, u_up, b):
    """pre = S + I(U) + b, before the ReLU; u_up = I(U) or None."""
    return s + b if u_up is None else s + u_up + b


def reduce_launch(a, x):
    """a^T x [N, M] and the column sums of a [N]; K = pixels."""
    return torch.einsum("bhwn,bhwm->nm", a, x), a.sum(dim=(0, 1, 2))


def forward(x, o_prev, wu, wc, b, it):
    """pre [B, h, w, chl] (O = relu(pre)), S, U."""
    s = mm_launch(x, wu)
    u = None if o_prev is None else mm_launch(o_prev, wc)
    return upadd_launch(s, None if u is None else it.up(u), b), s, u


def backward(x, o_prev, wu, wc, g, mask, it):
    """The gradients of <G, O> with O > 0 given as `mask`: dict gpre, gb, gwu, gx and, with an up path, gu, gwc, gprev."""
    out = {"gpre": g * mask}
    out["gwu"], out["gb"] = reduce_launch(out["gpre"], x)
    out["gx"] = out["gpre"] @ wu
    if o_prev is not None:
        out["gu"] = it.down(out["gpre"])
        out["gwc"], _ = reduce_launch(out["gu"], o_prev)
        out["gprev"] = out["gu"] @ wc
    return out


def forward_bounds(x, o_prev, wu, wc, b, it):
    """Bound on |kernel - restatement| of O for the composed fp32 forward on the same fp32 operands, and the magnitude
    sum |x||wu| + I(sum |o_prev||wc|) + |b| the tie condition is stated in.  No up path: ONE launch, (Cin + 2) u mag.  Otherwise
    e_S = (Cin + 2) u |X||Wu|^T, e_U = (chl + 2) u |O_prev||Wc|^T, and upadd's own 6 u on its (perturbed) inputs plus what they carry:
    e_O = 6 u (mag + e_S + I(e_U)) + e_S + I(e_U); relu is 1-Lipschitz."""
    cin, chl = x.shape[-1], wu.shape[0]
    mag_s = x.abs() @ wu.abs().T
    if o_prev is None:
        mag = mag_s + b.abs()
        return (cin + 2) * U * mag, mag
    mag_u = it.up(o_prev.abs() @ wc.abs().T)
    e_s, e_u = (cin + 2) * U * mag_s, (chl + 2) * U * mag_u
    mag = mag_s + mag_u + b.abs()
    return 6 * U * (mag + e_s + e_u) + e_s + e_u, mag


def backward_bounds(x, o_prev, wu, wc, g, mask, it):
    """Bounds for the composed backward given the mask both sides use: each launch's chain bound on its own (perturbed) inputs plus the
    perturbation carried through.  gPre is a selection: exact."""
    chl = wu.shape[0]
    K = red_chain(x.shape[0] * x.shape[1] * x.shape[2])          # the sliced reduction's chain length, not the pixel count
    ga = (g * mask).abs()
    out = {"gpre": torch.zeros_like(ga)}
    w_mag, b_mag = reduce_launch(ga, x.abs())
    out["gwu"], out["gb"] = (K + 2) * U * w_mag, (K + 2) * U * b_mag
    out["gx"] = (chl + 2) * U * (ga @ wu.abs())
    if o_prev is not None:
        Kl = red_chain(o_prev.shape[0] * o_prev.shape[1] * o_prev.shape[2])
        gu_mag = it.down(ga)
        e_gu = (it.taps[None, :, :, None] + 3) * U * gu_mag
        out["gu"] = e_gu
        out["gwc"] = (Kl + 2) * U * reduce_launch(gu_mag + e_gu, o_prev.abs())[0] + reduce_launch(e_gu, o_prev.abs())[0]
        out["gprev"] = (chl + 2) * U * ((gu_mag + e_gu) @ wc.abs()) + e_gu @ wc.abs()
    return out


# the fold (matrix=True: the weight of a 1x1 trunk conv as [out, in]) and its chain rule with frozen statistics: the same as for a head conv
fold, unfold_grads = HR.fold, HR.unfold_grads


def scene_operands(name):
    """The scene's fp32-valued operands as float64 tensors: x, o_prev, g, and per module its parameter dict."""
    x_np, p_np, g_np = TS.inputs(name)
    sd = {k: v.double() for k, v in TS.weights(name).items()}
    params = {m: {k: sd["%s.%s" % (m, k)] for k in TS.PARAM_KINDS + TS.STATS} for m in TS.module_names(name)}
    t = lambda a: None if a is None else torch.from_numpy(a).double()
    return t(x_np), t(p_np), t(g_np), params
