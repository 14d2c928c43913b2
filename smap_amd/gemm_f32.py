"""What the fp32 training GEMMs' callers share on the Python side: the mirror of the host half of csrc/gemm_f32_device.h (the slicing of
a reduction over the pixels, the smap_heads_x operand descriptor, the operand checks, a workspace) and the BN fold in front of both
heads.py (the head arms) and trunk.py (u_skip, up_conv).  smap_amd/finetune.py is what builds on the two."""
import torch

from . import lib as L

SLICE_MIN, SLICE_MAX_N, BK = 256, 64, 16      # csrc/gemm_f32_device.h


def round64(n):
    return (n + 63) // 64 * 64


def slice_len(P):
    """Pixels per reduction slice (slice_len_of)."""
    if P <= SLICE_MIN * SLICE_MAX_N:
        return SLICE_MIN
    per = (P + SLICE_MAX_N - 1) // SLICE_MAX_N
    return (per + BK - 1) // BK * BK


def slices(P):
    """Slices of a reduction over P pixels (slices_of); none for no pixels."""
    return -(-P // slice_len(P)) if P else 0


def new_workspace(nbytes, device):
    """A workspace tensor (uint8; torch's allocator aligns it to 512 bytes)."""
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def x_descriptor(x):
    """(smap_heads_x, B, h, w, C) of X: [B, h, w, C] fp32 or fp16, or [B, h, w, 2, C] fp16 hi|lo; frames and pixels back to back."""
    if not x.is_cuda:
        raise ValueError("X must live on the GPU")
    if x.dim() == 5 and x.dtype == torch.float16 and x.shape[3] == 2:
        B, h, w, _, chl = x.shape
        layout, pix = L.HEADS_X_F16_HILO, x.stride(2)
        ok = x.stride(4) == 1 and x.stride(3) == chl
    elif x.dim() == 4 and x.dtype in (torch.float32, torch.float16):
        B, h, w, chl = x.shape
        layout, pix = (L.HEADS_X_F32 if x.dtype == torch.float32 else L.HEADS_X_F16), x.stride(2)
        ok = x.stride(3) == 1
    else:
        raise ValueError("X: [B, h, w, chl] fp32 / fp16 or [B, h, w, 2, chl] fp16, not %s %s" % (tuple(x.shape), x.dtype))
    if not ok or x.stride(1) != w * pix or x.stride(0) != h * w * pix:
        raise ValueError("X: channels, pixels and frames must lie back to back (strides %s)" % (x.stride(),))
    return L.HeadsX(x.data_ptr(), layout, pix), B, h, w, chl


def dense_fp32(t, shape, what):
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError("%s: dense fp32 %s expected, got %s %s" % (what, tuple(shape), tuple(t.shape), t.dtype))
    return t


def fold_bn(weight, bias, gamma, beta, mean, var, eps=1e-5):
    """Eval-mode BN folded into the conv before it: w' = w g / sqrt(var + eps), b' = (b - mean) g / sqrt(var + eps) + beta.  Plain
    differentiable torch ops: autograd carries d / d w' and d / d b' on to weight, bias (may be None), gamma and beta."""
    scale = gamma / torch.sqrt(var + eps)
    b = -mean if bias is None else bias - mean
    return weight * scale.view(-1, *([1] * (weight.dim() - 1))), b * scale + beta


def folded(params, prefix, eps=1e-5):
    """fold_bn of the conv_bn_relu module `prefix` from `params` (state_dict keys -> fp32 tensors, leaves where a gradient is wanted)."""
    return fold_bn(params[prefix + ".conv.weight"], params.get(prefix + ".conv.bias"), params[prefix + ".bn.weight"], params[prefix + ".bn.bias"],
                   params[prefix + ".bn.running_mean"], params[prefix + ".bn.running_var"], eps)
