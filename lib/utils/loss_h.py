"""JointsL2Loss and DepthLoss under the reference's import path (lib/utils/loss_h.py), over the fused kernels of smap_amd/loss.py.

A training script that builds its own loss from these two modules switches to the GPU loss by import path alone.  Each call is ONE
head of smap_loss_forward's single-head mode (unit weights): a fixed-order reduction, a finish, and one backward launch.  A script
that wants the whole network's loss in three launches uses smap_amd.loss.SMAPLoss instead.

    JointsL2Loss(has_ohkm=False, topk=8, thres=0, paf_num=0)(output, valid, label)
        output, label [B, C, H, W] with C = 43 (15 key points + 2 * 14 part-affinity channels) or C = 14 (relative depth);
        valid [B, C, 1] or [B, C]; the per-channel mean squared error times (valid > thres), then its mean over (B, C) -- or, with
        has_ohkm, the mean of the topk largest per frame (paf_num = 0), or of the topk largest key-point channels plus that of the
        2 * topk largest of the 2 * paf_num part-affinity channels.  Ties go to the lower channel index.
    DepthLoss()(output, rdepth)
        output [B, 1, H, W], rdepth [B, R, 3] rows (y, x, Z): mean of |output[b, 0, int(y), int(x)] - Z| over the rows with Z > 0,
        0 when there is none.  A row outside the map gives NaN.

Only `thres == 0` exists in the kernels (the network's loss uses no other value), and only C = 43 and C = 14, with or without
has_ohkm: the reference's module takes any C, this one raises ValueError for another.  The kernels read labels in the 57-channel
layout of a training sample, so every JointsL2Loss call first gathers its label into a zeroed [B, 1, 57, H, W] tensor and its valid
into [B, 57] -- torch operations on the device, no host synchronisation (the channel index is uploaded once per device and kept)."""
import torch
import torch.nn as nn

from smap_amd import loss as K


_index_cache = {}


def _label_index(device):
    """LABEL_CHANNEL as a long tensor on `device`: uploaded once per device."""
    if device not in _index_cache:
        _index_cache[device] = torch.tensor(K.LABEL_CHANNEL, dtype=torch.long, device=device)
    return _index_cache[device]


def _output_order_to_labels(label, first):
    """label [B, C, H, W] in output order (channels first .. first + C of the 57) -> [B, 1, 57, H, W] in label order, zeros elsewhere."""
    B, C, H, W = label.shape
    full = torch.zeros((B, 1, K.NC, H, W), dtype=label.dtype, device=label.device)
    full[:, 0].index_copy_(1, _label_index(label.device)[first:first + C], label.detach())
    return full


class DepthLoss(nn.Module):
    def forward(self, output, rdepth):
        if output.dim() != 4 or output.shape[1] != 1:
            raise ValueError("DepthLoss: output is [B, 1, H, W], got %s" % (tuple(output.shape),))
        return K.single_head_loss(rd=output, rdepth=rdepth)[0]


class JointsL2Loss(nn.Module):
    def __init__(self, has_ohkm=False, topk=8, thres=0, paf_num=0):
        super().__init__()
        if thres != 0:
            raise NotImplementedError("JointsL2Loss: only thres == 0 is implemented on the GPU, got %r" % (thres,))
        if paf_num not in (0, 14):
            raise NotImplementedError("JointsL2Loss: paf_num is 0 or 14, got %r" % (paf_num,))
        self.has_ohkm, self.topk, self.thres, self.paf_num = bool(has_ohkm), int(topk), thres, int(paf_num)

    def forward(self, output, valid, label):
        if output.dim() != 4 or tuple(output.shape) != tuple(label.shape):
            raise ValueError("JointsL2Loss: output and label are [B, C, H, W] alike, got %s and %s" % (tuple(output.shape), tuple(label.shape)))
        B, C = output.shape[:2]
        want = (K.N2D if self.paf_num else K.NDD) if self.has_ohkm else C
        if C != want or C not in (K.N2D, K.NDD):
            raise ValueError("JointsL2Loss: %d channels; the kernels know 43 (2D, paf_num = 14) and 14 (relative depth, paf_num = 0)" % C)
        first = 0 if C == K.N2D else K.N2D
        if valid.dim() == 3 and valid.shape[2] == 1:
            valid = valid[:, :, 0]
        if tuple(valid.shape) != (B, C):
            raise ValueError("JointsL2Loss: valid is [%d, %d(, 1)], got %s" % (B, C, tuple(valid.shape)))
        valids = torch.zeros((B, K.NC), dtype=torch.float32, device=output.device)
        valids[:, first:first + C] = valid
        labels = _output_order_to_labels(label, first)
        maps = dict(hm=output) if C == K.N2D else dict(dd=output)
        return K.single_head_loss(labels=labels, valids=valids, ohkm=self.has_ohkm, topk=self.topk, **maps)[0]
