"""The training loss of the network on the GPU (reference: model/smap.py:355-401 SMAP._calculate_loss, lib/utils/loss_h.py).

`SMAPLoss` takes what the reference's loss takes -- the outputs of all 4 * stage_num heads, `valids`, `labels` (as `render_labels`
returns them) and `rdepth` -- and returns the reference's dict.  The value is two launches (smap_loss_forward: a fixed-order
reduction per (channel, frame, head), then one workgroup that selects, averages and weighs), the gradient one launch
(smap_loss_backward), with no host synchronisation in either: csrc/loss.hip, csrc/loss_core.h, DESIGN.md section 13.

Differences from the reference, on purpose:
  * only `total_loss` is differentiable.  `loss_2d`, `loss_bone` and `loss_root` are detached logging values; the reference's carry
    graphs too, and nothing backpropagates them.
  * hard-keypoint mining breaks ties towards the LOWER channel index; torch.topk leaves them unspecified.
  * a root-depth row with Z > 0 whose cell lies outside the map makes `total_loss` NaN (result[4] counts such rows; `strict=True`
    reads it -- one synchronisation -- and raises); the reference wraps around or raises an IndexError there.
  * there is no CPU path and no fallback: the tensors live on the GPU.

`EngineLoss` is the same value, forward only, for the validation loss: it reads the 36 head tensors where an all-heads engine
(smap_amd/engine.py, BackboneEngine(all_heads=True).head_sources()) leaves them, at their own resolutions, and interpolates to H x W inside
the reduction (smap_loss_forward_src).  Its values carry no graph.

`SMAPLossNative` is SMAPLoss for heads that were not upsampled: value (smap_loss_forward_src) and gradient (smap_loss_backward_src, the
adjoint of the upsampling: two launches, a fixed summation order) at the tensors' own resolutions, one autograd.Function.
`EngineLoss.value_and_grad` is the same pair on an all-heads engine's tensors, gradients in their layout.
"""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import lib as L

NKP, N2D, NDD, NC, MAX_HEADS, GRAD_C = 15, 43, 14, 57, 16, 58
# label channel of every output channel: the 43 2D channels (key points, then the x, y of every limb), then the 14 depth channels
LABEL_CHANNEL = tuple(list(range(NKP)) + [NKP + 3 * (c // 2) + c % 2 for c in range(N2D - NKP)] + [NKP + 3 * c + 2 for c in range(NDD)])


def workspace_layout(n_heads, B, R):
    """Byte offsets of the workspace's sections and its size (csrc/loss_core.h workspace_layout)."""
    n, rows = n_heads * B * NC, n_heads * B * R
    w = {"sums": 0}
    w["m"] = w["sums"] + n * 8
    w["part"] = w["m"] + n * 8
    w["headloss"] = w["part"] + n_heads * B * 6 * 8
    w["coef"] = w["headloss"] + MAX_HEADS * 5 * 8
    w["sel"] = w["coef"] + n * 4
    w["rd_at"] = w["sel"] + n * 4
    w["root_fac"] = w["rd_at"] + rows * 4
    w["root_cell"] = w["root_fac"] + rows * 4
    w["bytes"] = (w["root_cell"] + rows * 4 + 7) // 8 * 8
    return w


def workspace_views(ws, n_heads, B, R):
    """dict of typed views of a workspace tensor (uint8 [bytes], device or host)."""
    w = workspace_layout(n_heads, B, R)
    v = lambda key, dtype, shape: ws[w[key]:w[key] + int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()].view(dtype).view(shape)
    return dict(sums=v("sums", torch.float64, (n_heads, B, NC)), m=v("m", torch.float64, (n_heads, B, NC)),
                part=v("part", torch.float64, (n_heads, B, 6)), headloss=v("headloss", torch.float64, (MAX_HEADS, 5)), coef=v("coef", torch.float32, (n_heads, B, NC)),
                sel=v("sel", torch.float32, (n_heads, B, NC)), rd_at=v("rd_at", torch.float32, (n_heads, B, R)),
                root_fac=v("root_fac", torch.float32, (n_heads, B, R)), root_cell=v("root_cell", torch.int32, (n_heads, B, R)))


class _Config:
    """The integers every entry point takes."""

    def __init__(self, stage_num, ohkm, topk, ctf, single, B, S, R, H, W):
        self.stage_num, self.ohkm, self.topk, self.ctf, self.single = int(stage_num), int(bool(ohkm)), int(topk), int(bool(ctf)), int(bool(single))
        self.B, self.S, self.R, self.H, self.W = int(B), int(S), int(R), int(H), int(W)
        self.n_heads = 1 if self.single else 4 * self.stage_num

    def head_args(self):
        return (self.stage_num, self.ohkm, self.topk, self.ctf, self.single)


def _ptr(t):
    return None if t is None else t.data_ptr()


def result_dict(result, logged=None):
    """The reference's dict of a result [8]; logged: where the three logging values come from (SMAPLoss: the detached result)."""
    logged = result if logged is None else logged
    return dict(total_loss=result[0], loss_2d=logged[1], loss_bone=logged[2], loss_root=logged[3])


def _head_array(tensors):
    return (C.c_void_p * len(tensors))(*[_ptr(t) for t in tensors])


def forward_raw(cfg, tensors, labels, valids, rdepth):
    """smap_loss_forward on the current stream: (result [8] fp32, workspace uint8).  tensors: 3 * n_heads checked device tensors (or
    None in single-head mode).  No synchronisation."""
    dev = rdepth.device
    bytes_ = workspace_layout(cfg.n_heads, cfg.B, cfg.R)["bytes"]
    ws = torch.empty((bytes_,), dtype=torch.uint8, device=dev)
    result = torch.empty((8,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().smap_loss_forward(_head_array(tensors), _ptr(labels), _ptr(valids), _ptr(rdepth), *cfg.head_args(), cfg.B, cfg.S,
                                           cfg.R, cfg.H, cfg.W, ws.data_ptr(), bytes_, result.data_ptr(),
                                           torch.cuda.current_stream(dev).cuda_stream), "smap_loss_forward")
    return result, ws


SOURCE_KEYS = (("heatmap_2d", N2D), ("det_d", NDD), ("root_d", 1))


def source_workspace_bytes(n_heads, B, R, H, W):
    """Bytes of smap_loss_forward_src's workspace: workspace_layout, then the per-chunk partial sums (csrc/loss.hip)."""
    return L.load().smap_loss_src_workspace_bytes(n_heads, B, R, H, W)


def forward_from_sources(cfg, sources, labels, valids, rdepth):
    """smap_loss_forward_src on the current stream: (result [8] fp32, workspace uint8).  sources: n_heads dicts
    {"heatmap_2d", "det_d", "root_d": (ptr, h, w, c, pix_stride, ch_stride, frame_stride)} (engine.HeadSource), strides in floats;
    labels, valids, rdepth: checked device tensors.  No synchronisation, no graph."""
    dev = rdepth.device
    arr = _source_array(cfg, sources, "sources")
    bytes_ = source_workspace_bytes(cfg.n_heads, cfg.B, cfg.R, cfg.H, cfg.W)
    ws = torch.empty((max(bytes_, 0),), dtype=torch.uint8, device=dev)      # (negative: sizes the library refuses below)
    result = torch.empty((8,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().smap_loss_forward_src(arr, _ptr(labels), _ptr(valids), _ptr(rdepth), cfg.stage_num, cfg.ohkm, cfg.topk, cfg.ctf,
                                               cfg.B, cfg.S, cfg.R, cfg.H, cfg.W, ws.data_ptr(), bytes_, result.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream), "smap_loss_forward_src")
    return result, ws


def _source_array(cfg, sources, what):
    """The 3 * n_heads smap_head_src descriptors of n_heads dicts of HeadSource tuples (a None entry or pointer: a null descriptor)."""
    if cfg.single or len(sources) != cfg.n_heads:
        raise ValueError("%s: %d heads for %d stages of 4" % (what, len(sources), cfg.stage_num))
    arr = (L.HeadSrc * (3 * cfg.n_heads))()
    for h, d in enumerate(sources):
        for k, (key, _) in enumerate(SOURCE_KEYS):
            if d.get(key) is None:
                continue
            ptr, sh, sw, c, pix, ch, frame = d[key]
            arr[3 * h + k] = L.HeadSrc(int(ptr) if ptr else None, int(sh), int(sw), int(c), int(pix), int(ch), 0, int(frame))
    return arr


def source_scratch_bytes(cfg, sources, grads):
    """Bytes of smap_loss_backward_src's scratch: f32 [B][c][h][w][4] per heatmap_2d / det_d tensor below H x W whose gradient is wanted
    (csrc/loss.hip part_floats; smap_loss_backward_src_scratch_bytes is the bound over all of them)."""
    total = 0
    for d, g in zip(sources, grads):
        for key, c in SOURCE_KEYS[:2]:
            _, sh, sw = d[key][:3]
            if g.get(key) is not None and g[key][0] and (sh, sw) != (cfg.H, cfg.W):
                total += cfg.B * c * sh * sw * 16
    return total


def backward_to_sources(cfg, sources, grads, labels, ws, upstream):
    """smap_loss_backward_src on the current stream, behind forward_from_sources on the same `sources` and `labels`: writes d total /
    d source * upstream[0] through the descriptors `grads` (n_heads dicts like `sources`: the same h, w, c, their own pointers and
    strides; None or a null pointer: not wanted).  ws: the workspace forward_from_sources returned; upstream: device fp32 tensor, its
    first element is read on the device.  No synchronisation, no graph.  Returns the scratch tensor (done with once the stream is)."""
    dev = ws.device
    src, dst = _source_array(cfg, sources, "sources"), _source_array(cfg, grads, "grads")
    bytes_ = source_scratch_bytes(cfg, sources, grads)
    scratch = torch.empty((max(bytes_, 16),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().smap_loss_backward_src(src, dst, _ptr(labels), cfg.stage_num, cfg.ohkm, cfg.topk, cfg.ctf, cfg.B, cfg.S, cfg.R,
                                                cfg.H, cfg.W, ws.data_ptr(), ws.numel(), scratch.data_ptr(), bytes_, upstream.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream), "smap_loss_backward_src")
    return scratch


def backward_raw(cfg, tensors, labels, ws, upstream):
    """smap_loss_backward on the current stream: one buffer [n_heads, 58 * B * H * W] fp32 and its 3 * n_heads views, in the order of
    `tensors` (None where the tensor was).  upstream: device fp32 tensor, its first element is d L / d total."""
    dev = ws.device
    HW = cfg.H * cfg.W
    grad = torch.empty((cfg.n_heads, GRAD_C * cfg.B * HW), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().smap_loss_backward(_head_array(tensors), _ptr(labels), *cfg.head_args(), cfg.B, cfg.S, cfg.R, cfg.H, cfg.W,
                                            ws.data_ptr(), ws.numel(), upstream.data_ptr(), grad.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream), "smap_loss_backward")
    views = []
    for h in range(cfg.n_heads):
        cut = (0, N2D * cfg.B * HW, NC * cfg.B * HW, GRAD_C * cfg.B * HW)
        for k, ch in enumerate((N2D, NDD, 1)):
            views.append(None if tensors[3 * h + k] is None else grad[h, cut[k]:cut[k + 1]].view(cfg.B, ch, cfg.H, cfg.W))
    return grad, views


class _LossFunction(torch.autograd.Function):
    """result [8] of smap_loss_forward as a function of the head tensors; the gradient flows from result[0] alone."""

    @staticmethod
    def forward(ctx, cfg, labels, valids, rdepth, *tensors):
        result, ws = forward_raw(cfg, tensors, labels, valids, rdepth)
        ctx.cfg, ctx.present, ctx.ws = cfg, [t is not None for t in tensors], ws     # ws: neither input nor output, kept on ctx
        ctx.save_for_backward(labels, *[t for t in tensors if t is not None])
        return result

    @staticmethod
    @once_differentiable                                     # the gradient is a constant to autograd: a double backward raises
    def backward(ctx, grad_result):
        labels, *given = ctx.saved_tensors
        ws = ctx.ws
        given = iter(given)
        tensors = [next(given) if here else None for here in ctx.present]
        _, views = backward_raw(ctx.cfg, tensors, labels, ws, grad_result.contiguous())
        return (None, None, None, None) + tuple(views)


def _device_fp32(t, what, shape=None):
    """A dense fp32 device tensor, or the error the input rules ask for."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a torch.Tensor, got %s" % (what, type(t).__name__))
    if t.dtype != torch.float32:
        raise TypeError("%s: expected float32, got %s" % (what, t.dtype))
    if t.device.type != "cuda":
        raise ValueError("%s: the loss runs on the GPU (smap_amd has no CPU path), got device %s" % (what, t.device))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s: expected shape %s, got %s" % (what, tuple(shape), tuple(t.shape)))
    return t.contiguous()


def _valids_2d(valids, B, what="valids"):
    if isinstance(valids, torch.Tensor) and valids.dim() == 3 and valids.shape[2] == 1:
        valids = valids[:, :, 0]
    return _device_fp32(valids, what, (B, NC))


def _on_device(t, dev, what="another"):
    if t.device != dev:
        raise ValueError("all tensors live on one GPU: labels on %s, %s on %s" % (dev, what, t.device))
    return t


def _rdepth_rows(rdepth, B):
    rdepth = _device_fp32(rdepth, "rdepth")
    if rdepth.dim() != 3 or rdepth.shape[0] != B or rdepth.shape[2] != 3 or rdepth.shape[1] < 1:
        raise ValueError("rdepth: expected [%d, R >= 1, 3], got %s" % (B, tuple(rdepth.shape)))
    return rdepth


def _settings(stage_num, ohkm, topk, ctf):
    """(stage_num, ohkm, topk, ctf) of a criterion, checked."""
    stage_num, ohkm, topk, ctf = int(stage_num), bool(ohkm), int(topk), bool(ctf)
    if not 1 <= stage_num <= 4:
        raise ValueError("stage_num is 1 to 4, got %d" % stage_num)
    if ohkm and not 1 <= topk <= NDD:
        raise ValueError("topk is 1 to %d with ohkm, got %d" % (NDD, topk))
    return stage_num, ohkm, topk, ctf


def _check_inputs(crit, valids, labels, rdepth):
    """(_Config, labels, valids, rdepth) of checked inputs: the rules every criterion (its stage_num, ohkm, topk, ctf) shares."""
    labels = _device_fp32(labels, "labels")
    if labels.dim() != 5 or labels.shape[2] != NC or labels.shape[1] < 4 + int(crit.ctf):
        raise ValueError("labels: expected [B, S >= %d, 57, H, W], got %s" % (4 + int(crit.ctf), tuple(labels.shape)))
    B, S, _, H, W = labels.shape
    valids, rdepth = _valids_2d(valids, B), _rdepth_rows(rdepth, B)
    _on_device(valids, labels.device), _on_device(rdepth, labels.device)
    return _Config(crit.stage_num, crit.ohkm, crit.topk, crit.ctf, 0, B, S, rdepth.shape[1], H, W), labels, valids, rdepth


def _upsampled(t, what, ch, cfg, dev):
    """The shape rule of SMAPLoss: exactly (B, ch, H, W)."""
    return _on_device(_device_fp32(t, what, (cfg.B, ch, cfg.H, cfg.W)), dev)


def _native(t, what, ch, cfg, dev):
    """The shape rule of SMAPLossNative: (B, ch, h <= H, w <= W)."""
    t = _device_fp32(t, what)
    if t.dim() != 4 or tuple(t.shape[:2]) != (cfg.B, ch) or not (1 <= t.shape[2] <= cfg.H and 1 <= t.shape[3] <= cfg.W):
        raise ValueError("%s: expected [%d, %d, h <= %d, w <= %d], got %s" % (what, cfg.B, ch, cfg.H, cfg.W, tuple(t.shape)))
    return _on_device(t, dev, what)


def _head_tensors(outputs, cfg, dev, rule):
    """outputs[key][i][j] of every head in the library's order, each through the shape rule."""
    tensors = []
    for i in range(cfg.stage_num):
        for j in range(4):
            for key, ch in SOURCE_KEYS:
                what = "outputs['%s'][%d][%d]" % (key, i, j)
                try:
                    t = outputs[key][i][j]
                except (KeyError, IndexError, TypeError):
                    raise ValueError("%s is missing: %d stages of 4 heads each" % (what, cfg.stage_num))
                tensors.append(rule(t, what, ch, cfg, dev))
    return tensors


class SMAPLoss:
    """SMAP._calculate_loss on the GPU.

        criterion = SMAPLoss.from_cfg(cfg)               # or SMAPLoss(stage_num=3, ohkm=True, topk=8, ctf=True)
        losses = criterion(outputs, valids, labels, rdepth)
        losses["total_loss"].backward()

    outputs: dict with 'heatmap_2d', 'det_d', 'root_d', each a list of stage_num lists of 4 tensors [B, 43 | 14 | 1, H, W] (what
    SMAP.forward collects); valids [B, 57, 1] or [B, 57]; labels [B, S, 57, H, W] with S >= 4 + ctf; rdepth [B, R, 3].  All fp32 on one
    GPU.  Returns {'total_loss', 'loss_2d', 'loss_bone', 'loss_root'}: 0-d fp32 tensors, the last three detached."""

    _function, _shape_rule = _LossFunction, staticmethod(_upsampled)      # what a subclass replaces

    def __init__(self, stage_num=3, ohkm=True, topk=8, ctf=True, strict=False):
        self.stage_num, self.ohkm, self.topk, self.ctf = _settings(stage_num, ohkm, topk, ctf)
        self.strict = bool(strict)

    @classmethod
    def from_cfg(cls, cfg, strict=False):
        return cls(cfg.MODEL.STAGE_NUM, cfg.LOSS.OHKM, cfg.LOSS.TOPK, cfg.LOSS.COARSE_TO_FINE, strict)

    def _check(self, outputs, valids, labels, rdepth):
        cfg, labels, valids, rdepth = _check_inputs(self, valids, labels, rdepth)
        return cfg, _head_tensors(outputs, cfg, labels.device, self._shape_rule), labels, valids, rdepth

    def __call__(self, outputs, valids, labels, rdepth):
        cfg, tensors, labels, valids, rdepth = self._check(outputs, valids, labels, rdepth)
        result = self._function.apply(cfg, labels, valids, rdepth, *tensors)
        if self.strict:
            bad = int(result[4].item())                       # the one synchronisation of strict mode
            if bad:
                raise ValueError("rdepth: %d row(s) with Z > 0 lie outside the %d x %d map" % (bad, cfg.H, cfg.W))
        return result_dict(result, result.detach())

    forward = __call__


def _nchw_source(t):
    """HeadSource tuple of a dense [B, c, h, w] tensor."""
    _, c, h, w = t.shape
    return (t.data_ptr(), h, w, c, 1, h * w, c * h * w)


class _NativeLossFunction(torch.autograd.Function):
    """result [8] of smap_loss_forward_src as a function of the head tensors at their own resolutions; the gradient (smap_loss_backward_src)
    flows from result[0] alone, into one buffer from which the 3 * n_heads views are cut."""

    @staticmethod
    def forward(ctx, cfg, labels, valids, rdepth, *tensors):
        sources = [{key: _nchw_source(tensors[3 * h + k]) for k, (key, _) in enumerate(SOURCE_KEYS)} for h in range(cfg.n_heads)]
        result, ws = forward_from_sources(cfg, sources, labels, valids, rdepth)
        ctx.cfg, ctx.ws = cfg, ws
        ctx.save_for_backward(labels, *tensors)
        return result

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_result):
        labels, *tensors = ctx.saved_tensors
        cfg = ctx.cfg
        buf = torch.empty((sum(t.numel() for t in tensors),), dtype=torch.float32, device=labels.device)
        views, sources, grads, at = [], [], [], 0
        for h in range(cfg.n_heads):
            s, g = {}, {}
            for k, (key, _) in enumerate(SOURCE_KEYS):
                t = tensors[3 * h + k]
                v = buf[at:at + t.numel()].view(t.shape)
                at += t.numel()
                views.append(v)
                s[key], g[key] = _nchw_source(t), _nchw_source(v)
            sources.append(s)
            grads.append(g)
        backward_to_sources(cfg, sources, grads, labels, ctx.ws, grad_result.contiguous())
        return (None, None, None, None) + tuple(views)


class SMAPLossNative(SMAPLoss):
    """SMAPLoss on heads that were NOT upsampled: outputs[key][i][j] is [B, 43 | 14 | 1, h, w] with any 1 <= h <= H, 1 <= w <= W (H x W:
    the labels' size), the tensor the reference hands to F.interpolate(size=(H, W), mode='bilinear', align_corners=True).  The upsampling
    happens inside the reduction (smap_loss_forward_src) and its adjoint inside the backward pass (smap_loss_backward_src): no H x W
    tensor is written in either direction, the gradients arrive at the tensors' own resolutions in a fixed summation order (the same bits
    run to run).  Call signature, returned dict, `strict` and the differences from the reference are SMAPLoss's."""

    _function, _shape_rule = _NativeLossFunction, staticmethod(_native)


class EngineLoss:
    """SMAP._calculate_loss, forward only, on the heads of an all-heads engine (the validation loss).

        eng = model.engine(B, H, W, device, all_heads=True)
        eng.run(imgs, out=out)
        losses = EngineLoss.from_cfg(cfg)(eng.head_sources(out), valids, labels, rdepth)

    sources: BackboneEngine.head_sources() (or n_heads dicts of HeadSource tuples describing any fp32 device tensors); valids, labels,
    rdepth as SMAPLoss takes them.  Returns {'total_loss', 'loss_2d', 'loss_bone', 'loss_root'}: 0-d fp32 device tensors without
    grad_fn.  Runs on the current stream behind whatever wrote the sources; no synchronisation."""

    def __init__(self, stage_num=3, ohkm=True, topk=8, ctf=True):
        self.stage_num, self.ohkm, self.topk, self.ctf = _settings(stage_num, ohkm, topk, ctf)

    @classmethod
    def from_cfg(cls, cfg):
        return cls(cfg.MODEL.STAGE_NUM, cfg.LOSS.OHKM, cfg.LOSS.TOPK, cfg.LOSS.COARSE_TO_FINE)

    def check(self, valids, labels, rdepth):
        """(_Config, labels, valids, rdepth) of checked inputs: SMAPLoss's rules."""
        return _check_inputs(self, valids, labels, rdepth)

    def raw(self, sources, valids, labels, rdepth):
        """(result [8], workspace): result[4] counts the rows with Z > 0 outside the map (total_loss is NaN then)."""
        cfg, labels, valids, rdepth = self.check(valids, labels, rdepth)
        return forward_from_sources(cfg, sources, labels, valids, rdepth)

    def __call__(self, sources, valids, labels, rdepth):
        with torch.no_grad():
            result, _ = self.raw(sources, valids, labels, rdepth)
        return result_dict(result)

    def value_and_grad(self, sources, valids, labels, rdepth, upstream=None):
        """(losses, grads): the dict of __call__ and d (total_loss * upstream) / d source for every head tensor, at its own resolution --
        the seam a backward pass through the backbone starts from (smap_loss_backward_src).  grads: one dict per head of
        {"heatmap_2d", "det_d", "root_d": tensor [B, c, h, w]}, each in its source's own order: a view of a zeroed [B, h, w, pix_stride]
        buffer where the source is NHWC with a padded pixel, dense NCHW otherwise.  upstream: None (1) or a device fp32 tensor whose
        first element is read on the device.  No graph, no synchronisation."""
        with torch.no_grad():
            cfg, labels, valids, rdepth = self.check(valids, labels, rdepth)
            result, ws = forward_from_sources(cfg, sources, labels, valids, rdepth)
            dev = labels.device
            if upstream is None:
                upstream = torch.ones((1,), dtype=torch.float32, device=dev)
            upstream = _device_fp32(upstream, "upstream").reshape(-1)
            grads, desc = [], []
            for d in sources:
                g, gd = {}, {}
                for key, _ in SOURCE_KEYS:
                    _, sh, sw, c, pix, ch, _ = d[key]
                    if ch == 1 and pix >= c:                  # NHWC, the pixel padded as the source's is
                        buf = torch.zeros((cfg.B, sh, sw, pix), dtype=torch.float32, device=dev)
                        g[key] = buf[..., :c].permute(0, 3, 1, 2)
                        gd[key] = (buf.data_ptr(), sh, sw, c, pix, 1, sh * sw * pix)
                    else:
                        g[key] = torch.empty((cfg.B, c, sh, sw), dtype=torch.float32, device=dev)
                        gd[key] = _nchw_source(g[key])
                grads.append(g)
                desc.append(gd)
            backward_to_sources(cfg, sources, desc, labels, ws, upstream)
        return result_dict(result), grads


class ValidationLoss:
    """The validation loss of a run (exps/stage3_root2/test.py --eval_loss 1): per loader batch the labels, channel mask and root rows
    are rendered from the batch's annotations as the training set's sample does (smap_amd/labels.py: render_labels, valid_vector,
    root_depth_labels), the loss is model(imgs, valids, labels, rdepth), and the four values are accumulated ON THE DEVICE weighted by
    the batch's frames.  The value depends on the batch size, as the training log's does: the root term and the hard-keypoint mining
    are normalised per batch.  raw() is the run's one read-back."""

    KEYS = ("total_loss", "loss_2d", "loss_bone", "loss_root")

    def __init__(self, model, cfg, device):
        from .labels import label_spec, valid_vector
        self.model, self.device = model, torch.device(device)
        self.spec = label_spec(cfg)
        self.valid = torch.from_numpy(valid_vector(cfg.DATASET.NAME)[:, 0].astype(np.float32))      # ("MIX": the annotated sets carry every channel)
        self.sums = torch.zeros((4,), dtype=torch.float64, device=self.device)
        self.frames = self.batches = 0

    def inputs(self, annotations, metas):
        """(valids [B, 57], labels [B, S, 57, H, W], rdepth [B, MAX_PEOPLE, 3]) on the device for a batch's annotations [B][P, 15, C >= 8]
        in network pixels (zero rows = padding) and its per-frame dicts with 'scale'.  Visibilities of joints outside the map as held
        are cleared first (JointDataset.remove_illegal_joint; GtMapsSource does the same)."""
        from .labels import render_labels, root_depth_labels
        H, W = self.spec.shape
        frames = []
        for a in annotations:
            a = np.array(a.numpy() if isinstance(a, torch.Tensor) else a, np.float64)
            off = (a[:, :, 0] >= W * self.spec.stride) | (a[:, :, 0] < 0) | (a[:, :, 1] >= H * self.spec.stride) | (a[:, :, 1] < 0)
            a[:, :, 3][off] = 0
            frames.append(a)
        labels = render_labels(frames, self.spec, device=self.device)
        scale = lambda m: float(np.asarray(m["scale"] if isinstance(m, dict) else m).reshape(-1)[0])
        rdepth = np.stack([root_depth_labels(a, scale(m), self.spec) for a, m in zip(frames, metas)]).astype(np.float32)
        valids = self.valid[None].repeat(len(frames), 1)
        return valids.to(self.device), labels, torch.from_numpy(rdepth).to(self.device)

    def update(self, imgs, annotations, metas):
        """One batch: imgs [B, 3, H, W] on the device -- the batch's real, unmirrored frames."""
        valids, labels, rdepth = self.inputs(annotations, metas)
        losses = self.model(imgs, valids, labels, rdepth)
        n = int(imgs.shape[0])
        self.sums += torch.stack([losses[k] for k in self.KEYS]).double() * n
        self.frames += n
        self.batches += 1
        return losses

    def raw(self):
        """[sum of frames * total, ... * 2d, ... * bone, ... * root, frames, batches] as floats (synchronises)."""
        return [float(v) for v in self.sums.cpu()] + [float(self.frames), float(self.batches)]

    @staticmethod
    def merge_raws(raws):
        return [sum(col) for col in zip(*raws)]

    def result_entry(self, raw=None):
        raw = self.raw() if raw is None else raw
        frames = raw[4]
        entry = {k: (raw[i] / frames if frames else float("nan")) for i, k in enumerate(self.KEYS)}
        entry.update(frames=int(frames), batches=int(raw[5]))
        return {"loss": entry}

    def log_lines(self, raw=None):
        return ["validation loss over {frames} frames in {batches} batches: total {total_loss:.6g}  2d {loss_2d:.6g}  bone {loss_bone:.6g}  "
                "root {loss_root:.6g}".format(**self.result_entry(raw)["loss"])]


def single_head_loss(hm=None, dd=None, rd=None, labels=None, valids=None, rdepth=None, ohkm=False, topk=8):
    """ONE head with unit weights (smap_loss_forward's single mode), for lib/utils/loss_h.py: result [8] = (2D + depth + root, 2D,
    depth, root, bad_rows, ...), differentiable through its first element.  labels [B, S >= 1, 57, H, W] (scale 0 is read), valids
    [B, 57] in output order; either may be None when hm and dd are."""
    given = [t for t in (hm, dd, rd) if t is not None]
    if not given:
        raise ValueError("at least one of hm, dd, rd")
    B, _, H, W = given[0].shape
    tensors = [None if t is None else _device_fp32(t, name, (B, ch, H, W)) for t, name, ch in ((hm, "hm", N2D), (dd, "dd", NDD), (rd, "rd", 1))]
    S = 1
    if hm is not None or dd is not None:
        labels = _device_fp32(labels, "labels")
        if labels.dim() != 5 or tuple(labels.shape[2:]) != (NC, H, W) or labels.shape[0] != B:
            raise ValueError("labels: expected [%d, S, 57, %d, %d], got %s" % (B, H, W, tuple(labels.shape)))
        S = labels.shape[1]
        valids = _valids_2d(valids, B)
    else:
        labels = valids = None
    if rdepth is None:
        rdepth = torch.zeros((B, 1, 3), dtype=torch.float32, device=given[0].device)
    rdepth = _rdepth_rows(rdepth, B)
    cfg = _Config(1, ohkm, topk, False, 1, B, S, rdepth.shape[1], H, W)
    return _LossFunction.apply(cfg, labels, valids, rdepth, *tensors)
