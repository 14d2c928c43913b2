"""GPU suite of the loss gradient at the heads' native resolution (csrc/loss.hip smap_loss_backward_src, smap_amd/loss.py SMAPLossNative,
EngineLoss.value_and_grad, SMAP.loss_and_head_gradients): the kernels against the numpy restatement tests/lossgrad_restate.py (which
tests/test_lossgrad_cpu.py holds against the reference's autograd), determinism, the bytes they may touch, autograd, and the engine seam."""
import functools

import numpy as np
import pytest
import torch

import lossgrad_restate as R
import lossgrad_scenes as GS
import valloss_inputs as VI
from helpers import make_cfg
from recipe import recipe_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("heatmap_2d", "det_d", "root_d")
CHANNELS = (43, 14, 1)
PADS = (48, 16, 8)            # the pixel strides the engine's head convs leave
GUARD = 8                     # floats before and after every gradient buffer
U = 2.0 ** -24


def scene_of(name):
    return GS.REAL if name == "real" else GS.SCENES[name]


@functools.lru_cache(maxsize=None)
def inputs_of(name):
    return GS.inputs(scene_of(name))


@functools.lru_cache(maxsize=None)
def restated_forward(name):
    return R.forward(scene_of(name), inputs_of(name))


class Run:
    """A scene's native tensors on the device in one layout, gradient buffers of the same layout between guard floats, everything
    filled with one byte first; run(): smap_loss_forward_src, then smap_loss_backward_src."""

    def __init__(self, name, layout, fill=0xFF, edit=None):
        from smap_amd.engine import HeadSource
        from smap_amd.loss import _Config
        s, x = scene_of(name), inputs_of(name)
        self.s, self.B, self.n_heads = s, s["B"], 4 * s["stage_num"]
        self.fill, self.hold, self.bufs, self.src, self.dst, self.geom = fill, [], [], [], [], []
        for h in range(self.n_heads):
            d, g = {}, {}
            for k, (key, c) in enumerate(zip(KEYS, CHANNELS)):
                a = x["src"][h][k] if edit is None else edit(h, k, x["src"][h][k])
                v = torch.from_numpy(a).to(DEV)
                sh, sw = v.shape[2:]
                if layout == "nchw":
                    t, strides = v.contiguous(), (1, sh * sw, c * sh * sw)
                else:                                      # NHWC, a padded pixel with junk behind the last channel
                    t = torch.full((self.B, sh, sw, PADS[k]), 1e30, dtype=torch.float32, device=DEV)
                    t[..., :c] = v.permute(0, 2, 3, 1)
                    strides = (PADS[k], 1, sh * sw * PADS[k])
                buf = torch.empty((self.B * strides[2] + 2 * GUARD,), dtype=torch.float32, device=DEV)
                buf.view(torch.uint8).fill_(fill)
                d[key] = HeadSource(t.data_ptr(), sh, sw, c, *strides)
                g[key] = HeadSource(buf.data_ptr() + 4 * GUARD, sh, sw, c, *strides)
                self.hold.append(t)
                self.bufs.append(buf)
                self.geom.append((c, sh, sw, strides))
            self.src.append(d)
            self.dst.append(g)
        self.labels, self.valids, self.rdepth = (torch.from_numpy(x[k]).to(DEV) for k in ("labels", "valids", "rdepth"))
        self.cfg = _Config(s["stage_num"], s["ohkm"], s["topk"], s["ctf"], 0, self.B, s["S"], self.rdepth.shape[1], s["H"], s["W"])
        self.upstream = torch.tensor([s["upstream"]], dtype=torch.float32, device=DEV)

    def run(self):
        from smap_amd.loss import backward_to_sources, forward_from_sources, workspace_views
        self.result, self.ws = forward_from_sources(self.cfg, self.src, self.labels, self.valids, self.rdepth)
        backward_to_sources(self.cfg, self.src, self.dst, self.labels, self.ws, self.upstream)
        self.views = workspace_views(self.ws, self.n_heads, self.B, self.cfg.R)
        return self

    def grad(self, i):
        """[B, c, h, w] view of gradient buffer i = 3 * head + k through its descriptor."""
        c, sh, sw, (pix, ch, frame) = self.geom[i]
        return torch.as_strided(self.bufs[i], (self.B, c, sh, sw), (frame, ch, sw * pix, pix), GUARD)

    def untouched(self, i):
        """The bytes of buffer i outside the described elements still hold the fill."""
        mask = torch.ones_like(self.bufs[i], dtype=torch.bool)
        c, sh, sw, (pix, ch, frame) = self.geom[i]
        torch.as_strided(mask, (self.B, c, sh, sw), (frame, ch, sw * pix, pix), GUARD).fill_(False)
        rest = self.bufs[i][mask].view(torch.uint8)
        return bool((rest == self.fill).all()) and int(mask.sum()) >= 2 * GUARD


@functools.lru_cache(maxsize=None)
def ran(name, layout, fill=0xFF):
    return Run(name, layout, fill).run()


def interval(n_in, n_out):
    """The largest number of output indices that share one i0."""
    return int(np.bincount(R.lerp_index(n_in, n_out)[0]).max())


def check_against_restatement(name, run):
    """Worst |kernel - restatement| / bound over every gradient element; the restatement is fed the kernel's own coef table, so f is the
    same fp32 number on both sides and what differs is the kernel's fp32 arithmetic alone.  Bound per element, from the kernel as
    written (csrc/loss.hip, -ffp-contract=off: every operation rounds once), with w = wy * wx the restated weights:
      * up: each tap passes through a product, a sum, a product and a sum -> 4 U sum |weight * source| =: 4 U |up|; the subtraction
        adds U |up - label| <= U (|up| + |label|), the product with f one more U |e|: k1 = 6 on sum w |f| (|up| + |label|);
      * the contractions: a term passes through the product with l(x) and at most nx sums, the product with l(y) and at most ny sums
        (nx, ny: the longest interval in x and y), then at most 8 sums of the fold's nine partial sums: k2 = 1,
        n = nx + ny + 2 + 9, on sum w |e|;
      bound = U * (6 * sum w |f| (|up| + |label|) + n * sum w |e|) * 1.001 (second order).  A source of H x W: the same formula with unit
      weights covers its two roundings.  root_d: per row root_fac's rounding to fp32, the product with upstream, the product of the two
      weights, the product of both and one sum per row on the cell: U * (4 + R) * sum over the rows of |factor * wy * wx|."""
    s, x, fwd = scene_of(name), inputs_of(name), restated_forward(name)
    H, W = s["H"], s["W"]
    coef = run.views["coef"].cpu().numpy()
    want = R.gradients(s, x, coef=coef, fwd=fwd)
    f = np.abs((coef * np.float32(s["upstream"])).astype(np.float32).astype(np.float64))
    sel = run.views["sel"].cpu().numpy()
    assert np.array_equal(coef != 0, fwd["coef"] != 0) and (sel.sum() > 0), "the kernel and the restatement mine the same channels"
    worst = 0.0
    for h in range(run.n_heads):
        sh, sw = x["src"][h][0].shape[2:]
        wy, wx = R.weights(sh, H), R.weights(sw, W)
        n = interval(sh, H) + interval(sw, W) + 11
        lab = np.abs(x["labels"][:, GS.head_scale(s, h)][:, R.LABEL_CHANNEL].astype(np.float64))
        fh = f[h][:, :, None, None]
        con = lambda a: wy.T @ a @ wx
        bound = U * (6 * con(fh * (fwd["abs_up"][h] + lab)) + n * con(np.abs(fwd["diff"][h]) * fh)) * 1.001
        got = torch.cat([run.grad(3 * h), run.grad(3 * h + 1)], 1).cpu().numpy().astype(np.float64)
        err = np.abs(got - np.concatenate(want[h][:2], axis=1))
        zero = f[h] == 0
        assert (got[zero] == 0).all(), "a zero-factor channel is exactly zero"
        worst = max(worst, float((err / (bound + 1e-300))[~zero].max()))
        rbound = np.zeros_like(want[h][2])
        for b, y, xx, fac in fwd["root"][h]:
            rbound[b, 0] += abs(fac * s["upstream"]) * np.outer(wy[y], wx[xx])
        rbound = U * (4 + run.cfg.R) * rbound
        rerr = np.abs(run.grad(3 * h + 2).cpu().numpy().astype(np.float64) - want[h][2])
        assert (rerr[rbound == 0] == 0).all(), "root_d is exactly zero away from the rows' taps"
        if (rbound > 0).any():
            worst = max(worst, float((rerr[rbound > 0] / rbound[rbound > 0]).max()))
    return worst


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("name", list(GS.SCENES))
def test_kernel_matches_the_restatement(name, layout):
    run = ran(name, layout)
    assert float(run.result[4]) == 0 and bool(torch.isfinite(run.result[:4]).all())
    losses = restated_forward(name)["losses"]
    assert (np.abs(run.result[:4].cpu().numpy() - losses) <= 2e-6 * np.abs(losses)).all()
    worst = check_against_restatement(name, run)
    print(name, layout, "gradients: worst error / bound", worst)
    assert worst <= 1.0


def test_one_head_group_at_the_real_geometry():
    """stage_num = 1, B = 1, 128 x 208 with sources 16x26, 32x52, 64x104, 128x208: intervals of 8 and 9 pixels (ratios 127 / 15 and
    207 / 25), more cells than one workgroup's threads."""
    run = ran("real", "nchw")
    worst = check_against_restatement("real", run)
    print("real geometry: worst error / bound", worst)
    assert worst <= 1.0


def nested(tensors, stage_num):
    return {key: [[tensors[3 * (4 * i + j) + k] for j in range(4)] for i in range(stage_num)] for k, key in enumerate(KEYS)}


def native_leaves(name, edit=None):
    x = inputs_of(name)
    return [torch.from_numpy(a if edit is None else edit(h, k, a)).to(DEV).requires_grad_(True) for h, head in enumerate(x["src"])
            for k, a in enumerate(head)]


def criterion(name, **kw):
    from smap_amd.loss import SMAPLossNative
    s = scene_of(name)
    return SMAPLossNative(s["stage_num"], s["ohkm"], s["topk"], s["ctf"], **kw)


def test_native_loss_equals_forward_src_and_autograd_fills_every_leaf():
    """SMAPLossNative's four values are smap_loss_forward_src's on the same (NCHW) descriptors bit for bit; total_loss.backward() fills
    .grad of all 36 leaves with what smap_loss_backward_src writes for upstream 1; (2 * total).backward() gives exactly the double (f
    doubles exactly, and so does every sum); a second derivative raises; forward and backward run under torch's synchronisation debug
    mode: no host synchronisation."""
    name = "small"
    s, x = scene_of(name), inputs_of(name)
    run = ran(name, "nchw")
    leaves = native_leaves(name)
    assert len(leaves) == 36
    labels, valids, rdepth = run.labels, run.valids, run.rdepth
    crit = criterion(name)
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = crit(nested(leaves, s["stage_num"]), valids[:, :, None], labels, rdepth)
        got["total_loss"].backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert list(got) == ["total_loss", "loss_2d", "loss_bone", "loss_root"]
    for n, k in enumerate(got):
        assert torch.equal(got[k].detach().view(torch.int32), run.result[n].view(torch.int32)), k
        assert got[k].dim() == 0 and (got[k].grad_fn is not None) == (k == "total_loss")
    first = [t.grad.clone() for t in leaves]
    assert all(g is not None and g.shape == t.shape and bool(torch.isfinite(g).all()) for g, t in zip(first, leaves))
    assert sum(int((g != 0).sum()) for g in first) > 10000
    # against the raw entry point at upstream 1: the same bits
    one = Run(name, "nchw")
    one.upstream = torch.ones(1, dtype=torch.float32, device=DEV)
    one.run()
    for i, g in enumerate(first):
        assert torch.equal(g.view(torch.int32), one.grad(i).view(torch.int32)), i
    for t in leaves:
        t.grad = None
    (2 * crit(nested(leaves, s["stage_num"]), valids, labels, rdepth)["total_loss"]).backward()
    for g, t in zip(first, leaves):
        assert torch.equal(t.grad, 2 * g)
    total = crit(nested(leaves, s["stage_num"]), valids, labels, rdepth)["total_loss"]
    g, = torch.autograd.grad(total, leaves[0], create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


@pytest.mark.parametrize("name", list(GS.SCENES))
def test_same_bits_run_to_run_and_in_both_layouts(name):
    a, b = ran(name, "nchw"), Run(name, "nchw").run()
    c = ran(name, "nhwc")
    assert torch.equal(a.result.view(torch.int32), b.result.view(torch.int32))
    for i in range(3 * a.n_heads):
        assert torch.equal(a.grad(i).view(torch.int32), b.grad(i).view(torch.int32)), i
        assert torch.equal(a.grad(i).view(torch.int32), c.grad(i).view(torch.int32)), ("layouts", i)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_only_the_described_elements_are_written(layout):
    """Gradient buffers, their padding floats and guard floats filled with 0xFF, then with 0x7B: the written elements are the same bytes
    under both fills, every other byte still holds its fill."""
    for name in ("small", "odd"):
        a, b = ran(name, layout, 0xFF), ran(name, layout, 0x7B)
        for i in range(3 * a.n_heads):
            assert torch.equal(a.grad(i).view(torch.int32), b.grad(i).view(torch.int32)), (name, i)
            assert a.untouched(i) and b.untouched(i), (name, i)
            assert not bool(torch.isnan(a.grad(i)).any()), "0xFF is a NaN: every described element was written"


def test_zero_factor_channel_with_nan_in_its_source_plane():
    """Frame 1 of 'small' carries the COCO mask: its depth channels weigh zero.  NaN in such a source plane (head 0, det_d channel 2,
    and the finest head's channel 5): those gradients are exactly 0 -- the planes are not read -- and every other element of those
    heads keeps the clean run's bits."""
    def edit(h, k, a):
        if k == 1 and h in (0, 3):
            a = a.copy()
            a[1, 2 if h == 0 else 5] = np.nan
        return a

    clean = ran("small", "nchw")
    for layout in ("nchw", "nhwc"):
        run = Run("small", layout, edit=edit).run()
        for h, ch in ((0, 2), (3, 5)):
            g = run.grad(3 * h + 1)
            assert bool((g[1, ch] == 0).all())
            assert torch.equal(g.view(torch.int32), clean.grad(3 * h + 1).view(torch.int32))
            assert torch.equal(run.grad(3 * h).view(torch.int32), clean.grad(3 * h).view(torch.int32))


def test_row_outside_the_map_gives_finite_gradients_and_nan_total():
    name = "ratios"
    s = scene_of(name)
    run = ran(name, "nchw")
    rdepth = run.rdepth.clone()
    rdepth[0, 0] = torch.tensor([3.0, float(s["W"]) + 2.0, 1.0])
    leaves = native_leaves(name)
    got = criterion(name)(nested(leaves, s["stage_num"]), run.valids, run.labels, rdepth)
    assert bool(torch.isnan(got["total_loss"]))
    got["total_loss"].backward()
    assert all(bool(torch.isfinite(t.grad).all()) for t in leaves)
    with pytest.raises(ValueError, match="outside"):
        criterion(name, strict=True)(nested(leaves, s["stage_num"]), run.valids, run.labels, rdepth)


def test_argument_errors():
    from smap_amd import lib as L
    from smap_amd.loss import backward_to_sources, source_scratch_bytes
    name = "ratios"
    s = scene_of(name)
    run = ran(name, "nchw")
    leaves = [t.detach() for t in native_leaves(name)]
    big = list(leaves)
    big[3] = torch.zeros((s["B"], 43, s["H"] + 1, 2), device=DEV)
    with pytest.raises(ValueError, match=r"outputs\['heatmap_2d'\]\[0\]\[1\]"):
        criterion(name)(nested(big, 1), run.valids, run.labels, run.rdepth)
    big[3] = torch.zeros((s["B"], 43, 2, s["W"] + 1), device=DEV)
    with pytest.raises(ValueError, match=r"outputs\['heatmap_2d'\]\[0\]\[1\]"):
        criterion(name)(nested(big, 1), run.valids, run.labels, run.rdepth)
    # the C entry point: mismatched grads geometry, short scratch, null upstream
    lib = L.load()
    cfg = run.cfg
    need = source_scratch_bytes(cfg, run.src, run.dst)
    assert 0 < need <= lib.smap_loss_backward_src_scratch_bytes(arr(L, run.src), run.n_heads, run.B)
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call(dst=run.dst, sb=need, upstream=run.upstream.data_ptr(), sp=scratch.data_ptr()):
        return lib.smap_loss_backward_src(arr(L, run.src), arr(L, dst), run.labels.data_ptr(), cfg.stage_num, cfg.ohkm, cfg.topk, cfg.ctf, cfg.B,
                                          cfg.S, cfg.R, cfg.H, cfg.W, run.ws.data_ptr(), run.ws.numel(), sp, sb, upstream,
                                          torch.cuda.current_stream().cuda_stream)

    assert call() == 0
    wrong = [dict(d) for d in run.dst]
    wrong[2]["det_d"] = wrong[2]["det_d"]._replace(h=wrong[2]["det_d"].h - 1)
    assert call(dst=wrong) == -1
    wrong = [dict(d) for d in run.dst]
    wrong[0]["root_d"] = wrong[0]["root_d"]._replace(c=14)
    assert call(dst=wrong) == -1
    assert call(sb=need - 4) == -1 and call(sp=scratch.data_ptr() + 4) == -1 and call(sp=None) == -1
    assert call(upstream=None) == -1
    with pytest.raises(L.SmapError):
        backward_to_sources(cfg, run.src, wrong, run.labels, run.ws, run.upstream)
    torch.cuda.synchronize()


def arr(L, descs):
    a = (L.HeadSrc * (3 * len(descs)))()
    for h, d in enumerate(descs):
        for k, key in enumerate(KEYS):
            v = d[key]
            a[3 * h + k] = L.HeadSrc(v.ptr, v.h, v.w, v.c, v.pix_stride, v.ch_stride, 0, v.frame_stride)
    return a


def test_null_gradient_descriptors_are_left_out():
    """A null grads pointer: that tensor's buffer keeps its fill, the others the full run's bits."""
    name = "odd"
    full = ran(name, "nhwc")
    run = Run(name, "nhwc")
    skip = (1, 5, 9, 23)
    for i in skip:
        h, k = divmod(i, 3)
        run.dst[h][KEYS[k]] = run.dst[h][KEYS[k]]._replace(ptr=0)
    run.run()
    for i in range(3 * run.n_heads):
        if i in skip:
            assert bool((run.bufs[i].view(torch.uint8) == 0xFF).all()), i
        else:
            assert torch.equal(run.grad(i).view(torch.int32), full.grad(i).view(torch.int32)), i


def test_engine_seam_equals_the_native_loss_on_copies_of_the_head_sources():
    """The small schedule of test_valloss_gpu.py (2 x 64 x 96, precision x3): SMAP.loss_and_head_gradients -- the heads where the engine
    leaves them, padded NHWC, gradients in the same layout -- equals SMAPLossNative applied to dense NCHW copies of
    eng.head_sources(out): the four losses and every gradient element bit for bit."""
    from smap_amd.loss import SMAPLossNative
    from smap_amd.model.smap import SMAP
    from test_valloss_gpu import source_tensor
    torch.manual_seed(0)
    net = SMAP(make_cfg((16, 24))).eval()
    net.load_state_dict(recipe_state_dict(net.state_dict()))
    net = net.to(DEV)
    net.precision = "x3"
    x = torch.from_numpy(np.load(f"{GS.__file__.rsplit('/', 1)[0]}/backbone_small.npz")["x"]).to(DEV)
    inp = {k: torch.from_numpy(v).to(DEV) for k, v in VI.inputs("coco").items()}
    losses, grads = net.loss_and_head_gradients(x, inp["valids"], inp["labels"], inp["rdepth"])
    eng = net.engine(2, 64, 96, x.device, all_heads=True)
    out = eng.new_output()
    eng.run(x, out=out)
    leaves = [source_tensor(eng, d[key], out).contiguous().clone().requires_grad_(True) for d in eng.head_sources(out) for key in KEYS]
    got = SMAPLossNative(3, True, 8, True)(nested(leaves, 3), inp["valids"], inp["labels"], inp["rdepth"])
    got["total_loss"].backward()
    assert bool(torch.isfinite(got["total_loss"]))
    for k in got:
        assert torch.equal(got[k].detach().view(torch.int32), losses[k].view(torch.int32)), k
        assert losses[k].grad_fn is None
    nonzero = 0
    for h, d in enumerate(grads):
        for k, key in enumerate(KEYS):
            g = d[key]
            assert g.shape == leaves[3 * h + k].shape and g.grad_fn is None
            assert torch.equal(g.contiguous().view(torch.int32), leaves[3 * h + k].grad.view(torch.int32)), (h, key)
            nonzero += int((g != 0).sum())
    assert nonzero > 10000
    with pytest.raises(RuntimeError, match="eval"):
        net.train().loss_and_head_gradients(x, inp["valids"], inp["labels"], inp["rdepth"])
    net.eval()
