"""Head arms on the GPU (smap_amd/heads.py, csrc/heads.hip) against the float64 restatement (tests/heads_restate.py, itself held to
the reference's results by tests/test_heads_cpu.py).

Bounds are derived, never measured: every launch is an fp32 fmaf chain of known length K plus one bias addition, so on the launch's
actual inputs |err| <= (K + 2) * 2^-24 * sum |a * b| on every element.  The second-order term of gamma_K fits in the + 2 while
K^2 * 2^-24 <= 2, that is up to K = 5792: true of every channel chain here, NOT of a chain over the pixels (16562 in l91x91) -- and a
reduction over P pixels is no such chain: its K is heads_restate.red_chain(P), at most K_red(P) = slice_len + slices, one fmaf chain
per slice and reduce_fold's additions of the slices in order, for which K_red asserts the condition.  The composed passes propagate
that bound through the chain on magnitudes (heads_restate.forward_bounds / backward_bounds).  The measured / bound ratios are printed (`pytest -s`) and recorded in DESIGN.md section 18.
ReLU sign ties (heads_scenes.py): only where float64's |Z| lies within the forward's own bound of zero may the kernel's mask differ;
there, and only there, the composed check takes the kernel's mask, read from the workspace's M."""
import pytest
import torch

import heads_restate as R
import heads_scenes as HS
from smap_amd import gemm_f32 as G
from smap_amd import heads as H
from train_kit import DEV, GUARD, U, guarded, held, layouts, unfolded_held

pytestmark = pytest.mark.gpu
_cache = {}


def scene(name):
    """Device operands of a scene (fp32, folded on the device by gemm_f32.fold_bn), their float64 copies, and one forward + backward run."""
    if name in _cache:
        return _cache[name]
    s = HS.SCENES[name]
    x_np, g_np = HS.inputs(name)
    x = torch.from_numpy(x_np).to(DEV)
    g = [torch.from_numpy(a).to(DEV) for a in g_np]
    params = {k: v.to(DEV) for k, v in HS.weights(name).items()}
    arms = HS.module_names(name)
    with torch.no_grad():
        w1cat, b1cat, w2, b2 = H.folded_unit_weights(params, arms, HS.EPS)
    ys = [torch.empty((HS.B, c, s["h"], s["w"]), dtype=torch.float32, device=DEV) for c in HS.ARM_C]
    H.forward(x, w1cat, b1cat, w2, b2, [H.nchw_source(y) for y in ys])
    gw1, gb1, gw2, gb2, gx, ws = H.backward(x, w1cat, b1cat, w2, [H.nchw_source(t) for t in g])
    v = H.workspace_views(ws, HS.B, s["h"], s["w"], s["chl"])
    d = lambda t: t.detach().double().cpu()
    out = dict(s=s, x=x, g=g, params=params, arms=arms, w1cat=w1cat, b1cat=b1cat, w2=w2, b2=b2,
               got=dict(y=[d(y) for y in ys], gw1=d(gw1), gb1=d(gb1), gw2=[d(t) for t in gw2], gb2=[d(t) for t in gb2], gx=d(gx),
                        m=d(v["m"]).flatten(3), gz=d(v["gz"]).flatten(3)),
               raw=dict(y=ys, gw1=gw1, gb1=gb1, gw2=gw2, gb2=gb2, gx=gx),
               f64=dict(x=d(x), g=[d(t) for t in g], w1cat=d(w1cat), b1cat=d(b1cat), w2=[d(t) for t in w2], b2=[d(t) for t in b2]))
    _cache[name] = out
    return out


@pytest.mark.parametrize("name", list(HS.SCENES))
def test_every_launch_on_its_own_inputs(name):
    c = scene(name)
    f, got, chl = c["f64"], c["got"], c["s"]["chl"]
    K = R.red_chain(HS.B * c["s"]["h"] * c["s"]["w"])           # the sliced reductions' chain length
    print(name)
    # Z | M: K = chl
    z = R.z_launch(f["x"], f["w1cat"], f["b1cat"])
    held("M", got["m"], torch.relu(z), (chl + 2) * U * R.z_launch(f["x"].abs(), f["w1cat"].abs(), f["b1cat"].abs()))
    m_k, gz_k = R.arms(got["m"], chl), got["gz"]
    for a in range(3):
        ca = HS.ARM_C[a]
        held("Y_%d" % a, got["y"][a], R.y_launch(m_k[a], f["w2"][a], f["b2"][a]),
             (9 * chl + 2) * U * R.y_launch(m_k[a], f["w2"][a].abs(), f["b2"][a].abs()))
        want = R.gm_launch(f["g"][a], f["w2"][a]) * (m_k[a] > 0)
        held("gZ_%d" % a, R.arms(gz_k, chl)[a], want, (9 * ca + 2) * U * R.gm_launch(f["g"][a].abs(), f["w2"][a].abs()) * (m_k[a] > 0))
        gw, gb = R.gw2_launch(f["g"][a], m_k[a])
        gw_mag, gb_mag = R.gw2_launch(f["g"][a].abs(), m_k[a])
        held("gW2_%d" % a, got["gw2"][a], gw, (K + 2) * U * gw_mag)
        held("gb2_%d" % a, got["gb2"][a], gb, (K + 2) * U * gb_mag)
    gw, gb = R.gw1_launch(gz_k, f["x"])
    gw_mag, gb_mag = R.gw1_launch(gz_k.abs(), f["x"].abs())
    held("gW1", got["gw1"], gw, (K + 2) * U * gw_mag)
    held("gb1", got["gb1"], gb, (K + 2) * U * gb_mag)
    held("gX", got["gx"], R.gx_launch(gz_k, f["w1cat"]), (3 * chl + 2) * U * R.gx_launch(gz_k.abs(), f["w1cat"].abs()))


@pytest.mark.parametrize("name", list(HS.SCENES))
def test_composed_forward_and_backward(name):
    c = scene(name)
    f, got, chl = c["f64"], c["got"], c["s"]["chl"]
    print(name)
    z, ys = R.forward(f["x"], f["w1cat"], f["b1cat"], f["w2"], f["b2"])
    e_m, e_y = R.forward_bounds(f["x"], f["w1cat"], f["b1cat"], f["w2"], f["b2"], z)
    for a in range(3):
        held("Y_%d" % a, got["y"][a], ys[a], e_y[a])
    tie, _ = HS.ties(name, f["x"], f["w1cat"], f["b1cat"])
    assert float(tie.double().mean()) <= HS.TIE_CAP
    kernel_mask = got["m"] > 0
    assert torch.equal(kernel_mask[~tie], (z > 0)[~tie])                 # away from the ties the two masks are the same
    mask = torch.where(tie, kernel_mask, z > 0)
    want = R.backward(f["x"], f["w1cat"], f["w2"], f["g"], z, mask)
    e = R.backward_bounds(f["x"], f["w1cat"], f["w2"], f["g"], z, mask, e_m)
    held("gZ", got["gz"], want["gz"], e["gz"])
    for a in range(3):
        held("gW2_%d" % a, got["gw2"][a], want["gw2"][a], e["gw2"][a])
        held("gb2_%d" % a, got["gb2"][a], want["gb2"][a], e["gb2"][a])
    for k in ("gw1", "gb1", "gx"):
        held(k, got[k], want[k], e[k])


def padded_nhwc(B, c, h, w, pad_to, fill=None):
    """A [B, h, w, pad_to] buffer and the HeadSource tuple of its first c channels."""
    buf = torch.zeros((B, h, w, pad_to), dtype=torch.float32, device=DEV) if fill is None else fill
    return buf, (buf.data_ptr(), h, w, c, pad_to, 1, h * w * pad_to)


PADS = (48, 16, 8)


def run_all(x, c, nhwc):
    """Forward and backward with X as given and the heads in one of the two HeadSource orders; every result as a dense tensor."""
    s = c["s"]
    B, h, w = HS.B, s["h"], s["w"]
    if nhwc:
        ybufs, ysrc = zip(*[padded_nhwc(B, ca, h, w, p) for ca, p in zip(HS.ARM_C, PADS)])
        gbufs = []
        for g, p in zip(c["g"], PADS):
            buf = torch.full((B, h, w, p), float("nan"), dtype=torch.float32, device=DEV)       # padding channels must never be read
            buf[..., :g.shape[1]] = g.permute(0, 2, 3, 1)
            gbufs.append(buf)
        gsrc = [padded_nhwc(B, ca, h, w, p, buf)[1] for ca, p, buf in zip(HS.ARM_C, PADS, gbufs)]
    else:
        ybufs = [torch.empty((B, ca, h, w), dtype=torch.float32, device=DEV) for ca in HS.ARM_C]
        ysrc, gsrc = [H.nchw_source(y) for y in ybufs], [H.nchw_source(g) for g in c["g"]]
    H.forward(x, c["w1cat"], c["b1cat"], c["w2"], c["b2"], list(ysrc))
    gw1, gb1, gw2, gb2, gx, ws = H.backward(x, c["w1cat"], c["b1cat"], c["w2"], list(gsrc))
    ys = [(y[..., :ca].permute(0, 3, 1, 2) if nhwc else y).contiguous() for y, ca in zip(ybufs, HS.ARM_C)]
    v = H.workspace_views(ws, B, h, w, s["chl"])
    return ys + [gw1, gb1, gx, v["m"].clone(), v["gz"].clone()] + gw2 + gb2


@pytest.mark.parametrize("name", ["o5x7", "o5x7w", "s33x41", "l91x91", "w9x15"])
def test_layouts_and_runs_give_the_same_bits(name):
    c = scene(name)
    variants = layouts(c["x"])                                 # values every layout can hold
    hi = c["x"].half()
    lo = (c["x"] - hi.float()).half()                          # a second case for the planes: hi + lo, rounded once to fp32
    base = run_all(variants["f32"], c, nhwc=False)
    again = run_all(variants["f32"], c, nhwc=False)
    assert all(torch.equal(a, b) for a, b in zip(base, again)), "two runs"
    for what, x in variants.items():
        for nhwc in (False, True):
            got = run_all(x, c, nhwc)
            assert all(torch.equal(a, b) for a, b in zip(base, got)), (what, nhwc)
    planes = torch.stack([hi, lo], dim=3)
    summed = hi.float() + lo.float()
    a, b = run_all(planes, c, nhwc=True), run_all(summed, c, nhwc=False)
    assert all(torch.equal(p, q) for p, q in zip(a, b)), "hi + lo"
    assert not torch.equal(summed, hi.float())


@pytest.mark.parametrize("name", ["b2x3", "o5x7w", "s33x41", "l91x91", "w9x15"])
def test_writes_stay_inside_the_described_elements(name):
    import ctypes as C
    import smap_amd.lib as L
    c = scene(name)
    s = c["s"]
    B, h, w, chl = HS.B, s["h"], s["w"], s["chl"]
    P, gx_stride = B * h * w, chl + 8
    ws_bytes, tail = H.workspace_bytes(B, h, w, chl, True), 4096
    results = {}
    for byte in (0xFF, 0x7B):
        sizes = dict(gw1=3 * chl * chl, gb1=3 * chl, gx=P * gx_stride)
        for a, (ca, p) in enumerate(zip(HS.ARM_C, PADS)):
            sizes.update({"y%d" % a: P * p, "gw2_%d" % a: ca * chl * 9, "gb2_%d" % a: ca})
        bufs = {k: guarded(n, byte) for k, n in sizes.items()}
        ws = torch.full((ws_bytes + tail,), byte, dtype=torch.uint8, device=DEV)
        ysrc = [(bufs["y%d" % a][1].data_ptr(), h, w, ca, p, 1, h * w * p) for a, (ca, p) in enumerate(zip(HS.ARM_C, PADS))]
        lib, stream = L.load(), torch.cuda.current_stream().cuda_stream
        xd = G.x_descriptor(c["x"])[0]
        ptrs = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
        srcs = lambda ss: (L.HeadSrc * 3)(*[L.HeadSrc(p, sh, sw, sc, pix, ch, 0, fr) for p, sh, sw, sc, pix, ch, fr in ss])
        L.check(lib.smap_heads_forward(C.byref(xd), c["w1cat"].data_ptr(), c["b1cat"].data_ptr(), ptrs(c["w2"]), ptrs(c["b2"]), srcs(ysrc),
                                       B, h, w, chl, ws.data_ptr(), ws_bytes, stream), "smap_heads_forward")
        L.check(lib.smap_heads_backward(C.byref(xd), c["w1cat"].data_ptr(), c["b1cat"].data_ptr(), ptrs(c["w2"]),
                                        srcs([H.nchw_source(g) for g in c["g"]]), B, h, w, chl, bufs["gw1"][1].data_ptr(),
                                        bufs["gb1"][1].data_ptr(), ptrs([bufs["gw2_%d" % a][1] for a in range(3)]),
                                        ptrs([bufs["gb2_%d" % a][1] for a in range(3)]), bufs["gx"][1].data_ptr(), gx_stride, ws.data_ptr(),
                                        ws_bytes, stream), "smap_heads_backward")
        torch.cuda.synchronize()
        assert bool((ws[ws_bytes:] == byte).all()), "workspace beyond ws_bytes"
        described = {}
        for k, (buf, payload) in bufs.items():
            raw = buf.view(-1, 4)
            assert bool((raw[:GUARD] == byte).all()) and bool((raw[-GUARD:] == byte).all()), (k, "guards")
            if k[0] == "y" or k == "gx":                          # padded pixels: the padding floats stay
                width, used = (PADS[int(k[1])], HS.ARM_C[int(k[1])]) if k[0] == "y" else (gx_stride, chl)
                rows = payload.view(P, width)
                assert bool((rows[:, used:].contiguous().view(torch.uint8) == byte).all()), (k, "padding channels")
                described[k] = rows[:, :used].clone()
            else:
                described[k] = payload.clone()
        results[byte] = described
    for k in results[0xFF]:
        assert torch.equal(results[0xFF][k], results[0x7B][k]), k
        assert bool(torch.isfinite(results[0xFF][k]).all()), k
    # and they are the scene's results
    for a, ca in enumerate(HS.ARM_C):
        assert torch.equal(results[0xFF]["y%d" % a].view(B, h, w, ca).permute(0, 3, 1, 2), c["raw"]["y"][a])
        assert torch.equal(results[0xFF]["gw2_%d" % a].view_as(c["raw"]["gw2"][a]), c["raw"]["gw2"][a])
    assert torch.equal(results[0xFF]["gx"].view_as(c["raw"]["gx"]), c["raw"]["gx"])
    assert torch.equal(results[0xFF]["gw1"].view_as(c["raw"]["gw1"]), c["raw"]["gw1"])


@pytest.mark.parametrize("name", ["o5x7", "f16x24"])
def test_unit_heads_autograd_reaches_the_unfolded_parameters(name):
    """UnitHeads under torch.autograd with gemm_f32.fold_bn in front: the gradients at conv.weight, conv.bias, bn.weight, bn.bias of the six
    modules and at X against the restatement's chain rule (frozen statistics).  Bound: the folded gradients' composed bounds carried
    through the fold's Jacobian on magnitudes, plus torch's own fp32 fold arithmetic: (n + 8) * 2^-24 on the magnitudes of its terms,
    n = the terms of bn.weight's sum (the conv's fan-in + 1)."""
    c = scene(name)
    f, chl = c["f64"], c["s"]["chl"]
    print(name)
    keys = [k for k in c["params"] if k.rsplit(".", 2)[-2] + "." + k.rsplit(".", 1)[-1] in HS.PARAM_KINDS]
    params = {k: v.clone().requires_grad_(k in keys) for k, v in c["params"].items()}
    x = c["x"].clone().requires_grad_(True)
    ys = H.unit_heads(x, params, c["arms"], HS.EPS)
    assert all(torch.equal(y, r) for y, r in zip(ys, c["raw"]["y"]))
    sum((g * y).sum() for g, y in zip(c["g"], ys)).backward()
    assert torch.equal(x.grad, c["raw"]["gx"])
    assert all(params[k].grad is None for k in params if k not in keys)          # running statistics: no gradient
    z, _ = R.forward(f["x"], f["w1cat"], f["b1cat"], f["w2"], f["b2"])
    e_m, _ = R.forward_bounds(f["x"], f["w1cat"], f["b1cat"], f["w2"], f["b2"], z)
    tie, _ = HS.ties(name, f["x"], f["w1cat"], f["b1cat"])
    mask = torch.where(tie, c["got"]["m"] > 0, z > 0)
    want = R.backward(f["x"], f["w1cat"], f["w2"], f["g"], z, mask)
    e = R.backward_bounds(f["x"], f["w1cat"], f["w2"], f["g"], z, mask, e_m)
    for a, (c1, c2) in enumerate(c["arms"]):
        sl = slice(a * chl, (a + 1) * chl)
        for m, gw, gb, ew, eb in ((c1, want["gw1"][sl], want["gb1"][sl], e["gw1"][sl], e["gb1"][sl]),
                                  (c2, want["gw2"][a], want["gb2"][a], e["gw2"][a], e["gb2"][a])):
            unfolded_held(m, params, lambda k: params[k].grad, gw, gb, ew, eb, HS.EPS)
