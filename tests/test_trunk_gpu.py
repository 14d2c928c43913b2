"""Upsample_unit trunk on the GPU (smap_amd/trunk.py, csrc/trunk.hip) against the float64 restatement (tests/trunk_restate.py, itself
held to the reference's results by tests/test_trunk_cpu.py), with the interpolation weights of ATen's fp32 rule taken exactly.

Bounds are derived, never measured: every GEMM launch is an fp32 fmaf chain of known length K plus at most one bias addition, so on the
launch's actual inputs |err| <= (K + 2) * 2^-24 * sum |a * b| on every element (the + 2 holds gamma_K's second-order term while
K^2 * 2^-24 <= 2: every channel chain here; a reduction over P pixels has K = heads_restate.red_chain(P) <= slice_len + slices, one fmaf
chain per slice and reduce_fold's additions, never the pixel count itself, for which the condition fails from 5793 on);
upadd_forward rounds at most six times on any term, 6 * 2^-24 * (|S| + sum w |U| + |b|); upadd_adjoint is a chain of n fused multiply-adds whose weight is one rounded product,
(n + 3) * 2^-24 * sum w |gPre| with n the cell's tap count.  The composed passes propagate those bounds through the chain on magnitudes
(trunk_restate.forward_bounds / backward_bounds).  The measured / bound ratios are printed (`pytest -s`) and recorded in
profiles/trunk_parity.json.  ReLU sign ties (trunk_scenes.py): only where float64's |pre| lies within the tie bound of zero may the
kernel's mask differ; there, and only there, the composed check takes the kernel's mask."""
import ctypes as C

import pytest
import torch

import trunk_restate as R
import trunk_scenes as TS
import smap_amd.lib as L
from smap_amd import gemm_f32 as G
from smap_amd import trunk as T
from train_kit import DEV, GUARD, U, guarded, held, layouts, unfolded_held

pytestmark = pytest.mark.gpu
_cache = {}


def dims_of(s):
    return (TS.B, s["h"], s["w"], s["hp"], s["wp"], s["cin"], s["chl"])


def scene(name):
    """Device operands of a scene (fp32, folded on the device by gemm_f32.fold_bn), their float64 copies, and one forward + backward run."""
    if name in _cache:
        return _cache[name]
    s = TS.SCENES[name]
    x_np, p_np, g_np = TS.inputs(name)
    x, g = torch.from_numpy(x_np).to(DEV), torch.from_numpy(g_np).to(DEV)
    o_prev = None if p_np is None else torch.from_numpy(p_np).to(DEV)
    params = {k: v.to(DEV) for k, v in TS.weights(name).items()}
    with torch.no_grad():
        wu, wc, b = T.folded_trunk_weights(params, s["unit"], s["ind"], TS.EPS)
    o, fws = T.forward(x, o_prev, wu, wc, b)
    gwu, gwc, gb, gprev, gx, bws = T.backward(x, o_prev, o, wu, wc, g, want_gx=True)
    d = lambda t: None if t is None else t.detach().double().cpu()
    fv = {k: d(v) for k, v in T.workspace_views(fws, *dims_of(s), False).items()} if s["ind"] > 0 else {}
    bv = {k: d(v) for k, v in T.workspace_views(bws, *dims_of(s), True).items()}
    out = dict(s=s, x=x, o_prev=o_prev, g=g, params=params, wu=wu, wc=wc, b=b,
               raw=dict(o=o, gwu=gwu, gwc=gwc, gb=gb, gprev=gprev, gx=gx),
               got=dict(o=d(o), gwu=d(gwu), gwc=d(gwc), gb=d(gb), gprev=d(gprev), gx=d(gx), **fv, **bv),
               f64=dict(x=d(x), o_prev=d(o_prev), g=d(g), wu=d(wu), wc=d(wc), b=d(b)),
               it=R.Interp(s["hp"], s["wp"], s["h"], s["w"], fp32=True) if s["ind"] > 0 else None)
    _cache[name] = out
    return out


@pytest.mark.parametrize("name", list(TS.SCENES))
def test_every_launch_on_its_own_inputs(name):
    c = scene(name)
    f, got, s, it = c["f64"], c["got"], c["s"], c["it"]
    cin, chl = s["cin"], s["chl"]
    K, Kl = R.red_chain(TS.B * s["h"] * s["w"]), (R.red_chain(TS.B * s["hp"] * s["wp"]) if it is not None else 0)      # the sliced reductions' chain lengths
    print(name)
    if it is None:                                          # ONE launch: O = relu(X Wu^T + b), K = Cin
        held("O", got["o"], torch.relu(R.mm_launch(f["x"], f["wu"]) + f["b"]), (cin + 2) * U * (R.mm_launch(f["x"].abs(), f["wu"].abs()) + f["b"].abs()))
    else:
        held("S", got["s"], R.mm_launch(f["x"], f["wu"]), (cin + 2) * U * R.mm_launch(f["x"].abs(), f["wu"].abs()))
        held("U", got["u"], R.mm_launch(f["o_prev"], f["wc"]), (chl + 2) * U * R.mm_launch(f["o_prev"].abs(), f["wc"].abs()))
        held("O (upadd_forward)", got["o"], torch.relu(R.upadd_launch(got["s"], it.up(got["u"]), f["b"])),
             6 * U * (got["s"].abs() + it.up(got["u"].abs()) + f["b"].abs()))
    gpre = got["gpre"]
    assert torch.equal(gpre, f["g"] * (got["o"] > 0)), "gPre is a selection of gO by the kernel's own O"
    gw, gb = R.reduce_launch(gpre, f["x"])
    gw_mag, gb_mag = R.reduce_launch(gpre.abs(), f["x"].abs())
    held("gWu", got["gwu"], gw, (K + 2) * U * gw_mag)
    held("gb", got["gb"], gb, (K + 2) * U * gb_mag)
    held("gX", got["gx"], gpre @ f["wu"], (chl + 2) * U * (gpre.abs() @ f["wu"].abs()))
    if it is not None:
        held("gU (upadd_adjoint)", got["gu"], it.down(gpre), (it.taps[None, :, :, None] + 3) * U * it.down(gpre.abs()))
        gu = got["gu"]
        if (s["hp"], s["wp"]) == (s["h"], s["w"]):
            # identity interpolation: one pixel names each cell, with the weights 1 * 1, 1 * 0, 0 * 1 and 0 * 0, and fmaf(1, g, 0) = g while
            # fmaf(0, g, acc) = acc for finite g, whichever tap comes first
            assert bool(torch.isfinite(gpre).all()) and torch.equal(gu, gpre), "identity interpolation: gU is gPre"
        held("gWc", got["gwc"], R.reduce_launch(gu, f["o_prev"])[0], (Kl + 2) * U * R.reduce_launch(gu.abs(), f["o_prev"].abs())[0])
        held("gO_prev", got["gprev"], gu @ f["wc"], (chl + 2) * U * (gu.abs() @ f["wc"].abs()))


@pytest.mark.parametrize("name", list(TS.SCENES))
def test_composed_forward_and_backward(name):
    c = scene(name)
    f, got, it = c["f64"], c["got"], c["it"]
    print(name)
    pre, _, _ = R.forward(f["x"], f["o_prev"], f["wu"], f["wc"], f["b"], it)
    e_o, _ = R.forward_bounds(f["x"], f["o_prev"], f["wu"], f["wc"], f["b"], it)
    held("O", got["o"], torch.relu(pre), e_o)
    tie, pre_scene = TS.ties(name, c["x"].cpu(), None if c["o_prev"] is None else c["o_prev"].cpu(), f["wu"], f["wc"], f["b"])
    assert float((pre_scene - pre).abs().max()) <= 1e-12 * float(pre.abs().max())
    share = float(tie.double().mean())
    print("  ties %.4f %%" % (100 * share))
    assert share <= TS.TIE_CAP
    kernel_mask = got["o"] > 0
    assert torch.equal(kernel_mask[~tie], (pre > 0)[~tie])                 # away from the ties the two masks are the same
    mask = torch.where(tie, kernel_mask, pre > 0)
    want = R.backward(f["x"], f["o_prev"], f["wu"], f["wc"], f["g"], mask, it)
    e = R.backward_bounds(f["x"], f["o_prev"], f["wu"], f["wc"], f["g"], mask, it)
    for k, g in (("gpre", "gpre"), ("gwu", "gwu"), ("gb", "gb"), ("gx", "gx"), ("gu", "gu"), ("gwc", "gwc"), ("gprev", "gprev")):
        if k in want:
            held(k, got[g], want[k], e[k])


def run_all(x, o_prev, c):
    o, _ = T.forward(x, o_prev, c["wu"], c["wc"], c["b"])
    gwu, gwc, gb, gprev, gx, _ = T.backward(x, o_prev, o, c["wu"], c["wc"], c["g"], want_gx=True)
    return [t for t in (o, gwu, gwc, gb, gprev, gx) if t is not None]


@pytest.mark.parametrize("name", ["a", "b", "f", "g", "h", "i"])
def test_layouts_and_runs_give_the_same_bits(name):
    c = scene(name)
    xs = layouts(c["x"])
    ps = layouts(c["o_prev"]) if c["o_prev"] is not None else {k: None for k in xs}
    base = run_all(xs["f32"], ps["f32"], c)
    again = run_all(xs["f32"], ps["f32"], c)
    assert all(torch.equal(a, b) for a, b in zip(base, again)), "two runs"
    for what in xs:
        got = run_all(xs[what], ps[what], c)
        assert all(torch.equal(a, b) for a, b in zip(base, got)), what
    hi = c["x"].half()
    lo = (c["x"] - hi.float()).half()
    a, b = run_all(torch.stack([hi, lo], dim=3), ps["f16"], c), run_all(hi.float() + lo.float(), ps["f32"], c)
    assert all(torch.equal(p, q) for p, q in zip(a, b)), "hi + lo"
    assert not torch.equal(hi.float() + lo.float(), hi.float())


@pytest.mark.parametrize("name", ["a", "b", "d", "f", "g", "h", "i"])
def test_writes_stay_inside_the_described_elements(name):
    c = scene(name)
    s = c["s"]
    dims = dims_of(s)
    B, h, w, hp, wp, cin, chl = dims
    up = s["ind"] > 0
    P, Pl, gx_stride, tail = B * h * w, B * hp * wp, cin + 8, 4096
    fwd_bytes, bwd_bytes = T.workspace_bytes(*dims, False), T.workspace_bytes(*dims, True)
    lib, stream = L.load(), torch.cuda.current_stream().cuda_stream
    xd = G.x_descriptor(c["x"])[0]
    pd = C.byref(G.x_descriptor(c["o_prev"])[0]) if up else None
    wc = c["wc"].data_ptr() if up else None
    results = {}
    for byte in (0xFF, 0x7B):
        sizes = dict(o=P * chl, gwu=chl * cin, gb=chl, gx=P * gx_stride)
        if up:
            sizes.update(gwc=chl * chl, gprev=Pl * chl)
        bufs = {k: guarded(n, byte) for k, n in sizes.items()}
        fws = torch.full((fwd_bytes + tail,), byte, dtype=torch.uint8, device=DEV)
        bws = torch.full((bwd_bytes + tail,), byte, dtype=torch.uint8, device=DEV)
        ptr = lambda k: bufs[k][1].data_ptr() if k in bufs else None
        L.check(lib.smap_trunk_forward(C.byref(xd), pd, c["wu"].data_ptr(), wc, c["b"].data_ptr(), ptr("o"), *dims, fws.data_ptr(), fwd_bytes, stream),
                "smap_trunk_forward")
        L.check(lib.smap_trunk_backward(C.byref(xd), pd, ptr("o"), c["wu"].data_ptr(), wc, c["g"].data_ptr(), ptr("gwu"), ptr("gwc"), ptr("gb"),
                                        ptr("gprev"), ptr("gx"), gx_stride, *dims, bws.data_ptr(), bwd_bytes, stream), "smap_trunk_backward")
        torch.cuda.synchronize()
        assert bool((fws[fwd_bytes:] == byte).all()) and bool((bws[bwd_bytes:] == byte).all()), "workspace beyond ws_bytes"
        described = {}
        for k, (buf, payload) in bufs.items():
            raw = buf.view(-1, 4)
            assert bool((raw[:GUARD] == byte).all()) and bool((raw[-GUARD:] == byte).all()), (k, "guards")
            if k == "gx":                                         # padded pixels: the padding floats stay
                rows = payload.view(P, gx_stride)
                assert bool((rows[:, cin:].contiguous().view(torch.uint8) == byte).all()), (k, "padding channels")
                described[k] = rows[:, :cin].clone()
            else:
                described[k] = payload.clone()
        results[byte] = described
    for k in results[0xFF]:
        assert torch.equal(results[0xFF][k], results[0x7B][k]), k
        assert bool(torch.isfinite(results[0xFF][k]).all()), k
        assert torch.equal(results[0xFF][k].view_as(c["raw"][k]), c["raw"][k]), k         # and they are the scene's results


@pytest.mark.parametrize("name", ["b", "d"])
def test_unit_trunk_autograd_reaches_the_unfolded_parameters(name):
    """UnitTrunk under torch.autograd with gemm_f32.fold_bn in front: the gradients at conv.weight, conv.bias, bn.weight, bn.bias of u_skip and
    up_conv and at O_prev against the restatement's chain rule (frozen statistics).  Bound: the folded gradients' composed bounds carried
    through the fold's Jacobian on magnitudes, plus torch's own fp32 fold arithmetic: (n + 8) * 2^-24 on the magnitudes of its terms,
    n = the terms of bn.weight's sum (the conv's fan-in + 1).  The ONE gb tensor of the call goes to both biases: bit-equal gradients."""
    c = scene(name)
    f, s, it = c["f64"], c["s"], c["it"]
    print(name)
    mods = TS.module_names(name)
    keys = [k for k in c["params"] if k.rsplit(".", 2)[-2] + "." + k.rsplit(".", 1)[-1] in TS.PARAM_KINDS]
    params = {k: v.clone().requires_grad_(k in keys) for k, v in c["params"].items()}
    o_prev = c["o_prev"].clone().requires_grad_(True)
    sink = {}
    o = T.unit_trunk(c["x"], o_prev, params, s["unit"], s["ind"], TS.EPS, sink=sink)
    assert torch.equal(o, c["raw"]["o"])
    (c["g"] * o).sum().backward()
    assert torch.equal(o_prev.grad, c["raw"]["gprev"]) and torch.equal(sink["gx"], c["raw"]["gx"])
    assert all(params[k].grad is None for k in params if k not in keys)          # running statistics: no gradient
    assert torch.equal(params[mods[0] + ".bn.bias"].grad, params[mods[1] + ".bn.bias"].grad)
    assert torch.equal(params[mods[0] + ".bn.bias"].grad, c["raw"]["gb"])
    pre, _, _ = R.forward(f["x"], f["o_prev"], f["wu"], f["wc"], f["b"], it)
    tie, _ = TS.ties(name, c["x"].cpu(), c["o_prev"].cpu(), f["wu"], f["wc"], f["b"])
    mask = torch.where(tie, c["got"]["o"] > 0, pre > 0)
    want = R.backward(f["x"], f["o_prev"], f["wu"], f["wc"], f["g"], mask, it)
    e = R.backward_bounds(f["x"], f["o_prev"], f["wu"], f["wc"], f["g"], mask, it)
    for m, gw, ew in ((mods[0], want["gwu"], e["gwu"]), (mods[1], want["gwc"], e["gwc"])):
        unfolded_held(m, params, lambda k: params[k].grad, gw, want["gb"], ew, e["gb"], TS.EPS)
