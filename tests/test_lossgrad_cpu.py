"""CPU suite of the loss gradient at the heads' native resolution: the numpy restatement (tests/lossgrad_restate.py) against the
reference's autograd through F.interpolate in float64 (tests/golden/lossgrad.npz), its negative controls, and the argument errors of
smap_loss_backward_src that need no device."""
import ctypes as C

import numpy as np
import pytest

import lossgrad_restate as R
import lossgrad_scenes as GS

U = 2.0 ** -24
K_INDEX = 3          # |delta l| <= K_INDEX * U * (in - 1): see index_rule_bound


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(f"{golden_dir}/lossgrad.npz")


@pytest.fixture(scope="module", params=list(GS.SCENES))
def scene(request):
    name = request.param
    s, x = GS.SCENES[name], GS.inputs(name)
    return name, s, x, R.forward(s, x)


def index_rule_bound(n_in):
    """How far a weight of the fp32 index rule (lerp_index) lies from the float64 rule's (ATen on the reference's float64 tensors).
    scale = fl((in - 1) / (out - 1)) is one rounding of an exact quotient, src = fl(scale * dst) one more: |delta src| <= 2 U src <=
    2 U (in - 1).  l1 = src - i0 is exact (src and i0 lie within 1 of each other), the clamp changes nothing in range, l0 = fl(1 - l1)
    is one rounding of a number <= 1: U / 2 <= U (in - 1) / 2.  A weight as a function of src is the hat function, Lipschitz 1, so a
    tap index that flips between the two rules moves no cell's weight by more than |delta src| either.  Hence k = 3 (2.5 rounded up
    for the second-order terms); in = 1 and in = out have exact weights."""
    return K_INDEX * U * (n_in - 1)


def near(n_in, n_out):
    """[n_out, n_in] 0 / 1: the source indices whose weight may differ between the two rules at all -- i0 - 1 .. i0 + 2."""
    i0 = R.lerp_index(n_in, n_out)[0]
    i = np.arange(n_in)[None]
    return ((i >= i0[:, None] - 1) & (i <= i0[:, None] + 2)).astype(np.float64)


def compare(name, s, x, fwd, golden, variant=None):
    """Worst |restatement - reference| / bound over every element of every native gradient of a scene.  The bound per element, all
    computed here: the weights differ by at most dy = index_rule_bound(h), dx = index_rule_bound(w) (zero where the size is 1 or the
    output's), carried linearly through the gradient  g = Wy^T e Wx,  e = f * (Wy v Wx^T - label):
        dy * near_y^T |e| Wx + dx * Wy^T |e| near_x + dy dx near_y^T |e| near_x                    (the adjoint's own weights)
      + |f| (3 dy + 3 dx + 9 dy dx) max |v| * Wy^T 1 Wx                                          (up itself: three cells a dimension)
    times 1.01 for what is of second order, plus 1e-12 relative for the float64 arithmetic of both sides and 2^-32 |g| for the stored
    gradient's 32 mantissa bits.  Tensors of H x W: coef * (out - label) from the fixture, 1e-12 relative."""
    H, W, B = s["H"], s["W"], s["B"]
    got = R.gradients(s, x, variant=variant, fwd=fwd)
    f = np.abs(fwd["coef"] * s["upstream"])
    worst = 0.0
    for h in range(4 * s["stage_num"]):
        sh, sw = x["src"][h][0].shape[2:]
        same = (sh, sw) == (H, W)
        dy = 0.0 if sh in (1, H) else index_rule_bound(sh)
        dx = 0.0 if sw in (1, W) else index_rule_bound(sw)
        wy, wx, ny, nx = R.weights(sh, H), R.weights(sw, W), near(sh, H), near(sw, W)
        e = np.abs(fwd["diff"][h]) * f[h][:, :, None, None]
        con = lambda a, b: a.T @ e @ b
        vmax = np.abs(np.concatenate(x["src"][h][:2], axis=1)).max(axis=(2, 3))
        bound = dy * con(ny, wx) + dx * con(wy, nx) + dy * dx * con(ny, nx)
        bound = bound + (f[h] * vmax * (3 * dy + 3 * dx + 9 * dy * dx))[:, :, None, None] * np.outer(wy.sum(0), wx.sum(0))
        bound = 1.01 * bound + 1e-12 * con(wy, wx)
        for k, (first, n) in enumerate(((0, R.N2D), (R.N2D, R.NDD))):
            if same:
                lab = x["labels"][:, GS.head_scale(s, h)][:, R.LABEL_CHANNEL[first:first + n]].astype(np.float64)
                want = golden["%s_coef%d_%d" % (name, h, k)][:, :, None, None] * (x["src"][h][k].astype(np.float64) - lab)
            else:
                want = golden["%s_g%d_%d" % (name, h, k)]
            allowed = bound[:, first:first + n] + 2.0 ** -32 * np.abs(want) + 1e-300
            worst = max(worst, float((np.abs(got[h][k] - want) / allowed).max()))
        # root_d: every row adds factor * outer(Wy[y], Wx[x])
        want = golden["%s_g%d_2" % (name, h)]
        allowed = np.zeros_like(want)
        for b, y, xx, fac in fwd["root"][h]:
            allowed[b, 0] += abs(fac * s["upstream"]) * (1.01 * (dy + dx + dy * dx) * np.outer(ny[y], nx[xx]) + 1e-12 * np.outer(wy[y], wx[xx]))
        allowed += 2.0 ** -32 * np.abs(want) + 1e-300
        worst = max(worst, float((np.abs(got[h][2] - want) / allowed).max()))
    return worst


def test_restatement_matches_the_reference_autograd(scene, golden):
    """Every element of every native gradient of every scene within the bound compare() computes (the only difference between the two
    sides is the fp32 index rule against the reference's float64 one); the four losses within 1e-6 relative."""
    name, s, x, fwd = scene
    assert golden[name + "_seed"] == s["seed"] and golden[name + "_upstream"] == s["upstream"]
    losses = golden[name + "_losses"]
    print(name, "losses", fwd["losses"], "reference", losses)
    assert (np.abs(fwd["losses"] - losses) <= 1e-6 * np.abs(losses)).all()
    worst = compare(name, s, x, fwd, golden)
    print(name, "gradients: worst error / bound", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("variant", ["drop_l1_into_last", "l0_both", "ignore_upstream"])
def test_wrong_restatements_are_flagged(golden, variant):
    """The negative controls: a restatement that loses the l1 weight that lands on the last source row or column, one that uses l0 for
    both taps, one that ignores upstream (scenes whose upstream is 1 cannot tell) -- the comparison of the test above must flag each on
    every scene it can change, or its bound is too loose."""
    for name, s in GS.SCENES.items():
        if variant == "ignore_upstream" and s["upstream"] == 1.0:
            continue
        x = GS.inputs(name)
        worst = compare(name, s, x, R.forward(s, x), golden, variant)
        print(variant, name, "worst error / bound", worst)
        assert worst > 1.0, (variant, name)


def test_dropping_l1_where_both_taps_coincide_cannot_be_told_apart(golden):
    """The control 'drop the l1 weight where i0 == i1' as the adjoint's definition words it.  Under lerp_index the taps coincide only
    at i0 = in - 1, which needs src = fl(scale * dst) >= in - 1 while src <= (in - 1)(1 + 2 U): the dropped weight is at most
    2 U (in - 1), inside index_rule_bound by construction, so NO sound bound can flag it.  Asserted here: that size of the dropped
    weights over every geometry of the scenes, and that the comparison passes with them dropped (its ratio is printed next to the
    true restatement's).  The flaggable form of the same mistake is 'drop_l1_into_last' above."""
    for name, s in GS.SCENES.items():
        for n_out, dim in ((s["H"], 0), (s["W"], 1)):
            for size in s["sizes"]:
                i0, i1, _, l1 = R.lerp_index(size[dim], n_out)
                assert (l1[i0 == i1] <= 2 * U * max(size[dim] - 1, 0)).all()
        x = GS.inputs(name)
        fwd = R.forward(s, x)
        worst, true = compare(name, s, x, fwd, golden, "drop_l1_at_last"), compare(name, s, x, fwd, golden)
        print(name, "worst error / bound with l1 dropped where i0 == i1", worst, "true restatement", true)
        assert worst <= 1.0


# ---- the C ABI's argument errors that need no device -------------------------------------------------------------------------------
def _descriptors(L, sizes, n_heads, B, base=0x10000):
    arr = (L.HeadSrc * (3 * n_heads))()
    for h in range(n_heads):
        sh, sw = sizes[h % 4]
        for k, c in enumerate((43, 14, 1)):
            arr[3 * h + k] = L.HeadSrc(base + 4096 * (3 * h + k), sh, sw, c, 1, sh * sw, c * sh * sw)
    return arr


def test_backward_src_argument_errors_without_a_device():
    """smap_loss_backward_src_scratch_bytes is host arithmetic; smap_loss_backward_src refuses every bad argument before it launches
    anything (the pointers below are never dereferenced on the host)."""
    from smap_amd import lib as L
    from smap_amd.loss import workspace_layout
    lib = L.load()
    sizes, n_heads, B, R, H, W = [(2, 3), (4, 6), (8, 12), (16, 24)], 12, 2, 3, 16, 24
    src = _descriptors(L, sizes, n_heads, B)
    want = sum(B * 57 * sh * sw * 16 for sh, sw in sizes) * 3
    assert lib.smap_loss_backward_src_scratch_bytes(src, n_heads, B) == want
    assert lib.smap_loss_backward_src_scratch_bytes(None, n_heads, B) == -1
    assert lib.smap_loss_backward_src_scratch_bytes(src, 0, B) == -1 and lib.smap_loss_backward_src_scratch_bytes(src, 17, B) == -1
    assert lib.smap_loss_backward_src_scratch_bytes(src, n_heads, 0) == -1
    src[4].h = 0
    assert lib.smap_loss_backward_src_scratch_bytes(src, n_heads, B) == -1
    wsb = workspace_layout(n_heads, B, R)["bytes"]
    need = want - 3 * B * 57 * 16 * 24 * 16

    def call(edit_src=None, edit_grad=None, src_=True, grads_=True, labels=0x1000000, wsp=0x2000000, wsb=wsb, scratch=0x3000000, sb=need,
             upstream=0x4000000, stage_num=3, topk=8, S=5, H=H, W=W, B=B):
        s, g = _descriptors(L, sizes, n_heads, B), _descriptors(L, sizes, n_heads, B, 0x800000)
        if edit_src:
            edit_src(s)
        if edit_grad:
            edit_grad(g)
        return lib.smap_loss_backward_src(s if src_ else None, g if grads_ else None, labels, stage_num, 1, topk, 1, B, S, R, H, W, wsp, wsb,
                                          scratch, sb, upstream, None)

    def setter(i, **kw):
        def edit(arr):
            for k, val in kw.items():
                setattr(arr[i], k, val)
        return edit

    bad = [dict(src_=False), dict(grads_=False), dict(labels=None), dict(wsp=None), dict(wsp=0x2000004), dict(wsb=wsb - 8), dict(upstream=None),
           dict(scratch=None), dict(scratch=0x3000008), dict(sb=need - 4), dict(stage_num=5), dict(topk=15), dict(S=4), dict(H=15), dict(B=0),
           dict(edit_src=setter(0, ptr=None)), dict(edit_src=setter(4, ptr=0x10002)), dict(edit_src=setter(0, c=42)),
           dict(edit_src=setter(9, h=17)), dict(edit_src=setter(0, pix_stride=2, ch_stride=3)),
           dict(edit_grad=setter(0, h=3)), dict(edit_grad=setter(1, w=2)), dict(edit_grad=setter(2, c=2)), dict(edit_grad=setter(3, ptr=0x800002)),
           dict(edit_grad=setter(5, pix_stride=2, ch_stride=3)), dict(edit_grad=setter(0, pix_stride=42, ch_stride=1)),
           dict(edit_grad=setter(0, frame_stride=0))]
    for kw in bad:
        assert call(**kw) == -1, kw
