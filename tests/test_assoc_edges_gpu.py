"""GPU: the HIP association / lifting / refinement kernels on CONSTRUCTED edge inputs (tests/assoc_scenes.py; their preconditions are
checked on the CPU in tests/test_assoc_edges_cpu.py), bit for bit against the CPU oracle and against answers known independently of it."""
import numpy as np
import pytest
import torch

import assoc_scenes as S
from helpers import synth_scene
from recipe import recipe_state_dict
from oracle import oracle_lib as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------ C1: depth order
_VECTORS = S.depth_vectors()
_CHUNKS = [_VECTORS[i:i + 15] for i in range(0, len(_VECTORS), 15)]


@pytest.mark.parametrize("chunk", range(len(_CHUNKS)), ids=[f"{c[0][0]}..{c[-1][0]}" for c in _CHUNKS])
def test_depth_order_of_the_group_kernel_on_constructed_depth_vectors(chunk):
    """kv_std_sort of the group kernel (iterative introsort, one lane on LDS) on root depths it never met in natural scenes: equal depths
    among more than 16 persons (median-of-three and unguarded-partition order visible), ascending / descending / organ-pipe, the
    heap-sort fallback (organ-pipe and the antiquicksort adversary at n = 127 reach depth == 0), the NaN-last order, and n <= 16
    (insertion sort only).  Fewer necks than persons: the order decides who gets one.  bodys / counts / peaks / scores equal O.connect
    bit for bit and, independently of the oracle, the roots come out in torch.sort's order.  The last chunk also carries
    synth_scene(20, seed=320), the tie scene of the CPU suite."""
    import dapalib
    items = [(n, S.grid_scene(d), d) for n, d in _CHUNKS[chunk]]
    if chunk == len(_CHUNKS) - 1:
        h, r, _, _ = synth_scene(20, seed=320)
        items.append(("synth20-320", (h, r), None))
    assert len(items) <= 16
    hms, rd = dev(np.stack([s[0] for _, s, _ in items])), dev(np.stack([s[1] for _, s, _ in items]))
    bodys, counts, peaks, scores = [t.cpu().numpy() for t in dapalib.connect_batch(hms, rd, return_intermediate=True)]
    for i, (name, (h, r), d) in enumerate(items):
        ob, opk, osc = O.connect(h, r)
        P = len(ob)
        assert np.array_equal(bits(peaks[i]), bits(opk)) and np.array_equal(bits(scores[i]), bits(osc)), name
        assert counts[i] == P and np.array_equal(bits(bodys[i, :P]), bits(ob)) and not bodys[i, P:].any(), name
        if d is None:
            d = np.array([r[int(opk[2, k + 1, 1]), int(opk[2, k + 1, 0])] for k in range(P)], np.float32)
            assert len(np.unique(d)) < P
        assert P == len(d)
        idx = torch.from_numpy(d.copy()).sort(0, False)[1].numpy()
        assert np.array_equal(bodys[i, :P, 2, :2], peaks[i, 2, 1 + idx, :2]), name


# ------------------------------------------------------------------ C2: score ties
def test_score_ties_go_to_the_lowest_candidate_index():
    """group_limb's arg-max on bitwise-equal scores: the tie between one lane's c0 and c1 (j = i + 64), between c0 of a lane and c1 of
    a lower lane, across two lanes' c0 and across two lanes' c1 -- two persons at different depths per tie, so used0 / used1 must
    retire exactly the candidate taken (bidx >= 64 included).  distFlag off and on (the penalty lowers both tied scores alike),
    rootIdx 2 (limb tree on five waves) and 0 (flat order on one wave).  Bit-equal to the oracle, and the known answer: the nearer
    person takes the lowest index, the other the next.  One destination coincides with its source: its score is -1, so the
    penalty's limb == 0 is never divided by and the person stays without that joint."""
    import dapalib
    hms, rd, info = S.tie_scene()
    h, r = dev(hms[None]), dev(rd[None])
    pk = O.nms(hms)
    sc = O.paf_score(hms, pk)
    for root in (2, 0):
        for dist in (False, True):
            bodys, counts, peaks, scores = [t.cpu().numpy() for t in
                                            dapalib.connect_batch(h, r, rootIdx=root, distFlag=dist, return_intermediate=True)]
            assert np.array_equal(bits(peaks[0]), bits(pk)) and np.array_equal(bits(scores[0]), bits(sc))
            ob = O.group(pk, sc, rd, root, dist)
            assert counts[0] == len(ob) == 9 and np.array_equal(bits(bodys[0, :9]), bits(ob)) and not bodys[0, 9:].any(), (root, dist)
            S.check_tie_answers(bodys[0, :9], info[root], root)


# ------------------------------------------------------------------ C3: NMS / PAF known answers, both peak-search forms
@pytest.mark.parametrize("size", S.KNOWN_ANSWER_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nms_and_paf_known_answers_on_both_peak_search_forms(size):
    """The questions the oracle is asked in test_oracle_cpu.py (plateau, border row, value == threshold, 300 peaks against the 127 cap
    in raster order, straight limb and its fallbacks, close points) plus clipped 7x7 windows holding negative values at x = 1, y = 1,
    x = W - 2, y = H - 2, one pixel in both end channels of a limb (norm <= 1e-6: -1) and a short limb whose default score
    sqrt(W * H) / 150 decides -- put to smap_nms_ws (extract_batch) AND to the single-launch smap_nms (fused_nms=True)."""
    import dapalib
    scenes = S.known_answer_scenes(*size)
    hms = dev(np.stack([h for _, h, _ in scenes]))
    for fused in (False, True):
        pk, sc = [t.cpu().numpy() for t in dapalib.extract_batch(hms, fused_nms=fused)]
        for i, (name, h, check) in enumerate(scenes):
            opk = O.nms(h)
            assert np.array_equal(bits(pk[i]), bits(opk)), (name, fused)
            assert np.array_equal(bits(sc[i]), bits(O.paf_score(h, opk))), (name, fused)
            check(pk[i], sc[i])


# ------------------------------------------------------------------ C4: scale_hms_
@pytest.mark.parametrize("case", ["odd-area", "grid-stride", "misaligned", "aligned"])
def test_scale_hms_scalar_kernel_and_alignment(case):
    """scale_hms_kernel_scalar, the path for H * W % 4 != 0 or a base pointer off 16-byte alignment, against IEEE division on the
    host: an odd area (13x21), 2 x 43 x 99 x 63 > 2048 x 256 elements (the scalar kernel's grid-stride loop iterates), a contiguous
    16x24 tensor whose storage offset puts the base 4 bytes off alignment; the aligned 16x24 tensor (float4 kernel) as the control."""
    import dapalib
    B, H, W = {"odd-area": (1, 13, 21), "grid-stride": (2, 99, 63), "misaligned": (2, 16, 24), "aligned": (2, 16, 24)}[case]
    n = B * 43 * H * W
    x = torch.randn(n, generator=torch.Generator().manual_seed(3)) * 100
    want = x.clone().view(B, 43, H, W)
    want[:, :15] /= 255            # test.py:111-112
    want[:, 15:] /= 127
    off = 1 if case == "misaligned" else 0
    buf = torch.zeros(n + 2, device=DEV)
    t = buf[off:off + n].view(B, 43, H, W)
    t.copy_(x.view(B, 43, H, W))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * off
    if case == "grid-stride":
        assert n > 2048 * 256 and (H * W) % 4
    if case == "odd-area":
        assert (H * W) % 2 == 1
    z = dapalib.scale_hms_(t)
    assert z.data_ptr() == t.data_ptr() and torch.equal(z.cpu(), want)
    assert buf[:off].eq(0).all() and buf[off + n:].eq(0).all()         # nothing written beside the tensor


# ------------------------------------------------------------------ C5: flip_merge_
@pytest.mark.parametrize("table", ["config", "non-involutive"])
@pytest.mark.parametrize("B,H,W", [(1, 13, 21), (3, 13, 21), (1, 16, 24), (3, 16, 24)])
def test_flip_merge_odd_width_batch_one_and_any_table(B, H, W, table):
    """flip_merge_kernel at an odd W, at batch 1 and with a pair table that is not an involution (a pair[c] read on the wrong side
    shows), against the elementwise formula in fp32 on the host in the kernel's operation order -- and merge_flip for the config table."""
    import dapalib
    from exps.stage3_root2.config import cfg
    from exps.stage3_root2.test_util import merge_flip
    g = torch.Generator().manual_seed(9)
    a = torch.randn(B, 43, H, W, generator=g) * 50
    b = torch.randn(B, 43, H, W, generator=g) * 50
    if table == "config":
        pair = list(cfg.DATASET.KEYPOINT.FLIP_ORDER) + [15 + c for c in cfg.DATASET.PAF.FLIP_CHANNEL]
    else:
        pair = np.random.default_rng(4).permutation(43).tolist()
        assert any(pair[pair[c]] != c for c in range(43)) and sorted(pair) == list(range(43))
    f = b[:, pair].flip(-1)
    neg = torch.tensor([c >= 15 and (c - 15) % 2 == 0 for c in range(43)]).view(1, 43, 1, 1)
    want = a + torch.where(neg, f * -1.0, f)
    want[:, 15:] = want[:, 15:] * 0.5
    if table == "config":
        assert torch.equal(want, merge_flip(a.clone(), b, cfg))
    got = dapalib.flip_merge_(a.to(DEV), b.to(DEV), pair)
    assert torch.equal(got.cpu(), want)


# ------------------------------------------------------------------ D: lifting and refinement
@pytest.fixture(scope="module")
def refine_weights():
    from smap_amd.model.refinenet import RefineNet
    net = RefineNet().eval()
    net.load_state_dict(recipe_state_dict(net.state_dict()))
    wt, bs = net.folded(DEV)
    return wt, bs, [w.t().contiguous().cpu().numpy() for w in wt], [b.cpu().numpy() for b in bs]


@pytest.mark.parametrize("size", [(16, 24), (128, 208)], ids=["16x24", "128x208"])
def test_lift_and_refine_random_edges_vs_oracle(size, refine_weights):
    """lift_kernel<false|true> and refine_kernel<float|double> against O.lift / O.lift_gt / O.refine / O.refine_gt, every bit: person
    counts 0, 1, 2, 17, 127, 5 (P = 0 and P = 127 among them), limbs exactly vertical (stepx == 0), horizontal (stepy == 0) and of
    length zero, 4 * coord and the ten samples on exact halves (rint: half to even), depth maps on 5 levels (ties at the percentile
    clamps), joints and one root per frame with score 0, an odd camera scale.  The fp32 refinement accumulates in the oracle's order
    without contraction: equality, not a tolerance."""
    import dapalib
    H, W = size
    bodys, counts, det_d, root_d, cams = S.lift_case(H, W, seed=11)
    wt, bs, Wn, Bn = refine_weights
    tb, tc = dev(bodys), dev(counts)
    for gt in (False, True):
        p2, p3, rz = dapalib.lift_batch(tb, tc, dev(det_d), dev(root_d), cams, gt_mode=gt)
        ref = dapalib.refine_batch(p2, p3, tc, wt, bs)
        assert p2.dtype == (torch.float64 if gt else torch.float32)
        p2, p3, rz, ref = p2.cpu().numpy(), p3.cpu().numpy(), rz.cpu().numpy(), ref.cpu().numpy()
        for b, P in enumerate(counts):
            o2, o3, orz = (O.lift_gt if gt else O.lift)(bodys[b, :P], det_d[b], root_d[b], cams[b])
            assert np.array_equal(p2[b, :P], o2) and np.array_equal(p3[b, :P], o3) and np.array_equal(rz[b, :P], orz), (gt, b)
            assert not p2[b, P:].any() and not p3[b, P:].any() and not rz[b, P:].any() and not ref[b, P:].any(), (gt, b)
            want = (O.refine_gt if gt else O.refine)(p2[b, :P], p3[b, :P], Wn, Bn)
            assert np.array_equal(ref[b, :P], want), (gt, b, np.abs(ref[b, :P] - want).max())
        assert np.isfinite(p3).all() and np.abs(p3[4, :, :, 2]).max() > 0


def test_refine_mlp_zero_and_one_row(refine_weights):
    """dapalib.refine_mlp: N = 0 gives a [0, 45] tensor without a launch; row 0 of an N = 1 call equals row 0 of a [127, 75] call."""
    import dapalib
    wt, bs, _, _ = refine_weights
    x = torch.randn(127, 75, generator=torch.Generator().manual_seed(2)).to(DEV)
    y0 = dapalib.refine_mlp(x[:0], wt, bs)
    assert tuple(y0.shape) == (0, 45) and y0.dtype == torch.float32 and y0.is_cuda
    y = dapalib.refine_mlp(x, wt, bs)
    y1 = dapalib.refine_mlp(x[:1], wt, bs)
    assert tuple(y1.shape) == (1, 45) and torch.equal(y1[0], y[0]) and y.abs().max() > 0
