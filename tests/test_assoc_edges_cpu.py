"""CPU suite: the preconditions of tests/test_assoc_edges_gpu.py, checked on the oracle, so that the GPU tests cannot pass vacuously --
the constructed scenes (tests/assoc_scenes.py) really contain what they claim: the depth vector, contested necks, bitwise-equal scores at
the intended candidate indices, the sort branches the classifier names, in-range lifting samples."""
import numpy as np
import pytest
import torch

import assoc_scenes as S
from oracle import oracle_lib as O


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vectors():
    return S.depth_vectors()


def torch_order(d):
    return torch.from_numpy(np.array(d, np.float32)).sort(0, False)[1].numpy()


def test_depth_vectors_cover_the_issue_list(vectors):
    names = [n for n, _ in vectors]
    assert len(set(names)) == len(names) == 2 + 5 * 8 + 1
    for n in (17, 33, 64, 100, 127):
        for kind in ("equal", "2-values", "3-values", "7-values", "ascending", "descending", "organ-pipe", "uniform-2-nan"):
            d = dict(vectors)[f"n{n}-{kind}"]
            assert d.dtype == np.float32 and len(d) == n
            if kind == "uniform-2-nan":
                assert np.isnan(d).sum() == 2 and len(np.unique(d[~np.isnan(d)])) < n - 2
            elif kind.endswith("values"):
                assert len(np.unique(d)) == int(kind[0])
        assert np.array_equal(dict(vectors)[f"n{n}-organ-pipe"] * 4096, np.concatenate([np.arange(n // 2), np.arange(n - n // 2)[::-1]]))
    assert len(dict(vectors)["n2-descending"]) == 2 and len(dict(vectors)["n16-3-values"]) == 16
    assert len(dict(vectors)["n127-antiquicksort"]) == 127


def test_grid_scenes_hold_their_depth_vector_and_the_oracle_sorts_like_torch(vectors):
    """Every grid scene: O.nms finds exactly n pelvis peaks on the intended lattice sites, the depths read back at them are the vector
    bit for bit, and O.connect's person order is torch's sort(0, False) of it; fewer necks than persons, all of them handed out."""
    for name, d in vectors:
        hms, rd = S.grid_scene(d)
        n = len(d)
        pk = O.nms(hms)
        assert pk[2, 0, 0] == n, name
        want = np.array([(x + 0.5, y + 0.5, 1.0) for y, x in S.LATTICE[:n]], np.float32)
        assert np.array_equal(pk[2, 1:1 + n], want), name
        back = np.array([rd[int(pk[2, r + 1, 1]), int(pk[2, r + 1, 0])] for r in range(n)], np.float32)
        assert np.array_equal(bits(back), bits(d)), name
        bodys, _, sc = O.connect(hms, rd)
        idx = torch_order(d)
        assert bodys.shape[0] == n and np.array_equal(bodys[:, 2, :2], pk[2, 1 + idx, :2]), name
        m = S.n_necks_for(n)
        assert pk[0, 0, 0] == m < n and (sc[1, :m, :n] > 0.27).all(), name
        got = bodys[:, 0, 3] > 0
        assert got[:m].all() and not got[m:].any(), name             # the first m persons of the depth order, nobody else


def test_classifier_matches_torch_sort_and_names_the_branches(vectors):
    """The Python restatement of the sort is pinned to torch.sort on every vector, and says that the set reaches the heap-sort fallback
    (organ-pipe and the antiquicksort adversary at n = 127; not ascending / descending / all-equal), ties beyond 16 persons, and NaN."""
    cls = {}
    for name, d in vectors:
        cls[name] = c = S.classify(d)
        assert np.array_equal(c["order"], torch_order(d)), name
        oi, _ = O.sort_depth(d)
        assert np.array_equal(c["order"], oi), name
    assert cls["n127-organ-pipe"]["heap"] and cls["n127-antiquicksort"]["heap"]
    assert not any(cls[f"n127-{k}"]["heap"] for k in ("ascending", "descending", "equal"))
    assert not any(c["heap"] or c["partitions"] for n, c in cls.items() if n.startswith(("n2-", "n16-")))
    assert sum(c["ties"] for c in cls.values()) >= 20 and sum(c["nan"] for c in cls.values()) == 5
    for n in (17, 33, 64, 100, 127):                                  # NaN last
        d = dict(vectors)[f"n{n}-uniform-2-nan"]
        assert np.isnan(d[cls[f"n{n}-uniform-2-nan"]["order"][-2:]]).all()
    print("heap-sort fallback reached by:", [n for n, c in cls.items() if c["heap"]])


def test_antiquicksort_vector_is_quadratic_for_this_partition_scheme():
    d = S.antiquicksort(127)
    assert S.classify(d)["heap"] and (d >= 0).all() and (d <= 126).all()
    rng = np.random.default_rng(0)
    assert not S.classify(rng.permutation(127).astype(np.float32))["heap"]


def test_depth_vectors_tell_a_mutated_sort_from_the_real_one(vectors):
    """Two mutations that still sort correctly and only move equal depths -- final-insertion threshold 16 -> 8, depth budget
    2 * lg -> lg -- applied to the restatement: each changes the person order of at least one vector (the same vectors catch the same
    mutations applied to the oracle's C sort), so a GPU sort with either slip cannot pass the depth-order test."""
    caught = {m: [n for n, d in vectors if S.classify(d, **kw)["order"] != S.classify(d)["order"]]
              for m, kw in (("threshold-8", dict(threshold=8)), ("depth-lg", dict(depth_mult=1)))}
    assert len(caught["threshold-8"]) >= 20 and "n127-equal" in caught["threshold-8"]
    assert caught["depth-lg"] == ["n100-organ-pipe", "n127-organ-pipe"]


def test_necks_are_contested(vectors):
    """Two permutations of the same tie-heavy depths give different bodys: who gets a neck depends on the person order."""
    d = dict(vectors)["n33-3-values"]
    rng = np.random.default_rng(7)
    b0, _, _ = O.connect(*S.grid_scene(d))
    b1, _, _ = O.connect(*S.grid_scene(d[rng.permutation(len(d))]))
    assert b0.shape == b1.shape and not np.array_equal(b0, b1)
    assert not np.array_equal(b0[:, 0], b1[:, 0])


@pytest.mark.parametrize("root", [2, 0])
def test_tie_scene_has_bitwise_equal_scores_where_intended(root):
    """The oracle's score table holds bitwise-equal positive scores at the intended candidate indices and nowhere else in the source's
    row: one pair (i < 64, j = i + 64), one pair (i < 64 <= j, j - 64 < i), one pair below 64, one pair above; with and without the
    distance penalty the oracle hands the lower index to the nearer person."""
    hms, rd, info = S.tie_scene()
    I = info[root]
    pk = O.nms(hms)
    sc = O.paf_score(hms, pk)
    assert pk[I["dst"], 0, 0] == I["n_dst"] <= 127 and pk[I["src"], 0, 0] == 9
    src = [tuple(p) for p in pk[I["src"], 1:10, :2]]
    dst = [tuple(p) for p in pk[I["dst"], 1:1 + I["n_dst"], :2]]
    spans = set()
    for G in I["groups"]:
        i, j = G["i"], G["j"]
        assert dst[i] == G["first"] and dst[j] == G["second"]
        for who in ("near", "far"):
            row = sc[I["limb"], src.index((G[who][0] + 0.5, G[who][1] + 0.5))]
            assert row[i] > 0 and bits(row[i]) == bits(row[j]), (G["name"], who)
            assert set(np.nonzero(row > 0)[0]) == {i, j}, (G["name"], who)
        spans.add("same-lane" if j == i + 64 else "lane-below" if i < 64 <= j and j - 64 < i else "c0" if j < 64 else "c1" if i >= 64 else "?")
    assert spans == {"same-lane", "lane-below", "c0", "c1"}
    c = src.index((I["coincident"][0] + 0.5, I["coincident"][1] + 0.5))
    assert dst[I["coincident_idx"]] == src[c] and (sc[I["limb"], c] == -1).all()
    for dist in (False, True):
        bodys = O.group(pk, sc, rd, root, dist)
        assert bodys.shape[0] == 9
        S.check_tie_answers(bodys, I, root)
    bone = (12.4644364, 26.42178982)[root == 0]                      # the penalty is live in every distFlag pick: the tied scores are
    for G in I["groups"]:                                              # lowered by the same amount, and stay positive (checked above)
        for who in ("near", "far"):
            limb = np.hypot(G["first"][0] - G[who][0] - 0.5, G["first"][1] - G[who][1] - 0.5)
            assert 1.2 * bone / float(rd[G[who][1], G[who][0]]) / limb / 4 - 1 < -0.1, (G["name"], who)


@pytest.mark.parametrize("size", S.KNOWN_ANSWER_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_known_answer_scenes_hold_on_the_oracle(size):
    seen = set()
    for name, hms, check in S.known_answer_scenes(*size):
        pk = O.nms(hms)
        check(pk, O.paf_score(hms, pk))
        seen.add(name)
    assert {"clipped_windows", "coincident_ends"} <= seen and ("short_limb" in seen or size == (3, 3))


@pytest.mark.parametrize("size", [(16, 24), (128, 208)], ids=["16x24", "128x208"])
def test_lift_inputs_stay_in_range(size):
    """For every joint rint(4 * coord) // 4 lies inside the map (so does every sample between two joints), coordinates sit on 1/8, and
    the cases hold what lift_case promises: vertical, horizontal and zero-length limbs, zero scores, tied depth samples."""
    H, W = size
    bodys, counts, det_d, root_d, cams = S.lift_case(H, W, seed=11)
    assert counts.tolist() == [0, 1, 2, 17, 127, 5] and bodys.shape == (6, 127, 15, 4)
    kinds = np.zeros(3, int)
    for b, P in enumerate(counts):
        xy = bodys[b, :P, :, :2]
        assert not bodys[b, P:].any()
        assert np.array_equal(xy * 8, np.rint(xy * 8))
        ix, iy = np.rint(4.0 * xy[..., 0]).astype(int) // 4, np.rint(4.0 * xy[..., 1]).astype(int) // 4
        assert ix.min(initial=0) >= 0 and iy.min(initial=0) >= 0 and ix.max(initial=0) < W and iy.max(initial=0) < H
        assert (xy[..., 0] >= 0.5).all() and (xy[..., 0] < W - 0.5).all() and (xy[..., 1] >= 0.5).all() and (xy[..., 1] < H - 0.5).all()
        if P:
            assert (bodys[b, :P, 2, 3] == 0).sum() == 1
        for s, d in S._PAIRS:
            same_x, same_y = xy[:, s, 0] == xy[:, d, 0], xy[:, s, 1] == xy[:, d, 1]
            kinds += [(same_x & ~same_y).sum(), (same_y & ~same_x).sum(), (same_x & same_y).sum()]
    assert (kinds > 50).all()
    sc = bodys[4, :, :, 3]
    assert 0.1 < (sc == 0).mean() < 0.3
    assert len(np.unique(det_d[0])) == 5 and len(np.unique(det_d[3])) > 1000
    assert (4 * bodys[..., :2] % 1 == 0.5).any()                       # samples on exact halves
    assert not np.array_equal(cams[0], cams[1]) and cams.shape == (6, 9)
