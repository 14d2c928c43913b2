"""Constructed edge inputs for the association / lifting kernels (tests/test_assoc_edges_cpu.py checks their preconditions on the
oracle, tests/test_assoc_edges_gpu.py runs them through the HIP kernels).  A plain module: builders only, no fixtures.

  grid_scene / depth_vectors   isolated pelvis peaks whose root depths are a chosen vector, with fewer reachable necks than persons
  introsort / classify         libstdc++'s introsort restated in Python, used ONLY to say which branches a depth vector reaches
  antiquicksort                McIlroy's adversary run against that partition scheme
  tie_scene                    mirrored destination candidates with bitwise-equal PAF scores, two persons per tie
  known_answer_scenes          NMS / PAF scenes whose answers follow from the reference's kernel semantics
  lift_case                    person arrays on exact halves, degenerate limbs, tied percentile samples
"""
import math

import numpy as np

H0, W0 = 128, 208
LATTICE = [(y, x) for y in range(4, 124, 8) for x in range(4, 204, 8)]       # test_nms_raster_order_and_cap's lattice, raster order
NECK_SITES = [p for p in LATTICE if p[0] >= 108]                              # the two bottom lattice rows: 50 sites
MAX_DEPTH = 1.0 / 32                                                          # see grid_scene: keeps the distance penalty at zero
DEFAULT_SCORE = np.float32(np.float32(0.1) + 1e-6)                            # bodyPartConnectorBase.cu:56-59


# ------------------------------------------------------------------ the sort, restated to classify inputs
def kv_lt(a, b):
    """KeyValueCompAsc on (value, index) pairs: NaN last, the index never compared."""
    return (not math.isnan(a[0]) and math.isnan(b[0])) or a[0] < b[0]


def _adjust_heap(a, base, hole, length, val, lt):
    top = child = hole
    while child < (length - 1) // 2:
        child = 2 * (child + 1)
        if lt(a[base + child], a[base + child - 1]):
            child -= 1
        a[base + hole] = a[base + child]
        hole = child
    if (length & 1) == 0 and child == (length - 2) // 2:
        child = 2 * (child + 1)
        a[base + hole] = a[base + child - 1]
        hole = child - 1
    while hole > top and lt(a[base + (hole - 1) // 2], val):
        a[base + hole] = a[base + (hole - 1) // 2]
        hole = (hole - 1) // 2
    a[base + hole] = val


def _heap_sort(a, base, length, lt):
    if length >= 2:
        for parent in range((length - 2) // 2, -1, -1):
            _adjust_heap(a, base, parent, length, a[base + parent], lt)
    while length > 1:
        length -= 1
        val = a[base + length]
        a[base + length] = a[base]
        _adjust_heap(a, base, 0, length, val, lt)


def _unguarded_linear_insert(a, last, lt):
    val = a[last]
    nxt = last - 1
    while lt(val, a[nxt]):
        assert nxt >= 0, "unguarded insertion ran off the array"
        a[last] = a[nxt]
        last = nxt
        nxt -= 1
    a[last] = val


def _insertion_sort(a, first, last, lt):
    for i in range(first + 1, last):
        if lt(a[i], a[first]):
            val = a[i]
            a[first + 1:i + 1] = a[first:i]
            a[first] = val
        else:
            _unguarded_linear_insert(a, i, lt)


def introsort(a, lt, threshold=16, depth_mult=2):
    """std::sort of libstdc++ (bits/stl_algo.h) on the list a, in place: median of three to first, unguarded partition, heap sort once
    the depth budget depth_mult * floor(log2 n) is spent, final insertion sort.  Returns {"heap": the fallback ran, "partitions": count}."""
    stats = {"heap": False, "partitions": 0}
    n = len(a)
    if n == 0:
        return stats

    def loop(first, last, depth):
        while last - first > threshold:
            if depth == 0:
                stats["heap"] = True
                _heap_sort(a, first, last - first, lt)
                return
            depth -= 1
            stats["partitions"] += 1
            pa, pb, pc = first + 1, first + (last - first) // 2, last - 1

            def swap(i, j):
                a[i], a[j] = a[j], a[i]
            if lt(a[pa], a[pb]):
                if lt(a[pb], a[pc]):
                    swap(first, pb)
                elif lt(a[pa], a[pc]):
                    swap(first, pc)
                else:
                    swap(first, pa)
            elif lt(a[pa], a[pc]):
                swap(first, pa)
            elif lt(a[pb], a[pc]):
                swap(first, pc)
            else:
                swap(first, pb)
            lo, hi = first + 1, last
            while True:
                while lt(a[lo], a[first]):
                    lo += 1
                hi -= 1
                while lt(a[first], a[hi]):
                    hi -= 1
                if not lo < hi:
                    break
                swap(lo, hi)
                lo += 1
            loop(lo, last, depth)
            last = lo

    loop(0, n, depth_mult * (n.bit_length() - 1))
    if n > threshold:
        _insertion_sort(a, 0, threshold, lt)
        for i in range(threshold, n):
            _unguarded_linear_insert(a, i, lt)
    else:
        _insertion_sort(a, 0, n, lt)
    return stats


def classify(d, threshold=16, depth_mult=2):
    """Which parts of the sort a depth vector reaches: {"order": person order, "heap": heap-sort fallback, "ties": equal depths among
    more than 16 persons (where the partition order shows), "nan": a NaN depth (sorted last)}."""
    d = np.asarray(d, np.float32)
    a = [(float(v), i) for i, v in enumerate(d)]
    stats = introsort(a, kv_lt, threshold, depth_mult)
    finite = d[~np.isnan(d)]
    return {"order": [i for _, i in a], "heap": stats["heap"], "partitions": stats["partitions"],
            "ties": len(d) > 16 and len(np.unique(finite)) < len(finite), "nan": bool(np.isnan(d).any())}


def antiquicksort(n):
    """M. D. McIlroy, "A killer adversary for quicksort" (1999), run against introsort above: every item starts as `gas`, a
    comparison of two gas items freezes one of them to the next solid value, so every pivot ends up among the smallest items of its
    range.  Returns the n values (integers < n) that drive this partition scheme through its worst case."""
    gas = n - 1
    val = [gas] * n
    state = {"solid": 0, "cand": 0}

    def freeze(x):
        val[x] = state["solid"]
        state["solid"] += 1

    def lt(x, y):
        if val[x] == gas and val[y] == gas:
            freeze(x if x == state["cand"] else y)
        if val[x] == gas:
            state["cand"] = x
        elif val[y] == gas:
            state["cand"] = y
        return val[x] < val[y]

    introsort(list(range(n)), lt)
    return np.asarray(val, np.float32)


def depth_vectors():
    """[(name, fp32 vector)]: the root depths of the grid scenes.  Integer-valued vectors are scaled by 2^-12 and the uniform ones drawn
    below MAX_DEPTH (order and ties are unchanged; grid_scene says why the depths are small)."""
    rng = np.random.default_rng(1234)
    s = np.float32(2.0 ** -12)
    out = [("n2-descending", np.array([2, 1], np.float32) * s),
           ("n16-3-values", rng.integers(1, 4, 16).astype(np.float32) * s)]
    for n in (17, 33, 64, 100, 127):
        out.append((f"n{n}-equal", np.full(n, 5, np.float32) * s))
        for k in (2, 3, 7):
            out.append((f"n{n}-{k}-values", rng.integers(1, k + 1, n).astype(np.float32) * s))
        out.append((f"n{n}-ascending", np.arange(n, dtype=np.float32) * s))
        out.append((f"n{n}-descending", np.arange(n, dtype=np.float32)[::-1] * s))
        out.append((f"n{n}-organ-pipe", np.concatenate([np.arange(n // 2), np.arange(n - n // 2)[::-1]]).astype(np.float32) * s))
        u = rng.uniform(0, MAX_DEPTH, n).astype(np.float32)
        u[rng.integers(0, n, n // 4)] = u[rng.integers(0, n, n // 4)]          # some repeats
        u[rng.choice(n, 2, replace=False)] = np.nan
        out.append((f"n{n}-uniform-2-nan", u))
    out.append(("n127-antiquicksort", antiquicksort(127) * s))
    return out


# ------------------------------------------------------------------ grid scenes
def n_necks_for(n):
    return max(1, min(n // 3, len(NECK_SITES)))


def grid_scene(depths, n_necks=None):
    """hms [43,128,208], rdepth [128,208]: len(depths) <= 127 single-pixel pelvis peaks (channel 2, value 1) on the first lattice sites
    in raster order -- the 7x7 centroid windows are disjoint, so peak r is exactly (x + 0.5, y + 0.5) -- with rdepth[y, x] = depths[r]:
    the group kernel sorts exactly `depths`.  n_necks < n neck peaks (channel 0) sit on the two bottom lattice rows and limb 1's PAF is
    (0, -1) everywhere: every neck -> pelvis direction points up (dy <= -64), so every (neck, pelvis) pair scores |uy| > 0.27 and only
    the first n_necks persons of the depth order get a neck -- the person order decides who.  Finite depths must lie in [0, 1/32]:
    then 1.2 * bone / depth / limb / 4 >= 1 for every limb on the map (limb < 227 px) and the distance penalty min(., 0) stays 0."""
    d = np.asarray(depths, np.float32)
    n = len(d)
    assert 1 <= n <= 127
    fin = d[~np.isnan(d)]
    assert (fin >= 0).all() and (fin <= MAX_DEPTH).all()
    m = n_necks_for(n) if n_necks is None else n_necks
    hms = np.zeros((43, H0, W0), np.float32)
    rdepth = np.full((H0, W0), 0.5, np.float32)
    for r in range(n):
        y, x = LATTICE[r]
        assert y < 100
        hms[2, y, x] = 1.0
        rdepth[y, x] = d[r]
    for y, x in NECK_SITES[:m]:
        hms[0, y, x] = 1.0
    hms[15 + 2 * 1 + 1] = -1.0
    return hms, rdepth


# ------------------------------------------------------------------ score ties
TIE_STRUCTS = {2: (2, 12, 8), 0: (0, 1, 0)}      # rootIdx -> (source channel, destination channel, limb): a limb that starts at the root
# a group: two sources on row sy (near = the smaller root depth), two candidates mirrored about that row at (cx, sy -+ e), inside a
# box where PAF = (sign, 0): dx, |dy|, n, ux and every sample ux * sign + uy * 0 are identical for both candidates of a source
_TIE_GROUPS = [dict(name="two-lanes-c0", sy=24, e=4, near=(10, 24), far=(14, 24), cx=40, box=(8, 46), sign=1.0),
               dict(name="c0-c1-lane-below", sy=60, e=8, near=(14, 60), far=(10, 60), cx=40, box=(8, 46), sign=1.0),
               dict(name="c0-c1-same-lane", sy=60, e=12, near=(74, 60), far=(78, 60), cx=50, box=(48, 80), sign=-1.0),
               dict(name="two-lanes-c1", sy=100, e=4, near=(10, 100), far=(14, 100), cx=40, box=(8, 46), sign=1.0)]
_TIE_FILLERS = ([(4, x) for x in range(84, 104, 4)] + [(56, x) for x in range(84, 208, 4)] + [(64, x) for x in range(84, 204, 4)])
_TIE_COINCIDENT = (110, 100)


def tie_scene():
    """One frame holding the same construction twice, once per root joint (TIE_STRUCTS).  Returns (hms, rdepth, info): info[root] =
    {"src", "dst", "limb", "groups": [{name, near, far, first, second, i, j}], "coincident": (x, y), "n_dst"} with first / second the
    (x + .5, y + .5) of the upper / lower candidate and i < j their raster indices among the destination peaks.  61 unsupported filler
    peaks sit between the upper and the lower candidates of the two row-60 groups: there i < 64 <= j, with j - i = 64 (one lane's c0
    and c1) in one group and j - 64 < i (c1 of a LOWER lane than c0) in the other; the row-24 group ties two lanes' c0, the row-100
    group two lanes' c1.  One destination peak coincides with its source: its PAF score is -1 (norm <= 1e-6), never a candidate."""
    hms = np.zeros((43, H0, W0), np.float32)
    rdepth = np.full((H0, W0), 0.9, np.float32)
    info = {}
    for g, G in enumerate(_TIE_GROUPS):
        rdepth[G["near"][1], G["near"][0]] = 0.40 + 0.04 * g
        rdepth[G["far"][1], G["far"][0]] = 0.42 + 0.04 * g
    rdepth[_TIE_COINCIDENT] = 0.6
    for root, (S, D, limb) in TIE_STRUCTS.items():
        dst = list(_TIE_FILLERS) + [_TIE_COINCIDENT]
        for G in _TIE_GROUPS:
            for xy in (G["near"], G["far"]):
                hms[S, xy[1], xy[0]] = 1.0
            dst += [(G["sy"] - G["e"], G["cx"]), (G["sy"] + G["e"], G["cx"])]
            x0, x1 = G["box"]
            hms[15 + 2 * limb, G["sy"] - G["e"] - 2:G["sy"] + G["e"] + 4, x0:x1 + 1] = G["sign"]
        hms[S, _TIE_COINCIDENT[0], _TIE_COINCIDENT[1]] = 1.0
        dst.sort()
        for y, x in dst:
            hms[D, y, x] = 1.0
        groups = []
        for G in _TIE_GROUPS:
            i, j = dst.index((G["sy"] - G["e"], G["cx"])), dst.index((G["sy"] + G["e"], G["cx"]))
            groups.append(dict(name=G["name"], near=G["near"], far=G["far"], i=i, j=j,
                               first=(G["cx"] + 0.5, G["sy"] - G["e"] + 0.5), second=(G["cx"] + 0.5, G["sy"] + G["e"] + 0.5)))
        info[root] = dict(src=S, dst=D, limb=limb, groups=groups, n_dst=len(dst), coincident=(_TIE_COINCIDENT[1], _TIE_COINCIDENT[0]),
                          coincident_idx=dst.index(_TIE_COINCIDENT))
    return hms, rdepth, info


def person_of(bodys, root, xy):
    """Row of the person whose root joint sits on pixel xy = (x, y)."""
    hit = np.nonzero((bodys[:, root, 0] == xy[0] + 0.5) & (bodys[:, root, 1] == xy[1] + 0.5))[0]
    assert len(hit) == 1, (xy, hit)
    return int(hit[0])


def check_tie_answers(bodys, info_root, root):
    """The known answer of tie_scene for one root joint: the nearer source of every group takes the LOWEST tied index (the upper
    candidate), the farther one the next; the person on the coincident peak gets nothing."""
    D = info_root["dst"]
    for G in info_root["groups"]:
        a, b = person_of(bodys, root, G["near"]), person_of(bodys, root, G["far"])
        assert a < b, G["name"]
        assert tuple(bodys[a, D, :2]) == G["first"] and bodys[a, D, 3] == 1.0, (G["name"], bodys[a, D])
        assert tuple(bodys[b, D, :2]) == G["second"] and bodys[b, D, 3] == 1.0, (G["name"], bodys[b, D])
    c = person_of(bodys, root, info_root["coincident"])
    assert not bodys[c, D].any()


# ------------------------------------------------------------------ NMS / PAF known answers
def _centroid64(ch, x, y):
    H, W = ch.shape
    win = [(yy, xx) for yy in range(max(0, y - 3), min(H, y + 4)) for xx in range(max(0, x - 3), min(W, x + 4)) if ch[yy, xx] > 0]
    s = sum(float(ch[p]) for p in win)
    return sum(p[1] * float(ch[p]) for p in win) / s + 0.5, sum(p[0] * float(ch[p]) for p in win) / s + 0.5


def _plateau_border_threshold(H, W):
    hms = np.zeros((43, H, W), np.float32)
    hms[0, 10, 10] = hms[0, 10, 11] = 0.9          # two equal neighbours: strict > -> no peak
    hms[1, 0, 5] = 0.9                              # border row never registers
    hms[2, 20, 20] = 0.2                            # == threshold: not > 0.2
    hms[4, 20, 20] = np.float32(0.2) + np.float32(1e-6)

    def check(pk, sc):
        assert pk[0, 0, 0] == 0 and pk[1, 0, 0] == 0 and pk[2, 0, 0] == 0 and pk[4, 0, 0] == 1
        assert abs(pk[4, 1, 0] - 20.5) < 1e-5 and abs(pk[4, 1, 1] - 20.5) < 1e-5 and pk[4, 1, 2] == hms[4, 20, 20]
    return hms, check


def _cap_raster(H, W):
    hms = np.zeros((43, H, W), np.float32)
    pts = LATTICE[:300]
    for i, (y, x) in enumerate(pts):
        hms[7, y, x] = 0.3 + 0.001 * (i % 50)

    def check(pk, sc):
        assert pk[7, 0, 0] == 127                   # truncated to maxPeaks (nmsBase.cu:131-133)
        for r in range(127):                        # r-th peak in raster (y-major) order
            y, x = pts[r]
            assert pk[7, r + 1, 2] == hms[7, y, x]
            assert abs(pk[7, r + 1, 0] - (x + 0.5)) < 1e-5 and abs(pk[7, r + 1, 1] - (y + 0.5)) < 1e-5
    return hms, check


def _straight_limb(H, W):
    hms = np.zeros((43, H, W), np.float32)
    hms[0, 30, 40] = 1.0      # neck
    hms[1, 30, 80] = 1.0      # head, 40 px to the right
    hms[15, 28:33, 38:84] = 1.0      # limb 0 PAF-x ribbon, unit vector (1,0)
    hms[2, 60, 100] = 1.0     # pelvis far away, no PAF evidence on limb 1

    def check(pk, sc):
        assert abs(sc[0, 0, 0] - 1.0) <= 1e-6                     # every sample agrees with the limb
        assert sc[0, 0, 1] == -1 and sc[0, 1, 0] == -1            # no such peak pair
        assert sc[1, 0, 0] == -1                                  # limb 1: no PAF evidence and far apart
    return hms, check


def _close_points(H, W):
    hms = np.zeros((43, H, W), np.float32)
    hms[0, 30, 40] = 1.0
    hms[0, 30, 41] = 0.5      # makes the neck centroid sub-pixel, still one peak
    hms[1, 31, 40] = 1.0      # head 1 px away, PAF empty -> distance fallback

    def check(pk, sc):
        assert sc[0, 0, 0] == DEFAULT_SCORE
    return hms, check


def _clipped_windows(H, W):
    """Peaks one pixel off every border: the 7x7 window is clipped to the map (it reaches the border row / column, whose corner pixel
    carries weight here) and everything else in it is negative, hence skipped."""
    hms = np.zeros((43, H, W), np.float32)
    hms[3] = -0.25
    corners = sorted({(1, 1), (1, W - 2), (H - 2, 1), (H - 2, W - 2)})
    for y, x in corners:
        hms[3, y, x] = 1.0
    hms[3, 0, 0] = 0.5

    def check(pk, sc):
        assert pk[3, 0, 0] == len(corners)
        for r, (y, x) in enumerate(corners):
            cx, cy = _centroid64(hms[3], x, y)
            assert abs(pk[3, r + 1, 0] - cx) < 1e-5 and abs(pk[3, r + 1, 1] - cy) < 1e-5 and pk[3, r + 1, 2] == 1.0
        if H > 8 and W > 8:                                         # windows of the four peaks disjoint: (1 * 1 + 0 * 0.5) / 1.5 + 0.5
            assert abs(pk[3, 1, 0] - (1 / 1.5 + 0.5)) < 1e-5 and abs(pk[3, 1, 1] - (1 / 1.5 + 0.5)) < 1e-5
            assert all(tuple(pk[3, r + 1, :2]) == (x + 0.5, y + 0.5) for r, (y, x) in enumerate(corners) if r)
    return hms, check


def _coincident_ends(H, W):
    """The same isolated pixel in both end channels of limb 3 (9 -> 10), PAF evidence present: norm <= 1e-6 gives -1."""
    hms = np.zeros((43, H, W), np.float32)
    y, x = H // 2, W // 2
    hms[9, y, x] = hms[10, y, x] = 1.0
    hms[15 + 2 * 3] = 1.0

    def check(pk, sc):
        assert pk[9, 0, 0] == 1 and pk[10, 0, 0] == 1 and tuple(pk[9, 1]) == tuple(pk[10, 1]) == (x + 0.5, y + 0.5, 1.0)
        assert sc[3, 0, 0] == -1
    return hms, check


def _short_limb(H, W):
    """Two neck / head pairs without PAF evidence, 1/17 px and 1/5 px apart: a pair gets the default score iff its length is below
    sqrt(W * H) / 150 -- 0.110 at 13x21, 0.119 at 5x64 (the first pair only), 1.09 at 128x208 (both)."""
    hms = np.zeros((43, H, W), np.float32)
    sites = [(H // 3, W // 4), (2 * H // 3, 3 * W // 4)]
    for (y, x), v in zip(sites, (0.0625, 0.25)):
        hms[0, y, x] = 1.0
        hms[0, y, x + 1] = v                                        # neck centroid v / (1 + v) px to the right
        hms[1, y, x] = 1.0
    th = math.sqrt(W * H) / 150

    def check(pk, sc):
        assert pk[0, 0, 0] == 2 and pk[1, 0, 0] == 2
        assert abs(pk[0, 1, 0] - (sites[0][1] + 0.5 + 1 / 17)) < 1e-5 and abs(pk[0, 2, 0] - (sites[1][1] + 0.5 + 0.2)) < 1e-5
        assert sc[0, 0, 0] == DEFAULT_SCORE
        assert sc[0, 1, 1] == (DEFAULT_SCORE if 0.2 < th else -1)
        assert sc[0, 0, 1] == -1 and sc[0, 1, 0] == -1
    return hms, check


KNOWN_ANSWER_SIZES = ((3, 3), (5, 64), (13, 21), (H0, W0))


def known_answer_scenes(H, W):
    """[(name, hms [43,H,W], check(peaks, scores))] for one map size; check asserts the known answers on a peak table / score table."""
    if (H, W) == (3, 3):
        mk = [_clipped_windows, _coincident_ends]
    elif (H, W) == (H0, W0):
        mk = [_plateau_border_threshold, _cap_raster, _straight_limb, _close_points, _clipped_windows, _coincident_ends, _short_limb]
    else:
        mk = [_clipped_windows, _coincident_ends, _short_limb]
    return [(f.__name__.strip("_"),) + f(H, W) for f in mk]


# ------------------------------------------------------------------ lifting
LIFT_COUNTS = (0, 1, 2, 17, 127, 5)
ODD_CAM = (0.37, 1333.0, 777.0, 832.0, 512.0, 1111.0, 1234.5, 660.25, 390.75)
_PAIRS = [(0, 1), (0, 2), (0, 9), (9, 10), (10, 11), (0, 3), (3, 4), (4, 5), (2, 12), (12, 13), (13, 14), (2, 6), (6, 7), (7, 8)]


def lift_case(H, W, seed):
    """(bodys [6,127,15,4] fp32, counts, det_d [6,14,H,W], root_d [6,H,W], cams [6,9]) for the lifting kernels: coordinates on
    multiples of 1/8 in [0.5, W - 0.5) x [0.5, H - 0.5) (4 * coord and the ten sample positions of a limb hit exact halves); per
    person about a quarter of the limbs each exactly vertical (stepx == 0), exactly horizontal (stepy == 0) and of length zero; 20 % of
    the joints and one root per frame with score 0; depth maps on 5 levels (ties at the percentile clamps) except the continuous
    frame 3; every other camera with an odd scale."""
    from benchkit.workload import PEOPLE_CAM
    rng = np.random.default_rng(seed)
    B = len(LIFT_COUNTS)
    bodys = np.zeros((B, 127, 15, 4), np.float32)
    for b, P in enumerate(LIFT_COUNTS):
        for p in range(P):
            xy = np.stack([rng.integers(4, 8 * W - 4, 15), rng.integers(4, 8 * H - 4, 15)], 1).astype(np.float32) / 8
            for (s, d), mode in zip(_PAIRS, rng.integers(0, 4, 14)):            # a limb's source is final before the limb is visited
                if mode == 1:
                    xy[d, 0] = xy[s, 0]
                elif mode == 2:
                    xy[d, 1] = xy[s, 1]
                elif mode == 3:
                    xy[d] = xy[s]
            bodys[b, p, :, :2] = xy
            bodys[b, p, :, 3] = np.where(rng.random(15) < 0.2, 0.0, rng.uniform(0.2, 1, 15))
            bodys[b, p, 2, 3] = rng.uniform(0.2, 1)
        if P:
            bodys[b, rng.integers(0, P), 2, 3] = 0.0
    det_d = (rng.integers(0, 5, (B, 14, H, W)) * 0.25 - 0.5).astype(np.float32)
    det_d[3] = rng.uniform(-0.5, 0.5, (14, H, W)).astype(np.float32)
    root_d = rng.uniform(0.2, 1.0, (B, H, W)).astype(np.float32)
    cams = np.stack([np.asarray(PEOPLE_CAM if b % 2 == 0 else ODD_CAM, np.float64) for b in range(B)])
    return bodys, np.asarray(LIFT_COUNTS, np.int32), det_d, root_d, cams
