"""What csrc/plan_check.cpp accepts of STEM, STEMPOOL, MAXPOOL, UPADD and HEADSUM, the kernels of csrc/plan.hip can compute: one valid
hand-made op per kind (tests/plan_ops.py, the builders test_plan_ops_gpu.py runs), one field changed at a time, through smap_plan_create
(no GPU involved) -- and the float32 index rule the GPU references restate, anchored to torch."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plan_ops as P


def _rc(o, alter=None):
    """smap_plan_create on a copy of `o` alone, after alter(copy)."""
    from smap_amd import lib as L
    one = (L.SmapOp * 1)(o)
    if alter:
        alter(one[0])
    h = C.c_void_p()
    rc = L.load().smap_plan_create(one, 1, C.byref(h))
    if rc == 0:
        L.load().smap_plan_destroy(h)
    return rc


def _set(field, val, idx=None):
    def alter(o):
        if idx is None:
            setattr(o, field, val)
        else:
            getattr(o, field)[idx] = val
    return alter


def _both(*alters):
    def alter(o):
        for a in alters:
            a(o)
    return alter


HB = 2                          # output frames of the HEADSUM base op
BASE = {                        # kind -> a valid op
    "STEM": lambda: P.laid_out_stem(2, 37, 61, False, flip_from=1),
    "STEMPOOL": lambda: P.laid_out_stem(2, 37, 61, True, flip_from=1, pool=True),
    "MAXPOOL": lambda: P.laid_out_maxpool(2, 19, 31, 64, True),
    "UPADD": lambda: P.laid_out_upadd(2, 13, 21, 64, 7, 11),
    "HEADSUM": lambda: P.laid_out_headsum(HB, 16, 24, 43, 48, [(16, 24), (8, 12), (4, 6)], flip=True, n_kpt=15, scale=True),
    "HEADSUM2": lambda: P.laid_out_headsum(1, 16, 40, 43, 48, [(16, 40), (8, 20)]),               # n_aux = 2
}
TABLE = [       # base, what changes, the change, accepted
    # float4 loads of the sources: channels Cin & ~3 .. Cout - 1 would never reach the LDS tile and be stored from it all the same
    ("HEADSUM", "Cin = 43", _set("Cin", 43), False),
    ("HEADSUM", "Cin = 46", _set("Cin", 46), False),
    ("HEADSUM", "Cin = 44", _set("Cin", 44), True),
    ("HEADSUM", "Cin = 42 < Cout", _set("Cin", 42), False),
    # the kernel reads frame b + flip_from of sources that the range walk sizes as 2 B frames
    ("HEADSUM", "flip_from = B - 1", _set("flip_from", HB - 1), False),
    ("HEADSUM", "flip_from = B + 1", _set("flip_from", HB + 1), False),
    ("HEADSUM", "flip_from = 2 B", _set("flip_from", 2 * HB), False),
    ("HEADSUM", "flip_from = B", _set("flip_from", HB), True),
    ("HEADSUM", "flip_from = -1", _set("flip_from", -1), False),
    ("HEADSUM", "flip_from = 0", _set("flip_from", 0), True),
    ("HEADSUM2", "aux_h[1] = 0", _set("aux_h", 0, 1), False),
    ("HEADSUM2", "aux_w[1] = 0", _set("aux_w", 0, 1), False),
    ("HEADSUM2", "aux_h[0] = -1", _set("aux_h", -1, 0), False),
    ("HEADSUM2", "aux_h[2] = 0 (beyond n_aux)", _set("aux_h", 0, 2), True),
    ("HEADSUM", "n_aux = 0", _set("n_aux", 0), False),
    ("HEADSUM", "n_aux = 4", _set("n_aux", 4), False),
    ("HEADSUM", "Cout = 49 (LDS tile of 48 rows)", _both(_set("Cout", 49), _set("Cin", 52)), False),
    ("HEADSUM", "n_kpt > Cout", _set("in_c_off", 44), False),
    ("HEADSUM", "scale_hms = 2", _set("scale_hms", 2), False),
    ("HEADSUM", "status_off = 6", _set("status_off", 6), False),
    ("HEADSUM", "aux_off[2] absent", _set("aux_off", -1, 2), False),
    ("UPADD", "Cout = 12", _set("Cout", 12), False),
    ("UPADD", "aux_h[0] = 0", _set("aux_h", 0, 0), False),
    ("UPADD", "aux_w[0] = -3", _set("aux_w", -3, 0), False),
    ("UPADD", "precision = 1", _set("precision", 1), False),
    ("UPADD", "Wo = 0", _set("Wo", 0), False),
    ("MAXPOOL", "Cin = 12", _both(_set("Cin", 12), _set("Cout", 12)), False),
    ("MAXPOOL", "Cin != Cout", _set("Cout", 72), False),
    ("MAXPOOL", "Ho one too many", _set("Ho", 11), False),
    ("MAXPOOL", "Wo one too few", _set("Wo", 15), False),
    ("STEM", "B = 3 != 2 flip_from", _set("B", 3), False),
    ("STEM", "flip_from = 2, B = 2", _set("flip_from", 2), False),
    ("STEM", "flip_from = -1", _set("flip_from", -1), False),
    ("STEM", "flip_from = 0", _set("flip_from", 0), True),
    ("STEM", "Cin = 4", _set("Cin", 4), False),
    ("STEM", "Cout = 32", _set("Cout", 32), False),
    ("STEM", "Ho one too many", _set("Ho", 20), False),
    ("STEM", "precision = 2", _set("precision", 2), False),
    ("STEMPOOL", "B = 3 != 2 flip_from", _set("B", 3), False),
    ("STEMPOOL", "Ho, Wo of the conv", _both(_set("Ho", 19), _set("Wo", 31)), False),
    ("STEMPOOL", "out_off absent", _set("out_off", -1), False),
]


@pytest.mark.parametrize("row", TABLE, ids=["%s: %s" % r[:2] for r in TABLE])
def test_checker_accepts_what_the_kernel_computes_and_nothing_else(row):
    base, what, alter, accepted = row
    assert _rc(BASE[base]()) == 0, base
    assert (_rc(BASE[base](), alter) == 0) == accepted, (base, what)


def test_checker_accepts_every_shape_the_gpu_tests_run():
    """Every op test_plan_ops_gpu.py hands to the GPU, built by the same functions from the same shape lists."""
    ops = []
    for x3 in (False, True):
        for pool in (False, True):
            ops += [P.laid_out_stem(*s, x3, pool=pool) for s in P.STEM_SHAPES]
            ops.append(P.laid_out_stem(*P.STEM_FLIP[:3], x3, flip_from=P.STEM_FLIP[3], pool=pool))
        ops += [P.laid_out_maxpool(*s, x3) for s in P.POOL_SHAPES]
    ops.append(P.laid_out_maxpool(*P.POOL_OVER_THE_CAP, False))
    ops += [P.laid_out_upadd(*s, relu) for s in P.UPADD_SHAPES + [P.UPADD_OVER_THE_CAP] for relu in (0, 1)]
    for i, (B, Ho, Wo, Cout, Cin, srcs) in enumerate(P.HEAD_CASES):
        for scale in (False, True):
            ops.append(P.laid_out_headsum(B, Ho, Wo, Cout, Cin, srcs, n_kpt=min(15, Cout), scale=scale))
            if i < 2:
                ops += [P.laid_out_headsum(B, Ho, Wo, Cout, Cin, srcs, flip=True, n_kpt=n_kpt, scale=scale) for n_kpt in (15, 0)]
    assert len(ops) == 2 * (2 * 6 + 4) + 1 + 14 + 6 * 2 + 2 * 2 * 2
    for o in ops:
        assert _rc(o) == 0, (o.kind, o.B, o.H, o.W, o.Cin, o.Ho, o.Wo, o.Cout, o.precision, o.flip_from)


def test_the_cap_cases_take_a_second_trip_of_the_grid_stride_loop():
    B, H, W, Cc = P.POOL_OVER_THE_CAP
    assert B * P.conv_out(H) * P.conv_out(W) * (Cc // 8) > P.GRID_CAP_ITEMS
    B, Ho, Wo, Cc, _, _ = P.UPADD_OVER_THE_CAP
    assert B * Ho * Wo * (Cc // 8) > P.GRID_CAP_ITEMS


LERP_SIZES = sorted({(i, o) for _, Ho, Wo, _, h, w in P.UPADD_SHAPES + [P.UPADD_OVER_THE_CAP] for i, o in ((h, Ho), (w, Wo))} |
                    {(i, o) for _, Ho, Wo, _, _, srcs in P.HEAD_CASES for h, w in srcs for i, o in ((h, Ho), (w, Wo))} | {(208, 416), (5, 832)})


def test_float32_index_rule_stays_in_range_and_matches_torch():
    """The restated lerp_index (plan_ops.lerp_taps) for every (in, out) extent the GPU tests use: both taps inside the source, the
    weights in [0, 1] summing to 1 within one float32 rounding, and the interpolated map within in_size * 2^-22 * max|v| of F.interpolate(bilinear,
    align_corners=True) in float64 -- the fp32 error of src, at most in_size * 2^-24 * 2, times a slope of at most 2 max|v| per unit of src."""
    g = torch.Generator().manual_seed(3)
    for n_in, n_out in LERP_SIZES:
        i0, i1, l0, l1 = P.lerp_taps(n_in, n_out)
        assert l0.dtype == l1.dtype == np.float32
        assert (0 <= i0).all() and (i0 <= i1).all() and (i1 <= n_in - 1).all() and (i1 - i0 <= 1).all(), (n_in, n_out)
        assert (l1 >= 0).all() and (l1 <= 1).all() and (np.abs(l0.astype(np.float64) + l1 - 1) <= 2.0 ** -24).all(), (n_in, n_out)
        for v in (torch.randn(2, n_in, 3, 5, generator=g, dtype=torch.float64), torch.randn(2, 3, n_in, 5, generator=g, dtype=torch.float64)):
            size = (n_out, 3) if v.shape[1] == n_in else (3, n_out)
            want = F.interpolate(v.permute(0, 3, 1, 2), size=size, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
            err = float((P.bilinear(v, *size) - want).abs().max())
            assert err <= n_in * 2.0 ** -22 * float(v.abs().max()), (n_in, n_out, err)


def test_references_on_known_values():
    """The float64 references against values worked out by hand: a 2 -> 3 bilinear map, a max-pool whose border windows are all negative, a
    head sum merge with the mirrored frame."""
    v = torch.tensor([0.0, 2.0], dtype=torch.float64).view(1, 1, 2, 1)
    assert torch.equal(P.bilinear(v, 1, 3).flatten(), torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64))
    m = P.maxpool_reference(torch.full((1, 3, 3, 1), -2.0, dtype=torch.float64))
    assert m.shape == (1, 2, 2, 1) and torch.equal(m, torch.full_like(m, -2.0))          # padding never wins
    s = torch.zeros(2, 1, 3, 4)                     # frames 0 (plain) and 1 (mirrored), one row of three pixels, channels 0..2 (+ 1 unused)
    s[0, 0, :, 0], s[0, 0, :, 1], s[0, 0, :, 2] = torch.tensor([1.0, 2.0, 3.0]), 10.0, 100.0
    s[1, 0, :, 0], s[1, 0, :, 1], s[1, 0, :, 2] = torch.tensor([4.0, 5.0, 6.0]), torch.tensor([7.0, 8.0, 9.0]), 1000.0
    val, mag, slack = P.headsum_reference([s], 1, 3, 3, 1, flip=True, pair=[1, 2, 0], n_kpt=1, scale=False)
    assert val[0, 0, 0].tolist() == [1 + 9, 2 + 8, 3 + 7]                  # key point 0: + channel pair[0] = 1 of the mirrored frame, reversed
    assert val[0, 1, 0].tolist() == [(10 - 1000) / 2] * 3                  # PAF x (c - n_kpt even): minus, halved
    assert val[0, 2, 0].tolist() == [(100 + 6) / 2, (100 + 5) / 2, (100 + 4) / 2]
    assert mag[0, 1, 0].tolist() == [(10 + 1000) / 2] * 3 and not slack.any()         # (equal sizes: the weights are constants)
