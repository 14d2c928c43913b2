"""CPU: the host half of the label renderer (smap_amd/labels.py) against tests/golden/labels.npz, which was written by running the
reference's dataset/representation.py (tests/golden/gen_golden_labels.py): the descriptor packer against what the reference's own
np.linalg.norm / round calls saw and returned, generate_rdepth, the channel mask, the blur taps, argument validation and the CLI's
refusal of --maps_from_gt in run_inference."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE = 4


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "labels.npz"))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def spec_for(shape, max_people=20):
    from labels_restate import KERNELS, LIMBS
    from smap_amd.labels import LabelSpec
    return LabelSpec(tuple(KERNELS), tuple(LIMBS), 1, STRIDE, tuple(int(v) for v in shape), 2, max_people)


def test_spec_comes_from_the_configuration():
    from exps.stage3_root2.config import cfg
    from labels_restate import KERNELS, LIMBS
    from smap_amd.labels import label_spec
    s = label_spec(cfg)
    assert s.kernels == tuple(KERNELS) and s.paf_vector == tuple(LIMBS) and s.shape == (128, 208) and s.stride == 4
    assert s.root_idx == 2 and s.max_people == 20 and s.thres == (3, 2, 1, 1, 1) and len(s.kernels) == 5
    assert label_spec(cfg, shape=(17, 23), kernels=[(5, 7)]).kernels == ((5, 7),)


@pytest.mark.parametrize("width", [3, 2, 1])
@pytest.mark.parametrize("mds", [False, True])
def test_descriptor_table_holds_what_the_reference_computed(z, width, mds):
    """Per valid limb in limb-major, person order: the unit vector is the recorded limb_vec / the recorded norm, the box is the recorded
    int(round()) values clipped to the grid, short limbs (recorded norm < 1) are absent -- all bit for bit / exactly."""
    from labels_restate import LIMBS
    from smap_amd.labels import pack_table, table_views
    name = "small_special20"
    H, W = z[name + "_shape"]
    key = "%s_desc_w%d_m%d" % (name, width, int(mds))
    vec, norm, rounded = z[key + "_vec"], z[key + "_norm"], z[key + "_round"]
    buf, ksizes, P = pack_table([z[name + "_bodys"]], [(1, 1)], [width], LIMBS, STRIDE, (H, W), mds)
    v = table_views(buf, 1, 1, P)
    n = v["limb_n"][0, 0]
    long = norm >= 1.0
    assert long.sum() == len(rounded) == n.sum() and (~long).sum() >= 1 and P == 20 and n.max() >= 12
    got_f = np.concatenate([v["limb_f"][0, 0, l, :n[l]] for l in range(14)])
    got_box = np.concatenate([v["limb_box"][0, 0, l, :n[l]] for l in range(14)])
    unit = vec[long] / norm[long][:, None]
    assert np.array_equal(bits(got_f[:, 2:4]), bits(unit))
    assert (got_f[:, 5] == width).all()
    want_box = np.stack([np.maximum(rounded[:, 0], 0), np.minimum(rounded[:, 1], W), np.maximum(rounded[:, 2], 0),
                         np.minimum(rounded[:, 3], H)], 1)
    assert np.array_equal(got_box, want_box)
    # centerA: the truncated joint over the stride; limb_z: the difference of the truncated depths
    bodys = z[name + "_bodys"]
    k = 0
    for l, (a, b) in enumerate(LIMBS):
        need = 2 if (width > 1 and mds) else 1
        for p in range(len(bodys)):
            if bodys[p, a, 3] < need or bodys[p, b, 3] < need:
                continue
            ca, cb = np.trunc(bodys[p, a, :3]), np.trunc(bodys[p, b, :3])
            if np.hypot(*(cb[:2] / STRIDE - ca[:2] / STRIDE)) < 1.0 - 1e-9:
                continue
            assert got_f[k, 0] == ca[0] / STRIDE and got_f[k, 1] == ca[1] / STRIDE and got_f[k, 4] == cb[2] - ca[2]
            k += 1
    assert k == len(got_f)
    if mds and width > 1:                                      # the flag drops limbs with an occluded end
        other = z["%s_desc_w%d_m0_norm" % (name, width)]
        assert len(other) > len(norm)


def test_impulses_are_a_set_and_the_taps_are_the_stated_ones(z):
    from labels_restate import KERNELS, LIMBS, taps
    from smap_amd.labels import gaussian_taps, pack_table, table_views
    name = "small_special20"
    bodys, (H, W) = z[name + "_bodys"], z[name + "_shape"]
    buf, ksizes, P = pack_table([bodys, bodys[:0]], KERNELS, [3, 2, 1, 1, 1], LIMBS, STRIDE, (H, W))
    v = table_views(buf, 2, 5, P)
    assert ksizes.tolist() == [list(k) for k in KERNELS] and not v["imp_n"][1].any() and not v["limb_n"][1].any()
    shared = 0
    for j in range(15):
        cells = {int(b[j, 1] / STRIDE) * W + int(b[j, 0] / STRIDE) for b in bodys if b[j, 3] >= 1}
        visible = sum(1 for b in bodys if b[j, 3] >= 1)
        shared += visible - len(cells)
        got = v["imp"][0, j, :v["imp_n"][0, j]].tolist()
        assert len(got) == len(set(got)) and set(got) == cells
    assert shared >= 15, "the scene has persons whose joints share a cell"
    assert gaussian_taps(5).tolist() == [0.0625, 0.25, 0.375, 0.25, 0.0625]
    assert gaussian_taps(7).tolist() == [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]
    for s, (kx, ky) in enumerate(KERNELS):
        k = gaussian_taps(kx)
        assert k.dtype == np.float32 and np.array_equal(bits(k), bits(taps(kx))) and np.array_equal(k, k[::-1])
        assert abs(float(k.astype(np.float64).sum()) - 1.0) < 8 * 2.0 ** -24
        assert np.array_equal(v["taps"][s, 0, :kx], k) and np.array_equal(v["taps"][s, 1, :ky], gaussian_taps(ky)) and not v["taps"][s, :, kx:].any()


def test_root_depth_labels_are_the_references(z):
    from smap_amd.labels import root_depth_labels
    seen = 0
    for name in z["names"]:
        bodys = z[name + "_bodys"]
        want = z[name + "_rdepth"]
        got = root_depth_labels(bodys, float(z["scale"]), spec_for(z[name + "_shape"]))
        assert got.dtype == np.float32 and got.shape == (20, 3) and np.array_equal(bits(got), bits(want)), name
        seen += int((want[:, 2] != 0).sum())
    assert seen >= 40
    few = root_depth_labels(z["pipe_bodys"], float(z["scale"]), spec_for((128, 208), max_people=2))       # j >= max_people is skipped
    assert few.shape == (2, 3) and (few[:, 2] > 0).all()


def test_valid_vector():
    from smap_amd.labels import valid_vector
    v = valid_vector("MUCO")
    assert v.shape == (57, 1) and v.dtype == np.float64 and (v == 1).all()
    c = valid_vector("coco")
    off = [1, 15, 16] + list(range(15 + 28, 57))                # head top, the two head-top limb channels, every depth channel
    assert c.shape == (57, 1) and sorted(np.flatnonzero(c[:, 0] == 0).tolist()) == off and c.sum() == 57 - len(off)


def test_root_depth_map_paints_far_to_near_and_clips(z):
    from smap_amd.labels import root_depth_map
    spec = spec_for((17, 23))
    a = np.zeros((3, 15, 11))
    a[:, :, 3] = 2
    a[:, :, 7] = 1000.0
    a[0, 2, :3] = (40.0, 30.0, 300.0)                          # cell (7, 10), near
    a[1, 2, :3] = (48.0, 30.0, 600.0)                          # cell (7, 12), far: overlaps the first
    a[2, 2, :3] = (1.0, 1.0, 450.0)                            # the corner: the patch is clipped
    a[2, 2, 3] = 1
    m = root_depth_map([a, a[:0]], [{"scale": 0.5}, 0.5], spec)
    assert m.shape == (2, 1, 17, 23) and m.dtype == np.float32 and not m[1].any()
    near, far, corner = np.float32(300.0 / 1000.0 / 0.5), np.float32(600.0 / 1000.0 / 0.5), np.float32(450.0 / 1000.0 / 0.5)
    want = np.zeros((17, 23), np.float32)
    want[4:11, 9:16] = far
    want[4:11, 7:14] = near
    want[0:4, 0:4] = corner
    assert np.array_equal(m[0, 0], want)
    a[1, 2, 3] = 0                                              # an invisible root is not painted
    assert (root_depth_map([a], [0.5], spec)[0, 0, 4:11, 14:16] == 0).all()


def test_arguments_are_validated(z):
    from labels_restate import KERNELS, LIMBS
    from smap_amd.labels import gaussian_taps, pack_table, render_labels, root_depth_labels
    bodys = z["small_p5_bodys"]
    ok = dict(kernels=[(5, 5)], thres=[1], paf_vector=LIMBS, stride=STRIDE, shape=(17, 23))
    pack_table([bodys], **ok)
    for change in (dict(shape=(7, 23)), dict(shape=(17, 7)), dict(shape=(256, 129)), dict(kernels=[(4, 5)]), dict(kernels=[(5, 17)]),
                   dict(kernels=[]), dict(thres=[1, 2]), dict(paf_vector=LIMBS[:13]), dict(kernels=[(5, 5)] * 9, thres=[1] * 9)):
        with pytest.raises(ValueError):
            pack_table([bodys], **dict(ok, **change))
    with pytest.raises(ValueError):
        pack_table([], **ok)
    for bad in (bodys[:, :14], bodys[:, :, :3], bodys[0], np.zeros((65, 15, 4))):
        with pytest.raises(ValueError):
            pack_table([bad], **ok)
    nan = bodys.copy()
    nan[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        pack_table([nan], **ok)
    for x, y in ((23 * STRIDE, 10.0), (10.0, 17 * STRIDE), (-0.5, 10.0), (10.0, -4.0)):
        out = bodys.copy()
        out[1, 3, :2], out[1, 3, 3] = (x, y), 1
        with pytest.raises(ValueError, match="outside"):
            pack_table([out], **ok)
        out[1, 3, 3] = 0                                       # invisible: not rendered, not an error
        pack_table([out], **ok)
    with pytest.raises(ValueError):
        gaussian_taps(6)
    with pytest.raises(ValueError, match="GPU"):
        render_labels([bodys], spec_for((17, 23)), device="cpu")
    with pytest.raises(ValueError):
        root_depth_labels(bodys[:, :, :7], 0.5, spec_for((17, 23)))


def test_run_inference_refuses_maps_from_gt(tmp_path):
    """-t run_inference has no annotations to render from: the flag is refused before anything is loaded, --dry_run included."""
    env = dict(os.environ, PROJECT_HOME=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, os.path.join(ROOT, "exps", "stage3_root2", "test.py"), "-t", "run_inference", "--maps_from_gt", "1",
           "--dataset_path", str(tmp_path)]
    for extra in ([], ["--dry_run", "1"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
        assert r.returncode == 2 and "--maps_from_gt 1" in r.stderr and "run_inference" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(cmd[:2] + ["-t", "generate_result", "--maps_from_gt", "1", "--dry_run", "1"], capture_output=True, text=True,
                       timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode == 2 and "--dry_run" in r.stderr
