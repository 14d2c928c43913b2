"""GPU: the label renderer (csrc/labels.hip smap_render_labels, smap_amd/labels.py, dataset/representation.py) and the paths built
on it (PosePipeline(maps_source=...), test.py --maps_from_gt 1).

The part-affinity / relative-depth fields are compared BIT FOR BIT with tests/golden/labels.npz, which holds the output of the
reference's own generate_paf (tests/golden/gen_golden_labels.py).  The heat-maps are compared bit for bit with the numpy restatement of
cv2.GaussianBlur in tests/golden/labels_restate.py (OpenCV is not installed where the fixture is written: stated, not executed)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
STRIDE, NJ = 4, 15
IMG_W, IMG_H = 1920, 1080                                      # the frame the annotations of the `pipe` scene belong to


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(bits(a), bits(b))


def spec_for(shape, kernels=None):
    from labels_restate import KERNELS, LIMBS
    from smap_amd.labels import LabelSpec
    return LabelSpec(tuple(KERNELS if kernels is None else kernels), tuple(LIMBS), 1, STRIDE, tuple(int(v) for v in shape), 2, 20)


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "labels.npz"))


@pytest.fixture(scope="module")
def rendered(z):
    """Every scene of the fixture rendered ONCE per with_mds value: name -> {flag: labels [5, 57, H, W]} (host copies)."""
    from smap_amd.labels import render_labels
    out = {}
    for name in z["names"]:
        spec = spec_for(z[name + "_shape"])
        out[str(name)] = {mds: render_labels([z[name + "_bodys"]], spec, with_mds=mds, device=DEV)[0].cpu().numpy() for mds in (False, True)}
    return out


def fixture_paf(z, name, width, mds):
    key = "%s_paf_w%d_m%d" % (name, width, int(mds))
    return z[key] if key in z.files else z[str(z[key + "_same"])]


def test_fields_equal_the_references_bit_for_bit(z, rendered):
    """Every scene x line width (3, 2, 1 = label scales 0, 1, 2) x with_mds; scales 3 and 4 repeat width 1."""
    checked, nonzero = 0, 0
    for name, by_flag in rendered.items():
        for mds, lab in by_flag.items():
            assert lab.shape[:2] == (5, 57)
            for s, width in enumerate((3, 2, 1, 1, 1)):
                want = fixture_paf(z, name, width, mds)
                assert same_bits(lab[s, NJ:], want), (name, width, mds)
                checked += 1
                nonzero += int((want != 0).sum())
    assert checked == len(z["names"]) * 10 and nonzero > 100000
    # the scenes hold what they are there for
    assert int(z["big_special20_max_cover"]) >= 3 and int(z["small_special20_max_cover"]) >= 3
    assert not rendered["small_invisible"][False].any() and not rendered["big_p0"][True].any()
    assert not same_bits(rendered["small_special20"][False][0], rendered["small_special20"][True][0])     # the flag matters at width 3
    b = z["big_special20_bodys"]
    assert np.array_equal(b[12], b[13])                                                                   # the two identical persons


def test_heatmaps_equal_the_restated_blur_bit_for_bit(z, rendered):
    """All five kernel sizes on every scene against labels_restate.heatmaps run here, and against the recorded output of the
    reference's generate_heatmap around that blur where the fixture has it; peaks are 255 up to the division's rounding."""
    import labels_restate as R
    recorded = 0
    for name, by_flag in rendered.items():
        shape, bodys = tuple(z[name + "_shape"]), z[name + "_bodys"]
        assert same_bits(by_flag[False][:, :NJ], by_flag[True][:, :NJ])                  # the flag does not touch the heat-maps
        for s, k in enumerate(R.KERNELS):
            want = R.heatmaps(bodys, shape, STRIDE, k)
            got = by_flag[False][s, :NJ]
            assert same_bits(got, want), (name, k)
            key = "%s_heat_k%d" % (name, k[0])
            if key in z.files:
                assert same_bits(got, z[key]), key
                recorded += 1
            visible = (bodys[:, :, 3] >= 1).any(0) if len(bodys) else np.zeros(NJ, bool)
            peak = got.reshape(NJ, -1).max(1)                    # m / fp32(m / 255): two fp32 roundings away from 255
            assert (np.abs(peak[visible] - 255.0) <= 255.0 * 2.0 ** -23).all() and not peak[~visible].any()
    assert recorded == 20
    corners = rendered["small_special20"][False][0, :NJ]
    H, W = corners.shape[1:]
    assert corners[5, 0, 0] > 0 and corners[11, 0, W - 1] > 0 and corners[8, H - 1, 0] > 0 and corners[14, H - 1, W - 1] > 0


def test_a_batch_equals_its_frames_rendered_alone(z, rendered):
    """Three frames with 5, 0 and 20 persons in one call (P = 20 for all), into out=, on a side stream."""
    from smap_amd.labels import render_labels
    names = ("small_p5", "small_p0", "small_special20")
    spec = spec_for((17, 23))
    out = torch.full((3, 5, 57, 17, 23), float("nan"), device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = render_labels([z[n + "_bodys"] for n in names], spec, with_mds=True, device=DEV, out=out)
    side.synchronize()
    assert got is out
    for i, n in enumerate(names):
        assert same_bits(out[i].cpu().numpy(), rendered[n][True]), n
    with pytest.raises(ValueError):
        render_labels([z["small_p5_bodys"]], spec, device=DEV, out=out)
    with pytest.raises(ValueError):
        render_labels([z["small_p5_bodys"]], spec, device=DEV, out=torch.zeros((1, 5, 57, 17, 23), dtype=torch.float64, device=DEV))


@pytest.mark.parametrize("shape", [(8, 4096), (4096, 8), (9, 11)])
def test_extreme_shapes_and_rectangular_kernels(shape):
    """The largest accepted map in both orientations and a small odd one, blur kernels that are not square (width, height), 1 and 3
    taps included: against the restatement, bit for bit."""
    import labels_restate as R
    from smap_amd.labels import render_labels
    H, W = shape
    rng = np.random.default_rng(H)
    bodys = np.zeros((3, 15, 8))
    bodys[:, :, 0] = rng.uniform(0, W * STRIDE - 0.01, (3, 15))
    bodys[:, :, 1] = rng.uniform(0, H * STRIDE - 0.01, (3, 15))
    bodys[:, :, 2] = rng.uniform(100, 900, (3, 15))
    bodys[:, :, 3] = rng.choice([1, 2], (3, 15))
    bodys[0, 0, :2], bodys[1, 0, :2] = (0.0, 0.0), (W * STRIDE - 0.01, H * STRIDE - 0.01)
    kernels = [(15, 5), (3, 13), (1, 1)]
    got = render_labels([bodys], spec_for(shape, kernels), device=DEV)[0].cpu().numpy()
    for s, k in enumerate(kernels):
        assert same_bits(got[s, :NJ], R.heatmaps(bodys, shape, STRIDE, k)), k
        assert same_bits(got[s, NJ:], R.pafs(bodys, shape, STRIDE, max(1, 3 - s), False)), s
    assert (got[:, NJ:] != 0).any()


def test_the_references_import_path(z, rendered):
    """dataset.representation's three functions: numpy in, numpy out, one frame and one scale per call, the same arrays."""
    from dataset.representation import generate_heatmap, generate_paf, generate_rdepth
    from labels_restate import LIMBS
    name = "small_special20"
    bodys = [b for b in z[name + "_bodys"]]
    lab = rendered[name]
    heat = generate_heatmap(bodys, (17, 23), STRIDE, 15, kernel=(9, 9))
    assert isinstance(heat, np.ndarray) and same_bits(heat, lab[False][2, :NJ])
    assert same_bits(generate_heatmap(bodys, (17, 23), STRIDE, 15), lab[False][3, :NJ])                   # the default (7, 7)
    params = {"stride": STRIDE, "crop_size_y": 17 * STRIDE, "crop_size_x": 23 * STRIDE}
    for width, mds in ((3, True), (2, False), (1, True)):
        paf = generate_paf(bodys, (17, 23), params, 14, LIMBS, width, mds)
        assert isinstance(paf, np.ndarray) and same_bits(paf, fixture_paf(z, name, width, mds))
    assert not generate_paf([], (17, 23), params, 14, LIMBS, 1, False).any()
    rd = generate_rdepth({"bodys": bodys, "scale": float(z["scale"])}, STRIDE, 2, 20)
    assert same_bits(rd, z[name + "_rdepth"])
    with pytest.raises(ValueError):
        generate_paf(bodys, (17, 24), params, 14, LIMBS, 1, False)


def test_gt_maps_are_the_sum_of_the_supervising_scales(z, rendered):
    from smap_amd.labels import gt_maps, root_depth_map
    name = "pipe"
    spec = spec_for((128, 208))
    lab = torch.from_numpy(rendered[name][False][None]).to(DEV)
    bodys, scale = z[name + "_bodys"], float(z["scale"])
    hms, det_d, root_d = gt_maps(lab, [bodys], [{"scale": scale}], spec)
    L = rendered[name][False]
    idx2d = list(range(NJ)) + [NJ + c for c in range(42) if c % 3 != 2]
    assert same_bits(hms[0].cpu().numpy(), (L[4][idx2d] + L[3][idx2d]) + L[2][idx2d])
    assert same_bits(det_d[0].cpu().numpy(), L[4][NJ + 2::3]) and tuple(det_d.shape) == (1, 14, 128, 208)
    assert same_bits(root_d.cpu().numpy(), root_depth_map([bodys], [scale], spec)) and int((root_d != 0).sum()) == 3 * 49
    with pytest.raises(ValueError):
        gt_maps(lab[:, :2], [bodys], [scale], spec)


def pipe_frame(z):
    """The `pipe` scene as the annotated loader hands it over: (padded fp32 annotations [20, 15, 11], meta dict)."""
    ann = np.zeros((20, 15, 11), np.float32)
    ann[:3] = z["pipe_bodys"]
    meta = {"scale": float(z["scale"]), "img_width": IMG_W, "img_height": IMG_H, "net_width": 832, "net_height": 512}
    return ann, meta


def test_pipeline_with_a_maps_source_records_what_the_maps_hold(z):
    """PosePipeline(record_mode="generate_result", maps_source=GtMapsSource) without a model: a frame with the three annotated persons
    and a frame without annotations.  The records are those benchkit.parity.frames_from_maps gives for the same (scaled) maps --
    the run_inference flavour of association + lifting, fp32 where the ground-truth flavour is fp64 -- matched by root; every root
    depth is the annotated Z within the fp32 roundings of Z / f / scale * scale * f."""
    from benchkit.parity import frames_from_maps
    from exps.stage3_root2.config import cfg
    from smap_amd.labels import GtMapsSource, label_spec
    from smap_amd.pipeline import PosePipeline
    from smap_amd.records import annotation_camera, kept_annotations
    assert int(z["pipe_found"]) == 3
    ann, meta = pipe_frame(z)
    kept = kept_annotations(ann, 2)
    assert len(kept) == 3
    cams = [annotation_camera(kept, meta), [1.0] * 9]
    pipe = PosePipeline(None, cfg, 2, 512, 832, DEV, record_mode="generate_result", maps_source=GtMapsSource(label_spec(cfg), DEV))
    assert pipe.engine is None
    assert pipe.submit(None, cams, ["a", "b"], annotations=[kept, kept[:0]], map_inputs=([ann, np.zeros_like(ann)], [meta, meta])) is None
    recs = pipe.flush()
    assert [r["image_path"] for r in recs] == ["a"]
    p2, p3, rz = (np.asarray(recs[0][k], np.float64) for k in ("pred_2d", "pred_3d", "root_d"))
    assert p2.shape == (3, 15, 4) and np.array_equal(np.asarray(recs[0]["gt_2d"], np.float32), kept[:, :, :4])
    hms, det_d, root_d = pipe.last_maps()
    assert not hms[1].any() and abs(float(hms[0, :NJ].max()) - 3.0) <= 3.0 * 2.0 ** -21     # three scales of ~255, / 255
    frames = frames_from_maps(hms, det_d, root_d, np.asarray(cams, np.float64))
    assert len(frames[0]["p2"]) == 3 and len(frames[1]["p2"]) == 0
    order = [int(np.argmin(np.abs(frames[0]["p2"][:, 2, :2] - p2[g, 2, :2]).sum(1))) for g in range(3)]
    assert sorted(order) == [0, 1, 2]
    f2, f3, fz = frames[0]["p2"][order], frames[0]["p3"][order], frames[0]["rz"][order]
    assert np.array_equal(f2.astype(np.float64)[:, :, :2], p2[:, :, :2]) and np.array_equal(f2[:, :, 3] > 0, p2[:, :, 3] > 0)
    # registration puts person g at annotation g: its root within a cell of the annotated one, its depth the annotated Z
    Z = kept[:, 2, 2].astype(np.float64)
    assert (np.abs(p2[:, 2, :2] - kept[:, 2, :2]) <= STRIDE).all()
    U = 2.0 ** -24
    print("root depth: max |rz - Z| / Z = %.3e (bound %.3e)" % (float(np.max(np.abs(rz - Z) / Z)), 5 * U))
    assert (np.abs(rz - Z) <= 5 * U * Z).all()             # fp32(Z / f / scale), fp32(scale), two fp32 products: 4 roundings (+ 2nd order)
    assert np.allclose(fz, rz, rtol=5 * U, atol=0)         # the fp64 flavour of the same product
    found = p2[:, :, 3] > 0
    assert found.sum() >= 30
    # the same formulas in fp32 and fp64 on the same maps: a dozen fp32 roundings on centimetres
    assert np.allclose(f3[found][:, :3], p3[found][:, :3], rtol=1e-5, atol=1e-3)
    with pytest.raises(ValueError, match="ground-truth"):
        PosePipeline(None, cfg, 2, 512, 832, DEV, maps_source=GtMapsSource(label_spec(cfg), DEV))


def write_annotations(tmp_path, z):
    """An annotation file of three frames (3, 2 and 1 persons of the `pipe` scene) whose image files do NOT exist."""
    from dataset.base_dataset import croppad_geometry
    scale, _, (left, top) = croppad_geometry(IMG_W, IMG_H, 832, 512)
    assert abs(scale - float(z["scale"])) < 1e-15
    root = tmp_path / "MultiPersonTestSet"
    root.mkdir()
    entries = []
    for i, n in enumerate((3, 2, 1)):
        b = z["pipe_bodys"][:n].copy()
        b[:, :, 0] = (b[:, :, 0] - left) / scale
        b[:, :, 1] = (b[:, :, 1] - top) / scale
        entries.append({"dataset": "MUCO", "img_paths": "TS1/missing_%06d.jpg" % i, "img_width": IMG_W, "img_height": IMG_H,
                        "isValidation": 1, "bodys": b.tolist()})
    (root / "M3E_gt.json").write_text(json.dumps({"root": entries}))
    return root


def test_cli_maps_from_gt_end_to_end(tmp_path, z):
    """`test.py -t generate_result --maps_from_gt 1 --eval_3d 1 --eval_maps 1` on annotations without images and without a
    checkpoint: exit status 0, one record per frame with every annotated person, an `error` dict; a second run writes the same file."""
    root = write_annotations(tmp_path, z)
    env = dict(os.environ, PROJECT_HOME=str(tmp_path), SMAP_TEST_ROOT=str(root),
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, os.path.join(ROOT, "exps", "stage3_root2", "test.py"), "-p", str(tmp_path / "no_such_checkpoint.pth"),
           "-t", "generate_result", "-d", "test", "--batch_size", "2", "--maps_from_gt", "1", "--eval_3d", "1", "--eval_maps", "1",
           "--do_flip", "1"]
    docs = []
    for tag in ("one", "two"):
        r = subprocess.run(cmd + ["--json_name", tag], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        assert "ignored" in r.stderr
        path = tmp_path / "model_logs" / "stage3_root2" / "result" / ("stage3_root2_generate_result_test_%s.json" % tag)
        docs.append(path.read_bytes())
    assert docs[0] == docs[1]
    doc = json.loads(docs[0])
    assert [r["image_path"] for r in doc["3d_pairs"]] == ["TS1/missing_%06d.jpg" % i for i in range(3)]
    for r, n in zip(doc["3d_pairs"], (3, 2, 1)):
        p3 = np.asarray(r["pred_3d"])
        assert p3.shape == (n, 15, 4) and len(r["gt_3d"]) == n and (p3[:, 2, 3] > 0).all()
        Z = np.asarray(r["gt_2d"])[:, 2, 2]
        assert np.allclose(np.asarray(r["root_d"]), Z, rtol=1e-6, atol=0)
    assert isinstance(doc["error"], dict) and sum(doc["error"]["count_gt"]) >= 6 * 15
    print("error:", {k: (np.round(v, 3).tolist() if isinstance(v, list) else v) for k, v in doc["error"].items()})
