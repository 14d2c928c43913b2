"""GPU suite of the JPEG decode: smap_jpeg_reconstruct (csrc/jpeg.hip) after the native Huffman decode equals what the loader hands
the network today (dataset.decode.read_bgr), torch.equal, on the fixture matrix of tests/jpeg_ref.py and full-size frames; the
pre-processed batch is the same; and `test.py --device_preprocess 1 --device_decode 1` writes the host loader's result file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_ref as R
from helpers import make_cfg
from recipe import recipe_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def _frames():
    out = R.fixture_matrix(large=True)
    for j, (ss, kind, kw) in enumerate([("4:2:0", "smooth", dict(optimize=True)), ("4:2:2", "noise", dict(restart_marker_rows=1)),
                                        ("4:4:4", "primaries", {}), ("grey", "smooth", {})]):
        out.append((f"1024x1664_{ss}_{kind}", R.encode(R.content(kind, 1024, 1664, j), 90, ss, grey=ss == "grey", **kw)))
    for o in range(1, 9):
        out.append((f"1081x1921_exif{o}", R.encode(R.content("smooth", 1081, 1921, o), 85, "4:2:0", orientation=o)))
    return out


def test_reconstruct_equals_pil():
    from smap_amd import jpeg as J
    n = 0
    for name, data in _frames():
        info = J.probe(data)
        assert info is not None, name
        got = J.reconstruct(J.decode_coefficients(data, info), info, DEV)
        want = torch.from_numpy(np.array(R.pil_bgr(data)))
        assert torch.equal(got.cpu(), want), (name, (got.cpu().int() - want.int()).abs().max().item())
        n += 1
    assert n > 290


def test_decode_falls_back_to_pil_with_the_same_tensor(tmp_path):
    from PIL import Image
    from smap_amd import jpeg as J
    rgb = R.content("smooth", 70, 90)
    prog = tmp_path / "p.jpg"
    Image.fromarray(rgb).save(prog, "JPEG", progressive=True)
    png = tmp_path / "x.png"
    Image.fromarray(rgb).save(png)
    base = R.encode(rgb, 80, "4:2:0", orientation=8)
    for src in (str(prog), str(png), base, prog.read_bytes()):
        data = src if isinstance(src, bytes) else open(src, "rb").read()
        got = J.decode(src, DEV)
        assert got.device == DEV and torch.equal(got.cpu(), torch.from_numpy(np.array(R.pil_bgr(data))))


def test_preprocess_batch_of_device_decoded_frames_equals_pil_frames():
    from exps.stage3_root2.config import cfg
    from smap_amd import jpeg as J
    from smap_amd.preprocess import preprocess_batch
    files = [R.encode(R.content(k, h, w, i), 90, ss, orientation=o) for i, (k, h, w, ss, o) in enumerate(
        [("smooth", 1080, 1920, "4:2:0", None), ("noise", 480, 640, "4:2:2", 6), ("primaries", 1024, 1664, "4:4:4", 3),
         ("smooth", 300, 900, "4:2:0", 8)])]
    dev = [J.decode(f, DEV) for f in files]
    pil = [R.pil_bgr(f) for f in files]
    a, sa = preprocess_batch(dev, cfg.INPUT.MEANS, cfg.INPUT.STDS, DEV)
    b, sb = preprocess_batch(pil, cfg.INPUT.MEANS, cfg.INPUT.STDS, DEV)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and sa == sb


def test_cli_device_decode_equals_host_loader(tmp_path):
    """`test.py --device_preprocess 1 --device_decode 1` on a folder of baseline JPEGs of several sizes and subsamplings, one progressive
    JPEG, one PNG and one EXIF-rotated JPEG (batch 2, a ragged last batch) writes the host loader's result file record for record; the two
    PIL fallbacks are counted in the log."""
    from PIL import Image
    from model.smap import SMAP
    imgdir = tmp_path / "imgs"
    imgdir.mkdir()
    specs = [((512, 832), "4:2:0", "noise"), ((480, 640), "4:2:2", "smooth"), ((1080, 1920), "4:4:4", "noise"),
             ((1024, 1664), "4:2:0", "primaries"), ((300, 900), "grey", "noise")]
    for i, ((h, w), ss, kind) in enumerate(specs):
        (imgdir / f"f{i}.jpg").write_bytes(R.encode(R.content(kind, h, w, i), 90, ss, grey=ss == "grey"))
    (imgdir / "f5.jpg").write_bytes(R.encode(R.content("noise", 640, 480, 5), 85, "4:2:0", orientation=6))
    Image.fromarray(R.content("noise", 400, 600, 6)).save(imgdir / "f6.jpg", "JPEG", progressive=True, quality=90)
    Image.fromarray(R.content("noise", 360, 500, 7)).save(imgdir / "f7.png")
    torch.manual_seed(0)
    net = SMAP(make_cfg((128, 208))).eval()
    sd = recipe_state_dict(net.state_dict())
    for k in list(sd):
        if k.endswith("up4.res_conv2.bn.bias"):
            sd[k] = sd[k] + 40.0
    torch.save({"model": sd}, tmp_path / "SMAP.pth")
    res, logs = {}, {}
    for tag, extra, env_extra in (("host", [], {}),
                                  ("devdec", ["--device_preprocess", "1", "--device_decode", "1"], {"SMAP_DECODE_THREADS": "3"}),
                                  ("devdec1", ["--device_preprocess", "1", "--device_decode", "1"], {"SMAP_DECODE_THREADS": "1"})):
        env = dict(os.environ, PROJECT_HOME=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""),
                   **env_extra)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "exps", "stage3_root2", "test.py"), "-p", str(tmp_path / "SMAP.pth"),
                            "-t", "run_inference", "-d", "test", "--batch_size", "2", "--dataset_path", str(imgdir), "--json_name", tag]
                           + extra, capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        logs[tag] = r.stderr
        res[tag] = json.loads((tmp_path / "model_logs" / "stage3_root2" / "result" / f"stage3_root2_run_inference_test_{tag}.json").read_text())
    assert len(res["host"]["3d_pairs"]) >= 3, "the set-up must produce frames with persons"
    assert res["devdec"] == res["host"]
    assert res["devdec1"] == res["host"]
    assert "device decode: 2 of 8 frames fell back to PIL" in logs["devdec"]
    assert "device decode: 2 of 8 frames fell back to PIL" in logs["devdec1"]
