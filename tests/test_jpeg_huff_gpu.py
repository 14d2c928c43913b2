"""GPU suite of the Huffman decode on the device (smap_amd/csrc/jpeg_huff.hip): smap_jpeg_decode_coefficients_device vouches (status 0)
for exactly the coefficients of the host decoder smap_jpeg_decode_coefficients -- existing code, the reference here -- torch.equal, on
the fixture matrix of tests/jpeg_ref.py and the extra files of tests/jpeg_huff_ref.py; it refuses the damaged files; and
`J.decode(..., huffman="device")` / `test.py --device_preprocess 1 --device_decode 2` give what PIL / the host loader give."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_huff_ref as H
import jpeg_ref as R
from helpers import make_cfg
from recipe import recipe_state_dict

pytestmark = pytest.mark.gpu
ROOT = H.ROOT
DEV = torch.device("cuda:0")
SUBSEQS = [16, 64, 0]                                             # 0 = the shipped default


@pytest.fixture(scope="module")
def files():
    return R.fixture_matrix(large=True) + H.extras()


@pytest.fixture(scope="module")
def reference(files):
    """(info, the host decoder's coefficients) of every file: computed once, never modified."""
    from smap_amd import jpeg as J
    out = []
    for name, data in files:
        info = J.probe(data)
        assert info is not None, name
        co = J.decode_coefficients(data, info, pin=False)
        assert co is not None, name
        out.append((info, co))
    return out


def _decode(data, info, subseq, rounds):
    """-> (coefficients on the device, status as an int)"""
    from smap_amd import jpeg as J
    scan = J.scan_tables(data, info)
    assert scan is not None
    co, st = J.decode_coefficients_device(data, info, scan, DEV, subseq_bytes=subseq, rounds=rounds)
    return co, int(st.item())


def _check(files, reference, subseq, enough_rounds, only=None):
    from smap_amd import jpeg as J
    bad = []
    for (name, data), (info, want) in zip(files, reference):
        if only is not None and not only(name):
            continue
        rounds = J.huff_groups(info, len(data), subseq) if enough_rounds else 0
        co, st = _decode(data, info, subseq, rounds)
        if st != 0 or not torch.equal(co, want.to(DEV)):
            bad.append((name, st))
    assert not bad, bad[:8]


@pytest.mark.parametrize("subseq", SUBSEQS)
def test_coefficients_bit_for_bit_with_provably_enough_rounds(files, reference, subseq):
    _check(files, reference, subseq, True)
    seen = {(i.ncomp, i.h_samp[0], i.v_samp[0], i.restart_interval > 0) for i, _ in reference}
    assert {(3, 1, 1), (3, 2, 1), (3, 2, 2), (1, 1, 1)} == {s[:3] for s in seen} and {s[3] for s in seen} == {False, True}
    size = subseq or H.DEFAULT_SUBSEQ
    assert max(H.groups(d, size) for _, d in files) > 4              # more subsequences than four workgroups hold
    # edge (a): a subsequence that starts on the 0x00 of a stuffed pair, and one that starts inside an RSTn -- present at this size
    stuffed, rst = H.boundary_census(files, size)
    assert stuffed > 0 and rst > 0, (stuffed, rst)


def test_shipped_defaults(files, reference):
    """Default subseq_bytes and rounds: status 0 on every file (NOT_CONVERGED is legal in production, not here)."""
    _check(files, reference, 0, False)


def test_edges(files, reference):
    names = [n for n, _ in files]
    # (b) blocks longer than several 16-byte subsequences, codes longer than 9 bits
    assert sum(n.startswith("long_blocks_") for n in names) == 2
    _check(files, reference, 16, True, lambda n: n.startswith("long_blocks_"))
    # (c) a scan shorter than one subsequence: the 1x1 files
    tiny = [d for n, d in files if n.startswith("1x1_")]
    from smap_amd import jpeg as J
    assert tiny and min(len(d) - J.probe(d).scan_offset for d in tiny) < 16
    for s in SUBSEQS:
        _check(files, reference, s, False, lambda n: n.startswith("1x1_"))
    # (d) a marker after every MCU, at 16 bytes and at the default
    assert reference[names.index("rst_every_mcu")][0].restart_interval == 1
    for s in (16, 0):
        _check(files, reference, s, False, lambda n: n == "rst_every_mcu")
        _check(files, reference, s, True, lambda n: n == "rst_every_mcu")
    # (e) 512x832 without restart markers, every sampling, default size: scans over many workgroups
    plain = [(n, d) for n, d in files if n.startswith("512x832_") and n.endswith("_plain")]
    assert len(plain) == 4 and all(H.groups(d, H.DEFAULT_SUBSEQ) > 4 for _, d in plain)
    assert all(reference[names.index(n)][0].restart_interval == 0 for n, _ in plain)
    _check(files, reference, 0, False, lambda n: n.endswith("_plain"))


def test_refusals():
    """The damaged baseline files (clean in the CPU twin under ASan: tests/test_jpeg_huff_cpu.py): the call returns, the status is not 0."""
    from smap_amd import jpeg as J
    for name, data in H.damaged():
        info = J.probe(data)
        assert info is not None and J.decode_coefficients(data, info, pin=False) is None, name
        for subseq, rounds in ((0, 0), (16, J.huff_groups(info, len(data), 16))):
            _, st = _decode(data, info, subseq, rounds)
            assert st != 0, (name, subseq)


def _frames():
    out = []
    for j, (ss, kind, kw) in enumerate([("4:2:0", "smooth", dict(optimize=True)), ("4:2:2", "noise", dict(restart_marker_rows=1)),
                                        ("4:4:4", "primaries", {}), ("grey", "smooth", {})]):
        out.append((f"1024x1664_{ss}_{kind}", R.encode(R.content(kind, 1024, 1664, j), 90, ss, grey=ss == "grey", **kw)))
    for o in range(1, 9):
        out.append((f"1081x1921_exif{o}", R.encode(R.content("smooth", 1081, 1921, o), 85, "4:2:0", orientation=o)))
    return out


def test_decode_with_device_huffman_equals_pil():
    from smap_amd import jpeg as J
    for name, data in _frames():
        info = J.probe(data)
        _, st = _decode(data, info, 0, 0)
        assert st == 0, name                                                 # (the device path, not its host fallback, is what is compared)
        got = J.decode(data, DEV, huffman="device")
        want = torch.from_numpy(np.array(R.pil_bgr(data)))
        assert got.device == DEV and torch.equal(got.cpu(), want), name


def test_two_decodes_give_identical_bytes(files, reference):
    names = [n for n, _ in files]
    for n in ("512x832_4:2:0_plain", "long_blocks_4:4:4", "rst_every_mcu"):
        k = names.index(n)
        runs = [_decode(files[k][1], reference[k][0], 0, 0) for _ in range(2)]
        assert runs[0][1] == runs[1][1] == 0 and torch.equal(runs[0][0], runs[1][0]), n


def test_cli_device_decode_2_equals_host_loader(tmp_path):
    """`test.py --device_preprocess 1 --device_decode 2` on the folder of test_jpeg_gpu's CLI test (baseline JPEGs of several sizes and
    samplings, an EXIF-rotated one, one progressive JPEG, one PNG; batch 2, a ragged last batch) writes the host loader's result file
    record for record, with pool threads and without.  With a truncated baseline file added -- the device refuses it, the host decoder
    refuses it, PIL refuses it -- the run ends with PIL's error, as every other loader's does."""
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

    def run(tag, extra, env_extra):
        env = dict(os.environ, PROJECT_HOME=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env_extra)
        return subprocess.run([sys.executable, os.path.join(ROOT, "exps", "stage3_root2", "test.py"), "-p", str(tmp_path / "SMAP.pth"),
                               "-t", "run_inference", "-d", "test", "--batch_size", "2", "--dataset_path", str(imgdir), "--json_name", tag]
                              + extra, capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    mode2 = ["--device_preprocess", "1", "--device_decode", "2"]
    res, logs = {}, {}
    for tag, extra, env_extra in (("host", [], {}), ("huff", mode2, {"SMAP_DECODE_THREADS": "3"}), ("huff1", mode2, {"SMAP_DECODE_THREADS": "1"})):
        r = run(tag, extra, env_extra)
        assert r.returncode == 0, r.stderr[-3000:]
        logs[tag] = r.stderr
        res[tag] = json.loads((tmp_path / "model_logs" / "stage3_root2" / "result" / f"stage3_root2_run_inference_test_{tag}.json").read_text())
    assert len(res["host"]["3d_pairs"]) >= 3, "the set-up must produce frames with persons"
    assert res["huff"] == res["host"]
    assert res["huff1"] == res["host"]
    for tag in ("huff", "huff1"):
        assert "device decode: 0 of 8 frames were redone on the host, 2 fell back to PIL" in logs[tag], logs[tag][-2000:]
    whole = (imgdir / "f0.jpg").read_bytes()
    (imgdir / "f8.jpg").write_bytes(whole[:len(whole) // 2])
    with pytest.raises(OSError):
        R.pil_bgr(whole[:len(whole) // 2])
    r = run("cut", mode2, {"SMAP_DECODE_THREADS": "3"})
    assert r.returncode != 0 and "OSError" in r.stderr, r.stderr[-3000:]
