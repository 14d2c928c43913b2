"""CPU suite of the Huffman decode on the device (smap_amd/csrc/jpeg_huff.h, jpeg_huff.hip): the host side (smap_jpeg_scan_tables and its
binding), the flag, and the ALGORITHM -- tests/c/jpeg_huff_twin_main.cpp runs the phases of the kernels over the same per-subsequence
functions as plain C++ under AddressSanitizer / UBSan: on every fixture it must vouch for (status 0) exactly the host decoder's
coefficients, and on damaged input it must either refuse or still be right."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import jpeg_huff_ref as H
import jpeg_ref as R

ROOT = H.ROOT
ASAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")


@pytest.fixture(scope="module")
def files():
    return R.fixture_matrix(large=True) + H.extras()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return H.build_twin(tmp_path_factory.mktemp("twin") / "jpeg_huff_twin")


@pytest.fixture(scope="module")
def on_disk(files, tmp_path_factory):
    d = tmp_path_factory.mktemp("huff_files")
    paths = []
    for i, (_, data) in enumerate(files):
        p = d / f"{i:03d}.jpg"
        p.write_bytes(data)
        paths.append(str(p))
    return paths


def _scan_rc(data, info=None):
    """(probe rc, scan_tables rc or None)"""
    from smap_amd import lib as L
    lib = L.load()
    own = L.JpegInfo()
    rc = lib.smap_jpeg_probe(data, len(data), C.byref(own))
    if rc != 0:
        return rc, None
    scan = L.JpegScan()
    return rc, lib.smap_jpeg_scan_tables(data, len(data), C.byref(info if info is not None else own), C.byref(scan))


def test_scan_tables_on_the_matrix(files):
    from smap_amd import jpeg as J
    from smap_amd import lib as L
    lib = L.load()
    assert lib.smap_sizeof_jpeg_scan() == C.sizeof(L.JpegScan)
    assert len(files) > 280
    for name, data in files:
        info = J.probe(data)
        scan = J.scan_tables(data, info)
        assert scan is not None, name
        per_mcu = sum(info.h_samp[c] * info.v_samp[c] for c in range(info.ncomp))
        assert (scan.ncomp, scan.blocks_per_mcu, scan.restart_interval) == (info.ncomp, per_mcu, info.restart_interval), name
        assert (scan.scan_offset, scan.file_bytes, scan.total_blocks) == (info.scan_offset, len(data), info.coef_bytes // 128), name
        comps = [scan.block_comp[j] for j in range(per_mcu)]
        assert comps == sorted(comps) and set(comps) == set(range(info.ncomp)), name
        frame = J.pack_frame(data, info, pin=False)                          # the one buffer a frame uploads: tables, then the bytes
        assert bytes(frame.numpy()[:C.sizeof(L.JpegScan)]) == bytes(scan) and bytes(J.frame_bytes(frame)) == data, name
    a, b = files[0][1], files[-1][1]
    assert _scan_rc(a, J.probe(b)) == (0, -1)                  # not this file's info: SMAP_E_ARG


def test_scan_tables_classifies_like_the_host_decoder_at_the_marker_level():
    from smap_amd.lib import JPEG_E_DATA as BAD, JPEG_UNSUPPORTED as UNSUP
    from PIL import Image
    im = Image.fromarray(R.content("smooth", 40, 56))

    def save(img, **kw):
        b = io.BytesIO()
        img.save(b, "JPEG", **kw)
        return b.getvalue()
    assert _scan_rc(save(im, progressive=True)) == (UNSUP, None)
    assert _scan_rc(save(im, keep_rgb=True)) == (UNSUP, None)
    assert _scan_rc(save(im.convert("CMYK"))) == (UNSUP, None)
    b444 = bytearray(save(im, subsampling="4:4:4"))
    sof = bytes(b444).index(b"\xff\xc0")
    b444[sof + 11] = 0x41
    assert _scan_rc(bytes(b444)) == (UNSUP, None)
    png = io.BytesIO()
    im.save(png, "PNG")
    assert _scan_rc(png.getvalue())[0] in (UNSUP, BAD)
    # damaged entropy-coded data is not a matter of the markers: the tables are packed, the decode refuses (the twin and GPU tests)
    for name, data in H.damaged():
        assert _scan_rc(data) == (0, 0), name
    # a DC category above 15 in a DHT segment: the probe and the table build refuse it alike
    from smap_amd import jpeg as J
    from smap_amd import lib as L
    good = save(im)
    plain = bytearray(good)
    dht = bytes(plain).index(b"\xff\xc4")
    assert plain[dht + 4] >> 4 == 0                                          # table class 0 = DC
    plain[dht + 5 + 16] = 16
    assert _scan_rc(bytes(plain))[0] == BAD
    scan = L.JpegScan()
    assert L.load().smap_jpeg_scan_tables(bytes(plain), len(plain), C.byref(J.probe(good)), C.byref(scan)) == BAD


def _run_twin(twin, args, paths):
    r = subprocess.run([twin] + args + paths, capture_output=True, text=True, timeout=600, env=ASAN_ENV)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    rows = [line.split() for line in r.stdout.splitlines()]
    assert len(rows) == len(paths)
    return [(int(x[0]), int(x[1]), int(x[2]), int(x[3]), int(x[4])) for x in rows]


@pytest.mark.parametrize("subseq", [16, 64, 0])
def test_twin_with_provably_enough_rounds(twin, on_disk, files, subseq):
    """4 lanes per group, rounds = the number of groups: status 0 and the host decoder's coefficients on every file."""
    rows = _run_twin(twin, ["--lanes=4", f"--subseq={subseq}", "--rounds=-1"], on_disk)
    bad = [(files[i][0], row) for i, row in enumerate(rows) if row[:3] != (0, 1, 0)]
    assert not bad, bad[:5]
    assert max(row[4] for row in rows) > 4 and max(row[3] for row in rows) > 0        # the cross-group rounds did real work


def test_twin_at_the_shipped_defaults(twin, on_disk, files):
    rows = _run_twin(twin, [], on_disk)
    bad = [(files[i][0], row) for i, row in enumerate(rows) if row[:3] != (0, 1, 0)]
    assert not bad, bad[:5]
    assert max(row[4] for row in rows) > 4


def test_twin_refuses_the_damaged_files(twin, tmp_path):
    paths = []
    for name, data in H.damaged():
        (tmp_path / f"{name}.jpg").write_bytes(data)
        paths.append(str(tmp_path / f"{name}.jpg"))
    for args in ([], ["--lanes=4", "--subseq=16", "--rounds=-1"]):
        for row, p in zip(_run_twin(twin, args, paths), paths):
            assert row[0] != 0 and row[2] != 0, (p, row)                     # as the host decoder (SMAP_JPEG_E_DATA)


@pytest.mark.parametrize("args", [[], ["--lanes=4", "--subseq=16", "--rounds=-1"]])
def test_twin_truncations_and_mutations(twin, tmp_path, args):
    """Every truncation and seeded random mutations of the entropy-coded data: no sanitizer report, and never status 0 with
    coefficients other than the host decoder's (in particular never status 0 where the host decoder returns SMAP_JPEG_E_DATA)."""
    cases = [R.encode(R.content("noise", 40, 70), 75, "4:2:0", restart_marker_blocks=2),
             R.encode(R.content("smooth", 33, 65), 95, "4:2:2", orientation=6, optimize=True),
             R.encode(R.content("primaries", 17, 9), 50, grey=True, restart_marker_rows=1),
             R.encode(R.content("noise", 24, 24), 100, "4:4:4")]
    for i, data in enumerate(cases):
        p = tmp_path / f"c{i}.jpg"
        p.write_bytes(data)
        r = subprocess.run([twin] + args + [str(p), "1500"], capture_output=True, text=True, timeout=600, env=ASAN_ENV)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        first, tally = r.stdout.splitlines()
        assert first.split()[:3] == ["0", "1", "0"]
        variants, ok, violations = map(int, tally.split())
        assert variants == len(data) + 1500 and violations == 0 and ok < variants


def test_device_decode_2_requires_device_preprocess():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "exps", "stage3_root2", "test.py"), "--dry_run", "1", "--device_decode", "2"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 2 and "--device_decode 2 requires --device_preprocess 1" in r.stderr, r.stderr[-2000:]
