"""CPU suite of the JPEG decode (smap_amd/jpeg.py, csrc/jpeg_host.cpp): the native marker parse + Huffman decode followed by the numpy
restatement of the GPU half (tests/jpeg_ref.py) equals what the loader hands the network today (dataset.decode.read_bgr: PIL on
libjpeg-turbo, EXIF transposed), byte for byte, on a matrix of Pillow-encoded fixtures; files outside the supported subset and damaged
files are classified, never decoded wrong; the host code is clean under AddressSanitizer; concurrent calls give the serial results."""
import ctypes as C
import io
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rc(data):
    """(probe rc, decode rc or None)"""
    from smap_amd import lib as L
    lib = L.load()
    info = L.JpegInfo()
    rc = lib.smap_jpeg_probe(data, len(data), C.byref(info))
    if rc != 0:
        return rc, None
    co = np.empty(info.coef_bytes // 2, np.int16)
    return rc, lib.smap_jpeg_decode_coefficients(data, len(data), C.byref(info), co.ctypes.data_as(C.c_void_p))


@pytest.fixture(scope="module")
def matrix():
    return R.fixture_matrix(large=True)


def test_native_decode_plus_reference_reconstruction_equals_pil(matrix):
    from smap_amd import jpeg as J
    assert len(matrix) > 250
    seen = set()
    for name, data in matrix:
        info = J.probe(data)
        assert info is not None, name
        co = J.decode_coefficients(data, info, pin=False)
        assert co is not None, name
        want = R.pil_bgr(data)
        assert J.output_shape(info) == want.shape[:2], name
        got = R.reconstruct(co.numpy(), info)
        assert np.array_equal(got, want), (name, int(np.abs(got.astype(int) - want.astype(int)).max()))
        seen.add((info.ncomp, info.h_samp[0], info.v_samp[0], info.orientation, info.restart_interval > 0))
    assert {(3, 1, 1), (3, 2, 1), (3, 2, 2), (1, 1, 1)} == {s[:3] for s in seen}
    assert {s[3] for s in seen} == set(range(1, 9)) and {s[4] for s in seen} == {False, True}


def _scan_start(data):
    from smap_amd import jpeg as J
    return J.probe(data).scan_offset


def test_classification_of_unsupported_and_damaged_files():
    from smap_amd.lib import JPEG_E_DATA as BAD, JPEG_UNSUPPORTED as UNSUP
    from PIL import Image
    rgb = R.content("smooth", 40, 56)
    im = Image.fromarray(rgb)

    def save(img, **kw):
        b = io.BytesIO()
        img.save(b, "JPEG", **kw)
        return b.getvalue()
    assert _rc(save(im, progressive=True)) == (UNSUP, None)
    assert _rc(save(im, keep_rgb=True)) == (UNSUP, None)                     # Adobe transform 0: RGB-coded
    assert _rc(save(im.convert("CMYK"))) == (UNSUP, None)
    # 4:1:1 (Pillow cannot write it): the luma sampling byte of a 4:4:4 file's SOF set to 4x1 -- refused at the marker parse already
    b444 = bytearray(save(im, subsampling="4:4:4"))
    sof = bytes(b444).index(b"\xff\xc0")
    assert b444[sof + 11] == 0x11
    b444[sof + 11] = 0x41
    assert _rc(bytes(b444)) == (UNSUP, None)
    # an APP1 that is not EXIF (XMP: PIL reads an orientation from it) is not guessed at
    plain = save(im)
    xmp = b"http://ns.adobe.com/xap/1.0/\x00<x:xmpmeta><tiff:Orientation>6</tiff:Orientation></x:xmpmeta>"
    seg = b"\xff\xe1" + (len(xmp) + 2).to_bytes(2, "big") + xmp
    assert _rc(plain[:2] + seg + plain[2:]) == (UNSUP, None)
    png = io.BytesIO()
    im.save(png, "PNG")
    assert _rc(png.getvalue())[0] in (UNSUP, BAD)
    rng = np.random.default_rng(3)
    for _ in range(20):
        assert _rc(rng.integers(0, 256, 300, dtype=np.uint8).tobytes())[0] in (UNSUP, BAD)
    # damaged baseline files: the markers parse, the entropy-coded data does not
    assert _rc(plain) == (0, 0)
    for cut in (len(plain) - 1, len(plain) - 2, (len(plain) + _scan_start(plain)) // 2):
        assert _rc(plain[:cut]) == (0, BAD), cut                               # truncated
    s0 = _scan_start(plain)
    mid = (s0 + len(plain)) // 2
    bad = plain[:mid] + b"\xff\x00" * 4 + plain[mid + 8:]                      # 32 one-bits: no Huffman code is all ones
    assert _rc(bad) == (0, BAD)
    assert _rc(plain[:-2] + b"\x12\x34" + plain[-2:]) == (0, BAD)              # data left over after the last MCU
    rst = save(im, restart_marker_blocks=1)
    k = rst.index(b"\xff\xd1", _scan_start(rst))                               # the second restart marker ...
    assert _rc(rst) == (0, 0)
    assert _rc(rst[:k] + b"\xff\xd2" + rst[k + 2:]) == (0, BAD)                # ... out of sequence
    assert _rc(rst[:k] + rst[k + 2:]) == (0, BAD)                              # ... missing
    # ... and in every one of these cases PIL still does what it always did (the caller falls back to it)
    with pytest.raises(OSError):
        R.pil_bgr(plain[:len(plain) // 2])


def test_exif_orientation_values_and_odd_exif():
    from smap_amd import jpeg as J
    from smap_amd.lib import JPEG_UNSUPPORTED as UNSUP
    rgb = R.content("primaries", 12, 20)
    for o in (0, 9, 300):                                                      # out of range: exif_transpose leaves the image alone
        data = R.encode(rgb, 90, "4:4:4", orientation=o)
        info = J.probe(data)
        assert info is not None and info.orientation == 1
        assert np.array_equal(R.reconstruct(J.decode_coefficients(data, info, pin=False).numpy(), info), R.pil_bgr(data))
    data = R.encode(rgb, 90, "4:4:4", orientation=6)
    i = data.index(b"Exif\x00\x00")
    assert _rc(data[:i + 6] + b"XX" + data[i + 8:])[0] == UNSUP              # not a TIFF header


def test_native_decode_from_many_threads_equals_serial(matrix):
    from smap_amd import jpeg as J
    files = [d for _, d in matrix][::7][:48]

    def one(data):
        info = J.probe(data)
        return J.decode_coefficients(data, info, pin=False).numpy().copy()
    serial = [one(d) for d in files]
    with ThreadPoolExecutor(8) as ex:
        for _ in range(3):
            par = list(ex.map(one, files))
            assert all(np.array_equal(a, b) for a, b in zip(serial, par))


def test_host_decoder_under_address_sanitizer(tmp_path):
    """tests/c/jpeg_asan_main.cpp + csrc/jpeg_host.cpp built for the CPU with -fsanitize=address,undefined: every truncation and a few
    thousand random byte mutations of several files -- no report, no crash, the intact files decode."""
    exe = tmp_path / "jpeg_asan"
    r = subprocess.run(["g++", "-g", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "jpeg_asan_main.cpp"),
                        os.path.join(ROOT, "smap_amd", "csrc", "jpeg_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = [R.encode(R.content("noise", 40, 70), 75, "4:2:0", restart_marker_blocks=2),
             R.encode(R.content("smooth", 33, 65), 95, "4:2:2", orientation=6, optimize=True),
             R.encode(R.content("primaries", 17, 9), 50, grey=True, restart_marker_rows=1),
             R.encode(R.content("smooth", 24, 24), 100, "4:4:4")]
    for i, data in enumerate(cases):
        p = tmp_path / f"c{i}.jpg"
        p.write_bytes(data)
        r = subprocess.run([str(exe), str(p), "3000"], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        first, ok, unsup, bad = map(int, r.stdout.split())
        assert first == 0 and bad > 0


def test_device_decode_flag_requires_device_preprocess():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "exps", "stage3_root2", "test.py"), "--dry_run", "1", "--device_decode", "1"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 2 and "--device_decode 1 requires --device_preprocess 1" in r.stderr, r.stderr[-2000:]
