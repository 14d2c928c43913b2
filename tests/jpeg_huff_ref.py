"""Fixtures the Huffman-decode-on-the-device tests share (tests/test_jpeg_huff_cpu.py, tests/test_jpeg_huff_gpu.py), on top of
tests/jpeg_ref.py: the extra files with the edges the parallel decoder can get wrong, the damaged files, and the boundary census."""
import io
import os

import numpy as np

import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_SUBSEQ = 128      # SMAP_JPEG_SUBSEQ_BYTES
LANES = 256               # subsequences per workgroup (smap_huff::kLanes)


def extras():
    """-> list of (name, bytes): blocks longer than several subsequences (and codes longer than 9 bits), a marker after every MCU, and
    one 512x832 file per sampling without restart markers (their scans span many workgroups)."""
    out = []
    for ss in ("4:4:4", "4:2:0"):
        out.append((f"long_blocks_{ss}", R.encode(R.content("noise", 96, 160, 11), 100, ss, optimize=True)))
    out.append(("rst_every_mcu", R.encode(R.content("noise", 64, 120, 12), 90, "4:2:0", restart_marker_blocks=1)))
    for j, ss in enumerate(R.SUBSAMPLINGS):
        out.append((f"512x832_{ss}_plain", R.encode(R.content("noise", 512, 832, 20 + j), 92, ss, grey=ss == "grey")))
    return out


def damaged():
    """The damaged baseline files of test_jpeg_cpu.test_classification_of_unsupported_and_damaged_files: the markers parse, the
    entropy-coded data does not.  -> list of (name, bytes)."""
    from PIL import Image
    from smap_amd import jpeg as J
    im = Image.fromarray(R.content("smooth", 40, 56))

    def save(**kw):
        b = io.BytesIO()
        im.save(b, "JPEG", **kw)
        return b.getvalue()
    plain = save()
    s0 = J.probe(plain).scan_offset
    out = [(f"cut{cut}", plain[:cut]) for cut in (len(plain) - 1, len(plain) - 2, (len(plain) + s0) // 2)]
    mid = (s0 + len(plain)) // 2
    out.append(("ones", plain[:mid] + b"\xff\x00" * 4 + plain[mid + 8:]))
    out.append(("leftover", plain[:-2] + b"\x12\x34" + plain[-2:]))
    rst = save(restart_marker_blocks=1)
    k = rst.index(b"\xff\xd1", J.probe(rst).scan_offset)
    out.append(("rst_out_of_sequence", rst[:k] + b"\xff\xd2" + rst[k + 2:]))
    out.append(("rst_missing", rst[:k] + rst[k + 2:]))
    return out


def boundary_census(files, subseq):
    """(files with a subsequence that starts on the 0x00 of a stuffed pair, files with one that starts on the second byte of an RSTn)."""
    from smap_amd import jpeg as J
    stuffed = rst = 0
    for _, data in files:
        a = np.frombuffer(data, np.uint8)
        s0 = J.probe(data).scan_offset
        at = np.arange(s0 + subseq, len(a), subseq)
        prev_ff = a[at - 1] == 0xFF
        stuffed += bool(np.any(prev_ff & (a[at] == 0)))
        rst += bool(np.any(prev_ff & (a[at] >= 0xD0) & (a[at] <= 0xD7)))
    return stuffed, rst


def groups(data, subseq):
    from smap_amd import jpeg as J
    nsub = -(-(len(data) - J.probe(data).scan_offset) // subseq)
    return -(-nsub // LANES)


def build_twin(exe):
    import subprocess
    r = subprocess.run(["g++", "-g", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "jpeg_huff_twin_main.cpp"),
                        os.path.join(ROOT, "smap_amd", "csrc", "jpeg_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)
