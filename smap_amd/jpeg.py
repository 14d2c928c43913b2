"""JPEG decode split between the host and the GPU (include/smap_hip.h "JPEG decode", DESIGN.md "JPEG decode").

    info = probe(data)                        # marker parse: a JpegInfo, or None = decode this file with PIL
    coeffs = decode_coefficients(data, info)  # Huffman decode on the host (native, no interpreter lock) -> page-locked int16
    bgr = reconstruct(coeffs, info, device)   # dequantise + IDCT + chroma upsampling + YCbCr->BGR + EXIF orientation, two HIP launches

`bgr` is a uint8 [H', W', 3] tensor on the device, bit for bit what dataset.decode.read_bgr (PIL on libjpeg-turbo, EXIF transposed)
returns for the same file.  `decode` does all three, with PIL for whatever the native decoder does not take.

The Huffman decode can run on the GPU as well (csrc/jpeg_huff.hip, DESIGN.md "Huffman decode on the GPU"):

    frame = pack_frame(data, info)                                  # host: the scan's tables + the file bytes, one page-locked buffer
    coeffs, status = decode_coefficients_device(frame, info, None, device)   # one upload, a fixed sequence of launches, no wait

`status` is a device int32: 0 = `coeffs` is bit for bit decode_coefficients' output; anything else = use the host decoder."""
import ctypes as C

import numpy as np
import torch

from . import lib as _L

JpegInfo = _L.JpegInfo


def _bytes_ptr(data):
    if isinstance(data, (bytes, bytearray, memoryview)):
        arr = np.frombuffer(data, np.uint8)
    else:
        arr = np.ascontiguousarray(data, np.uint8)
    return arr, C.c_void_p(arr.ctypes.data), arr.nbytes


def probe(data):
    """-> JpegInfo when the native decoder takes these file bytes; None when the caller must use PIL (a valid file outside the supported
    subset, or malformed data: PIL then raises as it always has)."""
    arr, p, n = _bytes_ptr(data)
    info = JpegInfo()
    rc = _L.load().smap_jpeg_probe(p, n, C.byref(info))
    if rc == 0:
        return info
    if rc == _L.JPEG_UNSUPPORTED or rc == _L.JPEG_E_DATA:
        return None
    _L.check(rc, "smap_jpeg_probe")


def output_shape(info):
    """(H', W') of the BGR frame: orientations 5-8 swap the stored width and height."""
    return (info.width, info.height) if info.orientation >= 5 else (info.height, info.width)


def decode_coefficients(data, info, out=None, pin=None):
    """Quantised coefficients of every block, int16 [coef_bytes / 2] in page-locked host memory (`out` is reused when it is a large
    enough int16 tensor, pinned when `pin`; pin defaults to "a GPU is present").  -> None when the entropy-coded data is malformed (the
    caller falls back to PIL)."""
    numel = info.coef_bytes // 2
    if pin is None:
        pin = torch.cuda.is_available()
    if out is None or out.dtype != torch.int16 or out.numel() < numel or (pin and not out.is_pinned()):
        out = torch.empty(numel, dtype=torch.int16, pin_memory=pin)
    else:
        out = out.view(-1)[:numel]
    arr, p, n = _bytes_ptr(data)
    rc = _L.load().smap_jpeg_decode_coefficients(p, n, C.byref(info), C.c_void_p(out.data_ptr()))
    if rc == _L.JPEG_E_DATA:
        return None
    _L.check(rc, "smap_jpeg_decode_coefficients")
    return out


JpegScan = _L.JpegScan
_FILE_OFF = (C.sizeof(JpegScan) + 15) & ~15            # a packed frame: the smap_jpeg_scan, then the file bytes 16-byte aligned


def scan_tables(data, info):
    """-> JpegScan: the scan's Huffman tables and MCU layout in the form the device decoder reads; None when the tables are malformed
    (the refusals of decode_coefficients at the marker level)."""
    arr, p, n = _bytes_ptr(data)
    scan = JpegScan()
    rc = _L.load().smap_jpeg_scan_tables(p, n, C.byref(info), C.byref(scan))
    if rc == _L.JPEG_E_DATA:
        return None
    _L.check(rc, "smap_jpeg_scan_tables")
    return scan


def pack_frame(data, info, scan=None, pin=None):
    """What one frame uploads for the device decoder, in ONE page-locked uint8 tensor: the JpegScan of `data` (computed here when
    `scan` is None), then the file bytes.  -> None when scan_tables refuses the file."""
    arr, p, n = _bytes_ptr(data)
    if pin is None:
        pin = torch.cuda.is_available()
    buf = torch.empty(_FILE_OFF + n, dtype=torch.uint8, pin_memory=pin)
    if scan is None:
        rc = _L.load().smap_jpeg_scan_tables(p, n, C.byref(info), C.c_void_p(buf.data_ptr()))
        if rc == _L.JPEG_E_DATA:
            return None
        _L.check(rc, "smap_jpeg_scan_tables")
    else:
        C.memmove(buf.data_ptr(), C.byref(scan), C.sizeof(JpegScan))
    np.copyto(buf.numpy()[_FILE_OFF:], arr.reshape(-1))
    return buf


def frame_bytes(frame):
    """The file bytes of a pack_frame tensor (a numpy view)."""
    return frame.numpy()[_FILE_OFF:]


def huff_groups(info, file_bytes, subseq_bytes=0):
    """Workgroups the device decoder runs for this file = the `rounds` that are provably enough."""
    s = subseq_bytes or _L.JPEG_SUBSEQ_BYTES
    return -(-(-(-(file_bytes - info.scan_offset) // s)) // _L.JPEG_HUFF_LANES)


def decode_coefficients_device(data_or_pinned, info, scan, device, subseq_bytes=0, rounds=0):
    """Huffman decode on the GPU.  data_or_pinned: the file bytes (with `scan` = scan_tables' result, or None to compute it), or a
    pack_frame tensor (`scan` is then not used).  -> (coeffs, status) on `device`, on its current stream, without waiting: coeffs int16
    [coef_bytes / 2] as decode_coefficients writes them, status int32 [1]: 0 = coeffs are bit for bit the host decoder's; non-zero
    (JPEG_DEV_E_DATA | JPEG_DEV_NOT_CONVERGED) = the caller decodes on the host."""
    lib = _L.load()
    device = torch.device(device)
    frame = data_or_pinned if isinstance(data_or_pinned, torch.Tensor) else pack_frame(data_or_pinned, info, scan)
    if frame is None:
        raise ValueError("scan_tables refuses this file: decode it on the host")
    n = frame.numel() - _FILE_OFF
    with torch.cuda.device(device):
        d = frame.to(device, non_blocking=True)
        ws_bytes = int(lib.smap_jpeg_huff_workspace_bytes(C.byref(info), n, subseq_bytes))
        if ws_bytes <= 0:
            raise ValueError("smap_jpeg_huff_workspace_bytes: bad info, file length or subseq_bytes")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        coeffs = torch.empty(info.coef_bytes // 2, dtype=torch.int16, device=device)
        status = torch.empty(1, dtype=torch.int32, device=device)
        st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _L.check(lib.smap_jpeg_decode_coefficients_device(
            C.c_void_p(d.data_ptr() + _FILE_OFF), n, C.byref(info), C.c_void_p(d.data_ptr()), subseq_bytes, rounds,
            C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(coeffs.data_ptr()), C.c_void_p(status.data_ptr()), st),
            "smap_jpeg_decode_coefficients_device")
    return coeffs, status


def reconstruct(coeffs, info, device):
    """coeffs (host or device int16, as decode_coefficients wrote them) -> uint8 [H', W', 3] BGR on `device`, on its current stream."""
    lib = _L.load()
    device = torch.device(device)
    with torch.cuda.device(device):
        d = coeffs.to(device, non_blocking=True)
        planes = torch.empty(int(lib.smap_jpeg_workspace_bytes(C.byref(info))), dtype=torch.uint8, device=device)
        out = torch.empty(output_shape(info) + (3,), dtype=torch.uint8, device=device)
        st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _L.check(lib.smap_jpeg_reconstruct(C.c_void_p(d.data_ptr()), C.byref(info), C.c_void_p(planes.data_ptr()),
                                           C.c_void_p(out.data_ptr()), st), "smap_jpeg_reconstruct")
    return out


def decode(path_or_bytes, device, huffman="host"):
    """A file (path or bytes) -> uint8 [H', W', 3] BGR on `device`: the native path when it takes the file, PIL otherwise (the same
    tensor either way).  huffman="device": the entropy decode runs on the GPU too; a frame it does not vouch for is decoded on the host."""
    if huffman not in ("host", "device"):
        raise ValueError('huffman: "host" or "device"')
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    info = probe(data)
    coeffs = None
    if info is not None and huffman == "device":
        frame = pack_frame(data, info)
        if frame is not None:
            coeffs, status = decode_coefficients_device(frame, info, None, device)
            if status.item() != 0:
                coeffs = None
    if info is not None and coeffs is None:
        coeffs = decode_coefficients(data, info)
    if coeffs is not None:
        return reconstruct(coeffs, info, device)
    import io
    from dataset.decode import read_bgr
    img = read_bgr(io.BytesIO(data))
    return torch.from_numpy(np.array(img)).to(device)               # (a copy: PIL's frame is a read-only view of its bytes)
