"""JPEG decode split between the host and the GPU (include/smap_hip.h "JPEG decode", DESIGN.md "JPEG decode").

    info = probe(data)                        # marker parse: a JpegInfo, or None = decode this file with PIL
    coeffs = decode_coefficients(data, info)  # Huffman decode on the host (native, no interpreter lock) -> page-locked int16
    bgr = reconstruct(coeffs, info, device)   # dequantise + IDCT + chroma upsampling + YCbCr->BGR + EXIF orientation, two HIP launches

`bgr` is a uint8 [H', W', 3] tensor on the device, bit for bit what dataset.decode.read_bgr (PIL on libjpeg-turbo, EXIF transposed)
returns for the same file.  `decode` does all three, with PIL for whatever the native decoder does not take."""
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


def decode(path_or_bytes, device):
    """A file (path or bytes) -> uint8 [H', W', 3] BGR on `device`: the native path when it takes the file, PIL otherwise (the same
    tensor either way)."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    info = probe(data)
    coeffs = decode_coefficients(data, info) if info is not None else None
    if coeffs is not None:
        return reconstruct(coeffs, info, device)
    import io
    from dataset.decode import read_bgr
    img = read_bgr(io.BytesIO(data))
    return torch.from_numpy(np.array(img)).to(device)               # (a copy: PIL's frame is a read-only view of its bytes)
