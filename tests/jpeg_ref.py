"""numpy restatement of the GPU half of the JPEG decode (smap_amd/csrc/jpeg.hip: dequantise, ISLOW IDCT, fancy chroma upsampling,
YCbCr -> BGR, EXIF orientation), written from libjpeg's published algorithm, and the Pillow-encoded fixtures the JPEG tests share.

Nothing here is read from a file: every fixture is encoded at test time by Pillow's own encoder."""
import io

import numpy as np


def _butterfly(x):
    """jidctint.c's 1-D ISLOW butterfly (both passes), before the descale; x: list of 8 ints."""
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    tmp0, tmp1 = (x[0] + x[4]) << 13, (x[0] - x[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0 += z1 + z3
    tmp1 += z2 + z4
    tmp2 += z2 + z3
    tmp3 += z1 + z4
    return [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]


# the butterfly is linear in integers: its matrix, column j = the image of the j-th unit vector
IDCT = np.array([_butterfly([int(i == j) for i in range(8)]) for j in range(8)], np.int64).T


def planes(coeffs, info):
    """-> list of uint8 component planes [blocks_h * 8, blocks_w * 8] (libjpeg's jpeg_idct_islow on every block)."""
    out = []
    for c in range(info.ncomp):
        bw, bh = info.blocks_w[c], info.blocks_h[c]
        o = info.coef_offset[c] // 2
        blk = np.asarray(coeffs[o:o + bw * bh * 64], np.int64).reshape(bh, bw, 8, 8)
        a = blk * np.array(info.quant[c], np.int64).reshape(8, 8)
        ws = (np.einsum("rv,yxvc->yxrc", IDCT, a) + (1 << 10)) >> 11                    # columns: CONST_BITS - PASS1_BITS
        px = (np.einsum("cu,yxru->yxrc", IDCT, ws) + (1 << 17)) >> 18                  # rows: CONST_BITS + PASS1_BITS + 3
        px = np.clip(px + 128, 0, 255).astype(np.uint8)
        out.append(px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return out


def _h_fancy(c, cw, even_round, odd_round, shift, edge):
    """libjpeg's horizontal triangle filter over the cw real columns of rows c (ints) -> 2 * cw columns."""
    c = c[:, :cw]
    out = np.empty((c.shape[0], 2 * cw), np.int64)
    prev = np.concatenate([c[:, :1], c[:, :-1]], 1)
    nxt = np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out[:, 0::2] = (3 * c + prev + even_round) >> shift
    out[:, 1::2] = (3 * c + nxt + odd_round) >> shift
    out[:, 0] = edge(c[:, 0], even_round)
    out[:, -1] = edge(c[:, -1], odd_round)
    return out


def upsample(plane, info, h, w):
    """A chroma plane at full resolution [h, w] (jdsample.c: h2v1 / h2v2 fancy upsampling; replication when at most 2 samples wide)."""
    hs, vs = info.h_samp[0], info.v_samp[0]
    cw, ch = -(-w // hs), -(-h // vs)
    p = plane.astype(np.int64)
    if hs == 1:
        return p[:h, :w]
    if cw <= 2:
        return np.repeat(np.repeat(p[:ch, :cw], vs, 0), 2, 1)[:h, :w]
    if vs == 1:                                                                      # h2v1
        return _h_fancy(p[:h], cw, 1, 2, 2, lambda v, r: v)[:, :w]
    rows = np.arange(h)
    near = rows >> 1
    far = np.clip(np.where(rows & 1, near + 1, near - 1), 0, ch - 1)
    colsum = 3 * p[near] + p[far]                                                    # h2v2: the vertical step first
    return _h_fancy(colsum, cw, 8, 7, 4, lambda v, r: (4 * v + r) >> 4)[:, :w]


def orient(img, o):
    """PIL's ImageOps.exif_transpose on an HxWxC array."""
    return {1: lambda a: a, 2: lambda a: a[:, ::-1], 3: lambda a: a[::-1, ::-1], 4: lambda a: a[::-1],
            5: lambda a: a.transpose(1, 0, 2), 6: lambda a: np.rot90(a, -1), 7: lambda a: a.transpose(1, 0, 2)[::-1, ::-1],
            8: lambda a: np.rot90(a, 1)}[o](img)


def reconstruct(coeffs, info):
    """coefficients (smap_jpeg_decode_coefficients) + info -> uint8 [H', W', 3] BGR, orientation applied."""
    h, w = info.height, info.width
    ps = planes(coeffs, info)
    y = ps[0][:h, :w].astype(np.int64)
    if info.ncomp == 1:
        bgr = np.stack([y, y, y], -1)
    else:
        x = upsample(ps[2], info, h, w) - 128                                        # Cr
        xb = upsample(ps[1], info, h, w) - 128                                       # Cb
        r = y + ((91881 * x + 32768) >> 16)
        g = y + ((-46802 * x - 22554 * xb + 32768) >> 16)
        b = y + ((116130 * xb + 32768) >> 16)
        bgr = np.stack([b, g, r], -1)
    return np.ascontiguousarray(orient(np.clip(bgr, 0, 255).astype(np.uint8), info.orientation))


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------

def content(kind, h, w, seed=0):
    """uint8 [h, w, 3] RGB: 'smooth' gradients, 'noise', or 'primaries' (saturated colour blocks with hard edges)."""
    rng = np.random.default_rng(seed + 7 * h + 13 * w)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "smooth":
        a = 127.5 + 127.5 * np.sin(xx / max(w, 2) * 3.1 + yy / max(h, 2) * 1.7)
        b = 255.0 * xx / max(w - 1, 1)
        c = 255.0 * yy / max(h - 1, 1)
        return np.stack([a, b, c], -1).round().astype(np.uint8)
    cols = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [0, 0, 0], [255, 255, 255]],
                    np.uint8)
    idx = ((xx // 5).astype(int) + 3 * (yy // 3).astype(int)) % len(cols)
    return cols[idx]


def encode(rgb, quality=75, subsampling="4:2:0", grey=False, orientation=None, **kw):
    """Pillow-encoded JPEG bytes of an RGB array (grey: mode L; orientation: an EXIF IFD0 with tag 0x0112)."""
    from PIL import Image
    im = Image.fromarray(rgb, "RGB")
    if grey:
        im = im.convert("L")
    args = dict(quality=quality, **kw)
    if not grey:
        args["subsampling"] = subsampling
    if orientation is not None:
        ex = Image.Exif()
        ex[0x0112] = orientation
        args["exif"] = ex.tobytes()
    buf = io.BytesIO()
    im.save(buf, "JPEG", **args)
    return buf.getvalue()


def pil_bgr(data):
    """What the loader hands the network for these bytes (dataset.decode.read_bgr)."""
    from dataset.decode import read_bgr
    return np.asarray(read_bgr(io.BytesIO(data)))


SIZES_SMALL = [(1, 1), (1, 17), (17, 1), (5, 2), (6, 3), (9, 4), (3, 5), (7, 9), (8, 8), (15, 17), (16, 16), (33, 65)]   # widths 1-4: chroma <= 2 wide
SUBSAMPLINGS = ["4:4:4", "4:2:2", "4:2:0", "grey"]
QUALITIES = [1, 50, 75, 95, 100]
KINDS = ["smooth", "noise", "primaries"]


def fixture_matrix(large=True):
    """-> list of (name, JPEG bytes).  Every size x subsampling x quality at the small sizes (content, optimize and the restart
    markers rotating through the combinations); the large sizes thinned to a few combinations each; all 8 orientations."""
    out = []
    i = 0
    for (h, w) in SIZES_SMALL:
        for ss in SUBSAMPLINGS:
            for q in QUALITIES:
                kind = KINDS[i % 3]
                kw = dict(optimize=bool(i % 2))
                if i % 5 == 1:
                    kw["restart_marker_blocks"] = 1 + i % 3
                elif i % 5 == 3:
                    kw["restart_marker_rows"] = 1
                out.append((f"{h}x{w}_{ss}_q{q}_{kind}_{kw}", encode(content(kind, h, w, i), q, ss, grey=ss == "grey", **kw)))
                i += 1
    large_sizes = [(512, 832), (1081, 1921)] if large else [(512, 832)]
    for (h, w) in large_sizes:
        for j, (ss, q, kind, kw) in enumerate([("4:2:0", 75, "smooth", {}), ("4:2:2", 95, "noise", dict(optimize=True)),
                                               ("4:4:4", 50, "primaries", dict(restart_marker_rows=2)),
                                               ("grey", 100, "smooth", dict(restart_marker_blocks=7)),
                                               ("4:2:0", 1, "primaries", dict(restart_marker_blocks=5, optimize=True))]):
            out.append((f"{h}x{w}_{ss}_q{q}_{kind}_{kw}", encode(content(kind, h, w, j), q, ss, grey=ss == "grey", **kw)))
    for o in range(1, 9):
        for (h, w), ss in (((37, 61), "4:2:0"), ((20, 33), "4:2:2"), ((9, 14), "4:4:4"), ((11, 6), "grey")):
            out.append((f"exif{o}_{h}x{w}_{ss}", encode(content("smooth", h, w, o), 90, ss, grey=ss == "grey", orientation=o)))
    return out
