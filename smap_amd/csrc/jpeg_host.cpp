// jpeg_host.cpp -- the host half of the JPEG decode (include/smap_hip.h "JPEG decode"): marker parsing and Huffman entropy decoding
// into quantised coefficients.  The per-pixel half (dequantisation, IDCT, upsampling, colour, orientation) is csrc/jpeg.hip.
// smap_jpeg_scan_tables hands the scan's decoding tables to the Huffman decode on the device (csrc/jpeg_huff.h, csrc/jpeg_huff.hip).
//
// Plain C++ with no HIP include, so that a test can build it alone for the CPU under AddressSanitizer (tests/c/jpeg_asan_main.cpp).
// No allocation, no global state: every call keeps its tables on its own stack, and the entry points are called from many pool threads
// at once (ctypes releases the interpreter lock).  Every byte read is bounds-checked against n; anything the parser does not fully
// understand is SMAP_JPEG_UNSUPPORTED (the caller decodes with PIL), anything malformed SMAP_JPEG_E_DATA -- it never guesses.
#include <stdint.h>
#include <string.h>

#include "smap_hip.h"

namespace {

constexpr int kLook = 9;                     // lookahead bits: codes up to 9 bits in one table probe, longer ones on the slow path
constexpr int kOk = 0, kUnsup = SMAP_JPEG_UNSUPPORTED, kBad = SMAP_JPEG_E_DATA;

// zig-zag index -> natural (row-major) index
constexpr uint8_t kNatural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff : smap_jpeg_huff {               // the decoding tables in the form the device kernels also read (include/smap_hip.h)
    bool defined;
};
static_assert(sizeof(((smap_jpeg_huff*)0)->look) == sizeof(uint16_t) << kLook, "smap_jpeg_huff::look is the kLook-bit lookahead");

struct Parsed {
    smap_jpeg_info info;
    Huff dc[4], ac[4];
    int comp_dc[3], comp_ac[3];
};

inline uint32_t be16(const uint8_t* p) { return (uint32_t(p[0]) << 8) | p[1]; }

// DHT table -> decoding tables (jdhuff.c jpeg_make_d_derived_tbl: canonical codes, an over-long code set is an error)
int build_huff(const uint8_t* counts, const uint8_t* vals, int nvals, bool is_dc, Huff* h) {
    memset(h->look, 0, sizeof(h->look));
    memset(h->vals, 0, sizeof(h->vals));                         // (the tables are also handed out whole: smap_jpeg_scan_tables)
    memcpy(h->vals, vals, size_t(nvals));
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        int cnt = counts[l - 1];
        h->valoff[l] = k - int(code);
        for (int i = 0; i < cnt; ++i, ++k, ++code) {
            if (code >= (1u << l)) return kBad;                   // more codes than fit this length
            if (l <= kLook) {
                int shift = kLook - l;
                for (uint32_t j = code << shift; j < ((code + 1) << shift); ++j) h->look[j] = uint16_t((l << 8) | vals[k]);
            }
        }
        h->maxcode[l] = cnt ? int32_t(code) - 1 : -1;
        code <<= 1;
    }
    h->maxcode[17] = 0x7fffffff;
    if (is_dc)
        for (int i = 0; i < nvals; ++i)
            if (vals[i] > 15) return kBad;                          // jdhuff.c: a DC category above 15 is a bad table
    h->defined = true;
    return kOk;
}

// EXIF orientation from the TIFF structure of an APP1 "Exif\0\0" segment (s: after the 6-byte prefix): tag 0x0112 of IFD0, as PIL's
// Image.getexif() / ImageOps.exif_transpose read it.  Anything unusual is "unsupported", never a guess.
int exif_orientation(const uint8_t* s, size_t len, int32_t* orient) {
    if (len < 8) return kUnsup;
    bool le;
    if (s[0] == 'I' && s[1] == 'I') le = true;
    else if (s[0] == 'M' && s[1] == 'M') le = false;
    else return kUnsup;
    auto u16 = [&](size_t o) { return le ? uint32_t(s[o]) | (uint32_t(s[o + 1]) << 8) : (uint32_t(s[o]) << 8) | s[o + 1]; };
    auto u32 = [&](size_t o) { return le ? u16(o) | (u16(o + 2) << 16) : (u16(o) << 16) | u16(o + 2); };
    if (u16(2) != 42) return kUnsup;
    size_t ifd = u32(4);
    if (ifd < 8 || ifd > len || len - ifd < 2) return kUnsup;
    size_t cnt = u16(ifd);
    if ((len - ifd - 2) / 12 < cnt) return kUnsup;
    bool found = false;
    *orient = 1;
    for (size_t i = 0; i < cnt; ++i) {
        size_t e = ifd + 2 + 12 * i;
        if (u16(e) != 0x0112) continue;
        if (found || u16(e + 2) != 3 || u32(e + 4) != 1) return kUnsup;   // repeated, or not one SHORT
        found = true;
        uint32_t v = u16(e + 8);
        *orient = (v >= 1 && v <= 8) ? int32_t(v) : 1;                   // exif_transpose: any other value transposes nothing
    }
    return kOk;
}

// Markers from SOI to the first SOS (jdmarker.c's subset).  tables = false: the Huffman tables are only checked, not built.
int parse(const uint8_t* d, size_t n, Parsed* p, bool tables) {
    smap_jpeg_info& info = p->info;
    memset(&info, 0, sizeof(info));
    info.orientation = 1;
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return kBad;
    for (int i = 0; i < 4; ++i) p->dc[i].defined = p->ac[i].defined = false;
    uint16_t qt[4][64];
    bool qdef[4] = {false, false, false, false};
    bool sof = false, jfif = false, adobe = false, exif = false;
    int adobe_transform = -1, nf = 0;
    int cid[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
    size_t pos = 2;
    for (;;) {
        if (pos >= n || d[pos] != 0xFF) return kBad;               // (libjpeg skips garbage between markers with a warning)
        while (pos < n && d[pos] == 0xFF) ++pos;                   // fill bytes
        if (pos >= n) return kBad;
        uint32_t m = d[pos++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return kBad;   // no parameters here: stuffing, TEM, RSTn, SOI, EOI
        if (n - pos < 2) return kBad;
        uint32_t L = be16(d + pos);
        if (L < 2 || n - pos < L) return kBad;
        const uint8_t* s = d + pos + 2;
        size_t len = L - 2;
        pos += L;
        if (m == 0xC0 || m == 0xC1) {                              // baseline / extended sequential, Huffman
            if (sof || len < 6) return kBad;
            sof = true;
            if (s[0] != 8) return kUnsup;                          // 12-bit
            info.height = int32_t(be16(s + 1));
            info.width = int32_t(be16(s + 3));
            nf = s[5];
            if (len != size_t(6 + 3 * nf) || nf == 0 || info.width == 0) return kBad;
            if (info.height == 0 || (nf != 1 && nf != 3)) return kUnsup;   // DNL-defined height; CMYK / YCCK / 2 components
            for (int c = 0; c < nf && c < 3; ++c) {
                const uint8_t* q = s + 6 + 3 * c;
                cid[c] = q[0];
                info.h_samp[c] = q[1] >> 4;
                info.v_samp[c] = q[1] & 15;
                ctq[c] = q[2];
                if (info.h_samp[c] < 1 || info.h_samp[c] > 4 || info.v_samp[c] < 1 || info.v_samp[c] > 4 || q[2] > 3) return kBad;
            }
        } else if ((m >= 0xC2 && m <= 0xCF && m != 0xC4) || m == 0xDC || m == 0xDE || m == 0xDF || (m >= 0xF0 && m <= 0xFD)) {
            return kUnsup;                                         // progressive, lossless, hierarchical, arithmetic (DAC), DNL, JPEG-LS ...
        } else if (m == 0xC4) {                                    // DHT
            size_t o = 0;
            while (o < len) {
                if (len - o < 17) return kBad;
                int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) return kBad;
                int total = 0;
                for (int i = 0; i < 16; ++i) total += s[o + 1 + i];
                if (total > 256 || len - o - 17 < size_t(total)) return kBad;
                Huff* h = tc ? &p->ac[th] : &p->dc[th];
                if (tables) {
                    if (build_huff(s + o + 1, s + o + 17, total, tc == 0, h) != kOk) return kBad;
                } else {
                    uint32_t code = 0;                              // (probe: the same checks, no tables built)
                    for (int l = 1; l <= 16; ++l) {
                        code += s[o + l];
                        if (code > (1u << l)) return kBad;
                        code <<= 1;
                    }
                    if (tc == 0)
                        for (int i = 0; i < total; ++i)
                            if (s[o + 17 + i] > 15) return kBad;
                    h->defined = true;
                }
                o += 17 + size_t(total);
            }
        } else if (m == 0xDB) {                                    // DQT, 8- or 16-bit entries
            size_t o = 0;
            while (o < len) {
                int pq = s[o] >> 4, tq = s[o] & 15;
                if (pq > 1 || tq > 3) return kBad;
                size_t need = 1 + 64 * size_t(pq + 1);
                if (len - o < need) return kBad;
                for (int i = 0; i < 64; ++i)
                    qt[tq][kNatural[i]] = uint16_t(pq ? be16(s + o + 1 + 2 * i) : s[o + 1 + i]);
                qdef[tq] = true;
                o += need;
            }
        } else if (m == 0xDD) {                                    // DRI
            if (len != 2) return kBad;
            info.restart_interval = int32_t(be16(s));
        } else if (m == 0xE0) {
            if (len >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xE1) {                                    // APP1: EXIF is read; XMP (PIL's fallback orientation source) or anything else is not
            if (exif || len < 6 || memcmp(s, "Exif\0\0", 6) != 0) return kUnsup;
            exif = true;
            if (exif_orientation(s + 6, len - 6, &info.orientation) != kOk) return kUnsup;
        } else if (m == 0xEE) {
            if (len >= 12 && memcmp(s, "Adobe", 5) == 0) {
                adobe = true;
                adobe_transform = s[11];
            }
        } else if ((m >= 0xE2 && m <= 0xEF) || m == 0xFE) {
            // other application segments, comments: nothing PIL's pixels depend on
        } else if (m == 0xDA) {                                    // SOS
            if (!sof || len < 1) return kBad;
            int ns = s[0];
            if (len != size_t(4 + 2 * ns) || ns < 1 || ns > 4) return kBad;
            if (ns != nf) return kUnsup;                           // multi-scan (non-interleaved) sequential
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != cid[c]) return kUnsup;         // scan order other than the frame's
                int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (td > 3 || ta > 3 || !p->dc[td].defined || !p->ac[ta].defined) return kBad;
                p->comp_dc[c] = td;
                p->comp_ac[c] = ta;
            }
            const uint8_t* t = s + 1 + 2 * ns;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0) return kBad;  // Ss, Se, Ah/Al of a sequential scan
            if (nf == 3) {
                // jdapimin.c default_decompress_parms: a JFIF marker means YCbCr, else the Adobe transform, else the component ids
                if (!jfif && ((adobe && adobe_transform != 1) || (!adobe && cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B'))) return kUnsup;
                bool luma_ok = info.v_samp[0] <= info.h_samp[0] && info.h_samp[0] <= 2 && info.v_samp[0] <= 2;   // 1x1, 2x1, 2x2
                for (int c = 1; c < 3; ++c)
                    if (info.h_samp[c] != 1 || info.v_samp[c] != 1) luma_ok = false;
                if (!luma_ok) return kUnsup;                       // 4:1:1, 4:4:0, chroma above luma ...
            } else {
                info.h_samp[0] = info.v_samp[0] = 1;                // one component: one non-interleaved scan of whole blocks
            }
            if (int64_t(info.width) * info.height > 89478485) return kUnsup;   // PIL's decompression-bomb threshold: its warning / error stays its own
            info.ncomp = nf;
            int hmax = info.h_samp[0], vmax = info.v_samp[0];
            int mcux = (info.width + 8 * hmax - 1) / (8 * hmax), mcuy = (info.height + 8 * vmax - 1) / (8 * vmax);
            int64_t off = 0;
            for (int c = 0; c < nf; ++c) {
                if (!qdef[ctq[c]]) return kBad;
                memcpy(info.quant[c], qt[ctq[c]], sizeof(info.quant[c]));
                info.blocks_w[c] = mcux * info.h_samp[c];
                info.blocks_h[c] = mcuy * info.v_samp[c];
                info.coef_offset[c] = off;
                off += int64_t(info.blocks_w[c]) * info.blocks_h[c] * 64 * 2;
            }
            info.coef_bytes = off;
            info.scan_offset = int64_t(pos);
            return kOk;
        } else {
            return kBad;                                           // reserved marker codes
        }
    }
}

// Bit reader over the entropy-coded segment: a 64-bit buffer, MSB first, refilled a byte at a time with the 0xFF00 stuffing removed.
// At a marker (or the end of the file) it appends zero bytes and counts them in `pad`: reading into them is an error.
struct Bits {
    const uint8_t* d;
    size_t n, pos;
    uint64_t buf;
    int cnt, pad;
    bool marker;

    void reset(size_t at) { pos = at; buf = 0; cnt = 0; pad = 0; marker = false; }
    inline void refill() {
        if (!marker && n - pos >= 8) {                             // fast path: whole bytes with no 0xFF among them
            while (cnt <= 56) {
                uint32_t b = d[pos];
                if (b == 0xFF) break;
                buf |= uint64_t(b) << (56 - cnt);
                cnt += 8;
                ++pos;
                if (n - pos < 2) break;
            }
        }
        while (cnt <= 56) {
            uint32_t b = 0;
            if (marker) {
                pad += 8;
            } else if (pos >= n) {
                marker = true;
                pad += 8;
            } else {
                b = d[pos];
                if (b == 0xFF) {
                    if (n - pos >= 2 && d[pos + 1] == 0x00) {
                        pos += 2;
                    } else {
                        marker = true;                             // pos stays on the marker's 0xFF
                        b = 0;
                        pad += 8;
                    }
                } else {
                    ++pos;
                }
            }
            buf |= uint64_t(b) << (56 - cnt);
            cnt += 8;
        }
    }
    inline uint32_t peek(int k) const { return uint32_t(buf >> (64 - k)); }
    inline void skip(int k) { buf <<= k; cnt -= k; }
    inline bool overran() const { return cnt < pad; }
};

inline int decode_sym(Bits& b, const Huff& h) {
    uint32_t e = h.look[b.peek(kLook)];
    if (e) {
        b.skip(int(e >> 8));
        return int(e & 0xFF);
    }
    for (int l = kLook + 1; l <= 16; ++l) {
        int32_t code = int32_t(b.peek(l));
        if (code <= h.maxcode[l]) {
            b.skip(l);
            return h.vals[code + h.valoff[l]];
        }
    }
    return -1;
}

inline int32_t receive_extend(Bits& b, int s) {
    int32_t r = int32_t(b.peek(s));
    b.skip(s);
    return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
}

// One block (jdhuff.c decode_mcu): DC difference + run/size coded AC terms, stored quantised in natural order.
inline int decode_block(Bits& b, const Huff& dc, const Huff& ac, int32_t* pred, int16_t* out) {
    memset(out, 0, 64 * sizeof(int16_t));
    if (b.cnt < 32) b.refill();
    int s = decode_sym(b, dc);
    if (s < 0) return kBad;
    if (s) {
        if (b.cnt < 32) b.refill();
        *pred += receive_extend(b, s);
    }
    out[0] = int16_t(*pred);
    for (int k = 1; k < 64; ++k) {
        if (b.cnt < 32) b.refill();
        int rs = decode_sym(b, ac);
        if (rs < 0) return kBad;
        int r = rs >> 4;
        s = rs & 15;
        if (s) {
            k += r;
            if (k > 63) return kBad;                               // (libjpeg writes such a term to position 63 of a corrupt block)
            out[kNatural[k]] = int16_t(receive_extend(b, s));
        } else {
            if (r != 15) break;                                    // EOB
            k += 15;                                               // ZRL
        }
    }
    return b.overran() ? kBad : kOk;
}

// End of an interval or of the scan: drop the byte's fill bits; what follows must be the marker, with no entropy-coded data left.
// -> the marker code (pos moved past it), or -1.
int take_marker(Bits& b) {
    b.skip(b.cnt & 7);
    if (b.cnt != b.pad) return -1;                                 // whole bytes of data before the marker
    const uint8_t* d = b.d;
    size_t pos = b.pos;
    if (pos >= b.n || d[pos] != 0xFF) return -1;
    while (pos < b.n && d[pos] == 0xFF) ++pos;
    if (pos >= b.n || d[pos] == 0x00) return -1;
    int m = d[pos];
    b.reset(pos + 1);
    return m;
}

}  // namespace

extern "C" {

int smap_sizeof_jpeg_info(void) { return int(sizeof(smap_jpeg_info)); }

int smap_jpeg_probe(const uint8_t* data, size_t n, smap_jpeg_info* info) {
    if (!data || !info) return SMAP_E_ARG;
    Parsed p;
    int rc = parse(data, n, &p, false);
    if (rc == kOk) *info = p.info;
    return rc;
}

int smap_jpeg_decode_coefficients(const uint8_t* data, size_t n, const smap_jpeg_info* info, int16_t* coeffs) {
    if (!data || !info || !coeffs) return SMAP_E_ARG;
    Parsed p;
    int rc = parse(data, n, &p, true);
    if (rc != kOk) return rc;
    if (memcmp(&p.info, info, sizeof(smap_jpeg_info)) != 0) return SMAP_E_ARG;   // not this file's info: the caller's buffer is sized by it
    const smap_jpeg_info& I = p.info;
    Bits b;
    b.d = data;
    b.n = n;
    b.reset(size_t(I.scan_offset));
    int32_t pred[3] = {0, 0, 0};
    const int nc = I.ncomp;
    const int mcux = I.blocks_w[0] / I.h_samp[0], mcuy = I.blocks_h[0] / I.v_samp[0];
    const int ri = I.restart_interval;
    int rst = 0;
    int16_t* plane[3];
    for (int c = 0; c < nc; ++c) plane[c] = coeffs + I.coef_offset[c] / 2;
    int64_t mcu = 0;
    for (int my = 0; my < mcuy; ++my) {
        for (int mx = 0; mx < mcux; ++mx, ++mcu) {
            if (ri && mcu && mcu % ri == 0) {                      // restart: byte-align, RST0..7 in sequence, DC predictors to 0
                if (take_marker(b) != 0xD0 + (rst & 7)) return kBad;
                ++rst;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < nc; ++c) {
                const Huff& dc = p.dc[p.comp_dc[c]];
                const Huff& ac = p.ac[p.comp_ac[c]];
                const int hs = I.h_samp[c], vs = I.v_samp[c], bw = I.blocks_w[c];
                for (int v = 0; v < vs; ++v)
                    for (int h = 0; h < hs; ++h) {
                        int64_t blk = int64_t(my * vs + v) * bw + (mx * hs + h);
                        if (decode_block(b, dc, ac, &pred[c], plane[c] + blk * 64) != kOk) return kBad;
                    }
            }
        }
    }
    return take_marker(b) == 0xD9 ? kOk : kBad;                    // EOI right after the last MCU
}

int64_t smap_jpeg_workspace_bytes(const smap_jpeg_info* info) { return info ? info->coef_bytes / 2 : 0; }

int smap_sizeof_jpeg_scan(void) { return int(sizeof(smap_jpeg_scan)); }

int smap_jpeg_scan_tables(const uint8_t* data, size_t n, const smap_jpeg_info* info, smap_jpeg_scan* scan) {
    if (!data || !info || !scan) return SMAP_E_ARG;
    Parsed p;
    int rc = parse(data, n, &p, true);
    if (rc != kOk) return rc;
    if (memcmp(&p.info, info, sizeof(smap_jpeg_info)) != 0) return SMAP_E_ARG;
    const smap_jpeg_info& I = p.info;
    memset(scan, 0, sizeof(*scan));
    scan->ncomp = I.ncomp;
    int nb = 0;
    for (int c = 0; c < I.ncomp; ++c) {
        scan->table[2 * c] = p.dc[p.comp_dc[c]];                   // (slices the `defined` flag off)
        scan->table[2 * c + 1] = p.ac[p.comp_ac[c]];
        for (int v = 0; v < I.v_samp[c]; ++v)
            for (int h = 0; h < I.h_samp[c]; ++h, ++nb) {
                if (nb >= SMAP_JPEG_MAX_MCU_BLOCKS) return SMAP_E_ARG;   // (parse admits 1x1, 2x1, 2x2 luma only: cannot happen)
                scan->block_comp[nb] = c;
                scan->block_v[nb] = v;
                scan->block_h[nb] = h;
            }
    }
    scan->blocks_per_mcu = nb;
    scan->restart_interval = I.restart_interval;
    scan->scan_offset = I.scan_offset;
    scan->file_bytes = int64_t(n);
    scan->total_blocks = I.coef_bytes / 128;
    return kOk;
}

}  // extern "C"
