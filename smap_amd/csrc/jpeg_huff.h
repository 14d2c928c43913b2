// jpeg_huff.h -- the Huffman decode of a baseline JPEG scan as a function of ONE SUBSEQUENCE of the entropy-coded segment: the single
// statement of the algorithm behind smap_jpeg_decode_coefficients_device (include/smap_hip.h, DESIGN.md "Huffman decode on the GPU").
// The kernels of csrc/jpeg_huff.hip run it one subsequence per lane; tests/c/jpeg_huff_twin_main.cpp includes it as plain host C++ and
// runs the same phases with loops in place of lanes and workgroups.  Inline functions only: no kernels, no __shared__ objects.
//
// A decoder STATE is (bit position in the raw file, block of the MCU, zig-zag index), taken between two symbols (a symbol = a Huffman
// code and its extra bits).  Two decoders in the same state have the same future.  Subsequence i owns the symbols that START in its
// bytes [scan_offset + i * S, scan_offset + (i + 1) * S); decode_subseq maps an entry state to the first state at or past the end.
//   decode_subseq<false>: SPECULATIVE.  It does not know its block number, so it takes a restart marker where it looks like one (MCU
//     boundary, only fill bits left) and, out of step, resynchronises at one; errors end in a guess.  Its result is never trusted.
//   decode_subseq<true>: EXACT.  It knows its block number, does what smap_jpeg_decode_coefficients does (csrc/jpeg_host.cpp:
//     decode_block, take_marker, the same checks) and writes the coefficients; any surprise is SMAP_JPEG_DEV_E_DATA.
#pragma once
#include <stdint.h>

#include "smap_hip.h"

#ifdef __HIPCC__
#define SMAP_HD __host__ __device__ inline
#else
#define SMAP_HD inline
#endif

namespace smap_huff {

constexpr int kLook = 9;                     // smap_jpeg_huff::look
constexpr int kLanes = 256;                  // subsequences per workgroup
constexpr int kChunk = 1024;                 // elements per workgroup of the prefix sums
constexpr int kMaxFill = 64;                 // 0xFF fill bytes accepted before a marker (the host decoder accepts any number: more is refused)
constexpr uint64_t kEnd = ~0ull;             // the state after EOI (and after an error of the exact pass)
constexpr int kEData = SMAP_JPEG_DEV_E_DATA, kNotConv = SMAP_JPEG_DEV_NOT_CONVERGED;

// What the kernels need of smap_jpeg_info and the file, by value.  geo_init refuses an info whose planes do not fit its own MCU grid.
struct Geo {
    int32_t ncomp, bpm, ri, mcux;            // components, blocks per MCU, restart interval (MCUs), MCUs per row
    int32_t total;                           // blocks of the scan
    uint32_t scan_off, n;                    // first byte of the entropy-coded segment, file length
    int32_t S, nsub, ngroups;                // subsequence bytes, subsequences, workgroups of kLanes
    int32_t comp[SMAP_JPEG_MAX_MCU_BLOCKS], bv[SMAP_JPEG_MAX_MCU_BLOCKS], bh[SMAP_JPEG_MAX_MCU_BLOCKS];
    int32_t hs[3], vs[3], bw[3];
    int32_t first_j[3];                      // first block of the MCU that belongs to the component
    int32_t first_elem[3];                   // first DC difference of the component in the scan-ordered array
    int64_t plane[3];                        // int16 index of the component's coefficient plane
};

inline bool geo_init(Geo* g, const smap_jpeg_info& I, size_t file_bytes, int subseq_bytes) {
    const int S = subseq_bytes ? subseq_bytes : SMAP_JPEG_SUBSEQ_BYTES;
    if (S < 8 || S > 128 || (S & 3)) return false;
    if (I.width <= 0 || I.height <= 0 || (I.ncomp != 1 && I.ncomp != 3) || I.restart_interval < 0) return false;
    const int hmax = I.h_samp[0], vmax = I.v_samp[0];
    if (!((hmax == 1 && vmax == 1) || (hmax == 2 && vmax == 1) || (hmax == 2 && vmax == 2))) return false;
    if (I.ncomp == 1 && hmax != 1) return false;
    if (file_bytes >= (size_t(1) << 28) || I.scan_offset < 2 || uint64_t(I.scan_offset) >= file_bytes) return false;   // bit positions are 32-bit
    const int64_t mcux = (I.width + 8 * hmax - 1) / (8 * hmax), mcuy = (I.height + 8 * vmax - 1) / (8 * vmax);
    int64_t off = 0, elem = 0;
    int nb = 0;
    for (int c = 0; c < I.ncomp; ++c) {
        const int hs = c ? 1 : hmax, vs = c ? 1 : vmax;
        if (I.h_samp[c] != hs || I.v_samp[c] != vs || I.blocks_w[c] != mcux * hs || I.blocks_h[c] != mcuy * vs || I.coef_offset[c] != off)
            return false;
        g->hs[c] = hs;
        g->vs[c] = vs;
        g->bw[c] = I.blocks_w[c];
        g->first_j[c] = nb;
        g->first_elem[c] = int32_t(elem);
        g->plane[c] = off / 2;
        for (int v = 0; v < vs; ++v)
            for (int h = 0; h < hs; ++h, ++nb) {
                g->comp[nb] = c;
                g->bv[nb] = v;
                g->bh[nb] = h;
            }
        off += int64_t(I.blocks_w[c]) * I.blocks_h[c] * 128;
        elem += int64_t(I.blocks_w[c]) * I.blocks_h[c];
        if (elem > (int64_t(1) << 28)) return false;
    }
    if (off != I.coef_bytes) return false;
    for (int c = I.ncomp; c < 3; ++c) {
        g->hs[c] = g->vs[c] = 1;
        g->bw[c] = 0;
        g->first_j[c] = nb;
        g->first_elem[c] = int32_t(elem);
        g->plane[c] = 0;
    }
    for (int j = nb; j < SMAP_JPEG_MAX_MCU_BLOCKS; ++j) g->comp[j] = g->bv[j] = g->bh[j] = 0;
    g->ncomp = I.ncomp;
    g->bpm = nb;
    g->ri = I.restart_interval;
    g->mcux = int32_t(mcux);
    g->total = int32_t(elem);
    g->scan_off = uint32_t(I.scan_offset);
    g->n = uint32_t(file_bytes);
    g->S = S;
    g->nsub = int32_t((g->n - g->scan_off + uint32_t(S) - 1) / uint32_t(S));
    g->ngroups = (g->nsub + kLanes - 1) / kLanes;
    return true;
}

// Workspace of one frame: the arrays the launches hand each other.  All offsets are multiples of 8 bytes.
struct Workspace {
    int64_t entry, exit, gexit, nblk, ntot, dcd, dctot, bytes;
};

inline Workspace workspace_layout(const Geo& g) {
    Workspace w;
    auto up8 = [](int64_t x) { return (x + 7) & ~int64_t(7); };
    int64_t o = 0;
    w.entry = o; o += int64_t(g.nsub) * 8;                               // uint64 entry state of every subsequence
    w.exit = o; o += int64_t(g.nsub) * 8;                                // uint64 exit state
    w.gexit = o; o += int64_t(g.ngroups) * 16;                           // uint64 [2][ngroups]: each workgroup's last exit state, by round parity
    w.nblk = o; o = up8(o + int64_t(g.nsub) * 4);                        // int32 blocks completed, then their inclusive sum per chunk
    w.ntot = o; o = up8(o + int64_t((g.nsub + kChunk - 1) / kChunk) * 4);
    w.dcd = o; o = up8(o + int64_t(g.total) * 4);                        // int32 DC differences in scan order per component, then sums
    w.dctot = o; o = up8(o + int64_t((g.total + kChunk - 1) / kChunk) * 4);
    w.bytes = o;
    return w;
}

SMAP_HD int natural(int k) {                 // zig-zag index -> natural (row-major) index
    const uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k & 63];
}

SMAP_HD uint64_t pack(uint32_t p, int b, int z) { return (uint64_t(p) << 16) | (uint64_t(uint32_t(b)) << 8) | uint64_t(uint32_t(z)); }

// The file bytes: a staged copy of [lo, lo + len) (LDS in the kernels) in front of the whole file.  at(i) requires i < n.
struct Src {
    const uint8_t* file;
    const uint8_t* stage;
    uint32_t n, lo, len;
    SMAP_HD uint32_t at(uint32_t i) const { return (i - lo < len) ? stage[i - lo] : file[i]; }
};

// csrc/jpeg_host.cpp's Bits over Src, plus the raw bit position of the next unread bit: `ff` remembers which of the last bytes loaded
// were 0xFF data bytes (each is followed by a stuffed 0x00 that the position has to step over).
struct Reader {
    uint64_t buf;
    int cnt, pad;
    uint32_t pos, ff;
    bool marker;

    SMAP_HD void reset(uint32_t at) { pos = at; buf = 0; cnt = 0; pad = 0; ff = 0; marker = false; }
    SMAP_HD void refill(const Src& s) {
        while (cnt <= 56) {
            uint32_t b = 0, isff = 0;
            if (marker) {
                pad += 8;
            } else if (pos >= s.n) {
                marker = true;
                pad += 8;
            } else {
                b = s.at(pos);
                if (b == 0xFF) {
                    if (s.n - pos >= 2 && s.at(pos + 1) == 0x00) {
                        pos += 2;
                        isff = 1;
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
            ff = (ff << 1) | isff;
        }
    }
    SMAP_HD uint32_t peek(int k) const { return uint32_t(buf >> (64 - k)); }   // 1 <= k <= 32
    SMAP_HD void skip(int k) { buf <<= k; cnt -= k; }
    SMAP_HD bool overran() const { return cnt < pad; }
    // raw position of the next unread bit (not overran): the bytes still in the buffer, and the stuffed byte behind each 0xFF among them
    SMAP_HD uint32_t bitpos() const {
        const uint32_t nb = uint32_t(cnt + 7) >> 3;
        const uint32_t m = ff & ((1u << nb) - 1u);
#ifdef __HIP_DEVICE_COMPILE__
        const uint32_t nff = uint32_t(__popc(m));
#else
        const uint32_t nff = uint32_t(__builtin_popcount(m));
#endif
        return (pos - nff) * 8u - uint32_t(cnt - pad);
    }
};

SMAP_HD int decode_sym(Reader& b, const smap_jpeg_huff& h) {
    const uint32_t e = h.look[b.peek(kLook)];
    if (e) {
        b.skip(int(e >> 8));
        return int(e & 0xFF);
    }
    for (int l = kLook + 1; l <= 16; ++l) {
        const int32_t code = int32_t(b.peek(l));
        if (code <= h.maxcode[l]) {
            b.skip(l);
            return h.vals[(code + h.valoff[l]) & 255];             // (in range for a table build_huff accepted)
        }
    }
    return -1;
}

SMAP_HD int32_t receive_extend(Reader& b, int s) {
    const int32_t r = int32_t(b.peek(s));
    b.skip(s);
    return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
}

// jpeg_host.cpp take_marker: drop the fill bits; what follows must be a marker with no entropy-coded data before it.
// -> the marker code, the reader past it; or -1.
SMAP_HD int take_marker(Reader& b, const Src& s) {
    b.skip(b.cnt & 7);
    if (b.cnt != b.pad) return -1;
    uint32_t pos = b.pos;
    if (pos >= s.n || s.at(pos) != 0xFF) return -1;
    int fill = 0;
    while (pos < s.n && s.at(pos) == 0xFF && fill <= kMaxFill) ++pos, ++fill;
    if (pos >= s.n || fill > kMaxFill || s.at(pos) == 0x00) return -1;
    const int m = int(s.at(pos));
    b.reset(pos + 1);
    return m;
}

// speculative: the reader stands at a marker (b.marker).  RSTn -> its code, the reader past it; anything else -> -1
SMAP_HD int skip_marker(Reader& b, const Src& s) {
    uint32_t pos = b.pos;
    int fill = 0;
    while (pos < s.n && s.at(pos) == 0xFF && fill <= kMaxFill) ++pos, ++fill;
    if (pos >= s.n || fill == 0 || fill > kMaxFill) return -1;
    const int m = int(s.at(pos));
    if (m < 0xD0 || m > 0xD7) return -1;
    b.reset(pos + 1);
    return m;
}

SMAP_HD uint32_t lane_end_bit(const Geo& g, int lane) {
    const uint64_t e = uint64_t(g.scan_off) + uint64_t(lane + 1) * uint32_t(g.S);
    return uint32_t(e < g.n ? e : g.n) * 8u;
}

// The state a subsequence starts from when nothing is known: (block 0, zig-zag 0) at its first byte -- one later when that byte is the
// 0x00 of a stuffed pair or the second byte of an RSTn.  Subsequence 0's is the true state of the scan's start.
SMAP_HD uint64_t fresh_state(const Src& s, const Geo& g, int lane) {
    if (lane >= g.nsub) return kEnd;
    uint32_t at = g.scan_off + uint32_t(lane) * uint32_t(g.S);
    if (lane > 0 && s.at(at - 1) == 0xFF) {
        const uint32_t c = s.at(at);
        if (c == 0x00 || (c >= 0xD0 && c <= 0xD7)) ++at;
    }
    return pack(at * 8u, 0, 0);
}

struct Out {
    int16_t* coeffs;                         // smap_jpeg_decode_coefficients' layout; DC slots are written by dc_store
    int32_t* dcd;                            // DC differences, scan order per component
};

struct Result {
    uint64_t exit;
    int32_t nblk;                            // blocks completed
    int32_t flags;
};

// block n of the scan (b = n % bpm) -> int16 index of its coefficients, index of its DC difference
SMAP_HD void locate(const Geo& g, int32_t n, int b, int64_t* cidx, int32_t* e) {
    const int c = g.comp[b];
    const int32_t mcu = n / g.bpm, my = mcu / g.mcux, mx = mcu - my * g.mcux;
    const int64_t blk = int64_t(my * g.vs[c] + g.bv[b]) * g.bw[c] + (mx * g.hs[c] + g.bh[b]);
    *cidx = g.plane[c] + blk * 64;
    *e = g.first_elem[c] + mcu * (g.hs[c] * g.vs[c]) + (b - g.first_j[c]);
}

// tab: the scan's six tables (smap_jpeg_scan::table).  n0 (EXACT): the scan-order number of the block the entry state is in.
template <bool EXACT>
SMAP_HD Result decode_subseq(const Src& src, const smap_jpeg_huff* tab, const Geo& g, int lane, uint64_t entry, int32_t n0, Out out) {
    Result R;
    R.exit = entry;
    R.nblk = 0;
    R.flags = 0;
    if (entry == kEnd) return R;
    uint32_t p = uint32_t(entry >> 16);
    int b = int(entry >> 8) & 255, z = int(entry) & 255;
    const uint32_t end_bit = lane_end_bit(g, lane);
    if (p >= end_bit) return R;
    int32_t n = n0;
    if (b >= g.bpm || z > 63 || (EXACT && (n < 0 || n % g.bpm != b || (n >= g.total && (b || z))))) {
        R.flags = kNotConv;                                        // not a state of this scan (cannot come from the passes below)
        R.exit = kEnd;
        return R;
    }
    Reader r;
    r.reset(p >> 3);
    r.refill(src);
    r.skip(int(p & 7));
    int64_t cidx = 0;
    int32_t e = 0;
    if (EXACT && n < g.total) locate(g, n, b, &cidx, &e);
    R.exit = EXACT ? kEnd : fresh_state(src, g, lane + 1);         // where an error leaves: the exact pass ends, the speculation guesses anew
    bool closed = false;
    const int maxit = g.S * 8 + 16;                                // every turn consumes a bit of the subsequence, passes a marker or ends
    for (int it = 0; it < maxit; ++it) {
        if (r.cnt < 32) r.refill(src);
        p = r.bitpos();
        if (p >= end_bit) {
            R.exit = pack(p, b, z);
            closed = true;
            break;
        }
        if (b == 0 && z == 0) {                                    // MCU boundary: the end of the scan or of a restart interval?
            if (EXACT) {
                if (n >= g.total) {                                // EOI right after the last MCU
                    if (take_marker(r, src) != 0xD9) R.flags |= kEData;
                    closed = true;
                    break;
                }
                const int32_t mcu = n / g.bpm;
                if (g.ri && mcu && mcu % g.ri == 0) {              // RST0..7 in sequence; the first symbol after it goes with it
                    if (take_marker(r, src) != 0xD0 + ((mcu / g.ri - 1) & 7)) break;
                    r.refill(src);
                }
            } else {
                const int real = r.cnt - r.pad;                    // a marker ahead and only one-bits left of the last byte: fill
                if (r.marker && real < 8 && (real == 0 || r.peek(real) == (1u << real) - 1u)) {
                    if (skip_marker(r, src) < 0) {
                        R.exit = kEnd;
                        closed = true;
                        break;
                    }
                    r.refill(src);
                }
            }
        }
        const int c = g.comp[b];
        if (z == 0) {                                              // DC difference
            const int s = decode_sym(r, tab[2 * c]);
            if (s < 0) break;
            int32_t diff = 0;
            if (s) {
                if (r.cnt < 32) r.refill(src);
                diff = receive_extend(r, s & 15);
            }
            if (EXACT) out.dcd[e] = diff;
            z = 1;
        } else {                                                   // run / size coded AC term
            const int rs = decode_sym(r, tab[2 * c + 1]);
            if (rs < 0) break;
            const int run = rs >> 4, s = rs & 15;
            if (s) {
                z += run;
                if (z > 63) {
                    if (EXACT) break;
                    r.skip(s);                                     // out of step: keep the bit position, wait for the end of the block
                    z = 1;
                } else {
                    const int32_t v = receive_extend(r, s);
                    if (EXACT) out.coeffs[cidx + natural(z)] = int16_t(v);
                    ++z;
                }
            } else if (run == 15) {
                z += 16;                                           // ZRL
            } else {
                z = 64;                                            // EOB
            }
        }
        if (r.overran()) {                                         // read into the zero bytes behind a marker or the end of the file
            if (EXACT) break;
            if (skip_marker(r, src) < 0) {
                R.exit = kEnd;
                closed = true;
                break;
            }
            b = z = 0;                                             // a restart marker is a free synchronisation point
            continue;
        }
        if (z >= 64) {
            z = 0;
            ++n;
            ++R.nblk;
            if (++b == g.bpm) b = 0;
            if (EXACT && n < g.total) locate(g, n, b, &cidx, &e);
        }
    }
    if (EXACT && !closed) R.flags |= kEData;
    return R;
}

// ---- DC: the differences are summed over the whole scan-ordered array; a block's predictor is its sum minus the sum before its
// restart interval (int32 arithmetic is exact and wraps as the host's running sum does) ----

// element e of the DC array -> int16 index of the block's DC slot, first element of its restart interval
SMAP_HD void dc_locate(const Geo& g, int32_t e, int64_t* cidx, int32_t* seg) {
    const int c = (g.ncomp > 1 && e >= g.first_elem[1]) + (g.ncomp > 2 && e >= g.first_elem[2]);
    const int32_t le = e - g.first_elem[c], per = g.hs[c] * g.vs[c];
    const int32_t mcu = le / per, j = le - mcu * per, v = j / g.hs[c], h = j - v * g.hs[c];
    const int32_t my = mcu / g.mcux, mx = mcu - my * g.mcux;
    *cidx = g.plane[c] + (int64_t(my * g.vs[c] + v) * g.bw[c] + (mx * g.hs[c] + h)) * 64;
    *seg = g.first_elem[c] + (g.ri ? (mcu / g.ri) * g.ri * per : 0);
}

// x: inclusive sums inside each chunk of kChunk; tot: exclusive sums of the chunk totals.  -> the inclusive sum up to i (0 for i < 0)
SMAP_HD int32_t sum_upto(const int32_t* x, const int32_t* tot, int32_t i) {
    return i < 0 ? 0 : int32_t(uint32_t(x[i]) + uint32_t(tot[i / kChunk]));
}

SMAP_HD void dc_store(const Geo& g, const int32_t* x, const int32_t* tot, int32_t e, int16_t* coeffs) {
    int64_t cidx;
    int32_t seg;
    dc_locate(g, e, &cidx, &seg);
    coeffs[cidx] = int16_t(uint32_t(sum_upto(x, tot, e)) - uint32_t(sum_upto(x, tot, seg - 1)));
}

}  // namespace smap_huff
