// svgr_jpeg.cpp -- the entropy-coded data of one JPEG scan decoded on the host (jpeg.py reads the markers), and, at the end of
// the file, coded on the host (write_jpeg).
//
// Huffman decoding is a serial walk over the bits (each code's length is known only once it is read; the DC predictor and
// the end-of-band run carry from block to block), so it is native host code, like the PNG filters, and rides in the same
// library.  One call decodes one scan into the frame's coefficient arrays: a sequential frame (SOF0 / SOF1) has one scan per
// component or one for all; a progressive frame (SOF2) has many, each adding a band of frequencies or one more bit, which
// is why the arrays persist between calls and start as zeros.  The per-pixel work (dequantisation, inverse DCT, upsampling,
// colour) is the device's: svgr_jpeg_decode.
//
// ITU-T T.81: F.2.2 (sequential), G.1.2 (progressive), F.1.2.3 / E.2.4 (restart intervals), B.1.1.5 (byte stuffing).
// Nothing here trusts the data: every table index, block index and bit count is checked, and reading past the end of the
// data is an error, not a read.
#include <cstdint>
#include <cstring>

#include "../../include/svgr.h"

namespace {

constexpr uint8_t kZigzag[64] = {   // position in the scan order -> natural (row-major) index
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
};

enum { kOk = 0, kTruncated = SVGR_JPEG_TRUNCATED, kBadCode = SVGR_JPEG_BAD_CODE, kBadRestart = SVGR_JPEG_BAD_RESTART,
       kBadIndex = SVGR_JPEG_BAD_INDEX };

// The bits of the entropy-coded segment, most significant first.  FF 00 is a stuffed FF; any other FF xx is a marker, where
// the reader stops and supplies zeros.  Bits that were never in the data are counted (`fake`): consuming one is an overrun.
struct Bits {
    const uint8_t* p;
    int64_t n, pos = 0;
    uint64_t buf = 0;
    int cnt = 0, fake = 0;
    bool stopped = false, overrun = false;

    Bits(const uint8_t* data, int64_t bytes) : p(data), n(bytes) {}
    void fill() {
        while (cnt <= 56) {
            uint64_t b = 0;
            if (!stopped && pos < n) {
                b = p[pos];
                if (b != 0xFF) {
                    ++pos;
                } else if (pos + 1 < n && p[pos + 1] == 0) {
                    pos += 2;
                } else {
                    stopped = true;
                    b = 0;
                }
            } else {
                stopped = true;
            }
            if (stopped) fake += 8;
            buf |= b << (56 - cnt);
            cnt += 8;
        }
    }
    uint32_t peek16() {
        fill();
        return (uint32_t)(buf >> 48);
    }
    void consume(int k) {
        buf <<= k;
        cnt -= k;
        if (cnt < fake) overrun = true;
    }
    int receive(int k) {   // 0 <= k <= 16
        if (k == 0) return 0;
        fill();
        const int v = (int)(buf >> (64 - k));
        consume(k);
        return v;
    }
    // the restart marker RSTm that must come next: drops the padding bits in front of it
    bool restart(int m) {
        buf = 0;
        cnt = fake = 0;
        stopped = false;
        if (pos >= n || p[pos] != 0xFF) return false;
        while (pos < n && p[pos] == 0xFF) ++pos;
        if (pos >= n || p[pos] != 0xD0 + m) return false;
        ++pos;
        return true;
    }
};

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }   // T.81 F.2.2.1, s >= 1

struct Huff {
    bool defined = false;
    uint16_t look[512];   // the next 9 bits -> length << 8 | symbol, 0: the code is longer
    int32_t end[17];      // end[len]: one past the largest code of that length
    int32_t off[17];      // vals index of a code c of length len: off[len] + c
    uint8_t vals[256];

    // counts[16] codes per length, then the symbols in code order (T.81 annex C)
    bool build(const uint8_t* counts, const uint8_t* symbols) {
        int total = 0;
        for (int i = 0; i < 16; ++i) total += counts[i];
        if (total == 0 || total > 256) return false;
        memset(look, 0, sizeof look);
        memcpy(vals, symbols, (size_t)total);
        int32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            off[len] = k - code;
            for (int i = 0; i < counts[len - 1]; ++i, ++code, ++k) {
                if (code >= (1 << len)) return false;   // (more codes than the length has)
                if (len <= 9)
                    for (int f = 0; f < (1 << (9 - len)); ++f) look[(code << (9 - len)) + f] = (uint16_t)(len << 8 | symbols[k]);
            }
            end[len] = code;
            code <<= 1;
        }
        defined = true;
        return true;
    }
    int decode(Bits& b) const {   // the symbol, or -1
        const uint32_t v = b.peek16();
        const uint16_t e = look[v >> 7];
        if (e) {
            b.consume(e >> 8);
            return e & 0xFF;
        }
        for (int len = 10; len <= 16; ++len) {
            const int32_t c = (int32_t)(v >> (16 - len));
            if (c < end[len]) {
                b.consume(len);
                return vals[off[len] + c];
            }
        }
        return -1;
    }
};

inline int16_t wrap16(int64_t v) { return (int16_t)(uint16_t)(uint64_t)v; }   // (a corrupt stream may ask for anything)

struct Scan {
    const svgr_jpeg_scan* s;
    Bits bits;
    Huff dc[4], ac[4];
    int32_t pred[3] = {0, 0, 0};
    int32_t eobrun = 0;

    Scan(const svgr_jpeg_scan* scan, const uint8_t* data, int64_t n) : s(scan), bits(data, n) {}

    int dc_diff(const Huff& h, int* diff) {
        const int t = h.decode(bits);
        if (t < 0 || t > 15) return kBadCode;
        *diff = t ? extend(bits.receive(t), t) : 0;
        return kOk;
    }

    int sequential_block(int16_t* blk, int ci, const Huff& hd, const Huff& ha) {
        int diff;
        if (int rc = dc_diff(hd, &diff)) return rc;
        pred[ci] = (int32_t)((uint32_t)pred[ci] + (uint32_t)diff);
        blk[0] = wrap16(pred[ci]);
        for (int k = 1; k < 64;) {
            const int rs = ha.decode(bits);
            if (rs < 0) return kBadCode;
            const int r = rs >> 4, sz = rs & 15;
            if (sz == 0) {
                if (r != 15) break;
                k += 16;
                continue;
            }
            k += r;
            if (k > 63) return kBadIndex;
            blk[kZigzag[k]] = (int16_t)extend(bits.receive(sz), sz);
            ++k;
        }
        return kOk;
    }

    int dc_first(int16_t* blk, int ci, const Huff& hd) {
        int diff;
        if (int rc = dc_diff(hd, &diff)) return rc;
        pred[ci] = (int32_t)((uint32_t)pred[ci] + (uint32_t)diff);
        blk[0] = wrap16((int64_t)pred[ci] * (1 << s->al));
        return kOk;
    }

    void dc_refine(int16_t* blk) {
        if (bits.receive(1)) blk[0] = (int16_t)(blk[0] | (1 << s->al));
    }

    int ac_first(int16_t* blk, const Huff& ha) {
        if (eobrun > 0) {
            --eobrun;
            return kOk;
        }
        for (int k = s->ss; k <= s->se;) {
            const int rs = ha.decode(bits);
            if (rs < 0) return kBadCode;
            const int r = rs >> 4, sz = rs & 15;
            if (sz == 0) {
                if (r < 15) {   // an end-of-band run of 2^r + (r more bits) blocks, this one included
                    eobrun = (1 << r) - 1;
                    if (r) eobrun += bits.receive(r);
                    break;
                }
                k += 16;
                continue;
            }
            k += r;
            if (k > s->se) return kBadIndex;
            blk[kZigzag[k]] = wrap16((int64_t)extend(bits.receive(sz), sz) * (1 << s->al));
            ++k;
        }
        return kOk;
    }

    // one more bit of a coefficient that is already non-zero (T.81 G.1.2.3)
    void refine_nonzero(int16_t* c, int p1) {
        if (bits.receive(1) && (*c & p1) == 0) *c = wrap16((int64_t)*c + (*c >= 0 ? p1 : -p1));
    }

    int ac_refine(int16_t* blk, const Huff& ha) {
        const int p1 = 1 << s->al;
        int k = s->ss;
        if (eobrun == 0) {
            while (k <= s->se) {
                const int rs = ha.decode(bits);
                if (rs < 0) return kBadCode;
                int r = rs >> 4;
                const int sz = rs & 15;
                int val = 0;
                if (sz == 0) {
                    if (r < 15) {
                        eobrun = 1 << r;
                        if (r) eobrun += bits.receive(r);
                        break;
                    }   // (r == 15: sixteen zero-history coefficients pass, the non-zero ones between them are refined)
                } else {
                    if (sz != 1) return kBadCode;
                    val = bits.receive(1) ? p1 : -p1;
                }
                for (; k <= s->se; ++k) {
                    int16_t* c = blk + kZigzag[k];
                    if (*c != 0) {
                        refine_nonzero(c, p1);
                    } else if (--r < 0) {
                        break;
                    }
                }
                if (sz) {
                    if (k > s->se) return kBadIndex;
                    blk[kZigzag[k]] = (int16_t)val;
                }
                ++k;
            }
        }
        if (eobrun > 0) {
            for (; k <= s->se; ++k) {
                int16_t* c = blk + kZigzag[k];
                if (*c != 0) refine_nonzero(c, p1);
            }
            --eobrun;
        }
        return kOk;
    }
};

}  // namespace

extern "C" {

int svgr_jpeg_entropy(const svgr_jpeg_scan* s, const uint8_t* huff_counts, const uint8_t* huff_symbols, const uint8_t* data,
                      int64_t n_bytes, int16_t* coef, int64_t n_coef) {
    if (!s || !huff_counts || !huff_symbols || !data || !coef || n_bytes < 0) return SVGR_E_INVALID;
    const svgr_jpeg_frame& f = s->frame;
    if ((f.n_comp != 1 && f.n_comp != 3) || f.width < 1 || f.height < 1 || f.width > 65535 || f.height > 65535) return SVGR_E_INVALID;
    int hmax = 1, vmax = 1;
    for (int i = 0; i < f.n_comp; ++i) {
        if (f.h[i] < 1 || f.h[i] > 2 || f.v[i] < 1 || f.v[i] > 2) return SVGR_E_INVALID;
        hmax = f.h[i] > hmax ? f.h[i] : hmax;
        vmax = f.v[i] > vmax ? f.v[i] : vmax;
    }
    if (f.n_comp == 1 && (hmax != 1 || vmax != 1)) return SVGR_E_INVALID;   // (a lone component is stored unsampled: A.2.2)
    const int64_t mcus_x = (f.width + 8 * hmax - 1) / (8 * hmax), mcus_y = (f.height + 8 * vmax - 1) / (8 * vmax);
    int64_t base[3], bw[3], total = 0;   // each component's first block and blocks per row, padded to whole MCUs
    for (int i = 0; i < f.n_comp; ++i) {
        base[i] = total;
        bw[i] = mcus_x * f.h[i];
        total += bw[i] * mcus_y * f.v[i];
    }
    if (n_coef != total * 64) return SVGR_E_INVALID;
    if (s->n_scan < 1 || s->n_scan > f.n_comp || s->restart_interval < 0 || s->restart_interval > 65535) return SVGR_E_INVALID;
    for (int j = 0; j < s->n_scan; ++j) {
        if (s->scan_comp[j] < 0 || s->scan_comp[j] >= f.n_comp || (j && s->scan_comp[j] <= s->scan_comp[j - 1])) return SVGR_E_INVALID;
        if (s->dc_table[j] < 0 || s->dc_table[j] > 3 || s->ac_table[j] < 0 || s->ac_table[j] > 3) return SVGR_E_INVALID;
    }
    const bool prog = s->progressive != 0;
    if (prog) {
        if (s->ss < 0 || s->se < s->ss || s->se > 63 || s->ah < 0 || s->ah > 13 || s->al < 0 || s->al > 13) return SVGR_E_INVALID;
        if (s->ss == 0 ? s->se != 0 : s->n_scan != 1) return SVGR_E_INVALID;   // (DC alone, or the AC band of one component)
        if (s->ah != 0 && s->ah != s->al + 1) return SVGR_E_INVALID;
    } else if (s->ss != 0 || s->se != 63 || s->ah != 0 || s->al != 0) {
        return SVGR_E_INVALID;
    }
    const bool need_dc = !prog || (s->ss == 0 && s->ah == 0), need_ac = !prog || s->ss > 0;

    Scan sc(s, data, n_bytes);
    for (int j = 0; j < s->n_scan; ++j) {
        const int d = s->dc_table[j], a = s->ac_table[j];
        if (need_dc && !sc.dc[d].defined && !sc.dc[d].build(huff_counts + 16 * d, huff_symbols + 256 * d)) return kBadCode;
        if (need_ac && !sc.ac[a].defined && !sc.ac[a].build(huff_counts + 16 * (4 + a), huff_symbols + 256 * (4 + a))) return kBadCode;
    }

    auto block = [&](int j, int64_t row, int64_t col) -> int {
        const int ci = s->scan_comp[j];
        int16_t* blk = coef + (base[ci] + row * bw[ci] + col) * 64;
        const Huff &hd = sc.dc[s->dc_table[j]], &ha = sc.ac[s->ac_table[j]];
        if (!prog) return sc.sequential_block(blk, ci, hd, ha);
        if (s->ss == 0) {
            if (s->ah == 0) return sc.dc_first(blk, ci, hd);
            sc.dc_refine(blk);
            return kOk;
        }
        return s->ah == 0 ? sc.ac_first(blk, ha) : sc.ac_refine(blk, ha);
    };

    // the scan's units: whole MCUs when it interleaves components, else the one component's own blocks (A.2.2, A.2.3)
    int64_t units_x = mcus_x, units_y = mcus_y;
    if (s->n_scan == 1) {
        const int ci = s->scan_comp[0];
        const int64_t cw = ((int64_t)f.width * f.h[ci] + hmax - 1) / hmax, ch = ((int64_t)f.height * f.v[ci] + vmax - 1) / vmax;
        units_x = (cw + 7) / 8;
        units_y = (ch + 7) / 8;
    }
    int64_t since_restart = 0;
    int next_restart = 0;
    for (int64_t uy = 0; uy < units_y; ++uy) {
        for (int64_t ux = 0; ux < units_x; ++ux) {
            if (s->restart_interval && since_restart == s->restart_interval) {
                if (sc.bits.overrun) return kTruncated;
                if (!sc.bits.restart(next_restart)) return kBadRestart;
                next_restart = (next_restart + 1) & 7;
                since_restart = 0;
                sc.pred[0] = sc.pred[1] = sc.pred[2] = 0;
                sc.eobrun = 0;
            }
            ++since_restart;
            if (s->n_scan == 1) {
                if (int rc = block(0, uy, ux)) return rc;
            } else {
                for (int j = 0; j < s->n_scan; ++j) {
                    const int ci = s->scan_comp[j];
                    for (int y = 0; y < f.v[ci]; ++y)
                        for (int x = 0; x < f.h[ci]; ++x)
                            if (int rc = block(j, uy * f.v[ci] + y, ux * f.h[ci] + x)) return rc;
                }
            }
            if (sc.bits.overrun) return kTruncated;
        }
    }
    return SVGR_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// The way back (write_jpeg): one baseline sequential scan coded from the frame's coefficients.  T.81 F.1.2 (Huffman
// encoding), with the byte stuffing and restart rules above.  The same walk either writes the bits or counts the symbols.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

// Bytes out, most significant bit first; never past `cap`, but `pos` counts on, so the caller learns the room needed.
struct BitsOut {
    uint8_t* p;
    int64_t cap, pos = 0;
    uint64_t buf = 0;   // the low `cnt` bits are waiting
    int cnt = 0;

    BitsOut(uint8_t* out, int64_t n) : p(out), cap(n) {}
    void byte(uint8_t b) {
        if (pos < cap) p[pos] = b;
        ++pos;
    }
    void put(uint32_t bits, int k) {   // 0 <= k <= 27, bits < 2^k
        buf = buf << k | bits;
        cnt += k;
        while (cnt >= 8) {
            const uint8_t b = (uint8_t)(buf >> (cnt - 8));
            byte(b);
            if (b == 0xFF) byte(0);
            cnt -= 8;
        }
    }
    void flush() {   // the last byte filled with ones
        if (cnt) put((1u << (8 - cnt)) - 1, 8 - cnt);
    }
    void marker(uint8_t code) {
        flush();
        byte(0xFF);
        byte(code);
    }
};

struct HuffCode {
    bool defined = false;
    uint16_t code[256];
    uint8_t len[256];   // 0: the table has no code for the symbol

    bool build(const uint8_t* counts, const uint8_t* symbols) {
        int total = 0;
        for (int i = 0; i < 16; ++i) total += counts[i];
        if (total == 0 || total > 256) return false;
        memset(len, 0, sizeof len);
        int32_t c = 0;
        int k = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < counts[l - 1]; ++i, ++c, ++k) {
                if (c >= (1 << l) || len[symbols[k]]) return false;   // (more codes than the length has; a symbol twice)
                code[symbols[k]] = (uint16_t)c;
                len[symbols[k]] = (uint8_t)l;
            }
            c <<= 1;
        }
        defined = true;
        return true;
    }
};

inline int category(int v) {   // the number of bits of |v|
    int a = v < 0 ? -v : v, n = 0;
    for (; a; a >>= 1) ++n;
    return n;
}

// What a walk does with a symbol and the extra bits behind it: write them, or count the symbol.
struct Writer {
    BitsOut bits;
    HuffCode dc[4], ac[4];
    bool missing = false;
    Writer(uint8_t* out, int64_t cap) : bits(out, cap) {}
    void symbol(bool is_ac, int table, int sym, uint32_t extra, int n_extra) {
        const HuffCode& h = is_ac ? ac[table] : dc[table];
        if (!h.len[sym]) {
            missing = true;
            return;
        }
        bits.put((uint32_t)h.code[sym] << n_extra | extra, h.len[sym] + n_extra);
    }
    void restart(int m) { bits.marker((uint8_t)(0xD0 + m)); }
};
struct Counter {
    int64_t* counts;
    bool missing = false;
    void symbol(bool is_ac, int table, int sym, uint32_t, int) { ++counts[256 * (4 * (int)is_ac + table) + sym]; }
    void restart(int) {}
};

// the description of a sequential scan checked as svgr_jpeg_entropy checks it, and each component's place in the array
struct ScanLayout {
    int64_t base[3], bw[3], mcus_x, mcus_y, units_x, units_y;
};
int scan_layout(const svgr_jpeg_scan* s, int64_t n_coef, ScanLayout& L) {
    const svgr_jpeg_frame& f = s->frame;
    if ((f.n_comp != 1 && f.n_comp != 3) || f.width < 1 || f.height < 1 || f.width > 65535 || f.height > 65535) return SVGR_E_INVALID;
    int hmax = 1, vmax = 1;
    for (int i = 0; i < f.n_comp; ++i) {
        if (f.h[i] < 1 || f.h[i] > 2 || f.v[i] < 1 || f.v[i] > 2) return SVGR_E_INVALID;
        hmax = f.h[i] > hmax ? f.h[i] : hmax;
        vmax = f.v[i] > vmax ? f.v[i] : vmax;
    }
    if (f.n_comp == 1 && (hmax != 1 || vmax != 1)) return SVGR_E_INVALID;
    L.mcus_x = (f.width + 8 * hmax - 1) / (8 * hmax);
    L.mcus_y = (f.height + 8 * vmax - 1) / (8 * vmax);
    int64_t total = 0;
    for (int i = 0; i < f.n_comp; ++i) {
        L.base[i] = total;
        L.bw[i] = L.mcus_x * f.h[i];
        total += L.bw[i] * L.mcus_y * f.v[i];
    }
    if (n_coef != total * 64) return SVGR_E_INVALID;
    if (s->n_scan < 1 || s->n_scan > f.n_comp || s->restart_interval < 0 || s->restart_interval > 65535) return SVGR_E_INVALID;
    for (int j = 0; j < s->n_scan; ++j) {
        if (s->scan_comp[j] < 0 || s->scan_comp[j] >= f.n_comp || (j && s->scan_comp[j] <= s->scan_comp[j - 1])) return SVGR_E_INVALID;
        if (s->dc_table[j] < 0 || s->dc_table[j] > 3 || s->ac_table[j] < 0 || s->ac_table[j] > 3) return SVGR_E_INVALID;
    }
    if (s->progressive || s->ss != 0 || s->se != 63 || s->ah != 0 || s->al != 0) return SVGR_E_INVALID;
    L.units_x = L.mcus_x;
    L.units_y = L.mcus_y;
    if (s->n_scan == 1) {   // (one component: its own blocks, A.2.2)
        const int ci = s->scan_comp[0];
        const int64_t cw = ((int64_t)f.width * f.h[ci] + hmax - 1) / hmax, ch = ((int64_t)f.height * f.v[ci] + vmax - 1) / vmax;
        L.units_x = (cw + 7) / 8;
        L.units_y = (ch + 7) / 8;
    }
    return SVGR_OK;
}

template <class Sink>
void code_block(Sink& sink, const int16_t* blk, int32_t* pred, int td, int ta) {
    const int diff = (int)blk[0] - *pred;
    *pred = blk[0];
    int n = category(diff);
    // (F.1.2.1: the low n bits of diff, of diff - 1 when it is negative; n beyond 11 has no symbol in a baseline table)
    if (n > 11) sink.missing = true;
    else sink.symbol(false, td, n, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1), n);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = blk[kZigzag[k]];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run >= 16; run -= 16) sink.symbol(true, ta, 0xF0, 0, 0);   // ZRL
        n = category(v);
        if (n > 10) sink.missing = true;
        else sink.symbol(true, ta, run << 4 | n, (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1), n);
        run = 0;
    }
    if (run) sink.symbol(true, ta, 0x00, 0, 0);   // EOB
}

template <class Sink>
void walk(const svgr_jpeg_scan* s, const ScanLayout& L, const int16_t* coef, Sink& sink) {
    const svgr_jpeg_frame& f = s->frame;
    int32_t pred[3] = {0, 0, 0};
    int64_t since_restart = 0;
    int next_restart = 0;
    for (int64_t uy = 0; uy < L.units_y; ++uy)
        for (int64_t ux = 0; ux < L.units_x; ++ux) {
            if (s->restart_interval && since_restart == s->restart_interval) {
                sink.restart(next_restart);
                next_restart = (next_restart + 1) & 7;
                since_restart = 0;
                pred[0] = pred[1] = pred[2] = 0;
            }
            ++since_restart;
            for (int j = 0; j < s->n_scan; ++j) {
                const int ci = s->scan_comp[j];
                const int nv = s->n_scan == 1 ? 1 : f.v[ci], nh = s->n_scan == 1 ? 1 : f.h[ci];
                for (int y = 0; y < nv; ++y)
                    for (int x = 0; x < nh; ++x)
                        code_block(sink, coef + (L.base[ci] + (uy * nv + y) * L.bw[ci] + ux * nh + x) * 64, &pred[ci], s->dc_table[j],
                                   s->ac_table[j]);
            }
        }
}

}  // namespace

extern "C" {

int svgr_jpeg_entropy_encode(const svgr_jpeg_scan* s, const uint8_t* huff_counts, const uint8_t* huff_symbols, const int16_t* coef,
                             int64_t n_coef, uint8_t* out, int64_t out_cap, int64_t* n_bytes) {
    if (!s || !huff_counts || !huff_symbols || !coef || !n_bytes || out_cap < 0 || (!out && out_cap)) return SVGR_E_INVALID;
    *n_bytes = 0;
    ScanLayout L;
    if (int rc = scan_layout(s, n_coef, L)) return rc;
    Writer w(out, out_cap);
    for (int j = 0; j < s->n_scan; ++j) {
        const int d = s->dc_table[j], a = s->ac_table[j];
        if (!w.dc[d].defined && !w.dc[d].build(huff_counts + 16 * d, huff_symbols + 256 * d)) return kBadCode;
        if (!w.ac[a].defined && !w.ac[a].build(huff_counts + 16 * (4 + a), huff_symbols + 256 * (4 + a))) return kBadCode;
    }
    walk(s, L, coef, w);
    w.bits.flush();
    if (w.missing) return kBadCode;
    *n_bytes = w.bits.pos;
    return w.bits.pos > out_cap ? SVGR_JPEG_NO_ROOM : SVGR_OK;
}

int svgr_jpeg_symbol_counts(const svgr_jpeg_scan* s, const int16_t* coef, int64_t n_coef, int64_t* counts) {
    if (!s || !coef || !counts) return SVGR_E_INVALID;
    ScanLayout L;
    if (int rc = scan_layout(s, n_coef, L)) return rc;
    Counter c{counts};
    walk(s, L, coef, c);
    return c.missing ? (int)kBadCode : (int)SVGR_OK;
}

}  // extern "C"
