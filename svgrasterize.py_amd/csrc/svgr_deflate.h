// svgr_deflate.h -- deflate (RFC 1951) for the PNG writer: the symbol maps, the token rule, the bit packing and the Adler-32
// pieces a lane computes, and the host's code builder.
//
// What is marked DEFL_HD is integer arithmetic compilable for the host (the CPU harness of tests/png_enc_harness.cpp) and for
// the device (k_deflate_tokens / k_deflate_emit of svgr_hip.hip); the code builder (deflate_build_codes) is host code shared by
// the library and the harness.  DESIGN.md 7n has the definitions; tests/png_enc_ref.py restates them in Python.
//
//   chunk     the input is cut into chunks of DEFLATE_CH bytes; chunk k is bytes [k * CH, min(n, (k + 1) * CH)).  Each chunk
//             is one deflate block of the one stream, so a match may reach back into earlier chunks (distance <= 32768) but is
//             cut at its own chunk's end
//   hash      position q has a hash when q + 2 lies in q's own chunk: deflate_hash3 of its three bytes, a bucket of a table of
//             2^DEFLATE_HASH_BITS.  Positions are entered sub-window by sub-window (DEFLATE_SUB positions, aligned to the chunk):
//             the hash candidate of p is the LARGEST position with p's bucket among the positions >= start - 32768 (start: p's
//             chunk's first byte) that lie in front of p's sub-window -- a maximum, so it does not depend on any order of insertion.
//             It counts only when p - q <= 32768
//   matcher   candidates in this order: distance 1 (p >= 1), distance 4 (p >= 4), the hash candidate.  The length of each is the
//             number of equal bytes src[p + i] == src[p - d + i], at most cap = min(258, chunk end - p).  The longest wins, a tie
//             goes to the earlier candidate.  Below 3, or 3 at a distance beyond DEFLATE_TOO_FAR, the position is a literal
//   parse     greedy from the chunk's first byte: a position with a match emits it and skips its length, any other emits its byte
//   token     uint32: a literal is its byte (< 256); a match is (length << 16) | (distance - 1)
//   bits      a Huffman code enters the stream most significant bit first, extra bits least significant first, and the stream
//             fills bytes from bit 0: the tables hold every code bit-reversed, so a token is ONE value OR-ed in at its bit offset
//   block     header bits, the tokens, symbol 256; every chunk but the last then ends with an empty stored block (000, pad to a
//             byte, 00 00 FF FF), the last is padded to a byte and carries BFINAL.  Every chunk begins on a byte boundary
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define DEFL_HD __host__ __device__ inline
#else
#define DEFL_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define DEFL_OR(p, v) atomicOr((p), (v))   // lanes share words of the slot: OR commutes, so the bytes do not depend on their order
#else
#define DEFL_OR(p, v) ((void)(*(p) |= (v)))
#endif

constexpr int DEFLATE_CH = 16384;          // bytes per chunk = per workgroup = per block of the stream
constexpr int DEFLATE_WINDOW = 32768;
constexpr int DEFLATE_MIN_MATCH = 3, DEFLATE_MAX_MATCH = 258;
constexpr int DEFLATE_TOO_FAR = 4096;      // a match of 3 further back costs more bits than its three literals (zlib's rule)
constexpr int DEFLATE_HASH_BITS = 13;
constexpr int DEFLATE_SUB = 256;           // positions per sub-window of the hash table's updates
constexpr int DEFLATE_NLIT = 286, DEFLATE_NDIST = 30, DEFLATE_NSYM = DEFLATE_NLIT + DEFLATE_NDIST;
constexpr int DEFLATE_EOB = 256;
constexpr int DEFLATE_HDR_MAX = 320;       // bytes: 3 + 14 + 19 * 3 + 316 * 7 bits at the most
// A chunk's slot: a byte costs at most 16 bits (a literal 15, a match of 3 bytes 48), then the header, symbol 256 and the tail
constexpr int DEFLATE_SLOT = 2 * DEFLATE_CH + 384;
constexpr int DEFLATE_FIXED = 0, DEFLATE_DYNAMIC = 1;
constexpr uint32_t ADLER_MOD = 65521;
static_assert(DEFLATE_CH % DEFLATE_SUB == 0 && DEFLATE_WINDOW % DEFLATE_CH == 0 && DEFLATE_SLOT % 64 == 0, "chunk geometry");

// One code pair for the whole stream, every code bit-reversed, and the block header's bits (BFINAL clear).
struct DeflateCodes {
    uint16_t lcode[288];
    uint16_t dcode[32];
    uint8_t llen[288];
    uint8_t dlen[32];
    uint32_t hdr_bits, pad;
    uint32_t hdr[DEFLATE_HDR_MAX / 4];
};

DEFL_HD int deflate_msb(uint32_t x) { return 31 - __builtin_clz(x); }   // x > 0

// length 3 .. 258 -> symbol 257 .. 285, the count of extra bits and their value (RFC 1951 3.2.5)
DEFL_HD void deflate_len_sym(int len, int& sym, int& nbits, int& val) {
    const int l = len - 3;
    if (len == DEFLATE_MAX_MATCH) { sym = 285; nbits = 0; val = 0; return; }
    if (l < 8) { sym = 257 + l; nbits = 0; val = 0; return; }
    const int e = deflate_msb((uint32_t)l) - 2;
    sym = 261 + 4 * e + ((l >> e) & 3);
    nbits = e;
    val = l & ((1 << e) - 1);
}
// distance 1 .. 32768 -> symbol 0 .. 29
DEFL_HD void deflate_dist_sym(int dist, int& sym, int& nbits, int& val) {
    const int d = dist - 1;
    if (d < 4) { sym = d; nbits = 0; val = 0; return; }
    const int e = deflate_msb((uint32_t)d) - 1;
    sym = 2 * e + 2 + ((d >> e) & 1);
    nbits = e;
    val = d & ((1 << e) - 1);
}

DEFL_HD int deflate_tok_len(uint32_t tok) { return (int)(tok >> 16); }            // 0: a literal
DEFL_HD int deflate_tok_dist(uint32_t tok) { return (int)(tok & 0xFFFFu) + 1; }
DEFL_HD int deflate_tok_hop(uint32_t tok) { return tok < 256 ? 1 : deflate_tok_len(tok); }

// The bucket of the three bytes at s.
DEFL_HD uint32_t deflate_hash3(const uint8_t* s) {
    const uint32_t v = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
    return (v * 0x9E3779B1u) >> (32 - DEFLATE_HASH_BITS);
}
// The end of the chunk position q lies in, and whether q has a hash.
DEFL_HD int64_t deflate_chunk_end(int64_t q, int64_t n) {
    const int64_t e = (q / DEFLATE_CH + 1) * DEFLATE_CH;
    return e < n ? e : n;
}
DEFL_HD bool deflate_hashed(int64_t q, int64_t n) { return q + 2 < deflate_chunk_end(q, n); }

// Equal bytes of src[p ..] and src[p - d ..], at most cap (eight at a time; both hosts of this code are little-endian).
DEFL_HD int deflate_match(const uint8_t* src, int64_t p, int64_t d, int cap) {
    const uint8_t* x = src + p;
    const uint8_t* y = src + p - d;
    int n = 0;
    while (n + 8 <= cap) {
        uint64_t u, v;
        memcpy(&u, x + n, 8);
        memcpy(&v, y + n, 8);
        if (u != v) return n + (__builtin_ctzll(u ^ v) >> 3);
        n += 8;
    }
    while (n < cap && x[n] == y[n]) ++n;
    return n;
}

// The token position p would emit: its best match by the matcher's rule, or its byte.  q: the hash candidate or -1.
DEFL_HD uint32_t deflate_best(const uint8_t* src, int64_t p, int64_t chunk_end, int64_t q) {
    const int64_t left = chunk_end - p;
    const int cap = left < DEFLATE_MAX_MATCH ? (int)left : DEFLATE_MAX_MATCH;
    int best = 0;
    int64_t best_d = 0;
    if (cap >= DEFLATE_MIN_MATCH) {
        const int64_t cand[3] = {p >= 1 ? 1 : 0, p >= 4 ? 4 : 0, q >= 0 && p - q <= DEFLATE_WINDOW ? p - q : 0};
        for (int k = 0; k < 3 && best < cap; ++k) {
            if (!cand[k]) continue;
            const int l = deflate_match(src, p, cand[k], cap);
            if (l > best) { best = l; best_d = cand[k]; }
        }
    }
    if (best < DEFLATE_MIN_MATCH || (best == DEFLATE_MIN_MATCH && best_d > DEFLATE_TOO_FAR)) return src[p];
    return ((uint32_t)best << 16) | (uint32_t)(best_d - 1);
}

// A token's bits as one value (at most 48 bits) and their count.
DEFL_HD int deflate_token_bits(const uint16_t* lcode, const uint8_t* llen, const uint16_t* dcode, const uint8_t* dlen, uint32_t tok,
                               uint64_t& v) {
    if (tok < 256) { v = lcode[tok]; return llen[tok]; }
    int sym, nb, val;
    deflate_len_sym(deflate_tok_len(tok), sym, nb, val);
    v = lcode[sym];
    int n = llen[sym];
    v |= (uint64_t)val << n;
    n += nb;
    deflate_dist_sym(deflate_tok_dist(tok), sym, nb, val);
    v |= (uint64_t)dcode[sym] << n;
    n += dlen[sym];
    v |= (uint64_t)val << n;
    return n + nb;
}
// The symbols a token counts for: its literal / length symbol and, for a match, its distance symbol (else -1).
DEFL_HD void deflate_token_syms(uint32_t tok, int& lsym, int& dsym) {
    if (tok < 256) { lsym = (int)tok; dsym = -1; return; }
    int nb, val;
    deflate_len_sym(deflate_tok_len(tok), lsym, nb, val);
    deflate_dist_sym(deflate_tok_dist(tok), dsym, nb, val);
}

// OR the low bits of v (at most 48) into the slot's words at bit offset pos.
DEFL_HD void deflate_put(uint32_t* words, uint32_t pos, uint64_t v) {
    const uint32_t s = pos & 31;
    uint32_t* w = words + (pos >> 5);
    const uint64_t lo = v << s;
    const uint32_t hi = s ? (uint32_t)(v >> (64 - s)) : 0u;
    if ((uint32_t)lo) DEFL_OR(w, (uint32_t)lo);
    if ((uint32_t)(lo >> 32)) DEFL_OR(w + 1, (uint32_t)(lo >> 32));
    if (hi) DEFL_OR(w + 2, hi);
}
// What follows a chunk's tokens, from bit offset pos: symbol 256, then the empty stored block or the padding.  The chunk's bytes.
DEFL_HD uint32_t deflate_chunk_tail(uint32_t* words, uint32_t pos, uint32_t eob_code, int eob_len, bool last) {
    deflate_put(words, pos, eob_code);
    pos += (uint32_t)eob_len;
    if (!last) {
        pos = (pos + 3 + 7) & ~7u;   // BFINAL 0, BTYPE 00, zero bits up to the byte
        deflate_put(words, pos, 0xFFFF0000ull);   // LEN 0, NLEN 0xFFFF
        pos += 32;
    } else {
        pos = (pos + 7) & ~7u;
    }
    return pos >> 3;
}

// Adler-32 in pieces.  A chunk of len bytes b[i] gives A = sum b[i], B = sum (len - i) * b[i], both mod 65521 (the sums a
// checksum started at (0, 0) would hold).  (a, b) -- started at (1, 0) -- takes the chunks in order.
DEFL_HD void adler_combine(uint32_t& a, uint32_t& b, uint32_t A, uint32_t B, int64_t len) {
    b = (uint32_t)(((uint64_t)b + (uint64_t)(len % ADLER_MOD) * a + B) % ADLER_MOD);
    a = (a + A) % ADLER_MOD;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host: the code builder
// ---------------------------------------------------------------------------------------------------------------------------
// An alphabet with fewer than two used symbols gets symbols 0 and 1 in (as zlib does): every code written is complete.
inline void deflate_two_symbols(uint64_t* cnt, int n) {
    int used = 0;
    for (int i = 0; i < n; ++i) used += cnt[i] != 0;
    for (int s = 0; s < 2 && used < 2; ++s)
        if (!cnt[s]) { cnt[s] = 1; ++used; }
}

// Code lengths of at most `limit` bits for the counts (at least two of them non-zero): a Huffman tree, then the lengths
// beyond the limit are cut to it and the Kraft sum is brought back to exactly 1 by lengthening the cheapest codes; the
// lengths go to the symbols by count, the longest to the rarest (ties: the higher symbol is the rarer).
inline void deflate_lengths(const uint64_t* cnt, int n, int limit, uint8_t* len) {
    std::vector<int> sym;
    for (int i = 0; i < n; ++i) {
        len[i] = 0;
        if (cnt[i]) sym.push_back(i);
    }
    const int m = (int)sym.size();
    if (m < 2) return;
    std::sort(sym.begin(), sym.end(), [&](int x, int y) { return cnt[x] != cnt[y] ? cnt[x] < cnt[y] : x > y; });
    std::vector<uint64_t> w(2 * m - 1);
    std::vector<int> parent(2 * m - 1, -1), depth(2 * m - 1, 0);
    for (int i = 0; i < m; ++i) w[i] = cnt[sym[i]];
    int leaf = 0, inner = m, nn = m;
    auto take = [&]() { return leaf < m && (inner >= nn || w[leaf] <= w[inner]) ? leaf++ : inner++; };
    while (nn < 2 * m - 1) {
        const int x = take(), y = take();
        w[nn] = w[x] + w[y];
        parent[x] = parent[y] = nn++;
    }
    std::vector<int> num(std::max(limit, 2 * m) + 1, 0);
    for (int i = 2 * m - 3; i >= 0; --i) {
        depth[i] = depth[parent[i]] + 1;
        if (i < m) ++num[std::min(depth[i], limit)];
    }
    uint64_t total = 0;
    for (int l = 1; l <= limit; ++l) total += (uint64_t)num[l] << (limit - l);
    while (total != (1ull << limit)) {
        --num[limit];
        for (int l = limit - 1; l > 0; --l)
            if (num[l]) { --num[l]; num[l + 1] += 2; break; }
        --total;
    }
    int j = m;
    for (int l = 1; l <= limit; ++l)
        for (int k = num[l]; k > 0; --k) len[sym[--j]] = (uint8_t)l;
}

// Canonical codes of the lengths (RFC 1951 3.2.2), each reversed over its own length.
inline void deflate_canonical(const uint8_t* len, int n, uint16_t* code_rev) {
    int count[16] = {0}, next[16] = {0};
    for (int i = 0; i < n; ++i) ++count[len[i]];
    count[0] = 0;
    for (int l = 1, code = 0; l < 16; ++l) {
        code = (code + count[l - 1]) << 1;
        next[l] = code;
    }
    for (int i = 0; i < n; ++i) {
        code_rev[i] = 0;
        if (!len[i]) continue;
        const int c = next[len[i]]++;
        int r = 0;
        for (int b = 0; b < len[i]; ++b) r |= ((c >> b) & 1) << (len[i] - 1 - b);
        code_rev[i] = (uint16_t)r;
    }
}

struct DeflateHdrWriter {
    uint32_t* words;
    uint32_t pos = 0;
    void put(uint32_t v, int n) { deflate_put(words, pos, v); pos += (uint32_t)n; }
};

// The code pair and the block header for a stream.  counts: the 286 literal / length counts (symbol 256 among them), then the 30
// distance counts; unused for the fixed code.
inline void deflate_build_codes(const uint64_t* counts, int huffman, DeflateCodes& c) {
    memset(&c, 0, sizeof c);
    DeflateHdrWriter hw{c.hdr};
    if (huffman == DEFLATE_FIXED) {
        for (int i = 0; i < 288; ++i) c.llen[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
        for (int i = 0; i < 32; ++i) c.dlen[i] = 5;
        deflate_canonical(c.llen, 288, c.lcode);
        deflate_canonical(c.dlen, 32, c.dcode);
        hw.put(0, 1);
        hw.put(1, 2);
        c.hdr_bits = hw.pos;
        return;
    }
    uint64_t lc[DEFLATE_NLIT], dc[DEFLATE_NDIST];
    memcpy(lc, counts, sizeof lc);
    memcpy(dc, counts + DEFLATE_NLIT, sizeof dc);
    if (!lc[DEFLATE_EOB]) lc[DEFLATE_EOB] = 1;
    deflate_two_symbols(lc, DEFLATE_NLIT);
    deflate_two_symbols(dc, DEFLATE_NDIST);
    deflate_lengths(lc, DEFLATE_NLIT, 15, c.llen);
    deflate_lengths(dc, DEFLATE_NDIST, 15, c.dlen);
    deflate_canonical(c.llen, DEFLATE_NLIT, c.lcode);
    deflate_canonical(c.dlen, DEFLATE_NDIST, c.dcode);
    int nl = DEFLATE_NLIT, nd = DEFLATE_NDIST;
    while (nl > 257 && !c.llen[nl - 1]) --nl;
    while (nd > 1 && !c.dlen[nd - 1]) --nd;
    // the code lengths as one sequence, run-length coded with 16 (repeat the last 3-6), 17 (3-10 zeros), 18 (11-138 zeros)
    std::vector<uint8_t> seq(c.llen, c.llen + nl);
    seq.insert(seq.end(), c.dlen, c.dlen + nd);
    struct Item { uint8_t sym, extra; };
    std::vector<Item> items;
    for (size_t i = 0; i < seq.size();) {
        size_t r = 1;
        while (i + r < seq.size() && seq[i + r] == seq[i]) ++r;
        const uint8_t v = seq[i];
        i += r;
        if (v) { items.push_back({v, 0}); --r; }
        while (r > 0) {
            if (!v && r >= 11) { const size_t t = std::min<size_t>(r, 138); items.push_back({18, (uint8_t)(t - 11)}); r -= t; }
            else if (!v && r >= 3) { items.push_back({17, (uint8_t)(r - 3)}); r = 0; }
            else if (v && r >= 3) { const size_t t = std::min<size_t>(r, 6); items.push_back({16, (uint8_t)(t - 3)}); r -= t; }
            else { items.push_back({v, 0}); --r; }
        }
    }
    uint64_t cc[19] = {0};
    for (const Item& it : items) ++cc[it.sym];
    deflate_two_symbols(cc, 19);
    uint8_t clen[19];
    uint16_t ccode[19];
    deflate_lengths(cc, 19, 7, clen);
    deflate_canonical(clen, 19, ccode);
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int ncl = 19;
    while (ncl > 4 && !clen[order[ncl - 1]]) --ncl;
    hw.put(0, 1);
    hw.put(2, 2);
    hw.put((uint32_t)(nl - 257), 5);
    hw.put((uint32_t)(nd - 1), 5);
    hw.put((uint32_t)(ncl - 4), 4);
    for (int i = 0; i < ncl; ++i) hw.put(clen[order[i]], 3);
    for (const Item& it : items) {
        hw.put(ccode[it.sym], clen[it.sym]);
        if (it.sym >= 16) hw.put(it.extra, it.sym == 16 ? 2 : it.sym == 17 ? 3 : 7);
    }
    c.hdr_bits = hw.pos;
}
