// CPU harness for the device PNG encoder: csrc/svgr_png.h and csrc/svgr_deflate.h driven serially on the host -- one loop
// iteration where the kernels of svgr_hip.hip have one lane, one pass over a chunk where they have one workgroup.  The
// arithmetic, the token rule and the code builder are the headers' own, so the stream this writes is the device's bit for bit.
// tests/test_png_encode_host.py holds it against tests/png_enc_ref.py and zlib; with -DPNG_ENC_HARNESS_MAIN it is a stand-alone
// program (for a run under a sanitizer).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../svgrasterize.py_amd/csrc/svgr_deflate.h"
#include "../svgrasterize.py_amd/csrc/svgr_png.h"

namespace {

// k_deflate_tokens: the tokens of the chunk that begins at `start`, appended to tok; the chunk's Adler pair
void chunk_tokens(const uint8_t* src, int64_t n, int64_t start, std::vector<uint32_t>& tok, uint32_t& A, uint32_t& B) {
    const int64_t end = deflate_chunk_end(start, n), base = start - DEFLATE_WINDOW;   // (an empty input has one empty chunk)
    const int len = (int)(end - start);
    std::vector<int64_t> table((size_t)1 << DEFLATE_HASH_BITS, -1), cand((size_t)len, -1);
    for (int64_t q = base > 0 ? base : 0; q < start; ++q)
        if (deflate_hashed(q, n)) {
            int64_t& e = table[deflate_hash3(src + q)];
            if (q > e) e = q;
        }
    for (int w = 0; w < len; w += DEFLATE_SUB) {
        const int w1 = w + DEFLATE_SUB < len ? w + DEFLATE_SUB : len;
        for (int i = w; i < w1; ++i)
            if (start + i + 2 < end) cand[(size_t)i] = table[deflate_hash3(src + start + i)];
        for (int i = w; i < w1; ++i)
            if (start + i + 2 < end) {
                int64_t& e = table[deflate_hash3(src + start + i)];
                if (start + i > e) e = start + i;
            }
    }
    uint64_t a = 0, b = 0;
    for (int i = 0; i < len; ++i) {
        a += src[start + i];
        b += (uint64_t)(len - i) * src[start + i];
    }
    A = (uint32_t)(a % ADLER_MOD);
    B = (uint32_t)(b % ADLER_MOD);
    for (int i = 0; i < len;) {
        const uint32_t t = deflate_best(src, start + i, end, cand[(size_t)i]);
        tok.push_back(t);
        i += deflate_tok_hop(t);
    }
}

// k_deflate_emit: one chunk's bytes, appended to out
void chunk_emit(const DeflateCodes& c, const uint32_t* tok, size_t n_tok, bool last, std::vector<uint8_t>& out) {
    std::vector<uint32_t> words(DEFLATE_SLOT / 4, 0);
    for (uint32_t i = 0; i < (c.hdr_bits + 31) / 32; ++i) words[i] |= c.hdr[i];
    if (last) words[0] |= 1u;
    uint32_t pos = c.hdr_bits;
    for (size_t i = 0; i < n_tok; ++i) {
        uint64_t v;
        const int nb = deflate_token_bits(c.lcode, c.llen, c.dcode, c.dlen, tok[i], v);
        deflate_put(words.data(), pos, v);
        pos += (uint32_t)nb;
    }
    const uint32_t nbytes = deflate_chunk_tail(words.data(), pos, c.lcode[DEFLATE_EOB], c.llen[DEFLATE_EOB], last);
    const uint8_t* p = (const uint8_t*)words.data();   // (little-endian words: byte k of the stream is byte k of the array)
    out.insert(out.end(), p, p + nbytes);
}

}  // namespace

extern "C" {

int h_deflate_chunk(void) { return DEFLATE_CH; }
int h_codes_size(void) { return (int)sizeof(DeflateCodes); }

// svgr_png_filter, serially
void h_png_filter(const uint8_t* rgba, int64_t rows, int64_t cols, int mode, uint8_t* out) {
    std::vector<uint32_t> px((size_t)(rows * cols));
    memcpy(px.data(), rgba, px.size() * 4);
    for (int64_t r = 0; r < rows; ++r) {
        int type = mode;
        if (mode == PNG_FILTER_ADAPTIVE) {
            uint32_t sums[PNG_FILTER_TYPES] = {0, 0, 0, 0, 0};
            for (int64_t x = 0; x < cols; ++x) {
                uint32_t p, a, b, c;
                png_neighbours(px.data(), r, cols, x, p, a, b, c);
                for (int t = 0; t < PNG_FILTER_TYPES; ++t) sums[t] += png_cost_px(png_filter_px(t, p, a, b, c));
            }
            type = png_pick(sums);
        }
        uint8_t* o = out + r * (1 + 4 * cols);
        o[0] = (uint8_t)type;
        for (int64_t x = 0; x < cols; ++x) {
            uint32_t p, a, b, c;
            png_neighbours(px.data(), r, cols, x, p, a, b, c);
            png_store_px(o, x, png_filter_px(type, p, a, b, c));
        }
    }
}
int h_paeth(int a, int b, int c) { return png_paeth(a, b, c); }
void h_row_sums(const uint8_t* rgba, int64_t rows, int64_t cols, int64_t r, uint32_t* sums) {
    std::vector<uint32_t> px((size_t)(rows * cols));
    memcpy(px.data(), rgba, px.size() * 4);
    for (int t = 0; t < PNG_FILTER_TYPES; ++t) sums[t] = 0;
    for (int64_t x = 0; x < cols; ++x) {
        uint32_t p, a, b, c;
        png_neighbours(px.data(), r, cols, x, p, a, b, c);
        for (int t = 0; t < PNG_FILTER_TYPES; ++t) sums[t] += png_cost_px(png_filter_px(t, p, a, b, c));
    }
}

void h_len_sym(int len, int* out3) { deflate_len_sym(len, out3[0], out3[1], out3[2]); }
void h_dist_sym(int dist, int* out3) { deflate_dist_sym(dist, out3[0], out3[1], out3[2]); }
void h_lengths(const uint64_t* cnt, int n, int limit, uint8_t* len) { deflate_lengths(cnt, n, limit, len); }
void h_build_codes(const uint64_t* counts, int huffman, DeflateCodes* c) { deflate_build_codes(counts, huffman, *c); }
void h_adler_combine(uint32_t* ab, uint32_t A, uint32_t B, int64_t len) { adler_combine(ab[0], ab[1], A, B, len); }

// svgr_deflate, serially.  Also the flat token list (tok_cap entries of room; *n_tok receives the count) and the symbol counts.
// Returns 0, or 5 when out_cap is short (*n_out receives the length in both cases).
int h_deflate(const uint8_t* src, int64_t n, int huffman, uint8_t* out, int64_t out_cap, int64_t* n_out, uint32_t* tok_out,
              int64_t tok_cap, int64_t* n_tok, uint64_t* counts_out) {
    const int64_t nc = n ? (n + DEFLATE_CH - 1) / DEFLATE_CH : 1;
    std::vector<uint32_t> tok;
    std::vector<size_t> first((size_t)nc + 1, 0);
    uint32_t s1 = 1, s2 = 0;
    for (int64_t k = 0; k < nc; ++k) {
        uint32_t A, B;
        chunk_tokens(src, n, k * DEFLATE_CH, tok, A, B);
        first[(size_t)k + 1] = tok.size();
        const int64_t len = n - k * DEFLATE_CH < DEFLATE_CH ? n - k * DEFLATE_CH : DEFLATE_CH;
        adler_combine(s1, s2, A, B, len);
    }
    uint64_t counts[DEFLATE_NSYM] = {0};
    counts[DEFLATE_EOB] = (uint64_t)nc;
    for (uint32_t t : tok) {
        int ls, ds;
        deflate_token_syms(t, ls, ds);
        ++counts[ls];
        if (ds >= 0) ++counts[DEFLATE_NLIT + ds];
    }
    if (counts_out) memcpy(counts_out, counts, sizeof counts);
    DeflateCodes c;
    deflate_build_codes(counts, huffman, c);
    std::vector<uint8_t> z = {0x78, 0x01};
    for (int64_t k = 0; k < nc; ++k) chunk_emit(c, tok.data() + first[(size_t)k], first[(size_t)k + 1] - first[(size_t)k], k == nc - 1, z);
    const uint32_t ad = (s2 << 16) | s1;
    for (int sh = 24; sh >= 0; sh -= 8) z.push_back((uint8_t)(ad >> sh));
    if (n_tok) *n_tok = (int64_t)tok.size();
    if (tok_out)
        for (size_t i = 0; i < tok.size() && (int64_t)i < tok_cap; ++i) tok_out[i] = tok[i];
    *n_out = (int64_t)z.size();
    if ((int64_t)z.size() > out_cap) return 5;
    memcpy(out, z.data(), z.size());
    return 0;
}

}  // extern "C"

#ifdef PNG_ENC_HARNESS_MAIN
// A few streams and a filtered image, for a run under a sanitizer: prints the lengths.
int main() {
    const int64_t sizes[] = {0, 1, 2, 3, 257, 258, 259, 260, 517, DEFLATE_CH - 1, DEFLATE_CH, DEFLATE_CH + 1, 2 * DEFLATE_CH + 5, 2 * 32769};
    for (int64_t n : sizes)
        for (int kind = 0; kind < 3; ++kind) {
            std::vector<uint8_t> src((size_t)n), out((size_t)(2 * n + 1024));
            uint32_t x = 12345;
            for (int64_t i = 0; i < n; ++i) {
                x = x * 1664525u + 1013904223u;
                src[(size_t)i] = kind == 0 ? 0 : kind == 1 ? (uint8_t)(x >> 24) : (uint8_t)((i % 32769) * 7 >> 3);
            }
            for (int huffman = 0; huffman < 2; ++huffman) {
                int64_t n_out = 0, n_tok = 0;
                const int rc = h_deflate(src.data(), n, huffman, out.data(), (int64_t)out.size(), &n_out, nullptr, 0, &n_tok, nullptr);
                printf("n %lld kind %d huffman %d: status %d, %lld bytes, %lld tokens\n", (long long)n, kind, huffman, rc, (long long)n_out, (long long)n_tok);
                if (rc) return 1;
            }
        }
    const int64_t rows = 7, cols = 301;
    std::vector<uint8_t> img((size_t)(rows * cols * 4)), f((size_t)(rows * (1 + 4 * cols)));
    for (size_t i = 0; i < img.size(); ++i) img[i] = (uint8_t)(i * 31 >> 4);
    for (int mode = 0; mode <= PNG_FILTER_ADAPTIVE; ++mode) h_png_filter(img.data(), rows, cols, mode, f.data());
    printf("filters ok\n");
    return 0;
}
#endif
