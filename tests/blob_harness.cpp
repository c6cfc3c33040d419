// blob_harness.cpp -- the layout / blob builder (csrc/svgr_blob.h) driven from tests/test_blob_host.py: a list of arrays, each
// given by element size and count, goes into a Layout and into a HostBlob in order, and the offsets, the total and the bytes
// come back; directly, or through HostBlob::build's two passes.  With -DBLOB_HARNESS_MAIN it is a program of its own (for a run under the host sanitizers).
#include <cstdint>
#include <cstdio>

#include "../svgrasterize.py_amd/csrc/svgr_blob.h"

namespace {
struct Elem48 { double v[6]; };   // (a part's matrix: the one element of the entries that is no scalar)

// one array into the blob: put (mode 0) or reserve and fill in place with the bytes of `src` (mode 1); returns its offset
template <class T>
size_t add(HostBlob& blob, const void* src, size_t n, int mode, size_t& count_back) {
    Section<T> s;
    if (mode == 0) {
        s = blob.put((const T*)src, n);
    } else {
        T* host = nullptr;
        s = blob.reserve<T>(n, host);
        for (size_t i = 0; host && i < n; ++i) host[i] = ((const T*)src)[i];   // (null in build()'s sizing pass)
    }
    count_back = s.n;
    // the typed views of the section agree with its offset
    if ((const char*)s.on((const void*)blob.data()) != blob.data() + s.off) return (size_t)-1;
    return s.off;
}
template <class T>
size_t take(Layout& lay, size_t n) { return lay.take<T>(n).off; }
}  // namespace

extern "C" {

long long bh_pad64(long long bytes) { return (long long)pad64((size_t)bytes); }

// k sections of a Layout: off[i], returns bytes(); -1 for an element size the harness does not know
long long bh_layout(int k, const int* elem, const long long* count, long long* off) {
    Layout lay;
    for (int i = 0; i < k; ++i) {
        const size_t n = (size_t)count[i];
        switch (elem[i]) {
            case 1: off[i] = (long long)take<uint8_t>(lay, n); break;
            case 2: off[i] = (long long)take<int16_t>(lay, n); break;
            case 4: off[i] = (long long)take<int32_t>(lay, n); break;
            case 8: off[i] = (long long)take<double>(lay, n); break;
            case 48: off[i] = (long long)take<Elem48>(lay, n); break;
            default: return -1;
        }
    }
    return (long long)lay.bytes();
}

// k arrays into a HostBlob (mode[i]: 0 put, 1 reserve + fill), one after the other or, with `built`, through build(): off[i],
// the blob's bytes into out[0 .. out_cap), returns bytes(); the allocation's capacity to *capacity
long long bh_blob(int k, const void* const* src, const int* elem, const long long* count, const int* mode, int built, long long* off,
                  unsigned char* out, long long out_cap, long long* capacity) {
    HostBlob blob;
    long long status = 0;
    auto fill = [&](HostBlob& b) {
        for (int i = 0; i < k && status == 0; ++i) {
            const size_t n = (size_t)count[i];
            size_t back = 0, o = 0;
            switch (elem[i]) {
                case 1: o = add<uint8_t>(b, src[i], n, mode[i], back); break;
                case 2: o = add<int16_t>(b, src[i], n, mode[i], back); break;
                case 4: o = add<int32_t>(b, src[i], n, mode[i], back); break;
                case 8: o = add<double>(b, src[i], n, mode[i], back); break;
                case 48: o = add<Elem48>(b, src[i], n, mode[i], back); break;
                default: status = -1; return;
            }
            if (o == (size_t)-1 || back != n) status = -2;
            off[i] = (long long)o;
        }
    };
    if (built) blob.build(fill);
    else fill(blob);
    if (status) return status;
    if (blob.bytes() != blob.lay.bytes() || blob.sizing) return -3;
    if (capacity) *capacity = (long long)blob.mem.capacity();
    for (size_t i = 0; i < blob.bytes() && (long long)i < out_cap; ++i) out[i] = (unsigned char)blob.data()[i];
    return (long long)blob.bytes();
}

}  // extern "C"

#ifdef BLOB_HARNESS_MAIN
// the shapes of tests/test_blob_host.py once more, so that the sanitizers see every path: an empty blob, null sources with no
// elements, odd sizes, a reserve between two puts, and the twelve arrays of the TrueType outline pass
int main() {
    alignas(64) static unsigned char bytes[65536];
    static unsigned char out[1 << 20];
    for (size_t i = 0; i < sizeof bytes; ++i) bytes[i] = (unsigned char)(i * 37 + 11);
    long long off[12];
    for (int built = 0; built < 2; ++built) {
    if (bh_blob(0, nullptr, nullptr, nullptr, nullptr, built, off, out, sizeof out, nullptr) != 0) return 1;
    {
        const void* src[4] = {nullptr, bytes, nullptr, bytes};
        const int elem[4] = {8, 1, 4, 2}, mode[4] = {0, 0, 0, 1};
        const long long count[4] = {0, 65, 0, 33};
        if (bh_blob(4, src, elem, count, mode, built, off, out, sizeof out, nullptr) != 128 + 128) return 2;
        if (off[0] != 0 || off[1] != 0 || off[2] != 128 || off[3] != 128) return 3;
    }
    {
        const long long npt = 65, nc = 3, ng = 2, np = 5;
        const void* src[12];
        for (auto& p : src) p = bytes;
        const int elem[12] = {2, 1, 4, 4, 4, 4, 4, 4, 48, 8, 8, 8}, mode[12] = {0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0};
        const long long count[12] = {npt * 2, npt, npt, nc + 1, ng + 1, np, np + 1, np + 1, np, np, np, np};
        long long cap = 0;
        const long long total = bh_blob(12, src, elem, count, mode, built, off, out, sizeof out, &cap);
        if (built && cap != total) return 6;
        long long lay_off[12];
        if (total != bh_layout(12, elem, count, lay_off)) return 4;
        for (int i = 0; i < 12; ++i)
            if (off[i] != lay_off[i] || off[i] % 64) return 5;
    }
    }
    std::puts("blob harness: ok");
    return 0;
}
#endif
