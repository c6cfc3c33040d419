// svgr_blob.h -- several arrays in one block: where each lies (Layout), and a host copy to upload in one piece (HostBlob).
// Host only, plain C++ (tests/blob_harness.cpp drives it on the CPU).  An entry of svgr_hip.hip that hands the device arrays of
// its caller states each array ONCE, with its element type and count -- `params = blob.put(seg_params, (size_t)n * 8)` -- and the
// kernel's view of it is `params.on(d_in)`, a const double*: the copy's size, the offset and the device pointer's type all come
// from the section, so they cannot disagree.  Sections are handed out in call order, each at the next multiple of 64 bytes; all
// arithmetic is size_t.  A Layout alone describes a block without a host side (device scratch, a result before its download).
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

inline size_t pad64(size_t bytes) { return (bytes + 63) & ~(size_t)63; }

// `n` elements of T at byte `off` of some block; `on(base)` is the array in the block that begins at `base` (host or device).
template <class T>
struct Section {
    size_t off = 0, n = 0;
    T* on(void* base) const { return (T*)((char*)base + off); }
    const T* on(const void* base) const { return (const T*)((const char*)base + off); }
};

struct Layout {
    size_t at = 0;
    template <class T>
    Section<T> take(size_t n) {
        const Section<T> s{at, n};
        at += pad64(n * sizeof(T));
        return s;
    }
    size_t bytes() const { return at; }   // the padded total
};

struct HostBlob {
    Layout lay;
    std::vector<char> mem;   // (the padding between the sections is zero)
    bool sizing = false;     // build()'s first pass: sections are handed out, nothing is stored
    // One allocation of exactly the sections' size, the way Carver lays out device arrays: `fill(blob)` states them -- put /
    // reserve -- and runs twice, first to add them up, then to copy.  (Without build() the blob grows with every section.)
    template <class Fill>
    void build(Fill&& fill) {
        sizing = true;
        fill(*this);
        mem.assign(lay.bytes(), 0);
        lay = Layout{};
        sizing = false;
        fill(*this);
    }
    // a section to fill in place: `host` is valid until the next put / reserve, and null in build()'s first pass
    template <class T>
    Section<T> reserve(size_t n, T*& host) {
        const Section<T> s = lay.take<T>(n);
        if (!sizing && mem.size() < lay.bytes()) mem.resize(lay.bytes());
        host = sizing ? nullptr : s.on((void*)mem.data());
        return s;
    }
    // a section holding a copy of src[0 .. n); with n == 0 `src` is not touched and may be null
    template <class T>
    Section<T> put(const T* src, size_t n) {
        T* host;
        const Section<T> s = reserve<T>(n, host);
        if (n && host) memcpy(host, src, n * sizeof(T));
        return s;
    }
    const char* data() const { return mem.data(); }
    size_t bytes() const { return mem.size(); }
};
