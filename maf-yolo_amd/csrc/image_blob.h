// The host-side checks the blob entry points share (maf_jpeg_decode, maf_png_decode, maf_jpeg_encode; maf-yolo_amd/staging.py builds what
// they read): a blob is a header record followed by sections at 16-byte-aligned offsets the header names, and it travels twice, as the
// host copy the entry point validates and as the device copy the kernels read.  Host only and free of HIP: plain C++.  A new codec or
// resizer starts here and in staging.py.
#pragma once
#include <cstdint>
#include <cstring>
#include <initializer_list>

// a section of `bytes` at byte offset `off` (16-byte aligned) inside a blob of `total` bytes
inline bool in_blob(int64_t off, int64_t bytes, int64_t total) { return off >= 0 && (off & 15) == 0 && bytes >= 0 && off <= total && bytes <= total - off; }

// every pointer of the list on a multiple of `a` bytes (a power of two)
inline bool maf_aligned(std::initializer_list<const void*> ptrs, uintptr_t a = 16) {
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & (a - 1)) return false;
    return true;
}

// the header record at the start of the host copy of a blob
template <typename Header>
inline Header maf_blob_header(const void* blob_host) {
    Header hd;
    std::memcpy(&hd, blob_host, sizeof(Header));
    return hd;
}

// the two range checks of every blob: 1 to 65535 images (files, jobs) per call, and a size below 2 GiB
inline bool maf_blob_count_ok(int64_t n) { return n > 0 && n <= 65535; }
inline bool maf_blob_size_ok(int64_t total) { return total > 0 && total < ((int64_t)1 << 31); }
