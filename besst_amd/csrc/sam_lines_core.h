// The line cutter's sequential rule (besst_dev_sam_lines, csrc/sam.hip), compilable on the host
// (tests/cpp/sam_lines_core_test.cpp runs it lane after lane): what one 16-byte slice of a text adds to the three answers
//
//   last_end    the offset behind the last '\n' of text[0, n)                                   (0: none)
//   first_rec   the smallest line start whose byte is not '@'                                   (kNone: none)
//               a line start is byte 0 and every byte behind a '\n' that lies inside the text; where the text's last
//               byte is a '\n' the place behind it, n, stands in with the lowest rank: every line is a header line and
//               the last one is complete
//   newlines    the '\n' of text[0, count_upto)
//
// A slice needs one fact from outside: whether the byte in front of it is a '\n' (or the slice is the text's first).
// Offsets are 32 bits: a text is below 2^32 - 16 bytes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BESST_LINES_HD __host__ __device__ __forceinline__
#else
#define BESST_LINES_HD inline
#endif

namespace besst_sam_lines {

constexpr uint32_t kNone = 0xffffffffu;

struct Slice {
    uint32_t nl, not_at, valid;                                  // 16-bit masks over the slice's bytes; bytes behind n are in none
};

struct Acc {
    uint32_t last_end, first_rec, newlines;
};

// the highest / the lowest set bit of a mask that is not 0, and the number of its bits
BESST_LINES_HD int top_bit(uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return 31 - __clz((int)m);
#else
    int k = 31;
    while (!((m >> k) & 1u)) --k;
    return k;
#endif
}
BESST_LINES_HD int low_bit(uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffs((int)m) - 1;
#else
    int k = 0;
    while (!((m >> k) & 1u)) ++k;
    return k;
#endif
}
BESST_LINES_HD uint32_t bit_count(uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(m);
#else
    uint32_t c = 0;
    for (; m; m &= m - 1u) ++c;
    return c;
#endif
}

BESST_LINES_HD Acc acc_none() { return Acc{0u, kNone, 0u}; }

// the masks of the 16 bytes in w (little endian, as loaded) of which `left` > 0 lie inside the text
BESST_LINES_HD Slice slice_masks(const uint32_t w[4], int64_t left) {
    Slice s{0u, 0u, 0u};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 16; ++k) {
        const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
        s.nl |= (uint32_t)(c == 10u) << k;
        s.not_at |= (uint32_t)(c != 64u) << k;
    }
    s.valid = left >= 16 ? 0xffffu : (1u << (int)left) - 1u;
    s.nl &= s.valid;
    s.not_at &= s.valid;
    return s;
}

// the slice at offset `off` of a text of n bytes; before: the byte in front of it is a '\n', or off == 0
BESST_LINES_HD void acc_slice(Acc& a, const Slice& s, uint32_t before, int64_t off, int64_t n, int64_t count_upto,
                              bool want_header_end) {
    if (s.nl) {
        const uint32_t end = (uint32_t)(off + top_bit(s.nl) + 1);
        if (end > a.last_end) a.last_end = end;
    }
    if (want_header_end) {
        const uint32_t starts = ((s.nl << 1) | (before & 1u)) & s.valid;
        const uint32_t cand = starts & s.not_at;
        if (cand) {
            const uint32_t at = (uint32_t)(off + low_bit(cand));
            if (at < a.first_rec) a.first_rec = at;
        }
        const int64_t last = n - 1 - off;                        // the text's last byte, where this slice holds it
        if (last >= 0 && last < 16 && ((s.nl >> (int)last) & 1u) && (uint32_t)n < a.first_rec) a.first_rec = (uint32_t)n;
    }
    const int64_t room = count_upto - off;
    if (room > 0) a.newlines += bit_count(s.nl & (room >= 16 ? 0xffffu : (1u << (int)room) - 1u));
}

// two parts of a text as one (in any order)
BESST_LINES_HD void acc_join(Acc& a, const Acc& b) {
    if (b.last_end > a.last_end) a.last_end = b.last_end;
    if (b.first_rec < a.first_rec) a.first_rec = b.first_rec;
    a.newlines += b.newlines;
}

}  // namespace besst_sam_lines
