// The sequence census (include/besst_amd.h, BESST_CENSUS_*): what one byte string holds - bases by class, lower case, and its
// runs of 'N' - as 16 words of int64, and the rule that joins the census of two neighbouring strings into the census of
// their concatenation.  Shared by the kernels of seq_census.hip, the host entry besst_host_seq_census and the stand-alone
// test program tests/cpp/seq_census_core_test.cpp: plain C++, no HIP, no allocation.
//
// A census is PARTIAL until census_finalise: the run of 'N' that starts at byte 0 (PRE) and the one that ends at the last
// byte (SUF) are kept open, because a neighbour may continue them; only runs that touch neither end are closed into
// RUNS / GAPS / GAP_BASES / LONGEST.  A string that is all 'N' has PRE == SUF == LEN and no closed run.
#pragma once

#include <stdint.h>

#include "../../include/besst_amd.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CENSUS_HD __host__ __device__ inline
#else
#define CENSUS_HD inline
#endif

namespace besst_census {

constexpr int kWords = BESST_CENSUS_WORDS;

// the word a byte is counted in: BESST_CENSUS_A .. BESST_CENSUS_OTHER.  The five base classes and IUPAC are exactly the bytes
// the emit stage's complement table maps: A C G T N and YRKMBVHDSW in either case, X in upper case only.
CENSUS_HD int census_class(uint32_t byte) {
    const uint32_t up = byte & 0xDFu;                              // a letter in upper case (other bytes: something else)
    if (up < 'A' || up > 'Z' || byte > 0x7Fu) return BESST_CENSUS_OTHER;
    switch (up) {
        case 'A': return BESST_CENSUS_A;
        case 'C': return BESST_CENSUS_C;
        case 'G': return BESST_CENSUS_G;
        case 'T': return BESST_CENSUS_T;
        case 'N': return BESST_CENSUS_N;
        case 'X': return byte == 'X' ? BESST_CENSUS_IUPAC : BESST_CENSUS_OTHER;
        default: break;
    }
    // Y R K M B V H D S W
    const uint32_t iupac = (1u << ('Y' - 'A')) | (1u << ('R' - 'A')) | (1u << ('K' - 'A')) | (1u << ('M' - 'A')) |
                           (1u << ('B' - 'A')) | (1u << ('V' - 'A')) | (1u << ('H' - 'A')) | (1u << ('D' - 'A')) |
                           (1u << ('S' - 'A')) | (1u << ('W' - 'A'));
    return ((iupac >> (up - 'A')) & 1u) ? BESST_CENSUS_IUPAC : BESST_CENSUS_OTHER;
}

CENSUS_HD bool census_is_lower(uint32_t byte) { return byte >= 'a' && byte <= 'z'; }

CENSUS_HD void census_clear(int64_t* w) {
    for (int k = 0; k < kWords; ++k) w[k] = 0;
}

// a run of `length` 'N' that touches neither end of its string
CENSUS_HD void census_close_run(int64_t* w, int64_t length, int64_t min_gap) {
    w[BESST_CENSUS_RUNS] += 1;
    if (length >= min_gap) {
        w[BESST_CENSUS_GAPS] += 1;
        w[BESST_CENSUS_GAP_BASES] += length;
    }
    if (length > w[BESST_CENSUS_LONGEST]) w[BESST_CENSUS_LONGEST] = length;
}

// the census of the string with one more byte behind it
CENSUS_HD void census_push(int64_t* w, uint32_t byte, int64_t min_gap) {
    const int cls = census_class(byte);
    const int64_t before = w[BESST_CENSUS_LEN];
    w[BESST_CENSUS_LEN] = before + 1;
    w[cls] += 1;
    if (census_is_lower(byte)) w[BESST_CENSUS_LOWER] += 1;
    if (cls == BESST_CENSUS_N) {
        if (w[BESST_CENSUS_PRE] == before) w[BESST_CENSUS_PRE] += 1;           // still all 'N'
        w[BESST_CENSUS_SUF] += 1;
    } else {
        const int64_t open = w[BESST_CENSUS_SUF];
        if (open > 0 && open != before) census_close_run(w, open, min_gap);   // (open == before: that run is PRE)
        w[BESST_CENSUS_SUF] = 0;
    }
}

// out = the census of a·b from the census of a and of b (out may be a or b)
CENSUS_HD void census_merge(const int64_t* a, const int64_t* b, int64_t min_gap, int64_t* out) {
    if (b[BESST_CENSUS_LEN] == 0) {
        for (int k = 0; k < kWords; ++k) out[k] = a[k];
        return;
    }
    if (a[BESST_CENSUS_LEN] == 0) {
        for (int k = 0; k < kWords; ++k) out[k] = b[k];
        return;
    }
    const bool all_a = a[BESST_CENSUS_PRE] == a[BESST_CENSUS_LEN], all_b = b[BESST_CENSUS_PRE] == b[BESST_CENSUS_LEN];
    const int64_t joined = a[BESST_CENSUS_SUF] + b[BESST_CENSUS_PRE];
    const int64_t pre = all_a ? a[BESST_CENSUS_LEN] + b[BESST_CENSUS_PRE] : a[BESST_CENSUS_PRE];
    const int64_t suf = all_b ? a[BESST_CENSUS_SUF] + b[BESST_CENSUS_LEN] : b[BESST_CENSUS_SUF];
    const int64_t longest = a[BESST_CENSUS_LONGEST] > b[BESST_CENSUS_LONGEST] ? a[BESST_CENSUS_LONGEST] : b[BESST_CENSUS_LONGEST];
    for (int k = BESST_CENSUS_LEN; k <= BESST_CENSUS_LOWER; ++k) out[k] = a[k] + b[k];
    out[BESST_CENSUS_RUNS] = a[BESST_CENSUS_RUNS] + b[BESST_CENSUS_RUNS];
    out[BESST_CENSUS_GAPS] = a[BESST_CENSUS_GAPS] + b[BESST_CENSUS_GAPS];
    out[BESST_CENSUS_GAP_BASES] = a[BESST_CENSUS_GAP_BASES] + b[BESST_CENSUS_GAP_BASES];
    out[BESST_CENSUS_LONGEST] = longest;
    out[BESST_CENSUS_PRE] = pre;
    out[BESST_CENSUS_SUF] = suf;
    out[15] = 0;
    if (!all_a && !all_b && joined > 0) census_close_run(out, joined, min_gap);
}

// after the last merge: the runs at the ends are runs like any other
CENSUS_HD void census_finalise(int64_t* w, int64_t min_gap) {
    if (w[BESST_CENSUS_LEN] > 0 && w[BESST_CENSUS_PRE] == w[BESST_CENSUS_LEN]) {
        census_close_run(w, w[BESST_CENSUS_LEN], min_gap);
    } else {
        if (w[BESST_CENSUS_PRE] > 0) census_close_run(w, w[BESST_CENSUS_PRE], min_gap);
        if (w[BESST_CENSUS_SUF] > 0) census_close_run(w, w[BESST_CENSUS_SUF], min_gap);
    }
    w[BESST_CENSUS_PRE] = w[BESST_CENSUS_SUF] = 0;
}

// Row i of an ascending, disjoint table: false if it lies in front of its predecessor's end or has a negative field.
CENSUS_HD bool census_row_in_order(const int64_t* seq_off, const int64_t* seq_len, int64_t i) {
    if (seq_off[i] < 0 || seq_len[i] < 0) return false;
    if (i == 0) return true;
    const int64_t prev_len = seq_len[i - 1] < 0 ? 0 : seq_len[i - 1];
    return seq_off[i] >= seq_off[i - 1] + prev_len;
}

// the last row whose offset is <= pos (0 if there is none): where the walk over the rows of a window begins
CENSUS_HD int64_t census_first_row(const int64_t* seq_off, int64_t n_seq, int64_t pos) {
    int64_t lo = 0, hi = n_seq;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (seq_off[mid] <= pos) lo = mid + 1; else hi = mid;
    }
    return lo > 0 ? lo - 1 : 0;
}

}  // namespace besst_census
