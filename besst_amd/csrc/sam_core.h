// The per-record rules of the SAM text reader, shared by the device kernels (sam.hip) and host programs
// (tests/cpp/sam_core_test.cpp): the number parsers, the CIGAR walk over text, the hash of a reference name and the
// probe of the reference table.  Every function takes a byte pointer and bounds; nothing here allocates or keeps state.
//
// A record is the first eleven tab-separated fields of a line.  Fields 2-9 (FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN)
// are decoded by sam_decode_fields from the bytes between tab 1 and tab 9; l_seq is the length of field 10 ('*': 0).
// qlen / alen / rlen follow pysam 0.8.4's AlignedRead properties, the rules of bam_reader.hip's record decode:
//   qlen = (l_seq, or the M/I/S/=/X total without a sequence) - leading soft clips (hard clips in front of them skipped)
//          - trailing soft clips (found without ever looking at the first operation), floored at 0, saturated at 65535
//   alen = the M/D/N/=/X total, rlen = l_seq.  CIGAR '*': no operations.  The optional fields are never read.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SAM_HD __host__ __device__ inline
#else
#define SAM_HD inline
#endif

namespace besst_sam {

// reason codes of a line that cannot be read (0: the line is fine)
enum Reason : uint32_t {
    kOk = 0,
    kFewFields = 1,      // fewer than eleven fields
    kEmptyLine = 2,
    kHeaderLine = 3,     // a line beginning with '@' behind the first record
    kBadFlag = 4,        // a numeric field that is empty, holds a non-digit or is out of range
    kBadPos = 5,
    kBadMapq = 6,
    kBadPnext = 7,
    kBadTlen = 8,
    kBadRname = 9,       // RNAME / RNEXT not among the references
    kBadRnext = 10,
    kBadCigar = 11,      // an operation without a count, a letter outside MIDNSHP=X, a count >= 2^28
    kReasons = 12
};

constexpr uint32_t kCigarCountLimit = 1u << 28;
constexpr uint32_t kNoOffset = 0xffffffffu;

struct Record {
    int32_t tid, mtid, pos, mpos, tlen;
    uint16_t flag, qlen;
    uint8_t mapq;
    int32_t rlen, alen;
    uint32_t saturated;   // 1: the aligned query length was above 65535 and is stored as 65535
};

// The reference table: open addressing over `cap` slots (a power of two >= 2 n_ref; 0 with no reference), a slot holds
// row + 1 (0: empty); the names lie end to end in `pool`, name r at pool[off[r]] .. pool[off[r + 1]].
struct RefTable {
    const uint32_t* slots;
    uint32_t cap;
    const uint8_t* pool;
    const int64_t* off;
};

// [0-9]+ with a value <= limit -> true and *out
SAM_HD bool parse_unsigned(const uint8_t* p, int64_t b, int64_t e, uint64_t limit, uint64_t* out) {
    if (b >= e) return false;
    uint64_t v = 0;
    for (int64_t i = b; i < e; ++i) {
        const uint32_t d = (uint32_t)p[i] - (uint32_t)'0';
        if (d > 9u) return false;
        v = v * 10u + d;
        if (v > limit) v = limit + 1;                            // stays out of range, never wraps
    }
    if (v > limit) return false;
    *out = v;
    return true;
}

// -?[0-9]+ within int32
SAM_HD bool parse_int32(const uint8_t* p, int64_t b, int64_t e, int32_t* out) {
    const bool neg = b < e && p[b] == (uint8_t)'-';
    uint64_t v;
    if (!parse_unsigned(p, neg ? b + 1 : b, e, neg ? 2147483648ull : 2147483647ull, &v)) return false;
    *out = neg ? (int32_t)(-(int64_t)v) : (int32_t)v;
    return true;
}

// M=0 I=1 D=2 N=3 S=4 H=5 P=6 '='=7 X=8, anything else 9
SAM_HD uint32_t cigar_op(uint32_t c) {
    switch (c) {
        case 'M': return 0;
        case 'I': return 1;
        case 'D': return 2;
        case 'N': return 3;
        case 'S': return 4;
        case 'H': return 5;
        case 'P': return 6;
        case '=': return 7;
        case 'X': return 8;
        default: return 9;
    }
}

// The CIGAR field [b, e) -> false: malformed.  One forward walk: `trail` is the soft-clipped total of the run of S / H
// operations the CIGAR ends with, the first operation left out - what the backward walk of bam_reader.hip (from the last
// operation down to the second, S adds, H passes, anything else stops) arrives at.
SAM_HD bool walk_cigar(const uint8_t* p, int64_t b, int64_t e, int64_t* q_total, int64_t* ref_len, int64_t* lead,
                       int64_t* trail) {
    *q_total = *ref_len = *lead = *trail = 0;
    if (e - b == 1 && p[b] == (uint8_t)'*') return true;
    if (b >= e) return false;
    bool in_lead = true, first = true;
    int64_t i = b;
    while (i < e) {
        uint64_t len = 0;
        const int64_t d0 = i;
        while (i < e && (uint32_t)p[i] - (uint32_t)'0' <= 9u) {
            len = len * 10u + ((uint32_t)p[i] - (uint32_t)'0');
            if (len >= kCigarCountLimit) len = kCigarCountLimit;
            ++i;
        }
        if (i == d0 || i >= e || len >= kCigarCountLimit) return false;      // no count, no operation, count too large
        const uint32_t op = cigar_op(p[i++]);
        if (op > 8u) return false;
        if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) *q_total += (int64_t)len;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) *ref_len += (int64_t)len;
        if (in_lead) {
            if (op == 4) *lead += (int64_t)len;
            else if (op != 5) in_lead = false;
        }
        if (!first) {
            if (op == 4) *trail += (int64_t)len;
            else if (op != 5) *trail = 0;
        }
        first = false;
    }
    return true;
}

// FNV-1a over the name's bytes
SAM_HD uint32_t name_hash(const uint8_t* p, int64_t b, int64_t e) {
    uint32_t h = 2166136261u;
    for (int64_t i = b; i < e; ++i) h = (h ^ p[i]) * 16777619u;
    return h;
}

// the row of the name [b, e) or -1: a slot counts only when the bytes are the pool's
SAM_HD int32_t lookup_name(const RefTable& t, const uint8_t* p, int64_t b, int64_t e) {
    if (t.cap == 0) return -1;
    const uint32_t mask = t.cap - 1u;
    uint32_t at = name_hash(p, b, e) & mask;
    for (uint32_t probes = 0; probes < t.cap; ++probes, at = (at + 1u) & mask) {
        const uint32_t s = t.slots[at];
        if (s == 0u) return -1;
        const int64_t o = t.off[s - 1u], len = t.off[s] - o;
        if (len != e - b) continue;
        int64_t k = 0;
        while (k < len && t.pool[o + k] == p[b + k]) ++k;
        if (k == len) return (int32_t)(s - 1u);
    }
    return -1;
}

// the end of the field that begins at b: the next tab in front of e, or e
SAM_HD int64_t field_end(const uint8_t* p, int64_t b, int64_t e) {
    while (b < e && p[b] != (uint8_t)'\t') ++b;
    return b;
}

// Fields 2-9 of a record, the bytes [b, e) between tab 1 and tab 9 (eight fields, seven tabs between them), with l_seq
// already known -> the reason the line cannot be read, fields tested in file order, or kOk and *r filled in.
SAM_HD uint32_t sam_decode_fields(const uint8_t* p, int64_t b, int64_t e, uint32_t l_seq, const RefTable& t, Record* r) {
    uint64_t v;
    int64_t f = b, g = field_end(p, f, e);                       // FLAG
    if (!parse_unsigned(p, f, g, 65535u, &v)) return kBadFlag;
    r->flag = (uint16_t)v;
    f = g + 1; g = field_end(p, f, e);                           // RNAME
    if (f > e) return kFewFields;
    if (g - f == 1 && p[f] == (uint8_t)'*') r->tid = -1;
    else if ((r->tid = lookup_name(t, p, f, g)) < 0) return kBadRname;
    f = g + 1; g = field_end(p, f, e);                           // POS
    if (f > e) return kFewFields;
    if (!parse_unsigned(p, f, g, 2147483647u, &v)) return kBadPos;
    r->pos = (int32_t)v - 1;
    f = g + 1; g = field_end(p, f, e);                           // MAPQ
    if (f > e) return kFewFields;
    if (!parse_unsigned(p, f, g, 255u, &v)) return kBadMapq;
    r->mapq = (uint8_t)v;
    f = g + 1; g = field_end(p, f, e);                           // CIGAR
    if (f > e) return kFewFields;
    int64_t q_total, ref_len, lead, trail;
    if (!walk_cigar(p, f, g, &q_total, &ref_len, &lead, &trail)) return kBadCigar;
    f = g + 1; g = field_end(p, f, e);                           // RNEXT
    if (f > e) return kFewFields;
    if (g - f == 1 && p[f] == (uint8_t)'=') r->mtid = r->tid;
    else if (g - f == 1 && p[f] == (uint8_t)'*') r->mtid = -1;
    else if ((r->mtid = lookup_name(t, p, f, g)) < 0) return kBadRnext;
    f = g + 1; g = field_end(p, f, e);                           // PNEXT
    if (f > e) return kFewFields;
    if (!parse_unsigned(p, f, g, 2147483647u, &v)) return kBadPnext;
    r->mpos = (int32_t)v - 1;
    f = g + 1; g = field_end(p, f, e);                           // TLEN
    if (f > e) return kFewFields;
    if (g != e || !parse_int32(p, f, g, &r->tlen)) return kBadTlen;
    int64_t q_aln = (l_seq ? (int64_t)l_seq : q_total) - lead - trail;
    if (q_aln < 0) q_aln = 0;
    r->saturated = q_aln > 65535 ? 1u : 0u;
    if (q_aln > 65535) q_aln = 65535;
    r->qlen = (uint16_t)q_aln;
    r->rlen = (int32_t)l_seq;
    r->alen = (int32_t)ref_len;
    return kOk;
}

// A whole line [s, e) (the terminator left out) whose tabs 1, 9 and 10 were found (kNoOffset: the line has none): the
// reason it cannot be read, or kOk and *r.
SAM_HD uint32_t sam_decode_line(const uint8_t* p, int64_t s, int64_t e, uint32_t tab1, uint32_t tab9, uint32_t tab10,
                                const RefTable& t, Record* r) {
    if (e > s && p[e - 1] == (uint8_t)'\r') --e;                 // (a '\r' in front of the '\n' belongs to the terminator)
    if (e <= s) return kEmptyLine;
    if (p[s] == (uint8_t)'@') return kHeaderLine;
    if (tab10 == kNoOffset || (int64_t)tab10 >= e) return kFewFields;
    const uint32_t n_seq = tab10 - tab9 - 1u;
    const uint32_t l_seq = (n_seq == 1u && p[tab9 + 1u] == (uint8_t)'*') ? 0u : n_seq;
    return sam_decode_fields(p, (int64_t)tab1 + 1, (int64_t)tab9, l_seq, t, r);
}

// ---- host side of the table ---------------------------------------------------------------------------------------------
SAM_HD uint32_t table_capacity(int64_t n_ref) {
    if (n_ref <= 0) return 0;
    uint32_t cap = 2;
    while ((int64_t)cap < 2 * n_ref) cap <<= 1;
    return cap;
}

// fills `slots` (table_capacity(n_ref) words, zeroed by the caller) -> -1, or the row whose name is an earlier row's
inline int64_t build_table(const uint8_t* pool, const int64_t* off, int64_t n_ref, uint32_t* slots, uint32_t cap) {
    const uint32_t mask = cap - 1u;
    for (int64_t r = 0; r < n_ref; ++r) {
        const RefTable t{slots, cap, pool, off};
        if (lookup_name(t, pool, off[r], off[r + 1]) >= 0) return r;
        uint32_t at = name_hash(pool, off[r], off[r + 1]) & mask;
        while (slots[at]) at = (at + 1u) & mask;
        slots[at] = (uint32_t)r + 1u;
    }
    return -1;
}

}  // namespace besst_sam
