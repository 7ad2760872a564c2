// The per-lane steps of the BGZF compressor (bgzf_deflate.hip): tokens, Huffman code lengths, the dynamic header and the
// bit writer.  Plain C++ over the workgroup's shared state, one call per lane and step, so that the kernel is these steps
// with barriers between them - and tests/cpp/bgzf_deflate_core_test.cpp can run the same steps lane after lane on the
// host and hand the result to zlib.  DESIGN.md section 10.2 has the format rules.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BESST_HD __host__ __device__ __forceinline__
#else
#define BESST_HD inline
#endif

namespace besst {
namespace deflate {

constexpr int kThreads = 256;                 // lanes of a block's workgroup
constexpr int kNumLit = 286, kNumCl = 19;     // literal / length alphabet, code-length alphabet
constexpr int kLitLimit = 15, kClLimit = 7;
constexpr uint32_t kEob = 256;
constexpr uint32_t kMaxPayload = 65280;       // htslib's block payload
constexpr uint32_t kSlotStride = 65536;       // a block's place in the workspace
constexpr uint32_t kHeaderBytes = 18, kTrailerBytes = 8, kStoredBytes = 5, kEofBytes = 28;
constexpr int kMaxHdr = 320;                  // code-length symbols of a dynamic header: at most 286 + 1

// the shared words several lanes add to: sums, ORs and XORs, so the order in which they land changes nothing
BESST_HD void shared_add(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
BESST_HD void shared_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}

struct CodeWork {                             // build of one code: symbols in use sorted by (frequency, symbol), the merge
    uint32_t sfreq[kNumLit];
    uint32_t ifreq[kNumLit];
    uint16_t ssym[kNumLit];
    uint16_t ch0[kNumLit], ch1[kNumLit], depth[kNumLit];
    uint32_t num[16], first[16];
    uint32_t n_used;
};

struct BlockState {
    uint32_t freq[kNumLit];
    uint32_t code[kNumLit];                   // bits, LSB first | length << 16
    uint32_t cl_freq[kNumCl];
    uint32_t cl_code[kNumCl];
    uint8_t len[kNumLit + 2];
    uint8_t cl_len[kNumCl + 1];
    uint16_t hdr[kMaxHdr];                    // the header's code-length symbols: symbol | extra bits' value << 8
    uint32_t n_hdr, hdr_bits, hlit, hclen;
    uint32_t extra_bits, n_match, crc;        // sums over the lanes (crc: XOR)
    uint32_t start[kThreads + 1];             // first bit of every lane in the block's slot
    uint32_t tail[kThreads];                  // bits other lanes add to the last, partial word of a lane
    CodeWork w;
};

// lane t's span of a payload of `len` bytes: a multiple of four bytes, so that a block that begins at an aligned address
// is read in aligned words
BESST_HD void span_of(uint32_t len, uint32_t t, uint32_t* lo, uint32_t* hi) {
    const uint32_t per = (((len + (uint32_t)kThreads - 1u) / (uint32_t)kThreads) + 3u) & ~3u;
    const uint32_t a = t * per, b = a + per;
    *lo = a < len ? a : len;
    *hi = b < len ? b : len;
}

// bytes of the block through the aligned word that holds them (a lane walks its span byte by byte: one load per four).
// The word around the input's first and last byte is read whole: up to 3 bytes in front of an input that does not begin
// at a multiple of four and up to 3 behind its end - an aligned word never crosses a page, so the bytes are readable.
// The host test's build (no HIP) reads byte by byte instead and only inside [host_lo, host_hi).
struct ByteReader {
    const uint8_t* base;
    uintptr_t at;
    uint32_t word;
    BESST_HD explicit ByteReader(const uint8_t* b) : base(b), at(~(uintptr_t)0), word(0) {}
    BESST_HD uint32_t get(uint32_t i) {
        const uintptr_t a = (uintptr_t)(base + i), wa = a & ~(uintptr_t)3;
        if (wa != at) {
            at = wa;
#if defined(__HIPCC__)
            word = *reinterpret_cast<const uint32_t*>(wa);
#else
            word = 0;
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint8_t* p = reinterpret_cast<const uint8_t*>(wa) + k;
                if (p >= host_lo && p < host_hi) word |= (uint32_t)*p << (8u * k);
            }
#endif
        }
        return (word >> (8u * (uint32_t)(a & 3u))) & 0xffu;
    }
#if !defined(__HIPCC__)
    const uint8_t* host_lo = nullptr;         // the input's first byte and the one behind its last
    const uint8_t* host_hi = nullptr;
#endif
};

// length 3..258 -> its symbol, the number of extra bits and their value (RFC 1951, 3.2.5, in closed form)
BESST_HD void length_symbol(uint32_t m, uint32_t* sym, uint32_t* ebits, uint32_t* eval) {
    const uint32_t l = m - 3u;
    if (m == 258u) { *sym = 285u; *ebits = 0u; *eval = 0u; return; }
    if (l < 8u) { *sym = 257u + l; *ebits = 0u; *eval = 0u; return; }
    uint32_t e = 1u;
    while ((l >> (e + 3u)) != 0u) ++e;        // l in [8 << (e - 1), 16 << (e - 1))
    *sym = 261u + 4u * e + ((l >> e) & 3u);
    *ebits = e;
    *eval = l & ((1u << e) - 1u);
}

// The tokens of bytes [lo, hi) of the block: every maximal run inside the span is one literal and matches of distance 1,
// or matches alone where the byte in front of the span is the run's byte and belongs to the block.  A match is 3..258
// bytes; the one in front of a rest of 1 or 2 is shortened so that the rest is a match too.  With span_of() as it is a
// span holds 256 bytes at most, so on the device a match is at most 256 bytes and neither the cap of 258 (symbol 285) nor
// the shortening is reached: they keep the tokens valid should span_of() ever hand out more.
template <class F>
BESST_HD void tokenize(ByteReader& rd, uint32_t lo, uint32_t hi, F& f) {
    if (lo >= hi) return;
    uint32_t prev = lo > 0u ? rd.get(lo - 1u) : 256u;
    uint32_t i = lo, c = rd.get(lo);
    while (i < hi) {
        uint32_t j = i + 1u, next = 256u;
        while (j < hi && (next = rd.get(j)) == c) ++j;
        uint32_t rem = j - i;
        if (c != prev) { f.literal(c); --rem; }
        while (rem != 0u) {
            if (rem < 3u) {
                f.literal(c);
                if (rem == 2u) f.literal(c);
                break;
            }
            uint32_t m = rem < 258u ? rem : 258u;
            if (rem - m == 1u || rem - m == 2u) m = rem - 3u;
            f.match(m);
            rem -= m;
        }
        prev = c;
        i = j;
        c = next;
    }
}

// ---- step 1: the symbols' frequencies -------------------------------------------------------------------------------
// (the four bases are counted in the lane's registers and added once: on nucleotide text every literal of all 256 lanes
// would otherwise be an atomic on one of four words)
struct CountTokens {
    BlockState& s;
    uint32_t extra, matches;
    uint32_t base[4];                         // A C G T
    BESST_HD void literal(uint32_t c) {
        if (c == 'A') ++base[0];
        else if (c == 'C') ++base[1];
        else if (c == 'G') ++base[2];
        else if (c == 'T') ++base[3];
        else shared_add(&s.freq[c], 1u);
    }
    BESST_HD void match(uint32_t m) {
        uint32_t sym, eb, ev;
        length_symbol(m, &sym, &eb, &ev);
        shared_add(&s.freq[sym], 1u);
        extra += eb;
        ++matches;
    }
};
BESST_HD void count_step(BlockState& s, ByteReader& rd, uint32_t lo, uint32_t hi, uint32_t t) {
    CountTokens f{s, 0u, 0u, {0u, 0u, 0u, 0u}};
    tokenize(rd, lo, hi, f);
    if (f.base[0]) shared_add(&s.freq['A'], f.base[0]);
    if (f.base[1]) shared_add(&s.freq['C'], f.base[1]);
    if (f.base[2]) shared_add(&s.freq['G'], f.base[2]);
    if (f.base[3]) shared_add(&s.freq['T'], f.base[3]);
    if (f.matches) {
        shared_add(&s.extra_bits, f.extra);
        shared_add(&s.n_match, f.matches);
    }
    if (t == 0u) shared_add(&s.freq[kEob], 1u);
}

// ---- step 2: code lengths of an alphabet, limited ---------------------------------------------------------------------
// (a) every lane ranks its symbols by (frequency, symbol) among those in use
BESST_HD void lengths_rank(const uint32_t* freq, uint32_t n_sym, uint8_t* len, CodeWork& w, uint32_t t) {
    for (uint32_t s = t; s < n_sym; s += (uint32_t)kThreads) {
        const uint32_t f = freq[s];
        len[s] = 0;
        if (f == 0u) continue;
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n_sym; ++j) {
            const uint32_t g = freq[j];
            rank += (g != 0u && (g < f || (g == f && j < s))) ? 1u : 0u;
        }
        w.sfreq[rank] = f;
        w.ssym[rank] = (uint16_t)s;
        shared_add(&w.n_used, 1u);
    }
}
// (b) one lane: the two-queue merge over the sorted frequencies (a tie takes the leaf), the number of leaves per depth
// with depths beyond the limit counted at the limit, the Kraft sum repaired (one code leaves the limit's length and joins
// a code of the longest shorter length one bit further down, until the sum is 1), and the lengths handed out longest to
// rarest.  The code is complete whenever two symbols or more are in use.
BESST_HD void lengths_serial(uint32_t limit, uint8_t* len, CodeWork& w) {
    const uint32_t n = w.n_used;
    for (uint32_t l = 0; l < 16u; ++l) w.num[l] = 0u;
    if (n == 1u) {
        w.num[1] = 1u;
    } else if (n >= 2u) {
        uint32_t leaf = 0, inner = 0;
        for (uint32_t k = 0; k + 1u < n; ++k) {
            uint32_t sum = 0;
            for (int side = 0; side < 2; ++side) {
                uint32_t pick;
                if (leaf < n && (inner >= k || w.sfreq[leaf] <= w.ifreq[inner])) {
                    pick = leaf;
                    sum += w.sfreq[leaf++];
                } else {
                    pick = n + inner;
                    sum += w.ifreq[inner++];
                }
                if (side == 0) w.ch0[k] = (uint16_t)pick; else w.ch1[k] = (uint16_t)pick;
            }
            w.ifreq[k] = sum;
        }
        w.depth[n - 2u] = 0;
        for (uint32_t k = n - 1u; k-- > 0u;) {
            const uint32_t d = (uint32_t)w.depth[k] + 1u;
            for (int side = 0; side < 2; ++side) {
                const uint32_t c = side == 0 ? w.ch0[k] : w.ch1[k];
                if (c >= n) w.depth[c - n] = (uint16_t)d;
                else w.num[d < limit ? d : limit] += 1u;
            }
        }
        uint32_t total = 0;
        for (uint32_t l = 1; l <= limit; ++l) total += w.num[l] << (limit - l);
        while (total > (1u << limit)) {
            w.num[limit] -= 1u;
            for (uint32_t l = limit - 1u; l > 0u; --l) {
                if (w.num[l]) {
                    w.num[l] -= 1u;
                    w.num[l + 1u] += 2u;
                    break;
                }
            }
            --total;
        }
    }
    uint32_t at = 0;
    for (uint32_t l = limit; l > 0u; --l)
        for (uint32_t c = 0; c < w.num[l]; ++c) len[w.ssym[at++]] = (uint8_t)l;
    uint32_t code = 0;
    w.first[0] = 0u;
    for (uint32_t l = 1; l < 16u; ++l) {
        code = (code + (l > 1u ? w.num[l - 1u] : 0u)) << 1;
        w.first[l] = code;
    }
}
// (c) every lane: the canonical code of its symbols, bits reversed into DEFLATE's order
BESST_HD void lengths_codes(uint32_t n_sym, const uint8_t* len, uint32_t* code_out, const CodeWork& w, uint32_t t) {
    for (uint32_t s = t; s < n_sym; s += (uint32_t)kThreads) {
        const uint32_t l = len[s];
        uint32_t v = 0;
        if (l) {
            uint32_t before = 0;
            for (uint32_t j = 0; j < s; ++j) before += len[j] == l ? 1u : 0u;
            const uint32_t code = w.first[l] + before;
            uint32_t rev = 0;
            for (uint32_t k = 0; k < l; ++k) rev |= ((code >> k) & 1u) << (l - 1u - k);
            v = rev | (l << 16);
        }
        code_out[s] = v;
    }
}

// ---- step 3 (one lane): the header's code lengths, run-length coded with 16 / 17 / 18 ----------------------------------
BESST_HD void header_rle(BlockState& s) {
    uint32_t hlit = kNumLit;
    while (hlit > 257u && s.len[hlit - 1u] == 0) --hlit;
    s.hlit = hlit;
    s.len[hlit] = s.n_match ? 1 : 0;                          // the one distance code (HDIST = 1) behind the literal / length ones
    const uint32_t n = hlit + 1u;
    for (uint32_t k = 0; k < (uint32_t)kNumCl; ++k) s.cl_freq[k] = 0u;
    uint32_t n_hdr = 0;
    auto emit = [&](uint32_t sym, uint32_t extra) {
        s.hdr[n_hdr++] = (uint16_t)(sym | (extra << 8));
        s.cl_freq[sym] += 1u;
    };
    for (uint32_t i = 0; i < n;) {
        const uint32_t v = s.len[i];
        uint32_t run = 1;
        while (i + run < n && s.len[i + run] == v) ++run;
        i += run;
        if (v == 0u) {
            while (run) {
                uint32_t m;
                if (run >= 11u) { m = run < 138u ? run : 138u; emit(18u, m - 11u); }
                else if (run >= 3u) { m = run; emit(17u, m - 3u); }
                else { m = 1u; emit(0u, 0u); }
                run -= m;
            }
        } else {
            emit(v, 0u);
            --run;
            while (run >= 3u) {
                const uint32_t m = run < 6u ? run : 6u;
                emit(16u, m - 3u);
                run -= m;
            }
            while (run) { emit(v, 0u); --run; }
        }
    }
    s.n_hdr = n_hdr;
}
BESST_HD uint32_t cl_order(uint32_t i) {      // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    return i < 3u ? 16u + i : i == 3u ? 0u : (i & 1u) ? 8u - ((i - 3u) >> 1) : 8u + ((i - 4u) >> 1);
}
BESST_HD uint32_t cl_extra_bits(uint32_t sym) { return sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u; }
BESST_HD void header_finish(BlockState& s) {
    uint32_t hclen = kNumCl;
    while (hclen > 4u && s.cl_len[cl_order(hclen - 1u)] == 0) --hclen;
    s.hclen = hclen;
    uint32_t bits = 3u + 5u + 5u + 4u + 3u * hclen;
    for (uint32_t k = 0; k < s.n_hdr; ++k) {
        const uint32_t sym = s.hdr[k] & 0xffu;
        bits += (uint32_t)s.cl_len[sym] + cl_extra_bits(sym);
    }
    s.hdr_bits = bits;
}

// ---- step 4: the bits of every lane's tokens --------------------------------------------------------------------------
struct MeasureTokens {
    const BlockState& s;
    uint32_t bits;
    BESST_HD void literal(uint32_t c) { bits += s.len[c]; }
    BESST_HD void match(uint32_t m) {
        uint32_t sym, eb, ev;
        length_symbol(m, &sym, &eb, &ev);
        bits += (uint32_t)s.len[sym] + eb + 1u;
    }
};
// lane 0 carries the gzip header, BSIZE and the DEFLATE header in front of its tokens, the last lane the end-of-block code
// behind them (the padding to a whole byte and the trailer are added once the sum is known)
BESST_HD uint32_t measure_step(const BlockState& s, ByteReader& rd, uint32_t lo, uint32_t hi, uint32_t t) {
    MeasureTokens f{s, 0u};
    tokenize(rd, lo, hi, f);
    if (t == 0u) f.bits += 8u * kHeaderBytes + s.hdr_bits;
    if (t == (uint32_t)kThreads - 1u) f.bits += s.len[kEob];
    return f.bits;
}
// the DEFLATE data's bytes in its dynamic form, from the bit behind the end-of-block code
BESST_HD uint32_t dynamic_bytes(uint32_t end_bit) { return (end_bit - 8u * kHeaderBytes + 7u) >> 3; }
BESST_HD bool takes_stored_form(uint32_t end_bit, uint32_t len) { return dynamic_bytes(end_bit) >= len + kStoredBytes; }

// ---- step 5: every lane writes its own bits ----------------------------------------------------------------------------
// A lane's bits begin at any bit of the slot.  Words that lie wholly in the lane's range are stored as they fill.  A word
// the lane shares is completed by ONE lane, the one that holds the word's first bit: that lane keeps its last, partial
// word back (tail_word), the lanes that begin further on in the same word OR theirs into tail[owner] - shared memory -,
// and after a barrier the owner stores the two together.
struct BitWriter {
    uint32_t* slot;                           // the block's slot as words
    uint32_t* tail;                           // BlockState::tail
    unsigned long long acc;
    uint32_t n, word, owner;
    bool shared_head;                         // the word being filled began in front of this lane
    uint32_t tail_word, tail_bits;
    bool has_tail;
    BESST_HD void begin(uint32_t* slot_, BlockState& s, uint32_t t) {
        slot = slot_;
        tail = s.tail;
        const uint32_t bit = s.start[t];
        word = bit >> 5;
        n = bit & 31u;
        acc = 0ull;
        shared_head = n != 0u;
        has_tail = false;
        tail_word = tail_bits = 0u;
        owner = t;
        if (shared_head) {                    // the last lane that begins at or before the word's first bit (it is not empty)
            const uint32_t first_bit = word << 5;
            uint32_t a = 0, b = t;            // start[a] <= first_bit < start[b]
            while (b - a > 1u) {
                const uint32_t m = (a + b) >> 1;
                if (s.start[m] <= first_bit) a = m; else b = m;
            }
            owner = a;
        }
    }
    BESST_HD void put(uint32_t v, uint32_t bits) {            // bits <= 32, v < 2^bits
        acc |= (unsigned long long)v << n;
        n += bits;
        if (n >= 32u) {
            const uint32_t x = (uint32_t)acc;
            if (shared_head) {
                shared_or(&tail[owner], x);
                shared_head = false;
            } else {
                slot[word] = x;
            }
            ++word;
            acc >>= 32;
            n -= 32u;
        }
    }
    BESST_HD void end() {
        if (n == 0u) return;
        if (shared_head) {
            shared_or(&tail[owner], (uint32_t)acc);
        } else {
            has_tail = true;
            tail_word = word;
            tail_bits = (uint32_t)acc;
        }
    }
    BESST_HD void finish(uint32_t t) {        // behind the barrier
        if (has_tail) slot[tail_word] = tail_bits | tail[t];
    }
};
struct WriteTokens {
    const BlockState& s;
    BitWriter& w;
    BESST_HD void literal(uint32_t c) {
        const uint32_t e = s.code[c];
        w.put(e & 0xffffu, e >> 16);
    }
    BESST_HD void match(uint32_t m) {
        uint32_t sym, eb, ev;
        length_symbol(m, &sym, &eb, &ev);
        const uint32_t e = s.code[sym];
        const uint32_t l = e >> 16;
        w.put((e & 0xffffu) | (ev << l), l + eb + 1u);     // code, extra bits, and the distance code's one bit: 0
    }
};
// end_bit: the bit behind the end-of-block code (start[kThreads] before padding and trailer were added)
BESST_HD void write_step(const BlockState& s, BitWriter& w, ByteReader& rd, uint32_t lo, uint32_t hi, uint32_t t, uint32_t len,
                         uint32_t end_bit) {
    if (t == 0u) {
        const uint32_t bsize = ((end_bit + 7u) >> 3) + kTrailerBytes;
        w.put(0x04088b1fu, 32); w.put(0u, 32); w.put(0x0006ff00u, 32); w.put(0x00024342u, 32);
        w.put(bsize - 1u, 16);
        w.put(1u | (2u << 1), 3);             // BFINAL, BTYPE = 2
        w.put(s.hlit - 257u, 5);
        w.put(0u, 5);                         // HDIST - 1
        w.put(s.hclen - 4u, 4);
        for (uint32_t k = 0; k < s.hclen; ++k) w.put(s.cl_len[cl_order(k)], 3);
        for (uint32_t k = 0; k < s.n_hdr; ++k) {
            const uint32_t sym = s.hdr[k] & 0xffu, extra = s.hdr[k] >> 8;
            const uint32_t e = s.cl_code[sym];
            const uint32_t l = e >> 16;
            w.put((e & 0xffffu) | (extra << l), l + cl_extra_bits(sym));
        }
    }
    WriteTokens f{s, w};
    tokenize(rd, lo, hi, f);
    if (t == (uint32_t)kThreads - 1u) {
        const uint32_t e = s.code[kEob];
        w.put(e & 0xffffu, e >> 16);
        w.put(0u, (8u - (end_bit & 7u)) & 7u);
        w.put(s.crc, 32);
        w.put(len, 32);
    }
    w.end();
}

// ---- sizes every caller can work out ------------------------------------------------------------------------------------
inline int64_t block_count(int64_t n_bytes, int32_t block_payload) { return (n_bytes + block_payload - 1) / block_payload; }
inline bool valid_payload(int32_t block_payload) { return block_payload >= 1 && block_payload <= (int32_t)kMaxPayload; }

}  // namespace deflate
}  // namespace besst
