// The sequential steps of the parallel inflate of a plain gzip member (gzip_stream.hip), written
// so that the host compiles them too: tests/cpp/gzip_stream_core_test.cpp runs them lane after lane against zlib.
//   probe_dynamic_header   is this bit position the start of a dynamic DEFLATE block?  zlib's header checks, no tables
//   Code / code_prepare / code_fill / code_lookup   a canonical Huffman code: counts, first codes and sorted symbols
//                          (one lane), the primary table (every lane its slots), one symbol (table, else canonical)
//   walk_chunk             block after block from a start bit to the landing: lengths only (the count), or 16-bit symbols
//                          (the decode): a literal, or kMarker | k = "byte k of the 32 KiB in front of this chunk"
//   link_chain             the live chunks: the landings followed from chunk 0, their places in the text
//   member_magic / member_data_offset / member_find / link_members   a file of SEVERAL members: the byte offsets that read
//                          like a member's start, a header's end, the list of those offsets, and the chain that passes
//                          from a member's final block over its trailer to the next member's first block
//   resolve_symbol         a 16-bit symbol -> its byte, given the text in front of the chunk
// Bit positions count from the first byte of the FILE (bit 0 of byte 0 is position 0), LSB first as RFC 1951 packs them.
// Everything a wave does in step is written for `lane` of `nlanes`: the device runs 64 lanes, the host one (or 64, one
// after the other, where a step has no barrier inside).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GZ_FN __host__ __device__ inline
#else
#define GZ_FN inline
#endif

namespace besst {
namespace gz {

// status of a chunk, and of the member (0 = good).  9 and 10 are BGZF's BESST_BGZF_BAD_SIZE / BESST_BGZF_BAD_CRC.
enum : uint32_t {
    kOk = 0, kBadBlockType, kBadStored, kBadLengths, kOversubscribed, kBadCode, kBadDistance, kOutputOverrun, kInputOverrun,
    kBadSize, kBadCrc, kTrailingBytes, kTooManyMembers, kStatusCount
};

constexpr uint32_t kNoCandidate = 0xffffffffu;
constexpr uint32_t kMarker = 0x8000u;
constexpr uint32_t kWindow = 32768u;
constexpr uint32_t kMaxLens = 320u;          // HLIT + HDIST + 258 at most (the fixed code: 288 + 32)

// ---- bits of a byte range: 32 bits from any position, zeros behind the end ------------------------------------------------
struct ByteBits {
    const uint8_t* data;
    uint64_t n_bytes;
    GZ_FN uint32_t peek(uint64_t bit) const {
        const uint64_t b = bit >> 3;
        uint64_t v = 0;
        for (uint32_t k = 0; k < 5u; ++k)
            if (b + k < n_bytes) v |= (uint64_t)data[b + k] << (8u * k);
        return (uint32_t)(v >> (bit & 7u));
    }
};

GZ_FN uint32_t bit_reverse(uint32_t v, uint32_t n) {         // the low n bits of v, reversed
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32u - n);
}

// ---- the code-length code: nineteen lengths of three bits packed in a word, decoded canonically bit by bit (no table: a
// probing lane has no memory of its own, and a block header holds ~300 of these symbols) ---------------------------------------
GZ_FN uint32_t cl_order(uint32_t i) {                        // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    return i < 3u ? 16u + i : i == 3u ? 0u : (i & 1u) ? 8u - ((i - 3u) >> 1) : 8u + ((i - 4u) >> 1);
}
GZ_FN uint32_t cl_len(uint64_t packed, uint32_t sym) { return (uint32_t)(packed >> (3u * sym)) & 7u; }
// -> the space the code leaves in units of 2^-7: 0 = complete, > 0 incomplete, < 0 oversubscribed
GZ_FN int32_t cl_left(uint64_t packed) {
    int32_t left = 128;
    for (uint32_t s = 0; s < 19u; ++s) {
        const uint32_t l = cl_len(packed, s);
        if (l) left -= (int32_t)(128u >> l);
    }
    return left;
}
// one symbol from the low bits of x -> symbol | bits << 8, or 0xffffffff (no code)
GZ_FN uint32_t cl_decode(uint64_t packed, uint32_t x) {
    uint32_t code = 0, first = 0;
    for (uint32_t L = 1; L <= 7u; ++L) {
        code |= (x >> (L - 1u)) & 1u;
        uint32_t count = 0;
        for (uint32_t s = 0; s < 19u; ++s) count += cl_len(packed, s) == L ? 1u : 0u;
        if (code - first < count) {
            uint32_t r = code - first;
            for (uint32_t s = 0; s < 19u; ++s) {
                if (cl_len(packed, s) == L) {
                    if (r == 0u) return s | (L << 8);
                    --r;
                }
            }
        }
        first = (first + count) << 1;
        code <<= 1;
    }
    return 0xffffffffu;
}
// HCLEN + 4 lengths from bit `p` on -> packed, p moved on
GZ_FN uint64_t cl_read(const ByteBits& in, uint64_t& p, uint32_t ncl) {
    uint64_t packed = 0;
    for (uint32_t i = 0; i < ncl; ++i) {
        packed |= (uint64_t)(in.peek(p) & 7u) << (3u * cl_order(i));
        p += 3u;
    }
    return packed;
}

// ---- the probe: does a dynamic block that zlib's inflate accepts begin at `bit`?  BTYPE = 2, HLIT <= 29, HDIST <= 29, a
// complete code-length code, legal repeats, a length for symbol 256, a complete literal / length code, a distance code that
// is complete or a single code of one bit - and all of the header in front of end_bit. ---------------------------------------
GZ_FN bool probe_dynamic_header(const ByteBits& in, uint64_t bit, uint64_t end_bit) {
    const uint32_t x = in.peek(bit);
    if (((x >> 1) & 3u) != 2u) return false;
    const uint32_t hlit = (x >> 3) & 31u, hdist = (x >> 8) & 31u, ncl = ((x >> 13) & 15u) + 4u;
    if (hlit > 29u || hdist > 29u) return false;
    uint64_t p = bit + 17u;
    if (p + 3u * ncl > end_bit) return false;
    const uint64_t packed = cl_read(in, p, ncl);
    if (cl_left(packed) != 0) return false;
    const uint32_t nlit = hlit + 257u, total = nlit + hdist + 1u;
    uint32_t have = 0, prev = 0, lit_sum = 0, dist_sum = 0, dist_codes = 0, len256 = 0;
    while (have < total) {
        if (p > end_bit) return false;
        const uint32_t y = in.peek(p);
        const uint32_t d = cl_decode(packed, y);
        if (d == 0xffffffffu) return false;
        const uint32_t sym = d & 0xffu, l = d >> 8;
        uint32_t rep = 1, val = sym, used = l;
        if (sym == 16u) {
            if (have == 0u) return false;
            rep = 3u + ((y >> l) & 3u); val = prev; used += 2u;
        } else if (sym == 17u) {
            rep = 3u + ((y >> l) & 7u); val = 0; used += 3u;
        } else if (sym == 18u) {
            rep = 11u + ((y >> l) & 127u); val = 0; used += 7u;
        }
        if (have + rep > total) return false;
        p += used;
        if (val) {
            for (uint32_t i = 0; i < rep; ++i) {
                const uint32_t at = have + i;
                if (at < nlit) {
                    lit_sum += 32768u >> val;
                    if (at == 256u) len256 = val;
                } else {
                    dist_sum += 32768u >> val;
                    ++dist_codes;
                }
            }
        }
        have += rep;
        prev = val;
    }
    if (p > end_bit) return false;
    if (len256 == 0u || lit_sum != 32768u) return false;
    return dist_sum == 32768u || (dist_codes == 1u && dist_sum == 16384u);
}

// ---- a canonical code with a primary table ------------------------------------------------------------------------------------
template <int N, int BITS>
struct Code {
    uint16_t cnt[16], first[16], offs[16], run[16];
    uint16_t sorted[N];
    uint16_t tab[1 << BITS];                 // symbol << 4 | length, 0: no code of at most BITS bits
};

// counts, first codes, offsets and the symbols sorted by (length, symbol): ONE lane.  false: oversubscribed.
template <int N, int BITS>
GZ_FN bool code_prepare(Code<N, BITS>& c, const uint8_t* lens, uint32_t n) {
    for (uint32_t L = 0; L < 16u; ++L) c.cnt[L] = 0;
    for (uint32_t s = 0; s < n; ++s) ++c.cnt[lens[s] & 15u];
    c.cnt[0] = 0;
    uint32_t code = 0, off = 0;
    int32_t left = 1;
    c.first[0] = c.offs[0] = c.run[0] = 0;
    for (uint32_t L = 1; L < 16u; ++L) {
        code = (code + c.cnt[L - 1u]) << 1;
        c.first[L] = (uint16_t)code;
        c.offs[L] = c.run[L] = (uint16_t)off;
        off += c.cnt[L];
        left = (left << 1) - (int32_t)c.cnt[L];
        if (left < 0) return false;
    }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = lens[s] & 15u;
        if (l) c.sorted[c.run[l]++] = (uint16_t)s;
    }
    return true;
}
// the primary table: lane `lane` of `nlanes` decodes the bit patterns of its slots canonically
template <int N, int BITS>
GZ_FN void code_fill(Code<N, BITS>& c, uint32_t lane, uint32_t nlanes) {
    for (uint32_t slot = lane; slot < (1u << BITS); slot += nlanes) {
        const uint32_t r = bit_reverse(slot, BITS);          // the slot's bits as an MSB-first code prefix
        uint32_t e = 0;
        for (uint32_t L = 1; L <= (uint32_t)BITS; ++L) {
            const uint32_t d = (r >> ((uint32_t)BITS - L)) - c.first[L];
            if (e == 0u && d < c.cnt[L]) e = ((uint32_t)c.sorted[c.offs[L] + d] << 4) | L;
        }
        c.tab[slot] = (uint16_t)e;
    }
}
// one symbol from the low bits of x -> symbol << 4 | length, 0: not a code
template <int N, int BITS>
GZ_FN uint32_t code_lookup(const Code<N, BITS>& c, uint32_t x) {
    const uint32_t e = c.tab[x & ((1u << BITS) - 1u)];
    if (e) return e;
    const uint32_t r = bit_reverse(x, 15);
    for (uint32_t L = (uint32_t)BITS + 1u; L < 16u; ++L) {
        const uint32_t d = (r >> (15u - L)) - c.first[L];
        if (d < c.cnt[L]) return ((uint32_t)c.sorted[c.offs[L] + d] << 4) | L;
    }
    return 0;
}

// RFC 1951's length and distance codes in closed form: base | extra bits << 16 (0: no such code)
GZ_FN uint32_t length_code(uint32_t k) {                     // k = symbol - 257
    if (k < 8u) return 3u + k;
    if (k == 28u) return 258u;
    if (k > 28u) return 0u;
    const uint32_t extra = (k - 4u) >> 2;
    return (3u + ((4u + (k & 3u)) << extra)) | (extra << 16);
}
GZ_FN uint32_t distance_code(uint32_t k) {
    if (k < 4u) return 1u + k;
    if (k > 29u) return 0u;
    const uint32_t extra = (k - 2u) >> 1;
    return (1u + ((2u + (k & 1u)) << extra)) | (extra << 16);
}

struct WalkTables {
    Code<288, 10> lit;
    Code<32, 9> dist;
    uint8_t lens[kMaxLens];
};

// a dynamic block's code lengths (the reader stands behind BTYPE) -> lens[0, nlit) and lens[288, 288 + ndist).  Every lane
// reads the same bits and writes the same bytes.
template <class Ctx>
GZ_FN uint32_t read_lengths(Ctx& c, uint8_t* lens, uint32_t& nlit, uint32_t& ndist) {
    uint32_t x = c.peek();
    const uint32_t hlit = (x & 31u) + 257u, hdist = ((x >> 5) & 31u) + 1u, ncl = ((x >> 10) & 15u) + 4u;
    c.drop(14);
    if (hlit > 286u || hdist > 30u) return kBadLengths;
    uint64_t packed = 0;
    for (uint32_t i = 0; i < ncl; ++i) {
        packed |= (uint64_t)(c.peek() & 7u) << (3u * cl_order(i));
        c.drop(3);
    }
    if (cl_left(packed) < 0) return kOversubscribed;
    const uint32_t total = hlit + hdist;
    uint32_t have = 0, prev = 0;
    while (have < total) {
        x = c.peek();
        const uint32_t d = c.uni(cl_decode(packed, x));
        if (d == 0xffffffffu) return kBadLengths;
        const uint32_t sym = d & 0xffu, l = d >> 8;
        uint32_t rep = 1, val = sym, used = l;
        if (sym == 16u) {
            if (have == 0u) return kBadLengths;
            rep = 3u + ((x >> l) & 3u); val = prev; used += 2u;
        } else if (sym == 17u) {
            rep = 3u + ((x >> l) & 7u); val = 0; used += 3u;
        } else if (sym == 18u) {
            rep = 11u + ((x >> l) & 127u); val = 0; used += 7u;
        }
        if (have + rep > total) return kBadLengths;
        c.drop(used);
        for (uint32_t i = 0; i < rep; ++i) {
            const uint32_t at = have + i;
            lens[at < hlit ? at : 288u + (at - hlit)] = (uint8_t)val;
        }
        have += rep;
        prev = val;
    }
    if (lens[256] == 0u) return kBadLengths;                 // no end-of-block code
    nlit = hlit;
    ndist = hdist;
    return kOk;
}

// what a walk is told and what it leaves
struct WalkArgs {
    uint64_t start_bit, end_bit;     // the chunk's start; the first bit behind the DEFLATE data's room (the trailer)
    // the count: a block end that is the candidate of the chunk it lies in is the landing
    const uint32_t* cand_rel;        // per chunk: its candidate's bit, counted from the chunk's first (kNoCandidate: none)
    uint64_t n_chunks, data_bit0, chunk_bits;
    // the decode: the landing found by the count, the bytes until there, the chunk's place in the text, and the place
    // where its member's text begins (a match may reach that byte and not one further)
    uint64_t stop_bit, out_cap, text_off, member_off;
};
struct WalkResult {
    uint64_t land_bit, out_bytes;
    uint32_t final_block, status;
};

// Block after block from a.start_bit.  kWrite = false (the count): lengths only, until BFINAL or the landing rule.
// kWrite = true (the decode): symbols to c.store(i, v), i counted from the chunk's first byte; a match reads c.load(i) of
// bytes in front of it; ends at a.stop_bit.  Every turn of every loop consumes input bits and tests them against
// a.end_bit; the decode tests every byte against a.out_cap.
// Ctx: lane, nlanes, peek() (32 bits at the position), drop(n), pos(), seek(bit), byte(i) (of the file), barrier(),
// uni(v) (a value all lanes hold), store / load.
template <bool kWrite, class Ctx>
GZ_FN WalkResult walk_chunk(Ctx& c, WalkTables& t, const WalkArgs& a) {
    WalkResult res = {0, 0, 0, kOk};
    uint64_t pos = 0;
    c.seek(a.start_bit);
    for (;;) {
        if (c.pos() + 3u > a.end_bit) { res.status = kInputOverrun; break; }
        const uint32_t hdr = c.peek();
        const uint32_t final_block = hdr & 1u, type = (hdr >> 1) & 3u;
        c.drop(3);
        if (type == 0u) {
            const uint64_t at = (c.pos() + 7u) & ~(uint64_t)7u;
            if (at + 32u > a.end_bit) { res.status = kInputOverrun; break; }
            c.seek(at);
            const uint32_t v = c.peek();
            const uint32_t len = v & 0xffffu;
            if (len != (~(v >> 16) & 0xffffu)) { res.status = kBadStored; break; }
            const uint64_t from = (at >> 3) + 4u;
            if ((from + len) * 8u > a.end_bit) { res.status = kInputOverrun; break; }
            if (kWrite) {
                if (pos + len > a.out_cap) { res.status = kOutputOverrun; break; }
                for (uint32_t i = c.lane; i < len; i += c.nlanes) c.store(pos + i, c.byte(from + i));
            }
            pos += len;
            c.seek((from + len) * 8u);
        } else if (type == 3u) {
            res.status = kBadBlockType;
            break;
        } else {
            uint32_t nlit = 288, ndist = 32;
            c.barrier();                                     // (the tables of the block before are no longer read)
            if (type == 1u) {
                for (uint32_t i = c.lane; i < 288u; i += c.nlanes) t.lens[i] = (uint8_t)(i < 144u ? 8 : i < 256u ? 9 : i < 280u ? 7 : 8);
                for (uint32_t i = c.lane; i < 32u; i += c.nlanes) t.lens[288u + i] = 5;
            } else {
                const uint32_t st = read_lengths(c, t.lens, nlit, ndist);
                if (st) { res.status = st; break; }
            }
            c.barrier();
            bool ok = true;
            if (c.lane == 0u) {
                ok = code_prepare(t.lit, t.lens, nlit);
                ok = code_prepare(t.dist, t.lens + 288, ndist) && ok;
                t.lit.run[0] = ok ? 1 : 0;                   // (told to the other lanes)
            }
            c.barrier();
            if (t.lit.run[0] == 0u) { res.status = kOversubscribed; break; }
            code_fill(t.lit, c.lane, c.nlanes);
            code_fill(t.dist, c.lane, c.nlanes);
            c.barrier();
            uint32_t st = kOk;
            for (;;) {
                if (c.pos() >= a.end_bit) { st = kInputOverrun; break; }
                uint32_t x = c.peek();
                uint32_t e = c.uni(code_lookup(t.lit, x));
                if (e == 0u) { st = kBadCode; break; }
                const uint32_t l = e & 15u, sym = e >> 4;
                if (sym < 256u) {
                    if (kWrite) {
                        if (pos >= a.out_cap) { st = kOutputOverrun; break; }
                        if (c.lane == 0u) c.store(pos, sym);
                    }
                    ++pos;
                    c.drop(l);
                    continue;
                }
                c.drop(l);
                if (sym == 256u) break;
                const uint32_t lc = length_code(sym - 257u);
                if (lc == 0u) { st = kBadCode; break; }
                const uint32_t len = (lc & 0xffffu) + ((x >> l) & ((1u << (lc >> 16)) - 1u));
                c.drop(lc >> 16);
                x = c.peek();
                e = c.uni(code_lookup(t.dist, x));
                if (e == 0u) { st = kBadCode; break; }
                const uint32_t dc = distance_code(e >> 4);
                if (dc == 0u) { st = kBadCode; break; }
                const uint32_t dist = (dc & 0xffffu) + ((x >> (e & 15u)) & ((1u << (dc >> 16)) - 1u));
                c.drop((e & 15u) + (dc >> 16));
                if (kWrite) {
                    if (pos + len > a.out_cap) { st = kOutputOverrun; break; }
                    if (dist > pos + (a.text_off - a.member_off)) { st = kBadDistance; break; }   // in front of the member's first byte
                    // byte i of the match is byte i mod dist of the dist bytes in front of it: every source lies in front of
                    // the match, inside the chunk (its symbol is copied) or in the window (a marker)
                    for (uint32_t i = c.lane; i < len; i += c.nlanes) {
                        const uint32_t j = dist < len ? i % dist : i;
                        const uint64_t back = dist - j;      // the source lies `back` bytes in front of pos
                        const uint32_t v = back > pos ? kMarker | (uint32_t)(kWindow - (back - pos)) : c.load(pos - back);
                        c.store(pos + i, v);
                    }
                }
                pos += len;
            }
            if (st) { res.status = st; break; }
        }
        const uint64_t e = c.pos();
        if (e > a.end_bit) { res.status = kInputOverrun; break; }
        res.land_bit = e;
        res.final_block = final_block;
        if (kWrite) {
            if (e == a.stop_bit || final_block) break;
        } else {
            if (final_block) break;
            const uint64_t j = (e - a.data_bit0) / a.chunk_bits;
            if (j < a.n_chunks && a.cand_rel[j] != kNoCandidate && a.data_bit0 + j * a.chunk_bits + a.cand_rel[j] == e) break;
        }
    }
    res.out_bytes = pos;
    if (kWrite && res.status == kOk && (res.land_bit != a.stop_bit || pos != a.out_cap)) res.status = kBadSize;
    return res;
}

// ---- the live chain --------------------------------------------------------------------------------------------------------------
// Follows the landings from chunk 0: live_idx[0, n_live) the chunks on the chain, live_off their places in the text.
// -> status of the first live chunk that has one; *text_bytes, *n_live, *end_bit (where the final block ended).
GZ_FN uint32_t link_chain(const uint64_t* land, const uint64_t* out_bytes, const uint32_t* final_block, const uint32_t* status,
                          uint64_t n_chunks, uint64_t data_bit0, uint64_t chunk_bits, uint32_t* live_idx, uint64_t* live_off,
                          uint64_t* text_bytes, uint64_t* n_live, uint64_t* end_bit) {
    uint64_t c = 0, n = 0, off = 0;
    uint32_t st = kOk;
    *end_bit = 0;
    for (;;) {
        live_idx[n] = (uint32_t)c;
        live_off[n] = off;
        ++n;
        if (status[c]) { st = status[c]; break; }
        off += out_bytes[c];
        *end_bit = land[c];
        if (final_block[c]) break;
        const uint64_t next = (land[c] - data_bit0) / chunk_bits;
        if (next <= c || next >= n_chunks) { st = kInputOverrun; break; }    // (a landing lies in a later chunk: n <= n_chunks)
        c = next;
    }
    *text_bytes = off;
    *n_live = n;
    return st;
}

// ---- a file of several members ---------------------------------------------------------------------------------------------
// A member start is FOUND like a block start: every byte offset behind the first that reads 1f 8b 08 and a FLG without
// reserved bits is a member candidate, whatever it lies in (compressed data, a stored block, another header's FNAME).  The
// candidates are kept as a list (in the order their finders arrived) with a chain per kMemberBucketBytes of the file, so
// that the link finds the one at a given offset; each has its header parsed and its first blocks walked by a wave of its own.
// The chain from member 0 then asks only for the candidate behind a trailer: every other one is dropped unseen.
constexpr uint64_t kNoMember = ~(uint64_t)0;
constexpr uint32_t kHeaderFieldLimit = 65536u;    // bytes a header's FNAME or FCOMMENT may take, its zero included
constexpr uint32_t kMemberBucketBytes = 4096u;
constexpr uint32_t kCrcSliceBytes = 1024u, kCrcGroupSlices = 64u;

GZ_FN bool member_magic(uint32_t w) {                        // the four bytes at an offset, little endian: ID1 ID2 CM FLG
    return (w & 0xffffffu) == 0x088b1fu && ((w >> 24) & 0xe0u) == 0u;
}

// The member header at byte `at` -> the offset of its DEFLATE data (the device's twin of GenerateOutput.gzip_header_bytes:
// CM = 8, no reserved flag, FEXTRA / FNAME / FCOMMENT / FHCRC skipped), kNoMember: not a header, a field that does not
// end inside the file or inside kHeaderFieldLimit, or no room for two bits of data and a trailer behind it.
GZ_FN uint64_t member_data_offset(const uint8_t* data, uint64_t n_bytes, uint64_t at) {
    if (at > n_bytes || n_bytes - at < 18u) return kNoMember;
    if (data[at] != 0x1fu || data[at + 1u] != 0x8bu || data[at + 2u] != 8u || (data[at + 3u] & 0xe0u)) return kNoMember;
    const uint32_t flg = data[at + 3u];
    uint64_t p = at + 10u;
    if (flg & 4u) {
        if (n_bytes - p < 2u) return kNoMember;
        p += 2u + ((uint32_t)data[p] | ((uint32_t)data[p + 1u] << 8));
    }
    for (uint32_t bit = 8u; bit <= 16u; bit <<= 1) {
        if (!(flg & bit)) continue;
        for (uint32_t k = 0;; ++k) {
            if (p >= n_bytes || k >= kHeaderFieldLimit) return kNoMember;
            if (data[p++] == 0u) break;
        }
    }
    if (flg & 2u) p += 2u;
    return p <= n_bytes && n_bytes - p >= 8u ? p : kNoMember;
}

// the member candidates: off[i] the offset, next[i] the chain of its bucket, head[b] the chain's first (kNoCandidate: none)
struct MemberList {
    const uint64_t* off;
    const uint32_t *next, *head;
    uint64_t n_buckets;
    uint32_t n;                      // candidates in the list
};
GZ_FN uint32_t member_find(const MemberList& l, uint64_t at) {
    const uint64_t b = at / kMemberBucketBytes;
    if (b >= l.n_buckets) return kNoCandidate;
    uint32_t i = l.head[b];
    for (uint32_t turns = 0; turns < l.n && i < l.n; ++turns) {
        if (l.off[i] == at) return i;
        i = l.next[i];
    }
    return kNoCandidate;
}

// a live member: where it lies in the file and in the text, and where its CRC slices and groups begin (the 1 KiB grid
// restarts at every member's first byte)
struct MemberRow {
    uint64_t comp_off, trailer_off, text_off, text_bytes, slice0, group0;
};
GZ_FN uint64_t crc_slices_of(uint64_t bytes) { return (bytes + kCrcSliceBytes - 1u) / kCrcSliceBytes; }
GZ_FN uint64_t crc_groups_of(uint64_t bytes) { return (crc_slices_of(bytes) + kCrcGroupSlices - 1u) / kCrcGroupSlices; }
// the member that holds slice (kGroup: group) `s`: the last row that begins at or in front of it (members without text
// share their successor's first slice and are passed over)
template <bool kGroup>
GZ_FN uint64_t member_of(const MemberRow* rows, uint64_t n_members, uint64_t s) {
    uint64_t lo = 0, hi = n_members;                         // rows[lo] begins <= s < rows[hi] begins
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if ((kGroup ? rows[mid].group0 : rows[mid].slice0) <= s) lo = mid; else hi = mid;
    }
    return lo;
}

// The walks: [0, n_chunks) from the chunks' candidates, n_chunks + i from member candidate i's data (m_start[i]: its first
// bit, kNoMember: no header).  Segments, not chunks, are live: several may begin in one chunk.
struct LinkArgs {
    const uint8_t* data;             // the file
    uint64_t n_bytes;
    const uint32_t* cand_rel;
    uint64_t n_chunks, data_bit0, chunk_bits;
    const uint64_t *land, *out_bytes;            // per walk
    const uint32_t *final_block, *status;
    const uint64_t* m_start;
    MemberList members;
    uint64_t seg_cap, row_cap;       // room in live_* and in rows
};
struct LinkResult {
    uint64_t text_bytes, n_live, n_members, end_bit, bad_member, bad_member_offset;
    uint32_t status;
};
GZ_FN uint32_t link_le32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
// Follows the landings from member 0's data: live_idx the walks on the chain, live_off their places in the text, live_mem
// the place where each one's member begins; rows the members.  At a final block: ISIZE against the member's bytes, then
// the file's end, or the candidate behind the trailer.  The status is that of the first walk or member that has one.
GZ_FN LinkResult link_members(const LinkArgs& a, uint32_t* live_idx, uint64_t* live_off, uint64_t* live_mem, MemberRow* rows) {
    LinkResult r = {0, 0, 0, 0, kNoMember, 0, kOk};
    // w: the walk; cur: the member it belongs to, which begins at byte mem_at of the file and mem_off of the text
    uint64_t w = 0, n = 0, off = 0, cur = 0, rows_made = 0, mem_off = 0, mem_at = 0, slice0 = 0, group0 = 0;
    uint64_t start = a.data_bit0;
    for (;;) {
        if (n >= a.seg_cap || cur >= a.row_cap) { r.status = kInputOverrun; break; }   // (every turn begins behind the one before)
        live_idx[n] = (uint32_t)w;
        live_off[n] = off;
        live_mem[n] = mem_off;
        ++n;
        if (a.status[w]) { r.status = a.status[w]; break; }
        const uint64_t land = a.land[w];
        if (land <= start) { r.status = kInputOverrun; break; }
        off += a.out_bytes[w];
        r.end_bit = land;
        if (!a.final_block[w]) {
            const uint64_t j = (land - a.data_bit0) / a.chunk_bits;
            if (j >= a.n_chunks || a.cand_rel[j] == kNoCandidate || a.data_bit0 + j * a.chunk_bits + a.cand_rel[j] != land) {
                r.status = kInputOverrun;
                break;
            }
            w = j;
            start = land;
            continue;
        }
        const uint64_t trailer = (land + 7u) >> 3, bytes = off - mem_off;       // (the walk ends in front of the last 8 bytes)
        if (trailer + 8u > a.n_bytes) { r.status = kInputOverrun; break; }
        const MemberRow row = {mem_at, trailer, mem_off, bytes, slice0, group0};
        rows[cur] = row;
        rows_made = cur + 1u;
        slice0 += crc_slices_of(bytes);
        group0 += crc_groups_of(bytes);
        if (link_le32(a.data + trailer + 4u) != (uint32_t)bytes) { r.status = kBadSize; break; }
        if (trailer + 8u == a.n_bytes) break;
        ++cur;
        mem_at = trailer + 8u;
        mem_off = off;
        const uint32_t i = member_find(a.members, mem_at);
        if (i == kNoCandidate || a.m_start[i] == kNoMember) { r.status = kTrailingBytes; break; }   // the host words it
        w = a.n_chunks + i;
        start = a.m_start[i];
    }
    r.text_bytes = off;
    r.n_live = n;
    r.n_members = rows_made;
    if (r.status) {
        r.bad_member = cur;
        r.bad_member_offset = mem_at;
    }
    return r;
}

// ---- a symbol's byte: `front` points at the first byte of the symbol's chunk in the text ----------------------------------
GZ_FN uint32_t resolve_symbol(uint32_t sym, const uint8_t* front) {
    return (sym & kMarker) ? front[(int64_t)(sym & 0x7fffu) - (int64_t)kWindow] : sym & 0xffu;
}

}  // namespace gz
}  // namespace besst
