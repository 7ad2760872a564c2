// The host's reading of BGZF block headers for the device ingest (ingest.hip): the descriptors of a chunk's blocks, the
// block boundary nearest to a place in the file, the cut of a file into parts and the sizes of an ingest's chunks.  Plain
// C++ over bytes in memory - no HIP, no reader -, so that tests/cpp/bgzf_scan_test.cpp can call it as it stands.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace besst {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct BgzfBlock {             // one BGZF block of a chunk: its DEFLATE payload in the chunk's compressed bytes, its place in
    uint32_t src_off, src_len; // the chunk's inflated scratch (256-byte aligned) and ISIZE
    uint32_t dst_off_lo, dst_off_hi;
    uint32_t dst_len, crc;     // and the CRC-32 of the inflated bytes from the gzip trailer
};

inline uint32_t bgzf_le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t bgzf_le32(const uint8_t* p) { return bgzf_le16(p) | (bgzf_le16(p + 2) << 16); }

// The BGZF blocks of [*fpos, ...) that fit one chunk: descriptors with offsets relative to the chunk's first byte,
// inflated places 256-byte aligned.  Stops at max_blocks, at comp_cap compressed bytes, or at the end of the file.
// false: not a BGZF block where one should be.
// dst0 / back_to_back: where the first block's bytes go and whether the blocks follow each other without padding (the
// ingest: a record may run on into the next block) or at 256-byte boundaries (the inflate test hook)
inline bool scan_bgzf_chunk(const uint8_t* map, size_t map_len, size_t* fpos, size_t max_blocks, size_t comp_cap, BgzfBlock* out,
                            uint32_t* n_out, size_t* comp_bytes, size_t* inflated_bytes, bool more_follows = false, size_t dst0 = 0,
                            bool back_to_back = false) {
    const size_t begin = *fpos;
    size_t at = begin, dst = dst0;
    uint32_t n = 0;
    while (n < max_blocks && at < map_len) {
        const uint8_t* hdr = map + at;
        if (map_len - at < 18) {                             // `map` is a window of the file: the block continues behind it
            if (more_follows) break;
            return false;
        }
        if (hdr[0] != 31 || hdr[1] != 139 || hdr[2] != 8 || !(hdr[3] & 4)) return false;
        const uint32_t xlen = bgzf_le16(hdr + 10);
        if (xlen < 6 || hdr[12] != 'B' || hdr[13] != 'C' || bgzf_le16(hdr + 14) != 2) return false;
        const size_t bsize = (size_t)bgzf_le16(hdr + 16) + 1;
        if (bsize < 18) return false;
        if (map_len - at < bsize) {
            if (more_follows) break;
            return false;
        }
        const size_t rest = bsize - 18, extra_left = xlen - 6;
        if (rest < extra_left + 8) return false;
        if (at + bsize - begin > comp_cap) {
            if (n == 0) return false;                        // (a block is at most 64 KiB: the cap is far larger)
            break;
        }
        const uint32_t isize = bgzf_le32(hdr + bsize - 4);
        if (isize > 65536u) return false;
        BgzfBlock& b = out[n++];
        b.src_off = (uint32_t)(at + 18 + extra_left - begin);
        b.src_len = (uint32_t)(rest - extra_left - 8);
        b.dst_off_lo = (uint32_t)dst;
        b.dst_off_hi = (uint32_t)((uint64_t)dst >> 32);
        b.dst_len = isize;
        b.crc = bgzf_le32(hdr + bsize - 8);
        dst += back_to_back ? (size_t)isize : align_up((size_t)isize, 256);
        at += bsize;
    }
    *fpos = at;
    *n_out = n;
    *comp_bytes = at - begin;
    *inflated_bytes = dst - dst0;
    return true;
}

// A whole byte range as a chain of BGZF blocks, by scan_bgzf_chunk's rules (any further extra subfields behind BC, empty
// blocks anywhere, no EOF block needed): the blocks up to the first byte that is no whole BGZF block, max_blocks at most.
// `end` equals map_len when the range is BGZF to its last byte.  What sizes a reader's buffers and tells it, before
// anything is allocated, whether the device inflate can take the file.
struct BgzfWalk {
    uint64_t n_blocks, inflated_bytes;
    size_t end;
};
inline BgzfWalk walk_bgzf(const uint8_t* map, size_t map_len, uint64_t max_blocks = ~(uint64_t)0) {
    BgzfWalk w{0, 0, 0};
    while (w.n_blocks < max_blocks && w.end < map_len) {
        BgzfBlock b;
        uint32_t n = 0;
        size_t at = w.end, comp = 0, inflated = 0;
        // (more_follows: a block cut by the end of the range ends the walk like any other byte that is no block)
        if (!scan_bgzf_chunk(map, map_len, &at, 1, ~(size_t)0, &b, &n, &comp, &inflated, true, 0, true) || n == 0) break;
        w.n_blocks += 1;
        w.inflated_bytes += inflated;
        w.end = at;
    }
    return w;
}

// First BGZF block boundary at or behind `from`: the gzip magic with the BC subfield, a plausible BSIZE, and two further
// blocks (or the end of the file) chained behind it - payload bytes that happen to spell a header do not survive that.
inline size_t find_bgzf_boundary(const uint8_t* map, size_t map_len, size_t from) {
    auto block_at = [&](size_t at, size_t* bsize) {
        if (map_len - at < 28) return false;
        const uint8_t* h = map + at;
        if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4) || bgzf_le16(h + 10) < 6 || h[12] != 'B' || h[13] != 'C' || bgzf_le16(h + 14) != 2)
            return false;
        *bsize = (size_t)bgzf_le16(h + 16) + 1;
        return *bsize >= 28 && *bsize <= map_len - at;
    };
    for (size_t at = from; at + 28 <= map_len; ++at) {
        size_t b0 = 0, b1 = 0, b2 = 0;
        if (!block_at(at, &b0)) continue;
        const size_t n1 = at + b0;
        if (n1 == map_len) return at;
        if (!block_at(n1, &b1)) continue;
        const size_t n2 = n1 + b1;
        if (n2 == map_len || block_at(n2, &b2)) return at;
    }
    return map_len;
}

// Part `part` of `parts` of the records of a file whose next unread record lies u0 bytes into the block at f0: the file is
// cut at the BGZF block boundaries nearest to part / parts of its bytes, never in front of f0.  One part is the file as
// it is; a part that does not begin at f0 begins with its first block's first byte.
struct BgzfPart {
    size_t begin, end;
    uint32_t u0;
};
inline BgzfPart cut_bgzf_part(const uint8_t* map, size_t file_len, size_t f0, uint32_t u0, int32_t part, int32_t parts) {
    if (parts <= 1) return BgzfPart{f0, file_len, u0};
    auto cut = [&](int32_t k) -> size_t {
        if (k <= 0) return f0;
        if (k >= parts) return file_len;
        const size_t at = find_bgzf_boundary(map, file_len, (size_t)((double)file_len * (double)k / (double)parts));
        return at < f0 ? f0 : at;
    };
    const size_t begin = cut(part);
    const size_t end = cut(part + 1);
    return BgzfPart{begin, end < begin ? begin : end, begin != f0 ? 0u : u0};
}

// The chunks of an ingest of [f0, map_len): nb blocks or comp_cap compressed bytes, whichever comes first.  The staging
// slots are pinned (~70 us per MB to allocate and release), so they are sized from the file's first blocks - ~5 KB each in
// a file of constant qualities, ~18 KB in a sequencer's - with a third in hand; denser blocks further on just make a
// chunk hold fewer.  A file (or part) of fewer blocks than a chunk gets slots for what it holds: every slot carries
// 64 KiB of inflated scratch per block, 0.5 GB at the default chunk, whatever the file's size.
constexpr size_t kBgzfTailRoom = (size_t)4 << 20;            // bytes a chunk may carry into the next one (one record)
struct BgzfChunkPlan {
    size_t nb, comp_cap;
    double first_per_block;      // compressed bytes per block over the file's first blocks (0: fewer than 16 seen)
    size_t nbw;                  // descriptors per chunk: descriptor 0 is the slot for the tail of the chunk before
    size_t desc_bytes, slot_bytes, inflated_cap;
};
inline BgzfChunkPlan plan_bgzf_chunks(const uint8_t* map, size_t map_len, size_t f0, size_t chunk_blocks) {
    BgzfChunkPlan p{};
    p.nb = chunk_blocks;
    p.comp_cap = (size_t)160 << 20;
    size_t at = f0, seen = 0;
    while (seen < 256 && at + 18 <= map_len && map[at] == 31 && map[at + 1] == 139) {
        at += (size_t)bgzf_le16(map + at + 16) + 1;
        ++seen;
    }
    if (seen >= 1 && at <= map_len + 65536) {
        const double per_block = (double)(at - f0) / (double)seen;
        if (seen >= 16) p.first_per_block = per_block;
        const size_t blocks = at >= map_len ? seen : (size_t)((double)(map_len - f0) / per_block * 1.25) + 64;
        if (blocks < p.nb) p.nb = blocks < 64 ? 64 : blocks;
    }
    if (seen >= 16 && at <= map_len) {
        const size_t guess = align_up((size_t)((double)(at - f0) / (double)seen * (double)p.nb * 1.35) + ((size_t)4 << 20), 4096);
        if (guess < p.comp_cap) p.comp_cap = guess;
    }
    if (p.comp_cap > map_len - f0 + 65536) p.comp_cap = align_up(map_len - f0 + 65536, 4096);
    if (p.comp_cap < ((size_t)1 << 20)) p.comp_cap = (size_t)1 << 20;
    p.nbw = p.nb + 1;
    p.desc_bytes = align_up(p.nbw * sizeof(BgzfBlock), 4096);
    p.slot_bytes = p.desc_bytes + p.comp_cap + 4096;         // (the bit reader's windows run up to 512 bytes past a payload)
    p.inflated_cap = kBgzfTailRoom + p.nb * 65536 + 4096;
    return p;
}

}  // namespace besst
