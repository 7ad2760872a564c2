// The per-lane rules of the ingest's layout step (besst_amd/csrc/ingest_layout_core.h) run on the host, lane after lane, the
// way bam_decode_kernel<true>, bam_entry_scan_kernel, bam_entries_kernel and bam_layout_seams_kernel use them: a workgroup
// of 256 threads per BGZF block, ballots over the 64 lanes of a wave, plain stores for the plane words a block owns whole
// and ORs for the words it shares.  The blocks are run in REVERSE order - no workgroup waits for another -, the chunks'
// scans in order.  Input: a case file written by tests/test_ingest_layout_cpu.py with the records, the BGZF blocks' record
// counts, the chunks, and the numpy model's planes and offsets; the exit status is the verdict.
//
//   int64  n_resident, n_new, n_refs, n_blocks, n_chunks
//   uint32 count[n_blocks]            records that begin in each BGZF block
//   uint32 chunk_first[n_chunks]      first block of each chunk
//   int32  tid[T], mtid[T]; uint32 flag[T]          T = n_resident + n_new
//   uint8  mate[(T + 7) / 8], runs[...], set[...]; uint32 offsets[ceil(T / 16384) + 1]      the model's answers
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../besst_amd/csrc/ingest_layout_core.h"

using namespace besst;

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (g_failures++ < 20) {          \
                fprintf(stderr, __VA_ARGS__); \
                fprintf(stderr, "\n");        \
            }                                 \
        }                                     \
    } while (0)

template <class T>
bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

struct Planes {
    std::vector<uint32_t> mate, runs, set;
    std::vector<uint8_t> stored;      // per word: 1 = a block stored it whole (nothing else may touch it)
};

// plane_put of the kernel: a whole word is stored - and must be nobody else's -, a shared one ORed
void put(std::vector<uint32_t>& plane, std::vector<uint8_t>* stored, int64_t word_first, uint32_t bits, bool whole) {
    const size_t w = (size_t)(word_first >> 5);
    if (whole) {
        if (stored) {
            CHECK(!(*stored)[w] && plane[w] == 0u, "word %zu stored whole although another block wrote it", w);
            (*stored)[w] = 1;
        }
        plane[w] = bits;
    } else {
        if (stored) CHECK(!(*stored)[w], "word %zu ORed into although a block stored it whole", w);
        plane[w] |= bits;
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s case-file\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t head[5];
    if (fread(head, sizeof(int64_t), 5, f) != 5) return 2;
    const int64_t n_res = head[0], n_new = head[1], T = n_res + n_new;
    const uint32_t n_refs = (uint32_t)head[2];
    const size_t n_blocks = (size_t)head[3], n_chunks = (size_t)head[4];
    const size_t n_bytes = (size_t)((T + 7) / 8), n_off = (size_t)((T + kLayoutTile - 1) / kLayoutTile + 1);
    std::vector<uint32_t> count, chunk_first, flag, want_off;
    std::vector<int32_t> tid, mtid;
    std::vector<uint8_t> want_mate, want_runs, want_set;
    if (!read_vec(f, count, n_blocks) || !read_vec(f, chunk_first, n_chunks) || !read_vec(f, tid, (size_t)T) || !read_vec(f, mtid, (size_t)T) ||
        !read_vec(f, flag, (size_t)T) || !read_vec(f, want_mate, n_bytes) || !read_vec(f, want_runs, n_bytes) || !read_vec(f, want_set, n_bytes) ||
        !read_vec(f, want_off, n_off)) {
        fprintf(stderr, "short case file\n");
        return 2;
    }
    fclose(f);

    // the planes as the call finds them: valid for the resident records, zero behind them
    const size_t n_words = (size_t)(T / 32 + 2);
    Planes p;
    p.mate.assign(n_words, 0u); p.runs.assign(n_words, 0u); p.set.assign(n_words, 0u); p.stored.assign(n_words, 0);
    auto bit = [](const std::vector<uint8_t>& b, int64_t i) { return (uint32_t)(b[(size_t)(i >> 3)] >> (i & 7)) & 1u; };
    for (int64_t i = 0; i < n_res; ++i) {
        p.mate[(size_t)(i >> 5)] |= bit(want_mate, i) << (i & 31);
        p.runs[(size_t)(i >> 5)] |= bit(want_runs, i) << (i & 31);
        p.set[(size_t)(i >> 5)] |= bit(want_set, i) << (i & 31);
    }
    std::vector<uint32_t> off(n_off + 1, 0xdeadbeefu);
    uint32_t entries_before = 0;
    for (int64_t i = 0; i < n_res; ++i) entries_before += bit(want_set, i);
    for (size_t b = 0; b * kLayoutTile < (size_t)n_res; ++b) off[b] = want_off[b];   // (the resident stream's: its blocks' first entries)

    // every block's first record, and which chunk it belongs to
    std::vector<int64_t> first(n_blocks + 1, n_res);
    for (size_t b = 0; b < n_blocks; ++b) first[b + 1] = first[b] + count[b];
    CHECK(first[n_blocks] == T, "the blocks' counts do not add up to the records");
    std::vector<size_t> chunk_of(n_blocks, 0);
    for (size_t c = 0; c < n_chunks; ++c)
        for (size_t b = chunk_first[c]; b < (c + 1 < n_chunks ? chunk_first[c + 1] : n_blocks); ++b) chunk_of[b] = c;

    // ---- the decode: one workgroup per block, blocks in reverse order
    std::vector<uint32_t> set_count(n_blocks, 0u);
    std::vector<int64_t> decoded(T > 0 ? (size_t)T : 1, 0);
    for (size_t b = n_blocks; b-- > 0;) {
        const int64_t fst = first[b];
        const uint32_t cnt = count[b];
        const uint32_t slots = layout_slots(fst, cnt);
        for (uint32_t s0 = 0; s0 < slots; s0 += kLayoutThreads)
            for (uint32_t wave = 0; wave < kLayoutThreads / 64; ++wave) {
                uint64_t m_mate = 0, m_run = 0, m_set = 0;
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint32_t slot = s0 + wave * 64 + lane;
                    if (!layout_slot_active(fst, cnt, slot)) continue;
                    const uint32_t i = slot - layout_shift(fst);
                    const int64_t r = fst + i;
                    CHECK(r == layout_word_first(fst, slot) + (int64_t)(lane & 31u), "slot %u of block %zu is not bit %u of its word", slot, b, lane & 31u);
                    ++decoded[(size_t)r];
                    bool run = false;
                    if (i > 0) run = tid[(size_t)r - 1] != tid[(size_t)r];
                    else {                                   // the last record of the nearest earlier block OF THE CHUNK with records
                        size_t pb = b;
                        while (pb > chunk_first[chunk_of[b]] && count[pb - 1] == 0u) --pb;
                        if (pb > chunk_first[chunk_of[b]]) run = tid[(size_t)r - 1] != tid[(size_t)r];
                    }
                    if (layout_mate_elsewhere(tid[(size_t)r], mtid[(size_t)r])) m_mate |= 1ull << lane;
                    if (run) m_run |= 1ull << lane;
                    if (layout_in_set(tid[(size_t)r], mtid[(size_t)r], flag[(size_t)r], n_refs)) m_set |= 1ull << lane;
                }
                for (uint32_t lane = 0; lane < 64; lane += 32) {
                    const int64_t word_first = layout_word_first(fst, s0 + wave * 64 + lane);
                    if (!layout_word_touched(word_first, fst, cnt)) {
                        CHECK((uint32_t)(m_mate >> lane) == 0u && (uint32_t)(m_set >> lane) == 0u, "bits in a word the block does not touch");
                        continue;
                    }
                    const bool whole = layout_word_whole(word_first, fst, cnt);
                    put(p.mate, &p.stored, word_first, (uint32_t)(m_mate >> lane), whole);
                    put(p.runs, nullptr, word_first, (uint32_t)(m_run >> lane), whole);
                    put(p.set, nullptr, word_first, (uint32_t)(m_set >> lane), whole);
                    set_count[b] += (uint32_t)__builtin_popcount((uint32_t)(m_set >> lane));
                }
            }
    }
    for (int64_t r = n_res; r < T; ++r) CHECK(decoded[(size_t)r] == 1, "record %lld decoded %lld times", (long long)r, (long long)decoded[(size_t)r]);

    // ---- the scans, chunk after chunk, from the running total; then the entries' positions and the borders, blocks reversed
    std::vector<uint32_t> ent_base(n_blocks, 0u);
    uint32_t total = entries_before;
    for (size_t b = 0; b < n_blocks; ++b) { ent_base[b] = total; total += set_count[b]; }
    std::vector<uint32_t> entry_of;                          // record index of every entry, by position
    entry_of.assign(total, 0xffffffffu);
    for (size_t b = n_blocks; b-- > 0;) {
        const int64_t fst = first[b];
        const uint32_t cnt = count[b];
        const int64_t border = layout_first_border(fst, cnt);
        uint32_t running = ent_base[b];
        bool seen_border = false;
        for (uint32_t i = 0; i < cnt; ++i) {                 // (a lane's position: the block's base + the set records before it)
            const int64_t r = fst + i;
            if (layout_is_border(r)) {
                CHECK(!seen_border ? (int64_t)i == border : (r - fst - border) % kLayoutTile == 0, "border of block %zu not where layout_first_border says", b);
                seen_border = true;
                off[(size_t)(r / kLayoutTile)] = running;
            }
            if (layout_in_set(tid[(size_t)r], mtid[(size_t)r], flag[(size_t)r], n_refs)) {
                CHECK(running < total && entry_of[running] == 0xffffffffu, "two records at entry %u", running);
                if (running < total) entry_of[running] = (uint32_t)r;
                ++running;
            }
        }
        CHECK(seen_border == (border >= 0), "block %zu: layout_first_border disagrees with the records", b);
    }
    // ---- the seams: the chunks' first records, and the last offset
    for (size_t c = 0; c < n_chunks; ++c) {
        const int64_t r = first[chunk_first[c]];
        if (r < T && (r == 0 || tid[(size_t)r] != tid[(size_t)r - 1])) p.runs[(size_t)(r >> 5)] |= 1u << (r & 31);
    }
    off[(size_t)((T + kLayoutTile - 1) / kLayoutTile)] = total;

    // ---- against the model
    for (int64_t i = 0; i < (int64_t)n_bytes * 8; ++i) {
        const size_t w = (size_t)(i >> 5);
        const uint32_t sh = (uint32_t)(i & 31);
        CHECK(((p.mate[w] >> sh) & 1u) == bit(want_mate, i), "mate bit %lld", (long long)i);
        CHECK(((p.runs[w] >> sh) & 1u) == bit(want_runs, i), "run bit %lld", (long long)i);
        CHECK(((p.set[w] >> sh) & 1u) == bit(want_set, i), "set bit %lld", (long long)i);
    }
    for (size_t b = 0; b < n_off; ++b) CHECK(off[b] == want_off[b], "offset %zu: %u, the model says %u", b, off[b], want_off[b]);
    uint32_t e = entries_before;
    for (int64_t r = n_res; r < T; ++r)
        if (bit(want_set, r)) {
            CHECK(e < total && entry_of[e] == (uint32_t)r, "entry %u is not record %lld", e, (long long)r);
            ++e;
        }
    CHECK(e == total, "entries: %u, the model says %u", total, e);
    // ---- the carving: always room for one entry more than there are, a multiple of 64, never more than a record each
    for (int64_t ent : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)64, (int64_t)100000})
        for (int64_t room : {(int64_t)0, (int64_t)1, (int64_t)5000, (int64_t)1 << 20})
            for (double share : {0.0, 0.01, 0.25, 1.0}) {
                const int64_t cap = layout_entry_cap(ent, room, share);
                CHECK(cap % 64 == 0 && cap >= ent + 1 && cap <= ent + room + 4096 + 1 + 63, "layout_entry_cap(%lld, %lld, %g) = %lld", (long long)ent,
                      (long long)room, share, (long long)cap);
            }
    CHECK(layout_entry_cap((int64_t)1 << 32, (int64_t)1 << 32, 1.0) <= 0xffffffc0ll, "the capacity must fit 32 bits");
    if (g_failures) { fprintf(stderr, "%d check(s) failed\n", g_failures); return 1; }
    printf("ok: %lld + %lld records, %zu blocks, %zu chunks, %u entries\n", (long long)n_res, (long long)n_new, n_blocks, n_chunks, total);
    return 0;
}
