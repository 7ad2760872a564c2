// Stand-alone test of besst_amd/csrc/bgzf_scan.h: the BGZF header walk, the boundary search, the part cut and the chunk
// plan on hand-made blocks.  Only headers and trailers matter (payload bytes are filler); every buffer is allocated at
// exactly its length, so a read one byte past a window is a read past an allocation.  Exit status 0: every check held.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../besst_amd/csrc/bgzf_scan.h"

using namespace besst;

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

typedef std::vector<uint8_t> Bytes;

// one BGZF block: 18 + extra + payload + 8 bytes
static Bytes block(size_t payload, uint32_t isize, size_t extra = 0, uint32_t crc = 0x01020304u) {
    const size_t total = 18 + extra + payload + 8;
    Bytes b(total, 0xAA);
    const uint8_t head[12] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, (uint8_t)(6 + extra), 0};
    memcpy(b.data(), head, 12);
    b[12] = 'B'; b[13] = 'C'; b[14] = 2; b[15] = 0;
    b[16] = (uint8_t)((total - 1) & 255); b[17] = (uint8_t)((total - 1) >> 8);
    for (int i = 0; i < 4; ++i) {
        b[total - 8 + i] = (uint8_t)(crc >> (8 * i));
        b[total - 4 + i] = (uint8_t)(isize >> (8 * i));
    }
    return b;
}

static Bytes join(const std::vector<Bytes>& blocks) {
    Bytes all;
    for (const Bytes& b : blocks) all.insert(all.end(), b.begin(), b.end());
    return all;
}

// the bytes on the heap, at exactly their length
struct Exact {
    std::unique_ptr<uint8_t[]> p;
    size_t len;
    explicit Exact(const Bytes& b) : Exact(b, b.size()) {}
    Exact(const Bytes& b, size_t n) : p(new uint8_t[n]), len(n) { memcpy(p.get(), b.data(), n); }   // the first n bytes of b
    const uint8_t* get() const { return p.get(); }
};

struct Scan {
    bool ok;
    size_t fpos = 0, comp = 0, inflated = 0;
    uint32_t n = 0;
    std::unique_ptr<BgzfBlock[]> d;
};
static Scan scan(const Exact& m, size_t max_blocks, size_t comp_cap, bool more_follows = false, size_t dst0 = 0, bool back_to_back = false) {
    Scan s;
    s.d.reset(new BgzfBlock[max_blocks]);
    s.ok = scan_bgzf_chunk(m.get(), m.len, &s.fpos, max_blocks, comp_cap, s.d.get(), &s.n, &s.comp, &s.inflated, more_follows, dst0, back_to_back);
    return s;
}
static uint64_t dst_of(const BgzfBlock& b) { return ((uint64_t)b.dst_off_hi << 32) | b.dst_off_lo; }

static void test_scan() {
    const Bytes b0 = block(7, 5), b1 = block(2, 0), b2 = block(100, 65536);
    const Exact three(join({b0, b1, b2}));
    const size_t cap = (size_t)1 << 20;
    {   // aligned mode
        const Scan s = scan(three, 3, cap);
        CHECK(s.ok && s.n == 3 && s.fpos == three.len && s.comp == three.len);
        CHECK(dst_of(s.d[0]) == 0 && dst_of(s.d[1]) == 256 && dst_of(s.d[2]) == 256);
        CHECK(s.inflated == 256 + 65536);
        CHECK(s.d[0].src_off == 18 && s.d[0].src_len == 7 && s.d[0].dst_len == 5 && s.d[0].crc == 0x01020304u);
        CHECK(s.d[1].src_off == b0.size() + 18 && s.d[1].src_len == 2 && s.d[1].dst_len == 0);
        CHECK(s.d[2].src_off == b0.size() + b1.size() + 18 && s.d[2].src_len == 100 && s.d[2].dst_len == 65536);
    }
    {   // back to back behind 4 MiB
        const size_t at = (size_t)4 << 20;
        const Scan s = scan(three, 3, cap, false, at, true);
        CHECK(s.ok && s.n == 3);
        CHECK(dst_of(s.d[0]) == at && dst_of(s.d[1]) == at + 5 && dst_of(s.d[2]) == at + 5);
        CHECK(s.inflated == 5 + 65536);
    }
    {   // a place beyond 32 bits
        const Scan s = scan(three, 3, cap, false, (size_t)1 << 32, true);
        CHECK(s.ok && s.d[0].dst_off_hi == 1 && s.d[0].dst_off_lo == 0 && s.d[1].dst_off_hi == 1 && s.d[1].dst_off_lo == 5);
    }
    {   // XLEN = 10: four extra bytes behind the BC subfield
        const Exact m(block(9, 3, 4));
        const Scan s = scan(m, 1, cap);
        CHECK(s.ok && s.n == 1 && s.d[0].src_off == 22 && s.d[0].src_len == 9 && s.d[0].dst_len == 3 && s.fpos == m.len);
    }
    {   // stops: max_blocks, comp_cap, a cap below the first block
        Scan s = scan(three, 2, cap);
        CHECK(s.ok && s.n == 2 && s.fpos == b0.size() + b1.size() && s.comp == s.fpos);
        s = scan(three, 3, b0.size() + b1.size() + b2.size() - 1);
        CHECK(s.ok && s.n == 2 && s.fpos == b0.size() + b1.size());
        s = scan(three, 3, b0.size() - 1);
        CHECK(!s.ok);
    }
    {   // a window that ends inside a header / one byte short of a block
        const Exact in_header(join({b0, b2}), b0.size() + 17), short_one(join({b0, b2}), b0.size() + b2.size() - 1);
        for (const Exact* m : {&in_header, &short_one}) {
            Scan s = scan(*m, 3, cap, true);
            CHECK(s.ok && s.n == 1 && s.fpos == b0.size() && s.comp == b0.size());
            s = scan(*m, 3, cap, false);
            CHECK(!s.ok);
        }
    }
    // not a BGZF block
    struct Bad { const char* what; Bytes b; };
    std::vector<Bad> bad;
    { Bytes b = block(9, 3); b[1] = 140; bad.push_back({"magic", b}); }
    { Bytes b = block(9, 3); b[3] = 0; bad.push_back({"FEXTRA clear", b}); }
    { Bytes b = block(9, 3); b[10] = 5; bad.push_back({"XLEN 5", b}); }
    { Bytes b = block(9, 3); b[13] = 'D'; bad.push_back({"subfield", b}); }
    { Bytes b = block(9, 3); b[14] = 3; bad.push_back({"SLEN 3", b}); }
    { Bytes b = block(9, 3); b[16] = 16; b[17] = 0; bad.push_back({"BSIZE + 1 < 18", b}); }
    { Bytes b = block(7, 3, 4); b[16] = 28; b.resize(29); bad.push_back({"trailer does not fit", b}); }   // rest 11 < 4 + 8
    { bad.push_back({"ISIZE 65537", block(9, 65537)}); }
    for (const Bad& c : bad) {
        const Exact m(c.b);
        const Scan s = scan(m, 2, cap);
        if (s.ok) fprintf(stderr, "accepted: %s\n", c.what);
        CHECK(!s.ok);
    }
}

static void test_boundary() {
    // block 1's payload spells a complete header (BSIZE + 1 = 30) with filler where its successor would begin
    Bytes decoy = block(60, 1);
    const Bytes fake = block(4, 0);
    memcpy(decoy.data() + 18 + 10, fake.data(), 18);
    const std::vector<Bytes> blocks = {block(30, 1), decoy, block(50, 1), block(10, 1), block(2, 0)};
    std::vector<size_t> start;
    size_t at = 0;
    for (const Bytes& b : blocks) { start.push_back(at); at += b.size(); }
    const Exact m(join(blocks));
    CHECK(find_bgzf_boundary(m.get(), m.len, start[0] + 20) == start[1]);       // the middle of a block
    CHECK(find_bgzf_boundary(m.get(), m.len, start[2]) == start[2]);            // on a start
    CHECK(find_bgzf_boundary(m.get(), m.len, start[1] + 28) == start[2]);       // on the decoy
    CHECK(find_bgzf_boundary(m.get(), m.len, start[1] + 1) == start[2]);        // in front of it
    CHECK(find_bgzf_boundary(m.get(), m.len, start[3] + 1) == start[4]);        // the file's last block
    CHECK(find_bgzf_boundary(m.get(), m.len, m.len - 27) == m.len);
    CHECK(find_bgzf_boundary(m.get(), m.len, m.len) == m.len);
    const Exact twenty(blocks[0], 20);
    CHECK(find_bgzf_boundary(twenty.get(), twenty.len, 0) == 20);
}

static void test_part_cut() {
    std::vector<Bytes> blocks(10, block(74, 1));             // ten blocks of 100 bytes
    const Exact m(join(blocks));
    auto is_start = [&](size_t x) { return x % 100 == 0 && x <= m.len; };
    {
        const BgzfPart p = cut_bgzf_part(m.get(), m.len, 100, 7, 0, 1);
        CHECK(p.begin == 100 && p.end == m.len && p.u0 == 7);
    }
    {
        BgzfPart p[3];
        for (int k = 0; k < 3; ++k) p[k] = cut_bgzf_part(m.get(), m.len, 0, 9, k, 3);
        CHECK(p[0].begin == 0 && p[0].end == p[1].begin && p[1].end == p[2].begin && p[2].end == m.len);
        for (int k = 0; k < 3; ++k) CHECK(is_start(p[k].begin) && is_start(p[k].end) && p[k].begin < p[k].end);
        CHECK(p[0].u0 == 9 && p[1].u0 == 0 && p[2].u0 == 0);
    }
    {   // the reader stands at block 5: the cut at a third of the file (block 4) clamps to it, the one at two thirds (block 7) holds
        BgzfPart p[3];
        for (int k = 0; k < 3; ++k) p[k] = cut_bgzf_part(m.get(), m.len, 500, 9, k, 3);
        CHECK(p[0].begin == 500 && p[0].end == 500 && p[0].u0 == 9);
        CHECK(p[1].begin == 500 && p[1].end == 700 && p[1].u0 == 9);
        CHECK(p[2].begin == 700 && p[2].end == m.len && p[2].u0 == 0);
    }
}

static void check_plan_bounds(const BgzfChunkPlan& p) {
    CHECK(p.comp_cap % 4096 == 0 && p.comp_cap >= ((size_t)1 << 20) && p.comp_cap <= ((size_t)160 << 20));
    CHECK(p.nbw == p.nb + 1 && p.desc_bytes % 4096 == 0 && p.desc_bytes >= p.nbw * sizeof(BgzfBlock));
    CHECK(p.slot_bytes == p.desc_bytes + p.comp_cap + 4096 && p.inflated_cap == kBgzfTailRoom + p.nb * 65536 + 4096);
}

static void test_chunk_plan() {
    {   // five blocks: a file of fewer blocks than the smallest chunk
        const Exact m(join(std::vector<Bytes>(5, block(74, 1))));
        const BgzfChunkPlan p = plan_bgzf_chunks(m.get(), m.len, 0, 5120);
        CHECK(p.nb == 64 && p.comp_cap == ((size_t)1 << 20) && p.first_per_block == 0.0);
        check_plan_bounds(p);
    }
    {   // 40 blocks of 60000 bytes = 2 400 000 bytes, all of them seen: blocks = 40 < 64 -> nb = 64;
        // guess = align_up(60000 * 64 * 1.35 + 4 MiB, 4096) = align_up(5 184 000 + 4 194 304 = 9 378 304) = 2290 * 4096 = 9 379 840;
        // the file holds less: align_up(2 400 000 + 65536 = 2 465 536, 4096) = 602 * 4096 = 2 465 792 (above the 1 MiB floor)
        const Exact m(join(std::vector<Bytes>(40, block(60000 - 26, 1))));
        CHECK(m.len == 2400000);
        const BgzfChunkPlan p = plan_bgzf_chunks(m.get(), m.len, 0, 5120);
        CHECK(p.nb == 64 && p.comp_cap == 2465792 && p.first_per_block == 60000.0);
        CHECK(p.desc_bytes == 4096 && p.slot_bytes == 2473984 && p.inflated_cap == 8392704);
        check_plan_bounds(p);
        // the same file for chunks of 16 blocks: guess = align_up(60000 * 16 * 1.35 + 4 MiB = 5 490 304, 4096) = 1341 * 4096,
        // above what the file holds
        const BgzfChunkPlan q = plan_bgzf_chunks(m.get(), m.len, 0, 16);
        CHECK(q.nb == 16 && q.comp_cap == 2465792);
        check_plan_bounds(q);
    }
    {   // 300 blocks of 100 bytes from the second block on: 256 seen (25 600 bytes), 29 900 to go through:
        // blocks = 29900 / 100 * 1.25 + 64 = 437 (truncated from 437.75); comp_cap: the file holds less than the 1 MiB floor
        const Exact m(join(std::vector<Bytes>(300, block(74, 1))));
        const BgzfChunkPlan p = plan_bgzf_chunks(m.get(), m.len, 100, 5120);
        CHECK(p.nb == 437 && p.comp_cap == ((size_t)1 << 20) && p.first_per_block == 100.0);
        check_plan_bounds(p);
    }
}

int main() {
    test_scan();
    test_boundary();
    test_part_cut();
    test_chunk_plan();
    if (g_failed) fprintf(stderr, "%d check(s) failed\n", g_failed);
    else printf("bgzf_scan: all checks passed\n");
    return g_failed ? 1 : 0;
}
