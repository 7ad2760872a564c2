// Stand-alone test of walk_bgzf (besst_amd/csrc/bgzf_scan.h): a byte range as a chain of BGZF blocks, up to the first byte
// that is no whole block.  Only headers and trailers matter (payload bytes are filler); every buffer is allocated at exactly
// its length, so a read one byte past a range is a read past an allocation (build with -fsanitize=address,undefined to
// have it reported).  Exit status 0: every check held.
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
static Bytes block(size_t payload, uint32_t isize, size_t extra = 0) {
    const size_t total = 18 + extra + payload + 8;
    Bytes b(total, 0xAA);
    const uint8_t head[12] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, (uint8_t)(6 + extra), 0};
    memcpy(b.data(), head, 12);
    b[12] = 'B'; b[13] = 'C'; b[14] = 2; b[15] = 0;
    b[16] = (uint8_t)((total - 1) & 255); b[17] = (uint8_t)((total - 1) >> 8);
    for (int i = 0; i < 4; ++i) b[total - 4 + i] = (uint8_t)(isize >> (8 * i));
    return b;
}

static Bytes join(const std::vector<Bytes>& blocks) {
    Bytes all;
    for (const Bytes& b : blocks) all.insert(all.end(), b.begin(), b.end());
    return all;
}

// the walk of the first n bytes of b, held on the heap at exactly that length
static BgzfWalk walk(const Bytes& b, size_t n, uint64_t max_blocks = ~(uint64_t)0) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
    if (n) memcpy(p.get(), b.data(), n);
    return walk_bgzf(p.get(), n, max_blocks);
}
static BgzfWalk walk(const Bytes& b) { return walk(b, b.size()); }
static bool is(const BgzfWalk& w, uint64_t n_blocks, uint64_t inflated, size_t end) {
    return w.n_blocks == n_blocks && w.inflated_bytes == inflated && w.end == end;
}

int main() {
    const Bytes data = block(40, 100), empty = block(2, 0), full = block(300, 65536), sub = block(9, 7, 10);
    CHECK(is(walk(Bytes()), 0, 0, 0));
    // layouts that are BGZF to the last byte: empty blocks first, in the middle and last, no EOF block, a second subfield
    CHECK(is(walk(join({data, full, empty})), 3, 65636, data.size() + full.size() + empty.size()));
    CHECK(is(walk(join({empty, data, empty, empty, full, empty})), 6, 65636, data.size() + full.size() + 4 * empty.size()));
    CHECK(is(walk(join({data, full})), 2, 65636, data.size() + full.size()));
    CHECK(is(walk(join({sub, data, sub})), 3, 114, data.size() + 2 * sub.size()));
    CHECK(is(walk(join({empty, empty})), 2, 0, 2 * empty.size()));
    {   // sums beyond 32 bits
        std::vector<Bytes> many(70000, block(1, 65536));
        CHECK(is(walk(join(many)), 70000, (uint64_t)70000 * 65536, (size_t)70000 * 27));
    }
    const Bytes three = join({data, sub, full});
    const size_t at1 = data.size(), at2 = data.size() + sub.size();
    // max_blocks: the offset of block k
    CHECK(is(walk(three, three.size(), 0), 0, 0, 0));
    CHECK(is(walk(three, three.size(), 1), 1, 100, at1));
    CHECK(is(walk(three, three.size(), 2), 2, 107, at2));
    CHECK(is(walk(three, three.size(), 3), 3, 65643, three.size()));
    CHECK(is(walk(three, three.size(), 9), 3, 65643, three.size()));
    // every cut: the walk ends in front of the block the cut goes through
    for (size_t n = 0; n <= three.size(); ++n) {
        const BgzfWalk w = walk(three, n);
        const size_t end = n < at1 ? 0 : n < at2 ? at1 : n < three.size() ? at2 : three.size();
        CHECK(w.end == end && w.n_blocks == (uint64_t)(end == 0 ? 0 : end == at1 ? 1 : end == at2 ? 2 : 3));
    }
    // something else behind the chain, and every header scan_bgzf_chunk rejects: the walk ends in front of it
    std::vector<Bytes> bad;
    for (int k = 0; k < 12; ++k) bad.push_back(sub);
    bad[0][0] = 30;                                              // magic
    bad[1][1] = 138;
    bad[2][2] = 7;                                               // not DEFLATE
    bad[3][3] = 0;                                               // no FEXTRA
    bad[4][10] = 5;                                              // XLEN too small for BC
    bad[5][12] = 'X';                                            // another subfield first
    bad[6][13] = 'X';
    bad[7][14] = 3;                                              // BC's length
    bad[8][16] = 16; bad[8][17] = 0;                             // BSIZE smaller than a header
    bad[9][10] = 200;                                            // XLEN larger than the block
    bad[10][sub.size() - 1] = 1;                                 // ISIZE > 65536
    bad[11][16] = 255; bad[11][17] = 255;                        // BSIZE beyond the range's end
    for (size_t k = 0; k < bad.size(); ++k) {
        CHECK(is(walk(join({data, bad[k], data})), 1, 100, at1));
        CHECK(is(walk(join({bad[k]})), 0, 0, 0));
    }
    Bytes gzip_member = {31, 139, 8, 0, 0, 0, 0, 0, 0, 3, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // what gzip makes of no bytes
    CHECK(is(walk(join({data, gzip_member})), 1, 100, at1));
    CHECK(is(walk(join({data, empty, Bytes(10, 0x5A)})), 2, 100, at1 + empty.size()));
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("bgzf_walk_test: ok\n");
    return 0;
}
