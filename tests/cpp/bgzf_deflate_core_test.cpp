// The steps of the BGZF compressor (besst_amd/csrc/bgzf_deflate_core.h) run lane after lane on the host, in the order the
// kernel runs them between its barriers, and every block handed to zlib: raw inflate of the block's DEFLATE data ALONE must
// end exactly at the trailer and give the payload back.  The CRC is zlib's here (the kernel has its own).  Exit status 0:
// every case held.  Build: c++ -std=c++17 bgzf_deflate_core_test.cpp -lz
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "../../besst_amd/csrc/bgzf_deflate_core.h"

using namespace besst::deflate;

static int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
            ++g_failed;                                   \
        }                                                 \
    } while (0)

// one block, the way bgzf_deflate_encode_kernel does it -> the block's bytes
static std::vector<uint8_t> encode_block(const uint8_t* buf, size_t buf_len, size_t at, uint32_t len, bool* stored_out) {
    static BlockState s;
    memset(&s, 0, sizeof(s));
    const uint8_t* in = buf + at;
    std::vector<ByteReader> rd;
    uint32_t lo[kThreads], hi[kThreads];
    for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) {
        span_of(len, t, &lo[t], &hi[t]);
        ByteReader r(in);
        r.host_lo = buf;
        r.host_hi = buf + buf_len;
        rd.push_back(r);
    }
    for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) count_step(s, rd[t], lo[t], hi[t], t);
    s.crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), in, len);
    for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) lengths_rank(s.freq, kNumLit, s.len, s.w, t);
    lengths_serial(kLitLimit, s.len, s.w);
    for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) lengths_codes(kNumLit, s.len, s.code, s.w, t);
    for (uint32_t c = 0; c < (uint32_t)kNumLit; ++c) CHECK(s.len[c] <= kLitLimit && (s.len[c] != 0) == (s.freq[c] != 0), "literal length of %u", c);
    header_rle(s);
    s.w.n_used = 0;
    for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) lengths_rank(s.cl_freq, kNumCl, s.cl_len, s.w, t);
    lengths_serial(kClLimit, s.cl_len, s.w);
    for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) lengths_codes(kNumCl, s.cl_len, s.cl_code, s.w, t);
    {
        uint32_t kraft = 0;
        for (uint32_t c = 0; c < (uint32_t)kNumCl; ++c) {
            CHECK(s.cl_len[c] <= kClLimit, "code-length length of %u", c);
            if (s.cl_len[c]) kraft += 1u << (kClLimit - s.cl_len[c]);
        }
        CHECK(kraft == 1u << kClLimit, "the code-length code is not complete: %u", kraft);
    }
    header_finish(s);
    uint32_t bit = 0;
    for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) {
        s.start[t] = bit;
        bit += measure_step(s, rd[t], lo[t], hi[t], t);
    }
    s.start[kThreads] = bit;
    const uint32_t end_bit = bit;
    std::vector<uint8_t> out;
    *stored_out = takes_stored_form(end_bit, len);
    if (*stored_out) {
        const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        out.assign(head, head + 16);
        const uint32_t bsize = kHeaderBytes + kStoredBytes + len + kTrailerBytes;
        out.push_back((uint8_t)((bsize - 1) & 0xff)); out.push_back((uint8_t)((bsize - 1) >> 8));
        out.push_back(1);
        out.push_back((uint8_t)(len & 0xff)); out.push_back((uint8_t)(len >> 8));
        out.push_back((uint8_t)(~len & 0xff)); out.push_back((uint8_t)((~len >> 8) & 0xff));
        out.insert(out.end(), in, in + len);
        for (int k = 0; k < 4; ++k) out.push_back((uint8_t)(s.crc >> (8 * k)));
        for (int k = 0; k < 4; ++k) out.push_back((uint8_t)(len >> (8 * k)));
        return out;
    }
    std::vector<uint32_t> slot(kSlotStride / 4, 0xdeadbeefu);      // (stale words: every word of the block must be written)
    std::vector<BitWriter> bw(kThreads);
    for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) {
        bw[t].begin(slot.data(), s, t);
        write_step(s, bw[t], rd[t], lo[t], hi[t], t, len, end_bit);
    }
    for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) bw[t].finish(t);
    const uint32_t size = ((end_bit + 7u) >> 3) + kTrailerBytes;
    out.resize(size);
    memcpy(out.data(), slot.data(), size);
    return out;
}

static std::vector<uint8_t> compress(const std::vector<uint8_t>& data, uint32_t payload, size_t* n_stored = nullptr) {
    std::vector<uint8_t> file;
    if (n_stored) *n_stored = 0;
    for (size_t at = 0; at < data.size(); at += payload) {
        const uint32_t len = (uint32_t)(data.size() - at < payload ? data.size() - at : payload);
        bool stored = false;
        const std::vector<uint8_t> block = encode_block(data.data(), data.size(), at, len, &stored);
        if (n_stored && stored) ++*n_stored;
        CHECK(block.size() <= (size_t)len + 31u, "a block of %zu bytes for %u", block.size(), len);
        // the block alone, through zlib
        CHECK(block.size() >= 26 && block[0] == 0x1f && block[3] == 4 && block[12] == 'B', "header");
        const uint32_t bsize = (uint32_t)block[16] + ((uint32_t)block[17] << 8) + 1u;
        CHECK(bsize == block.size(), "BSIZE %u of %zu", bsize, block.size());
        std::vector<uint8_t> back(len + 1u);
        z_stream z;
        memset(&z, 0, sizeof(z));
        CHECK(inflateInit2(&z, -15) == Z_OK, "inflateInit2");
        z.next_in = const_cast<uint8_t*>(block.data()) + 18;
        z.avail_in = (uInt)(block.size() - 18 - 8);
        z.next_out = back.data();
        z.avail_out = (uInt)back.size();
        const int rc = inflate(&z, Z_FINISH);
        CHECK(rc == Z_STREAM_END, "inflate: %d (%s) at block %zu, payload %u, %s", rc, z.msg ? z.msg : "", at / payload, payload, stored ? "stored" : "dynamic");
        CHECK(z.avail_in == 0, "%u bytes in front of the trailer unused", z.avail_in);
        CHECK(z.total_out == len && memcmp(back.data(), data.data() + at, len) == 0, "the payload came back different");
        inflateEnd(&z);
        uint32_t isize = 0;
        memcpy(&isize, block.data() + block.size() - 4, 4);
        CHECK(isize == len, "ISIZE");
        file.insert(file.end(), block.begin(), block.end());
    }
    return file;
}

static size_t zlib_level(const std::vector<uint8_t>& data, uint32_t payload, int level) {
    size_t total = 0;
    std::vector<uint8_t> out(payload + 1024);
    for (size_t at = 0; at < data.size(); at += payload) {
        const uint32_t len = (uint32_t)(data.size() - at < payload ? data.size() - at : payload);
        z_stream z;
        memset(&z, 0, sizeof(z));
        deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
        z.next_in = const_cast<uint8_t*>(data.data()) + at;
        z.avail_in = len;
        z.next_out = out.data();
        z.avail_out = (uInt)out.size();
        deflate(&z, Z_FINISH);
        total += z.total_out + 26;
        deflateEnd(&z);
    }
    return total;
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

static std::vector<uint8_t> scaffold_text(size_t n) {
    std::vector<uint8_t> v;
    int k = 0;
    while (v.size() < n) {
        if (rnd() % 8 == 0) {
            const std::string h = (v.empty() ? ">scaffold_" : "\n>scaffold_") + std::to_string(++k) + "_uid_1700000000\n";
            v.insert(v.end(), h.begin(), h.end());
        }
        const uint32_t bases = 200 + rnd() % 20000;
        for (uint32_t i = 0; i < bases; ++i) v.push_back("ACGT"[rnd() & 3]);
        const uint32_t gap = 1 + rnd() % 2000;
        if (rnd() % 4 == 0) v.push_back('n');
        else v.insert(v.end(), gap, 'N');
    }
    v.resize(n);
    return v;
}

int main() {
    const uint32_t payloads[] = {65280, 16, 255, 256, 257, 4096};
    // lengths around nothing and around a block
    for (uint32_t p : payloads) {
        const size_t lens[] = {0, 1, 2, 3, 4, 5, p - 1, p, p + 1, 2 * (size_t)p, 2 * (size_t)p + 1};
        for (size_t n : lens) {
            std::vector<uint8_t> one(n, 'N'), two(n), acgt(n);
            for (size_t i = 0; i < n; ++i) { two[i] = (uint8_t)("AN"[(i / 3) & 1]); acgt[i] = (uint8_t)"ACGT"[rnd() & 3]; }
            compress(one, p); compress(two, p); compress(acgt, p);
        }
    }
    // runs that start, end and straddle block and span borders
    for (uint32_t p : {16u, 255u, 256u, 257u, 4096u}) {
        const uint32_t runs[] = {2, 3, 4, 5, 6, 257, 258, 259, 260, 261, 262, 263, 515, 516, 517, 518, 519, 520};
        for (uint32_t run : runs) {
            for (int place = 0; place < 3; ++place) {        // the run starts at, ends at, lies across border + shift
                for (int shift = -3; shift <= 3; ++shift) {
                    std::vector<uint8_t> v(3 * (size_t)p + 1200);
                    for (auto& c : v) c = (uint8_t)"ACGT"[rnd() & 3];
                    for (long border : {600L + (long)p, 600L + 2 * (long)p}) {
                        const long from = border + shift - (place == 0 ? 0L : place == 1 ? (long)run : (long)run / 2);
                        for (long i = from; i < from + (long)run; ++i) v[(size_t)i] = 'N';
                    }
                    // (the text begins 600 bytes into its buffer's blocks: cut that off so that the borders fall on p and 2 p)
                    compress(std::vector<uint8_t>(v.begin() + 600, v.end()), p);
                }
            }
        }
    }
    {   // 259, 262 and a whole block of equal bytes
        for (size_t n : {259u, 262u, 65280u}) compress(std::vector<uint8_t>(n, 'x'), 65280);
    }
    {   // random bytes: stored, exactly payload + 31
        std::vector<uint8_t> v(70000);
        for (auto& c : v) c = (uint8_t)rnd();
        size_t stored = 0;
        const auto file = compress(v, 65280, &stored);
        CHECK(stored == 2 && file.size() == v.size() + 2 * 31, "random bytes: %zu blocks stored, %zu bytes", stored, file.size());
    }
    {   // 22 symbols with Fibonacci counts: the unlimited tree is 21 deep
        std::vector<uint8_t> v;
        uint32_t a = 1, b = 1;
        for (int k = 0; k < 22; ++k) {
            v.insert(v.end(), a, (uint8_t)('A' + k));
            const uint32_t c = a + b; a = b; b = c;
        }
        CHECK(v.size() <= 65280, "Fibonacci payload of %zu bytes", v.size());
        compress(v, 65280);                                  // sorted: runs
        for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[rnd() % i]);
        compress(v, 65280);
    }
    // seeded payloads: alphabets of 1..256 symbols, four frequency shapes
    for (int k = 0; k < 300; ++k) {
        const uint32_t alphabet = 1 + rnd() % 256, shape = k & 3;
        const uint32_t p = payloads[rnd() % 6];
        const size_t n = 1 + rnd() % (3 * (size_t)(p < 4096 ? p : 4096));
        std::vector<uint8_t> v(n);
        for (auto& c : v) {
            uint32_t sym;
            if (shape == 0) sym = rnd() % alphabet;
            else if (shape == 1) { sym = 0; while (sym + 1 < alphabet && (rnd() & 1)) ++sym; }
            else if (shape == 2) { sym = (uint32_t)((double)alphabet / (1.0 + (rnd() % 1000))) % alphabet; }
            else { sym = 0; uint32_t r = rnd(); while (sym + 1 < alphabet && (r % 1000) < 618) { ++sym; r = rnd(); } }
            c = (uint8_t)(sym * 37u + (uint32_t)k);
        }
        compress(v, p);
    }
    {   // size: scaffold-like text against zlib level 1 on the same blocks
        const auto v = scaffold_text(1 << 20);
        const auto file = compress(v, 65280);
        const size_t z1 = zlib_level(v, 65280, 1), z6 = zlib_level(v, 65280, 6);
        printf("1 MiB of scaffold text: %zu bytes, zlib level 1 %zu, level 6 %zu\n", file.size(), z1, z6);
        CHECK(file.size() <= z1, "larger than zlib level 1");
        // the same bytes twice
        const auto again = compress(v, 65280);
        CHECK(again == file, "a second run gave other bytes");
    }
    if (g_failed) printf("%d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
