// The steps of the parallel gzip inflate (besst_amd/csrc/gzip_stream_core.h) on the host, against zlib: streams made by
// zlib's deflate at several levels, memLevels and strategies, with flushes and a stored block that holds DEFLATE data, are
// taken through probe, count, link, decode, windows and translation exactly as gzip_stream.hip's kernels take them - the
// wave as one lane (and the table fill as 64 lanes, one after the other) - and must give back the text.  Damaged files must
// end in a status or in a text whose CRC-32 is not the trailer's, and never leave their buffers (build this file with
// -fsanitize=address,undefined to have that checked).  Exit status 0: all good.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "../../besst_amd/csrc/gzip_stream_core.h"

namespace gz = besst::gz;

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++g_failures;                                 \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
        }                                                 \
    } while (0)

struct HostCtx {
    gz::ByteBits in;
    uint64_t bit;
    uint32_t lane, nlanes;
    std::vector<uint16_t>* sym;
    uint64_t sym0;
    void seek(uint64_t b) { bit = b; }
    uint64_t pos() const { return bit; }
    uint32_t peek() const { return in.peek(bit); }
    void drop(uint32_t n) { bit += n; }
    uint32_t byte(uint64_t i) const { return i < in.n_bytes ? in.data[i] : 0u; }
    void barrier() const {}
    uint32_t uni(uint32_t v) const { return v; }
    void store(uint64_t i, uint32_t v) const { sym->at(sym0 + i) = (uint16_t)v; }
    uint32_t load(uint64_t i) const { return sym->at(sym0 + i); }
};

uint32_t g_rng = 12345u;
uint32_t rnd() {                                            // xorshift32
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5;
    return g_rng >> 3;
}

std::string fasta_text(size_t bytes, uint32_t seed, bool repeat) {
    g_rng = seed;
    std::string t;
    int ctg = 0;
    while (t.size() < bytes) {
        char head[64];
        snprintf(head, sizeof head, ">contig_%d len=%u\n", ctg++, rnd() % 9000u);
        t += head;
        const size_t n = 200u + rnd() % 6000u;
        const size_t from = t.size();
        for (size_t i = 0; i < n; ++i) {
            t += "ACGT"[rnd() & 3u];
            if (i % 60u == 59u) t += '\n';
        }
        t += '\n';
        if (repeat && (ctg % 3) == 0 && t.size() > 33000u) t += t.substr(t.size() - 32700u - (rnd() % 60u), t.size() - from);
    }
    return t;
}

std::vector<uint8_t> raw_deflate(const std::string& text, int level, int mem_level, int strategy, size_t flush_every, int flush) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, level, Z_DEFLATED, -15, mem_level, strategy) != Z_OK) return {};
    std::vector<uint8_t> out(deflateBound(&z, (uLong)text.size()) + text.size() / (flush_every ? flush_every : text.size() + 1) * 16 + 64);
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    size_t at = 0;
    while (at < text.size()) {
        const size_t n = flush_every && text.size() - at > flush_every ? flush_every : text.size() - at;
        z.next_in = reinterpret_cast<Bytef*>(const_cast<char*>(text.data() + at));
        z.avail_in = (uInt)n;
        at += n;
        deflate(&z, at == text.size() ? Z_FINISH : flush);
    }
    if (text.empty()) deflate(&z, Z_FINISH);
    out.resize(z.total_out);
    deflateEnd(&z);
    return out;
}

std::vector<uint8_t> gzip_member(const std::vector<uint8_t>& raw, const std::string& text) {
    std::vector<uint8_t> f = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
    f.insert(f.end(), raw.begin(), raw.end());
    const uint32_t crc = (uint32_t)crc32(0, reinterpret_cast<const Bytef*>(text.data()), (uInt)text.size());
    const uint32_t isize = (uint32_t)text.size();
    for (int k = 0; k < 4; ++k) f.push_back((uint8_t)(crc >> (8 * k)));
    for (int k = 0; k < 4; ++k) f.push_back((uint8_t)(isize >> (8 * k)));
    return f;
}

struct Outcome {
    uint32_t status = 0;
    uint64_t chunks = 0, candidates = 0, live = 0;
    std::string text;
};

// the procedure of gzip_stream.hip, step by step
Outcome inflate_parallel(const std::vector<uint8_t>& file, uint64_t data_off, uint64_t chunk_bytes) {
    Outcome o;
    const gz::ByteBits in = {file.data(), file.size()};
    const uint64_t bit0 = data_off * 8u, end_bit = (file.size() - 8u) * 8u, chunk_bits = chunk_bytes * 8u;
    const uint64_t data = file.size() - 8u - data_off;
    const uint64_t n = data ? (data + chunk_bytes - 1u) / chunk_bytes : 1u;
    o.chunks = n;
    std::vector<uint32_t> cand(n, gz::kNoCandidate), status(n, 0), fin(n, 0), live_idx(n, 0);
    std::vector<uint64_t> land(n, 0), out_bytes(n, 0), live_off(n, 0);
    cand[0] = 0;
    for (uint64_t bit = bit0 + chunk_bits; bit < end_bit; ++bit) {                   // the probe
        const uint64_t j = (bit - bit0) / chunk_bits;
        if (cand[j] != gz::kNoCandidate) { bit = bit0 + (j + 1u) * chunk_bits - 1u; continue; }
        if (gz::probe_dynamic_header(in, bit, end_bit)) cand[j] = (uint32_t)(bit - bit0 - j * chunk_bits);
    }
    static gz::WalkTables tables;
    for (uint64_t j = 0; j < n; ++j) {                                               // the count
        if (cand[j] == gz::kNoCandidate) continue;
        if (j) ++o.candidates;
        HostCtx c = {in, 0, 0, 1, nullptr, 0};
        gz::WalkArgs a = {};
        a.start_bit = bit0 + j * chunk_bits + cand[j];
        a.end_bit = end_bit;
        a.cand_rel = cand.data();
        a.n_chunks = n;
        a.data_bit0 = bit0;
        a.chunk_bits = chunk_bits;
        const gz::WalkResult r = gz::walk_chunk<false>(c, tables, a);
        land[j] = r.land_bit; out_bytes[j] = r.out_bytes; fin[j] = r.final_block; status[j] = r.status;
    }
    uint64_t text_bytes = 0, n_live = 0, end = 0;                                    // the link
    o.status = gz::link_chain(land.data(), out_bytes.data(), fin.data(), status.data(), n, bit0, chunk_bits, live_idx.data(),
                              live_off.data(), &text_bytes, &n_live, &end);
    o.live = n_live;
    if (o.status) return o;
    const uint64_t trailer = (end + 7u) >> 3;
    if (trailer + 8u != file.size()) { o.status = gz::kTrailingBytes; return o; }
    uint32_t isize = 0, crc = 0;
    memcpy(&crc, file.data() + trailer, 4);
    memcpy(&isize, file.data() + trailer + 4, 4);
    if (isize != (uint32_t)text_bytes) { o.status = gz::kBadSize; return o; }
    if (text_bytes > ((uint64_t)64 << 20)) { o.status = gz::kOutputOverrun; return o; }   // (this test's texts are small)
    std::vector<uint16_t> sym(text_bytes, 0xffffu);
    for (uint64_t i = 0; i < n_live; ++i) {                                          // the decode
        const uint64_t j = live_idx[i];
        HostCtx c = {in, 0, 0, 1, &sym, live_off[i]};
        gz::WalkArgs a = {};
        a.start_bit = bit0 + j * chunk_bits + cand[j];
        a.end_bit = end_bit;
        a.stop_bit = land[j];
        a.out_cap = out_bytes[j];
        a.text_off = live_off[i];
        const uint32_t st = gz::walk_chunk<true>(c, tables, a).status;
        if (st && !o.status) o.status = st;
    }
    if (o.status) return o;
    std::vector<uint8_t> text(text_bytes + 1u, 0);
    for (uint64_t i = 0; i < n_live; ++i) {                                          // the windows
        const uint64_t off = live_off[i], len = out_bytes[live_idx[i]], tail = len < gz::kWindow ? len : gz::kWindow;
        for (uint64_t p = off + len - tail; p < off + len; ++p) text[p] = (uint8_t)gz::resolve_symbol(sym[p], text.data() + off);
    }
    for (uint64_t i = 0; i < n_live; ++i) {                                          // the translation
        const uint64_t off = live_off[i], len = out_bytes[live_idx[i]], head = len > gz::kWindow ? len - gz::kWindow : 0u;
        for (uint64_t p = off; p < off + head; ++p) text[p] = (uint8_t)gz::resolve_symbol(sym[p], text.data() + off);
    }
    o.text.assign(reinterpret_cast<const char*>(text.data()), text_bytes);
    if ((uint32_t)crc32(0, text.data(), (uInt)text_bytes) != crc) o.status = gz::kBadCrc;
    return o;
}

void check_stream(const char* name, const std::vector<uint8_t>& raw, const std::string& text, uint64_t min_live_at_1k) {
    const std::vector<uint8_t> file = gzip_member(raw, text);
    for (uint64_t chunk : {256u, 512u, 1024u, 65536u}) {
        const Outcome o = inflate_parallel(file, 10, chunk);
        CHECK(o.status == 0, "%s chunk %llu: status %u", name, (unsigned long long)chunk, o.status);
        CHECK(o.text == text, "%s chunk %llu: the text differs (%zu bytes for %zu)", name, (unsigned long long)chunk, o.text.size(), text.size());
        if (chunk == 1024u) CHECK(o.live >= min_live_at_1k, "%s: %llu live chunks at 1 KiB, %llu wanted", name, (unsigned long long)o.live,
                                  (unsigned long long)min_live_at_1k);
        printf("%-28s chunk %6llu: %5llu chunks %5llu candidates %5llu live, %zu -> %zu bytes\n", name, (unsigned long long)chunk,
               (unsigned long long)o.chunks, (unsigned long long)o.candidates, (unsigned long long)o.live, file.size(), text.size());
    }
}

void append_bits(std::vector<uint8_t>& v, const std::vector<uint8_t>& more) { v.insert(v.end(), more.begin(), more.end()); }

}  // namespace

int main() {
    // the table fill by 64 lanes, one after the other, is the fill by one
    {
        static gz::Code<288, 10> one, many;
        uint8_t lens[288];
        for (int i = 0; i < 288; ++i) lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        CHECK(gz::code_prepare(one, lens, 288) && gz::code_prepare(many, lens, 288), "the fixed code is a code");
        gz::code_fill(one, 0, 1);
        for (uint32_t lane = 0; lane < 64; ++lane) gz::code_fill(many, lane, 64);
        CHECK(memcmp(one.tab, many.tab, sizeof one.tab) == 0, "64 lanes fill the table one lane fills");
        for (uint32_t x = 0; x < 32768u; ++x) CHECK(gz::code_lookup(one, x) != 0u, "the fixed code is complete (%u)", x);
        lens[0] = 1; lens[1] = 1; lens[2] = 1;
        CHECK(!gz::code_prepare(one, lens, 288), "three codes of one bit oversubscribe");
    }
    const std::string text = fasta_text(150000, 7, false);
    for (int level : {1, 6, 9}) {
        char name[64];
        snprintf(name, sizeof name, "memLevel 1 level %d", level);
        check_stream(name, raw_deflate(text, level, 1, Z_DEFAULT_STRATEGY, 0, 0), text, 10);
    }
    check_stream("memLevel 8 level 6", raw_deflate(text, 6, 8, Z_DEFAULT_STRATEGY, 0, 0), text, 1);
    check_stream("fixed codes", raw_deflate(text.substr(0, 40000), 6, 8, Z_FIXED, 0, 0), text.substr(0, 40000), 1);
    check_stream("huffman only", raw_deflate(text, 6, 1, Z_HUFFMAN_ONLY, 0, 0), text, 10);
    check_stream("sync flushes", raw_deflate(text.substr(0, 60000), 6, 8, Z_DEFAULT_STRATEGY, 300, Z_SYNC_FLUSH), text.substr(0, 60000), 10);
    check_stream("partial flushes", raw_deflate(text.substr(0, 60000), 6, 8, Z_DEFAULT_STRATEGY, 300, Z_PARTIAL_FLUSH), text.substr(0, 60000), 10);
    check_stream("stored (level 0)", raw_deflate(text.substr(0, 70000), 0, 8, Z_DEFAULT_STRATEGY, 0, 0), text.substr(0, 70000), 1);
    check_stream("empty", raw_deflate("", 6, 8, Z_DEFAULT_STRATEGY, 0, 0), "", 1);
    const std::string rep = fasta_text(200000, 11, true);
    check_stream("repeats memLevel 1", raw_deflate(rep, 9, 1, Z_DEFAULT_STRATEGY, 0, 0), rep, 10);
    check_stream("repeats memLevel 8", raw_deflate(rep, 9, 8, Z_DEFAULT_STRATEGY, 0, 0), rep, 1);
    // stitched: dynamic / fixed / a stored block whose payload is DEFLATE data / level 0 / dynamic
    {
        const std::string a = text.substr(0, 30000), b = text.substr(30000, 8000), d = text.substr(40000, 9000), e = text.substr(50000, 30000);
        std::vector<uint8_t> inner = raw_deflate(text.substr(90000, 20000), 6, 1, Z_DEFAULT_STRATEGY, 0, 0);
        inner.resize(2048);
        const std::string c(reinterpret_cast<const char*>(inner.data()), inner.size());
        std::vector<uint8_t> raw;
        auto part = [&](const std::string& t, int level, int mem, int strategy, bool last) {
            z_stream z;
            memset(&z, 0, sizeof z);
            deflateInit2(&z, level, Z_DEFLATED, -15, mem, strategy);
            std::vector<uint8_t> out(deflateBound(&z, (uLong)t.size()) + 64);
            z.next_in = reinterpret_cast<Bytef*>(const_cast<char*>(t.data()));
            z.avail_in = (uInt)t.size();
            z.next_out = out.data();
            z.avail_out = (uInt)out.size();
            deflate(&z, last ? Z_FINISH : Z_FULL_FLUSH);
            out.resize(z.total_out);
            deflateEnd(&z);
            append_bits(raw, out);
        };
        part(a, 6, 1, Z_DEFAULT_STRATEGY, false);
        part(b, 6, 8, Z_FIXED, false);
        const uint8_t stored[5] = {0, (uint8_t)(c.size() & 0xff), (uint8_t)(c.size() >> 8), (uint8_t)(~c.size() & 0xff), (uint8_t)((~c.size() >> 8) & 0xff)};
        raw.insert(raw.end(), stored, stored + 5);
        raw.insert(raw.end(), c.begin(), c.end());
        part(d, 0, 8, Z_DEFAULT_STRATEGY, false);
        part(e, 6, 1, Z_DEFAULT_STRATEGY, true);
        check_stream("stitched", raw, a + b + c + d + e, 10);
    }
    // damage: a status or a CRC that is not the trailer's; never a byte outside the buffers
    {
        const std::vector<uint8_t> good = gzip_member(raw_deflate(text.substr(0, 50000), 6, 1, Z_DEFAULT_STRATEGY, 0, 0), text.substr(0, 50000));
        g_rng = 99;
        for (int trial = 0; trial < 60; ++trial) {
            std::vector<uint8_t> bad = good;
            if (trial < 50) bad[10 + rnd() % (bad.size() - 10)] ^= (uint8_t)(1u << (rnd() & 7u));
            else bad.resize(10 + 8 + rnd() % (bad.size() - 18));
            const Outcome o = inflate_parallel(bad, 10, trial & 1 ? 512 : 1024);
            CHECK(o.status != 0 || o.text == text.substr(0, 50000), "damage %d went unnoticed", trial);
        }
    }
    if (g_failures) fprintf(stderr, "%d checks failed\n", g_failures);
    return g_failures ? 1 : 0;
}
