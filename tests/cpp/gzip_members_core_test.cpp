// The steps of the parallel inflate of a gzip file of SEVERAL members (besst_amd/csrc/gzip_stream_core.h: member_magic,
// member_data_offset, member_find, link_members, member_of, and walk_chunk's distance rule relative to the member) on the
// host, against zlib: the files tests/gzip_members_design.py builds, handed over as one binary (argv[1]; per file: a name of
// 64 bytes, its length as 8 bytes little endian, its bytes), are taken through mark, probe, count, link, decode, windows,
// translation and the per-member CRC exactly as gzip_stream.hip's kernels take them - the wave as one lane.  A file zlib
// reads as a series of members must give its text at every chunk size and list capacity that holds its candidates; a
// file zlib refuses must end in a status.  No byte outside the buffers (build with -fsanitize=address,undefined to have
// that checked).  Exit status 0: all good.
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

// zlib on a series of members -> true and the text, false where it refuses the file
bool zlib_members(const std::vector<uint8_t>& file, std::string* text) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 31) != Z_OK) return false;
    z.next_in = const_cast<Bytef*>(file.data());
    z.avail_in = (uInt)file.size();
    std::vector<uint8_t> buf(1 << 16);
    bool ok = true, at_end = false;
    while (ok) {
        z.next_out = buf.data();
        z.avail_out = (uInt)buf.size();
        const int r = inflate(&z, Z_NO_FLUSH);
        text->append(reinterpret_cast<const char*>(buf.data()), buf.size() - z.avail_out);
        if (r == Z_STREAM_END) {
            at_end = true;
            if (z.avail_in == 0) break;
            at_end = false;
            ok = inflateReset(&z) == Z_OK;
        } else if (r != Z_OK) {
            ok = false;
        } else if (z.avail_in == 0 && z.avail_out != 0) {
            ok = false;                                      // the file ends inside a member
        }
    }
    inflateEnd(&z);
    return ok && at_end;
}

struct Outcome {
    uint32_t status = 0;
    uint64_t chunks = 0, candidates = 0, live = 0, members = 0, member_candidates = 0, bad_member = 0;
    std::string text;
};

// the procedure of besst_dev_gzip_members_plan / _inflate, step by step
Outcome inflate_members(const std::vector<uint8_t>& file, uint64_t chunk_bytes, uint64_t cap) {
    Outcome o;
    const uint64_t size = file.size();
    const uint64_t data_off = gz::member_data_offset(file.data(), size, 0);
    if (data_off == gz::kNoMember) { o.status = gz::kTrailingBytes; return o; }
    const gz::ByteBits in = {file.data(), size};
    const uint64_t bit0 = data_off * 8u, end_bit = (size - 8u) * 8u, chunk_bits = chunk_bytes * 8u;
    const uint64_t data = size - 8u - data_off;
    const uint64_t n = data ? (data + chunk_bytes - 1u) / chunk_bytes : 1u;
    o.chunks = n;
    const uint64_t walks = n + cap, n_buckets = size / gz::kMemberBucketBytes + 1u;
    std::vector<uint32_t> cand(n, gz::kNoCandidate), status(walks, 0), fin(walks, 0), live_idx(walks, 0), m_next(cap + 1u, 0),
        m_head(n_buckets, gz::kNoCandidate);
    std::vector<uint64_t> land(walks, 0), out_bytes(walks, 0), live_off(walks, 0), live_mem(walks, 0), m_off(cap + 1u, 0), m_start(cap + 1u, 0);
    std::vector<gz::MemberRow> rows(cap + 1u);
    cand[0] = 0;
    for (uint64_t at = 1; at + 4u <= size; ++at) {                                   // the marks
        uint32_t w = 0;
        memcpy(&w, file.data() + at, 4);
        if (!gz::member_magic(w)) continue;
        const uint64_t slot = o.member_candidates++;
        if (slot < cap) {
            m_off[slot] = at;
            m_next[slot] = m_head[at / gz::kMemberBucketBytes];
            m_head[at / gz::kMemberBucketBytes] = (uint32_t)slot;
        }
    }
    if (o.member_candidates > cap) { o.status = gz::kTooManyMembers; return o; }
    for (uint64_t bit = bit0 + chunk_bits; bit < end_bit; ++bit) {                   // the probe
        const uint64_t j = (bit - bit0) / chunk_bits;
        if (cand[j] != gz::kNoCandidate) { bit = bit0 + (j + 1u) * chunk_bits - 1u; continue; }
        if (gz::probe_dynamic_header(in, bit, end_bit)) cand[j] = (uint32_t)(bit - bit0 - j * chunk_bits);
    }
    static gz::WalkTables tables;
    auto count = [&](uint64_t w, uint64_t start) {
        HostCtx c = {in, 0, 0, 1, nullptr, 0};
        gz::WalkArgs a = {};
        a.start_bit = start;
        a.end_bit = end_bit;
        a.cand_rel = cand.data();
        a.n_chunks = n;
        a.data_bit0 = bit0;
        a.chunk_bits = chunk_bits;
        const gz::WalkResult r = gz::walk_chunk<false>(c, tables, a);
        land[w] = r.land_bit; out_bytes[w] = r.out_bytes; fin[w] = r.final_block; status[w] = r.status;
    };
    for (uint64_t j = 0; j < n; ++j) {                                               // the count: chunks ...
        if (cand[j] == gz::kNoCandidate) continue;
        if (j) ++o.candidates;
        count(j, bit0 + j * chunk_bits + cand[j]);
    }
    for (uint64_t i = 0; i < o.member_candidates; ++i) {                             // ... and member candidates
        const uint64_t at = gz::member_data_offset(file.data(), size, m_off[i]);
        m_start[i] = at == gz::kNoMember ? gz::kNoMember : at * 8u;
        status[n + i] = gz::kInputOverrun;
        if (at != gz::kNoMember) count(n + i, at * 8u);
    }
    gz::LinkArgs la;                                                                 // the link
    la.data = file.data();
    la.n_bytes = size;
    la.cand_rel = cand.data();
    la.n_chunks = n;
    la.data_bit0 = bit0;
    la.chunk_bits = chunk_bits;
    la.land = land.data();
    la.out_bytes = out_bytes.data();
    la.final_block = fin.data();
    la.status = status.data();
    la.m_start = m_start.data();
    la.members = {m_off.data(), m_next.data(), m_head.data(), n_buckets, (uint32_t)o.member_candidates};
    la.seg_cap = walks;
    la.row_cap = cap + 1u;
    const gz::LinkResult lr = gz::link_members(la, live_idx.data(), live_off.data(), live_mem.data(), rows.data());
    o.status = lr.status;
    o.live = lr.n_live;
    o.members = lr.n_members;
    o.bad_member = lr.bad_member;
    if (o.status) return o;
    const uint64_t text_bytes = lr.text_bytes;
    if (text_bytes > ((uint64_t)64 << 20)) { o.status = gz::kOutputOverrun; return o; }   // (this test's texts are small)
    std::vector<uint16_t> sym(text_bytes, 0xffffu);
    for (uint64_t i = 0; i < lr.n_live; ++i) {                                       // the decode
        const uint64_t w = live_idx[i];
        HostCtx c = {in, 0, 0, 1, &sym, live_off[i]};
        gz::WalkArgs a = {};
        a.start_bit = w < n ? bit0 + w * chunk_bits + cand[w] : m_start[w - n];
        a.end_bit = end_bit;
        a.stop_bit = land[w];
        a.out_cap = out_bytes[w];
        a.text_off = live_off[i];
        a.member_off = live_mem[i];
        const uint32_t st = gz::walk_chunk<true>(c, tables, a).status;
        if (st && !o.status) o.status = st;
    }
    if (o.status) return o;
    std::vector<uint8_t> text(text_bytes + 1u, 0);
    for (uint64_t i = 0; i < lr.n_live; ++i) {                                       // the windows
        const uint64_t off = live_off[i], len = out_bytes[live_idx[i]], tail = len < gz::kWindow ? len : gz::kWindow;
        for (uint64_t p = off + len - tail; p < off + len; ++p) text[p] = (uint8_t)gz::resolve_symbol(sym[p], text.data() + off);
    }
    for (uint64_t i = 0; i < lr.n_live; ++i) {                                       // the translation
        const uint64_t off = live_off[i], len = out_bytes[live_idx[i]], head = len > gz::kWindow ? len - gz::kWindow : 0u;
        for (uint64_t p = off; p < off + head; ++p) text[p] = (uint8_t)gz::resolve_symbol(sym[p], text.data() + off);
    }
    o.text.assign(reinterpret_cast<const char*>(text.data()), text_bytes);
    // the CRC: every slice and group finds its member, the rows tile the text
    const gz::MemberRow last = rows[lr.n_members - 1u];
    const uint64_t n_slices = last.slice0 + gz::crc_slices_of(last.text_bytes), n_groups = last.group0 + gz::crc_groups_of(last.text_bytes);
    uint64_t covered = 0;
    for (uint64_t s = 0; s < n_slices; ++s) {
        const gz::MemberRow row = rows[gz::member_of<false>(rows.data(), lr.n_members, s)];
        const uint64_t in_member = (s - row.slice0) * gz::kCrcSliceBytes;
        CHECK(s >= row.slice0 && in_member < row.text_bytes, "slice %llu lies in no member", (unsigned long long)s);
        if (in_member < row.text_bytes) covered += row.text_bytes - in_member < gz::kCrcSliceBytes ? row.text_bytes - in_member : gz::kCrcSliceBytes;
    }
    CHECK(covered == text_bytes, "the slices cover %llu bytes of %llu", (unsigned long long)covered, (unsigned long long)text_bytes);
    for (uint64_t g = 0; g < n_groups; ++g) {
        const gz::MemberRow row = rows[gz::member_of<true>(rows.data(), lr.n_members, g)];
        CHECK(g >= row.group0 && g - row.group0 < gz::crc_groups_of(row.text_bytes), "group %llu lies in no member", (unsigned long long)g);
    }
    for (uint64_t m = 0; m < lr.n_members && !o.status; ++m) {
        uint32_t crc = 0;
        memcpy(&crc, file.data() + rows[m].trailer_off, 4);
        if ((uint32_t)crc32(0, text.data() + rows[m].text_off, (uInt)rows[m].text_bytes) != crc) {
            o.status = gz::kBadCrc;
            o.bad_member = m;
        }
    }
    return o;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s FILES.bin\n", argv[0]);
        return 2;
    }
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    int n_files = 0;
    for (;;) {
        char name[65] = {0};
        uint8_t len8[8];
        if (fread(name, 1, 64, fh) != 64) break;
        if (fread(len8, 1, 8, fh) != 8) { CHECK(false, "%s: no length", name); break; }
        uint64_t len = 0;
        for (int k = 0; k < 8; ++k) len |= (uint64_t)len8[k] << (8 * k);
        std::vector<uint8_t> file(len);
        if (len > ((uint64_t)1 << 24) || fread(file.data(), 1, len, fh) != len) { CHECK(false, "%s: cut", name); break; }
        ++n_files;
        std::string want;
        const bool good = zlib_members(file, &want);
        for (uint64_t chunk : {256u, 1024u, 65536u}) {
            const Outcome o = inflate_members(file, chunk, file.size() / 256u + 4096u);
            if (good) {
                CHECK(o.status == 0, "%s chunk %llu: status %u (member %llu)", name, (unsigned long long)chunk, o.status, (unsigned long long)o.bad_member);
                CHECK(o.text == want, "%s chunk %llu: the text differs (%zu bytes for %zu)", name, (unsigned long long)chunk, o.text.size(), want.size());
            } else {
                CHECK(o.status != 0, "%s chunk %llu: zlib refuses the file, the steps take it", name, (unsigned long long)chunk);
            }
            printf("%-28s chunk %6llu: status %2u %5llu chunks %5llu candidates %5llu live %5llu members %5llu member candidates\n", name,
                   (unsigned long long)chunk, o.status, (unsigned long long)o.chunks, (unsigned long long)o.candidates, (unsigned long long)o.live,
                   (unsigned long long)o.members, (unsigned long long)o.member_candidates);
            // the list's capacity: exactly the candidates is enough, one fewer is too many
            if (good && chunk == 1024u && o.member_candidates) {
                const Outcome at = inflate_members(file, chunk, o.member_candidates), under = inflate_members(file, chunk, o.member_candidates - 1u);
                CHECK(at.status == 0 && at.text == want, "%s: a list of exactly its candidates: status %u", name, at.status);
                CHECK(under.status == gz::kTooManyMembers, "%s: a list one short: status %u", name, under.status);
            }
        }
    }
    fclose(fh);
    CHECK(n_files > 0, "no file in %s", argv[1]);
    if (g_failures) fprintf(stderr, "%d checks failed\n", g_failures);
    return g_failures ? 1 : 0;
}
