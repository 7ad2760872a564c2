// Host program over besst_amd/csrc/sam_core.h, the per-record rules of the SAM reader, for tests/test_sam_core.py.
//
//   sam_core_test <names> <records> [<queries>]
//
// <names>: the reference names, one per line.  <records>: record lines ('\n' ends a line, a last line without one is a
// line).  For every line the program finds the line's end and its tabs 1, 9 and 10 the way the index pass leaves them,
// calls sam_decode_line and prints "<offset> ok tid mtid pos mpos tlen flag mapq qlen rlen alen saturated" or
// "<offset> err <reason>".  <queries>: names, one per line; "row <r>" is printed for each (the table probe alone).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../besst_amd/csrc/sam_core.h"

static std::vector<uint8_t> slurp(const char* path) {
    FILE* fh = fopen(path, "rb");
    if (!fh) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<uint8_t> out;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), fh)) > 0) out.insert(out.end(), buf, buf + got);
    fclose(fh);
    return out;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: sam_core_test <names> <records> [<queries>]\n"); return 2; }
    const std::vector<uint8_t> names = slurp(argv[1]);
    std::vector<uint8_t> pool;
    std::vector<int64_t> off(1, 0);
    for (size_t at = 0; at < names.size();) {
        const void* nl = memchr(names.data() + at, '\n', names.size() - at);
        const size_t end = nl ? (size_t)((const uint8_t*)nl - names.data()) : names.size();
        pool.insert(pool.end(), names.begin() + (long)at, names.begin() + (long)end);
        off.push_back((int64_t)pool.size());
        at = end + 1;
    }
    const int64_t n_ref = (int64_t)off.size() - 1;
    const uint32_t cap = besst_sam::table_capacity(n_ref);
    std::vector<uint32_t> slots(cap ? cap : 1, 0u);
    if (pool.empty()) pool.push_back(0);
    const int64_t twice = besst_sam::build_table(pool.data(), off.data(), n_ref, slots.data(), cap);
    if (twice >= 0) { printf("duplicate %lld\n", (long long)twice); return 0; }
    const besst_sam::RefTable table{slots.data(), cap, pool.data(), off.data()};
    printf("table %lld %u\n", (long long)n_ref, cap);

    // exactly the file's bytes on the heap: a read past either end is the sanitizer's to report
    const std::vector<uint8_t> text = slurp(argv[2]);
    const int64_t n = (int64_t)text.size();
    for (int64_t s = 0; s < n;) {
        int64_t e = s;
        uint32_t tabs = 0, tab1 = besst_sam::kNoOffset, tab9 = besst_sam::kNoOffset, tab10 = besst_sam::kNoOffset;
        while (e < n && text[(size_t)e] != '\n') {
            if (text[(size_t)e] == '\t') {
                ++tabs;
                if (tabs == 1) tab1 = (uint32_t)e;
                if (tabs == 9) tab9 = (uint32_t)e;
                if (tabs == 10) tab10 = (uint32_t)e;
            }
            ++e;
        }
        besst_sam::Record r{};
        const uint32_t reason = besst_sam::sam_decode_line(text.data(), s, e, tab1, tab9, tab10, table, &r);
        if (reason) printf("%lld err %u\n", (long long)s, reason);
        else
            printf("%lld ok %d %d %d %d %d %u %u %u %d %d %u\n", (long long)s, r.tid, r.mtid, r.pos, r.mpos, r.tlen,
                   (unsigned)r.flag, (unsigned)r.mapq, (unsigned)r.qlen, r.rlen, r.alen, r.saturated);
        s = e + 1;
    }
    if (argc > 3) {
        const std::vector<uint8_t> q = slurp(argv[3]);
        for (size_t at = 0; at < q.size();) {
            const void* nl = memchr(q.data() + at, '\n', q.size() - at);
            const size_t end = nl ? (size_t)((const uint8_t*)nl - q.data()) : q.size();
            printf("row %d\n", besst_sam::lookup_name(table, q.data(), (int64_t)at, (int64_t)end));
            at = end + 1;
        }
    }
    return 0;
}
