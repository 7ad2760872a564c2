// Host program over besst_amd/csrc/seq_census_core.h, the census record and its merge rule, for tests/test_seq_census_core.py.
//
//   seq_census_core_test classes
//       prints "class <byte> <word> <lower>" for every byte value
//   seq_census_core_test <stream> <table> <min_gap> <window>
//       <stream>: the bytes.  <table>: "offset length" per line, ascending and disjoint.  The stream is walked in windows of
//       <window> bytes; the bytes of every row inside a window are pushed one by one into a partial census, which is merged
//       into the row's accumulator as the right-hand neighbour.  Prints "part <row> <16 words>" for every row, then
//       "final <row> <16 words>" after census_finalise, and "order <first row out of order, or -1>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../besst_amd/csrc/seq_census_core.h"

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

static void print_row(const char* what, size_t row, const int64_t* w) {
    printf("%s %zu", what, row);
    for (int k = 0; k < besst_census::kWords; ++k) printf(" %lld", (long long)w[k]);
    printf("\n");
}

int main(int argc, char** argv) {
    using namespace besst_census;
    if (argc == 2 && argv[1][0] == 'c') {
        for (uint32_t b = 0; b < 256; ++b) printf("class %u %d %d\n", b, census_class(b), census_is_lower(b) ? 1 : 0);
        return 0;
    }
    if (argc != 5) { fprintf(stderr, "usage: seq_census_core_test classes | <stream> <table> <min_gap> <window>\n"); return 2; }
    // exactly the file's bytes on the heap: a read past either end is the sanitizer's to report
    const std::vector<uint8_t> stream = slurp(argv[1]);
    std::vector<int64_t> off, len;
    {
        FILE* fh = fopen(argv[2], "r");
        if (!fh) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
        long long o, l;
        while (fscanf(fh, "%lld %lld", &o, &l) == 2) { off.push_back(o); len.push_back(l); }
        fclose(fh);
    }
    const int64_t min_gap = atoll(argv[3]), window = atoll(argv[4]), n = (int64_t)stream.size();
    const size_t rows = off.size();
    if (window < 1) { fprintf(stderr, "window must be positive\n"); return 2; }
    int64_t bad = -1;
    for (size_t i = 0; i < rows && bad < 0; ++i)
        if (!census_row_in_order(off.data(), len.data(), (int64_t)i)) bad = (int64_t)i;
    std::vector<int64_t> acc(rows * kWords + 1, 0);
    if (bad < 0) {
        for (int64_t lo = 0; lo < n; lo += window) {
            const int64_t hi = lo + window < n ? lo + window : n;
            for (int64_t i = census_first_row(off.data(), (int64_t)rows, lo); i < (int64_t)rows && off[(size_t)i] < hi; ++i) {
                const int64_t s = off[(size_t)i] > lo ? off[(size_t)i] : lo;
                const int64_t e = off[(size_t)i] + len[(size_t)i] < hi ? off[(size_t)i] + len[(size_t)i] : hi;
                if (e <= s) continue;
                int64_t part[kWords];
                census_clear(part);
                for (int64_t p = s; p < e; ++p) census_push(part, stream[(size_t)p], min_gap);
                census_merge(&acc[(size_t)i * kWords], part, min_gap, &acc[(size_t)i * kWords]);
            }
        }
    }
    for (size_t i = 0; i < rows; ++i) print_row("part", i, &acc[i * kWords]);
    for (size_t i = 0; i < rows; ++i) {
        census_finalise(&acc[i * kWords], min_gap);
        print_row("final", i, &acc[i * kWords]);
    }
    printf("order %lld\n", (long long)bad);
    return 0;
}
