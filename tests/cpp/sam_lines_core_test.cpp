// Host run of the line cutter's rule (besst_amd/csrc/sam_lines_core.h), lane after lane as the kernel of csrc/sam.hip walks a
// text: 64 lanes of 16 bytes a round, the byte in front of a slice handed on from the slice before, a lane's answers joined
// at the end.  Built by tests/test_sam_stream_model.py with -Wall -Wextra -fsanitize=address,undefined.
//
//   sam_lines_core_test TEXT [N WANT_HEADER_END COUNT_UPTO]...
//
// For every query: the text is the file's first N bytes in a buffer of N rounded up to 16 - what the kernel may read -,
// the bytes behind N are the file's (or 0xff), so that they have to be masked.  Prints out[0] out[1] out[2] out[3].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../besst_amd/csrc/sam_lines_core.h"

namespace L = besst_sam_lines;

int main(int argc, char** argv) {
    if (argc < 2 || (argc - 2) % 3) {
        std::fprintf(stderr, "usage: %s TEXT [N WANT_HEADER_END COUNT_UPTO]...\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> file;
    if (FILE* fh = std::fopen(argv[1], "rb")) {
        uint8_t buf[65536];
        size_t got;
        while ((got = std::fread(buf, 1, sizeof(buf), fh)) > 0) file.insert(file.end(), buf, buf + got);
        std::fclose(fh);
    } else {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    for (int q = 2; q + 2 < argc; q += 3) {
        const int64_t n = std::atoll(argv[q]), upto = std::atoll(argv[q + 2]);
        const bool want = std::atoi(argv[q + 1]) != 0;
        if (n < 0 || (size_t)n > file.size() || upto < 0 || upto > n) {
            std::fprintf(stderr, "query out of range\n");
            return 2;
        }
        const size_t room = ((size_t)n + 15) / 16 * 16;
        std::vector<uint8_t> text(room ? room : 16, 0xff);
        std::memcpy(text.data(), file.data(), room < file.size() ? room : file.size());
        L::Acc lanes[64];
        for (auto& a : lanes) a = L::acc_none();
        uint32_t before = 1u;                                    // byte 0 opens a line
        for (int64_t off = 0; off < n; off += 16) {
            uint32_t w[4];
            std::memcpy(w, text.data() + off, 16);
            const L::Slice s = L::slice_masks(w, n - off);
            L::acc_slice(lanes[(off / 16) % 64], s, before, off, n, upto, want);
            before = (s.nl >> 15) & 1u;
        }
        L::Acc all = L::acc_none();
        for (int k = 63; k >= 0; --k) L::acc_join(all, lanes[k]);
        std::printf("%u %lld %u 0\n", all.last_end, all.first_rec == L::kNone ? -1ll : (long long)all.first_rec, all.newlines);
    }
    return 0;
}
