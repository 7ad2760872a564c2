// The per-lane rules of the ingest's layout step (bgzf_gpu.hip: bam_decode_kernel<true>, bam_entry_scan_kernel,
// bam_entries_kernel), in plain C++: which records get a candidate entry, which lane of a workgroup decodes which record so
// that a wave's ballot IS a plane word, which plane words a workgroup may store whole and which it shares with its
// neighbours, and where a 16 384-record border falls inside a BGZF block.  The kernels add only loads, ballots and stores;
// tests/cpp/ingest_layout_core_test.cpp runs these functions lane after lane on the host.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LAYOUT_FN __host__ __device__ inline
#else
#define LAYOUT_FN inline
#endif

namespace besst {

constexpr uint32_t kLayoutTile = 16384;          // records per block of the candidate side stream (kClsTile)
constexpr uint32_t kLayoutThreads = 256;         // threads of a decode / entry workgroup

// ---- the rules per record (include/besst_amd.h: besst_lib_params.mate_bits / tid_bits, besst_cand_stream) -----------
LAYOUT_FN bool layout_mate_elsewhere(int32_t tid, int32_t mtid) { return tid != mtid; }

LAYOUT_FN bool layout_in_set(int32_t tid, int32_t mtid, uint32_t flag, uint32_t n_refs) {
    const bool read2_mapped = (flag & 0x80u) && !(flag & 0x4u);
    const bool unmapped_read1 = (flag & 0x4u) && (flag & 0x40u);
    return tid != mtid && (read2_mapped || unmapped_read1 || (uint32_t)mtid >= n_refs);
}

// ---- which lane decodes which record --------------------------------------------------------------------------------
// A workgroup owns the records [first, first + cnt) of one BGZF block.  Its threads are laid over the records from the
// plane word that holds `first`: slot s of the workgroup (turn * 256 + thread) stands for record
// (first & ~31) + s, so lanes 0-31 and 32-63 of every wave hold one aligned group of 32 records each and the halves of
// a 64-lane ballot are two plane words.  Slots in front of `first` and behind the last record are idle.
LAYOUT_FN uint32_t layout_shift(int64_t first) { return (uint32_t)(first & 31); }
LAYOUT_FN uint32_t layout_slots(int64_t first, uint32_t cnt) { return cnt ? layout_shift(first) + cnt : 0u; }
LAYOUT_FN bool layout_slot_active(int64_t first, uint32_t cnt, uint32_t slot) {
    const uint32_t shift = layout_shift(first);
    return slot >= shift && slot - shift < cnt;
}
// the first record of the plane word that slot `slot` lies in
LAYOUT_FN int64_t layout_word_first(int64_t first, uint32_t slot) { return (first & ~(int64_t)31) + (int64_t)(slot & ~31u); }

// ---- which words are the workgroup's alone --------------------------------------------------------------------------
// A word all of whose 32 records are the workgroup's is stored plainly; one that it shares with the workgroup of the
// BGZF block before or behind (or of another chunk, or with the records that were resident before) is ORed into a zeroed
// plane.  A word none of whose records is the workgroup's is not touched.
LAYOUT_FN bool layout_word_touched(int64_t word_first, int64_t first, uint32_t cnt) {
    return cnt != 0u && word_first + 32 > first && word_first < first + (int64_t)cnt;
}
LAYOUT_FN bool layout_word_whole(int64_t word_first, int64_t first, uint32_t cnt) {
    return word_first >= first && word_first + 32 <= first + (int64_t)cnt;
}

// ---- the borders of the side stream's blocks ------------------------------------------------------------------------
// offsets[r / 16384] is written by the lane that holds record r when r is a multiple of 16384: it is that record's
// entry position whether the record is in the set or not.  Index inside the BGZF block of the first such record, or -1.
LAYOUT_FN bool layout_is_border(int64_t r) { return (r & (int64_t)(kLayoutTile - 1u)) == 0; }
LAYOUT_FN int64_t layout_first_border(int64_t first, uint32_t cnt) {
    const int64_t r = (first + (int64_t)kLayoutTile - 1) & ~(int64_t)(kLayoutTile - 1u);
    return r < first + (int64_t)cnt ? r - first : -1;
}

// ---- how many entries the columns are carved for --------------------------------------------------------------------
// `entries` are there; `room` more records may come, of which `share` get an entry - plus a quarter (never more than
// `room`) and 4096, at least one more than there are (the record loop's idle lanes read one entry behind the last), a
// multiple of 64.  kLayoutDefaultShare: the share while none has been seen - every record, so that the first carving holds
// whatever the file brings.
constexpr double kLayoutDefaultShare = 1.0;
LAYOUT_FN int64_t layout_entry_cap(int64_t entries, int64_t room, double share) {
    if (room < 0) room = 0;
    double more = (double)room * share * 1.25;
    if (more > (double)room) more = (double)room;
    int64_t want = entries + (int64_t)more + 4096 + 1;
    if (want < entries + 1) want = entries + 1;
    want = (want + 63) / 64 * 64;
    return want > 0xffffffc0ll ? 0xffffffc0ll : want;        // (a context holds fewer than 2^32 records)
}

}  // namespace besst
