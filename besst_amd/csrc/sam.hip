// SAM text, read on the device: one chunk of record lines in HBM -> the context's eight record columns.
//
// The chunk begins at a line start and ends at a line end or at the end of the file.  '\n' ends a line (a '\r' in front
// of it belongs to the terminator), a last line without '\n' is a line.  A record is the first eleven tab-separated
// fields of a line; the per-record rules are sam_core.h's.  Where a line's fields lie depends on two facts that cross
// tile borders: how many lines begin in front of a byte (the line's row) and how many tabs precede it in its line (the
// tab's ordinal, counted up to 11).  One wave owns one tile of tile_bytes and walks it in rounds of 1 KiB, 16 bytes per
// lane, '\n' and '\t' each a 16-bit mask:
//
//   flags_kernel    per tile: holds a newline / the tabs behind its last newline (all its tabs without one) / the
//                   lines that begin in it
//   state_kernel    one workgroup: the tab ordinal at every tile's entry by a forward composition of those flags, the
//                   exclusive sum of the line counts, the total to the info block
//   index_kernel    the same walk with its entry state: the lane that holds a line's first byte, its tab 1, 9 or 10 or
//                   its '\n' writes that offset into the line's row (five columns of 32-bit offsets in the chunk); a
//                   row keeps "none" where the line has no such tab
//   decode_kernel   one lane per record, from its row: fields 2-9 are the bytes between tab 1 and tab 9 (numbers, the
//                   CIGAR walk, RNAME / RNEXT through the reference table), l_seq is tab 10 - tab 9 - 1; the eight
//                   column stores are coalesced across lanes
//
// No pass walks SEQ, QUAL or the optional fields a byte per lane, a line may span any number of tiles, and no order
// depends on an atomic: a record's row is its line's rank.  Errors are a status: the smallest offending file offset (the
// line's first byte) with the line's reason code below it in one word, by 64-bit atomicMin.
//
// The line cutter (besst_dev_sam_lines) serves a reader that fills a buffer with inflated text and has to know where its
// last whole line ends without fetching the text: one pass of the same 16-byte loads and newline masks, a wave per run of
// rounds, the rule of a slice in sam_lines_core.h; a wave reduces by shuffles and adds at most one atomic per answer.
#include <vector>

#include "common.h"
#include "context.h"
#include "sam_core.h"
#include "sam_lines_core.h"

namespace besst {

namespace {

using namespace besst_sam;

constexpr int kSamWaves = 4;                                     // tiles per workgroup
constexpr int kSamThreads = kSamWaves * 64;
constexpr int64_t kSamRound = 64 * 16;
constexpr int64_t kSamMinTile = kSamRound, kSamMaxTile = 64 * kSamRound, kSamDefaultTile = 16 * kSamRound;
constexpr int kSamScanThreads = 1024;
constexpr int kSamDecodeThreads = 256;
constexpr uint32_t kTabSat = 11u;
constexpr uint32_t kElemNl = 16u;                                // a span as one byte: holds a newline | tabs behind the last

typedef uint32_t sam_u32x4 __attribute__((ext_vector_type(4), aligned(16)));

struct SamLane {
    uint32_t nl, tab, valid;                                     // 16-bit masks over the lane's bytes; bytes past the end are in none
};

// the 16 bytes at chunk offset `off` (16-byte aligned in memory) of a text of n bytes
__device__ __forceinline__ SamLane sam_load_lane(const uint8_t* __restrict__ text, int64_t n, int64_t off) {
    SamLane b{0u, 0u, 0u};
    if (off >= n) return b;
    const sam_u32x4 v = *reinterpret_cast<const sam_u32x4*>(text + off);     // at most 15 bytes past the end: the pad
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
        b.nl |= (uint32_t)(c == 10u) << k;
        b.tab |= (uint32_t)(c == 9u) << k;
    }
    const int64_t left = n - off;
    b.valid = left >= 16 ? 0xffffu : (1u << (int)left) - 1u;
    b.nl &= b.valid;
    b.tab &= b.valid;
    return b;
}

__device__ __forceinline__ uint32_t sam_tail_mask(uint32_t nl) {             // the bits behind the last newline
    return nl ? 0xffffu & ~((2u << (31 - __clz((int)nl))) - 1u) : 0xffffu;
}
__device__ __host__ __forceinline__ uint32_t sat_tabs(uint32_t c) { return c > kTabSat ? kTabSat : c; }
// two spans end to end as one
__device__ __host__ __forceinline__ uint32_t elem_join(uint32_t left, uint32_t right) {
    return (right & kElemNl) ? right : ((left & kElemNl) | sat_tabs((left & 15u) + (right & 15u)));
}
// the tabs a byte behind span `e` has in front of it in its line, with `entry` of them in front of the span
__device__ __host__ __forceinline__ uint32_t elem_apply(uint32_t entry, uint32_t e) {
    return (e & kElemNl) ? (e & 15u) : sat_tabs(entry + (e & 15u));
}

// one round of a wave's walk: the lane's masks, its line starts, and what it enters with
struct SamRound {
    SamLane b;
    uint32_t starts;                                             // bytes that open a line
    uint32_t tabs_in;                                            // tabs in front of the lane's first byte in its line
    uint32_t starts_before;                                      // line starts of the round in the lanes below
    uint32_t starts_total;
};

// `entry_tabs` / `prev_nl` hold in front of the round and are moved behind it
__device__ __forceinline__ SamRound sam_round(const uint8_t* __restrict__ text, int64_t n, int64_t off, int lane,
                                              uint32_t& entry_tabs, bool& prev_nl) {
    SamRound r;
    r.b = sam_load_lane(text, n, off);
    const int up = __shfl_up((int)(r.b.nl >> 15), 1);
    const uint32_t before = lane == 0 ? (uint32_t)prev_nl : (uint32_t)up;
    r.starts = ((r.b.nl << 1) | before) & r.b.valid;
    prev_nl = __shfl((int)(r.b.nl >> 15), 63) != 0;
    const uint32_t mine = (r.b.nl ? kElemNl : 0u) | sat_tabs((uint32_t)__popc(r.b.tab & sam_tail_mask(r.b.nl)));
    uint32_t incl = mine, cnt = (uint32_t)__popc(r.starts);
    const uint32_t own = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t e = (uint32_t)__shfl_up((int)incl, d), c = (uint32_t)__shfl_up((int)cnt, d);
        if (lane >= d) { incl = elem_join(e, incl); cnt += c; }
    }
    const uint32_t below = (uint32_t)__shfl_up((int)incl, 1);
    r.tabs_in = lane == 0 ? entry_tabs : elem_apply(entry_tabs, below);
    r.starts_before = cnt - own;
    r.starts_total = (uint32_t)__shfl((int)cnt, 63);
    entry_tabs = elem_apply(entry_tabs, (uint32_t)__shfl((int)incl, 63));
    return r;
}

__device__ __forceinline__ bool nl_before(const uint8_t* __restrict__ text, int64_t off) {
    return off == 0 || text[off - 1] == (uint8_t)'\n';
}

// ---- pass 1: what a tile is to its neighbours ----------------------------------------------------------------------------
__global__ __launch_bounds__(kSamThreads) void sam_flags_kernel(const uint8_t* __restrict__ text, int64_t n, int rounds,
                                                                int64_t n_tiles, uint8_t* __restrict__ flags,
                                                                uint32_t* __restrict__ tile_lines) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * kSamWaves + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const int64_t base = tile * rounds * kSamRound;
    bool prev_nl = nl_before(text, base);
    uint32_t elem = 0u, lines = 0u;
    for (int r = 0; r < rounds; ++r) {
        const int64_t off = base + r * kSamRound + lane * 16;
        const SamLane b = sam_load_lane(text, n, off);
        const int up = __shfl_up((int)(b.nl >> 15), 1);
        const uint32_t before = lane == 0 ? (uint32_t)prev_nl : (uint32_t)up;
        const uint32_t starts = ((b.nl << 1) | before) & b.valid;
        prev_nl = __shfl((int)(b.nl >> 15), 63) != 0;
        const unsigned long long t = __ballot(b.nl != 0u);
        uint32_t tabs = (uint32_t)__popc(b.tab & sam_tail_mask(b.nl)), cnt = (uint32_t)__popc(starts);
        if (t != 0ull && lane < 63 - __clzll((long long)t)) tabs = 0u;       // in front of the round's last newline
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            tabs += (uint32_t)__shfl_xor((int)tabs, d);
            cnt += (uint32_t)__shfl_xor((int)cnt, d);
        }
        elem = elem_join(elem, (t ? kElemNl : 0u) | sat_tabs(tabs));         // the round as one span, behind the tile so far
        lines += cnt;
    }
    if (lane == 0) {
        flags[tile] = (uint8_t)elem;
        tile_lines[tile] = lines;
    }
}

// ---- pass 2: the tab ordinal at every tile's entry and the rank of its first line.  One workgroup; a thread owns a run
// of consecutive tiles. ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSamScanThreads) void sam_state_kernel(const uint8_t* __restrict__ flags, int64_t n_tiles,
                                                                    uint8_t* __restrict__ state,
                                                                    uint32_t* __restrict__ tile_lines,
                                                                    unsigned long long* __restrict__ total) {
    __shared__ uint8_t part[kSamScanThreads];
    __shared__ uint8_t entry[kSamScanThreads];
    __shared__ unsigned long long lines[kSamScanThreads];
    const int t = threadIdx.x;
    const int64_t per = (n_tiles + kSamScanThreads - 1) / kSamScanThreads;
    const int64_t lo = (int64_t)t * per < n_tiles ? (int64_t)t * per : n_tiles;
    const int64_t hi = lo + per < n_tiles ? lo + per : n_tiles;
    uint32_t e = 0u;
    unsigned long long sum = 0ull;
    for (int64_t i = lo; i < hi; ++i) {
        e = elem_join(e, flags[i]);
        sum += tile_lines[i];
    }
    part[t] = (uint8_t)e;
    lines[t] = sum;
    __syncthreads();
    if (t == 0) {
        uint32_t tabs = 0u;
        unsigned long long run = 0ull;
        for (int i = 0; i < kSamScanThreads; ++i) {
            entry[i] = (uint8_t)tabs;
            tabs = elem_apply(tabs, part[i]);
            const unsigned long long v = lines[i];
            lines[i] = run;
            run += v;
        }
        *total = run;
    }
    __syncthreads();
    uint32_t tabs = entry[t];
    unsigned long long run = lines[t];
    for (int64_t i = lo; i < hi; ++i) {
        state[i] = (uint8_t)tabs;
        tabs = elem_apply(tabs, flags[i]);
        const uint32_t v = tile_lines[i];
        tile_lines[i] = (uint32_t)run;                           // (a chunk is below 4 GiB: fewer lines than 2^32)
        run += v;
    }
}

// ---- pass 3: one row per line ----------------------------------------------------------------------------------------
struct SamRows {
    uint32_t *start, *tab1, *tab9, *tab10, *end;
    uint32_t n;
};

__global__ __launch_bounds__(kSamThreads) void sam_index_kernel(const uint8_t* __restrict__ text, int64_t n, int rounds,
                                                                int64_t n_tiles, const uint8_t* __restrict__ state,
                                                                const uint32_t* __restrict__ tile_rank, SamRows rows) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * kSamWaves + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const int64_t base = tile * rounds * kSamRound;
    bool prev_nl = nl_before(text, base);
    uint32_t entry_tabs = state[tile];
    uint32_t rank = tile_rank[tile];                             // line starts in front of the round
    for (int r = 0; r < rounds; ++r) {
        const int64_t off = base + r * kSamRound + lane * 16;
        const SamRound w = sam_round(text, n, off, lane, entry_tabs, prev_nl);
        const uint32_t lane_rank = rank + w.starts_before;       // line starts in front of the lane
        for (uint32_t m = w.starts; m; m &= m - 1u) {
            const int k = __ffs((int)m) - 1;
            const uint32_t row = lane_rank + (uint32_t)__popc(w.starts & ((1u << k) - 1u));
            if (row < rows.n) rows.start[row] = (uint32_t)(off + k);
        }
        uint32_t tabs = w.tabs_in;
        for (uint32_t m = w.b.tab | w.b.nl; m; m &= m - 1u) {
            const int k = __ffs((int)m) - 1;
            // the line the byte lies in: the last one that begins at or in front of it
            const uint32_t row = lane_rank + (uint32_t)__popc(w.starts & ((2u << k) - 1u)) - 1u;
            if ((w.starts >> k) & 1u) tabs = 0u;                 // the byte opens its line
            if ((w.b.nl >> k) & 1u) {
                if (row < rows.n) rows.end[row] = (uint32_t)(off + k);
                tabs = 0u;
            } else {
                tabs = sat_tabs(tabs + 1u);
                if (row < rows.n) {
                    if (tabs == 1u) rows.tab1[row] = (uint32_t)(off + k);
                    else if (tabs == 9u) rows.tab9[row] = (uint32_t)(off + k);
                    else if (tabs == 10u) rows.tab10[row] = (uint32_t)(off + k);
                }
            }
        }
        if (off <= n - 1 && n - 1 < off + 16) {                  // the chunk's last byte: a last line without '\n' ends here
            const int k = (int)(n - 1 - off);
            if (!((w.b.nl >> k) & 1u)) {
                const uint32_t row = lane_rank + (uint32_t)__popc(w.starts & ((2u << k) - 1u)) - 1u;
                if (row < rows.n) rows.end[row] = (uint32_t)n;
            }
        }
        rank += w.starts_total;
    }
}

// ---- pass 4: one lane per record ---------------------------------------------------------------------------------------
struct SamOut {
    int32_t *tid, *mtid, *pos, *mpos, *tlen;
    uint16_t *flag, *qlen;
    uint8_t* mapq;
    int32_t *head_rlen, *head_alen;                              // the context's first head_records records
    uint16_t* head_qlen;
    int64_t out_base, head_records;
};

__global__ __launch_bounds__(kSamDecodeThreads) void sam_decode_kernel(const uint8_t* __restrict__ text, int64_t n,
                                                                       int64_t file_offset, SamRows rows, RefTable table,
                                                                       SamOut o, unsigned long long* __restrict__ err,
                                                                       unsigned long long* __restrict__ saturated) {
    const int64_t i = (int64_t)blockIdx.x * kSamDecodeThreads + threadIdx.x;
    uint32_t sat = 0u;
    if (i < (int64_t)rows.n) {
        const uint32_t s = rows.start[i], e = rows.end[i];
        Record rec{};
        uint32_t reason;
        if (s == kNoOffset || e == kNoOffset || e < s || (int64_t)e > n) reason = kFewFields;       // (no walk leaves such a row)
        else reason = sam_decode_line(text, s, e, rows.tab1[i], rows.tab9[i], rows.tab10[i], table, &rec);
        if (reason != kOk) {
            const unsigned long long at = (unsigned long long)(file_offset + (s == kNoOffset ? 0 : s));
            atomicMin(err, (at << 8) | reason);
        }
        const int64_t g = o.out_base + i;
        o.tid[g] = rec.tid; o.mtid[g] = rec.mtid; o.pos[g] = rec.pos; o.mpos[g] = rec.mpos; o.tlen[g] = rec.tlen;
        o.flag[g] = rec.flag; o.qlen[g] = rec.qlen; o.mapq[g] = rec.mapq;
        if (g < o.head_records) {
            o.head_rlen[g] = rec.rlen; o.head_alen[g] = rec.alen; o.head_qlen[g] = rec.qlen;
        }
        sat = rec.saturated;
    }
    const unsigned long long m = __ballot(sat != 0u);
    if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(saturated, (unsigned long long)__popcll(m));
}

// ---- the line cutter: where the last line ends, where the header ends, the newlines in front of a byte -----------------
constexpr int kLinesMaxBlocks = 2048;                            // waves enough for every CU; a wave's run of rounds grows behind that

__global__ __launch_bounds__(kSamThreads) void sam_lines_kernel(const uint8_t* __restrict__ text, int64_t n, int64_t count_upto,
                                                                int want_header_end, int64_t n_rounds, int64_t per_wave,
                                                                unsigned long long* __restrict__ out) {
    namespace L = besst_sam_lines;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * kSamWaves + (threadIdx.x >> 6);
    const int64_t r0 = wave * per_wave;
    const int64_t r1 = r0 + per_wave < n_rounds ? r0 + per_wave : n_rounds;
    if (r0 >= r1) return;
    bool prev_nl = nl_before(text, r0 * kSamRound);
    L::Acc a = L::acc_none();
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t off = r * kSamRound + lane * 16;
        L::Slice s{0u, 0u, 0u};
        if (off < n) {
            const sam_u32x4 v = *reinterpret_cast<const sam_u32x4*>(text + off);     // at most 15 bytes past the end: the pad
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            s = L::slice_masks(w, n - off);
        }
        const int up = __shfl_up((int)(s.nl >> 15), 1);
        const uint32_t before = lane == 0 ? (uint32_t)prev_nl : (uint32_t)up;
        prev_nl = __shfl((int)(s.nl >> 15), 63) != 0;
        if (off < n) L::acc_slice(a, s, before, off, n, count_upto, want_header_end != 0);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        L::Acc b;
        b.last_end = (uint32_t)__shfl_xor((int)a.last_end, d);
        b.first_rec = (uint32_t)__shfl_xor((int)a.first_rec, d);
        b.newlines = (uint32_t)__shfl_xor((int)a.newlines, d);
        L::acc_join(a, b);
    }
    if (lane == 0) {
        if (a.last_end) atomicMax(out, (unsigned long long)a.last_end);
        if (a.first_rec != L::kNone) atomicMin(out + 1, (unsigned long long)a.first_rec);
        if (a.newlines) atomicAdd(out + 2, (unsigned long long)a.newlines);
    }
}

struct SamPlan {
    int rounds;
    int64_t n_tiles;
    size_t o_flags, o_state, o_lines, o_status, bytes;
};

// -> false: tile_bytes is not accepted
bool plan_sam(int64_t text_bytes, int64_t tile_bytes, SamPlan* p) {
    if (tile_bytes == 0) tile_bytes = kSamDefaultTile;
    if (text_bytes < 0 || text_bytes >= ((int64_t)1 << 32) - 16 || tile_bytes < kSamMinTile || tile_bytes > kSamMaxTile ||
        tile_bytes % kSamRound)
        return false;
    p->rounds = (int)(tile_bytes / kSamRound);
    p->n_tiles = (text_bytes + tile_bytes - 1) / tile_bytes;
    const size_t t = (size_t)(p->n_tiles ? p->n_tiles : 1);
    size_t o = 0;
    p->o_flags = o; o += align_up(t, 256);
    p->o_state = o; o += align_up(t, 256);
    p->o_lines = o; o += align_up(t * 4, 256);
    p->o_status = o; o += 256;                                   // line count, error word, saturated records
    p->bytes = o;
    return true;
}

// the events of a timed push (besst_ctx_sam_pass_times): gone with the call, however it returns
struct SamEvents {
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // flags | state | (wait) | index | decode
    bool on = false;
    hipError_t create() {
        on = true;
        for (auto& e : ev) {
            const hipError_t rc = hipEventCreate(&e);
            if (rc != hipSuccess) return rc;
        }
        return hipSuccess;
    }
    hipError_t mark(int k, hipStream_t s) const { return on ? hipEventRecord(ev[k], s) : hipSuccess; }
    ~SamEvents() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// Room for the chunk's n records behind the `have` resident ones.  When the columns have to grow they grow once, to what
// the rest of the announced text (besst_ctx_sam_expect_text) will need at the records per byte seen so far plus 3 % - never
// more than a record per 22 bytes, the shortest line -; without an announcement they double.  If that much memory is not
// to be had, the chunk's own records are asked for.
int reserve_sam_records(besst_ctx* c, int64_t have, int64_t n) {
    const int64_t need = have + n;
    if ((size_t)need <= c->tid.cap && (size_t)need <= c->mapq.cap) return reserve_records(c, have, need);
    int64_t want = need > 2 * have ? need : 2 * have;
    const int64_t left = c->sam_expect_bytes - c->sam_seen_bytes;
    if (c->sam_expect_bytes > 0 && c->sam_seen_bytes > 0) {
        const double per_byte = (double)(c->sam_file_records + n) / (double)c->sam_seen_bytes;
        int64_t more = left > 0 ? (int64_t)((double)left * per_byte * 1.03) + 1024 : 0;
        if (left > 0 && more > left / 22 + 1) more = left / 22 + 1;
        want = need + more;
    }
    if (want >= ((int64_t)1 << 32)) want = ((int64_t)1 << 32) - 1;
    int rc = reserve_records(c, have, want);
    if (rc == BESST_ERR_NOMEM && want > need) rc = reserve_records(c, have, need);
    return rc;
}

}  // namespace

}  // namespace besst

using namespace besst;

extern "C" {

size_t besst_dev_sam_workspace_bytes(int64_t text_bytes, int64_t tile_bytes) {
    SamPlan p;
    return plan_sam(text_bytes, tile_bytes, &p) ? p.bytes : 0;
}

int besst_dev_sam_lines(void* stream, const uint8_t* text, int64_t n_bytes, int32_t want_header_end, int64_t count_upto,
                        int64_t* out) {
    BESST_REQUIRE(out && (text || n_bytes == 0), "sam_lines: null pointer");
    BESST_REQUIRE(n_bytes >= 0 && n_bytes < ((int64_t)1 << 32) - 16, "sam_lines: n_bytes must lie in 0..2^32-17");
    BESST_REQUIRE((reinterpret_cast<uintptr_t>(text) & 15) == 0, "sam_lines: text must be 16-byte aligned");
    BESST_REQUIRE(count_upto >= 0 && count_upto <= n_bytes, "sam_lines: count_upto must lie in 0..n_bytes");
    hipStream_t s = static_cast<hipStream_t>(stream);
    BESST_HIP_TRY(hipMemsetAsync(out, 0, 32, s));
    BESST_HIP_TRY(hipMemsetAsync(out + 1, 0xff, 8, s));           // no such line start: -1
    if (n_bytes == 0) return BESST_OK;
    const int64_t n_rounds = (n_bytes + kSamRound - 1) / kSamRound;
    const int64_t max_waves = (int64_t)kLinesMaxBlocks * kSamWaves;
    const int64_t per_wave = (n_rounds + max_waves - 1) / max_waves;
    const int64_t waves = (n_rounds + per_wave - 1) / per_wave;
    hipLaunchKernelGGL(sam_lines_kernel, dim3((uint32_t)((waves + kSamWaves - 1) / kSamWaves)), dim3(kSamThreads), 0, s, text,
                       n_bytes, count_upto, (int)want_header_end, n_rounds, per_wave,
                       reinterpret_cast<unsigned long long*>(out));
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

int besst_ctx_set_sam_references(besst_ctx* c, const uint8_t* names, const int64_t* name_off, int64_t n_ref) {
    BESST_REQUIRE(c, "null context");
    BESST_REQUIRE(n_ref >= 0 && n_ref < ((int64_t)1 << 30), "set_sam_references: n_ref out of range");
    BESST_REQUIRE(n_ref == 0 || (names && name_off), "set_sam_references: null pointer");
    for (int64_t r = 0; r < n_ref; ++r)
        BESST_REQUIRE(name_off[r] >= 0 && name_off[r] < name_off[r + 1], "set_sam_references: a name is empty or the offsets fall");
    int rc = use_device(c);
    if (rc) return rc;
    const uint32_t cap = besst_sam::table_capacity(n_ref);
    c->sam_cap = 0;
    c->sam_refs = 0;
    if (n_ref == 0) return BESST_OK;
    std::vector<uint32_t> slots(cap, 0u);
    const int64_t twice = besst_sam::build_table(names, name_off, n_ref, slots.data(), cap);
    if (twice >= 0) {
        set_error("set_sam_references: the name of reference %lld is an earlier reference's", (long long)twice);
        return BESST_ERR_ARG;
    }
    const size_t pool_bytes = (size_t)name_off[n_ref];
    if ((rc = c->sam_slots.ensure(cap)) || (rc = c->sam_pool.ensure(pool_bytes)) || (rc = c->sam_off.ensure((size_t)n_ref + 1)))
        return rc;
    BESST_HIP_TRY(hipMemcpyAsync(c->sam_slots.p, slots.data(), (size_t)cap * 4, hipMemcpyHostToDevice, c->stream));
    BESST_HIP_TRY(hipMemcpyAsync(c->sam_pool.p, names, pool_bytes, hipMemcpyHostToDevice, c->stream));
    BESST_HIP_TRY(hipMemcpyAsync(c->sam_off.p, name_off, ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, c->stream));
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));             // slots is a local, the names are the caller's
    c->sam_cap = cap;
    c->sam_refs = n_ref;
    return BESST_OK;
}

int besst_ctx_sam_pass_times(besst_ctx* c, int enable, double* ms) {
    BESST_REQUIRE(c, "null context");
    if (ms)
        for (int k = 0; k < 4; ++k) ms[k] = c->sam_ms[k];
    for (int k = 0; k < 4; ++k) c->sam_ms[k] = 0.0;
    c->sam_timing = enable != 0;
    return BESST_OK;
}

int besst_ctx_sam_expect_text(besst_ctx* c, int64_t text_bytes) {
    BESST_REQUIRE(c, "null context");
    BESST_REQUIRE(text_bytes >= 0, "sam_expect_text: negative size");
    c->sam_expect_bytes = text_bytes;
    c->sam_seen_bytes = 0;
    c->sam_file_records = 0;
    return BESST_OK;
}

int besst_ctx_push_sam_text(besst_ctx* c, void* stream, const uint8_t* text, int64_t text_bytes, int64_t file_offset,
                            int64_t tile_bytes, int64_t head_records, int32_t* head_rlen, int32_t* head_alen,
                            uint16_t* head_qlen, int64_t* info) {
    BESST_REQUIRE(c, "null context");
    SamPlan p;
    BESST_REQUIRE(plan_sam(text_bytes, tile_bytes, &p),
                  "push_sam_text: tile_bytes must be 0 or a multiple of 1024 in 1024..65536, text_bytes in 0..2^32-17");
    BESST_REQUIRE(info && (text || text_bytes == 0), "push_sam_text: null pointer");
    BESST_REQUIRE((reinterpret_cast<uintptr_t>(text) & 15) == 0, "push_sam_text: text must be 16-byte aligned");
    BESST_REQUIRE(file_offset >= 0 && file_offset < ((int64_t)1 << 55), "push_sam_text: file_offset out of range");
    BESST_REQUIRE(head_records >= 0 && head_records < ((int64_t)1 << 31) &&
                      (head_records == 0 || (head_rlen && head_alen && head_qlen)),
                  "push_sam_text: head_records needs the three head arrays");
    info[0] = info[1] = 0;
    info[2] = -1;
    info[3] = 0;
    if (text_bytes == 0) return BESST_OK;
    int rc = use_device(c);
    if (rc) return rc;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    if ((rc = c->sam_ws.ensure(p.bytes))) return rc;
    if (head_records && (rc = c->sam_head.ensure((size_t)head_records * 10))) return rc;
    char* ws = c->sam_ws.p;
    uint8_t* flags = reinterpret_cast<uint8_t*>(ws + p.o_flags);
    uint8_t* state = reinterpret_cast<uint8_t*>(ws + p.o_state);
    uint32_t* lines = reinterpret_cast<uint32_t*>(ws + p.o_lines);
    unsigned long long* status = reinterpret_cast<unsigned long long*>(ws + p.o_status);
    BESST_HIP_TRY(hipMemsetAsync(status, 0, 24, s));
    BESST_HIP_TRY(hipMemsetAsync(status + 1, 0xff, 8, s));        // no error: all ones
    const uint32_t grid = (uint32_t)((p.n_tiles + kSamWaves - 1) / kSamWaves);
    SamEvents timed;
    if (c->sam_timing) BESST_HIP_TRY(timed.create());
    auto mark = [&](int k) { return timed.mark(k, s); };
    BESST_HIP_TRY(mark(0));
    hipLaunchKernelGGL(sam_flags_kernel, dim3(grid), dim3(kSamThreads), 0, s, text, text_bytes, p.rounds, p.n_tiles, flags,
                       lines);
    BESST_HIP_TRY(mark(1));
    hipLaunchKernelGGL(sam_state_kernel, dim3(1), dim3(kSamScanThreads), 0, s, flags, p.n_tiles, state, lines, status);
    BESST_HIP_TRY(mark(2));
    BESST_HIP_TRY(hipGetLastError());
    unsigned long long got[3] = {0ull, 0ull, 0ull};
    BESST_HIP_TRY(hipMemcpyAsync(got, status, 8, hipMemcpyDeviceToHost, s));
    BESST_HIP_TRY(hipStreamSynchronize(s));                      // the one wait between the passes: the record count
    const int64_t n = (int64_t)got[0];
    BESST_REQUIRE(n >= 1 && n <= text_bytes, "push_sam_text: the line count is not this text's");
    BESST_REQUIRE(c->n_records + n < ((int64_t)1 << 32), "more than 2^32-1 records in one context");
    const int64_t have = c->n_records;
    c->sam_seen_bytes += text_bytes;
    if ((rc = reserve_sam_records(c, have, n))) return rc;
    if ((rc = c->sam_rows.ensure((size_t)n * 5))) return rc;
    SamRows rows{c->sam_rows.p, c->sam_rows.p + n, c->sam_rows.p + 2 * n, c->sam_rows.p + 3 * n, c->sam_rows.p + 4 * n, (uint32_t)n};
    BESST_HIP_TRY(mark(3));
    BESST_HIP_TRY(hipMemsetAsync(rows.start, 0xff, (size_t)n * 5 * 4, s));
    hipLaunchKernelGGL(sam_index_kernel, dim3(grid), dim3(kSamThreads), 0, s, text, text_bytes, p.rounds, p.n_tiles, state,
                       lines, rows);
    BESST_HIP_TRY(mark(4));
    int32_t* h_rlen = reinterpret_cast<int32_t*>(c->sam_head.p);
    int32_t* h_alen = h_rlen + head_records;
    uint16_t* h_qlen = reinterpret_cast<uint16_t*>(h_alen + head_records);
    const RefTable table{c->sam_slots.p, c->sam_cap, c->sam_pool.p, c->sam_off.p};
    const SamOut out{c->tid.p, c->mtid.p, c->pos.p, c->mpos.p, c->tlen.p, c->flag.p, c->qlen.p, c->mapq.p,
                     h_rlen, h_alen, h_qlen, have, head_records};
    hipLaunchKernelGGL(sam_decode_kernel, dim3((uint32_t)((n + kSamDecodeThreads - 1) / kSamDecodeThreads)),
                       dim3(kSamDecodeThreads), 0, s, text, text_bytes, file_offset, rows, table, out, status + 1, status + 2);
    BESST_HIP_TRY(mark(5));
    BESST_HIP_TRY(hipGetLastError());
    BESST_HIP_TRY(hipMemcpyAsync(got, status, sizeof(got), hipMemcpyDeviceToHost, s));
    const int64_t head_to = have + n < head_records ? have + n : head_records;
    if (have < head_to) {
        const size_t k = (size_t)(head_to - have);
        BESST_HIP_TRY(hipMemcpyAsync(head_rlen + have, h_rlen + have, k * 4, hipMemcpyDeviceToHost, s));
        BESST_HIP_TRY(hipMemcpyAsync(head_alen + have, h_alen + have, k * 4, hipMemcpyDeviceToHost, s));
        BESST_HIP_TRY(hipMemcpyAsync(head_qlen + have, h_qlen + have, k * 2, hipMemcpyDeviceToHost, s));
    }
    BESST_HIP_TRY(hipStreamSynchronize(s));
    if (c->sam_timing) {
        const int from[4] = {0, 1, 3, 4};
        for (int k = 0; k < 4; ++k) {
            float ms = 0.f;
            BESST_HIP_TRY(hipEventElapsedTime(&ms, timed.ev[from[k]], timed.ev[from[k] + 1]));
            c->sam_ms[k] += (double)ms;
        }
    }
    info[0] = n;
    info[1] = (int64_t)got[2];
    if (got[1] != ~0ull) {                                       // the chunk's records do not become the context's
        info[2] = (int64_t)(got[1] >> 8);
        info[3] = (int64_t)(got[1] & 0xffu);
        return BESST_OK;
    }
    c->n_records = have + n;
    c->sam_file_records += n;
    c->built = false;
    return BESST_OK;
}

}  // extern "C"
