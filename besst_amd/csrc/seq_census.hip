// The sequence census (include/besst_amd.h, BESST_CENSUS_*; the record and its merge rule: seq_census_core.h): base classes,
// lower case and the runs of 'N' of every row of a segment table, counted over a window of the byte stream where it lies.
//
// seq_census_kernel   one WAVE per tile of BESST_CENSUS_TILE_BYTES bytes (tiles begin at 16-byte aligned addresses), four
//                     tiles per workgroup.  The wave finds the first row of its tile by a search in seq_off, then walks
//                     the rows 64 at a time - one row per lane: clipped to tile and window, held against its predecessor
//                     for `status` - and takes the rows that have bytes in the tile one after the other, each as ONE work
//                     item "row ∩ tile" for the whole wave:
//                       every lane reads 16-byte groups (four loads in flight), invalid bytes of the first and last
//                       group are zeroed;
//                       A C G T and lower case are counted on four bytes at a time with word arithmetic; only a group
//                       that holds another byte looks for N and classifies what is left with census_class;
//                       the runs of N come from the 16-bit N mask of a group: a run is closed where a byte that is not N
//                       follows an N, its start is the latest start in the lane's own mask, else of the nearest lane
//                       below that has one (one ballot and one shuffle), else what earlier groups left; all run
//                       counters are sums and maxima, so the lanes keep their own and the wave adds them up once.
//                     A row whose bytes in the window all lie in this tile is merged into acc by the wave itself (no other
//                     wave touches that row in this call); a row that goes on into the next tile or came from the
//                     previous one leaves its partial in the tile's two workspace slots (128 bytes each, word 15: the
//                     row + 1, 0 for an unused slot).
// seq_census_join     one wave per tile again: where slot 1 of the tile is in use a row begins that runs on, and the wave
//                     merges the chain - slot 1, then slot 0 of the tiles behind it up to the row's last - IN ORDER: 64
//                     partials per turn, one per lane, reduced by an ordered tree of shuffles (lane l takes l + d in), the
//                     turns folded in lane 0; then acc[row] = merge(acc[row], chain).
// Integers only, no atomics on the result, plain stores: the same input gives the same words, bit for bit.
#include "common.h"
#include "seq_census_core.h"

namespace besst {

namespace {

using namespace besst_census;

constexpr int kTile = BESST_CENSUS_TILE_BYTES;
constexpr int kWavesPerBlock = 4;
constexpr int kLoads = 4;                       // 16-byte groups a lane has in flight
constexpr int kSlotWords = 2 * kWords;          // per tile: slot 0 (the row came from the tile before), slot 1 (it goes on)
static_assert(kTile % (64 * 16) == 0, "a tile is whole turns of the wave");

struct CensusArgs {
    const uint8_t* buf;
    int64_t origin, n, n_seq;
    const int64_t *seq_off, *seq_len;
    int64_t min_gap;
    int64_t* ws;
    int64_t* acc;
    unsigned long long* status;
    int64_t n_tiles;
    int64_t lead;                               // bytes between the aligned address tile 0 begins at and buf
};

__device__ __forceinline__ int64_t shfl64(int64_t v, int src) {
    const int lo = __shfl((int)(uint32_t)(uint64_t)v, src), hi = __shfl((int)(uint32_t)((uint64_t)v >> 32), src);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

__device__ __forceinline__ int64_t shfl64_down(int64_t v, int d) {
    const int lo = __shfl_down((int)(uint32_t)(uint64_t)v, d), hi = __shfl_down((int)(uint32_t)((uint64_t)v >> 32), d);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
        v = o > v ? o : v;
    }
    return v;
}

// 0x80 in every byte of x (all bytes < 0x80 or not) that equals the byte of `pat` (< 0x80, the same in all four places)
__device__ __forceinline__ uint32_t eq_bytes(uint32_t x, uint32_t pat) {
    const uint32_t y = x ^ pat;
    return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;
}

// bits 0..3 -> 0xFF in bytes 0..3
__device__ __forceinline__ uint32_t spread_bits(uint32_t four) { return ((four * 0x00204081u) & 0x01010101u) * 0xFFu; }

// 0x80 marks of bytes 0..3 -> bits 0..3
__device__ __forceinline__ uint32_t gather_marks(uint32_t marks) { return (((marks >> 7) * 0x00204081u) >> 21) & 0xFu; }

struct LaneCounts {
    uint32_t a, c, g, t, n, iupac, lower;
    uint32_t runs, gaps, gap_bases, longest, pre;
};

// One 16-byte group: `valid` has a bit for every byte that belongs to the item.  -> the 16-bit mask of its N bytes.
__device__ __forceinline__ uint32_t count_group(uint4 v, uint32_t valid, LaneCounts& k) {
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t ma = 0, mc = 0, mg = 0, mt = 0, ml = 0, unknown[4];
    uint32_t any_unknown = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t bytes = spread_bits((valid >> (4 * j)) & 0xFu);
        w[j] &= bytes;                                            // a byte outside the item: 0, in no class that is counted
        const uint32_t f = w[j] & 0xDFDFDFDFu;                    // case folded (only 0x41 and 0x61 become 0x41, and so on)
        const uint32_t a = eq_bytes(f, 0x41414141u), c = eq_bytes(f, 0x43434343u), g = eq_bytes(f, 0x47474747u),
                       t = eq_bytes(f, 0x54545454u);
        ma |= a >> j; mc |= c >> j; mg |= g >> j; mt |= t >> j;
        // 'a'..'z': at least 0x61, below 0x7B, below 0x80
        const uint32_t low7 = w[j] & 0x7F7F7F7Fu;
        ml |= (((low7 + 0x1F1F1F1Fu) & ~(low7 + 0x05050505u) & ~w[j]) & 0x80808080u) >> j;
        unknown[j] = (bytes & 0x80808080u) & ~(a | c | g | t);
        any_unknown |= unknown[j];
    }
    k.a += __popc(ma); k.c += __popc(mc); k.g += __popc(mg); k.t += __popc(mt); k.lower += __popc(ml);
    uint32_t n_mask = 0;
    if (any_unknown) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t n = eq_bytes(w[j] & 0xDFDFDFDFu, 0x4E4E4E4Eu);
            k.n += __popc(n);
            n_mask |= gather_marks(n) << (4 * j);
            uint32_t rest = unknown[j] & ~n;
            while (rest) {
                const int bit = __ffs(rest) - 1;                  // 7, 15, 23 or 31
                rest &= rest - 1;
                if (census_class((w[j] >> (bit - 7)) & 0xFFu) == BESST_CENSUS_IUPAC) k.iupac += 1;
            }
        }
    }
    return n_mask;
}

// The census of buf-relative bytes [s, e) (0 < e - s <= kTile, inside one tile) by the whole wave -> out[0..16) in every lane.
__device__ __forceinline__ void census_item(const uint8_t* buf, int64_t s, int64_t e, int64_t min_gap, int lane, int64_t* out) {
    const uint8_t* p = buf + s;
    const int head = (int)(reinterpret_cast<uintptr_t>(p) & 15u);
    const uint8_t* g0 = p - head;
    const int nbytes = (int)(e - s);
    const int ngroups = (head + nbytes + 15) >> 4;
    LaneCounts k = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int last_start = -1;                                          // (wave-uniform) the latest start of a run so far
    uint32_t prev_n = 0, end_n = 0;                               // the byte in front of this turn / the item's last byte is N
    for (int base = 0; base < ngroups; base += 64 * kLoads) {
        uint4 v[kLoads];
#pragma unroll
        for (int j = 0; j < kLoads; ++j) {
            const int g = base + j * 64 + lane;
            v[j] = g < ngroups ? *reinterpret_cast<const uint4*>(g0 + 16 * (int64_t)g) : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int j = 0; j < kLoads; ++j) {
            if (base + j * 64 >= ngroups) break;                  // (uniform)
            const int g = base + j * 64 + lane;
            int first_bit = g == 0 ? head : 0, end_bit = head + nbytes - 16 * g;
            end_bit = end_bit > 16 ? 16 : end_bit;
            const uint32_t valid = g < ngroups ? ((1u << end_bit) - 1u) & ~((1u << first_bit) - 1u) : 0u;
            const uint32_t m = count_group(v[j], valid, k);
            if (__ballot(m != 0) == 0 && prev_n == 0) continue;   // no N here and none open: the usual turn
            const uint32_t up = (uint32_t)__shfl_up((int)m, 1);
            const uint32_t prev_bit = lane == 0 ? prev_n : (up >> 15) & 1u;
            const uint32_t after_n = ((m << 1) | prev_bit) & 0xFFFFu;          // bytes whose predecessor is N
            const uint32_t starts = m & ~after_n, closers = ~m & valid & after_n;
            const int gbase = g * 16 - head;                      // position in the item of the group's byte 0
            const int top = starts ? gbase + 31 - __clz((int)starts) : -1;
            const uint64_t with_start = __ballot(starts != 0);
            if (__ballot(closers != 0)) {
                const uint64_t below = with_start & ((1ull << lane) - 1ull);
                const int src = below ? 63 - __clzll((long long)below) : lane;
                const int theirs = __shfl(top, src);
                const int before = below ? theirs : last_start;
                uint32_t todo = closers;
                while (todo) {
                    const int bit = __ffs(todo) - 1;
                    todo &= todo - 1;
                    const uint32_t mine = starts & ((1u << bit) - 1u);
                    const int from = mine ? gbase + 31 - __clz((int)mine) : before;
                    const uint32_t length = (uint32_t)(gbase + bit - from);
                    if (from == 0) {
                        k.pre = length;                           // the run at the item's first byte stays open
                    } else {
                        k.runs += 1;
                        if ((int64_t)length >= min_gap) { k.gaps += 1; k.gap_bases += length; }
                        k.longest = length > k.longest ? length : k.longest;
                    }
                }
            }
            if (with_start) last_start = __shfl(top, 63 - __clzll((long long)with_start));
            prev_n = ((uint32_t)__shfl((int)m, 63) >> 15) & 1u;
            end_n |= __ballot(g == ngroups - 1 && ((m >> (end_bit - 1)) & 1u)) != 0 ? 1u : 0u;
        }
    }
    const uint32_t a = wave_sum(k.a), c = wave_sum(k.c), g = wave_sum(k.g), t = wave_sum(k.t), n = wave_sum(k.n),
                   iupac = wave_sum(k.iupac), lower = wave_sum(k.lower), runs = wave_sum(k.runs), gaps = wave_sum(k.gaps),
                   gap_bases = wave_sum(k.gap_bases), longest = wave_max(k.longest);
    uint32_t pre = wave_max(k.pre), suf = 0;
    if (end_n) {
        suf = (uint32_t)(nbytes - last_start);
        if (last_start == 0) pre = (uint32_t)nbytes;              // all N
    }
    out[BESST_CENSUS_LEN] = nbytes;
    out[BESST_CENSUS_A] = a; out[BESST_CENSUS_C] = c; out[BESST_CENSUS_G] = g; out[BESST_CENSUS_T] = t;
    out[BESST_CENSUS_N] = n; out[BESST_CENSUS_IUPAC] = iupac;
    out[BESST_CENSUS_OTHER] = (int64_t)nbytes - (int64_t)(a + c + g + t + n + iupac);
    out[BESST_CENSUS_LOWER] = lower;
    out[BESST_CENSUS_PRE] = pre; out[BESST_CENSUS_SUF] = suf;
    out[BESST_CENSUS_RUNS] = runs; out[BESST_CENSUS_GAPS] = gaps; out[BESST_CENSUS_GAP_BASES] = gap_bases;
    out[BESST_CENSUS_LONGEST] = longest;
    out[15] = 0;
}

// acc = merge(acc, part) by one lane
__device__ __forceinline__ void fold_into(int64_t* acc, const int64_t* part, int64_t min_gap) {
    int64_t have[kWords];
#pragma unroll
    for (int w = 0; w < kWords; ++w) have[w] = acc[w];
    census_merge(have, part, min_gap, have);
#pragma unroll
    for (int w = 0; w < kWords; ++w) acc[w] = have[w];
}

__global__ __launch_bounds__(kWavesPerBlock * 64) void seq_census_kernel(CensusArgs a) {
    const int lane = (int)threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + ((int)threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;
    // the tile's bytes of the window, buf-relative, and in stream coordinates
    int64_t lo = tile * kTile - a.lead, hi = lo + kTile;
    lo = lo < 0 ? 0 : lo;
    hi = hi > a.n ? a.n : hi;
    const int64_t s_lo = a.origin + lo, s_hi = a.origin + hi, w_lo = a.origin, w_hi = a.origin + a.n;
    int64_t* slot = a.ws + tile * kSlotWords;
    uint32_t used = 0;                                            // bit 0 / 1: slot 0 / 1 was written
    // the walk begins at the turn of 64 rows that holds the last row at or in front of the tile's first byte
    const int64_t first = census_first_row(a.seq_off, a.n_seq, s_lo) & ~(int64_t)63;
    for (int64_t b = first; b < a.n_seq; b += 64) {
        const int64_t i = b + lane;
        const bool in = i < a.n_seq;
        int64_t off = 0, len = 0;
        if (in) {
            off = a.seq_off[i];
            len = a.seq_len[i];
            if (!census_row_in_order(a.seq_off, a.seq_len, i)) atomicMin(a.status, (unsigned long long)i);
            if (off < 0 || len < 0) atomicMin(a.status + 1, (unsigned long long)i);
        }
        // clipped to the window, and to the tile; a field below zero or a sum past int64: an empty row
        const bool sane = in && off >= 0 && len > 0 && off <= INT64_MAX - len;
        const int64_t row_lo = sane ? (off > w_lo ? off : w_lo) : 0, row_hi = sane ? (off + len < w_hi ? off + len : w_hi) : 0;
        const int64_t s = row_lo > s_lo ? row_lo : s_lo, e = row_hi < s_hi ? row_hi : s_hi;
        uint64_t todo = __ballot(sane && e > s);
        while (todo) {                                            // (uniform) one row ∩ tile at a time, the whole wave
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int64_t row = b + src;
            const int64_t is = shfl64(s, src), ie = shfl64(e, src), rl = shfl64(row_lo, src), rh = shfl64(row_hi, src);
            int64_t part[kWords];
            census_item(a.buf, is - a.origin, ie - a.origin, a.min_gap, lane, part);
            const bool from_before = rl < is, goes_on = rh > ie;
            if (!from_before && !goes_on) {
                if (lane == 0) fold_into(a.acc + row * kWords, part, a.min_gap);
            } else {
                const int which = from_before ? 0 : 1;
                part[15] = row + 1;
                int64_t word = 0;
#pragma unroll
                for (int w = 0; w < kWords; ++w) word = lane == w ? part[w] : word;
                if (lane < kWords) slot[which * kWords + lane] = word;
                used |= 1u << which;
            }
        }
        if (__ballot(!in || off >= s_hi)) break;
    }
    if (lane < 2 && !((used >> lane) & 1u)) slot[lane * kWords + 15] = 0;
}

__global__ __launch_bounds__(kWavesPerBlock * 64) void seq_census_join(CensusArgs a) {
    const int lane = (int)threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + ((int)threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;
    const int64_t* head = a.ws + tile * kSlotWords + kWords;     // slot 1: a row that begins here and goes on
    const int64_t tag = head[15];
    if (tag <= 0 || tag > a.n_seq) return;
    const int64_t row = tag - 1;
    // the last tile that holds a byte of the row inside the window
    const int64_t off = a.seq_off[row], len = a.seq_len[row];
    if (off < 0 || len <= 0 || off > INT64_MAX - len) return;
    int64_t end = off + len < a.origin + a.n ? off + len : a.origin + a.n;
    int64_t last = (end - 1 - a.origin + a.lead) / kTile;
    last = last >= a.n_tiles ? a.n_tiles - 1 : last;
    int64_t total[kWords];
#pragma unroll
    for (int w = 0; w < kWords; ++w) total[w] = head[w];
    total[15] = 0;
    for (int64_t t0 = tile + 1; t0 <= last; t0 += 64) {
        const int64_t t = t0 + lane;
        int64_t x[kWords];
#pragma unroll
        for (int w = 0; w < kWords; ++w) x[w] = 0;
        if (t <= last) {
            const int64_t* from = a.ws + t * kSlotWords;          // slot 0: the row came from the tile before
            if (from[15] == tag) {
#pragma unroll
                for (int w = 0; w < 15; ++w) x[w] = from[w];
            }
        }
        // ordered: after the step of width d lane l (a multiple of 2 d) holds the merge of lanes l .. l + 2 d - 1
        for (int d = 1; d < 64; d <<= 1) {
            int64_t y[kWords];
#pragma unroll
            for (int w = 0; w < 15; ++w) y[w] = shfl64_down(x[w], d);
            y[15] = 0;
            if ((lane & (2 * d - 1)) == 0) census_merge(x, y, a.min_gap, x);
        }
        if (lane == 0) census_merge(total, x, a.min_gap, total);
    }
    if (lane == 0) fold_into(a.acc + row * kWords, total, a.min_gap);
}

int64_t tiles_of(int64_t lead, int64_t n) { return (lead + n + kTile - 1) / kTile; }

}  // namespace

}  // namespace besst

using namespace besst;

extern "C" {

int64_t besst_dev_seq_census_tile_bytes(void) { return kTile; }

size_t besst_dev_seq_census_workspace_bytes(int64_t window_bytes, int64_t n_seq) {
    (void)n_seq;                                                  // the partials are per tile, whatever the table holds
    if (window_bytes < 0 || window_bytes > ((int64_t)1 << 46)) return 0;
    return (size_t)(tiles_of(15, window_bytes) + 1) * kSlotWords * sizeof(int64_t);
}

int besst_dev_seq_census(void* stream, const uint8_t* buf, int64_t origin, int64_t n, int64_t n_seq, const int64_t* seq_off,
                         const int64_t* seq_len, int64_t min_gap, void* workspace, int64_t* acc, int64_t* status) {
    BESST_REQUIRE(n >= 0 && n <= ((int64_t)1 << 46) && n_seq >= 0 && origin >= 0 && origin <= INT64_MAX - n,
                  "seq_census: size out of range");
    if (n == 0 || n_seq == 0) return BESST_OK;
    BESST_REQUIRE(buf && seq_off && seq_len && workspace && acc && status, "seq_census: null pointer");
    BESST_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0, "seq_census: the workspace is not 16-byte aligned");
    CensusArgs a;
    a.buf = buf; a.origin = origin; a.n = n; a.n_seq = n_seq; a.seq_off = seq_off; a.seq_len = seq_len;
    a.min_gap = min_gap;
    a.ws = static_cast<int64_t*>(workspace);
    a.acc = acc;
    a.status = reinterpret_cast<unsigned long long*>(status);
    a.lead = (int64_t)(reinterpret_cast<uintptr_t>(buf) & 15u);
    a.n_tiles = tiles_of(a.lead, n);
    const int64_t blocks = (a.n_tiles + kWavesPerBlock - 1) / kWavesPerBlock;
    BESST_REQUIRE(blocks < ((int64_t)1 << 31), "seq_census: the window is too large for one launch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(seq_census_kernel, dim3((uint32_t)blocks), dim3(kWavesPerBlock * 64), 0, s, a);
    BESST_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(seq_census_join, dim3((uint32_t)blocks), dim3(kWavesPerBlock * 64), 0, s, a);
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

int besst_host_seq_census(const uint8_t* buf, int64_t origin, int64_t n, int64_t n_seq, const int64_t* seq_off,
                          const int64_t* seq_len, int64_t min_gap, int64_t* acc) {
    BESST_REQUIRE(n >= 0 && n_seq >= 0 && origin >= 0 && origin <= INT64_MAX - n, "seq_census: size out of range");
    if (n == 0 || n_seq == 0) return BESST_OK;
    BESST_REQUIRE(buf && seq_off && seq_len && acc, "seq_census: null pointer");
    for (int64_t i = 0; i < n_seq; ++i) {
        if (!census_row_in_order(seq_off, seq_len, i) || seq_off[i] > INT64_MAX - seq_len[i]) {
            set_error("seq_census: row %lld of the segment table is out of order or overlaps its predecessor", (long long)i);
            return BESST_ERR_ARG;
        }
    }
    for (int64_t i = census_first_row(seq_off, n_seq, origin); i < n_seq && seq_off[i] < origin + n; ++i) {
        const int64_t lo = seq_off[i] > origin ? seq_off[i] : origin;
        const int64_t hi = seq_off[i] + seq_len[i] < origin + n ? seq_off[i] + seq_len[i] : origin + n;
        if (hi <= lo) continue;
        int64_t part[kWords];
        census_clear(part);
        for (int64_t p = lo; p < hi; ++p) census_push(part, buf[p - origin], min_gap);
        census_merge(acc + i * kWords, part, min_gap, acc + i * kWords);
    }
    return BESST_OK;
}

}  // extern "C"
