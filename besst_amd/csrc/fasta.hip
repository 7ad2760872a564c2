// The contig FASTA, read on the device: ReadInContigseqs (runBESST:45-74) on the bytes of the file.
//
// The whole file lies in HBM.  `\n` and `\r` end a line; a line whose first byte is '>' is a header, every other line a
// sequence line whose bytes are kept from its first to its last non-whitespace byte (str.strip(): interior whitespace
// stays).  The kept bytes of all lines, end to end, are the sequence pool of emit.hip; header h starts contig h at the
// number of bytes kept in front of it (contig 0 at 0: text in front of the first header belongs to the first contig).
//
// Whether a byte is kept depends on three facts that cross tile borders: the line it lies in is a header (h), a
// non-whitespace byte precedes it in its line (a), a non-whitespace byte follows it in its line (b).  a and h run
// forward and are cut by every terminator, b runs backward.  One wave owns one tile of tile_bytes and walks it in rounds
// of 1 KiB, 16 bytes per lane, every byte class a 16-bit mask:
//
//   flags_kernel    per tile: has a terminator / non-whitespace after the last one / header start after the last one /
//                   non-whitespace before the first one; the first byte >= 0x80 goes to the error word
//   state_kernel    one workgroup: (a, h) at every tile's entry by a forward scan of those flags, b by a backward scan
//   walk_kernel<0>  per tile, with its entry state: kept bytes, header lines, name bytes; a header without a name token
//                   goes to the error word
//   offsets_kernel  one workgroup: exclusive prefix sums of the three counts, totals to the info block
//   walk_kernel<1>  the same walk, writing: kept bytes are ranked by a wave prefix sum, compacted through a ring in LDS
//                   and leave in 16-byte stores aligned on the pool; the lane that holds a '>' writes the contig's row
//   rows_kernel     ctg_len from neighbouring ctg_off, the closing name_off, the contig without a header
//
// Inside a lane the three facts are occluded fills over its 16-bit masks (terminators stop them), seeded across lanes
// by ballots: the nearest lane with a terminator decides, lanes without one pass the state through.  A header's name
// (first whitespace-delimited token after '>') is read byte by byte by the lane that holds the '>': one in ten thousand
// lanes on an assembly.  Errors are a status: the smallest offending file offset, by 64-bit atomicMin.
#include "common.h"

namespace besst {

namespace {

constexpr int kFastaWaves = 4;                                   // tiles per workgroup
constexpr int kFastaThreads = kFastaWaves * 64;
constexpr int64_t kRoundBytes = 64 * 16;
constexpr int64_t kMinTile = kRoundBytes, kMaxTile = 64 * kRoundBytes, kDefaultTile = 16 * kRoundBytes;
constexpr int kRing = 2048;                                      // per wave: < 16 pending bytes + one round, a power of two
constexpr int kScanThreads = 1024;

// tile flags (flags_kernel) and tile entry state (state_kernel)
constexpr uint8_t kHasTerm = 1, kPostA = 2, kPostH = 4, kPreA = 8;
constexpr uint8_t kInA = 1, kInH = 2, kInB = 4;

typedef uint32_t fa_u32x4 __attribute__((ext_vector_type(4), aligned(16)));

__host__ __device__ inline bool is_term(uint32_t c) { return c == 10u || c == 13u; }
__host__ __device__ inline bool is_space(uint32_t c) { return (c - 9u) <= 4u || (c - 28u) <= 4u; }   // str.strip(), ASCII

struct LaneBytes {
    uint32_t w[4];                                               // the lane's 16 bytes
    uint32_t term, nonws, gt, high;                              // 16-bit masks over them; bytes past the end are in none
};

// the 16 bytes at file offset `off` (16-byte aligned in memory) of a text of n bytes
__device__ __forceinline__ LaneBytes load_lane(const uint8_t* __restrict__ text, int64_t n, int64_t off) {
    LaneBytes b;
    b.w[0] = b.w[1] = b.w[2] = b.w[3] = 0u;
    b.term = b.nonws = b.gt = b.high = 0u;
    if (off >= n) return b;
    const fa_u32x4 v = *reinterpret_cast<const fa_u32x4*>(text + off);       // at most 15 bytes past the end: the pad
    b.w[0] = v.x; b.w[1] = v.y; b.w[2] = v.z; b.w[3] = v.w;
    uint32_t space = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t c = (b.w[k >> 2] >> (8 * (k & 3))) & 0xffu;
        b.term |= (uint32_t)is_term(c) << k;
        space |= (uint32_t)is_space(c) << k;
        b.gt |= (uint32_t)(c == (uint32_t)'>') << k;
        b.high |= (uint32_t)(c >= 128u) << k;
    }
    const int64_t left = n - off;
    const uint32_t valid = left >= 16 ? 0xffffu : (1u << (int)left) - 1u;
    b.term &= valid; b.gt &= valid; b.high &= valid;
    b.nonws = ~space & valid;
    return b;
}

// every bit of g spreads towards higher (lower) bits through the bits of p; 16-bit masks
__device__ __forceinline__ uint32_t fill_up(uint32_t g, uint32_t p) {
    g |= p & (g << 1); p &= p << 1;
    g |= p & (g << 2); p &= p << 2;
    g |= p & (g << 4); p &= p << 4;
    g |= p & (g << 8);
    return g & 0xffffu;
}
__device__ __forceinline__ uint32_t fill_down(uint32_t g, uint32_t p) {
    g |= p & (g >> 1); p &= p >> 1;
    g |= p & (g >> 2); p &= p >> 2;
    g |= p & (g >> 4); p &= p >> 4;
    g |= p & (g >> 8);
    return g;
}

__device__ __forceinline__ uint32_t head_mask(uint32_t term) {   // the bits in front of the first terminator
    return term ? (1u << (__ffs((int)term) - 1)) - 1u : 0xffffu;
}
__device__ __forceinline__ uint32_t tail_mask(uint32_t term) {   // the bits behind the last terminator
    return term ? 0xffffu & ~((2u << (31 - __clz((int)term))) - 1u) : 0xffffu;
}
__device__ __forceinline__ unsigned long long lanes_upto(int j) {           // lanes 0..j
    return j >= 63 ? ~0ull : (2ull << j) - 1ull;
}

// the '>' bytes that open a line: the byte before them is a terminator (or the file begins there).  `prev_term`: the
// byte in front of the wave's first byte is one.
__device__ __forceinline__ uint32_t header_starts(const LaneBytes& b, int lane, bool prev_term) {
    const int up = __shfl_up((int)(b.term >> 15), 1);
    const uint32_t before = lane == 0 ? (uint32_t)prev_term : (uint32_t)up;
    return b.gt & ((b.term << 1) | before) & 0xffffu;
}

__device__ __forceinline__ bool term_before(const uint8_t* __restrict__ text, int64_t off) {
    return off == 0 || is_term(text[off - 1]);
}

// a wave's forward state (a, h) over one round: what lane `lane` enters with; the state moves on behind the round
struct Forward {
    bool a, h;                                                   // in front of the round; enter() moves them behind it
    __device__ __forceinline__ void enter(const LaneBytes& b, uint32_t hs, int lane, bool& a_in, bool& h_in) {
        const uint32_t tail = tail_mask(b.term);
        const unsigned long long t = __ballot(b.term != 0u), am = __ballot((b.nonws & tail) != 0u),
                                 hm = __ballot((hs & tail) != 0u);
        const unsigned long long below = (1ull << lane) - 1ull, tb = t & below;
        if (tb == 0) {
            a_in = a || (am & below) != 0;
            h_in = h || (hm & below) != 0;
        } else {
            const int j = 63 - __clzll((long long)tb);
            a_in = ((am & below) >> j) != 0;
            h_in = ((hm & below) >> j) != 0;
        }
        if (t == 0) {
            a = a || am != 0;
            h = h || hm != 0;
        } else {
            const int j = 63 - __clzll((long long)t);
            a = (am >> j) != 0;
            h = (hm >> j) != 0;
        }
    }
};

// the backward state b over one round: `b_right` holds behind the round; -> what lane `lane` has on its right, and
// b_right becomes the state in front of the round
__device__ __forceinline__ bool backward_enter(const LaneBytes& b, int lane, bool& b_right) {
    const unsigned long long t = __ballot(b.term != 0u), pm = __ballot((b.nonws & head_mask(b.term)) != 0u);
    const unsigned long long above = ~lanes_upto(lane), ta = t & above;
    bool b_in;
    if (ta == 0) {
        b_in = b_right || (pm & above) != 0;
    } else {
        b_in = (pm & above & lanes_upto(__ffsll((long long)ta) - 1)) != 0;
    }
    if (t == 0) b_right = b_right || pm != 0;
    else b_right = (pm & lanes_upto(__ffsll((long long)t) - 1)) != 0;
    return b_in;
}

// the lane's kept bytes
__device__ __forceinline__ uint32_t keep_mask(const LaneBytes& b, uint32_t hs, bool a_in, bool h_in, bool b_in) {
    const uint32_t open = ~b.term & 0xffffu, head = head_mask(b.term), tail = tail_mask(b.term);
    const uint32_t header = fill_up(hs, open) | (h_in ? head : 0u);
    const uint32_t seen = fill_up(b.nonws, open) | (a_in ? head : 0u);
    const uint32_t follows = fill_down(b.nonws, open) | (b_in ? tail : 0u);
    return seen & follows & ~header & open;
}

__device__ __forceinline__ uint32_t wave_exclusive(uint32_t v, int lane, uint32_t& total) {
    uint32_t s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)s, d);
        if (lane >= d) s += u;
    }
    total = (uint32_t)__shfl((int)s, 63);
    return s - v;
}
__device__ __forceinline__ int64_t wave_exclusive64(int64_t v, int lane, int64_t& total) {
    int64_t s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t u = __shfl_up(s, d);
        if (lane >= d) s += u;
    }
    total = __shfl(s, 63);
    return s - v;
}

// the name of the header whose '>' lies at gt: -> its length, *start its first byte
__device__ inline int64_t scan_name(const uint8_t* __restrict__ text, int64_t n, int64_t gt, int64_t* start) {
    int64_t p = gt + 1;
    while (p < n && is_space(text[p]) && !is_term(text[p])) ++p;
    int64_t q = p;
    while (q < n && !is_space(text[q])) ++q;
    *start = p;
    return q - p;
}

// ---- pass 1: what a tile is to its neighbours ----------------------------------------------------------------------------
__global__ __launch_bounds__(kFastaThreads) void fasta_flags_kernel(const uint8_t* __restrict__ text, int64_t n, int rounds,
                                                                    int64_t n_tiles, uint8_t* __restrict__ flags,
                                                                    unsigned long long* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * kFastaWaves + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const int64_t base = tile * rounds * kRoundBytes;
    bool prev_term = term_before(text, base);
    bool has_term = false, post_a = false, post_h = false, pre_a = false;
    for (int r = 0; r < rounds; ++r) {
        const int64_t off = base + r * kRoundBytes + lane * 16;
        const LaneBytes b = load_lane(text, n, off);
        if (b.high) atomicMin(err, (unsigned long long)(off + __ffs((int)b.high) - 1));
        const uint32_t hs = header_starts(b, lane, prev_term);
        prev_term = __shfl((int)(b.term >> 15), 63) != 0;
        const uint32_t tail = tail_mask(b.term);
        const unsigned long long t = __ballot(b.term != 0u), am = __ballot((b.nonws & tail) != 0u),
                                 hm = __ballot((hs & tail) != 0u), pm = __ballot((b.nonws & head_mask(b.term)) != 0u);
        if (!has_term) pre_a = pre_a || (t ? (pm & lanes_upto(__ffsll((long long)t) - 1)) != 0 : pm != 0);
        if (t == 0) {
            post_a = post_a || am != 0;
            post_h = post_h || hm != 0;
        } else {
            const int j = 63 - __clzll((long long)t);
            post_a = (am >> j) != 0;
            post_h = (hm >> j) != 0;
            has_term = true;
        }
    }
    if (lane == 0)
        flags[tile] = (uint8_t)((has_term ? kHasTerm : 0) | (post_a ? kPostA : 0) | (post_h ? kPostH : 0) | (pre_a ? kPreA : 0));
}

// ---- pass 2: the state at every tile's entry.  One workgroup; a thread owns a run of consecutive tiles. -----------------
__global__ __launch_bounds__(kScanThreads) void fasta_state_kernel(const uint8_t* __restrict__ flags, int64_t n_tiles,
                                                                   uint8_t* __restrict__ state) {
    __shared__ uint8_t part[kScanThreads];                       // a run as one tile: the same four flags
    __shared__ uint8_t entry[kScanThreads];
    const int t = threadIdx.x;
    const int64_t per = (n_tiles + kScanThreads - 1) / kScanThreads;
    const int64_t lo = (int64_t)t * per < n_tiles ? (int64_t)t * per : n_tiles;
    const int64_t hi = lo + per < n_tiles ? lo + per : n_tiles;
    bool has = false, a = false, h = false, pre = false;
    for (int64_t i = lo; i < hi; ++i) {
        const uint8_t f = flags[i];
        if (!has) pre = pre || (f & kPreA);
        if (f & kHasTerm) { a = f & kPostA; h = f & kPostH; has = true; }
        else { a = a || (f & kPostA); h = h || (f & kPostH); }
    }
    part[t] = (uint8_t)((has ? kHasTerm : 0) | (a ? kPostA : 0) | (h ? kPostH : 0) | (pre ? kPreA : 0));
    __syncthreads();
    if (t == 0) {
        bool ca = false, ch = false;
        for (int i = 0; i < kScanThreads; ++i) {
            entry[i] = (uint8_t)((ca ? kInA : 0) | (ch ? kInH : 0));
            const uint8_t f = part[i];
            if (f & kHasTerm) { ca = f & kPostA; ch = f & kPostH; }
            else { ca = ca || (f & kPostA); ch = ch || (f & kPostH); }
        }
        bool cb = false;                                         // the end of the file ends its last line
        for (int i = kScanThreads - 1; i >= 0; --i) {
            if (cb) entry[i] |= kInB;
            const uint8_t f = part[i];
            cb = (f & kHasTerm) ? (f & kPreA) != 0 : (cb || (f & kPreA));
        }
    }
    __syncthreads();
    a = entry[t] & kInA; h = entry[t] & kInH;
    for (int64_t i = lo; i < hi; ++i) {
        state[i] = (uint8_t)((a ? kInA : 0) | (h ? kInH : 0));
        const uint8_t f = flags[i];
        if (f & kHasTerm) { a = f & kPostA; h = f & kPostH; }
        else { a = a || (f & kPostA); h = h || (f & kPostH); }
    }
    bool b = entry[t] & kInB;
    for (int64_t i = hi - 1; i >= lo; --i) {
        if (b) state[i] |= kInB;
        const uint8_t f = flags[i];
        b = (f & kHasTerm) ? (f & kPreA) != 0 : (b || (f & kPreA));
    }
}

// ---- passes 3 and 5: the walk ----------------------------------------------------------------------------------------
struct FastaOut {
    uint8_t* pool;
    int64_t pool_bytes;
    int64_t n_contigs;
    int64_t* ctg_off;
    uint8_t* names;
    int64_t names_bytes;
    int64_t* name_off;
};

// the wave's ring holds the pool bytes [flushed, upto) at their offset modulo kRing: write out what is complete
__device__ __forceinline__ void flush_ring(const uint8_t* ring, const FastaOut& o, int64_t& flushed, int64_t upto, bool last,
                                           int lane) {
    if ((flushed & 15) && flushed < upto) {                      // the 16-byte group shared with the tile in front
        const int64_t edge = (flushed + 15) & ~(int64_t)15;
        const int64_t e = edge < upto ? edge : upto;
        if (e == edge || last) {
            const int64_t p = flushed + lane;
            if (p < e && p < o.pool_bytes) o.pool[p] = ring[p & (kRing - 1)];
            flushed = e;
        }
    }
    if ((flushed & 15) == 0) {
        const int64_t groups = (upto - flushed) >> 4;
        for (int64_t g = lane; g < groups; g += 64) {
            const int64_t p = flushed + g * 16;
            if (p + 16 <= o.pool_bytes)
                *reinterpret_cast<fa_u32x4*>(o.pool + p) = *reinterpret_cast<const fa_u32x4*>(ring + (p & (kRing - 1)));
        }
        flushed += groups * 16;
        if (last && flushed < upto) {                            // fewer than 16 bytes: the group shared with the next tile
            const int64_t p = flushed + lane;
            if (p < upto && p < o.pool_bytes) o.pool[p] = ring[p & (kRing - 1)];
            flushed = upto;
        }
    }
}

template <bool kWrite>
__global__ __launch_bounds__(kFastaThreads) void fasta_walk_kernel(const uint8_t* __restrict__ text, int64_t n, int rounds,
                                                                   int64_t n_tiles, const uint8_t* __restrict__ state,
                                                                   int64_t* __restrict__ tile_kept,
                                                                   int64_t* __restrict__ tile_rows,
                                                                   int64_t* __restrict__ tile_names, FastaOut o,
                                                                   unsigned long long* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) uint8_t rings[kWrite ? kFastaWaves : 1][kWrite ? kRing : 16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * kFastaWaves + wave;
    const bool live = tile < n_tiles;                            // a wave without a tile walks an empty text: the barriers
    const int64_t len = live ? n : 0;                            // below are the workgroup's
    const int64_t base = tile * rounds * kRoundBytes;
    const uint8_t st = live ? state[tile] : (uint8_t)0;
    // b behind every round, last round first
    unsigned long long b_behind = 0;
    {
        bool b_right = st & kInB;
        for (int r = rounds - 1; r >= 0; --r) {
            if (b_right) b_behind |= 1ull << r;
            const LaneBytes b = load_lane(text, len, base + r * kRoundBytes + lane * 16);
            (void)backward_enter(b, lane, b_right);
        }
    }
    Forward fw{(st & kInA) != 0, (st & kInH) != 0};
    bool prev_term = live ? term_before(text, base) : true;
    int64_t kept = 0, rows = 0, name_bytes = 0;                  // of the tile so far
    int64_t out0 = 0, row0 = 0, name0 = 0, flushed = 0;
    if (kWrite && live) {
        out0 = tile_kept[tile]; row0 = tile_rows[tile]; name0 = tile_names[tile];
        flushed = out0;
    }
    uint8_t* ring = rings[kWrite ? wave : 0];
    for (int r = 0; r < rounds; ++r) {
        const int64_t off = base + r * kRoundBytes + lane * 16;
        const LaneBytes b = load_lane(text, len, off);
        const uint32_t hs = header_starts(b, lane, prev_term);
        prev_term = __shfl((int)(b.term >> 15), 63) != 0;
        bool a_in, h_in, b_right = (b_behind >> r) & 1;
        fw.enter(b, hs, lane, a_in, h_in);
        const bool b_in = backward_enter(b, lane, b_right);
        const uint32_t keep = keep_mask(b, hs, a_in, h_in, b_in);
        uint32_t total;
        const uint32_t mine = wave_exclusive((uint32_t)__popc(keep) | ((uint32_t)__popc(hs) << 16), lane, total);
        const int64_t lane_out = out0 + kept + (mine & 0xffffu), lane_row = row0 + rows + (mine >> 16);
        if (__ballot(hs != 0u)) {                                // rare: a '>' opens a line in this KiB
            int64_t sum = 0, first;                              // at most 8 header lines in 16 bytes
            for (uint32_t m = hs; m; m &= m - 1) {
                const int64_t gt = off + __ffs((int)m) - 1;
                const int64_t length = scan_name(text, len, gt, &first);
                if (!kWrite && length == 0) atomicMin(err, (unsigned long long)gt);
                sum += length;
            }
            int64_t all;
            int64_t at = name0 + name_bytes + wave_exclusive64(sum, lane, all);
            name_bytes += all;
            if (kWrite) {
                int k = 0;
                for (uint32_t m = hs; m; m &= m - 1, ++k) {
                    const int bit = __ffs((int)m) - 1;
                    const int64_t row = lane_row + k;
                    const int64_t length = scan_name(text, len, off + bit, &first);
                    if (row < o.n_contigs) {
                        o.ctg_off[row] = row == 0 ? 0 : lane_out + __popc(keep & ((1u << bit) - 1u));
                        o.name_off[row] = at;
                        if (at + length <= o.names_bytes)
                            for (int64_t i = 0; i < length; ++i) o.names[at + i] = text[first + i];
                    }
                    at += length;
                }
            }
        }
        if (kWrite) {
            int64_t p = lane_out;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if ((keep >> k) & 1u) ring[(p++) & (kRing - 1)] = (uint8_t)(b.w[k >> 2] >> (8 * (k & 3)));
        }
        kept += total & 0xffffu;
        rows += total >> 16;
        if (kWrite) {
            __syncthreads();                                     // the round's bytes are in the ring
            flush_ring(ring, o, flushed, out0 + kept, r == rounds - 1, lane);
        }
    }
    if (!kWrite && live && lane == 0) {
        tile_kept[tile] = kept;
        tile_rows[tile] = rows;
        tile_names[tile] = name_bytes;
    }
}

// ---- pass 4: where every tile's output begins.  One workgroup, in place. -------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void fasta_offsets_kernel(int64_t n_tiles, int64_t* __restrict__ tile_kept,
                                                                     int64_t* __restrict__ tile_rows,
                                                                     int64_t* __restrict__ tile_names,
                                                                     int64_t* __restrict__ info) {
    __shared__ int64_t part[3][kScanThreads];
    const int t = threadIdx.x;
    const int64_t per = (n_tiles + kScanThreads - 1) / kScanThreads;
    const int64_t lo = (int64_t)t * per < n_tiles ? (int64_t)t * per : n_tiles;
    const int64_t hi = lo + per < n_tiles ? lo + per : n_tiles;
    int64_t s0 = 0, s1 = 0, s2 = 0;
    for (int64_t i = lo; i < hi; ++i) { s0 += tile_kept[i]; s1 += tile_rows[i]; s2 += tile_names[i]; }
    part[0][t] = s0; part[1][t] = s1; part[2][t] = s2;
    __syncthreads();
    if (t < 3) {
        int64_t run = 0;
        for (int i = 0; i < kScanThreads; ++i) { const int64_t v = part[t][i]; part[t][i] = run; run += v; }
        // info: contigs, pool bytes, name bytes; a file without a header line is one contig without a name
        if (t == 0) info[1] = run;
        if (t == 1) { info[0] = run ? run : 1; info[5] = run; }
        if (t == 2) info[2] = run;
    }
    __syncthreads();
    s0 = part[0][t]; s1 = part[1][t]; s2 = part[2][t];
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t k = tile_kept[i], r = tile_rows[i], m = tile_names[i];
        tile_kept[i] = s0; tile_rows[i] = s1; tile_names[i] = s2;
        s0 += k; s1 += r; s2 += m;
    }
}

// ---- pass 6: lengths ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fasta_rows_kernel(int64_t n_contigs, int64_t pool_bytes, int64_t names_bytes,
                                                         const int64_t* __restrict__ info, int64_t* __restrict__ ctg_off,
                                                         int32_t* __restrict__ ctg_len, int64_t* __restrict__ name_off,
                                                         unsigned long long* __restrict__ too_long) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_contigs) return;
    if (i == 0) {
        name_off[n_contigs] = names_bytes;
        if (info[5] == 0) { ctg_off[0] = 0; name_off[0] = 0; }   // no header line wrote row 0
    }
    const int64_t begin = i == 0 ? 0 : ctg_off[i], end = i + 1 < n_contigs ? ctg_off[i + 1] : pool_bytes;
    const int64_t length = end - begin;
    if (length < 0 || length >= ((int64_t)1 << 31)) {
        atomicMin(too_long, (unsigned long long)i);
        ctg_len[i] = 0;
    } else {
        ctg_len[i] = (int32_t)length;
    }
}

struct FastaPlan {
    int rounds;
    int64_t n_tiles;
    size_t o_flags, o_state, o_kept, o_rows, o_names, bytes;
};

// -> false: tile_bytes is not accepted
bool plan_fasta(int64_t text_bytes, int64_t tile_bytes, FastaPlan* p) {
    if (tile_bytes == 0) tile_bytes = kDefaultTile;
    if (text_bytes < 0 || tile_bytes < kMinTile || tile_bytes > kMaxTile || tile_bytes % kRoundBytes) return false;
    p->rounds = (int)(tile_bytes / kRoundBytes);
    p->n_tiles = (text_bytes + tile_bytes - 1) / tile_bytes;
    if (p->n_tiles >= ((int64_t)1 << 31) * kFastaWaves) return false;
    const size_t t = (size_t)(p->n_tiles ? p->n_tiles : 1);
    size_t o = 0;
    p->o_flags = o; o += align_up(t, 256);
    p->o_state = o; o += align_up(t, 256);
    p->o_kept = o; o += align_up(t * 8, 256);
    p->o_rows = o; o += align_up(t * 8, 256);
    p->o_names = o; o += align_up(t * 8, 256);
    p->bytes = o;
    return true;
}

}  // namespace

}  // namespace besst

using namespace besst;

extern "C" {

size_t besst_dev_fasta_workspace_bytes(int64_t text_bytes, int64_t tile_bytes) {
    FastaPlan p;
    return plan_fasta(text_bytes, tile_bytes, &p) ? p.bytes : 0;
}

int besst_dev_fasta_scan(void* stream, const uint8_t* text, int64_t text_bytes, int64_t tile_bytes, void* workspace,
                         size_t workspace_bytes, int64_t* info) {
    FastaPlan p;
    BESST_REQUIRE(plan_fasta(text_bytes, tile_bytes, &p),
                  "fasta_scan: tile_bytes must be 0 or a multiple of 1024 in 1024..65536, text_bytes not negative");
    BESST_REQUIRE(info && workspace && (text || text_bytes == 0), "fasta_scan: null pointer");
    BESST_REQUIRE(workspace_bytes >= p.bytes, "fasta_scan: workspace too small (besst_dev_fasta_workspace_bytes)");
    BESST_REQUIRE((reinterpret_cast<uintptr_t>(text) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0 &&
                      (reinterpret_cast<uintptr_t>(info) & 7) == 0,
                  "fasta_scan: text must be 16-byte aligned, the workspace 256-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    uint8_t* flags = reinterpret_cast<uint8_t*>(ws + p.o_flags);
    uint8_t* state = reinterpret_cast<uint8_t*>(ws + p.o_state);
    int64_t* kept = reinterpret_cast<int64_t*>(ws + p.o_kept);
    int64_t* rows = reinterpret_cast<int64_t*>(ws + p.o_rows);
    int64_t* names = reinterpret_cast<int64_t*>(ws + p.o_names);
    unsigned long long* err = reinterpret_cast<unsigned long long*>(info + 3);
    BESST_HIP_TRY(hipMemsetAsync(info, 0xff, BESST_FASTA_INFO_WORDS * sizeof(int64_t), s));
    const uint32_t grid = (uint32_t)((p.n_tiles + kFastaWaves - 1) / kFastaWaves);
    if (grid) {
        hipLaunchKernelGGL(fasta_flags_kernel, dim3(grid), dim3(kFastaThreads), 0, s, text, text_bytes, p.rounds, p.n_tiles,
                           flags, err);
        hipLaunchKernelGGL(fasta_state_kernel, dim3(1), dim3(kScanThreads), 0, s, flags, p.n_tiles, state);
        const FastaOut none{};
        hipLaunchKernelGGL(fasta_walk_kernel<false>, dim3(grid), dim3(kFastaThreads), 0, s, text, text_bytes, p.rounds,
                           p.n_tiles, state, kept, rows, names, none, err);
    }
    hipLaunchKernelGGL(fasta_offsets_kernel, dim3(1), dim3(kScanThreads), 0, s, p.n_tiles, kept, rows, names, info);
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

int besst_dev_fasta_pack(void* stream, const uint8_t* text, int64_t text_bytes, int64_t tile_bytes, const void* workspace,
                         size_t workspace_bytes, int64_t* info, int64_t n_contigs, int64_t pool_bytes,
                         int64_t names_bytes, uint8_t* pool, int64_t* ctg_off, int32_t* ctg_len, uint8_t* names,
                         int64_t* name_off) {
    FastaPlan p;
    BESST_REQUIRE(plan_fasta(text_bytes, tile_bytes, &p),
                  "fasta_pack: tile_bytes must be 0 or a multiple of 1024 in 1024..65536, text_bytes not negative");
    BESST_REQUIRE(n_contigs >= 1 && pool_bytes >= 0 && pool_bytes <= text_bytes && names_bytes >= 0 &&
                      names_bytes <= text_bytes && n_contigs <= text_bytes / 2 + 1,
                  "fasta_pack: sizes are not those of a scan of this text");
    BESST_REQUIRE(info && workspace && pool && ctg_off && ctg_len && names && name_off && (text || text_bytes == 0),
                  "fasta_pack: null pointer");
    BESST_REQUIRE(workspace_bytes >= p.bytes, "fasta_pack: workspace too small (besst_dev_fasta_workspace_bytes)");
    BESST_REQUIRE((reinterpret_cast<uintptr_t>(text) & 15) == 0 && (reinterpret_cast<uintptr_t>(pool) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
                  "fasta_pack: text and pool must be 16-byte aligned, the workspace 256-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = const_cast<char*>(static_cast<const char*>(workspace));
    const uint8_t* state = reinterpret_cast<const uint8_t*>(ws + p.o_state);
    int64_t* kept = reinterpret_cast<int64_t*>(ws + p.o_kept);
    int64_t* rows = reinterpret_cast<int64_t*>(ws + p.o_rows);
    int64_t* tnames = reinterpret_cast<int64_t*>(ws + p.o_names);
    const uint32_t grid = (uint32_t)((p.n_tiles + kFastaWaves - 1) / kFastaWaves);
    if (grid) {
        const FastaOut out{pool, pool_bytes, n_contigs, ctg_off, names, names_bytes, name_off};
        hipLaunchKernelGGL(fasta_walk_kernel<true>, dim3(grid), dim3(kFastaThreads), 0, s, text, text_bytes, p.rounds,
                           p.n_tiles, state, kept, rows, tnames, out, nullptr);
    }
    hipLaunchKernelGGL(fasta_rows_kernel, dim3((uint32_t)((n_contigs + 255) / 256)), dim3(256), 0, s, n_contigs, pool_bytes,
                       names_bytes, info, ctg_off, ctg_len, name_off, reinterpret_cast<unsigned long long*>(info + 4));
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

}  // extern "C"
