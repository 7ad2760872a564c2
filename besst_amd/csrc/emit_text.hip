// Scaffold output, the text files: info-pass<n>.agp / info-pass<n>.gff (BESST/GenerateOutput.py:156-195, 208-221) and the
// wrapped FASTA of repeats.fa / low_coverage_contigs.fa (:47-53, 68-74), formatted on the device.
//
// AGP / GFF.  The host hands over flat columns in output order (position, length, store row, direction, scaffold ordinal
// per contig; first contig per scaffold) - the names stay where they are, in the store's name pool.  Every contig owns
// its lines of either file: the gap line in front of it (when it is not the first of its scaffold and lies behind the end
// of its predecessor) and its own line.
//
//   text_flags_kernel    the gap flag of every contig
//   text_scan_kernel<1>  exclusive scan of the flags: with the scaffold's first contig this gives the component number
//   text_measure_kernel  bytes of every contig's AGP and GFF lines (a formatter that only counts)
//   text_scan_kernel<2>  exclusive scans of the two byte counts behind the file headers: offsets (n + 1 entries), totals
//   text_emit_kernel     a workgroup owns a fixed tile of the requested byte range of the file, finds the contigs whose
//                        lines meet the tile by binary search in the offsets, each lane formats the lines of its contigs
//                        (the same formatter, writing) into the tile in LDS, clipped to it, and the tile leaves in
//                        aligned 16-byte stores; only the last, partial 16-byte group of a range is stored by bytes.
//
// The scans run in one workgroup, BESST_TEXT_SCAN_CHUNK entries per turn (100 k contigs: all of measuring takes 0.2 ms;
// not timed at millions of contigs, where a multi-workgroup scan may pay).  Numbers are signed decimals as Python's
// str(int) writes them; a gap is formed modulo 2^64 and written unsigned, so positions up to 2^62 in magnitude cannot overflow.
//
// wrap_fasta_kernel      '>' name '\n', then the sequence in lines of 60 bytes.  Output-tile-owned like emit_kernel: a
//                        lane builds 16 output bytes and stores them once.  The host supplies the prefix sum of the record
//                        sizes; the kernel checks every record against names and lengths, so a wrong table is a status.
//                        A group that lies inside one sequence holds at most one line end: 16 source bytes are loaded
//                        from aligned dwords and the '\n' is shifted in; groups on a record edge are built byte by byte.
#include "common.h"

namespace besst {

namespace {

constexpr int kTextThreads = BESST_TEXT_THREADS;
constexpr int64_t kTextTile = BESST_TEXT_TILE_BYTES;
constexpr int kScanThreads = 1024;
constexpr int kScanItems = 4;
static_assert(kScanThreads * kScanItems == BESST_TEXT_SCAN_CHUNK, "the exported chunk is the kernel's");
constexpr int kWrapThreads = 256;
constexpr int kWrapGroups = 4;                                   // 16-byte groups per lane
static_assert((int64_t)kWrapThreads * 16 * kWrapGroups == BESST_WRAP_TILE_BYTES, "the exported tile is the kernel's");
constexpr int kLine = 60;                                        // bases per FASTA line

typedef besst_text_columns Cols;
typedef uint32_t u32x4_aligned __attribute__((ext_vector_type(4), aligned(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ int digits_of(uint64_t v) {
    int d = 1;
    while (v >= 10) { v /= 10; ++d; }
    return d;
}

// ---- the two sinks of the formatter: one counts, one writes the bytes that fall into [t0, t1) to tile[byte - t0] -----
struct CountSink {
    int64_t at;
    __device__ __forceinline__ void ch(char) { ++at; }
    template <int N> __device__ __forceinline__ void lit(const char (&)[N]) { at += N - 1; }
    __device__ __forceinline__ void u64(uint64_t v) { at += digits_of(v); }
    __device__ __forceinline__ void bytes(const uint8_t*, int64_t n) { at += n; }
};

struct TileSink {
    int64_t at, t0, t1;
    uint8_t* tile;
    __device__ __forceinline__ void put(int64_t where, uint8_t c) { if (where >= t0 && where < t1) tile[where - t0] = c; }
    __device__ __forceinline__ void ch(char c) { put(at, (uint8_t)c); ++at; }
    template <int N> __device__ __forceinline__ void lit(const char (&s)[N]) {
#pragma unroll
        for (int j = 0; j < N - 1; ++j) put(at + j, (uint8_t)s[j]);
        at += N - 1;
    }
    __device__ __forceinline__ void u64(uint64_t v) {
        const int d = digits_of(v);
        for (int j = d - 1; j >= 0; --j) { put(at + j, (uint8_t)('0' + v % 10)); v /= 10; }
        at += d;
    }
    __device__ __forceinline__ void bytes(const uint8_t* p, int64_t n) {
        const int64_t lo = t0 > at ? t0 - at : 0, hi = t1 - at < n ? t1 - at : n;      // the part inside the tile
        for (int64_t j = lo; j < hi; ++j) tile[at + j - t0] = p[j];
        at += n;
    }
};

template <class S> __device__ __forceinline__ void put_i64(S& s, int64_t v) {
    if (v < 0) { s.ch('-'); s.u64((uint64_t)0 - (uint64_t)v); } else { s.u64((uint64_t)v); }
}

// ---- what a contig's lines are made of ------------------------------------------------------------------------------
struct ContigLines {
    int64_t pos, len, prev_end, component, ordinal;              // component: of the contig's own line
    const uint8_t* name;
    int64_t name_len, short_len;
    bool gap, forward, bad;
};

// the gap flag: not the first of its scaffold and behind the end of its predecessor
__device__ __forceinline__ bool has_gap(const Cols& c, int64_t i) {
    return i > 0 && c.scaffold[i] == c.scaffold[i - 1] && c.pos[i] > c.pos[i - 1] + c.len[i - 1];
}

// gaps: exclusive scan of the gap flags (n + 1 entries)
__device__ __forceinline__ ContigLines read_contig(const Cols& c, const int64_t* __restrict__ gaps, int64_t i) {
    ContigLines l;
    l.pos = c.pos[i];
    l.len = c.len[i];
    l.forward = c.forward[i] != 0;
    l.bad = false;
    l.ordinal = c.scaffold[i];
    int64_t start = i;
    if (l.ordinal < 0 || l.ordinal >= c.n_scaffolds) {
        l.bad = true;
    } else {
        start = c.scaffold_start[l.ordinal];
        if (start < 0 || start > i) { l.bad = true; start = i; }
    }
    l.gap = gaps[i + 1] - gaps[i] == 1;
    l.prev_end = l.gap ? c.pos[i - 1] + c.len[i - 1] : 0;
    l.component = (i - start) + 1 + (gaps[i + 1] - gaps[start]);
    const int64_t row = c.row[i];
    l.name = c.names;
    l.name_len = 0;
    if (row < 0 || row >= c.n_names) {
        l.bad = true;
    } else {
        const int64_t a = c.name_off[row], b = c.name_off[row + 1];
        if (a < 0 || b < a || b > c.names_bytes) {
            l.bad = true;
        } else {
            l.name = c.names + a;
            l.name_len = b - a;
        }
    }
    l.short_len = l.name_len;                                    // up to the second '_', the whole name without one
    return l;
}

__device__ __forceinline__ int64_t short_name_len(const ContigLines& l) {
    int seen = 0;
    for (int64_t j = 0; j < l.name_len; ++j)
        if (l.name[j] == '_' && ++seen == 2) return j;
    return l.name_len;
}

template <class S> __device__ __forceinline__ void put_scaffold(S& s, const Cols& c, const ContigLines& l) {
    s.lit("scaffold_");
    s.u64((uint64_t)(l.ordinal + 1));
    s.lit("_uid_");
    put_i64(s, c.unique_id);
}

template <class S> __device__ __forceinline__ void put_agp(S& s, const Cols& c, const ContigLines& l) {
    if (l.gap) {
        put_scaffold(s, c, l);
        s.ch('\t'); put_i64(s, l.prev_end + 1);
        s.ch('\t'); put_i64(s, l.pos);
        s.ch('\t'); s.u64((uint64_t)(l.component - 1));
        s.lit("\tN\t");
        s.u64((uint64_t)l.pos - (uint64_t)l.prev_end);
        s.lit("\tscaffold\tyes\tpaired-ends\n");
    }
    put_scaffold(s, c, l);
    s.ch('\t'); put_i64(s, l.pos + 1);
    s.ch('\t'); put_i64(s, l.pos + l.len);
    s.ch('\t'); s.u64((uint64_t)l.component);
    s.lit("\tW\t");
    s.bytes(l.name, l.name_len);
    s.lit("\t1\t");
    put_i64(s, l.len);
    s.ch('\t'); s.ch(l.forward ? '+' : '-'); s.ch('\n');
}

template <class S> __device__ __forceinline__ void put_gff(S& s, const Cols& c, const ContigLines& l) {
    if (l.gap) {
        put_scaffold(s, c, l);
        s.lit("\tbesst_assembly\tgap\t");
        put_i64(s, l.prev_end + 1);
        s.ch('\t'); put_i64(s, l.pos);
        s.lit("\t.\t.\t.\t\n");
    }
    put_scaffold(s, c, l);
    s.lit("\tbesst_assembly\tcontig\t");
    put_i64(s, l.pos + 1);
    s.ch('\t'); put_i64(s, l.pos + l.len);
    s.lit("\t.\t");
    s.ch(l.forward ? '+' : '-');
    s.lit("\t.\tID=");
    s.bytes(l.name, l.name_len);
    s.lit(";Name=");
    s.bytes(l.name, l.short_len);
    s.ch('\n');
}

#define BESST_AGP_HEADER "##agp-version 2.0\n#lw-scaffolder output\n"
#define BESST_GFF_HEADER "##gff-version 3\n"
template <class S> __device__ __forceinline__ void put_header(S& s, bool gff) {
    if (gff) s.lit(BESST_GFF_HEADER); else s.lit(BESST_AGP_HEADER);
}

// ---- flags, measure ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTextThreads) void text_flags_kernel(Cols c, int64_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kTextThreads + threadIdx.x;
    if (i < c.n_contigs) flags[i] = has_gap(c, i) ? 1 : 0;
}

__global__ __launch_bounds__(kTextThreads) void text_measure_kernel(Cols c, const int64_t* __restrict__ gaps,
                                                                    int64_t* __restrict__ agp_len, int64_t* __restrict__ gff_len,
                                                                    unsigned long long* __restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * kTextThreads + threadIdx.x;
    if (i >= c.n_contigs) return;
    ContigLines l = read_contig(c, gaps, i);
    l.short_len = short_name_len(l);
    if (l.bad) atomicMin(err, (unsigned long long)i);
    CountSink a{0}, g{0};
    put_agp(a, c, l);
    put_gff(g, c, l);
    agp_len[i] = a.at;
    gff_len[i] = g.at;
}

// ---- exclusive scan of NC int64 columns of n entries in one workgroup: out[c][i] = base[c] + sum(in[c][0..i)), n + 1
// entries, the last also to total[c].  in and out may be the same array. ---------------------------------------------------
template <int NC> struct ScanCols {
    const int64_t* in[NC];
    int64_t* out[NC];
    int64_t base[NC];
    int64_t* total[NC];
};

template <int NC> __global__ __launch_bounds__(kScanThreads) void text_scan_kernel(ScanCols<NC> s, int64_t n) {
    __shared__ int64_t wave_sum[NC][kScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t carry[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) carry[c] = s.base[c];
    for (int64_t chunk = 0; chunk < n; chunk += (int64_t)kScanThreads * kScanItems) {
        const int64_t i0 = chunk + (int64_t)threadIdx.x * kScanItems;
        int64_t v[NC][kScanItems], incl[NC], mine[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            mine[c] = 0;
#pragma unroll
            for (int k = 0; k < kScanItems; ++k) {
                v[c][k] = i0 + k < n ? s.in[c][i0 + k] : 0;
                mine[c] += v[c][k];
            }
            int64_t x = mine[c];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int64_t y = __shfl_up((long long)x, d, 64);
                if (lane >= d) x += y;
            }
            incl[c] = x;
            if (lane == 63) wave_sum[c][wave] = x;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            int64_t before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < kScanThreads / 64; ++w) {
                const int64_t t = wave_sum[c][w];
                if (w < wave) before += t;
                all += t;
            }
            int64_t run = carry[c] + before + incl[c] - mine[c];
#pragma unroll
            for (int k = 0; k < kScanItems; ++k) {
                if (i0 + k < n) s.out[c][i0 + k] = run;
                run += v[c][k];
            }
            carry[c] += all;
        }
        __syncthreads();                                         // wave_sum is written again in the next turn
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            s.out[c][n] = carry[c];
            if (s.total[c]) *s.total[c] = carry[c];
        }
    }
}

// ---- emission of a byte range of one of the two files -----------------------------------------------------------------
// off: n + 1 entries, off[i] = file offset of contig i's lines, off[0] = bytes of the file header, off[n] = file size
__global__ __launch_bounds__(kTextThreads) void text_emit_kernel(Cols c, const int64_t* __restrict__ gaps,
                                                                 const int64_t* __restrict__ off, int gff, int64_t begin,
                                                                 int64_t end, uint8_t* __restrict__ out,
                                                                 unsigned long long* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[kTextTile];
    const int64_t n = c.n_contigs;
    const int64_t t0 = begin + (int64_t)blockIdx.x * kTextTile;
    const int64_t t1 = t0 + kTextTile < end ? t0 + kTextTile : end;
    if (t1 > off[n]) {                                           // a range past the end of the file: those bytes are 0
        for (int j = threadIdx.x; j < (int)(kTextTile / 16); j += kTextThreads)
            reinterpret_cast<u32x4_aligned*>(tile)[j] = u32x4_aligned{0u, 0u, 0u, 0u};
        __syncthreads();
    }
    if (t0 < off[0] && threadIdx.x == 0) {
        TileSink s{0, t0, t1, tile};
        put_header(s, gff != 0);
    }
    // the contigs whose lines meet [t0, t1): the first i with off[i + 1] > t0 up to the first with off[i] >= t1
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid + 1] > t0) hi = mid; else lo = mid + 1;
    }
    const int64_t first = lo;
    hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] >= t1) hi = mid; else lo = mid + 1;
    }
    const int64_t stop = lo;
    for (int64_t i = first + threadIdx.x; i < stop; i += kTextThreads) {
        ContigLines l = read_contig(c, gaps, i);
        if (l.bad) atomicMin(err, (unsigned long long)i);
        TileSink s{off[i], t0, t1, tile};
        if (gff) {
            l.short_len = short_name_len(l);
            put_gff(s, c, l);
        } else {
            put_agp(s, c, l);
        }
    }
    __syncthreads();
    const int nb = (int)(t1 - t0), groups = nb >> 4;
    uint8_t* dst = out + (t0 - begin);
    for (int g = threadIdx.x; g < groups; g += kTextThreads)
        reinterpret_cast<u32x4_aligned*>(dst)[g] = reinterpret_cast<const u32x4_aligned*>(tile)[g];
    for (int j = (groups << 4) + threadIdx.x; j < nb; j += kTextThreads) dst[j] = tile[j];   // the range's last few bytes
}

// ---- wrapped FASTA -----------------------------------------------------------------------------------------------------
struct WrapArgs {
    const uint8_t* pool;
    int64_t pool_bytes, n_contigs;
    const int64_t* ctg_off;
    const int32_t* ctg_len;
    const uint8_t* names;
    int64_t names_bytes;
    const int64_t* name_off;
    int64_t n_rows;
    const int64_t* rows;
    const int64_t* rec_off;                                      // n_rows + 1: exclusive prefix sum of the record sizes
    unsigned long long* err;
};

struct WrapRecord {
    int64_t begin, end, name_at, name_len, seq_at, seq_len;
    bool ok;
};

__device__ __forceinline__ WrapRecord read_record(const WrapArgs& a, int64_t r) {
    WrapRecord w{a.rec_off[r], a.rec_off[r + 1], 0, 0, 0, 0, false};
    const int64_t row = a.rows[r];
    if (row >= 0 && row < a.n_contigs) {
        const int64_t na = a.name_off[row], nb = a.name_off[row + 1], so = a.ctg_off[row], sl = a.ctg_len[row];
        if (na >= 0 && nb >= na && nb <= a.names_bytes && so >= 0 && sl >= 0 && so + sl <= a.pool_bytes &&
            w.end - w.begin == 2 + (nb - na) + sl + (sl + kLine - 1) / kLine) {
            w.name_at = na; w.name_len = nb - na; w.seq_at = so; w.seq_len = sl; w.ok = true;
        }
    }
    if (!w.ok) atomicMin(a.err, (unsigned long long)r);
    return w;
}

// byte x of the record
__device__ __forceinline__ uint8_t record_byte(const WrapArgs& a, const WrapRecord& w, int64_t x) {
    if (!w.ok) return (uint8_t)'?';
    if (x == 0) return (uint8_t)'>';
    if (x <= w.name_len) return a.names[w.name_at + x - 1];
    if (x == w.name_len + 1) return (uint8_t)'\n';
    const int64_t q = x - 2 - w.name_len;                        // byte of the body: 60 bases, '\n', 60 bases, ...
    if (q % (kLine + 1) == kLine || x == w.end - w.begin - 1) return (uint8_t)'\n';
    return a.pool[w.seq_at + q - q / (kLine + 1)];
}

__global__ __launch_bounds__(kWrapThreads) void wrap_fasta_kernel(WrapArgs a, int64_t begin, int64_t end,
                                                                  uint8_t* __restrict__ out) {
    const int64_t t0 = begin + (int64_t)blockIdx.x * BESST_WRAP_TILE_BYTES;
    const int64_t t1 = t0 + BESST_WRAP_TILE_BYTES < end ? t0 + BESST_WRAP_TILE_BYTES : end;
    // the records of the tile: the last r with rec_off[r] <= t0 (a record has at least two bytes), the last with
    // rec_off[r] < t1
    int64_t lo = 0, hi = a.n_rows;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.rec_off[mid] <= t0) lo = mid; else hi = mid;
    }
    const int64_t r_first = lo;
    hi = a.n_rows;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.rec_off[mid] < t1) lo = mid; else hi = mid;
    }
    const int64_t r_last = lo;
#pragma unroll 1
    for (int g = 0; g < kWrapGroups; ++g) {
        const int64_t o = t0 + ((int64_t)g * kWrapThreads + threadIdx.x) * 16;
        if (o >= t1) break;
        const int64_t o_end = o + 16 < t1 ? o + 16 : t1;
        int64_t r = r_first, top = r_last + 1;
        while (top - r > 1) {
            const int64_t mid = (r + top) >> 1;
            if (a.rec_off[mid] <= o) r = mid; else top = mid;
        }
        WrapRecord w = read_record(a, r);
        uint8_t* dst = out + (o - begin);
        const int64_t body = w.begin + 2 + w.name_len;
        if (w.ok && o >= body && o + 16 < w.end && o + 16 <= t1) {
            // inside one sequence, in front of its last byte: at most one line end among the 16 bytes
            const int64_t q = o - body;
            const int k = kLine - (int)(q % (kLine + 1));        // the group's byte k is the '\n' (0..60)
            const uint8_t* p = a.pool + (w.seq_at + q - q / (kLine + 1));
            const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
            const uint32_t* d = reinterpret_cast<const uint32_t*>(p - sh);
            const u32x4 v = *reinterpret_cast<const u32x4*>(d);
            const uint32_t d4 = d[4];
            const uint64_t s0 = __builtin_amdgcn_alignbyte(v.y, v.x, sh), s1 = __builtin_amdgcn_alignbyte(v.z, v.y, sh),
                           s2 = __builtin_amdgcn_alignbyte(v.w, v.z, sh), s3 = __builtin_amdgcn_alignbyte(d4, v.w, sh);
            uint64_t w0 = s0 | (s1 << 32), w1 = s2 | (s3 << 32);
            if (k < 8) {
                const uint64_t below = k ? ~0ull >> (64 - 8 * k) : 0ull;
                w1 = (w1 << 8) | (w0 >> 56);
                w0 = (w0 & below) | ((uint64_t)'\n' << (8 * k)) | ((w0 & ~below) << 8);
            } else if (k < 16) {
                const int k1 = k - 8;
                const uint64_t below = k1 ? ~0ull >> (64 - 8 * k1) : 0ull;
                w1 = (w1 & below) | ((uint64_t)'\n' << (8 * k1)) | ((w1 & ~below) << 8);
            }
            *reinterpret_cast<u32x4_aligned*>(dst) =
                u32x4_aligned{(uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32)};
            continue;
        }
        uint32_t rr[4] = {0u, 0u, 0u, 0u};
        for (int j = 0; j < (int)(o_end - o); ++j) {
            while (o + j >= w.end && r + 1 < a.n_rows) w = read_record(a, ++r);
            const uint8_t b = o + j < w.end ? record_byte(a, w, o + j - w.begin) : (uint8_t)0;
            rr[j >> 2] |= (uint32_t)b << (8 * (j & 3));
        }
        if (o_end - o == 16) {
            *reinterpret_cast<u32x4_aligned*>(dst) = u32x4_aligned{rr[0], rr[1], rr[2], rr[3]};
        } else {
            for (int j = 0; j < (int)(o_end - o); ++j) dst[j] = (uint8_t)(rr[j >> 2] >> (8 * (j & 3)));
        }
    }
}

struct TextPlan {
    size_t o_gaps, o_agp, o_gff, bytes;
};

bool plan_text(int64_t n, TextPlan* p) {
    if (n < 0 || n >= ((int64_t)1 << 31)) return false;
    const size_t col = align_up((size_t)(n + 1) * 8, 256);
    p->o_gaps = 0;
    p->o_agp = col;
    p->o_gff = 2 * col;
    p->bytes = 3 * col;
    return true;
}

int check_columns(const Cols* c, const void* workspace, size_t workspace_bytes, TextPlan* p) {
    BESST_REQUIRE(c && workspace, "text: null pointer");
    BESST_REQUIRE(plan_text(c->n_contigs, p) && c->n_scaffolds >= 0 && c->n_scaffolds <= c->n_contigs && c->n_names >= 0 &&
                      c->names_bytes >= 0,
                  "text: size out of range");
    BESST_REQUIRE(workspace_bytes >= p->bytes, "text: workspace too small (besst_dev_text_workspace_bytes)");
    BESST_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "text: the workspace must be 256-byte aligned");
    if (c->n_contigs)
        BESST_REQUIRE(c->pos && c->len && c->row && c->forward && c->scaffold && c->scaffold_start && c->name_off &&
                          (c->names || c->names_bytes == 0),
                      "text: null column");
    return BESST_OK;
}

}  // namespace

}  // namespace besst

using namespace besst;

extern "C" {

size_t besst_dev_text_workspace_bytes(int64_t n_contigs) {
    TextPlan p;
    return plan_text(n_contigs, &p) ? p.bytes : 0;
}

int besst_dev_text_measure(void* stream, const besst_text_columns* cols, void* workspace, size_t workspace_bytes,
                           int64_t* info) {
    TextPlan p;
    const int rc = check_columns(cols, workspace, workspace_bytes, &p);
    if (rc != BESST_OK) return rc;
    BESST_REQUIRE(info && (reinterpret_cast<uintptr_t>(info) & 7) == 0, "text_measure: info must be an aligned pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    int64_t* gaps = reinterpret_cast<int64_t*>(ws + p.o_gaps);
    int64_t* agp = reinterpret_cast<int64_t*>(ws + p.o_agp);
    int64_t* gff = reinterpret_cast<int64_t*>(ws + p.o_gff);
    const int64_t n = cols->n_contigs;
    BESST_HIP_TRY(hipMemsetAsync(info, 0xff, BESST_TEXT_INFO_WORDS * sizeof(int64_t), s));
    const uint32_t grid = (uint32_t)((n + kTextThreads - 1) / kTextThreads);
    if (grid) hipLaunchKernelGGL(text_flags_kernel, dim3(grid), dim3(kTextThreads), 0, s, *cols, gaps);
    const ScanCols<1> one{{gaps}, {gaps}, {0}, {nullptr}};
    hipLaunchKernelGGL(text_scan_kernel<1>, dim3(1), dim3(kScanThreads), 0, s, one, n);
    if (grid)
        hipLaunchKernelGGL(text_measure_kernel, dim3(grid), dim3(kTextThreads), 0, s, *cols, gaps, agp, gff,
                           reinterpret_cast<unsigned long long*>(info + 2));
    const ScanCols<2> two{{agp, gff}, {agp, gff}, {(int64_t)sizeof(BESST_AGP_HEADER) - 1, (int64_t)sizeof(BESST_GFF_HEADER) - 1},
                          {info, info + 1}};
    hipLaunchKernelGGL(text_scan_kernel<2>, dim3(1), dim3(kScanThreads), 0, s, two, n);
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

int besst_dev_text_emit(void* stream, const besst_text_columns* cols, const void* workspace, size_t workspace_bytes,
                        int32_t which, int64_t begin, int64_t end, uint8_t* out, int64_t* info) {
    TextPlan p;
    const int rc = check_columns(cols, workspace, workspace_bytes, &p);
    if (rc != BESST_OK) return rc;
    BESST_REQUIRE(which == BESST_TEXT_AGP || which == BESST_TEXT_GFF, "text_emit: which must be BESST_TEXT_AGP or BESST_TEXT_GFF");
    BESST_REQUIRE(begin >= 0 && begin <= end, "text_emit: bad output range");
    if (begin == end) return BESST_OK;
    BESST_REQUIRE(out && info, "text_emit: null pointer");
    BESST_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "text_emit: out must be 16-byte aligned");
    const int64_t tiles = (end - begin + kTextTile - 1) / kTextTile;
    BESST_REQUIRE(tiles < ((int64_t)1 << 31), "text_emit: output range too long for one call");
    const char* ws = static_cast<const char*>(workspace);
    const int64_t* gaps = reinterpret_cast<const int64_t*>(ws + p.o_gaps);
    const int64_t* off = reinterpret_cast<const int64_t*>(ws + (which == BESST_TEXT_GFF ? p.o_gff : p.o_agp));
    hipLaunchKernelGGL(text_emit_kernel, dim3((uint32_t)tiles), dim3(kTextThreads), 0, static_cast<hipStream_t>(stream), *cols,
                       gaps, off, (int)which, begin, end, out, reinterpret_cast<unsigned long long*>(info + 2));
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

int besst_dev_wrap_fasta(void* stream, const uint8_t* pool, int64_t pool_bytes, int64_t n_contigs, const int64_t* ctg_off,
                         const int32_t* ctg_len, const uint8_t* names, int64_t names_bytes, const int64_t* name_off,
                         int64_t n_rows, const int64_t* rows, const int64_t* rec_off, int64_t begin, int64_t end,
                         uint8_t* out, uint64_t* err) {
    BESST_REQUIRE(pool_bytes >= 0 && n_contigs >= 0 && names_bytes >= 0 && n_rows >= 0 && n_rows < ((int64_t)1 << 31),
                  "wrap_fasta: size out of range");
    BESST_REQUIRE(begin >= 0 && begin <= end, "wrap_fasta: bad output range");
    if (begin == end) return BESST_OK;
    BESST_REQUIRE(n_rows > 0, "wrap_fasta: output range past the end of an empty table");
    BESST_REQUIRE(pool && ctg_off && ctg_len && (names || names_bytes == 0) && name_off && rows && rec_off && out && err,
                  "wrap_fasta: null pointer");
    BESST_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "wrap_fasta: out must be 16-byte aligned");
    BESST_REQUIRE((reinterpret_cast<uintptr_t>(pool) & 3) == 0, "wrap_fasta: pool must be 4-byte aligned");
    const int64_t tiles = (end - begin + BESST_WRAP_TILE_BYTES - 1) / BESST_WRAP_TILE_BYTES;
    BESST_REQUIRE(tiles < ((int64_t)1 << 31), "wrap_fasta: output range too long for one call");
    const WrapArgs a{pool, pool_bytes, n_contigs, ctg_off, ctg_len, names, names_bytes, name_off, n_rows, rows, rec_off,
                     reinterpret_cast<unsigned long long*>(err)};
    hipLaunchKernelGGL(wrap_fasta_kernel, dim3((uint32_t)tiles), dim3(kWrapThreads), 0, static_cast<hipStream_t>(stream), a,
                       begin, end, out);
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

}  // extern "C"
