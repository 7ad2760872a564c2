// The BAM report: one pass over the eight resident record columns (25 bytes per record) that counts what `samtools flagstat`
// and `samtools idxstats` print, the mapq / aligned-length / insert-size distributions, and a 16-byte digest of the columns.
// Everything is a sum (or an xor) of 64-bit integers over ALL records, so the result is exact and the same in any order.
//
// Word layout of the result (include/besst_amd.h, besst_dev_library_report): 40 scalar words (16 census rows x {QC-pass,
// QC-fail}, unplaced, tid_out_of_range, the four pair classes, the digest's sum and xor), mapq[256], qlen[65536],
// mapped[n_refs], placed_unmapped[n_refs], then innie / outie / tandem |tlen| histograms of isize_bins + 1 words each.
//
// The digest, so that a script over another decoder's records can reproduce it (all arithmetic mod 2^64):
//     splitmix64(x): x += 0x9e3779b97f4a7c15; x = (x ^ x >> 30) * 0xbf58476d1ce4e5b9; x = (x ^ x >> 27) * 0x94d049bb133111eb;
//                    return x ^ x >> 31
//     a = (u32)tid | (u64)(u32)mtid << 32;  b = (u32)pos | (u64)(u32)mpos << 32;  c = (u32)tlen | (u64)flag << 32 | (u64)qlen << 48
//     h = splitmix64(splitmix64(splitmix64(splitmix64(a) ^ b) ^ c) ^ mapq)
//     word 38 = sum of h over the records, word 39 = xor of h over the records
//
// The kernel.  512 threads, a fixed grid (two workgroups per CU, 69 KB of LDS each), every workgroup takes one CONTIGUOUS
// piece of the stream - a wave then meets the same reference in step after step of a coordinate-sorted stream - and every
// lane four consecutive records per step (16-byte loads of the int32 columns, 8 of the uint16 ones, 4 of mapq).  A column that
// is not aligned for its vector at the first group is read element by element instead; the up to three records in front of
// the first aligned group and behind the last whole one are taken by one wave of workgroup 0 in a step of its own.
//   census, pair classes  per-wave ballots + population counts in scalar registers; one LDS add per wave, one 64-bit global
//                         atomic per counter and workgroup at the end
//   mapq                  256 LDS bins per workgroup (the values most lanes share are added once per wave), flushed once
//   qlen                  1024 LDS bins for the short reads every library is made of, flushed once; longer: global atomics,
//                         once per wave for the values lanes share
//   |tlen|                innie and outie: 8192 LDS bins each, flushed once; above, and tandem: global atomics; the overflow
//                         bins are counted like the census
//   per reference         a wave whose lanes lie on one reference adds two population counts to a (reference, mapped,
//                         unmapped) run it keeps in scalar registers and writes the run out - two atomics - when the reference
//                         changes; a mixed wave takes the references several lanes share first, then one atomic per lane
// No workgroup waits for another, nothing spins, and there is no float anywhere.
#include <stdlib.h>

#include "common.h"

namespace besst {

namespace {

constexpr int kThreads = 512;
constexpr int kQlenLds = 1024;       // qlen values below this are counted in LDS
constexpr int kIsizeLds = 8192;      // |tlen| below this (innie, outie) is counted in LDS
constexpr int kBlockCounters = BESST_REPORT_MAPQ + 3;      // the scalar words + the three overflow bins
// BESST_REPORT_CUT (tools/time_bam_report.py): a mask of parts the kernel leaves out, to see where its time goes; the report is
// then incomplete
constexpr uint32_t kCutMapq = 1, kCutQlen = 2, kCutIsize = 4, kCutRefs = 8, kCutDigest = 16;

struct Shared {
    unsigned long long counters[kBlockCounters];
    uint32_t mapq[256];
    uint32_t qlen[kQlenLds];
    uint32_t isize[2][kIsizeLds];
};

struct Rec {
    int32_t tid, mtid, pos, mpos, tlen;
    uint32_t flag, qlen, mapq;
};

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ uint32_t popc64(uint64_t m) { return (uint32_t)__popcll(m); }

// hist[v] += 1 for every lane with `on`: the values that several lanes share are added once per wave for the first `rounds`
// distinct ones, what is left lane by lane.  Every lane of the wave calls it.
template <typename T>
__device__ __forceinline__ void wave_hist_add(T* hist, uint32_t v, bool on, int rounds, int lane) {
    for (int it = 0; it < rounds; ++it) {
        const uint64_t todo = __ballot(on);
        if (todo == 0) return;
        const int lead = __builtin_ctzll(todo);
        const uint32_t lv = (uint32_t)__shfl((int)v, lead);
        const bool same = on && v == lv;
        const uint32_t cnt = popc64(__ballot(same));
        if (lane == lead) atomicAdd(hist + lv, (T)cnt);
        on = on && !same;
    }
    if (on) atomicAdd(hist + v, (T)1);
}

struct WaveState {
    uint32_t census[32];          // row r: [2 r] QC-pass, [2 r + 1] QC-fail
    uint32_t unplaced, out_of_range, cls[4], over[3];
    int32_t run_tid;              // the reference of the run the wave is counting (-1: none)
    uint32_t run_mapped, run_unmapped;
    uint64_t sum, xr;             // per lane
};

__device__ __forceinline__ void flush_run(WaveState& w, unsigned long long* ref, int64_t n_refs, int lane) {
    if (lane == 0 && w.run_tid >= 0) {
        if (w.run_mapped) atomicAdd(ref + w.run_tid, (unsigned long long)w.run_mapped);
        if (w.run_unmapped) atomicAdd(ref + n_refs + w.run_tid, (unsigned long long)w.run_unmapped);
    }
    w.run_mapped = w.run_unmapped = 0;
}

// One record per lane (`valid`: the lane has one).  Every lane of the wave calls it.
__device__ __forceinline__ void take(const Rec& r, bool valid, WaveState& w, Shared& sh, unsigned long long* out, int64_t n_refs,
                                     uint32_t isize_bins, int lane, uint32_t cut) {
    const uint32_t f = r.flag;
    const bool mapped = valid && !(f & 0x4);
    const bool fail = (f & 0x200) != 0;
    const bool primary = valid && !(f & 0x900);
    const bool paired = primary && (f & 0x1);
    const bool both = paired && !(f & 0x4) && !(f & 0x8);
    const bool diff = both && r.tid != r.mtid;
    // ---- census: the sixteen rows as one bit each, then a ballot per row
    uint32_t rows = 0;
    rows |= valid ? 1u << 0 : 0u;                                         // in total
    rows |= primary ? 1u << 1 : 0u;                                       // primary
    rows |= (valid && (f & 0x100)) ? 1u << 2 : 0u;                        // secondary
    rows |= (valid && !(f & 0x100) && (f & 0x800)) ? 1u << 3 : 0u;        // supplementary
    rows |= (valid && (f & 0x400)) ? 1u << 4 : 0u;                        // duplicates
    rows |= (primary && (f & 0x400)) ? 1u << 5 : 0u;                      // primary duplicates
    rows |= mapped ? 1u << 6 : 0u;                                        // mapped
    rows |= (primary && !(f & 0x4)) ? 1u << 7 : 0u;                       // primary mapped
    rows |= paired ? 1u << 8 : 0u;                                        // paired in sequencing
    rows |= (paired && (f & 0x40)) ? 1u << 9 : 0u;                        // read1
    rows |= (paired && (f & 0x80)) ? 1u << 10 : 0u;                       // read2
    rows |= (paired && (f & 0x2) && !(f & 0x4)) ? 1u << 11 : 0u;          // properly paired
    rows |= both ? 1u << 12 : 0u;                                         // with itself and mate mapped
    rows |= (paired && (f & 0x8) && !(f & 0x4)) ? 1u << 13 : 0u;          // singletons
    rows |= diff ? 1u << 14 : 0u;                                         // with mate mapped to a different chr
    rows |= (diff && r.mapq >= 5) ? 1u << 15 : 0u;                        // ... (mapQ>=5)
    const uint64_t failed = __ballot(fail);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint64_t m = __ballot((rows >> k) & 1u);
        w.census[2 * k] += popc64(m & ~failed);
        w.census[2 * k + 1] += popc64(m & failed);
    }
    // ---- digest
    if (valid && !(cut & kCutDigest)) {
        const uint64_t a = (uint64_t)(uint32_t)r.tid | ((uint64_t)(uint32_t)r.mtid << 32);
        const uint64_t b = (uint64_t)(uint32_t)r.pos | ((uint64_t)(uint32_t)r.mpos << 32);
        const uint64_t c = (uint64_t)(uint32_t)r.tlen | ((uint64_t)f << 32) | ((uint64_t)r.qlen << 48);
        const uint64_t h = splitmix64(splitmix64(splitmix64(splitmix64(a) ^ b) ^ c) ^ (uint64_t)r.mapq);
        w.sum += h;
        w.xr ^= h;
    }
    // ---- mapq and qlen of the mapped records
    if (!(cut & kCutMapq)) wave_hist_add(sh.mapq, r.mapq, mapped, 2, lane);
    if (!(cut & kCutQlen)) {
        wave_hist_add(sh.qlen, r.qlen, mapped && r.qlen < (uint32_t)kQlenLds, 2, lane);
        const bool long_q = mapped && r.qlen >= (uint32_t)kQlenLds;
        if (__ballot(long_q)) wave_hist_add(out + BESST_REPORT_QLEN, r.qlen, long_q, 4, lane);
    }
    // ---- per reference
    const bool in_range = valid && (uint64_t)(uint32_t)r.tid < (uint64_t)n_refs && r.tid >= 0;
    w.unplaced += popc64(__ballot(valid && r.tid < 0));
    w.out_of_range += popc64(__ballot(valid && r.tid >= 0 && !in_range));
    unsigned long long* ref = out + BESST_REPORT_REFS;
    const uint64_t placed = (cut & kCutRefs) ? 0ull : __ballot(in_range);
    if (placed) {
        const int32_t t0 = __shfl(r.tid, __builtin_ctzll(placed));
        const uint64_t same = __ballot(in_range && r.tid == t0);
        if (same == placed) {
            if (t0 != w.run_tid) {
                flush_run(w, ref, n_refs, lane);
                w.run_tid = t0;
            }
            const uint32_t m = popc64(__ballot(in_range && mapped));
            w.run_mapped += m;
            w.run_unmapped += popc64(placed) - m;
        } else {
            bool todo = in_range;
            for (int it = 0; it < 4; ++it) {
                const uint64_t left = __ballot(todo);
                if (left == 0) break;
                const int lead = __builtin_ctzll(left);
                const int32_t tv = __shfl(r.tid, lead);
                const bool hit = todo && r.tid == tv;
                const uint32_t all = popc64(__ballot(hit)), m = popc64(__ballot(hit && mapped));
                if (lane == lead) {
                    if (m) atomicAdd(ref + tv, (unsigned long long)m);
                    if (all - m) atomicAdd(ref + n_refs + tv, (unsigned long long)(all - m));
                }
                todo = todo && !hit;
            }
            if (todo) atomicAdd(ref + (mapped ? 0 : n_refs) + r.tid, 1ull);
        }
    }
    // ---- pair geometry: read 2 of a pair on one reference
    const bool geo = both && (f & 0x80) && r.tid == r.mtid && in_range;
    const bool rev = (f & 0x10) != 0, mrev = (f & 0x20) != 0;
    const bool tandem = geo && rev == mrev;
    const bool other = geo && rev != mrev && r.tlen == 0;
    const bool innie = geo && rev != mrev && ((rev && r.tlen < 0) || (!rev && r.tlen > 0));
    const bool outie = geo && rev != mrev && r.tlen != 0 && !innie;
    w.cls[0] += popc64(__ballot(innie));
    w.cls[1] += popc64(__ballot(outie));
    w.cls[2] += popc64(__ballot(tandem));
    w.cls[3] += popc64(__ballot(other));
    if (!(cut & kCutIsize) && __ballot(innie || outie || tandem)) {
        // |tlen| in 64 bits: INT32_MIN becomes 2^31, above every bin
        const uint32_t a = r.tlen < 0 ? (uint32_t)(-(int64_t)r.tlen) : (uint32_t)r.tlen;
        const bool over = a >= isize_bins;
        w.over[0] += popc64(__ballot(innie && over));
        w.over[1] += popc64(__ballot(outie && over));
        w.over[2] += popc64(__ballot(tandem && over));
        unsigned long long* hist = ref + 2 * n_refs;
        const int which = innie ? 0 : outie ? 1 : 2;
        if ((innie || outie || tandem) && !over) {
            if (which < 2 && a < (uint32_t)kIsizeLds)
                atomicAdd(&sh.isize[which][a], 1u);
            else
                atomicAdd(hist + (uint64_t)which * ((uint64_t)isize_bins + 1) + a, 1ull);
        }
    }
}

struct ReportKernelArgs {
    const int32_t *tid, *mtid, *pos, *mpos, *tlen;
    const uint16_t *flag, *qlen;
    const uint8_t* mapq;
    long long n;            // records
    long long head;         // records in front of the first group of four
    long long n_groups;     // whole groups of four behind them
    long long groups_per_block;
    long long n_refs;
    uint32_t isize_bins;
    uint32_t vec;           // bit c: column c (the order above) is aligned for its vector at record `head`
    uint32_t cut;           // BESST_REPORT_CUT: parts left out (timing variants only, launch_library_report)
};

__device__ __forceinline__ Rec load_one(const ReportKernelArgs& a, long long i) {
    Rec r;
    r.tid = a.tid[i]; r.mtid = a.mtid[i]; r.pos = a.pos[i]; r.mpos = a.mpos[i]; r.tlen = a.tlen[i];
    r.flag = a.flag[i]; r.qlen = a.qlen[i]; r.mapq = a.mapq[i];
    return r;
}

__device__ __forceinline__ void load_i32x4(const int32_t* p, bool vec, int32_t* v) {
    if (vec) {
        const int4 x = *reinterpret_cast<const int4*>(p);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = p[k];
    }
}

__device__ __forceinline__ void load_u16x4(const uint16_t* p, bool vec, uint32_t* v) {
    if (vec) {
        const uint2 x = *reinterpret_cast<const uint2*>(p);
        v[0] = x.x & 0xffffu; v[1] = x.x >> 16; v[2] = x.y & 0xffffu; v[3] = x.y >> 16;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = p[k];
    }
}

__global__ __launch_bounds__(kThreads) void library_report_kernel(ReportKernelArgs a, unsigned long long* __restrict__ out) {
    __shared__ Shared sh;
    const int t = (int)threadIdx.x, lane = t & 63;
    {
        uint32_t* z = reinterpret_cast<uint32_t*>(&sh);
        for (int i = t; i < (int)(sizeof(Shared) / 4); i += kThreads) z[i] = 0;
    }
    __syncthreads();
    WaveState w;
#pragma unroll
    for (int k = 0; k < 32; ++k) w.census[k] = 0;
    w.unplaced = w.out_of_range = 0;
    w.cls[0] = w.cls[1] = w.cls[2] = w.cls[3] = 0;
    w.over[0] = w.over[1] = w.over[2] = 0;
    w.run_tid = -1;
    w.run_mapped = w.run_unmapped = 0;
    w.sum = w.xr = 0;
    unsigned long long* ref = out + BESST_REPORT_REFS;

    const long long g_lo = (long long)blockIdx.x * a.groups_per_block;
    const long long g_hi = g_lo + a.groups_per_block < a.n_groups ? g_lo + a.groups_per_block : a.n_groups;
    for (long long g0 = g_lo; g0 < g_hi; g0 += kThreads) {
        const long long g = g0 + t;
        const bool valid = g < g_hi;
        int32_t tid[4], mtid[4], pos[4], mpos[4], tlen[4];
        uint32_t flag[4], qlen[4], mapq[4];
        if (valid) {
            const long long i = a.head + 4 * g;
            load_i32x4(a.tid + i, a.vec & 1u, tid);
            load_i32x4(a.mtid + i, a.vec & 2u, mtid);
            load_i32x4(a.pos + i, a.vec & 4u, pos);
            load_i32x4(a.mpos + i, a.vec & 8u, mpos);
            load_i32x4(a.tlen + i, a.vec & 16u, tlen);
            load_u16x4(a.flag + i, a.vec & 32u, flag);
            load_u16x4(a.qlen + i, a.vec & 64u, qlen);
            if (a.vec & 128u) {
                const uint32_t x = *reinterpret_cast<const uint32_t*>(a.mapq + i);
                mapq[0] = x & 0xffu; mapq[1] = (x >> 8) & 0xffu; mapq[2] = (x >> 16) & 0xffu; mapq[3] = x >> 24;
            } else {
                for (int k = 0; k < 4; ++k) mapq[k] = a.mapq[i + k];
            }
        } else {
            for (int k = 0; k < 4; ++k) {
                tid[k] = mtid[k] = pos[k] = mpos[k] = tlen[k] = 0;
                flag[k] = qlen[k] = mapq[k] = 0;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            Rec r;
            r.tid = tid[k]; r.mtid = mtid[k]; r.pos = pos[k]; r.mpos = mpos[k]; r.tlen = tlen[k];
            r.flag = flag[k]; r.qlen = qlen[k]; r.mapq = mapq[k];
            take(r, valid, w, sh, out, a.n_refs, a.isize_bins, lane, a.cut);
        }
    }
    // the records in front of the first group and behind the last one: at most three each, one lane each
    if (blockIdx.x == 0 && t < 64) {
        const long long tail_lo = a.head + 4 * a.n_groups;
        const long long n_tail = a.n - tail_lo;
        long long i = -1;
        if (t < a.head) i = t;
        else if (t - a.head < n_tail) i = tail_lo + (t - a.head);
        Rec r = {0, 0, 0, 0, 0, 0u, 0u, 0u};
        if (i >= 0) r = load_one(a, i);
        take(r, i >= 0, w, sh, out, a.n_refs, a.isize_bins, lane, a.cut);
    }
    flush_run(w, ref, a.n_refs, lane);
    // ---- the wave's counters to LDS, the lanes' digests too
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (w.census[k]) atomicAdd(&sh.counters[BESST_REPORT_CENSUS + k], (unsigned long long)w.census[k]);
        if (w.unplaced) atomicAdd(&sh.counters[BESST_REPORT_UNPLACED], (unsigned long long)w.unplaced);
        if (w.out_of_range) atomicAdd(&sh.counters[BESST_REPORT_TID_OUT_OF_RANGE], (unsigned long long)w.out_of_range);
        for (int k = 0; k < 4; ++k)
            if (w.cls[k]) atomicAdd(&sh.counters[BESST_REPORT_PAIR_CLASSES + k], (unsigned long long)w.cls[k]);
        for (int k = 0; k < 3; ++k)
            if (w.over[k]) atomicAdd(&sh.counters[BESST_REPORT_MAPQ + k], (unsigned long long)w.over[k]);
    }
    // (the sum and the xor of a wave: across its lanes first)
    uint64_t s = w.sum, x = w.xr;
    for (int d = 32; d > 0; d >>= 1) {
        s += (uint64_t)__shfl_xor((unsigned long long)s, d);
        x ^= (uint64_t)__shfl_xor((unsigned long long)x, d);
    }
    if (lane == 0) {
        atomicAdd(&sh.counters[BESST_REPORT_DIGEST_SUM], (unsigned long long)s);
        atomicXor(&sh.counters[BESST_REPORT_DIGEST_XOR], (unsigned long long)x);
    }
    __syncthreads();
    // ---- the workgroup's counters and bins to the result: one atomic per word that is not zero
    const uint64_t isize_words = (uint64_t)a.isize_bins + 1;
    unsigned long long* hist = ref + 2 * a.n_refs;
    if (t < kBlockCounters) {
        const unsigned long long v = sh.counters[t];
        if (v) {
            if (t == BESST_REPORT_DIGEST_XOR) atomicXor(out + t, v);
            else if (t < BESST_REPORT_MAPQ) atomicAdd(out + t, v);
            else atomicAdd(hist + (uint64_t)(t - BESST_REPORT_MAPQ) * isize_words + a.isize_bins, v);
        }
    }
    for (int i = t; i < 256; i += kThreads)
        if (sh.mapq[i]) atomicAdd(out + BESST_REPORT_MAPQ + i, (unsigned long long)sh.mapq[i]);
    for (int i = t; i < kQlenLds; i += kThreads)
        if (sh.qlen[i]) atomicAdd(out + BESST_REPORT_QLEN + i, (unsigned long long)sh.qlen[i]);
    for (int i = t; i < 2 * kIsizeLds; i += kThreads) {
        const int which = i / kIsizeLds, bin = i % kIsizeLds;
        const uint32_t v = sh.isize[which][bin];
        if (v && (uint32_t)bin < a.isize_bins) atomicAdd(hist + (uint64_t)which * isize_words + bin, (unsigned long long)v);
    }
}

int compute_units() {
    static int cached[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cached[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev] = n;
    }
    return cached[dev];
}

}  // namespace

int launch_library_report(hipStream_t s, const besst_report_args& r, unsigned long long* out) {
    if (r.n_records <= 0) return BESST_OK;
    ReportKernelArgs a;
    a.tid = r.tid; a.mtid = r.mtid; a.pos = r.pos; a.mpos = r.mpos; a.tlen = r.tlen;
    a.flag = r.flag; a.qlen = r.qlen; a.mapq = r.mapq;
    a.n = r.n_records;
    a.n_refs = r.n_refs;
    a.isize_bins = (uint32_t)r.isize_bins;
    // records in front of the first 16-byte line of tid; the other columns are vector-read when that record aligns them too
    long long head = (long long)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(r.tid) & 15u)) & 15u) / 4u);
    if (head > a.n) head = a.n;
    a.head = head;
    a.n_groups = (a.n - head) / 4;
    auto aligned = [&](const void* p, size_t elem, size_t width) {
        return ((reinterpret_cast<uintptr_t>(p) + (size_t)head * elem) & (width - 1)) == 0;
    };
    a.vec = (aligned(r.tid, 4, 16) ? 1u : 0u) | (aligned(r.mtid, 4, 16) ? 2u : 0u) | (aligned(r.pos, 4, 16) ? 4u : 0u) |
            (aligned(r.mpos, 4, 16) ? 8u : 0u) | (aligned(r.tlen, 4, 16) ? 16u : 0u) | (aligned(r.flag, 2, 8) ? 32u : 0u) |
            (aligned(r.qlen, 2, 8) ? 64u : 0u) | (aligned(r.mapq, 1, 4) ? 128u : 0u);
    const char* cut_env = getenv("BESST_REPORT_CUT");
    a.cut = cut_env ? (uint32_t)atoi(cut_env) : 0u;
    const long long steps = (a.n_groups + kThreads - 1) / kThreads;            // workgroup steps in all
    long long blocks = 2ll * compute_units();
    if (blocks > steps) blocks = steps;
    if (blocks < 1) blocks = 1;
    a.groups_per_block = (steps + blocks - 1) / blocks * kThreads;
    hipLaunchKernelGGL(library_report_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a, out);
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

}  // namespace besst
