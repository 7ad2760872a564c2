// Scaffold output: the sequence work of GenerateOutput.PrintOutput (BESST/GenerateOutput.py:88-234) on the device.
//
// The contigs of a run lie end to end in one byte pool in HBM (one byte per base: case and IUPAC codes survive), with
// BESST_EMIT_PAD readable bytes before and after it.  Two kernels read it:
//
//   seq_overlap_kernel   check_kmer_overlap (:110-116) for the junctions the host selects: one wave per junction stages
//                        the last K bytes of the oriented left contig and the first K bytes of the oriented right
//                        contig in LDS (complemented on load where the contig is reversed); the lanes take candidate
//                        lengths, longest first, and the first round in which a lane matches gives the maximum.
//   emit_kernel          the FASTA file as a gather.  A piece table (src_off, len, mode) + out_off (exclusive prefix
//                        sum of len, n + 1 entries) names the source of every output byte: a stretch of the pool as it
//                        stands, a stretch reverse-complemented, a run of 'N', or a stretch of a small literal pool
//                        (headers, '\n', 'n').  A workgroup owns a fixed tile of the requested output range, finds the
//                        piece of the tile's first byte by one binary search and walks on from there (per wave, in
//                        scalar registers: a wave whose KiB lies in one piece reads the row once); a lane builds 16
//                        output bytes from aligned source dwords (shifted with v_alignbyte, byte-reversed with v_perm,
//                        complemented through a 256-byte table in LDS) and writes them with one 16-byte store.
//                        A 16-byte group that spans several pieces takes one turn of the same loop per piece and
//                        merges under a byte mask; the over-read this needs stays inside the pads.
//
// A byte without a complement in a stretch that is written reversed is the reference's KeyError: the kernel records
// the smallest (piece, distance from the start of the piece) in one word with a 64-bit atomicMin and carries on.
#include "common.h"

namespace besst {

namespace {

constexpr int kEmitThreads = 256;
constexpr int kEmitGroups = 4;                                   // 16-byte groups per lane
constexpr int64_t kEmitTile = (int64_t)kEmitThreads * 16 * kEmitGroups;
constexpr int kOverlapWaves = 4;                                 // junctions per workgroup
constexpr int kMaxK = BESST_MAX_CONTIG_OVERLAP;

// complement of every byte that has one (rev_nuc, GenerateOutput.py:25); 0 = none (the reference's KeyError)
struct CompTable {
    uint8_t v[256];
};
constexpr CompTable make_comp_table() {
    CompTable t{};
    const char from[] = "ACGTYRKMBVHDSWN";
    const char to[] = "TGCARYMKVBDHSWN";
    for (int i = 0; from[i]; ++i) {
        t.v[(uint8_t)from[i]] = (uint8_t)to[i];
        t.v[(uint8_t)(from[i] | 0x20)] = (uint8_t)(to[i] | 0x20);
    }
    t.v[(uint8_t)'X'] = (uint8_t)'X';                             // upper case only
    return t;
}
__constant__ CompTable kComp = make_comp_table();
const CompTable kCompHost = make_comp_table();

__device__ __forceinline__ void load_comp_table(uint8_t* lds) {  // 256 bytes, one dword per lane of the first wave
    if (threadIdx.x < 64)
        reinterpret_cast<uint32_t*>(lds)[threadIdx.x] = reinterpret_cast<const uint32_t*>(kComp.v)[threadIdx.x];
}

// ---- overlap of two oriented contig ends ----------------------------------------------------------------------------
__global__ __launch_bounds__(kOverlapWaves * 64) void seq_overlap_kernel(
    const uint8_t* __restrict__ pool, int64_t pool_bytes, int64_t n_contigs, const int64_t* __restrict__ ctg_off,
    const int32_t* __restrict__ ctg_len, int64_t n, const int32_t* __restrict__ left, const int32_t* __restrict__ right,
    const uint8_t* __restrict__ forward, int32_t K, int32_t* __restrict__ overlap, unsigned long long* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) uint8_t comp[256];
    __shared__ uint8_t win[kOverlapWaves][2][kMaxK];
    load_comp_table(comp);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kOverlapWaves + wave;
    uint8_t* end1 = win[wave][0];
    uint8_t* end2 = win[wave][1];
    int wa = 0, wb = 0;
    bool valid = false;
    int64_t off_a = 0, off_b = 0;
    int32_t len_a = 0, len_b = 0;
    bool fwd_a = true, fwd_b = true;
    if (c < n) {
        const int64_t a = left[c], b = right[c];
        if (a >= 0 && a < n_contigs && b >= 0 && b < n_contigs) {
            off_a = ctg_off[a]; len_a = ctg_len[a];
            off_b = ctg_off[b]; len_b = ctg_len[b];
            valid = len_a >= 0 && len_b >= 0 && off_a >= 0 && off_b >= 0 && off_a + len_a <= pool_bytes &&
                    off_b + len_b <= pool_bytes;
        }
        if (valid) {
            const uint8_t f = forward[c];
            fwd_a = f & 1; fwd_b = f & 2;
            wa = len_a < K ? len_a : K;
            wb = len_b < K ? len_b : K;
        }
    }
    __syncthreads();                                             // the complement table is in LDS
    // end1[j] = oriented_left[len_a - wa + j], end2[j] = oriented_right[j]
    for (int j = lane; j < wa; j += 64)
        end1[j] = fwd_a ? pool[off_a + len_a - wa + j] : comp[pool[off_a + wa - 1 - j]];
    unsigned long long bad = ~0ull;
    for (int j = lane; j < wb; j += 64) {
        uint8_t v;
        if (fwd_b) {
            v = pool[off_b + j];
        } else {
            v = comp[pool[off_b + len_b - 1 - j]];
            if (v == 0 && bad == ~0ull) bad = ((unsigned long long)c << 32) | (unsigned)j;
        }
        end2[j] = v;
    }
    if (bad != ~0ull) atomicMin(err, bad);                       // (junction, oriented position): the lowest is the first
    __syncthreads();
    const int top = wa < wb ? wa : wb;
    int best = 0;
    for (int base = top; base > 0 && best == 0; base -= 64) {    // wave-uniform: `best` comes out of a ballot
        const int i = base - lane;                               // this lane's candidate length
        bool hit = false;
        if (i > 0) {
            const uint8_t* p = end1 + (wa - i);
            int j = 0;
            while (j < i && p[j] == end2[j]) ++j;
            hit = j == i;
        }
        const unsigned long long m = __ballot(hit);
        if (m) best = base - (__ffsll((long long)m) - 1);        // the lowest lane holds the longest
    }
    if (c < n && lane == 0) overlap[c] = valid ? best : -1;
}

// ---- the gather ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bytes_below(int n) {          // mask of the bytes 0..n-1 of a dword, any n
    return n <= 0 ? 0u : n >= 4 ? 0xffffffffu : (1u << (8 * n)) - 1u;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x4_aligned __attribute__((ext_vector_type(4), aligned(16)));

// 16 bytes from byte address p (any alignment) out of aligned dwords
__device__ __forceinline__ void load16(const uint8_t* p, uint32_t v[4]) {
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);   // (pointer arithmetic: the loads stay global loads)
    const u32x4 d = *reinterpret_cast<const u32x4*>(q);          // one 16-byte load at dword alignment + one dword
    const uint32_t d0 = d.x, d1 = d.y, d2 = d.z, d3 = d.w, d4 = q[4];
    v[0] = __builtin_amdgcn_alignbyte(d1, d0, sh);
    v[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
    v[2] = __builtin_amdgcn_alignbyte(d3, d2, sh);
    v[3] = __builtin_amdgcn_alignbyte(d4, d3, sh);
}

struct EmitTable {
    const uint8_t* pool;
    int64_t pool_bytes;
    const uint8_t* literals;
    int64_t literal_bytes;
    const int64_t* src_off;
    const int64_t* len;
    const uint8_t* mode;
    unsigned long long* err;
};

// The 16 bytes that piece q (output bytes [q_lo, q_hi)) supplies to the group that starts `rel` bytes into it
// (-15 .. len - 1); only the group's bytes [b0, b1) belong to the piece, the rest of v is over-read from the pads.
__device__ __forceinline__ void piece16(const EmitTable& t, const uint8_t* comp, int64_t q, int64_t q_lo, int64_t q_hi,
                                        int64_t rel, int b0, int b1, uint32_t v[4]) {
    const uint32_t m = t.mode[q];
    if (m == BESST_PIECE_FILL_N) {
        v[0] = v[1] = v[2] = v[3] = 0x4e4e4e4eu;
        return;
    }
    const int64_t s = t.src_off[q], l = t.len[q];
    const bool lit = m == BESST_PIECE_LITERAL;
    const int64_t room = lit ? t.literal_bytes : t.pool_bytes;
    if (m > BESST_PIECE_LITERAL || s < 0 || l != q_hi - q_lo || s + l > room) {      // a row that points outside
        atomicMin(t.err + 1, (unsigned long long)q);
        v[0] = v[1] = v[2] = v[3] = 0x3f3f3f3fu;
    } else if (m == BESST_PIECE_REVCOMP) {
        uint32_t u[4];
        load16(t.pool + (s + l - 1 - rel - 15), u);              // output byte j <- source byte s + l - 1 - (rel + j)
        int first_bad = 16;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t w = __builtin_amdgcn_perm(0u, u[3 - k], 0x00010203u);
            const uint32_t c0 = comp[w & 0xff], c1 = comp[(w >> 8) & 0xff], c2 = comp[(w >> 16) & 0xff], c3 = comp[w >> 24];
            v[k] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
            // a zero byte inside [b0,b1): no complement
            const uint32_t inside = bytes_below(b1 - 4 * k) & ~bytes_below(b0 - 4 * k);
            const uint32_t z = ((c0 ? 0u : 0xffu) | (c1 ? 0u : 0xff00u) | (c2 ? 0u : 0xff0000u) | (c3 ? 0u : 0xff000000u)) &
                               inside;
            if (z && first_bad == 16) first_bad = 4 * k + ((__ffs((int)z) - 1) >> 3);
        }
        if (first_bad < 16) atomicMin(t.err, ((unsigned long long)q << 32) | (unsigned long long)(rel + first_bad));
    } else {
        load16((lit ? t.literals : t.pool) + (s + rel), v);
    }
}

__global__ __launch_bounds__(kEmitThreads) void emit_kernel(EmitTable t, int64_t n_pieces, const int64_t* __restrict__ out_off,
                                                            int64_t begin, int64_t end, uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t comp[256];
    load_comp_table(comp);
    const int64_t tile = begin + (int64_t)blockIdx.x * kEmitTile;
    // the piece that holds the tile's first byte: the last p with out_off[p] <= tile (pieces of length 0 are passed over)
    int64_t lo = 0, hi = n_pieces;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (out_off[mid] <= tile) lo = mid; else hi = mid;
    }
    int64_t p = lo;                                              // the same in every lane of a wave from here on: in SGPRs
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    constexpr int kWaveBytes = 64 * 16;
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kEmitGroups; ++g) {
        const int64_t w0 = tile + ((int64_t)g * kEmitThreads + wave * 64) * 16;     // file offset of the wave's 1 KiB
        if (w0 >= end) break;
        while (p + 1 < n_pieces && out_off[p + 1] <= w0) ++p;
        const int64_t p_lo = out_off[p], p_hi = out_off[p + 1];
        const int64_t o = w0 + lane * 16;                        // file offset of this lane's group
        uint32_t r[4] = {0u, 0u, 0u, 0u};
        if (w0 + kWaveBytes <= end && p_hi >= w0 + kWaveBytes) {
            // the usual case: the wave's whole KiB lies in one piece - its row is read once, with scalar loads
            piece16(t, comp, p, p_lo, p_hi, o - p_lo, 0, 16, r);
            *reinterpret_cast<u32x4_aligned*>(out + (o - begin)) = u32x4_aligned{r[0], r[1], r[2], r[3]};
            continue;
        }
        if (o >= end) continue;
        const int64_t o_end = o + 16 < end ? o + 16 : end;
        int64_t q = p;
        while (q + 1 < n_pieces && out_off[q + 1] <= o) ++q;
        for (; q < n_pieces && out_off[q] < o_end; ++q) {        // one turn per piece that touches the group
            const int64_t q_lo = out_off[q], q_hi = out_off[q + 1];
            if (q_hi <= q_lo) continue;
            const int b0 = (int)((q_lo > o ? q_lo : o) - o), b1 = (int)((q_hi < o_end ? q_hi : o_end) - o);   // bytes [b0,b1)
            uint32_t v[4];
            piece16(t, comp, q, q_lo, q_hi, o - q_lo, b0, b1, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t inside = bytes_below(b1 - 4 * k) & ~bytes_below(b0 - 4 * k);
                r[k] = (r[k] & ~inside) | (v[k] & inside);
            }
        }
        uint8_t* dst = out + (o - begin);
        if (o_end - o == 16) {
            *reinterpret_cast<u32x4_aligned*>(dst) = u32x4_aligned{r[0], r[1], r[2], r[3]};
        } else {
            for (int j = 0; j < (int)(o_end - o); ++j) dst[j] = (uint8_t)(r[j >> 2] >> (8 * (j & 3)));
        }
    }
}

int check_emit_args(const void* pool, int64_t pool_bytes, const void* literals, int64_t literal_bytes, int64_t n_pieces,
                    const void* src_off, const void* len, const void* mode, const void* out_off, int64_t begin,
                    int64_t end, const void* out, const void* err) {
    BESST_REQUIRE(pool_bytes >= 0 && literal_bytes >= 0 && n_pieces >= 0 && n_pieces < ((int64_t)1 << 31),
                  "emit_scaffolds: size out of range");
    BESST_REQUIRE(begin >= 0 && begin <= end, "emit_scaffolds: bad output range");
    if (begin == end) return BESST_OK;
    BESST_REQUIRE(n_pieces > 0, "emit_scaffolds: output range past the end of an empty table");
    BESST_REQUIRE(pool && literals && src_off && len && mode && out_off && out && err, "emit_scaffolds: null pointer");
    return BESST_OK;
}

}  // namespace

}  // namespace besst

using namespace besst;

extern "C" {

const uint8_t* besst_host_complement_table(void) { return kCompHost.v; }

int besst_dev_seq_overlaps(void* stream, const uint8_t* pool, int64_t pool_bytes, int64_t n_contigs,
                           const int64_t* ctg_off, const int32_t* ctg_len, int64_t n, const int32_t* left,
                           const int32_t* right, const uint8_t* forward, int32_t max_overlap, int32_t* overlap,
                           uint64_t* err) {
    BESST_REQUIRE(max_overlap >= 0 && max_overlap <= kMaxK, "seq_overlaps: max_overlap outside 0..BESST_MAX_CONTIG_OVERLAP");
    BESST_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && n_contigs >= 0 && pool_bytes >= 0, "seq_overlaps: size out of range");
    if (n == 0) return BESST_OK;
    BESST_REQUIRE(pool && ctg_off && ctg_len && left && right && forward && overlap && err, "seq_overlaps: null pointer");
    const dim3 grid((uint32_t)((n + kOverlapWaves - 1) / kOverlapWaves)), block(kOverlapWaves * 64);
    hipLaunchKernelGGL(seq_overlap_kernel, grid, block, 0, static_cast<hipStream_t>(stream), pool, pool_bytes, n_contigs,
                       ctg_off, ctg_len, n, left, right, forward, max_overlap, overlap,
                       reinterpret_cast<unsigned long long*>(err));
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

int besst_dev_emit_scaffolds(void* stream, const uint8_t* pool, int64_t pool_bytes, const uint8_t* literals,
                             int64_t literal_bytes, int64_t n_pieces, const int64_t* src_off, const int64_t* len,
                             const uint8_t* mode, const int64_t* out_off, int64_t begin, int64_t end, uint8_t* out,
                             uint64_t* err) {
    const int rc = check_emit_args(pool, pool_bytes, literals, literal_bytes, n_pieces, src_off, len, mode, out_off, begin,
                                   end, out, err);
    if (rc != BESST_OK || begin == end) return rc;
    BESST_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "emit_scaffolds: out must be 16-byte aligned");
    BESST_REQUIRE((reinterpret_cast<uintptr_t>(pool) & 3) == 0 && (reinterpret_cast<uintptr_t>(literals) & 3) == 0,
                  "emit_scaffolds: pool and literals must be 4-byte aligned");
    const int64_t tiles = (end - begin + kEmitTile - 1) / kEmitTile;
    BESST_REQUIRE(tiles < ((int64_t)1 << 31), "emit_scaffolds: output range too long for one call");
    const EmitTable table{pool, pool_bytes, literals, literal_bytes, src_off, len, mode,
                          reinterpret_cast<unsigned long long*>(err)};
    hipLaunchKernelGGL(emit_kernel, dim3((uint32_t)tiles), dim3(kEmitThreads), 0, static_cast<hipStream_t>(stream), table,
                       n_pieces, out_off, begin, end, out);
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

}  // extern "C"

// ---- host-pointer twins: allocate, upload (with the pads), run, fetch ------------------------------------------------
namespace {

struct DeviceArena {                                             // one allocation, carved in 256-byte steps
    char* base = nullptr;
    size_t size = 0;
    size_t carve(size_t bytes) { const size_t o = size; size += align_up(bytes ? bytes : 1, 256); return o; }
    ~DeviceArena() { if (base) (void)hipFree(base); }
};

}  // namespace

extern "C" {

int besst_host_seq_overlaps(int device, const uint8_t* pool, int64_t pool_bytes, int64_t n_contigs, const int64_t* ctg_off,
                            const int32_t* ctg_len, int64_t n, const int32_t* left, const int32_t* right,
                            const uint8_t* forward, int32_t max_overlap, int32_t* overlap, uint64_t* err) {
    BESST_REQUIRE(max_overlap >= 0 && max_overlap <= kMaxK, "seq_overlaps: max_overlap outside 0..BESST_MAX_CONTIG_OVERLAP");
    BESST_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && n_contigs >= 0 && pool_bytes >= 0, "seq_overlaps: size out of range");
    BESST_REQUIRE(err, "seq_overlaps: null pointer");
    *err = ~(uint64_t)0;
    if (n == 0) return BESST_OK;
    BESST_REQUIRE((pool || pool_bytes == 0) && ctg_off && ctg_len && left && right && forward && overlap,
                  "seq_overlaps: null pointer");
    for (int64_t i = 0; i < n_contigs; ++i)
        BESST_REQUIRE(ctg_len[i] >= 0 && ctg_off[i] >= 0 && ctg_off[i] + ctg_len[i] <= pool_bytes,
                      "seq_overlaps: a contig lies outside the pool");
    for (int64_t i = 0; i < n; ++i)
        BESST_REQUIRE(left[i] >= 0 && left[i] < n_contigs && right[i] >= 0 && right[i] < n_contigs,
                      "seq_overlaps: contig index out of range");
    BESST_HIP_TRY(hipSetDevice(device));
    DeviceArena d;
    const size_t o_pool = d.carve((size_t)pool_bytes + 2 * BESST_EMIT_PAD), o_off = d.carve((size_t)n_contigs * 8),
                 o_len = d.carve((size_t)n_contigs * 4), o_l = d.carve((size_t)n * 4), o_r = d.carve((size_t)n * 4),
                 o_f = d.carve((size_t)n), o_ov = d.carve((size_t)n * 4), o_err = d.carve(8);
    BESST_HIP_TRY(hipMalloc(&d.base, d.size));
    BESST_HIP_TRY(hipMemset(d.base, 0, d.size));
    if (pool_bytes) BESST_HIP_TRY(hipMemcpy(d.base + o_pool + BESST_EMIT_PAD, pool, (size_t)pool_bytes, hipMemcpyHostToDevice));
    if (n_contigs) {
        BESST_HIP_TRY(hipMemcpy(d.base + o_off, ctg_off, (size_t)n_contigs * 8, hipMemcpyHostToDevice));
        BESST_HIP_TRY(hipMemcpy(d.base + o_len, ctg_len, (size_t)n_contigs * 4, hipMemcpyHostToDevice));
    }
    BESST_HIP_TRY(hipMemcpy(d.base + o_l, left, (size_t)n * 4, hipMemcpyHostToDevice));
    BESST_HIP_TRY(hipMemcpy(d.base + o_r, right, (size_t)n * 4, hipMemcpyHostToDevice));
    BESST_HIP_TRY(hipMemcpy(d.base + o_f, forward, (size_t)n, hipMemcpyHostToDevice));
    BESST_HIP_TRY(hipMemset(d.base + o_err, 0xff, 8));
    const int rc = besst_dev_seq_overlaps(nullptr, (const uint8_t*)(d.base + o_pool + BESST_EMIT_PAD), pool_bytes, n_contigs,
                                          (const int64_t*)(d.base + o_off), (const int32_t*)(d.base + o_len), n,
                                          (const int32_t*)(d.base + o_l), (const int32_t*)(d.base + o_r),
                                          (const uint8_t*)(d.base + o_f), max_overlap, (int32_t*)(d.base + o_ov),
                                          (uint64_t*)(d.base + o_err));
    if (rc != BESST_OK) return rc;
    BESST_HIP_TRY(hipMemcpy(overlap, d.base + o_ov, (size_t)n * 4, hipMemcpyDeviceToHost));
    BESST_HIP_TRY(hipMemcpy(err, d.base + o_err, 8, hipMemcpyDeviceToHost));
    return BESST_OK;
}

int besst_host_emit_scaffolds(int device, const uint8_t* pool, int64_t pool_bytes, const uint8_t* literals,
                              int64_t literal_bytes, int64_t n_pieces, const int64_t* src_off, const int64_t* len,
                              const uint8_t* mode, const int64_t* out_off, int64_t begin, int64_t end, uint8_t* out,
                              uint64_t* err) {
    BESST_REQUIRE(err, "emit_scaffolds: null pointer");
    err[0] = err[1] = ~(uint64_t)0;
    static const uint8_t nothing[4] = {0, 0, 0, 0};
    if (!pool && pool_bytes == 0) pool = nothing;
    if (!literals && literal_bytes == 0) literals = nothing;
    const int rc0 = check_emit_args(pool, pool_bytes, literals, literal_bytes, n_pieces, src_off, len, mode, out_off, begin,
                                    end, out, err);
    if (rc0 != BESST_OK || begin == end) return rc0;
    BESST_REQUIRE(out_off[0] == 0 && end <= out_off[n_pieces], "emit_scaffolds: output range past the end of the table");
    for (int64_t i = 0; i < n_pieces; ++i) {
        BESST_REQUIRE(len[i] >= 0 && out_off[i + 1] - out_off[i] == len[i], "emit_scaffolds: out_off is not the prefix sum of len");
        BESST_REQUIRE(mode[i] <= BESST_PIECE_LITERAL, "emit_scaffolds: unknown piece mode");
        if (mode[i] != BESST_PIECE_FILL_N)
            BESST_REQUIRE(src_off[i] >= 0 && src_off[i] + len[i] <= (mode[i] == BESST_PIECE_LITERAL ? literal_bytes : pool_bytes),
                          "emit_scaffolds: a piece lies outside its pool");
    }
    BESST_HIP_TRY(hipSetDevice(device));
    DeviceArena d;
    const size_t n_out = (size_t)(end - begin);
    const size_t o_pool = d.carve((size_t)pool_bytes + 2 * BESST_EMIT_PAD),
                 o_lit = d.carve((size_t)literal_bytes + 2 * BESST_EMIT_PAD), o_src = d.carve((size_t)n_pieces * 8),
                 o_len = d.carve((size_t)n_pieces * 8), o_mode = d.carve((size_t)n_pieces),
                 o_off = d.carve((size_t)(n_pieces + 1) * 8), o_out = d.carve(n_out), o_err = d.carve(16);
    BESST_HIP_TRY(hipMalloc(&d.base, d.size));
    BESST_HIP_TRY(hipMemset(d.base, 0, o_src));                  // the pads
    if (pool_bytes) BESST_HIP_TRY(hipMemcpy(d.base + o_pool + BESST_EMIT_PAD, pool, (size_t)pool_bytes, hipMemcpyHostToDevice));
    if (literal_bytes)
        BESST_HIP_TRY(hipMemcpy(d.base + o_lit + BESST_EMIT_PAD, literals, (size_t)literal_bytes, hipMemcpyHostToDevice));
    BESST_HIP_TRY(hipMemcpy(d.base + o_src, src_off, (size_t)n_pieces * 8, hipMemcpyHostToDevice));
    BESST_HIP_TRY(hipMemcpy(d.base + o_len, len, (size_t)n_pieces * 8, hipMemcpyHostToDevice));
    BESST_HIP_TRY(hipMemcpy(d.base + o_mode, mode, (size_t)n_pieces, hipMemcpyHostToDevice));
    BESST_HIP_TRY(hipMemcpy(d.base + o_off, out_off, (size_t)(n_pieces + 1) * 8, hipMemcpyHostToDevice));
    BESST_HIP_TRY(hipMemset(d.base + o_err, 0xff, 16));
    const int rc = besst_dev_emit_scaffolds(nullptr, (const uint8_t*)(d.base + o_pool + BESST_EMIT_PAD), pool_bytes,
                                            (const uint8_t*)(d.base + o_lit + BESST_EMIT_PAD), literal_bytes, n_pieces,
                                            (const int64_t*)(d.base + o_src), (const int64_t*)(d.base + o_len),
                                            (const uint8_t*)(d.base + o_mode), (const int64_t*)(d.base + o_off), begin, end,
                                            (uint8_t*)(d.base + o_out), (uint64_t*)(d.base + o_err));
    if (rc != BESST_OK) return rc;
    BESST_HIP_TRY(hipMemcpy(out, d.base + o_out, n_out, hipMemcpyDeviceToHost));
    BESST_HIP_TRY(hipMemcpy(err, d.base + o_err, 16, hipMemcpyDeviceToHost));
    return BESST_OK;
}

}  // extern "C"
