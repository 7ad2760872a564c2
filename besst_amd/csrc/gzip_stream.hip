// A plain gzip member (one DEFLATE stream, gzip's own output) inflated on the GPU: the scheme of pugz.  A DEFLATE stream
// has no index, but a block start can be FOUND, a chunk can be decoded against a window nobody knows yet, and the windows
// can be resolved afterwards (the steps that are sequential by nature are in gzip_stream_core.h,
// which the host compiles too).  The compressed file lies in device memory; bit positions count from its first byte.
//   gz_probe_kernel      a thread per byte, its eight bit positions: the first position of every chunk that passes zlib's checks of a dynamic
//                        block header is the chunk's CANDIDATE (atomic minimum per chunk); chunk 0 starts at the first bit
//   gz_count_kernel      a wave per chunk with a start: block after block, lengths only, until BFINAL or a block end that is
//                        the candidate of the chunk it lies in (the landing); bytes made, as a 64-bit count
//   gz_link_kernel       one thread: the landings followed from chunk 0 (the live chunks), their places in the text, ISIZE
//   -- the host reads the text's size here and allocates it --
//   gz_decode_kernel     a wave per live chunk: the same walk, now into one 16-bit symbol per byte at the chunk's place - a
//                        literal, or "byte k of the 32 KiB in front of this chunk"; a match inside the chunk copies symbols
//   gz_windows_kernel    one workgroup, live chunk after live chunk: the last 32 KiB of each resolved against the text in
//                        front of it (what a chunk shorter than that leaves open is its predecessors' and already there)
//   gz_translate_kernel  everything else, in parallel: the sources now all lie in resolved text
//   gz_crc_*             CRC-32 of the text: slices of 1 KiB, groups of 64 slices, one fold, against the trailer
// The decode is wave-uniform: one symbol per turn for the whole wave, the lanes share the table build and the copies.
// A file of SEVERAL members (besst_dev_gzip_members_*): member starts are found and walked the same way, and the chain
// passes from member to member; those kernels stand behind the ones above, which they share.
#include <stdint.h>

#include "bgzf_crc.h"
#include "common.h"
#include "gzip_stream_core.h"

namespace besst {

namespace {

enum : int { kInfoStatus = 0, kInfoText, kInfoChunks, kInfoCandidates, kInfoLive, kInfoEndBit, kInfoBadChunk, kInfoCrc };
constexpr uint32_t kCrcSlice = 1024, kCrcGroup = 64;
constexpr int kTranslateSplit = 8;

// where the parts of the plan's workspace lie (n = chunks)
struct PlanWs {
    uint32_t *cand_rel, *status, *final_block, *live_idx;
    uint64_t *land, *out_bytes, *live_off;
    size_t bytes;
};
PlanWs plan_layout(void* ws, size_t n) {
    PlanWs p;
    char* at = static_cast<char*>(ws);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* r = at + off; off += align_up(bytes, 256); return r; };
    p.cand_rel = reinterpret_cast<uint32_t*>(take(n * 4));
    p.status = reinterpret_cast<uint32_t*>(take(n * 4));
    p.final_block = reinterpret_cast<uint32_t*>(take(n * 4));
    p.live_idx = reinterpret_cast<uint32_t*>(take(n * 4));
    p.land = reinterpret_cast<uint64_t*>(take(n * 8));
    p.out_bytes = reinterpret_cast<uint64_t*>(take(n * 8));
    p.live_off = reinterpret_cast<uint64_t*>(take(n * 8));
    p.bytes = off;
    return p;
}
struct InflateWs {
    uint16_t* sym;
    uint32_t *status, *crc_slice, *crc_group;
    size_t bytes;
};
size_t crc_slices(size_t text_bytes) { return (text_bytes + kCrcSlice - 1) / kCrcSlice; }
size_t crc_groups(size_t text_bytes) { return (crc_slices(text_bytes) + kCrcGroup - 1) / kCrcGroup; }
InflateWs inflate_layout(void* ws, size_t text_bytes, size_t n_live) {
    InflateWs p;
    char* at = static_cast<char*>(ws);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* r = at + off; off += align_up(bytes + 1, 256); return r; };
    p.sym = reinterpret_cast<uint16_t*>(take(text_bytes * 2));
    p.status = reinterpret_cast<uint32_t*>(take(n_live * 4));
    p.crc_slice = reinterpret_cast<uint32_t*>(take(crc_slices(text_bytes) * 4));
    p.crc_group = reinterpret_cast<uint32_t*>(take(crc_groups(text_bytes) * 4));
    p.bytes = off;
    return p;
}

// the wave's view of the input: 64 dwords of the file from word `wbase` on, a dword per lane; the position is uniform
struct WaveCtx {
    const uint32_t* words;
    const uint8_t* bytes;
    uint64_t last_word;              // the last dword that holds a byte of the file: nothing behind it is read
    uint64_t wbase, bit;
    uint32_t win;
    uint32_t lane;
    static constexpr uint32_t nlanes = 64;
    uint16_t* sym;                   // the chunk's first symbol (the decode)

    __device__ __forceinline__ void refill() {
        wbase = bit >> 5;
        const uint64_t w = wbase + lane;
        win = words[w < last_word ? w : last_word];
    }
    __device__ __forceinline__ void seek(uint64_t b) { bit = b; refill(); }
    __device__ __forceinline__ uint64_t pos() const { return bit; }
    __device__ __forceinline__ uint32_t peek() const {
        const int i = __builtin_amdgcn_readfirstlane((int)((bit >> 5) - wbase));     // <= 62
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)win, i);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)win, i + 1);
        return (uint32_t)((((uint64_t)hi << 32) | lo) >> (bit & 31u));
    }
    __device__ __forceinline__ void drop(uint32_t n) {
        bit += n;
        if ((bit >> 5) - wbase >= 63u) refill();
    }
    __device__ __forceinline__ uint32_t byte(uint64_t i) const { return bytes[i]; }
    __device__ __forceinline__ void barrier() const { __syncthreads(); }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    // (a wave's vector memory instructions are processed in order; the loads skip the CU's L1, as bgzf_inflate_kernel's do)
    __device__ __forceinline__ void store(uint64_t i, uint32_t v) const {
        __hip_atomic_store(sym + i, (uint16_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ uint32_t load(uint64_t i) const {
        return __hip_atomic_load(sym + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

__global__ __launch_bounds__(256) void gz_init_kernel(uint32_t* __restrict__ cand_rel, uint64_t n_chunks, unsigned long long* info) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n_chunks) cand_rel[i] = i == 0u ? 0u : gz::kNoCandidate;
    if (i < 8u) info[i] = i == (uint64_t)kInfoChunks ? n_chunks : 0ull;
}

// A thread per BYTE of the data: its eight bit positions share three loaded bytes, and the three checks that need no more than
// those (BTYPE, HLIT, HDIST: four positions in five fail them) are made on that word; what passes goes through
// gz::probe_dynamic_header, which reads for itself.  (A thread per bit position, every one loading its own bytes: 164 ms for
// the 412 MB file; this form: DESIGN.md section 11.2.)
__global__ __launch_bounds__(256) void gz_probe_kernel(const uint8_t* __restrict__ comp, uint64_t comp_bytes, uint64_t data_bit0,
                                                       uint64_t end_bit, uint64_t chunk_bits, uint64_t n_chunks, uint32_t* cand_rel) {
    const uint64_t byte = ((data_bit0 + chunk_bits) >> 3) + (uint64_t)blockIdx.x * 256u + threadIdx.x;   // (chunks begin at bytes)
    const uint64_t bit0 = byte * 8u;
    if (bit0 >= end_bit) return;
    const uint64_t j = (bit0 - data_bit0) / chunk_bits;
    if (j >= n_chunks) return;
    const uint32_t rel = (uint32_t)(bit0 - data_bit0 - j * chunk_bits);
    if (cand_rel[j] < rel) return;                           // (an earlier position of the chunk already is a candidate)
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k)
        if (byte + k < comp_bytes) v |= (uint32_t)comp[byte + k] << (8u * k);
    const gz::ByteBits in = {comp, comp_bytes};
    for (uint32_t k = 0; k < 8u; ++k) {
        const uint32_t x = v >> k;
        if (((x >> 1) & 3u) != 2u || ((x >> 3) & 31u) > 29u || ((x >> 8) & 31u) > 29u) continue;
        if (gz::probe_dynamic_header(in, bit0 + k, end_bit)) {
            atomicMin(&cand_rel[j], rel + k);
            break;                                           // (the byte's later positions are no minimum)
        }
    }
}

__device__ __forceinline__ WaveCtx wave_ctx(const uint8_t* comp, uint64_t comp_bytes) {
    WaveCtx c;
    c.words = reinterpret_cast<const uint32_t*>(comp);
    c.bytes = comp;
    c.last_word = (comp_bytes - 1u) >> 2;
    c.lane = threadIdx.x;
    c.sym = nullptr;
    c.wbase = c.bit = 0;
    c.win = 0;
    return c;
}

__global__ __launch_bounds__(64) void gz_count_kernel(const uint8_t* __restrict__ comp, uint64_t comp_bytes, uint64_t data_bit0,
                                                      uint64_t end_bit, uint64_t chunk_bits, uint64_t n_chunks,
                                                      const uint32_t* __restrict__ cand_rel, uint64_t* __restrict__ land,
                                                      uint64_t* __restrict__ out_bytes, uint32_t* __restrict__ final_block,
                                                      uint32_t* __restrict__ status, unsigned long long* info) {
    __shared__ gz::WalkTables t;
    const uint64_t j = blockIdx.x;
    if (j >= n_chunks) return;
    const uint32_t rel = cand_rel[j];
    if (rel == gz::kNoCandidate) return;                     // uniform
    WaveCtx c = wave_ctx(comp, comp_bytes);
    gz::WalkArgs a = {};
    a.start_bit = data_bit0 + j * chunk_bits + rel;
    a.end_bit = end_bit;
    a.cand_rel = cand_rel;
    a.n_chunks = n_chunks;
    a.data_bit0 = data_bit0;
    a.chunk_bits = chunk_bits;
    const gz::WalkResult r = gz::walk_chunk<false>(c, t, a);
    if (threadIdx.x == 0u) {
        land[j] = r.land_bit;
        out_bytes[j] = r.out_bytes;
        final_block[j] = r.final_block;
        status[j] = r.status;
        if (j) atomicAdd(&info[kInfoCandidates], 1ull);
    }
}

__device__ __forceinline__ uint32_t le32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__global__ void gz_link_kernel(const uint8_t* __restrict__ comp, uint64_t comp_bytes, uint64_t data_bit0, uint64_t chunk_bits,
                               uint64_t n_chunks, const uint64_t* __restrict__ land, const uint64_t* __restrict__ out_bytes,
                               const uint32_t* __restrict__ final_block, const uint32_t* __restrict__ status, uint32_t* live_idx,
                               uint64_t* live_off, unsigned long long* info) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    uint64_t text = 0, n_live = 0, end_bit = 0;
    uint32_t st = gz::link_chain(land, out_bytes, final_block, status, n_chunks, data_bit0, chunk_bits, live_idx, live_off, &text,
                                 &n_live, &end_bit);
    if (st == gz::kOk) {
        const uint64_t trailer = (end_bit + 7u) >> 3;        // (the walk ends in front of the room kept for the trailer)
        if (trailer + 8u != comp_bytes) st = gz::kTrailingBytes;             // another member, or bytes that are none
        else if (le32(comp + trailer + 4u) != (uint32_t)text) st = gz::kBadSize;
    }
    info[kInfoStatus] = st;
    info[kInfoText] = text;
    info[kInfoLive] = n_live;
    info[kInfoEndBit] = end_bit;
    info[kInfoBadChunk] = st ? live_idx[n_live - 1u] : 0u;
}

__global__ __launch_bounds__(64) void gz_decode_kernel(const uint8_t* __restrict__ comp, uint64_t comp_bytes, uint64_t data_bit0,
                                                       uint64_t end_bit, uint64_t chunk_bits, const uint32_t* __restrict__ cand_rel,
                                                       const uint64_t* __restrict__ land, const uint64_t* __restrict__ out_bytes,
                                                       const uint32_t* __restrict__ live_idx, const uint64_t* __restrict__ live_off,
                                                       uint64_t n_live, uint64_t text_bytes, uint16_t* sym, uint32_t* __restrict__ status,
                                                       const unsigned long long* __restrict__ info) {
    __shared__ gz::WalkTables t;
    const uint64_t i = blockIdx.x;
    if (i >= n_live || info[kInfoStatus] != 0ull) return;
    const uint64_t j = live_idx[i];
    WaveCtx c = wave_ctx(comp, comp_bytes);
    gz::WalkArgs a = {};
    a.start_bit = data_bit0 + j * chunk_bits + cand_rel[j];
    a.end_bit = end_bit;
    a.stop_bit = land[j];
    a.out_cap = out_bytes[j];
    a.text_off = live_off[i];
    uint32_t st = gz::kOutputOverrun;
    if (a.text_off <= text_bytes && a.out_cap <= text_bytes - a.text_off) {      // (the chunk's symbols lie inside the buffer)
        c.sym = sym + a.text_off;
        st = gz::walk_chunk<true>(c, t, a).status;
    }
    if (threadIdx.x == 0u) status[i] = st;
}

// One workgroup.  First the decode's statuses (the first bad live chunk ends the member), then live chunk after live chunk:
// the last 32 KiB of its symbols become text.  Their markers point into the 32 KiB in front of the chunk, which earlier
// turns of this loop wrote: a chunk of 32 KiB or more wrote all of the window behind it, a shorter one its own bytes - the
// rest of that window is the window it had itself.  The text is the window: no copy of it is kept.
__global__ __launch_bounds__(1024) void gz_windows_kernel(const uint16_t* __restrict__ sym, const uint64_t* __restrict__ out_bytes,
                                                          const uint32_t* __restrict__ live_idx, const uint64_t* __restrict__ live_off,
                                                          const uint32_t* __restrict__ status, uint64_t n_live, uint8_t* text,
                                                          unsigned long long* info) {
    __shared__ unsigned long long s_bad;
    if (info[kInfoStatus] != 0ull) return;
    if (threadIdx.x == 0u) s_bad = ~0ull;
    __syncthreads();
    for (uint64_t i = threadIdx.x; i < n_live; i += 1024u)
        if (status[i]) atomicMin(&s_bad, (i << 8) | status[i]);
    __syncthreads();
    if (s_bad != ~0ull) {                                    // uniform
        if (threadIdx.x == 0u) {
            info[kInfoStatus] = s_bad & 0xffu;
            info[kInfoBadChunk] = live_idx[s_bad >> 8];
        }
        return;
    }
    // A turn's loads all stand in front of its stores (they read in front of the chunk, the stores write inside it): three
    // round trips to memory per chunk - symbols, window bytes, stores - not one per byte of a thread; the next chunk's place
    // is fetched while this one is resolved.  (One byte after the other, 32 per thread: 24 us per chunk, 149 ms for 6283.)
    constexpr int kPerThread = (int)(gz::kWindow / 1024u);
    uint64_t off = live_off[0], n = out_bytes[live_idx[0]];
    for (uint64_t i = 0; i < n_live; ++i) {
        uint64_t next_off = 0, next_n = 0;
        if (i + 1u < n_live) {
            next_off = live_off[i + 1u];
            next_n = out_bytes[live_idx[i + 1u]];
        }
        const uint64_t tail = n < gz::kWindow ? n : gz::kWindow;
        const uint64_t first = off + n - tail;
        uint32_t v[kPerThread];
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const uint64_t p = (uint64_t)k * 1024u + threadIdx.x;
            v[k] = p < tail ? sym[first + p] : 0u;
        }
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) v[k] = gz::resolve_symbol(v[k], text + off);
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const uint64_t p = (uint64_t)k * 1024u + threadIdx.x;
            if (p < tail) text[first + p] = (uint8_t)v[k];
        }
        __syncthreads();                                     // (the next chunk reads these bytes)
        off = next_off;
        n = next_n;
    }
}

__global__ __launch_bounds__(256) void gz_translate_kernel(const uint16_t* __restrict__ sym, const uint64_t* __restrict__ out_bytes,
                                                           const uint32_t* __restrict__ live_idx, const uint64_t* __restrict__ live_off,
                                                           uint64_t n_live, uint8_t* text, const unsigned long long* __restrict__ info) {
    const uint64_t i = blockIdx.x;
    if (i >= n_live || info[kInfoStatus] != 0ull) return;
    const uint64_t off = live_off[i], n = out_bytes[live_idx[i]];
    const uint64_t head = n > gz::kWindow ? n - gz::kWindow : 0u;
    for (uint64_t p = (uint64_t)blockIdx.y * 256u + threadIdx.x; p < head; p += (uint64_t)gridDim.y * 256u)
        text[off + p] = (uint8_t)gz::resolve_symbol(sym[off + p], text + off);
}

// CRC-32 of the text: a thread per slice of 1 KiB (aligned 16-byte words; the last slice's odd bytes one by one) ...
__global__ __launch_bounds__(256) void gz_crc_slice_kernel(const uint8_t* __restrict__ text, uint64_t text_bytes, uint32_t* __restrict__ crc_slice,
                                                           const unsigned long long* __restrict__ info) {
    __shared__ uint32_t s_tab[4][256];
    if (info[kInfoStatus] != 0ull) return;
    crc_fill_tables(s_tab, threadIdx.x);
    __syncthreads();
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t lo = s * kCrcSlice;
    if (lo >= text_bytes) return;
    const uint32_t len = text_bytes - lo < kCrcSlice ? (uint32_t)(text_bytes - lo) : kCrcSlice;
    const uint4* src = reinterpret_cast<const uint4*>(text + lo);
    uint32_t crc = 0xffffffffu;
    uint32_t q = 0;
    for (; (q + 1u) * 16u <= len; ++q) {
        const uint4 w = src[q];
        crc = crc_dword(s_tab, crc, w.x);
        crc = crc_dword(s_tab, crc, w.y);
        crc = crc_dword(s_tab, crc, w.z);
        crc = crc_dword(s_tab, crc, w.w);
    }
    for (uint32_t k = q * 16u; k < len; ++k) crc = crc_byte(s_tab, crc, text[lo + k]);
    crc_slice[s] = ~crc;
}
// ... the slices of a group folded as zlib's crc32_combine does - crc(A B) = crc(A) x^(8 |B|) + crc(B) -, a thread per group ...
__global__ __launch_bounds__(256) void gz_crc_group_kernel(const uint32_t* __restrict__ crc_slice, uint64_t text_bytes,
                                                           uint32_t* __restrict__ crc_group, const unsigned long long* __restrict__ info) {
    if (info[kInfoStatus] != 0ull) return;
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t n_slices = (text_bytes + kCrcSlice - 1u) / kCrcSlice;
    const uint64_t lo = g * kCrcGroup;
    if (lo >= n_slices) return;
    const uint64_t hi = lo + kCrcGroup < n_slices ? lo + kCrcGroup : n_slices;
    const uint32_t whole = crc_x8n(kCrcSlice);
    uint32_t acc = 0;
    for (uint64_t s = lo; s < hi; ++s) {
        const uint64_t bytes = s + 1u == n_slices ? text_bytes - s * kCrcSlice : (uint64_t)kCrcSlice;
        acc = crc_mul_lanes(acc, bytes == kCrcSlice ? whole : crc_x8n((uint32_t)bytes)) ^ crc_slice[s];
    }
    crc_group[g] = acc;
}
// ... and the groups by one thread, against the trailer
__global__ void gz_crc_check_kernel(const uint8_t* __restrict__ comp, const uint32_t* __restrict__ crc_group, uint64_t text_bytes,
                                    unsigned long long* info) {
    if (blockIdx.x != 0u || threadIdx.x != 0u || info[kInfoStatus] != 0ull) return;
    const uint64_t group_bytes = (uint64_t)kCrcSlice * kCrcGroup;
    const uint64_t n_groups = (text_bytes + group_bytes - 1u) / group_bytes;
    const uint32_t whole = crc_x8n((uint32_t)group_bytes);
    uint32_t acc = 0;
    for (uint64_t g = 0; g < n_groups; ++g) {
        const uint64_t bytes = g + 1u == n_groups ? text_bytes - g * group_bytes : group_bytes;
        acc = crc_mul_lanes(acc, bytes == group_bytes ? whole : crc_x8n((uint32_t)bytes)) ^ crc_group[g];
    }
    info[kInfoCrc] = acc;
    const uint64_t trailer = (info[kInfoEndBit] + 7u) >> 3;
    if (acc != le32(comp + trailer)) info[kInfoStatus] = gz::kBadCrc;
}

bool plan_geometry(int64_t comp_bytes, int64_t data_off, int64_t chunk_bytes, uint64_t* n_chunks) {
    if (chunk_bytes < 256 || chunk_bytes > ((int64_t)1 << 24) || (chunk_bytes & 15) != 0) return false;
    if (data_off < 0 || comp_bytes < data_off + 8 || comp_bytes > ((int64_t)1 << 35)) return false;
    const uint64_t data = (uint64_t)(comp_bytes - data_off - 8);
    const uint64_t n = (data + (uint64_t)chunk_bytes - 1u) / (uint64_t)chunk_bytes;
    *n_chunks = n ? n : 1u;
    return *n_chunks <= 0x7fffffffull;
}

// ---- a file of several members (besst_dev_gzip_members_*) -------------------------------------------------------------------
// The probe, the chunks' count, the windows and the translation above serve this path as they are; what is its own:
//   gz_member_mark_kernel    a thread per 16 bytes: every offset behind the first that reads like a member's start joins
//                            the candidate list and the chain of its 4 KiB bucket
//   gz_member_count_kernel   a wave per member candidate: the header parsed, then the same count from its first block
//   gz_member_link_kernel    one thread: gz::link_members - segments (walks of chunks and of members), and the member table
//   gz_segment_decode_kernel a wave per live segment; a match reaches its member's first byte and not one further
//   gz_member_crc_*          the 1 KiB slice grid restarts at every member: slices, groups, a thread per member's fold
enum : int { kInfoMembers = 8, kInfoMemberCandidates, kInfoBadMember, kInfoBadMemberOffset, kMemberInfoWords = 16 };
constexpr unsigned kMemberCountBlocks = 2048;

struct MemberPlanWs {
    uint32_t *cand_rel, *status, *final_block, *live_idx, *m_next, *m_head;
    uint64_t *land, *out_bytes, *live_off, *live_mem, *m_off, *m_start;
    gz::MemberRow* rows;
    size_t n_buckets, bytes;
};
// n chunks, cap member candidates: n + cap walks and as many segments at most, cap + 1 members
MemberPlanWs member_plan_layout(void* ws, size_t n, size_t cap, size_t comp_bytes) {
    MemberPlanWs p;
    char* at = static_cast<char*>(ws);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* r = at + off; off += align_up(bytes + 1, 256); return r; };
    const size_t walks = n + cap;
    p.n_buckets = comp_bytes / gz::kMemberBucketBytes + 1;
    p.cand_rel = reinterpret_cast<uint32_t*>(take(n * 4));
    p.status = reinterpret_cast<uint32_t*>(take(walks * 4));
    p.final_block = reinterpret_cast<uint32_t*>(take(walks * 4));
    p.live_idx = reinterpret_cast<uint32_t*>(take(walks * 4));
    p.m_next = reinterpret_cast<uint32_t*>(take(cap * 4));
    p.m_head = reinterpret_cast<uint32_t*>(take(p.n_buckets * 4));
    p.land = reinterpret_cast<uint64_t*>(take(walks * 8));
    p.out_bytes = reinterpret_cast<uint64_t*>(take(walks * 8));
    p.live_off = reinterpret_cast<uint64_t*>(take(walks * 8));
    p.live_mem = reinterpret_cast<uint64_t*>(take(walks * 8));
    p.m_off = reinterpret_cast<uint64_t*>(take(cap * 8));
    p.m_start = reinterpret_cast<uint64_t*>(take(cap * 8));
    p.rows = reinterpret_cast<gz::MemberRow*>(take((cap + 1) * sizeof(gz::MemberRow)));
    p.bytes = off;
    return p;
}
struct MemberInflateWs {
    uint16_t* sym;
    uint32_t *status, *crc_slice, *crc_group;
    size_t slices, groups, bytes;
};
// (a member's last slice and last group may be short: one more of each per member than the text alone would need)
MemberInflateWs member_inflate_layout(void* ws, size_t text_bytes, size_t n_live, size_t n_members) {
    MemberInflateWs p;
    char* at = static_cast<char*>(ws);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* r = at + off; off += align_up(bytes + 1, 256); return r; };
    p.slices = text_bytes / kCrcSlice + n_members;
    p.groups = text_bytes / ((size_t)kCrcSlice * kCrcGroup) + n_members;
    p.sym = reinterpret_cast<uint16_t*>(take(text_bytes * 2));
    p.status = reinterpret_cast<uint32_t*>(take(n_live * 4));
    p.crc_slice = reinterpret_cast<uint32_t*>(take(p.slices * 4));
    p.crc_group = reinterpret_cast<uint32_t*>(take(p.groups * 4));
    p.bytes = off;
    return p;
}

__global__ __launch_bounds__(256) void gz_member_init_kernel(uint32_t* __restrict__ cand_rel, uint64_t n_chunks, uint32_t* __restrict__ m_head,
                                                             uint64_t n_buckets, unsigned long long* info) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n_chunks) cand_rel[i] = i == 0u ? 0u : gz::kNoCandidate;
    if (i < n_buckets) m_head[i] = gz::kNoCandidate;
    if (i < (uint64_t)kMemberInfoWords)
        info[i] = i == (uint64_t)kInfoChunks ? n_chunks : i == (uint64_t)kInfoBadMember ? ~0ull : 0ull;
}

// A thread per 16 bytes of the file: five dwords (none behind the one that holds the file's last byte), the sixteen offsets'
// four bytes each shifted out of them.  A candidate is rare (a few per file that are none; the members themselves).
__global__ __launch_bounds__(256) void gz_member_mark_kernel(const uint32_t* __restrict__ words, uint64_t comp_bytes, uint64_t cap,
                                                             uint64_t* __restrict__ m_off, uint32_t* __restrict__ m_next, uint32_t* m_head,
                                                             unsigned long long* info) {
    const uint64_t base = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 16u;
    if (base + 4u > comp_bytes) return;
    const uint64_t last_word = (comp_bytes - 1u) >> 2;
    uint32_t v[5];
#pragma unroll
    for (uint32_t k = 0; k < 5u; ++k) {
        const uint64_t w = (base >> 2) + k;
        v[k] = words[w < last_word ? w : last_word];
    }
#pragma unroll
    for (uint32_t k = 0; k < 16u; ++k) {
        const uint64_t at = base + k;
        const uint32_t x = (uint32_t)((((uint64_t)v[(k >> 2) + 1u] << 32) | v[k >> 2]) >> (8u * (k & 3u)));
        if (at == 0u || at + 4u > comp_bytes || !gz::member_magic(x)) continue;      // (all four bytes lie inside the file)
        const unsigned long long slot = atomicAdd(&info[kInfoMemberCandidates], 1ull);
        if (slot < cap) {
            m_off[slot] = at;
            m_next[slot] = atomicExch(&m_head[at / gz::kMemberBucketBytes], (uint32_t)slot);
        }
    }
}

// A wave per member candidate (a fixed grid walks the list): every lane parses the header (the same bytes), then the count
// from the member's first block as gz_count_kernel makes it from a chunk's candidate.  More candidates than the list
// holds: nothing is walked, the link says so.
__global__ __launch_bounds__(64) void gz_member_count_kernel(const uint8_t* __restrict__ comp, uint64_t comp_bytes, uint64_t data_bit0,
                                                             uint64_t end_bit, uint64_t chunk_bits, uint64_t n_chunks, uint64_t cap,
                                                             const uint32_t* __restrict__ cand_rel, const uint64_t* __restrict__ m_off,
                                                             uint64_t* __restrict__ m_start, uint64_t* __restrict__ land,
                                                             uint64_t* __restrict__ out_bytes, uint32_t* __restrict__ final_block,
                                                             uint32_t* __restrict__ status, const unsigned long long* info) {
    __shared__ gz::WalkTables t;
    const uint64_t count = info[kInfoMemberCandidates];
    if (count > cap) return;
    for (uint64_t i = blockIdx.x; i < count; i += gridDim.x) {
        const uint64_t parsed = gz::member_data_offset(comp, comp_bytes, m_off[i]);
        const uint64_t data = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(parsed >> 32)) << 32) |
                              (uint32_t)__builtin_amdgcn_readfirstlane((int)parsed);
        gz::WalkResult r = {0, 0, 0, gz::kInputOverrun};
        if (data != gz::kNoMember) {                             // uniform
            WaveCtx c = wave_ctx(comp, comp_bytes);
            gz::WalkArgs a = {};
            a.start_bit = data * 8u;
            a.end_bit = end_bit;
            a.cand_rel = cand_rel;
            a.n_chunks = n_chunks;
            a.data_bit0 = data_bit0;
            a.chunk_bits = chunk_bits;
            r = gz::walk_chunk<false>(c, t, a);
        }
        if (threadIdx.x == 0u) {
            m_start[i] = data == gz::kNoMember ? gz::kNoMember : data * 8u;
            land[n_chunks + i] = r.land_bit;
            out_bytes[n_chunks + i] = r.out_bytes;
            final_block[n_chunks + i] = r.final_block;
            status[n_chunks + i] = r.status;
        }
        __syncthreads();                                         // (the tables are the next candidate's now)
    }
}

__global__ void gz_member_link_kernel(const uint8_t* __restrict__ comp, uint64_t comp_bytes, uint64_t data_bit0, uint64_t chunk_bits,
                                      uint64_t n_chunks, uint64_t cap, MemberPlanWs p, unsigned long long* info) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    const uint64_t count = info[kInfoMemberCandidates];
    if (count > cap) {
        info[kInfoStatus] = gz::kTooManyMembers;
        return;
    }
    gz::LinkArgs a;
    a.data = comp;
    a.n_bytes = comp_bytes;
    a.cand_rel = p.cand_rel;
    a.n_chunks = n_chunks;
    a.data_bit0 = data_bit0;
    a.chunk_bits = chunk_bits;
    a.land = p.land;
    a.out_bytes = p.out_bytes;
    a.final_block = p.final_block;
    a.status = p.status;
    a.m_start = p.m_start;
    a.members = {p.m_off, p.m_next, p.m_head, (uint64_t)p.n_buckets, (uint32_t)count};
    a.seg_cap = n_chunks + cap;
    a.row_cap = cap + 1u;
    const gz::LinkResult r = gz::link_members(a, p.live_idx, p.live_off, p.live_mem, p.rows);
    info[kInfoStatus] = r.status;
    info[kInfoText] = r.text_bytes;
    info[kInfoLive] = r.n_live;
    info[kInfoEndBit] = r.end_bit;
    info[kInfoBadChunk] = r.status ? p.live_idx[r.n_live - 1u] : 0u;
    info[kInfoMembers] = r.n_members;
    info[kInfoBadMember] = r.bad_member;
    info[kInfoBadMemberOffset] = r.bad_member_offset;
}

__global__ __launch_bounds__(64) void gz_segment_decode_kernel(const uint8_t* __restrict__ comp, uint64_t comp_bytes, uint64_t data_bit0,
                                                               uint64_t end_bit, uint64_t chunk_bits, uint64_t n_chunks,
                                                               const uint32_t* __restrict__ cand_rel, const uint64_t* __restrict__ m_start,
                                                               const uint64_t* __restrict__ land, const uint64_t* __restrict__ out_bytes,
                                                               const uint32_t* __restrict__ live_idx, const uint64_t* __restrict__ live_off,
                                                               const uint64_t* __restrict__ live_mem, uint64_t n_live, uint64_t text_bytes,
                                                               uint16_t* sym, uint32_t* __restrict__ status,
                                                               const unsigned long long* __restrict__ info) {
    __shared__ gz::WalkTables t;
    const uint64_t i = blockIdx.x;
    if (i >= n_live || info[kInfoStatus] != 0ull) return;
    const uint64_t w = live_idx[i];
    WaveCtx c = wave_ctx(comp, comp_bytes);
    gz::WalkArgs a = {};
    a.start_bit = w < n_chunks ? data_bit0 + w * chunk_bits + cand_rel[w] : m_start[w - n_chunks];
    a.end_bit = end_bit;
    a.stop_bit = land[w];
    a.out_cap = out_bytes[w];
    a.text_off = live_off[i];
    a.member_off = live_mem[i];
    uint32_t st = gz::kOutputOverrun;
    if (a.member_off <= a.text_off && a.text_off <= text_bytes && a.out_cap <= text_bytes - a.text_off) {
        c.sym = sym + a.text_off;
        st = gz::walk_chunk<true>(c, t, a).status;
    }
    if (threadIdx.x == 0u) status[i] = st;
}

// CRC-32 per member.  A thread per slice of 1 KiB, counted from its member's first byte: the bytes in front of the first
// 16-byte boundary one by one, aligned 16-byte words, the odd bytes behind them.  (The one-member file: the grid of
// gz_crc_slice_kernel, no head.)
__global__ __launch_bounds__(256) void gz_member_crc_slice_kernel(const uint8_t* __restrict__ text, const gz::MemberRow* __restrict__ rows,
                                                                  uint32_t* __restrict__ crc_slice, uint64_t max_slices,
                                                                  const unsigned long long* __restrict__ info) {
    __shared__ uint32_t s_tab[4][256];
    if (info[kInfoStatus] != 0ull) return;
    crc_fill_tables(s_tab, threadIdx.x);
    __syncthreads();
    const uint64_t n_members = info[kInfoMembers];
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const gz::MemberRow last = rows[n_members - 1u];
    if (s >= max_slices || s >= last.slice0 + gz::crc_slices_of(last.text_bytes)) return;
    const gz::MemberRow row = rows[gz::member_of<false>(rows, n_members, s)];
    const uint64_t in_member = (s - row.slice0) * kCrcSlice;
    const uint64_t lo = row.text_off + in_member;
    const uint32_t len = row.text_bytes - in_member < kCrcSlice ? (uint32_t)(row.text_bytes - in_member) : kCrcSlice;
    uint32_t crc = 0xffffffffu;
    uint32_t k = 0;
    const uint32_t head = (uint32_t)(-(int64_t)lo & 15);
    for (; k < head && k < len; ++k) crc = crc_byte(s_tab, crc, text[lo + k]);
    const uint4* src = reinterpret_cast<const uint4*>(text + lo + k);
    for (uint32_t q = 0; k + 16u <= len; ++q, k += 16u) {
        const uint4 w = src[q];
        crc = crc_dword(s_tab, crc, w.x);
        crc = crc_dword(s_tab, crc, w.y);
        crc = crc_dword(s_tab, crc, w.z);
        crc = crc_dword(s_tab, crc, w.w);
    }
    for (; k < len; ++k) crc = crc_byte(s_tab, crc, text[lo + k]);
    crc_slice[s] = ~crc;
}
// ... a thread per group of 64 slices of one member ...
__global__ __launch_bounds__(256) void gz_member_crc_group_kernel(const uint32_t* __restrict__ crc_slice, const gz::MemberRow* __restrict__ rows,
                                                                  uint32_t* __restrict__ crc_group, uint64_t max_groups,
                                                                  const unsigned long long* __restrict__ info) {
    if (info[kInfoStatus] != 0ull) return;
    const uint64_t n_members = info[kInfoMembers];
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const gz::MemberRow last = rows[n_members - 1u];
    if (g >= max_groups || g >= last.group0 + gz::crc_groups_of(last.text_bytes)) return;
    const gz::MemberRow row = rows[gz::member_of<true>(rows, n_members, g)];
    const uint64_t n_slices = gz::crc_slices_of(row.text_bytes);
    const uint64_t lo = (g - row.group0) * kCrcGroup;
    const uint64_t hi = lo + kCrcGroup < n_slices ? lo + kCrcGroup : n_slices;
    const uint32_t whole = crc_x8n(kCrcSlice);
    uint32_t acc = 0;
    for (uint64_t s = lo; s < hi; ++s) {
        const uint64_t bytes = s + 1u == n_slices ? row.text_bytes - s * kCrcSlice : (uint64_t)kCrcSlice;
        acc = crc_mul_lanes(acc, bytes == kCrcSlice ? whole : crc_x8n((uint32_t)bytes)) ^ crc_slice[row.slice0 + s];
    }
    crc_group[g] = acc;
}
// ... and one workgroup: a thread per member folds its groups and holds them against its trailer; the first bad member by
// file order is the one reported
__global__ __launch_bounds__(256) void gz_member_crc_check_kernel(const uint8_t* __restrict__ comp, const uint32_t* __restrict__ crc_group,
                                                                  const gz::MemberRow* __restrict__ rows, unsigned long long* info) {
    __shared__ unsigned long long s_bad;
    if (info[kInfoStatus] != 0ull) return;
    if (threadIdx.x == 0u) s_bad = ~0ull;
    __syncthreads();
    const uint64_t n_members = info[kInfoMembers];
    const uint64_t group_bytes = (uint64_t)kCrcSlice * kCrcGroup;
    const uint32_t whole = crc_x8n((uint32_t)group_bytes);
    for (uint64_t m = threadIdx.x; m < n_members; m += 256u) {
        const gz::MemberRow row = rows[m];
        const uint64_t n_groups = gz::crc_groups_of(row.text_bytes);
        uint32_t acc = 0;
        for (uint64_t g = 0; g < n_groups; ++g) {
            const uint64_t bytes = g + 1u == n_groups ? row.text_bytes - g * group_bytes : group_bytes;
            acc = crc_mul_lanes(acc, bytes == group_bytes ? whole : crc_x8n((uint32_t)bytes)) ^ crc_group[row.group0 + g];
        }
        if (m + 1u == n_members) info[kInfoCrc] = acc;
        if (acc != le32(comp + row.trailer_off)) atomicMin(&s_bad, (unsigned long long)m);
    }
    __syncthreads();
    if (threadIdx.x == 0u && s_bad != ~0ull) {
        info[kInfoStatus] = gz::kBadCrc;
        info[kInfoBadMember] = s_bad;
        info[kInfoBadMemberOffset] = rows[s_bad].comp_off;
    }
}

bool member_plan_geometry(int64_t comp_bytes, int64_t data_off, int64_t chunk_bytes, int64_t member_cap, uint64_t* n_chunks) {
    if (member_cap < 0 || member_cap > ((int64_t)1 << 28)) return false;
    return plan_geometry(comp_bytes, data_off, chunk_bytes, n_chunks) && *n_chunks + (uint64_t)member_cap <= 0x7fffffffull;
}

}  // namespace

}  // namespace besst

using namespace besst;

extern "C" {

size_t besst_dev_gzip_plan_workspace_bytes(int64_t comp_bytes, int64_t data_off, int64_t chunk_bytes) {
    uint64_t n = 0;
    if (!plan_geometry(comp_bytes, data_off, chunk_bytes, &n)) return 0;
    return plan_layout(nullptr, (size_t)n).bytes;
}

int besst_dev_gzip_plan(void* stream, const void* comp, int64_t comp_bytes, int64_t data_off, int64_t chunk_bytes, int32_t steps,
                        void* workspace, size_t workspace_bytes, uint64_t* info) {
    BESST_REQUIRE(comp && workspace && info, "dev_gzip_plan: null pointer");
    uint64_t n = 0;
    BESST_REQUIRE(plan_geometry(comp_bytes, data_off, chunk_bytes, &n), "dev_gzip_plan: sizes out of range");
    BESST_REQUIRE(workspace_bytes >= plan_layout(nullptr, (size_t)n).bytes, "dev_gzip_plan: workspace too small");
    BESST_REQUIRE(((uintptr_t)comp & 3u) == 0 && ((uintptr_t)workspace & 15u) == 0 && ((uintptr_t)info & 7u) == 0,
                  "dev_gzip_plan: comp, workspace or info misaligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PlanWs p = plan_layout(workspace, (size_t)n);
    const uint8_t* c = static_cast<const uint8_t*>(comp);
    unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
    const uint64_t bit0 = (uint64_t)data_off * 8u, end_bit = (uint64_t)(comp_bytes - 8) * 8u, chunk_bits = (uint64_t)chunk_bytes * 8u;
    const uint32_t all = steps == 0 ? ~0u : (uint32_t)steps;
    if (all & 1u) {
        hipLaunchKernelGGL(gz_init_kernel, dim3((unsigned)((n + 255u) / 256u) + 1u), dim3(256), 0, s, p.cand_rel, n, inf);
        const uint64_t probe_bits = end_bit > bit0 + chunk_bits ? end_bit - bit0 - chunk_bits : 0u;
        if (probe_bits)
            hipLaunchKernelGGL(gz_probe_kernel, dim3((unsigned)((probe_bits / 8u + 255u) / 256u)), dim3(256), 0, s, c, (uint64_t)comp_bytes, bit0,
                               end_bit, chunk_bits, n, p.cand_rel);
    }
    if (all & 2u)
        hipLaunchKernelGGL(gz_count_kernel, dim3((unsigned)n), dim3(64), 0, s, c, (uint64_t)comp_bytes, bit0, end_bit, chunk_bits, n, p.cand_rel,
                           p.land, p.out_bytes, p.final_block, p.status, inf);
    if (all & 4u)
        hipLaunchKernelGGL(gz_link_kernel, dim3(1), dim3(1), 0, s, c, (uint64_t)comp_bytes, bit0, chunk_bits, n, p.land, p.out_bytes,
                           p.final_block, p.status, p.live_idx, p.live_off, inf);
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

size_t besst_dev_gzip_inflate_workspace_bytes(int64_t text_bytes, int64_t n_live) {
    if (text_bytes < 0 || text_bytes > ((int64_t)1 << 44) || n_live < 1 || n_live > 0x7fffffff) return 0;
    return inflate_layout(nullptr, (size_t)text_bytes, (size_t)n_live).bytes;
}

int besst_dev_gzip_inflate(void* stream, const void* comp, int64_t comp_bytes, int64_t data_off, int64_t chunk_bytes, int32_t steps,
                           const void* plan_workspace, int64_t n_live, int64_t text_bytes, void* text, void* workspace,
                           size_t workspace_bytes, uint64_t* info) {
    BESST_REQUIRE(comp && plan_workspace && text && workspace && info, "dev_gzip_inflate: null pointer");
    uint64_t n = 0;
    BESST_REQUIRE(plan_geometry(comp_bytes, data_off, chunk_bytes, &n), "dev_gzip_inflate: sizes out of range");
    const size_t need = besst_dev_gzip_inflate_workspace_bytes(text_bytes, n_live);
    BESST_REQUIRE(need != 0 && (uint64_t)n_live <= n, "dev_gzip_inflate: text_bytes or n_live out of range");
    BESST_REQUIRE(workspace_bytes >= need, "dev_gzip_inflate: workspace too small");
    BESST_REQUIRE(((uintptr_t)comp & 3u) == 0 && ((uintptr_t)workspace & 15u) == 0 && ((uintptr_t)plan_workspace & 15u) == 0 &&
                      ((uintptr_t)text & 15u) == 0 && ((uintptr_t)info & 7u) == 0,
                  "dev_gzip_inflate: comp, text, a workspace or info misaligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PlanWs p = plan_layout(const_cast<void*>(plan_workspace), (size_t)n);
    const InflateWs w = inflate_layout(workspace, (size_t)text_bytes, (size_t)n_live);
    const uint8_t* c = static_cast<const uint8_t*>(comp);
    uint8_t* out = static_cast<uint8_t*>(text);
    unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
    const uint64_t bit0 = (uint64_t)data_off * 8u, end_bit = (uint64_t)(comp_bytes - 8) * 8u, chunk_bits = (uint64_t)chunk_bytes * 8u;
    const uint64_t live = (uint64_t)n_live, bytes = (uint64_t)text_bytes;
    const uint32_t all = steps == 0 ? ~0u : (uint32_t)steps;
    if (all & 1u)
        hipLaunchKernelGGL(gz_decode_kernel, dim3((unsigned)live), dim3(64), 0, s, c, (uint64_t)comp_bytes, bit0, end_bit, chunk_bits,
                           p.cand_rel, p.land, p.out_bytes, p.live_idx, p.live_off, live, bytes, w.sym, w.status, inf);
    if (all & 2u)
        hipLaunchKernelGGL(gz_windows_kernel, dim3(1), dim3(1024), 0, s, w.sym, p.out_bytes, p.live_idx, p.live_off, w.status, live, out, inf);
    if (all & 4u)
        hipLaunchKernelGGL(gz_translate_kernel, dim3((unsigned)live, kTranslateSplit), dim3(256), 0, s, w.sym, p.out_bytes, p.live_idx,
                           p.live_off, live, out, inf);
    if (all & 8u) {
        const size_t slices = crc_slices((size_t)bytes), groups = crc_groups((size_t)bytes);
        if (slices) {
            hipLaunchKernelGGL(gz_crc_slice_kernel, dim3((unsigned)((slices + 255u) / 256u)), dim3(256), 0, s, out, bytes, w.crc_slice, inf);
            hipLaunchKernelGGL(gz_crc_group_kernel, dim3((unsigned)((groups + 255u) / 256u)), dim3(256), 0, s, w.crc_slice, bytes, w.crc_group, inf);
        }
        hipLaunchKernelGGL(gz_crc_check_kernel, dim3(1), dim3(1), 0, s, c, w.crc_group, bytes, inf);
    }
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

size_t besst_dev_gzip_members_plan_workspace_bytes(int64_t comp_bytes, int64_t data_off, int64_t chunk_bytes, int64_t member_cap) {
    uint64_t n = 0;
    if (!member_plan_geometry(comp_bytes, data_off, chunk_bytes, member_cap, &n)) return 0;
    return member_plan_layout(nullptr, (size_t)n, (size_t)member_cap, (size_t)comp_bytes).bytes;
}

int besst_dev_gzip_members_plan(void* stream, const void* comp, int64_t comp_bytes, int64_t data_off, int64_t chunk_bytes,
                                int64_t member_cap, int32_t steps, void* workspace, size_t workspace_bytes, uint64_t* info) {
    BESST_REQUIRE(comp && workspace && info, "dev_gzip_members_plan: null pointer");
    uint64_t n = 0;
    BESST_REQUIRE(member_plan_geometry(comp_bytes, data_off, chunk_bytes, member_cap, &n), "dev_gzip_members_plan: sizes out of range");
    const uint64_t cap = (uint64_t)member_cap;
    BESST_REQUIRE(workspace_bytes >= member_plan_layout(nullptr, (size_t)n, (size_t)cap, (size_t)comp_bytes).bytes,
                  "dev_gzip_members_plan: workspace too small");
    BESST_REQUIRE(((uintptr_t)comp & 3u) == 0 && ((uintptr_t)workspace & 15u) == 0 && ((uintptr_t)info & 7u) == 0,
                  "dev_gzip_members_plan: comp, workspace or info misaligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const MemberPlanWs p = member_plan_layout(workspace, (size_t)n, (size_t)cap, (size_t)comp_bytes);
    const uint8_t* c = static_cast<const uint8_t*>(comp);
    unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
    const uint64_t bit0 = (uint64_t)data_off * 8u, end_bit = (uint64_t)(comp_bytes - 8) * 8u, chunk_bits = (uint64_t)chunk_bytes * 8u;
    const uint32_t all = steps == 0 ? ~0u : (uint32_t)steps;
    if (all & 1u) {
        const uint64_t init = n > p.n_buckets ? n : (uint64_t)p.n_buckets;
        hipLaunchKernelGGL(gz_member_init_kernel, dim3((unsigned)((init + 255u) / 256u) + 1u), dim3(256), 0, s, p.cand_rel, n, p.m_head,
                           (uint64_t)p.n_buckets, inf);
        hipLaunchKernelGGL(gz_member_mark_kernel, dim3((unsigned)(((uint64_t)comp_bytes / 16u + 256u) / 256u)), dim3(256), 0, s,
                           static_cast<const uint32_t*>(comp), (uint64_t)comp_bytes, cap, p.m_off, p.m_next, p.m_head, inf);
        const uint64_t probe_bits = end_bit > bit0 + chunk_bits ? end_bit - bit0 - chunk_bits : 0u;
        if (probe_bits)
            hipLaunchKernelGGL(gz_probe_kernel, dim3((unsigned)((probe_bits / 8u + 255u) / 256u)), dim3(256), 0, s, c, (uint64_t)comp_bytes, bit0,
                               end_bit, chunk_bits, n, p.cand_rel);
    }
    if (all & 2u) {
        hipLaunchKernelGGL(gz_count_kernel, dim3((unsigned)n), dim3(64), 0, s, c, (uint64_t)comp_bytes, bit0, end_bit, chunk_bits, n, p.cand_rel,
                           p.land, p.out_bytes, p.final_block, p.status, inf);
        if (cap)
            hipLaunchKernelGGL(gz_member_count_kernel, dim3(cap < kMemberCountBlocks ? (unsigned)cap : kMemberCountBlocks), dim3(64), 0, s, c,
                               (uint64_t)comp_bytes, bit0, end_bit, chunk_bits, n, cap, p.cand_rel, p.m_off, p.m_start, p.land, p.out_bytes,
                               p.final_block, p.status, inf);
    }
    if (all & 4u)
        hipLaunchKernelGGL(gz_member_link_kernel, dim3(1), dim3(1), 0, s, c, (uint64_t)comp_bytes, bit0, chunk_bits, n, cap, p, inf);
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

size_t besst_dev_gzip_members_inflate_workspace_bytes(int64_t text_bytes, int64_t n_live, int64_t n_members) {
    if (text_bytes < 0 || text_bytes > ((int64_t)1 << 44) || n_live < 1 || n_live > 0x7fffffff || n_members < 1 || n_members > n_live)
        return 0;
    return member_inflate_layout(nullptr, (size_t)text_bytes, (size_t)n_live, (size_t)n_members).bytes;
}

int besst_dev_gzip_members_inflate(void* stream, const void* comp, int64_t comp_bytes, int64_t data_off, int64_t chunk_bytes,
                                   int64_t member_cap, int32_t steps, const void* plan_workspace, int64_t n_live, int64_t n_members,
                                   int64_t text_bytes, void* text, void* workspace, size_t workspace_bytes, uint64_t* info) {
    BESST_REQUIRE(comp && plan_workspace && text && workspace && info, "dev_gzip_members_inflate: null pointer");
    uint64_t n = 0;
    BESST_REQUIRE(member_plan_geometry(comp_bytes, data_off, chunk_bytes, member_cap, &n), "dev_gzip_members_inflate: sizes out of range");
    const uint64_t cap = (uint64_t)member_cap;
    const size_t need = besst_dev_gzip_members_inflate_workspace_bytes(text_bytes, n_live, n_members);
    BESST_REQUIRE(need != 0 && (uint64_t)n_live <= n + cap && (uint64_t)n_members <= cap + 1u,
                  "dev_gzip_members_inflate: text_bytes, n_live or n_members out of range");
    BESST_REQUIRE(workspace_bytes >= need, "dev_gzip_members_inflate: workspace too small");
    BESST_REQUIRE(((uintptr_t)comp & 3u) == 0 && ((uintptr_t)workspace & 15u) == 0 && ((uintptr_t)plan_workspace & 15u) == 0 &&
                      ((uintptr_t)text & 15u) == 0 && ((uintptr_t)info & 7u) == 0,
                  "dev_gzip_members_inflate: comp, text, a workspace or info misaligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const MemberPlanWs p = member_plan_layout(const_cast<void*>(plan_workspace), (size_t)n, (size_t)cap, (size_t)comp_bytes);
    const MemberInflateWs w = member_inflate_layout(workspace, (size_t)text_bytes, (size_t)n_live, (size_t)n_members);
    const uint8_t* c = static_cast<const uint8_t*>(comp);
    uint8_t* out = static_cast<uint8_t*>(text);
    unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
    const uint64_t bit0 = (uint64_t)data_off * 8u, end_bit = (uint64_t)(comp_bytes - 8) * 8u, chunk_bits = (uint64_t)chunk_bytes * 8u;
    const uint64_t live = (uint64_t)n_live, bytes = (uint64_t)text_bytes;
    const uint32_t all = steps == 0 ? ~0u : (uint32_t)steps;
    if (all & 1u)
        hipLaunchKernelGGL(gz_segment_decode_kernel, dim3((unsigned)live), dim3(64), 0, s, c, (uint64_t)comp_bytes, bit0, end_bit, chunk_bits, n,
                           p.cand_rel, p.m_start, p.land, p.out_bytes, p.live_idx, p.live_off, p.live_mem, live, bytes, w.sym, w.status, inf);
    if (all & 2u)
        hipLaunchKernelGGL(gz_windows_kernel, dim3(1), dim3(1024), 0, s, w.sym, p.out_bytes, p.live_idx, p.live_off, w.status, live, out, inf);
    if (all & 4u)
        hipLaunchKernelGGL(gz_translate_kernel, dim3((unsigned)live, kTranslateSplit), dim3(256), 0, s, w.sym, p.out_bytes, p.live_idx,
                           p.live_off, live, out, inf);
    if (all & 8u) {
        if (bytes) {
            hipLaunchKernelGGL(gz_member_crc_slice_kernel, dim3((unsigned)((w.slices + 255u) / 256u)), dim3(256), 0, s, out, p.rows, w.crc_slice,
                               (uint64_t)w.slices, inf);
            hipLaunchKernelGGL(gz_member_crc_group_kernel, dim3((unsigned)((w.groups + 255u) / 256u)), dim3(256), 0, s, w.crc_slice, p.rows,
                               w.crc_group, (uint64_t)w.groups, inf);
        }
        hipLaunchKernelGGL(gz_member_crc_check_kernel, dim3(1), dim3(256), 0, s, c, w.crc_group, p.rows, inf);
    }
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

}  // extern "C"
