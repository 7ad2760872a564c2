// BGZF compression on the GPU: the scaffold FASTA leaves the device compressed (GenerateOutput.py: --bgzf_outputs).
//
// Nucleotide text needs no general compressor: four letters carry two bits, and what LZ77 finds in them beyond that is
// runs - the 'N' gaps.  A block's DEFLATE data is ONE final dynamic-Huffman block of literals and matches of distance 1,
// or a stored block where that would not be smaller; blocks are independent, so a block is a workgroup:
//
//   bgzf_deflate_encode_kernel   one workgroup of 256 lanes per block of `block_payload` input bytes, into the block's slot
//                                of 64 KiB in the workspace.  A lane owns a span of the payload and walks its tokens three
//                                times (the input comes from L2 after the first): frequencies into a histogram in LDS
//                                and the CRC-32 of the span; bits per lane, once the code lengths are known (all lanes rank
//                                the symbols by frequency, one lane runs the two-queue merge, limits the lengths and
//                                writes the header's run-length code; the same steps again for the code-length alphabet);
//                                and, behind a workgroup scan of those bit counts, the bits themselves - gzip header,
//                                BSIZE, DEFLATE header, tokens, end of block, CRC and ISIZE are one bit stream that the
//                                lanes write side by side.  A word two lanes share is completed in LDS by the lane
//                                that holds its first bit (bgzf_deflate_core.h: BitWriter).
//   bgzf_deflate_scan_kernel     one workgroup: exclusive scan of the block sizes to 64-bit offsets, the total, the EOF block
//   bgzf_deflate_pack_kernel     one workgroup per block: the slot's bytes to their place in the file, 16-byte stores
//                                between byte stores at the two ends
//
// Three launches in stream order; no output byte depends on the order of atomics (the shared words are sums, ORs and an
// XOR).  The steps themselves live in bgzf_deflate_core.h, where the host test runs them too.  DESIGN.md section 10.2.
#include "bgzf_crc.h"
#include "bgzf_deflate_core.h"
#include "common.h"

namespace besst {

namespace {

using namespace deflate;

__device__ const uint8_t kEofBlock[kEofBytes] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                                                 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// exclusive scan of one value per lane over the workgroup of 256 (four waves); *total: the sum
__device__ __forceinline__ uint32_t block_scan_256(uint32_t v, uint32_t t, uint32_t* wave_sum, uint32_t* total) {
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)x, d, 64);
        if ((t & 63u) >= (uint32_t)d) x += o;
    }
    if ((t & 63u) == 63u) wave_sum[t >> 6] = x;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < (t >> 6); ++w) before += wave_sum[w];
    *total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    __syncthreads();                                         // (wave_sum may be used again)
    return before + x - v;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void bgzf_deflate_encode_kernel(const uint8_t* __restrict__ src, unsigned long long n_bytes,
                                                                       uint32_t block_payload, uint8_t* __restrict__ slots,
                                                                       uint32_t* __restrict__ sizes) {
    __shared__ BlockState s;
    __shared__ uint32_t s_crc[4][256];
    __shared__ uint32_t s_wave[4];
    const uint32_t t = threadIdx.x;
    const unsigned long long b = blockIdx.x;
    const unsigned long long at = b * block_payload;
    if (at >= n_bytes) return;                               // (uniform; the grid is the number of blocks)
    const uint32_t len = n_bytes - at < block_payload ? (uint32_t)(n_bytes - at) : block_payload;
    const uint8_t* in = src + at;
    uint8_t* slot = slots + b * kSlotStride;

    crc_fill_tables(s_crc, t);
    for (uint32_t i = t; i < (uint32_t)kNumLit; i += (uint32_t)kThreads) s.freq[i] = 0u;
    s.tail[t] = 0u;
    if (t == 0u) {
        s.extra_bits = 0u; s.n_match = 0u; s.crc = 0u; s.w.n_used = 0u;
    }
    __syncthreads();

    uint32_t lo, hi;
    span_of(len, t, &lo, &hi);
    ByteReader rd(in);
    // ---- 1. frequencies, and the span's CRC carried over the bytes behind it (zlib's crc32_combine; XOR of the lanes)
    count_step(s, rd, lo, hi, t);
    if (hi > lo) {
        uint32_t crc = 0xffffffffu;
        const uint8_t* p = in + lo;
        const uint8_t* e = in + hi;
        while (p < e && ((uintptr_t)p & 3u)) crc = crc_byte(s_crc, crc, *p++);
        for (; p + 4 <= e; p += 4) crc = crc_dword(s_crc, crc, *reinterpret_cast<const uint32_t*>(p));
        while (p < e) crc = crc_byte(s_crc, crc, *p++);
        crc = ~crc;
        if (hi < len) crc = crc_mul_lanes(crc_x8n(len - hi), crc);
        atomicXor(&s.crc, crc);
    }
    __syncthreads();
    // ---- 2. the literal / length code
    lengths_rank(s.freq, kNumLit, s.len, s.w, t);
    __syncthreads();
    if (t == 0u) lengths_serial(kLitLimit, s.len, s.w);
    __syncthreads();
    lengths_codes(kNumLit, s.len, s.code, s.w, t);
    __syncthreads();
    // ---- 3. the header: its code-length symbols, their code
    if (t == 0u) {
        header_rle(s);
        s.w.n_used = 0u;
    }
    __syncthreads();
    lengths_rank(s.cl_freq, kNumCl, s.cl_len, s.w, t);
    __syncthreads();
    if (t == 0u) lengths_serial(kClLimit, s.cl_len, s.w);
    __syncthreads();
    lengths_codes(kNumCl, s.cl_len, s.cl_code, s.w, t);
    __syncthreads();
    if (t == 0u) header_finish(s);
    __syncthreads();
    // ---- 4. bits per lane, where each lane begins
    const uint32_t bits = measure_step(s, rd, lo, hi, t);
    uint32_t end_bit;
    const uint32_t begin = block_scan_256(bits, t, s_wave, &end_bit);
    s.start[t] = begin;
    __syncthreads();
    if (takes_stored_form(end_bit, len)) {                   // (uniform)
        // ---- stored: the payload as it is behind five bytes
        const uint32_t bsize = kHeaderBytes + kStoredBytes + len + kTrailerBytes;
        if (t < 16u) slot[t] = kEofBlock[t];                 // (the fixed 16 bytes of every BGZF header)
        if (t == 16u) {
            slot[16] = (uint8_t)((bsize - 1u) & 0xffu);
            slot[17] = (uint8_t)((bsize - 1u) >> 8);
            slot[18] = 1;                                    // BFINAL, BTYPE = 0
            slot[19] = (uint8_t)(len & 0xffu);
            slot[20] = (uint8_t)(len >> 8);
            slot[21] = (uint8_t)(~len & 0xffu);
            slot[22] = (uint8_t)((~len >> 8) & 0xffu);
        }
        uint8_t* body = slot + kHeaderBytes + kStoredBytes;
        for (uint32_t i = t; i < len; i += (uint32_t)kThreads) body[i] = in[i];
        if (t < 4u) body[len + t] = (uint8_t)(s.crc >> (8u * t));
        else if (t < 8u) body[len + t] = (uint8_t)(len >> (8u * (t - 4u)));
        if (t == 0u) sizes[b] = bsize;
        return;
    }
    // ---- 5. the bits
    BitWriter w;
    w.begin(reinterpret_cast<uint32_t*>(slot), s, t);
    write_step(s, w, rd, lo, hi, t, len, end_bit);
    __syncthreads();
    w.finish(t);
    if (t == 0u) sizes[b] = ((end_bit + 7u) >> 3) + kTrailerBytes;
}

// offsets of the blocks in the file (exclusive scan of their sizes), the file's length, and the EOF block behind the last
__global__ __launch_bounds__(kThreads) void bgzf_deflate_scan_kernel(const uint32_t* __restrict__ sizes, unsigned long long n_blocks,
                                                                     int with_eof, long long* __restrict__ offsets,
                                                                     long long* __restrict__ block_off, uint8_t* __restrict__ out,
                                                                     long long* __restrict__ out_bytes) {
    __shared__ uint32_t s_wave[4];
    const uint32_t t = threadIdx.x;
    unsigned long long carry = 0;
    for (unsigned long long base = 0; base < n_blocks; base += (unsigned long long)kThreads) {
        const unsigned long long i = base + t;
        const uint32_t v = i < n_blocks ? sizes[i] : 0u;
        uint32_t sum;
        const uint32_t before = block_scan_256(v, t, s_wave, &sum);
        if (i < n_blocks) {
            offsets[i] = (long long)(carry + before);
            if (block_off) block_off[i] = (long long)(carry + before);
        }
        carry += sum;
    }
    if (t == 0u) {
        offsets[n_blocks] = (long long)carry;
        if (block_off) block_off[n_blocks] = (long long)carry;
        if (out_bytes) *out_bytes = (long long)carry + (with_eof ? (long long)kEofBytes : 0ll);
    }
    if (with_eof && t < kEofBytes) out[carry + t] = kEofBlock[t];
}

__global__ __launch_bounds__(kThreads) void bgzf_deflate_pack_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ sizes,
                                                                     const long long* __restrict__ offsets, uint8_t* __restrict__ out) {
    const uint32_t t = threadIdx.x;
    const unsigned long long b = blockIdx.x;
    const uint32_t size = sizes[b];
    const uint8_t* from = slots + b * kSlotStride;           // (16-byte aligned; the words behind `size` belong to the slot)
    uint8_t* to = out + offsets[b];
    uint32_t head = (uint32_t)(16u - ((uintptr_t)to & 15u)) & 15u;
    if (head > size) head = size;
    const uint32_t mid = (size - head) >> 4;                 // whole 16-byte words of the destination
    if (t < head) to[t] = from[t];
    // the source of a destination word begins at any byte: five aligned dwords, shifted into four
    const uint32_t* words = reinterpret_cast<const uint32_t*>(from + (head & ~3u));
    const uint32_t shift = (head & 3u) * 8u;
    for (uint32_t q = t; q < mid; q += (uint32_t)kThreads) {
        const uint32_t* p = words + 4u * q;
        const uint32_t a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3], a4 = p[4];
        uint4 v;
        v.x = __builtin_amdgcn_alignbit(a1, a0, shift);
        v.y = __builtin_amdgcn_alignbit(a2, a1, shift);
        v.z = __builtin_amdgcn_alignbit(a3, a2, shift);
        v.w = __builtin_amdgcn_alignbit(a4, a3, shift);
        *reinterpret_cast<uint4*>(to + head + 16u * q) = v;
    }
    const uint32_t done = head + 16u * mid;
    if (t < size - done) to[done + t] = from[done + t];
}

namespace {

struct Plan {
    int64_t n_blocks;
    size_t slots_bytes, sizes_bytes, offsets_bytes, total;
};
Plan plan_of(int64_t n_bytes, int32_t block_payload) {
    Plan p{};
    p.n_blocks = block_count(n_bytes, block_payload);
    p.slots_bytes = (size_t)p.n_blocks * kSlotStride;
    p.sizes_bytes = align_up((size_t)p.n_blocks * 4 + 4, 256);
    p.offsets_bytes = align_up((size_t)(p.n_blocks + 1) * 8, 256);
    p.total = 256 + p.slots_bytes + p.sizes_bytes + p.offsets_bytes;    // (256: the slots begin at an aligned address)
    return p;
}

}  // namespace

extern "C" {

size_t besst_dev_bgzf_deflate_bound(int64_t n_bytes, int32_t block_payload, int32_t with_eof) {
    if (n_bytes < 0 || !valid_payload(block_payload)) return 0;
    return (size_t)n_bytes + 31u * (size_t)block_count(n_bytes, block_payload) + (with_eof ? (size_t)kEofBytes : 0u);
}

size_t besst_dev_bgzf_deflate_workspace_bytes(int64_t n_bytes, int32_t block_payload) {
    if (n_bytes < 0 || !valid_payload(block_payload)) return 0;
    return plan_of(n_bytes, block_payload).total;
}

int besst_dev_bgzf_deflate(void* stream, const void* src, int64_t n_bytes, int32_t block_payload, int32_t with_eof, void* workspace,
                           size_t workspace_bytes, void* out, size_t out_cap, int64_t* out_bytes, int64_t* block_off) {
    BESST_REQUIRE(n_bytes >= 0, "bgzf_deflate: n_bytes is negative");
    BESST_REQUIRE(valid_payload(block_payload), "bgzf_deflate: block_payload must be in 1..65280");
    BESST_REQUIRE(workspace && out_bytes && (n_bytes == 0 || (src && out)) && (out || !with_eof), "bgzf_deflate: null pointer");
    const Plan p = plan_of(n_bytes, block_payload);
    BESST_REQUIRE(p.n_blocks < ((int64_t)1 << 31), "bgzf_deflate: too many blocks for one call");
    BESST_REQUIRE(workspace_bytes >= p.total, "bgzf_deflate: workspace smaller than besst_dev_bgzf_deflate_workspace_bytes");
    BESST_REQUIRE(out_cap >= besst_dev_bgzf_deflate_bound(n_bytes, block_payload, with_eof), "bgzf_deflate: output smaller than besst_dev_bgzf_deflate_bound");
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* slots = reinterpret_cast<uint8_t*>(align_up((size_t)(uintptr_t)workspace, 256));
    uint32_t* sizes = reinterpret_cast<uint32_t*>(slots + p.slots_bytes);
    long long* offsets = reinterpret_cast<long long*>(slots + p.slots_bytes + p.sizes_bytes);
    if (p.n_blocks)
        hipLaunchKernelGGL(bgzf_deflate_encode_kernel, dim3((uint32_t)p.n_blocks), dim3(kThreads), 0, s, static_cast<const uint8_t*>(src),
                           (unsigned long long)n_bytes, (uint32_t)block_payload, slots, sizes);
    hipLaunchKernelGGL(bgzf_deflate_scan_kernel, dim3(1), dim3(kThreads), 0, s, sizes, (unsigned long long)p.n_blocks, with_eof ? 1 : 0, offsets,
                       reinterpret_cast<long long*>(block_off), static_cast<uint8_t*>(out), reinterpret_cast<long long*>(out_bytes));
    if (p.n_blocks)
        hipLaunchKernelGGL(bgzf_deflate_pack_kernel, dim3((uint32_t)p.n_blocks), dim3(kThreads), 0, s, slots, sizes, offsets,
                           static_cast<uint8_t*>(out));
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

int besst_bgzf_deflate_device(int device, const void* src, size_t n_bytes, int32_t block_payload, int32_t with_eof, void* out, size_t out_cap,
                              size_t* out_len) {
    BESST_REQUIRE(out_len && (src || n_bytes == 0) && (out || out_cap == 0), "bgzf_deflate_device: null pointer");
    BESST_REQUIRE(valid_payload(block_payload), "bgzf_deflate_device: block_payload must be in 1..65280");
    BESST_REQUIRE(n_bytes < ((size_t)1 << 62), "bgzf_deflate_device: too many bytes");
    const size_t bound = besst_dev_bgzf_deflate_bound((int64_t)n_bytes, block_payload, with_eof);
    BESST_REQUIRE(out_cap >= bound, "bgzf_deflate_device: output smaller than besst_dev_bgzf_deflate_bound");
    BESST_HIP_TRY(hipSetDevice(device));
    const size_t ws_bytes = besst_dev_bgzf_deflate_workspace_bytes((int64_t)n_bytes, block_payload);
    uint8_t *d_src = nullptr, *d_ws = nullptr, *d_out = nullptr;
    int64_t* d_len = nullptr;
    auto release = [&]() {
        if (d_src) (void)hipFree(d_src);
        if (d_ws) (void)hipFree(d_ws);
        if (d_out) (void)hipFree(d_out);
        if (d_len) (void)hipFree(d_len);
    };
    int rc = BESST_OK;
    int64_t len = 0;
    hipError_t e = hipMalloc((void**)&d_src, n_bytes + 64);
    if (e == hipSuccess) e = hipMalloc((void**)&d_ws, ws_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&d_out, bound + 64);
    if (e == hipSuccess) e = hipMalloc((void**)&d_len, 8);
    if (e == hipSuccess && n_bytes) e = hipMemcpy(d_src, src, n_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = besst_dev_bgzf_deflate(nullptr, d_src, (int64_t)n_bytes, block_payload, with_eof, d_ws, ws_bytes, d_out, bound + 64, d_len, nullptr);
        if (rc == BESST_OK) {
            e = hipMemcpy(&len, d_len, 8, hipMemcpyDeviceToHost);
            if (e == hipSuccess && (len < 0 || (size_t)len > bound)) {
                set_error("bgzf_deflate_device: %lld bytes came out, beyond the bound of %zu", (long long)len, bound);
                rc = BESST_ERR_UNSUPPORTED;
            } else if (e == hipSuccess && len) {
                e = hipMemcpy(out, d_out, (size_t)len, hipMemcpyDeviceToHost);
            }
        }
    }
    if (e != hipSuccess) {
        set_error("bgzf_deflate_device: %s", hipGetErrorString(e));
        rc = e == hipErrorOutOfMemory ? BESST_ERR_NOMEM : BESST_ERR_HIP;
    }
    release();
    if (rc) return rc;
    *out_len = (size_t)len;
    return BESST_OK;
}

}  // extern "C"

}  // namespace besst
