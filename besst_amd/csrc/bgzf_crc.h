// CRC-32 (the gzip trailer's) on the device, shared by the inflate's check (bgzf_gpu.hip: bgzf_crc_kernel) and the
// compressor (bgzf_deflate.hip): byte tables for slicing by four in shared memory, a slice's CRC word by word, and the
// multiplication modulo the CRC polynomial that carries a slice's CRC over the bytes behind it (zlib's crc32_combine).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace besst {
namespace {

constexpr uint32_t kCrcPoly = 0xedb88320u;
__device__ const uint32_t kCrcX2n[32] = {           // x^(2^k) mod the polynomial, reflected (zlib's x2n_table)
    0x40000000u, 0x20000000u, 0x08000000u, 0x00800000u, 0x00008000u, 0xedb88320u, 0xb1e6b092u, 0xa06a2517u,
    0xed627daeu, 0x88d14467u, 0xd7bbfe6au, 0xec447f11u, 0x8e7ea170u, 0x6427800eu, 0x4d47bae0u, 0x09fe548fu,
    0x83852d0fu, 0x30362f1au, 0x7b5a9cc3u, 0x31fec169u, 0x9fec022au, 0x6c8dedc4u, 0x15d6874du, 0x5fde7a4eu,
    0xbad90e37u, 0x2e4e5eefu, 0x4eaba214u, 0xa8a472c0u, 0x429a969eu, 0x148d302au, 0xc40ba6d0u, 0xc4e22c3cu};

// a(x) * b(x) modulo the polynomial (both reflected: bit 31 is x^0), any operands per lane
__device__ __forceinline__ uint32_t crc_mul_lanes(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll 8
    for (int j = 0; j < 32; ++j) {
        p ^= (a & (1u << 31)) ? b : 0u;
        a <<= 1;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

// x^(8 n) modulo the polynomial: binary exponentiation over the table (a multiplication per set bit of n)
__device__ __forceinline__ uint32_t crc_x8n(uint32_t n) {
    uint32_t p = 1u << 31;                                   // x^0
    for (uint32_t k = 3u; n; n >>= 1, ++k)
        if (n & 1u) p = crc_mul_lanes(kCrcX2n[k & 31u], p);
    return p;
}

// The four byte tables of slicing by four, filled by a workgroup of 256 threads (thread t: entry t of each): entry [j][t]
// is byte t carried over j further zero bytes, so that a dword of input costs four INDEPENDENT look-ups instead of a
// chain of four.  Holds a barrier; the caller puts one behind it.
__device__ __forceinline__ void crc_fill_tables(uint32_t (*tab)[256], uint32_t t) {
    uint32_t c = t;
#pragma unroll
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
    tab[0][t] = c;
    __syncthreads();
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        c = tab[0][c & 0xffu] ^ (c >> 8);
        tab[j][t] = c;
    }
}
__device__ __forceinline__ uint32_t crc_dword(const uint32_t (*tab)[256], uint32_t crc, uint32_t w) {
    const uint32_t x = crc ^ w;
    return tab[3][x & 0xffu] ^ tab[2][(x >> 8) & 0xffu] ^ tab[1][(x >> 16) & 0xffu] ^ tab[0][x >> 24];
}
__device__ __forceinline__ uint32_t crc_byte(const uint32_t (*tab)[256], uint32_t crc, uint32_t byte) {
    return tab[0][(crc ^ byte) & 0xffu] ^ (crc >> 8);
}

}  // namespace
}  // namespace besst
