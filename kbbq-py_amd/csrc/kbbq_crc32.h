// kbbq_crc32.h -- the CRC32 of gzip (reflected, polynomial 0xedb88320) cut into strips: what bz_deflate (kbbq_bgzf.h) computes of the
// text it packs and bi_inflate (kbbq_bgzf_inflate.h) of the text it produced, and what the host twin of the latter checks with.
//
// A strip's CRC is taken through a 256-entry table; it is moved to its place by x^(8 * bytes after it) mod P and xored in: the CRC
// of a concatenation is linear in its parts.  Compiled for the device and, without HIP, for the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CRC_HD __host__ __device__ __forceinline__
#else
#define CRC_HD inline
#endif

constexpr uint32_t CRC_POLY = 0xedb88320u;

// entry i of the byte table
CRC_HD uint32_t crc_table_entry(uint32_t i)
{
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1;
    return c;
}

// a * b mod P over GF(2), reflected (bit 31 is x^0)
CRC_HD uint32_t crc_gf2_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}

// x2n[k] = x^(2^k) mod P, k = 0..31
CRC_HD void crc_x2n_fill(uint32_t* x2n)
{
    uint32_t p = 0x40000000u;                              // x^1
    x2n[0] = p;
    for (int k = 1; k < 32; ++k) { p = crc_gf2_mul(p, p); x2n[k] = p; }
}

// x^(8 * bytes) mod P
CRC_HD uint32_t crc_x8n(const uint32_t* x2n, uint32_t bytes)
{
    uint32_t p = 0x80000000u;
    for (uint32_t k = 3; bytes; bytes >>= 1, ++k)
        if (bytes & 1) p = crc_gf2_mul(x2n[k & 31], p);
    return p;
}

// what s[lo, hi) adds to the CRC32 of s[0, n): xor the strips' values together
CRC_HD uint32_t crc_strip(const uint32_t* tab, const uint32_t* x2n, const uint8_t* s, uint32_t lo, uint32_t hi, uint32_t n)
{
    uint32_t c = 0xffffffffu;
    for (uint32_t i = lo; i < hi; ++i) c = tab[(c ^ s[i]) & 255] ^ (c >> 8);
    c ^= 0xffffffffu;
    if (hi < n) c = crc_gf2_mul(crc_x8n(x2n, n - hi), c);
    return c;
}

// the strip of thread `t` of `nt`: a length in words that is odd, so that the lanes of a wave read different LDS banks
CRC_HD void crc_strip_of(uint32_t n, uint32_t t, uint32_t nt, uint32_t* lo, uint32_t* hi)
{
    uint32_t L = ((n + nt - 1) / nt + 3) & ~3u;
    if (!(L & 4)) L += 4;
    *lo = n < t * L ? n : t * L;
    *hi = n < *lo + L ? n : *lo + L;
}
