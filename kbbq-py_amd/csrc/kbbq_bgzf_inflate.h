// kbbq_bgzf_inflate.h -- BGZF input: inflate on the GPU, one BGZF member per workgroup (include/kbbq_hip.h "BGZF input").
//
// bi_member is the decoder, written once: RFC 1951 over one member's payload (any number of stored, fixed and dynamic blocks) into
// a window of exactly ISIZE bytes.  It is compiled for the device (bi_inflate) and for the host (kbbq_inflate_bgzf_host, the twin
// that the tests compare with zlib and that is fuzzed under the sanitizers).  It takes `nl` lanes of which the caller is `lane`:
// every lane runs the WHOLE decoder on the same bits -- a wave executes one instruction stream anyway, so the bit buffer, the table
// lookups and the Huffman tables cost what one lane would cost, and no lane has to be told what another decoded -- and the lanes
// differ only where bytes move: a literal is stored by lane 0, the bytes of a match and of a stored block are shared out,
//     out[p + j] = out[p - d + (j mod d)],  j = lane, lane + nl, ...
// which reads only bytes below p: an overlapping copy (d < length) needs no order among the lanes.  The host calls it with one
// lane.
//
// Bounded by construction: the bit reader never looks past payload[n) (need() before every take()), every write is checked against
// ISIZE before it is made, a distance against the bytes produced; the table builder refuses what does not fit its tables; every
// symbol is range-checked where it is used, so a stale or unused table entry can make a wrong byte -- which the CRC32 finds --
// but not a wild address.  Every loop consumes at least one payload bit per turn or ends.  A member the decoder does not fully
// verify gets a status (KBBQ_INFLATE_*) and the caller inflates it again on the host: zlib decides what a damaged input is.
//
// Huffman tables: canonical codes from the lengths, a primary lookup (10 bits literal/length, 8 bits distance, 7 bits code-length
// code) whose entries are  symbol << 16 | code length,  and for longer codes a pointer  offset << 16 | bits << 8 | 0x80  to a
// sub-table sized for the longest code under that prefix.
//
// bi_inflate, 256 threads, one workgroup per CU (the grid walks the members), LDS: the payload (64 KiB), the window (64 KiB),
// ~13 KiB of tables.  All threads stage the payload with 16-byte loads; wave 0 decodes; all threads take the CRC32 of the window in
// strips (kbbq_crc32.h) and, if it is the trailer's, write the text with 16-byte stores.  Payload and window lie in LDS at the
// alignment (mod 16) their bytes have in device memory.  Plain vector loads and stores and ordinary LDS atomics only.
#pragma once
#include "../../include/kbbq_hip.h"
#include "kbbq_crc32.h"
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BI_HD __host__ __device__ __forceinline__
#else
#define BI_HD inline
#endif

// what a lane stored is read by the others only behind this (LDS operations of a wave are processed in order)
#if defined(__HIP_DEVICE_COMPILE__)
#define BI_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
#else
#define BI_WAVE_SYNC() do { } while (0)
#endif

constexpr uint32_t BI_MAX_TEXT = 65536, BI_MAX_PAYLOAD = 65536;
constexpr uint32_t BI_LL_BITS = 10, BI_D_BITS = 8, BI_CL_BITS = 7;
constexpr uint32_t BI_LL_ENTRIES = (1u << BI_LL_BITS) + 1024, BI_D_ENTRIES = (1u << BI_D_BITS) + 512, BI_CL_ENTRIES = 1u << BI_CL_BITS;
constexpr uint32_t BI_NLENS = 320;                        // 288 literal/length + 32 distance code lengths
constexpr uint32_t BI_SUB = 0x80;

struct BiTables {
    uint32_t ll[BI_LL_ENTRIES], d[BI_D_ENTRIES], cl[BI_CL_ENTRIES];
    uint16_t sorted[BI_NLENS];                            // the used symbols by (code length, symbol)
    uint16_t count[16], offs[16];
    uint8_t lens[BI_NLENS];
};

struct BiBits {
    const uint8_t* in; uint32_t n, pos;                   // pos: the next byte to load
    uint64_t buf; uint32_t cnt;                           // cnt valid bits of buf, low bit first
};

// 33 bits or more in the buffer, or all that is left: whole aligned words while they last, bytes at the edges
BI_HD void bi_refill(BiBits& b)
{
    while (b.cnt <= 32 && b.pos < b.n) {
        if ((((uintptr_t)b.in + b.pos) & 3) == 0 && b.pos + 4 <= b.n) {
            uint32_t w;
            __builtin_memcpy(&w, __builtin_assume_aligned(b.in + b.pos, 4), 4);
            b.buf |= (uint64_t)w << b.cnt;
            b.cnt += 32; b.pos += 4;
        } else {
            b.buf |= (uint64_t)b.in[b.pos] << b.cnt;
            b.cnt += 8; b.pos += 1;
        }
    }
}

BI_HD uint32_t bi_take(BiBits& b, uint32_t k)            // k <= 16 bits, b.cnt >= k
{
    const uint32_t v = (uint32_t)b.buf & ((1u << k) - 1);
    b.buf >>= k; b.cnt -= k;
    return v;
}

BI_HD uint32_t bi_rev(uint32_t v, uint32_t bits)         // the low `bits` (1..16) bits of v in reverse order
{
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
    v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
    return v >> (16 - bits);
}

// The lookup table of the code with lengths lens[0, nsym) (0: unused, at most 15): `pb` primary bits, `cap` entries in all.
// single_ok: a lone code of one bit is accepted although the set is incomplete (zlib does for the two alphabets of the data, never
// for the code-length code); its unused half decodes as length 0, which every user refuses.  No code at all is an empty table.
BI_HD uint32_t bi_build(BiTables* t, const uint8_t* lens, uint32_t nsym, uint32_t pb, uint32_t* tab, uint32_t cap, bool single_ok)
{
    for (uint32_t l = 0; l < 16; ++l) t->count[l] = 0;
    for (uint32_t s = 0; s < nsym; ++s) t->count[lens[s] & 15] += 1;
    const uint32_t used = nsym - t->count[0];
    int left = 1;
    for (uint32_t l = 1; l < 16; ++l) {
        left = (left << 1) - (int)t->count[l];
        if (left < 0) return KBBQ_INFLATE_CODE;            // over-subscribed
    }
    if (used && left > 0 && !(single_ok && used == 1 && t->count[1] == 1)) return KBBQ_INFLATE_CODE;   // incomplete
    for (uint32_t i = 0; i < (1u << pb); ++i) tab[i] = 0;
    if (!used) return KBBQ_INFLATE_OK;
    t->offs[1] = 0;
    for (uint32_t l = 1; l < 15; ++l) t->offs[l + 1] = (uint16_t)(t->offs[l] + t->count[l]);
    for (uint32_t s = 0; s < nsym; ++s) {
        const uint32_t l = lens[s] & 15;
        if (l) t->sorted[t->offs[l]++] = (uint16_t)s;
    }
    uint32_t code = 0, len = lens[t->sorted[0]] & 15, next = 1u << pb;
    for (uint32_t i = 0; i < used;) {
        const uint32_t s = t->sorted[i], l = lens[s] & 15;
        code <<= (l - len); len = l;
        if (l <= pb) {
            for (uint32_t k = bi_rev(code, l); k < (1u << pb); k += 1u << l) tab[k] = (s << 16) | l;
            ++i; ++code;
            continue;
        }
        // the codes that begin with these pb bits follow one another in this order; the last of them is the longest
        const uint32_t prefix = code >> (l - pb);
        uint32_t j = i, c = code, cl = l, longest = l;
        while (j < used) {
            const uint32_t lj = lens[t->sorted[j]] & 15;
            c <<= (lj - cl); cl = lj;
            if ((c >> (lj - pb)) != prefix) break;
            longest = lj; ++j; ++c;
        }
        const uint32_t sb = longest - pb, size = 1u << sb;
        if (next + size > cap) return KBBQ_INFLATE_TABLE;
        tab[bi_rev(prefix, pb)] = (next << 16) | (sb << 8) | BI_SUB;
        for (uint32_t k = 0; k < size; ++k) tab[next + k] = 0;
        for (; i < j; ++i, ++code) {
            const uint32_t si = t->sorted[i], li = lens[si] & 15;
            code <<= (li - len); len = li;
            for (uint32_t k = bi_rev(code, li) >> pb; k < size; k += 1u << (li - pb)) tab[next + k] = (si << 16) | li;
        }
        next += size;
    }
    return KBBQ_INFLATE_OK;
}

// the entry of the code at the front of the buffer: symbol << 16 | code length, or length 0 for a code that is not in the set
BI_HD uint32_t bi_lookup(const uint32_t* tab, uint32_t pb, uint64_t buf)
{
    uint32_t e = tab[(uint32_t)buf & ((1u << pb) - 1)];
    if (e & BI_SUB) e = tab[(e >> 16) + ((uint32_t)(buf >> pb) & ((1u << ((e >> 8) & 15)) - 1))];
    return e;
}

// the two codes of a fixed-Huffman block (RFC 1951 3.2.6)
BI_HD uint32_t bi_fixed(BiTables* t)
{
    for (uint32_t s = 0; s < 288; ++s) t->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (uint32_t s = 0; s < 32; ++s) t->lens[288 + s] = 5;
    uint32_t st = bi_build(t, t->lens, 288, BI_LL_BITS, t->ll, BI_LL_ENTRIES, true);
    if (!st) st = bi_build(t, t->lens + 288, 32, BI_D_BITS, t->d, BI_D_ENTRIES, true);
    return st;
}

// the two codes of a dynamic-Huffman block from its header (RFC 1951 3.2.7)
BI_HD uint32_t bi_dynamic(BiTables* t, BiBits& b)
{
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    bi_refill(b);
    if (b.cnt < 14) return KBBQ_INFLATE_INPUT;
    const uint32_t hlit = bi_take(b, 5) + 257, hdist = bi_take(b, 5) + 1, hclen = bi_take(b, 4) + 4;
    if (hlit > 286 || hdist > 30) return KBBQ_INFLATE_CODE;
    for (uint32_t i = 0; i < 19; ++i) t->lens[i] = 0;
    for (uint32_t i = 0; i < hclen; ++i) {
        bi_refill(b);
        if (b.cnt < 3) return KBBQ_INFLATE_INPUT;
        t->lens[order[i]] = (uint8_t)bi_take(b, 3);
    }
    uint32_t st = bi_build(t, t->lens, 19, BI_CL_BITS, t->cl, BI_CL_ENTRIES, false);
    if (st) return st;
    const uint32_t total = hlit + hdist;
    for (uint32_t n = 0; n < total;) {
        bi_refill(b);
        const uint32_t e = bi_lookup(t->cl, BI_CL_BITS, b.buf), l = e & 15, s = e >> 16;
        if (!l) return KBBQ_INFLATE_CODE;
        if (l > b.cnt) return KBBQ_INFLATE_INPUT;
        bi_take(b, l);
        if (s < 16) { t->lens[n++] = (uint8_t)s; continue; }
        const uint32_t xb = s == 16 ? 2 : s == 17 ? 3 : 7;
        if (b.cnt < xb) return KBBQ_INFLATE_INPUT;
        const uint32_t rep = (s == 18 ? 11 : 3) + bi_take(b, xb);
        if (s == 16 && n == 0) return KBBQ_INFLATE_CODE;   // nothing to repeat
        if (n + rep > total) return KBBQ_INFLATE_CODE;
        const uint8_t v = s == 16 ? t->lens[n - 1] : (uint8_t)0;
        for (uint32_t k = 0; k < rep; ++k) t->lens[n++] = v;
    }
    if (!t->lens[256]) return KBBQ_INFLATE_CODE;           // no end of block
    // the distance lengths move behind the 288 places of the other alphabet before either table is built from them
    for (uint32_t k = hdist; k-- > 0;) t->lens[288 + k] = t->lens[hlit + k];
    st = bi_build(t, t->lens, hlit, BI_LL_BITS, t->ll, BI_LL_ENTRIES, true);
    if (!st) st = bi_build(t, t->lens + 288, hdist, BI_D_BITS, t->d, BI_D_ENTRIES, true);
    return st;
}

// One BGZF member: the deflate payload in[0, n) into out[0, isize).  0, or the KBBQ_INFLATE_* that stopped it; out[0, isize) is
// the only memory written.  `nl` lanes call it together with the same arguments (the host: lane 0 of 1).
BI_HD uint32_t bi_member(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t isize, BiTables* t, uint32_t lane, uint32_t nl)
{
    BiBits b{in, n, 0, 0, 0};
    uint32_t p = 0;                                        // bytes produced
    for (uint32_t last = 0; !last;) {
        bi_refill(b);
        if (b.cnt < 3) return KBBQ_INFLATE_INPUT;
        last = bi_take(b, 1);
        const uint32_t btype = bi_take(b, 2);
        if (btype == 3) return KBBQ_INFLATE_BTYPE;
        if (btype == 0) {
            bi_take(b, b.cnt & 7);                         // to the byte boundary
            bi_refill(b);
            if (b.cnt < 32) return KBBQ_INFLATE_INPUT;
            const uint32_t len = bi_take(b, 16), nlen = bi_take(b, 16);
            if ((len ^ nlen) != 0xffffu) return KBBQ_INFLATE_STORED;
            b.pos -= b.cnt >> 3; b.cnt = 0; b.buf = 0;     // whole bytes were left in the buffer: they are read as bytes
            if (len > n - b.pos) return KBBQ_INFLATE_INPUT;
            if (len > isize - p) return KBBQ_INFLATE_OUTPUT;
            for (uint32_t j = lane; j < len; j += nl) out[p + j] = in[b.pos + j];
            BI_WAVE_SYNC();
            p += len; b.pos += len;
            continue;
        }
        const uint32_t st = btype == 1 ? bi_fixed(t) : bi_dynamic(t, b);
        if (st) return st;
        for (;;) {
            bi_refill(b);
            uint32_t e = bi_lookup(t->ll, BI_LL_BITS, b.buf), l = e & 15;
            const uint32_t sym = e >> 16;
            if (!l) return KBBQ_INFLATE_CODE;
            if (l > b.cnt) return KBBQ_INFLATE_INPUT;
            bi_take(b, l);
            if (sym < 256) {
                if (p >= isize) return KBBQ_INFLATE_OUTPUT;
                if (lane == 0) out[p] = (uint8_t)sym;
                ++p;
                continue;
            }
            if (sym == 256) break;
            if (sym >= 286) return KBBQ_INFLATE_SYMBOL;
            const uint32_t li = sym - 257;
            uint32_t len, xb = 0;
            if (li < 8) len = 3 + li;
            else if (li == 28) len = 258;
            else { xb = (li - 4) >> 2; len = 3 + ((4 + (li & 3)) << xb); }
            if (b.cnt < xb) return KBBQ_INFLATE_INPUT;
            len += bi_take(b, xb);
            bi_refill(b);
            e = bi_lookup(t->d, BI_D_BITS, b.buf); l = e & 15;
            const uint32_t ds = e >> 16;
            if (!l) return KBBQ_INFLATE_CODE;
            if (l > b.cnt) return KBBQ_INFLATE_INPUT;
            bi_take(b, l);
            if (ds >= 30) return KBBQ_INFLATE_SYMBOL;
            uint32_t dist = ds + 1;
            if (ds >= 4) {
                xb = (ds >> 1) - 1;
                if (b.cnt < xb) return KBBQ_INFLATE_INPUT;
                dist = 1 + ((2 + (ds & 1)) << xb) + bi_take(b, xb);
            }
            if (dist > p) return KBBQ_INFLATE_DISTANCE;
            if (len > isize - p) return KBBQ_INFLATE_OUTPUT;
            BI_WAVE_SYNC();                                // the literals lane 0 stored
            const uint8_t* from = out + p - dist;
            if (dist >= len) for (uint32_t j = lane; j < len; j += nl) out[p + j] = from[j];
            else for (uint32_t j = lane; j < len; j += nl) out[p + j] = from[j % dist];
            BI_WAVE_SYNC();
            p += len;
        }
    }
    if (p != isize) return KBBQ_INFLATE_ISIZE;
    if ((n - b.pos) + (b.cnt >> 3) != 0) return KBBQ_INFLATE_TRAILING;
    BI_WAVE_SYNC();
    return KBBQ_INFLATE_OK;
}

// the host's CRC32 of s[0, n) by the strips of the kernel (four of them, so that the moving of a strip's value is exercised)
inline uint32_t bi_crc_host(const uint8_t* s, uint32_t n)
{
    uint32_t tab[256], x2n[32], crc = 0;
    for (uint32_t i = 0; i < 256; ++i) tab[i] = crc_table_entry(i);
    crc_x2n_fill(x2n);
    for (uint32_t k = 0; k < 4; ++k) {
        uint32_t lo, hi;
        crc_strip_of(n, k, 4, &lo, &hi);
        if (lo < hi) crc ^= crc_strip(tab, x2n, s, lo, hi, n);
    }
    return crc;
}

// the host twin of bi_inflate's work on one member
inline uint32_t bi_member_host(const uint8_t* payload, uint32_t n, uint8_t* out, uint32_t isize, uint32_t crc, BiTables* t)
{
    if (n > BI_MAX_PAYLOAD || isize > BI_MAX_TEXT) return KBBQ_INFLATE_RANGE;
    const uint32_t st = bi_member(payload, n, out, isize, t, 0, 1);
    if (st) return st;
    return bi_crc_host(out, isize) == crc ? (uint32_t)KBBQ_INFLATE_OK : (uint32_t)KBBQ_INFLATE_CRC;
}

#if defined(__HIPCC__)
constexpr int BI_THREADS = 256;

struct BiParams {
    const uint8_t* src; uint64_t src_bytes;
    const kbbq_bgzf_block* blocks; uint32_t nblocks;
    uint8_t* out; uint64_t out_bytes;
    uint32_t* status;
};

struct BiSmall { uint32_t crc_tab[256], x2n[32], crc, status; };

constexpr size_t BI_IN_LDS = BI_MAX_PAYLOAD + 16, BI_WIN_LDS = BI_MAX_TEXT + 16;
constexpr size_t BI_TAB_LDS = (sizeof(BiTables) + 15) & ~(size_t)15;
constexpr size_t BI_LDS_BYTES = BI_IN_LDS + BI_WIN_LDS + BI_TAB_LDS + ((sizeof(BiSmall) + 15) & ~(size_t)15);

// dst[0, n) <- src[0, n) by the workgroup: single bytes up to the first 16-byte boundary and behind the last, 16 bytes between.
// dst and src are equal mod 16.
__device__ __forceinline__ void bi_copy16(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t tid)
{
    uint32_t head = (uint32_t)(0 - (uintptr_t)src) & 15u;
    if (head > n) head = n;
    const uint32_t body = (n - head) >> 4, tail = head + (body << 4);
    if (tid < head) dst[tid] = src[tid];
    const uint4* s4 = reinterpret_cast<const uint4*>(src + head);
    uint4* d4 = reinterpret_cast<uint4*>(dst + head);
    for (uint32_t i = tid; i < body; i += BI_THREADS) d4[i] = s4[i];
    if (tail + tid < n) dst[tail + tid] = src[tail + tid];
}

__global__ __launch_bounds__(BI_THREADS) void bi_inflate(BiParams q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bi_lds[];
    BiTables* const tb = reinterpret_cast<BiTables*>(bi_lds + BI_IN_LDS + BI_WIN_LDS);
    BiSmall* const sm = reinterpret_cast<BiSmall*>(bi_lds + BI_IN_LDS + BI_WIN_LDS + BI_TAB_LDS);
    const uint32_t tid = threadIdx.x;

    sm->crc_tab[tid] = crc_table_entry(tid);
    if (tid == 0) crc_x2n_fill(sm->x2n);

    for (uint32_t m = blockIdx.x; m < q.nblocks; m += gridDim.x) {
        const kbbq_bgzf_block k = q.blocks[m];
        __syncthreads();                                   // the member before has left LDS
        if (k.csize > BI_MAX_PAYLOAD || k.isize > BI_MAX_TEXT || k.src > q.src_bytes || k.csize > q.src_bytes - k.src
            || k.dst > q.out_bytes || k.isize > q.out_bytes - k.dst) {
            if (tid == 0) q.status[m] = KBBQ_INFLATE_RANGE;
            continue;
        }
        const uint8_t* const g = q.src + k.src;
        uint8_t* const o = q.out + k.dst;
        uint8_t* const in = bi_lds + ((uintptr_t)g & 15);
        uint8_t* const win = bi_lds + BI_IN_LDS + ((uintptr_t)o & 15);
        bi_copy16(in, g, k.csize, tid);
        if (tid == 0) sm->crc = 0;
        __syncthreads();
        if (tid < 64) {
            const uint32_t st = bi_member(in, k.csize, win, k.isize, tb, tid, 64);
            if (tid == 0) sm->status = st;
        }
        __syncthreads();
        uint32_t st = sm->status;
        if (!st) {
            uint32_t lo, hi;
            crc_strip_of(k.isize, tid, BI_THREADS, &lo, &hi);
            if (lo < hi) atomicXor(&sm->crc, crc_strip(sm->crc_tab, sm->x2n, win, lo, hi, k.isize));
            __syncthreads();
            if (sm->crc != k.crc) st = KBBQ_INFLATE_CRC;
        }
        if (!st) bi_copy16(o, win, k.isize, tid);
        if (tid == 0) q.status[m] = st;
    }
}
#endif
