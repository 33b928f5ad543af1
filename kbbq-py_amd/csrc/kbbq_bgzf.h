// BGZF output (--bgzf; kbbq/_bgzf.py): deflate on the GPU, one BGZF block per workgroup.
//
// The text is cut at multiples of block_bytes (1..65280); block b becomes a complete gzip member at blocks + b * 65536:
//   18 header bytes (1f 8b 08 04 00 00 00 00 00 ff 06 00 'B' 'C' 02 00, BSIZE - 1) | raw deflate | CRC32 of the text | ISIZE
// and its length goes to sizes[b].  The bytes are a function of (text, block_bytes) alone: every choice below is made from
// values that do not depend on which thread got where first -- maxima, sums, xors and prefix sums.
//
// bz_deflate, 512 threads, one workgroup per CU (the grid walks the blocks), LDS: the block's text (64 KiB), a table of 16,384
// words (64 KiB: hash heads while matching, the output bits afterwards) and ~11 KiB of small tables.
//   1. CRC32: a strip per thread through a 256-entry table, each strip's CRC moved to its place by x^(8 * bytes after it)
//      mod P and xored in (the CRC of a concatenation is linear in its parts).
//   2. LZ77, tile by tile of 512 positions, a thread a position.  The table holds, per hash of 4 bytes, the LATEST position
//      of the tiles before this one (atomicMax when a tile is done: the candidate does not depend on thread order); a match is
//      4..258 bytes at distance 1..32768, never before the block's first byte, never past its last.  The greedy parse of a
//      tile -- a position is a token iff the chain literal -> +1, match -> +length reaches it from where the tile before
//      left off -- is nine rounds of pointer doubling; a prefix sum over the reached positions numbers the tokens, which go
//      to a scratch array in device memory (4 bytes a token, at most 65,280) while their symbols are counted in LDS.
//   3. Two length-limited Huffman codes (literal/length: 15 bits, distance: 15 bits), one thread each, in different waves:
//      the symbols sorted by (count, symbol) by rank (a thread a symbol), the in-place minimum-redundancy lengths of
//      Moffat & Katajainen, lengths over the limit folded into it and the Kraft sum restored, canonical codes.  Then one
//      thread run-length codes the lengths (16, 17, 18), builds the code-length code (7 bits) and sizes the block.
//   4. If the dynamic-Huffman form (BTYPE 10) is smaller than the stored one (BTYPE 00, text + 5 bytes), every thread sums the
//      bits of its run of tokens, a prefix sum gives each run its bit offset, and the bits are ORed into LDS; else the text is
//      copied behind a stored header.  Header, trailer and payload leave LDS as aligned words.
// bz_scan_sizes / bz_pack: an exclusive scan of the sizes and a copy, so that only compressed bytes cross PCIe.
// Plain vector loads and stores and ordinary LDS / global atomics only.
#pragma once
#include "kbbq_helpers.h"
#include "kbbq_crc32.h"

constexpr int BZ_THREADS = 512;
constexpr u32 BZ_TILE = 512, BZ_ROUNDS = 9;               // 2^BZ_ROUNDS >= BZ_TILE: a chain inside a tile has at most BZ_TILE steps
constexpr u32 BZ_MAX_TEXT = 65280, BZ_SLOT = 65536;
constexpr u32 BZ_HASH_BITS = 14, BZ_TAB_WORDS = 1u << BZ_HASH_BITS;
constexpr u32 BZ_MIN_MATCH = 4, BZ_MAX_MATCH = 258, BZ_MAX_DIST = 32768;
constexpr u32 BZ_NLL = 288, BZ_ND = 32, BZ_NCL = 20;      // the alphabets (286, 30 and 19 symbols), rounded up
constexpr u32 BZ_TEXT_LDS = BZ_MAX_TEXT + 16;
static_assert((1u << BZ_ROUNDS) >= BZ_TILE && BZ_TILE == (u32)BZ_THREADS, "a thread a position, BZ_ROUNDS doublings a tile");
static_assert(BZ_TAB_WORDS * 4 >= BZ_SLOT, "the output bits of a block fit where the hash heads were");

struct BgzfParams {
    const uint8_t* text; int64_t n; u32 block_bytes; u32 nblocks;
    uint8_t* blocks;                  // [nblocks][BZ_SLOT]
    u32* sizes;                       // [nblocks]
    u32* tok;                         // [gridDim.x][BZ_MAX_TEXT] token scratch
};

struct BzSmall {
    u32 crc_tab[256], x2n[32];
    u32 freq_ll[BZ_NLL], freq_d[BZ_ND], freq_cl[BZ_NCL];
    u32 key_ll[BZ_NLL], key_d[BZ_ND], key_cl[BZ_NCL];     // the counts in ascending order; the length calculation works in place
    u32 cnt_ll[2][16], cnt_d[2][16], cnt_cl[2][16];       // codes per length, first code per length
    u32 jump[BZ_TILE], reach[BZ_TILE];
    u32 wsum[BZ_THREADS / 64];
    u32 crc, carry, carry_next, n_cl, hlit, hdist, hclen, hdr_bits, body_bits, coded;
    uint16_t sym_ll[BZ_NLL], sym_d[BZ_ND], sym_cl[BZ_NCL];
    uint16_t code_ll[BZ_NLL], code_d[BZ_ND], code_cl[BZ_NCL];
    uint16_t cl_stream[BZ_NLL + BZ_ND];                   // symbol | extra << 8
    uint8_t len_ll[BZ_NLL], len_d[BZ_ND], len_cl[BZ_NCL];
};

constexpr size_t BZ_LDS_BYTES = BZ_TEXT_LDS + (size_t)BZ_TAB_WORDS * 4 + ((sizeof(BzSmall) + 15) & ~(size_t)15);

// exclusive prefix sum of v over the workgroup and its total; two barriers
__device__ __forceinline__ u32 bz_scan(u32 v, u32* wsum, u32* total)
{
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 inc = v;
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 o = __shfl_up(inc, d);
        if (lane >= (u32)d) inc += o;
    }
    __syncthreads();                                       // the sums of the scan before have been read
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    u32 base = 0, tot = 0;
    #pragma unroll
    for (u32 w = 0; w < BZ_THREADS / 64; ++w) {
        const u32 s = wsum[w];
        if (w < wave) base += s;
        tot += s;
    }
    *total = tot;
    return base + inc - v;
}

// ---- symbols ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 bz_log2(u32 x) { return 31u - (u32)__clz((int)x); }

// length - 3 (0..255) -> literal/length symbol, number of extra bits, their value
__device__ __forceinline__ void bz_len_sym(u32 l, u32* sym, u32* eb, u32* ev)
{
    if (l < 8) { *sym = 257 + l; *eb = 0; *ev = 0; return; }
    if (l == 255) { *sym = 285; *eb = 0; *ev = 0; return; }
    const u32 e = bz_log2(l) - 2;
    *sym = 261 + 4 * e + ((l >> e) & 3); *eb = e; *ev = l & ((1u << e) - 1);
}

// distance - 1 (0..32767) -> distance symbol, number of extra bits, their value
__device__ __forceinline__ void bz_dist_sym(u32 d, u32* sym, u32* eb, u32* ev)
{
    if (d < 4) { *sym = d; *eb = 0; *ev = 0; return; }
    const u32 e = bz_log2(d) - 1;
    *sym = 2 * e + 2 + ((d >> e) & 1); *eb = e; *ev = d & ((1u << e) - 1);
}

__device__ __forceinline__ u32 bz_ll_extra(u32 sym) { return sym >= 265 && sym < 285 ? (sym - 261) >> 2 : 0; }
__device__ __forceinline__ u32 bz_d_extra(u32 sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }

constexpr u32 BZ_TOK_MATCH = 0x80000000u;                 // token: a literal's byte, or this | (length - 3) << 16 | (distance - 1)

// ---- Huffman ------------------------------------------------------------------------------------------------------------
// symbol i's place among the used symbols in ascending (count, symbol) order
__device__ __forceinline__ void bz_rank(const u32* freq, u32 nsym, u32 i, u32* key, uint16_t* sym)
{
    const u32 f = freq[i];
    if (!f) return;
    u32 r = 0;
    for (u32 j = 0; j < nsym; ++j) {
        const u32 g = freq[j];
        r += (g && (g < f || (g == f && j < i))) ? 1u : 0u;
    }
    key[r] = f; sym[r] = (uint16_t)i;
}

// One thread: code lengths of at most `limit` bits and canonical codes (bit-reversed: deflate sends a code's first bit first,
// everything else low bit first) for the symbols bz_rank has sorted.  len[] arrives zeroed.  A lone symbol gets one bit.
__device__ void bz_build_code(const u32* freq, u32 nsym, u32 limit, u32* A, const uint16_t* sym, u32 (*cnt)[16],
                                           uint8_t* len, uint16_t* code)
{
    int m = 0;
    for (u32 j = 0; j < nsym; ++j) m += freq[j] ? 1 : 0;
    if (m == 0) return;
    u32* count = cnt[0];
    u32* next = cnt[1];
    for (u32 i = 0; i < 16; ++i) count[i] = 0;
    if (m == 1) {
        A[0] = 1;
    } else {
        // minimum-redundancy lengths in place (Moffat & Katajainen 1995): parents, then depths of the internal nodes, then leaves
        A[0] += A[1];
        int root = 0, leaf = 2, nx;
        for (nx = 1; nx < m - 1; ++nx) {
            if (leaf >= m || A[root] < A[leaf]) { A[nx] = A[root]; A[root++] = (u32)nx; } else A[nx] = A[leaf++];
            if (leaf >= m || (root < nx && A[root] < A[leaf])) { A[nx] += A[root]; A[root++] = (u32)nx; } else A[nx] += A[leaf++];
        }
        A[m - 2] = 0;
        for (nx = m - 3; nx >= 0; --nx) A[nx] = A[A[nx]] + 1;
        int avbl = 1, used = 0;
        u32 depth = 0;
        root = m - 2; nx = m - 1;
        while (avbl > 0) {
            while (root >= 0 && A[root] == depth) { ++used; --root; }
            while (avbl > used) { A[nx--] = depth; --avbl; }
            avbl = 2 * used; ++depth; used = 0;
        }
    }
    // fold what is longer than the limit into it, then give codes back until the Kraft sum is 1 again
    for (int i = 0; i < m; ++i) count[min(A[i], limit)] += 1;
    if (m > 1) {
        u32 total = 0;
        for (u32 i = limit; i >= 1; --i) total += count[i] << (limit - i);
        while (total != (1u << limit)) {
            count[limit] -= 1;
            for (u32 i = limit - 1; i >= 1; --i)
                if (count[i]) { count[i] -= 1; count[i + 1] += 2; break; }
            total -= 1;
        }
    }
    // the shortest lengths to the most frequent symbols
    int j = m;
    for (u32 i = 1; i <= limit; ++i)
        for (u32 l = count[i]; l > 0; --l) len[sym[--j]] = (uint8_t)i;
    u32 c = 0;
    next[0] = 0;
    for (u32 bits = 1; bits <= limit; ++bits) { c = (c + (bits > 1 ? count[bits - 1] : 0)) << 1; next[bits] = c; }
    for (u32 s = 0; s < nsym; ++s) {
        const u32 l = len[s];
        if (l) code[s] = (uint16_t)(__brev(next[l]++) >> (32 - l));
    }
}

// nbits (<= 48) of val at bit `pos` of buf, low bit first
__device__ __forceinline__ void bz_put(u32* buf, u32 pos, u64 val, u32 nbits)
{
    const u32 w = pos >> 5, sh = pos & 31;
    const u64 lo = val << sh;
    atomicOr(&buf[w], (u32)lo);
    if (sh + nbits > 32) atomicOr(&buf[w + 1], (u32)(lo >> 32));
    if (sh + nbits > 64) atomicOr(&buf[w + 2], (u32)(val >> (64 - sh)));
}

// a token's bits: literal/length code, length extra bits, distance code, distance extra bits
__device__ __forceinline__ u32 bz_token_bits(const BzSmall* sm, u32 t, u64* val)
{
    if (!(t & BZ_TOK_MATCH)) { *val = sm->code_ll[t]; return sm->len_ll[t]; }
    u32 ls, le, lv, ds, de, dv;
    bz_len_sym((t >> 16) & 255, &ls, &le, &lv);
    bz_dist_sym(t & 0x7fff, &ds, &de, &dv);
    u32 n = sm->len_ll[ls];
    u64 v = sm->code_ll[ls];
    v |= (u64)lv << n; n += le;
    v |= (u64)sm->code_d[ds] << n; n += sm->len_d[ds];
    v |= (u64)dv << n; n += de;
    *val = v;
    return n;
}

// One thread: the code lengths of both alphabets run-length coded, the code-length code, and the sizes of the block
__device__ void bz_plan_header(BzSmall* sm, u32 n)
{
    u32 hlit = 286, hdist = 30;
    while (hlit > 257 && !sm->len_ll[hlit - 1]) --hlit;
    while (hdist > 1 && !sm->len_d[hdist - 1]) --hdist;
    const u32 N = hlit + hdist;
    for (u32 i = 0; i < BZ_NCL; ++i) { sm->freq_cl[i] = 0; sm->len_cl[i] = 0; sm->code_cl[i] = 0; }
    u32 ncl = 0;
    auto at = [&](u32 i) -> u32 { return i < hlit ? sm->len_ll[i] : sm->len_d[i - hlit]; };
    auto emit = [&](u32 s, u32 extra) { sm->cl_stream[ncl++] = (uint16_t)(s | (extra << 8)); sm->freq_cl[s] += 1; };
    for (u32 i = 0; i < N;) {
        const u32 v = at(i);
        u32 run = 1;
        while (i + run < N && at(i + run) == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 3) { const u32 r = min(run, 138u); if (r >= 11) emit(18, r - 11); else emit(17, r - 3); run -= r; }
            while (run) { emit(0, 0); --run; }
        } else {
            emit(v, 0); --run;
            while (run >= 3) { const u32 r = min(run, 6u); emit(16, r - 3); run -= r; }
            while (run) { emit(v, 0); --run; }
        }
    }
    for (u32 i = 0; i < 19; ++i) bz_rank(sm->freq_cl, 19, i, sm->key_cl, sm->sym_cl);
    bz_build_code(sm->freq_cl, 19, 7, sm->key_cl, sm->sym_cl, sm->cnt_cl, sm->len_cl, sm->code_cl);
    u32 used = 0, only = 0;
    for (u32 i = 0; i < 19; ++i) if (sm->len_cl[i]) { ++used; only = i; }
    // Not reachable from bz_deflate: the stream codes N >= 258 lengths, at least two of them not zero (a literal or a length,
    // and the end of block).  One distinct symbol would be a length v itself (16, 17 and 18 need a length or a zero beside
    // them), so 258 equal lengths in one run -- which is coded with 16s.  Kept for a caller with a shorter list.
    if (used == 1) {                                       // the code-length code must be complete: a second one-bit code, never sent
        const u32 other = only ? 0 : 18;
        sm->len_cl[other] = 1;
        sm->code_cl[only] = only < other ? 0 : 1; sm->code_cl[other] = only < other ? 1 : 0;
    }
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    u32 hclen = 4;
    for (u32 i = 0; i < 19; ++i) if (sm->len_cl[order[i]] && i + 1 > hclen) hclen = i + 1;
    u32 hdr = 3 + 5 + 5 + 4 + 3 * hclen;
    for (u32 i = 0; i < ncl; ++i) {
        const u32 s = sm->cl_stream[i] & 255;
        hdr += sm->len_cl[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
    }
    u32 body = 0;
    for (u32 s = 0; s < 286; ++s) body += sm->freq_ll[s] * (sm->len_ll[s] + bz_ll_extra(s));
    for (u32 s = 0; s < 30; ++s) body += sm->freq_d[s] * (sm->len_d[s] + bz_d_extra(s));
    sm->n_cl = ncl; sm->hlit = hlit; sm->hdist = hdist; sm->hclen = hclen; sm->hdr_bits = hdr; sm->body_bits = body;
    sm->coded = ((hdr + body + 7) >> 3) < n + 5 ? 1 : 0;
}

// One thread: the dynamic block's header from bit `pos` on
__device__ void bz_put_header(const BzSmall* sm, u32* buf, u32 pos)
{
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    bz_put(buf, pos, 5, 3); pos += 3;                      // BFINAL = 1, BTYPE = 10
    bz_put(buf, pos, sm->hlit - 257, 5); pos += 5;
    bz_put(buf, pos, sm->hdist - 1, 5); pos += 5;
    bz_put(buf, pos, sm->hclen - 4, 4); pos += 4;
    for (u32 i = 0; i < sm->hclen; ++i) { bz_put(buf, pos, sm->len_cl[order[i]], 3); pos += 3; }
    for (u32 i = 0; i < sm->n_cl; ++i) {
        const u32 e = sm->cl_stream[i], s = e & 255;
        const u32 l = sm->len_cl[s], x = s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0;
        bz_put(buf, pos, (u64)sm->code_cl[s] | ((u64)(e >> 8) << l), l + x);
        pos += l + x;
    }
}

__global__ __launch_bounds__(BZ_THREADS) void bz_deflate(BgzfParams q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bz_lds[];
    uint8_t* const s = bz_lds;
    u32* const tab = reinterpret_cast<u32*>(bz_lds + BZ_TEXT_LDS);
    BzSmall* const sm = reinterpret_cast<BzSmall*>(bz_lds + BZ_TEXT_LDS + BZ_TAB_WORDS * 4);
    const u32 tid = threadIdx.x;
    u32* const tok = q.tok + (size_t)blockIdx.x * BZ_MAX_TEXT;

    if (tid < 256) sm->crc_tab[tid] = crc_table_entry(tid);
    if (tid == 256) crc_x2n_fill(sm->x2n);

    for (u32 b = blockIdx.x; b < q.nblocks; b += gridDim.x) {
        const int64_t first = (int64_t)b * q.block_bytes;
        const int64_t left = q.n - first;
        const u32 n = left < (int64_t)q.block_bytes ? (u32)left : q.block_bytes;
        const uint8_t* const g = q.text + first;
        __syncthreads();                                   // the block before has left LDS

        // ---- the text, an empty table, empty counts
        if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
            const uint4* g4 = reinterpret_cast<const uint4*>(g);
            uint4* s4 = reinterpret_cast<uint4*>(s);
            for (u32 i = tid; i < n / 16; i += BZ_THREADS) s4[i] = g4[i];
            for (u32 i = (n & ~15u) + tid; i < n; i += BZ_THREADS) s[i] = g[i];
        } else {
            for (u32 i = tid; i < n; i += BZ_THREADS) s[i] = g[i];
        }
        if (tid < 16) s[n + tid] = 0;
        for (u32 i = tid; i < BZ_TAB_WORDS / 4; i += BZ_THREADS) reinterpret_cast<uint4*>(tab)[i] = make_uint4(0, 0, 0, 0);
        for (u32 i = tid; i < BZ_NLL; i += BZ_THREADS) { sm->freq_ll[i] = 0; sm->len_ll[i] = 0; sm->code_ll[i] = 0; }
        if (tid < BZ_ND) { sm->freq_d[tid] = 0; sm->len_d[tid] = 0; sm->code_d[tid] = 0; }
        if (tid == 0) { sm->crc = 0; sm->carry = 0; sm->carry_next = 0; }
        __syncthreads();

        // ---- CRC32: strips whose length in words is odd, so that the lanes of a wave read different banks (kbbq_crc32.h)
        {
            u32 lo, hi;
            crc_strip_of(n, tid, BZ_THREADS, &lo, &hi);
            if (lo < hi) atomicXor(&sm->crc, crc_strip(sm->crc_tab, sm->x2n, s, lo, hi, n));
        }

        // ---- LZ77, tile by tile
        u32 ntok = 0;
        for (u32 t0 = 0; t0 < n; t0 += BZ_TILE) {
            const u32 p = t0 + tid;
            u32 len = 1, dist = 0, h = 0;
            const bool ins = p + BZ_MIN_MATCH <= n;
            if (ins) {
                const u32 v = (u32)s[p] | ((u32)s[p + 1] << 8) | ((u32)s[p + 2] << 16) | ((u32)s[p + 3] << 24);
                h = (v * 2654435761u) >> (32 - BZ_HASH_BITS);
                const u32 c1 = tab[h];                      // position + 1 of the candidate, 0: none
                if (c1 && p - (c1 - 1) <= BZ_MAX_DIST) {
                    const u32 c = c1 - 1, most = min(BZ_MAX_MATCH, n - p);
                    u32 l = 0;
                    while (l < most && s[c + l] == s[p + l]) ++l;
                    if (l >= BZ_MIN_MATCH) { len = l; dist = p - c; }
                }
            }
            sm->jump[tid] = tid + len;
            sm->reach[tid] = (tid == sm->carry && p < n) ? 1u : 0u;
            __syncthreads();
            if (ins) atomicMax(&tab[h], p + 1);
            // the positions the parse visits: after round k every one within 2^(k+1) steps of the first is marked.  A mark
            // read in the round that sets it only marks another visited position early.
            for (u32 r = 0; r < BZ_ROUNDS; ++r) {
                const u32 j = sm->jump[tid];
                const bool inside = j < BZ_TILE && t0 + j < n;
                if (inside && sm->reach[tid]) sm->reach[j] = 1;
                const u32 j2 = inside ? sm->jump[j] : j;
                __syncthreads();
                sm->jump[tid] = j2;
                __syncthreads();
            }
            const bool is_tok = p < n && sm->reach[tid] != 0;
            if (is_tok && tid + len >= BZ_TILE) sm->carry_next = tid + len - BZ_TILE;    // the one token that leaves the tile
            u32 total;
            const u32 at = bz_scan(is_tok ? 1u : 0u, sm->wsum, &total);
            if (is_tok) {
                if (len == 1) {
                    tok[ntok + at] = s[p];
                    atomicAdd(&sm->freq_ll[s[p]], 1u);
                } else {
                    tok[ntok + at] = BZ_TOK_MATCH | ((len - 3) << 16) | (dist - 1);
                    u32 sy, eb, ev;
                    bz_len_sym(len - 3, &sy, &eb, &ev);
                    atomicAdd(&sm->freq_ll[sy], 1u);
                    bz_dist_sym(dist - 1, &sy, &eb, &ev);
                    atomicAdd(&sm->freq_d[sy], 1u);
                }
            }
            ntok += total;
            __syncthreads();
            if (tid == 0) { sm->carry = sm->carry_next; sm->carry_next = 0; }
            __syncthreads();
        }

        // ---- the two codes
        if (tid == 0) sm->freq_ll[256] = 1;                // end of block
        __syncthreads();
        if (tid < 286) bz_rank(sm->freq_ll, 286, tid, sm->key_ll, sm->sym_ll);
        else if (tid >= 320 && tid < 350) bz_rank(sm->freq_d, 30, tid - 320, sm->key_d, sm->sym_d);
        __syncthreads();
        if (tid == 0) bz_build_code(sm->freq_ll, 286, 15, sm->key_ll, sm->sym_ll, sm->cnt_ll, sm->len_ll, sm->code_ll);
        if (tid == 320) bz_build_code(sm->freq_d, 30, 15, sm->key_d, sm->sym_d, sm->cnt_d, sm->len_d, sm->code_d);
        __syncthreads();
        if (tid == 0) bz_plan_header(sm, n);
        for (u32 i = tid; i < BZ_TAB_WORDS / 4; i += BZ_THREADS) reinterpret_cast<uint4*>(tab)[i] = make_uint4(0, 0, 0, 0);
        __syncthreads();

        // ---- the block's bytes from byte 16 on, in `tab`: BSIZE - 1 | payload | CRC32 | ISIZE
        u32 payload;
        if (sm->coded) {
            const u32 body0 = 16 + sm->hdr_bits;
            if (tid == 0) bz_put_header(sm, tab, 16);
            const u32 per = (ntok + BZ_THREADS - 1) / BZ_THREADS;
            const u32 lo = min(ntok, tid * per), hi = min(ntok, lo + per);
            u32 bits = 0;
            u64 val;
            for (u32 i = lo; i < hi; ++i) bits += bz_token_bits(sm, tok[i], &val);
            u32 total;
            u32 pos = body0 + bz_scan(bits, sm->wsum, &total);
            for (u32 i = lo; i < hi; ++i) {
                const u32 nb = bz_token_bits(sm, tok[i], &val);
                bz_put(tab, pos, val, nb);
                pos += nb;
            }
            if (tid == 0) bz_put(tab, body0 + total, sm->code_ll[256], sm->len_ll[256]);
            payload = (sm->hdr_bits + sm->body_bits + 7) >> 3;
        } else {
            uint8_t* const o = reinterpret_cast<uint8_t*>(tab);
            if (tid == 0) {
                o[2] = 1;                                  // BFINAL = 1, BTYPE = 00
                o[3] = (uint8_t)n; o[4] = (uint8_t)(n >> 8); o[5] = (uint8_t)~n; o[6] = (uint8_t)(~n >> 8);
            }
            for (u32 i = tid; i < n; i += BZ_THREADS) o[7 + i] = s[i];
            payload = n + 5;
        }
        __syncthreads();
        const u32 size = 18 + payload + 8;
        if (tid == 0) {
            bz_put(tab, 0, size - 1, 16);
            bz_put(tab, 8 * (2 + payload), sm->crc, 32);
            bz_put(tab, 8 * (2 + payload) + 32, n, 32);
            q.sizes[b] = size;
        }
        __syncthreads();
        u32* const out = reinterpret_cast<u32*>(q.blocks + (size_t)b * BZ_SLOT);
        if (tid == 0) { out[0] = 0x04088b1fu; out[1] = 0; out[2] = 0x0006ff00u; out[3] = 0x00024342u; }
        for (u32 i = tid; i < (size - 16 + 3) / 4; i += BZ_THREADS) out[4 + i] = tab[i];
    }
}

// offsets[b] = sizes[0] + ... + sizes[b - 1], offsets[nblocks] = the packed length.  One workgroup.
__global__ __launch_bounds__(BZ_THREADS) void bz_scan_sizes(const u32* sizes, u32 nblocks, u64* offsets)
{
    __shared__ u64 part[BZ_THREADS];
    const u32 tid = threadIdx.x, per = (nblocks + BZ_THREADS - 1) / BZ_THREADS;
    const u32 lo = min(nblocks, tid * per), hi = min(nblocks, lo + per);
    u64 sum = 0;
    for (u32 i = lo; i < hi; ++i) sum += sizes[i];
    part[tid] = sum;
    __syncthreads();
    for (u32 d = 1; d < (u32)BZ_THREADS; d <<= 1) {
        const u64 o = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += o;
        __syncthreads();
    }
    u64 at = part[tid] - sum;
    for (u32 i = lo; i < hi; ++i) { offsets[i] = at; at += sizes[i]; }
    if (tid == BZ_THREADS - 1) offsets[nblocks] = part[tid];
}

// block b's bytes to packed + offsets[b]
__global__ __launch_bounds__(256) void bz_pack(const uint8_t* blocks, const u32* sizes, const u64* offsets, uint8_t* packed)
{
    const uint8_t* src = blocks + (size_t)blockIdx.x * BZ_SLOT;
    uint8_t* dst = packed + offsets[blockIdx.x];
    const u32 n = sizes[blockIdx.x];
    for (u32 i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
}
