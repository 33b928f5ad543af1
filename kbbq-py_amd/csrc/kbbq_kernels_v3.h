// kbbq_kernels_v3.h -- table-driven, branch-free forms of K1 and K2 (the default path).
//
// Measured on MI355X (profiles/r01_pmc_v1.md): the first kernels (kbbq_kernels.h) were bound
// by VALU issue -- ~24 (K1) / ~22 (K2) vector instructions per base at 4 cycles per wave64
// integer instruction -- not by LDS (removing every LDS op bought 7 %) and not by HBM.
// These versions move per-base decisions into table layout so that a base costs ~7 (K1) /
// ~6 (K2) vector instructions:
//   K1: no "counted?" / "context defined?" tests: the LDS histogram has a TRASH row (all
//       qualities below minscore clamp onto it with one v_max) and TRASH context slots (the
//       context index is 5*code(prev)+code(cur) with code 4 = N / no previous base, so it is
//       always in range); trash is never flushed.  Second-in-pair columns are stored
//       mirrored so that both mates walk upwards and the per-base column step is an
//       instruction immediate.
//   K2: the LUT is indexed by the RAW quality byte: row 0 (padding) yields 0, rows of
//       uncounted qualities are identity rows, so there is no clamp, no "q >= minscore"
//       test and no select; a mirrored copy of the cycle entries serves second-in-pair
//       reads with ascending addresses.
// Same read-block / 16-byte-chunk decomposition, same error semantics (rare exact paths)
// and the same C ABI as the first kernels, which remain as the fallback for shapes these
// layouts do not fit in LDS (very long reads, many read groups).
#pragma once
#include "kbbq_helpers.h"
#include <type_traits>

#define K1V3_THREADS 1024        // one workgroup per CU: the replicated context table needs ~150 KB of LDS
#define K1V3_DNREP 16            // copies of the context-count table (copy = lane & (DN - 1)); long reads use 8 to fit the LDS
#define K2V3_THREADS 512
#define K2V3_NBUF 2             // chunk buffers in the prefetch ring
#define K2V3_WAVES 4            // waves per SIMD the register allocation aims at
#define K1V3_FLUSH_ITERS 48          // 48 * 16 waves * 64 reads = 49,152 reads per workgroup between flushes (< 65,535)

struct K1v3Params {
    const uint8_t* seq; const uint8_t* cseq; const uint8_t* qual; const u32* meta;
    long long nreads; int pitch; int cpr; u32 cpr_magic; int R; int S;
    int minscore;               // counting threshold: row r of the LDS tables is quality minscore + r - 1
    int type_minscore;          // threshold of the dinucleotide lookup (TypeError rule); differs in SPLIT
    u32 qlo_m1;                 // 32 + minscore: quality bytes <= this hit the trash row
    u32 dlo;                    // SPLIT only: 33 + dinucleotide minscore
    int nrows;                  // 44 - minscore: one row per counted quality (row = 42 - q) + the trash row LAST
    u32 row_bytes;              // pos row stride in bytes ((3S | 1) words)
    u32 slack_bytes;            // after the last (trash) row: padding bytes of short reads index past its end
    int minlen;                 // rows are trimmed to 3S - minlen words: a shorter read is reported (ST_INDEX), not counted
    int dn_flush_iters;         // workgroup iterations between flushes of the (16-bit packed) context table
    int maxlen;                 // longest row the tables take: S, or 2S + 1 for mate-pair rows
    int gap;                    // mate-pair rows: 1 (the separator byte between the mates), else 0
    int twins;                  // mate-pair rows holding two FIRST-in-pair reads (single-end input packed two to a row): the second
                                // half counts into the forward columns [0, S) like the first, not into the mirrored ones
    int gS2;                    // columns of the GLOBAL cycle tables (2 x the longest read of the whole input); S may be
                                // smaller -- the longest read of THIS batch -- because a second-in-pair column
                                // 2*len-1-i does not depend on the S the LDS table is laid out for
    const long long* seg;       // rows grouped by read group: slice g owns rows [seg[g], seg[g + 1]); NULL: every slice scans all rows
    u64* tables; u64* status;
    // ALN form (aligned reads tallied in place, K6 fused into K1: see k1v3_body): seq = the reads as aligned, cseq = K4's plane of
    // flags (bit 0 error, bit 1 skip), qual = the OQ characters; per read, instead of `meta`:
    const u32* aflags;          // bit 0 reverse strand, bit 1 read 2, bits 16.. read group
    const u32* aclip;           // query_alignment_start | query_alignment_end << 16
    const u32* atrim;           // skipped range lo | hi << 16 (adaptor; lo == hi: none)
    // REF form (K4 folded in as well, for reads that are ONE M / = / X operation over all their bases): bit 2 of a read's aflags
    // word says "no plane of flags for this read: compare it with the reference here" -- cseq is then only read for the other
    // reads (k4v2_find_errors wrote their rows), and a chunk of such a read loads 16 bytes of `genome` (bit 7 of a byte: the
    // site's skip flag) at ag0[read] + its offset in the read instead
    const uint8_t* genome; const long long* ag0;
    // copies of the cycle table (1, 2 or 4; KJ == 0 forms): a chunk counts into copy (row slot & (copies - 1)), the flush sums them.
    // Narrow rows put many lanes of a wave on the same few columns (pitch 48: 21 lanes per column), i.e. onto the same (quality,
    // column) words: same-address LDS atomics serialise.  Their tables are small, so copies fit the LDS beside the context table.
    int pos_copies; u32 pos_copy_bytes;      // bytes from one copy to the next (rows + slack)
    // trash rows (1, 2, 4 or 8; KJ == 0 forms): every uncounted byte -- below minscore, and ALL the padding behind a read's last
    // base -- is binned on the trash row at its column, so the lanes of a wave that sit on the last chunk of their rows hit the same
    // few trash words over and over (a 16- to 21-way same-address atomic for narrow rows).  With several trash rows a chunk uses row
    // (row slot & (ntrash - 1)) of them: the clamp's upper bound becomes a per-chunk value, nothing is added per base.
    int ntrash;
};

// nucleotide decode of 4 bases: code (A0 T1 G2 C3, N/other 4), 5*code, and the character each
// code stands for (alphabet check), all by v_perm_b32 with the data as selector
__device__ __forceinline__ void decode4x(u32 w, u32& code, u32& code5, u32& expect)
{
    const u32 h = (w >> 1) & 0x07070707u;                                // A->0 C->1 T->2 G->3 N->7
    code   = __builtin_amdgcn_perm(0x04040404u, 0x02010300u, h);
    code5  = __builtin_amdgcn_perm(0x14141414u, 0x0A050F00u, h);         // 5 * code: A0 C15 T5 G10, N/other 20
    expect = __builtin_amdgcn_perm(0x4E000000u, 0x47544341u, h);
}

// increment of both count tables for base B of a word: errs << 16 | total = (seq byte != cseq byte) ? 0x10001 : 1.
// One sub-dword compare on byte B of xw = seq ^ cseq and one select (the compiler's own sequence masks the
// byte out first: three instructions).
template <int B>
__device__ __forceinline__ u32 k1_increment(u32 xw, u32 zero, u32 both)
{
    u32 inc;
    if (B == 0)      asm("v_cmp_ne_u32_sdwa vcc, %1, %2 src0_sel:BYTE_0 src1_sel:DWORD\n\tv_cndmask_b32_e32 %0, 1, %3, vcc" : "=v"(inc) : "v"(xw), "v"(zero), "v"(both) : "vcc");
    else if (B == 1) asm("v_cmp_ne_u32_sdwa vcc, %1, %2 src0_sel:BYTE_1 src1_sel:DWORD\n\tv_cndmask_b32_e32 %0, 1, %3, vcc" : "=v"(inc) : "v"(xw), "v"(zero), "v"(both) : "vcc");
    else if (B == 2) asm("v_cmp_ne_u32_sdwa vcc, %1, %2 src0_sel:BYTE_2 src1_sel:DWORD\n\tv_cndmask_b32_e32 %0, 1, %3, vcc" : "=v"(inc) : "v"(xw), "v"(zero), "v"(both) : "vcc");
    else             asm("v_cmp_ne_u32_sdwa vcc, %1, %2 src0_sel:BYTE_3 src1_sel:DWORD\n\tv_cndmask_b32_e32 %0, 1, %3, vcc" : "=v"(inc) : "v"(xw), "v"(zero), "v"(both) : "vcc");
    return inc;
}

// The uniform-block loop of the joint-row forms (k1v3_body, KJ > 0) bins a base in five vector instructions; these are the three
// that work on a part of a register (SDWA), B the base's byte in its word:
// row of the tables: min(byte B of qn = 255 - quality, tcl)
template <int B>
__device__ __forceinline__ u32 k1_joint_row(u32 qn, u32 tcl)
{
    u32 tq;
    if (B == 0)      asm("v_min_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(tq) : "v"(qn), "v"(tcl));
    else if (B == 1) asm("v_min_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(tq) : "v"(qn), "v"(tcl));
    else if (B == 2) asm("v_min_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(tq) : "v"(qn), "v"(tcl));
    else             asm("v_min_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(tq) : "v"(qn), "v"(tcl));
    return tq;
}
// increment of both count tables, errs << 16 | total: the HIGH half of `inc` becomes min(byte B of xw, 1) -- xw = seq ^ cseq on codes,
// a byte of it is 0..7 -- and the low half keeps the 1 it was given.
template <int B>
__device__ __forceinline__ void k1_joint_increment(u32& inc, u32 xw, u32 one)
{
    if (B == 0)      asm("v_min_u32_sdwa %0, %1, %2 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_0 src1_sel:DWORD" : "+v"(inc) : "v"(xw), "v"(one));
    else if (B == 1) asm("v_min_u32_sdwa %0, %1, %2 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1 src1_sel:DWORD" : "+v"(inc) : "v"(xw), "v"(one));
    else if (B == 2) asm("v_min_u32_sdwa %0, %1, %2 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_2 src1_sel:DWORD" : "+v"(inc) : "v"(xw), "v"(one));
    else             asm("v_min_u32_sdwa %0, %1, %2 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_3 src1_sel:DWORD" : "+v"(inc) : "v"(xw), "v"(one));
}
// (x << 6) + y in one instruction (the compiler moves a mask of x behind its own shift and then needs three)
__device__ __forceinline__ u32 k1_shl6_add(u32 x, u32 y)
{
    u32 r;
    asm("v_lshl_add_u32 %0, %1, 6, %2" : "=v"(r) : "v"(x), "v"(y));
    return r;
}
// address of the context word: the cycle word's plus 16-bit half H of e
template <int H>
__device__ __forceinline__ u32 k1_joint_delta(u32 a, u32 e)
{
    u32 ad;
    if (H == 0) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(ad) : "v"(a), "v"(e));
    else        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(ad) : "v"(a), "v"(e));
    return ad;
}


// ---- 4-bit sequence planes ("packed" layouts) ------------------------------------------------
// A seq / cseq plane may hold one NIBBLE per base instead of one character: the nucleotide code itself
// (A0 T1 G2 C3, compare_reads.py:199; 4 = N, the separator and the padding), 8 bytes per 16-base chunk, row
// stride pitch / 2.  Word w of a chunk (w = 0, 1) carries bases 8w .. 8w+3 in the LOW nibbles of its four bytes and
// bases 8w+4 .. 8w+7 in the HIGH nibbles, so that `w & 0x0F0F0F0F` and `(w >> 4) & 0x0F0F0F0F` are the codes of four
// consecutive bases as bytes -- the form the per-base code below (and the quality words) use.  Only reads whose
// seq AND cseq are entirely ACGTN can be packed (k7_lay_out reports anything else and the caller keeps the
// byte planes, which carry the reference's exact TypeError semantics); the comparison of A1
// (recalibrate.py:13-20) is then a comparison of codes.  HBM traffic: K1 2 B/base instead of 3, K2 2.5 instead of 3.
#define NIBM 0x0F0F0F0Fu
__device__ __forceinline__ u32 nib_lo(u32 w) { return w & NIBM; }
__device__ __forceinline__ u32 nib_hi(u32 w) { return (w >> 4) & NIBM; }
// some nibble of w is not a code (>= 5)
__device__ __forceinline__ u32 nib_invalid(u32 w) { return (((w & 0x77777777u) + 0x33333333u) | w) & 0x88888888u; }
// KBBQ_ROWS_ERRBIT planes (EB; 4-bit mate-pair rows of 19 / 13 chunks only): bits 0-2 of a seq nibble are the code, bit 3 is set
// exactly where the corrected read's code differs -- all K1 ever took from the cseq plane (xw = seq ^ cseq, then min(byte, 1)), so
// K1 does not load that plane at all (1.57 B/base instead of 2.08) and K2 masks the bit away.  `w & 0x08080808` / `w & 0x80808080`
// are the error bytes of the low / high nibbles as they stand: a byte of them is 0 or not, which is all the increment asks.
// Without EB every function below is the expression it replaces.
#define NIBM3 0x07070707u
template <bool EB> __device__ __forceinline__ u32 nib_lo_code(u32 w) { return w & (EB ? NIBM3 : NIBM); }
template <bool EB> __device__ __forceinline__ u32 nib_hi_code(u32 w) { return (w >> 4) & (EB ? NIBM3 : NIBM); }
template <bool EB> __device__ __forceinline__ u32 nib_bad(u32 w)
{
    if constexpr (EB) return ((w & 0x77777777u) + 0x33333333u) & 0x88888888u;       // the low three bits are 5..7
    else return nib_invalid(w);
}
// 4 characters -> 4 codes as bytes (0..4), and whether all four are in ACGTN
__device__ __forceinline__ u32 chars_to_codes(u32 w, u32& bad)
{
    const u32 h = (w >> 1) & 0x07070707u;
    bad |= __builtin_amdgcn_perm(0x4E000000u, 0x47544341u, h) ^ w;
    return __builtin_amdgcn_perm(0x04040404u, 0x02010300u, h);
}
// 4 codes as bytes -> their characters
__device__ __forceinline__ u32 codes_to_chars(u32 c) { return __builtin_amdgcn_perm(0x4E4E4E4Eu, 0x43475441u, c & 0x07070707u); }

// 0x01 in every byte of x that is non-zero
__device__ __forceinline__ u32 nonzero_bytes(u32 x)
{
    return ((x | ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) >> 7) & 0x01010101u;
}

// 16 bytes starting at ANY byte offset: one global_load_dwordx4 with an unaligned address (the
// amdhsa targets run with unaligned access mode on; the compiler itself emits this for a
// 1-byte-aligned 16-byte copy).  The caller guarantees the 16 bytes are readable.
__device__ __forceinline__ void load16_any(const uint8_t* base, long long off, u32 out[4])
{
    uint4 v;
    __builtin_memcpy(&v, base + off, 16);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
}

__device__ __forceinline__ void reverse16(u32 v[4])                      // byte i <- byte 15 - i
{
    const u32 a0 = v[0], a1 = v[1], a2 = v[2], a3 = v[3];
    v[0] = __builtin_amdgcn_perm(0u, a3, 0x00010203u); v[1] = __builtin_amdgcn_perm(0u, a2, 0x00010203u);
    v[2] = __builtin_amdgcn_perm(0u, a1, 0x00010203u); v[3] = __builtin_amdgcn_perm(0u, a0, 0x00010203u);
}

typedef __attribute__((address_space(3))) u32 lds_u32;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;

struct K1Chunk { u32 s[4], c[4], q[4]; u32 mk; u32 off; int k; int j; int nb; u32 fl, clip, trim; int jj; u32 g0lo, g0hi; };

// LDS: dn [nrows][32][16] u32 context counts (errs << 16 | total), 16 copies (copy = lane & 15:
//          the table is tiny and hot -- measured 15 LDS cycles per wave-atomic unreplicated --
//          copies cut the bank and same-address collisions), slot = 5*code(prev)+code(cur).
//          16-bit halves: a copy can receive 64 lanes x 16*cpr bases per workgroup iteration in
//          the worst case (every base the same bin), so this table alone is flushed every
//          dn_flush_iters = 65535 / (1024 * cpr) iterations: 6 for 150-base reads one to a row (10 chunks), 3 for their
//          mate-pair rows (19 chunks: ~32 flushes per workgroup on the headline, about 2 % of K1 before the joint-row forms
//          got a flush of their own, profiles/r10_k1_block_pipeline.md), 4 for 13-chunk rows.
//      pos[nrows][row_bytes/4] u32 (errs << 16 | total): [0,S) first-in-pair cycle = position;
//          [S, 3S) second-in-pair, index x = position + 2*(S - len)  <->  column 2S-1-x
//      rows are ordered by the INVERTED quality byte (row = 42 - q, one v_min clamps every
//      uncounted byte onto the trash row, which is last); bytes past the end of a short read
//      (quality 0 -> trash) can index beyond the trash row's end: `slack_bytes` absorb that.
// KJ > 0 (mate-pair rows of exactly KJ chunks): the cycle table is laid out CHUNK-POSITION MAJOR -- position 16 j + k of
// a row lives in word k * KJ + j of a table row whose stride is a multiple of 32 words.  The bank of a lane's atomic is
// then (k * KJ + j) mod 32 whatever its quality: for the 16-base unroll's fixed k, lanes of one row hit DIFFERENT banks
// (only the lanes of the next row, 19 chunks on, meet them again: 2 LDS cycles per half-wave), where the
// position-major layout lets the random quality row pick the bank (a 32-lane half-wave on 32 banks: ~3.5 cycles).
// These forms keep `dn` and `pos` in JOINT rows: row r = [pos row r: CYC words | dn row r: 32 x 16 words], 832 (KJ = 19) / 736
// (13) words, multiples of 32 like CYC itself, so both tables keep their banks and a base's two addresses share the row term.
// Measured (profiles/r02_k1_lds.md): the cycle-table atomics were the larger half of K1's LDS time once the 4-bit
// sequence planes had made K1 LDS-bound.  The per-base offset 4 * k * KJ is an instruction immediate.
// The kernel's body: workgroup `bx` of the `gx` that share this batch (k1v3_accumulate: the whole grid; k1v3_bands: the
// workgroups one length band was given), read-group slice `g`.
// ALN (K6 fused into K1, gatk/bqsr.py:52-123 in one pass over the aligned reads instead of K6 writing canonical reads for K1 to
// read back): the lane's chunk is 16 bytes of the read AS ALIGNED -- for a reverse-strand read the chunks are taken last to
// first and byte-reversed in registers, bases complemented on their codes (A0 T1 G2 C3: code ^ 1), so that lane order and
// byte order are sequencing order for either strand and everything below the prologue is the FASTQ kernel's: canonical
// position c = i - qs (forward) or qe - 1 - i (reverse) is the cycle, read 2 takes the mirrored columns, the previous base
// in sequencing order gives the context.  A base is uncounted (quality byte 0 -> trash row) outside the aligned part
// [qs, qe), inside the trimmed range, where K4 set the skip flag or where it is N (bqsr.py:86-88); bases outside the
// aligned part are no context either (code 4).  The error flag is K4's bit 0.  A forward read with a letter outside ACGTN
// is reported (ST_LUT): the caller repeats the tally through K6's character planes, where the reference's TypeError is decided.
// (The stages below -- the two flushes, the compaction, fetch, the decoders, the binning loop -- are lambdas over the body's
//  locals and stay so for now: written as __forceinline__ functions over explicit state, even the two flushes alone, every one
//  of the 24 instances came out with other instructions and other register counts (profiles/r06_kernel_headers.md section 4).
//  Cutting them out is a change to measure on the device, not one to make under "identical device code".)
template <bool SPLIT, int DN, bool NIB, int KJ, bool ALN = false, bool REF = false, bool EB = false>
__device__ __forceinline__ void k1v3_body(const K1v3Params& p, u32* lds, const int bx, const int gx, const int g)
{
    static_assert(!ALN || (!NIB && KJ == 0), "the aligned-read form reads character planes");
    static_assert(!REF || ALN, "the reference comparison belongs to the aligned-read form");
    static_assert(!EB || (NIB && KJ > 0), "the error bit lives in the 4-bit mate-pair rows of the joint-row forms");
    // KJ > 0: JOINT rows -- a quality's cycle words and its context words in ONE row of JROW bytes, [CYC cycle words | 32 slots x DN
    // copies], so that one multiply by the row serves both atomics of a base (the uniform-block loop below).  CYC and JROW / 4 are multiples
    // of 32: the bank of a cycle word stays (k * KJ + j) mod 32 and that of a context word (slot * DN + copy) mod 32 whatever the row.
    constexpr bool JOINT = KJ > 0;
    constexpr int CYC = (16 * KJ + 31) & ~31;
    constexpr u32 JROW = (u32)(CYC + 32 * DN) * 4u;
    static_assert(!JOINT || (NIB && DN == 16), "joint rows: 4-bit planes, 64 bytes per context slot");
    const int ntrash = p.ntrash;                       // (the host gives the 19-chunk form one trash row: several were measured, nothing)
    const int dn_words = JOINT ? 0 : (p.nrows - 1 + ntrash) * 32 * DN;
    const int ncopies = KJ > 0 ? 1 : p.pos_copies;
    const int pos_words = KJ > 0 ? (p.nrows - 1 + ntrash) * (int)(JROW >> 2) : ncopies * (int)(p.pos_copy_bytes >> 2);
    u32* dnt = JOINT ? lds + CYC : lds;
    u32* pos = lds + dn_words;
    for (int i = threadIdx.x; i < dn_words + pos_words; i += blockDim.x) lds[i] = 0u;
    __syncthreads();

    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform: block bases live in SGPRs
    const int nwaves = blockDim.x >> 6;
    // rows grouped by read group: this slice's rows are contiguous (every lane useful, no compaction)
    const long long seg_lo = p.seg ? p.seg[g] : 0ll, seg_hi = p.seg ? p.seg[g + 1] : p.nreads;
    const long long nblocks = (seg_hi - seg_lo + 63) >> 6;
    const long long iters = (nblocks + nwaves - 1) / nwaves;
    const int S = p.S, S2 = 2 * p.S;
    const u32 row_bytes = JOINT ? JROW : p.row_bytes;
    const u32 tclamp = 255u - p.qlo_m1;                                // inverted bytes >= this are uncounted
    const u32 pos_base = (u32)dn_words * 4u - 180u * row_bytes;        // 180 = 255 - 'K': inverted byte of q = 42 is row 0
    const u32 dnt_row = JOINT ? JROW : 128u * DN;              // bytes per row of the replicated totals
    // LDS byte address (the low half of the flat address is the LDS offset) of this lane's copy, less the row bias
    const u32 dnt_base = (u32)reinterpret_cast<size_t>(lds) - 180u * dnt_row + 4u * (u32)(lane_id() & (DN - 1)) + (JOINT ? 4u * CYC : 0u);
    int since_flush = 0, since_dn_flush = 0;
    // work item of this lane at step 0 and the per-step advances (64 / 128 items)
    const int lane_k0 = p.cpr == 1 ? lane : (int)__umulhi((u32)lane, p.cpr_magic);
    const int lane_j0 = lane - lane_k0 * p.cpr;
    const int dk1 = 64 / p.cpr, dj1 = 64 - dk1 * p.cpr;
    const int dk2 = 128 / p.cpr, dj2 = 128 - dk2 * p.cpr;

    u64* pos_errs = p.tables;
    u64* pos_total = p.tables + (size_t)p.R * KQ * p.gS2;
    u64* dn_errs = p.tables + 2 * (size_t)p.R * KQ * p.gS2;
    u64* dn_total = dn_errs + (size_t)p.R * KQ * KND;

    auto flush_dn = [&]() {
        if constexpr (JOINT) {
            // One bin per thread -- thread t: row t / 16, context (t / 4) % 4 then t % 4 -- so no thread has a second bin whose LDS
            // reads would queue behind the first one's global atomics: 16 copies read and zeroed, then at most two atomics that
            // nothing waits for (the tables are read after the kernel).  At most 43 rows: 688 of the 1024 threads.
            static_assert(K1V3_THREADS >= 16 * KQ, "one thread per bin of the context table");
            const int t = (int)threadIdx.x, r = t >> 4;
            if (r < p.nrows - 1) {                                     // the last row is trash
                const int a = (t >> 2) & 3, b = t & 3;
                lds_u32x4* at = reinterpret_cast<lds_u32x4*>((u32)reinterpret_cast<size_t>(lds) + 4u * (u32)(r * (int)(JROW >> 2) + CYC + (5 * a + b) * DN));
                u32 vt = 0u, ve = 0u;
#pragma unroll
                for (int i = 0; i < DN / 4; ++i) {
                    // four copies to a 16-byte read.  The 16 threads of a row start on different quarters: their bins are 16 or 80
                    // words apart, so that the same quarter everywhere would put them all on the same 8 banks
                    const int qu = (i + t) & 3;
                    const u32x4 v = at[qu];
                    at[qu] = u32x4{0u, 0u, 0u, 0u};
                    vt += (v.x & 0xFFFFu) + (v.y & 0xFFFFu) + (v.z & 0xFFFFu) + (v.w & 0xFFFFu);
                    ve += (v.x >> 16) + (v.y >> 16) + (v.z >> 16) + (v.w >> 16);
                }
                if (vt) {
                    const size_t e = ((size_t)g * KQ + (KQ - 1 - r)) * KND + 4 * a + b;
                    atomicAdd(&dn_total[e], (u64)vt);
                    if (ve) atomicAdd(&dn_errs[e], (u64)ve);
                }
            }
            return;
        }
        for (int r = wave; r < p.nrows - 1; r += nwaves) {           // the last row is trash
            const int q = KQ - 1 - r;
            if (lane < 25) {
                const int a = lane / 5, b = lane - 5 * a;
                if (a < 4 && b < 4) {
                    u32 vt = 0u, ve = 0u;
                    const int at = JOINT ? r * (int)(JROW >> 2) + lane * DN : (r * 32 + lane) * DN;
                    for (int cpy = 0; cpy < DN; ++cpy) {
                        const u32 v = dnt[at + cpy];
                        dnt[at + cpy] = 0u;
                        vt += v & 0xFFFFu; ve += v >> 16;
                    }
                    if (vt) {
                        const size_t e = ((size_t)g * KQ + q) * KND + 4 * a + b;
                        atomicAdd(&dn_total[e], (u64)vt);
                        if (ve) atomicAdd(&dn_errs[e], (u64)ve);
                    }
                }
            }
        }
    };
    auto flush_pos = [&]() {
        for (int r = wave; r < p.nrows - 1; r += nwaves) {
            const int q = KQ - 1 - r;
            const size_t grow = ((size_t)g * KQ + q) * p.gS2;
            u32* prow = pos + (size_t)r * (row_bytes >> 2);
            if (KJ > 0) {
                for (int x = lane; x < 16 * KJ; x += 64) {
                    const u32 v = prow[x];
                    if (v) {
                        prow[x] = 0u;
                        const int k = x / KJ, j = x - k * KJ, at = 16 * j + k;       // byte offset within the mate-pair row
                        if (at == S || at > S2) continue;                           // separator / padding: never counted
                        const int col = at < S ? at : (p.twins ? at - S - 1 : S2 - 1 - (at - S - 1));
                        atomicAdd(&pos_total[grow + col], (u64)(v & 0xFFFFu));
                        if (v >> 16) atomicAdd(&pos_errs[grow + col], (u64)(v >> 16));
                    }
                }
                continue;
            }
            for (int x = lane; x < 3 * S - p.minlen; x += 64) {
                u32 v = prow[x];
                if (ncopies > 1) {                                            // sum the copies (16-bit halves apart: they are counts)
                    u32 vt = v & 0xFFFFu, ve = v >> 16;
                    for (int cpy = 1; cpy < ncopies; ++cpy) {
                        u32* q = prow + (size_t)cpy * (p.pos_copy_bytes >> 2);
                        const u32 w = q[x];
                        if (w) { q[x] = 0u; vt += w & 0xFFFFu; ve += w >> 16; }
                    }
                    if (vt | ve) {
                        prow[x] = 0u;
                        if (p.gap && x == S) continue;
                        const int col = x < S ? x : (p.twins ? x - S - p.gap : S2 - 1 - (x - S - p.gap));
                        atomicAdd(&pos_total[grow + col], (u64)vt);
                        if (ve) atomicAdd(&pos_errs[grow + col], (u64)ve);
                    }
                    continue;
                }
                if (v) {
                    prow[x] = 0u;
                    if (p.gap && x == S) continue;                            // the separator byte of a mate-pair row is never counted
                    const int col = x < S ? x : (p.twins ? x - S - p.gap : S2 - 1 - (x - S - p.gap));
                    atomicAdd(&pos_total[grow + col], (u64)(v & 0xFFFFu));
                    if (v >> 16) atomicAdd(&pos_errs[grow + col], (u64)(v >> 16));
                }
            }
        }
    };

    // (every XCD's workgroups walking a contiguous eighth of the rows instead of every eighth iteration: measured, four alternating
    //  rounds on the headline layout, 3.40-3.44 against 3.36-3.43 ms -- nothing; K2's short-lived tiles do gain from it, kbbq_k2_tile.h)
    // Joint-row forms: ONE software pipeline across uniform blocks.  While the last step of a uniform block is binned, the wave
    // already has in flight the sidecar words of its next block (`m_next`) and that block's step-0 loads (`ub`: in a uniform
    // block they are 16 l bytes from the block's base whatever the sidecar says); the ballot on `m_next` then decides whether
    // the step is used (uniform again) or dropped (the general loop starts over from the sidecar words).  The loads stay in
    // flight across a flush of the context table, which touches neither.
    // INVARIANT: the next block is prefetched only if its 64 rows lie wholly inside [seg_lo, seg_hi) -- no address outside the
    // slice's rows is ever formed; where there is no such block the loads re-read the CURRENT block's step 0 (a uniform block:
    // 64 rows inside the slice) and are dropped, so that their number does not depend on a branch.
    K1Chunk ua, ub;
    u32 m_next = 0u;
    bool ahead = false;                                 // wave-uniform: m_next / ub belong to this wave's block of the next iteration
    for (long long it = bx; it < iters; it += gx) {
        const long long blk = it * nwaves + wave;
        if (blk < nblocks) {
            const long long read0 = seg_lo + (blk << 6);
            const long long myread = read0 + lane;
            u32 m, afl = 0u, aclip = 0u, atrim = 0u, ag0lo = 0u, ag0hi = 0u;
            const bool fed = JOINT && ahead;        // this block's sidecar words and step 0 are on their way
            if constexpr (ALN) {
                afl = myread < seg_hi ? p.aflags[myread] : 0u;
                aclip = myread < seg_hi ? p.aclip[myread] : 0u;
                atrim = myread < seg_hi ? p.atrim[myread] : 0u;
                if constexpr (REF) {
                    const long long g0 = myread < seg_hi ? p.ag0[myread] : 0ll;
                    ag0lo = (u32)g0; ag0hi = (u32)((u64)g0 >> 32);
                }
                m = myread < seg_hi ? ((u32)p.S | ((afl >> 16) << 16) | ((afl & 2u) << 30)) : 0u;     // every read has the common length S
            } else if (fed) {
                m = m_next;
            } else {
                m = myread < seg_hi ? p.meta[myread] : 0u;
            }
            ahead = false;
            const bool match = myread < seg_hi && (int)((m >> 16) & 0x7FFFu) == g && (m & 0xFFFFu) != 0u;
            const u64 mask = __ballot(match);
            const int n = __popcll(mask);
            u32 cm = m, coff = (u32)lane;
            if (n != 64 && n > 0) {            // compact the matching reads to lanes 0..n-1
                const int rank = __popcll(mask & ((1ull << lane) - 1ull));
                const int dst = match ? rank : 63;
                cm = (u32)__builtin_amdgcn_ds_permute(dst << 2, (int)(match ? m : 0u));
                coff = (u32)__builtin_amdgcn_ds_permute(dst << 2, (int)(match ? (u32)lane : 0u));
                if constexpr (ALN) {
                    afl = (u32)__builtin_amdgcn_ds_permute(dst << 2, (int)(match ? afl : 0u));
                    aclip = (u32)__builtin_amdgcn_ds_permute(dst << 2, (int)(match ? aclip : 0u));
                    atrim = (u32)__builtin_amdgcn_ds_permute(dst << 2, (int)(match ? atrim : 0u));
                    if constexpr (REF) {
                        ag0lo = (u32)__builtin_amdgcn_ds_permute(dst << 2, (int)(match ? ag0lo : 0u));
                        ag0hi = (u32)__builtin_amdgcn_ds_permute(dst << 2, (int)(match ? ag0hi : 0u));
                    }
                }
            }
            const uint8_t* bseq = p.seq + (size_t)read0 * (NIB ? p.pitch >> 1 : p.pitch);
            const uint8_t* bcseq = EB ? nullptr : p.cseq + (size_t)read0 * (NIB ? p.pitch >> 1 : p.pitch);     // EB: no cseq address is formed
            const uint8_t* bqual = p.qual + (size_t)read0 * p.pitch;
            const int total = n * p.cpr;
            u32 carry_code = 20u, carry_char = 0u;      // 5 * code of the previous chunk's last base

            // fetch: issue the three 16-byte loads of one step (no wait); process: bin them.
            // The loop below keeps one step in flight while the previous one is binned.
            // (k, j) = (read slot, chunk) of the lane's work item; advanced incrementally.
            auto advance = [&](K1Chunk& ch, int dk, int dj) {
                const int jj = ch.j + dj;
                const bool wrap = jj >= p.cpr;
                ch.j = wrap ? jj - p.cpr : jj;
                ch.k = ch.k + dk + (wrap ? 1 : 0);
            };
            auto fetch = [&](K1Chunk& ch) {
                const bool act0 = ch.k < n;
                const int k = act0 ? ch.k : 0;
                ch.mk = bperm(cm, k);
                ch.off = n == 64 ? (u32)k : bperm(coff, k);
                ch.nb = act0 ? ((int)(ch.mk & 0xFFFFu) - 16 * ch.j) : 0;
                ch.jj = ch.j;
                if constexpr (ALN) {
                    ch.fl = bperm(afl, k); ch.clip = bperm(aclip, k); ch.trim = bperm(atrim, k);
                    if (ch.fl & 1u) ch.jj = p.cpr - 1 - ch.j;          // a reverse-strand read: its chunks last to first
                    if constexpr (REF) { ch.g0lo = bperm(ag0lo, k); ch.g0hi = bperm(ag0hi, k); }
                }
                // lanes without work re-read the block's first chunk (valid memory, result unused)
                const u32 rowoff = ch.nb > 0 ? __umul24(ch.off, (u32)p.pitch) + (u32)(16 * ch.jj) : 0u;
                if constexpr (EB) {
                    const uint2 sv = *reinterpret_cast<const uint2*>(bseq + (rowoff >> 1));
                    ch.s[0] = sv.x; ch.s[1] = sv.y;
                } else if constexpr (NIB) {
                    const uint2 sv = *reinterpret_cast<const uint2*>(bseq + (rowoff >> 1));
                    const uint2 cv = *reinterpret_cast<const uint2*>(bcseq + (rowoff >> 1));
                    ch.s[0] = sv.x; ch.s[1] = sv.y; ch.c[0] = cv.x; ch.c[1] = cv.y;
                } else if constexpr (REF) {
                    // a one-operation read: the chunk's reference window (any byte offset) instead of its row of K4's flags --
                    // ONE unconditional 16-byte load from whichever address applies (a load under a branch would be waited for
                    // at the branch's end)
                    const uint4 sv = *reinterpret_cast<const uint4*>(bseq + rowoff);
                    const bool inref = ch.nb > 0 && (ch.fl & 4u) != 0u;
                    const long long g0 = (long long)(((u64)ch.g0hi << 32) | (u64)ch.g0lo);
                    const uint8_t* src = inref ? p.genome + g0 + 16 * ch.jj : bcseq + rowoff;
                    load16_any(src, 0, ch.c);
                    ch.s[0] = sv.x; ch.s[1] = sv.y; ch.s[2] = sv.z; ch.s[3] = sv.w;
                } else {
                    const uint4 sv = *reinterpret_cast<const uint4*>(bseq + rowoff);
                    const uint4 cv = *reinterpret_cast<const uint4*>(bcseq + rowoff);
                    ch.s[0] = sv.x; ch.s[1] = sv.y; ch.s[2] = sv.z; ch.s[3] = sv.w;
                    ch.c[0] = cv.x; ch.c[1] = cv.y; ch.c[2] = cv.z; ch.c[3] = cv.w;
                }
                const uint4 qv = *reinterpret_cast<const uint4*>(bqual + rowoff);
                ch.q[0] = qv.x; ch.q[1] = qv.y; ch.q[2] = qv.z; ch.q[3] = qv.w;
            };
            auto process = [&](const K1Chunk& ch) {
                const int j = ch.j, nb = ch.nb;
                const bool act = nb > 0;
                const int len = (int)(ch.mk & 0xFFFFu);
                const bool second = (ch.mk >> 31) != 0u;
                const int pos0 = 16 * j;
                // byte-parallel decode; alphabet and q-range screening (no byte masks: bytes past
                // the read are 'N' in seq/cseq and 0 in qual by the layout contract; anything else
                // only costs a visit to the exact checker)
                u32 code[4], code5[4], xw[4], qv[4], badbits = 0u, hiq = 0u;
                int c0 = pos0;                       // canonical position (= cycle) of the chunk's byte 0
                if constexpr (ALN) {
                    // the prologue of the aligned-read form (see above): from 16 bytes of the read as aligned to codes, error
                    // flags and qualities in sequencing order
                    const bool rev = (ch.fl & 1u) != 0u;
                    const int qs = (int)(ch.clip & 0xFFFFu), qe = (int)(ch.clip >> 16);
                    const int tlo = (int)(ch.trim & 0xFFFFu), thi = (int)(ch.trim >> 16);
                    const int i0 = 16 * ch.jj;                                       // position in the read of the loaded byte 0
                    auto bits = [](int lo, int hi) -> u32 {                          // bit b set for lo <= b < hi, 0 <= b < 16
                        lo = lo < 0 ? 0 : (lo > 16 ? 16 : lo); hi = hi < 0 ? 0 : (hi > 16 ? 16 : hi);
                        return hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
                    };
                    u32 aligned = bits(qs - i0, qe - i0);                            // inside the aligned part
                    u32 counted = aligned & ~bits(tlo - i0, thi - i0);               // ... and not trimmed away (adaptor)
                    u32 sv[4] = {ch.s[0], ch.s[1], ch.s[2], ch.s[3]}, fv[4] = {ch.c[0], ch.c[1], ch.c[2], ch.c[3]};
                    u32 ov[4] = {ch.q[0], ch.q[1], ch.q[2], ch.q[3]};
                    if constexpr (REF) {
                        // compare_reads.py:109-114 for a chunk inside the read's one M / = / X operation, as k4v2_find_errors' plain
                        // path makes them: error = read byte != reference byte, skip = the site's flag (bit 7 of the reference byte)
                        if (ch.fl & 4u) {
#pragma unroll
                            for (int wd = 0; wd < 4; ++wd)
                                fv[wd] = nonzero_bytes(sv[wd] ^ (fv[wd] & 0x7F7F7F7Fu)) | ((fv[wd] >> 6) & 0x02020202u);
                        }
                    }
                    if (rev) {
                        reverse16(sv); reverse16(fv); reverse16(ov);
                        aligned = __brev(aligned) >> 16; counted = __brev(counted) >> 16;
                    }
                    c0 = rev ? qe - i0 - 16 : i0 - qs;
                    const u32 rev1 = rev ? 0x01010101u : 0u;
#pragma unroll
                    for (int wd = 0; wd < 4; ++wd) {
                        const u32 am = (((aligned >> (4 * wd)) & 0xFu) * 0x00204081u & 0x01010101u) * 0xFFu;    // 4 bits -> 4 byte masks
                        const u32 cm_ = (((counted >> (4 * wd)) & 0xFu) * 0x00204081u & 0x01010101u) * 0xFFu;
                        u32 cd, cd5, expect;
                        decode4x(sv[wd], cd, cd5, expect);
                        const u32 odd = nonzero_bytes(expect ^ sv[wd]) * 0xFFu;      // letters that are none of ACGTN
                        badbits |= rev ? 0u : (odd & am);                            // a forward read keeps its letters: all must be ACGTN
                        cd = (cd & ~odd) | (0x04040404u & odd);                      // reverse strand: complement.get(x, 'N') (bqsr.py:43-45)
                        const u32 not_n = nonzero_bytes(sv[wd] ^ 0x4E4E4E4Eu);       // bqsr.py:86-88: an N is skipped
                        const u32 skipped = ((fv[wd] >> 1) & 0x01010101u) | (not_n ^ 0x01010101u);
                        cd ^= (~cd >> 2) & rev1;                                     // complement on codes (A0 T1 G2 C3; 4 stays 4)
                        cd = (cd & am) | (0x04040404u & ~am);                        // outside the aligned part: no base, no context
                        code[wd] = cd; code5[wd] = (cd << 2) + cd;
                        xw[wd] = fv[wd] & 0x01010101u;                               // K4's error flag
                        qv[wd] = ov[wd] & cm_ & ~(skipped * 0xFFu);
                    }
                } else {
                    qv[0] = ch.q[0]; qv[1] = ch.q[1]; qv[2] = ch.q[2]; qv[3] = ch.q[3];
                }
                if constexpr (EB) {
                    code[0] = nib_lo_code<true>(ch.s[0]); code[1] = nib_hi_code<true>(ch.s[0]);
                    code[2] = nib_lo_code<true>(ch.s[1]); code[3] = nib_hi_code<true>(ch.s[1]);
                    xw[0] = ch.s[0] & 0x08080808u; xw[1] = ch.s[0] & 0x80808080u;    // recalibrate.py:13-20: the packer compared the codes
                    xw[2] = ch.s[1] & 0x08080808u; xw[3] = ch.s[1] & 0x80808080u;
                    badbits = nib_bad<true>(ch.s[0]) | nib_bad<true>(ch.s[1]);
                } else if constexpr (NIB) {
                    code[0] = nib_lo(ch.s[0]); code[1] = nib_hi(ch.s[0]); code[2] = nib_lo(ch.s[1]); code[3] = nib_hi(ch.s[1]);
                    const u32 x0 = ch.s[0] ^ ch.c[0], x1 = ch.s[1] ^ ch.c[1];        // recalibrate.py:13-20 on codes
                    xw[0] = nib_lo(x0); xw[1] = nib_hi(x0); xw[2] = nib_lo(x1); xw[3] = nib_hi(x1);
                    badbits = nib_invalid(ch.s[0]) | nib_invalid(ch.s[1]);          // not a plane k7_lay_out wrote
                }
#pragma unroll
                for (int wd = 0; wd < 4; ++wd) {
                    if constexpr (NIB) {
                        code5[wd] = (code[wd] << 2) + code[wd];
                    } else if constexpr (!ALN) {
                        u32 expect;
                        decode4x(ch.s[wd], code[wd], code5[wd], expect);
                        badbits |= expect ^ ch.s[wd];
                        xw[wd] = ch.s[wd] ^ ch.c[wd];
                    }
                    hiq |= (qv[wd] + 0x34343434u) | qv[wd];                          // bit 7 of a byte: q > 42
                }
                hiq &= 0x80808080u;
                const u32 last_code5 = code5[3] >> 24;
                u32 prev_code5 = wave_shr1(last_code5, carry_code);
                carry_code = (u32)__builtin_amdgcn_readlane((int)last_code5, 63);
                u32 prev_char = 0u;
                if constexpr (!NIB && !ALN) {
                    const u32 last_char = ch.s[3] >> 24;
                    prev_char = wave_shr1(last_char, carry_char);
                    carry_char = (u32)__builtin_amdgcn_readlane((int)last_char, 63);
                }
                if (j == 0) { prev_code5 = 20u; prev_char = 0u; }                    // dinuc[0] = -1
                if (act) {
                    const long long read = read0 + ch.off;
                    const bool fits_tables = (u32)(len - p.minlen) <= (u32)(p.maxlen - p.minlen);
                    if (hiq || !fits_tables) flag(p.status, ST_INDEX, read);         // recalibrate.py:114-115; read longer (shorter) than the tables
                    if constexpr (NIB || ALN) {
                        if (badbits) flag(p.status, ST_LUT, 0);                      // the caller must use byte planes (ALN: K6's character planes)
                    } else {
                        if (badbits && chunk_type_error(ch.s[0], ch.s[1], ch.s[2], ch.s[3], ch.q[0], ch.q[1], ch.q[2], ch.q[3],
                                                        prev_char, nb, pos0, p.type_minscore))
                            flag(p.status, ST_TYPE, read);                           // compare_reads.py:224,292
                    }
                    if (!hiq && fits_tables && !((NIB || ALN) && badbits)) {
                        // A: pos address less the row term; both mates ascend with the base index
                        const u32 half = second ? (u32)(S + 2 * (S - len)) : 0u;     // column 2*len-1-pos
                        const u32 copy_off = KJ > 0 ? 0u : (u32)(ch.k & (ncopies - 1)) * p.pos_copy_bytes;     // this chunk's copy of the cycle table
                        const u32 tcl = tclamp + (u32)(ch.k & (ntrash - 1));                                   // ... and its trash row
                        const u32 A = KJ > 0 ? pos_base + 4u * (u32)j : pos_base + copy_off + (half + (u32)pos0) * 4u;
                        // ALN: bases before the aligned part have NEGATIVE canonical positions.  They are uncounted, i.e. they land on
                        // the trash row (the last one) -- up to 15 words before its start when the chunk holds the first aligned
                        // base: the tail of the row before it, which this form never uses and never flushes (every read has length S:
                        // columns < 2S + 16 of 3S words; the host sets minlen = S, the flush stops at 2S) as long as S >= 32 (the host
                        // sends shorter reads through K6); a chunk wholly outside the aligned part is sent to column 0.
                        int colA = ((int)half + c0) * 4;
                        if constexpr (ALN) { if (colA < -60) colA = 0; }
                        u32 pc5 = prev_code5 << 24;
#pragma unroll
                        for (int wd = 0; wd < 4; ++wd) {
                            const u32 pw5 = __builtin_amdgcn_alignbyte(code5[wd], pc5, 3);
                            const u32 d5 = pw5 + code[wd];                            // 5*prev + cur per byte, <= 24
                            pc5 = code5[wd];
                            const u32 xwd = xw[wd];
                            const u32 qn = ~qv[wd];
                            const u32 zero = 0u, both = 0x10001u;
                            auto one_base = [&](auto bsel) {
                                constexpr int b = decltype(bsel)::value;
                                const u32 qi = (qn >> (8 * b)) & 0xFFu;                 // 255 - quality byte
                                const u32 tq = qi < tcl ? qi : tcl;                    // below minscore (and padding): a trash row
                                const u32 inc = k1_increment<b>(xwd, zero, both);      // recalibrate.py:13-20: errs << 16 | total
                                u32 a;
                                if constexpr (ALN) {
                                    const int co = colA + 4 * (4 * wd + b);
                                    a = __umul24(tq, row_bytes) + pos_base + copy_off + (u32)co;
                                } else {
                                    a = __umul24(tq, row_bytes) + A + (u32)(KJ > 0 ? 4 * KJ * (4 * wd + b) : 4 * (4 * wd + b));
                                }
                                atomicAdd(reinterpret_cast<u32*>(reinterpret_cast<char*>(lds) + a), inc);   // recalibrate.py:116-117
                                u32 slot = (d5 >> (8 * b)) & 0xFFu;
                                if (SPLIT) slot = qi <= 255u - p.dlo ? slot : 24u;             // context needs q >= its own threshold
                                const u32 trow = tq * dnt_row + dnt_base;                      // constant powers of two: two shift-adds,
                                const u32 ad = slot * (4u * DN) + trow;                // the LDS base is inside dnt_base
                                __hip_atomic_fetch_add(reinterpret_cast<lds_u32*>(ad), inc, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_WORKGROUP);          // recalibrate.py:118-119
                            };
                            one_base(std::integral_constant<int, 0>{}); one_base(std::integral_constant<int, 1>{});
                            one_base(std::integral_constant<int, 2>{}); one_base(std::integral_constant<int, 3>{});
                        }
                    }
                }
            };

            bool walk = total > 0;
            if constexpr (NIB && KJ > 0) {
                // A UNIFORM block: all 64 rows inside the slice, every meta word that of a complete pair of the launch's common
                // length in read group g (from the meta load above and one ballot; wave-uniform) has its own loop.  What `fetch` / `process` work out per chunk is a constant here: the compaction
                // is the identity (row slot = k, no bperm), every row has KJ chunks of which each holds counted bases
                // (len = maxlen > 16 (KJ - 1); act, fits_tables: true), the pitch is 16 KJ bytes, so the chunk of lane l at
                // step s is chunk 64 s + l of the block and its loads are 16 (8) bytes at 1024 (512) s + 16 (8) l.  What is
                // left per chunk: j and k of the chunk that is binned (one of each: the steps are binned in order), the
                // carry of the previous base, the data's own screens -- and the 16 bases.
                static_assert((KJ & 1) != 0, "the loop below fetches steps in twos and bins the last one alone");
                if (__ballot(myread < seg_hi && m == ((u32)p.maxlen | ((u32)g << 16))) == ~0ull) {
                    walk = false;
                    constexpr int DK = 64 / KJ, DJ = 64 - DK * KJ;
                    int j4 = 4 * lane_j0, k = lane_k0;                   // 4 j: the chunk's word in a table row
                    const u32 at = 16u * (u32)lane;
                    const u32 lds_at = (u32)reinterpret_cast<size_t>(lds);
                    const u32 ctx_at = 4u * CYC + 4u * (u32)(lane & (DN - 1));       // from a row's cycle word 0 to this lane's copy of slot 0
                    const u32 dlo4 = (p.dlo < 128u ? p.dlo : 128u) * 0x01010101u;     // (a counted quality byte is below 128)
                    const u32 one = 1u;
                    u32 inc_a = 1u, inc_b = 1u;                                    // two increments in turn; their low halves stay 1
                    auto fetch_at = [&](K1Chunk& ch, const uint8_t* fseq, const uint8_t* fcseq, const uint8_t* fqual, u32 o) {
                        const uint2 sv = *reinterpret_cast<const uint2*>(fseq + (o >> 1));
                        if constexpr (!EB) {
                            const uint2 cv = *reinterpret_cast<const uint2*>(fcseq + (o >> 1));
                            ch.c[0] = cv.x; ch.c[1] = cv.y;
                        }
                        const uint4 qv = *reinterpret_cast<const uint4*>(fqual + o);
                        ch.s[0] = sv.x; ch.s[1] = sv.y;
                        ch.q[0] = qv.x; ch.q[1] = qv.y; ch.q[2] = qv.z; ch.q[3] = qv.w;
                    };
                    auto fetch_u = [&](K1Chunk& ch, int s) { fetch_at(ch, bseq, bcseq, bqual, at + 1024u * (u32)s); };
                    auto process_u = [&](const K1Chunk& ch) {
                        u32 code[4], code5[4], xw[4], hiq = 0u;
                        code[0] = nib_lo_code<EB>(ch.s[0]); code[1] = nib_hi_code<EB>(ch.s[0]);
                        code[2] = nib_lo_code<EB>(ch.s[1]); code[3] = nib_hi_code<EB>(ch.s[1]);
                        if constexpr (EB) {                                  // the error bytes are bit 3 of the nibbles, where they stand
                            xw[0] = ch.s[0] & 0x08080808u; xw[1] = ch.s[0] & 0x80808080u;
                            xw[2] = ch.s[1] & 0x08080808u; xw[3] = ch.s[1] & 0x80808080u;
                        } else {
                            const u32 x0 = ch.s[0] ^ ch.c[0], x1 = ch.s[1] ^ ch.c[1];
                            xw[0] = nib_lo(x0); xw[1] = nib_hi(x0); xw[2] = nib_lo(x1); xw[3] = nib_hi(x1);
                        }
                        const u32 badbits = nib_bad<EB>(ch.s[0]) | nib_bad<EB>(ch.s[1]);
#pragma unroll
                        for (int wd = 0; wd < 4; ++wd) {
                            code5[wd] = (code[wd] << 2) + code[wd];
                            hiq |= (ch.q[wd] + 0x34343434u) | ch.q[wd];
                        }
                        hiq &= 0x80808080u;
                        const u32 last_code5 = code5[3] >> 24;
                        u32 prev_code5 = wave_shr1(last_code5, carry_code);
                        carry_code = (u32)__builtin_amdgcn_readlane((int)last_code5, 63);
                        if (j4 == 0) prev_code5 = 20u;
                        if (hiq | badbits) {                                 // a flagged chunk reports what `process` reports and counts nothing
                            if (hiq) flag(p.status, ST_INDEX, read0 + k);
                            if (badbits) flag(p.status, ST_LUT, 0);
                        } else {
                            // the 16 bases, binned as `process` bins them (KJ > 0, not ALN) in five vector instructions each: the
                            // joint row makes the context word's address the cycle word's plus a 16-bit delta
                            //     CYC * 4 - 4 j + 64 slot + 4 (lane & 15)          (0 < delta < JROW: no carry between halves)
                            // of which a register E holds two bases' worth (k1_joint_delta); the increment comes from one
                            // sub-dword min (k1_joint_increment)
                            const u32 A = lds_at + pos_base + (u32)j4;            // LDS address of cycle word j of row 0, less the row bias
                            const u32 tcl = tclamp + (u32)(k & (ntrash - 1));
                            const u32 (&qv)[4] = ch.q;
                            const u32 kd = ctx_at - (u32)j4;
                            const u32 kd2 = kd | (kd << 16);
                            u32 pc5 = prev_code5 << 24;
#pragma unroll
                            for (int wd = 0; wd < 4; ++wd) {
                                const u32 pw5 = __builtin_amdgcn_alignbyte(code5[wd], pc5, 3);
                                u32 d5 = pw5 + code[wd];                          // 5*prev + cur per byte, <= 24
                                pc5 = code5[wd];
                                if (SPLIT) {                                      // context needs q >= its own threshold: slot 24 otherwise
                                    const u32 t = ((qv[wd] | 0x80808080u) - dlo4) & 0x80808080u;      // bit 7 of a byte: q >= dlo (q < 128 here)
                                    d5 = (d5 & (t - (t >> 7))) | (0x18181818u & ~(t - (t >> 7)));
                                }
                                const u32 e02 = k1_shl6_add(d5 & 0x00FF00FFu, kd2);                    // deltas of bases 0 | 2 << 16
                                const u32 e13 = k1_shl6_add(__builtin_amdgcn_perm(0u, d5, 0x0C030C01u), kd2);   // ... of bases 1 | 3 << 16
                                const u32 xwd = xw[wd];
                                const u32 qn = ~qv[wd];
                                auto one_base = [&](auto bsel) {
                                    constexpr int b = decltype(bsel)::value;
                                    const u32 tq = k1_joint_row<b>(qn, tcl);       // 255 - quality byte; below minscore (and padding): a trash row
                                    u32& inc = (b & 1) ? inc_b : inc_a;
                                    k1_joint_increment<b>(inc, xwd, one);         // recalibrate.py:13-20: errs << 16 | total
                                    const u32 a = __umul24(tq, JROW) + A;
                                    __hip_atomic_fetch_add(reinterpret_cast<lds_u32*>(a + (u32)(4 * KJ * (4 * wd + b))), inc, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_WORKGROUP);          // recalibrate.py:116-117
                                    const u32 ad = k1_joint_delta<(b >> 1)>(a, (b & 1) ? e13 : e02);
                                    __hip_atomic_fetch_add(reinterpret_cast<lds_u32*>(ad), inc, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_WORKGROUP);          // recalibrate.py:118-119
                                };
                                one_base(std::integral_constant<int, 0>{}); one_base(std::integral_constant<int, 1>{});
                                one_base(std::integral_constant<int, 2>{}); one_base(std::integral_constant<int, 3>{});
                            }
                        }
                        const int jn = j4 + 4 * DJ;
                        const bool wrap = jn >= 4 * KJ;
                        j4 = wrap ? jn - 4 * KJ : jn;
                        k += DK + (wrap ? 1 : 0);
                    };
                    // KJ is odd: the step fetched ahead sits in the buffer a block ends on, not the one it starts on (eight v_mov a block)
                    if (fed) {
                        ua.s[0] = ub.s[0]; ua.s[1] = ub.s[1];
                        if constexpr (!EB) { ua.c[0] = ub.c[0]; ua.c[1] = ub.c[1]; }
                        ua.q[0] = ub.q[0]; ua.q[1] = ub.q[1]; ua.q[2] = ub.q[2]; ua.q[3] = ub.q[3];
                    } else {
                        fetch_u(ua, 0);
                    }
#pragma unroll 1
                    for (int s = 0; s + 1 < KJ; s += 2) {
                        fetch_u(ub, s + 1);
                        process_u(ua);
                        fetch_u(ua, s + 2);
                        process_u(ub);
                    }
                    // the wave's block of the next iteration, if it is a whole block of this slice (see INVARIANT above)
                    const long long nblk = blk + (long long)gx * nwaves;
                    ahead = ((nblk + 1) << 6) <= seg_hi - seg_lo;
                    const long long nread0 = ahead ? seg_lo + (nblk << 6) : read0;
                    m_next = p.meta[nread0 + lane];
                    fetch_at(ub, p.seq + (size_t)nread0 * (p.pitch >> 1), EB ? nullptr : p.cseq + (size_t)nread0 * (p.pitch >> 1),
                             p.qual + (size_t)nread0 * p.pitch, at);
                    process_u(ua);
                }
            }
            if (walk) {
                // one step in flight while the previous one is binned; fetches are unconditional
                // (past the end they re-read the block's first chunk) so that the outstanding
                // loads can be counted (s_waitcnt vmcnt(3)) instead of drained
                K1Chunk ca, cb;
                ca.k = lane_k0; ca.j = lane_j0;
                cb.k = lane_k0; cb.j = lane_j0; advance(cb, dk1, dj1);
                fetch(ca);
                for (int w0 = 0; w0 < total; w0 += 128) {
                    fetch(cb);
                    process(ca);
                    if (w0 + 64 < total) {
                        advance(ca, dk2, dj2);
                        fetch(ca);
                        process(cb);
                        advance(cb, dk2, dj2);
                    }
                }
                // The loop leaves the loads of a step nobody bins in flight.  The joint-row forms drain them here (vmcnt(0), gfx9
                // encoding), once per general block: otherwise every later use of their registers -- the flush of the context
                // table, the loop's own bookkeeping -- has to wait for ALL loads of the wave, those fetched ahead for the next
                // uniform block and the flush's own atomics included.
                if constexpr (JOINT) __builtin_amdgcn_s_waitcnt(0x0F70);
            }
        }
        ++since_flush; ++since_dn_flush;
        if (since_flush == K1V3_FLUSH_ITERS || since_dn_flush == p.dn_flush_iters) {
            __syncthreads();
            flush_dn(); since_dn_flush = 0;
            if (since_flush == K1V3_FLUSH_ITERS) { flush_pos(); since_flush = 0; }
            __syncthreads();
        }
    }
    __syncthreads();
    flush_dn(); flush_pos();
}

template <bool SPLIT, int DN = K1V3_DNREP, bool NIB = false, int KJ = 0, bool EB = false>
__global__ __launch_bounds__(K1V3_THREADS) void k1v3_accumulate(K1v3Params p)
{
    extern __shared__ __attribute__((aligned(16))) u32 lds[];
    k1v3_body<SPLIT, DN, NIB, KJ, false, false, EB>(p, lds, (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.y);
}

// the aligned-read form (K6 fused into K1): the BAM-sourced tally of gatk/bqsr.py:52-123 straight from the reads as aligned
template <bool SPLIT, int DN>
__global__ __launch_bounds__(K1V3_THREADS) void k1v3_aligned(K1v3Params p)
{
    extern __shared__ __attribute__((aligned(16))) u32 lds[];
    k1v3_body<SPLIT, DN, false, 0, true>(p, lds, (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.y);
}

// ... and K4 folded in for reads of one M / = / X operation (kbbq_tally_aligned_dev): read bytes, OQ and the reference window
template <bool SPLIT, int DN>
__global__ __launch_bounds__(K1V3_THREADS) void k1v3_aligned_ref(K1v3Params p)
{
    extern __shared__ __attribute__((aligned(16))) u32 lds[];
    k1v3_body<SPLIT, DN, false, 0, true, true>(p, lds, (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.y);
}

// ONE launch over all length bands of a mixed-length input (BASELINE config 5; recalibrate.py:81-101 grows its arrays as the
// reads get longer, the file path cuts the reads into bands of one row width each: kbbq/fastx.py BAND_CLASSES).  A launch
// per band is 9-10 iterations per workgroup for the narrow bands -- pipeline fill, table zeroing and the final flush of a
// 100 KB table paid eight times per step; here every band gets its share of the CUs' workgroups (wg_start, by the host:
// proportional to the band's chunks plus a per-row term) and they all run at once, each workgroup with ITS band's
// parameters -- row pitch, LDS table geometry for the band's longest / shortest read, copies of the context table.
#define K1V3_MAX_BANDS 16
struct K1BandsParams {
    int nbands;
    int wg_start[K1V3_MAX_BANDS + 1];     // band b owns workgroups [wg_start[b], wg_start[b + 1]) of blockIdx.x
    int dn[K1V3_MAX_BANDS];               // copies of the context table: K1V3_DNREP or 8
    unsigned long long* dbg;              // diagnostic (KBBQ_K1_BANDS_DBG): [2 * workgroups] start / end of every workgroup (s_memrealtime, 100 MHz)
    K1v3Params band[K1V3_MAX_BANDS];
};

template <bool SPLIT, bool NIB>
__global__ __launch_bounds__(K1V3_THREADS) void k1v3_bands(K1BandsParams t)
{
    extern __shared__ __attribute__((aligned(16))) u32 lds[];
    int b = 0;
    while (b + 1 < t.nbands && (int)blockIdx.x >= t.wg_start[b + 1]) ++b;
    const K1v3Params& p = t.band[b];
    const int bx = (int)blockIdx.x - t.wg_start[b], gx = t.wg_start[b + 1] - t.wg_start[b];
    if (t.dbg && threadIdx.x == 0 && blockIdx.y == 0) t.dbg[blockIdx.x] = wall_clock64();
    if (t.dn[b] == K1V3_DNREP) k1v3_body<SPLIT, K1V3_DNREP, NIB, 0>(p, lds, bx, gx, (int)blockIdx.y);
    else k1v3_body<SPLIT, 8, NIB, 0>(p, lds, bx, gx, (int)blockIdx.y);
    if (t.dbg && threadIdx.x == 0 && blockIdx.y == 0) t.dbg[gridDim.x + blockIdx.x] = wall_clock64();
}

// ---------------------------------------------------------------- K2 (table-driven)
// "Full" LUT, int8, one row per (read group, RAW quality byte qb in [0, 33+Qt)):
//     row[0 .. W)         cycle entry for first-in-pair reads, index = position   (W = S2 + 16:
//     row[W .. 2W)        the same entries mirrored: W + position <-> column S2-1-position
//     row[2W .. +32)      context entry, index 5*code(prev)+code(cur) (25 used)
// the 16 extra entries per region keep the padding positions of a 16-byte chunk in-region)
// qb = 0 (padding): cycle entries -33, contexts 0  -> output byte 0
// qb below 33 + minscore: identity rows (cycle entry = qb - 33, contexts 0) -> byte unchanged
// otherwise the model rows.  new byte = cycle entry + context entry + 33.
__host__ __device__ __forceinline__ int full_lut_width(int S2) { return S2 + 16; }
__host__ __device__ __forceinline__ int full_lut_row_bytes(int S2)
{
    int rb = (2 * full_lut_width(S2) + 32 + 3) & ~3;
    if (((rb >> 2) & 1) == 0) rb += 4;        // odd number of dwords per row: rows start on different banks
    return rb;
}

// ---------------------------------------------------------------- mate-pair rows
// Optional device layout for paired reads of one length S (2 x 150 bp): ONE row per pair,
//     [mate 1: S bytes][separator][mate 2: S bytes][padding to a multiple of 16]
// separator and padding are 'N' (seq, cseq) / 0 (qual), i.e. uncounted bases.  2S + 1 = 301 -> pitch 304
// instead of 2 x 160: 5 % fewer bytes through HBM for the same bases, and K1 / K2 run unchanged on the
// rows as if they were single reads: byte offset b IS the stored cycle index (K1's table keeps
// second-in-pair cycles mirrored from S upwards, here from S + 1; K2's pair LUT likewise), and the 'N'
// separator gives mate 2's first base "no previous base" exactly like position 0 of a read.
__host__ __device__ __forceinline__ int pair_pitch(int S2) { return (S2 + 1 + 15) & ~15; }
__host__ __device__ __forceinline__ int pair_lut_row_bytes(int S2)
{
    int rb = pair_pitch(S2) + 32;
    if (((rb >> 2) & 1) == 0) rb += 4;        // odd number of dwords per row
    return rb;
}

struct K2Chunk { u32 s[4], q[4]; u32 mk; u32 dlo, dhi; int kk; int k; int j; int nb; bool act0; };

struct K2v3Params {
    const uint8_t* seq; const uint8_t* qual; const u32* meta;
    long long nreads; int pitch; int cpr; u32 cpr_magic; int R; int Qt; int S2; int minscore; u32 qlo;
    const int16_t* lut16;      // canonical LUT (exact path)
    const int8_t* full;        // full LUT (global copy, staged into LDS)
    int full_bytes; int rs16;
    u32 rb;                    // bytes per row of the staged LUT
    u32 W;                     // offset of the second-in-pair (mirrored) cycle entries within a row
    u32 ctx_off;               // offset of the context entries within a row
    int maxlen;                // longest row the LUT serves: S2 (H1: any single read), or S2 + 1 for mate-pair rows
    int pairs;                 // mate-pair rows: rows the fast path cannot serve are reported (KBBQ_E_LUT), not emulated
    const long long* seg;      // rows grouped by read group: slice blockIdx.y stages only its group's LUT rows; NULL: all groups
    int rpb;                   // rows per wave block (<= 64): a wave's contiguous footprint is rpb * pitch bytes per plane
    int parts;                 // > 1: the workgroups walk the rows as `parts` sequential fronts (workgroup b: part b % parts) instead of one: the 2 read +
                               // 1 written traversal of 50 M character rows 4.68-4.78 -> 4.44-4.48 ms with 4 ... 32 fronts (the host passes 8; kbbq_k2_tile.h
                               // has the same for the short-lived kernel; K1's read-only traversal does not care)
    const long long* perm;     // rows grouped by read group: row i is stored as row perm[i] of `out` (straight back into input order); NULL: row i
    uint8_t* out; u64* status;
};

// EB: the seq plane carries KBBQ_ROWS_ERRBIT's flag in bit 3 of its nibbles; the codes are bits 0-2
template <bool NIB = false, bool EB = false>
__global__ __launch_bounds__(K2V3_THREADS) __attribute__((amdgpu_waves_per_eu(K2V3_WAVES, 8))) void k2v3_apply(K2v3Params p)
{
    extern __shared__ __attribute__((aligned(16))) u32 lds[];
    const u32 rb = p.rb;
    const u32 rg_bytes = (u32)(33 + p.Qt) * rb;
    const int g = blockIdx.y;                                   // grouped rows: the read group of this slice
    {
        // grouped: only the rows of this slice's read group are staged (any number of groups at the LDS cost of one)
        const u32* src = reinterpret_cast<const u32*>(p.full + (p.seg ? (size_t)g * rg_bytes : 0));
        const int nw = (int)((p.seg ? rg_bytes : (u32)p.full_bytes) >> 2);
        for (int i = threadIdx.x; i < nw; i += blockDim.x) lds[i] = src[i];
        __syncthreads();
    }
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwaves = blockDim.x >> 6;
    const long long seg_lo = p.seg ? p.seg[g] : 0ll, seg_hi = p.seg ? p.seg[g + 1] : p.nreads;
    const long long nblocks = (seg_hi - seg_lo + p.rpb - 1) / p.rpb;
    const u32 hi_add = (u32)(0x80 - (p.Qt + 33)) * 0x01010101u;   // byte >= Qt+33 <=> bit 7 after the add
    const int lane_k0 = p.cpr == 1 ? lane : (int)__umulhi((u32)lane, p.cpr_magic);
    const int lane_j0 = lane - lane_k0 * p.cpr;
    const int dk1 = 64 / p.cpr, dj1 = 64 - dk1 * p.cpr;
    const int dkn = (64 * K2V3_NBUF) / p.cpr, djn = 64 * K2V3_NBUF - dkn * p.cpr;

    long long blk0 = (long long)blockIdx.x * nwaves + wave, blk_step = (long long)gridDim.x * nwaves, blk_end = nblocks;
    if (p.parts > 1 && (int)gridDim.x % p.parts == 0) {
        const long long per = (nblocks + p.parts - 1) / p.parts;
        const int part = (int)blockIdx.x % p.parts;
        blk0 = part * per + (long long)((int)blockIdx.x / p.parts) * nwaves + wave;
        blk_step = (long long)((int)gridDim.x / p.parts) * nwaves;
        blk_end = (part + 1) * per < nblocks ? (part + 1) * per : nblocks;
    }
    for (long long blk = blk0; blk < blk_end; blk += blk_step) {
        const long long read0 = seg_lo + blk * p.rpb;
        const long long myread = read0 + lane;
        const int n = (int)((seg_hi - read0) < p.rpb ? (seg_hi - read0) : p.rpb);
        const u32 m = lane < n ? p.meta[myread] : 0u;
        const long long pm = (p.perm && lane < n) ? p.perm[myread] : 0ll;
        const int total = n * p.cpr;
        const uint8_t* bseq = p.seq + (size_t)read0 * (NIB ? p.pitch >> 1 : p.pitch);
        const uint8_t* bqual = p.qual + (size_t)read0 * p.pitch;
        uint8_t* bout = p.out + (size_t)read0 * p.pitch;
        u32 carry_code = 20u, carry_char = 0u;

        auto advance = [&](K2Chunk& ch, int dk, int dj) {
            const int jj = ch.j + dj;
            const bool wrap = jj >= p.cpr;
            ch.j = wrap ? jj - p.cpr : jj;
            ch.kk = ch.kk + dk + (wrap ? 1 : 0);
        };
        auto fetch = [&](K2Chunk& ch) {
            ch.act0 = ch.kk < n;
            ch.k = ch.act0 ? ch.kk : 0;
            ch.mk = bperm(m, ch.k);
            if (p.perm) { ch.dlo = bperm((u32)pm, ch.k); ch.dhi = bperm((u32)(pm >> 32), ch.k); }
            ch.nb = ch.act0 ? ((int)(ch.mk & 0xFFFFu) - 16 * ch.j) : 0;
            const u32 rowoff = ch.nb > 0 ? __umul24((u32)ch.k, (u32)p.pitch) + (u32)(16 * ch.j) : 0u;
            if constexpr (NIB) {
                const uint2 sv = *reinterpret_cast<const uint2*>(bseq + (rowoff >> 1));
                ch.s[0] = sv.x; ch.s[1] = sv.y;
            } else {
                const uint4 sv = *reinterpret_cast<const uint4*>(bseq + rowoff);
                ch.s[0] = sv.x; ch.s[1] = sv.y; ch.s[2] = sv.z; ch.s[3] = sv.w;
            }
            const uint4 qv = *reinterpret_cast<const uint4*>(bqual + rowoff);
            ch.q[0] = qv.x; ch.q[1] = qv.y; ch.q[2] = qv.z; ch.q[3] = qv.w;
        };
        auto process = [&](const K2Chunk& ch) {
            const int j = ch.j, nb = ch.nb, k = ch.k;
            const bool act = nb > 0;
            const int len = (int)(ch.mk & 0xFFFFu);
            const int rg = (int)((ch.mk >> 16) & 0x7FFFu);
            const bool second = (ch.mk >> 31) != 0u;
            const int pos0 = 16 * j;
            u32 code[4], code5[4], badbits = 0u, hiq = 0u;
            if constexpr (NIB) {
                code[0] = nib_lo_code<EB>(ch.s[0]); code[1] = nib_hi_code<EB>(ch.s[0]);
                code[2] = nib_lo_code<EB>(ch.s[1]); code[3] = nib_hi_code<EB>(ch.s[1]);
                badbits = nib_bad<EB>(ch.s[0]) | nib_bad<EB>(ch.s[1]);
            }
#pragma unroll
            for (int wd = 0; wd < 4; ++wd) {
                if constexpr (NIB) {
                    code5[wd] = (code[wd] << 2) + code[wd];
                } else {
                    u32 expect;
                    decode4x(ch.s[wd], code[wd], code5[wd], expect);
                    badbits |= expect ^ ch.s[wd];
                }
                hiq |= ((ch.q[wd] & 0x7F7F7F7Fu) + hi_add) | ch.q[wd];
            }
            hiq &= 0x80808080u;
            const u32 last_code5 = code5[3] >> 24;
            u32 prev_code5 = wave_shr1(last_code5, carry_code);
            carry_code = (u32)__builtin_amdgcn_readlane((int)last_code5, 63);
            u32 prev_char = 0u;
            if constexpr (!NIB) {
                const u32 last_char = ch.s[3] >> 24;
                prev_char = wave_shr1(last_char, carry_char);
                carry_char = (u32)__builtin_amdgcn_readlane((int)last_char, 63);
            }
            if (j == 0) { prev_code5 = 20u; prev_char = 0u; }
            if (ch.act0) {
                u32 o[4] = {0u, 0u, 0u, 0u};
                if (act) {
                    const long long read = read0 + k;
                    if constexpr (NIB) {
                        if (badbits) flag(p.status, ST_LUT, 0);                      // not a plane k7_lay_out wrote
                    } else {
                        if (badbits && chunk_type_error(ch.s[0], ch.s[1], ch.s[2], ch.s[3], ch.q[0], ch.q[1], ch.q[2], ch.q[3],
                                                        prev_char, nb, pos0, p.minscore))
                            flag(p.status, ST_TYPE, read);
                    }
                    u32 d5[4];
                    u32 pc5 = prev_code5 << 24;
#pragma unroll
                    for (int wd = 0; wd < 4; ++wd) {
                        d5[wd] = __builtin_amdgcn_alignbyte(code5[wd], pc5, 3) + code[wd];   // 5*prev + cur per byte
                        pc5 = code5[wd];
                    }
                    const bool trouble = hiq != 0u || rg >= p.R || len > p.maxlen || (p.seg && rg != g) || (NIB && badbits);
                    if (trouble && (p.pairs || (p.seg && rg != g) || (NIB && badbits))) {
                        flag(p.status, ST_LUT, 0);                       // the caller re-runs on one-read-per-row planes
                    } else if (trouble) {
                        const uint4 e = chunk_apply_exact(p.lut16, p.rs16, p.R, p.Qt, p.S2, p.qlo, rg, second, pos0, nb,
                                                          ch.q[0], ch.q[1], ch.q[2], ch.q[3], d5[0], d5[1], d5[2], d5[3],
                                                          p.status, read);
                        o[0] = e.x; o[1] = e.y; o[2] = e.z; o[3] = e.w;
                    } else {
                        const u32 rgb = p.seg ? 0u : (u32)rg * rg_bytes;
                        const u32 A = rgb + (second ? p.W : 0u) + (u32)pos0;
                        const u32 C = rgb + p.ctx_off;
#pragma unroll
                        for (int wd = 0; wd < 4; ++wd) {
                            // issue the word's eight LDS reads before combining any of them
                            int v1[4], v2[4];
#pragma unroll
                            for (int b = 0; b < 4; ++b) {
                                const u32 qb = (ch.q[wd] >> (8 * b)) & 0xFFu;
                                const u32 rowq = __umul24(qb, rb);
                                const u32 dd = (d5[wd] >> (8 * b)) & 0xFFu;
                                v1[b] = *reinterpret_cast<const int8_t*>(reinterpret_cast<const char*>(lds) + (rowq + A + (u32)(4 * wd + b)));
                                v2[b] = *reinterpret_cast<const int8_t*>(reinterpret_cast<const char*>(lds) + (rowq + C + dd));
                            }
                            // FAST mode is only legal for range-safe LUTs (flags == 0): every sum is 0..255
#pragma unroll
                            for (int b = 0; b < 4; ++b) o[wd] |= (u32)(v1[b] + v2[b] + 33) << (8 * b);
                        }
                    }
                }
                uint8_t* dst = p.perm ? p.out + (size_t)(((u64)ch.dhi << 32) | ch.dlo) * (size_t)p.pitch + (size_t)pos0
                                      : bout + (__umul24((u32)k, (u32)p.pitch) + (u32)pos0);
                *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
            }
        };

        if (total > 0) {
            // ring of K2V3_NBUF chunk buffers: while one step is processed the next NBUF-1 are in flight
            K2Chunk c[K2V3_NBUF];
#pragma unroll
            for (int b = 0; b < K2V3_NBUF; ++b) {
                c[b].kk = lane_k0; c[b].j = lane_j0;
#pragma unroll
                for (int t = 0; t < b; ++t) advance(c[b], dk1, dj1);
            }
#pragma unroll
            for (int b = 0; b < K2V3_NBUF - 1; ++b) fetch(c[b]);
            for (int w0 = 0; w0 < total; w0 += 64 * K2V3_NBUF) {
#pragma unroll
                for (int b = 0; b < K2V3_NBUF; ++b) {
                    if (b == 0 || w0 + 64 * b < total) {
                        fetch(c[(b + K2V3_NBUF - 1) % K2V3_NBUF]);      // unconditional: inactive chunks load row 0
                        process(c[b]);
                        advance(c[b], dkn, djn);
                    }
                }
            }
        }
    }
}
