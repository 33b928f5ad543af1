// kbbq_bam_in.h -- BAM input: the records of an inflated BAM stream, decoded where the kernels want them (include/kbbq_hip.h
// "BAM input", kbbq/_bamin.py).
//
// The host reader renders every record as a SAM line (csrc/bam_host.cpp format_record), parses the line again (csrc/sam_host.cpp
// kbbq_sam_open) and copies SEQ / QUAL / OQ out of the text (kbbq_sam_fill).  Everything the kernels consume is a fixed-offset
// field of the binary record or a tag found by one walk of its aux bytes: bd_record is the one statement of that, compiled for
// the device (kbd_decode: BD_LANES lanes per record, BD_RECORDS records per workgroup) and for the host (kbbq_bam_decode: one
// "lane").  What it writes is what the reader's arrays hold for the same record -- or a status bit: a record the text route
// could read differently (or refuse) is not decoded, its rows and CIGAR words are zeros, and the caller hands the file to the reader.
//
// A record in three steps:
//   bd_open    lane 0: the fixed fields, every length against the record's end (64-bit), the tag walk (skipping by type size; the
//              NUL of a Z / H value a dword at a time), the read group, the CIGAR's span / clips and the adaptor trim.
//   bd_copy    all lanes: QNAME bytes looked at, CIGAR words copied, the three rows written chunk by chunk.  Destination rows are
//              16-byte aligned, so every lane stores whole 16-byte chunks: chunk c of SEQ from the 8 source bytes at seq + 8c,
//              of QUAL / OQ from 16 source bytes, read at whatever alignment the record has (gfx950 reads a misaligned dwordx4
//              from global memory; kbbq_bam_out.h relies on the same); the last chunk of a field is built BYTEWISE from the
//              bytes the field has, so no read passes the record's end and the slab needs no slack; the rest of the pitch is zeros.
//   bd_finish  all lanes: a flagged record's rows and CIGAR words become zeros; lane 0 writes the record's 16 words.
// Whatever the bytes, nothing outside the slab is read and nothing outside rows [0, m) x pitch, words [0, m) and the record's
// CIGAR range cigar[cig_off[r], cig_off[r + 1]) is written.  Plain C++ stores only.
#pragma once
#include "../../include/kbbq_hip.h"
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BD_HD __host__ __device__ __forceinline__
#else
#define BD_HD inline
#endif

constexpr int BD_THREADS = 256;
constexpr int BD_LANES = 16;
constexpr int BD_RECORDS = BD_THREADS / BD_LANES;

struct alignas(16) bd_v16 { uint32_t w[4]; };

BD_HD uint32_t bd_u16(const uint8_t* p) { uint16_t v; memcpy(&v, p, 2); return v; }
BD_HD uint32_t bd_u32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
BD_HD int32_t bd_s32(const uint8_t* p) { return (int32_t)bd_u32(p); }

// nibble -> letter over "=ACMGRSVTWYHKDBN": the table is two 64-bit constants
BD_HD uint32_t bd_letter(uint32_t nib)
{
    const uint64_t t = (nib & 8u) ? 0x4E42444B48595754ull : 0x565352474D43413Dull;      // "TWYHKDBN" : "=ACMGRSV"
    return (uint32_t)(t >> ((nib & 7u) * 8u)) & 255u;
}

// per dword: has it a byte below n (n <= 128) / above n (n <= 127)?
BD_HD bool bd_any_below(uint32_t w, uint32_t n) { return ((w - 0x01010101u * n) & ~w & 0x80808080u) != 0; }
BD_HD bool bd_any_above(uint32_t w, uint32_t n) { return (((w + 0x01010101u * (127u - n)) | w) & 0x80808080u) != 0; }

// what one call works on (host or device memory alike); any output may be NULL: it is not written
struct BdJob {
    const uint8_t* slab; uint64_t slab_bytes;            // whole records, each behind its block_size word
    const uint32_t* rec_off;                             // [m] offset of every record's body (behind block_size) in the slab
    uint32_t m, pitch;
    const uint32_t* rg_off; const uint8_t* rg_ids;       // the @RG IDs in header order: ID g is rg_ids[rg_off[g], rg_off[g + 1])
    int32_t n_rg, n_ref;
    const uint32_t* cig_off; uint64_t cig_cap;           // [m + 1] the records' CIGAR ranges in `cigar`, which holds cig_cap words
    uint8_t* seq; uint8_t* qual; uint8_t* oq;            // [m, pitch] planes, 16-byte aligned
    kbbq_bam_words* words;                               // [m]
    uint32_t* cigar;
};

// what lane 0 found, for all lanes of the record
struct BdInfo {
    kbbq_bam_words w;
    const uint8_t* r;                                    // the record's body; NULL: the record lies outside the slab
    uint32_t l_name, cig, seq, qual, oq;                 // offsets in the body (oq: of the last OQ:Z value)
    uint32_t cig_lo, cig_n;                              // the record's range of `cigar` (cig_n 0 when the range is no range)
};

// the NUL of a Z / H value in r[p, end): its offset, or `end`; *ctrl when a byte in front of it is below 0x20 (a tab or a line
// end would change how the rendered line splits)
BD_HD uint64_t bd_find_nul(const uint8_t* r, uint64_t p, uint64_t end, bool* ctrl)
{
    while (end - p >= 4) {
        if (bd_any_below(bd_u32(r + p), 0x20)) break;    // a NUL or a control byte among these four: bytewise from here
        p += 4;
    }
    for (; p < end; ++p) {
        if (r[p] == 0) return p;
        if (r[p] < 0x20) {
            *ctrl = true;
            // (the dword loop may take over again behind this byte: it stops at the next such byte at the latest)
            while (end - (p + 1) >= 4 && !bd_any_below(bd_u32(r + p + 1), 0x20)) p += 4;
        }
    }
    return end;
}

BD_HD uint32_t bd_clamp16(int64_t v) { return (uint32_t)(v < 0 ? 0 : v > 65535 ? 65535 : v); }

// kbbq_sam_adaptor_trim's word (csrc/sam_host.cpp) for one record: the boundary from FLAG / POS / PNEXT / TLEN, then the walk
// over the CIGAR of the records it falls into
BD_HD uint32_t bd_trim(const kbbq_bam_words& w, const uint8_t* cg)
{
    const int32_t fl = w.flag;
    const bool rev = fl & 16, mate_rev = fl & 32;
    const int64_t tlen = w.tlen, pnext = w.pnext;
    if (tlen == 0 || !(fl & 1) || (fl & 4) || (fl & 8) || rev == mate_rev) return 0;
    const int64_t start = w.pos, end = start + w.ref_span, nq = w.qual_len, nops = w.cig_n;
    int64_t lo = 0, hi = 0;
    if (rev) {
        if (!(end - 1 > pnext)) return 0;
        const int64_t boundary = pnext - 1;
        if (boundary < start) return 0;
        int64_t q = 0, r = end;
        for (int64_t k = 0; k < nops; ++k) {
            const uint32_t o = bd_u32(cg + 4 * k), op = o & 15u;
            if (op == 0 || op == 7 || op == 8 || op == 1 || op == 4) q += o >> 4;
        }
        bool reached = false, found = false;
        for (int64_t k = nops - 1; k >= 0 && !found; --k) {
            const uint32_t o = bd_u32(cg + 4 * k), op = o & 15u;
            const int64_t l = o >> 4;
            if (op == 0 || op == 7 || op == 8) {
                if (reached) { hi = q; found = true; }
                else if (r - l <= boundary) { hi = q - ((r - 1) - (boundary < r - 1 ? boundary : r - 1)); found = true; }
                else { q -= l; r -= l; }
            } else if (op == 1 || op == 4) {
                if (reached) { hi = q; found = true; } else q -= l;
            } else if (op == 2 || op == 3) {
                if (r - l <= boundary) reached = true;
                r -= l;
            }
        }
        if (!found) return 0;
    } else {
        if (!(start <= pnext + tlen)) return 0;
        const int64_t boundary = start + (tlen < 0 ? -tlen : tlen);
        if (boundary > end - 1) return 0;
        int64_t q = 0, r = start;
        bool reached = false, found = false;
        hi = nq;
        for (int64_t k = 0; k < nops && !found; ++k) {
            const uint32_t o = bd_u32(cg + 4 * k), op = o & 15u;
            const int64_t l = o >> 4;
            if (op == 0 || op == 7 || op == 8) {
                if (reached) { lo = q; found = true; }
                else if (r + l > boundary) { lo = q + (boundary - r > 0 ? boundary - r : 0); found = true; }
                else { q += l; r += l; }
            } else if (op == 1 || op == 4) {
                if (reached) { lo = q; found = true; } else q += l;
            } else if (op == 2 || op == 3) {
                if (r + l > boundary) reached = true;
                r += l;
            }
        }
        if (!found) lo = nq;
    }
    return (uint32_t)(lo & 0xFFFF) | (uint32_t)(hi & 0xFFFF) << 16;
}

BD_HD void bd_open_at(const BdJob& J, uint64_t off, BdInfo& I);

// lane 0: everything of record `row` but its rows.  I.w.status != 0: the record is not decoded (nothing else of I.w is meaningful).
BD_HD void bd_open(const BdJob& J, uint32_t row, BdInfo& I)
{
    memset(&I, 0, sizeof I);
    kbbq_bam_words& w = I.w;
    // the record's CIGAR range, as the caller states it
    const uint64_t clo = J.cigar ? J.cig_off[row] : 0, chi = J.cigar ? J.cig_off[row + 1] : 0;
    const bool cig_range = clo <= chi && chi <= J.cig_cap;
    if (cig_range) { I.cig_lo = (uint32_t)clo; I.cig_n = (uint32_t)(chi - clo); }
    else w.status |= KBBQ_BAM_ST_RANGE;
    bd_open_at(J, J.rec_off[row], I);
}

// bd_open behind the CIGAR range: the record whose body lies at `off` of the slab (any 64-bit offset: kbbq_bam_recode.h walks a
// whole stream by it).  I is zeroed but for cig_lo / cig_n and the range's status bit.
BD_HD void bd_open_at(const BdJob& J, uint64_t off, BdInfo& I)
{
    kbbq_bam_words& w = I.w;
    const bool cig_range = !(w.status & KBBQ_BAM_ST_RANGE);
    // the record inside the slab: its block_size word in front of the body, the body's end
    if (off < 4 || off > J.slab_bytes) { w.status |= KBBQ_BAM_ST_RANGE; return; }
    const int32_t bs = bd_s32(J.slab + off - 4);
    if (bs < 0 || (uint64_t)bs > J.slab_bytes - off) { w.status |= KBBQ_BAM_ST_RANGE; return; }
    const uint8_t* r = J.slab + off;
    const uint64_t len = (uint64_t)bs;
    I.r = r;
    if (len < 32) { w.status |= KBBQ_BAM_ST_RECORD; return; }
    const uint32_t l_name = r[8], n_cig = bd_u16(r + 12);
    const int32_t l_seq = bd_s32(r + 16), next_ref = bd_s32(r + 20);
    w.ref_id = bd_s32(r); w.pos = bd_s32(r + 4); w.flag = (int32_t)bd_u16(r + 14); w.pnext = bd_s32(r + 24); w.tlen = bd_s32(r + 28);
    if (l_seq < 0 || l_name == 0) { w.status |= KBBQ_BAM_ST_RECORD; return; }
    const uint64_t L = (uint64_t)l_seq;
    const uint64_t need = 32 + (uint64_t)l_name + 4 * (uint64_t)n_cig + (L + 1) / 2 + L;
    if (need > len) { w.status |= KBBQ_BAM_ST_RECORD; return; }
    if (l_seq > 65535) { w.status |= KBBQ_BAM_ST_LONG; return; }
    I.l_name = l_name; I.cig = 32 + l_name; I.seq = I.cig + 4 * n_cig; I.qual = I.seq + (uint32_t)((L + 1) / 2);
    if (r[32 + l_name - 1] != 0) { w.status |= KBBQ_BAM_ST_RECORD; return; }
    if (w.ref_id >= J.n_ref || next_ref >= J.n_ref) { w.status |= KBBQ_BAM_ST_RECORD; return; }
    if (J.cigar && cig_range && I.cig_n != n_cig) w.status |= KBBQ_BAM_ST_RANGE;
    w.qlen = l_seq; w.cig_n = (int32_t)n_cig; w.oq_len = -1; w.rg = -1;
    // "no QUAL" as the text says it: '*' -- which is also what ONE quality of 9 renders as
    const uint32_t q0 = l_seq ? r[I.qual] : 0xFFu;
    w.qual_len = (l_seq == 0 || q0 == 0xFFu || (l_seq == 1 && q0 == 9u)) ? 0 : l_seq;
    // the tags: tag(2) type(1) value
    uint64_t p = (uint64_t)I.qual + L, rg_at = 0, rg_n = 0;
    bool has_rg = false, ctrl = false;
    while (p < len) {
        if (len - p < 3) { w.status |= KBBQ_BAM_ST_RECORD; return; }
        const uint32_t t0 = r[p], t1 = r[p + 1], type = r[p + 2];
        p += 3;
        if (t0 < 0x21 || t0 > 0x7E || t1 < 0x21 || t1 > 0x7E) ctrl = true;
        uint64_t size = 0;
        switch (type) {
            case 'A': case 'c': case 'C': size = 1; break;
            case 's': case 'S': size = 2; break;
            case 'i': case 'I': case 'f': size = 4; break;
            case 'Z': case 'H': {
                const uint64_t z = bd_find_nul(r, p, len, &ctrl);
                if (z == len) { w.status |= KBBQ_BAM_ST_RECORD; return; }
                if (type == 'Z' && t0 == 'R' && t1 == 'G') { has_rg = true; rg_at = p; rg_n = z - p; }
                if (type == 'Z' && t0 == 'O' && t1 == 'Q') { I.oq = (uint32_t)p; w.oq_len = (int32_t)(z - p > 0x7FFFFFFFull ? 0x7FFFFFFF : z - p); }
                p = z + 1;
                continue;
            }
            case 'B': {
                if (len - p < 5) { w.status |= KBBQ_BAM_ST_RECORD; return; }
                const uint32_t sub = r[p];
                const uint64_t count = bd_u32(r + p + 1);
                p += 5;
                const uint64_t each = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
                if (each == 0 || count * each > len - p) { w.status |= KBBQ_BAM_ST_RECORD; return; }
                p += count * each;
                continue;
            }
            default: w.status |= KBBQ_BAM_ST_RECORD; return;
        }
        if (len - p < size) { w.status |= KBBQ_BAM_ST_RECORD; return; }
        if (type == 'A' && r[p] < 0x20) ctrl = true;
        p += size;
    }
    if (ctrl) w.status |= KBBQ_BAM_ST_TEXT;
    if (w.oq_len > 32767) w.status |= KBBQ_BAM_ST_LONG;                     // (kbbq_sam_fields refuses length + 1 > 32768)
    if (has_rg) {
        // the FIRST @RG line with the ID of the record's LAST RG:Z tag; -2: the header has none
        for (uint64_t j = 0; j < rg_n; ++j) if (r[rg_at + j] < 0x21 || r[rg_at + j] > 0x7E) w.status |= KBBQ_BAM_ST_TEXT;
        w.rg = -2;
        for (int32_t g = 0; g < J.n_rg; ++g) {
            const uint32_t a = J.rg_off[g], b = J.rg_off[g + 1];
            if ((uint64_t)(b - a) != rg_n) continue;
            uint64_t j = 0;
            while (j < rg_n && J.rg_ids[a + j] == r[rg_at + j]) ++j;
            if (j == rg_n) { w.rg = g; break; }
        }
    }
    // the CIGAR: an operation above 8 renders as '?', which the reader stores as 15; span, clips
    const uint8_t* cg = r + I.cig;
    int64_t span = 0, lead = 0, tail = 0;
    for (uint32_t k = 0; k < n_cig; ++k) {
        const uint32_t o = bd_u32(cg + 4 * k), op = o & 15u;
        if (op > 8) w.status |= KBBQ_BAM_ST_TEXT;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += o >> 4;
    }
    for (uint32_t k = 0; k < n_cig; ++k) { const uint32_t o = bd_u32(cg + 4 * k), op = o & 15u; if (op == 4) lead += o >> 4; else if (op != 5) break; }
    for (int64_t k = (int64_t)n_cig - 1; k >= 0; --k) { const uint32_t o = bd_u32(cg + 4 * k), op = o & 15u; if (op == 4) tail += o >> 4; else if (op != 5) break; }
    w.ref_span = (int32_t)(span > 0x7FFFFFFF ? 0x7FFFFFFF : span);
    w.clip = bd_clamp16(lead) | bd_clamp16((int64_t)l_seq - tail) << 16;
    w.trim = bd_trim(w, cg);
}

// row[0, pitch) <- the field's n bytes (truncated at pitch), zero padded: chunk c by lane c % nl
template <class Op> BD_HD void bd_row(uint8_t* row, uint32_t pitch, uint32_t n, uint32_t lane, uint32_t nl, const Op& op)
{
    if (n > pitch) n = pitch;
    for (uint32_t c = lane; c < pitch / 16; c += nl) {
        const uint32_t base = c * 16;
        bd_v16 v = {{0, 0, 0, 0}};
        if (base + 16 <= n) op.vec(c, v);
        else if (base < n) {
            // (constant indices into v: a variable one would move it out of registers)
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (uint32_t i = 0; i < 16; ++i) if (base + i < n) v.w[i >> 2] |= op.byte(base + i) << ((i & 3u) * 8u);
        }
        *reinterpret_cast<bd_v16*>(row + base) = v;
    }
}

struct BdSeq {                                           // two letters from every source byte, the high nibble first
    const uint8_t* src;
    BD_HD uint32_t byte(uint32_t j) const { return bd_letter((uint32_t)src[j >> 1] >> ((j & 1u) ? 0 : 4)); }
    BD_HD void vec(uint32_t c, bd_v16& v) const
    {
        uint32_t in[2];
        memcpy(in, src + 8 * c, 8);
        for (int k = 0; k < 4; ++k) {
            const uint32_t h = in[k >> 1] >> ((k & 1) * 16);          // two source bytes
            v.w[k] = bd_letter(h >> 4) | bd_letter(h) << 8 | bd_letter(h >> 12) << 16 | bd_letter(h >> 8) << 24;
        }
    }
};

struct BdQual {                                          // byte + 33; *st when one is above 93
    const uint8_t* src; uint32_t* st;
    BD_HD uint32_t byte(uint32_t j) const { const uint32_t b = src[j]; if (b > 93) *st |= KBBQ_BAM_ST_QUAL; return (b + 33u) & 255u; }
    BD_HD void vec(uint32_t c, bd_v16& v) const
    {
        memcpy(&v, src + 16 * c, 16);
        for (int k = 0; k < 4; ++k) {
            if (bd_any_above(v.w[k], 93)) *st |= KBBQ_BAM_ST_QUAL;
            v.w[k] += 0x21212121u;                       // no byte carries into its neighbour when all are <= 222
        }
    }
};

struct BdText {                                          // the OQ value as it is; *st for a byte outside 0x21..0x7E
    const uint8_t* src; uint32_t* st;
    BD_HD uint32_t byte(uint32_t j) const { const uint32_t b = src[j]; if (b < 0x21 || b > 0x7E) *st |= KBBQ_BAM_ST_TEXT; return b; }
    BD_HD void vec(uint32_t c, bd_v16& v) const
    {
        memcpy(&v, src + 16 * c, 16);
        for (int k = 0; k < 4; ++k) if (bd_any_below(v.w[k], 0x21) || bd_any_above(v.w[k], 0x7E)) *st |= KBBQ_BAM_ST_TEXT;
    }
};

struct BdZero {
    BD_HD uint32_t byte(uint32_t) const { return 0; }
    BD_HD void vec(uint32_t, bd_v16&) const {}
};

// all lanes, for a record bd_open left without a status: the status bits this lane met
BD_HD uint32_t bd_copy(const BdJob& J, uint32_t row, const BdInfo& I, uint32_t lane, uint32_t nl)
{
    uint32_t st = 0;
    const uint8_t* r = I.r;
    // QNAME: a control byte splits the rendered line, a leading '@' makes it a header line
    for (uint32_t j = lane; j + 1 < I.l_name; j += nl) if (r[32 + j] < 0x20 || (j == 0 && r[32] == '@')) st |= KBBQ_BAM_ST_TEXT;
    if (J.cigar) for (uint32_t k = lane; k < I.cig_n; k += nl) J.cigar[I.cig_lo + k] = bd_u32(r + I.cig + 4 * k);
    const size_t at = (size_t)row * J.pitch;
    const uint32_t qlen = (uint32_t)I.w.qlen, oq_n = I.w.oq_len > 0 ? (uint32_t)I.w.oq_len : 0;
    if (J.seq) bd_row(J.seq + at, J.pitch, qlen, lane, nl, BdSeq{r + I.seq});
    if (I.w.qual_len) {
        // (all of QUAL is looked at, also what lies behind the pitch and is not written)
        if (J.qual) bd_row(J.qual + at, J.pitch, qlen, lane, nl, BdQual{r + I.qual, &st});
        const uint32_t from = J.qual ? (J.pitch < qlen ? J.pitch : qlen) : 0;
        for (uint32_t j = from + lane; j < qlen; j += nl) if (r[I.qual + j] > 93) st |= KBBQ_BAM_ST_QUAL;
    } else if (J.qual) bd_row(J.qual + at, J.pitch, 0, lane, nl, BdZero{});
    if (J.oq) bd_row(J.oq + at, J.pitch, oq_n, lane, nl, BdText{r + I.oq, &st});
    const uint32_t from = J.oq ? (J.pitch < oq_n ? J.pitch : oq_n) : 0;
    for (uint32_t j = from + lane; j < oq_n; j += nl) if (r[I.oq + j] < 0x21 || r[I.oq + j] > 0x7E) st |= KBBQ_BAM_ST_TEXT;
    return st;
}

// all lanes, with the record's status complete: a flagged record's rows and CIGAR words are zeros; lane 0 writes the words
BD_HD void bd_finish(const BdJob& J, uint32_t row, const BdInfo& I, uint32_t status, uint32_t lane, uint32_t nl)
{
    if (status) {
        const size_t at = (size_t)row * J.pitch;
        if (J.seq) bd_row(J.seq + at, J.pitch, 0, lane, nl, BdZero{});
        if (J.qual) bd_row(J.qual + at, J.pitch, 0, lane, nl, BdZero{});
        if (J.oq) bd_row(J.oq + at, J.pitch, 0, lane, nl, BdZero{});
        if (J.cigar) for (uint32_t k = lane; k < I.cig_n; k += nl) J.cigar[I.cig_lo + k] = 0;
    }
    if (lane == 0 && J.words) {
        kbbq_bam_words w = I.w;
        if (status) { memset(&w, 0, sizeof w); w.status = status; }
        J.words[row] = w;
    }
}

// one record by one "lane": the host twin's statement
BD_HD uint32_t bd_record(const BdJob& J, uint32_t row)
{
    BdInfo I;
    bd_open(J, row, I);
    const uint32_t status = I.w.status ? I.w.status : bd_copy(J, row, I, 0, 1);
    bd_finish(J, row, I, status, 0, 1);
    return status;
}

#if defined(__HIPCC__)
struct BdParams { BdJob job; uint32_t* any; };           // any: the OR of every record's status

__global__ __launch_bounds__(BD_THREADS) void kbd_decode(BdParams p)
{
    __shared__ BdInfo info[BD_RECORDS];
    __shared__ uint32_t met[BD_RECORDS];
    const uint32_t k = threadIdx.x / BD_LANES, lane = threadIdx.x % BD_LANES, row = blockIdx.x * BD_RECORDS + k;
    const bool live = row < p.job.m;
    if (lane == 0) {
        met[k] = 0;
        if (live) bd_open(p.job, row, info[k]);
    }
    __syncthreads();
    if (live && !info[k].w.status) {
        const uint32_t st = bd_copy(p.job, row, info[k], lane, BD_LANES);
        if (st) atomicOr(&met[k], st);
    }
    __syncthreads();
    if (live) {
        const uint32_t status = info[k].w.status | met[k];
        bd_finish(p.job, row, info[k], status, lane, BD_LANES);
        if (lane == 0 && status) atomicOr(p.any, status);
    }
}
#endif
