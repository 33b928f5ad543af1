// kbbq_bam_recode.h -- BAM in, BAM out: the --bam-out skeleton and descriptors of records that are resident as BAM records
// (include/kbbq_hip.h "BAM recode").
//
// The host route renders a binary record as a SAM line (csrc/bam_host.cpp format_record), parses the line (csrc/sam_host.cpp
// kbbq_sam_open) and encodes QNAME, CIGAR and tags again (kbbq_bam_layout, kbbq_bam_skeleton).  Every byte of that skeleton is in
// the record already, but for three things: the `bin` field is computed, an integer tag takes the first type of c C s S i I that
// holds its value (bam_tag), and an absent QUAL -- a first byte of 0xFF, or ONE quality of 9, which the text shows as '*' -- is
// 0xFF throughout.  br_size / br_write are the one statement of that, compiled for the device (kbr_size, kbr_write: BR_LANES lanes
// per record, BR_RECORDS records per workgroup) and for the host (kbbq_bam_recode: one "lane").
//
// Three steps:
//   size   bd_open_at + bd_copy (kbbq_bam_in.h) vouch for the record exactly as the decode does -- same code, same status bits --;
//          one walk of the aux bytes gives the tail's size and the bits below; lane 0 writes the descriptor (offsets 0) and the status.
//   scan   the exclusive scan of the records' skeleton and stream sizes: kbr_sums, kbr_scan_blocks, kbr_offsets (wave64
//          __shfl_up scans, 64-bit sums); the host twin adds them up in a loop.
//   write  head | kept QUAL | tail at skel + skel_off.  All lanes of a record walk its aux bytes alike (the loads are one
//          address per record, so the walk costs what it would cost lane 0 alone and nothing is passed between lanes); the
//          stores are divided: a run of aux bytes that goes over unchanged -- up to the next integer tag whose stored type is not
//          the smallest; in files written by htslib the whole tail -- is one bo_segment (kbbq_bam_out.h), a re-typed tag is lane 0's.
//
// A record whose text round trip is not provably the identity gets a status bit, a descriptor of zeros and no skeleton byte.
// Beyond what the decode flags (KBBQ_BAM_ST_RECORD .. KBBQ_BAM_ST_RANGE):
//   KBBQ_BAM_ST_FLOAT  an `f` tag or a B:f array: the reader renders floats with %g, which does not always read back the same bits
//   KBBQ_BAM_ST_REF    a refID or next_refID below -1: the reader shows '*' for every negative one, and the text route writes -1
// Whatever the bytes: every length is checked against the record's end (64-bit) before it is used, nothing outside the image is
// read, and nothing outside desc[0, m), status[0, m) and skel[0, skel_bytes) is written -- the write step never leaves the
// record's range [skel_off, skel_off + head + kept QUAL + tail) the size step measured.  Plain C++ stores only.
#pragma once
#include "kbbq_bam_in.h"
#include "kbbq_bam_out.h"

constexpr int BR_THREADS = 256;
constexpr int BR_LANES = 16;
constexpr int BR_RECORDS = BR_THREADS / BR_LANES;

struct BrJob {
    const uint8_t* image; uint64_t image_bytes;          // the inflated BAM stream (whole records, each behind its block_size word)
    const uint64_t* rec_off;                             // [m] the offset of every record's body in the image (kbbq_bam_scan's, from `first`)
    uint32_t m; int32_t n_ref; uint32_t set_oq;
    const uint8_t* keep;                                 // [m] nonzero: QUAL stays as read; NULL: none does
    kbbq_bam_desc* desc; uint32_t* status;               // [m]
    uint8_t* skel; uint64_t skel_bytes;                  // the compact skeleton (the write step's; skel_bytes: the scan's total)
};

// the decode's job over the same image: no planes, no words, no CIGAR output -- bd_open_at / bd_copy only look
BD_HD BdJob br_decode_job(const BrJob& J)
{
    BdJob D;
    memset(&D, 0, sizeof D);
    D.slab = J.image; D.slab_bytes = J.image_bytes; D.m = J.m; D.pitch = 16; D.n_ref = J.n_ref;
    return D;
}

BD_HD bool br_is_int(uint32_t t) { return t == 'c' || t == 'C' || t == 's' || t == 'S' || t == 'i' || t == 'I'; }
BD_HD uint32_t br_int_bytes(uint32_t t) { return (t == 'c' || t == 'C') ? 1u : (t == 's' || t == 'S') ? 2u : 4u; }

// the value of an integer tag of type t at p (its bytes lie inside the record)
BD_HD int64_t br_int_value(uint32_t t, const uint8_t* p)
{
    switch (t) {
        case 'c': return (int8_t)p[0];
        case 'C': return p[0];
        case 's': return (int16_t)bd_u16(p);
        case 'S': return bd_u16(p);
        case 'i': return bd_s32(p);
        default: return bd_u32(p);
    }
}

// the first of c C s S i I that holds v (csrc/sam_host.cpp bam_tag)
BD_HD uint32_t br_int_type(int64_t v)
{
    if (v >= -128 && v <= 127) return 'c';
    if (v >= 0 && v <= 255) return 'C';
    if (v >= -32768 && v <= 32767) return 's';
    if (v >= 0 && v <= 65535) return 'S';
    if (v >= -2147483647 - 1 && v <= 2147483647) return 'i';
    return 'I';
}

constexpr uint32_t BR_W_FLOAT = 1, BR_W_OQ = 2, BR_W_BAD = 4;

struct BrWalk {
    uint64_t saved;                                      // bytes the re-typed tags passed so far are shorter by
    uint32_t met;                                        // BR_W_*
    uint32_t type; int64_t value;                        // of the tag the walk stopped at: its new type, its value
    uint32_t old_bytes;                                  // ... the bytes of its stored value
};

// The aux bytes r[p, len) tag by tag.  stop: return the offset of the first integer tag whose stored type is not the smallest
// (W.type / W.value / W.old_bytes are its); otherwise, and when there is none, `len`.  A tag that overruns the record ends the
// walk with BR_W_BAD (bd_open_at has refused such a record before).
BD_HD uint64_t br_walk(const uint8_t* r, uint64_t p, uint64_t len, bool stop, BrWalk& W)
{
    while (p < len) {
        if (len - p < 3) { W.met |= BR_W_BAD; return len; }
        const uint32_t t0 = r[p], t1 = r[p + 1], type = r[p + 2];
        const uint64_t v = p + 3;
        uint64_t size;
        if (br_is_int(type)) {
            size = br_int_bytes(type);
            if (len - v < size) { W.met |= BR_W_BAD; return len; }
            const int64_t x = br_int_value(type, r + v);
            const uint32_t nt = br_int_type(x);
            if (nt != type) {
                if (stop) { W.type = nt; W.value = x; W.old_bytes = (uint32_t)size; return p; }
                W.saved += size - br_int_bytes(nt);
            }
        } else if (type == 'A') size = 1;
        else if (type == 'f') { size = 4; W.met |= BR_W_FLOAT; }
        else if (type == 'Z' || type == 'H') {
            bool ctrl = false;
            const uint64_t z = bd_find_nul(r, v, len, &ctrl);
            if (z == len) { W.met |= BR_W_BAD; return len; }
            if (type == 'Z' && t0 == 'O' && t1 == 'Q') W.met |= BR_W_OQ;
            size = z + 1 - v;
        } else if (type == 'B') {
            if (len - v < 5) { W.met |= BR_W_BAD; return len; }
            const uint32_t sub = r[v];
            const uint64_t count = bd_u32(r + v + 1);
            if (sub == 'f') W.met |= BR_W_FLOAT;
            else if (!br_is_int(sub)) { W.met |= BR_W_BAD; return len; }
            size = 5 + count * br_int_bytes(sub);
        } else { W.met |= BR_W_BAD; return len; }
        if (len - v < size) { W.met |= BR_W_BAD; return len; }
        p = v + size;
    }
    return len;
}

// reg2bin of [beg, end) as csrc/sam_host.cpp bam_reg2bin has it
BD_HD uint32_t br_reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}

// what the size step found of a record, for all its lanes
struct BrInfo {
    BdInfo d;
    uint32_t tail;                                       // the tail's bytes (an added OQ included)
};

// ---- size ----------------------------------------------------------------------------------------------------------------------
// lane 0: the record opened as the decode opens it, then the walk.  R.d.w.status != 0: not vouched for.
BD_HD void br_open(const BrJob& J, const BdJob& D, uint32_t row, BrInfo& R)
{
    memset(&R, 0, sizeof R);
    bd_open_at(D, J.rec_off[row], R.d);
    kbbq_bam_words& w = R.d.w;
    if (w.status) return;
    const uint8_t* r = R.d.r;
    const uint64_t len = (uint64_t)bd_s32(r - 4), aux = (uint64_t)R.d.qual + (uint64_t)w.qlen;
    if (w.ref_id < -1 || bd_s32(r + 20) < -1) w.status |= KBBQ_BAM_ST_REF;
    BrWalk W;
    memset(&W, 0, sizeof W);
    br_walk(r, aux, len, false, W);
    if (W.met & BR_W_BAD) w.status |= KBBQ_BAM_ST_RECORD;
    if (W.met & BR_W_FLOAT) w.status |= KBBQ_BAM_ST_FLOAT;
    uint64_t tail = len - aux - W.saved;
    if (J.set_oq && !(W.met & BR_W_OQ) && w.qual_len) tail += 3 + (uint64_t)w.qlen + 1;
    R.tail = (uint32_t)tail;                             // (a record is shorter than 2^31 bytes, an added OQ than 2^16 + 4)
}

// lane 0, with the record's status complete: its descriptor (the offsets are the scan's to write) and its status word
BD_HD void br_close(const BrJob& J, uint32_t row, const BrInfo& R, uint32_t status)
{
    kbbq_bam_desc d;
    memset(&d, 0, sizeof d);
    if (!status) {
        d.head_bytes = 36u + R.d.l_name + 4u * (uint32_t)R.d.w.cig_n;
        d.tail_bytes = R.tail;
        d.l_seq = (uint32_t)R.d.w.qlen;
        d.qual_src = (!R.d.w.qual_len || (J.keep && J.keep[row])) ? KBBQ_BAM_QUAL_SKELETON : KBBQ_BAM_QUAL_PLANE;
    }
    J.desc[row] = d;
    J.status[row] = status;
}

BD_HD uint64_t br_skel_size(const kbbq_bam_desc& d) { return (uint64_t)d.head_bytes + (d.qual_src == KBBQ_BAM_QUAL_SKELETON ? d.l_seq : 0u) + d.tail_bytes; }
BD_HD uint64_t br_stream_size(const kbbq_bam_desc& d) { return (uint64_t)d.head_bytes + ((uint64_t)d.l_seq + 1) / 2 + d.l_seq + d.tail_bytes; }

// one record by one "lane": the host twin's size step
BD_HD uint32_t br_size(const BrJob& J, const BdJob& D, uint32_t row)
{
    BrInfo R;
    br_open(J, D, row, R);
    const uint32_t status = R.d.w.status ? R.d.w.status : bd_copy(D, row, R.d, 0, 1);
    br_close(J, row, R, status);
    return status;
}

// ---- write ---------------------------------------------------------------------------------------------------------------------
struct BrFill {                                          // an absent QUAL
    BO_HD uint8_t byte(uint32_t) const { return 0xFF; }
    BO_HD void vec(uint32_t, bo_v16& v) const { v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0xFFFFFFFFu; }
};

struct BrPlus33 {                                        // QUAL as the text shows it (every byte <= 93: the size step has looked)
    const uint8_t* src;
    BO_HD uint8_t byte(uint32_t j) const { return (uint8_t)(src[j] + 33u); }
    BO_HD void vec(uint32_t j, bo_v16& v) const { memcpy(&v, src + j, 16); for (int k = 0; k < 4; ++k) v.w[k] += 0x21212121u; }
};

// One record the size step vouched for (status 0), d its descriptor with the scan's offsets: all `nl` lanes alike.
BD_HD void br_write(const BrJob& J, uint32_t row, const kbbq_bam_desc& d, uint32_t lane, uint32_t nl)
{
    const uint64_t size = br_skel_size(d);
    if ((uint64_t)d.skel_off + size > J.skel_bytes || d.head_bytes < 36) return;        // (not the scan's descriptor: nothing is written)
    const uint8_t* r = J.image + J.rec_off[row];
    const uint64_t len = (uint64_t)bd_s32(r - 4);
    const uint32_t l_name = r[8], n_cig = bd_u16(r + 12), L = d.l_seq;
    const uint64_t cig = 32 + (uint64_t)l_name, qual = cig + 4 * (uint64_t)n_cig + ((uint64_t)L + 1) / 2, aux = qual + L;
    if (d.head_bytes != 36u + l_name + 4u * n_cig || bd_u32(r + 16) != L || aux > len) return;
    uint8_t* o = J.skel + d.skel_off;
    // the head: block_size, the 32 fixed bytes with bin computed, then QNAME and CIGAR as they are
    int64_t span = 0;
    for (uint32_t k = 0; k < n_cig; ++k) {
        const uint32_t w = bd_u32(r + cig + 4 * k), op = w & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += w >> 4;
    }
    if (span > 0x7FFFFFFF) span = 0x7FFFFFFF;
    const int64_t pos = bd_s32(r + 4);
    const uint32_t bin = br_reg2bin(pos, pos + (span > 1 ? span : 1));
    const uint32_t block = (uint32_t)(br_stream_size(d) - 4);
    for (uint32_t j = lane; j < 36; j += nl)
        o[j] = (uint8_t)(j < 4 ? block >> (8 * j) : j == 14 ? bin : j == 15 ? bin >> 8 : r[j - 4]);
    bo_segment(o + 36, d.head_bytes - 36, lane, nl, BoCopy{r + 32});
    o += d.head_bytes;
    // a kept QUAL: as read, or 0xFF throughout where the text says '*'
    const uint32_t q0 = L ? r[qual] : 0xFFu;
    const bool star = L == 0 || q0 == 0xFFu || (L == 1 && q0 == 9u);
    if (d.qual_src == KBBQ_BAM_QUAL_SKELETON) {
        if (star) bo_segment(o, L, lane, nl, BrFill{});
        else bo_segment(o, L, lane, nl, BoCopy{r + qual});
        o += L;
    }
    // the tail: unchanged runs by all lanes, a re-typed integer tag by lane 0
    uint64_t room = d.tail_bytes, p = aux;
    BrWalk W;
    memset(&W, 0, sizeof W);
    while (p < len) {
        const uint64_t q = br_walk(r, p, len, true, W);
        if ((W.met & BR_W_BAD) || q - p > room) return;
        bo_segment(o, (uint32_t)(q - p), lane, nl, BoCopy{r + p});
        o += q - p; room -= q - p;
        if (q >= len) break;
        const uint32_t nb = br_int_bytes(W.type);
        if (3 + (uint64_t)nb > room) return;
        if (lane == 0) {
            o[0] = r[q]; o[1] = r[q + 1]; o[2] = (uint8_t)W.type;
            for (uint32_t k = 0; k < nb; ++k) o[3 + k] = (uint8_t)((uint64_t)W.value >> (8 * k));
        }
        o += 3 + nb; room -= 3 + nb;
        p = q + 3 + W.old_bytes;
    }
    if (J.set_oq && !(W.met & BR_W_OQ) && !star && room == 3 + (uint64_t)L + 1) {
        if (lane == 0) { o[0] = 'O'; o[1] = 'Q'; o[2] = 'Z'; o[3 + L] = 0; }
        bo_segment(o + 3, L, lane, nl, BrPlus33{r + qual});
    }
}

#if defined(__HIPCC__)
struct BrParams {
    BrJob job; BdJob dec;
    uint32_t* any;                                       // the OR of every record's status
    uint64_t* part;                                      // [2 * blocks] per scan workgroup: skeleton and stream bytes, then their exclusive scan
    uint64_t* total;                                     // [2] skeleton and stream bytes of all records
};

__global__ __launch_bounds__(BR_THREADS) void kbr_size(BrParams p)
{
    __shared__ BrInfo info[BR_RECORDS];
    __shared__ uint32_t met[BR_RECORDS];
    const uint32_t k = threadIdx.x / BR_LANES, lane = threadIdx.x % BR_LANES, row = blockIdx.x * BR_RECORDS + k;
    const bool live = row < p.job.m;
    if (lane == 0) {
        met[k] = 0;
        if (live) br_open(p.job, p.dec, row, info[k]);
    }
    __syncthreads();
    if (live && !info[k].d.w.status) {
        const uint32_t st = bd_copy(p.dec, row, info[k].d, lane, BR_LANES);
        if (st) atomicOr(&met[k], st);
    }
    __syncthreads();
    if (live && lane == 0) {
        const uint32_t status = info[k].d.w.status | met[k];
        br_close(p.job, row, info[k], status);
        if (status) atomicOr(p.any, status);
    }
}

// the inclusive scan of (a, b) over the workgroup's BR_THREADS threads; tot: the workgroup's sums
__device__ __forceinline__ void br_scan_wg(uint64_t& a, uint64_t& b, uint64_t (&tot)[2], uint64_t (*waves)[2])
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t ua = __shfl_up((unsigned long long)a, d, 64), ub = __shfl_up((unsigned long long)b, d, 64);
        if (lane >= d) { a += ua; b += ub; }
    }
    __syncthreads();                                     // (waves[] may still be read from the call before)
    if (lane == 63) { waves[wave][0] = a; waves[wave][1] = b; }
    __syncthreads();
    tot[0] = tot[1] = 0;
    for (uint32_t w = 0; w < BR_THREADS / 64; ++w) {
        if (w < wave) { a += waves[w][0]; b += waves[w][1]; }
        tot[0] += waves[w][0]; tot[1] += waves[w][1];
    }
}

__global__ __launch_bounds__(BR_THREADS) void kbr_sums(BrParams p)
{
    __shared__ uint64_t waves[BR_THREADS / 64][2];
    const uint32_t row = blockIdx.x * BR_THREADS + threadIdx.x;
    uint64_t a = 0, b = 0, tot[2];
    if (row < p.job.m) { const kbbq_bam_desc d = p.job.desc[row]; a = br_skel_size(d); b = br_stream_size(d); }
    br_scan_wg(a, b, tot, waves);
    if (threadIdx.x == 0) { p.part[2 * blockIdx.x] = tot[0]; p.part[2 * blockIdx.x + 1] = tot[1]; }
}

// one workgroup: part[] becomes its exclusive scan, total[] the sums
__global__ __launch_bounds__(BR_THREADS) void kbr_scan_blocks(BrParams p, uint32_t nblocks)
{
    __shared__ uint64_t waves[BR_THREADS / 64][2];
    uint64_t base[2] = {0, 0};
    for (uint32_t lo = 0; lo < nblocks; lo += BR_THREADS) {
        const uint32_t i = lo + threadIdx.x;
        uint64_t a = 0, b = 0, tot[2];
        if (i < nblocks) { a = p.part[2 * i]; b = p.part[2 * i + 1]; }
        const uint64_t own_a = a, own_b = b;
        br_scan_wg(a, b, tot, waves);
        if (i < nblocks) { p.part[2 * i] = base[0] + a - own_a; p.part[2 * i + 1] = base[1] + b - own_b; }
        base[0] += tot[0]; base[1] += tot[1];
    }
    if (threadIdx.x == 0) { p.total[0] = base[0]; p.total[1] = base[1]; }
}

__global__ __launch_bounds__(BR_THREADS) void kbr_offsets(BrParams p)
{
    __shared__ uint64_t waves[BR_THREADS / 64][2];
    const uint32_t row = blockIdx.x * BR_THREADS + threadIdx.x;
    uint64_t a = 0, b = 0, tot[2];
    kbbq_bam_desc d;
    memset(&d, 0, sizeof d);
    if (row < p.job.m) { d = p.job.desc[row]; a = br_skel_size(d); b = br_stream_size(d); }
    const uint64_t own_a = a, own_b = b;
    br_scan_wg(a, b, tot, waves);
    if (row < p.job.m) {
        // (a stream of 2^31 bytes or more is refused by the caller before these offsets are used)
        p.job.desc[row].skel_off = (uint32_t)(p.part[2 * blockIdx.x] + a - own_a);
        p.job.desc[row].stream_off = (uint32_t)(p.part[2 * blockIdx.x + 1] + b - own_b);
    }
}

__global__ __launch_bounds__(BR_THREADS) void kbr_write(BrParams p)
{
    const uint32_t row = blockIdx.x * BR_RECORDS + threadIdx.x / BR_LANES, lane = threadIdx.x % BR_LANES;
    if (row >= p.job.m || p.job.status[row]) return;
    br_write(p.job, row, p.job.desc[row], lane, BR_LANES);
}
#endif
