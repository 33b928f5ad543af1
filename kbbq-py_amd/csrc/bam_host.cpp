// bam_host.cpp -- see bam_host.h.  Host only, no GPU code.
#include "bam_host.h"
#include "bam_scan.h"
#include "fast_inflate.h"
#include "host_threads.h"
#include "parallel_gunzip.h"

#include <algorithm>
#include <atomic>
#include <charconv>
#include <cstdio>
#include <cstring>
#include <thread>

#include <zlib.h>

namespace {

inline uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline int32_t les32(const uint8_t* p) { return (int32_t)le32(p); }

template <typename F> void threads_over(size_t n, unsigned nt, F f)
{
    if (nt <= 1 || n < 2) { f(0, n); return; }
    std::vector<std::thread> th;
    const size_t per = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; ++t) {
        const size_t lo = std::min(n, t * per), hi = std::min(n, lo + per);
        if (lo < hi) th.emplace_back([=]() { f(lo, hi); });
    }
    for (auto& t : th) t.join();
}

// BGZF: every member is  1f 8b 08 04 | mtime xfl os (6) | xlen (2) | subfields ... 'B' 'C' 02 00 BSIZE(2) ... | deflate | crc32 isize
// The members of s[0, n): how many, how much text; blocks (if not NULL) receives the first `cap` of them.  false: not BGZF.
bool index_bgzf(const uint8_t* s, size_t n, kbbq_bgzf_block* blocks, size_t cap, size_t* count, size_t* text)
{
    size_t at = 0, out = 0, nb = 0;
    while (at < n) {
        if (n - at < 18 || s[at] != 0x1f || s[at + 1] != 0x8b || s[at + 2] != 8 || !(s[at + 3] & 4)) return false;
        const size_t xlen = le16(s + at + 10);
        if (n - at < 12 + xlen + 8) return false;
        size_t bsize = 0;
        for (size_t x = at + 12; x + 4 <= at + 12 + xlen;) {
            const size_t slen = le16(s + x + 2);
            if (s[x] == 'B' && s[x + 1] == 'C' && slen == 2 && x + 6 <= at + 12 + xlen) bsize = (size_t)le16(s + x + 4) + 1;
            x += 4 + slen;
        }
        if (bsize < 12 + xlen + 8 || bsize > n - at) return false;
        kbbq_bgzf_block b;
        b.src = at + 12 + xlen; b.csize = (uint32_t)(bsize - (12 + xlen) - 8);
        b.crc = le32(s + at + bsize - 8); b.isize = le32(s + at + bsize - 4); b.dst = out; b.pad = 0;
        if (b.isize > (1u << 16)) return false;                               // BGZF blocks hold at most 64 KiB
        out += b.isize; at += bsize;
        if (nb < cap) blocks[nb] = b;
        ++nb;
    }
    *count = nb; *text = out;
    return true;
}

bool index_bgzf(const uint8_t* s, size_t n, std::vector<kbbq_bgzf_block>& blocks, size_t* text)
{
    size_t nb = 0;
    if (!index_bgzf(s, n, nullptr, 0, &nb, text)) return false;
    blocks.resize(nb);
    return index_bgzf(s, n, blocks.data(), nb, &nb, text);
}

// gzip members one after the other through libdeflate (fast_inflate.h); false: not available or anything but success -- zlib
// takes the input from its start and decides what is wrong with it
bool inflate_members_fast(const uint8_t* src, size_t n, kbbq_bytes& out)
{
    const kbbq_libdeflate* l = kbbq_libdeflate_get();
    if (!l || n < 18) return false;
    void* d = l->alloc_decompressor();
    if (!d) return false;
    // a single member's trailer names its inflated size (mod 2^32); several members, or more than 4 GB: the buffer grows
    out.resize(std::max<size_t>({n * 4, (size_t)le32(src + n - 4) + 64, (size_t)1 << 16}));
    size_t used = 0, at = 0;
    bool ok = true;
    while (at < n && ok) {
        size_t in_used = 0, out_used = 0;
        const int rc = l->gzip_decompress_ex(d, src + at, n - at, out.data() + used, out.size() - used, &in_used, &out_used);
        if (rc == 3) { out.resize(out.size() * 2); continue; }                 // insufficient space: the member again, into twice the room
        if (rc != 0 || in_used == 0) { ok = false; break; }
        at += in_used; used += out_used;
    }
    l->free_decompressor(d);
    if (ok) out.resize(used);
    return ok;
}

bool inflate_serial(const uint8_t* src, size_t n, kbbq_bytes& out, std::string& err)
{
    // large members on all threads (parallel_gunzip.cpp), else one thread through libdeflate, else -- and for whatever those two
    // do not report as success -- zlib
    if (n >= kbbq_pgz_min_bytes() && n >= 18 && kbbq_host_thread_ceiling() > 1) {
        out.clear();
        const size_t hint = le32(src + n - 4);                                 // one member below 4 GB: its size; else the vector grows
        out.reserve(std::max<size_t>(hint >= n ? hint : 0, n * 3));
        kbbq_advise_huge(out.data(), out.capacity());
        if (kbbq_parallel_gunzip(src, n, out, 0)) return true;
        out.clear();
    }
    if (inflate_members_fast(src, n, out)) return true;
    z_stream z; memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 15 + 32) != Z_OK) { err = "zlib: inflateInit2 failed"; return false; }
    out.resize(std::max<size_t>(n * 4, 1 << 16));
    size_t used = 0, at = 0;
    while (at < n) {
        z.next_in = const_cast<Bytef*>(src + at); z.avail_in = (uInt)std::min<size_t>(n - at, 1u << 30);
        const size_t in0 = z.avail_in;
        for (;;) {
            if (used == out.size()) out.resize(out.size() * 2);
            z.next_out = out.data() + used; z.avail_out = (uInt)std::min<size_t>(out.size() - used, 1u << 30);
            const size_t out0 = z.avail_out;
            const int rc = inflate(&z, Z_NO_FLUSH);
            used += out0 - z.avail_out;
            if (rc == Z_STREAM_END) {                                          // next member, if any
                at += in0 - z.avail_in;
                if (at < n && inflateReset(&z) != Z_OK) { inflateEnd(&z); err = "zlib: inflateReset failed"; return false; }
                break;
            }
            if (rc != Z_OK && rc != Z_BUF_ERROR) { inflateEnd(&z); err = "corrupt gzip stream"; return false; }
            if (z.avail_in == 0 && z.avail_out != 0) {                        // input exhausted inside a member
                at += in0;
                if (at >= n) { inflateEnd(&z); err = "truncated gzip stream"; return false; }
                break;
            }
        }
    }
    inflateEnd(&z);
    out.resize(used);
    return true;
}

const char kSeqCodes[] = "=ACMGRSVTWYHKDBN";
const char kCigarOps[] = "MIDNSHP=X???????";

inline void put(kbbq_bytes& o, const void* p, size_t n) { const uint8_t* b = (const uint8_t*)p; o.insert(o.end(), b, b + n); }
inline void put(kbbq_bytes& o, char c) { o.push_back((uint8_t)c); }
template <typename I> inline void put_int(kbbq_bytes& o, I v)
{
    char tmp[24];
    auto r = std::to_chars(tmp, tmp + sizeof tmp, v);
    put(o, tmp, (size_t)(r.ptr - tmp));
}
inline void put_float(kbbq_bytes& o, float v)
{
    char tmp[40];
    const int k = snprintf(tmp, sizeof tmp, "%g", (double)v);
    put(o, tmp, (size_t)std::max(k, 0));
}

// Where a thread renders its records: room() once per record for the longest line the record can become, then unchecked writes
// (vector::insert per field -- a capacity check and an iterator dance for every few bytes -- ran at 130 MB/s per thread).
struct Sink {
    kbbq_bytes buf; size_t n = 0;
    void room(size_t k) { if (buf.size() - n < k) buf.resize(std::max(buf.size() * 2, n + k)); }
    uint8_t* at() { return buf.data() + n; }
};
inline void put(Sink& o, const void* p, size_t n) { memcpy(o.at(), p, n); o.n += n; }
inline void put(Sink& o, char c) { *o.at() = (uint8_t)c; ++o.n; }
template <typename I> inline void put_int(Sink& o, I v)
{
    auto r = std::to_chars((char*)o.at(), (char*)o.at() + 24, v);
    o.n = (size_t)((uint8_t*)r.ptr - o.buf.data());
}
inline void put_float(Sink& o, float v)
{
    const int k = snprintf((char*)o.at(), 40, "%g", (double)v);
    o.n += (size_t)std::max(k, 0);
}

// one record (without its block_size word) -> one SAM line; false if the record is inconsistent.  longest_ref: of the reference names.
// No field expands more than 5x (an element of a B:c array: one byte -> ",-128"), the fixed fields are < 100 characters.
bool format_record(const uint8_t* r, size_t len, const std::vector<std::string>& refs, size_t longest_ref, Sink& o)
{
    if (len < 32) return false;
    o.room(6 * len + 2 * longest_ref + 256);
    const int32_t ref_id = les32(r), pos = les32(r + 4);
    const uint32_t l_name = r[8], mapq = r[9], n_cig = le16(r + 12), flag = le16(r + 14);
    const int32_t l_seq = les32(r + 16), next_ref = les32(r + 20), next_pos = les32(r + 24), tlen = les32(r + 28);
    if (l_seq < 0 || l_name == 0) return false;
    const size_t need = 32 + (size_t)l_name + 4 * (size_t)n_cig + ((size_t)l_seq + 1) / 2 + (size_t)l_seq;
    if (need > len) return false;
    const uint8_t* name = r + 32; const uint8_t* cig = name + l_name; const uint8_t* seq = cig + 4 * (size_t)n_cig;
    const uint8_t* qual = seq + ((size_t)l_seq + 1) / 2; const uint8_t* aux = qual + l_seq; const uint8_t* end = r + len;
    if (name[l_name - 1] != 0) return false;
    put(o, name, l_name - 1); put(o, '\t'); put_int(o, flag); put(o, '\t');
    if (ref_id < 0) put(o, '*'); else if ((size_t)ref_id < refs.size()) put(o, refs[(size_t)ref_id].data(), refs[(size_t)ref_id].size()); else return false;
    put(o, '\t'); put_int(o, (int64_t)pos + 1); put(o, '\t'); put_int(o, mapq); put(o, '\t');
    if (n_cig == 0) put(o, '*');
    for (uint32_t c = 0; c < n_cig; ++c) { const uint32_t w = le32(cig + 4 * c); put_int(o, w >> 4); put(o, kCigarOps[w & 15u]); }
    put(o, '\t');
    if (next_ref < 0) put(o, '*'); else if (next_ref == ref_id) put(o, '='); else if ((size_t)next_ref < refs.size()) put(o, refs[(size_t)next_ref].data(), refs[(size_t)next_ref].size()); else return false;
    put(o, '\t'); put_int(o, (int64_t)next_pos + 1); put(o, '\t'); put_int(o, tlen); put(o, '\t');
    if (l_seq == 0) put(o, '*');
    else {
        uint8_t* w = o.at();
        for (int32_t i = 0; i + 1 < l_seq; i += 2) { const uint8_t b = seq[i >> 1]; w[i] = (uint8_t)kSeqCodes[b >> 4]; w[i + 1] = (uint8_t)kSeqCodes[b & 15]; }
        if (l_seq & 1) w[l_seq - 1] = (uint8_t)kSeqCodes[seq[(l_seq - 1) >> 1] >> 4];
        o.n += (size_t)l_seq;
    }
    put(o, '\t');
    if (l_seq == 0 || qual[0] == 0xFF) put(o, '*');
    else { uint8_t* w = o.at(); for (int32_t i = 0; i < l_seq; ++i) w[i] = (uint8_t)(qual[i] + 33); o.n += (size_t)l_seq; }
    // optional fields: tag(2) type(1) value
    const uint8_t* p = aux;
    while (p < end) {
        if (end - p < 3) return false;
        put(o, '\t'); put(o, p, 2); put(o, ':');
        const char type = (char)p[2]; p += 3;
        auto ints = [&](char t, const uint8_t*& q) -> bool {                  // one integer / float of BAM type t
            switch (t) {
            case 'c': if (end - q < 1) return false; put_int(o, (int)(int8_t)q[0]); q += 1; return true;
            case 'C': if (end - q < 1) return false; put_int(o, (unsigned)q[0]); q += 1; return true;
            case 's': if (end - q < 2) return false; put_int(o, (int)(int16_t)le16(q)); q += 2; return true;
            case 'S': if (end - q < 2) return false; put_int(o, (unsigned)le16(q)); q += 2; return true;
            case 'i': if (end - q < 4) return false; put_int(o, les32(q)); q += 4; return true;
            case 'I': if (end - q < 4) return false; put_int(o, le32(q)); q += 4; return true;
            case 'f': { if (end - q < 4) return false; float v; const uint32_t w = le32(q); memcpy(&v, &w, 4); put_float(o, v); q += 4; return true; }
            default: return false;
            }
        };
        if (type == 'A') { if (end - p < 1) return false; put(o, "A:", 2); put(o, (char)p[0]); p += 1; }
        else if (type == 'Z' || type == 'H') {
            const uint8_t* z = (const uint8_t*)memchr(p, 0, (size_t)(end - p));
            if (!z) return false;
            put(o, type); put(o, ':'); put(o, p, (size_t)(z - p)); p = z + 1;
        } else if (type == 'B') {
            if (end - p < 5) return false;
            const char sub = (char)p[0]; const uint32_t count = le32(p + 1); p += 5;
            put(o, "B:", 2); put(o, sub);
            for (uint32_t k = 0; k < count; ++k) { put(o, ','); if (!ints(sub, p)) return false; }
        } else if (type == 'f') { put(o, "f:", 2); if (!ints('f', p)) return false; }
        else { put(o, "i:", 2); if (!ints(type, p)) return false; }
    }
    put(o, '\n');
    return true;
}

}  // namespace

bool kbbq_inflate_blocks_host(const uint8_t* src, const kbbq_bgzf_block* blocks, const uint32_t* which, size_t count, uint8_t* out,
                              size_t work, std::string& err)
{
    std::atomic<int> bad(0);
    threads_over(count, kbbq_threads_for(work), [&](size_t lo, size_t hi) {
        kbbq_block_inflater fast;
        z_stream z; memset(&z, 0, sizeof z);
        if (inflateInit2(&z, -15) != Z_OK) { bad = 1; return; }
        for (size_t b = lo; b < hi && !bad.load(); ++b) {
            const kbbq_bgzf_block& k = blocks[which ? which[b] : b];
            if (fast.block(src + k.src, k.csize, out + k.dst, k.isize, k.crc)) continue;
            Bytef nothing = 0;                                   // an empty block (bgzip's EOF marker; an empty file is ONLY that):
            z.next_in = const_cast<Bytef*>(src + k.src); z.avail_in = (uInt)k.csize;   // zlib rejects a NULL next_out
            z.next_out = k.isize ? out + k.dst : &nothing; z.avail_out = k.isize;
            const int rc = k.isize || k.csize ? inflate(&z, Z_FINISH) : Z_STREAM_END;
            if ((rc != Z_STREAM_END && !(rc == Z_OK && z.avail_out == 0)) || z.avail_out != 0
                || crc32(crc32(0L, Z_NULL, 0), k.isize ? out + k.dst : &nothing, k.isize) != k.crc) { bad = 2; break; }
            inflateReset(&z);
        }
        inflateEnd(&z);
    });
    if (bad.load()) { err = bad.load() == 1 ? "zlib: inflateInit2 failed" : "corrupt BGZF block (inflate / CRC mismatch)"; return false; }
    return true;
}

// ---- the device route of kbbq_inflate_all (include/kbbq_hip.h "BGZF input") ------------------------------------------------------------
namespace {
std::atomic<kbbq_ctx*> g_inflate_ctx(nullptr);
std::atomic<kbbq_inflate_route> g_inflate_route(nullptr);
std::atomic<uint64_t> g_inflate_stats[4];                 // device blocks, host blocks, bytes up, bytes down

size_t gpu_inflate_min_bytes()
{
    const char* e = getenv("KBBQ_GPU_INFLATE_MIN_BYTES");
    if (!e || !*e) return (size_t)1 << 20;
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    return end == e ? (size_t)1 << 20 : (size_t)v;
}
}  // namespace

void kbbq_inflate_forget_ctx_(kbbq_ctx* c)
{
    kbbq_ctx* expect = c;
    g_inflate_ctx.compare_exchange_strong(expect, nullptr);
}

void kbbq_inflate_set_route_(kbbq_ctx* c, kbbq_inflate_route route)
{
    g_inflate_route.store(route);
    g_inflate_ctx.store(route ? c : nullptr);
}

extern "C" int kbbq_inflate_stats_get(kbbq_inflate_stats* stats)
{
    if (!stats) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_inflate_stats_get: stats is NULL");
    stats->device_blocks = g_inflate_stats[0].load(); stats->host_blocks = g_inflate_stats[1].load();
    stats->bytes_up = g_inflate_stats[2].load(); stats->bytes_down = g_inflate_stats[3].load();
    return KBBQ_OK;
}

extern "C" int kbbq_inflate_index(const uint8_t* src, size_t n, kbbq_bgzf_block* blocks, size_t cap, size_t* nblocks, size_t* text_bytes)
{
    if (!nblocks || !text_bytes || (n && !src)) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_inflate_index: NULL src or result pointer");
    *nblocks = 0; *text_bytes = 0;
    if (!index_bgzf(src, n, nullptr, 0, nblocks, text_bytes)) { *nblocks = 0; *text_bytes = 0; return KBBQ_INFLATE_NOT_BGZF; }
    if (!blocks) return KBBQ_OK;
    if (cap < *nblocks) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_inflate_index: blocks holds fewer descriptors than the stream has members");
    index_bgzf(src, n, blocks, cap, nblocks, text_bytes);
    return KBBQ_OK;
}

bool kbbq_inflate_all(const uint8_t* src, size_t n, kbbq_bytes& out, std::string& err)
{
    std::vector<kbbq_bgzf_block> blocks;
    size_t total = 0;
    if (!index_bgzf(src, n, blocks, &total)) return inflate_serial(src, n, out, err);   // plain gzip (or a damaged BGZF: zlib decides)
    kbbq_resize_fresh(out, total);
    kbbq_ctx* ctx = g_inflate_ctx.load();
    const kbbq_inflate_route route = g_inflate_route.load();
    const char* on = getenv("KBBQ_GPU_INFLATE");
    if (ctx && route && on && on[0] == '1' && !on[1] && n >= gpu_inflate_min_bytes()) {
        kbbq_inflate_stats st;
        bool data_error = false;
        const int rc = route(ctx, src, n, blocks.data(), blocks.size(), out.data(), &st, &data_error);
        if (rc == KBBQ_OK) {
            g_inflate_stats[0] += st.device_blocks; g_inflate_stats[1] += st.host_blocks;
            g_inflate_stats[2] += st.bytes_up; g_inflate_stats[3] += st.bytes_down;
            return true;
        }
        if (data_error) { err = "corrupt BGZF block (inflate / CRC mismatch)"; return false; }
        // anything else (no memory, a HIP error): the host route, as if no context had been registered
    }
    return kbbq_inflate_blocks_host(src, blocks.data(), nullptr, blocks.size(), out.data(), n, err);
}

bool kbbq_bam_to_sam(const uint8_t* bam, size_t n, kbbq_bytes& text, std::string& err)
{
    kbbq_bam_head H;
    if (!kbbq_bam_read_head(bam, n, H, err)) return false;
    const std::vector<std::string>& refs = H.refs;
    text.clear();
    kbbq_bam_head_text(H, text);
    // record offsets (a chain of block_size words), then the lines in parallel
    std::vector<size_t> rec;
    if (!kbbq_bam_chain(bam, n, H.records_off, err, [&](size_t body, size_t) { rec.push_back(body); })) return false;
    rec.push_back(n + 4);
    const unsigned nt = kbbq_threads_for(n);
    std::vector<Sink> parts(nt);
    std::atomic<long long> bad(-1);
    const size_t nrec = rec.size() - 1, per = (nrec + nt - 1) / std::max(1u, nt);
    size_t longest_ref = 0;
    for (const auto& nm : refs) longest_ref = std::max(longest_ref, nm.size());
    kbbq_parallel(nt, [&](unsigned t) {
        const size_t lo = std::min(nrec, t * per), hi = std::min(nrec, lo + per);
        if (lo >= hi) return;
        Sink& o = parts[t];
        kbbq_resize_fresh(o.buf, (rec[hi] - rec[lo]) * 2 + 4096);
        for (size_t i = lo; i < hi; ++i)
            if (!format_record(bam + rec[i], rec[i + 1] - rec[i] - 4, refs, longest_ref, o)) {
                long long cur = bad.load();
                while ((cur < 0 || (long long)i < cur) && !bad.compare_exchange_weak(cur, (long long)i)) {}
                return;
            }
    });
    if (bad.load() >= 0) { err = "BAM: malformed alignment record " + std::to_string(bad.load()); return false; }
    std::vector<size_t> at_part(nt + 1, text.size());                          // the parts side by side into their places
    for (unsigned t = 0; t < nt; ++t) at_part[t + 1] = at_part[t] + parts[t].n;
    kbbq_resize_fresh(text, at_part[nt]);
    kbbq_parallel(nt, [&](unsigned t) {
        if (parts[t].n) memcpy(text.data() + at_part[t], parts[t].buf.data(), parts[t].n);
        kbbq_bytes().swap(parts[t].buf);
    });
    return true;
}

// ---- BAM input: what the decode needs of an image (include/kbbq_hip.h "BAM input"; the records themselves: kbbq_bam_in.h) --------
extern "C" int kbbq_bam_scan(const uint8_t* image, size_t n, kbbq_bam_scan_info* info, uint8_t* header, uint32_t* rg_off, uint8_t* rg_ids,
                             uint64_t* rec_off, uint64_t* cig_off)
{
    if (!info || (n && !image)) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_bam_scan: NULL image or info");
    memset(info, 0, sizeof *info);
    kbbq_bam_head H;
    std::string err;
    if (!kbbq_bam_read_head(image, n, H, err)) return kbbq_set_error_(KBBQ_E_ARG, err.c_str());
    kbbq_bytes text;
    kbbq_bam_head_text(H, text);
    std::vector<std::string> ids;
    kbbq_bam_rg_ids(text.data(), text.size(), ids);
    if (ids.size() > (size_t)INT32_MAX) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_bam_scan: more than 2^31 - 1 @RG lines");
    size_t rg_bytes = 0;
    for (const auto& id : ids) rg_bytes += id.size();
    if (rg_bytes > UINT32_MAX) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_bam_scan: the @RG IDs take 4 GiB or more");
    // the chain is one read of block_size; l_seq and n_cigar_op lie in the same cache line
    int64_t count = 0, max_l_seq = 0;
    uint64_t cig = 0, max_record = 0;
    if (cig_off) cig_off[0] = 0;
    if (!kbbq_bam_chain(image, n, H.records_off, err, [&](size_t body, size_t bs) {
            const uint64_t n_cig = (uint64_t)image[body + 12] | (uint64_t)image[body + 13] << 8;
            max_l_seq = std::max<int64_t>(max_l_seq, kbbq_bam_les32(image + body + 16));
            max_record = std::max<uint64_t>(max_record, bs + 4);
            if (rec_off) rec_off[count] = body;
            cig += n_cig;
            if (cig_off) cig_off[count + 1] = cig;
            ++count;
        })) return kbbq_set_error_(KBBQ_E_ARG, err.c_str());
    info->n = count; info->cig_total = (int64_t)cig; info->max_l_seq = (int32_t)max_l_seq; info->n_ref = H.n_ref;
    info->n_rg = (int32_t)ids.size(); info->header_bytes = text.size(); info->rg_bytes = rg_bytes; info->refs_off = H.refs_off;
    info->records_off = H.records_off; info->max_record = max_record;
    if (header && !text.empty()) memcpy(header, text.data(), text.size());
    if (rg_off) {
        uint32_t at = 0;
        for (size_t g = 0; g < ids.size(); ++g) {
            rg_off[g] = at;
            if (rg_ids && !ids[g].empty()) memcpy(rg_ids + at, ids[g].data(), ids[g].size());
            at += (uint32_t)ids[g].size();
        }
        rg_off[ids.size()] = at;
    }
    return KBBQ_OK;
}
