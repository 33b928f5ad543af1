// sam_host.cpp -- host-side SAM text reader for the truth-set benchmark and the BAM-sourced tally (no GPU code).
//
// Replaces, for those paths, what the reference gets from pysam.AlignmentFile / AlignedSegment
// (benchmark.py:57-74,102-143; gatk/bqsr.py:23-123): per alignment the flag, contig, position, CIGAR,
// mate position, template length, sequence, qualities and the RG / OQ tags -- as ARRAYS, because the
// kernels (K4 find_errors, K6 canonical reads) take whole batches.  The file is mapped, lines are indexed and
// parsed in parallel; BAM and gzip-compressed SAM are inflated (BGZF blocks in parallel) and BAM records rendered
// as SAM lines first (bam_host.cpp: zlib only, no htslib).
//
// Field semantics follow the SAM specification and pysam's attribute definitions:
//   reference_start = POS - 1; next_reference_start = PNEXT - 1; reference_end = start + sum of M/D/N/=/X;
//   query_alignment_start / _end = leading / trailing soft clip (hard clips outside them are ignored).
// CIGAR operations are stored as (length << 4 | op) with BAM op codes MIDNSHP=X = 0..8; an unknown
// operation letter is stored as op 15 and rejected by K4 (ValueError, like the reference's walk).
#include "../../include/kbbq_hip.h"
#include "kbbq_lib_host.h"
#include "host_threads.h"
#include "bam_host.h"

#include <algorithm>
#include <atomic>
#include <functional>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

struct kbbq_sam {
    const uint8_t* buf = nullptr; size_t size = 0;
    kbbq_bytes owned;                          // the text when it was inflated / rendered from BAM instead of mapped
    std::vector<uint64_t> hdr0; std::vector<uint32_t> hdrlen;      // header lines ('@...')
    std::vector<uint64_t> line0; std::vector<uint32_t> linelen;    // alignment lines
    // per alignment
    std::vector<uint32_t> name_len, seq_len, qual_len, oq_len, rgtag_len, cig_n, clip;
    std::vector<uint64_t> seq0, qual0, oq0, rgtag0, cig_off;
    std::vector<int32_t> flag, contig, ref_span, rg;
    std::vector<int64_t> pos, pnext, tlen;
    std::vector<uint32_t> cigar;
    std::vector<std::string> contigs;          // first-appearance order of RNAME
    std::vector<std::string> rg_ids;           // @RG ID in header order
    ~kbbq_sam() { if (buf && owned.empty()) munmap((void*)buf, size); }
};

namespace {

unsigned threads_for(size_t work) { return kbbq_threads_for(work); }

template <typename F> void par_for(int64_t n, unsigned nt, F f)
{
    if (nt <= 1 || n < 4096) { f(0, n); return; }
    kbbq_parallel_parts((size_t)n, nt, [&](unsigned, size_t lo, size_t hi) { f((int64_t)lo, (int64_t)hi); });      // parked workers (host_threads.h)
}

bool parse_int(const uint8_t* p, const uint8_t* e, int64_t& out)
{
    if (p >= e) return false;
    bool neg = false;
    if (*p == '-' || *p == '+') { neg = *p == '-'; ++p; if (p >= e) return false; }
    int64_t v = 0;
    for (; p < e; ++p) {
        if (*p < '0' || *p > '9') return false;
        if (v > (INT64_MAX - 9) / 10) return false;
        v = v * 10 + (*p - '0');
    }
    out = neg ? -v : v;
    return true;
}

int cigar_code(uint8_t c)
{
    switch (c) {
        case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
        case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; default: return 15;
    }
}

// one pass over a CIGAR string: count the operations (ops == nullptr) or write them
int64_t walk_cigar(const uint8_t* p, const uint8_t* e, uint32_t* ops, bool& bad)
{
    if (e - p == 1 && *p == '*') return 0;
    int64_t n = 0; uint64_t len = 0; bool have = false;
    for (; p < e; ++p) {
        if (*p >= '0' && *p <= '9') { len = len * 10 + (uint64_t)(*p - '0'); have = true; if (len > 0x0FFFFFFFull) bad = true; }
        else {
            if (!have) bad = true;
            if (ops) ops[n] = (uint32_t)(len << 4) | (uint32_t)cigar_code(*p);
            ++n; len = 0; have = false;
        }
    }
    if (have) bad = true;                       // trailing digits without an operation
    return n;
}

}  // namespace

extern "C" {

int kbbq_sam_open(const char* path, kbbq_sam** out)
{
    if (!path || !out) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_open: NULL argument");
    *out = nullptr;
    int fd = open(path, O_RDONLY);
    if (fd < 0) return kbbq_set_error_(KBBQ_E_ARG, (std::string("cannot open ") + path).c_str());
    struct stat st;
    if (fstat(fd, &st) != 0) { close(fd); return kbbq_set_error_(KBBQ_E_ARG, "fstat failed"); }
    kbbq_sam* f = new kbbq_sam();
    f->size = (size_t)st.st_size;
    if (f->size) {
        void* m = mmap(nullptr, f->size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) { close(fd); f->size = 0; delete f; return kbbq_set_error_(KBBQ_E_ARG, "mmap failed"); }
        f->buf = (const uint8_t*)m;
        madvise(m, f->size, MADV_SEQUENTIAL);
    }
    close(fd);
    if (f->size >= 4 && (!memcmp(f->buf, "BAM\1", 4) || (f->buf[0] == 0x1f && f->buf[1] == 0x8b))) {
        // gzip / BGZF: inflate; BAM (inflated or not): render the records as SAM lines; then parse the text as usual
        kbbq_bytes raw, text; std::string err;
        bool ok = true;
        const bool zipped = f->buf[0] == 0x1f;
        if (zipped) ok = kbbq_inflate_all(f->buf, f->size, raw, err);
        const uint8_t* img = zipped ? raw.data() : f->buf; const size_t img_n = zipped ? raw.size() : f->size;
        const bool bam = ok && img_n >= 4 && !memcmp(img, "BAM\1", 4);
        if (bam) ok = kbbq_bam_to_sam(img, img_n, text, err);
        if (!ok) { delete f; return kbbq_set_error_(KBBQ_E_ARG, (std::string(path) + ": " + err).c_str()); }
        munmap((void*)f->buf, f->size);
        f->owned = bam ? std::move(text) : std::move(raw);
        if (f->owned.empty()) f->owned.push_back('\n');          // keeps "owned" distinguishable from "mapped"
        f->buf = f->owned.data(); f->size = f->owned.size();
    }
    // line ends, in parallel; then every thread classifies ITS lines (blank / header / alignment) into lists of its own, which are
    // concatenated in thread order = file order (round 4: this loop and the list merge used to run on one thread: 16 M lines)
    const unsigned nt = threads_for(f->size);
    struct Part { std::vector<uint64_t> nl, hdr0, line0; std::vector<uint32_t> hdrlen, linelen; uint64_t first_start = 0; };
    std::vector<Part> parts(nt);
    const size_t per = (f->size + nt - 1) / std::max(nt, 1u);
    kbbq_parallel(nt, [&](unsigned t) {
        const size_t lo = std::min(f->size, (size_t)t * per), hi = std::min(f->size, lo + per);
        const uint8_t* p = f->buf + lo; const uint8_t* e = f->buf + hi;
        auto& v = parts[t].nl;
        v.reserve((hi - lo) / 200 + 16);
        while (p < e) {
            const uint8_t* nl = (const uint8_t*)memchr(p, '\n', (size_t)(e - p));
            if (!nl) break;
            v.push_back((uint64_t)(nl - f->buf));
            p = nl + 1;
        }
    });
    {
        // the last line may lack its line end; a part's first line starts behind the last line end of the parts before it
        int last = -1;
        for (unsigned t = 0; t < nt; ++t) if (!parts[t].nl.empty()) last = (int)t;
        if (f->size && (last < 0 || parts[(size_t)last].nl.back() != f->size - 1)) parts[nt - 1].nl.push_back(f->size);
        uint64_t start = 0;
        for (unsigned t = 0; t < nt; ++t) { parts[t].first_start = start; if (!parts[t].nl.empty()) start = parts[t].nl.back() + 1; }
    }
    kbbq_parallel(nt, [&](unsigned t) {
        Part& P = parts[t];
        uint64_t start = P.first_start;
        for (uint64_t end : P.nl) {
            uint64_t e = end;
            if (e > start && f->buf[e - 1] == '\r') --e;
            bool blank = true;
            for (uint64_t k = start; k < e; ++k) if (f->buf[k] != ' ' && f->buf[k] != '\t') { blank = false; break; }
            if (!blank) {
                if (f->buf[start] == '@') { P.hdr0.push_back(start); P.hdrlen.push_back((uint32_t)(e - start)); }
                else { P.line0.push_back(start); P.linelen.push_back((uint32_t)(e - start)); }
            }
            start = end + 1;
        }
    });
    {
        size_t nh = 0, nl_ = 0;
        for (auto& P : parts) { nh += P.hdr0.size(); nl_ += P.line0.size(); }
        f->hdr0.reserve(nh); f->hdrlen.reserve(nh); f->line0.resize(nl_); f->linelen.resize(nl_);
        std::vector<size_t> at(nt + 1, 0);
        for (unsigned t = 0; t < nt; ++t) at[t + 1] = at[t] + parts[t].line0.size();
        for (auto& P : parts) { f->hdr0.insert(f->hdr0.end(), P.hdr0.begin(), P.hdr0.end()); f->hdrlen.insert(f->hdrlen.end(), P.hdrlen.begin(), P.hdrlen.end()); }
        kbbq_parallel(nt, [&](unsigned t) {
            if (parts[t].line0.empty()) return;
            memcpy(f->line0.data() + at[t], parts[t].line0.data(), parts[t].line0.size() * sizeof(uint64_t));
            memcpy(f->linelen.data() + at[t], parts[t].linelen.data(), parts[t].linelen.size() * sizeof(uint32_t));
        });
    }
    // @RG IDs in header order
    for (size_t h = 0; h < f->hdr0.size(); ++h) {
        const uint8_t* p = f->buf + f->hdr0[h]; const uint8_t* e = p + f->hdrlen[h];
        if (e - p < 3 || memcmp(p, "@RG", 3) != 0) continue;
        std::string id;
        const uint8_t* q = p;
        while (q < e) {
            const uint8_t* t = (const uint8_t*)memchr(q, '\t', (size_t)(e - q));
            const uint8_t* fe = t ? t : e;
            if (fe - q > 3 && q[0] == 'I' && q[1] == 'D' && q[2] == ':') id.assign((const char*)q + 3, (size_t)(fe - q - 3));
            q = fe + 1;
        }
        f->rg_ids.push_back(id);
    }
    std::unordered_map<std::string, int> rgmap;
    for (size_t i = 0; i < f->rg_ids.size(); ++i) rgmap.emplace(f->rg_ids[i], (int)i);

    const int64_t n = (int64_t)f->line0.size();
    std::vector<uint64_t> rname0, cig0; std::vector<uint32_t> rname_len, cig_len;
    {
        // 23 arrays of n entries (2 GB at 16 M alignments): sized and zeroed side by side instead of one after the other
        // (huge pages asked for behind the large ones: raw_vector.h)
        auto fresh = [](auto& v, size_t count, auto value) {
            using T = typename std::remove_reference_t<decltype(v)>::value_type;
            if (count * sizeof(T) >= ((size_t)8 << 20) && v.capacity() < count) { v.reserve(count); kbbq_advise_huge(v.data(), v.capacity() * sizeof(T)); }
            v.assign(count, (T)value);
        };
        const std::function<void()> fills[] = {
            [&]() { fresh(f->name_len, (size_t)(n), 0); }, [&]() { fresh(f->seq_len, (size_t)(n), 0); }, [&]() { fresh(f->qual_len, (size_t)(n), 0); }, [&]() { fresh(f->oq_len, (size_t)(n), 0); },
            [&]() { fresh(f->rgtag_len, (size_t)(n), 0); }, [&]() { fresh(f->cig_n, (size_t)(n), 0); }, [&]() { fresh(f->clip, (size_t)(n), 0); }, [&]() { fresh(f->seq0, (size_t)(n), 0); },
            [&]() { fresh(f->qual0, (size_t)(n), 0); }, [&]() { fresh(f->oq0, (size_t)(n), 0); }, [&]() { fresh(f->rgtag0, (size_t)(n), 0); }, [&]() { fresh(f->cig_off, (size_t)(n + 1), 0); },
            [&]() { fresh(f->flag, (size_t)(n), 0); }, [&]() { fresh(f->contig, (size_t)(n), -1); }, [&]() { fresh(f->ref_span, (size_t)(n), 0); }, [&]() { fresh(f->rg, (size_t)(n), -1); },
            [&]() { fresh(f->pos, (size_t)(n), 0); }, [&]() { fresh(f->pnext, (size_t)(n), 0); }, [&]() { fresh(f->tlen, (size_t)(n), 0); }, [&]() { fresh(rname0, (size_t)(n), 0); },
            [&]() { fresh(cig0, (size_t)(n), 0); }, [&]() { fresh(rname_len, (size_t)(n), 0); }, [&]() { fresh(cig_len, (size_t)(n), 0); }};
        const unsigned nf = (unsigned)(sizeof fills / sizeof fills[0]);
        std::atomic<unsigned> next(0);
        kbbq_parallel(std::min(nt, nf), [&](unsigned) { for (unsigned k; (k = next.fetch_add(1)) < nf;) fills[k](); });
    }
    std::atomic<int64_t> badline(-1);
    auto flagbad = [&](int64_t i) { int64_t cur = badline.load(); while ((cur < 0 || i < cur) && !badline.compare_exchange_weak(cur, i)) {} };
    // pass 1: split fields, numbers, tags, count CIGAR operations
    par_for(n, nt, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const uint8_t* p = f->buf + f->line0[i]; const uint8_t* e = p + f->linelen[i];
            const uint8_t* fs[12]; const uint8_t* fe[12]; int nf = 0;
            const uint8_t* q = p;
            while (nf < 11 && q <= e) {
                const uint8_t* t = (const uint8_t*)memchr(q, '\t', (size_t)(e - q));
                fs[nf] = q; fe[nf] = t ? t : e; ++nf;
                if (!t) { q = e + 1; break; }
                q = t + 1;
            }
            if (nf < 11) { flagbad(i); continue; }
            int64_t v;
            f->name_len[i] = (uint32_t)(fe[0] - fs[0]);
            if (!parse_int(fs[1], fe[1], v)) { flagbad(i); continue; }
            f->flag[i] = (int32_t)v;
            rname0[i] = (uint64_t)(fs[2] - f->buf); rname_len[i] = (uint32_t)(fe[2] - fs[2]);
            if (!parse_int(fs[3], fe[3], v)) { flagbad(i); continue; }
            f->pos[i] = v - 1;
            cig0[i] = (uint64_t)(fs[5] - f->buf); cig_len[i] = (uint32_t)(fe[5] - fs[5]);
            if (!parse_int(fs[7], fe[7], v)) { flagbad(i); continue; }
            f->pnext[i] = v - 1;
            if (!parse_int(fs[8], fe[8], v)) { flagbad(i); continue; }
            f->tlen[i] = v;
            f->seq0[i] = (uint64_t)(fs[9] - f->buf); f->seq_len[i] = (uint32_t)(fe[9] - fs[9]);
            f->qual0[i] = (uint64_t)(fs[10] - f->buf); f->qual_len[i] = (uint32_t)(fe[10] - fs[10]);
            if (f->seq_len[i] > 65535) { flagbad(i); continue; }
            bool bad = false;
            f->cig_n[i] = (uint32_t)walk_cigar(fs[5], fe[5], nullptr, bad);
            if (bad) { flagbad(i); continue; }
            // tags
            while (q < e) {
                const uint8_t* t = (const uint8_t*)memchr(q, '\t', (size_t)(e - q));
                const uint8_t* te = t ? t : e;
                if (te - q >= 5 && q[2] == ':' && q[4] == ':') {
                    if (q[0] == 'R' && q[1] == 'G' && q[3] == 'Z') { f->rgtag0[i] = (uint64_t)(q + 5 - f->buf); f->rgtag_len[i] = (uint32_t)(te - q - 5) + 1; }
                    else if (q[0] == 'O' && q[1] == 'Q' && q[3] == 'Z') { f->oq0[i] = (uint64_t)(q + 5 - f->buf); f->oq_len[i] = (uint32_t)(te - q - 5) + 1; }
                }
                q = te + 1;
            }
            if (f->rgtag_len[i]) {
                auto it = rgmap.find(std::string((const char*)f->buf + f->rgtag0[i], f->rgtag_len[i] - 1));
                f->rg[i] = it == rgmap.end() ? -2 : it->second;          // -2: tag names a group the header lacks
            }
        }
    });
    if (badline.load() >= 0) {
        const int64_t b = badline.load();
        const std::string head((const char*)f->buf + f->line0[b], std::min<size_t>(60, f->linelen[b]));
        delete f;
        return kbbq_set_error_(KBBQ_E_RANGE, ("not a SAM alignment line: " + head).c_str());
    }
    // contigs in first-appearance order (serial: the order matters)
    std::unordered_map<std::string, int> cmap;
    const uint8_t* last_name = nullptr; uint32_t last_len = 0; int last_id = -1;        // neighbours mostly share a contig: no string, no hash for them
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t* nm = f->buf + rname0[i];
        if (last_name && rname_len[i] == last_len && memcmp(nm, last_name, last_len) == 0) f->contig[i] = last_id;
        else {
            std::string name((const char*)nm, rname_len[i]);
            auto it = cmap.find(name);
            if (it == cmap.end()) { it = cmap.emplace(name, (int)f->contigs.size()).first; f->contigs.push_back(name); }
            f->contig[i] = last_id = it->second; last_name = nm; last_len = rname_len[i];
        }
        f->cig_off[i + 1] = f->cig_off[i] + f->cig_n[i];
    }
    f->cigar.assign(f->cig_off[n], 0);
    // pass 2: CIGAR operations, reference span, soft clips
    par_for(n, nt, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            bool bad = false;
            uint32_t* ops = f->cigar.data() + f->cig_off[i];
            const int64_t m = walk_cigar(f->buf + cig0[i], f->buf + cig0[i] + cig_len[i], ops, bad);
            int64_t span = 0;
            for (int64_t k = 0; k < m; ++k) { const uint32_t op = ops[k] & 15u; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += ops[k] >> 4; }
            f->ref_span[i] = (int32_t)std::min<int64_t>(span, INT32_MAX);
            int64_t lead = 0, tail = 0;
            for (int64_t k = 0; k < m; ++k) { const uint32_t op = ops[k] & 15u; if (op == 4) lead += ops[k] >> 4; else if (op != 5) break; }
            for (int64_t k = m - 1; k >= 0; --k) { const uint32_t op = ops[k] & 15u; if (op == 4) tail += ops[k] >> 4; else if (op != 5) break; }
            const int64_t L = (f->seq_len[i] == 1 && f->buf[f->seq0[i]] == '*') ? 0 : f->seq_len[i];
            const int64_t qs = std::min<int64_t>(lead, 65535), qe = std::max<int64_t>(0, std::min<int64_t>(L - tail, 65535));
            f->clip[i] = (uint32_t)qs | ((uint32_t)qe << 16);
        }
    });
    *out = f;
    return KBBQ_OK;
}

int kbbq_sam_close(kbbq_sam* f) { delete f; return KBBQ_OK; }

// ---- a whole text file, inflated if it is gzip / bgzip: what the Python-side readers of FASTA / VCF / BED files take their bytes from
// (bgzip blocks side by side, gzip members chunk-wise: bam_host.cpp kbbq_inflate_all) instead of Python's gzip module on one thread
struct kbbq_text { const uint8_t* buf = nullptr; size_t size = 0; bool mapped = false; kbbq_bytes owned;
                   ~kbbq_text() { if (mapped && buf) munmap((void*)buf, size); } };

int kbbq_text_open(const char* path, kbbq_text** out, const uint8_t** data, size_t* n)
{
    if (!path || !out || !data || !n) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_text_open: NULL argument");
    *out = nullptr; *data = nullptr; *n = 0;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return kbbq_set_error_(KBBQ_E_ARG, (std::string("cannot open ") + path).c_str());
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { close(fd); return kbbq_set_error_(KBBQ_E_ARG, (std::string(path) + ": not a regular file").c_str()); }
    kbbq_text* t = new kbbq_text();
    t->size = (size_t)st.st_size;
    if (t->size) {
        void* m = mmap(nullptr, t->size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) { close(fd); delete t; return kbbq_set_error_(KBBQ_E_ARG, "mmap failed"); }
        t->buf = (const uint8_t*)m; t->mapped = true;
    }
    close(fd);
    if (t->size >= 2 && t->buf[0] == 0x1f && t->buf[1] == 0x8b) {
        std::string err;
        if (!kbbq_inflate_all(t->buf, t->size, t->owned, err)) { delete t; return kbbq_set_error_(KBBQ_E_ARG, (std::string(path) + ": " + err).c_str()); }
        munmap((void*)t->buf, t->size);
        t->mapped = false; t->buf = t->owned.data(); t->size = t->owned.size();
    }
    *out = t; *data = t->buf; *n = t->size;
    return KBBQ_OK;
}

int kbbq_text_close(kbbq_text* t) { delete t; return KBBQ_OK; }

// info = { alignments, CIGAR operations in total, longest SEQ, contigs seen, @RG lines, header lines }
int kbbq_sam_info(const kbbq_sam* f, int64_t* info6)
{
    if (!f || !info6) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_info: NULL argument");
    const int64_t n = (int64_t)f->line0.size();
    int64_t maxlen = 0;
    for (int64_t i = 0; i < n; ++i) maxlen = std::max<int64_t>(maxlen, f->seq_len[i]);
    info6[0] = n; info6[1] = (int64_t)f->cigar.size(); info6[2] = maxlen; info6[3] = (int64_t)f->contigs.size();
    info6[4] = (int64_t)f->rg_ids.size(); info6[5] = (int64_t)f->hdr0.size();
    return KBBQ_OK;
}

// any output pointer may be NULL
int kbbq_sam_fields(const kbbq_sam* f, int32_t* flag, int32_t* contig, int64_t* pos, int64_t* pnext, int64_t* tlen,
                    int32_t* qlen, int32_t* ref_span, uint32_t* clip, uint32_t* cig_off, uint32_t* cig_n, int32_t* rg,
                    int32_t* has_qual_oq)
{
    if (!f) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_fields: NULL handle");
    const int64_t n = (int64_t)f->line0.size();
    if (has_qual_oq)                                             // the two lengths share one int32: 16 bits / 15 bits
        for (int64_t i = 0; i < n; ++i)
            if (f->qual_len[i] > 65535 || f->oq_len[i] > 32768)
                return kbbq_set_error_(KBBQ_E_ARG, "a QUAL field longer than 65535 or an OQ tag longer than 32768 characters: malformed line");
    par_for(n, threads_for((size_t)n * 64), [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i) {
        if (flag) flag[i] = f->flag[i];
        if (contig) contig[i] = f->contig[i];
        if (pos) pos[i] = f->pos[i];
        if (pnext) pnext[i] = f->pnext[i];
        if (tlen) tlen[i] = f->tlen[i];
        if (qlen) qlen[i] = (f->seq_len[i] == 1 && f->buf[f->seq0[i]] == '*') ? 0 : (int32_t)f->seq_len[i];
        if (ref_span) ref_span[i] = f->ref_span[i];
        if (clip) clip[i] = f->clip[i];
        if (cig_off) cig_off[i] = (uint32_t)f->cig_off[i];
        if (cig_n) cig_n[i] = f->cig_n[i];
        if (rg) rg[i] = f->rg[i];
        if (has_qual_oq) {
            const bool noqual = f->qual_len[i] == 1 && f->buf[f->qual0[i]] == '*';
            has_qual_oq[i] = (noqual ? 0 : (int32_t)f->qual_len[i]) | (f->oq_len[i] ? (int32_t)(f->oq_len[i] - 1) << 16 : -65536);
        }
    }
    });
    return KBBQ_OK;
}

int kbbq_sam_cigar(const kbbq_sam* f, uint32_t* ops)
{
    if (!f || (!ops && !f->cigar.empty())) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_cigar: NULL argument");
    if (!f->cigar.empty()) memcpy(ops, f->cigar.data(), f->cigar.size() * sizeof(uint32_t));
    return KBBQ_OK;
}

// Query positions [lo, hi) of every alignment that lie past its adaptor boundary, as lo | hi << 16 (0: nothing to trim) --
// what gatk/bqsr.py bamread_adaptor_boundary + _trim_range compute per read (reference bqsr.py:131-206), for all
// alignments at once: the boundary from FLAG / POS / PNEXT / TLEN, then one walk over the CIGAR of the few reads it falls into.
int kbbq_sam_adaptor_trim(const kbbq_sam* f, uint32_t* trim)
{
    if (!f || (!trim && !f->line0.empty())) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_adaptor_trim: NULL argument");
    const int64_t n = (int64_t)f->line0.size();
    par_for(n, threads_for((size_t)n * 64), [&](int64_t lo_i, int64_t hi_i) {
    for (int64_t i = lo_i; i < hi_i; ++i) {
        trim[i] = 0;
        const int32_t fl = f->flag[i];
        const bool rev = fl & 16, mate_rev = fl & 32;
        if (f->tlen[i] == 0 || !(fl & 1) || (fl & 4) || (fl & 8) || rev == mate_rev) continue;
        const int64_t start = f->pos[i], end = start + f->ref_span[i];
        const bool noqual = f->qual_len[i] == 1 && f->buf[f->qual0[i]] == '*';
        const int64_t nq = noqual ? 0 : (int64_t)f->qual_len[i];
        const uint32_t* ops = f->cigar.data() + f->cig_off[i];
        const int64_t nops = f->cig_n[i];
        auto on_query_and_ref = [](uint32_t op) { return op == 0 || op == 7 || op == 8; };
        int64_t lo = 0, hi = 0;
        if (rev) {
            if (!(end - 1 > f->pnext[i])) continue;
            const int64_t boundary = f->pnext[i] - 1;
            if (boundary < start) continue;
            int64_t q = 0, r = end;
            for (int64_t k = 0; k < nops; ++k) { const uint32_t op = ops[k] & 15; if (on_query_and_ref(op) || op == 1 || op == 4) q += ops[k] >> 4; }
            bool reached = false, found = false;
            for (int64_t k = nops - 1; k >= 0 && !found; --k) {
                const uint32_t op = ops[k] & 15; const int64_t l = ops[k] >> 4;
                if (on_query_and_ref(op)) {
                    if (reached) { hi = q; found = true; }
                    else if (r - l <= boundary) { hi = q - ((r - 1) - std::min(boundary, r - 1)); found = true; }
                    else { q -= l; r -= l; }
                } else if (op == 1 || op == 4) {
                    if (reached) { hi = q; found = true; } else q -= l;
                } else if (op == 2 || op == 3) {
                    if (r - l <= boundary) reached = true;
                    r -= l;
                }
            }
            if (!found) continue;
        } else {
            if (!(start <= f->pnext[i] + f->tlen[i])) continue;
            const int64_t boundary = start + (f->tlen[i] < 0 ? -f->tlen[i] : f->tlen[i]);
            if (boundary > end - 1) continue;
            int64_t q = 0, r = start;
            bool reached = false, found = false;
            hi = nq;
            for (int64_t k = 0; k < nops && !found; ++k) {
                const uint32_t op = ops[k] & 15; const int64_t l = ops[k] >> 4;
                if (on_query_and_ref(op)) {
                    if (reached) { lo = q; found = true; }
                    else if (r + l > boundary) { lo = q + std::max<int64_t>(boundary - r, 0); found = true; }
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
        trim[i] = (uint32_t)(lo & 0xFFFF) | (uint32_t)(hi & 0xFFFF) << 16;
    }
    });
    return KBBQ_OK;
}

// which: 0 SEQ, 1 QUAL, 2 OQ tag; rows [0, n) <- alignments [first, first + n), zero padded; a missing / '*' field
// leaves its row zero
int kbbq_sam_fill(const kbbq_sam* f, int64_t first, int64_t n, int pitch, int which, uint8_t* plane)
{
    if (!f || (n > 0 && !plane)) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_fill: NULL argument");
    if (first < 0 || n < 0 || first + n > (int64_t)f->line0.size() || pitch <= 0 || which < 0 || which > 2)
        return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_fill: bad range / pitch / plane");
    par_for(n, threads_for((size_t)n * (size_t)pitch), [&](int64_t lo, int64_t hi) {
        for (int64_t r = lo; r < hi; ++r) {
            const int64_t i = first + r;
            uint64_t off; uint32_t len;
            if (which == 0) { off = f->seq0[i]; len = f->seq_len[i]; }
            else if (which == 1) { off = f->qual0[i]; len = f->qual_len[i]; }
            else { off = f->oq0[i]; len = f->oq_len[i] ? f->oq_len[i] - 1 : 0; }
            if (len == 1 && which != 2 && f->buf[off] == '*') len = 0;
            len = std::min<uint32_t>(len, (uint32_t)pitch);
            uint8_t* row = plane + (size_t)r * pitch;
            if (len) memcpy(row, f->buf + off, len);
            memset(row + len, 0, (size_t)pitch - len);
        }
    });
    return KBBQ_OK;
}

// what: 0 QNAME of alignment i, 1 whole alignment line i, 2 header line i, 3 contig name i, 4 @RG ID i
int kbbq_sam_text(const kbbq_sam* f, int what, int64_t i, const char** p, int64_t* len)
{
    if (!f || !p || !len) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_text: NULL argument");
    const int64_t lim = what <= 1 ? (int64_t)f->line0.size() : what == 2 ? (int64_t)f->hdr0.size()
                      : what == 3 ? (int64_t)f->contigs.size() : what == 4 ? (int64_t)f->rg_ids.size() : -1;
    if (i < 0 || i >= lim) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_text: index out of range");
    switch (what) {
        case 0: *p = (const char*)f->buf + f->line0[i]; *len = f->name_len[i]; break;
        case 1: *p = (const char*)f->buf + f->line0[i]; *len = f->linelen[i]; break;
        case 2: *p = (const char*)f->buf + f->hdr0[i]; *len = f->hdrlen[i]; break;
        case 3: *p = f->contigs[i].data(); *len = (int64_t)f->contigs[i].size(); break;
        default: *p = f->rg_ids[i].data(); *len = (int64_t)f->rg_ids[i].size(); break;
    }
    return KBBQ_OK;
}

// applybqsr's output: every alignment line as read, its QUAL field replaced by the new qualities (row r of qplane, the field's own
// length) and, with set_oq, "\tOQ:Z:<QUAL as read>" appended to a record that has no OQ tag -- GATK keeps an existing one.  Two
// passes in parallel: the size of every line, then every line at its offset.
int kbbq_sam_render(const kbbq_sam* f, int64_t first, int64_t n, const uint8_t* qplane, int pitch, int set_oq,
                    uint8_t* out, size_t cap, size_t* used)
{
    if (!f || !used || (n > 0 && !qplane)) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_render: NULL argument");
    if (first < 0 || n < 0 || first + n > (int64_t)f->line0.size() || pitch <= 0)
        return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_render: bad range / pitch");
    auto star = [&](int64_t i) { return f->qual_len[i] == 1 && f->buf[f->qual0[i]] == '*'; };
    auto adds_oq = [&](int64_t i) { return set_oq && !f->oq_len[i] && !star(i); };
    for (int64_t r = 0; r < n; ++r)
        if (!star(first + r) && f->qual_len[first + r] > (uint32_t)pitch)
            return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_render: a QUAL field is wider than the plane's pitch");
    std::vector<size_t> at((size_t)n + 1, 0);
    for (int64_t r = 0; r < n; ++r) {
        const int64_t i = first + r;
        at[(size_t)r + 1] = at[(size_t)r] + f->linelen[i] + 1 + (adds_oq(i) ? 6 + (size_t)f->qual_len[i] : 0);
    }
    *used = at[(size_t)n];
    if (!out) return KBBQ_OK;
    if (cap < at[(size_t)n]) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_render: output buffer too small");
    par_for(n, threads_for(at[(size_t)n]), [&](int64_t lo, int64_t hi) {
        for (int64_t r = lo; r < hi; ++r) {
            const int64_t i = first + r;
            const uint8_t* line = f->buf + f->line0[i];
            uint8_t* o = out + at[(size_t)r];
            memcpy(o, line, f->linelen[i]);
            if (!star(i)) memcpy(o + (f->qual0[i] - f->line0[i]), qplane + (size_t)r * pitch, f->qual_len[i]);
            o += f->linelen[i];
            if (adds_oq(i)) {
                memcpy(o, "\tOQ:Z:", 6);
                memcpy(o + 6, f->buf + f->qual0[i], f->qual_len[i]);
                o += 6 + f->qual_len[i];
            }
            *o = '\n';
        }
    });
    return KBBQ_OK;
}

}  // extern "C"

// ---- BAM output: what only the text knows (include/kbbq_hip.h "BAM output"; the device adds SEQ and QUAL: kbbq_bam_out.h) -------
namespace {

enum BamBad { BAM_FINE = 0, BAM_RNAME, BAM_RNEXT, BAM_QNAME, BAM_NCIGAR, BAM_CIGAR_OP, BAM_TAG, BAM_TAG_INT, BAM_SEQ_QUAL, BAM_QUAL_LEN,
              BAM_FLAG, BAM_MAPQ };

struct BamRefs {
    std::vector<std::pair<std::string, int64_t>> sq;     // the @SQ lines in order: SN, LN
    std::unordered_map<std::string, int> index;
    std::vector<int> of_contig;                          // the reader's contig number -> refID; -1 for '*', -2 when @SQ lacks it
};

using BamLines = std::vector<std::pair<const uint8_t*, size_t>>;       // header lines, without their line ends

BamLines bam_header_lines(const kbbq_sam* f)
{
    BamLines lines;
    for (size_t h = 0; h < f->hdr0.size(); ++h) lines.emplace_back(f->buf + f->hdr0[h], (size_t)f->hdrlen[h]);
    return lines;
}

// the references of the @SQ lines among `lines`
bool bam_refs_of(const BamLines& lines, BamRefs& R, std::string& err)
{
    for (const auto& line : lines) {
        const uint8_t* p = line.first; const uint8_t* e = p + line.second;
        if (e - p < 3 || memcmp(p, "@SQ", 3) != 0) continue;
        std::string name; int64_t len = -1; bool has_name = false;
        const uint8_t* q = (const uint8_t*)memchr(p, '\t', (size_t)(e - p));
        for (q = q ? q + 1 : e; q < e;) {
            const uint8_t* t = (const uint8_t*)memchr(q, '\t', (size_t)(e - q));
            const uint8_t* fe = t ? t : e;
            if (fe - q >= 3 && q[2] == ':') {
                if (q[0] == 'S' && q[1] == 'N') { name.assign((const char*)q + 3, (size_t)(fe - q - 3)); has_name = true; }
                else if (q[0] == 'L' && q[1] == 'N' && !parse_int(q + 3, fe, len)) len = -1;
            }
            q = fe + 1;
        }
        if (!has_name || len < 0 || len > INT32_MAX) {
            err = "an @SQ line without SN or a decimal LN: " + std::string((const char*)p, std::min<size_t>(60, (size_t)(e - p)));
            return false;
        }
        R.index[name] = (int)R.sq.size();                 // (a name given twice: its last line's index)
        R.sq.emplace_back(name, len);
    }
    return true;
}

bool bam_refs(const kbbq_sam* f, BamRefs& R, std::string& err)
{
    if (!bam_refs_of(bam_header_lines(f), R, err)) return false;
    R.of_contig.resize(f->contigs.size());
    for (size_t c = 0; c < f->contigs.size(); ++c) {
        if (f->contigs[c] == "*") { R.of_contig[c] = -1; continue; }
        auto it = R.index.find(f->contigs[c]);
        R.of_contig[c] = it == R.index.end() ? -2 : it->second;
    }
    return true;
}

struct BamLine { const uint8_t* s[11]; const uint8_t* e[11]; const uint8_t* tags; const uint8_t* end; };

void bam_split(const kbbq_sam* f, int64_t i, BamLine& F)   // (kbbq_sam_open has seen eleven fields in every line)
{
    const uint8_t* q = f->buf + f->line0[i]; F.end = q + f->linelen[i];
    for (int k = 0; k < 11; ++k) {
        const uint8_t* t = q <= F.end ? (const uint8_t*)memchr(q, '\t', (size_t)(F.end - q)) : nullptr;
        F.s[k] = std::min(q, F.end); F.e[k] = t ? t : F.end;
        q = F.e[k] + 1;
    }
    F.tags = std::min(q, F.end);
}

bool bam_float(const uint8_t* p, const uint8_t* e, float& out)      // as Python's float(), then rounded to 32 bits
{
    char buf[64];
    const size_t n = (size_t)(e - p);
    if (n == 0 || n >= sizeof buf || p[0] == ' ' || p[0] == '\t') return false;
    memcpy(buf, p, n); buf[n] = 0;
    char* stop = nullptr;
    const double v = strtod(buf, &stop);
    if (stop != buf + n) return false;
    out = (float)v;
    return true;
}

template <typename T> uint8_t* bam_put(uint8_t* o, T v) { memcpy(o, &v, sizeof v); return o + sizeof v; }

// an integer as BAM type `t` (c C s S i I) to o (NULL: nothing is written); false when the type does not hold it
bool bam_put_int(char t, int64_t v, uint8_t*& o)
{
    switch (t) {
        case 'c': if (v < -128 || v > 127) return false; if (o) o = bam_put(o, (int8_t)v); return true;
        case 'C': if (v < 0 || v > 255) return false; if (o) o = bam_put(o, (uint8_t)v); return true;
        case 's': if (v < -32768 || v > 32767) return false; if (o) o = bam_put(o, (int16_t)v); return true;
        case 'S': if (v < 0 || v > 65535) return false; if (o) o = bam_put(o, (uint16_t)v); return true;
        case 'i': if (v < INT32_MIN || v > INT32_MAX) return false; if (o) o = bam_put(o, (int32_t)v); return true;
        case 'I': if (v < 0 || v > (int64_t)UINT32_MAX) return false; if (o) o = bam_put(o, (uint32_t)v); return true;
        default: return false;
    }
}

int bam_int_bytes(char t) { return t == 'c' || t == 'C' ? 1 : t == 's' || t == 'S' ? 2 : 4; }

// one tag field [p, e) as BAM bytes at out (NULL: only counted): the bytes, or -BAM_TAG / -BAM_TAG_INT
int64_t bam_tag(const uint8_t* p, const uint8_t* e, uint8_t* out)
{
    if (e - p < 5 || p[2] != ':' || p[4] != ':') return -BAM_TAG;
    const uint8_t* v = p + 5;
    const int64_t vn = e - v;
    uint8_t* o = out;
    if (o) { o[0] = p[0]; o[1] = p[1]; o += 2; }
    switch (p[3]) {
        case 'A':
            if (vn != 1) return -BAM_TAG;
            if (o) { o[0] = 'A'; o[1] = v[0]; }
            return 4;
        case 'i': {
            int64_t x;
            if (!parse_int(v, e, x)) return -BAM_TAG;
            for (const char* t = "cCsSiI"; *t; ++t) {
                uint8_t* none = nullptr;
                if (!bam_put_int(*t, x, none)) continue;
                if (o) { *o++ = (uint8_t)*t; bam_put_int(*t, x, o); }
                return 3 + bam_int_bytes(*t);
            }
            return -BAM_TAG_INT;
        }
        case 'f': {
            float x;
            if (!bam_float(v, e, x)) return -BAM_TAG;
            if (o) { *o++ = 'f'; bam_put(o, x); }
            return 7;
        }
        case 'Z': case 'H':
            if (o) { *o++ = p[3]; memcpy(o, v, (size_t)vn); o[vn] = 0; }
            return 3 + vn + 1;
        case 'B': {
            if (vn < 1 || !strchr("cCsSiIf", v[0]) || v[0] == 0 || (vn > 1 && v[1] != ',')) return -BAM_TAG;
            const char sub = (char)v[0];
            const int width = sub == 'f' ? 4 : bam_int_bytes(sub);
            uint8_t* count_at = nullptr;
            if (o) { *o++ = 'B'; *o++ = (uint8_t)sub; count_at = o; o += 4; }
            int32_t count = 0;
            for (const uint8_t* q = v + 2; vn > 1 && q <= e;) {
                const uint8_t* t = (const uint8_t*)memchr(q, ',', (size_t)(e - q));
                const uint8_t* fe = t ? t : e;
                if (sub == 'f') {
                    float x;
                    if (!bam_float(q, fe, x)) return -BAM_TAG;
                    if (o) o = bam_put(o, x);
                } else {
                    int64_t x;
                    uint8_t* none = nullptr;
                    if (!parse_int(q, fe, x) || !(o ? bam_put_int(sub, x, o) : bam_put_int(sub, x, none))) return -BAM_TAG;
                }
                ++count;
                q = fe + 1;
            }
            if (count_at) bam_put(count_at, count);
            return 3 + 1 + 4 + (int64_t)count * width;
        }
        default: return -BAM_TAG;
    }
}

// the tags of a line (empty fields skipped) as BAM bytes at out (NULL: only counted): the bytes, or -BAM_TAG / -BAM_TAG_INT
int64_t bam_tags(const BamLine& F, uint8_t* out)
{
    int64_t total = 0;
    for (const uint8_t* q = F.tags; q < F.end;) {
        const uint8_t* t = (const uint8_t*)memchr(q, '\t', (size_t)(F.end - q));
        const uint8_t* te = t ? t : F.end;
        if (te > q) {
            const int64_t m = bam_tag(q, te, out ? out + total : nullptr);
            if (m < 0) return m;
            total += m;
        }
        q = te + 1;
    }
    return total;
}

bool bam_star(const uint8_t* s, const uint8_t* e) { return e - s == 1 && *s == '*'; }

// RNEXT -> next_refID; -2: not in @SQ
int bam_next_ref(const BamRefs& R, const BamLine& F, int ref)
{
    if (bam_star(F.s[6], F.e[6])) return -1;
    if (F.e[6] - F.s[6] == 1 && *F.s[6] == '=') return ref;
    if (F.e[6] - F.s[6] == F.e[2] - F.s[2] && !memcmp(F.s[6], F.s[2], (size_t)(F.e[2] - F.s[2]))) return ref;
    auto it = R.index.find(std::string((const char*)F.s[6], (size_t)(F.e[6] - F.s[6])));
    return it == R.index.end() ? -2 : it->second;
}

// what BAM cannot hold of alignment i (the order of include/kbbq_hip.h)
BamBad bam_record_bad(const kbbq_sam* f, const BamRefs& R, int64_t i)
{
    BamLine F;
    bam_split(f, i, F);
    const int ref = R.of_contig[(size_t)f->contig[i]];
    if (ref == -2) return BAM_RNAME;
    if (bam_next_ref(R, F, ref) == -2) return BAM_RNEXT;
    if (f->name_len[i] > 254) return BAM_QNAME;
    if (f->cig_n[i] > 65535) return BAM_NCIGAR;
    const uint32_t* ops = f->cigar.data() + f->cig_off[i];
    for (uint32_t k = 0; k < f->cig_n[i]; ++k) if ((ops[k] & 15u) > 8u) return BAM_CIGAR_OP;
    const int64_t t = bam_tags(F, nullptr);
    if (t < 0) return (BamBad)-t;
    const bool seq_star = bam_star(F.s[9], F.e[9]), qual_star = bam_star(F.s[10], F.e[10]);
    if (seq_star && !qual_star) return BAM_SEQ_QUAL;
    if (!qual_star && f->qual_len[i] != f->seq_len[i]) return BAM_QUAL_LEN;
    if (f->flag[i] < 0 || f->flag[i] > 65535) return BAM_FLAG;
    int64_t mapq;
    if (!parse_int(F.s[4], F.e[4], mapq) || mapq < 0 || mapq > 255) return BAM_MAPQ;
    return BAM_FINE;
}

const char* bam_bad_text(BamBad b)
{
    switch (b) {
        case BAM_RNAME: return "its RNAME is not in @SQ";
        case BAM_RNEXT: return "its RNEXT is not in @SQ";
        case BAM_QNAME: return "a QNAME longer than 254 bytes";
        case BAM_NCIGAR: return "more than 65535 CIGAR operations (no CG tag is written)";
        case BAM_CIGAR_OP: return "an unknown CIGAR operation";
        case BAM_TAG: return "a malformed tag";
        case BAM_TAG_INT: return "an integer tag outside int32 and uint32";
        case BAM_SEQ_QUAL: return "SEQ is '*' but QUAL is not";
        case BAM_QUAL_LEN: return "SEQ and QUAL lengths differ";
        case BAM_FLAG: return "a FLAG outside 0..65535";
        case BAM_MAPQ: return "a MAPQ outside 0..255";
        default: return "";
    }
}

int bam_reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (int)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(1 + (beg >> 26));
    return 0;
}

bool bam_range_ok(const kbbq_sam* f, int64_t first, int64_t n) { return first >= 0 && n >= 0 && first + n <= (int64_t)f->line0.size(); }

int bam_refs_or_error(const kbbq_sam* f, BamRefs& R)
{
    std::string err;
    return bam_refs(f, R, err) ? KBBQ_OK : kbbq_set_error_(KBBQ_E_RANGE, err.c_str());
}

// the stream's head of header lines: magic, the text (every line with its '\n'), the references of the @SQ lines
int bam_header_of(const char* who, const BamLines& lines, uint8_t* out, size_t cap, size_t* used)
{
    BamRefs R;
    std::string err;
    if (!bam_refs_of(lines, R, err)) return kbbq_set_error_(KBBQ_E_RANGE, err.c_str());
    size_t text = 0, need = 12;
    for (const auto& line : lines) text += line.second + 1;
    for (auto& sq : R.sq) need += 4 + sq.first.size() + 1 + 4;
    need += text;
    *used = need;
    if (!out) return KBBQ_OK;
    if (cap < need) return kbbq_set_error_(KBBQ_E_ARG, (std::string(who) + ": output buffer too small").c_str());
    if (text > (size_t)INT32_MAX) return kbbq_set_error_(KBBQ_E_RANGE, (std::string(who) + ": a header text of 2^31 bytes or more").c_str());
    uint8_t* o = out;
    memcpy(o, "BAM\1", 4); o += 4;
    o = bam_put(o, (int32_t)text);
    for (const auto& line : lines) { memcpy(o, line.first, line.second); o += line.second; *o++ = '\n'; }
    o = bam_put(o, (int32_t)R.sq.size());
    for (auto& sq : R.sq) {
        o = bam_put(o, (int32_t)(sq.first.size() + 1));
        memcpy(o, sq.first.data(), sq.first.size()); o += sq.first.size(); *o++ = 0;
        o = bam_put(o, (int32_t)sq.second);
    }
    return KBBQ_OK;
}

}  // namespace

extern "C" {

int kbbq_bam_header(const kbbq_sam* f, uint8_t* out, size_t cap, size_t* used)
{
    if (!f || !used) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_bam_header: NULL argument");
    return bam_header_of("kbbq_bam_header", bam_header_lines(f), out, cap, used);
}

int kbbq_bam_header_text(const uint8_t* text, size_t n, uint8_t* out, size_t cap, size_t* used)
{
    if (!used || (n && !text)) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_bam_header_text: NULL argument");
    BamLines lines;
    for (size_t at = 0; at < n;) {
        const uint8_t* nl = (const uint8_t*)memchr(text + at, '\n', n - at);
        const size_t end = nl ? (size_t)(nl - text) : n;
        if (end > at) lines.emplace_back(text + at, end - at);
        at = end + 1;
    }
    return bam_header_of("kbbq_bam_header_text", lines, out, cap, used);
}

int kbbq_bam_check(const kbbq_sam* f, int64_t first, int64_t n, int64_t* bad_index)
{
    if (bad_index) *bad_index = -1;
    if (!f || !bad_index) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_bam_check: NULL argument");
    if (!bam_range_ok(f, first, n)) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_bam_check: bad range");
    BamRefs R;
    if (int rc = bam_refs_or_error(f, R)) return rc;
    std::atomic<int64_t> lowest(INT64_MAX);
    par_for(n, threads_for((size_t)n * 256), [&](int64_t lo, int64_t hi) {
        for (int64_t i = first + lo; i < first + hi && i < lowest.load(std::memory_order_relaxed); ++i)
            if (bam_record_bad(f, R, i) != BAM_FINE) {
                int64_t cur = lowest.load();
                while (i < cur && !lowest.compare_exchange_weak(cur, i)) {}
                break;
            }
    });
    if (lowest.load() == INT64_MAX) return KBBQ_OK;
    const int64_t i = lowest.load();
    *bad_index = i;
    char msg[256];
    snprintf(msg, sizeof msg, "alignment %lld cannot be written as BAM: %s", (long long)i, bam_bad_text(bam_record_bad(f, R, i)));
    return kbbq_set_error_(KBBQ_E_RANGE, msg);
}

int kbbq_bam_layout(const kbbq_sam* f, int64_t first, int64_t n, int set_oq, const uint8_t* keep_qual, kbbq_bam_desc* desc,
                    size_t* skel_bytes, size_t* stream_bytes)
{
    if (!f || !skel_bytes || !stream_bytes || (n > 0 && !desc)) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_bam_layout: NULL argument");
    *skel_bytes = *stream_bytes = 0;
    if (!bam_range_ok(f, first, n)) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_bam_layout: bad range");
    std::atomic<bool> bad(false);
    par_for(n, threads_for((size_t)n * 256), [&](int64_t lo, int64_t hi) {
        for (int64_t r = lo; r < hi; ++r) {
            const int64_t i = first + r;
            BamLine F;
            bam_split(f, i, F);
            const bool seq_star = bam_star(F.s[9], F.e[9]), qual_star = bam_star(F.s[10], F.e[10]);
            int64_t tags = bam_tags(F, nullptr);
            if (tags < 0 || (!qual_star && f->qual_len[i] != f->seq_len[i]) || (seq_star && !qual_star)) { bad = true; tags = 0; }
            if (set_oq && !f->oq_len[i] && !qual_star) tags += 3 + (int64_t)f->qual_len[i] + 1;
            kbbq_bam_desc& d = desc[r];
            d.skel_off = d.stream_off = 0;
            d.head_bytes = 36u + f->name_len[i] + 1u + 4u * f->cig_n[i];
            d.tail_bytes = (uint32_t)std::min<int64_t>(tags, UINT32_MAX);
            d.l_seq = seq_star ? 0u : f->seq_len[i];
            d.qual_src = (qual_star || (keep_qual && keep_qual[r])) ? KBBQ_BAM_QUAL_SKELETON : KBBQ_BAM_QUAL_PLANE;
        }
    });
    if (bad) return kbbq_set_error_(KBBQ_E_RANGE, "kbbq_bam_layout: a record BAM cannot hold (kbbq_bam_check names it)");
    uint64_t skel = 0, stream = 0;
    for (int64_t r = 0; r < n; ++r) {
        kbbq_bam_desc& d = desc[r];
        if (stream >= ((uint64_t)1 << 31)) break;
        d.skel_off = (uint32_t)skel; d.stream_off = (uint32_t)stream;
        skel += (uint64_t)d.head_bytes + (d.qual_src == KBBQ_BAM_QUAL_SKELETON ? d.l_seq : 0u) + d.tail_bytes;
        stream += (uint64_t)d.head_bytes + ((uint64_t)d.l_seq + 1) / 2 + d.l_seq + d.tail_bytes;
    }
    if (stream >= ((uint64_t)1 << 31))
        return kbbq_set_error_(KBBQ_E_RANGE, "kbbq_bam_layout: the stream of a slab must stay below 2^31 bytes (offsets are 32 bits): fewer records per slab");
    *skel_bytes = (size_t)skel; *stream_bytes = (size_t)stream;
    return KBBQ_OK;
}

int kbbq_bam_skeleton(const kbbq_sam* f, int64_t first, int64_t n, int set_oq, const kbbq_bam_desc* desc, uint8_t* skel, size_t cap)
{
    if (!f || (n > 0 && (!desc || !skel))) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_bam_skeleton: NULL argument");
    if (!bam_range_ok(f, first, n)) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_bam_skeleton: bad range");
    BamRefs R;
    if (int rc = bam_refs_or_error(f, R)) return rc;
    std::atomic<bool> bad(false);
    par_for(n, threads_for((size_t)n * 256), [&](int64_t lo, int64_t hi) {
        for (int64_t r = lo; r < hi; ++r) {
            const int64_t i = first + r;
            const kbbq_bam_desc& d = desc[r];
            BamLine F;
            bam_split(f, i, F);
            const bool qual_star = bam_star(F.s[10], F.e[10]), adds_oq = set_oq && !f->oq_len[i] && !qual_star;
            const bool keeps = d.qual_src == KBBQ_BAM_QUAL_SKELETON;
            const int64_t tags = bam_tags(F, nullptr);
            const int ref = R.of_contig[(size_t)f->contig[i]], next = bam_next_ref(R, F, ref);
            int64_t mapq = 0;
            // the descriptor is this record's, and inside the buffer?
            if (tags < 0 || ref == -2 || next == -2 || !parse_int(F.s[4], F.e[4], mapq)
                || d.head_bytes != 36u + f->name_len[i] + 1u + 4u * f->cig_n[i]
                || d.tail_bytes != (uint64_t)tags + (adds_oq ? 3 + (uint64_t)f->qual_len[i] + 1 : 0)
                || d.l_seq != (bam_star(F.s[9], F.e[9]) ? 0u : f->seq_len[i]) || (qual_star && !keeps)
                || (keeps && !qual_star && f->qual_len[i] != d.l_seq) || f->name_len[i] > 254
                || (uint64_t)d.skel_off + d.head_bytes + (keeps ? d.l_seq : 0u) + d.tail_bytes > cap) { bad = true; continue; }
            uint8_t* o = skel + d.skel_off;
            const uint32_t L = d.l_seq;
            o = bam_put(o, (int32_t)(d.head_bytes - 4 + (L + 1) / 2 + L + d.tail_bytes));
            o = bam_put(o, (int32_t)ref);
            o = bam_put(o, (int32_t)f->pos[i]);
            *o++ = (uint8_t)(f->name_len[i] + 1);
            *o++ = (uint8_t)mapq;
            o = bam_put(o, (uint16_t)bam_reg2bin(f->pos[i], f->pos[i] + std::max<int64_t>(f->ref_span[i], 1)));
            o = bam_put(o, (uint16_t)f->cig_n[i]);
            o = bam_put(o, (uint16_t)f->flag[i]);
            o = bam_put(o, (uint32_t)L);
            o = bam_put(o, (int32_t)next);
            o = bam_put(o, (int32_t)f->pnext[i]);
            o = bam_put(o, (int32_t)f->tlen[i]);
            memcpy(o, F.s[0], f->name_len[i]); o += f->name_len[i]; *o++ = 0;
            if (f->cig_n[i]) { memcpy(o, f->cigar.data() + f->cig_off[i], 4u * f->cig_n[i]); o += 4u * f->cig_n[i]; }
            if (keeps) {
                if (qual_star) memset(o, 0xFF, L);
                else for (uint32_t k = 0; k < L; ++k) o[k] = (uint8_t)(F.s[10][k] - 33);
                o += L;
            }
            o += bam_tags(F, o);
            if (adds_oq) {
                memcpy(o, "OQZ", 3); o += 3;
                memcpy(o, F.s[10], f->qual_len[i]); o += f->qual_len[i];
                *o++ = 0;
            }
        }
    });
    if (bad) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_bam_skeleton: the descriptors are not kbbq_bam_layout's of these records, or the buffer is too small");
    return KBBQ_OK;
}

// benchmark.py:102-124: FASTQ reads are matched to alignments by name -- the FASTQ name up to its first '_'
// against QNAME + "/1" | "/2" (second-in-pair flag); of several alignments with one name the LAST wins (a dict
// in the reference).  idx[i] = alignment of FASTQ read i, or -1 (the reference's KeyError).
int kbbq_sam_match_fastq(const kbbq_sam* f, const kbbq_fastq* fq, int64_t* idx)
{
    if (!f || !fq) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_match_fastq: NULL argument");
    const int64_t n = kbbq_fastq_count(fq);
    if (n > 0 && !idx) return kbbq_set_error_(KBBQ_E_ARG, "kbbq_sam_match_fastq: NULL argument");
    std::unordered_map<std::string, int64_t> row;
    const int64_t na = (int64_t)f->line0.size();
    row.reserve((size_t)na * 2);
    for (int64_t i = 0; i < na; ++i) {
        std::string key((const char*)f->buf + f->line0[i], f->name_len[i]);
        key += (f->flag[i] & 128) ? "/2" : "/1";
        row[key] = i;
    }
    par_for(n, threads_for((size_t)n * 64), [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const char* p = nullptr; int len = 0;
            if (kbbq_fastq_name(fq, i, &p, &len) != KBBQ_OK) { idx[i] = -1; continue; }
            const void* us = memchr(p, '_', (size_t)len);
            if (us) len = (int)((const char*)us - p);
            auto it = row.find(std::string(p, (size_t)len));
            idx[i] = it == row.end() ? -1 : it->second;
        }
    });
    return KBBQ_OK;
}

}  // extern "C"
