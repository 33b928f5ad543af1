// bam_scan.h -- the head of an inflated BAM image and its chain of records: the one statement both kbbq_bam_to_sam (the host
// reader's BAM -> SAM text) and kbbq_bam_scan (include/kbbq_hip.h "BAM input") go by.  Host only, the standard library only (a
// stand-alone test program compiles it under the sanitizers: tests/native/bam_in_sanitize.cpp).
#pragma once
#include <charconv>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

struct kbbq_bam_head {
    const uint8_t* htext = nullptr; size_t hlen = 0;     // the header text without its NUL padding
    int32_t n_ref = 0;
    std::vector<std::string> refs; std::vector<int32_t> ref_len;
    size_t refs_off = 0, records_off = 0;
};

inline int32_t kbbq_bam_les32(const uint8_t* p)
{
    return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

// magic, header text, reference list; false + err for a defect
inline bool kbbq_bam_read_head(const uint8_t* bam, size_t n, kbbq_bam_head& H, std::string& err)
{
    if (n < 12 || memcmp(bam, "BAM\1", 4) != 0) { err = "not a BAM file"; return false; }
    size_t at = 4;
    const int32_t l_text = kbbq_bam_les32(bam + at); at += 4;
    if (l_text < 0 || (size_t)l_text > n - at - 4) { err = "BAM header text runs past the file"; return false; }
    H.htext = bam + at; at += (size_t)l_text;
    H.hlen = (size_t)l_text; while (H.hlen && H.htext[H.hlen - 1] == 0) --H.hlen;          // NUL padding
    H.n_ref = kbbq_bam_les32(bam + at); at += 4;
    if (H.n_ref < 0) { err = "BAM: negative reference count"; return false; }
    H.refs_off = at;
    for (int32_t i = 0; i < H.n_ref; ++i) {
        if (n - at < 4) { err = "BAM reference list runs past the file"; return false; }
        const int32_t l_name = kbbq_bam_les32(bam + at); at += 4;
        if (l_name <= 0 || (size_t)l_name + 4 > n - at) { err = "BAM reference list runs past the file"; return false; }
        H.refs.emplace_back((const char*)bam + at, (size_t)l_name - 1); at += (size_t)l_name;
        H.ref_len.push_back(kbbq_bam_les32(bam + at)); at += 4;
    }
    H.records_off = at;
    return true;
}

// the header lines in front of the records' lines, appended to `text` (a vector of bytes): the text as read, a final '\n' added;
// without an @SQ line in it, one per entry of the binary list, which is authoritative
template <class Bytes> inline void kbbq_bam_head_text(const kbbq_bam_head& H, Bytes& text)
{
    auto put = [&](const void* p, size_t k) { const uint8_t* b = (const uint8_t*)p; text.insert(text.end(), b, b + k); };
    put(H.htext, H.hlen);
    if (H.hlen && text.back() != '\n') text.push_back((uint8_t)'\n');
    bool has_sq = false;
    for (size_t i = 0; i + 3 <= H.hlen; ++i) if ((i == 0 || H.htext[i - 1] == '\n') && !memcmp(H.htext + i, "@SQ", 3)) { has_sq = true; break; }
    if (!has_sq)
        for (size_t i = 0; i < H.refs.size(); ++i) {
            put("@SQ\tSN:", 7); put(H.refs[i].data(), H.refs[i].size()); put("\tLN:", 4);
            char tmp[24];
            auto r = std::to_chars(tmp, tmp + sizeof tmp, H.ref_len[i]);
            put(tmp, (size_t)(r.ptr - tmp));
            text.push_back((uint8_t)'\n');
        }
}

// the chain of block_size words from `at`: see(offset of the record's body, block_size) for every record; false + err when a
// record is cut short
template <class See> inline bool kbbq_bam_chain(const uint8_t* bam, size_t n, size_t at, std::string& err, See see)
{
    while (at < n) {
        if (n - at < 4) { err = "BAM: truncated record"; return false; }
        const int32_t bs = kbbq_bam_les32(bam + at);
        if (bs < 32 || (size_t)bs > n - at - 4) { err = "BAM: truncated record"; return false; }
        see(at + 4, (size_t)bs);
        at += 4 + (size_t)bs;
    }
    return true;
}

// the ID of every @RG line of the header lines in text[0, n), in order, as kbbq_sam_open takes them: the line's last field that
// begins with "ID:" and holds more, the empty string without one
inline void kbbq_bam_rg_ids(const uint8_t* text, size_t n, std::vector<std::string>& ids)
{
    size_t at = 0;
    while (at < n) {
        const uint8_t* nl = (const uint8_t*)memchr(text + at, '\n', n - at);
        const uint8_t* p = text + at; const uint8_t* e = nl ? nl : text + n;
        at = (size_t)(e - text) + 1;
        if (e > p && e[-1] == '\r') --e;
        if (e - p < 3 || memcmp(p, "@RG", 3) != 0) continue;
        std::string id;
        for (const uint8_t* q = p; q < e;) {
            const uint8_t* t = (const uint8_t*)memchr(q, '\t', (size_t)(e - q));
            const uint8_t* fe = t ? t : e;
            if (fe - q > 3 && q[0] == 'I' && q[1] == 'D' && q[2] == ':') id.assign((const char*)q + 3, (size_t)(fe - q - 3));
            q = fe + 1;
        }
        ids.push_back(id);
    }
}
