// fuzz_bgzf_inflate.cpp -- the host twin of the BGZF inflate kernel (csrc/kbbq_bgzf_inflate.h bi_member_host) under the sanitizers.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I kbbq-py_amd/csrc \
//       tests/tools/fuzz_bgzf_inflate.cpp -lz -o fuzz_bgzf_inflate && ./fuzz_bgzf_inflate [seconds] [seed]
//
// A CPU program with its own main: no GPU, no Python.  It runs the valid and the damaged members of tests/test_bgzf_inflate_host.py
// (built here with zlib and by hand), then random bit flips, byte changes and truncations of valid members for `seconds`.  Every
// member is decoded into a buffer of exactly ISIZE bytes between two guard zones that the sanitizer watches and the program compares;
// a status of 0 must mean the bytes zlib gives.  Exit status 0 and "clean" when nothing differed.
#include "kbbq_bgzf_inflate.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include <zlib.h>

typedef std::vector<uint8_t> bytes;

struct Member { std::string name; bytes payload; uint32_t isize, crc; };

static bytes deflate_raw(const bytes& text, int level, int strategy, size_t flush_at = 0)
{
    z_stream z; memset(&z, 0, sizeof z);
    if (deflateInit2(&z, level, Z_DEFLATED, -15, 8, strategy) != Z_OK) abort();
    bytes out(deflateBound(&z, text.size()) + 64);
    z.next_out = out.data(); z.avail_out = (uInt)out.size();
    static uint8_t none = 0;
    z.next_in = text.empty() ? &none : const_cast<Bytef*>(text.data());
    if (flush_at) {
        z.avail_in = (uInt)flush_at;
        if (deflate(&z, Z_FULL_FLUSH) != Z_OK) abort();
    }
    z.avail_in = (uInt)(text.size() - flush_at);
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) abort();
    out.resize(out.size() - z.avail_out);
    deflateEnd(&z);
    return out;
}

// zlib's verdict on a raw deflate payload that should give isize bytes: true and the text, or false
static bool inflate_raw(const bytes& payload, uint32_t isize, bytes& text)
{
    z_stream z; memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) abort();
    text.assign((size_t)isize + 1, 0);
    static uint8_t none = 0;
    z.next_in = payload.empty() ? &none : const_cast<Bytef*>(payload.data()); z.avail_in = (uInt)payload.size();
    z.next_out = text.data(); z.avail_out = (uInt)text.size();
    const int rc = inflate(&z, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && z.total_out == isize;
    inflateEnd(&z);
    text.resize(isize);
    return ok;
}

static Member member(const std::string& name, const bytes& text, const bytes& payload)
{
    return Member{name, payload, (uint32_t)text.size(), (uint32_t)crc32(crc32(0L, Z_NULL, 0), text.data(), (uInt)text.size())};
}

struct BitWriter {
    bytes out; uint32_t nbits = 0;
    void put(uint32_t v, uint32_t n) { for (uint32_t i = 0; i < n; ++i, ++nbits) { if (!(nbits & 7)) out.push_back(0); out.back() |= ((v >> i) & 1) << (nbits & 7); } }
    void code(uint32_t c, uint32_t n) { for (uint32_t i = n; i-- > 0;) put((c >> i) & 1, 1); }      // a Huffman code: first bit first
    void fixed_ll(uint32_t s) { if (s < 144) code(0x30 + s, 8); else if (s < 256) code(0x190 + s - 144, 9); else if (s < 280) code(s - 256, 7); else code(0xc0 + s - 280, 8); }
};

static int failures = 0;
static BiTables tables;

// the twin on one member between guard zones; returns its status
static uint32_t run(const Member& m, bool must_be_ok, bool must_fail)
{
    const size_t G = 64;
    bytes buf(G + m.isize + G, 0xA5);
    bytes in = m.payload;                                                      // exactly sized: the sanitizer sees a read past it
    const uint32_t st = bi_member_host(in.data(), (uint32_t)in.size(), buf.data() + G, m.isize, m.crc, &tables);
    for (size_t i = 0; i < G; ++i)
        if (buf[i] != 0xA5 || buf[G + m.isize + i] != 0xA5) { printf("FAIL %s: a byte outside the output range was written\n", m.name.c_str()); ++failures; break; }
    bytes want;
    const bool zok = inflate_raw(m.payload, m.isize, want)
                     && (uint32_t)crc32(crc32(0L, Z_NULL, 0), want.data(), (uInt)want.size()) == m.crc;
    if (st == 0 && (!zok || memcmp(want.data(), buf.data() + G, m.isize) != 0)) { printf("FAIL %s: status 0 but not zlib's bytes\n", m.name.c_str()); ++failures; }
    if (must_be_ok && st != 0) { printf("FAIL %s: status %u on a valid member\n", m.name.c_str(), st); ++failures; }
    if (must_fail && st == 0) { printf("FAIL %s: status 0 on a damaged member\n", m.name.c_str()); ++failures; }
    return st;
}

int main(int argc, char** argv)
{
    const double seconds = argc > 1 ? atof(argv[1]) : 3.0;
    std::mt19937 rng(argc > 2 ? (unsigned)atoi(argv[2]) : 12345u);
    auto fastq = [&](size_t n) { bytes t(n); const char* a = "ACGT"; for (size_t i = 0; i < n; ++i) t[i] = (i % 151 == 150) ? '\n' : (uint8_t)a[rng() & 3]; return t; };
    auto noise = [&](size_t n) { bytes t(n); for (auto& c : t) c = (uint8_t)rng(); return t; };

    std::vector<Member> valid;
    const bytes text = fastq(40000);
    for (int level : {0, 1, 6, 9}) valid.push_back(member("level " + std::to_string(level), text, deflate_raw(text, level, Z_DEFAULT_STRATEGY)));
    valid.push_back(member("Z_FIXED", text, deflate_raw(text, 6, Z_FIXED)));
    valid.push_back(member("full flush", text, deflate_raw(text, 6, Z_DEFAULT_STRATEGY, 20000)));
    for (size_t n : {(size_t)0, (size_t)1, (size_t)65280, (size_t)65536}) { const bytes t = fastq(n); valid.push_back(member("length " + std::to_string(n), t, deflate_raw(t, 6, Z_DEFAULT_STRATEGY))); }
    { const bytes t(65536, 'A'); valid.push_back(member("equal bytes", t, deflate_raw(t, 9, Z_DEFAULT_STRATEGY))); }
    {   // zlib never looks back farther than 32768 - 262: the longest distance by hand, in the fixed code
        bytes t = noise(32768);
        BitWriter w; w.put(1, 1); w.put(1, 2);
        for (uint8_t c : t) w.fixed_ll(c);
        w.fixed_ll(285); w.code(29, 5); w.put(32768 - 24577, 13); w.fixed_ll(256);
        t.insert(t.end(), t.begin(), t.begin() + 258);
        valid.push_back(member("distance 32768", t, w.out));
    }
    {   // literal codes of up to 15 bits: byte k 2^k times, no matches
        bytes t;
        for (int k = 0; k < 15; ++k) t.insert(t.end(), (size_t)1 << k, (uint8_t)('A' + k));
        std::shuffle(t.begin(), t.end(), rng);
        valid.push_back(member("literal codes of 15 bits", t, deflate_raw(t, 6, Z_HUFFMAN_ONLY)));
    }
    { const bytes t = noise(50000); valid.push_back(member("random", t, deflate_raw(t, 6, Z_DEFAULT_STRATEGY))); }
    { const bytes t = fastq(3000); valid.push_back(member("huffman only", t, deflate_raw(t, 6, Z_HUFFMAN_ONLY))); }
    for (const Member& m : valid) run(m, true, false);

    std::vector<Member> bad;
    const Member& v = valid[2];                                                // level 6: a dynamic block
    auto cut = [&](const char* name, size_t n) { Member m = v; m.name = name; m.payload.resize(n); bad.push_back(m); };
    cut("truncated in the block header", 0); cut("truncated in the code lengths", 10); cut("truncated in the body", v.payload.size() / 2);
    cut("truncated at the end", v.payload.size() - 1);
    { Member m = v; m.name = "flipped payload bit"; m.payload[m.payload.size() / 2] ^= 0x10; bad.push_back(m); }
    { Member m = v; m.name = "flipped CRC bit"; m.crc ^= 0x100; bad.push_back(m); }
    { Member m = v; m.name = "flipped ISIZE bit"; m.isize ^= 0x4; bad.push_back(m); }
    { Member m = v; m.name = "ISIZE too small"; m.isize -= 100; bad.push_back(m); }
    auto hand = [&](const char* name, const BitWriter& w) { Member m; m.name = name; m.payload = w.out; m.isize = 4; m.crc = 0; bad.push_back(m); };
    { BitWriter w; w.put(1, 1); w.put(1, 2); w.fixed_ll('a'); w.fixed_ll(257); w.code(1, 5); w.fixed_ll(256); hand("distance before the start", w); }
    for (uint32_t s : {286u, 287u}) { BitWriter w; w.put(1, 1); w.put(1, 2); w.fixed_ll('a'); w.fixed_ll(s); w.code(0, 5); w.fixed_ll(256); hand("literal/length symbol 286/287", w); }
    for (uint32_t s : {30u, 31u}) { BitWriter w; w.put(1, 1); w.put(1, 2); w.fixed_ll('a'); w.fixed_ll(257); w.code(s, 5); w.fixed_ll(256); hand("distance symbol 30/31", w); }
    { BitWriter w; w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(15, 4); for (int i = 0; i < 19; ++i) w.put(1, 3); w.put(0, 32); hand("over-subscribed code", w); }
    { BitWriter w; w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(15, 4); w.put(1, 3); for (int i = 1; i < 19; ++i) w.put(0, 3); w.put(0, 32); hand("incomplete code", w); }
    { BitWriter w; w.put(1, 1); w.put(3, 2); w.put(0, 29); hand("block type 3", w); }
    { BitWriter w; w.put(1, 1); w.put(0, 2); w.put(0, 5); w.put(4, 16); w.put(0xfffa, 16); w.put(0x64636261, 32); hand("stored LEN / NLEN", w); }
    for (const Member& m : bad) run(m, false, true);

    // random damage: a status of 0 must still mean zlib's bytes, and nothing may be touched outside the output range
    uint64_t rounds = 0, accepted = 0;
    const auto t0 = std::chrono::steady_clock::now();
    while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < seconds) {
        Member m = valid[rng() % valid.size()];
        m.name = "random damage of " + m.name + " (round " + std::to_string(rounds) + ")";
        const unsigned kind = rng() % 4;
        if (m.payload.empty()) continue;
        if (kind == 0) for (unsigned k = 1 + rng() % 3; k; --k) m.payload[rng() % m.payload.size()] ^= (uint8_t)(1u << (rng() & 7));
        else if (kind == 1) m.payload.resize(rng() % m.payload.size());
        else if (kind == 2) m.payload[rng() % std::min<size_t>(m.payload.size(), 80)] = (uint8_t)rng();   // the headers of the first block
        else m.isize = (uint32_t)(rng() % 65537);
        accepted += run(m, false, false) == 0;
        ++rounds;
    }
    printf("%zu valid members, %zu damaged members, %llu rounds of random damage (%llu still valid): %s\n", valid.size(), bad.size(),
           (unsigned long long)rounds, (unsigned long long)accepted, failures ? "FAILED" : "clean");
    return failures ? 1 : 0;
}
