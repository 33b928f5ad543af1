// bam_in_sanitize.cpp -- the scan of a BAM image (csrc/bam_scan.h) and the host twin of the decode kernel (csrc/kbbq_bam_in.h
// bd_record) under AddressSanitizer / UndefinedBehaviorSanitizer: tests/test_bam_in_host.py compiles this file alone (both headers
// are self-contained) and runs it on the CPU over well-formed and damaged images.
//   bam_in_sanitize PITCH SLAB_BYTES IMAGE...      one line per image:  <file> scan: <error>   or   <file> n=<records> status=<OR> sum=<bytes of all planes, words and CIGAR words, summed>
// Every buffer is a heap block of exactly the size the interface names -- the image, each slab (a copy of its bytes), the planes of
// a slab's rows, its words, its CIGAR range -- so a read or a write one byte outside any of them is reported.
#include "../../kbbq-py_amd/csrc/bam_scan.h"
#include "../../kbbq-py_amd/csrc/kbbq_bam_in.h"

#include <cstdio>
#include <cstdlib>

static uint8_t* block(size_t n, int fill)              // 16-byte aligned, exactly n bytes (n a multiple of 16, or rounded up by the caller)
{
    uint8_t* p = (uint8_t*)aligned_alloc(16, n ? n : 16);
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    memset(p, fill, n ? n : 16);
    return p;
}

int main(int argc, char** argv)
{
    if (argc < 4) { fprintf(stderr, "usage: bam_in_sanitize PITCH SLAB_BYTES IMAGE...\n"); return 2; }
    const uint32_t pitch = (uint32_t)atoi(argv[1]);
    const size_t slab_bytes = (size_t)atoll(argv[2]);
    if (pitch == 0 || pitch % 16) { fprintf(stderr, "PITCH must be a positive multiple of 16\n"); return 2; }
    for (int a = 3; a < argc; ++a) {
        FILE* fh = fopen(argv[a], "rb");
        if (!fh) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        fseek(fh, 0, SEEK_END);
        const size_t n = (size_t)ftell(fh);
        fseek(fh, 0, SEEK_SET);
        uint8_t* img = (uint8_t*)malloc(n ? n : 1);
        if (n && fread(img, 1, n, fh) != n) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        fclose(fh);
        kbbq_bam_head H;
        std::string err;
        std::vector<uint64_t> rec, end, cig(1, 0);
        if (!kbbq_bam_read_head(img, n, H, err)
            || !kbbq_bam_chain(img, n, H.records_off, err, [&](size_t body, size_t bs) {
                   rec.push_back(body); end.push_back(body + bs);
                   cig.push_back(cig.back() + ((uint64_t)img[body + 12] | (uint64_t)img[body + 13] << 8));
               })) {
            printf("%s scan: %s\n", argv[a], err.c_str());
            free(img);
            continue;
        }
        std::vector<uint8_t> text;
        kbbq_bam_head_text(H, text);
        std::vector<std::string> ids;
        kbbq_bam_rg_ids(text.data(), text.size(), ids);
        std::vector<uint32_t> rg_off(1, 0);
        std::vector<uint8_t> rg_ids;
        for (const auto& id : ids) { rg_ids.insert(rg_ids.end(), id.begin(), id.end()); rg_off.push_back((uint32_t)rg_ids.size()); }
        uint32_t status = 0;
        uint64_t sum = 0;
        for (size_t lo = 0; lo < rec.size();) {
            size_t hi = lo + 1;                                    // whole records: at least one, then as many as fit
            const uint64_t first = rec[lo] - 4;
            while (hi < rec.size() && end[hi] - first <= slab_bytes) ++hi;
            const size_t bytes = (size_t)(end[hi - 1] - first), m = hi - lo, ncig = (size_t)(cig[hi] - cig[lo]);
            uint8_t* slab = (uint8_t*)malloc(bytes);
            memcpy(slab, img + first, bytes);
            std::vector<uint32_t> off(m), coff(m + 1);
            for (size_t r = 0; r < m; ++r) off[r] = (uint32_t)(rec[lo + r] - first);
            for (size_t r = 0; r <= m; ++r) coff[r] = (uint32_t)(cig[lo + r] - cig[lo]);
            uint8_t* planes[3];
            for (auto& p : planes) p = block(m * pitch, 0xA5);     // nothing is zeroed first
            kbbq_bam_words* words = (kbbq_bam_words*)block(m * sizeof(kbbq_bam_words), 0xA5);
            uint32_t* ops = (uint32_t*)block((ncig * 4 + 15) / 16 * 16, 0xA5);
            const BdJob J{slab, bytes, off.data(), (uint32_t)m, pitch, rg_off.data(), rg_ids.data(), (int32_t)ids.size(), H.n_ref,
                          coff.data(), ncig, planes[0], planes[1], planes[2], words, ops};
            for (size_t r = 0; r < m; ++r) status |= bd_record(J, (uint32_t)r);
            for (auto& p : planes) { for (size_t k = 0; k < m * pitch; ++k) sum += p[k]; free(p); }
            for (size_t k = 0; k < m * sizeof(kbbq_bam_words); ++k) sum += ((const uint8_t*)words)[k];
            for (size_t k = 0; k < ncig * 4; ++k) sum += ((const uint8_t*)ops)[k];
            free(words); free(ops); free(slab);
            lo = hi;
        }
        printf("%s n=%zu status=%u sum=%llu\n", argv[a], rec.size(), status, (unsigned long long)sum);
        free(img);
    }
    return 0;
}
