// bam_recode_sanitize.cpp -- the host twin of the recode kernels (csrc/kbbq_bam_recode.h br_size / br_write) under AddressSanitizer /
// UndefinedBehaviorSanitizer: tests/test_bam_recode_host.py compiles this file alone (the headers are self-contained) and runs it on
// the CPU over well-formed and damaged images.
//   bam_recode_sanitize SET_OQ IMAGE...      one line per image:  <file> scan: <error>   or
//                                            <file> n=<records> status=<OR> skel=<bytes> stream=<bytes> sum=<descriptor, status and skeleton bytes, summed>
// Every buffer is a heap block of exactly the size the interface names -- the image, the offsets, the keep bytes (every other
// record keeps its QUAL), the descriptors, the status words, and a skeleton of exactly the bytes the size step measured -- so a
// read or a write one byte outside any of them is reported.
#include "../../kbbq-py_amd/csrc/bam_scan.h"
#include "../../kbbq-py_amd/csrc/kbbq_bam_recode.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: bam_recode_sanitize SET_OQ IMAGE...\n"); return 2; }
    const uint32_t set_oq = atoi(argv[1]) ? 1u : 0u;
    for (int a = 2; a < argc; ++a) {
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
        std::vector<uint64_t> rec;
        if (!kbbq_bam_read_head(img, n, H, err) || !kbbq_bam_chain(img, n, H.records_off, err, [&](size_t body, size_t) { rec.push_back(body); })) {
            printf("%s scan: %s\n", argv[a], err.c_str());
            free(img);
            continue;
        }
        const size_t m = rec.size();
        uint64_t* off = (uint64_t*)malloc(m ? m * 8 : 8);
        uint8_t* keep = (uint8_t*)malloc(m ? m : 1);
        kbbq_bam_desc* desc = (kbbq_bam_desc*)malloc(m ? m * sizeof(kbbq_bam_desc) : 1);
        uint32_t* status = (uint32_t*)malloc(m ? m * 4 : 4);
        for (size_t r = 0; r < m; ++r) { off[r] = rec[r]; keep[r] = (uint8_t)(r & 1); }
        memset(desc, 0xA5, m * sizeof(kbbq_bam_desc));
        memset(status, 0xA5, m * 4);
        BrJob J{img, n, off, (uint32_t)m, H.n_ref, set_oq, keep, desc, status, nullptr, 0};
        const BdJob D = br_decode_job(J);
        uint32_t any = 0;
        for (size_t r = 0; r < m; ++r) any |= br_size(J, D, (uint32_t)r);
        uint64_t skel = 0, stream = 0;
        for (size_t r = 0; r < m; ++r) {
            desc[r].skel_off = (uint32_t)skel; desc[r].stream_off = (uint32_t)stream;
            skel += br_skel_size(desc[r]); stream += br_stream_size(desc[r]);
        }
        uint8_t* out = (uint8_t*)malloc(skel ? skel : 1);
        memset(out, 0xA5, skel ? skel : 1);
        J.skel = out; J.skel_bytes = skel;
        for (size_t r = 0; r < m; ++r) if (!status[r]) br_write(J, (uint32_t)r, desc[r], 0, 1);
        uint64_t sum = 0;
        for (size_t k = 0; k < m * sizeof(kbbq_bam_desc); ++k) sum += ((const uint8_t*)desc)[k];
        for (size_t k = 0; k < m * 4; ++k) sum += ((const uint8_t*)status)[k];
        for (size_t k = 0; k < skel; ++k) sum += out[k];
        printf("%s n=%zu status=%u skel=%llu stream=%llu sum=%llu\n", argv[a], m, any, (unsigned long long)skel, (unsigned long long)stream,
               (unsigned long long)sum);
        free(out); free(status); free(desc); free(keep); free(off); free(img);
    }
    return 0;
}
