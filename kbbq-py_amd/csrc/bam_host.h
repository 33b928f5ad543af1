// bam_host.h -- gzip / BGZF inflation and BAM -> SAM text, for the SAM reader (internal to libkbbq_hip's host C++).
//
// The reference reads its alignments through pysam / htslib (benchmark.py:57-74, gatk/bqsr.py:52-123), i.e. from
// BAM files.  htslib is not part of this build; zlib is.  A BAM file is a series of BGZF blocks (independent gzip
// members carrying their compressed size in a 'BC' extra field: inflated in parallel here) holding a binary header
// and binary alignment records (SAM specification, section 4); the records are rendered as SAM text lines -- what
// `samtools view -h` prints -- and parsed by the SAM reader like any other text.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "raw_vector.h"

#include "../../include/kbbq_hip.h"
#include "kbbq_lib_host.h"

// Inflate a whole gzip / BGZF file image (any number of members).  false + err on corrupt input.
// BGZF of KBBQ_GPU_INFLATE_MIN_BYTES or more goes through the device (kbbq_inflate_bgzf_indexed_) when a context has been registered
// (kbbq_inflate_use_ctx) and KBBQ_GPU_INFLATE is 1; everything else, and that route when it fails for another reason than the data,
// is inflated on the host.
bool kbbq_inflate_all(const uint8_t* src, size_t n, kbbq_bytes& out, std::string& err);

// BGZF members on the host: libdeflate, then zlib, which decides what a damaged member is.  which[0, count): indices into blocks,
// or NULL for blocks[0, count).  Member b's text goes to out + blocks[b].dst.  work: the compressed bytes, which size the threads.
bool kbbq_inflate_blocks_host(const uint8_t* src, const kbbq_bgzf_block* blocks, const uint32_t* which, size_t count, uint8_t* out,
                              size_t work, std::string& err);

// The device route of an indexed stream (kbbq_bgzf.hip kbbq_inflate_bgzf_indexed_), handed over with its context by
// kbbq_inflate_use_ctx: this file calls nothing of the GPU half by name and links without it.  kbbq_ctx_destroy takes the context back.
typedef int (*kbbq_inflate_route)(kbbq_ctx* c, const uint8_t* src, size_t n, const kbbq_bgzf_block* blocks, size_t nblocks, uint8_t* out,
                                  kbbq_inflate_stats* stats, bool* data_error);
void kbbq_inflate_set_route_(kbbq_ctx* c, kbbq_inflate_route route);
void kbbq_inflate_forget_ctx_(kbbq_ctx* c);

// Uncompressed BAM image -> SAM text (header lines, then one line per record).  false + err on malformed input.
bool kbbq_bam_to_sam(const uint8_t* bam, size_t n, kbbq_bytes& text, std::string& err);
