// kbbq_bgzf.hip -- libkbbq_hip.so: BGZF on the GPU -- deflate (output) and inflate (input), with the inflate's staging of its own
// (C ABI: include/kbbq_hip.h; shared: kbbq_lib.h).
#include "kbbq_bgzf.h"
#include "kbbq_bgzf_inflate.h"
#include "kbbq_lib.h"
#include "bam_host.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

// ---- kernels launched with dynamic LDS ---------------------------------------------------------------------------------
// Each of them is named HERE and nowhere else (as K1 / K2 in kbbq_hip.hip): the launches take a kernel's address from this table,
// and bgzf_full_lds (for kbbq_ctx_create) walks it to allow every one of them the full LDS as dynamic shared memory.
enum BgzfLdsKernel { LK_BGZF, LK_BGZF_INFLATE, LK_BGZF_COUNT };
static const void* const BGZF_LDS_KERNELS[LK_BGZF_COUNT] = {(const void*)bz_deflate, (const void*)bi_inflate};

void bgzf_full_lds(int lds_bytes, const CtxLap& lap)
{
    for (const void* kernel : BGZF_LDS_KERNELS) (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    lap("the BGZF kernels' attributes");
}

extern "C" {

// ---- BGZF output (csrc/kbbq_bgzf.h) -------------------------------------------------------------------------------------------
static int64_t bgzf_blocks_of(int64_t n, int block_bytes) { return (n + block_bytes - 1) / block_bytes; }

static int bgzf_block_bytes_ok(const char* who, int block_bytes)
{
    if (block_bytes < 1 || block_bytes > (int)BZ_MAX_TEXT)
        return fail(KBBQ_E_ARG, "%s: block_bytes %d is not in 1..%u", who, block_bytes, BZ_MAX_TEXT);
    return KBBQ_OK;
}

// the launches of one piece of text (n > 0, arguments checked): blocks, sizes, offsets, packed bytes; the packed length is left
// in c->bgzf_off[nblocks]
static int bgzf_launch(kbbq_ctx* c, const uint8_t* d_text, int64_t n, int block_bytes, uint8_t* d_blocks, uint32_t* d_sizes,
                       uint8_t* d_packed)
{
    const int64_t nb = bgzf_blocks_of(n, block_bytes);
    const unsigned grid = (unsigned)std::min<int64_t>(nb, std::max(c->cus, 1));
    int rc = grow_scratch(c, c->bgzf_tok, (size_t)grid * BZ_MAX_TEXT * sizeof(u32));
    if (!rc) rc = grow_scratch(c, c->bgzf_off, (size_t)(nb + 1) * sizeof(u64));
    if (rc) return rc;
    BgzfParams q{d_text, n, (u32)block_bytes, (u32)nb, d_blocks, d_sizes, (u32*)c->bgzf_tok.p};
    void* args[] = {&q};
    (void)hipLaunchKernel(BGZF_LDS_KERNELS[LK_BGZF], dim3(grid), dim3(BZ_THREADS), args, BZ_LDS_BYTES, c->stream);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(bz_scan_sizes, dim3(1), dim3(BZ_THREADS), 0, c->stream, (const u32*)d_sizes, (u32)nb, (u64*)c->bgzf_off.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(bz_pack, dim3((unsigned)nb), dim3(256), 0, c->stream, (const uint8_t*)d_blocks, (const u32*)d_sizes,
                       (const u64*)c->bgzf_off.p, d_packed);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

size_t kbbq_bgzf_bound(int64_t n, int block_bytes)
{
    if (n <= 0 || block_bytes < 1 || block_bytes > (int)BZ_MAX_TEXT) return 0;
    return (size_t)n + 31 * (size_t)bgzf_blocks_of(n, block_bytes);
}

int kbbq_bgzf_eof(uint8_t* out)
{
    static const uint8_t eof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0,
                                    0, 0, 0, 0, 0, 0, 0, 0};
    if (!out) return fail(KBBQ_E_ARG, "kbbq_bgzf_eof: out is NULL");
    memcpy(out, eof, sizeof eof);
    return KBBQ_OK;
}

int kbbq_bgzf_deflate_dev(kbbq_ctx* c, const uint8_t* d_text, int64_t n, int block_bytes, uint8_t* d_blocks, uint32_t* d_sizes,
                          uint8_t* d_packed, size_t* packed_bytes)
{
    int rc = bgzf_block_bytes_ok("kbbq_bgzf_deflate_dev", block_bytes);
    if (rc) return rc;
    if (!c || !packed_bytes) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate_dev: NULL ctx or packed_bytes");
    *packed_bytes = 0;
    if (n < 0) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate_dev: n < 0");
    if (n == 0) return KBBQ_OK;
    if (!d_text || !d_blocks || !d_sizes || !d_packed) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate_dev: NULL buffer");
    if (((uintptr_t)d_blocks & 3) || ((uintptr_t)d_sizes & 3)) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate_dev: d_blocks and d_sizes are 4-byte aligned");
    if (bgzf_blocks_of(n, block_bytes) > (int64_t)INT_MAX) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate_dev: more than 2^31 - 1 blocks");
    HIPCHK(hipSetDevice(c->device));
    rc = bgzf_launch(c, d_text, n, block_bytes, d_blocks, d_sizes, d_packed);
    if (rc) return rc;
    u64 total = 0;
    HIPCHK(hipMemcpyAsync(&total, (const u64*)c->bgzf_off.p + bgzf_blocks_of(n, block_bytes), sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *packed_bytes = (size_t)total;
    return KBBQ_OK;
}

int kbbq_bgzf_deflate(kbbq_ctx* c, const uint8_t* text, int64_t n, int block_bytes, uint8_t* out, size_t out_cap, size_t* out_bytes)
{
    int rc = bgzf_block_bytes_ok("kbbq_bgzf_deflate", block_bytes);
    if (rc) return rc;
    if (!c || !out_bytes) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate: NULL ctx or out_bytes");
    *out_bytes = 0;
    if (n < 0) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate: n < 0");
    if (n == 0) return KBBQ_OK;
    if (!text || !out) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate: NULL buffer");
    if (out_cap < kbbq_bgzf_bound(n, block_bytes))
        return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate: out holds %zu bytes, kbbq_bgzf_bound is %zu", out_cap, kbbq_bgzf_bound(n, block_bytes));
    HIPCHK(hipSetDevice(c->device));
    // a slab: `per` blocks.  Host: text | packed | packed length; device: text | packed | sizes; the blocks before packing in
    // scratch of the context's.  While the kernels of slab k run, the host copies slab k + 1 in and slab k - 1 out.
    const char* e = getenv("KBBQ_STAGE_MB");
    const size_t budget = (size_t)(e && atoi(e) > 0 ? atoi(e) : 96) << 20;
    const int64_t nb = bgzf_blocks_of(n, block_bytes);
    const int64_t per = std::max<int64_t>(1, std::min<int64_t>(nb, (int64_t)(budget / (3 * (size_t)BZ_SLOT))));
    const size_t text_cap = align16((size_t)per * block_bytes), packed_cap = align16((size_t)per * (block_bytes + 31));
    const size_t bytes = text_cap + packed_cap + align16((size_t)per * 4 + 8);
    rc = stage_prepare(c, bytes);
    if (!rc) rc = grow_scratch(c, c->bgzf_blocks, (size_t)per * BZ_SLOT);
    if (rc) return rc;
    size_t written = 0;
    auto finish = [&](int buf) -> int {                    // slab in `buf`: its packed bytes to `out`
        HIPCHK(hipEventSynchronize(c->stage_up[buf]));
        const u64 total = *(const u64*)((const char*)c->stage_host[buf] + text_cap + packed_cap);
        if (written + total > out_cap) return fail(KBBQ_E_HIP, "kbbq_bgzf_deflate: more bytes than kbbq_bgzf_bound");
        HIPCHK(hipMemcpyAsync((char*)c->stage_host[buf] + text_cap, (const char*)c->stage_dev[buf] + text_cap, (size_t)total,
                              hipMemcpyDeviceToHost, c->stage_down_stream));
        HIPCHK(hipStreamSynchronize(c->stage_down_stream));
        threaded_copy(out + written, (const char*)c->stage_host[buf] + text_cap, (size_t)total);
        written += (size_t)total;
        return KBBQ_OK;
    };
    int64_t k = 0;
    for (int64_t lo = 0; lo < nb; lo += per, ++k) {
        const int buf = (int)(k & 1);
        const int64_t first = lo * block_bytes, m = std::min<int64_t>(n - first, per * block_bytes), mb = bgzf_blocks_of(m, block_bytes);
        threaded_copy(c->stage_host[buf], text + first, (size_t)m);
        uint8_t* d = (uint8_t*)c->stage_dev[buf];
        rc = hipMemcpyAsync(d, c->stage_host[buf], (size_t)m, hipMemcpyHostToDevice, c->stream) == hipSuccess
                 ? KBBQ_OK : fail(KBBQ_E_HIP, "kbbq_bgzf_deflate: upload failed");
        if (!rc) rc = bgzf_launch(c, d, m, block_bytes, (uint8_t*)c->bgzf_blocks.p, (uint32_t*)(d + text_cap + packed_cap), d + text_cap);
        if (!rc && hipMemcpyAsync((char*)c->stage_host[buf] + text_cap + packed_cap, (const u64*)c->bgzf_off.p + mb, sizeof(u64),
                                  hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            rc = fail(KBBQ_E_HIP, "kbbq_bgzf_deflate: download failed");
        if (!rc && hipEventRecord(c->stage_up[buf], c->stream) != hipSuccess) rc = fail(KBBQ_E_HIP, "kbbq_bgzf_deflate: hipEventRecord failed");
        if (!rc && k > 0) rc = finish(buf ^ 1);
        if (rc) return stage_drain(c, rc);
    }
    rc = finish((int)((k - 1) & 1));
    if (rc) return stage_drain(c, rc);
    *out_bytes = written;
    return KBBQ_OK;
}

// ---- BGZF input (csrc/kbbq_bgzf_inflate.h) ------------------------------------------------------------------------------------
static int inflate_launch(kbbq_ctx* c, hipStream_t stream, const uint8_t* d_src, size_t src_bytes, const kbbq_bgzf_block* d_blocks,
                          int64_t nblocks, uint8_t* d_out, size_t out_bytes, uint32_t* d_status)
{
    if ((size_t)c->lds_bytes < BI_LDS_BYTES) return fail(KBBQ_E_ARG, "bi_inflate needs %zu bytes of LDS, the device has %d", BI_LDS_BYTES, c->lds_bytes);
    const unsigned grid = (unsigned)std::min<int64_t>(nblocks, std::max(c->cus, 1));
    BiParams q{d_src, (uint64_t)src_bytes, d_blocks, (uint32_t)nblocks, d_out, (uint64_t)out_bytes, d_status};
    void* args[] = {&q};
    (void)hipLaunchKernel(BGZF_LDS_KERNELS[LK_BGZF_INFLATE], dim3(grid), dim3(BI_THREADS), args, BI_LDS_BYTES, stream);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

static int inflate_stage_prepare(kbbq_ctx* c, size_t bytes)
{
    if (!c->inflate_stream) {
        HIPCHK(hipStreamCreateWithFlags(&c->inflate_stream, hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) HIPCHK(hipEventCreateWithFlags(&c->inflate_done[b], hipEventDisableTiming));
    }
    if (c->inflate_bytes < bytes) {
        HIPCHK(hipStreamSynchronize(c->inflate_stream));
        for (int b = 0; b < 2; ++b) {
            if (c->inflate_host[b]) { (void)hipHostFree(c->inflate_host[b]); c->inflate_host[b] = nullptr; }
            if (c->inflate_dev[b]) { (void)hipFree(c->inflate_dev[b]); c->inflate_dev[b] = nullptr; }
        }
        c->inflate_bytes = 0;
        for (int b = 0; b < 2; ++b) {
            HIPCHK(hipHostMalloc(&c->inflate_host[b], bytes, hipHostMallocDefault));
            HIPCHK(hipMalloc(&c->inflate_dev[b], bytes));
        }
        c->inflate_bytes = bytes;
    }
    return KBBQ_OK;
}

// The members of an indexed stream (kbbq_inflate_index) into out, slab by slab of whole members; members the kernel gave a status are
// inflated again by kbbq_inflate_blocks_host.  *data_error: that failed too -- the input is damaged, the text is in the error.
static int kbbq_inflate_bgzf_indexed_(kbbq_ctx* c, const uint8_t* src, size_t n, const kbbq_bgzf_block* blocks, size_t nblocks, uint8_t* out,
                                      kbbq_inflate_stats* stats, bool* data_error)
{
    *data_error = false;
    kbbq_inflate_stats st = {0, 0, 0, 0};
    if (stats) *stats = st;
    if (!nblocks) return KBBQ_OK;
    std::lock_guard<std::mutex> guard(c->inflate_lock);
    HIPCHK(hipSetDevice(c->device));
    // a slab: up to `per` members.  Host and device alike: compressed bytes | descriptors | status words | text
    const char* e = getenv("KBBQ_STAGE_MB");
    const size_t budget = (size_t)(e && atoi(e) > 0 ? atoi(e) : 96) << 20;
    const size_t per = std::max<size_t>(1, std::min<size_t>(nblocks, budget / (2 * (size_t)BI_MAX_TEXT + 64)));
    const size_t o_blocks = align16(per * (size_t)BI_MAX_PAYLOAD), o_status = o_blocks + per * sizeof(kbbq_bgzf_block);
    const size_t o_text = align16(o_status + per * 4), bytes = o_text + per * (size_t)BI_MAX_TEXT;
    int rc = inflate_stage_prepare(c, bytes);
    if (rc) return rc;
    hipStream_t s = c->inflate_stream;
    std::vector<uint32_t> again;                           // members for the host
    struct Slab { size_t lo, hi; } slab[2] = {{0, 0}, {0, 0}};
    auto finish = [&](int buf) -> int {                    // the slab in `buf`: its text to `out`, its refused members to `again`
        HIPCHK(hipEventSynchronize(c->inflate_done[buf]));
        const size_t lo = slab[buf].lo, hi = slab[buf].hi;
        const size_t text = (size_t)(blocks[hi - 1].dst + blocks[hi - 1].isize - blocks[lo].dst);
        threaded_copy(out + blocks[lo].dst, (const char*)c->inflate_host[buf] + o_text, text);
        const uint32_t* status = (const uint32_t*)((const char*)c->inflate_host[buf] + o_status);
        for (size_t b = lo; b < hi; ++b) if (status[b - lo]) again.push_back((uint32_t)b);
        st.bytes_down += text + (hi - lo) * 4;
        return KBBQ_OK;
    };
    size_t k = 0;
    for (size_t lo = 0; lo < nblocks; ++k) {
        const int buf = (int)(k & 1);
        const size_t hi = std::min(nblocks, lo + per);
        const size_t base = (size_t)blocks[lo].src, comp = (size_t)(blocks[hi - 1].src + blocks[hi - 1].csize) - base;
        const size_t text = (size_t)(blocks[hi - 1].dst + blocks[hi - 1].isize - blocks[lo].dst);
        if (comp > per * (size_t)BI_MAX_PAYLOAD || text > per * (size_t)BI_MAX_TEXT || base + comp > n)
            { rc = fail(KBBQ_E_ARG, "kbbq_inflate_bgzf: the block table does not describe BGZF members"); break; }
        if (k >= 2) { rc = finish(buf); if (rc) break; }   // the slab that used this buffer
        char* h = (char*)c->inflate_host[buf];
        char* d = (char*)c->inflate_dev[buf];
        threaded_copy(h, src + base, comp);
        kbbq_bgzf_block* hb = (kbbq_bgzf_block*)(h + o_blocks);
        for (size_t b = lo; b < hi; ++b) {
            hb[b - lo] = blocks[b];
            hb[b - lo].src -= base; hb[b - lo].dst -= blocks[lo].dst;
        }
        slab[buf] = Slab{lo, hi};
        if (hipMemcpyAsync(d, h, comp, hipMemcpyHostToDevice, s) != hipSuccess
            || hipMemcpyAsync(d + o_blocks, h + o_blocks, (hi - lo) * sizeof(kbbq_bgzf_block), hipMemcpyHostToDevice, s) != hipSuccess)
            rc = fail(KBBQ_E_HIP, "kbbq_inflate_bgzf: upload failed");
        if (!rc) rc = inflate_launch(c, s, (const uint8_t*)d, comp, (const kbbq_bgzf_block*)(d + o_blocks), (int64_t)(hi - lo),
                                     (uint8_t*)d + o_text, text, (uint32_t*)(d + o_status));
        if (!rc && (hipMemcpyAsync(h + o_status, d + o_status, (hi - lo) * 4, hipMemcpyDeviceToHost, s) != hipSuccess
                    || (text && hipMemcpyAsync(h + o_text, d + o_text, text, hipMemcpyDeviceToHost, s) != hipSuccess)))
            rc = fail(KBBQ_E_HIP, "kbbq_inflate_bgzf: download failed");
        if (!rc && hipEventRecord(c->inflate_done[buf], s) != hipSuccess) rc = fail(KBBQ_E_HIP, "kbbq_inflate_bgzf: hipEventRecord failed");
        if (rc) break;
        st.bytes_up += comp + (hi - lo) * sizeof(kbbq_bgzf_block);
        lo = hi;
    }
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    if (k >= 2) rc = finish((int)(k & 1));
    if (!rc) rc = finish((int)((k - 1) & 1));
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    st.device_blocks = nblocks - again.size(); st.host_blocks = again.size();
    if (stats) *stats = st;
    if (!again.empty()) {
        std::string err;
        if (!kbbq_inflate_blocks_host(src, blocks, again.data(), again.size(), out, again.size() << 14, err)) { *data_error = true; return fail(KBBQ_E_ARG, "%s", err.c_str()); }
    }
    return KBBQ_OK;
}

int kbbq_inflate_bgzf_dev(kbbq_ctx* c, const uint8_t* d_src, size_t src_bytes, const kbbq_bgzf_block* d_blocks, int64_t nblocks,
                          uint8_t* d_out, size_t out_bytes, uint32_t* d_status)
{
    if (!c) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf_dev: NULL ctx");
    if (nblocks < 0 || nblocks > (int64_t)INT_MAX) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf_dev: nblocks must be in 0..2^31 - 1");
    if (nblocks == 0) return KBBQ_OK;
    if (!d_blocks || !d_status || (src_bytes && !d_src) || (out_bytes && !d_out)) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf_dev: NULL buffer");
    if (((uintptr_t)d_blocks & 7) || ((uintptr_t)d_status & 3))
        return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf_dev: d_blocks is 8-byte and d_status 4-byte aligned");
    HIPCHK(hipSetDevice(c->device));
    int rc = inflate_launch(c, c->stream, d_src, src_bytes, d_blocks, nblocks, d_out, out_bytes, d_status);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return KBBQ_OK;
}

int kbbq_inflate_bgzf(kbbq_ctx* c, const uint8_t* src, size_t n, uint8_t* out, size_t out_cap, size_t* text_bytes,
                      kbbq_inflate_stats* stats)
{
    if (!c || !text_bytes) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf: NULL ctx or text_bytes");
    *text_bytes = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n == 0) return KBBQ_OK;
    if (!src) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf: NULL buffer");
    size_t nb = 0, total = 0;
    int rc = kbbq_inflate_index(src, n, nullptr, 0, &nb, &total);
    if (rc == KBBQ_INFLATE_NOT_BGZF) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf: the input is not BGZF");
    if (rc) return rc;
    if (total > out_cap || (total && !out)) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf: out holds %zu bytes, the text is %zu", out_cap, total);
    std::vector<kbbq_bgzf_block> blocks(nb);
    rc = kbbq_inflate_index(src, n, blocks.data(), nb, &nb, &total);
    if (rc) return rc;
    bool data_error = false;
    rc = kbbq_inflate_bgzf_indexed_(c, src, n, blocks.data(), nb, out, stats, &data_error);
    if (!rc) *text_bytes = total;
    return rc;
}

int kbbq_inflate_use_ctx(kbbq_ctx* c)
{
    kbbq_inflate_set_route_(c, c ? &kbbq_inflate_bgzf_indexed_ : nullptr);
    return KBBQ_OK;
}

int kbbq_inflate_bgzf_host(const uint8_t* payload, uint32_t n, uint8_t* out, uint32_t isize, uint32_t crc)
{
    if ((n && !payload) || (isize && !out)) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf_host: NULL buffer");
    std::unique_ptr<BiTables> t(new BiTables);
    static uint8_t none[4];
    return (int)bi_member_host(payload ? payload : none, n, out ? out : none, isize, crc, t.get());
}

} // extern "C"
