// kbbq_staging.hip -- libkbbq_hip.so: the host-buffer entry points' way to the device -- slabs of rows through page-locked staging
// (shared: kbbq_lib.h; no entry point of the C ABI is defined here: kbbq_accumulate, kbbq_apply, kbbq_apply_aligned*, the kbbq_kmer_*
// forms on host buffers and kbbq_bgzf_deflate run through it).
#include "kbbq_lib.h"
#include "host_threads.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

// ---- host-buffer entry points: slabs of rows through page-locked staging -------------------------------------------------
// A caller's NumPy arrays are pageable memory: hipMemcpy from them goes through the runtime's own small staging buffers, one
// plane after the other, and the kernel starts when the last byte has arrived.  Here the rows travel in slabs: host threads
// copy slab k + 1 into a page-locked buffer while the copy engine uploads slab k and the kernel runs on slab k - 1 (apply: the
// new qualities of slab k - 2 come back meanwhile, PCIe being full duplex); device memory is two slabs, whatever the input's size.
static size_t stage_slab_rows(int pitch, int planes, int64_t nreads)
{
    const char* e = getenv("KBBQ_STAGE_MB");                       // staging bytes per slab (all planes), default 96 MB
    const size_t budget = (size_t)(e && atoi(e) > 0 ? atoi(e) : 96) << 20;
    size_t rows = budget / ((size_t)pitch * planes + 4);
    rows = std::max<size_t>(rows & ~(size_t)63, 64);
    return (size_t)std::min<int64_t>((int64_t)rows, std::max<int64_t>(nreads, 1));
}

int stage_prepare(kbbq_ctx* c, size_t bytes)
{
    if (!c->stage_stream) {
        HIPCHK(hipStreamCreateWithFlags(&c->stage_stream, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&c->stage_down_stream, hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) {
            HIPCHK(hipEventCreateWithFlags(&c->stage_up[b], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&c->stage_used[b], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&c->stage_down[b], hipEventDisableTiming));
        }
    }
    if (c->stage_bytes < bytes) {
        HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipStreamSynchronize(c->stage_stream)); HIPCHK(hipStreamSynchronize(c->stage_down_stream));
        for (int b = 0; b < 2; ++b) {
            if (c->stage_host[b]) { (void)hipHostFree(c->stage_host[b]); c->stage_host[b] = nullptr; }
            if (c->stage_dev[b]) { (void)hipFree(c->stage_dev[b]); c->stage_dev[b] = nullptr; }
        }
        c->stage_bytes = 0;
        for (int b = 0; b < 2; ++b) {
            HIPCHK(hipHostMalloc(&c->stage_host[b], bytes, hipHostMallocDefault));
            HIPCHK(hipMalloc(&c->stage_dev[b], bytes));
        }
        c->stage_bytes = bytes;
    }
    return KBBQ_OK;
}

// copy `bytes` with all host threads (a slab is tens of MB: one thread moves ~10 GB/s, PCIe takes ~55)
void threaded_copy(void* dst, const void* src, size_t bytes)
{
    const unsigned nt = kbbq_threads_for(bytes / 4);
    if (nt <= 1 || bytes < ((size_t)4 << 20)) { memcpy(dst, src, bytes); return; }
    const size_t per = ((bytes + nt - 1) / nt + 4095) & ~(size_t)4095;
    kbbq_parallel(nt, [&](unsigned t) {
        const size_t lo = std::min(bytes, (size_t)t * per), hi = std::min(bytes, lo + per);
        if (lo < hi) memcpy((char*)dst + lo, (const char*)src + lo, hi - lo);
    });
}

// Every exit of a pipelined run that leaves before its last slab -- a launch or a copy failed -- waits for what is still in
// flight: the staging buffers and their events belong to the context, and the next call's first two slabs do not wait on
// events of an earlier call.
int stage_drain(kbbq_ctx* c, int rc)
{
    if (c->stage_stream) (void)hipStreamSynchronize(c->stage_stream);
    if (c->stage_down_stream) (void)hipStreamSynchronize(c->stage_down_stream);
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

// The status words hold the SMALLEST flagged read index of every kind over all launches since they were last read; slabs number
// their reads from 0, so after a pipelined run that flagged something the slabs are looked at again one by one (input errors
// are the rare case): the first slab that reproduces a status decides, its read index made file-wide (and handed back in
// *bad_read when the caller asks for it).
static int first_offender(kbbq_ctx* c, int64_t nreads, size_t slab, const std::function<int(int64_t, int64_t)>& run_slab,
                          int64_t* bad_read)
{
    for (int64_t lo = 0; lo < nreads; lo += (int64_t)slab) {
        const int64_t m = std::min<int64_t>((int64_t)slab, nreads - lo);
        int rc = run_slab(lo, m);
        if (rc) return rc;
        int64_t idx = -1;
        rc = kbbq_ctx_status(c, &idx);
        if (rc) {
            if (idx >= 0) {
                if (bad_read) *bad_read = lo + idx;
                const std::string what = kbbq_last_error();
                const size_t colon = what.find(": ");
                return fail(rc, "read %lld%s", (long long)(lo + idx), colon == std::string::npos ? "" : what.c_str() + colon);
            }
            return rc;
        }
    }
    return KBBQ_OK;
}

// The pipelined run of a host-buffer entry point.  A slab holds the input planes `in`, the output plane (when `out` is given),
// then the meta words; `launch(d, plane, m)` runs the kernel on the m rows of device slab d, whose planes are `plane` bytes apart.
// Order of a slab k in buffers b = k & 1: [host] wait for slab k - 2 (with an output plane: for its download, whose rows then
// go to the caller -- everything of slab k - 2 on these buffers has finished, kernel included; without one: for its upload,
// and the upload stream waits for its kernel) -> host copy in -> upload (upload stream) -> kernel (launch stream, behind the
// upload's event) -> download (DOWNLOAD stream, behind the kernel's event).  Uploads and downloads are on different streams,
// so slab k + 1 goes up while slab k's kernel runs and slab k's (or k - 1's) output comes back: both directions of PCIe busy
// at once (with both on one in-order stream the order was strictly U k, K k, D k, U k + 1).
// `exact` (optional): the launch's kernel may answer KBBQ_E_LUT -- rows its fast form does not serve, no read named.  The entry
// point must not hand that to its caller: exact() switches `launch` to the form that decides (false: it already is that form)
// and the WHOLE input runs again -- such rows are the rare case -- so that clean rows with odd padding get their output and bad
// ones the reference's error with the read's index, here and slab by slab in first_offender.
// `see_meta` (optional): called with every slab's sidecar words (words, first read, count) as the slab is staged.
int stage_run(kbbq_ctx* c, const char* who, std::initializer_list<const uint8_t*> in, const uint32_t* meta, uint8_t* out,
              int64_t n, int pitch, const std::function<int(uint8_t*, size_t, int64_t)>& launch, int64_t* bad_read,
              const std::function<bool()>& exact, const std::function<void(const uint32_t*, int64_t, int64_t)>& see_meta)
{
    const int planes = (int)in.size() + (out ? 1 : 0);
    const size_t slab = stage_slab_rows(pitch, planes, n);
    const size_t plane = slab * (size_t)pitch, o_out = in.size() * plane, o_meta = (size_t)planes * plane;
    int rc = stage_prepare(c, o_meta + slab * 4);
    if (rc) return rc;
    auto stage_in = [&](int b, int64_t lo, int64_t m) {
        uint8_t* h = (uint8_t*)c->stage_host[b];
        const size_t off = (size_t)lo * pitch, nb = (size_t)m * pitch;
        size_t at = 0;
        for (const uint8_t* p : in) { threaded_copy(h + at, p + off, nb); at += plane; }
        memcpy(h + o_meta, meta + lo, (size_t)m * 4);
        if (see_meta) see_meta(reinterpret_cast<const uint32_t*>(h + o_meta), lo, m);   // the slab's words, just copied: while earlier slabs upload and run
    };
    auto upload = [&](int b, int64_t m, hipStream_t st) -> int {        // the input planes, then the meta words
        HIPCHK(hipMemcpyAsync(c->stage_dev[b], c->stage_host[b], o_out, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync((uint8_t*)c->stage_dev[b] + o_meta, (uint8_t*)c->stage_host[b] + o_meta, (size_t)m * 4, hipMemcpyHostToDevice, st));
        return KBBQ_OK;
    };
    struct Out { int64_t lo, m; };
    Out pending[2] = {{0, 0}, {0, 0}};                                   // downloads in flight, by buffer
    auto stage_out = [&](int b) -> int {                                 // wait for buffer b's download and hand its rows to the caller
        if (!pending[b].m) return KBBQ_OK;
        HIPCHK(hipEventSynchronize(c->stage_down[b]));
        threaded_copy(out + (size_t)pending[b].lo * pitch, (uint8_t*)c->stage_host[b] + o_out, (size_t)pending[b].m * pitch);
        pending[b].m = 0;
        return KBBQ_OK;
    };
    int64_t k = 0;
    auto pipelined = [&]() -> int {
        for (int64_t lo = 0; lo < n; lo += (int64_t)slab, ++k) {
            const int b = (int)(k & 1);
            const int64_t m = std::min<int64_t>((int64_t)slab, n - lo);
            int r2 = stage_out(b);                                            // slab k - 2 (same buffers): downloaded -> the caller's rows
            if (r2) return r2;
            if (!out && k >= 2) HIPCHK(hipEventSynchronize(c->stage_up[b]));  // the page-locked slab has been uploaded: free again
            stage_in(b, lo, m);
            if (!out && k >= 2) HIPCHK(hipStreamWaitEvent(c->stage_stream, c->stage_used[b], 0));   // the device slab's kernel has run
            r2 = upload(b, m, c->stage_stream);
            if (r2) return r2;
            HIPCHK(hipEventRecord(c->stage_up[b], c->stage_stream));
            HIPCHK(hipStreamWaitEvent(c->stream, c->stage_up[b], 0));
            r2 = launch((uint8_t*)c->stage_dev[b], plane, m);
            if (r2) return r2;
            HIPCHK(hipEventRecord(c->stage_used[b], c->stream));
            if (!out) continue;
            HIPCHK(hipStreamWaitEvent(c->stage_down_stream, c->stage_used[b], 0));
            HIPCHK(hipMemcpyAsync((uint8_t*)c->stage_host[b] + o_out, (uint8_t*)c->stage_dev[b] + o_out, (size_t)m * pitch, hipMemcpyDeviceToHost, c->stage_down_stream));
            HIPCHK(hipEventRecord(c->stage_down[b], c->stage_down_stream));
            pending[b] = {lo, m};
        }
        return KBBQ_OK;
    };
    for (int pass = 0; ; ++pass) {
        k = 0;
        rc = pipelined();
        if (rc) return stage_drain(c, rc);
        rc = kbbq_ctx_status(c, nullptr);
        if (rc != KBBQ_E_LUT || pass || !exact || !exact()) break;
        (void)stage_drain(c, rc);                                      // the fast run's last downloads: not the caller's rows
        pending[0].m = pending[1].m = 0;
    }
    if (rc == KBBQ_E_FULL) return stage_drain(c, rc);                  // the table, not a read: nothing to look for slab by slab
    if (rc) {
        // something was flagged: which read of the WHOLE input comes first?
        (void)stage_drain(c, rc);
        rc = first_offender(c, n, slab, [&](int64_t lo, int64_t m) {
            stage_in(0, lo, m);
            int r2 = upload(0, m, c->stream);
            return r2 ? r2 : launch((uint8_t*)c->stage_dev[0], plane, m);
        }, bad_read);
        return rc ? rc : fail(KBBQ_E_HIP, "%s: a status reported by the pipelined run did not reproduce slab by slab", who);
    }
    for (int b = 0; b < 2; ++b) { rc = stage_out((int)((k + b) & 1)); if (rc) return stage_drain(c, rc); }     // the older of the two first
    return KBBQ_OK;
}
