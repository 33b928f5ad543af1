// kbbq_hip.hip -- libkbbq_hip.so, the rows unit (it keeps the name of the file the other units were split off): K1 / K2 on rows -- one read per row, mate-pair rows, rows grouped by read group, length
// bands -- with the LUT's layouts, the layout passes and the synthetic reads (C ABI: include/kbbq_hip.h; shared: kbbq_lib.h).
// K1 / K2 launch through one layer: the kernel tables (K1_VARIANTS, LDS_KERNELS) and launch_lds; K1's LDS geometry is k1_geometry +
// k1_lds_plan + launch_k1, K2's choice between persistent and short-lived workgroups k2_tile_serves; k2v3_params / k2t_params /
// fill_row_lut fill the parameter structs.
#include "kbbq_kernels.h"
#include "kbbq_kernels_v3.h"
#include "kbbq_k2_tile.h"
#include "kbbq_row_lut_kernels.h"
#include "kbbq_layout_kernels.h"
#include "kbbq_lib.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

// Tuned launch constants (measured in earlier rounds: DESIGN.md, profiles/)
constexpr size_t K2T_ROW_LUT_MAX = 52 << 10;  // short-lived K2 on one-read-per-row planes: a read group's LUT of up to 52 KB
constexpr int K2V3_FRONTS = 8;               // sequential fronts of the persistent K2 traversal (K2v3Params::parts)
constexpr int K2T_XCD_TILES = 1;             // short-lived K2: every XCD walks a contiguous eighth of the planes (K2tParams::xcd_tiles)
constexpr int K2T_XCD = 8;                   // k2t_order: the read groups' workgroups of one position on the same XCD
constexpr int K7_FRONTS = 8;                 // sequential fronts of k7_lay_out (LayOutParams::parts)

// ---- kernels launched with dynamic LDS ---------------------------------------------------------------------------------
// Each of them is named HERE and nowhere else: launch_lds takes a kernel's address from these tables, and rows_full_lds walks the
// same tables (for kbbq_ctx_create) to allow every one of them the full LDS as dynamic shared memory.  An instance that is not listed is not
// instantiated and cannot be selected.
// K1 (table-driven): form x copies of the context table (DN) x 4-bit planes (NIB) x chunk-position-major cycle table of KJ chunks
// x the error flag in bit 3 of the seq nibbles (EB, KBBQ_ROWS_ERRBIT: the KJ forms only), each without and with SPLIT (a dinucleotide
// threshold above the counting one)
struct K1Variant { K1Form form; int dn, nib, kj, eb; const void* kernel[2]; };   // kernel[split]
#define K1_SPLITS(K, ...) {(const void*)(K<false, __VA_ARGS__>), (const void*)(K<true, __VA_ARGS__>)}
static const K1Variant K1_VARIANTS[] = {
    {K1_ROWS, K1V3_DNREP, 0, 0, 0, K1_SPLITS(k1v3_accumulate, K1V3_DNREP)},
    {K1_ROWS, 8, 0, 0, 0, K1_SPLITS(k1v3_accumulate, 8)},
    {K1_ROWS, K1V3_DNREP, 1, 0, 0, K1_SPLITS(k1v3_accumulate, K1V3_DNREP, true)},
    {K1_ROWS, 8, 1, 0, 0, K1_SPLITS(k1v3_accumulate, 8, true)},
    {K1_ROWS, K1V3_DNREP, 1, 13, 0, K1_SPLITS(k1v3_accumulate, K1V3_DNREP, true, 13)},
    {K1_ROWS, K1V3_DNREP, 1, 19, 0, K1_SPLITS(k1v3_accumulate, K1V3_DNREP, true, 19)},
    {K1_ROWS, K1V3_DNREP, 1, 13, 1, K1_SPLITS(k1v3_accumulate, K1V3_DNREP, true, 13, true)},
    {K1_ROWS, K1V3_DNREP, 1, 19, 1, K1_SPLITS(k1v3_accumulate, K1V3_DNREP, true, 19, true)},
    {K1_ALIGNED, K1V3_DNREP, 0, 0, 0, K1_SPLITS(k1v3_aligned, K1V3_DNREP)},
    {K1_ALIGNED, 8, 0, 0, 0, K1_SPLITS(k1v3_aligned, 8)},
    {K1_ALIGNED_REF, K1V3_DNREP, 0, 0, 0, K1_SPLITS(k1v3_aligned_ref, K1V3_DNREP)},
    {K1_ALIGNED_REF, 8, 0, 0, 0, K1_SPLITS(k1v3_aligned_ref, 8)},
    {K1_BANDS, 0, 0, 0, 0, K1_SPLITS(k1v3_bands, false)},                          // every band brings its own DN (K1BandsParams::dn)
    {K1_BANDS, 0, 1, 0, 0, K1_SPLITS(k1v3_bands, true)},
};
#undef K1_SPLITS

static const void* k1_kernel(K1Form form, bool split, int dn, int nib, int kj, int eb = 0)
{
    for (const K1Variant& v : K1_VARIANTS)
        if (v.form == form && v.dn == dn && v.nib == nib && v.kj == kj && v.eb == eb) return v.kernel[split];
    return nullptr;                                                             // launch_lds reports it
}

// the others: the round-1 kernels (tables beyond the LDS, KBBQ_APPLY_CHECKED) and K2
enum LdsKernel { LK_K1_PLAIN, LK_K1_PLAIN_SPLIT, LK_K1_TILED, LK_K1_TILED_SPLIT, LK_K2V3, LK_K2V3_NIB, LK_K2V3_NIB_EB, LK_K2T, LK_K2T_NIB, LK_K2T_BANDS, LK_K2T_PAIR19, LK_K2T_PAIR13, LK_K2T_PAIR19_EB, LK_K2T_PAIR13_EB, LK_K2_LDS16, LK_K2_LDS8, LK_COUNT };
static const void* const LDS_KERNELS[LK_COUNT] = {
    (const void*)k1_accumulate<false>, (const void*)k1_accumulate<true>,
    (const void*)k1_accumulate_tiled<false>, (const void*)k1_accumulate_tiled<true>,
    (const void*)k2v3_apply<false>, (const void*)k2v3_apply<true>, (const void*)k2v3_apply<true, true>,
    (const void*)k2t_apply<false>, (const void*)k2t_apply<true>, (const void*)k2t_bands,
    (const void*)k2t_apply_pair<19>, (const void*)k2t_apply_pair<13>, (const void*)k2t_apply_pair<19, true>, (const void*)k2t_apply_pair<13, true>,
    (const void*)k2_apply<int16_t, true, true>, (const void*)k2_apply<int8_t, true, false>,
};

// the one launch of a kernel with dynamic LDS: `kernel` comes from K1_VARIANTS (k1_kernel) or LDS_KERNELS, all of which take one
// parameter struct; `which`: the timer the launch counts for (kbbq_ctx_kernel_ms: 0 = K1, 1 = K2)
static int launch_lds(kbbq_ctx* c, int which, const void* kernel, dim3 grid, dim3 block, size_t lds, const void* params)
{
    if (!kernel) return fail(KBBQ_E_HIP, "libkbbq_hip has no instance of K1 for this launch (K1_VARIANTS)");
    void* args[] = {const_cast<void*>(params)};
    {
        Timed t(c, which);
        (void)hipLaunchKernel(kernel, grid, block, args, lds, c->stream);
    }
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// K1's LDS beside `dn` copies of the context table, once the cycle rows are laid out (q.row_bytes, q.slack_bytes): several
// trash rows first (K1v3Params::ntrash: the padding behind every read's last base is the hotter spot), then copies of the cycle
// table for rows of up to 12 chunks (K1v3Params::pos_copies: wider rows spread a wave's lanes over enough columns), as many of
// 8 / 4 / 2 and 4 / 2 as the LDS holds; KBBQ_K1_NTRASH / KBBQ_K1_POSCOPIES cap them (=1: none).  Returns the LDS bytes.
size_t k1_lds_plan(K1v3Params& q, int dn, const kbbq_ctx* c)
{
    auto bytes_for = [&](int nt, int pc) {
        const size_t rows = (size_t)q.nrows - 1 + nt;
        return rows * 128 * dn + (size_t)pc * (rows * q.row_bytes + q.slack_bytes);
    };
    const char* nt_env = getenv("KBBQ_K1_NTRASH");
    const char* pc_env = getenv("KBBQ_K1_POSCOPIES");
    const int most_t = nt_env ? atoi(nt_env) : 8, most = pc_env ? atoi(pc_env) : 4;
    q.ntrash = 1; q.pos_copies = 1;
    for (int nt = 8; nt >= 2; nt >>= 1)
        if (nt <= most_t && bytes_for(nt, 1) <= (size_t)c->lds_bytes) { q.ntrash = nt; break; }
    if (q.cpr <= 12)
        for (int pc = 4; pc >= 2; pc >>= 1)
            if (pc <= most && bytes_for(q.ntrash, pc) <= (size_t)c->lds_bytes) { q.pos_copies = pc; break; }
    q.pos_copy_bytes = (u32)((size_t)(q.nrows - 1 + q.ntrash) * q.row_bytes + q.slack_bytes);
    return bytes_for(q.ntrash, q.pos_copies);
}

// One attempt at K1's LDS geometry: `copies` of the context table beside cycle rows of 3S - cut words (3S words serve reads
// of any length: one word per first-in-pair position [0, S) and per second-in-pair index S + 2(S - len) + pos <= 3S - len - 1).
// False: the tables do not fit the LDS, or the 16-bit packed context counts could overflow between two flushes.
bool k1_geometry(K1v3Params& q, const kbbq_ctx* c, int copies, int cut, int minlen)
{
    q.row_bytes = (u32)((3 * q.S - cut) | 1) * 4u;
    q.minlen = minlen;
    // bytes past a read's end (quality 0) land on the trash row, the last one, at indexes up to 3S - cut - 1 + 15
    q.slack_bytes = (u32)(q.S + 32) * 4u;
    q.dn_flush_iters = std::max(1, 65535 / ((K1V3_THREADS / copies) * 16 * q.cpr));
    const size_t lds = (size_t)q.nrows * 128 * copies + (size_t)q.nrows * q.row_bytes + q.slack_bytes;
    return lds <= (size_t)c->lds_bytes && (K1V3_THREADS / copies) * 16 * q.cpr <= 65535;
}

static bool k1_split(const K1v3Params& q) { return q.type_minscore > q.minscore; }
// iterations one workgroup per read group would make over the rows: no launch has more workgroups per group than this
static int64_t k1_iters(const K1v3Params& q) { return ((q.nreads + 63) / 64 + (K1V3_THREADS / 64) - 1) / (K1V3_THREADS / 64); }

// K1 on the rows of su.q: one 16-wave workgroup per CU, the read groups side by side in grid.y
int launch_k1(kbbq_ctx* c, K1Form form, const K1Setup& su, int nib)
{
    const int gx = (int)std::min<int64_t>(k1_iters(su.q), std::max(1, c->cus / su.q.R));
    return launch_lds(c, 0, k1_kernel(form, k1_split(su.q), su.dn, nib, su.kj, su.eb), dim3((unsigned)gx, (unsigned)su.q.R, 1), dim3(K1V3_THREADS),
                      su.lds, &su.q);
}

// for kbbq_ctx_create: every kernel of the two tables may use the full LDS as dynamic shared memory
void rows_full_lds(int lds_bytes, const CtxLap& lap)
{
    auto full_lds = [&](const void* kernel) {
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (kernel == LDS_KERNELS[0]) lap("first hipFuncSetAttribute");     // the first call loads this unit's code object
    };
    for (const void* kernel : LDS_KERNELS) full_lds(kernel);
    for (const K1Variant& v : K1_VARIANTS) { full_lds(v.kernel[0]); full_lds(v.kernel[1]); }
    lap("the other attributes");
}

extern "C" {

int kbbq_lut_row_stride(int S2) { return lut_row_stride(S2); }

size_t kbbq_full_lut_bytes(int R, int Qt, int S2) { return (size_t)R * (33 + Qt) * (size_t)full_lut_row_bytes(S2); }
size_t kbbq_lut_bytes(int R, int Qt, int S2) { return lut_flags_offset(R, Qt, S2) + 16; }

size_t kbbq_lut_count(int R, int Qt, int S2)
{
    return (size_t)R * Qt * (size_t)lut_row_stride(S2);     // even: K2 stages the LUT as 32-bit words
}

int kbbq_accumulate_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_cseq,
                        const uint8_t* d_qual, const uint32_t* d_meta,
                        int64_t nreads, int pitch, int R, int S2, int minscore, int64_t* d_tables)
{
    return kbbq_accumulate_ex_dev(c, d_seq, d_cseq, d_qual, d_meta, nreads, pitch, R, S2,
                                  minscore, minscore, d_tables);
}

static int accumulate_rows(kbbq_ctx* c, const char* who, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                           const uint32_t* d_meta, int64_t nrows, int pitch, int pairs, int R, int S2, int minscore,
                           int dinuc_minscore, const int64_t* d_seg, int64_t* d_tables, bool* fits, int S_band = 0, int S_min = 0, int nib = 0,
                           int twins = 0, K1Setup* setup_only = nullptr, int errbit = 0);

int kbbq_accumulate_ex_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_cseq,
                           const uint8_t* d_qual, const uint32_t* d_meta,
                           int64_t nreads, int pitch, int R, int S2, int minscore,
                           int dinuc_minscore, int64_t* d_tables)
{
    return kbbq_accumulate_band_dev(c, d_seq, d_cseq, d_qual, d_meta, nreads, pitch, R, S2, 0, 0, minscore, dinuc_minscore, d_tables);
}

int kbbq_accumulate_band_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_cseq,
                             const uint8_t* d_qual, const uint32_t* d_meta,
                             int64_t nreads, int pitch, int R, int S2, int S_band, int S_min, int minscore,
                             int dinuc_minscore, int64_t* d_tables)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_planes("kbbq_accumulate_dev", nreads, pitch, d_seq, d_cseq, d_qual);
    if (rc) return rc;
    if (R <= 0 || R > 32767) return fail(KBBQ_E_ARG, "kbbq_accumulate_dev: R out of range (%d)", R);
    if (S2 <= 0 || (S2 & 1)) return fail(KBBQ_E_ARG, "kbbq_accumulate_dev: S2 must be positive and even (%d)", S2);
    if (minscore < 0 || minscore > KQ - 1) return fail(KBBQ_E_ARG, "kbbq_accumulate_dev: minscore out of range (%d)", minscore);
    if (dinuc_minscore < 0 || dinuc_minscore > 222) return fail(KBBQ_E_ARG, "kbbq_accumulate_dev: dinuc_minscore out of range (%d)", dinuc_minscore);
    if (nreads == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));

    const int64_t nblocks = (nreads + 63) / 64;
    const bool split = dinuc_minscore > minscore;
    bool fits = false;
    rc = accumulate_rows(c, "kbbq_accumulate_dev", d_seq, d_cseq, d_qual, d_meta, nreads, pitch, 0, R, S2, minscore,
                         dinuc_minscore, nullptr, d_tables, &fits, S_band, S_min);
    if (rc || fits) return rc;                          // launched (or a real error); otherwise the tables do not fit the LDS
    K1Params p;
    p.seq = d_seq; p.cseq = d_cseq; p.qual = d_qual; p.meta = d_meta;
    p.nreads = nreads; p.pitch = pitch; p.cpr = pitch / 16; p.cpr_magic = magic_for(p.cpr);
    p.R = R; p.S2 = S2; p.minscore = dinuc_minscore;   // the TypeError rule follows the dinucleotide threshold
    p.qlo = 33u + (u32)minscore; p.dlo = 33u + (u32)dinuc_minscore;
    p.pos_stride = S2 | 1;                         // odd row stride spreads q rows over the banks
    p.tables = reinterpret_cast<u64*>(d_tables); p.status = c->d_status;
    auto lds_of = [](int stride) { return ((size_t)(((KQ * stride) + 1) & ~1)) * 4 + (size_t)KQ * KND * 8; };
    size_t lds = lds_of(p.pos_stride);
    K1TiledParams tp;
    int tiles = 1;
    if (lds > (size_t)c->lds_bytes) {
        // the KQ x S2 table is beyond the LDS: the fewest equal tiles of an even number of columns whose KQ x (tile_w | 1) table fits
        const int max_w = (int)((((size_t)c->lds_bytes - (size_t)KQ * KND * 8) / 4 - 1) / KQ - 1) & ~1;
        if (max_w < 2) return fail(KBBQ_E_ARG, "kbbq_accumulate_dev: %d B of LDS hold no tile of the tables", c->lds_bytes);
        tiles = (S2 + max_w - 1) / max_w;
        tp.tile_w = ((S2 + tiles - 1) / tiles + 1) & ~1;
        tiles = (S2 + tp.tile_w - 1) / tp.tile_w;
        p.pos_stride = tp.tile_w | 1;
        lds = lds_of(p.pos_stride);
    }
    int per_cu = std::min<int>((int)(c->lds_bytes / lds), 2048 / K1_THREADS);
    per_cu = std::max(per_cu, 1);
    if (tiles > 1) {                                // k1_accumulate_tiled: a workgroup iteration is K1_THREADS chunks
        tp.k = p;
        const int64_t iters = (nreads * p.cpr + K1_THREADS - 1) / K1_THREADS;
        const int gx = (int)std::min<int64_t>(iters, std::max<int64_t>(1, (int64_t)c->cus * per_cu / ((int64_t)R * tiles)));
        return launch_lds(c, 0, LDS_KERNELS[split ? LK_K1_TILED_SPLIT : LK_K1_TILED], dim3((unsigned)gx, (unsigned)R, (unsigned)tiles),
                          dim3(K1_THREADS), lds, &tp);
    }
    const int64_t iters = (nblocks + (K1_THREADS / 64) - 1) / (K1_THREADS / 64);
    int gx = (int)std::min<int64_t>(iters, std::max(1, c->cus * per_cu / R));
    return launch_lds(c, 0, LDS_KERNELS[split ? LK_K1_PLAIN_SPLIT : LK_K1_PLAIN], dim3((unsigned)gx, (unsigned)R, 1), dim3(K1_THREADS), lds, &p);
}

// host twin of k3_fill_full_lut (same rules; the GPU test compares the two blobs byte for byte)
static int fill_full_lut_host(const int16_t* lut16, int rs16, int R, int Qt, int S2, int minscore, int8_t* full,
                              int8_t* compact8)
{
    const int rb = full_lut_row_bytes(S2);
    const int NR = 33 + Qt;
    int bad = 0;
    for (int r = 0; r < R; ++r)
        for (int qb = 0; qb < NR; ++qb) {
            int8_t* row = full + ((size_t)r * NR + qb) * rb;
            for (int x = 0; x < rb; ++x) {
                const int W = full_lut_width(S2);
                int v = 0;
                if (qb < 33 + minscore) { if (x < 2 * W) v = qb == 0 ? -33 : qb - 33; }
                else {
                    const int16_t* src = lut16 + ((size_t)r * Qt + (qb - 33)) * rs16;
                    if (x < S2) v = src[x];
                    else if (x >= W && x < W + S2) v = src[S2 - 1 - (x - W)];
                    else if (x >= 2 * W && x < 2 * W + 25) v = src[S2 + (x - 2 * W)];
                }
                if (v < -128 || v > 127) bad |= 1;
                row[x] = (int8_t)v;
            }
        }
    for (size_t i = 0; i < (size_t)R * Qt * rs16; ++i) {
        if (lut16[i] < -128 || lut16[i] > 127) bad |= 1;
        compact8[i] = (int8_t)lut16[i];
    }
    for (int r = 0; r < R; ++r)
        for (int q = minscore; q < Qt; ++q) {
            const int16_t* src = lut16 + ((size_t)r * Qt + q) * rs16;
            int lo1 = 32767, hi1 = -32768, lo2 = 32767, hi2 = -32768;
            for (int x = 0; x < S2; ++x) { lo1 = std::min<int>(lo1, src[x]); hi1 = std::max<int>(hi1, src[x]); }
            for (int x = 0; x < 25; ++x) { lo2 = std::min<int>(lo2, src[S2 + x]); hi2 = std::max<int>(hi2, src[S2 + x]); }
            if (lo1 + lo2 + 33 < 0 || hi1 + hi2 + 33 > 255) bad |= 2;
        }
    return bad;
}

int kbbq_build_lut(int R, int Qt, int S2, int D, int minscore, const int64_t* meanq, const int64_t* rgdq,
                   const int64_t* qdq, const int64_t* posdq, const int64_t* dinucdq, void* blob,
                   int* flags_out)
{
    // D = 17 is what get_delta_qs returns (applybqsr.py:98-101); D = 16 is accepted because the
    // reference's own apply test passes an unpadded table (index -1 then aliases column 15)
    if (R <= 0 || Qt <= 0 || Qt > 95 || S2 <= 0 || D < 16 || D > 17 || minscore < 0)
        return fail(KBBQ_E_ARG, "kbbq_build_lut: bad shape R=%d Qt=%d S2=%d D=%d minscore=%d", R, Qt, S2, D, minscore);
    memset(blob, 0, kbbq_lut_bytes(R, Qt, S2));
    int16_t* out = reinterpret_cast<int16_t*>(blob);
    const int rs = lut_row_stride(S2);
    for (int r = 0; r < R; ++r)
        for (int q = 0; q < Qt; ++q) {
            const size_t cell = (size_t)r * Qt + q;
            int16_t* row = out + cell * rs;
            const int64_t base = meanq[r] + rgdq[r] + qdq[cell];
            for (int s = 0; s < S2; ++s) {
                const int64_t v = base + posdq[cell * S2 + s];
                if (v < -32768 || v > 32767) return fail(KBBQ_E_RANGE, "kbbq_build_lut: value %lld does not fit the LUT", (long long)v);
                row[s] = (int16_t)v;
            }
            // dinucleotide index 5 * prev + cur, codes A0 T1 G2 C3 and 4 = N / no previous base;
            // anything involving code 4 is the reference's index -1, i.e. column D - 1
            for (int a = 0; a < 5; ++a)
                for (int b = 0; b < 5; ++b) {
                    const int64_t v = (a < 4 && b < 4) ? dinucdq[cell * D + 4 * a + b] : dinucdq[cell * D + (D - 1)];
                    if (v < -32768 || v > 32767) return fail(KBBQ_E_RANGE, "kbbq_build_lut: value %lld does not fit the LUT", (long long)v);
                    row[S2 + 5 * a + b] = (int16_t)v;
                }
        }
    int8_t* full = reinterpret_cast<int8_t*>(blob) + lut_full_offset(R, Qt, S2);
    int8_t* compact8 = reinterpret_cast<int8_t*>(blob) + lut_compact8_offset(R, Qt, S2);
    const int flags = fill_full_lut_host(out, rs, R, Qt, S2, std::min(minscore, Qt), full, compact8);
    *reinterpret_cast<int*>(reinterpret_cast<char*>(blob) + lut_flags_offset(R, Qt, S2)) = flags;
    if (flags_out) *flags_out = flags;
    return KBBQ_OK;
}

// K2 on one-read-per-row planes of this pitch: the cycle width Sb of the LUT, the columns such rows can reach
// (KBBQ_K2_ROWLUT=0: the tables' full S2, A/B timing)
static int row_lut_width(int pitch, int S2) { return env_is("KBBQ_K2_ROWLUT", "0") ? S2 : std::min(pitch, S2); }

// the LUT of cycle width Sb (k3_fill_row_lut) written to `dst`, on the launch stream in front of the apply kernel that reads it
static const int8_t* fill_row_lut(kbbq_ctx* c, const void* d_lut_blob, int R, int Qt, int S2, int Sb, int minscore, void* dst)
{
    RowLutParams f;
    f.lut16 = reinterpret_cast<const int16_t*>(d_lut_blob); f.rs16 = lut_row_stride(S2); f.R = R; f.Qt = Qt; f.S2 = S2; f.Sb = Sb;
    f.minscore = std::min(std::max(minscore, 0), Qt);
    f.out = reinterpret_cast<int8_t*>(dst);
    hipLaunchKernelGGL(k3_fill_row_lut, dim3((unsigned)(R * (33 + Qt))), dim3(256), 0, c->stream, f);
    return f.out;
}

// ... when Sb < S2, that narrowed LUT in context-owned scratch (Sb == S2: the blob's own full LUT is used, *lut untouched).
// False: no scratch for it.
static bool narrowed_row_lut(kbbq_ctx* c, const void* d_lut_blob, int R, int Qt, int S2, int Sb, int minscore, const int8_t** lut)
{
    if (Sb >= S2) return true;
    if (grow_scratch(c, c->rowlut, (size_t)R * (33 + Qt) * full_lut_row_bytes(Sb))) return false;
    *lut = fill_row_lut(c, d_lut_blob, R, Qt, S2, Sb, minscore, c->rowlut.p);
    return true;
}

// Does K2 run with short-lived workgroups (kbbq_k2_tile.h) on rows of `cpr` chunks, `rg_bytes` of LUT per read group?  Mate-pair
// rows and one-read-per-row planes, 4-bit and character planes (round 4; KBBQ_K2_TILE_CHARS=0: the persistent kernel as before),
// one read group or rows grouped by read group, unless KBBQ_K2_TILE=0 (A/B timing); everything else, and LUTs of one group beyond
// a third of the LDS, keeps the persistent kernel
// (one read per row: while two workgroups' copies of the narrowed LUT fit a CU -- rows of up to ~300 bases; measured up to
//  there, scripts/gpu_tilekb.sh: config 5's K2 0.651 -> 0.687 of roofline going from a 32 KB to a 52 KB limit)
static bool k2_tile_serves(const kbbq_ctx* c, int pairs, int nib, int R, bool grouped, int cpr, size_t rg_bytes)
{
    if (env_is("KBBQ_K2_TILE", "0") || (!nib && env_is("KBBQ_K2_TILE_CHARS", "0"))) return false;
    if ((R != 1 && !grouped) || cpr < 2 || cpr > 4096) return false;
    return pairs ? rg_bytes * 3 <= (size_t)c->lds_bytes : rg_bytes <= K2T_ROW_LUT_MAX;
}

// K2v3Params of rows whose LUT has Qt quality rows and, one read per row, the cycle width Sb (mate-pair rows: their own LUT,
// d_pair_lut).  q.full is the blob's full LUT: the caller narrows it (narrowed_row_lut, fill_row_lut) when Sb < S2.
static K2v3Params k2v3_params(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta, int64_t nrows, int pitch,
                              int pairs, int R, int Qt, int S2, int Sb, int minscore, const void* d_lut_blob, const void* d_pair_lut,
                              const int64_t* d_seg, const int64_t* d_perm, uint8_t* d_out)
{
    K2v3Params q;
    q.seq = d_seq; q.qual = d_qual; q.meta = d_meta; q.nreads = nrows; q.pitch = pitch;
    q.cpr = pitch / 16; q.cpr_magic = magic_for(q.cpr);
    q.R = R; q.Qt = Qt; q.S2 = S2; q.minscore = minscore; q.qlo = 33u + (u32)minscore;
    q.lut16 = reinterpret_cast<const int16_t*>(d_lut_blob); q.rs16 = lut_row_stride(S2);
    q.full = pairs ? reinterpret_cast<const int8_t*>(d_pair_lut)
                   : reinterpret_cast<const int8_t*>(d_lut_blob) + lut_full_offset(R, Qt, S2);
    q.rb = (u32)(pairs ? pair_lut_row_bytes(S2) : full_lut_row_bytes(Sb));
    q.full_bytes = (int)((size_t)R * (33 + Qt) * q.rb);
    if (pairs) { q.W = 0u; q.ctx_off = (u32)pair_pitch(S2); q.maxlen = S2 + 1; }
    else { q.W = (u32)full_lut_width(Sb); q.ctx_off = 2u * q.W; q.maxlen = Sb; }
    q.pairs = pairs; q.seg = reinterpret_cast<const long long*>(d_seg);
    q.perm = reinterpret_cast<const long long*>(d_perm);
    q.parts = K2V3_FRONTS;
    q.rpb = 64;      // the persistent kernel's wave block; smaller blocks were measured slower (profiles/r01_traversal_microbench.md)
    q.out = d_out; q.status = c->d_status;
    return q;
}

// the persistent K2 on these rows: every read group's LUT in the LDS, or -- rows grouped by read group -- a slice of the grid
// per group with that group's
static int launch_k2v3(kbbq_ctx* c, const K2v3Params& q, int nib, int errbit = 0)
{
    const int slices = q.seg ? q.R : 1;
    const size_t lds = (size_t)(33 + q.Qt) * q.rb * (size_t)(q.seg ? 1 : q.R);
    // resident workgroups per CU: LDS copies of the LUT, and the register allocation's waves per SIMD
    const int per_cu = std::max(1, std::min<int>((int)(c->lds_bytes / lds), (K2V3_WAVES * 4 * 64) / K2V3_THREADS));
    const int64_t nblocks = (q.nreads + q.rpb - 1) / q.rpb;
    const int64_t want = (nblocks + (K2V3_THREADS / 64) - 1) / (K2V3_THREADS / 64);
    const int gx = (int)std::min<int64_t>(want, std::max<int64_t>(1, (int64_t)c->cus * per_cu / slices));
    return launch_lds(c, 1, LDS_KERNELS[errbit ? LK_K2V3_NIB_EB : nib ? LK_K2V3_NIB : LK_K2V3], dim3((unsigned)std::max(gx, 1), (unsigned)slices, 1), dim3(K2V3_THREADS), lds, &q);
}

static int apply_rows(kbbq_ctx* c, const char* who, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta,
                      int64_t nrows, int pitch, int pairs, int R, int S2, int minscore, const void* d_lut_blob,
                      const void* d_pair_lut, const int64_t* d_seg, uint8_t* d_out, int nib = 0, const int64_t* d_perm = nullptr, int errbit = 0);

int kbbq_apply_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta,
                   int64_t nreads, int pitch, int R, int Qt, int S2, int minscore,
                   const void* d_lut, int mode, uint8_t* d_out)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_planes("kbbq_apply_dev", nreads, pitch, d_seq, d_qual, d_out);
    if (rc) return rc;
    if (R <= 0 || R > 32767 || Qt <= 0 || Qt > 95 || S2 <= 0 || S2 > 65536)
        return fail(KBBQ_E_ARG, "kbbq_apply_dev: bad table shape R=%d Qt=%d S2=%d (Qt <= 95)", R, Qt, S2);
    if (minscore < 0 || minscore > 222) return fail(KBBQ_E_ARG, "kbbq_apply_dev: minscore out of range");
    if ((uintptr_t)d_lut & 15) return fail(KBBQ_E_ARG, "kbbq_apply_dev: LUT must be 16-byte aligned");
    if (mode != KBBQ_APPLY_CHECKED && mode != KBBQ_APPLY_FAST) return fail(KBBQ_E_ARG, "kbbq_apply_dev: bad mode %d", mode);
    if (nreads == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    const int64_t nblocks = (nreads + 63) / 64;

    // the LUT of the columns rows of this pitch can reach (narrowed_row_lut): a band of short reads under wide tables
    const int Sb = row_lut_width(pitch, S2);
    const size_t full_bytes = (size_t)R * (33 + Qt) * full_lut_row_bytes(Sb);
    // one read group, rows as a caller holds them (one character row per read): the short-lived kernel through apply_rows when it
    // serves them.  What it cannot serve (a foreign letter, q > 42, a read longer than the LUT, a read group other than 0 -- and,
    // because it screens whole 16-byte chunks, a byte other than 'N' in the sequence padding of a read's last chunk) it reports as
    // KBBQ_E_LUT with no read index: a KBBQ_APPLY_CHECKED run over the same rows decides, as for a LUT that is not range-safe.
    // Who re-runs: the caller of this entry point (kbbq/_device.py apply); kbbq_apply does it itself (stage_run's `exact`).
    if (mode == KBBQ_APPLY_FAST && R == 1 && Qt == KQ && !(S2 & 1) && S2 <= 65534
        && k2_tile_serves(c, 0, 0, R, false, pitch / 16, (size_t)(33 + KQ) * full_lut_row_bytes(Sb)))
        return apply_rows(c, "kbbq_apply_dev", d_seq, d_qual, d_meta, nreads, pitch, 0, R, S2, minscore, d_lut, nullptr, nullptr, d_out, 0, nullptr);
    if (mode == KBBQ_APPLY_FAST && full_bytes <= (size_t)c->lds_bytes) {
        // the persistent kernel as apply_rows launches it, for any Qt and an odd S2 too (apply_rows takes neither)
        K2v3Params q = k2v3_params(c, d_seq, d_qual, d_meta, nreads, pitch, 0, R, Qt, S2, Sb, minscore, d_lut, nullptr, nullptr, nullptr, d_out);
        if (!narrowed_row_lut(c, d_lut, R, Qt, S2, Sb, minscore, &q.full)) return fail(KBBQ_E_HIP, "kbbq_apply_dev: no scratch for the narrowed LUT");
        return launch_k2v3(c, q, 0);
    }

    K2Params p;
    p.seq = d_seq; p.qual = d_qual; p.meta = d_meta; p.nreads = nreads; p.pitch = pitch;
    p.cpr = pitch / 16; p.cpr_magic = magic_for(p.cpr);
    p.R = R; p.Qt = Qt; p.S2 = S2; p.minscore = minscore; p.qlo = 33u + (u32)minscore;
    p.lut = reinterpret_cast<const int16_t*>(d_lut); p.lut_count = (int)kbbq_lut_count(R, Qt, S2);
    p.out = d_out; p.status = c->d_status;
    // FAST (flags == 0): every value fits int8 -> stage the one-byte copy; CHECKED: the int16 LUT.
    // Too big for LDS either way: per-base exact path from global memory.
    const bool fast = mode == KBBQ_APPLY_FAST;
    const size_t stage_bytes = fast ? lut_compact8_bytes(R, Qt, S2) : (size_t)p.lut_count * 2;
    const bool in_lds = stage_bytes + 16 <= (size_t)c->lds_bytes;
    p.lut_in_lds = in_lds ? 1 : 0;
    p.stage = fast ? (const void*)(reinterpret_cast<const char*>(d_lut) + lut_compact8_offset(R, Qt, S2)) : d_lut;
    p.stage_bytes = (int)stage_bytes;
    const size_t lds = in_lds ? ((stage_bytes + 15) & ~(size_t)15) : 0;
    // 256-thread workgroups while >= 4 of them fit a CU, else 1024-thread ones (same waves per CU)
    int threads = 256, per_cu = 8;
    if (in_lds) {
        per_cu = (int)(c->lds_bytes / lds);
        if (per_cu < 4) { threads = 1024; per_cu = std::min(per_cu, 2); }
        per_cu = std::max(1, std::min(per_cu, 2048 / threads));
    }
    const int64_t want = (nblocks + (threads / 64) - 1) / (threads / 64);
    int gx = (int)std::min<int64_t>(want, (int64_t)c->cus * per_cu);
    dim3 grid((unsigned)std::max(gx, 1), 1, 1), block((unsigned)threads, 1, 1);
    if (in_lds) return launch_lds(c, 1, LDS_KERNELS[fast ? LK_K2_LDS8 : LK_K2_LDS16], grid, block, lds, &p);
    {
        Timed t(c, 1);
        hipLaunchKernelGGL((k2_apply<int16_t, false, true>), grid, block, 0, c->stream, p);       // the LUT stays in global memory: no LDS
    }
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_synth_dev(kbbq_ctx* c, uint8_t* d_seq, uint8_t* d_cseq, uint8_t* d_qual, uint32_t* d_meta,
                   int64_t first, int64_t nreads, int64_t total, int pitch, uint64_t seed,
                   int len_lo, int len_hi, int nrg, int qlo, int qhi, const uint32_t* thr43)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_planes("kbbq_synth_dev", nreads, pitch, d_seq, d_cseq, d_qual);
    if (rc) return rc;
    if (len_lo < 0 || len_hi < len_lo || len_hi > pitch || nrg <= 0 || nrg > 32767 || qlo < 0 || qhi < qlo || qhi >= KQ || total <= 0)
        return fail(KBBQ_E_ARG, "kbbq_synth_dev: bad shape");
    if (nreads == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    KSParams p;
    p.seq = d_seq; p.cseq = d_cseq; p.qual = d_qual; p.meta = d_meta;
    p.first = first; p.nreads = nreads; p.total = total; p.pitch = pitch; p.cpr = pitch / 16;
    p.seed = seed; p.len_lo = len_lo; p.len_hi = len_hi; p.nrg = nrg; p.qlo = qlo; p.qhi = qhi;
    memcpy(p.thr, thr43, sizeof p.thr);
    const int64_t nchunks = nreads * p.cpr;
    int gx = (int)std::min<int64_t>((nchunks + 255) / 256, (int64_t)c->cus * 8);
    hipLaunchKernelGGL(ks_synth, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// ---- mate-pair rows ---------------------------------------------------------
int kbbq_pair_pitch(int S2) { return pair_pitch(S2); }
size_t kbbq_pair_lut_bytes(int R, int Qt, int S2) { return (size_t)R * (33 + Qt) * pair_lut_row_bytes(S2); }

static int check_pairs(const char* who, int64_t npairs, int S2)
{
    if (npairs < 0) return fail(KBBQ_E_ARG, "%s: npairs < 0", who);
    if (S2 <= 0 || (S2 & 1) || S2 > 65534) return fail(KBBQ_E_ARG, "%s: S2 must be positive and even (%d)", who, S2);
    return KBBQ_OK;
}

int kbbq_pack_pairs_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                        const uint32_t* d_meta, int64_t npairs, int pitch, int S2,
                        uint8_t* d_pseq, uint8_t* d_pcseq, uint8_t* d_pqual, uint32_t* d_pmeta)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_pairs("kbbq_pack_pairs_dev", npairs, S2);
    if (rc) return rc;
    if (pitch <= 0 || (pitch & 15) || pitch < S2 / 2) return fail(KBBQ_E_ARG, "kbbq_pack_pairs_dev: bad pitch %d", pitch);
    if (!d_seq || !d_qual || !d_meta || !d_pseq || !d_pqual || !d_pmeta || (d_cseq && !d_pcseq))
        return fail(KBBQ_E_ARG, "kbbq_pack_pairs_dev: NULL pointer");
    if (((uintptr_t)d_pseq | (uintptr_t)d_pcseq | (uintptr_t)d_pqual) & 15) return fail(KBBQ_E_ARG, "kbbq_pack_pairs_dev: planes must be 16-byte aligned");
    if (npairs == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    PairPackParams p;
    p.src[0] = d_seq; p.src[1] = d_cseq; p.src[2] = d_qual;
    p.dst[0] = d_pseq; p.dst[1] = d_pcseq; p.dst[2] = d_pqual;
    p.fill[0] = 'N'; p.fill[1] = 'N'; p.fill[2] = 0;
    p.meta = d_meta; p.pmeta = d_pmeta; p.npairs = npairs; p.pitch = pitch; p.ppitch = pair_pitch(S2); p.S = S2 / 2; p.unpack = 0;
    const int64_t nchunks = npairs * (p.ppitch / 16);
    const int gx = bounded_grid((nchunks + 255) / 256, c, 256);
    hipLaunchKernelGGL(k7_pack_pairs, dim3((unsigned)gx), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_unpack_pairs_dev(kbbq_ctx* c, const uint8_t* d_pplane, int64_t npairs, int S2, int pitch, uint8_t* d_plane)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_pairs("kbbq_unpack_pairs_dev", npairs, S2);
    if (rc) return rc;
    if (pitch <= 0 || (pitch & 15) || pitch < S2 / 2) return fail(KBBQ_E_ARG, "kbbq_unpack_pairs_dev: bad pitch %d", pitch);
    if (!d_pplane || !d_plane || ((uintptr_t)d_plane & 15)) return fail(KBBQ_E_ARG, "kbbq_unpack_pairs_dev: bad pointer");
    if (npairs == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    PairPackParams p;
    p.src[0] = d_pplane; p.src[1] = nullptr; p.src[2] = nullptr; p.dst[0] = d_plane; p.dst[1] = nullptr; p.dst[2] = nullptr;
    p.fill[0] = p.fill[1] = p.fill[2] = 0;
    p.meta = nullptr; p.pmeta = nullptr; p.npairs = npairs; p.pitch = pitch; p.ppitch = pair_pitch(S2); p.S = S2 / 2; p.unpack = 1;
    const int64_t nchunks = 2 * npairs * (pitch / 16);
    const int gx = bounded_grid((nchunks + 255) / 256, c, 256);
    hipLaunchKernelGGL(k7_pack_pairs, dim3((unsigned)gx), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// K1 (table-driven kernel) on one-read-per-row or mate-pair rows, optionally grouped by read group
static int accumulate_rows(kbbq_ctx* c, const char* who, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                           const uint32_t* d_meta, int64_t nrows, int pitch, int pairs, int R, int S2, int minscore,
                           int dinuc_minscore, const int64_t* d_seg, int64_t* d_tables, bool* fits, int S_band, int S_min, int nib, int twins,
                           K1Setup* setup_only, int errbit)
{
    if (fits) *fits = true;
    if (S_band < 0 || S_band > S2 / 2 || (pairs && S_band)) return fail(KBBQ_E_ARG, "%s: S_band out of range (%d)", who, S_band);
    if (S_min < 0 || S_min > (S_band ? S_band : S2 / 2)) return fail(KBBQ_E_ARG, "%s: S_min out of range (%d)", who, S_min);
    // KBBQ_ROWS_ERRBIT: the corrected plane is not read (and may be NULL); only the joint-row forms below know the flag
    if (errbit) d_cseq = nullptr;
    if (errbit && !(pairs && nib && (pitch == 16 * 19 || pitch == 16 * 13)))
        return fail(KBBQ_E_ARG, "%s: KBBQ_ROWS_ERRBIT describes 4-bit mate-pair rows of 19 or 13 chunks (pitch %d)", who, pitch);
    int rc = check_planes(who, nrows, pitch, d_seq, d_cseq, d_qual);
    if (rc) return rc;
    if (R <= 0 || R > 32767) return fail(KBBQ_E_ARG, "%s: R out of range (%d)", who, R);
    if (S2 <= 0 || (S2 & 1) || S2 > 65534) return fail(KBBQ_E_ARG, "%s: S2 must be positive and even (%d)", who, S2);
    if (minscore < 0 || minscore > KQ - 1) return fail(KBBQ_E_ARG, "%s: minscore out of range (%d)", who, minscore);
    if (dinuc_minscore < 0 || dinuc_minscore > 222) return fail(KBBQ_E_ARG, "%s: dinuc_minscore out of range (%d)", who, dinuc_minscore);
    if (pairs && pitch != pair_pitch(S2)) return fail(KBBQ_E_ARG, "%s: mate-pair rows of %d-base reads have pitch %d, not %d", who, S2 / 2, pair_pitch(S2), pitch);
    if (nrows == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    const int S = S_band ? S_band : S2 / 2;          // the LDS tables are laid out for the longest read of THIS batch
    K1Setup su;
    K1v3Params& q = su.q;
    q.aflags = nullptr; q.aclip = nullptr; q.atrim = nullptr;
    q.seq = d_seq; q.cseq = d_cseq; q.qual = d_qual; q.meta = d_meta;
    q.nreads = nrows; q.pitch = pitch; q.cpr = pitch / 16; q.cpr_magic = magic_for(q.cpr);
    q.R = R; q.S = S; q.gS2 = S2; q.minscore = minscore; q.type_minscore = dinuc_minscore;
    q.qlo_m1 = 32u + (u32)minscore; q.dlo = 33u + (u32)dinuc_minscore;
    q.nrows = KQ + 1 - minscore;
    q.maxlen = pairs ? S2 + 1 : S; q.gap = pairs ? 1 : 0; q.twins = (pairs && twins) ? 1 : 0;
    q.seg = reinterpret_cast<const long long*>(d_seg);
    q.tables = reinterpret_cast<u64*>(d_tables); q.status = c->d_status;
    q.genome = nullptr; q.ag0 = nullptr;
    // LDS geometry (k1_geometry).  When 3S words per cycle row do not fit (reads of ~200 bases and more), a band whose shortest
    // read is S_min needs only 3S - S_min words, and 8 copies of the context table instead of 16 free the rest: reads of up to
    // ~300 bases still run this kernel.
    const int trim = (!pairs && S_min > 0) ? std::min(S_min, S) : 0;
    // mate-pair rows of 19 or 13 chunks (2 x 150, 2 x 100 bp) on 4-bit planes: the chunk-position-major cycle table (kernel comment), the
    // 13-chunk form with 8 trash rows (K1v3Params::ntrash; 19 chunks were measured with 4 and 8 of them: nothing).  Measured for the other
    // lengths instruments emit (profiles/): 2 x 100 bp 1.37 -> 1.31 ms per 3 Gbases; 2 x 50 bp (7 chunks) is FASTER position-major with its
    // copies of the cycle table (1.52 against 1.64 ms); 2 x 75 / 2 x 125 / 2 x 250 bp never take mate-pair rows (2 S + 1 rounds up to
    // twice the single read's pitch: no bytes saved).
    if (pairs && nib && (q.cpr == 19 || q.cpr == 13)) {
        // joint rows (k1v3_body): a quality's cycle words, then its 32 context slots x 16 copies -- 832 / 736 words, multiples of 32
        q.row_bytes = (u32)((((16 * q.cpr + 31) & ~31) + 32 * K1V3_DNREP) * 4);
        q.minlen = 0; q.slack_bytes = 0; q.pos_copies = 1;
        q.dn_flush_iters = std::max(1, 65535 / ((K1V3_THREADS / K1V3_DNREP) * 16 * q.cpr));
        for (int nt = q.cpr == 19 ? 1 : 8; nt >= 1 && !su.dn; nt >>= 1) {
            const size_t rows = (size_t)q.nrows - 1 + nt;
            su.lds = rows * q.row_bytes;
            if (su.lds > (size_t)c->lds_bytes) continue;
            su.dn = K1V3_DNREP; su.kj = q.cpr; su.eb = errbit ? 1 : 0;       // the form applies AND its tables fit
            q.ntrash = nt; q.pos_copy_bytes = (u32)(rows * q.row_bytes);
        }
    }
    // (44 rows of 3328 / 2944 bytes at most: they fit the 160 KB of a gfx950 CU.  A guard, not a fallback: no other form of K1 knows the flag)
    if (errbit && !su.kj) return fail(KBBQ_E_ARG, "%s: the joint-row tables of KBBQ_ROWS_ERRBIT rows do not fit the LDS (%d bytes)", who, c->lds_bytes);
    for (int attempt = 0; attempt < (trim ? 3 : 1) && !su.dn; ++attempt) {
        const int copies = attempt == 2 ? 8 : K1V3_DNREP, cut = attempt ? trim : 0;
        if (k1_geometry(q, c, copies, cut, cut)) su.dn = copies;
    }
    if (!su.dn) {
        if (fits) { *fits = false; return KBBQ_OK; }     // the caller has another kernel for this shape
        return fail(KBBQ_E_LUT, "%s: %d-base reads with minscore %d do not fit the LDS tables; use plain one-read-per-row planes", who, S, minscore);
    }
    if (!su.kj) su.lds = k1_lds_plan(q, su.dn, c);
    if (setup_only) { *setup_only = su; return KBBQ_OK; }
    return launch_k1(c, K1_ROWS, su, nib);
}

int kbbq_accumulate_pairs_dev(kbbq_ctx* c, const uint8_t* d_pseq, const uint8_t* d_pcseq, const uint8_t* d_pqual,
                              const uint32_t* d_pmeta, int64_t npairs, int R, int S2, int minscore,
                              int dinuc_minscore, int64_t* d_tables)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_pairs("kbbq_accumulate_pairs_dev", npairs, S2);
    if (rc) return rc;
    return accumulate_rows(c, "kbbq_accumulate_pairs_dev", d_pseq, d_pcseq, d_pqual, d_pmeta, npairs, pair_pitch(S2), 1,
                           R, S2, minscore, dinuc_minscore, nullptr, d_tables, nullptr);
}

int kbbq_accumulate_grouped_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                                const uint32_t* d_meta, int64_t nrows, int pitch, int pairs, int R, int S2, int S_band,
                                int S_min, int minscore, int dinuc_minscore, const int64_t* d_seg, int64_t* d_tables)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (!d_seg) return fail(KBBQ_E_ARG, "kbbq_accumulate_grouped_dev: d_seg is NULL");
    return accumulate_rows(c, "kbbq_accumulate_grouped_dev", d_seq, d_cseq, d_qual, d_meta, nrows, pitch, pairs ? 1 : 0,
                           R, S2, minscore, dinuc_minscore, d_seg, d_tables, nullptr, S_band, S_min);
}

int kbbq_pair_lut_dev(kbbq_ctx* c, const void* d_lut_blob, int R, int S2, int minscore, void* d_pair_lut)
{
    return kbbq_pair_lut_rows_dev(c, d_lut_blob, R, S2, minscore, KBBQ_ROWS_PAIRS, d_pair_lut);
}

int kbbq_pair_lut_rows_dev(kbbq_ctx* c, const void* d_lut_blob, int R, int S2, int minscore, int flags, void* d_pair_lut)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_pairs("kbbq_pair_lut_dev", 0, S2);
    if (rc) return rc;
    if (!(flags & KBBQ_ROWS_PAIRS) || (flags & ~(KBBQ_ROWS_PAIRS | KBBQ_ROWS_NIBBLES | KBBQ_ROWS_TWINS | KBBQ_ROWS_ERRBIT)))
        return fail(KBBQ_E_ARG, "kbbq_pair_lut_rows_dev: flags 0x%x are not those of mate-pair rows", flags);
    if (R <= 0 || R > 32767 || !d_lut_blob || !d_pair_lut) return fail(KBBQ_E_ARG, "kbbq_pair_lut_dev: bad argument");
    HIPCHK(hipSetDevice(c->device));
    PairLutParams f;
    f.lut16 = reinterpret_cast<const int16_t*>(d_lut_blob); f.rs16 = lut_row_stride(S2); f.R = R; f.Qt = KQ; f.S2 = S2;
    f.minscore = std::min(std::max(minscore, 0), KQ);
    f.twins = (flags & KBBQ_ROWS_TWINS) ? 1 : 0;
    f.out = reinterpret_cast<int8_t*>(d_pair_lut);
    hipLaunchKernelGGL(k3_fill_pair_lut, dim3((unsigned)(R * (33 + KQ))), dim3(256), 0, c->stream, f);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// the short-lived kernel's parameters for the rows and the LUT of `q` (no workgroup plan: one read group, all rows)
static K2tParams k2t_params(const K2v3Params& q)
{
    K2tParams t;
    t.seq = q.seq; t.qual = q.qual; t.meta = q.meta; t.nchunks = q.nreads * q.cpr; t.cpr = q.cpr; t.cpr_magic = q.cpr_magic;
    t.Qt = q.Qt; t.S2 = q.S2; t.maxlen = q.maxlen; t.lut = q.full; t.lut_bytes = (int)(((size_t)(33 + q.Qt) * q.rb + 15) & ~(size_t)15);
    t.rb = q.rb; t.ctx_off = q.ctx_off; t.W = q.W; t.seg = q.seg; t.R = q.R; t.wg_start = nullptr; t.order = nullptr;
    t.perm = q.perm; t.pitch = q.pitch; t.out = q.out; t.status = q.status;
    t.xcd_tiles = K2T_XCD_TILES;
    return t;
}

// K2 (table-driven kernel) on one-read-per-row or mate-pair rows, optionally grouped by read group
static int apply_rows(kbbq_ctx* c, const char* who, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta,
                      int64_t nrows, int pitch, int pairs, int R, int S2, int minscore, const void* d_lut_blob,
                      const void* d_pair_lut, const int64_t* d_seg, uint8_t* d_out, int nib, const int64_t* d_perm, int errbit)
{
    int rc = check_planes(who, nrows, pitch, d_seq, d_qual, d_out);
    if (rc) return rc;
    if (errbit && !(pairs && nib && (pitch == 16 * 19 || pitch == 16 * 13)))
        return fail(KBBQ_E_ARG, "%s: KBBQ_ROWS_ERRBIT describes 4-bit mate-pair rows of 19 or 13 chunks (pitch %d)", who, pitch);
    if (R <= 0 || R > 32767 || !d_lut_blob || (pairs && (!d_pair_lut || ((uintptr_t)d_pair_lut & 15)))) return fail(KBBQ_E_ARG, "%s: bad argument", who);
    if (S2 <= 0 || (S2 & 1) || S2 > 65534) return fail(KBBQ_E_ARG, "%s: S2 must be positive and even (%d)", who, S2);
    if (minscore < 0 || minscore > 222) return fail(KBBQ_E_ARG, "%s: minscore out of range", who);
    if (pairs && pitch != pair_pitch(S2)) return fail(KBBQ_E_ARG, "%s: mate-pair rows of %d-base reads have pitch %d, not %d", who, S2 / 2, pair_pitch(S2), pitch);
    // one read per row: the LUT of the columns rows of this pitch can reach (narrowed_row_lut)
    const int Sb = pairs ? S2 : row_lut_width(pitch, S2);
    K2v3Params q = k2v3_params(c, d_seq, d_qual, d_meta, nrows, pitch, pairs, R, KQ, S2, Sb, minscore, d_lut_blob, d_pair_lut, d_seg, d_perm, d_out);
    const size_t rg_bytes = (size_t)(33 + KQ) * q.rb;
    const size_t lds = d_seg ? rg_bytes : rg_bytes * (size_t)R;
    if (lds > (size_t)c->lds_bytes)
        return fail(KBBQ_E_LUT, "%s: the apply LUT (%zu B) does not fit the LDS; group the rows by read group or use kbbq_apply_dev", who, lds);
    if (nrows == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    if (!pairs && !narrowed_row_lut(c, d_lut_blob, R, KQ, S2, Sb, minscore, &q.full)) return fail(KBBQ_E_HIP, "%s: no scratch for the narrowed LUT", who);
    if (!k2_tile_serves(c, pairs, nib, R, d_seg != nullptr, q.cpr, rg_bytes)) return launch_k2v3(c, q, nib, errbit);

    K2tParams t = k2t_params(q);
    const int64_t per_wg = (int64_t)(K2T_THREADS / 64) * 64 * K2T_STEPS;
    int64_t gt = (t.nchunks + per_wg - 1) / per_wg;
    if (d_seg) {
        gt += R;                                     // every group rounds its last workgroup up
        const bool interleave = d_perm && R > 1;
        const int64_t ints = (int64_t)(R + 1) + 1 + (interleave ? 2 * gt : 0);
        if (ints > 0x7FFFFFFF) return fail(KBBQ_E_ARG, "%s: too many workgroups", who);
        rc = grow_scratch(c, c->wgplan, (size_t)ints * sizeof(int));
        if (rc) return rc;
        int* wg_start = reinterpret_cast<int*>(c->wgplan.p);
        K2tPlanParams pl; pl.seg = t.seg; pl.R = R; pl.cpr = q.cpr; pl.wg_start = wg_start;
        hipLaunchKernelGGL(k2t_plan, dim3(1), dim3(64), 0, c->stream, pl);
        t.wg_start = wg_start;
        if (interleave) {
            K2tOrderParams op; op.wg_start = wg_start; op.R = R;
            op.xcd = K2T_XCD;
            op.order = reinterpret_cast<int2*>(wg_start + ((R + 2) & ~1));           // 8-byte aligned behind the starts
            hipLaunchKernelGGL(k2t_order, dim3((unsigned)((gt + 255) / 256)), dim3(256), 0, c->stream, op);
            t.order = op.order;
        }
    }
    // 4-bit mate-pair rows of 19 / 13 chunks: the instance with that geometry compiled in (K1's KJ instances' counterpart)
    const int kj = (pairs && nib) ? k2t_pair_form(t) : 0;
    if (kj < 0) return fail(KBBQ_E_ARG, "%s: mate-pair rows of %d chunks do not have the geometry k2t_apply_pair was compiled for", who, q.cpr);
    if (errbit && kj <= 0) return fail(KBBQ_E_ARG, "%s: no instance of K2 reads KBBQ_ROWS_ERRBIT rows of %d chunks", who, q.cpr);
    const LdsKernel k = kj == 19 ? (errbit ? LK_K2T_PAIR19_EB : LK_K2T_PAIR19) : kj == 13 ? (errbit ? LK_K2T_PAIR13_EB : LK_K2T_PAIR13)
                        : nib ? LK_K2T_NIB : LK_K2T;
    return launch_lds(c, 1, LDS_KERNELS[k], dim3((unsigned)gt), dim3(K2T_THREADS), (size_t)t.lut_bytes, &t);
}

int kbbq_apply_pairs_dev(kbbq_ctx* c, const uint8_t* d_pseq, const uint8_t* d_pqual, const uint32_t* d_pmeta,
                         int64_t npairs, int R, int S2, int minscore, const void* d_lut_blob, const void* d_pair_lut,
                         uint8_t* d_pout)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_pairs("kbbq_apply_pairs_dev", npairs, S2);
    if (rc) return rc;
    return apply_rows(c, "kbbq_apply_pairs_dev", d_pseq, d_pqual, d_pmeta, npairs, pair_pitch(S2), 1, R, S2, minscore,
                      d_lut_blob, d_pair_lut, nullptr, d_pout);
}

int kbbq_apply_grouped_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta,
                           int64_t nrows, int pitch, int pairs, int R, int S2, int minscore, const void* d_lut_blob,
                           const void* d_pair_lut, const int64_t* d_seg, uint8_t* d_out)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (!d_seg) return fail(KBBQ_E_ARG, "kbbq_apply_grouped_dev: d_seg is NULL");
    return apply_rows(c, "kbbq_apply_grouped_dev", d_seq, d_qual, d_meta, nrows, pitch, pairs ? 1 : 0, R, S2, minscore,
                      d_lut_blob, d_pair_lut, d_seg, d_out);
}

// ---- layouts: rows as handed over -> what K1 / K2 run fastest on ------------
int kbbq_accumulate_rows_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                             const uint32_t* d_meta, int64_t nrows, int pitch, int flags, int R, int S2, int S_band,
                             int S_min, int minscore, int dinuc_minscore, const int64_t* d_seg, int64_t* d_tables)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = layout_flags_ok("kbbq_accumulate_rows_dev", flags, true);
    if (rc) return rc;
    const int pairs = (flags & KBBQ_ROWS_PAIRS) ? 1 : 0;
    if (pairs) { rc = check_pairs("kbbq_accumulate_rows_dev", nrows, S2); if (rc) return rc; }
    return accumulate_rows(c, "kbbq_accumulate_rows_dev", d_seq, d_cseq, d_qual, d_meta, nrows, pitch, pairs, R, S2, minscore,
                           dinuc_minscore, d_seg, d_tables, nullptr, pairs ? 0 : S_band, pairs ? 0 : S_min,
                           (flags & KBBQ_ROWS_NIBBLES) ? 1 : 0, (flags & KBBQ_ROWS_TWINS) ? 1 : 0, nullptr, (flags & KBBQ_ROWS_ERRBIT) ? 1 : 0);
}

int kbbq_apply_rows_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta, int64_t nrows,
                        int pitch, int flags, int R, int S2, int minscore, const void* d_lut_blob, const void* d_pair_lut,
                        const int64_t* d_seg, const int64_t* d_perm, uint8_t* d_out)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = layout_flags_ok("kbbq_apply_rows_dev", flags, true);
    if (rc) return rc;
    const int pairs = (flags & KBBQ_ROWS_PAIRS) ? 1 : 0;
    if (pairs) { rc = check_pairs("kbbq_apply_rows_dev", nrows, S2); if (rc) return rc; }
    return apply_rows(c, "kbbq_apply_rows_dev", d_seq, d_qual, d_meta, nrows, pitch, pairs, R, S2, minscore, d_lut_blob,
                      d_pair_lut, d_seg, d_out, (flags & KBBQ_ROWS_NIBBLES) ? 1 : 0, d_perm, (flags & KBBQ_ROWS_ERRBIT) ? 1 : 0);
}

// ---- all length bands of a mixed-length input in ONE launch per kernel -------------------------------------------
static int band_accumulate_alone(kbbq_ctx* c, const kbbq_band& b, int R, int S2, int minscore, int dinuc_minscore, int64_t* d_tables)
{
    if (b.flags || b.d_seg)
        return kbbq_accumulate_rows_dev(c, b.d_seq, b.d_cseq, b.d_qual, b.d_meta, b.nrows, b.pitch, b.flags, R, S2, b.S_band, b.S_min,
                                        minscore, dinuc_minscore, b.d_seg, d_tables);
    return kbbq_accumulate_band_dev(c, b.d_seq, b.d_cseq, b.d_qual, b.d_meta, b.nrows, b.pitch, R, S2, b.S_band, b.S_min, minscore,
                                    dinuc_minscore, d_tables);
}

// workgroups for every band of a merged launch: one each, the rest of `total` by largest remainder of weight / sum(weight),
// never more than a band can use (`cap`)
static void share_workgroups(const std::vector<double>& weight, const std::vector<int64_t>& cap, int total, std::vector<int>& out)
{
    const size_t n = weight.size();
    out.assign(n, 1);
    int left = total - (int)n;
    double sum = 0; for (double w : weight) sum += w;
    for (int round = 0; round < 4 && left > 0 && sum > 0; ++round) {            // a capped band's surplus goes round again
        std::vector<std::pair<double, size_t>> frac;
        int given = 0; double open_sum = 0;
        for (size_t i = 0; i < n; ++i) if (out[i] < cap[i]) open_sum += weight[i];
        if (open_sum <= 0) break;
        const int pool = left;
        for (size_t i = 0; i < n; ++i) {
            if (out[i] >= cap[i]) continue;
            const double want = pool * weight[i] / open_sum;
            int add = (int)std::min<int64_t>((int64_t)want, cap[i] - out[i]);
            out[i] += add; given += add;
            if (out[i] < cap[i]) frac.push_back({want - (int64_t)want, i});
        }
        left -= given;
        std::sort(frac.begin(), frac.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
        for (auto& f : frac) { if (left <= 0) break; if (out[f.second] < cap[f.second]) { ++out[f.second]; --left; } }
    }
}

int kbbq_accumulate_bands_dev(kbbq_ctx* c, const kbbq_band* bands, int nbands, int R, int S2, int minscore, int dinuc_minscore,
                              int64_t* d_tables)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nbands < 0 || (nbands > 0 && !bands)) return fail(KBBQ_E_ARG, "kbbq_accumulate_bands_dev: bad band list");
    // which bands the merged kernel (k1v3_bands) takes: the table-driven K1 fits their LDS geometry, position-major cycle
    // table (not the chunk-position-major form of 2 x 150 bp mate-pair rows), all on 4-bit planes or all on character planes
    std::vector<K1Setup> setups; std::vector<int> merged, alone;
    const bool merge = !env_is("KBBQ_K1_BANDS", "0");                // "0": a launch per band (A/B timing)
    int nib_of_merge = -1;
    for (int i = 0; i < nbands; ++i) {
        const kbbq_band& b = bands[i];
        if (b.nrows == 0) continue;
        int rc = layout_flags_ok("kbbq_accumulate_bands_dev", b.flags, true);      // (an ERRBIT band is a KJ form: it goes alone, never into k1v3_bands)
        if (rc) return rc;
        const int pairs = (b.flags & KBBQ_ROWS_PAIRS) ? 1 : 0, nib = (b.flags & KBBQ_ROWS_NIBBLES) ? 1 : 0;
        K1Setup su; bool fits = false;
        bool can = merge && (int)merged.size() < K1V3_MAX_BANDS;
        if (can) {
            if (pairs) { rc = check_pairs("kbbq_accumulate_bands_dev", b.nrows, S2); if (rc) return rc; }
            rc = accumulate_rows(c, "kbbq_accumulate_bands_dev", b.d_seq, b.d_cseq, b.d_qual, b.d_meta, b.nrows, b.pitch, pairs, R, S2, minscore,
                                 dinuc_minscore, b.d_seg, d_tables, &fits, pairs ? 0 : b.S_band, pairs ? 0 : b.S_min, nib,
                                 (b.flags & KBBQ_ROWS_TWINS) ? 1 : 0, &su, (b.flags & KBBQ_ROWS_ERRBIT) ? 1 : 0);
            if (rc) return rc;
            can = fits && !su.kj && (nib_of_merge < 0 || nib_of_merge == nib);
        }
        if (can) { nib_of_merge = nib; merged.push_back(i); setups.push_back(su); }
        else alone.push_back(i);
    }
    // at least two bands, no more than one 16-wave workgroup per CU and read group gives each of them: ONE launch; anything else goes alone
    const int G = std::max(1, c->cus / std::max(R, 1));
    if (merged.size() < 2 || (int)merged.size() > G) { for (int i : merged) alone.push_back(i); merged.clear(); }
    for (int i : alone) {
        int rc = band_accumulate_alone(c, bands[i], R, S2, minscore, dinuc_minscore, d_tables);
        if (rc) return rc;
    }
    HIPCHK(hipSetDevice(c->device));
    if (merged.empty()) return KBBQ_OK;
    // a band's share of the workgroups follows its work: chunks to bin plus a per-row term (a 64-row block pays the sidecar
    // -> row address -> first chunk latency whatever its width: narrow rows run at half the rate of wide ones) ...
    constexpr double row_cost = 1.25;
    // ... and a chunk of a WIDE row costs more than a chunk of a narrow one (larger tables to zero and flush, 8 instead of 16 copies
    // of the context table, more cycle columns for the same lanes): with equal cost per chunk the widest band of BASELINE config 5
    // ended 25 % after the narrowest (KBBQ_K1_BANDS_DBG=1 prints every band's workgroup end times): + 1 % per chunk of row width
    constexpr double slope = 0.01;
    constexpr double dn8_cost = 1.06;                     // a band on 8 copies of the context table: twice the same-address atomics there
    K1BandsParams t;
    memset(&t, 0, sizeof t);
    t.nbands = (int)merged.size();
    std::vector<double> weight; std::vector<int64_t> cap; std::vector<int> share;
    size_t lds = 0;
    for (const K1Setup& su : setups) {
        weight.push_back((double)su.q.nreads * (su.q.cpr + row_cost) * (1.0 + slope * su.q.cpr) * (su.dn == K1V3_DNREP ? 1.0 : dn8_cost));
        cap.push_back(std::max<int64_t>(1, k1_iters(su.q)));
        lds = std::max(lds, su.lds);
    }
    share_workgroups(weight, cap, G, share);
    int run = 0;
    for (size_t j = 0; j < setups.size(); ++j) {
        t.wg_start[j] = run; run += share[j];
        t.dn[j] = setups[j].dn; t.band[j] = setups[j].q;
    }
    t.wg_start[setups.size()] = run;
    unsigned long long* dbg = nullptr;                    // KBBQ_K1_BANDS_DBG=1: when did every band's workgroups start and end?
    if (getenv("KBBQ_K1_BANDS_DBG")) { HIPCHK(hipMalloc((void**)&dbg, sizeof(unsigned long long) * 2 * (size_t)run)); t.dbg = dbg; }
    int rc = launch_lds(c, 0, k1_kernel(K1_BANDS, k1_split(setups[0].q), 0, nib_of_merge, 0), dim3((unsigned)run, (unsigned)R, 1),
                        dim3(K1V3_THREADS), lds, &t);
    if (rc) return rc;
    if (dbg) {
        std::vector<unsigned long long> h(2 * (size_t)run);
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(h.data(), dbg, h.size() * sizeof h[0], hipMemcpyDeviceToHost));
        (void)hipFree(dbg);
        unsigned long long t0 = ~0ull;
        for (int w = 0; w < run; ++w) t0 = std::min(t0, h[(size_t)w]);
        for (int j = 0; j < t.nbands; ++j) {
            unsigned long long s1 = 0, e0 = ~0ull, e1 = 0;
            for (int w = t.wg_start[j]; w < t.wg_start[j + 1]; ++w) {
                s1 = std::max(s1, h[(size_t)w] - t0); e0 = std::min(e0, h[(size_t)run + w] - t0); e1 = std::max(e1, h[(size_t)run + w] - t0);
            }
            fprintf(stderr, "[k1v3_bands] band %d pitch %3d rows %9lld: %3d workgroups, last start %7.1f us, ends %7.1f .. %7.1f us\n", j, t.band[j].pitch,
                    (long long)t.band[j].nreads, t.wg_start[j + 1] - t.wg_start[j], s1 / 100.0, e0 / 100.0, e1 / 100.0);
        }
    }
    return KBBQ_OK;
}

static int band_apply_alone(kbbq_ctx* c, const kbbq_band& b, int R, int S2, int minscore, const void* d_lut_blob)
{
    if (b.flags || b.d_seg)
        return kbbq_apply_rows_dev(c, b.d_seq, b.d_qual, b.d_meta, b.nrows, b.pitch, b.flags, R, S2, minscore, d_lut_blob, b.d_pair_lut,
                                   b.d_seg, b.d_perm, b.d_out);
    return kbbq_apply_dev(c, b.d_seq, b.d_qual, b.d_meta, b.nrows, b.pitch, R, KQ, S2, minscore, d_lut_blob, KBBQ_APPLY_FAST, b.d_out);
}

int kbbq_apply_bands_dev(kbbq_ctx* c, const kbbq_band* bands, int nbands, int R, int S2, int minscore, const void* d_lut_blob)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nbands < 0 || (nbands > 0 && !bands) || !d_lut_blob) return fail(KBBQ_E_ARG, "kbbq_apply_bands_dev: bad argument");
    if (R <= 0 || R > 32767 || S2 <= 0 || (S2 & 1) || S2 > 65534 || minscore < 0 || minscore > 222) return fail(KBBQ_E_ARG, "kbbq_apply_bands_dev: bad shape");
    // the merged kernel (k2t_bands) takes what the short-lived kernel takes (k2_tile_serves) of one-read-per-row 4-bit planes
    // with one read group; the rest goes band by band.
    // Unlike apply_rows, the LUT's cycle width is min(pitch, S2) whatever KBBQ_K2_ROWLUT says, only R == 1 merges (not rows
    // grouped by read group), and pointers and alignment are tested here: a band that fails them goes alone and is reported there.
    std::vector<int> merged, alone;
    for (int i = 0; i < nbands; ++i) {
        const kbbq_band& b = bands[i];
        if (b.nrows == 0) continue;
        int rc = layout_flags_ok("kbbq_apply_bands_dev", b.flags, true);           // (k2t_bands takes b.flags == KBBQ_ROWS_NIBBLES alone)
        if (rc) return rc;
        const int Sb = std::min(b.pitch, S2);
        const bool can = (int)merged.size() < K2T_MAX_BANDS && R == 1
                         && b.flags == KBBQ_ROWS_NIBBLES && !b.d_seg && !b.d_perm && b.pitch > 0 && !(b.pitch & 15)
                         && k2_tile_serves(c, 0, 1, R, false, b.pitch / 16, (size_t)(33 + KQ) * full_lut_row_bytes(Sb))
                         && !(((uintptr_t)b.d_seq | (uintptr_t)b.d_qual | (uintptr_t)b.d_out) & 15) && b.d_seq && b.d_qual && b.d_meta && b.d_out;
        (can ? merged : alone).push_back(i);
    }
    if (merged.size() < 2) { for (int i : merged) alone.push_back(i); merged.clear(); }
    for (int i : alone) {
        int rc = band_apply_alone(c, bands[i], R, S2, minscore, d_lut_blob);
        if (rc) return rc;
    }
    if (merged.empty()) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    // every band's LUT, narrowed to the columns rows of its pitch can reach, side by side in the context's scratch
    std::vector<size_t> lut_off; size_t need = 0;
    for (int i : merged) { lut_off.push_back(need); need += ((size_t)R * (33 + KQ) * full_lut_row_bytes(std::min(bands[i].pitch, S2)) + 255) & ~(size_t)255; }
    int rc = grow_scratch(c, c->rowlut, need);
    if (rc) return rc;
    K2tBandsParams t;
    memset(&t, 0, sizeof t);
    t.nbands = (int)merged.size();
    const int64_t per_wg = (int64_t)(K2T_THREADS / 64) * 64 * K2T_STEPS;
    int64_t run = 0; size_t lds = 0;
    for (size_t k = 0; k < merged.size(); ++k) {
        const kbbq_band& b = bands[merged[k]];
        const int Sb = std::min(b.pitch, S2);
        K2v3Params rows = k2v3_params(c, b.d_seq, b.d_qual, b.d_meta, b.nrows, b.pitch, 0, R, KQ, S2, Sb, minscore, d_lut_blob, nullptr, nullptr, nullptr, b.d_out);
        rows.full = fill_row_lut(c, d_lut_blob, R, KQ, S2, Sb, minscore, reinterpret_cast<char*>(c->rowlut.p) + lut_off[k]);
        const K2tParams& q = t.band[k] = k2t_params(rows);
        lds = std::max(lds, (size_t)q.lut_bytes);
        t.wg_start[k] = (int)run;
        run += (q.nchunks + per_wg - 1) / per_wg;
        if (run > 0x7FFFFFFF) return fail(KBBQ_E_ARG, "kbbq_apply_bands_dev: too many workgroups");
    }
    t.wg_start[merged.size()] = (int)run;
    return launch_lds(c, 1, LDS_KERNELS[LK_K2T_BANDS], dim3((unsigned)run), dim3(K2T_THREADS), lds, &t);
}

int kbbq_meta_stats_dev(kbbq_ctx* c, const uint32_t* d_meta, int64_t nreads, int32_t* h_stats8)
{
    if (!c || !h_stats8) return fail(KBBQ_E_ARG, "kbbq_meta_stats_dev: NULL argument");
    if (nreads < 0) return fail(KBBQ_E_ARG, "kbbq_meta_stats_dev: nreads < 0");
    static const int init[K7_NSTATS] = {0x7FFFFFFF, 0, 0, 0, 0, 0, 0, 0};
    memcpy(h_stats8, init, sizeof init);
    if (nreads == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    if (!c->d_stats) HIPCHK(hipMalloc((void**)&c->d_stats, sizeof init));
    HIPCHK(hipMemcpyAsync(c->d_stats, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    MetaStatsParams p; p.meta = d_meta; p.n = nreads; p.stats = c->d_stats;
    const int64_t npairs = (nreads + 1) / 2;
    int gx = (int)std::min<int64_t>((npairs + 255) / 256, (int64_t)c->cus * 8);
    hipLaunchKernelGGL(k7_meta_stats, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_stats8, c->d_stats, sizeof init, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return KBBQ_OK;
}

size_t kbbq_group_rows_work_bytes(int64_t nrows, int R)
{
    const int64_t nblocks = (nrows + K7_SORT_ROWS - 1) / K7_SORT_ROWS;
    return (size_t)std::max<int64_t>(nblocks, 1) * (size_t)std::max(R, 1) * sizeof(u32);
}

int kbbq_group_rows_dev(kbbq_ctx* c, const uint32_t* d_meta, int64_t nrows, int pairs, int R, void* d_work,
                        int64_t* d_perm, int64_t* d_seg)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nrows < 0 || nrows >= (1ll << 32)) return fail(KBBQ_E_ARG, "kbbq_group_rows_dev: nrows out of range");
    if (R <= 0 || R > K7_SORT_MAXR) return fail(KBBQ_E_ARG, "kbbq_group_rows_dev: 1 <= R <= %d (got %d)", K7_SORT_MAXR, R);
    if (!d_meta || !d_work || !d_perm || !d_seg) return fail(KBBQ_E_ARG, "kbbq_group_rows_dev: NULL pointer");
    HIPCHK(hipSetDevice(c->device));
    if (nrows == 0) { HIPCHK(hipMemsetAsync(d_seg, 0, (size_t)(R + 1) * 8, c->stream)); return KBBQ_OK; }
    RgSortParams p;
    p.meta = d_meta; p.nrows = nrows; p.pairs = pairs ? 1 : 0; p.R = R;
    p.nblocks = (nrows + K7_SORT_ROWS - 1) / K7_SORT_ROWS;
    p.hist = reinterpret_cast<u32*>(d_work); p.perm = reinterpret_cast<long long*>(d_perm); p.status = c->d_status;
    hipLaunchKernelGGL(k7_rg_sort<false>, dim3((unsigned)p.nblocks), dim3(K7_SORT_THREADS), 0, c->stream, p);
    RgScanParams s;
    s.hist = p.hist; s.count = p.nblocks * R; s.nblocks = p.nblocks; s.R = R; s.nrows = nrows; s.seg = reinterpret_cast<long long*>(d_seg);
    hipLaunchKernelGGL(k7_rg_scan, dim3(1), dim3(1024), 0, c->stream, s);
    hipLaunchKernelGGL(k7_rg_sort<true>, dim3((unsigned)p.nblocks), dim3(K7_SORT_THREADS), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_lay_out_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual, const uint32_t* d_meta,
                     int64_t nreads, int pitch, int flags, int S2, const int64_t* d_perm,
                     uint8_t* d_lseq, uint8_t* d_lcseq, uint8_t* d_lqual, uint32_t* d_lmeta)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = layout_flags_ok("kbbq_lay_out_dev", flags, true);
    if (rc) return rc;
    const int pairs = (flags & KBBQ_ROWS_PAIRS) ? 1 : 0, nib = (flags & KBBQ_ROWS_NIBBLES) ? 1 : 0, errbit = (flags & KBBQ_ROWS_ERRBIT) ? 1 : 0;
    if (errbit && (!d_cseq || (pair_pitch(S2) != 16 * 19 && pair_pitch(S2) != 16 * 13)))
        return fail(KBBQ_E_ARG, "kbbq_lay_out_dev: KBBQ_ROWS_ERRBIT needs the corrected reads and mate-pair rows of 19 or 13 chunks");
    rc = check_planes("kbbq_lay_out_dev", nreads, pitch, d_seq, d_cseq, d_qual);
    if (rc) return rc;
    if (!d_seq || !d_qual || !d_meta || !d_lseq || !d_lqual || !d_lmeta || (d_cseq && !d_lcseq && !errbit)) return fail(KBBQ_E_ARG, "kbbq_lay_out_dev: NULL pointer");
    if (((uintptr_t)d_lseq | (uintptr_t)d_lcseq | (uintptr_t)d_lqual) & 15) return fail(KBBQ_E_ARG, "kbbq_lay_out_dev: planes must be 16-byte aligned");
    if (pairs) {
        rc = check_pairs("kbbq_lay_out_dev", (nreads + 1) / 2, S2);
        if (rc) return rc;
        if ((nreads & 1) && !(flags & KBBQ_ROWS_TWINS)) return fail(KBBQ_E_ARG, "kbbq_lay_out_dev: mate-pair rows need an even number of reads");
        if (pitch < S2 / 2) return fail(KBBQ_E_ARG, "kbbq_lay_out_dev: pitch %d < read length %d", pitch, S2 / 2);
    }
    if (nreads == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    LayOutParams p;
    p.src[0] = d_seq; p.src[1] = d_cseq; p.src[2] = d_qual; p.dst[0] = d_lseq; p.dst[1] = d_lcseq; p.dst[2] = d_lqual;
    p.meta = d_meta; p.dmeta = d_lmeta; p.perm = reinterpret_cast<const long long*>(d_perm);
    p.nrows = pairs ? (nreads + 1) / 2 : nreads; p.nsrc = nreads; p.pitch = pitch; p.dpitch = pairs ? pair_pitch(S2) : pitch; p.S = pairs ? S2 / 2 : 0;
    p.pairs = pairs; p.nib = nib; p.errbit = errbit; p.status = c->d_status;
    const int rpb7 = (p.dpitch / 16) <= 256 ? 256 / (p.dpitch / 16) : 1;      // destination rows per workgroup iteration
    const int gx = bounded_grid((p.nrows + rpb7 - 1) / rpb7, c, 256);
    p.parts = K7_FRONTS;
    hipLaunchKernelGGL(k7_lay_out, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_tables_add_dev(kbbq_ctx* c, int64_t* d_dst, const int64_t* d_src, size_t n)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (n && (!d_dst || !d_src)) return fail(KBBQ_E_ARG, "kbbq_tables_add_dev: NULL pointer");
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    AddTablesParams p; p.dst = (long long*)d_dst; p.src = (const long long*)d_src; p.n = (long long)n;
    int gx = (int)std::min<size_t>((n + 255) / 256, (size_t)c->cus * 8);
    hipLaunchKernelGGL(k7_add_tables, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_unpack_nibbles_dev(kbbq_ctx* c, const uint8_t* d_nib, int64_t nbases, uint8_t* d_chars)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nbases < 0 || (nbases & 15) || ((uintptr_t)d_nib & 7) || ((uintptr_t)d_chars & 15)) return fail(KBBQ_E_ARG, "kbbq_unpack_nibbles_dev: bad size or alignment");
    if (nbases == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    UnNibParams p; p.src = d_nib; p.dst = d_chars; p.nchunks = nbases / 16;
    int gx = (int)std::min<int64_t>((p.nchunks + 255) / 256, (int64_t)c->cus * 16);
    hipLaunchKernelGGL(k7_unpack_nibbles, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_accumulate(kbbq_ctx* c, const uint8_t* seq, const uint8_t* cseq, const uint8_t* qual,
                    const uint32_t* meta, int64_t nreads, int pitch, int R, int S2, int minscore,
                    int64_t* pos_errs, int64_t* pos_total, int64_t* dinuc_errs, int64_t* dinuc_total)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nreads < 0 || pitch <= 0 || (pitch & 15)) return fail(KBBQ_E_ARG, "kbbq_accumulate: bad nreads/pitch");
    if (nreads > 0 && (!seq || !cseq || !qual || !meta)) return fail(KBBQ_E_ARG, "kbbq_accumulate: NULL plane");
    if (R <= 0 || S2 <= 0 || !pos_errs || !pos_total || !dinuc_errs || !dinuc_total) return fail(KBBQ_E_ARG, "kbbq_accumulate: bad tables");
    HIPCHK(hipSetDevice(c->device));
    const size_t npos = (size_t)R * KQ * S2, ndn = (size_t)R * KQ * KND;
    DevBuf dt;
    HIPCHK(dt.alloc(kbbq_tables_count(R, S2) * 8));
    HIPCHK(hipMemsetAsync(dt.p, 0, kbbq_tables_count(R, S2) * 8, c->stream));
    // K1 gives each of the R read groups its own walk over the rows and never meets a read of any other group: the reference's
    // IndexError for it (recalibrate.py:111-117 index the group axis) is found here, on every slab's sidecars as the slab is staged.
    // A read the kernels flag before it comes first; the read itself comes before anything else about it (the group is indexed first).
    int64_t stray = -1, bad = -1;
    // a slab: seq | cseq | qual | meta; when a read is flagged nothing reaches the caller's tables
    int rc = stage_run(c, "kbbq_accumulate", {seq, cseq, qual}, meta, nullptr, nreads, pitch, [&](uint8_t* d, size_t plane, int64_t m) {
        return kbbq_accumulate_dev(c, d, d + plane, d + 2 * plane, (const uint32_t*)(d + 3 * plane), m, pitch, R, S2, minscore, (int64_t*)dt.p);
    }, &bad, nullptr, [&](const uint32_t* w, int64_t lo, int64_t m) {
        if (stray >= 0 && stray < lo) return;
        for (int64_t i = 0; i < m; ++i) if ((int)((w[i] >> 16) & 0x7FFFu) >= R) { if (stray < 0 || lo + i < stray) stray = lo + i; return; }
    });
    if (rc && (stray < 0 || bad < 0 || bad < stray)) return rc;
    if (stray >= 0) return fail(KBBQ_E_INDEX, "read %lld: quality/read-group/cycle beyond the tables (reference: IndexError)", (long long)stray);
    std::vector<int64_t> h(kbbq_tables_count(R, S2));
    HIPCHK(hipMemcpyAsync(h.data(), dt.p, h.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < npos; ++i) { pos_errs[i] += h[i]; pos_total[i] += h[npos + i]; }
    for (size_t i = 0; i < ndn; ++i) { dinuc_errs[i] += h[2 * npos + i]; dinuc_total[i] += h[2 * npos + ndn + i]; }
    return KBBQ_OK;
}

int kbbq_apply(kbbq_ctx* c, const uint8_t* seq, const uint8_t* qual, const uint32_t* meta,
               int64_t nreads, int pitch, int R, int Qt, int S2, int D, int minscore,
               const int64_t* meanq, const int64_t* rgdq, const int64_t* qdq,
               const int64_t* posdq, const int64_t* dinucdq, uint8_t* qual_out)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nreads < 0 || pitch <= 0 || (pitch & 15)) return fail(KBBQ_E_ARG, "kbbq_apply: bad nreads/pitch");
    if (nreads > 0 && (!seq || !qual || !meta || !qual_out)) return fail(KBBQ_E_ARG, "kbbq_apply: NULL plane");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> lut((kbbq_lut_bytes(R, Qt, S2) + 7) / 8);      // 8-byte words: aligned storage
    int flags = 0;
    int rc = kbbq_build_lut(R, Qt, S2, D, minscore, meanq, rgdq, qdq, posdq, dinucdq, lut.data(), &flags);
    if (rc) return rc;
    DevBuf dl;
    HIPCHK(dl.alloc(lut.size() * 8));
    HIPCHK(hipMemcpyAsync(dl.p, lut.data(), lut.size() * 8, hipMemcpyHostToDevice, c->stream));
    int mode = flags ? KBBQ_APPLY_CHECKED : KBBQ_APPLY_FAST;
    // a slab: seq | qual | out | meta (the output plane travels back from the same device slab).  Rows the fast kernel of one read
    // group only reports (kbbq_apply_dev) run again in checked mode: the caller sees their output or the reference's error, never KBBQ_E_LUT
    return stage_run(c, "kbbq_apply", {seq, qual}, meta, qual_out, nreads, pitch, [&](uint8_t* d, size_t plane, int64_t m) {
        return kbbq_apply_dev(c, d, d + plane, (const uint32_t*)(d + 3 * plane), m, pitch, R, Qt, S2, minscore, dl.p, mode, d + 2 * plane);
    }, nullptr, [&]() { const bool was_fast = mode == KBBQ_APPLY_FAST; mode = KBBQ_APPLY_CHECKED; return was_fast; });
}

} // extern "C"
