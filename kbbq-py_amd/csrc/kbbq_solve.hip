// kbbq_solve.hip -- libkbbq_hip.so: K3, the model solve on the device and the LUT blob it leaves for K2 (C ABI: include/kbbq_hip.h;
// shared: kbbq_lib.h).
#include "kbbq_solve_kernels.h"
#include "kbbq_lut_kernels.h"
#include "kbbq_lib.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>

extern "C" {

// ---- K3: model solve ------------------------------------------------------
static int load_consts(SolveConsts& c, const double* h_consts)
{
    if (!h_consts) return fail(KBBQ_E_ARG, "model constants are NULL");
    memcpy(c.prior, h_consts, sizeof c.prior);
    memcpy(c.logp, h_consts + KSOLVE_NQ, sizeof c.logp);
    memcpy(c.log1mp, h_consts + 2 * KSOLVE_NQ, sizeof c.log1mp);
    return KBBQ_OK;
}

int kbbq_delta_q_dev(kbbq_ctx* c, const int64_t* d_prior_q, const int64_t* d_errs, const int64_t* d_total,
                     const double* d_comb, int64_t ncells, const double* h_consts129, int64_t* d_dq)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (ncells < 0) return fail(KBBQ_E_ARG, "kbbq_delta_q_dev: ncells < 0");
    if (ncells == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    K3CellParams p;
    p.prior_q = (const long long*)d_prior_q; p.errs = (const long long*)d_errs; p.total = (const long long*)d_total;
    p.comb = d_comb; p.n = ncells; p.dq = (long long*)d_dq;
    int rc = load_consts(p.c, h_consts129);
    if (rc) return rc;
    int gx = (int)std::min<int64_t>((ncells + 255) / 256, (int64_t)c->cus * 8);
    hipLaunchKernelGGL(k3_delta_q, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_posterior_q_dev(kbbq_ctx* c, const double* d_prior_q, const int64_t* d_errs, const int64_t* d_total,
                         const double* d_comb, int64_t ncells, const double* h_consts129, int64_t* d_post)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (ncells < 0) return fail(KBBQ_E_ARG, "kbbq_posterior_q_dev: ncells < 0");
    if (ncells == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    K3PostParams p;
    p.prior_q = d_prior_q; p.errs = (const long long*)d_errs; p.total = (const long long*)d_total;
    p.comb = d_comb; p.n = ncells; p.post = (long long*)d_post;
    int rc = load_consts(p.c, h_consts129);
    if (rc) return rc;
    int gx = (int)std::min<int64_t>((ncells + 255) / 256, (int64_t)c->cus * 8);
    hipLaunchKernelGGL(k3_posterior_q, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

size_t kbbq_solve_aux_count(int R, int S2) { return (size_t)R + (size_t)R * KQ + (size_t)R * KQ * S2 + (size_t)R * KQ * KND; }
size_t kbbq_solve_dq_count(int R, int S2) { return (size_t)R + (size_t)R * KQ + (size_t)R * KQ * S2 + (size_t)R * KQ * 17; }

static int launch_solve(kbbq_ctx* c, K3FusedParams& p, int minscore);

int kbbq_solve_dev(kbbq_ctx* c, const int64_t* d_tables, int R, int S2, int minscore, const int32_t* d_meanq,
                   const double* d_aux, const double* h_consts129, int32_t* d_post_q,
                   void* d_lut, int32_t* d_dq)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (R <= 0 || R > 32767 || S2 <= 0 || S2 > 65536) return fail(KBBQ_E_ARG, "kbbq_solve_dev: bad shape R=%d S2=%d", R, S2);
    if (!d_tables || !d_meanq || !d_aux || !d_post_q || !d_lut) return fail(KBBQ_E_ARG, "kbbq_solve_dev: NULL device pointer");
    HIPCHK(hipSetDevice(c->device));
    K3FusedParams p;
    p.tables = (const long long*)d_tables; p.R = R; p.S2 = S2; p.rs = lut_row_stride(S2);
    p.meanq = d_meanq; p.aux = d_aux; p.post_q = d_post_q; p.lut = reinterpret_cast<int16_t*>(d_lut); p.dq = d_dq;
    p.logtab = nullptr; p.meanq_out = nullptr; p.status = c->d_status;
    memset(p.perr, 0, sizeof p.perr);
    int rc = load_consts(p.c, h_consts129);
    if (rc) return rc;
    return launch_solve(c, p, minscore);
}

static int launch_solve(kbbq_ctx* c, K3FusedParams& p, int minscore)
{
    const int R = p.R, S2 = p.S2;
    void* d_lut = p.lut;
    hipLaunchKernelGGL(k3_levels_ab, dim3((unsigned)R), dim3(1024), 0, c->stream, p);
    const int64_t cells = (int64_t)R * KQ * ((int64_t)S2 + KND);              // one wave per cell
    int gx = (int)std::min<int64_t>((cells + 3) / 4, (int64_t)c->cus * 32);
    hipLaunchKernelGGL(k3_level_c, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    // derive the table-driven (int8) LUT and the flags the fast apply kernel relies on
    LutFillParams f;
    f.lut16 = p.lut; f.rs16 = p.rs; f.R = R; f.Qt = KQ; f.S2 = S2; f.minscore = std::min(std::max(minscore, 0), KQ);
    f.full = reinterpret_cast<int8_t*>(d_lut) + lut_full_offset(R, KQ, S2);
    f.compact8 = reinterpret_cast<int8_t*>(d_lut) + lut_compact8_offset(R, KQ, S2);
    f.flags = reinterpret_cast<int*>(reinterpret_cast<char*>(d_lut) + lut_flags_offset(R, KQ, S2));
    f.status = c->d_status;
    HIPCHK(hipMemsetAsync(f.flags, 0, 16, c->stream));
    hipLaunchKernelGGL(k3_fill_full_lut, dim3((unsigned)(R * (33 + KQ))), dim3(256), 0, c->stream, f);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_solve_device_dev(kbbq_ctx* c, const int64_t* d_tables, int R, int S2, int minscore, const double* d_logtab,
                          const double* h_consts172, int32_t* d_post_q, void* d_lut, int32_t* d_dq, int32_t* d_meanq_out)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (R <= 0 || R > 32767 || S2 <= 0 || S2 > 65536) return fail(KBBQ_E_ARG, "kbbq_solve_device_dev: bad shape R=%d S2=%d", R, S2);
    if (!d_tables || !d_logtab || !h_consts172 || !d_post_q || !d_lut) return fail(KBBQ_E_ARG, "kbbq_solve_device_dev: NULL pointer");
    HIPCHK(hipSetDevice(c->device));
    K3FusedParams p;
    p.tables = (const long long*)d_tables; p.R = R; p.S2 = S2; p.rs = lut_row_stride(S2);
    p.meanq = nullptr; p.aux = nullptr; p.post_q = d_post_q; p.lut = reinterpret_cast<int16_t*>(d_lut); p.dq = d_dq;
    p.logtab = d_logtab; p.meanq_out = d_meanq_out; p.status = c->d_status;
    memcpy(p.perr, h_consts172 + 3 * KSOLVE_NQ, sizeof p.perr);
    int rc = load_consts(p.c, h_consts172);
    if (rc) return rc;
    return launch_solve(c, p, minscore);
}

int kbbq_gammaln_dev(kbbq_ctx* c, const double* d_x, int64_t n, const double* d_logtab, double* d_out)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!d_x || !d_out)) || !d_logtab) return fail(KBBQ_E_ARG, "kbbq_gammaln_dev: bad argument");
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    K3GammalnParams p; p.x = d_x; p.n = n; p.logtab = d_logtab; p.out = d_out;
    int gx = (int)std::min<int64_t>((n + 255) / 256, (int64_t)c->cus * 8);
    hipLaunchKernelGGL(k3_gammaln, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

} // extern "C"
