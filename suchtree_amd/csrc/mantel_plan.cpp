// mantel_plan.cpp -- see mantel_plan.h.  Argument checks, the invariant sums and the restatement of the device sums: no
// GPU calls.
#include "mantel_plan.h"

#include <algorithm>
#include <cmath>

namespace st {

static void mantel_put(i128 v, uint64_t &lo, int64_t &hi)
{
    lo = (uint64_t)v;
    hi = (int64_t)(v >> 64);
}

int mantel_plan(const int32_t *x_sq, const int32_t *y, const int32_t *z, int32_t n, int64_t permutations, int32_t stream, int64_t chunk_tasks,
                st_mantel_moments *moments, const st_mantel_sums *out, MantelPlan &P, std::string &err)
{
    if (const int rc = matrix_call_args(n, permutations, chunk_tasks, stream, err); rc != ST_OK) return rc;
    if (!x_sq || !y) return fail(ST_ERR_ARG, err, "x_sq or y is NULL");
    if (!moments || !out) return fail(ST_ERR_ARG, err, "moments or out is NULL");
    if (const int rc = symmetric_arg("x_sq", x_sq, n, err); rc != ST_OK) return rc;
    P = MantelPlan{};
    P.n = n;
    P.rows = permutations + 1;
    P.partial = z != nullptr;
    P.wave = n <= kMantelWaveMax;
    P.items = P.wave ? 1 : ((int64_t)n + 1) / 2;

    i128 sx = 0, sy = 0, sz = 0, sxx = 0, syy = 0, szz = 0, syz = 0;
    for (int64_t i = 1; i < n; i++) {      // (a row's sums in 64 bits: at most 2^14 terms of 2^31, and of 2^62 as unsigned halves)
        const int32_t *xr = x_sq + i * n, *yr = y + i * (i - 1) / 2, *zr = z ? z + i * (i - 1) / 2 : nullptr;
        int64_t rx = 0, ry = 0, rz = 0;
        uint64_t xx_lo = 0, xx_hi = 0, yy_lo = 0, yy_hi = 0;
        for (int64_t j = 0; j < i; j++) {
            const int64_t xv = xr[j], yv = yr[j];
            const uint64_t xx = (uint64_t)(xv * xv), yy = (uint64_t)(yv * yv);
            rx += xv;
            ry += yv;
            xx_lo += xx & 0xFFFFFFFFu;
            xx_hi += xx >> 32;
            yy_lo += yy & 0xFFFFFFFFu;
            yy_hi += yy >> 32;
        }
        sx += rx;
        sy += ry;
        sxx += ((i128)xx_hi << 32) + xx_lo;
        syy += ((i128)yy_hi << 32) + yy_lo;
        for (int64_t j = 0; zr && j < i; j++) {
            const int64_t yv = yr[j], zv = zr[j];
            rz += zv;
            szz += zv * zv;
            syz += yv * zv;
        }
        sz += rz;
    }
    *moments = st_mantel_moments{};
    mantel_put(sx, moments->sx_lo, moments->sx_hi);
    mantel_put(sy, moments->sy_lo, moments->sy_hi);
    mantel_put(sz, moments->sz_lo, moments->sz_hi);
    mantel_put(sxx, moments->sxx_lo, moments->sxx_hi);
    mantel_put(syy, moments->syy_lo, moments->syy_hi);
    mantel_put(szz, moments->szz_lo, moments->szz_hi);
    mantel_put(syz, moments->syz_lo, moments->syz_hi);

    matrix_cut(P, std::min(kDispersionSigmaBytes / (2 * (int64_t)n), kMantelBlockTasks / P.items), chunk_tasks);
    return ST_OK;
}

void mantel_record(const int32_t *x_sq, const int32_t *y, const int32_t *z, int32_t n, const int32_t *sigma, i128 &sxy, i128 &sxz)
{
    sxy = 0;
    sxz = 0;
    int64_t k = 0;
    for (int64_t i = 1; i < n; i++) {
        const int32_t *row = x_sq + (int64_t)sigma[i] * n;
        for (int64_t j = 0; j < i; j++, k++) {
            const int64_t xv = row[sigma[j]];
            sxy += xv * (int64_t)y[k];
            if (z) sxz += xv * (int64_t)z[k];
        }
    }
}

void mantel_host(const int32_t *x_sq, const int32_t *y, const int32_t *z, const MantelPlan &P, uint64_t seed, int32_t stream, st_mantel_sums *out)
{
    std::vector<int32_t> sigma((size_t)P.n);
    for (int64_t p = 0; p < P.rows; p++) {
        perm_host(seed, stream, p, 0, P.n, sigma.data());
        i128 sxy, sxz;
        mantel_record(x_sq, y, z, P.n, sigma.data(), sxy, sxz);
        out[p] = mantel_sums(sxy, sxz);
    }
}

int mantel_quantise(const double *v, int64_t n, int32_t shift, int32_t *out, int32_t *out_shift, std::string &err)
{
    if (n < 0) return fail(ST_ERR_ARG, err, "n < 0");
    if (n > 0 && !v) return fail(ST_ERR_ARG, err, "v is NULL");
    const bool automatic = shift == ST_MANTEL_SHIFT_AUTO;
    if (!automatic && (shift < -kMantelShiftLimit || shift > kMantelShiftLimit))
        return fail(ST_ERR_ARG, err, "shift " + std::to_string(shift) + ": -" + std::to_string(kMantelShiftLimit) + " to " +
                                         std::to_string(kMantelShiftLimit) + ", or ST_MANTEL_SHIFT_AUTO");
    double top = 0.0;
    for (int64_t k = 0; k < n; k++) {
        if (!std::isfinite(v[k])) return fail(ST_ERR_ARG, err, "v[" + std::to_string(k) + "] is not finite");
        top = std::max(top, std::fabs(v[k]));
    }
    int s = shift;
    if (automatic) {
        s = top == 0.0 ? 0 : 30 - std::ilogb(top);
        if (std::llrint(std::ldexp(top, s)) >= ((int64_t)1 << 31)) s--;      // (a top that rounds up to 2^31 lands on 2^30 instead)
    }
    if (std::fabs(std::ldexp(top, s)) >= 2147483647.5)
        return fail(ST_ERR_ARG, err, "shift " + std::to_string(s) + " puts the largest value, " + std::to_string(top) + ", at 2^31 or more");
    for (int64_t k = 0; k < n; k++)
        if (out) out[k] = (int32_t)std::llrint(std::ldexp(v[k], s));
    if (out_shift) *out_shift = s;
    return ST_OK;
}

}  // namespace st
