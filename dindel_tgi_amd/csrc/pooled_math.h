// pooled_math.h — the arithmetic of the pooled analysis' EM loop (estimateHaplotypeFrequenciesBayesEM, reference DInDel.cpp:2412-2543),
// defined once for the host (pooled_em_host.cpp) and the device (pooled_em_kernel.hip).
//
// exp, log, digamma and addLogs are written in fp64 + - * /, explicit __builtin_fma and integer operations on the bits of a double, with
// literal coefficients: no libm and no device math library call, so that both sides evaluate the same correctly rounded operations in the
// same order and agree in every bit.  Every unit that includes this file is compiled with -ffp-contract=off: only the fused operations
// written out below are fused.  pm_em_slot_serial() is the loop itself over one slot (one window, one set of active variants) as the host
// runs it; the kernel spreads the reads over the 64 lanes of a wavefront and keeps the same order of every sum.  DESIGN 20 holds the
// definition, the measured errors against exact arithmetic and the two knowing deviations from the reference (the order of the sums over
// reads, and denormal results of exp flushed to zero).
#ifndef DD_POOLED_MATH_H
#define DD_POOLED_MATH_H
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PM_HD __host__ __device__ __forceinline__
#else
#define PM_HD inline
#endif

#define PM_LANES 64            /* read r belongs to partial r mod 64, on both sides */
#define PM_MAX_ITER 25         /* the reference's `iter > 25`: at most 27 iterations */
#define PM_INCOMPATIBLE (-100.0)

PM_HD int64_t pm_bits(double x) { int64_t b; __builtin_memcpy(&b, &x, 8); return b; }
PM_HD double pm_from_bits(int64_t b) { double x; __builtin_memcpy(&x, &b, 8); return x; }
PM_HD double pm_inf() { return pm_from_bits(0x7ff0000000000000LL); }
PM_HD double pm_abs(double x) { return pm_from_bits(pm_bits(x) & 0x7fffffffffffffffLL); }

// exp(x): x = k ln2 + r with |r| <= ln2 / 2 (Cody-Waite, ln2 split so that k * hi is exact), the Taylor polynomial of degree 14 in r
// (remainder below 2^-62), times 2^k through the exponent field.  Results below the normal range are 0.
PM_HD double pm_exp(double x)
{
    if (x != x) return x;
    if (x > 709.782712893384) return pm_inf();
    if (x < -708.3964185322641) return 0.0;
    const double shift = 0x1.8p52;
    const double kd = (x * 0x1.71547652b82fep+0 + shift) - shift;      // round(x / ln2), |kd| <= 1024
    double r = __builtin_fma(-kd, 0x1.62e42fee00000p-1, x);
    r = __builtin_fma(-kd, 0x1.a39ef35793c76p-33, r);
    double p = 0x1.93974a8c07c9dp-37;                                  // 1/14!
    p = __builtin_fma(p, r, 0x1.6124613a86d09p-33);
    p = __builtin_fma(p, r, 0x1.1eed8eff8d898p-29);
    p = __builtin_fma(p, r, 0x1.ae64567f544e4p-26);
    p = __builtin_fma(p, r, 0x1.27e4fb7789f5cp-22);
    p = __builtin_fma(p, r, 0x1.71de3a556c734p-19);
    p = __builtin_fma(p, r, 0x1.a01a01a01a01ap-16);
    p = __builtin_fma(p, r, 0x1.a01a01a01a01ap-13);
    p = __builtin_fma(p, r, 0x1.6c16c16c16c17p-10);
    p = __builtin_fma(p, r, 0x1.1111111111111p-7);
    p = __builtin_fma(p, r, 0x1.5555555555555p-5);
    p = __builtin_fma(p, r, 0x1.5555555555555p-3);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);                                      // in (0.70, 1.42)
    const int64_t b = pm_bits(p), e = ((b >> 52) & 0x7ff) + (int64_t)kd;
    if (e <= 0) return 0.0;
    if (e >= 0x7ff) return pm_inf();
    return pm_from_bits((b & 0x800fffffffffffffLL) | (e << 52));
}

// log(x): x = 2^k m with m in [sqrt(1/2), sqrt 2), s = (m - 1) / (m + 1), log m = 2 atanh s by its odd series through s^23 (the next
// term is below 2^-65 of the sum), plus k ln2 with the same split as pm_exp.
PM_HD double pm_log(double x)
{
    if (x != x || x < 0.0) return pm_from_bits(0x7ff8000000000000LL);
    if (x == 0.0) return -pm_inf();
    if (x == pm_inf()) return x;
    int64_t k = 0;
    if (x < 0x1p-1022) { x = x * 0x1p54; k = -54; }
    int64_t b = pm_bits(x);
    k += ((b >> 52) & 0x7ff) - 1023;
    double m = pm_from_bits((b & 0x000fffffffffffffLL) | 0x3ff0000000000000LL);   // [1, 2)
    if (m > 0x1.6a09e667f3bcdp+0) { m = m * 0.5; k += 1; }
    const double s = (m - 1.0) / (m + 1.0), z = s * s;
    double p = 0x1.642c8590b2164p-4;                                   // 2/23
    p = __builtin_fma(p, z, 0x1.8618618618618p-4);
    p = __builtin_fma(p, z, 0x1.af286bca1af28p-4);
    p = __builtin_fma(p, z, 0x1.e1e1e1e1e1e1ep-4);
    p = __builtin_fma(p, z, 0x1.1111111111111p-3);
    p = __builtin_fma(p, z, 0x1.3b13b13b13b14p-3);
    p = __builtin_fma(p, z, 0x1.745d1745d1746p-3);
    p = __builtin_fma(p, z, 0x1.c71c71c71c71cp-3);
    p = __builtin_fma(p, z, 0x1.2492492492492p-2);
    p = __builtin_fma(p, z, 0x1.999999999999ap-2);
    p = __builtin_fma(p, z, 0x1.5555555555555p-1);                     // 2/3
    const double kd = (double)k;
    const double lo = __builtin_fma(kd, 0x1.a39ef35793c76p-33, s * (z * p));
    return kd * 0x1.62e42fee00000p-1 + (2.0 * s + lo);
}

// digamma(x), x > 0: psi(x) = psi(x + 1) - 1/x up to x >= 10, there ln x - 1/(2x) - sum_n B_2n / (2n x^2n) through n = 8 (the next
// term is below 4e-18 at x = 10).  x <= 0 is not a value the EM has (a0 > 0): NaN.
PM_HD double pm_digamma(double x)
{
    if (!(x > 0.0)) return pm_from_bits(0x7ff8000000000000LL);
    if (x == pm_inf()) return x;
    double acc = 0.0;
    while (x < 10.0) { acc = acc + 1.0 / x; x = x + 1.0; }
    const double ix = 1.0 / x, w = ix * ix;
    double p = -0x1.c5e5e5e5e5e5ep-2;                                  // B16/16
    p = __builtin_fma(p, w, 0x1.5555555555555p-4);                     // B14/14
    p = __builtin_fma(p, w, -0x1.5995995995996p-6);                    // B12/12
    p = __builtin_fma(p, w, 0x1.f07c1f07c1f08p-8);                     // B10/10
    p = __builtin_fma(p, w, -0x1.1111111111111p-8);                    // B8/8
    p = __builtin_fma(p, w, 0x1.0410410410410p-8);                     // B6/6
    p = __builtin_fma(p, w, -0x1.1111111111111p-7);                    // B4/4
    p = __builtin_fma(p, w, 0x1.5555555555555p-4);                     // B2/2
    return ((pm_log(x) - 0.5 * ix) - w * p) - acc;
}

// addLogs (reference Utils.hpp:29-38); addLogs(-HUGE_VAL, x) = x without a detour through exp and log
PM_HD double pm_add_logs(double l1, double l2)
{
    if (l1 == -pm_inf()) return l2;
    if (l1 > l2) { const double diff = l2 - l1; return l1 + pm_log(1.0 + pm_exp(diff)); }
    const double diff = l1 - l2;
    return l2 + pm_log(1.0 + pm_exp(diff));
}

// The serial Lanes of the host: partial sums in arrays of PM_LANES, combined x[i] += x[i + off] for off = 32 ... 1, which is what the
// wavefront's shuffle reduction computes for lane 0.
struct PmSerialSum {
    double x[PM_LANES];
    PM_HD void clear() { for (int i = 0; i < PM_LANES; i++) x[i] = 0.0; }
    PM_HD double total()
    {
        for (int off = PM_LANES / 2; off >= 1; off >>= 1)
            for (int i = 0; i < off; i++) x[i] = x[i] + x[i + off];
        return x[0];
    }
};

// The M-step for one haplotype (reference DInDel.cpp:2468-2477) once ahat's digamma is known.
PM_HD void pm_m_step(bool compatible, double nk, double a0, double dahat, double denom, double &lpi, double &pi)
{
    if (compatible) {
        lpi = pm_digamma(nk + a0) - dahat;
        pi = pm_log((a0 + nk) / denom);
    } else {
        lpi = PM_INCOMPATIBLE;
        pi = PM_INCOMPATIBLE;
    }
}

// The loop of one slot on the host, in the order the kernel keeps: H haplotypes, R reads, rl[h * R + r] (the likelihood kernels' layout),
// compat[h]; work: 2 H doubles (lpi, pi), nk: H sums.  Outputs: loglik, freqs[H], iterations, the last |eOld - eNew|.
inline void pm_em_slot_serial(int H, int R, const double *rl, const uint8_t *compat, double a0, double tol, double *lpi, double *pi, double *nk_tot,
                              PmSerialSum *nk, double *loglik_out, double *freqs, int32_t *iters_out, double *ediff_out)
{
    int numah = 0;
    for (int h = 0; h < H; h++) numah += compat[h] != 0;
    const double lpi0 = numah ? pm_log(1.0 / (double)numah) : 0.0;
    for (int h = 0; h < H; h++) lpi[h] = compat[h] ? lpi0 : PM_INCOMPATIBLE;
    const double denom = (double)numah * a0 + (double)R;
    double eOld = -pm_inf(), loglik = 0.0, ediff = 0.0;
    int iter = 0;
    bool converged = false;
    PmSerialSum S, L;
    while (!converged) {
        for (int h = 0; h < H; h++) nk[h].clear();
        S.clear(); L.clear();
        for (int r = 0; r < R; r++) {
            const int lane = r & (PM_LANES - 1);
            double lognorm = -pm_inf();
            for (int h = 0; h < H; h++) lognorm = pm_add_logs(lognorm, lpi[h] + rl[(int64_t)h * R + r]);
            for (int h = 0; h < H; h++) {
                const double v = rl[(int64_t)h * R + r], z = pm_exp((lpi[h] + v) - lognorm);
                nk[h].x[lane] = nk[h].x[lane] + z;
                S.x[lane] = S.x[lane] + z * v;
            }
            L.x[lane] = L.x[lane] + lognorm;
        }
        loglik = L.total();
        double eNew = S.total(), ahat = 0.0;
        for (int h = 0; h < H; h++) {
            nk_tot[h] = nk[h].total();
            if (compat[h]) ahat = ahat + (nk_tot[h] + a0);
        }
        const double dahat = numah ? pm_digamma(ahat) : 0.0;
        for (int h = 0; h < H; h++) pm_m_step(compat[h] != 0, nk_tot[h], a0, dahat, denom, lpi[h], pi[h]);
        for (int h = 0; h < H; h++) eNew = eNew + pi[h] * nk_tot[h];
        ediff = pm_abs(eOld - eNew);
        converged = ediff < tol || iter > PM_MAX_ITER;
        eOld = eNew;
        iter++;
    }
    double zsum = 0.0;
    for (int h = 0; h < H; h++) zsum = zsum + pm_exp(pi[h]);
    for (int h = 0; h < H; h++) freqs[h] = pm_exp(pi[h]) / zsum;
    *loglik_out = loglik; *iters_out = iter; *ediff_out = ediff;
}
#endif
