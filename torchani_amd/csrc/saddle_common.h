// Device helpers shared by the saddle search (saddle.hip) and the reaction-path follower (irc.hip): both keep one workgroup
// of 256 threads per molecule, the rigid motions of a molecule as six vectors of n = 3A doubles in LDS, the projection as a
// rank-12 correction streamed over [C][n][n] in blocks of 16 rows, and the Bofill update of the Cartesian model Hessian.
#pragma once
#include "anihip_common.h"

namespace anihip {

constexpr int SD_THREADS = 256;
constexpr int SD_WAVES = SD_THREADS / WAVE;
constexpr int SD_ROWS = 16;                       // rows per workgroup of the streaming passes
constexpr int SD_MAX_N = ANIHIP_SADDLE_MAX_COORDS;
constexpr int SD_PER_LANE = SD_MAX_N / WAVE;      // coordinates per lane of wave 0
constexpr int SD_Q = 6;
constexpr double SD_RANK_TOL = 1e-8;
static_assert(SD_MAX_N % WAVE == 0, "whole lanes");

static inline size_t sd_align(size_t b) { return (b + 255) & ~(size_t)255; }

__device__ __forceinline__ double sd_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ double sd_wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

__device__ __forceinline__ double sd_wave_min(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
    return v;
}

// Wave 0: classical Gram-Schmidt, twice, of the six vectors in LDS against the vectors kept so far (a dropped one is zero and
// takes nothing away).  Lane owns coordinates d = lane + 64 m and never looks at another lane's: no barrier.
__device__ __forceinline__ void sd_gram_schmidt(double (*s_q)[SD_MAX_N], int lane)
{
    for (int j = 0; j < SD_Q; ++j) {
        double len2 = 0.0;
#pragma unroll
        for (int m = 0; m < SD_PER_LANE; ++m) len2 = fma(s_q[j][lane + WAVE * m], s_q[j][lane + WAVE * m], len2);
        len2 = sd_wave_sum(len2);
        for (int pass = 0; pass < 2; ++pass) {
            double dot[SD_Q];
            for (int l = 0; l < j; ++l) {
                double acc = 0.0;
#pragma unroll
                for (int m = 0; m < SD_PER_LANE; ++m) acc = fma(s_q[l][lane + WAVE * m], s_q[j][lane + WAVE * m], acc);
                dot[l] = sd_wave_sum(acc);
            }
            for (int l = 0; l < j; ++l) {
#pragma unroll
                for (int m = 0; m < SD_PER_LANE; ++m) s_q[j][lane + WAVE * m] -= dot[l] * s_q[l][lane + WAVE * m];
            }
        }
        double rem2 = 0.0;
#pragma unroll
        for (int m = 0; m < SD_PER_LANE; ++m) rem2 = fma(s_q[j][lane + WAVE * m], s_q[j][lane + WAVE * m], rem2);
        rem2 = sd_wave_sum(rem2);
        const bool keep = rem2 > SD_RANK_TOL * SD_RANK_TOL * len2;
        const double sc = keep ? 1.0 / sqrt(rem2) : 0.0;
#pragma unroll
        for (int m = 0; m < SD_PER_LANE; ++m) s_q[j][lane + WAVE * m] *= sc;
    }
}

// Wave 0: gp = g - Q Q^T g with g in the registers of the lanes, and Q copied to gq [6][n]
__device__ __forceinline__ void sd_project_gradient(double (*s_q)[SD_MAX_N], const double (&g)[SD_PER_LANE], int lane, int64_t n,
                                                    double *gp, double *gq)
{
    double dot[SD_Q];
    for (int l = 0; l < SD_Q; ++l) {
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < SD_PER_LANE; ++m) acc = fma(s_q[l][lane + WAVE * m], g[m], acc);
        dot[l] = sd_wave_sum(acc);
    }
#pragma unroll
    for (int m = 0; m < SD_PER_LANE; ++m) {
        const int64_t d = lane + WAVE * m;
        if (d >= n) continue;
        double v = g[m];
        for (int l = 0; l < SD_Q; ++l) v -= dot[l] * s_q[l][d];
        gp[d] = v;
        for (int l = 0; l < SD_Q; ++l) gq[l * n + d] = s_q[l][d];
    }
}

// The whole workgroup, gb [6][n] = W = D H Q on entry (written by this workgroup before a barrier): M = Q^T W with one wave per
// element, then B = W - Q (M + M^T) / 4 - mu Q / 2 into gb, so that P H P + mu Q Q^T = D H D - Q B^T - B Q^T
__device__ __forceinline__ void sd_rank12_correction(double (*s_q)[SD_MAX_N], double (*s_m)[SD_Q], double *gb, double mu, int64_t n,
                                                     int tid, int lane, int wave)
{
    for (int p = wave; p < SD_Q * SD_Q; p += SD_WAVES) {
        const int l = p / SD_Q, m = p % SD_Q;
        double acc = 0.0;
        for (int64_t k = lane; k < n; k += WAVE) acc = fma(s_q[l][k], gb[m * n + k], acc);
        acc = sd_wave_sum(acc);
        if (lane == 0) s_m[l][m] = acc;
    }
    __syncthreads();
    for (int64_t d = tid; d < n; d += SD_THREADS) {
        double w[SD_Q];
#pragma unroll
        for (int l = 0; l < SD_Q; ++l) w[l] = gb[l * n + d];
#pragma unroll
        for (int l = 0; l < SD_Q; ++l) {
            double v = w[l] - 0.5 * mu * s_q[l][d];
#pragma unroll
            for (int m = 0; m < SD_Q; ++m) v -= 0.25 * (s_m[m][l] + s_m[l][m]) * s_q[m][d];
            gb[l * n + d] = v;
        }
    }
}

// Rows 16 rb .. 16 rb + 15 of out = D H' D + mu (I - D) - Q B^T - B Q^T, one wave per row; H'_ik = H_ik (scale == nullptr) or
// scale_i H_ik scale_k
__device__ __forceinline__ void sd_project_rows(const uint8_t *kind, const double *gq, const double *gb, double mu, const double *H,
                                                const double *scale, double *out, int64_t n, int64_t rb, int lane, int wave)
{
    for (int r = wave; r < SD_ROWS; r += SD_WAVES) {
        const int64_t i = rb * SD_ROWS + r;
        if (i >= n) break;
        const bool ai = kind[i / 3] == 1;
        double qi[SD_Q], bi[SD_Q];
#pragma unroll
        for (int l = 0; l < SD_Q; ++l) qi[l] = gq[l * n + i], bi[l] = gb[l * n + i];
        for (int64_t k = lane; k < n; k += WAVE) {
            const bool ak = kind[k / 3] == 1;
            double v = ai && ak ? (scale ? scale[i] * H[i * n + k] * scale[k] : H[i * n + k]) : 0.0;
            if (i == k && !ai) v = mu;
#pragma unroll
            for (int l = 0; l < SD_Q; ++l) v -= qi[l] * gb[l * n + k] + bi[l] * gq[l * n + k];
            out[i * n + k] = v;
        }
    }
}

// The whole workgroup: xi = D (y - H s) with one wave per row, y = f - f_new, s in s_s (LDS, zero beyond n), then wave 0 the
// three scalars of the Bofill update into c[0 .. 2] and whether it applies into c[3]; xi goes to gxi [n].  Ends with a barrier.
__device__ __forceinline__ void sd_bofill_scalars(const uint8_t *kind, const double *H, const float *f, const float *fn,
                                                  const double *s_s, double *s_xi, double *gxi, double *c, int64_t n, int tid,
                                                  int lane, int wave)
{
    for (int64_t i = wave; i < n; i += SD_WAVES) {
        if (kind[i / 3] != 1) continue;   // (wave-uniform)
        double acc = 0.0;
        for (int64_t k = lane; k < n; k += WAVE) acc = fma(H[i * n + k], s_s[k], acc);
        acc = sd_wave_sum(acc);
        if (lane == 0) s_xi[i] = ((double)f[i] - (double)fn[i]) - acc;   // y = g' - g = f - f'
    }
    __syncthreads();
    if (wave == 0) {
        double xs = 0.0, xx = 0.0, ss = 0.0;
#pragma unroll
        for (int m = 0; m < SD_PER_LANE; ++m) {
            const double s = s_s[lane + WAVE * m], xi = s_xi[lane + WAVE * m];
            xs = fma(xi, s, xs), xx = fma(xi, xi, xx), ss = fma(s, s, ss);
        }
        xs = sd_wave_sum(xs), xx = sd_wave_sum(xx), ss = sd_wave_sum(ss);
        if (lane == 0) {
            const bool upd = xx > 0.0 && ss > 0.0 && isfinite(xx) && isfinite(ss);
            double c1 = 0.0, c2 = 0.0, c3 = 0.0;
            if (upd) {
                const double phi = xs == 0.0 ? 0.0 : xs * xs / (xx * ss);
                c1 = xs == 0.0 ? 0.0 : phi / xs;
                c2 = (1.0 - phi) / ss;
                c3 = (1.0 - phi) * xs / (ss * ss);
            }
            c[0] = c1, c[1] = c2, c[2] = c3, c[3] = upd ? 1.0 : 0.0;
        }
    }
    for (int64_t d = tid; d < n; d += SD_THREADS) gxi[d] = s_xi[d];
    __syncthreads();   // (the old forces were read above)
}

// Rows 16 rb .. 16 rb + 15 of the rank-two update H += c1 xi xi^T + c2 (xi s^T + s xi^T) - c3 s s^T, one wave per row
__device__ __forceinline__ void sd_bofill_rows(double *H, const double *s, const double *xi, double c1, double c2, double c3,
                                               int64_t n, int64_t rb, int lane, int wave)
{
#pragma clang fp contract(off)
    for (int r = wave; r < SD_ROWS; r += SD_WAVES) {
        const int64_t i = rb * SD_ROWS + r;
        if (i >= n) break;
        const double si = s[i], xii = xi[i];
        for (int64_t k = lane; k < n; k += WAVE) {
            const double sk = s[k], xik = xi[k];
            // each term is symmetric in i and k bit for bit: contraction is off here, since a fused multiply-add would round
            // xi_i s_k + s_i xi_k differently from xi_k s_i + s_k xi_i
            const double up = (c1 * (xii * xik) + c2 * (xii * sk + si * xik)) - c3 * (si * sk);
            H[i * n + k] = H[i * n + k] + up;
        }
    }
}

}  // namespace anihip
