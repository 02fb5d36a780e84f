// The multistate Bennett acceptance ratio estimator (MBAR, binless WHAM) on the series that biased and tempered MD records
// (torchani_amd.md.MBAR).  include/anihip.h has the exact definition.
//
//   k_mbar_check          the tables and the samples of a call: status bits by integer atomics, ln N_k to the workspace
//   k_mbar_samples        launch 1 of an iteration: d_n = lse_k(ln N_k + f_k - u_k(x_n)) over the states with N_k > 0.  Two samples
//                         per thread in registers, the state table (ln N_k + f_k, beta_k, restraint rows) staged in LDS in tiles
//                         of at most 32 KB and read by broadcast, one running (max, sum) pair per sample: one exp per pair
//   k_mbar_states         launch 2: a workgroup stages a fixed chunk of samples (d, E, CV columns) in LDS, its four waves deal
//                         the states among them; a wave holds one state's row in registers and walks the chunk twice (the
//                         maximum of -u_k - d_n, then the sum of exp against it), both reduced over the lanes in a fixed order
//   k_mbar_finish         one workgroup: the chunks' (max, sum) pairs combined in chunk order, f'_k = -lse, the shift by f'_0,
//                         delta = max |f' - f|
//   k_mbar_target_*       ln W_n of one target state, normalized over all samples by the same chunked reduction
//   k_mbar_all            ln W_nk = f_k - u_k(x_n) - d_n of every state over a slab of samples
//   k_mbar_hist_*         log-sum-exp of log weights per bin: the bin maxima by integer atomics on an order-preserving key (the
//                         maximum does not depend on the order of arrival), then sums of exp(w - max) per chunk of samples by one
//                         wave each, equal bins within a wave added by a butterfly, the chunks added in chunk order
//
// fp64 throughout, every log-sum-exp against a maximum.  No floating-point atomics and every sum in a fixed order: two calls on
// the same input are bit-identical.  The reduced potential of the structured mode is the restraint of k_md_bias_apply
// (md_bias.hip) on recorded CV values, with cv_wrap of md_cv.h (cv_wrap_by in the two hot kernels: the same expression).  What lives in device memory is checked by k_mbar_check; a call
// that finds the status word set writes nothing.
#include <algorithm>
#include <math.h>

#include "anihip_common.h"
#include "md_cv.h"
#include "md_sums.h"

namespace anihip {

constexpr int MBAR_CVS = ANIHIP_MD_BIAS_MAX_CVS;
constexpr int MBAR_SPT = 2;                               // samples per thread of k_mbar_samples
constexpr int MBAR_TILE_BYTES = 32 * 1024;                // state tile of k_mbar_samples: five workgroups share a CU's 160 KB
constexpr int MBAR_CHUNK_DOUBLES = 6144;                  // sample chunk of k_mbar_states: 48 KB, three workgroups per CU
constexpr int MBAR_MAX_CHUNK = 2048;
constexpr int MBAR_TARGET_CHUNK = 1024;                   // samples per workgroup of k_mbar_target_chunks
constexpr int MBAR_HIST_MAX_CHUNKS = 1024, MBAR_HIST_MIN_CHUNK = 2048;
static_assert(MBAR_CVS == 16, "the dispatch of mbar_launch covers 0 .. 16 columns");

struct MbarArgs {
    anihip_mbar p;
    const double *f;       // [K]
    double *ln_n;          // [K]: ln N_k, -inf where N_k = 0
    double *d;             // [N]
    double *part;          // [n_chunks][K][2]: (max, sum) of a chunk
    int64_t n_first, n_count;
    int32_t chunk, n_chunks, tile;
};

__device__ __forceinline__ uint32_t mbar_dihedral_mask(const anihip_mbar &p)
{
    uint32_t m = 0;
    if (!p.u_kn)
        for (int r = 0; r < p.n_cvs; ++r)
            if (p.cv_kind[r] == ANIHIP_MD_CV_DIHEDRAL) m |= 1u << r;
    return m;
}

// the restraint of k_md_bias_apply on the CV value s: (center, k, half_width) = row[0 .. 2]
__device__ __forceinline__ double mbar_restraint(double s, const double *row, bool dihedral)
{
    double d = s - row[0];
    if (dihedral) d = cv_wrap(d);
    const double e = fmax(0.0, fabs(d) - row[2]);
    return 0.5 * row[1] * e * e;
}

// u = beta (E + sum over the columns in order of the restraint energies), the columns of the sample in registers.  Every one of
// the RMAX columns is evaluated: those past R are padded with zero rows, which add +0.  DIH: some column is a dihedral, and
// period[r] (LDS, 2 pi or 0) wraps by value, so that no column costs a predicate or a branch in the loop over the states.
template <int RMAX, bool DIH>
__device__ __forceinline__ double mbar_u(double beta, const double *rows, double E, const double (&s)[RMAX > 0 ? RMAX : 1],
                                         const double *period)
{
    double bias = 0.0;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        double d = s[r] - rows[3 * r];
        if (DIH) d = cv_wrap_by(d, period[r]);
        const double e = fmax(0.0, fabs(d) - rows[3 * r + 2]);
        bias += 0.5 * rows[3 * r + 1] * e * e;
    }
    return beta * (E + bias);
}

// 2 pi for the dihedral columns, 0 for the others and for the padding (called by the whole workgroup, before a barrier)
__device__ __forceinline__ void mbar_periods(const anihip_mbar &p, double *period)
{
    if (threadIdx.x < MBAR_CVS)
        period[threadIdx.x] = !p.u_kn && (int)threadIdx.x < p.n_cvs && p.cv_kind[threadIdx.x] == ANIHIP_MD_CV_DIHEDRAL ? CV_TWO_PI : 0.0;
}

// the same for one sample read from memory (the kernels that are not in the iteration)
__device__ __forceinline__ double mbar_u_at(const anihip_mbar &p, uint32_t dih, double beta, const double *rows, int64_t n)
{
    double bias = 0.0;
    for (int r = 0; r < p.n_cvs; ++r) bias += mbar_restraint(p.cv[n * p.n_cvs + r], rows + 3 * r, dih >> r & 1u);
    return beta * ((p.energy ? p.energy[n] : 0.0) + bias);
}

// ---- the check ------------------------------------------------------------------------------------------------------------------
struct CheckArgs {
    anihip_mbar p;
    double *ln_n;
    int64_t n_first, n_count;
    const double *t_beta, *t_rows, *t_u;   // an external target, or null
};

__device__ __forceinline__ bool mbar_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // (false for NaN)

__global__ __launch_bounds__(MD_BLOCK) void k_mbar_check(CheckArgs a)
{
    const anihip_mbar &p = a.p;
    const int K = p.n_states, R = p.n_cvs;
    int bad = 0;
    if (blockIdx.x == 0) {   // the tables
        __shared__ int sh_any;
        if (threadIdx.x == 0) sh_any = 0;
        __syncthreads();
        int any = 0;
        for (int k = threadIdx.x; k < K; k += MD_BLOCK) {
            const double n = p.n_k[k];
            if (!mbar_finite(n) || n < 0.0) bad |= ANIHIP_MBAR_BAD_COUNTS;
            if (n > 0.0) any = 1;
            a.ln_n[k] = n > 0.0 ? log(n) : -INFINITY;
            if (!p.u_kn && !mbar_finite(p.beta[k])) bad |= ANIHIP_MBAR_BAD_STATES;
        }
        if (any) atomicOr(&sh_any, 1);   // (on LDS, an integer)
        if (!p.u_kn) {
            for (int64_t w = threadIdx.x; w < (int64_t)K * R; w += MD_BLOCK) {
                const double *row = p.restraint + 3 * w;
                if (!mbar_finite(row[0]) || !mbar_finite(row[1]) || !mbar_finite(row[2]) || row[1] < 0.0 || row[2] < 0.0)
                    bad |= ANIHIP_MBAR_BAD_STATES;
            }
            for (int r = threadIdx.x; r < R; r += MD_BLOCK)
                if (p.cv_kind[r] < ANIHIP_MD_CV_DISTANCE || p.cv_kind[r] > ANIHIP_MD_CV_DIHEDRAL) bad |= ANIHIP_MBAR_BAD_STATES;
            if (a.t_beta && threadIdx.x == 0 && !mbar_finite(a.t_beta[0])) bad |= ANIHIP_MBAR_BAD_STATES;
            if (a.t_rows)
                for (int r = threadIdx.x; r < R; r += MD_BLOCK) {
                    const double *row = a.t_rows + 3 * r;
                    if (!mbar_finite(row[0]) || !mbar_finite(row[1]) || !mbar_finite(row[2]) || row[1] < 0.0 || row[2] < 0.0)
                        bad |= ANIHIP_MBAR_BAD_STATES;
                }
        }
        __syncthreads();
        if (threadIdx.x == 0 && !sh_any) bad |= ANIHIP_MBAR_BAD_COUNTS;
    }
    // the samples first <= n < first + count
    const int64_t stride = (int64_t)gridDim.x * MD_BLOCK, t0 = blockIdx.x * (int64_t)MD_BLOCK + threadIdx.x;
    if (p.u_kn) {
        for (int64_t w = t0; w < K * a.n_count; w += stride)
            if (!mbar_finite(p.u_kn[(w / a.n_count) * p.n_samples + a.n_first + w % a.n_count])) bad |= ANIHIP_MBAR_BAD_SAMPLES;
        if (a.t_u)
            for (int64_t w = t0; w < a.n_count; w += stride)
                if (!mbar_finite(a.t_u[a.n_first + w])) bad |= ANIHIP_MBAR_BAD_SAMPLES;
    } else {
        for (int64_t w = t0; w < R * a.n_count; w += stride)
            if (!mbar_finite(p.cv[a.n_first * R + w])) bad |= ANIHIP_MBAR_BAD_SAMPLES;
        if (p.energy)
            for (int64_t w = t0; w < a.n_count; w += stride)
                if (!mbar_finite(p.energy[a.n_first + w])) bad |= ANIHIP_MBAR_BAD_SAMPLES;
    }
    if (bad) atomicOr(p.status, bad);   // (an integer: the order does not matter)
}

// ---- launch 1: d_n ----------------------------------------------------------------------------------------------------------------
template <int RMAX, bool DENSE, bool DIH>
__device__ __forceinline__ void mbar_samples_body(const MbarArgs &a)
{
    extern __shared__ double mbar_tile[];   // [tile][W]: ln N_k + f_k, beta_k, the RMAX rows of state k (zeros past R)
    __shared__ double period[MBAR_CVS];
    const anihip_mbar &p = a.p;
    if (*p.status) return;   // (the same for every thread)
    constexpr int RA = RMAX > 0 ? RMAX : 1, W = DENSE ? 1 : 2 + 3 * RMAX;
    const int R = DENSE ? 0 : p.n_cvs, K = p.n_states;
    mbar_periods(p, period);   // (the barrier of the first tile stands before its first use)
    const int64_t end = a.n_first + a.n_count, base = a.n_first + blockIdx.x * (int64_t)(MD_BLOCK * MBAR_SPT) + threadIdx.x;
    int64_t n[MBAR_SPT];
    double E[MBAR_SPT], s[MBAR_SPT][RA], m[MBAR_SPT], acc[MBAR_SPT];
#pragma unroll
    for (int j = 0; j < MBAR_SPT; ++j) {
        n[j] = min(base + j * MD_BLOCK, end - 1);   // (a thread past the end repeats the last sample and stores nothing)
        E[j] = !DENSE && p.energy ? p.energy[n[j]] : 0.0;
#pragma unroll
        for (int r = 0; r < RA; ++r) s[j][r] = r < R ? p.cv[n[j] * R + r] : 0.0;
        m[j] = -INFINITY, acc[j] = 0.0;
    }
    for (int k0 = 0; k0 < K; k0 += a.tile) {
        const int nt = min(a.tile, K - k0);
        __syncthreads();   // (the tile before is read until here)
        for (int w = threadIdx.x; w < nt * W; w += MD_BLOCK) {
            const int k = k0 + w / W, q = w % W;
            mbar_tile[w] = q == 0 ? a.ln_n[k] + a.f[k] : q == 1 ? p.beta[k] : q - 2 < 3 * R ? p.restraint[(int64_t)k * 3 * R + (q - 2)] : 0.0;
        }
        __syncthreads();
        for (int t = 0; t < nt; ++t) {
            const double *st = mbar_tile + t * W;
            const double a0 = st[0];
            if (a0 == -INFINITY) continue;   // N_k = 0 (the same for every thread)
#pragma unroll
            for (int j = 0; j < MBAR_SPT; ++j) {
                const double u = DENSE ? p.u_kn[(int64_t)(k0 + t) * p.n_samples + n[j]] : mbar_u<RMAX, DIH>(st[1], st + 2, E[j], s[j], period);
                const double v = a0 - u, e = exp(-fabs(v - m[j]));
                acc[j] = v > m[j] ? acc[j] * e + 1.0 : acc[j] + e;
                m[j] = fmax(m[j], v);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MBAR_SPT; ++j)
        if (base + j * MD_BLOCK < end) a.d[n[j]] = m[j] + log(acc[j]);
}

// (the kind of the columns lives in device memory: the kernel picks the body, the same in every thread)
template <int RMAX, bool DENSE>
__global__ __launch_bounds__(MD_BLOCK) void k_mbar_samples(MbarArgs a)
{
    if (!DENSE && RMAX > 0 && mbar_dihedral_mask(a.p))
        mbar_samples_body<RMAX, DENSE, RMAX != 0>(a);
    else
        mbar_samples_body<RMAX, DENSE, false>(a);
}

// ---- launch 2: (max, sum) of -u_k - d_n per (chunk, state) ---------------------------------------------------------------------------
__device__ __forceinline__ double wave_max64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

__device__ __forceinline__ double wave_sum64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <int RMAX, bool DENSE, bool DIH>
__device__ __forceinline__ void mbar_states_body(const MbarArgs &a)
{
    extern __shared__ double mbar_chunk[];   // d [S], E [S], cv [RMAX][S] (zeros past R)
    __shared__ double period[MBAR_CVS];
    const anihip_mbar &p = a.p;
    if (*p.status) return;
    constexpr int RA = RMAX > 0 ? RMAX : 1;
    const int R = DENSE ? 0 : p.n_cvs, K = p.n_states, S = a.chunk;
    mbar_periods(p, period);
    const int64_t n0 = (int64_t)blockIdx.x * S;
    const int cnt = (int)min((int64_t)S, p.n_samples - n0);
    double *sh_d = mbar_chunk, *sh_E = sh_d + S, *sh_cv = sh_E + S;
    for (int i = threadIdx.x; i < cnt; i += MD_BLOCK) {
        sh_d[i] = a.d[n0 + i];
        if (!DENSE) {
            sh_E[i] = p.energy ? p.energy[n0 + i] : 0.0;
            for (int r = 0; r < RMAX; ++r) sh_cv[r * S + i] = r < R ? p.cv[(n0 + i) * R + r] : 0.0;
        }
    }
    __syncthreads();
    const int wave = uniform(threadIdx.x / WAVE), lane = lane_id();
    for (int k = wave; k < K; k += MD_BLOCK / WAVE) {
        double beta = 0.0, rows[3 * RA];
        if (!DENSE) {
            beta = p.beta[k];
#pragma unroll
            for (int q = 0; q < 3 * RMAX; ++q) rows[q] = q < 3 * R ? p.restraint[(int64_t)k * 3 * R + q] : 0.0;
        }
        const double *urow = DENSE ? p.u_kn + (int64_t)k * p.n_samples + n0 : nullptr;
        double mx = -INFINITY, sum = 0.0;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            for (int i = lane; i < cnt; i += WAVE) {
                double u;
                if (DENSE) {
                    u = urow[i];
                } else {
                    double s[RA];
#pragma unroll
                    for (int r = 0; r < RMAX; ++r) s[r] = sh_cv[r * S + i];
                    u = mbar_u<RMAX, DIH>(beta, rows, sh_E[i], s, period);
                }
                const double v = -u - sh_d[i];
                if (pass == 0)
                    mx = fmax(mx, v);
                else
                    sum += exp(v - mx);
            }
            if (pass == 0) mx = wave_max64(mx);
        }
        sum = wave_sum64(sum);
        if (lane == 0) {
            double *dst = a.part + ((int64_t)blockIdx.x * K + k) * 2;
            dst[0] = mx, dst[1] = sum;
        }
    }
}

// (the kind of the columns lives in device memory: the kernel picks the body, the same in every thread)
template <int RMAX, bool DENSE>
__global__ __launch_bounds__(MD_BLOCK) void k_mbar_states(MbarArgs a)
{
    if (!DENSE && RMAX > 0 && mbar_dihedral_mask(a.p))
        mbar_states_body<RMAX, DENSE, RMAX != 0>(a);
    else
        mbar_states_body<RMAX, DENSE, false>(a);
}

struct FinishArgs {
    const int32_t *status;
    const double *part, *f_old;
    double *f_raw, *f_new, *delta;
    int32_t K, n_chunks;
};

// the chunks of a state in ascending order against their maximum
__device__ __forceinline__ double mbar_combine(const double *part, int64_t stride, int n_chunks)
{
    double mx = -INFINITY, sum = 0.0;
    for (int c = 0; c < n_chunks; ++c) mx = fmax(mx, part[c * stride]);
    for (int c = 0; c < n_chunks; ++c) sum += part[c * stride + 1] * exp(part[c * stride] - mx);
    return mx + log(sum);
}

__global__ __launch_bounds__(MD_BLOCK) void k_mbar_finish(FinishArgs a)
{
    if (*a.status) return;
    __shared__ double sh_f0, sh_max[MD_BLOCK / WAVE];
    for (int k = threadIdx.x; k < a.K; k += MD_BLOCK) {
        const double f = -mbar_combine(a.part + 2 * (int64_t)k, 2 * (int64_t)a.K, a.n_chunks);
        a.f_raw[k] = f;   // (read back by this thread alone)
        if (k == 0) sh_f0 = f;
    }
    __syncthreads();
    double dmax = 0.0;
    for (int k = threadIdx.x; k < a.K; k += MD_BLOCK) {
        const double f = a.f_raw[k] - sh_f0;
        dmax = fmax(dmax, fabs(f - a.f_old[k]));
        a.f_new[k] = f;
    }
    dmax = wave_max64(dmax);
    if (lane_id() == 0) sh_max[threadIdx.x / WAVE] = dmax;
    __syncthreads();
    if (threadIdx.x == 0) a.delta[0] = fmax(fmax(sh_max[0], sh_max[1]), fmax(sh_max[2], sh_max[3]));
}

// ---- log weights ------------------------------------------------------------------------------------------------------------------
struct TargetArgs {
    anihip_mbar p;
    const double *beta, *rows, *u;   // the target: beta [1] and rows [R][3], or its dense row [N]
    const double *d;
    double *raw, *part, *ln_z, *out;
    int64_t n_first, n_count;
    int32_t n_chunks;
};

// a_n = -u_t(x_n) - d_n of every sample, and (max, sum) of each chunk of 1024
__global__ __launch_bounds__(MD_BLOCK) void k_mbar_target_chunks(TargetArgs a)
{
    const anihip_mbar &p = a.p;
    if (*p.status) return;
    __shared__ double sh[MD_BLOCK / WAVE];
    const uint32_t dih = mbar_dihedral_mask(p);
    const double beta = a.u ? 0.0 : a.beta[0];
    const int64_t n0 = (int64_t)blockIdx.x * MBAR_TARGET_CHUNK;
    constexpr int PER = MBAR_TARGET_CHUNK / MD_BLOCK;
    double v[PER], mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int64_t n = n0 + j * MD_BLOCK + threadIdx.x;
        v[j] = -INFINITY;
        if (n < p.n_samples) {
            v[j] = -(a.u ? a.u[n] : mbar_u_at(p, dih, beta, a.rows, n)) - a.d[n];
            a.raw[n] = v[j];
        }
        mx = fmax(mx, v[j]);
    }
    mx = wave_max64(mx);
    if (lane_id() == 0) sh[threadIdx.x / WAVE] = mx;
    __syncthreads();
    mx = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
    double sum[1] = {0.0};
#pragma unroll
    for (int j = 0; j < PER; ++j) sum[0] += exp(v[j] - mx);   // (exp(-inf) = 0 past the end)
    md_block_sum<1>(sum);
    if (threadIdx.x == 0) a.part[2 * blockIdx.x] = mx, a.part[2 * blockIdx.x + 1] = sum[0];
}

__global__ void k_mbar_target_finish(TargetArgs a)
{
    if (*a.p.status) return;
    a.ln_z[0] = mbar_combine(a.part, 2, a.n_chunks);
}

__global__ __launch_bounds__(MD_BLOCK) void k_mbar_target_write(TargetArgs a)
{
    if (*a.p.status) return;
    const int64_t i = blockIdx.x * (int64_t)MD_BLOCK + threadIdx.x;
    if (i < a.n_count) a.out[i] = a.raw[a.n_first + i] - a.ln_z[0];
}

// ln W_nk = f_k - u_k(x_n) - d_n, out [n_count][K]: one thread per pair, consecutive threads on consecutive states
__global__ __launch_bounds__(MD_BLOCK) void k_mbar_all(MbarArgs a, double *out)
{
    const anihip_mbar &p = a.p;
    if (*p.status) return;
    const uint32_t dih = mbar_dihedral_mask(p);
    const int K = p.n_states;
    const int64_t total = a.n_count * K;
    for (int64_t w = blockIdx.x * (int64_t)MD_BLOCK + threadIdx.x; w < total; w += (int64_t)gridDim.x * MD_BLOCK) {
        const int64_t n = a.n_first + w / K;
        const int k = (int)(w % K);
        const double u = p.u_kn ? p.u_kn[(int64_t)k * p.n_samples + n]
                                : mbar_u_at(p, dih, p.beta[k], p.restraint + (int64_t)k * 3 * p.n_cvs, n);
        out[w] = a.f[k] - u - a.d[n];
    }
}

// ---- histogram --------------------------------------------------------------------------------------------------------------------
struct HistArgs {
    int64_t n, chunk;
    const double *log_w, *cv;
    int32_t stride, n_cols, col[2], bins[2], n_chunks;
    double lo[2], hi[2], inv_width[2];
    unsigned long long *key, *counts;
    double *part, *out;
};

// keys that order as the doubles do
__device__ __forceinline__ unsigned long long mbar_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return b >> 63 ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double mbar_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)(k >> 63 ? k & 0x7FFFFFFFFFFFFFFFull : ~k));
}

// the bin of sample n, or -1: outside lo <= s < hi in a column, or a weight that is NaN
__device__ __forceinline__ int mbar_bin(const HistArgs &a, int64_t n)
{
    if (a.log_w[n] != a.log_w[n]) return -1;
    int bin = 0;
    for (int c = 0; c < a.n_cols; ++c) {
        const double s = a.cv[n * a.stride + a.col[c]];
        if (!(s >= a.lo[c] && s < a.hi[c])) return -1;
        bin = bin * a.bins[c] + min((int)((s - a.lo[c]) * a.inv_width[c]), a.bins[c] - 1);
    }
    return bin;
}

__global__ __launch_bounds__(MD_BLOCK) void k_mbar_hist_max(HistArgs a)
{
    const int64_t n = blockIdx.x * (int64_t)MD_BLOCK + threadIdx.x;
    if (n >= a.n) return;
    const int bin = mbar_bin(a, n);
    if (bin < 0) return;
    atomicMax(a.key + bin, mbar_key(a.log_w[n]));   // (integers: the result does not depend on the order)
    atomicAdd(a.counts + bin, 1ull);
}

// one wave per chunk of samples: the bins' sums of exp(w - max) in LDS, lanes of equal bin added by a butterfly
__global__ __launch_bounds__(WAVE) void k_mbar_hist_sum(HistArgs a)
{
    extern __shared__ double mbar_bins[];
    const int B = a.bins[0] * (a.n_cols > 1 ? a.bins[1] : 1), lane = threadIdx.x;
    for (int b = lane; b < B; b += WAVE) mbar_bins[b] = 0.0;
    wave_sync();
    const int64_t lo = blockIdx.x * a.chunk, hi = min(lo + a.chunk, a.n);
    for (int64_t base = lo; base < hi; base += WAVE) {
        const int64_t n = base + lane;
        const int bin = n < hi ? mbar_bin(a, n) : -1;
        double t = 0.0;
        if (bin >= 0) {
            const double mx = mbar_unkey(a.key[bin]);
            t = mx == -INFINITY ? 0.0 : exp(a.log_w[n] - mx);
        }
        unsigned long long todo = __ballot(bin >= 0);
        while (todo) {   // (the same in every lane)
            const int b = __shfl(bin, __ffsll((long long)todo) - 1);
            const bool mine = bin == b;
            const double v = wave_sum64(mine ? t : 0.0);
            if (lane == 0) mbar_bins[b] += v;
            todo &= ~__ballot(mine);
        }
    }
    wave_sync();
    for (int b = lane; b < B; b += WAVE) a.part[(int64_t)blockIdx.x * B + b] = mbar_bins[b];
}

__global__ __launch_bounds__(MD_BLOCK) void k_mbar_hist_finish(HistArgs a)
{
    const int B = a.bins[0] * (a.n_cols > 1 ? a.bins[1] : 1), b = blockIdx.x * MD_BLOCK + threadIdx.x;
    if (b >= B) return;
    if (!a.counts[b]) {
        a.out[b] = -INFINITY;
        return;
    }
    double sum = 0.0;
    for (int c = 0; c < a.n_chunks; ++c) sum += a.part[(int64_t)c * B + b];
    a.out[b] = mbar_unkey(a.key[b]) + log(sum);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// the instantiation that serves R columns: R rounded up to 0, 1, 2, 4, 8 or 16
static int mbar_rmax(int R) { return R <= 2 ? R : R <= 4 ? 4 : R <= 8 ? 8 : 16; }
static int mbar_chunk_samples(int R) { return std::min(MBAR_MAX_CHUNK, MBAR_CHUNK_DOUBLES / (2 + mbar_rmax(R)) / WAVE * WAVE); }

struct MbarLayout {
    int32_t chunk, n_chunks, target_chunks;
    size_t ln_n, f_a, f_b, f_raw, d, raw, part, target_part, ln_z, total;
};

static MbarLayout mbar_layout(const anihip_mbar *p)
{
    MbarLayout l{};
    const size_t K = (size_t)p->n_states, N = (size_t)p->n_samples;
    l.chunk = mbar_chunk_samples(p->u_kn ? 0 : p->n_cvs);
    l.n_chunks = (int32_t)((N + l.chunk - 1) / l.chunk);
    l.target_chunks = (int32_t)((N + MBAR_TARGET_CHUNK - 1) / MBAR_TARGET_CHUNK);
    size_t off = 0;
    auto take = [&](size_t doubles) { const size_t at = off; off += doubles * sizeof(double); return at; };
    l.ln_n = take(K), l.f_a = take(K), l.f_b = take(K), l.f_raw = take(K), l.d = take(N), l.raw = take(N);
    l.part = take((size_t)l.n_chunks * K * 2), l.target_part = take((size_t)l.target_chunks * 2), l.ln_z = take(1);
    l.total = off;
    return l;
}

static int mbar_validate(const anihip_mbar *p)
{
    ANIHIP_REQUIRE(p, "null pointer argument");
    ANIHIP_REQUIRE(p->n_states >= 1, "n_states must be >= 1, got %d", p->n_states);
    ANIHIP_REQUIRE(p->n_cvs >= 0 && p->n_cvs <= MBAR_CVS, "n_cvs must be in 0 .. %d, got %d", MBAR_CVS, p->n_cvs);
    ANIHIP_REQUIRE(p->n_samples >= 1, "n_samples must be >= 1, got %lld", (long long)p->n_samples);
    ANIHIP_REQUIRE(p->n_samples < ((int64_t)1 << 40), "n_samples must stay below 2^40");
    ANIHIP_REQUIRE(p->n_k && p->status, "null pointer in the problem: n_k and status are needed");
    if (!p->u_kn) {
        ANIHIP_REQUIRE(p->beta, "null pointer in the problem: the structured mode needs beta");
        ANIHIP_REQUIRE(p->n_cvs == 0 || (p->restraint && p->cv_kind && p->cv),
                       "null pointer in the problem: n_cvs > 0 needs restraint, cv_kind and cv");
    }
    return 0;
}

static int mbar_check(hipStream_t st, const anihip_mbar *p, double *ln_n, int64_t n_first, int64_t n_count, const double *t_beta,
                      const double *t_rows, const double *t_u)
{
    zero_words_async(st, p->status, sizeof(int32_t));
    CheckArgs c{*p, ln_n, n_first, n_count, t_beta, t_rows, t_u};
    const int64_t items = n_count * std::max<int64_t>(1, p->u_kn ? p->n_states : p->n_cvs);
    hipLaunchKernelGGL(k_mbar_check, dim3((unsigned)std::min<int64_t>((items + MD_BLOCK - 1) / MD_BLOCK, 2048)), dim3(MD_BLOCK), 0,
                       st, c);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

template <bool STATES>
static void mbar_launch(hipStream_t st, const MbarArgs &a, unsigned blocks, size_t lds)
{
#define MBAR_CASE(RMAX, DENSE)                                                                                        \
    if (STATES)                                                                                                       \
        hipLaunchKernelGGL((k_mbar_states<RMAX, DENSE>), dim3(blocks), dim3(MD_BLOCK), lds, st, a);                   \
    else                                                                                                              \
        hipLaunchKernelGGL((k_mbar_samples<RMAX, DENSE>), dim3(blocks), dim3(MD_BLOCK), lds, st, a)
    const int R = mbar_rmax(a.p.n_cvs);
    if (a.p.u_kn) { MBAR_CASE(0, true); }
    else if (R == 0) { MBAR_CASE(0, false); }
    else if (R == 1) { MBAR_CASE(1, false); }
    else if (R == 2) { MBAR_CASE(2, false); }
    else if (R == 4) { MBAR_CASE(4, false); }
    else if (R == 8) { MBAR_CASE(8, false); }
    else { MBAR_CASE(16, false); }
#undef MBAR_CASE
}

// d_n of the samples first <= n < first + count from f
static int mbar_samples(hipStream_t st, MbarArgs &a, const double *f, int64_t n_first, int64_t n_count)
{
    const int W = a.p.u_kn ? 1 : 2 + 3 * mbar_rmax(a.p.n_cvs);
    a.f = f, a.n_first = n_first, a.n_count = n_count;
    a.tile = std::min<int>(a.p.n_states, MBAR_TILE_BYTES / (int)sizeof(double) / W);
    const int64_t per = MD_BLOCK * MBAR_SPT;
    mbar_launch<false>(st, a, (unsigned)((n_count + per - 1) / per), (size_t)a.tile * W * sizeof(double));
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace anihip

using namespace anihip;

extern "C" size_t anihip_mbar_workspace_bytes(const anihip_mbar *problem)
{
    if (mbar_validate(problem)) return 0;
    return mbar_layout(problem).total;
}

extern "C" int anihip_mbar_iterate(void *stream, const anihip_mbar *problem, const double *f_in, int32_t n_iter, double *f_out,
                                   double *delta, void *workspace, size_t workspace_bytes)
{
    if (int rc = mbar_validate(problem)) return rc;
    ANIHIP_REQUIRE(f_in && f_out && delta, "null pointer argument");
    ANIHIP_REQUIRE(n_iter >= 1, "n_iter must be >= 1, got %d", n_iter);
    const MbarLayout l = mbar_layout(problem);
    ANIHIP_REQUIRE(workspace && workspace_bytes >= l.total, "workspace holds %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    MbarArgs a{};
    a.p = *problem, a.ln_n = (double *)(ws + l.ln_n), a.d = (double *)(ws + l.d), a.part = (double *)(ws + l.part);
    a.chunk = l.chunk, a.n_chunks = l.n_chunks;
    if (int rc = mbar_check(st, problem, a.ln_n, 0, problem->n_samples, nullptr, nullptr, nullptr)) return rc;
    double *buf[2] = {(double *)(ws + l.f_a), (double *)(ws + l.f_b)};
    const double *f = f_in;
    const int R = problem->u_kn ? 0 : mbar_rmax(problem->n_cvs);
    for (int it = 0; it < n_iter; ++it) {
        if (int rc = mbar_samples(st, a, f, 0, problem->n_samples)) return rc;
        mbar_launch<true>(st, a, (unsigned)l.n_chunks, (size_t)l.chunk * (2 + R) * sizeof(double));
        ANIHIP_CHECK_HIP(hipGetLastError());
        double *f_new = it == n_iter - 1 ? f_out : buf[it & 1];
        FinishArgs fin{problem->status, a.part, f, (double *)(ws + l.f_raw), f_new, delta, problem->n_states, l.n_chunks};
        hipLaunchKernelGGL(k_mbar_finish, dim3(1), dim3(MD_BLOCK), 0, st, fin);
        ANIHIP_CHECK_HIP(hipGetLastError());
        f = f_new;
    }
    return 0;
}

extern "C" int anihip_mbar_log_weights(void *stream, const anihip_mbar *problem, const double *f, int32_t target,
                                       const double *target_beta, const double *target_restraint, const double *target_u,
                                       int64_t n_first, int64_t n_count, double *out, void *workspace, size_t workspace_bytes)
{
    if (int rc = mbar_validate(problem)) return rc;
    ANIHIP_REQUIRE(f && out, "null pointer argument");
    ANIHIP_REQUIRE(target >= ANIHIP_MBAR_TARGET_ALL && target < problem->n_states, "target must be a state below %d, "
                   "ANIHIP_MBAR_TARGET_EXTERNAL or ANIHIP_MBAR_TARGET_ALL, got %d", problem->n_states, target);
    ANIHIP_REQUIRE(n_first >= 0 && n_count >= 1 && n_first + n_count <= problem->n_samples,
                   "the slab %lld + %lld does not lie in the %lld samples", (long long)n_first, (long long)n_count,
                   (long long)problem->n_samples);
    const int R = problem->n_cvs;
    if (target == ANIHIP_MBAR_TARGET_EXTERNAL) {
        if (problem->u_kn)
            ANIHIP_REQUIRE(target_u, "an external target of a dense problem needs target_u");
        else
            ANIHIP_REQUIRE(target_beta && (R == 0 || target_restraint), "an external target needs target_beta and target_restraint");
    }
    const MbarLayout l = mbar_layout(problem);
    ANIHIP_REQUIRE(workspace && workspace_bytes >= l.total, "workspace holds %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    MbarArgs a{};
    a.p = *problem, a.ln_n = (double *)(ws + l.ln_n), a.d = (double *)(ws + l.d), a.part = (double *)(ws + l.part);
    a.chunk = l.chunk, a.n_chunks = l.n_chunks;
    if (target == ANIHIP_MBAR_TARGET_ALL) {
        if (int rc = mbar_check(st, problem, a.ln_n, n_first, n_count, nullptr, nullptr, nullptr)) return rc;
        if (int rc = mbar_samples(st, a, f, n_first, n_count)) return rc;
        const int64_t total = n_count * problem->n_states;
        hipLaunchKernelGGL(k_mbar_all, dim3((unsigned)std::min<int64_t>((total + MD_BLOCK - 1) / MD_BLOCK, 65536)), dim3(MD_BLOCK), 0,
                           st, a, out);
        ANIHIP_CHECK_HIP(hipGetLastError());
        return 0;
    }
    // one target: normalized over all samples, whatever the slab
    TargetArgs t{};
    t.p = *problem;
    if (target >= 0) {
        if (problem->u_kn)
            t.u = problem->u_kn + (int64_t)target * problem->n_samples;
        else
            t.beta = problem->beta + target, t.rows = problem->restraint + (int64_t)target * 3 * R;
    } else if (problem->u_kn) {
        t.u = target_u;
    } else {
        t.beta = target_beta, t.rows = target_restraint;
    }
    const bool external = target == ANIHIP_MBAR_TARGET_EXTERNAL;
    if (int rc = mbar_check(st, problem, a.ln_n, 0, problem->n_samples, external ? t.beta : nullptr, external ? t.rows : nullptr,
                            external ? t.u : nullptr))
        return rc;
    if (int rc = mbar_samples(st, a, f, 0, problem->n_samples)) return rc;
    t.d = a.d, t.raw = (double *)(ws + l.raw), t.part = (double *)(ws + l.target_part), t.ln_z = (double *)(ws + l.ln_z);
    t.out = out, t.n_first = n_first, t.n_count = n_count, t.n_chunks = l.target_chunks;
    hipLaunchKernelGGL(k_mbar_target_chunks, dim3((unsigned)l.target_chunks), dim3(MD_BLOCK), 0, st, t);
    ANIHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_mbar_target_finish, dim3(1), dim3(1), 0, st, t);
    ANIHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_mbar_target_write, dim3((unsigned)((n_count + MD_BLOCK - 1) / MD_BLOCK)), dim3(MD_BLOCK), 0, st, t);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

static int hist_chunks(int64_t n, int64_t *chunk)
{
    int64_t chunks = std::min<int64_t>((n + MBAR_HIST_MIN_CHUNK - 1) / MBAR_HIST_MIN_CHUNK, MBAR_HIST_MAX_CHUNKS);
    *chunk = ((n + chunks - 1) / chunks + WAVE - 1) / WAVE * WAVE;
    return (int)((n + *chunk - 1) / *chunk);
}

extern "C" size_t anihip_mbar_histogram_workspace_bytes(int64_t n_samples, int32_t n_bins)
{
    if (n_samples < 1 || n_bins < 1 || n_bins > ANIHIP_MBAR_MAX_BINS) {
        set_error("anihip_mbar_histogram_workspace_bytes: n_samples must be >= 1 and n_bins in 1 .. %d", ANIHIP_MBAR_MAX_BINS);
        return 0;
    }
    int64_t chunk;
    return ((size_t)hist_chunks(n_samples, &chunk) + 1) * (size_t)n_bins * sizeof(double);
}

extern "C" int anihip_mbar_histogram(void *stream, int64_t n_samples, const double *log_weights, const double *cv, int32_t cv_stride,
                                     int32_t n_columns, const int32_t *columns, const double *lo, const double *hi,
                                     const int32_t *bins, double *out, int64_t *counts, void *workspace, size_t workspace_bytes)
{
    ANIHIP_REQUIRE(log_weights && cv && columns && lo && hi && bins && out && counts, "null pointer argument");
    ANIHIP_REQUIRE(n_samples >= 1 && n_samples < ((int64_t)1 << 40), "n_samples must be in 1 .. 2^40 - 1, got %lld",
                   (long long)n_samples);
    ANIHIP_REQUIRE(n_columns == 1 || n_columns == 2, "a histogram has one or two columns, got %d", n_columns);
    ANIHIP_REQUIRE(cv_stride >= 1, "cv_stride must be >= 1, got %d", cv_stride);
    HistArgs a{};
    int64_t B = 1;
    for (int c = 0; c < n_columns; ++c) {
        ANIHIP_REQUIRE(columns[c] >= 0 && columns[c] < cv_stride, "column %d is outside 0 .. %d", columns[c], cv_stride - 1);
        ANIHIP_REQUIRE(bins[c] >= 1 && bins[c] <= ANIHIP_MBAR_MAX_BINS, "bins must be in 1 .. %d, got %d", ANIHIP_MBAR_MAX_BINS, bins[c]);
        ANIHIP_REQUIRE(hi[c] > lo[c] && hi[c] - lo[c] < 1e300, "the edges need lo < hi, got %g and %g", lo[c], hi[c]);
        a.col[c] = columns[c], a.bins[c] = bins[c], a.lo[c] = lo[c], a.hi[c] = hi[c], a.inv_width[c] = (double)bins[c] / (hi[c] - lo[c]);
        B *= bins[c];
    }
    ANIHIP_REQUIRE(B <= ANIHIP_MBAR_MAX_BINS, "%lld bins in all, more than %d", (long long)B, ANIHIP_MBAR_MAX_BINS);
    a.n = n_samples, a.n_chunks = hist_chunks(n_samples, &a.chunk);
    const size_t need = ((size_t)a.n_chunks + 1) * (size_t)B * sizeof(double);
    ANIHIP_REQUIRE(workspace && workspace_bytes >= need, "workspace holds %zu bytes, %zu needed", workspace_bytes, need);
    a.log_w = log_weights, a.cv = cv, a.stride = cv_stride, a.n_cols = n_columns;
    a.key = (unsigned long long *)workspace, a.part = (double *)workspace + B, a.counts = (unsigned long long *)counts, a.out = out;
    hipStream_t st = (hipStream_t)stream;
    zero_words_async(st, a.key, (size_t)B * 8);   // (key 0 lies below the key of every double)
    zero_words_async(st, counts, (size_t)B * 8);
    hipLaunchKernelGGL(k_mbar_hist_max, dim3((unsigned)((n_samples + MD_BLOCK - 1) / MD_BLOCK)), dim3(MD_BLOCK), 0, st, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_mbar_hist_sum, dim3((unsigned)a.n_chunks), dim3(WAVE), (size_t)B * sizeof(double), st, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_mbar_hist_finish, dim3((unsigned)((B + MD_BLOCK - 1) / MD_BLOCK)), dim3(MD_BLOCK), 0, st, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}
