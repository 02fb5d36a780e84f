// Phonons from block-sparse supercell Hessians (torchani_amd/phonons.py).  All arithmetic fp64, every output
// element written once by one thread, no atomics, sums in a fixed order: two calls give the same bits.
//
//   k_ph_fold    one thread per compact entry e = (b; b', n), given as (b, j): j the supercell atom of the home cell's column
//                of b the entry came from.  The block of translation t = (t1, t2, t3) sits in column t n + b at row
//                (cell of j + t mod repeats) n + b': a binary search in that column's sorted int32 rows of
//                anihip_block_hessian_prepare.  Pass 1 sums the N_c blocks in the order of t (a block that is not stored counts
//                as zero and in missing[e]), pass 2 takes max |block - mean| (defect[e]).  Neighbouring entries of a column have
//                neighbouring rows in every translated column, so neighbouring lanes read neighbouring 36-byte blocks.
//                ablocks[p][x][y] = H_(row x),(column y); Phi(b; b', n)_xy = H_(column x),(row y) is its transpose.
//   k_ph_asr     one thread per (b, xy): Phi(b; b, 0)_xy = -1/2 sum over the other entries e of b of (Phi_e,xy + Phi_e,yx).  No
//                thread reads what another writes (the diagonal entries are skipped by every sum).
//   k_ph_dynmat  one wave per output block (b, b') and 64 q points, lane = q.  The run of entries of (b, b') (contiguous: the
//                entries are sorted by (b, b')) is wave-uniform, so Phi, n and R = n a come through scalar loads and every lane
//                keeps the 3 x 3 complex block (and its three derivatives) of its own q in registers: no cross-lane step.
//                The phase is sincospi(2 frac(q . n)).  A lane stores 3 rows of 48 contiguous bytes; the four waves of a
//                workgroup take four consecutive b', i.e. 192 contiguous bytes of each row of each of the 64 matrices.
//   k_ph_dos     one workgroup per bin: thread t sums the modes t, t + 256, .. in that order, the 64 lanes of a wave by a fixed
//                butterfly, the four waves in LDS in the order ((0 + 1) + (2 + 3)).
#include "anihip_common.h"

namespace anihip {

constexpr int PH_WPB = 4;   // waves per workgroup of k_ph_dynmat and k_ph_dos

__device__ __forceinline__ int64_t ph_find(const int32_t *__restrict__ rows, int64_t lo, int64_t hi, int32_t key)
{
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (rows[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return (lo < end && rows[lo] == key) ? lo : -1;
}

__global__ __launch_bounds__(256) void k_ph_fold(int m, int n, int r1, int r2, int r3, const int64_t *__restrict__ coff,
                                                 const int32_t *__restrict__ rows, const float *__restrict__ ablocks,
                                                 const int32_t *__restrict__ ent_b, const int32_t *__restrict__ ent_j,
                                                 double *__restrict__ phi, int32_t *__restrict__ missing,
                                                 double *__restrict__ defect)
{
    const int nc = r1 * r2 * r3;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const int b = ent_b[e], j = ent_j[e];
    double *o = phi + 9 * (size_t)e;
    if (b < 0 || b >= n || j < 0 || j >= nc * n) {   // not an entry of this supercell: nothing is read
#pragma unroll
        for (int c = 0; c < 9; ++c) o[c] = 0.0;
        missing[e] = nc;
        defect[e] = 0.0;
        return;
    }
    const int bp = j % n, lc = j / n;
    const int l3 = lc % r3, l2 = (lc / r3) % r2, l1 = lc / (r3 * r2);
    double mean[9];
    int miss = 0;
    double dmax = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int t = 0;
        for (int t1 = 0; t1 < r1; ++t1)
            for (int t2 = 0; t2 < r2; ++t2)
                for (int t3 = 0; t3 < r3; ++t3, ++t) {
                    const int64_t col = (int64_t)t * n + b;
                    const int rc = (((l1 + t1) % r1) * r2 + (l2 + t2) % r2) * r3 + (l3 + t3) % r3;
                    const int64_t p = ph_find(rows, coff[col], coff[col + 1], rc * n + bp);
                    const float *blk = ablocks + 9 * (size_t)(p < 0 ? 0 : p);
                    if (pass == 0) {
                        if (p < 0) {
                            ++miss;
                            continue;
                        }
#pragma unroll
                        for (int c = 0; c < 9; ++c) s[c] += (double)blk[c];
                    } else {
#pragma unroll
                        for (int c = 0; c < 9; ++c) dmax = fmax(dmax, fabs((p < 0 ? 0.0 : (double)blk[c]) - mean[c]));
                    }
                }
        if (pass == 0) {
#pragma unroll
            for (int c = 0; c < 9; ++c) mean[c] = s[c] / (double)nc;
        }
    }
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y) o[3 * x + y] = mean[3 * y + x];
    missing[e] = miss;
    defect[e] = dmax;
}

__global__ __launch_bounds__(256) void k_ph_asr(int n, int m, const int32_t *__restrict__ boff,
                                                const int32_t *__restrict__ diag_entry, double *phi)
{
    const int tid = blockIdx.x * 256 + threadIdx.x;
    if (tid >= 9 * n) return;
    const int b = tid / 9, c = tid % 9, x = c / 3, y = c % 3;
    const int d = diag_entry[b];
    if (d < 0 || d >= m) return;
    int e0 = boff[b], e1 = boff[b + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > m) e1 = m;
    double sxy = 0.0, syx = 0.0;
    for (int e = e0; e < e1; ++e) {
        if (e == d) continue;
        sxy += phi[9 * (size_t)e + 3 * x + y];
        syx += phi[9 * (size_t)e + 3 * y + x];
    }
    phi[9 * (size_t)d + c] = -0.5 * (sxy + syx);
}

template <bool DERIV>
__global__ __launch_bounds__(PH_WPB *WAVE) void k_ph_dynmat(int n, int64_t n_q, const int32_t *__restrict__ poff,
                                                            const int32_t *__restrict__ nvec, const double *__restrict__ phi,
                                                            const double *__restrict__ rvec, const double *__restrict__ masses,
                                                            const double *__restrict__ q, double *__restrict__ dmat,
                                                            double *__restrict__ dderiv)
{
    const int pair = uniform((int)blockIdx.x * PH_WPB + (int)(threadIdx.x >> 6));   // b n + b'
    if (pair >= n * n) return;   // (a whole wave: no block barrier here)
    const int b = pair / n, bp = pair % n;
    const int e0 = uniform(poff[pair]), e1 = uniform(poff[pair + 1]);
    const double w = 1.0 / sqrt(masses[b] * masses[bp]);
    const size_t dim = 3 * (size_t)n;
    for (int64_t chunk = blockIdx.y; chunk * WAVE < n_q; chunk += gridDim.y) {
        const int64_t iq = chunk * WAVE + lane_id();
        const bool act = iq < n_q;
        const double q0 = act ? q[3 * iq] : 0.0, q1 = act ? q[3 * iq + 1] : 0.0, q2 = act ? q[3 * iq + 2] : 0.0;
        double re[9], im[9], dre[DERIV ? 27 : 1], dim_[DERIV ? 27 : 1];
#pragma unroll
        for (int k = 0; k < 9; ++k) re[k] = im[k] = 0.0;
        if (DERIV) {
#pragma unroll
            for (int k = 0; k < 27; ++k) dre[k] = dim_[k] = 0.0;
        }
        for (int e = e0; e < e1; ++e) {
            const double t = fma(q0, (double)nvec[3 * e], fma(q1, (double)nvec[3 * e + 1], q2 * (double)nvec[3 * e + 2]));
            double s, c;
            sincospi(2.0 * (t - rint(t)), &s, &c);
            const double *p = phi + 9 * (size_t)e;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                re[k] = fma(p[k], c, re[k]);
                im[k] = fma(p[k], s, im[k]);
            }
            if (DERIV) {   // d/dk_a of exp(i k . R) = i R_a (c + i s)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double ra = rvec[3 * e + a];
#pragma unroll
                    for (int k = 0; k < 9; ++k) {
                        const double pr = p[k] * ra;
                        dre[9 * a + k] = fma(-pr, s, dre[9 * a + k]);
                        dim_[9 * a + k] = fma(pr, c, dim_[9 * a + k]);
                    }
                }
            }
        }
        if (!act) continue;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            double2 *o = reinterpret_cast<double2 *>(dmat) + ((size_t)iq * dim + 3 * b + x) * dim + 3 * bp;
#pragma unroll
            for (int y = 0; y < 3; ++y) o[y] = make_double2(w * re[3 * x + y], w * im[3 * x + y]);
        }
        if (DERIV) {
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    double2 *o = reinterpret_cast<double2 *>(dderiv) + (((size_t)iq * 3 + a) * dim + 3 * b + x) * dim + 3 * bp;
#pragma unroll
                    for (int y = 0; y < 3; ++y)
                        o[y] = make_double2(w * dre[9 * a + 3 * x + y], w * dim_[9 * a + 3 * x + y]);
                }
        }
    }
}

__global__ __launch_bounds__(PH_WPB *WAVE) void k_ph_dos(int64_t n_modes, const double *__restrict__ freqs,
                                                         const double *__restrict__ weights, double f_first, double df,
                                                         double inv_sigma, double norm, double *__restrict__ dos)
{
    __shared__ double s_w[PH_WPB];
    const double fk = f_first + (double)blockIdx.x * df;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n_modes; i += PH_WPB * WAVE) {
        const double x = (fk - freqs[i]) * inv_sigma;
        acc += weights[i] * exp(-0.5 * x * x);
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane_id() == 0) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) dos[blockIdx.x] = ((s_w[0] + s_w[1]) + (s_w[2] + s_w[3])) * norm;
}

}  // namespace anihip

using namespace anihip;

extern "C" int anihip_phonon_fold(void *stream, int32_t n_basis, int32_t r1, int32_t r2, int32_t r3, const int64_t *coff,
                                  const int32_t *rows, const float *ablocks, int32_t m, const int32_t *ent_b,
                                  const int32_t *ent_j, const int32_t *boff, const int32_t *diag_entry, double *phi,
                                  int32_t *missing, double *defect)
{
    ANIHIP_REQUIRE(n_basis >= 1 && r1 >= 1 && r2 >= 1 && r3 >= 1 && m >= 0, "n_basis and repeats must be >= 1 and m >= 0");
    ANIHIP_REQUIRE((int64_t)n_basis * r1 * r2 * r3 < ((int64_t)1 << 31) && (int64_t)m * 9 < ((int64_t)1 << 31),
                   "the supercell must hold fewer than 2^31 atoms and the pattern fewer than 2^31 / 9 entries");
    ANIHIP_REQUIRE((boff == nullptr) == (diag_entry == nullptr), "boff and diag_entry go together");
    if (m == 0) return 0;
    ANIHIP_REQUIRE(coff && rows && ablocks && ent_b && ent_j && phi && missing && defect, "null pointer argument");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ph_fold, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, m, n_basis, r1, r2, r3, coff, rows, ablocks,
                       ent_b, ent_j, phi, missing, defect);
    ANIHIP_CHECK_HIP(hipGetLastError());
    if (boff) {
        hipLaunchKernelGGL(k_ph_asr, dim3((unsigned)((9 * n_basis + 255) / 256)), dim3(256), 0, s, n_basis, m, boff, diag_entry,
                           phi);
        ANIHIP_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int anihip_phonon_dynmat(void *stream, int32_t n_basis, int64_t n_q, const int32_t *poff, const int32_t *nvec,
                                    const double *phi, const double *rvec, const double *masses, const double *q, double *dmat,
                                    double *dderiv)
{
    ANIHIP_REQUIRE(n_basis >= 1 && n_basis <= 10922 && n_q >= 1, "n_basis must be 1 .. 10922 and n_q >= 1");
    ANIHIP_REQUIRE(poff && nvec && phi && masses && q && dmat, "null pointer argument");
    ANIHIP_REQUIRE(dderiv == nullptr || rvec != nullptr, "the derivatives need rvec");
    const int64_t pairs = (int64_t)n_basis * n_basis, chunks = (n_q + WAVE - 1) / WAVE;
    const dim3 grid((unsigned)((pairs + PH_WPB - 1) / PH_WPB), (unsigned)(chunks < 65535 ? chunks : 65535)), block(PH_WPB * WAVE);
    hipStream_t s = (hipStream_t)stream;
    if (dderiv)
        hipLaunchKernelGGL(k_ph_dynmat<true>, grid, block, 0, s, n_basis, n_q, poff, nvec, phi, rvec, masses, q, dmat, dderiv);
    else
        hipLaunchKernelGGL(k_ph_dynmat<false>, grid, block, 0, s, n_basis, n_q, poff, nvec, phi, rvec, masses, q, dmat, dderiv);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_phonon_dos(void *stream, int64_t n_modes, const double *freqs, const double *weights, double f_first,
                                 double df, double sigma, int32_t bins, double *dos)
{
    ANIHIP_REQUIRE(n_modes >= 0 && bins >= 1, "n_modes must be >= 0 and bins >= 1");
    ANIHIP_REQUIRE(sigma > 0.0 && df > 0.0, "sigma and df must be positive");
    ANIHIP_REQUIRE(dos && (n_modes == 0 || (freqs && weights)), "null pointer argument");
    hipLaunchKernelGGL(k_ph_dos, dim3((unsigned)bins), dim3(PH_WPB * WAVE), 0, (hipStream_t)stream, n_modes, freqs, weights,
                       f_first, df, 1.0 / sigma, 1.0 / (sigma * 2.5066282746310002), dos);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}
