// Lowest normal modes of block-sparse Hessians (grad.sparse_vibrational_analysis): the operator
//
//     A = M^-1/2 ((H + H^T) / 2) M^-1/2
//
// over the blocks of a tuples.BlockHessian, in a layout of its own, and its product with a block of m vectors.
//
//   k_hm_offsets  column offsets coff[a] = first entry of column a (a lower bound in index[1]); clears diag[]
//   k_hm_blocks   per stored block (row j, column a): the int32 row, the transpose partner (binary search for row a in column
//                 j, whose rows are sorted), the symmetrized mass-weighted block A~_ja = (B_ja + B_aj^T) / (2 sqrt(m_j m_a)),
//                 the position of each atom's diagonal block; bad input sets bits of *status
//   k_hm_gersh    per atom the largest Gershgorin row sum of its three rows (the bound ||A||_G <= max over a molecule)
//   k_hm_spmm     Y = A X for X, Y [N][3][m] fp32 (vector index fastest).  A is symmetric, so row a of Y comes from column a's
//                 contiguous blocks:  Y[a] = sum_{p in column a} A~[p]^T X[rows[p]].  One wave per column atom; the lanes
//                 are G = 64 / MW groups of MW >= m vector lanes, group g taking the blocks g, g + G, ..  of the column (staged
//                 through LDS, 64 at a time: one coalesced read of the column's blocks).  Products and sums in fp64, the
//                 groups reduced by a fixed butterfly: every output row is written once, no atomics, bit-identical run to run.
#include "anihip_common.h"

namespace anihip {

constexpr int HM_WPB = 4;       // waves (neighbouring column atoms) per block of k_hm_spmm
constexpr int HM_STAGE = 64;    // blocks staged in LDS per wave and step
constexpr uint32_t HM_BAD_INDEX = ANIHIP_BLOCK_HESSIAN_BAD_INDEX, HM_NO_PARTNER = ANIHIP_BLOCK_HESSIAN_NO_PARTNER,
                   HM_NO_DIAGONAL = ANIHIP_BLOCK_HESSIAN_NO_DIAGONAL;

__device__ __forceinline__ int64_t lower_bound64(const int64_t *__restrict__ v, int64_t lo, int64_t hi, int64_t key)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_hm_offsets(int64_t n_atoms, int64_t nnz, const int64_t *__restrict__ index,
                                                    int64_t *__restrict__ coff, int64_t *__restrict__ diag)
{
    for (int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; a <= n_atoms; a += (int64_t)gridDim.x * blockDim.x) {
        coff[a] = lower_bound64(index + nnz, 0, nnz, a);
        if (a < n_atoms) diag[a] = -1;
    }
}

__global__ __launch_bounds__(256) void k_hm_blocks(int64_t n_atoms, int64_t nnz, const int64_t *__restrict__ index,
                                                   const float *__restrict__ blocks, const double *__restrict__ masses,
                                                   const int64_t *__restrict__ coff, int32_t *__restrict__ rows,
                                                   int64_t *__restrict__ partner, float *__restrict__ ablocks,
                                                   int64_t *__restrict__ diag, uint32_t *__restrict__ status)
{
    const int64_t *row = index, *col = index + nnz;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = row[p], a = col[p];
        float *o = ablocks + 9 * (size_t)p;
        bool ok = 0 <= j && j < n_atoms && 0 <= a && a < n_atoms;
        if (ok && p > 0 && (col[p - 1] > a || (col[p - 1] == a && row[p - 1] >= j))) ok = false;   // not column-sorted
        if (!ok) {
            atomicOr(status, HM_BAD_INDEX);
            rows[p] = 0;
            partner[p] = -1;
#pragma unroll
            for (int e = 0; e < 9; ++e) o[e] = 0.f;
            continue;
        }
        rows[p] = (int32_t)j;
        const int64_t j0 = coff[j], j1 = coff[j + 1];
        const int64_t q = lower_bound64(row, j0, j1 > j0 ? j1 : j0, a);
        if (q >= j1 || row[q] != a) {
            atomicOr(status, HM_NO_PARTNER);
            partner[p] = -1;
#pragma unroll
            for (int e = 0; e < 9; ++e) o[e] = 0.f;
            continue;
        }
        partner[p] = q;
        if (j == a) {
            diag[a] = p;
        } else {   // every atom with a block must have its diagonal block
            const int64_t d = lower_bound64(row, j0, j1 > j0 ? j1 : j0, j);
            if (d >= j1 || row[d] != j) atomicOr(status, HM_NO_DIAGONAL);
        }
        const double w = 0.5 / sqrt(masses[j] * masses[a]);
        const float *b = blocks + 9 * (size_t)p, *bt = blocks + 9 * (size_t)q;
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) o[3 * x + y] = (float)(((double)b[3 * x + y] + (double)bt[3 * y + x]) * w);
    }
}

__global__ __launch_bounds__(256) void k_hm_gersh(int64_t n_atoms, const int64_t *__restrict__ coff,
                                                  const float *__restrict__ ablocks, double *__restrict__ gersh)
{
    for (int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; a < n_atoms; a += (int64_t)gridDim.x * blockDim.x) {
        double s[3] = {0.0, 0.0, 0.0};   // rows (a, x) of A: sum_j sum_y |A~_ja[y][x]|
        for (int64_t p = coff[a]; p < coff[a + 1]; ++p) {
            const float *b = ablocks + 9 * (size_t)p;
#pragma unroll
            for (int x = 0; x < 3; ++x) s[x] += fabs((double)b[x]) + fabs((double)b[3 + x]) + fabs((double)b[6 + x]);
        }
        gersh[a] = fmax(s[0], fmax(s[1], s[2]));
    }
}

template <int MW>
__global__ __launch_bounds__(HM_WPB *WAVE) void k_hm_spmm(int64_t n_atoms, int m, const int64_t *__restrict__ coff,
                                                          const int32_t *__restrict__ rows,
                                                          const float *__restrict__ ablocks, const float *__restrict__ x,
                                                          float *__restrict__ y)
{
    constexpr int G = WAVE / MW;
    __shared__ float s_b[HM_WPB][HM_STAGE * 9];
    __shared__ int s_j[HM_WPB][HM_STAGE];
    const int wib = threadIdx.x >> 6, lane = lane_id();
    const int64_t a = blockIdx.x * (int64_t)HM_WPB + wib;
    if (a >= n_atoms) return;   // (a whole wave: k_hm_spmm has no block barrier)
    const int v = lane & (MW - 1), g = lane / MW;
    const bool act = v < m;
    float *sb = s_b[wib];
    int *sj = s_j[wib];
    const int64_t p0 = coff[a], p1 = coff[a + 1];
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    for (int64_t base = p0; base < p1; base += HM_STAGE) {
        const int n = (int)(p1 - base < HM_STAGE ? p1 - base : HM_STAGE);
        const float *src = ablocks + 9 * (size_t)base;
        for (int e = lane; e < 9 * n; e += WAVE) sb[e] = src[e];
        if (lane < n) sj[lane] = rows[base + lane];
        wave_sync();
        if (act) {
            for (int q = g; q < n; q += G) {
                const float *xj = x + (size_t)sj[q] * 3 * m + v;
                const double x0 = xj[0], x1 = xj[m], x2 = xj[2 * m];
                const float *b = sb + 9 * q;   // A~[p][y][x]: Y[a][x] += sum_y b[3 y + x] X[j][y]
                acc0 = fma((double)b[0], x0, fma((double)b[3], x1, fma((double)b[6], x2, acc0)));
                acc1 = fma((double)b[1], x0, fma((double)b[4], x1, fma((double)b[7], x2, acc1)));
                acc2 = fma((double)b[2], x0, fma((double)b[5], x1, fma((double)b[8], x2, acc2)));
            }
        }
        wave_sync();
    }
#pragma unroll
    for (int off = MW; off < WAVE; off <<= 1) {
        acc0 += __shfl_xor(acc0, off);
        acc1 += __shfl_xor(acc1, off);
        acc2 += __shfl_xor(acc2, off);
    }
    if (g == 0 && act) {
        float *ya = y + (size_t)a * 3 * m + v;
        ya[0] = (float)acc0;
        ya[m] = (float)acc1;
        ya[2 * m] = (float)acc2;
    }
}

static unsigned hm_grid(int64_t n, int64_t per, int64_t cap)
{
    int64_t b = (n + per - 1) / per;
    if (b > cap) b = cap;
    return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace anihip

using namespace anihip;

extern "C" int anihip_block_hessian_prepare(void *stream, int64_t n_atoms, int64_t nnz, const int64_t *index,
                                            const float *blocks, const double *masses, int64_t *coff, int32_t *rows,
                                            int64_t *partner, float *ablocks, double *gersh, int64_t *diag,
                                            uint32_t *status)
{
    ANIHIP_REQUIRE(coff && diag && gersh && status, "null pointer argument");
    ANIHIP_REQUIRE(nnz == 0 || (index && blocks && masses && rows && partner && ablocks), "null pointer argument");
    ANIHIP_REQUIRE(n_atoms >= 0 && n_atoms < ((int64_t)1 << 31) && nnz >= 0, "n_atoms must be in 0 .. 2^31 and nnz >= 0");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_hm_offsets, dim3(hm_grid(n_atoms + 1, 256, 8192)), dim3(256), 0, s, n_atoms, nnz, index, coff, diag);
    ANIHIP_CHECK_HIP(hipGetLastError());
    if (nnz > 0) {
        hipLaunchKernelGGL(k_hm_blocks, dim3(hm_grid(nnz, 256, 65536)), dim3(256), 0, s, n_atoms, nnz, index, blocks, masses,
                           coff, rows, partner, ablocks, diag, status);
        ANIHIP_CHECK_HIP(hipGetLastError());
    }
    if (n_atoms > 0) {
        hipLaunchKernelGGL(k_hm_gersh, dim3(hm_grid(n_atoms, 256, 8192)), dim3(256), 0, s, n_atoms, coff, ablocks, gersh);
        ANIHIP_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int anihip_block_hessian_spmm(void *stream, int64_t n_atoms, int32_t m, const int64_t *coff, const int32_t *rows,
                                         const float *ablocks, const float *x, float *y)
{
    ANIHIP_REQUIRE(coff && rows && ablocks && x && y, "null pointer argument");
    ANIHIP_REQUIRE(1 <= m && m <= ANIHIP_BLOCK_HESSIAN_MAX_VECTORS, "m must be 1 .. %d", ANIHIP_BLOCK_HESSIAN_MAX_VECTORS);
    ANIHIP_REQUIRE(n_atoms >= 0 && n_atoms < ((int64_t)1 << 31), "n_atoms must be in 0 .. 2^31");
    if (n_atoms == 0) return 0;
    const dim3 grid(hm_grid(n_atoms, HM_WPB, (int64_t)1 << 30)), block(HM_WPB * WAVE);
    hipStream_t s = (hipStream_t)stream;
    const int mw = m <= 1 ? 1 : m <= 2 ? 2 : m <= 4 ? 4 : m <= 8 ? 8 : m <= 16 ? 16 : m <= 32 ? 32 : 64;
    switch (mw) {
    case 1: hipLaunchKernelGGL(k_hm_spmm<1>, grid, block, 0, s, n_atoms, m, coff, rows, ablocks, x, y); break;
    case 2: hipLaunchKernelGGL(k_hm_spmm<2>, grid, block, 0, s, n_atoms, m, coff, rows, ablocks, x, y); break;
    case 4: hipLaunchKernelGGL(k_hm_spmm<4>, grid, block, 0, s, n_atoms, m, coff, rows, ablocks, x, y); break;
    case 8: hipLaunchKernelGGL(k_hm_spmm<8>, grid, block, 0, s, n_atoms, m, coff, rows, ablocks, x, y); break;
    case 16: hipLaunchKernelGGL(k_hm_spmm<16>, grid, block, 0, s, n_atoms, m, coff, rows, ablocks, x, y); break;
    case 32: hipLaunchKernelGGL(k_hm_spmm<32>, grid, block, 0, s, n_atoms, m, coff, rows, ablocks, x, y); break;
    default: hipLaunchKernelGGL(k_hm_spmm<64>, grid, block, 0, s, n_atoms, m, coff, rows, ablocks, x, y); break;
    }
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}
