// Structure of block-sparse Hessians with respect to the coordinates (grad.energies_forces_and_sparse_hessians): the
// row lists R(a), the block pattern P(a), the per-chunk item rows and the extraction of the blocks.
//
// The AEV of atom i depends on the coordinates of R(i) = {i} U rows(i) only (rows(i) = the atoms of its neighbor row,
// periodic images folded onto their atom index).  So d^2 E / d r_a d r_j can be non-zero only if some central atom i has
// a and j in R(i); the rows are symmetric, so i in R(a) and
//
//     P(a) = U_{i in R(a)} R(i).
//
// A unit direction (atom a, component c) changes the AEVs of the central atoms i in R(a) only: its WORK ITEMS are those
// (direction, i) rows, and its Hessian column is non-zero on P(a) only.  Everything here is built from the rows'
// structure, never from values, in O(nnz) memory:
//   k_hs_rlist    R(a) deduplicated (an atom may sit in a row several times through periodic images, or be its own image)
//   k_hs_pattern  P(a) deduplicated and sorted, one work group per atom: LDS hash set, then a rank sort in LDS
//   k_hs_items    the rows (direction, i) of a chunk of direction atoms, ordered so that the rows of a species are
//                 contiguous (what the network GEMMs need), from a scan of the per-(species, atom) counts
//   k_hs_extract  the pattern blocks of a chunk's direction atoms out of the dense [K, N, 3] scratch into the blocks, writing
//                 zeros back to exactly those positions (the scratch is zeroed once per call, never per chunk)
#include "anihip_common.h"

namespace anihip {

constexpr int HS_WPB = 4;            // waves per block of k_hs_rlist
constexpr int HS_TAB = 8192;         // LDS hash slots of k_hs_pattern (a power of two)
constexpr int HS_CAP = 4096;         // largest |P(a)|: rows of at most ANIHIP_MAX_RAD atoms within the radial cutoff bound
                                     // the density, and so |P(a)| to ~8 ANIHIP_MAX_RAD = 2048
constexpr int HS_ITEMS_THREADS = 1024;

// ---- R(a) ------------------------------------------------------------------------------------------------------------
// one wave per atom; roff NULL: rcnt[a] = |R(a)| (0 for padding); else rlist[roff[a] ..] = a, then the other atoms of R(a) in
// row order
__global__ __launch_bounds__(HS_WPB * WAVE) void k_hs_rlist(int64_t n_atoms, const int32_t *__restrict__ species,
                                                            const uint32_t *__restrict__ meta,
                                                            const float4 *__restrict__ ent, const int64_t *__restrict__ roff,
                                                            int32_t *__restrict__ rcnt, int32_t *__restrict__ rlist)
{
    __shared__ int s_j[HS_WPB][MAXR];
    const int wib = threadIdx.x >> 6, lane = lane_id();
    int *sj = s_j[wib];
    const int64_t nw = (int64_t)gridDim.x * HS_WPB;
    for (int64_t a = blockIdx.x * (int64_t)HS_WPB + wib; a < n_atoms; a += nw) {
        if (species[a] < 0) {
            if (!roff && lane == 0) rcnt[a] = 0;
            continue;
        }
        const uint32_t start = meta[(size_t)a * META_W], c = meta[(size_t)a * META_W + 1];
        const int nR = (int)(c & 0xFFFFu) + (int)(c >> 16);
        for (int e = lane; e < nR; e += WAVE) sj[e] = (int)(__float_as_uint(ent[start + e].w) & IDX_MASK);
        wave_sync();
        int n = 1;   // a itself
        for (int e0 = 0; e0 < nR; e0 += WAVE) {
            const int e = e0 + lane;
            bool keep = false;
            if (e < nR) {
                const int j = sj[e];
                keep = j != (int)a && j < n_atoms;
                for (int q = 0; q < e && keep; ++q) keep = sj[q] != j;
            }
            const uint64_t m = __ballot(keep);
            if (roff && keep) rlist[roff[a] + n + mbcnt(m)] = sj[e];
            n += __popcll(m);
        }
        if (lane == 0) {
            if (roff) rlist[roff[a]] = (int)a;
            else rcnt[a] = n;
        }
        wave_sync();
    }
}

// ---- P(a) ------------------------------------------------------------------------------------------------------------
// one 256-thread block per atom a; poff NULL: pcnt[a] = |P(a)|; else index[0][poff[a] + r] = the r-th smallest atom of
// P(a), index[1][..] = a (the pattern by columns: the entries of column a are contiguous and sorted by row).  |P(a)| above
// HS_CAP sets bit 0 of *status and writes nothing for a.
__global__ __launch_bounds__(256) void k_hs_pattern(int64_t n_atoms, const int64_t *__restrict__ roff,
                                                    const int32_t *__restrict__ rlist, const int64_t *__restrict__ poff,
                                                    int64_t nnz, int32_t *__restrict__ pcnt, int64_t *__restrict__ index,
                                                    uint32_t *__restrict__ status)
{
    __shared__ int s_tab[HS_TAB];
    __shared__ int s_list[HS_CAP];
    __shared__ int s_n;
    const int tid = threadIdx.x, wib = tid >> 6, lane = lane_id();
    for (int64_t a = blockIdx.x; a < n_atoms; a += gridDim.x) {
        const int64_t r0 = roff[a], r1 = roff[a + 1];
        if (r1 == r0) {   // padding
            if (!poff && tid == 0) pcnt[a] = 0;
            continue;
        }
        for (int k = tid; k < HS_TAB; k += 256) s_tab[k] = -1;
        if (tid == 0) s_n = 0;
        __syncthreads();
        // insert R(i) for every i in R(a): wave w takes the i, lanes the atoms of R(i)
        for (int64_t q = r0 + wib; q < r1; q += 4) {
            const int i = rlist[q];
            const int64_t b0 = roff[i], b1 = roff[i + 1];
            for (int64_t e = b0 + lane; e < b1; e += WAVE) {
                const int j = rlist[e];
                uint32_t h = ((uint32_t)j * 2654435761u) & (HS_TAB - 1);
                for (int probe = 0; probe < HS_TAB; ++probe) {
                    const int old = atomicCAS(&s_tab[h], -1, j);
                    if (old == -1) {
                        const int k = atomicAdd(&s_n, 1);
                        if (k < HS_CAP) s_list[k] = j;
                        break;
                    }
                    if (old == j) break;
                    h = (h + 1) & (HS_TAB - 1);
                }
            }
        }
        __syncthreads();
        const int n = s_n;
        if (n > HS_CAP) {
            if (tid == 0) {
                atomicOr(status, 1u);
                if (!poff) pcnt[a] = 0;
            }
            __syncthreads();
            continue;
        }
        if (!poff) {
            if (tid == 0) pcnt[a] = n;
        } else {
            const int64_t base = poff[a];
            if (base + n <= nnz) {
                for (int k = tid; k < n; k += 256) {   // rank sort: the keys are distinct
                    const int key = s_list[k];
                    int r = 0;
                    for (int m = 0; m < n; ++m) r += s_list[m] < key;
                    index[base + r] = key;
                    index[nnz + base + r] = a;
                }
            }
        }
        __syncthreads();
    }
}

// ---- the item rows of a chunk ------------------------------------------------------------------------------------------
// One block.  Direction atoms n0 <= a < n1, rows (direction 3 a + c, central atom i) for i in R(a), c = 0, 1, 2: the items
// (a, i) sorted by species of i (then by a, then by position in R(a)), three rows per item.  cnt: scratch of
// S (n1 - n0) + 1 ints.
__global__ __launch_bounds__(HS_ITEMS_THREADS) void k_hs_items(int64_t n0, int64_t n1, int S,
                                                               const int32_t *__restrict__ species,
                                                               const int64_t *__restrict__ roff,
                                                               const int32_t *__restrict__ rlist, int32_t *__restrict__ cnt,
                                                               int32_t *__restrict__ row_atom, int32_t *__restrict__ row_dir)
{
    __shared__ int s_scan[HS_ITEMS_THREADS];
    __shared__ int s_carry;
    const int tid = threadIdx.x;
    const int64_t nA = n1 - n0;
    for (int64_t k = tid; k < nA; k += HS_ITEMS_THREADS) {   // counts per (species, direction atom)
        int c[MAX_S];
#pragma unroll
        for (int s = 0; s < MAX_S; ++s) c[s] = 0;
        for (int64_t e = roff[n0 + k]; e < roff[n0 + k + 1]; ++e) {
            const int s = species[rlist[e]];
#pragma unroll
            for (int t = 0; t < MAX_S; ++t) c[t] += t == s;
        }
#pragma unroll
        for (int s = 0; s < MAX_S; ++s)
            if (s < S) cnt[s * nA + k] = c[s];
    }
    __syncthreads();
    // exclusive scan of cnt in place, HS_ITEMS_THREADS entries at a time
    if (tid == 0) s_carry = 0;
    const int64_t total = S * nA;
    for (int64_t b = 0; b < total; b += HS_ITEMS_THREADS) {
        __syncthreads();
        const int v = b + tid < total ? cnt[b + tid] : 0;
        s_scan[tid] = v;
        __syncthreads();
        for (int off = 1; off < HS_ITEMS_THREADS; off <<= 1) {
            const int u = tid >= off ? s_scan[tid - off] : 0;
            __syncthreads();
            s_scan[tid] += u;
            __syncthreads();
        }
        if (b + tid < total) cnt[b + tid] = s_carry + s_scan[tid] - v;
        __syncthreads();
        if (tid == HS_ITEMS_THREADS - 1) s_carry += s_scan[tid];
    }
    __syncthreads();
    for (int64_t k = tid; k < nA; k += HS_ITEMS_THREADS) {
        int pos[MAX_S];
#pragma unroll
        for (int s = 0; s < MAX_S; ++s) pos[s] = s < S ? cnt[s * nA + k] : 0;
        const int a = (int)(n0 + k);
        for (int64_t e = roff[n0 + k]; e < roff[n0 + k + 1]; ++e) {
            const int i = rlist[e];
            const int s = species[i];
            int p = 0;
#pragma unroll
            for (int t = 0; t < MAX_S; ++t)
                if (t == s) p = pos[t]++;
            for (int c = 0; c < 3; ++c) {
                row_atom[3 * (size_t)p + c] = i;
                row_dir[3 * (size_t)p + c] = 3 * a + c;
            }
        }
    }
}

// ---- extraction ---------------------------------------------------------------------------------------------------------
// entries p0 <= p < p1 (the pattern entries of a chunk's direction atoms): column a = index[1][p], row j = index[0][p];
// direction 3 a + c is slab 3 a + c - dir0 of scratch [n_dir][n_atoms][3], whose row j holds H[(j, y), (a, c)]
__global__ __launch_bounds__(256) void k_hs_extract(int64_t n_atoms, int64_t p0, int64_t p1, const int64_t *__restrict__ index,
                                                    int64_t nnz, int64_t dir0, int64_t n_dir, float *__restrict__ scratch,
                                                    float *__restrict__ blocks)
{
    for (int64_t p = p0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < p1; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = index[p], a = index[nnz + p];
        if (j < 0 || j >= n_atoms || 3 * a - dir0 < 0 || 3 * a + 2 - dir0 >= n_dir) continue;   // (not a chunk entry)
        float v[9];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float *s = scratch + ((size_t)(3 * a + c - dir0) * n_atoms + j) * 3;
#pragma unroll
            for (int y = 0; y < 3; ++y) {
                v[3 * y + c] = s[y];
                s[y] = 0.f;
            }
        }
        float *o = blocks + 9 * (size_t)p;
#pragma unroll
        for (int q = 0; q < 9; ++q) o[q] = v[q];
    }
}

}  // namespace anihip

using namespace anihip;

extern "C" int anihip_hess_sparse_rlist(void *stream, int64_t n_atoms, const int32_t *species, const uint32_t *meta,
                                        const float *ent, const int64_t *roff, int32_t *rcnt, int32_t *rlist)
{
    ANIHIP_REQUIRE(species && meta && ent, "null pointer argument");
    ANIHIP_REQUIRE(roff ? rlist != nullptr : rcnt != nullptr, "count pass needs rcnt, fill pass needs rlist");
    ANIHIP_REQUIRE(n_atoms >= 0 && n_atoms < ((int64_t)1 << 28), "n_atoms must be below 2^28");
    if (n_atoms == 0) return 0;
    int64_t b = (n_atoms + HS_WPB - 1) / HS_WPB;
    if (b > 4096) b = 4096;
    hipLaunchKernelGGL(k_hs_rlist, dim3((unsigned)b), dim3(HS_WPB * WAVE), 0, (hipStream_t)stream, n_atoms, species, meta,
                       (const float4 *)ent, roff, rcnt, rlist);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_hess_sparse_pattern(void *stream, int64_t n_atoms, const int64_t *roff, const int32_t *rlist,
                                          const int64_t *poff, int64_t nnz, int32_t *pcnt, int64_t *index,
                                          uint32_t *status)
{
    ANIHIP_REQUIRE(roff && rlist && status, "null pointer argument");
    ANIHIP_REQUIRE(poff ? index != nullptr : pcnt != nullptr, "count pass needs pcnt, fill pass needs index");
    ANIHIP_REQUIRE(n_atoms >= 0 && nnz >= 0, "negative size");
    if (n_atoms == 0) return 0;
    int64_t b = n_atoms < 8192 ? n_atoms : 8192;
    hipLaunchKernelGGL(k_hs_pattern, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, n_atoms, roff, rlist, poff, nnz,
                       pcnt, index, status);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_hess_sparse_items(void *stream, int32_t num_species, int64_t n0, int64_t n1, const int32_t *species,
                                        const int64_t *roff, const int32_t *rlist, int32_t *scratch, int32_t *row_atom,
                                        int32_t *row_dir)
{
    ANIHIP_REQUIRE(species && roff && rlist && scratch && row_atom && row_dir, "null pointer argument");
    ANIHIP_REQUIRE(num_species >= 1 && num_species <= MAX_S - 1, "num_species must be 1..7");
    ANIHIP_REQUIRE(0 <= n0 && n0 <= n1, "direction atoms n0 .. n1 out of order");
    if (n1 == n0) return 0;
    hipLaunchKernelGGL(k_hs_items, dim3(1), dim3(HS_ITEMS_THREADS), 0, (hipStream_t)stream, n0, n1, (int)num_species, species,
                       roff, rlist, scratch, row_atom, row_dir);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_hess_sparse_extract(void *stream, int64_t n_atoms, int64_t p0, int64_t p1, const int64_t *index,
                                          int64_t nnz, int64_t dir0, int64_t n_dir, float *scratch, float *blocks)
{
    ANIHIP_REQUIRE(index && scratch && blocks, "null pointer argument");
    ANIHIP_REQUIRE(0 <= p0 && p0 <= p1 && p1 <= nnz, "entries p0 .. p1 outside 0 .. nnz");
    if (p1 == p0) return 0;
    int64_t b = (p1 - p0 + 255) / 256;
    if (b > 8192) b = 8192;
    hipLaunchKernelGGL(k_hs_extract, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, n_atoms, p0, p1, index, nnz, dir0,
                       n_dir, scratch, blocks);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}
