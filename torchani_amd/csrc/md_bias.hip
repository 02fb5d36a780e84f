// Biased MD on the batches of md.hip (torchani_amd.md.BatchedDynamics(bias=...)): restraints on collective variables and
// metadynamics, added to the forces held between the evaluation and the kick.  include/anihip.h has the exact definition.
//
//   k_md_bias_hills_entries   one workgroup per (entry, chunk of 1024 hills): the entry's one or two metadynamics CVs, then V,
//                             dV/ds_0 and dV/ds_1 of the chunk by md_block_sum, written to the workspace
//   k_md_bias_apply           one workgroup per entry: the chunk sums added in chunk order, one thread per CV (value, gradient,
//                             restraint), one thread per atom of a CV (the fp64 force sum in CV order, one fp32 rounding)
//   k_md_bias_deposit_hills, k_md_bias_deposit_count   one thread per entry appends its hill, then one per list advances `used`
//   k_md_bias_hills_points    one workgroup per point: V and dV/ds of one list, the chunks summed as above
//
// Everything is fp64 on x = coords + coords_lo; the CV formulas are in md_cv.h, shared with geom_constraints.hip.  No atomics
// on memory and every sum in a fixed order: two calls on the same input are bit-identical, and an entry gives the same bits wherever it sits in the batch.  Tables live in device memory, so
// the kernels check every index they follow: an entry with a table out of range writes its status word and nothing else.
#include "anihip_common.h"
#include "md_cv.h"
#include "md_sums.h"

namespace anihip {

constexpr int BIAS_CVS = ANIHIP_MD_BIAS_MAX_CVS, BIAS_CHUNK = ANIHIP_MD_BIAS_CHUNK;
static_assert(4 * BIAS_CVS <= MD_BLOCK, "k_md_bias_apply has one thread per atom of every CV");

struct BiasArgs {
    int64_t A;
    int32_t n_chunks;   // chunks of the hills kernel's grid
    const float *coords, *coords_lo;
    float *forces;
    double *e_bias, *e_meta, *cv_values, *part;   // part: [C][n_chunks][3]
};

using BiasCv = Cv;   // (md_cv.h)

__device__ __forceinline__ double bias_wrap(double d) { return cv_wrap(d); }

// the CVs and the list of entry c: 0, or the ANIHIP_MD_BIAS_BAD_* bit of the first table that is out of range (then n = 0, g = -1)
__device__ __forceinline__ int bias_entry(const anihip_md_bias &b, int64_t c, int &lo, int &n, int &g)
{
    lo = b.cv_offset[c];
    const int hi = b.cv_offset[c + 1];
    n = 0, g = -1;
    if (lo < 0 || hi < lo || hi > b.n_cvs || hi - lo > BIAS_CVS) return ANIHIP_MD_BIAS_BAD_OFFSET;
    if (b.n_lists > 0) {
        const int l = b.list[c];
        if (l < -1 || l >= b.n_lists) return ANIHIP_MD_BIAS_BAD_LIST;
        if (l >= 0) {
            const int m0 = b.meta_cv[2 * c], m1 = b.meta_cv[2 * c + 1], r = b.rank_in_list[c];
            if (m0 < 0 || m0 >= hi - lo || m1 < -1 || m1 >= hi - lo || m1 == m0 || r < 0 || r >= b.members[l])
                return ANIHIP_MD_BIAS_BAD_LIST;
        }
        g = l;
    }
    n = hi - lo;
    return 0;
}

// kind and atoms of CV r of entry c: the atoms distinct and inside the entry
__device__ __forceinline__ int bias_cv_load(const anihip_md_bias &b, int64_t A, int64_t c, int r, BiasCv &cv)
{
    return cv_load(b.kind, b.atoms, A, c, r, cv) ? 0 : ANIHIP_MD_BIAS_BAD_CV;
}

// s and its gradient on every atom at x = coords + coords_lo (md_cv.h has the formulas)
__device__ __forceinline__ void bias_cv_eval(const BiasArgs &a, BiasCv &cv)
{
    double x[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t at = cv.at[k] < 0 ? cv.at[0] : cv.at[k];
#pragma unroll
        for (int d = 0; d < 3; ++d) x[k][d] = (double)a.coords[3 * at + d] + (double)a.coords_lo[3 * at + d];
    }
    cv_eval(x, cv);
}

__device__ __forceinline__ int bias_hills_held(const anihip_md_bias &b, int g, int bound)
{
    return min(min(max(b.used[g], 0), b.capacity), bound);
}

// V, dV/ds_0, dV/ds_1 of the hills j BIAS_CHUNK .. min(n_hills, (j + 1) BIAS_CHUNK) - 1 of list g at s: thread t adds the hills
// t, t + 256, ... in that order; the sum is in thread 0.  Called by the whole workgroup.
__device__ __forceinline__ void bias_chunk(const anihip_md_bias &b, int g, int n_hills, int j, int nd, const double (&s)[2],
                                           const double (&is2)[2], const bool (&periodic)[2], double (&sum)[3])
{
    const int64_t cap = b.capacity;
    const double *c0 = b.centers + (int64_t)g * 2 * cap, *c1 = c0 + cap, *w = b.heights + (int64_t)g * cap;
    const int end = min(n_hills, (j + 1) * BIAS_CHUNK);
    sum[0] = sum[1] = sum[2] = 0.0;
    for (int h = j * BIAS_CHUNK + (int)threadIdx.x; h < end; h += MD_BLOCK) {
        double d0 = s[0] - c0[h], d1 = 0.0;
        if (periodic[0]) d0 = bias_wrap(d0);
        double arg = d0 * d0 * is2[0];
        if (nd == 2) {
            d1 = s[1] - c1[h];
            if (periodic[1]) d1 = bias_wrap(d1);
            arg += d1 * d1 * is2[1];
        }
        const double gh = w[h] * exp(-0.5 * arg);
        sum[0] += gh, sum[1] -= gh * d0 * is2[0], sum[2] -= gh * d1 * is2[1];
    }
    md_block_sum<3>(sum);
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_bias_hills_entries(BiasArgs a, anihip_md_bias b)
{
    const int64_t c = blockIdx.x / a.n_chunks;
    const int j = blockIdx.x % a.n_chunks;
    int lo, n, g;
    if (bias_entry(b, c, lo, n, g) || g < 0) return;   // (the same for every thread; k_md_bias_apply reports it)
    const int n_hills = bias_hills_held(b, g, a.n_chunks * BIAS_CHUNK);
    if (j * BIAS_CHUNK >= n_hills) return;
    __shared__ double sh_s[2];
    __shared__ int sh_kind[2];
    const int m[2] = {b.meta_cv[2 * c], b.meta_cv[2 * c + 1]};
    if (threadIdx.x < 2) {
        const int t = threadIdx.x, mt = t ? m[1] : m[0];
        sh_s[t] = 0.0, sh_kind[t] = -1;
        BiasCv cv;
        if (mt >= 0 && bias_cv_load(b, a.A, c, lo + mt, cv) == 0) {
            bias_cv_eval(a, cv);
            sh_s[t] = cv.s, sh_kind[t] = cv.kind;
        }
    }
    __syncthreads();
    if (sh_kind[0] < 0 || (m[1] >= 0 && sh_kind[1] < 0)) return;   // a bad CV: the entry moves nothing
    const double s[2] = {sh_s[0], sh_s[1]}, is2[2] = {b.inv_sigma2[2 * c], b.inv_sigma2[2 * c + 1]};
    const bool periodic[2] = {sh_kind[0] == ANIHIP_MD_CV_DIHEDRAL, sh_kind[1] == ANIHIP_MD_CV_DIHEDRAL};
    double sum[3];
    bias_chunk(b, g, n_hills, j, m[1] >= 0 ? 2 : 1, s, is2, periodic, sum);
    if (threadIdx.x == 0) {
        double *dst = a.part + (c * a.n_chunks + j) * 3;
        dst[0] = sum[0], dst[1] = sum[1], dst[2] = sum[2];
    }
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_bias_apply(BiasArgs a, anihip_md_bias b)
{
    const int64_t c = blockIdx.x;
    const int t = threadIdx.x;
    __shared__ int sh_bad, sh_n[BIAS_CVS];
    __shared__ int32_t sh_at[BIAS_CVS][4];
    __shared__ double sh_s[BIAS_CVS], sh_g[BIAS_CVS][4][3], sh_E[BIAS_CVS], sh_dE[BIAS_CVS], sh_hills[3];
    int lo, n, g;
    const int bad_entry = bias_entry(b, c, lo, n, g);   // (the same for every thread)
    if (t == 0) sh_bad = bad_entry;
    __syncthreads();
    BiasCv cv;
    if (t < n) {
        const int bad = bias_cv_load(b, a.A, c, lo + t, cv);
        if (bad) atomicOr(&sh_bad, bad);   // (on LDS, an integer: the order does not matter)
    }
    __syncthreads();
    if (sh_bad) {
        if (t == 0) b.status[c] = sh_bad;
        return;
    }
    if (t < n) {
        bias_cv_eval(a, cv);
        sh_s[t] = cv.s, sh_n[t] = cv.n;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sh_at[t][k] = cv.at[k];
#pragma unroll
            for (int d = 0; d < 3; ++d) sh_g[t][k][d] = cv.g[k][d];
        }
    }
    if (t == 0) {   // the chunk sums of the hills kernel, in chunk order
        double V = 0.0, d0 = 0.0, d1 = 0.0;
        if (g >= 0) {
            const int chunks = (bias_hills_held(b, g, a.n_chunks * BIAS_CHUNK) + BIAS_CHUNK - 1) / BIAS_CHUNK;
            const double *src = a.part + c * a.n_chunks * 3;
            for (int j = 0; j < chunks; ++j) V += src[3 * j], d0 += src[3 * j + 1], d1 += src[3 * j + 2];
        }
        sh_hills[0] = V, sh_hills[1] = d0, sh_hills[2] = d1;
    }
    __syncthreads();
    if (t < n) {
        const double *res = b.restraint + 3 * (int64_t)(lo + t);
        double d = cv.s - res[0];
        if (cv.kind == ANIHIP_MD_CV_DIHEDRAL) d = bias_wrap(d);
        const double e = fmax(0.0, fabs(d) - res[2]);
        double dE = copysign(res[1] * e, d);
        if (g >= 0) {
            if (t == b.meta_cv[2 * c]) dE += sh_hills[1];
            if (t == b.meta_cv[2 * c + 1]) dE += sh_hills[2];
        }
        sh_E[t] = 0.5 * res[1] * e * e, sh_dE[t] = dE;
        a.cv_values[lo + t] = cv.s;
    }
    __syncthreads();
    // one thread per (CV, slot); the first pair that names an atom adds every pair of that atom, in CV order
    if (t < 4 * n && (t & 3) < sh_n[t >> 2]) {
        const int32_t at = sh_at[t >> 2][t & 3];
        bool first = true;
        for (int p = 0; p < t; ++p)
            if ((p & 3) < sh_n[p >> 2] && sh_at[p >> 2][p & 3] == at) first = false;
        if (first) {
            double f[3] = {0.0, 0.0, 0.0};
            for (int p = t; p < 4 * n; ++p)
                if ((p & 3) < sh_n[p >> 2] && sh_at[p >> 2][p & 3] == at) {
#pragma unroll
                    for (int d = 0; d < 3; ++d) f[d] += -sh_dE[p >> 2] * sh_g[p >> 2][p & 3][d];
                }
            float *dst = a.forces + 3 * (int64_t)at;
#pragma unroll
            for (int d = 0; d < 3; ++d) dst[d] = (float)((double)dst[d] + f[d]);
        }
    }
    if (t == 0) {
        double E = 0.0;
        for (int r = 0; r < n; ++r) E += sh_E[r];
        a.e_bias[c] = E + sh_hills[0], a.e_meta[c] = sh_hills[0];
        b.status[c] = 0;
    }
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_bias_deposit_hills(anihip_md_bias b, const float *kT, const double *cv_values,
                                                                   const double *meta_energies)
{
    const int64_t c = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x;
    if (c >= b.n_entries) return;
    int lo, n, g;
    if (bias_entry(b, c, lo, n, g) || g < 0 || b.status[c] != 0) return;   // (status: what k_md_bias_apply found)
    const int held = b.used[g], m = b.members[g];   // (m >= 1 and rank < m: bias_entry)
    if (held < 0 || held > b.capacity - m) return;   // it would not fit: k_md_bias_deposit_count counts the members as dropped
    const int64_t cap = b.capacity, h = held + b.rank_in_list[c];
    const int m1 = b.meta_cv[2 * c + 1];
    b.centers[((int64_t)g * 2) * cap + h] = cv_values[lo + b.meta_cv[2 * c]];
    b.centers[((int64_t)g * 2 + 1) * cap + h] = m1 >= 0 ? cv_values[lo + m1] : 0.0;
    double w = b.height[c];
    const double gamma = b.bias_factor[g];
    if (gamma > 0.0 && kT) w = w * exp(-meta_energies[c] / ((gamma - 1.0) * (double)kT[c]));
    b.heights[(int64_t)g * cap + h] = w;
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_bias_deposit_count(anihip_md_bias b)
{
    const int g = blockIdx.x * MD_BLOCK + threadIdx.x;
    if (g >= b.n_lists) return;
    const int held = b.used[g], m = b.members[g];
    if (m < 1) return;
    if (held < 0 || held > b.capacity - m) b.dropped[g] += m;
    else b.used[g] = held + m;
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_bias_hills_points(anihip_md_bias b, int g, const double *values, double *out_V,
                                                                  double *out_dV)
{
    const int64_t p = blockIdx.x;
    const int64_t c = b.list_entry[g];
    int lo = 0, n = 0, l = -1, kind[2] = {-1, -1}, m[2] = {-1, -1};
    bool ok = c >= 0 && c < b.n_entries && bias_entry(b, c, lo, n, l) == 0 && l == g;
    if (ok) {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            m[d] = b.meta_cv[2 * c + d];
            if (m[d] >= 0) kind[d] = b.kind[lo + m[d]];
            if (m[d] >= 0 && (kind[d] < ANIHIP_MD_CV_DISTANCE || kind[d] > ANIHIP_MD_CV_DIHEDRAL)) ok = false;
        }
    }
    if (!ok) {   // (the same for every thread)
        if (threadIdx.x == 0) out_V[p] = out_dV[2 * p] = out_dV[2 * p + 1] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const double s[2] = {values[2 * p], values[2 * p + 1]}, is2[2] = {b.inv_sigma2[2 * c], b.inv_sigma2[2 * c + 1]};
    const bool periodic[2] = {kind[0] == ANIHIP_MD_CV_DIHEDRAL, kind[1] == ANIHIP_MD_CV_DIHEDRAL};
    const int n_hills = bias_hills_held(b, g, b.capacity), chunks = (n_hills + BIAS_CHUNK - 1) / BIAS_CHUNK;
    double tot[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < chunks; ++j) {
        double sum[3];
        bias_chunk(b, g, n_hills, j, m[1] >= 0 ? 2 : 1, s, is2, periodic, sum);
        if (threadIdx.x == 0) tot[0] += sum[0], tot[1] += sum[1], tot[2] += sum[2];
        __syncthreads();   // (md_block_sum's LDS is read by thread 0 until here)
    }
    if (threadIdx.x == 0) out_V[p] = tot[0], out_dV[2 * p] = tot[1], out_dV[2 * p + 1] = tot[2];
}

// what the host can see of the tables; the chunks of the hills kernel's grid
static int bias_args(const anihip_md_params *params, const anihip_md_bias *bias, int32_t &n_chunks)
{
    ANIHIP_REQUIRE(bias, "null pointer argument");
    const anihip_md_bias &b = *bias;
    ANIHIP_REQUIRE(b.n_entries >= 1 && b.n_cvs >= 0 && b.n_lists >= 0, "n_entries must be >= 1, n_cvs and n_lists >= 0");
    if (params) {
        ANIHIP_REQUIRE(params->n_mol >= 1 && params->atoms_per_mol >= 1, "n_mol and atoms_per_mol must be >= 1");
        ANIHIP_REQUIRE((int64_t)params->n_mol * params->atoms_per_mol < ((int64_t)1 << 31), "n_mol x atoms_per_mol must stay below 2^31");
        ANIHIP_REQUIRE(b.n_entries == params->n_mol, "bias tables of %d entries for a batch of %d", b.n_entries, params->n_mol);
    }
    ANIHIP_REQUIRE(b.cv_offset && b.status, "null pointer in the bias tables");
    ANIHIP_REQUIRE(b.n_cvs == 0 || (b.kind && b.atoms && b.restraint), "null pointer in the CV tables");
    n_chunks = 0;
    if (b.n_lists == 0) return 0;
    ANIHIP_REQUIRE(b.capacity >= 1 && b.capacity <= (1 << 30), "capacity must be in 1 .. 2^30, got %d", b.capacity);
    ANIHIP_REQUIRE(b.hills_bound >= 0 && b.hills_bound <= b.capacity, "hills_bound must be in 0 .. capacity, got %d", b.hills_bound);
    ANIHIP_REQUIRE(b.meta_cv && b.inv_sigma2 && b.height && b.list && b.rank_in_list && b.members && b.list_entry && b.bias_factor
                       && b.used && b.dropped && b.centers && b.heights,
                   "null pointer in the metadynamics tables");
    n_chunks = ((b.hills_bound ? b.hills_bound : b.capacity) + BIAS_CHUNK - 1) / BIAS_CHUNK;
    ANIHIP_REQUIRE((int64_t)b.n_entries * n_chunks < ((int64_t)1 << 31), "entries x chunks of hills must stay below 2^31");
    return 0;
}

}  // namespace anihip

using namespace anihip;

extern "C" size_t anihip_md_bias_workspace_bytes(const anihip_md_params *params, const anihip_md_bias *bias)
{
    if (!params || !bias || params->n_mol < 1 || bias->n_lists < 0 || bias->capacity < 0 || bias->capacity > (1 << 30)) {
        set_error("anihip_md_bias_workspace_bytes: n_mol must be >= 1, n_lists >= 0 and capacity in 0 .. 2^30");
        return 0;
    }
    if (bias->n_lists == 0) return 0;
    return (size_t)params->n_mol * (size_t)((bias->capacity + BIAS_CHUNK - 1) / BIAS_CHUNK) * 3 * sizeof(double);
}

extern "C" int anihip_md_bias_apply(void *stream, const anihip_md_params *params, const anihip_md_bias *bias, const float *coords,
                                    const float *coords_lo, float *forces, double *bias_energies, double *meta_energies,
                                    double *cv_values, void *workspace, size_t workspace_bytes)
{
    ANIHIP_REQUIRE(params, "null pointer argument");
    BiasArgs a{};
    if (int rc = bias_args(params, bias, a.n_chunks)) return rc;
    ANIHIP_REQUIRE(coords && coords_lo && forces && bias_energies && meta_energies && (cv_values || bias->n_cvs == 0),
                   "null pointer argument");
    const size_t need = anihip_md_bias_workspace_bytes(params, bias);
    ANIHIP_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "workspace holds %zu bytes, %zu needed", workspace_bytes, need);
    a.A = params->atoms_per_mol;
    a.coords = coords, a.coords_lo = coords_lo, a.forces = forces;
    a.e_bias = bias_energies, a.e_meta = meta_energies, a.cv_values = cv_values, a.part = (double *)workspace;
    hipStream_t s = (hipStream_t)stream;
    if (bias->n_lists > 0) {
        hipLaunchKernelGGL(k_md_bias_hills_entries, dim3((unsigned)(params->n_mol * a.n_chunks)), dim3(MD_BLOCK), 0, s, a, *bias);
        ANIHIP_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_md_bias_apply, dim3((unsigned)params->n_mol), dim3(MD_BLOCK), 0, s, a, *bias);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_md_bias_deposit(void *stream, const anihip_md_params *params, const anihip_md_bias *bias, const float *kT,
                                      const double *cv_values, const double *meta_energies)
{
    ANIHIP_REQUIRE(params, "null pointer argument");
    int32_t n_chunks;
    if (int rc = bias_args(params, bias, n_chunks)) return rc;
    if (bias->n_lists == 0) return 0;
    ANIHIP_REQUIRE(cv_values && meta_energies, "null pointer argument");
    // (bias_factor lives on the device: with kT = NULL a well-tempered list deposits the plain height)
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_md_bias_deposit_hills, dim3((unsigned)((params->n_mol + MD_BLOCK - 1) / MD_BLOCK)), dim3(MD_BLOCK), 0, s,
                       *bias, kT, cv_values, meta_energies);
    ANIHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_md_bias_deposit_count, dim3((unsigned)((bias->n_lists + MD_BLOCK - 1) / MD_BLOCK)), dim3(MD_BLOCK), 0, s,
                       *bias);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_md_bias_hills(void *stream, const anihip_md_bias *bias, int32_t list, int64_t n_points, const double *values,
                                    double *out_V, double *out_dV)
{
    int32_t n_chunks;
    if (int rc = bias_args(nullptr, bias, n_chunks)) return rc;
    ANIHIP_REQUIRE(list >= 0 && list < bias->n_lists, "list %d is outside 0 .. n_lists - 1 = %d", list, bias->n_lists - 1);
    ANIHIP_REQUIRE(n_points >= 0 && n_points < ((int64_t)1 << 31), "n_points out of range");
    if (n_points == 0) return 0;
    ANIHIP_REQUIRE(values && out_V && out_dV, "null pointer argument");
    hipLaunchKernelGGL(k_md_bias_hills_points, dim3((unsigned)n_points), dim3(MD_BLOCK), 0, (hipStream_t)stream, *bias, (int)list,
                       values, out_V, out_dV);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}
