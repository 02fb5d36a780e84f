// Holonomic constraints on internal coordinates for the batched L-BFGS of lbfgs.hip (torchani_amd.geomopt.GeometryOptimizer(
// constraints=...)): distances, angles and dihedrals held at targets, the way ASE's FixInternals works with its LBFGS.
// include/anihip.h has the exact definition.
//
//   k_geom_project   f <- f - J^T lambda with (J J^T) lambda = J f: the forces an optimizer may follow without leaving the
//                    constraint surface to first order; lambda is the slope of the relaxed energy along the targets
//   k_geom_restore   Newton iteration back onto the targets by the minimum-norm correction x <- x - J^T mu, (J J^T) mu = r
//
// One wave per entry (a workgroup of 64 threads): constraint k on lane k, the element (a, b) of G = J J^T on lane 8 a + b, one
// lane per (constraint, slot) for what is read and written per atom, the Cholesky factorization on lane 0; gradients,
// positions and multipliers in LDS.  Everything is fp64 on the fp32 coords read exactly.  No atomics on memory and every sum
// in a fixed order: two calls on the same input are bit-identical, and an entry gives the same bits wherever it sits in the
// batch.  Tables live in device memory, so the kernels check every index they follow: an entry with a table out of range ORs
// ANIHIP_GEOM_BAD_TABLE into its status word and writes nothing else; so does a singular one with ANIHIP_GEOM_SINGULAR.
#include "anihip_common.h"
#include "md_cv.h"

namespace anihip {

constexpr int GC_MAX = ANIHIP_GEOM_MAX_CONSTRAINTS, GC_SLOTS = 4 * GC_MAX;
constexpr double GC_PIVOT = 1e-12;   // a pivot <= GC_PIVOT x the largest diagonal element of G is singular
static_assert(GC_MAX * GC_MAX <= WAVE, "one lane per element of G");

struct GeomShared {
    int n[GC_MAX], own[GC_SLOTS], flag;
    int32_t at[GC_SLOTS];                       // the atom of slot 4 k + j, -1 for a slot the kind does not use
    double w[GC_SLOTS];                         // 1 for a free atom, 0 for a fixed one
    double x[GC_SLOTS][3];                      // positions, held at the first slot that names the atom (own)
    double g[GC_SLOTS][3];                      // J: the gradient of constraint k on slot j, zeroed on fixed atoms
    double s[GC_MAX], rhs[GC_MAX], sol[GC_MAX], G[GC_MAX][GC_MAX];
};

// Loads and checks the tables of entry c.  Returns the number of constraints, 0 for none, -1 for a broken table.  Fills n, at,
// own, w and x (from coords) of sh.  Called by the whole wave; ends with a barrier.
__device__ __forceinline__ int geom_load(const anihip_geom_constraints &t, int64_t A, int64_t c, const uint8_t *active,
                                         const float *coords, GeomShared &sh, Cv &cv, int &lo)
{
    const int lane = threadIdx.x;
    lo = t.offset[c];
    const int hi = t.offset[c + 1];
    if (lo < 0 || hi < lo || hi > t.n_constraints || hi - lo > GC_MAX) return -1;   // (the same for every lane)
    const int n = hi - lo;
    if (n == 0) return 0;
    if (lane == 0) sh.flag = 0;
    __syncthreads();
    if (lane < n) {
        if (!cv_load(t.kind, t.atoms, A, c, lo + lane, cv)) {
            sh.flag = 1;   // (every writer stores the same value)
        } else {
            sh.n[lane] = cv.n;
#pragma unroll
            for (int j = 0; j < 4; ++j) sh.at[4 * lane + j] = cv.at[j];
        }
    }
    __syncthreads();
    if (sh.flag) return -1;
    if (lane < 4 * n && sh.at[lane] >= 0) {
        const int32_t at = sh.at[lane];
        int own = lane;
        for (int p = lane - 1; p >= 0; --p)
            if (sh.at[p] == at) own = p;
        sh.own[lane] = own;
        sh.w[lane] = active[at] != 0 ? 1.0 : 0.0;
        if (own == lane) {
#pragma unroll
            for (int d = 0; d < 3; ++d) sh.x[lane][d] = (double)coords[3 * (int64_t)at + d];
        }
    }
    __syncthreads();
    return n;
}

// s and J of every constraint at sh.x, then G = J J^T.  Called by the whole wave; ends with a barrier.
__device__ __forceinline__ void geom_eval(int n, GeomShared &sh, Cv &cv)
{
    const int lane = threadIdx.x;
    if (lane < n) {
        double x[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = 4 * lane + (j < cv.n ? j : 0);
#pragma unroll
            for (int d = 0; d < 3; ++d) x[j][d] = sh.x[sh.own[p]][d];
        }
        cv_eval(x, cv);
        sh.s[lane] = cv.s;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double w = j < cv.n ? sh.w[4 * lane + j] : 0.0;
#pragma unroll
            for (int d = 0; d < 3; ++d) sh.g[4 * lane + j][d] = w != 0.0 ? cv.g[j][d] : 0.0;
        }
    }
    __syncthreads();
    const int a = lane >> 3, b = lane & 7;
    if (a < n && b < n) {
        double acc = 0.0;
        for (int i = 0; i < sh.n[a]; ++i)
            for (int j = 0; j < sh.n[b]; ++j)
                if (sh.at[4 * a + i] == sh.at[4 * b + j]) acc += dot3(sh.g[4 * a + i], sh.g[4 * b + j]);
        sh.G[a][b] = acc;
    }
    __syncthreads();
}

// G sol = rhs by Cholesky in the stored order, on lane 0 (G is overwritten by its factor); sh.flag = 1 for a singular G.
// Called by the whole wave; ends with a barrier.
__device__ __forceinline__ void geom_solve(int n, GeomShared &sh)
{
    if (threadIdx.x == 0) {
        double top = 0.0;
        for (int k = 0; k < n; ++k) top = fmax(top, sh.G[k][k]);   // (fmax drops a NaN: the pivot test catches it)
        const double least = GC_PIVOT * top;
        int singular = 0;
        for (int j = 0; j < n && !singular; ++j) {
            double d = sh.G[j][j];
            for (int k = 0; k < j; ++k) d -= sh.G[j][k] * sh.G[j][k];
            if (!(d > least) || isinf(d)) {   // (also NaN and infinity: collinear atoms of an angle or dihedral)
                singular = 1;
                break;
            }
            const double l = sqrt(d);
            sh.G[j][j] = l;
            for (int i = j + 1; i < n; ++i) {
                double v = sh.G[i][j];
                for (int k = 0; k < j; ++k) v -= sh.G[i][k] * sh.G[j][k];
                sh.G[i][j] = v / l;
            }
        }
        if (!singular) {
            for (int i = 0; i < n; ++i) {
                double v = sh.rhs[i];
                for (int k = 0; k < i; ++k) v -= sh.G[i][k] * sh.sol[k];
                sh.sol[i] = v / sh.G[i][i];
            }
            for (int i = n - 1; i >= 0; --i) {
                double v = sh.sol[i];
                for (int k = i + 1; k < n; ++k) v -= sh.G[k][i] * sh.sol[k];
                sh.sol[i] = v / sh.G[i][i];
                if (!isfinite(sh.sol[i])) singular = 1;
            }
        }
        sh.flag = singular;
    }
    __syncthreads();
}

// sum over the slots q >= p that name the atom of slot p, in constraint order, of sol_k J_q
__device__ __forceinline__ void geom_atom_sum(int n, int p, const GeomShared &sh, double (&sum)[3])
{
    sum[0] = sum[1] = sum[2] = 0.0;
    const int32_t at = sh.at[p];
    for (int q = p; q < 4 * n; ++q)
        if (sh.at[q] == at) {
#pragma unroll
            for (int d = 0; d < 3; ++d) sum[d] += sh.sol[q >> 2] * sh.g[q][d];
        }
}

__global__ __launch_bounds__(WAVE) void k_geom_project(anihip_geom_constraints t, int64_t A, const uint8_t *active,
                                                       const float *coords, float *forces)
{
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    __shared__ GeomShared sh;
    Cv cv;
    int lo;
    const int n = geom_load(t, A, c, active, coords, sh, cv, lo);
    if (n == 0) return;
    if (n < 0) {
        if (lane == 0) t.status[c] |= ANIHIP_GEOM_BAD_TABLE;
        return;
    }
    geom_eval(n, sh, cv);
    if (lane < n) {   // (J f)_k, the slots in order
        double acc = 0.0;
        for (int j = 0; j < sh.n[lane]; ++j) {
            const float *f = forces + 3 * (int64_t)sh.at[4 * lane + j];
            const double fd[3] = {(double)f[0], (double)f[1], (double)f[2]};
            acc += dot3(sh.g[4 * lane + j], fd);
        }
        sh.rhs[lane] = acc;
    }
    __syncthreads();
    geom_solve(n, sh);
    if (sh.flag) {
        if (lane == 0) t.status[c] |= ANIHIP_GEOM_SINGULAR;
        return;
    }
    if (lane < 4 * n && sh.at[lane] >= 0 && sh.own[lane] == lane) {
        double sum[3];
        geom_atom_sum(n, lane, sh, sum);
        float *f = forces + 3 * (int64_t)sh.at[lane];
#pragma unroll
        for (int d = 0; d < 3; ++d) f[d] = (float)((double)f[d] - sum[d]);
    }
    if (lane < n) t.multipliers[lo + lane] = sh.sol[lane], t.values[lo + lane] = sh.s[lane];
}

__global__ __launch_bounds__(WAVE) void k_geom_restore(anihip_geom_constraints t, int64_t A, const uint8_t *active, float *coords)
{
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    __shared__ GeomShared sh;
    __shared__ double sh_worst;
    Cv cv;
    int lo;
    const int n = geom_load(t, A, c, active, coords, sh, cv, lo);
    if (n == 0) return;
    if (n < 0) {
        if (lane == 0) t.status[c] |= ANIHIP_GEOM_BAD_TABLE;
        return;
    }
    const double target = lane < n ? t.target[lo + lane] : 0.0;
    int it = 0;
    for (;;) {
        geom_eval(n, sh, cv);
        if (lane < n) {
            double r = cv.s - target;
            if (cv.kind == ANIHIP_MD_CV_DIHEDRAL) r = cv_wrap(r);
            sh.rhs[lane] = r;
        }
        __syncthreads();
        if (lane == 0) {
            double worst = 0.0;
            for (int k = 0; k < n; ++k) worst = fabs(sh.rhs[k]) > worst || sh.rhs[k] != sh.rhs[k] ? fabs(sh.rhs[k]) : worst;
            sh_worst = worst;
        }
        __syncthreads();
        if (sh_worst <= t.tolerance) break;   // (LDS: the same for every lane)
        if (it == t.max_iterations) {
            if (lane == 0) t.status[c] |= ANIHIP_GEOM_NOT_CONVERGED;
            return;
        }
        geom_solve(n, sh);
        if (sh.flag) {
            if (lane == 0) t.status[c] |= ANIHIP_GEOM_SINGULAR;
            return;
        }
        if (lane < 4 * n && sh.at[lane] >= 0 && sh.own[lane] == lane) {
            double sum[3];
            geom_atom_sum(n, lane, sh, sum);
#pragma unroll
            for (int d = 0; d < 3; ++d) sh.x[lane][d] -= sum[d];
        }
        ++it;
        __syncthreads();
    }
    if (it > 0) {   // the fp32 coordinates, and the values at them
        if (lane < 4 * n && sh.at[lane] >= 0 && sh.own[lane] == lane) {
            float *x = coords + 3 * (int64_t)sh.at[lane];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float r = (float)sh.x[lane][d];
                x[d] = r, sh.x[lane][d] = (double)r;
            }
        }
        __syncthreads();
        geom_eval(n, sh, cv);
    }
    if (lane < n) t.values[lo + lane] = sh.s[lane];
    if (lane == 0) t.iterations[c] = it;
}

static int geom_args(int64_t n_mol, int64_t atoms_per_mol, const anihip_geom_constraints *tables)
{
    ANIHIP_REQUIRE(tables, "null pointer argument");
    const anihip_geom_constraints &t = *tables;
    ANIHIP_REQUIRE(n_mol >= 1 && atoms_per_mol >= 1, "n_mol and atoms_per_mol must be >= 1");
    ANIHIP_REQUIRE(n_mol * atoms_per_mol < ((int64_t)1 << 31), "n_mol x atoms_per_mol must stay below 2^31");
    ANIHIP_REQUIRE(t.n_constraints >= 0, "n_constraints must be >= 0, got %d", t.n_constraints);
    ANIHIP_REQUIRE(t.tolerance > 0.0, "tolerance must be > 0, got %g", t.tolerance);
    ANIHIP_REQUIRE(t.max_iterations >= 1, "max_iterations must be >= 1, got %d", t.max_iterations);
    ANIHIP_REQUIRE(t.offset && t.iterations && t.status, "null pointer in the constraint tables");
    ANIHIP_REQUIRE(t.n_constraints == 0 || (t.kind && t.atoms && t.target && t.values && t.multipliers),
                   "null pointer in the constraint tables");
    return 0;
}

}  // namespace anihip

using namespace anihip;

extern "C" int anihip_geom_constraints_project(void *stream, int64_t n_mol, int64_t atoms_per_mol,
                                               const anihip_geom_constraints *tables, const uint8_t *active, const float *coords,
                                               float *forces)
{
    if (int rc = geom_args(n_mol, atoms_per_mol, tables)) return rc;
    ANIHIP_REQUIRE(active && coords && forces, "null pointer argument");
    if (tables->n_constraints == 0) return 0;
    hipLaunchKernelGGL(k_geom_project, dim3((unsigned)n_mol), dim3(WAVE), 0, (hipStream_t)stream, *tables, atoms_per_mol, active,
                       coords, forces);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_geom_constraints_restore(void *stream, int64_t n_mol, int64_t atoms_per_mol,
                                               const anihip_geom_constraints *tables, const uint8_t *active, float *coords)
{
    if (int rc = geom_args(n_mol, atoms_per_mol, tables)) return rc;
    ANIHIP_REQUIRE(active && coords, "null pointer argument");
    if (tables->n_constraints == 0) return 0;
    hipLaunchKernelGGL(k_geom_restore, dim3((unsigned)n_mol), dim3(WAVE), 0, (hipStream_t)stream, *tables, atoms_per_mol, active,
                       coords);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}
