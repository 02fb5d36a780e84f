// Molecular-dynamics integrator of batches of molecules (torchani_amd.md.BatchedDynamics): velocity Verlet (NVE) and Langevin
// dynamics in the BAOAB splitting (Leimkuhler and Matthews 2013), every molecule with a temperature and a friction of its own.
// A step is   anihip_md_drift (B A [O A])  ->  energies and forces at the new coordinates  ->  anihip_md_kick (B, kinetic energy):
//
//   k_md_drift     one thread per atom: v += dt/2 f / m;  NVE x += dt v;  Langevin x += dt/2 v, v = c1 v + sigma xi, x += dt/2 v
//   k_md_kick      one thread per atom: v += dt/2 f / m, and the fp64 kinetic energy of each 256-atom chunk
//   k_md_sum       one workgroup per molecule: the chunk sums added in chunk order (only for molecules of more than one chunk)
//   k_md_momentum, k_md_sum, k_md_sub_vcm   anihip_md_remove_drift: sum m v and sum m per chunk, per molecule, then v -= v_cm
//   k_md_barostat_cell, k_md_barostat_scale   anihip_md_barostat (stochastic cell rescaling): one thread per molecule draws the
//                  volume move and rescales the cell, then one thread per atom rescales positions and velocities, all in fp64
//   k_md_constrain<mode, atoms, constraints>   one thread per cluster of bond-length constraints (SHAKE / RATTLE in fp64, the cluster staged in LDS):
//                  the drift, the kick or the velocity projection alone of the atoms that clusters own (active == 2), which
//                  k_md_drift and the kick of k_md_kick skip
//   k_md_group_clusters, k_md_group_sum, k_md_group_total   anihip_md_group_terms: the centre-of-mass kinetic energy and the
//                  internal virial of the scaling groups (constraint clusters and free atoms), per cluster, chunk and molecule
//   k_md_barostat_groups_cell, k_md_barostat_groups_free, k_md_barostat_groups_move   anihip_md_barostat_groups (molecular cell
//                  rescaling): the volume move from the molecular pressure, free atoms rescaled, clusters translated rigidly
//   k_md_rp_drift, k_md_rp_estimators   anihip_md_rp_drift / anihip_md_rp_estimators (ring polymers over the beads of a batch):
//                  B, the exact free ring-polymer propagation in normal modes with the PILE thermostat on them, one thread per
//                  (mode, atom, component); the spring energy, the centroid-virial sum and the centroids of every polymer
//   k_md_exchange_pairs, k_md_exchange_scale   anihip_md_exchange (temperature replica exchange between the entries of a batch):
//                  one thread per pair of neighboring rungs decides the swap of their temperatures and writes the tables, then
//                  one thread per atom rescales the velocities of the entries that changed rung
//
// Positions are pairs of floats, coords + coords_lo: every `x +=` is a two-sum, so a step far below one ulp of the coordinate
// is not lost, and coords (what the engine reads) is the fp32 nearest to the pair.  The noise xi is a pure function of (seed,
// step, replica id, atom index): Philox4x32-10 and Box-Muller (md_normals), the same for a replica wherever it sits in the batch.
// No atomics and every sum in a fixed order: trajectories are bit-identical run to run for bit-identical forces.
#include <vector>

#include "anihip_common.h"
#include "md_sums.h"

namespace anihip {

struct MdArgs {
    int64_t A, Gc;
    int langevin;
    float dt, hdt;
    double dtd;
    uint32_t key0, key1, step0, step1;
    const uint8_t *active;
    const float *inv_mass, *mass, *kT, *friction, *forces;
    const int64_t *replica_ids;
    float *coords, *coords_lo, *vel;
    double *part, *out;   // per-chunk sums [C][Gc][W] and per-molecule sums [C][W]
};

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ k0, c[1] = lo1, c[2] = hi0 ^ c[3] ^ k1, c[3] = lo0;
}

// Philox4x32-10 (Salmon et al. 2011), the counter replaced by its output
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}

// uniform in (0, 1) on a grid of 2^-24, exact in fp32
__device__ __forceinline__ float md_uniform(uint32_t u) { return ((float)(u >> 9) + 0.5f) * 0x1p-23f; }

// the three normal variates of (atom, replica, step): precise logf / sincospif (fast __logf near 1 would cost ~1e-3 in xi)
__device__ __forceinline__ void md_normals(const MdArgs &a, uint32_t atom, uint32_t replica, float (&xi)[3])
{
    uint32_t c[4] = {atom, replica, a.step0, a.step1};
    philox4x32_10(c, a.key0, a.key1);
    const float r0 = sqrtf(-2.f * logf(md_uniform(c[0]))), r1 = sqrtf(-2.f * logf(md_uniform(c[2])));
    float s, co;
    sincospif(2.f * md_uniform(c[1]), &s, &co);
    xi[0] = r0 * co, xi[1] = r0 * s, xi[2] = r1 * cospif(2.f * md_uniform(c[3]));
}

__device__ __forceinline__ uint32_t md_replica(const MdArgs &a, int64_t c)
{
    return a.replica_ids ? (uint32_t)a.replica_ids[c] : (uint32_t)c;
}

// (x, lo) += d: the sum of the three is kept in two floats, x the one nearest to it (Knuth's two-sum: no assumption on
// the magnitudes, so it holds for an atom near the origin too)
__device__ __forceinline__ void md_two_add(float &x, float &lo, float d)
{
    const float t = lo + d, s = x + t, bb = s - x;
    lo = (x - (s - bb)) + (t - bb);
    x = s;
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_noise(MdArgs a, float *out)
{
    const int64_t c = blockIdx.x / a.Gc, i = (blockIdx.x % a.Gc) * MD_BLOCK + threadIdx.x;
    if (i >= a.A) return;
    float xi[3];
    md_normals(a, (uint32_t)i, md_replica(a, c), xi);
    float *o = out + 3 * (c * a.A + i);
    o[0] = xi[0], o[1] = xi[1], o[2] = xi[2];
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_drift(MdArgs a)
{
    const int64_t c = blockIdx.x / a.Gc, i = (blockIdx.x % a.Gc) * MD_BLOCK + threadIdx.x;
    if (i >= a.A) return;
    const int64_t at = c * a.A + i;
    float *v = a.vel + 3 * at;
    if (!a.active[at]) {
        v[0] = v[1] = v[2] = 0.f;
        return;
    }
    if (a.active[at] == ANIHIP_MD_ATOM_CLUSTER) return;   // moved by k_md_constrain
    const float im = a.inv_mass[at], kick = a.hdt * im;
    float *x = a.coords + 3 * at, *lo = a.coords_lo + 3 * at;
    const float *f = a.forces + 3 * at;
    float c1 = 1.f, sigma = 0.f, xi[3] = {0.f, 0.f, 0.f};
    if (a.langevin) {
        // c1 = exp(-gamma dt), sigma^2 = kT (1 - c1^2) / m: in fp64, 1 - c1^2 from expm1 (gamma dt ~ 1e-3 would lose
        // four digits to the cancellation in fp32)
        const double gdt = (double)a.friction[c] * a.dtd;
        c1 = (float)exp(-gdt);
        sigma = (float)sqrt((double)a.kT[c] * -expm1(-2.0 * gdt) * (double)im);
        md_normals(a, (uint32_t)i, md_replica(a, c), xi);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float vk = v[k] + kick * f[k], xk = x[k], lk = lo[k];
        if (a.langevin) {
            md_two_add(xk, lk, a.hdt * vk);
            vk = c1 * vk + sigma * xi[k];
            md_two_add(xk, lk, a.hdt * vk);
        } else {
            md_two_add(xk, lk, a.dt * vk);
        }
        v[k] = vk, x[k] = xk, lo[k] = lk;
    }
}

// a molecule of one chunk has its sums written straight to `out`, scaled; a longer one goes through k_md_sum
template <int W>
__device__ __forceinline__ void md_store_sums(const MdArgs &a, int64_t c, int64_t b, const double (&s)[W], double scale)
{
    if (threadIdx.x != 0) return;
    double *dst = a.Gc == 1 ? a.out + c * W : a.part + (c * a.Gc + b) * W;
#pragma unroll
    for (int w = 0; w < W; ++w) dst[w] = a.Gc == 1 ? s[w] * scale : s[w];
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_kick(MdArgs a)
{
    const int64_t c = blockIdx.x / a.Gc, b = blockIdx.x % a.Gc, i = b * MD_BLOCK + threadIdx.x;
    double ke[1] = {0.0};
    if (i < a.A) {
        const int64_t at = c * a.A + i;
        float *v = a.vel + 3 * at;
        if (a.active[at] == ANIHIP_MD_ATOM_CLUSTER) {   // kicked and projected by k_md_constrain, which ran first
            const float vx = v[0], vy = v[1], vz = v[2];
            ke[0] = 0.5 * (double)a.mass[at] * ((double)vx * vx + (double)vy * vy + (double)vz * vz);
        } else if (a.active[at]) {
            const float m = a.mass[at], kick = a.hdt * (float)(ANIHIP_MD_ACC_UNIT / (double)m);
            const float *f = a.forces + 3 * at;
            const float vx = v[0] + kick * f[0], vy = v[1] + kick * f[1], vz = v[2] + kick * f[2];
            v[0] = vx, v[1] = vy, v[2] = vz;
            ke[0] = 0.5 * (double)m * ((double)vx * vx + (double)vy * vy + (double)vz * vz);
        } else {
            v[0] = v[1] = v[2] = 0.f;
        }
    }
    md_block_sum<1>(ke);
    md_store_sums<1>(a, c, b, ke, 1.0 / ANIHIP_MD_ACC_UNIT);
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_momentum(MdArgs a)
{
    const int64_t c = blockIdx.x / a.Gc, b = blockIdx.x % a.Gc, i = b * MD_BLOCK + threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (i < a.A && a.active[c * a.A + i]) {
        const double m = a.mass[c * a.A + i];
        const float *v = a.vel + 3 * (c * a.A + i);
        s[0] = m * v[0], s[1] = m * v[1], s[2] = m * v[2], s[3] = m;
    }
    md_block_sum<4>(s);
    md_store_sums<4>(a, c, b, s, 1.0);
}

// out[c][w] = scale * sum over the chunks of part[c][.][w], in chunk order within each thread's stride
template <int W>
__global__ __launch_bounds__(MD_BLOCK) void k_md_sum(MdArgs a, double scale)
{
    const int64_t c = blockIdx.x;
    double s[W];
#pragma unroll
    for (int w = 0; w < W; ++w) s[w] = 0.0;
    for (int64_t q = threadIdx.x; q < a.Gc; q += MD_BLOCK) {
#pragma unroll
        for (int w = 0; w < W; ++w) s[w] += a.part[(c * a.Gc + q) * W + w];
    }
    md_block_sum<W>(s);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < W; ++w) a.out[c * W + w] = s[w] * scale;
    }
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_sub_vcm(MdArgs a)
{
    const int64_t c = blockIdx.x / a.Gc, i = (blockIdx.x % a.Gc) * MD_BLOCK + threadIdx.x;
    if (i >= a.A || !a.active[c * a.A + i]) return;
    const double *p = a.out + 4 * c;   // sum m v [3], sum m (> 0: this atom is active)
    float *v = a.vel + 3 * (c * a.A + i);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (float)((double)v[k] - p[k] / p[3]);
}

// ---- bond-length constraints (include/anihip.h has the definition) ---------------------------------------------------------
// One thread per cluster, MDC_BLOCK clusters per workgroup.  The constraints address the atoms of their cluster by slots known
// only at run time, and an array of a thread indexed that way would live in scratch memory: the cluster is staged in LDS
// instead, [row][thread] with the thread fastest, so that the threads of a wave never share a bank whatever slots they read.

constexpr int MDC_BLOCK = 64;
constexpr int MDC_NA = ANIHIP_MD_CLUSTER_ATOMS, MDC_NB = ANIHIP_MD_CLUSTER_BONDS;
constexpr int MDC_SMALL = 4;   // a second instance for tables of clusters of at most 4 atoms and 4 constraints (rigid waters, XH3)
enum { MDC_DRIFT = 0, MDC_KICK = 1, MDC_PROJECT = 2 };

struct MdCluster {   // the rows of one thread
    double (*x)[MDC_BLOCK], (*ref)[MDC_BLOCK], (*v)[MDC_BLOCK], (*w)[MDC_BLOCK], (*d2)[MDC_BLOCK];
    int (*bond)[MDC_BLOCK];   // a | b << 8
    int t, n, nb;
    double tol;
    int max_it;
};

// SHAKE: x holds the unconstrained positions, ref the positions the move started from (the correction directions).  Gauss-
// Seidel in the stored constraint order; returns the number of sweeps that corrected a constraint (max_it: not converged).
__device__ __forceinline__ int mdc_shake(const MdCluster &q)
{
    const int t = q.t;
    int it = 0;
    for (; it < q.max_it; ++it) {
        bool moved = false;
        for (int k = 0; k < q.nb; ++k) {
            const int ab = q.bond[k][t], a = 3 * (ab & 255), b = 3 * (ab >> 8);
            const double sx = q.x[a][t] - q.x[b][t], sy = q.x[a + 1][t] - q.x[b + 1][t], sz = q.x[a + 2][t] - q.x[b + 2][t];
            const double d2 = q.d2[k][t], diff = sx * sx + sy * sy + sz * sz - d2;
            if (fabs(diff) <= 2.0 * q.tol * d2) continue;   // (a NaN fails this test and is corrected until max_it)
            moved = true;
            const double rx = q.ref[a][t] - q.ref[b][t], ry = q.ref[a + 1][t] - q.ref[b + 1][t],
                         rz = q.ref[a + 2][t] - q.ref[b + 2][t];
            const double wa = q.w[a / 3][t], wb = q.w[b / 3][t];
            const double g = diff / (2.0 * (wa + wb) * (sx * rx + sy * ry + sz * rz));
            q.x[a][t] -= wa * g * rx, q.x[a + 1][t] -= wa * g * ry, q.x[a + 2][t] -= wa * g * rz;
            q.x[b][t] += wb * g * rx, q.x[b + 1][t] += wb * g * ry, q.x[b + 2][t] += wb * g * rz;
        }
        if (!moved) break;
    }
    return it;
}

// move(x, v, h): x' = x + h v + W J(x)^T lambda on the constraint manifold, v' = (x' - x) / h; ref = x' afterwards
__device__ __forceinline__ int mdc_move(const MdCluster &q, double h)
{
    const int t = q.t;
    for (int r = 0; r < 3 * q.n; ++r) q.x[r][t] += h * q.v[r][t];
    const int it = mdc_shake(q);
    const double ih = 1.0 / h;
    for (int r = 0; r < 3 * q.n; ++r) {
        const double x1 = q.x[r][t];
        q.v[r][t] = (x1 - q.ref[r][t]) * ih;
        q.ref[r][t] = x1;
    }
    return it;
}

// project_v(x, v): v' = v - W J^T mu with r . (v'_a - v'_b) = 0 (RATTLE's velocity stage), Gauss-Seidel; a constraint is
// converged at |r . dv| <= tol d v_scale, v_scale the largest |v| component of the cluster when the projection starts
__device__ __forceinline__ int mdc_project(const MdCluster &q)
{
    const int t = q.t;
    double vs = 0.0;
    for (int r = 0; r < 3 * q.n; ++r) vs = fmax(vs, fabs(q.v[r][t]));
    int it = 0;
    for (; it < q.max_it; ++it) {
        bool moved = false;
        for (int k = 0; k < q.nb; ++k) {
            const int ab = q.bond[k][t], a = 3 * (ab & 255), b = 3 * (ab >> 8);
            const double rx = q.x[a][t] - q.x[b][t], ry = q.x[a + 1][t] - q.x[b + 1][t], rz = q.x[a + 2][t] - q.x[b + 2][t];
            const double rv = rx * (q.v[a][t] - q.v[b][t]) + ry * (q.v[a + 1][t] - q.v[b + 1][t])
                            + rz * (q.v[a + 2][t] - q.v[b + 2][t]);
            if (fabs(rv) <= q.tol * sqrt(q.d2[k][t]) * vs) continue;
            moved = true;
            const double wa = q.w[a / 3][t], wb = q.w[b / 3][t];
            const double g = rv / ((wa + wb) * (rx * rx + ry * ry + rz * rz));
            q.v[a][t] -= wa * g * rx, q.v[a + 1][t] -= wa * g * ry, q.v[a + 2][t] -= wa * g * rz;
            q.v[b][t] += wb * g * rx, q.v[b + 1][t] += wb * g * ry, q.v[b + 2][t] += wb * g * rz;
        }
        if (!moved) break;
    }
    return it;
}

// NA, NB: the most atoms and constraints a cluster of this launch may have (the tables keep their strides of 8 and 12): the
// LDS of a workgroup, and with it the workgroups a CU holds, follows the clusters that are there
template <int MODE, int NA, int NB>
__global__ __launch_bounds__(MDC_BLOCK) void k_md_constrain(MdArgs a, anihip_md_clusters cl, int64_t n_atoms)
{
    __shared__ double sx[3 * NA][MDC_BLOCK], sv[3 * NA][MDC_BLOCK], sw[NA][MDC_BLOCK], sd2[NB][MDC_BLOCK];
    __shared__ double sref[MODE == MDC_DRIFT ? 3 * NA : 1][MDC_BLOCK];
    __shared__ int sbond[NB][MDC_BLOCK], sat[NA][MDC_BLOCK];
    const int t = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * MDC_BLOCK + t;
    if (c >= cl.n_clusters) return;   // (no barrier below: a thread reads only the LDS column it wrote)
    MdCluster q = {sx, sref, sv, sw, sd2, sbond, t, cl.count[2 * c], cl.count[2 * c + 1], cl.tolerance, cl.max_iterations};
    int32_t *iters = cl.iterations + 2 * c + (MODE == MDC_DRIFT ? 0 : 1);
    // The tables and then the atoms are read by loops of constant length into registers, the slots past the cluster's own
    // reading slot 0 again: every load of a phase is in flight at once, where a loop over the cluster's own length would wait
    // for them one by one (a single wave per workgroup has little else to hide the latency with).
    // A table that does not hold what the header asks for moves nothing and reports max_iterations.
    bool ok = q.n >= 2 && q.n <= NA && q.nb >= 1 && q.nb <= NB;
    int64_t g[NA];
    double w[NA];
#pragma unroll
    for (int s = 0; s < NA; ++s) {
        g[s] = cl.atoms[MDC_NA * c + s];
        w[s] = cl.w[MDC_NA * c + s];
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const int ia = cl.bonds[2 * (MDC_NB * c + k)], ib = cl.bonds[2 * (MDC_NB * c + k) + 1];
        ok = ok && (k >= q.nb || (ia < q.n && ib < q.n && ia != ib));
        sbond[k][t] = ia | ib << 8;
        sd2[k][t] = cl.d2[MDC_NB * c + k];
    }
#pragma unroll
    for (int s = 0; s < NA; ++s) {
        ok = ok && (s >= q.n || (g[s] >= 0 && g[s] < n_atoms));
        if (s >= q.n) g[s] = g[0];
    }
    if (!ok) {
        *iters = cl.max_iterations;
        return;
    }
    const double hdt = 0.5 * a.dtd;
    float xh[NA][3], xl[NA][3], v0[NA][3], f0[NA][3];
#pragma unroll
    for (int s = 0; s < NA; ++s) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            xh[s][k] = a.coords[3 * g[s] + k], xl[s][k] = a.coords_lo[3 * g[s] + k], v0[s][k] = a.vel[3 * g[s] + k];
            f0[s][k] = MODE != MDC_PROJECT ? a.forces[3 * g[s] + k] : 0.f;
        }
    }
#pragma unroll
    for (int s = 0; s < NA; ++s) {
        if (s >= q.n) break;
        sw[s][t] = w[s];
        sat[s][t] = (int)g[s];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double x = (double)xh[s][k] + (double)xl[s][k];   // exact
            sx[3 * s + k][t] = x;
            if (MODE == MDC_DRIFT) sref[3 * s + k][t] = x;
            // B; a fixed anchor stays at rest
            sv[3 * s + k][t] = w[s] != 0.0 ? (double)v0[s][k] + hdt * (double)f0[s][k] * w[s] : 0.0;
        }
    }
    int it;
    if (MODE == MDC_DRIFT) {
        if (a.langevin) {
            it = mdc_move(q, hdt);
            const int64_t mol = g[0] / a.A;   // (a cluster lies in one molecule)
            const double gdt = (double)a.friction[mol] * a.dtd, c1 = exp(-gdt);
            const double s2 = (double)a.kT[mol] * -expm1(-2.0 * gdt);
            const uint32_t replica = md_replica(a, mol);
            for (int s = 0; s < q.n; ++s) {   // O, with the noise of the atom's own index
                const double w = sw[s][t];
                if (w == 0.0) continue;
                float xi[3];
                md_normals(a, (uint32_t)(sat[s][t] - mol * a.A), replica, xi);
                const double sigma = sqrt(s2 * w);
#pragma unroll
                for (int k = 0; k < 3; ++k) sv[3 * s + k][t] = c1 * sv[3 * s + k][t] + sigma * (double)xi[k];
            }
            it = max(it, mdc_move(q, hdt));
        } else {
            it = mdc_move(q, a.dtd);
        }
    } else {
        it = mdc_project(q);
    }
    *iters = it;
    for (int s = 0; s < q.n; ++s) {
        if (sw[s][t] == 0.0) continue;   // a fixed anchor is never written
        const int64_t at = sat[s][t];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a.vel[3 * at + k] = (float)sv[3 * s + k][t];
            if (MODE == MDC_DRIFT) {
                const double x = sx[3 * s + k][t];
                const float hi = (float)x;
                a.coords[3 * at + k] = hi;
                a.coords_lo[3 * at + k] = (float)(x - (double)hi);
            }
        }
    }
}

// ---- stochastic cell rescaling (include/anihip.h has the definition) -------------------------------------------------------
// Two launches because the move of a molecule is one number that every atom of it needs: the first forms mu from the cell, the
// kinetic energy and the virial as they are and rescales the cell; the second reads mu from `scale`.  (One launch would have
// atoms read a cell that another workgroup is rewriting.)

struct MdBarostat {
    double beta_over_tau;   // beta_T / tau_p, Angstrom^3 / (Hartree fs)
    const double *pressure, *virial;
    double *kinetic, *cell64, *scale;
    float *cell32;
};

__global__ __launch_bounds__(MD_BLOCK) void k_md_barostat_cell(MdArgs a, MdBarostat b, int64_t n_mol)
{
    const int64_t c = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x;
    if (c >= n_mol) return;
    double h[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = b.cell64[9 * c + k];
    const double V = fabs(h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6])
                          + h[2] * (h[3] * h[7] - h[4] * h[6]));
    const double *W = b.virial + 9 * c;
    const double K = b.kinetic[c], p_int = (2.0 * K - (W[0] + W[4] + W[8])) / (3.0 * V);
    float xi[3];
    md_normals(a, 0u, md_replica(a, c), xi);
    const double rate = b.beta_over_tau * a.dtd;
    const double deps = -rate * (b.pressure[c] - p_int) + sqrt(2.0 * (double)a.kT[c] * rate / V) * (double)xi[0];
    const double mu = exp(deps / 3.0);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double hk = mu * h[k];
        b.cell64[9 * c + k] = hk;
        b.cell32[9 * c + k] = (float)hk;
    }
    b.kinetic[c] = K / (mu * mu);
    b.scale[c] = mu;
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_barostat_scale(MdArgs a, const double *scale)
{
    const int64_t c = blockIdx.x / a.Gc, i = (blockIdx.x % a.Gc) * MD_BLOCK + threadIdx.x;
    if (i >= a.A) return;
    const int64_t at = c * a.A + i;
    if (!a.active[at]) return;
    const double mu = scale[c], inv_mu = 1.0 / mu;
    float *x = a.coords + 3 * at, *lo = a.coords_lo + 3 * at, *v = a.vel + 3 * at;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double xk = mu * ((double)x[k] + (double)lo[k]);   // (the sum of the pair is exact in fp64)
        const float hi = (float)xk;
        x[k] = hi, lo[k] = (float)(xk - (double)hi);
        v[k] = (float)((double)v[k] * inv_mu);
    }
}

// ---- molecular cell rescaling: the barostat with bond constraints (include/anihip.h has the definition) ---------------------
// A constraint cluster is a scaling group: the move translates it rigidly by the displacement of its centre of mass, so bond
// vectors and relative velocities are kept and no solver pass follows.  One thread per cluster in both cluster kernels.  The
// atoms are read by loops of constant length into registers, the slots past the cluster's own reading slot 0 again with mass
// 0 (as k_md_constrain reads them): no array of a thread is indexed by a run-time slot, so there is no LDS and no scratch.

struct MdGroup {
    int n;
    bool anchored;         // a slot of w = 0: the cluster neither moves nor enters a sum
    int64_t g[MDC_NA];     // global atom of each slot
    float m[MDC_NA], xh[MDC_NA][3], xl[MDC_NA][3], v[MDC_NA][3];
    double X[3], V[3], M;   // centre of mass, its velocity, the total mass
};

// false: the table entries of cluster q are out of range, and nothing of it may be touched
__device__ __forceinline__ bool md_group_load(const MdArgs &a, const anihip_md_clusters &cl, int64_t q, int64_t n_atoms, MdGroup &G)
{
    G.n = cl.count[2 * q];
    bool ok = G.n >= 2 && G.n <= MDC_NA;
    G.anchored = false;
    double w[MDC_NA];
#pragma unroll
    for (int s = 0; s < MDC_NA; ++s) {
        G.g[s] = cl.atoms[MDC_NA * q + s];
        w[s] = cl.w[MDC_NA * q + s];
    }
#pragma unroll
    for (int s = 0; s < MDC_NA; ++s) {
        const bool in = s < G.n;
        ok = ok && (!in || (G.g[s] >= 0 && G.g[s] < n_atoms));
        G.anchored = G.anchored || (in && w[s] == 0.0);
        if (!in) G.g[s] = G.g[0];
    }
    if (!ok) return false;
#pragma unroll
    for (int s = 0; s < MDC_NA; ++s) {
        G.m[s] = s < G.n ? a.mass[G.g[s]] : 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            G.xh[s][k] = a.coords[3 * G.g[s] + k], G.xl[s][k] = a.coords_lo[3 * G.g[s] + k], G.v[s][k] = a.vel[3 * G.g[s] + k];
    }
    G.M = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) G.X[k] = G.V[k] = 0.0;
#pragma unroll
    for (int s = 0; s < MDC_NA; ++s) {   // in slot order
        const double m = G.m[s];
        G.M += m;
#pragma unroll
        for (int k = 0; k < 3; ++k) G.X[k] += m * ((double)G.xh[s][k] + (double)G.xl[s][k]), G.V[k] += m * (double)G.v[s][k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) G.X[k] /= G.M, G.V[k] /= G.M;
    return true;
}

// terms[at] = (1/2 M |V|^2 in amu A^2 / fs^2, sum f . (x - X)) at the atom of slot 0 and zeros at the cluster's other atoms
__global__ __launch_bounds__(MD_BLOCK) void k_md_group_clusters(MdArgs a, anihip_md_clusters cl, int64_t n_atoms, double *terms)
{
    const int64_t q = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x;
    if (q >= cl.n_clusters) return;
    MdGroup G;
    if (!md_group_load(a, cl, q, n_atoms, G)) return;
    float f[MDC_NA][3];
#pragma unroll
    for (int s = 0; s < MDC_NA; ++s) {
#pragma unroll
        for (int k = 0; k < 3; ++k) f[s][k] = a.forces[3 * G.g[s] + k];
    }
    double ke = 0.0, vir = 0.0;
    if (!G.anchored) {
        ke = 0.5 * G.M * (G.V[0] * G.V[0] + G.V[1] * G.V[1] + G.V[2] * G.V[2]);
#pragma unroll
        for (int s = 0; s < MDC_NA; ++s) {
            if (s >= G.n) break;
#pragma unroll
            for (int k = 0; k < 3; ++k) vir += (double)f[s][k] * (((double)G.xh[s][k] + (double)G.xl[s][k]) - G.X[k]);
        }
    }
#pragma unroll
    for (int s = 0; s < MDC_NA; ++s) {
        if (s >= G.n) break;
        terms[2 * G.g[s]] = s == 0 ? ke : 0.0;
        terms[2 * G.g[s] + 1] = s == 0 ? vir : 0.0;
    }
}

struct MdGroupSums {
    double *kinetic_mol, *virial_mol;   // [C] each
};

// per 256-atom chunk: the free atoms' own 1/2 m v^2 (the expression of k_md_kick) and what the clusters left in `terms`
__global__ __launch_bounds__(MD_BLOCK) void k_md_group_sum(MdArgs a, const double *terms, MdGroupSums o)
{
    const int64_t c = blockIdx.x / a.Gc, b = blockIdx.x % a.Gc, i = b * MD_BLOCK + threadIdx.x;
    double s[2] = {0.0, 0.0};
    if (i < a.A) {
        const int64_t at = c * a.A + i;
        if (a.active[at] == ANIHIP_MD_ATOM_CLUSTER) {
            s[0] = terms[2 * at], s[1] = terms[2 * at + 1];
        } else if (a.active[at]) {
            const float *v = a.vel + 3 * at;
            const float vx = v[0], vy = v[1], vz = v[2];
            s[0] = 0.5 * (double)a.mass[at] * ((double)vx * vx + (double)vy * vy + (double)vz * vz);
        }
    }
    md_block_sum<2>(s);
    if (threadIdx.x != 0) return;
    if (a.Gc == 1) {
        o.kinetic_mol[c] = s[0] * (1.0 / ANIHIP_MD_ACC_UNIT), o.virial_mol[c] = s[1];
    } else {
        a.part[(c * a.Gc + b) * 2] = s[0], a.part[(c * a.Gc + b) * 2 + 1] = s[1];
    }
}

// molecules of more than one chunk: the chunk sums added as k_md_sum adds them, the two totals to their own arrays
__global__ __launch_bounds__(MD_BLOCK) void k_md_group_total(MdArgs a, MdGroupSums o)
{
    const int64_t c = blockIdx.x;
    double s[2] = {0.0, 0.0};
    for (int64_t q = threadIdx.x; q < a.Gc; q += MD_BLOCK) s[0] += a.part[(c * a.Gc + q) * 2], s[1] += a.part[(c * a.Gc + q) * 2 + 1];
    md_block_sum<2>(s);
    if (threadIdx.x == 0) o.kinetic_mol[c] = s[0] * (1.0 / ANIHIP_MD_ACC_UNIT), o.virial_mol[c] = s[1];
}

// k_md_barostat_cell with the molecular pressure; the kinetic energy loses what its centre-of-mass part loses
__global__ __launch_bounds__(MD_BLOCK) void k_md_barostat_groups_cell(MdArgs a, MdBarostat b, MdGroupSums o, int64_t n_mol)
{
    const int64_t c = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x;
    if (c >= n_mol) return;
    double h[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = b.cell64[9 * c + k];
    const double V = fabs(h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6])
                          + h[2] * (h[3] * h[7] - h[4] * h[6]));
    const double *W = b.virial + 9 * c;
    const double K = o.kinetic_mol[c], p_int = (2.0 * K - ((W[0] + W[4] + W[8]) + o.virial_mol[c])) / (3.0 * V);
    float xi[3];
    md_normals(a, 0u, md_replica(a, c), xi);
    const double rate = b.beta_over_tau * a.dtd;
    const double deps = -rate * (b.pressure[c] - p_int) + sqrt(2.0 * (double)a.kT[c] * rate / V) * (double)xi[0];
    const double mu = exp(deps / 3.0);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double hk = mu * h[k];
        b.cell64[9 * c + k] = hk;
        b.cell32[9 * c + k] = (float)hk;
    }
    const double K1 = K / (mu * mu);
    b.kinetic[c] = (b.kinetic[c] - K) + K1;   // = kinetic - (1 - mu^-2) K_mol: the part internal to the groups stays
    o.kinetic_mol[c] = K1;
    b.scale[c] = mu;
}

// k_md_barostat_scale for the free atoms alone
__global__ __launch_bounds__(MD_BLOCK) void k_md_barostat_groups_free(MdArgs a, const double *scale)
{
    const int64_t c = blockIdx.x / a.Gc, i = (blockIdx.x % a.Gc) * MD_BLOCK + threadIdx.x;
    if (i >= a.A) return;
    const int64_t at = c * a.A + i;
    if (a.active[at] != 1) return;
    const double mu = scale[c], inv_mu = 1.0 / mu;
    float *x = a.coords + 3 * at, *lo = a.coords_lo + 3 * at, *v = a.vel + 3 * at;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double xk = mu * ((double)x[k] + (double)lo[k]);
        const float hi = (float)xk;
        x[k] = hi, lo[k] = (float)(xk - (double)hi);
        v[k] = (float)((double)v[k] * inv_mu);
    }
}

// x_i += (mu - 1) X, v_i += (1 / mu - 1) V: every atom of the cluster gets the same two vectors
__global__ __launch_bounds__(MD_BLOCK) void k_md_barostat_groups_move(MdArgs a, anihip_md_clusters cl, int64_t n_atoms,
                                                                      const double *scale)
{
    const int64_t q = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x;
    if (q >= cl.n_clusters) return;
    MdGroup G;
    if (!md_group_load(a, cl, q, n_atoms, G) || G.anchored) return;
    const double mu = scale[G.g[0] / a.A], dx = mu - 1.0, dv = 1.0 / mu - 1.0;   // (a cluster lies in one molecule)
#pragma unroll
    for (int s = 0; s < MDC_NA; ++s) {
        if (s >= G.n) break;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double xk = ((double)G.xh[s][k] + (double)G.xl[s][k]) + dx * G.X[k];
            const float hi = (float)xk;
            a.coords[3 * G.g[s] + k] = hi, a.coords_lo[3 * G.g[s] + k] = (float)(xk - (double)hi);
            a.vel[3 * G.g[s] + k] = (float)((double)G.v[s][k] + dv * G.V[k]);
        }
    }
}

// ---- ring polymers: path-integral MD over the beads of a batch (include/anihip.h has the definition) -----------------------
// k_md_rp_drift: one thread per (bead or mode, atom, Cartesian component).  A workgroup of RP_BLOCK = 1024 threads takes NE =
// 1024 / P consecutive floats of the polymer's [A][3] layout, thread t = m NE + el the element el of bead m: a bead is read and
// written in contiguous runs of NE floats (128 bytes at P = 32, 64 at P = 64).  The positions (the exact fp64 sum of the pair)
// and the kicked velocities go to LDS; after a barrier thread (m, el) forms mode m of its element by a dot product of P terms,
// propagates it (A [O A]), and the modes go back through LDS the same way: P terms per thread and transform, not P^2, which is
// what matters for the latency of a small batch.  Before that the workgroup builds in LDS, in fp64, the P values of cos and
// sin(2 pi m / P), from them the mode matrix C, and the propagator and thermostat coefficients of every mode (thread k those
// of mode k: one sin, one sincos, one exp and one expm1 per mode and workgroup).  The thread of mode k draws the Philox block
// of (atom, stream of entry r P + k) itself and takes its component.  Any P in 2 .. 64 at run time, one instance.
//
// Precision: everything between the loads and the stores is fp64 (gfx950 issues fp64 FMAs at the fp32 rate), so the only
// roundings of a step are the final ones to the pair and to fp32.  Mode 0 is the centroid itself, the fp64 mean of the pairs,
// so a centroid step far below one ulp of the coordinate is kept as k_md_drift keeps it; modes k > 0 are formed from the
// offsets q_j - centroid and v_j - mean v: beads that are equal give offsets, and with them modes, that are exactly zero, and
// the beads stay equal bit for bit.

constexpr int RP_BLOCK = 1024, RP_MAX = ANIHIP_MD_RP_MAX_BEADS;

struct RpArgs {
    int P, NE;        // beads, 2 .. RP_MAX, and elements per workgroup, RP_BLOCK / P
    int64_t Gr;       // workgroups per polymer
    double lambda;    // PILE: gamma_k = 2 lambda omega_k
};

__global__ __launch_bounds__(RP_BLOCK) void k_md_rp_drift(MdArgs a, RpArgs rp)
{
    __shared__ double sC[RP_MAX][RP_MAX + 1];   // sC[k][j] = C_jk for 0 < k < P (the row padded: a wave reads several k at one j); row 0 is 1, the centroid's share of every bead
    __shared__ double sTrig[RP_MAX][2];         // cos and sin(2 pi m / P)
    __shared__ double sA[RP_MAX][3];            // A(h) of mode k: cos(w h), sin(w h) / w, -w sin(w h); mode 0: 1, h, 0
    __shared__ double sO[RP_MAX][2];            // O of mode k: c_k and sqrt(P kT (1 - c_k^2)); mode 0, the centroid velocity: sqrt(kT (1 - c_0^2))
    __shared__ double sQ[RP_BLOCK], sV[RP_BLOCK];   // [bead or mode][el]
    const int t = threadIdx.x, P = rp.P, NE = rp.NE;
    const int m = t / NE, el = t % NE;
    const int64_t r = blockIdx.x / rp.Gr, chunk = blockIdx.x % rp.Gr;
    const int64_t c0 = r * P;   // the polymer's first bead
    const double h = a.langevin ? 0.5 * a.dtd : a.dtd;
    if (t < P) {
        double co, si, cs = 1.0, sw = h, ws = 0.0, ck = 1.0, sk = 0.0;
        sincospi(2.0 * (double)t / (double)P, &si, &co);
        const double kT = a.kT[c0], wP = (double)P * kT / ANIHIP_MD_HBAR, wk = 2.0 * wP * sinpi((double)t / (double)P);
        if (t > 0) {
            double s;
            sincos(wk * h, &s, &cs);
            sw = s / wk, ws = -wk * s;
        }
        if (a.langevin) {
            const double gdt = (t == 0 ? (double)a.friction[c0] : 2.0 * rp.lambda * wk) * a.dtd;
            ck = exp(-gdt);
            sk = sqrt((t == 0 ? 1.0 : (double)P) * kT * -expm1(-2.0 * gdt));
        }
        sTrig[t][0] = co, sTrig[t][1] = si;
        sA[t][0] = cs, sA[t][1] = sw, sA[t][2] = ws;
        sO[t][0] = ck, sO[t][1] = sk;
    }
    __syncthreads();
    {
        const double n1 = sqrt(1.0 / (double)P), n2 = sqrt(2.0 / (double)P);
        for (int q = t; q < P * P; q += RP_BLOCK) {
            const int k = q / P, j = q % P, mm = (j * k) % P;
            // (k = P / 2: mm is 0 or P / 2, cos = +-1)
            sC[k][j] = k == 0 ? 1.0 : 2 * k < P ? n2 * sTrig[mm][0] : 2 * k == P ? n1 * sTrig[mm][0] : n2 * sTrig[mm][1];
        }
    }
    const int64_t A3 = 3 * a.A, e = chunk * NE + el;
    const bool in = m < P && e < A3;
    const int64_t i = in ? e / 3 : 0, at0 = c0 * a.A + i, g = in ? (c0 + m) * A3 + e : 0;
    const uint8_t act = in ? a.active[at0] : 0;
    const bool move = act == 1;   // (0: padding or fixed, v = 0 and the coordinates untouched; an atom of a constraint cluster is not moved at all)
    double im = 0.0, x = 0.0, y = 0.0;
    if (move) {
        im = a.inv_mass[at0];
        const float hi = a.coords[g], lo = a.coords_lo[g], v0 = a.vel[g], f0 = a.forces[g];
        x = (double)hi + (double)lo;                  // exact
        y = (double)v0 + 0.5 * a.dtd * im * (double)f0;   // B
    }
    sQ[t] = x, sV[t] = y;
    __syncthreads();
    double u = 0.0, w = 0.0;
    if (move) {
        double qbar = 0.0, vbar = 0.0;
        for (int j = 0; j < P; ++j) qbar += sQ[j * NE + el], vbar += sV[j * NE + el];
        qbar /= (double)P, vbar /= (double)P;
        if (m == 0) {
            u = qbar, w = vbar;
        } else {
            for (int j = 0; j < P; ++j) {
                const double c = sC[m][j];
                u += c * (sQ[j * NE + el] - qbar), w += c * (sV[j * NE + el] - vbar);
            }
        }
        // A(h) [O A(h)]: the centroid drifts freely, every other mode turns in its own phase space
        const double cs = sA[m][0], sw = sA[m][1], ws = sA[m][2];
        double u1 = u * cs + w * sw, w1 = u * ws + w * cs;
        if (a.langevin) {
            float xi[3];
            md_normals(a, (uint32_t)i, md_replica(a, c0 + m), xi);
            const int comp = (int)(e - 3 * i);
            w1 = sO[m][0] * w1 + sO[m][1] * sqrt(im) * (double)(comp == 0 ? xi[0] : comp == 1 ? xi[1] : xi[2]);
            const double u2 = u1 * cs + w1 * sw;
            w1 = u1 * ws + w1 * cs, u1 = u2;
        }
        u = u1, w = w1;
    }
    __syncthreads();   // every thread has read the beads
    sQ[t] = u, sV[t] = w;
    __syncthreads();
    if (move) {
        x = 0.0, y = 0.0;
        for (int k = 0; k < P; ++k) {   // k = 0 first: the centroid, then the offsets
            const double c = sC[k][m];
            x += c * sQ[k * NE + el], y += c * sV[k * NE + el];
        }
        const float xh = (float)x;
        a.coords[g] = xh, a.coords_lo[g] = (float)(x - (double)xh);
        a.vel[g] = (float)y;
    } else if (in && !act) {
        a.vel[g] = 0.f;
    }
}

// per atom: the centroid, and over the active atoms the spring and centroid-virial terms of its P beads, summed per chunk as
// k_md_kick sums the kinetic energy (out[r] = (S_r, W_r); polymers of more than one chunk through k_md_sum<2>)
__global__ __launch_bounds__(MD_BLOCK) void k_md_rp_estimators(MdArgs a, int P, double *centroids)
{
    const int64_t r = blockIdx.x / a.Gc, b = blockIdx.x % a.Gc, i = b * MD_BLOCK + threadIdx.x;
    double s[2] = {0.0, 0.0};
    if (i < a.A) {
        const int64_t c0 = r * P, at0 = c0 * a.A + i;
        double qbar[3] = {0.0, 0.0, 0.0};
        for (int j = 0; j < P; ++j) {
            const int64_t g = 3 * (at0 + j * a.A);
#pragma unroll
            for (int k = 0; k < 3; ++k) qbar[k] += (double)a.coords[g + k] + (double)a.coords_lo[g + k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            qbar[k] /= (double)P;
            centroids[3 * (r * a.A + i) + k] = qbar[k];
        }
        if (a.active[at0]) {
            double q0[3], prev[3], spring = 0.0;
            for (int j = 0; j < P; ++j) {
                const int64_t g = 3 * (at0 + j * a.A);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double q = (double)a.coords[g + k] + (double)a.coords_lo[g + k];
                    s[1] += (q - qbar[k]) * (double)a.forces[g + k];
                    if (j == 0) q0[k] = q;
                    else spring += (q - prev[k]) * (q - prev[k]);
                    prev[k] = q;
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) spring += (q0[k] - prev[k]) * (q0[k] - prev[k]);   // bead P - 1 to bead 0
            const double wP = (double)P * (double)a.kT[c0] / ANIHIP_MD_HBAR;
            s[0] = 0.5 * (double)a.mass[at0] * wP * wP * spring * (1.0 / ANIHIP_MD_ACC_UNIT);
        }
    }
    md_block_sum<2>(s);
    md_store_sums<2>(a, r, b, s, 1.0);
}

// ---- temperature replica exchange (include/anihip.h has the definition) ----------------------------------------------------
// Two launches, as the barostat: the decision of a pair is one number per entry that every atom of the entry needs.  The first
// has one thread per pair of rungs (k, k + 1), k = 2 j + parity; a thread owns its two slots and its two entries, so no
// thread reads what another writes.  It writes scale[c] for every entry of a ladder, 1 for those that keep their rung; the
// second launch rescales the velocities of the entries whose scale is not 1 and writes nothing else.

__global__ __launch_bounds__(MD_BLOCK) void k_md_exchange_pairs(MdArgs a, anihip_md_ladders ld, const double *energies,
                                                                double *kinetic, int64_t n_mol)
{
    const int K = ld.max_rungs, per_ladder = K / 2 + 1, parity = (int)(a.step0 & 1u);
    const int64_t t = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x, l = t / per_ladder;
    if (l >= ld.n_ladders) return;
    const int j = (int)(t % per_ladder), n = min(max(ld.count[l], 0), K), k = 2 * j + parity;
    int32_t *slot = ld.slot + l * K;
    if (parity == 1 && j == 0 && n > 0) {   // rung 0 sits an odd attempt out
        const int32_t e0 = slot[0];
        if (e0 >= 0 && e0 < n_mol) ld.scale[e0] = 1.0;
    }
    if (k >= n) return;
    const int32_t ea = slot[k], eb = k + 1 < n ? slot[k + 1] : -1;
    const bool has_a = ea >= 0 && ea < n_mol, has_b = eb >= 0 && eb < n_mol;
    if (!has_a || !has_b || eb == ea) {   // an unpaired top rung, or a slot out of range: whoever is there keeps its rung
        if (has_a) ld.scale[ea] = 1.0;
        if (has_b) ld.scale[eb] = 1.0;
        return;
    }
    const double kT_lo = (double)ld.rung_kT[l * K + k], kT_hi = (double)ld.rung_kT[l * K + k + 1];
    const double arg = (1.0 / kT_lo - 1.0 / kT_hi) * (energies[ea] - energies[eb]);
    uint32_t c[4] = {(uint32_t)k, ld.ladder_ids ? (uint32_t)ld.ladder_ids[l] : (uint32_t)l, a.step0, a.step1};
    philox4x32_10(c, a.key0, a.key1);
    const bool accept = log((double)md_uniform(c[0])) < arg;
    const int64_t pair = l * (K - 1) + k;
    ld.attempts[pair] += 1;
    if (!accept) {
        ld.scale[ea] = ld.scale[eb] = 1.0;
        return;
    }
    ld.accepts[pair] += 1;
    slot[k] = eb, slot[k + 1] = ea;
    ld.rung_of[ea] = k + 1, ld.rung_of[eb] = k;
    const double up = kT_hi / kT_lo, down = kT_lo / kT_hi;
    kinetic[ea] *= up, kinetic[eb] *= down;
    ld.scale[ea] = sqrt(up), ld.scale[eb] = sqrt(down);
    if (k + 1 == n - 1) ld.direction[ea] = -1;
    if (k == 0) {
        if (ld.direction[eb] == -1) ld.round_trips[eb] += 1;
        ld.direction[eb] = 1;
    }
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_exchange_scale(MdArgs a, const int32_t *rung_of, const double *scale)
{
    const int64_t c = blockIdx.x / a.Gc, i = (blockIdx.x % a.Gc) * MD_BLOCK + threadIdx.x;
    if (i >= a.A || rung_of[c] < 0) return;   // (an entry in no ladder has no scale)
    const double s = scale[c];
    const int64_t at = c * a.A + i;
    if (s == 1.0 || !a.active[at]) return;
    const float sf = (float)s;
    float *v = a.vel + 3 * at;
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] *= sf;
}

static int md_args(const anihip_md_params *params, MdArgs &a)
{
    ANIHIP_REQUIRE(params, "null pointer argument");
    const anihip_md_params &P = *params;
    ANIHIP_REQUIRE(P.n_mol >= 1 && P.atoms_per_mol >= 1, "n_mol and atoms_per_mol must be >= 1");
    ANIHIP_REQUIRE(P.dt > 0.0, "dt must be > 0");
    a = MdArgs{};
    a.A = P.atoms_per_mol;
    a.Gc = (a.A + MD_BLOCK - 1) / MD_BLOCK;
    ANIHIP_REQUIRE((int64_t)P.n_mol * a.A < ((int64_t)1 << 31) && (int64_t)P.n_mol * a.Gc < ((int64_t)1 << 31),
                   "n_mol x atoms_per_mol must stay below 2^31");
    a.langevin = (P.flags & ANIHIP_MD_LANGEVIN) != 0;
    a.dtd = P.dt, a.dt = (float)P.dt, a.hdt = (float)(0.5 * P.dt);
    a.key0 = (uint32_t)P.seed, a.key1 = (uint32_t)(P.seed >> 32);
    a.step0 = (uint32_t)P.step, a.step1 = (uint32_t)(P.step >> 32);
    return 0;
}

static inline dim3 md_grid(const anihip_md_params *p, const MdArgs &a) { return dim3((unsigned)(p->n_mol * a.Gc)); }

}  // namespace anihip

using namespace anihip;

extern "C" size_t anihip_md_workspace_bytes(int64_t n_mol, int64_t atoms_per_mol)
{
    if (n_mol < 1 || atoms_per_mol < 1) {
        set_error("n_mol and atoms_per_mol must be >= 1");
        return 0;
    }
    const int64_t Gc = (atoms_per_mol + MD_BLOCK - 1) / MD_BLOCK;
    return (size_t)(n_mol * Gc + n_mol) * 4 * sizeof(double);
}

extern "C" int anihip_md_noise(void *stream, uint64_t seed, uint64_t step, int64_t n_mol, int64_t atoms_per_mol,
                               const int64_t *replica_ids, float *out)
{
    ANIHIP_REQUIRE(out, "null pointer argument");
    ANIHIP_REQUIRE(n_mol >= 1 && n_mol < ((int64_t)1 << 31) && atoms_per_mol >= 1 && atoms_per_mol < ((int64_t)1 << 31),
                   "n_mol and atoms_per_mol must be >= 1");
    const anihip_md_params P = {(int32_t)n_mol, (int32_t)atoms_per_mol, 0, 0, 1.0, seed, step};
    MdArgs a;
    if (int rc = md_args(&P, a)) return rc;
    a.replica_ids = replica_ids;
    hipLaunchKernelGGL(k_md_noise, md_grid(&P, a), dim3(MD_BLOCK), 0, (hipStream_t)stream, a, out);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_md_drift(void *stream, const anihip_md_params *params, const uint8_t *active, const float *inv_mass,
                               const float *kT, const float *friction, const int64_t *replica_ids, float *coords,
                               float *coords_lo, float *velocities, const float *forces)
{
    MdArgs a;
    if (int rc = md_args(params, a)) return rc;
    ANIHIP_REQUIRE(active && inv_mass && coords && coords_lo && velocities && forces, "null pointer argument");
    ANIHIP_REQUIRE(!a.langevin || (kT && friction), "Langevin dynamics needs kT and friction");
    a.active = active, a.inv_mass = inv_mass, a.kT = kT, a.friction = friction, a.replica_ids = replica_ids;
    a.coords = coords, a.coords_lo = coords_lo, a.vel = velocities, a.forces = forces;
    hipLaunchKernelGGL(k_md_drift, md_grid(params, a), dim3(MD_BLOCK), 0, (hipStream_t)stream, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

// the per-chunk sums of molecules longer than one chunk live in the caller's workspace: [C][Gc][W] then [C][W]
static int md_workspace(const anihip_md_params *params, MdArgs &a, void *workspace, size_t workspace_bytes)
{
    const size_t need = anihip_md_workspace_bytes(params->n_mol, params->atoms_per_mol);
    ANIHIP_REQUIRE(workspace && workspace_bytes >= need, "workspace holds %zu bytes, %zu needed", workspace_bytes, need);
    a.part = (double *)workspace;
    a.out = a.part + (size_t)params->n_mol * a.Gc * 4;
    return 0;
}

extern "C" int anihip_md_kick(void *stream, const anihip_md_params *params, const uint8_t *active, const float *mass,
                              float *velocities, const float *forces, double *kinetic, void *workspace,
                              size_t workspace_bytes)
{
    MdArgs a;
    if (int rc = md_args(params, a)) return rc;
    ANIHIP_REQUIRE(active && mass && velocities && forces && kinetic, "null pointer argument");
    if (int rc = md_workspace(params, a, workspace, workspace_bytes)) return rc;
    a.active = active, a.mass = mass, a.vel = velocities, a.forces = forces, a.out = kinetic;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_md_kick, md_grid(params, a), dim3(MD_BLOCK), 0, s, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    if (a.Gc > 1) {
        hipLaunchKernelGGL(k_md_sum<1>, dim3((unsigned)params->n_mol), dim3(MD_BLOCK), 0, s, a, 1.0 / ANIHIP_MD_ACC_UNIT);
        ANIHIP_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int anihip_md_remove_drift(void *stream, const anihip_md_params *params, const uint8_t *active, const float *mass,
                                      float *velocities, void *workspace, size_t workspace_bytes)
{
    MdArgs a;
    if (int rc = md_args(params, a)) return rc;
    ANIHIP_REQUIRE(active && mass && velocities, "null pointer argument");
    if (int rc = md_workspace(params, a, workspace, workspace_bytes)) return rc;
    a.active = active, a.mass = mass, a.vel = velocities;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_md_momentum, md_grid(params, a), dim3(MD_BLOCK), 0, s, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    if (a.Gc > 1) {
        hipLaunchKernelGGL(k_md_sum<4>, dim3((unsigned)params->n_mol), dim3(MD_BLOCK), 0, s, a, 1.0);
        ANIHIP_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_md_sub_vcm, md_grid(params, a), dim3(MD_BLOCK), 0, s, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_md_barostat(void *stream, const anihip_md_params *params, double beta_T, double tau_p,
                                  const uint8_t *active, const float *kT, const double *pressure, const int64_t *replica_ids,
                                  const double *virial, double *kinetic, double *cell64, float *cell32, float *coords,
                                  float *coords_lo, float *velocities, double *scale)
{
    MdArgs a;
    if (int rc = md_args(params, a)) return rc;
    ANIHIP_REQUIRE(beta_T > 0.0 && tau_p > 0.0, "beta_T and tau_p must be > 0");
    ANIHIP_REQUIRE(a.langevin, "the barostat needs Langevin dynamics (ANIHIP_MD_LANGEVIN): its noise is scaled by kT");
    ANIHIP_REQUIRE(params->step < ANIHIP_MD_BAROSTAT_STEP, "step must stay below 2^62");
    ANIHIP_REQUIRE(active && kT && pressure && virial && kinetic && cell64 && cell32 && coords && coords_lo && velocities && scale,
                   "null pointer argument");
    a.step1 |= (uint32_t)(ANIHIP_MD_BAROSTAT_STEP >> 32);   // a stream of its own, apart from every drift's
    a.active = active, a.kT = kT, a.replica_ids = replica_ids;
    a.coords = coords, a.coords_lo = coords_lo, a.vel = velocities;
    const MdBarostat b = {beta_T / tau_p, pressure, virial, kinetic, cell64, scale, cell32};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_md_barostat_cell, dim3((unsigned)((params->n_mol + MD_BLOCK - 1) / MD_BLOCK)), dim3(MD_BLOCK), 0, s, a, b,
                       (int64_t)params->n_mol);
    ANIHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_md_barostat_scale, md_grid(params, a), dim3(MD_BLOCK), 0, s, a, (const double *)scale);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

static int md_clusters(const anihip_md_clusters *clusters)
{
    ANIHIP_REQUIRE(clusters, "null pointer argument");
    const anihip_md_clusters &q = *clusters;
    ANIHIP_REQUIRE(q.n_clusters >= 0 && q.n_clusters < ((int64_t)1 << 31) * MDC_BLOCK, "n_clusters out of range");
    ANIHIP_REQUIRE(q.n_clusters == 0 || (q.atoms && q.count && q.bonds && q.w && q.d2 && q.iterations),
                   "null pointer in the cluster tables");
    ANIHIP_REQUIRE(q.tolerance > 0.0 && q.max_iterations >= 1, "tolerance must be > 0 and max_iterations >= 1");
    ANIHIP_REQUIRE(q.max_atoms >= 0 && q.max_bonds >= 0, "max_atoms and max_bonds must be >= 0");
    return 0;
}

template <int MODE>
static int md_constrain(void *stream, const anihip_md_params *params, const anihip_md_clusters *clusters, MdArgs &a)
{
    if (int rc = md_clusters(clusters)) return rc;
    if (clusters->n_clusters == 0) return 0;
    const unsigned grid = (unsigned)((clusters->n_clusters + MDC_BLOCK - 1) / MDC_BLOCK);
    const int64_t n_atoms = (int64_t)params->n_mol * a.A;
    // (max_atoms = 0: not known; a cluster larger than the launch allows moves nothing and reports max_iterations)
    if (clusters->max_atoms >= 2 && clusters->max_atoms <= MDC_SMALL && clusters->max_bonds >= 1 && clusters->max_bonds <= MDC_SMALL)
        hipLaunchKernelGGL((k_md_constrain<MODE, MDC_SMALL, MDC_SMALL>), dim3(grid), dim3(MDC_BLOCK), 0, (hipStream_t)stream, a,
                           *clusters, n_atoms);
    else
        hipLaunchKernelGGL((k_md_constrain<MODE, MDC_NA, MDC_NB>), dim3(grid), dim3(MDC_BLOCK), 0, (hipStream_t)stream, a,
                           *clusters, n_atoms);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_md_constrain_drift(void *stream, const anihip_md_params *params, const anihip_md_clusters *clusters,
                                         const float *kT, const float *friction, const int64_t *replica_ids, float *coords,
                                         float *coords_lo, float *velocities, const float *forces)
{
    MdArgs a;
    if (int rc = md_args(params, a)) return rc;
    ANIHIP_REQUIRE(coords && coords_lo && velocities && forces, "null pointer argument");
    ANIHIP_REQUIRE(!a.langevin || (kT && friction), "Langevin dynamics needs kT and friction");
    a.kT = kT, a.friction = friction, a.replica_ids = replica_ids;
    a.coords = coords, a.coords_lo = coords_lo, a.vel = velocities, a.forces = forces;
    return md_constrain<MDC_DRIFT>(stream, params, clusters, a);
}

extern "C" int anihip_md_constrain_kick(void *stream, const anihip_md_params *params, const anihip_md_clusters *clusters,
                                        const float *coords, const float *coords_lo, float *velocities, const float *forces)
{
    MdArgs a;
    if (int rc = md_args(params, a)) return rc;
    ANIHIP_REQUIRE(coords && coords_lo && velocities && forces, "null pointer argument");
    a.coords = const_cast<float *>(coords), a.coords_lo = const_cast<float *>(coords_lo), a.vel = velocities, a.forces = forces;
    return md_constrain<MDC_KICK>(stream, params, clusters, a);
}

extern "C" int anihip_md_project_velocities(void *stream, const anihip_md_params *params, const anihip_md_clusters *clusters,
                                            const float *coords, const float *coords_lo, float *velocities)
{
    MdArgs a;
    if (int rc = md_args(params, a)) return rc;
    ANIHIP_REQUIRE(coords && coords_lo && velocities, "null pointer argument");
    a.coords = const_cast<float *>(coords), a.coords_lo = const_cast<float *>(coords_lo), a.vel = velocities;
    return md_constrain<MDC_PROJECT>(stream, params, clusters, a);
}

extern "C" int anihip_md_group_terms(void *stream, const anihip_md_params *params, const anihip_md_clusters *clusters,
                                     const uint8_t *active, const float *mass, const float *coords, const float *coords_lo,
                                     const float *velocities, const float *forces, double *scratch, double *kinetic_mol,
                                     double *virial_mol)
{
    MdArgs a;
    if (int rc = md_args(params, a)) return rc;
    if (int rc = md_clusters(clusters)) return rc;
    ANIHIP_REQUIRE(active && mass && coords && coords_lo && velocities && forces && scratch && kinetic_mol && virial_mol,
                   "null pointer argument");
    a.active = active, a.mass = mass, a.forces = forces;
    a.coords = const_cast<float *>(coords), a.coords_lo = const_cast<float *>(coords_lo), a.vel = const_cast<float *>(velocities);
    const int64_t n_atoms = (int64_t)params->n_mol * a.A;
    a.part = scratch + 2 * n_atoms;   // [C][A][2] per-atom terms, then [C][Gc][2] chunk sums
    const MdGroupSums o = {kinetic_mol, virial_mol};
    hipStream_t s = (hipStream_t)stream;
    if (clusters->n_clusters > 0) {
        hipLaunchKernelGGL(k_md_group_clusters, dim3((unsigned)((clusters->n_clusters + MD_BLOCK - 1) / MD_BLOCK)), dim3(MD_BLOCK), 0,
                           s, a, *clusters, n_atoms, scratch);
        ANIHIP_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_md_group_sum, md_grid(params, a), dim3(MD_BLOCK), 0, s, a, (const double *)scratch, o);
    ANIHIP_CHECK_HIP(hipGetLastError());
    if (a.Gc > 1) {
        hipLaunchKernelGGL(k_md_group_total, dim3((unsigned)params->n_mol), dim3(MD_BLOCK), 0, s, a, o);
        ANIHIP_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int anihip_md_barostat_groups(void *stream, const anihip_md_params *params, double beta_T, double tau_p,
                                         const uint8_t *active, const float *kT, const double *pressure,
                                         const int64_t *replica_ids, const double *virial, double *kinetic, double *cell64,
                                         float *cell32, float *coords, float *coords_lo, float *velocities, double *scale,
                                         const anihip_md_clusters *clusters, const float *mass, double *kinetic_mol,
                                         const double *virial_mol)
{
    MdArgs a;
    if (int rc = md_args(params, a)) return rc;
    ANIHIP_REQUIRE(beta_T > 0.0 && tau_p > 0.0, "beta_T and tau_p must be > 0");
    ANIHIP_REQUIRE(a.langevin, "the barostat needs Langevin dynamics (ANIHIP_MD_LANGEVIN): its noise is scaled by kT");
    ANIHIP_REQUIRE(params->step < ANIHIP_MD_BAROSTAT_STEP, "step must stay below 2^62");
    if (int rc = md_clusters(clusters)) return rc;
    ANIHIP_REQUIRE(active && kT && pressure && virial && kinetic && cell64 && cell32 && coords && coords_lo && velocities && scale
                       && mass && kinetic_mol && virial_mol,
                   "null pointer argument");
    a.step1 |= (uint32_t)(ANIHIP_MD_BAROSTAT_STEP >> 32);   // the stream of anihip_md_barostat
    a.active = active, a.kT = kT, a.replica_ids = replica_ids, a.mass = mass;
    a.coords = coords, a.coords_lo = coords_lo, a.vel = velocities;
    const MdBarostat b = {beta_T / tau_p, pressure, virial, kinetic, cell64, scale, cell32};
    const MdGroupSums o = {kinetic_mol, const_cast<double *>(virial_mol)};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_md_barostat_groups_cell, dim3((unsigned)((params->n_mol + MD_BLOCK - 1) / MD_BLOCK)), dim3(MD_BLOCK), 0, s,
                       a, b, o, (int64_t)params->n_mol);
    ANIHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_md_barostat_groups_free, md_grid(params, a), dim3(MD_BLOCK), 0, s, a, (const double *)scale);
    ANIHIP_CHECK_HIP(hipGetLastError());
    if (clusters->n_clusters > 0) {
        hipLaunchKernelGGL(k_md_barostat_groups_move, dim3((unsigned)((clusters->n_clusters + MD_BLOCK - 1) / MD_BLOCK)),
                           dim3(MD_BLOCK), 0, s, a, *clusters, (int64_t)params->n_mol * a.A, (const double *)scale);
        ANIHIP_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

static int md_rp_args(const anihip_md_params *params, int32_t beads, MdArgs &a)
{
    if (int rc = md_args(params, a)) return rc;
    ANIHIP_REQUIRE(beads >= 2 && beads <= ANIHIP_MD_RP_MAX_BEADS, "beads must be in 2 .. %d, got %d", ANIHIP_MD_RP_MAX_BEADS, beads);
    ANIHIP_REQUIRE(params->n_mol % beads == 0, "n_mol = %d is no multiple of beads = %d", params->n_mol, beads);
    return 0;
}

extern "C" int anihip_md_rp_drift(void *stream, const anihip_md_params *params, int32_t beads, double pile_lambda,
                                  const uint8_t *active, const float *inv_mass, const float *kT, const float *friction,
                                  const int64_t *replica_ids, float *coords, float *coords_lo, float *velocities,
                                  const float *forces)
{
    MdArgs a;
    if (int rc = md_rp_args(params, beads, a)) return rc;
    ANIHIP_REQUIRE(active && inv_mass && kT && coords && coords_lo && velocities && forces, "null pointer argument");
    ANIHIP_REQUIRE(!a.langevin || friction, "the PILE thermostat needs friction");
    ANIHIP_REQUIRE(pile_lambda >= 0.0, "pile_lambda must be >= 0");
    a.active = active, a.inv_mass = inv_mass, a.kT = kT, a.friction = friction, a.replica_ids = replica_ids;
    a.coords = coords, a.coords_lo = coords_lo, a.vel = velocities, a.forces = forces;
    const int NE = RP_BLOCK / beads;
    const RpArgs rp = {beads, NE, (3 * a.A + NE - 1) / NE, pile_lambda};
    hipLaunchKernelGGL(k_md_rp_drift, dim3((unsigned)((params->n_mol / beads) * rp.Gr)), dim3(RP_BLOCK), 0, (hipStream_t)stream, a,
                       rp);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_md_rp_estimators(void *stream, const anihip_md_params *params, int32_t beads, const uint8_t *active,
                                       const float *mass, const float *kT, const float *coords, const float *coords_lo,
                                       const float *forces, double *estimators, double *centroids, void *workspace,
                                       size_t workspace_bytes)
{
    MdArgs a;
    if (int rc = md_rp_args(params, beads, a)) return rc;
    ANIHIP_REQUIRE(active && mass && kT && coords && coords_lo && forces && estimators && centroids, "null pointer argument");
    if (int rc = md_workspace(params, a, workspace, workspace_bytes)) return rc;   // (sized for n_mol entries: R of them are used)
    a.active = active, a.mass = mass, a.kT = kT, a.forces = forces, a.out = estimators;
    a.coords = const_cast<float *>(coords), a.coords_lo = const_cast<float *>(coords_lo);
    const unsigned R = (unsigned)(params->n_mol / beads);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_md_rp_estimators, dim3((unsigned)(R * a.Gc)), dim3(MD_BLOCK), 0, s, a, (int)beads, centroids);
    ANIHIP_CHECK_HIP(hipGetLastError());
    if (a.Gc > 1) {
        hipLaunchKernelGGL(k_md_sum<2>, dim3(R), dim3(MD_BLOCK), 0, s, a, 1.0);
        ANIHIP_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int anihip_md_exchange(void *stream, const anihip_md_params *params, const anihip_md_ladders *ladders,
                                  const double *energies, const uint8_t *active, float *velocities, double *kinetic)
{
    MdArgs a;
    if (int rc = md_args(params, a)) return rc;
    ANIHIP_REQUIRE(ladders, "null pointer argument");
    const anihip_md_ladders &ld = *ladders;
    ANIHIP_REQUIRE(ld.n_ladders >= 1 && ld.max_rungs >= 2, "a ladder needs at least 2 rungs (n_ladders %d, max_rungs %d)",
                   ld.n_ladders, ld.max_rungs);
    ANIHIP_REQUIRE((int64_t)ld.n_ladders * (ld.max_rungs / 2 + 1) < ((int64_t)1 << 31) * MD_BLOCK, "n_ladders x max_rungs out of range");
    ANIHIP_REQUIRE(a.langevin, "replica exchange needs Langevin dynamics (ANIHIP_MD_LANGEVIN): the rungs are temperatures");
    ANIHIP_REQUIRE(params->step < ANIHIP_MD_EXCHANGE_STEP, "step (the attempt number) must stay below 2^61");
    ANIHIP_REQUIRE(ld.slot && ld.count && ld.rung_of && ld.rung_kT && ld.attempts && ld.accepts && ld.direction && ld.round_trips
                       && ld.scale && energies && active && velocities && kinetic,
                   "null pointer argument");
    hipStream_t s = (hipStream_t)stream;
    if (ld.flags & ANIHIP_MD_LADDERS_CHECK) {   // the one host read of this file, and only on request
        std::vector<int32_t> slot((size_t)ld.n_ladders * ld.max_rungs);
        ANIHIP_CHECK_HIP(hipMemcpyAsync(slot.data(), ld.slot, slot.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        ANIHIP_CHECK_HIP(hipStreamSynchronize(s));
        for (size_t q = 0; q < slot.size(); ++q)
            ANIHIP_REQUIRE(slot[q] >= -1 && slot[q] < params->n_mol, "slot[%zu][%zu] = %d is outside -1 .. n_mol - 1 = %d",
                           q / ld.max_rungs, q % ld.max_rungs, slot[q], params->n_mol - 1);
    }
    a.step1 |= (uint32_t)(ANIHIP_MD_EXCHANGE_STEP >> 32);   // a stream of its own, apart from the drifts' and the barostat's
    a.active = active, a.vel = velocities;
    const int64_t threads = (int64_t)ld.n_ladders * (ld.max_rungs / 2 + 1);
    hipLaunchKernelGGL(k_md_exchange_pairs, dim3((unsigned)((threads + MD_BLOCK - 1) / MD_BLOCK)), dim3(MD_BLOCK), 0, s, a, ld,
                       energies, kinetic, (int64_t)params->n_mol);
    ANIHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_md_exchange_scale, md_grid(params, a), dim3(MD_BLOCK), 0, s, a, (const int32_t *)ld.rung_of,
                       (const double *)ld.scale);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}
