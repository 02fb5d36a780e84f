// Molecular-dynamics integrator of batches of molecules (torchani_amd.md.BatchedDynamics): velocity Verlet (NVE) and Langevin
// dynamics in the BAOAB splitting (Leimkuhler and Matthews 2013), every molecule with a temperature and a friction of its own.
// A step is   anihip_md_drift (B A [O A])  ->  energies and forces at the new coordinates  ->  anihip_md_kick (B, kinetic energy):
//
//   k_md_drift     one thread per atom: v += dt/2 f / m;  NVE x += dt v;  Langevin x += dt/2 v, v = c1 v + sigma xi, x += dt/2 v
//   k_md_kick      one thread per atom: v += dt/2 f / m, and the fp64 kinetic energy of each 256-atom chunk
//   k_md_sum       one workgroup per molecule: the chunk sums added in chunk order (only for molecules of more than one chunk)
//   k_md_momentum, k_md_sum, k_md_sub_vcm   anihip_md_remove_drift: sum m v and sum m per chunk, per molecule, then v -= v_cm
//
// Positions are pairs of floats, coords + coords_lo: every `x +=` is a two-sum, so a step far below one ulp of the coordinate
// is not lost, and coords (what the engine reads) is the fp32 nearest to the pair.  The noise xi is a pure function of (seed,
// step, replica id, atom index): Philox4x32-10 and Box-Muller (md_normals), the same for a replica wherever it sits in the batch.
// No atomics and every sum in a fixed order: trajectories are bit-identical run to run for bit-identical forces.
#include "anihip_common.h"

namespace anihip {

constexpr int MD_BLOCK = 256;   // atoms per chunk, threads per workgroup

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

// sum of W values per thread over the workgroup, waves and lanes in a fixed order; the result in thread 0
template <int W>
__device__ __forceinline__ void md_block_sum(double (&s)[W])
{
    __shared__ double sh[MD_BLOCK / WAVE][W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[w] += __shfl_xor(s[w], off);
    }
    const int wave = threadIdx.x / WAVE;
    if (lane_id() == 0) {
#pragma unroll
        for (int w = 0; w < W; ++w) sh[wave][w] = s[w];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < W; ++w) s[w] = (sh[0][w] + sh[1][w]) + (sh[2][w] + sh[3][w]);
    }
}
static_assert(MD_BLOCK == 4 * WAVE, "md_block_sum adds four waves");

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
        if (a.active[at]) {
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
