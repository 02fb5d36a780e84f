// Observables accumulated along a trajectory on the device (torchani_amd.md.RadialDistribution, MeanSquaredDisplacement,
// VelocityAutocorrelation).  include/anihip.h has the exact definition.
//
//   k_md_rdf          pair-distance histograms from neighbor rows: a workgroup owns a contiguous run of central atoms, one wave
//                     per atom and lanes over its row (as k_d3_cn); a uint32 histogram [P][bins] in LDS, added to the global
//                     uint64 counters by integer atomics, non-zero bins only, when the workgroup's entry changes (per_entry) and
//                     at its end.  Integer sums: the result does not depend on the order of arrival.
//   k_md_corr         one sample of a multiple-time-origin correlation: one thread per slot of the species-sorted gather table
//                     holds the sample in registers, writes it to ring slot k mod M and walks the lags with coalesced reads of the
//                     ring ([M][C][3][G]: a component of consecutive atoms is contiguous); per lag a butterfly over the wave for
//                     every species the wave holds, the four waves added in order in tiles of 64 lags
//   k_md_corr_finish  S[c][s][l] += the chunks' partial sums in ascending order
//
//   k_md_heat_flux    the three sums of the heat flux per entry (kinetic convective, potential convective, virial term) from
//                     per-atom inputs: chunks stride over the atoms of an entry, md_block_sum, k_md_heat_flux_finish adds the chunks
//
// The correlation and heat-flux kernels use no atomics and sum in a fixed order: two calls on the same input are bit-identical.  Tables live in
// device memory, so the kernels check every index they follow.
#include "anihip_common.h"
#include "md_sums.h"

namespace anihip {

constexpr int RDF_MAX_PAIRS = ANIHIP_MD_RDF_MAX_PAIRS, RDF_MAX_BINS = ANIHIP_MD_RDF_MAX_BINS;
constexpr int RDF_MIN_CHUNK = 16, RDF_MAX_BLOCKS = 2048;
constexpr int RDF_WAVES = MD_BLOCK / WAVE;
constexpr int CORR_TILE = 64;   // lags between two workgroup sums

struct RdfArgs {
    int64_t n, A, chunk, ent_capacity;
    int32_t P, bins, per_entry;
    double r_max, inv_delta;
    int8_t slot[64];
    const int32_t *species;
    const uint32_t *meta;
    const float4 *ent;
    unsigned long long *counts;
};

// the workgroup's histogram added to dst and cleared
__device__ __forceinline__ void rdf_flush(uint32_t *hist, int words, unsigned long long *dst)
{
    __syncthreads();   // (every wave's adds have landed)
    for (int w = threadIdx.x; w < words; w += MD_BLOCK) {
        const uint32_t v = hist[w];
        if (v) {
            atomicAdd(dst + w, (unsigned long long)v);
            hist[w] = 0;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void rdf_row(const RdfArgs &a, const int8_t *slot, int64_t i, uint32_t *hist)
{
    const int si = a.species[i];
    if (si < 0 || si >= 8) return;
    const uint32_t start = a.meta[(size_t)i * META_W], c = a.meta[(size_t)i * META_W + 1];
    const int nR = (int)(c & 0xFFFFu) + (int)(c >> 16);
    if (nR > MAXR || (int64_t)start + nR > a.ent_capacity) return;
    for (int k = lane_id(); k < nR; k += WAVE) {
        const float4 d = a.ent[start + k];
        const int p = slot[si * 8 + (int)((__float_as_uint(d.w) >> 28) & 7u)];
        if (p < 0) continue;
        const double r = sqrt((double)d.x * d.x + (double)d.y * d.y + (double)d.z * d.z);
        if (!(r < a.r_max)) continue;
        const int b = min((int)(r * a.inv_delta), a.bins - 1);
        atomicAdd(&hist[p * a.bins + b], 1u);
    }
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_rdf(RdfArgs a)
{
    extern __shared__ uint32_t rdf_hist[];
    __shared__ int8_t slot[64];
    const int64_t lo = blockIdx.x * a.chunk, hi = min(lo + a.chunk, a.n);
    if (lo >= hi) return;
    const int words = a.P * a.bins, wave = threadIdx.x / WAVE;
    for (int w = threadIdx.x; w < words; w += MD_BLOCK) rdf_hist[w] = 0;
    if (threadIdx.x < 64) slot[threadIdx.x] = a.slot[threadIdx.x];
    __syncthreads();
    // (everything that decides a flush is the same in every thread: the flush holds barriers)
    int64_t cur = a.per_entry ? lo / a.A : 0;
    for (int64_t base = lo; base < hi; base += RDF_WAVES) {
        const int64_t last = min(base + RDF_WAVES - 1, hi - 1);
        if (!a.per_entry || base / a.A == last / a.A) {
            const int64_t e = a.per_entry ? base / a.A : 0;
            if (e != cur) {
                rdf_flush(rdf_hist, words, a.counts + cur * words);
                cur = e;
            }
            if (base + wave <= last) rdf_row(a, slot, base + wave, rdf_hist);
        } else {   // the atoms of this round lie in more than one entry: one atom after the other
            for (int w = 0; base + w <= last; ++w) {
                const int64_t e = (base + w) / a.A;
                if (e != cur) {
                    rdf_flush(rdf_hist, words, a.counts + cur * words);
                    cur = e;
                }
                if (wave == w) rdf_row(a, slot, base + w, rdf_hist);
            }
        }
    }
    rdf_flush(rdf_hist, words, a.counts + cur * words);
}

struct CorrArgs {
    int64_t A, G, sample;
    int32_t n_mol, n_chunks, M, S;
    const int32_t *gather, *gather_species;
    const float *x, *x_lo;
    void *ring;
    double *part, *sums;
};

template <typename T, bool MSD>
__global__ __launch_bounds__(MD_BLOCK) void k_md_corr(CorrArgs a)
{
    __shared__ double sh[RDF_WAVES][CORR_TILE][MAX_S];
    const int c = blockIdx.x / a.n_chunks, chunk = blockIdx.x % a.n_chunks;
    const int wave = threadIdx.x / WAVE, lane = lane_id();
    const int64_t g = (int64_t)chunk * MD_BLOCK + threadIdx.x;
    int s = -1;
    double y[3] = {0.0, 0.0, 0.0};
    if (g < a.G) {
        const int idx = a.gather[(int64_t)c * a.G + g], sp = a.gather_species[(int64_t)c * a.G + g];
        if (idx >= 0 && idx < a.A && sp >= 0 && sp < a.S) {
            s = sp;
            const int64_t at = (int64_t)c * a.A + idx;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                y[d] = (double)a.x[3 * at + d];
                if (MSD && a.x_lo) y[d] += (double)a.x_lo[3 * at + d];
            }
        }
    }
    T *ring = (T *)a.ring;
    const int64_t slot_stride = (int64_t)a.n_mol * 3 * a.G, off = (int64_t)c * 3 * a.G + g;
    const int cur = (int)(a.sample % a.M);
    if (g < a.G) {   // (a skipped slot holds zeros: no slot of the ring is ever read before it was written)
#pragma unroll
        for (int d = 0; d < 3; ++d) ring[cur * slot_stride + off + d * a.G] = (T)y[d];
    }
    uint32_t present = 0;   // the species of this wave, the same in every lane
    for (int sp = 0; sp < a.S; ++sp)
        if (__ballot(s == sp)) present |= 1u << sp;
    const int L = (int)min(a.sample, (int64_t)a.M - 1);   // the last lag
    double *part = a.part + ((int64_t)c * a.n_chunks + chunk) * a.S * a.M;
    for (int l0 = 0; l0 <= L; l0 += CORR_TILE) {
        for (int w = threadIdx.x; w < RDF_WAVES * CORR_TILE * MAX_S; w += MD_BLOCK) (&sh[0][0][0])[w] = 0.0;
        __syncthreads();
        const int nl = min(CORR_TILE, L + 1 - l0);
        for (int t = 0; t < nl; ++t) {
            double term = 0.0;
            if (s >= 0) {
                int slot = cur - (l0 + t);
                if (slot < 0) slot += a.M;
                const T *p = ring + slot * slot_stride + off;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const double q = (double)p[d * a.G];
                    term += MSD ? (y[d] - q) * (y[d] - q) : y[d] * q;
                }
            }
            for (int sp = 0; sp < a.S; ++sp) {
                if (!(present >> sp & 1u)) continue;
                double v = s == sp ? term : 0.0;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
                if (lane == 0) sh[wave][t][sp] = v;
            }
        }
        __syncthreads();
        for (int w = threadIdx.x; w < nl * a.S; w += MD_BLOCK) {
            const int sp = w / nl, t = w % nl;
            part[(int64_t)sp * a.M + l0 + t] = (sh[0][t][sp] + sh[1][t][sp]) + (sh[2][t][sp] + sh[3][t][sp]);
        }
        __syncthreads();   // (sh is read until here)
    }
}
static_assert(RDF_WAVES == 4, "k_md_corr adds four waves");

__global__ __launch_bounds__(MD_BLOCK) void k_md_corr_finish(CorrArgs a, int L)
{
    const int64_t n = (int64_t)a.n_mol * a.S * (L + 1);
    for (int64_t w = blockIdx.x * (int64_t)MD_BLOCK + threadIdx.x; w < n; w += (int64_t)gridDim.x * MD_BLOCK) {
        const int64_t cs = w / (L + 1), l = w % (L + 1), c = cs / a.S, sp = cs % a.S;
        double acc = 0.0;
        for (int k = 0; k < a.n_chunks; ++k) acc += a.part[((c * a.n_chunks + k) * a.S + sp) * a.M + l];
        a.sums[cs * a.M + l] += acc;
    }
}

// ---- heat flux: the three sums of J per entry ------------------------------------------------------------------------------
struct FluxArgs {
    int64_t A;
    int32_t n_mol, n_chunks;
    const float *mass, *vel, *flux_atoms;
    const double *energy;
    const int32_t *species;
    double *part, *out;
};

constexpr int FLUX_MAX_CHUNKS = 1024;   // chunks of an entry: each strides over its atoms

// chunk k of entry c: atoms k MD_BLOCK + t, + n_chunks MD_BLOCK, ...; nine sums per thread, workgroup sum in a fixed order
__global__ __launch_bounds__(MD_BLOCK) void k_md_heat_flux(FluxArgs a)
{
    const int c = blockIdx.x / a.n_chunks, chunk = blockIdx.x % a.n_chunks;
    double s[9];
#pragma unroll
    for (int w = 0; w < 9; ++w) s[w] = 0.0;
    for (int64_t i = (int64_t)chunk * MD_BLOCK + threadIdx.x; i < a.A; i += (int64_t)a.n_chunks * MD_BLOCK) {
        const int64_t at = (int64_t)c * a.A + i;
        if (a.species[at] < 0) continue;
        const double vx = (double)a.vel[3 * at], vy = (double)a.vel[3 * at + 1], vz = (double)a.vel[3 * at + 2];
        const double ke = 0.5 * (double)a.mass[at] * (vx * vx + vy * vy + vz * vz) * (1.0 / ANIHIP_MD_ACC_UNIT);
        const double e = a.energy[at];
        s[0] += ke * vx; s[1] += ke * vy; s[2] += ke * vz;
        s[3] += e * vx; s[4] += e * vy; s[5] += e * vz;
        s[6] -= (double)a.flux_atoms[3 * at]; s[7] -= (double)a.flux_atoms[3 * at + 1]; s[8] -= (double)a.flux_atoms[3 * at + 2];
    }
    md_block_sum<9>(s);
    if (threadIdx.x == 0) {
        double *dst = a.n_chunks == 1 ? a.out + (int64_t)c * 9 : a.part + ((int64_t)c * a.n_chunks + chunk) * 9;
#pragma unroll
        for (int w = 0; w < 9; ++w) dst[w] = s[w];
    }
}

// out[c][w] = the chunks' partial sums in ascending order
__global__ __launch_bounds__(MD_BLOCK) void k_md_heat_flux_finish(FluxArgs a)
{
    const int64_t w = blockIdx.x * (int64_t)MD_BLOCK + threadIdx.x;
    if (w >= (int64_t)a.n_mol * 9) return;
    const int64_t c = w / 9, q = w % 9;
    double acc = 0.0;
    for (int k = 0; k < a.n_chunks; ++k) acc += a.part[(c * a.n_chunks + k) * 9 + q];
    a.out[w] = acc;
}

static int flux_chunks(int64_t atoms_per_mol)
{
    return (int)std::min<int64_t>((atoms_per_mol + MD_BLOCK - 1) / MD_BLOCK, FLUX_MAX_CHUNKS);
}

}  // namespace anihip

using namespace anihip;

extern "C" size_t anihip_md_heat_flux_workspace_bytes(int64_t n_mol, int64_t atoms_per_mol)
{
    if (n_mol < 1 || atoms_per_mol < 1) {
        set_error("anihip_md_heat_flux_workspace_bytes: n_mol and atoms_per_mol must be >= 1");
        return 0;
    }
    return (size_t)n_mol * (size_t)flux_chunks(atoms_per_mol) * 9 * sizeof(double);
}

extern "C" int anihip_md_heat_flux(void *stream, const anihip_md_params *params, const float *masses, const double *atomic_energies,
                                   const int32_t *species, const float *velocities, const float *flux_atoms, double *flux,
                                   void *workspace, size_t workspace_bytes)
{
    ANIHIP_REQUIRE(params && masses && atomic_energies && species && velocities && flux_atoms && flux, "null pointer argument");
    ANIHIP_REQUIRE(params->n_mol >= 1 && params->atoms_per_mol >= 1, "n_mol and atoms_per_mol must be >= 1");
    FluxArgs a{};
    a.A = params->atoms_per_mol, a.n_mol = params->n_mol, a.n_chunks = flux_chunks(params->atoms_per_mol);
    ANIHIP_REQUIRE((int64_t)a.n_mol * a.n_chunks < ((int64_t)1 << 31), "entries x chunks must stay below 2^31");
    if (a.n_chunks > 1) {
        const size_t need = anihip_md_heat_flux_workspace_bytes(a.n_mol, a.A);
        ANIHIP_REQUIRE(workspace && workspace_bytes >= need, "workspace holds %zu bytes, %zu needed", workspace_bytes, need);
    }
    a.mass = masses, a.vel = velocities, a.flux_atoms = flux_atoms, a.energy = atomic_energies, a.species = species;
    a.part = (double *)workspace, a.out = flux;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_md_heat_flux, dim3((unsigned)(a.n_mol * a.n_chunks)), dim3(MD_BLOCK), 0, st, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    if (a.n_chunks > 1) {
        hipLaunchKernelGGL(k_md_heat_flux_finish, dim3((unsigned)(((int64_t)a.n_mol * 9 + MD_BLOCK - 1) / MD_BLOCK)),
                           dim3(MD_BLOCK), 0, st, a);
        ANIHIP_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int anihip_md_rdf_accumulate(void *stream, const anihip_md_params *params, int32_t n_pairs, int32_t bins, double r_max,
                                        int32_t per_entry, const int8_t *pair_slot, const int32_t *species, const uint32_t *meta,
                                        const float *ent, int64_t ent_capacity, uint64_t *counts)
{
    ANIHIP_REQUIRE(params && pair_slot && species && meta && ent && counts, "null pointer argument");
    ANIHIP_REQUIRE(params->n_mol >= 1 && params->atoms_per_mol >= 1, "n_mol and atoms_per_mol must be >= 1");
    ANIHIP_REQUIRE(n_pairs >= 1 && n_pairs <= RDF_MAX_PAIRS && bins >= 1 && bins <= RDF_MAX_BINS && n_pairs * bins <= 8192,
                   "n_pairs must be in 1 .. %d, bins in 1 .. %d and n_pairs x bins <= 8192, got %d and %d", RDF_MAX_PAIRS,
                   RDF_MAX_BINS, n_pairs, bins);
    ANIHIP_REQUIRE(r_max > 0.0 && r_max < 1e30, "r_max must be > 0, got %g", r_max);
    ANIHIP_REQUIRE(ent_capacity >= 0, "ent_capacity must be >= 0");
    RdfArgs a{};
    a.n = (int64_t)params->n_mol * params->atoms_per_mol, a.A = params->atoms_per_mol, a.ent_capacity = ent_capacity;
    ANIHIP_REQUIRE(a.n < ((int64_t)1 << 31), "n_mol x atoms_per_mol must stay below 2^31");
    for (int k = 0; k < 64; ++k) {
        ANIHIP_REQUIRE(pair_slot[k] >= -1 && pair_slot[k] < n_pairs, "pair_slot[%d] = %d is not a pair below %d or -1", k,
                       (int)pair_slot[k], n_pairs);
        a.slot[k] = pair_slot[k];
    }
    a.P = n_pairs, a.bins = bins, a.per_entry = per_entry ? 1 : 0, a.r_max = r_max, a.inv_delta = (double)bins / r_max;
    a.species = species, a.meta = meta, a.ent = (const float4 *)ent, a.counts = (unsigned long long *)counts;
    // (a workgroup's uint32 histogram takes at most chunk x 256 row entries: chunk stays below 2^31 / 2048)
    int64_t blocks = std::min<int64_t>((a.n + RDF_MIN_CHUNK - 1) / RDF_MIN_CHUNK, RDF_MAX_BLOCKS);
    a.chunk = ((a.n + blocks - 1) / blocks + RDF_WAVES - 1) / RDF_WAVES * RDF_WAVES;
    blocks = (a.n + a.chunk - 1) / a.chunk;
    hipLaunchKernelGGL(k_md_rdf, dim3((unsigned)blocks), dim3(MD_BLOCK), (size_t)n_pairs * bins * sizeof(uint32_t),
                       (hipStream_t)stream, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" size_t anihip_md_corr_workspace_bytes(int64_t n_mol, int64_t max_atoms, int64_t lags, int64_t n_species)
{
    if (n_mol < 1 || max_atoms < 1 || lags < 1 || n_species < 1) {
        set_error("anihip_md_corr_workspace_bytes: n_mol, max_atoms, lags and n_species must be >= 1");
        return 0;
    }
    return (size_t)n_mol * (size_t)((max_atoms + MD_BLOCK - 1) / MD_BLOCK) * (size_t)n_species * (size_t)lags * sizeof(double);
}

extern "C" int anihip_md_corr_accumulate(void *stream, const anihip_md_params *params, int32_t kind, int32_t lags,
                                         int32_t n_species, int32_t max_atoms, int64_t sample, const int32_t *gather,
                                         const int32_t *gather_species, const float *x, const float *x_lo, void *ring, double *S,
                                         void *workspace, size_t workspace_bytes)
{
    ANIHIP_REQUIRE(params && gather && gather_species && x && ring && S, "null pointer argument");
    ANIHIP_REQUIRE(params->n_mol >= 1 && params->atoms_per_mol >= 1, "n_mol and atoms_per_mol must be >= 1");
    ANIHIP_REQUIRE(kind == ANIHIP_MD_CORR_MSD || kind == ANIHIP_MD_CORR_VACF, "unknown correlation kind %d", kind);
    ANIHIP_REQUIRE(lags >= 1 && lags <= 65536 && n_species >= 1 && n_species <= MAX_S && max_atoms >= 1 && sample >= 0,
                   "lags must be in 1 .. 65536, n_species in 1 .. %d, max_atoms >= 1 and sample >= 0", MAX_S);
    ANIHIP_REQUIRE(max_atoms <= params->atoms_per_mol, "max_atoms = %d exceeds atoms_per_mol = %d", max_atoms,
                   params->atoms_per_mol);
    ANIHIP_REQUIRE((int64_t)params->n_mol * params->atoms_per_mol < ((int64_t)1 << 31),
                   "n_mol x atoms_per_mol must stay below 2^31");
    const size_t need = anihip_md_corr_workspace_bytes(params->n_mol, max_atoms, lags, n_species);
    ANIHIP_REQUIRE(workspace && workspace_bytes >= need, "workspace holds %zu bytes, %zu needed", workspace_bytes, need);
    CorrArgs a{};
    a.A = params->atoms_per_mol, a.G = max_atoms, a.sample = sample;
    a.n_mol = params->n_mol, a.n_chunks = (int32_t)((max_atoms + MD_BLOCK - 1) / MD_BLOCK), a.M = lags, a.S = n_species;
    ANIHIP_REQUIRE((int64_t)a.n_mol * a.n_chunks < ((int64_t)1 << 31), "entries x chunks must stay below 2^31");
    a.gather = gather, a.gather_species = gather_species, a.x = x, a.x_lo = x_lo, a.ring = ring;
    a.part = (double *)workspace, a.sums = S;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(a.n_mol * a.n_chunks));
    if (kind == ANIHIP_MD_CORR_MSD)
        hipLaunchKernelGGL((k_md_corr<double, true>), grid, dim3(MD_BLOCK), 0, st, a);
    else
        hipLaunchKernelGGL((k_md_corr<float, false>), grid, dim3(MD_BLOCK), 0, st, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    const int L = (int)std::min<int64_t>(sample, (int64_t)lags - 1);
    const int64_t n = (int64_t)a.n_mol * a.S * (L + 1);
    hipLaunchKernelGGL(k_md_corr_finish, dim3((unsigned)std::min<int64_t>((n + MD_BLOCK - 1) / MD_BLOCK, 4096)), dim3(MD_BLOCK),
                       0, st, a, L);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}
