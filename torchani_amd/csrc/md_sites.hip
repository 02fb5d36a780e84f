// Group collective variables of biased MD (torchani_amd.md.center, md.coordination): centres of groups of atoms and coordination
// numbers enter the unchanged kernels of md_bias.hip as SITES, pseudo-atoms appended to every entry.  include/anihip.h has the
// exact definition.
//
//   k_md_sites_coord    one workgroup per (coordination CV, chunk of 256 atoms of its group A, tile of 256 atoms of group B): one
//                       thread per atom of A loops over the tile, staged in LDS; the sum by md_block_sum to the workspace
//   k_md_sites_gather   per entry, one workgroup per chunk of 256 real atoms (coordinates and forces copied to the extended
//                       arrays) and one more for the sites: it checks the entry's tables, then writes every site (a centre by
//                       one strided sum and md_block_sum, a coordination number by its partial sums in (chunk, tile) order)
//   k_md_sites_spread   one workgroup per (entry, chunk of 64 atoms), four threads per atom: the force that anihip_md_bias_apply
//                       left on the sites carried back to the atoms through the inverse table atom -> (site, role, weight), in
//                       fp64, one fp32 rounding; the workgroup walks the entry's sites together, so the other group of a
//                       coordination number is staged through LDS, a quarter of every tile to each of an atom's threads
//
// Everything is fp64 on x = coords + coords_lo.  No atomics on memory and every sum in a fixed order: two calls on the same input
// are bit-identical, and an entry gives the same bits wherever it sits in the batch.  Tables live in device memory, so the
// kernels check every index they follow.
#include "anihip_common.h"
#include "md_sums.h"

namespace anihip {

constexpr int SITES_MAX = ANIHIP_MD_SITES_MAX;
static_assert(SITES_MAX <= MD_BLOCK, "the site workgroup has one thread per site when it places the sites of a bad entry");

struct SitesArgs {
    int64_t A, Ax;      // atoms of an entry, and of an extended entry (A + max_sites)
    int32_t n_chunks;   // chunks of 256 atoms of an entry
    const float *coords, *coords_lo, *forces_in;
    float *coords_ext, *coords_lo_ext, *forces_ext, *forces_out;
    double *part;       // [Nq][n_chunks][n_chunks]
};

struct SitesSwitch {
    double r0, d0, r_max, b;
    double r_max2;   // r_max^2 (1 + 1e-12): a squared distance above it is surely beyond r_max
    int n;
};

struct SitesCoord {
    int c, v, a_lo, a_n, b_lo, b_n;
    SitesSwitch p;
};

__device__ __forceinline__ void sites_x(const float *coords, const float *coords_lo, int64_t at, double (&x)[3])
{
#pragma unroll
    for (int d = 0; d < 3; ++d) x[d] = (double)coords[3 * at + d] + (double)coords_lo[3 * at + d];
}

// d brought to its nearest image along the periodic directions (rows of cell are the lattice vectors)
__device__ __forceinline__ void sites_mic(const anihip_md_sites &s, double (&d)[3])
{
    if (!(s.pbc[0] | s.pbc[1] | s.pbc[2])) return;
    double n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        n[k] = s.pbc[k] ? rint(d[0] * s.inv_cell[k] + d[1] * s.inv_cell[3 + k] + d[2] * s.inv_cell[6 + k]) : 0.0;
    const double d0 = d[0], d1 = d[1], d2 = d[2];
    d[0] = d0 - (n[0] * s.cell[0] + n[1] * s.cell[3] + n[2] * s.cell[6]);
    d[1] = d1 - (n[0] * s.cell[1] + n[1] * s.cell[4] + n[2] * s.cell[7]);
    d[2] = d2 - (n[0] * s.cell[2] + n[1] * s.cell[5] + n[2] * s.cell[8]);
}

// sw(r) and dsw/dr (include/anihip.h): x^n by repeated multiplication
__device__ __forceinline__ void sites_switch(const SitesSwitch &p, double r, double &sw, double &dsw)
{
    sw = dsw = 0.0;
    if (!(r < p.r_max)) return;
    const double x = fmax(r - p.d0, 0.0) / p.r0;
    double pm = x;   // x^(n - 1)
    for (int k = 2; k < p.n; ++k) pm *= x;
    const double q = 1.0 + pm * x;
    sw = (1.0 / q - p.b) / (1.0 - p.b);
    if (r > p.d0) dsw = -(double)p.n * pm / (p.r0 * (q * q)) / (1.0 - p.b);
}

// the atoms group_offset[g] .. group_offset[g + 1] - 1 of group g: false for an offset that falls or leaves 0 .. n_group_atoms
__device__ __forceinline__ bool sites_group(const anihip_md_sites &s, int g, int &lo, int &n)
{
    if (g < 0 || g >= s.n_groups) return false;
    lo = s.group_offset[g];
    const int hi = s.group_offset[g + 1];
    n = hi - lo;
    return lo >= 0 && hi >= lo && hi <= s.n_group_atoms;
}

// row q of the coordination tables with both its groups: false for anything out of range
__device__ __forceinline__ bool sites_coord_load(const anihip_md_sites &s, int q, SitesCoord &k)
{
    if (q < 0 || q >= s.n_coord) return false;
    const int32_t *row = s.coord + 5 * (int64_t)q;
    k.c = row[0], k.v = row[3], k.p.n = row[4];
    if (k.c < 0 || k.c >= s.n_entries || k.v < 1 || k.v >= s.max_sites || k.p.n < 2 || k.p.n > 32) return false;
    if (!sites_group(s, row[1], k.a_lo, k.a_n) || !sites_group(s, row[2], k.b_lo, k.b_n)) return false;
    const double *p = s.coord_params + 4 * (int64_t)q;
    k.p.r0 = p[0], k.p.d0 = p[1], k.p.r_max = p[2], k.p.b = p[3];
    k.p.r_max2 = k.p.r_max * k.p.r_max * (1.0 + 1e-12);
    return k.p.r0 > 0.0 && k.p.d0 >= 0.0 && k.p.r_max > k.p.d0 && k.p.b >= 0.0 && k.p.b < 1.0;
}

// Atom i (position xi, index gi) against the n <= 64 atoms base .. base + n - 1 staged in LDS, in ascending order:
// add(sw, dsw, d, r) for every atom that may lie within r_max.  Two passes: the first marks those atoms one bit each (no square
// root, no division, the same work in every lane), the second visits the marked ones -- few of them when r_max is short against
// the group's extent, so the lanes of a wave do not all pay the switching function for a pair that one of them has within reach.
template <typename F>
__device__ __forceinline__ void sites_word_pairs(const anihip_md_sites &s, const SitesSwitch &p, const double (&xi)[3], int64_t gi,
                                                 const double (*sh_x)[3], const int32_t *sh_at, int base, int n, F &&add)
{
    uint64_t near = 0;
#pragma unroll 4
    for (int b = 0; b < n; ++b) {
        const int u = base + b;
        double d[3] = {xi[0] - sh_x[u][0], xi[1] - sh_x[u][1], xi[2] - sh_x[u][2]};
        sites_mic(s, d);
        const double r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        // (a squared distance above r_max2 is surely beyond r_max: sw = dsw = 0)
        const bool in = sh_at[u] >= 0 && sh_at[u] != gi && !(r2 > p.r_max2);
        near |= (uint64_t)in << b;
    }
    for (; near; near &= near - 1) {
        const int u = base + __ffsll((unsigned long long)near) - 1;
        double d[3] = {xi[0] - sh_x[u][0], xi[1] - sh_x[u][1], xi[2] - sh_x[u][2]};
        sites_mic(s, d);
        const double r = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        double sw, dsw;
        sites_switch(p, r, sw, dsw);
        add(sw, dsw, d, r);
    }
}

// the same against a whole tile of n_tile <= 256 atoms
template <typename F>
__device__ __forceinline__ void sites_tile_pairs(const anihip_md_sites &s, const SitesSwitch &p, const double (&xi)[3], int64_t gi,
                                                 const double (*sh_x)[3], const int32_t *sh_at, int n_tile, F &&add)
{
#pragma unroll
    for (int w = 0; w < MD_BLOCK / WAVE; ++w) sites_word_pairs(s, p, xi, gi, sh_x, sh_at, WAVE * w, min(WAVE, n_tile - WAVE * w), add);
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_sites_coord(SitesArgs a, anihip_md_sites s)
{
    const int tb = blockIdx.x % a.n_chunks, j = (blockIdx.x / a.n_chunks) % a.n_chunks, t = threadIdx.x;
    const int q = blockIdx.x / (a.n_chunks * a.n_chunks), tile = tb * MD_BLOCK;
    SitesCoord k;
    // (the same for every thread; the gather reports a broken row)
    if (!sites_coord_load(s, q, k) || j * MD_BLOCK >= k.a_n || tile >= k.b_n) return;
    __shared__ double sh_x[MD_BLOCK][3];
    __shared__ int32_t sh_at[MD_BLOCK];
    const int64_t first = (int64_t)k.c * a.A, end = first + a.A;
    int64_t gi = -1;
    double xi[3] = {0.0, 0.0, 0.0};
    if (j * MD_BLOCK + t < k.a_n) {
        gi = s.group_atoms[k.a_lo + j * MD_BLOCK + t];
        if (gi < first || gi >= end) gi = -1;
        else sites_x(a.coords, a.coords_lo, gi, xi);
    }
    if (tile + t < k.b_n) {
        int64_t gj = s.group_atoms[k.b_lo + tile + t];
        if (gj < first || gj >= end) gj = -1;
        sh_at[t] = (int32_t)gj;
        if (gj >= 0) sites_x(a.coords, a.coords_lo, gj, sh_x[t]);
    }
    __syncthreads();
    double sum[1] = {0.0};
    if (gi >= 0)
        sites_tile_pairs(s, k.p, xi, gi, sh_x, sh_at, min(MD_BLOCK, k.b_n - tile),
                         [&](double sw, double, const double (&)[3], double) { sum[0] += sw; });
    md_block_sum<1>(sum);
    if (t == 0) a.part[((int64_t)q * a.n_chunks + j) * a.n_chunks + tb] = sum[0];
}

// ANIHIP_MD_SITES_BAD_GROUP if an atom of the group's lies outside the entry (every thread takes a stride of the group)
__device__ __forceinline__ int sites_group_atoms(const anihip_md_sites &s, int lo, int n, int64_t first, int64_t end)
{
    int bad = 0;
    for (int u = threadIdx.x; u < n; u += MD_BLOCK) {
        const int64_t at = s.group_atoms[lo + u];
        if (at < first || at >= end) bad = ANIHIP_MD_SITES_BAD_GROUP;
    }
    return bad;
}

__device__ __forceinline__ void sites_write(const SitesArgs &a, int64_t at, double x, double y, double z)
{
    const double p[3] = {x, y, z};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float hi = (float)p[d];
        a.coords_ext[3 * at + d] = hi, a.coords_lo_ext[3 * at + d] = (float)(p[d] - (double)hi), a.forces_ext[3 * at + d] = 0.0f;
    }
}

__global__ __launch_bounds__(MD_BLOCK) void k_md_sites_gather(SitesArgs a, anihip_md_sites s)
{
    const int64_t c = blockIdx.x / (a.n_chunks + 1);
    const int j = blockIdx.x % (a.n_chunks + 1), t = threadIdx.x, V = s.max_sites;
    if (j < a.n_chunks) {   // the real atoms of chunk j
        const int64_t i = (int64_t)j * MD_BLOCK + t;
        if (i >= a.A) return;
        const int64_t src = 3 * (c * a.A + i), dst = 3 * (c * a.Ax + i);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            a.coords_ext[dst + d] = a.coords[src + d], a.coords_lo_ext[dst + d] = a.coords_lo[src + d];
            a.forces_ext[dst + d] = a.forces_in[src + d];
        }
        return;
    }
    // ---- the sites of entry c: first every table the entry's sites and atoms name ----
    __shared__ int sh_bad;
    if (t == 0) sh_bad = 0;
    __syncthreads();
    const int64_t first = c * a.A, end = first + a.A;
    const int32_t *kinds = s.site_kind + c * V, *refs = s.site_ref + c * V;
    int bad = 0;
    for (int v = 0; v < V; ++v) {   // (the same trip for every thread)
        const int kind = kinds[v], ref = refs[v];
        if (kind == ANIHIP_MD_SITE_NONE) continue;
        if (kind == ANIHIP_MD_SITE_CENTER) {
            int lo, n;
            if (!sites_group(s, ref, lo, n) || n < 1 || n > a.A) bad |= ANIHIP_MD_SITES_BAD_SITE;
            else bad |= sites_group_atoms(s, lo, n, first, end);
        } else if (kind == ANIHIP_MD_SITE_ANCHOR) {
            if (v + 1 >= V || kinds[v + 1] != ANIHIP_MD_SITE_VALUE || refs[v + 1] != ref) bad |= ANIHIP_MD_SITES_BAD_SITE;
        } else if (kind == ANIHIP_MD_SITE_VALUE) {
            SitesCoord k;
            if (!sites_coord_load(s, ref, k) || k.c != c || k.v != v || kinds[v - 1] != ANIHIP_MD_SITE_ANCHOR || refs[v - 1] != ref
                || k.a_n < 1 || k.a_n > a.A || k.b_n < 1 || k.b_n > a.A)
                bad |= ANIHIP_MD_SITES_BAD_SITE;   // (k.v == v >= 1: v - 1 is a slot)
            else
                bad |= sites_group_atoms(s, k.a_lo, k.a_n, first, end) | sites_group_atoms(s, k.b_lo, k.b_n, first, end);
        } else {
            bad |= ANIHIP_MD_SITES_BAD_SITE;
        }
    }
    for (int64_t i = t; i < a.A; i += MD_BLOCK) {   // the inverse table of the entry's atoms
        const int lo = s.member_offset[first + i], hi = s.member_offset[first + i + 1];
        if (lo < 0 || hi < lo || hi > s.n_members) {
            bad |= ANIHIP_MD_SITES_BAD_MEMBER;
            continue;
        }
        for (int m = lo; m < hi; ++m) {
            const int v = s.member_site[2 * (int64_t)m], role = s.member_site[2 * (int64_t)m + 1];
            if (v < 0 || v >= V || role < ANIHIP_MD_SITE_ROLE_CENTER || role > ANIHIP_MD_SITE_ROLE_B
                || kinds[v] != (role == ANIHIP_MD_SITE_ROLE_CENTER ? ANIHIP_MD_SITE_CENTER : ANIHIP_MD_SITE_VALUE))
                bad |= ANIHIP_MD_SITES_BAD_MEMBER;
        }
    }
    if (bad) atomicOr(&sh_bad, bad);   // (on LDS, an integer: the order does not matter)
    __syncthreads();
    bad = sh_bad;
    if (t == 0) s.status[c] = bad;
    if (bad) {   // finite geometry for the bias kernels: site v at (v + 1, 0, 0)
        if (t < V && kinds[t] != ANIHIP_MD_SITE_NONE) sites_write(a, c * a.Ax + a.A + t, (double)(t + 1), 0.0, 0.0);
        return;
    }
    // ---- then the sites, one after the other ----
    for (int v = 0; v < V; ++v) {
        const int kind = kinds[v], ref = refs[v];
        const int64_t at = c * a.Ax + a.A + v;
        if (kind == ANIHIP_MD_SITE_CENTER) {
            int lo, n;
            sites_group(s, ref, lo, n);
            double x[3] = {0.0, 0.0, 0.0};
            for (int u = t; u < n; u += MD_BLOCK) {   // thread t adds the atoms t, t + 256, ... in that order
                double xa[3];
                sites_x(a.coords, a.coords_lo, s.group_atoms[lo + u], xa);
                const double w = s.group_weights[lo + u];
                x[0] += w * xa[0], x[1] += w * xa[1], x[2] += w * xa[2];
            }
            md_block_sum<3>(x);
            if (t == 0) sites_write(a, at, x[0], x[1], x[2]);
            __syncthreads();   // (md_block_sum's LDS is read by thread 0 until here)
        } else if (kind == ANIHIP_MD_SITE_ANCHOR) {
            if (t == 0) sites_write(a, at, 0.0, 0.0, 0.0);
        } else if (kind == ANIHIP_MD_SITE_VALUE && t == 0) {
            SitesCoord k;
            sites_coord_load(s, ref, k);
            const int chunks_a = (k.a_n + MD_BLOCK - 1) / MD_BLOCK, chunks_b = (k.b_n + MD_BLOCK - 1) / MD_BLOCK;
            double sum = 0.0;
            for (int jc = 0; jc < chunks_a; ++jc)
                for (int tb = 0; tb < chunks_b; ++tb) sum += a.part[((int64_t)ref * a.n_chunks + jc) * a.n_chunks + tb];
            sites_write(a, at, fmax(sum, 0x1p-64), 0.0, 0.0);
        }
    }
}

// One workgroup per (entry, chunk of SPREAD_ATOMS atoms), four threads per atom: lane l of every wave works for atom l of the
// chunk, and wave w takes the quarter w of every staged tile.  The four keep the same cursor and the same sums (the quarters'
// sums are exchanged through LDS and added in a fixed order), and wave 0 writes.
constexpr int SPREAD_ATOMS = WAVE, SPREAD_PARTS = MD_BLOCK / WAVE;
static_assert(SPREAD_PARTS == 4, "k_md_sites_spread adds four partial sums");

__global__ __launch_bounds__(MD_BLOCK) void k_md_sites_spread(SitesArgs a, anihip_md_sites s, int n_chunks)
{
    const int64_t c = blockIdx.x / n_chunks;
    const int t = threadIdx.x, V = s.max_sites, lane = t % WAVE, part = t / WAVE;
    const int64_t i = (int64_t)(blockIdx.x % n_chunks) * SPREAD_ATOMS + lane;
    if (s.status[c] != 0) return;   // (status: what k_md_sites_gather found; such an entry keeps the model's forces)
    const bool real = i < a.A;      // (the other threads of the last chunk still stage the groups)
    const int64_t first = c * a.A, end = first + a.A, gi = first + i, sites = c * a.Ax + a.A;
    const int32_t *kinds = s.site_kind + c * V, *refs = s.site_ref + c * V;
    int m = 0, hi = 0;   // the atom's rows of the inverse table still to come, in ascending slot order
    double acc[3] = {0.0, 0.0, 0.0}, xi[3] = {0.0, 0.0, 0.0};
    if (real) {
        const float *fe = a.forces_ext + 3 * (c * a.Ax + i);
        acc[0] = (double)fe[0], acc[1] = (double)fe[1], acc[2] = (double)fe[2];
        m = s.member_offset[gi], hi = s.member_offset[gi + 1];
        if (m < 0 || hi < m || hi > s.n_members) hi = m = 0;
        if (hi > m) sites_x(a.coords, a.coords_lo, gi, xi);
    }
    __shared__ double sh_x[MD_BLOCK][3], sh_g[SPREAD_PARTS][SPREAD_ATOMS][3];
    __shared__ int32_t sh_at[MD_BLOCK];
    for (int v = 0; v < V; ++v) {   // in site order (the same trip for every thread)
        const int kind = kinds[v];
        if (kind != ANIHIP_MD_SITE_CENTER && kind != ANIHIP_MD_SITE_VALUE) continue;
        const float *fs = a.forces_ext + 3 * (sites + v);
        while (m < hi && s.member_site[2 * (int64_t)m] < v) ++m;
        if (kind == ANIHIP_MD_SITE_CENTER) {
            if (m < hi && s.member_site[2 * (int64_t)m] == v && s.member_site[2 * (int64_t)m + 1] == ANIHIP_MD_SITE_ROLE_CENTER) {
                const double w = s.member_weight[m];
                acc[0] += w * (double)fs[0], acc[1] += w * (double)fs[1], acc[2] += w * (double)fs[2];
                ++m;
            }
            continue;
        }
        SitesCoord k;
        if (!sites_coord_load(s, refs[v], k) || k.c != c) continue;
        const double G = (double)fs[0];   // -dE/ds, as anihip_md_bias_apply rounded it
        for (int role = ANIHIP_MD_SITE_ROLE_A; role <= ANIHIP_MD_SITE_ROLE_B; ++role) {
            const bool mine = m < hi && s.member_site[2 * (int64_t)m] == v && s.member_site[2 * (int64_t)m + 1] == role;
            if (!__syncthreads_or(mine)) continue;   // no atom of this chunk is on this side
            // the other group, staged through LDS: ds/dx_i = sum_j dsw/dr(r_ij) (x_i - x_j) / r_ij whichever side i is on
            const int o_lo = role == ANIHIP_MD_SITE_ROLE_A ? k.b_lo : k.a_lo, o_n = role == ANIHIP_MD_SITE_ROLE_A ? k.b_n : k.a_n;
            double g[3] = {0.0, 0.0, 0.0};
            for (int tile = 0; tile < o_n; tile += MD_BLOCK) {
                __syncthreads();
                if (tile + t < o_n) {
                    int64_t gj = s.group_atoms[o_lo + tile + t];
                    if (gj < first || gj >= end) gj = -1;
                    sh_at[t] = (int32_t)gj;
                    if (gj >= 0) sites_x(a.coords, a.coords_lo, gj, sh_x[t]);
                }
                __syncthreads();
                if (!mine) continue;
                const int n_tile = min(MD_BLOCK, o_n - tile);
                sites_word_pairs(s, k.p, xi, gi, sh_x, sh_at, WAVE * part, min(WAVE, n_tile - WAVE * part),
                                 [&](double, double dsw, const double (&d)[3], double r) {
                                     if (dsw != 0.0) g[0] += dsw * (d[0] / r), g[1] += dsw * (d[1] / r), g[2] += dsw * (d[2] / r);
                                 });
            }
            sh_g[part][lane][0] = g[0], sh_g[part][lane][1] = g[1], sh_g[part][lane][2] = g[2];
            __syncthreads();
            if (mine) {
#pragma unroll
                for (int d = 0; d < 3; ++d)
                    acc[d] += G * ((sh_g[0][lane][d] + sh_g[1][lane][d]) + (sh_g[2][lane][d] + sh_g[3][lane][d]));
                ++m;
            }
            __syncthreads();   // (sh_g is read until here)
        }
    }
    if (real && part == 0) {
        float *out = a.forces_out + 3 * gi;
        out[0] = (float)acc[0], out[1] = (float)acc[1], out[2] = (float)acc[2];
    }
}

// what the host can see of the tables
static int sites_args(const anihip_md_params *params, const anihip_md_sites *sites, SitesArgs &a)
{
    ANIHIP_REQUIRE(params && sites, "null pointer argument");
    const anihip_md_sites &s = *sites;
    ANIHIP_REQUIRE(params->n_mol >= 1 && params->atoms_per_mol >= 1, "n_mol and atoms_per_mol must be >= 1");
    ANIHIP_REQUIRE(s.n_entries == params->n_mol, "site tables of %d entries for a batch of %d", s.n_entries, params->n_mol);
    ANIHIP_REQUIRE(s.max_sites >= 1 && s.max_sites <= SITES_MAX, "max_sites must be in 1 .. %d, got %d", SITES_MAX, s.max_sites);
    ANIHIP_REQUIRE(s.n_groups >= 0 && s.n_group_atoms >= 0 && s.n_coord >= 0 && s.n_members >= 0,
                   "n_groups, n_group_atoms, n_coord and n_members must be >= 0");
    ANIHIP_REQUIRE((int64_t)params->n_mol * ((int64_t)params->atoms_per_mol + s.max_sites) < ((int64_t)1 << 31),
                   "n_mol x (atoms_per_mol + max_sites) must stay below 2^31");
    ANIHIP_REQUIRE(s.site_kind && s.site_ref && s.group_offset && s.member_offset && s.status, "null pointer in the site tables");
    ANIHIP_REQUIRE(s.n_group_atoms == 0 || (s.group_atoms && s.group_weights), "null pointer in the group tables");
    ANIHIP_REQUIRE(s.n_coord == 0 || (s.coord && s.coord_params), "null pointer in the coordination tables");
    ANIHIP_REQUIRE(s.n_members == 0 || (s.member_site && s.member_weight), "null pointer in the inverse tables");
    a.A = params->atoms_per_mol, a.Ax = a.A + s.max_sites;
    a.n_chunks = (int32_t)((a.A + MD_BLOCK - 1) / MD_BLOCK);
    ANIHIP_REQUIRE((int64_t)params->n_mol * (a.n_chunks + 1) < ((int64_t)1 << 31)
                       && (int64_t)s.n_coord * a.n_chunks * a.n_chunks < ((int64_t)1 << 31),
                   "entries x chunks and coordination numbers x chunks^2 must stay below 2^31");
    return 0;
}

}  // namespace anihip

using namespace anihip;

extern "C" size_t anihip_md_sites_workspace_bytes(const anihip_md_params *params, const anihip_md_sites *sites)
{
    if (!params || !sites || params->atoms_per_mol < 1 || sites->n_coord < 0) {
        set_error("anihip_md_sites_workspace_bytes: atoms_per_mol must be >= 1 and n_coord >= 0");
        return 0;
    }
    const size_t chunks = (size_t)((params->atoms_per_mol + MD_BLOCK - 1) / MD_BLOCK);
    return (size_t)sites->n_coord * chunks * chunks * sizeof(double);
}

extern "C" int anihip_md_sites_gather(void *stream, const anihip_md_params *params, const anihip_md_sites *sites,
                                      const float *coords, const float *coords_lo, const float *forces, float *coords_ext,
                                      float *coords_lo_ext, float *forces_ext, void *workspace, size_t workspace_bytes)
{
    SitesArgs a{};
    if (int rc = sites_args(params, sites, a)) return rc;
    ANIHIP_REQUIRE(coords && coords_lo && forces && coords_ext && coords_lo_ext && forces_ext, "null pointer argument");
    const size_t need = anihip_md_sites_workspace_bytes(params, sites);
    ANIHIP_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "workspace holds %zu bytes, %zu needed", workspace_bytes, need);
    a.coords = coords, a.coords_lo = coords_lo, a.forces_in = forces;
    a.coords_ext = coords_ext, a.coords_lo_ext = coords_lo_ext, a.forces_ext = forces_ext, a.part = (double *)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (sites->n_coord > 0) {
        hipLaunchKernelGGL(k_md_sites_coord, dim3((unsigned)(sites->n_coord * a.n_chunks * a.n_chunks)), dim3(MD_BLOCK), 0, st, a,
                           *sites);
        ANIHIP_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_md_sites_gather, dim3((unsigned)(params->n_mol * (a.n_chunks + 1))), dim3(MD_BLOCK), 0, st, a, *sites);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_md_sites_spread(void *stream, const anihip_md_params *params, const anihip_md_sites *sites,
                                      const float *coords, const float *coords_lo, const float *forces_ext, float *forces)
{
    SitesArgs a{};
    if (int rc = sites_args(params, sites, a)) return rc;
    ANIHIP_REQUIRE(coords && coords_lo && forces_ext && forces, "null pointer argument");
    a.coords = coords, a.coords_lo = coords_lo, a.forces_ext = const_cast<float *>(forces_ext), a.forces_out = forces;
    const int64_t n_chunks = (a.A + SPREAD_ATOMS - 1) / SPREAD_ATOMS;
    ANIHIP_REQUIRE(params->n_mol * n_chunks < ((int64_t)1 << 31), "entries x chunks of %d atoms must stay below 2^31", SPREAD_ATOMS);
    hipLaunchKernelGGL(k_md_sites_spread, dim3((unsigned)(params->n_mol * n_chunks)), dim3(MD_BLOCK), 0, (hipStream_t)stream, a,
                       *sites, (int)n_chunks);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}
