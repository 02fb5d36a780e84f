// Pair potentials evaluated on the neighbor rows of nbr.hip (cutoff envelope and half-per-atom bookkeeping of
// potentials/core.py:155-207): the analytic family k_pair<KIND> -- xTB repulsion (potentials/xtb.py:17-77), ZBL screened
// nuclear repulsion (zbl.py:10-81), Lennard-Jones 12 / 6 terms (lj.py:42-108), fixed-charge Coulomb with optional MNOK
// damping (fixed_coulomb.py:8-75) -- and DFT-D3(BJ) dispersion below.
//
// One wave per central atom, lane = neighbor.  The rows are a FULL symmetric list, so atom i finishes everything that
// concerns itself from its own row: atomic energy sum_j e_ij / 2 (core.py:195-198) and gradient
// sum_j e'(d_ij) d r_ij / d r_i -- no atomics, deterministic.  (Rows from a LAMMPS full list are not symmetric: there the
// pair term is pushed to the neighbor with float atomics, flag ANIHIP_PAIR_PUSH.)
#include "hess_rows.h"

#include <type_traits>

namespace anihip {

constexpr float A2B = 1.8897261258369282f;   // torchani/units.py:41

struct PairExtra {
    float v[8];   // ZBL: screening coefficients c_0..3 and exponents b_0..3
};

// bare pair energy (no envelope) and its derivative with respect to r [Angstrom]; p = table entry of the species pair
template <int KIND>
__device__ __forceinline__ void pair_eval(const float4 p, const PairExtra &x, float r, float &base, float &dbase)
{
    if constexpr (KIND == ANIHIP_PAIR_XTB) {            // {y_ab, sqrt(alpha_ab), k_ab}: y / d exp(-sqrt(alpha) d^k), d [Bohr]
        const float rb = r * A2B;
        const float pw = __builtin_amdgcn_exp2f(p.z * __builtin_amdgcn_logf(rb));   // rb^k
        const float ex = __expf(-p.y * pw);
        base = p.x / rb * ex;
        dbase = base * (-1.0f / rb - p.y * p.z * pw / rb) * A2B;
    } else if constexpr (KIND == ANIHIP_PAIR_ZBL) {     // {Za Zb, (Za^kz + Zb^kz) / k}: Za Zb / d sum_i c_i exp(-b_i d s), d [Bohr]
        const float rb = r * A2B, xr = rb * p.y;
        float phi = 0.f, dphi = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float t = x.v[i] * __expf(-x.v[4 + i] * xr);
            phi += t;
            dphi -= x.v[4 + i] * t;
        }
        const float cl = p.x / rb;
        base = cl * phi;
        dbase = (cl * dphi * p.y - cl / rb * phi) * A2B;
    } else if constexpr (KIND == ANIHIP_PAIR_LJ) {      // {4 eps_ab, sigma_ab, c12, c6}: 4 eps (c12 x^12 + c6 x^6), x = sigma / r
        const float ir = 1.0f / r, xs = p.y * ir, x2 = xs * xs, x6 = x2 * x2 * x2, x12 = x6 * x6;
        base = p.x * (p.z * x12 + p.w * x6);
        dbase = -p.x * (12.0f * p.z * x12 + 6.0f * p.w * x6) * ir;
    } else {                                            // Coulomb {q_a q_b / dielectric, 1 / eta_ab}: qq / sqrt(d^2 + 1 / eta^2), d [Bohr]
        const float rb = r * A2B;
        const float is = __builtin_amdgcn_rsqf(rb * rb + p.y * p.y);
        base = p.x * is;
        dbase = -p.x * rb * is * is * is * A2B;
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_pair(int64_t lo, int64_t hi, const int32_t *__restrict__ species,
                                              const uint32_t *__restrict__ meta, const float4 *__restrict__ ent,
                                              const float *__restrict__ tab /* [8][8][4] per species pair */,
                                              PairExtra extra, float cutoff, int smooth, int push, int clamp_r,
                                              float *__restrict__ atomic_e, float *__restrict__ grad_coords,
                                              double *__restrict__ virial)
{
    const int lane = lane_id();
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
    float vxx = 0.f, vyy = 0.f, vzz = 0.f, vxy = 0.f, vxz = 0.f, vyz = 0.f;
    const float inv_rc = 1.0f / cutoff, rev_rc = 0.5f / cutoff, pi_rc = 3.14159265358979f / cutoff;
    for (int64_t i = lo + blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); i < hi; i += nw) {
        const int si = species[i];
        if (si < 0) continue;
        const uint32_t start = meta[(size_t)i * META_W], c = meta[(size_t)i * META_W + 1];
        const int nR = (int)(c & 0xFFFFu) + (int)(c >> 16);
        float e = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
        for (int e0 = 0; e0 < nR; e0 += WAVE) {
            const int k = e0 + lane;
            if (k >= nR) continue;
            const float4 d = ent[start + k];
            const uint32_t w = __float_as_uint(d.w);
            const int sj = (int)(w >> 28);
            const float r2 = d.x * d.x + d.y * d.y + d.z * d.z;
            const float inv = __builtin_amdgcn_rsqf(r2);
            const float r = clamp_r ? fmaxf(r2 * inv, 1e-7f) : r2 * inv;   // (core.py:138-139 clamp)
            if (r > cutoff) continue;
            float fc, dfc;   // envelope and its derivative (cutoffs.py:74-101)
            if (smooth) {
                const float q = r * inv_rc, m1 = (1.0f - q) * (1.0f + q);
                const float im = 1.0f / fmaxf(1e-10f, m1);
                fc = __expf(1.0f - im);
                dfc = m1 - 1e-10f >= 0.0f ? -2.0f * r * inv_rc * inv_rc * fc * im * im : 0.0f;
            } else {
                fc = 0.5f * __builtin_amdgcn_cosf(r * rev_rc) + 0.5f;
                dfc = -0.5f * pi_rc * __builtin_amdgcn_sinf(r * rev_rc);
            }
            const float4 p = reinterpret_cast<const float4 *>(tab)[si * 8 + sj];
            float base, dbase;
            pair_eval<KIND>(p, extra, r, base, dbase);
            const float eij = base * fc;
            const float de = dbase * fc + base * dfc;
            e += 0.5f * eij;
            // d r_ij / d r_i = -u_ij, u = d / r;  the pair contributes e_ij / 2 to BOTH atoms: gradient on i = -de u
            const float ux = d.x * inv, uy = d.y * inv, uz = d.z * inv;
            // (an atom's own periodic image moves with it: the pair has no gradient, only a virial.  Its two signs are both
            // in the row and would cancel up to the rounding of the lane sums; left out, the zero is exact)
            const bool image_of_i = (int64_t)(w & IDX_MASK) == i;
            const float dg = image_of_i ? 0.0f : de;
            gx -= dg * ux; gy -= dg * uy; gz -= dg * uz;
            if (push && grad_coords && !image_of_i) {   // asymmetric rows: this row's half of the pair acts on the neighbor too
                float *gj = grad_coords + 3 * (size_t)(w & IDX_MASK);
                atomicAdd(gj + 0, 0.5f * de * ux); atomicAdd(gj + 1, 0.5f * de * uy); atomicAdd(gj + 2, 0.5f * de * uz);
            }
            if (virial) {   // sum over ordered pairs of (dE_i / d d_ij) (x) d_ij with E_i = sum_j e_ij / 2
                const float h = 0.5f * de;
                vxx += h * ux * d.x; vyy += h * uy * d.y; vzz += h * uz * d.z;
                vxy += h * ux * d.y; vxz += h * ux * d.z; vyz += h * uy * d.z;
            }
        }
        e = wave_sum(e);
        if (lane == 0 && atomic_e) atomic_e[i] += e;
        if (grad_coords) {
            const float sc = push ? 0.5f : 1.0f;   // (symmetric rows: the partner's row supplies the other half)
            gx = wave_sum(gx) * sc; gy = wave_sum(gy) * sc; gz = wave_sum(gz) * sc;
            if (lane == 0) {
                float *gi = grad_coords + 3 * (size_t)i;
                if (push) { atomicAdd(gi + 0, gx); atomicAdd(gi + 1, gy); atomicAdd(gi + 2, gz); }
                else { gi[0] += gx; gi[1] += gy; gi[2] += gz; }
            }
        }
    }
    if (virial) {
        vxx = wave_sum(vxx); vyy = wave_sum(vyy); vzz = wave_sum(vzz);
        vxy = wave_sum(vxy); vxz = wave_sum(vxz); vyz = wave_sum(vyz);
        if (lane == 0) {
            atomicAdd(virial + 0, (double)vxx); atomicAdd(virial + 4, (double)vyy); atomicAdd(virial + 8, (double)vzz);
            atomicAdd(virial + 1, (double)vxy); atomicAdd(virial + 3, (double)vxy);
            atomicAdd(virial + 2, (double)vxz); atomicAdd(virial + 6, (double)vxz);
            atomicAdd(virial + 5, (double)vyz); atomicAdd(virial + 7, (double)vyz);
        }
    }
}

// ---- Hessian-vector products of the closed-form pair terms ------------------------------------------------------
// For a pair with d = r_j - r_i, r = |d|, u = d / r and e(r) = base(r) fc(r), d^2 e / d d^2 = B = a I + c u u^T with
// a = e'(r) / r, c = e''(r) - a.  On symmetric rows atom i owns every pair of its row in full (as in k_pair's gradient), so
//   (H v)_i = sum_{j in row i} B_ij (v_i - v_j)
// and a periodic image of i itself (j == i) contributes v_i - v_i = 0, which is the second derivative of a constant.

// bare pair energy and its first and second derivatives with respect to r [Angstrom] (the same forms as pair_eval)
template <int KIND>
__device__ __forceinline__ void pair_eval2(const float4 p, const PairExtra &x, float r, float &base, float &dbase,
                                           float &d2base)
{
    constexpr float B2 = A2B * A2B;
    if constexpr (KIND == ANIHIP_PAIR_XTB) {            // f = y / d exp(-s d^k): f' = f g, f'' = f (g^2 + g'), g = -1/d - s k d^(k-1)
        const float rb = r * A2B, irb = 1.0f / rb;
        const float pw = __builtin_amdgcn_exp2f(p.z * __builtin_amdgcn_logf(rb));   // rb^k
        const float ex = __expf(-p.y * pw);
        base = p.x / rb * ex;
        const float g = -irb - p.y * p.z * pw * irb;
        const float dg = (1.0f - p.y * p.z * (p.z - 1.0f) * pw) * irb * irb;
        dbase = base * g * A2B;
        d2base = base * (g * g + dg) * B2;
    } else if constexpr (KIND == ANIHIP_PAIR_ZBL) {     // f = cl phi(s d), cl = Za Zb / d
        const float rb = r * A2B, irb = 1.0f / rb, xr = rb * p.y;
        float phi = 0.f, dphi = 0.f, d2phi = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float t = x.v[i] * __expf(-x.v[4 + i] * xr);
            phi += t;
            dphi -= x.v[4 + i] * t;
            d2phi += x.v[4 + i] * x.v[4 + i] * t;
        }
        const float cl = p.x * irb;
        base = cl * phi;
        dbase = cl * (p.y * dphi - phi * irb) * A2B;
        d2base = cl * (p.y * p.y * d2phi - 2.0f * p.y * dphi * irb + 2.0f * phi * irb * irb) * B2;
    } else if constexpr (KIND == ANIHIP_PAIR_LJ) {      // d^2 / dr^2 x^n = n (n + 1) x^n / r^2
        const float ir = 1.0f / r, xs = p.y * ir, x2 = xs * xs, x6 = x2 * x2 * x2, x12 = x6 * x6;
        base = p.x * (p.z * x12 + p.w * x6);
        dbase = -p.x * (12.0f * p.z * x12 + 6.0f * p.w * x6) * ir;
        d2base = p.x * (156.0f * p.z * x12 + 42.0f * p.w * x6) * ir * ir;
    } else {                                            // f = qq (d^2 + h^2)^-1/2: f'' = qq is^3 (3 d^2 is^2 - 1)
        const float rb = r * A2B;
        const float is = __builtin_amdgcn_rsqf(rb * rb + p.y * p.y), is3 = is * is * is;
        base = p.x * is;
        dbase = -p.x * rb * is3 * A2B;
        d2base = p.x * is3 * (3.0f * rb * rb * is * is - 1.0f) * B2;
    }
}

// envelope and its first and second derivatives (cutoffs.py:74-101; the smooth one's max(eps, .) guard as in k_pair: both
// derivatives are 0 beyond it, and fc im^2 is formed first so that fc = 0 never meets an overflowed power of im)
__device__ __forceinline__ void envelope2(float r, float inv_rc, float rev_rc, float pi_rc, int smooth, float &fc,
                                          float &dfc, float &d2fc)
{
    if (smooth) {
        const float q = r * inv_rc, m1 = (1.0f - q) * (1.0f + q);
        const float im = 1.0f / fmaxf(1e-10f, m1);
        fc = __expf(1.0f - im);
        if (m1 - 1e-10f >= 0.0f) {
            const float irc2 = inv_rc * inv_rc, fi2 = fc * im * im, s = r * r * irc2;
            dfc = -2.0f * r * irc2 * fi2;
            d2fc = fi2 * irc2 * (4.0f * s * im * im - 8.0f * s * im - 2.0f);
        } else {
            dfc = 0.f;
            d2fc = 0.f;
        }
    } else {
        const float cs = __builtin_amdgcn_cosf(r * rev_rc);
        fc = 0.5f * cs + 0.5f;
        dfc = -0.5f * pi_rc * __builtin_amdgcn_sinf(r * rev_rc);
        d2fc = -0.5f * pi_rc * pi_rc * cs;
    }
}

// out[k] += H t[k] for k < n_dir.  One wave per central atom, lane = neighbor, as k_pair: each lane evaluates its pair's
// (a, c, u) once, in registers (up to HVP_ROUNDS x 64 neighbors = ANIHIP_MAX_RAD, every row of the library's builders),
// then for every direction gathers t[k][j], applies B and the wave sums give (H t[k])_i.  No atomics: deterministic.
constexpr int HVP_ROUNDS = (MAXR + WAVE - 1) / WAVE;

// M (hess_rows.h): Dense -- central atoms lo <= i < hi, the n_dir directions of tangent [n_dir][n_atoms][3].  Item
// (anihip_pair_analytic_hvp_items, sparse Hessians): the wave's index q runs over item rows lo <= q < hi, ONE direction
// each, output slab row_dir[q] - dir0 of out [n_dir][n_atoms][3] (an item row names each (direction, atom) once: still no
// atomics).  Strain (anihip_pair_analytic_hvp_strain, strain second derivatives): central atoms lo <= i < hi, the n_dir = 9
// strain directions S_ab (k = 3 a + b) each:  out[k][i] += -sum_j B_ij d'_ij (no atomics).  Each lane also keeps, over its
// pairs, M_xp = sum d_x d_p a / 2 (the pair virial) and the fully symmetric T_xypq = sum c r^2 u_x u_y u_p u_q / 2
// (6 + 15 numbers); the strain-strain term
//   ss[mol][3 x + y][3 p + q] += sum_pairs d_x (B d'_pq)_y / 2 = delta_yq M_xp + T_xypq
// and virial[mol][3 x + y] += M_xy are added per molecule (mol = i / sa.atoms_per_mol) to sa.ss and sa.virial with one wave
// reduction and fp64 atomics whenever the wave's molecule changes.
template <int KIND, Dir M>
__global__ __launch_bounds__(256) void k_pair_hvp(int64_t n_atoms, int64_t lo, int64_t hi,
                                                  const int32_t *__restrict__ species, const uint32_t *__restrict__ meta,
                                                  const float4 *__restrict__ ent, const float *__restrict__ tab,
                                                  PairExtra extra, float cutoff, int smooth, int clamp_r, int64_t n_dir,
                                                  const float *__restrict__ tangent, float *__restrict__ out,
                                                  const int32_t *__restrict__ row_atom,
                                                  const int32_t *__restrict__ row_dir, int64_t dir0, StrainAcc sa)
{
    constexpr bool ITEMS = M == Dir::Item, STRAIN = M == Dir::Strain;
    const int lane = lane_id();
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
    const size_t stride = (size_t)n_atoms * 3;
    const float inv_rc = 1.0f / cutoff, rev_rc = 0.5f / cutoff, pi_rc = 3.14159265358979f / cutoff;
    constexpr int NS = STRAIN ? 21 : 1;
    float sm[NS];   // STRAIN: M (6, pairs x <= p) then T (15, by the powers of x and y)
    if (STRAIN) {
#pragma unroll
        for (int c = 0; c < NS; ++c) sm[c] = 0.f;
    }
    int64_t mol = -1;
    auto flush = [&]() {   // (wave-uniform) the lane partials of molecule `mol` into ss / virial, then zero them
#pragma unroll
        for (int c = 0; c < NS; ++c) sm[c] = wave_sum(sm[c]);
        for (int l = lane; l < 81; l += WAVE) {   // (81 components over the 64 lanes)
            const int xy = l / 9, pq = l - 9 * xy;
            const int x = xy / 3, y = xy - 3 * x, pp = pq / 3, qq = pq - 3 * pp;
            const int lo_ = min(x, pp), hi_ = max(x, pp);
            const int im = lo_ * 3 - (lo_ * (lo_ - 1)) / 2 + (hi_ - lo_);
            const int nx = (x == 0) + (y == 0) + (pp == 0) + (qq == 0), ny = (x == 1) + (y == 1) + (pp == 1) + (qq == 1);
            const int it = nx * 5 - (nx * (nx - 1)) / 2 + ny;
            float mv = 0.f, tv = 0.f;
#pragma unroll
            for (int c = 0; c < 6; ++c) mv = c == im ? sm[c] : mv;
#pragma unroll
            for (int c = 0; c < 15; ++c) tv = c == it ? sm[(STRAIN ? 6 + c : 0)] : tv;
            atomicAdd(sa.ss + (size_t)mol * 81 + l, (double)((y == qq ? mv : 0.f) + tv));
            if (sa.virial && pq == 0) {   // (l = 0, 9, .., 72: component xy of the virial = M_xy)
                const int lm = min(x, y), hm = max(x, y);
                const int iv = lm * 3 - (lm * (lm - 1)) / 2 + (hm - lm);
                float vv = 0.f;
#pragma unroll
                for (int c = 0; c < 6; ++c) vv = c == iv ? sm[c] : vv;
                atomicAdd(sa.virial + (size_t)mol * 9 + xy, (double)vv);
            }
        }
#pragma unroll
        for (int c = 0; c < NS; ++c) sm[c] = 0.f;
    };
    for (int64_t qi = lo + blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); qi < hi; qi += nw) {
        const DirRow row = ITEMS ? dir_item(row_atom, row_dir, qi, dir0) : DirRow{qi, 0, -1, 0};
        const int64_t i = row.i;
        if (STRAIN && i / sa.atoms_per_mol != mol) {
            if (mol >= 0) flush();
            mol = i / sa.atoms_per_mol;
        }
        const int si = species[i];
        if (si < 0) continue;
        if (ITEMS && (row.slab < 0 || row.slab >= n_dir)) continue;   // (a row outside the caller's slabs)
        const uint32_t start = meta[(size_t)i * META_W], c = meta[(size_t)i * META_W + 1];
        const int nR = (int)(c & 0xFFFFu) + (int)(c >> 16);
        for (int b0 = 0; b0 < nR; b0 += HVP_ROUNDS * WAVE) {   // (one pass for every row of at most ANIHIP_MAX_RAD entries)
            float ba[HVP_ROUNDS], bc[HVP_ROUNDS], ux[HVP_ROUNDS], uy[HVP_ROUNDS], uz[HVP_ROUNDS];
            float rr[STRAIN ? HVP_ROUNDS : 1];   // STRAIN: r (d = r u)
            int jj[HVP_ROUNDS];   // (atom indices have 28 bits: IDX_MASK)
#pragma unroll
            for (int q = 0; q < HVP_ROUNDS; ++q) {
                ba[q] = 0.f; bc[q] = 0.f; ux[q] = 0.f; uy[q] = 0.f; uz[q] = 0.f;
                if (STRAIN) rr[(STRAIN ? q : 0)] = 0.f;
                jj[q] = (int)i;   // (an empty slot gathers v_i and adds B (v_i - v_i) with B = 0)
                const int k = b0 + q * WAVE + lane;
                if (k >= nR) continue;
                const float4 d = ent[start + k];
                const uint32_t w = __float_as_uint(d.w);
                const int sj = (int)(w >> 28);
                const int j = (int)(w & IDX_MASK);
                if (j >= n_atoms) continue;
                const float r2 = d.x * d.x + d.y * d.y + d.z * d.z;
                const float inv = __builtin_amdgcn_rsqf(r2);
                const float r = clamp_r ? fmaxf(r2 * inv, 1e-7f) : r2 * inv;   // (core.py:138-139 clamp)
                if (r > cutoff) continue;
                float fc, dfc, d2fc;
                envelope2(r, inv_rc, rev_rc, pi_rc, smooth, fc, dfc, d2fc);
                const float4 p = reinterpret_cast<const float4 *>(tab)[si * 8 + sj];
                float base, dbase, d2base;
                pair_eval2<KIND>(p, extra, r, base, dbase, d2base);
                const float e1 = dbase * fc + base * dfc;
                const float e2 = d2base * fc + 2.0f * dbase * dfc + base * d2fc;
                ba[q] = e1 / r;
                bc[q] = e2 - ba[q];
                ux[q] = d.x * inv; uy[q] = d.y * inv; uz[q] = d.z * inv;
                jj[q] = j;
                if (STRAIN) {
                    rr[(STRAIN ? q : 0)] = r;
                    const float w1 = 0.5f * ba[q] * r * r, w2 = 0.5f * bc[q] * r * r;
                    const float u3[3] = {ux[q], uy[q], uz[q]};
                    int c = 0;
#pragma unroll
                    for (int x = 0; x < 3; ++x)
#pragma unroll
                        for (int pp = x; pp < 3; ++pp) sm[(STRAIN ? c++ : 0)] += w1 * u3[x] * u3[pp];
                    const float px[5] = {1.f, ux[q], ux[q] * ux[q], ux[q] * ux[q] * ux[q], ux[q] * ux[q] * ux[q] * ux[q]};
                    const float py[5] = {1.f, uy[q], uy[q] * uy[q], uy[q] * uy[q] * uy[q], uy[q] * uy[q] * uy[q] * uy[q]};
                    const float pz[5] = {1.f, uz[q], uz[q] * uz[q], uz[q] * uz[q] * uz[q], uz[q] * uz[q] * uz[q] * uz[q]};
#pragma unroll
                    for (int nx = 0; nx <= 4; ++nx)
#pragma unroll
                        for (int ny = 0; ny <= 4 - nx; ++ny) sm[(STRAIN ? c++ : 0)] += w2 * px[nx] * py[ny] * pz[4 - nx - ny];
                }
            }
            for (int64_t kd = 0; kd < (ITEMS ? 1 : n_dir); ++kd) {
                const float *tk = ITEMS ? nullptr : tangent + (size_t)kd * stride;
                const DirRow dk = STRAIN ? dir_row(i, kd, (int)kd) : row;
                const float3 ti = dir_tangent3<M>(tk, dk, i);
                float hx = 0.f, hy = 0.f, hz = 0.f;
#pragma unroll
                for (int q = 0; q < HVP_ROUNDS; ++q) {
                    if (b0 + q * WAVE >= nR) break;   // (wave-uniform)
                    // B_ij acts on t_i - t_j: the d' of the entry seen from j (neighbor i, displacement -d = -r u)
                    const float rq = STRAIN ? rr[(STRAIN ? q : 0)] : 0.f;
                    const float3 tj = dir_tangent3<M>(tk, dk, jj[q]);
                    const float3 dp = STRAIN ? dir_dprime<M>(tk, dk, tj, i, make_float3(-ux[q] * rq, -uy[q] * rq, -uz[q] * rq))
                                             : make_float3(ti.x - tj.x, ti.y - tj.y, ti.z - tj.z);
                    const float dx = dp.x, dy = dp.y, dz = dp.z;
                    const float cu = bc[q] * (ux[q] * dx + uy[q] * dy + uz[q] * dz);
                    hx += ba[q] * dx + cu * ux[q];
                    hy += ba[q] * dy + cu * uy[q];
                    hz += ba[q] * dz + cu * uz[q];
                }
                hx = wave_sum(hx); hy = wave_sum(hy); hz = wave_sum(hz);
                if (lane == 0) {
                    float *o = out + (size_t)(ITEMS ? row.slab : kd) * stride + 3 * i;
                    o[0] += hx; o[1] += hy; o[2] += hz;
                }
            }
        }
    }
    if (STRAIN && mol >= 0) flush();
}

// ---- DFT-D3(BJ) two-body dispersion (potentials/dftd3.py:113-330) -------------------------------------------------
// Three passes over the rows, one wave per central atom, lane = neighbor, all gathers (the rows are full and symmetric):
//   k_d3_cn     CN_i = sum_j count(d_ij)                                                    (:256-279 _coordnums)
//   k_d3_pair   per pair the C6 interpolation over the 5 x 5 references (:281-330), e_ij, its derivative at fixed C6
//               (energy and direct gradient of atom i), and gcn_i = dE / dCN_i = sum_j (de_ij / dC6) (dC6_ij / dCN_i)
//               -- the pair (i, j) sits in both rows and C6_ji(CN_j, CN_i) = C6_ij(CN_i, CN_j), so the two halves of
//               dE / dCN_i are equal and row i alone gives the whole of it
//   k_d3_cngrad grad_i += sum_j (gcn_i + gcn_j) count'(d_ij) d d_ij / d r_i
struct D3P {
    float s6, s8, a1, a2;
    float cov[8], sq[8];
};
constexpr float D3_K1 = 16.0f, D3_K2 = 4.0f / 3.0f, D3_K3 = 4.0f, D3_EPS = 1e-35f;

__device__ __forceinline__ void d3_envelope(float r, float cutoff, int smooth, float &fc, float &dfc)
{
    if (smooth) {
        const float inv_rc = 1.0f / cutoff, q = r * inv_rc, m1 = (1.0f - q) * (1.0f + q);
        const float im = 1.0f / fmaxf(1e-10f, m1);
        fc = __expf(1.0f - im);
        dfc = m1 - 1e-10f >= 0.0f ? -2.0f * r * inv_rc * inv_rc * fc * im * im : 0.0f;
    } else {
        const float rev_rc = 0.5f / cutoff;
        fc = 0.5f * __builtin_amdgcn_cosf(r * rev_rc) + 0.5f;
        dfc = -0.5f * (3.14159265358979f / cutoff) * __builtin_amdgcn_sinf(r * rev_rc);
    }
}

// count(d) and d count / d d (d in Bohr)
__device__ __forceinline__ float d3_count(float rsum, float d, float &dcnt)
{
    const float t = expf(-D3_K1 * (D3_K2 * rsum / d - 1.0f));
    const float c = 1.0f / (1.0f + t);
    dcnt = -c * (1.0f - c) * D3_K1 * D3_K2 * rsum / (d * d);
    return c;
}

__global__ __launch_bounds__(256) void k_d3_cn(int64_t n, const int32_t *__restrict__ species,
                                               const uint32_t *__restrict__ meta, const float4 *__restrict__ ent, D3P p,
                                               float cutoff, float *__restrict__ cn)
{
    const int lane = lane_id();
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t i = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += nw) {
        const int si = species[i];
        float acc = 0.f;
        if (si >= 0) {
            const uint32_t start = meta[(size_t)i * META_W], c = meta[(size_t)i * META_W + 1];
            const int nR = (int)(c & 0xFFFFu) + (int)(c >> 16);
            for (int k = lane; k < nR; k += WAVE) {
                const float4 d = ent[start + k];
                const int sj = (int)(__float_as_uint(d.w) >> 28);
                const float r = fmaxf(sqrtf(d.x * d.x + d.y * d.y + d.z * d.z), 1e-7f);
                if (r > cutoff) continue;
                float dc;
                acc += d3_count(p.cov[si] + p.cov[sj], r * A2B, dc);
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) cn[i] = acc;
    }
}

__global__ __launch_bounds__(256) void k_d3_pair(int64_t n, int64_t lo, int64_t hi, const int32_t *__restrict__ species,
                                                 const uint32_t *__restrict__ meta, const float4 *__restrict__ ent,
                                                 const float4 *__restrict__ tab, D3P p, float cutoff, int smooth,
                                                 const float *__restrict__ cn, float *__restrict__ gcn,
                                                 float *__restrict__ atomic_e, float *__restrict__ grad_coords,
                                                 double *__restrict__ virial)
{
    const int lane = lane_id();
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
    float vxx = 0.f, vyy = 0.f, vzz = 0.f, vxy = 0.f, vxz = 0.f, vyz = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += nw) {
        const int si = species[i];
        if (si < 0) {
            if (lane == 0) gcn[i] = 0.f;
            continue;
        }
        const bool own = i >= lo && i < hi;
        const uint32_t start = meta[(size_t)i * META_W], c = meta[(size_t)i * META_W + 1];
        const int nR = (int)(c & 0xFFFFu) + (int)(c >> 16);
        const float cni = cn[i];
        float e = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, gc = 0.f;
        for (int k = lane; k < nR; k += WAVE) {
            const float4 d = ent[start + k];
            const uint32_t w = __float_as_uint(d.w);
            const int sj = (int)(w >> 28);
            const float r2 = d.x * d.x + d.y * d.y + d.z * d.z;
            const float inv = __builtin_amdgcn_rsqf(r2);
            const float r = fmaxf(r2 * inv, 1e-7f);
            if (r > cutoff) continue;
            const float cnj = cn[w & IDX_MASK];
            // C6 and d C6 / d CN_i from the 25 reference pairs
            const float4 *t = tab + (si * 8 + sj) * 25;
            const int nv = (int)t[0].w;   // the pair's references with c6ref > 0 come first (H-H: 4 of the 25)
            // (the weights are formed relative to the largest one: coordination numbers far from every reference --
            // dense random geometries -- give weights below the fp32 range, which the reference's fp64 still resolves;
            // its 1e-35 guards, dftd3.py:322-330, are applied to the rescaled sums)
            float amin = 3.0e38f;
            for (int q = 0; q < nv; ++q) {
                const float4 ref = t[q];
                const float da = cni - ref.y, db = cnj - ref.z;
                amin = fminf(amin, D3_K3 * (da * da + db * db));
            }
            float W = 0.f, Z = 0.f, dW = 0.f, dZ = 0.f;
            for (int q = 0; q < nv; ++q) {
                const float4 ref = t[q];
                const float da = cni - ref.y, db = cnj - ref.z;
                const float L = expf(amin - D3_K3 * (da * da + db * db));
                W += L; Z += ref.x * L;
                dW += L * da; dZ += ref.x * L * da;
            }
            const float sc = expf(-amin);   // (0 when there is no reference at all: C6 = eps / eps = 1 like the reference)
            W = W * sc + D3_EPS; Z = Z * sc + D3_EPS;
            const float iW = 1.0f / W;
            const float c6 = Z * iW;
            const float dc6 = -2.0f * D3_K3 * sc * (dZ - c6 * dW) * iW;   // d C6 / d CN_i
            const float qab = p.sq[si] * p.sq[sj];
            const float R = p.a1 * sqrtf(3.0f * qab) + p.a2;
            const float R2 = R * R, R6 = R2 * R2 * R2, R8 = R6 * R2;
            const float rb = r * A2B, rb2 = rb * rb, rb6 = rb2 * rb2 * rb2, rb8 = rb6 * rb2;
            const float i6 = 1.0f / (rb6 + R6), i8 = 1.0f / (rb8 + R8);
            const float k6 = p.s6, k8 = 3.0f * p.s8 * qab;
            float fc, dfc;
            d3_envelope(r, cutoff, smooth, fc, dfc);
            const float per_c6 = -(k6 * i6 + k8 * i8);                 // e / C6 without the envelope
            const float bare = c6 * per_c6;
            // d bare / d r [Angstrom] at fixed C6
            const float dbare = c6 * (k6 * 6.0f * rb2 * rb2 * rb * i6 * i6 + k8 * 8.0f * rb6 * rb * i8 * i8) * A2B;
            const float de = dbare * fc + bare * dfc;
            gc += per_c6 * fc * dc6;
            if (own) {
                e += 0.5f * bare * fc;
                const float ux = d.x * inv, uy = d.y * inv, uz = d.z * inv;
                const float dg = (int64_t)(w & IDX_MASK) == i ? 0.0f : de;   // (own image: no gradient, as in k_pair)
                gx -= dg * ux; gy -= dg * uy; gz -= dg * uz;
                if (virial) {
                    const float h = 0.5f * de;
                    vxx += h * ux * d.x; vyy += h * uy * d.y; vzz += h * uz * d.z;
                    vxy += h * ux * d.y; vxz += h * ux * d.z; vyz += h * uy * d.z;
                }
            }
        }
        gc = wave_sum(gc);
        if (lane == 0) gcn[i] = gc;
        if (own) {
            e = wave_sum(e);
            if (lane == 0 && atomic_e) atomic_e[i] += e;
            if (grad_coords) {
                gx = wave_sum(gx); gy = wave_sum(gy); gz = wave_sum(gz);
                if (lane == 0) {
                    float *gi = grad_coords + 3 * (size_t)i;
                    gi[0] += gx; gi[1] += gy; gi[2] += gz;
                }
            }
        }
    }
    if (virial) {
        vxx = wave_sum(vxx); vyy = wave_sum(vyy); vzz = wave_sum(vzz);
        vxy = wave_sum(vxy); vxz = wave_sum(vxz); vyz = wave_sum(vyz);
        if (lane == 0) {
            atomicAdd(virial + 0, (double)vxx); atomicAdd(virial + 4, (double)vyy); atomicAdd(virial + 8, (double)vzz);
            atomicAdd(virial + 1, (double)vxy); atomicAdd(virial + 3, (double)vxy);
            atomicAdd(virial + 2, (double)vxz); atomicAdd(virial + 6, (double)vxz);
            atomicAdd(virial + 5, (double)vyz); atomicAdd(virial + 7, (double)vyz);
        }
    }
}

__global__ __launch_bounds__(256) void k_d3_cngrad(int64_t lo, int64_t hi, const int32_t *__restrict__ species,
                                                   const uint32_t *__restrict__ meta, const float4 *__restrict__ ent,
                                                   D3P p, float cutoff, const float *__restrict__ gcn,
                                                   float *__restrict__ grad_coords, double *__restrict__ virial)
{
    const int lane = lane_id();
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
    float vxx = 0.f, vyy = 0.f, vzz = 0.f, vxy = 0.f, vxz = 0.f, vyz = 0.f;
    for (int64_t i = lo + blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); i < hi; i += nw) {
        const int si = species[i];
        if (si < 0) continue;
        const uint32_t start = meta[(size_t)i * META_W], c = meta[(size_t)i * META_W + 1];
        const int nR = (int)(c & 0xFFFFu) + (int)(c >> 16);
        const float gi_ = gcn[i];
        float gx = 0.f, gy = 0.f, gz = 0.f;
        for (int k = lane; k < nR; k += WAVE) {
            const float4 d = ent[start + k];
            const uint32_t w = __float_as_uint(d.w);
            const int sj = (int)(w >> 28);
            const float r2 = d.x * d.x + d.y * d.y + d.z * d.z;
            const float inv = __builtin_amdgcn_rsqf(r2);
            const float r = fmaxf(r2 * inv, 1e-7f);
            if (r > cutoff) continue;
            float dc;
            d3_count(p.cov[si] + p.cov[sj], r * A2B, dc);
            const float de = (gi_ + gcn[w & IDX_MASK]) * dc * A2B;   // d E / d r_ij [Angstrom] through the CNs
            const float ux = d.x * inv, uy = d.y * inv, uz = d.z * inv;
            const float dg = (int64_t)(w & IDX_MASK) == i ? 0.0f : de;   // (own image: no gradient, as in k_pair)
            gx -= dg * ux; gy -= dg * uy; gz -= dg * uz;
            if (virial) {
                const float h = 0.5f * de;
                vxx += h * ux * d.x; vyy += h * uy * d.y; vzz += h * uz * d.z;
                vxy += h * ux * d.y; vxz += h * ux * d.z; vyz += h * uy * d.z;
            }
        }
        if (!grad_coords) continue;   // (the virial alone: its coordination-number term still comes from this kernel)
        gx = wave_sum(gx); gy = wave_sum(gy); gz = wave_sum(gz);
        if (lane == 0) {
            float *gi = grad_coords + 3 * (size_t)i;
            gi[0] += gx; gi[1] += gy; gi[2] += gz;
        }
    }
    if (virial) {
        vxx = wave_sum(vxx); vyy = wave_sum(vyy); vzz = wave_sum(vzz);
        vxy = wave_sum(vxy); vxz = wave_sum(vxz); vyz = wave_sum(vyz);
        if (lane == 0) {
            atomicAdd(virial + 0, (double)vxx); atomicAdd(virial + 4, (double)vyy); atomicAdd(virial + 8, (double)vzz);
            atomicAdd(virial + 1, (double)vxy); atomicAdd(virial + 3, (double)vxy);
            atomicAdd(virial + 2, (double)vxz); atomicAdd(virial + 6, (double)vxz);
            atomicAdd(virial + 5, (double)vyz); atomicAdd(virial + 7, (double)vyz);
        }
    }
}

// the checks and launch constants shared by the anihip_pair_analytic* entry points (hvp: the Hessian-vector products)
struct PairSetup {
    PairExtra x;
    int smooth, clamp_r;
};

static int pair_setup(int32_t kind, int64_t n_atoms, const float *extra, float cutoff, int32_t cutoff_kind, int32_t flags,
                      bool hvp, PairSetup *s)
{
    ANIHIP_REQUIRE(!hvp || n_atoms <= (int64_t)IDX_MASK, "more atoms than a neighbor row can index");
    ANIHIP_REQUIRE(cutoff > 0.f, "cutoff must be positive (the rows hold pairs up to their own radial cutoff)");
    ANIHIP_REQUIRE(cutoff_kind == ANIHIP_CUTOFF_COSINE || cutoff_kind == ANIHIP_CUTOFF_SMOOTH, "unknown cutoff_kind");
    ANIHIP_REQUIRE(kind >= ANIHIP_PAIR_XTB && kind <= ANIHIP_PAIR_COULOMB, "unknown pair potential kind");
    ANIHIP_REQUIRE(kind != ANIHIP_PAIR_ZBL || extra, "ZBL needs its 4 + 4 screening constants");
    ANIHIP_REQUIRE(!hvp || !(flags & ANIHIP_PAIR_PUSH),
                   "pair Hessian-vector products need symmetric rows (ANIHIP_PAIR_PUSH rows are not supported)");
    *s = PairSetup{};
    if (extra)
        for (int k = 0; k < 8; ++k) s->x.v[k] = extra[k];
    s->smooth = cutoff_kind == ANIHIP_CUTOFF_SMOOTH ? 1 : 0;
    s->clamp_r = (flags & ANIHIP_PAIR_NO_CLAMP) ? 0 : 1;
    return 0;
}

// four waves per 256-thread block, one per central atom (row), at most 2048 blocks
static unsigned pair_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, 256 * 8)); }

// f(std::integral_constant<int, KIND>{}) for the runtime kind (checked by pair_setup)
template <class F>
static void with_kind(int32_t kind, F &&f)
{
    switch (kind) {
        case ANIHIP_PAIR_XTB: f(std::integral_constant<int, ANIHIP_PAIR_XTB>{}); break;
        case ANIHIP_PAIR_ZBL: f(std::integral_constant<int, ANIHIP_PAIR_ZBL>{}); break;
        case ANIHIP_PAIR_LJ: f(std::integral_constant<int, ANIHIP_PAIR_LJ>{}); break;
        default: f(std::integral_constant<int, ANIHIP_PAIR_COULOMB>{}); break;
    }
}

template <Dir M>
static int pair_hvp_launch(void *stream, int32_t kind, const PairSetup &s, int64_t n_atoms, int64_t lo, int64_t hi,
                           const int32_t *species, const uint32_t *meta, const float *ent, const float *pair_table,
                           float cutoff, int64_t n_dir, const float *tangent, float *out, const int32_t *row_atom,
                           const int32_t *row_dir, int64_t dir0, StrainAcc sa)
{
    with_kind(kind, [&](auto K) {
        hipLaunchKernelGGL((k_pair_hvp<decltype(K)::value, M>), dim3(pair_blocks(hi - lo)), dim3(256), 0,
                           (hipStream_t)stream, n_atoms, lo, hi, species, meta, (const float4 *)ent, pair_table, s.x, cutoff,
                           s.smooth, s.clamp_r, n_dir, tangent, out, row_atom, row_dir, dir0, sa);
    });
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace anihip

using namespace anihip;

extern "C" int anihip_pair_analytic(void *stream, int32_t kind, int64_t n_atoms, int64_t lo, int64_t hi,
                                    const int32_t *species, const uint32_t *meta, const float *ent,
                                    const float *pair_table, const float *extra, float cutoff, int32_t cutoff_kind,
                                    int32_t flags, float *atomic_e, float *grad_coords, double *virial)
{
    ANIHIP_REQUIRE(species && meta && ent && pair_table, "null pointer argument");
    ANIHIP_REQUIRE(0 <= lo && lo <= hi && hi <= n_atoms, "central range outside 0..n_atoms");
    PairSetup s;
    if (int rc = pair_setup(kind, n_atoms, extra, cutoff, cutoff_kind, flags, false, &s)) return rc;
    if (hi == lo) return 0;
    const int push = (flags & ANIHIP_PAIR_PUSH) ? 1 : 0;
    with_kind(kind, [&](auto K) {
        hipLaunchKernelGGL((k_pair<decltype(K)::value>), dim3(pair_blocks(hi - lo)), dim3(256), 0, (hipStream_t)stream, lo,
                           hi, species, meta, (const float4 *)ent, pair_table, s.x, cutoff, s.smooth, push, s.clamp_r,
                           atomic_e, grad_coords, virial);
    });
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_pair_analytic_hvp(void *stream, int32_t kind, int64_t n_atoms, int64_t lo, int64_t hi,
                                        const int32_t *species, const uint32_t *meta, const float *ent,
                                        const float *pair_table, const float *extra, float cutoff, int32_t cutoff_kind,
                                        int32_t flags, int64_t n_dir, const float *tangent, float *out)
{
    ANIHIP_REQUIRE(species && meta && ent && pair_table, "null pointer argument");
    ANIHIP_REQUIRE(0 <= lo && lo <= hi && hi <= n_atoms, "central range outside 0..n_atoms");
    PairSetup s;
    if (int rc = pair_setup(kind, n_atoms, extra, cutoff, cutoff_kind, flags, true, &s)) return rc;
    ANIHIP_REQUIRE(n_dir >= 0, "n_dir must not be negative");
    if (hi == lo || n_dir == 0) return 0;
    ANIHIP_REQUIRE(tangent && out, "null pointer argument");
    return pair_hvp_launch<Dir::Dense>(stream, kind, s, n_atoms, lo, hi, species, meta, ent, pair_table, cutoff, n_dir,
                                       tangent, out, nullptr, nullptr, 0, StrainAcc{});
}

extern "C" int anihip_pair_analytic_hvp_items(void *stream, int32_t kind, int64_t n_atoms, const int32_t *species,
                                              const uint32_t *meta, const float *ent, const float *pair_table,
                                              const float *extra, float cutoff, int32_t cutoff_kind, int32_t flags,
                                              int64_t n_rows, const int32_t *row_atom, const int32_t *row_dir, int64_t dir0,
                                              int64_t n_dir, float *out)
{
    ANIHIP_REQUIRE(species && meta && ent && pair_table && row_atom && row_dir && out, "null pointer argument");
    ANIHIP_REQUIRE(n_atoms >= 0 && n_rows >= 0 && n_dir >= 0, "negative size");
    PairSetup s;
    if (int rc = pair_setup(kind, n_atoms, extra, cutoff, cutoff_kind, flags, true, &s)) return rc;
    if (n_rows == 0 || n_dir == 0) return 0;
    return pair_hvp_launch<Dir::Item>(stream, kind, s, n_atoms, 0, n_rows, species, meta, ent, pair_table, cutoff, n_dir,
                                      nullptr, out, row_atom, row_dir, dir0, StrainAcc{});
}

extern "C" int anihip_pair_analytic_hvp_strain(void *stream, int32_t kind, int64_t n_atoms, int64_t atoms_per_mol, int64_t lo,
                                               int64_t hi, const int32_t *species, const uint32_t *meta, const float *ent,
                                               const float *pair_table, const float *extra, float cutoff,
                                               int32_t cutoff_kind, int32_t flags, float *out, double *ss, double *virial)
{
    ANIHIP_REQUIRE(species && meta && ent && pair_table && out && ss, "null pointer argument");
    ANIHIP_REQUIRE(0 <= lo && lo <= hi && hi <= n_atoms, "central range outside 0..n_atoms");
    ANIHIP_REQUIRE(atoms_per_mol >= 1 && n_atoms % atoms_per_mol == 0,
                   "atoms_per_mol must be >= 1 and divide n_atoms (got %lld, %lld)", (long long)atoms_per_mol,
                   (long long)n_atoms);
    PairSetup s;
    if (int rc = pair_setup(kind, n_atoms, extra, cutoff, cutoff_kind, flags, true, &s)) return rc;
    if (hi == lo) return 0;
    return pair_hvp_launch<Dir::Strain>(stream, kind, s, n_atoms, lo, hi, species, meta, ent, pair_table, cutoff, 9, nullptr,
                                        out, nullptr, nullptr, 0, StrainAcc{ss, virial, atoms_per_mol});
}

extern "C" int anihip_pair_xtb_repulsion(void *stream, int64_t n_atoms, int64_t lo, int64_t hi, const int32_t *species,
                                         const uint32_t *meta, const float *ent, const float *pair_table, float cutoff,
                                         int32_t cutoff_kind, int32_t flags, float *atomic_e, float *grad_coords,
                                         double *virial)
{
    return anihip_pair_analytic(stream, ANIHIP_PAIR_XTB, n_atoms, lo, hi, species, meta, ent, pair_table, nullptr, cutoff,
                                cutoff_kind, flags, atomic_e, grad_coords, virial);
}

extern "C" int anihip_pair_d3(void *stream, int64_t n_atoms, int64_t lo, int64_t hi, const int32_t *species,
                              const uint32_t *meta, const float *ent, const float *c6_table,
                              const anihip_d3_params *params, float cutoff, int32_t cutoff_kind, float *cn, float *gcn,
                              float *atomic_e, float *grad_coords, double *virial)
{
    ANIHIP_REQUIRE(species && meta && ent && c6_table && params && cn && gcn, "null pointer argument");
    ANIHIP_REQUIRE(0 <= lo && lo <= hi && hi <= n_atoms, "central range outside 0..n_atoms");
    ANIHIP_REQUIRE(cutoff > 0.f, "cutoff must be positive (the rows hold pairs up to their own radial cutoff)");
    ANIHIP_REQUIRE(cutoff_kind == ANIHIP_CUTOFF_COSINE || cutoff_kind == ANIHIP_CUTOFF_SMOOTH, "unknown cutoff_kind");
    if (n_atoms == 0) return 0;
    D3P p;
    p.s6 = params->s6; p.s8 = params->s8; p.a1 = params->a1; p.a2 = params->a2;
    for (int k = 0; k < 8; ++k) { p.cov[k] = params->cov_radius_bohr[k]; p.sq[k] = params->sqrt_q[k]; }
    const int smooth = cutoff_kind == ANIHIP_CUTOFF_SMOOTH ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_d3_cn, dim3(pair_blocks(n_atoms)), dim3(256), 0, st, n_atoms, species, meta,
                       (const float4 *)ent, p, cutoff, cn);
    hipLaunchKernelGGL(k_d3_pair, dim3(pair_blocks(n_atoms)), dim3(256), 0, st, n_atoms, lo, hi, species, meta,
                       (const float4 *)ent, (const float4 *)c6_table, p, cutoff, smooth, cn, gcn, atomic_e,
                       grad_coords, virial);
    if ((grad_coords || virial) && hi > lo)
        hipLaunchKernelGGL(k_d3_cngrad, dim3(pair_blocks(hi - lo)), dim3(256), 0, st, lo, hi, species, meta,
                           (const float4 *)ent, p, cutoff, gcn, grad_coords, virial);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}
