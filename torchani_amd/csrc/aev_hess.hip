// Second-order AEV backward: the derivative of the analytic backward along a coordinate direction, for Hessians of the
// energy with respect to the coordinates (anihip_aev_backward_second, include/anihip.h).
//
// The first-order backward maps grad_aev to grad_coords = J^T grad_aev (J = d aev / d coords).  A Hessian-vector product
// H v = J^T (H_net (J v)) + (D_v J^T) g needs, besides the AEV-space product, the derivative of J^T g itself along the
// motion v with g held fixed.  This kernel computes, for n_dir directions t[k] at once,
//
//     out[k] += J^T dgrad[k] + (D_{t[k]} J^T) grad_aev
//
// as ONE dual-number evaluation of the backward of aev_generic.hip: every quantity is a pair (value, derivative along
// t[k]); the geometry of an entry carries d' = t_j - t_i (any periodic image: the shift does not move), grad_aev carries
// dgrad[k], and the tangent part of the resulting gradient is exactly the sum above.  The second derivatives follow
// mechanically from the first-order chain rule of the backward (cutoffs.py:71-101, aev/_terms.py:99-104,171-186,324-343
// of the reference restated in aev_generic.hip); the only explicitly written second derivatives are those of the two
// cutoff envelopes.
//
// One wave per (central atom, direction): blockIdx.y = direction.  Same row format, same push of the per-neighbor sums
// (LDS ds_add_f32, then one global float atomic per component per neighbor) as the first-order general kernel; any grid
// the general kernels serve, the tuned ANI-1x / ANI-2x grids included (their tables hold the plain shifts as well).
#include "aev_gen.h"
#include "hess_rows.h"

namespace anihip {

constexpr int HESS_WPB = 2;
constexpr float H_LOG2E = 1.4426950408889634f;
constexpr float H_LN2 = 0.6931471805599453f;
constexpr float H_PI = 3.14159265358979323846f;

// ---- dual numbers: v + d eps, eps^2 = 0 ----------------------------------------------------------------------------
struct Dual {
    float v, d;
};
__device__ __forceinline__ Dual dl(float v, float d = 0.f) { return Dual{v, d}; }
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return Dual{a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return Dual{a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dual operator-(Dual a) { return Dual{-a.v, -a.d}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return Dual{a.v * b.v, a.v * b.d + a.d * b.v}; }
__device__ __forceinline__ Dual operator*(float s, Dual a) { return Dual{s * a.v, s * a.d}; }
__device__ __forceinline__ Dual operator*(Dual a, float s) { return Dual{s * a.v, s * a.d}; }
__device__ __forceinline__ Dual operator+(Dual a, float s) { return Dual{a.v + s, a.d}; }
__device__ __forceinline__ Dual operator-(Dual a, float s) { return Dual{a.v - s, a.d}; }
__device__ __forceinline__ Dual operator-(float s, Dual a) { return Dual{s - a.v, -a.d}; }
__device__ __forceinline__ Dual operator+(float s, Dual a) { return Dual{s + a.v, a.d}; }
__device__ __forceinline__ Dual &operator+=(Dual &a, Dual b) { a.v += b.v; a.d += b.d; return a; }
__device__ __forceinline__ Dual dinv(Dual a) { const float r = 1.0f / a.v; return Dual{r, -a.d * r * r}; }
__device__ __forceinline__ Dual dexp2(Dual a) { const float e = __builtin_amdgcn_exp2f(a.v); return Dual{e, e * H_LN2 * a.d}; }
__device__ __forceinline__ Dual dlog2(Dual a) { return Dual{__builtin_amdgcn_logf(a.v), a.d / (a.v * H_LN2)}; }
__device__ __forceinline__ Dual dsqrt(Dual a) { const float s = sqrtf(a.v); return Dual{s, s > 0.f ? 0.5f * a.d / s : 0.f}; }
__device__ __forceinline__ Dual dmax(Dual a, float c) { return a.v >= c ? a : Dual{c, 0.f}; }

// {fc, fc', fc''} of either envelope at r (first and second derivative with respect to r)
__device__ __forceinline__ float3 hess_cutoff(float r, float rc, bool smooth)
{
    if (smooth) {   // fc = exp(1 - 1/m), m = 1 - (r/rc)^2;  p = dm/dr = -2 r / rc^2
        const float q = r / rc;
        const float m1 = (1.0f - q) * (1.0f + q);
        const float im = 1.0f / fmaxf(1e-10f, m1);
        const float f = __builtin_amdgcn_exp2f((1.0f - im) * H_LOG2E);
        if (!(m1 - 1e-10f >= 0.0f)) return make_float3(f, 0.f, 0.f);
        const float p = -2.0f * r / (rc * rc);
        const float im2 = im * im;
        const float f1 = p * f * im2;
        // d/dr (p f im^2) = p' f im^2 + p f' im^2 + 2 p f im (d im/dr),  d im/dr = -im^2 p
        const float f2 = (-2.0f / (rc * rc)) * f * im2 + p * f1 * im2 - 2.0f * p * p * f * im2 * im;
        return make_float3(f, f1, f2);
    }
    const float x = r / rc;   // fc = cos(pi x) / 2 + 1/2; the hardware cosf / sinf take revolutions
    const float k = H_PI / rc;
    const float c = __builtin_amdgcn_cosf(0.5f * x), s = __builtin_amdgcn_sinf(0.5f * x);
    return make_float3(0.5f * c + 0.5f, -0.5f * k * s, -0.5f * k * k * c);
}

// M (hess_rows.h): Dense -- central atoms lo <= q < hi, direction blockIdx.y of tangent, dgrad and out.  Item
// (anihip_aev_backward_second_items, sparse Hessians) and Strain (anihip_aev_backward_second_strain_items, strain second
// derivatives): the wave's index q runs over item rows lo <= q < hi, dgrad row q, output slab row_dir[q] - dir0 of out
// [n_slabs][n_atoms][3] (Strain: dir0 = 0, n_slabs = 9); blockIdx.y = 0.  A strain row also adds sum_e d_{e,x} g_{e,y} --
// g = the tangent part of d E_i / d d_e, i.e. the derivative of the row's virial along S_ab -- to
// sa.ss[i / sa.atoms_per_mol][3 x + y][3 a + b] (one wave sum per component, one fp64 atomic per component and row).
template <Dir M>
__global__ __launch_bounds__(HESS_WPB * WAVE) void k_aev_bwd2(GenArgs a, const float *__restrict__ tab, int64_t n_atoms,
                                                             int64_t lo, int64_t hi, const int32_t *__restrict__ species,
                                                             const uint32_t *__restrict__ meta,
                                                             const float4 *__restrict__ ent,
                                                             const float *__restrict__ grad_aev,
                                                             const float *__restrict__ tangent,
                                                             const float *__restrict__ dgrad, float *__restrict__ out,
                                                             const int32_t *__restrict__ row_atom,
                                                             const int32_t *__restrict__ row_dir, int64_t dir0,
                                                             int64_t n_slabs, StrainAcc sa)
{
    constexpr bool ITEMS = M != Dir::Dense, STRAIN = M == Dir::Strain;
    __shared__ float4 s_u[HESS_WPB][MAXR];     // unit vector, r
    __shared__ float4 s_ud[HESS_WPB][MAXR];    // its derivative along the direction: u', r'
    __shared__ float4 s_fcr[HESS_WPB][MAXR];   // radial envelope fc, fc', fc''
    __shared__ float4 s_fca[HESS_WPB][MAXR];   // angular envelope (angular-range entries)
    __shared__ int s_j[HESS_WPB][MAXR];
    __shared__ float s_g[HESS_WPB][3][MAXR];   // tangent part of the gradient on the neighbors of the row
    const int wib = threadIdx.x >> 6, lane = lane_id();
    float4 *su = s_u[wib], *sud = s_ud[wib], *sfr = s_fcr[wib], *sfa = s_fca[wib];
    int *sj = s_j[wib];
    float *gx = s_g[wib][0], *gy = s_g[wib][1], *gz = s_g[wib][2];
    const int64_t dir = blockIdx.y;
    const float *tg = ITEMS ? nullptr : tangent + (size_t)dir * 3 * n_atoms;
    const float *dg = ITEMS ? dgrad : dgrad + (size_t)dir * n_atoms * a.L;
    float *o = out + (size_t)dir * 3 * n_atoms;
    const int64_t nw = (int64_t)gridDim.x * HESS_WPB;
    const int nAZ = a.nA * a.nZ;
    for (int64_t q = lo + blockIdx.x * (int64_t)HESS_WPB + wib; q < hi; q += nw) {
        const DirRow row = ITEMS ? dir_item(row_atom, row_dir, q, dir0) : DirRow{q, dir, -1, 0};
        const int64_t i = row.i;
        if (species[i] < 0) continue;
        const GenHdr h = gen_hdr(meta, i);
        const int nR = h.nA + h.nF;
        if (nR == 0) continue;
        if (ITEMS) {
            if (row.slab < 0 || row.slab >= n_slabs) continue;   // (a row outside the caller's slabs)
            o = out + (size_t)row.slab * 3 * n_atoms;
        }
        const float3 ti = dir_tangent3<M>(tg, row, i);
        for (int e = lane; e < nR; e += WAVE) {
            const float4 d = ent[h.start + e];
            const float r = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z), ir = 1.0f / r;
            const float ux = d.x * ir, uy = d.y * ir, uz = d.z * ir;
            const int jn = (int)(__float_as_uint(d.w) & IDX_MASK);
            const float3 dp = dir_dprime<M>(tg, row, ti, jn, make_float3(d.x, d.y, d.z));
            const float dx = dp.x, dy = dp.y, dz = dp.z;
            const float rd = ux * dx + uy * dy + uz * dz;
            su[e] = make_float4(ux, uy, uz, r);
            sud[e] = make_float4((dx - ux * rd) * ir, (dy - uy * rd) * ir, (dz - uz * rd) * ir, rd);
            const float3 fr = hess_cutoff(r, a.Rcr, a.smooth != 0);
            sfr[e] = make_float4(fr.x, fr.y, fr.z, 0.f);
            const float3 fa = e < h.nA ? hess_cutoff(r, a.Rca, a.smooth != 0) : make_float3(0.f, 0.f, 0.f);
            sfa[e] = make_float4(fa.x, fa.y, fa.z, 0.f);
            sj[e] = jn;
        }
        wave_sync();
        const float *w = grad_aev + (size_t)i * a.L;
        const float *wd = dg + (size_t)q * a.L;
        float ox = 0.f, oy = 0.f, oz = 0.f;   // minus the tangent part of the gradient on the central atom, per lane
        // ---- radial (lane = neighbor) ----
        for (int e = lane; e < nR; e += WAVE) {
            const float4 U = su[e], Ud = sud[e], F = sfr[e];
            const Dual r = dl(U.w, Ud.w), fc = dl(F.x, F.y * Ud.w), fcd = dl(F.y, F.z * Ud.w);
            const int t = (int)(__float_as_uint(ent[h.start + e].w) >> 28);
            const float *wr = w + t * a.nR, *wrd = wd + t * a.nR;
            Dual dR = dl(0.f);
            for (int k = 0; k < a.nR; ++k) {
                const Dual dr = r - tab[TAB_SHFR + k];
                const Dual ex = 0.25f * dexp2(-a.EtaR * H_LOG2E * (dr * dr));
                dR += dl(wr[k], wrd[k]) * (ex * fcd - 2.0f * a.EtaR * (dr * ex * fc));
            }
            // v = dR u:  tangent part dR.d u + dR.v u'
            const float vx = dR.d * U.x + dR.v * Ud.x, vy = dR.d * U.y + dR.v * Ud.y, vz = dR.d * U.z + dR.v * Ud.z;
            gx[e] = vx; gy[e] = vy; gz[e] = vz;
            ox += vx; oy += vy; oz += vz;
        }
        wave_sync();
        // ---- angular (lane = pair) ----
        int o1 = 0;
        for (int s1 = 0; s1 < a.S; ++s1) {
            const int n1 = gen_cnt(h.pkA, s1);
            int o2 = o1;
            for (int s2 = s1; s2 < a.S; ++s2) {
                const int n2 = gen_cnt(h.pkA, s2);
                const bool same = s1 == s2;
                const int np = same ? (n1 * (n1 - 1)) / 2 : n1 * n2;
                const int boff = a.radlen + gen_triu(a.S, s1, s2) * nAZ;
                const float *ww = w + boff, *wwd = wd + boff;
                for (int t0 = 0; t0 < np; t0 += WAVE) {
                    const int t = t0 + lane;
                    if (t < np) {
                        int j, k;
                        gen_pair(same, t, n1, n2, j, k);
                        const int e1 = o1 + j, e2 = (same ? o1 : o2) + k;
                        const float4 A1 = su[e1], A2 = su[e2], B1 = sud[e1], B2 = sud[e2];
                        const float4 G1 = sfa[e1], G2 = sfa[e2];
                        const Dual u1x = dl(A1.x, B1.x), u1y = dl(A1.y, B1.y), u1z = dl(A1.z, B1.z), r1 = dl(A1.w, B1.w);
                        const Dual u2x = dl(A2.x, B2.x), u2y = dl(A2.y, B2.y), u2z = dl(A2.z, B2.z), r2 = dl(A2.w, B2.w);
                        const Dual f1c = dl(G1.x, G1.y * B1.w), f1cd = dl(G1.y, G1.z * B1.w);
                        const Dual f2c = dl(G2.x, G2.y * B2.w), f2cd = dl(G2.y, G2.z * B2.w);
                        const Dual c = u1x * u2x + u1y * u2y + u1z * u2z;
                        const Dual ct = 0.95f * c;
                        const Dual sn = dsqrt(dmax(1.0f - ct * ct, 0.f));
                        const Dual rm = 0.5f * (r1 + r2);
                        Dual C0 = dl(0.f), Cth = dl(0.f), CR = dl(0.f);   // sum w f1 f2, sum w f1' f2, sum w f1 f2'
                        for (int z = 0; z < a.nZ; ++z) {
                            const float cz = tab[TAB_COSZ + z], sz = tab[TAB_SINZ + z];
                            const Dual hh = dmax(0.5f + 0.5f * (ct * cz + sn * sz), 1e-30f);
                            const Dual lg = dlog2(hh);
                            const Dual f1 = 2.0f * dexp2(a.Zeta * lg);
                            const Dual df1 = -a.Zeta * (dexp2((a.Zeta - 1.0f) * lg) * (sn * cz - ct * sz));
                            for (int u = 0; u < a.nA; ++u) {
                                const Dual dr = rm - tab[TAB_SHFA + u];
                                const Dual f2 = dexp2(-a.EtaA * H_LOG2E * (dr * dr));
                                const Dual wz = dl(ww[u * a.nZ + z], wwd[u * a.nZ + z]);
                                const Dual wf2 = wz * f2;
                                C0 += f1 * wf2;
                                Cth += df1 * wf2;
                                CR += f1 * (-2.0f * a.EtaA) * (dr * wf2);
                            }
                        }
                        const Dual fcc = f1c * f2c;
                        const Dual kth = Cth * fcc * (-0.95f * dinv(sn));   // dE / d cos(angle)
                        const Dual k1 = 0.5f * CR * fcc + C0 * f1cd * f2c;
                        const Dual k2 = 0.5f * CR * fcc + C0 * f1c * f2cd;
                        const Dual i1 = dinv(r1), i2 = dinv(r2);
                        const Dual a1 = kth * i1, a2 = kth * i2;
                        const Dual g1x = a1 * (u2x - c * u1x) + k1 * u1x;
                        const Dual g1y = a1 * (u2y - c * u1y) + k1 * u1y;
                        const Dual g1z = a1 * (u2z - c * u1z) + k1 * u1z;
                        const Dual g2x = a2 * (u1x - c * u2x) + k2 * u2x;
                        const Dual g2y = a2 * (u1y - c * u2y) + k2 * u2y;
                        const Dual g2z = a2 * (u1z - c * u2z) + k2 * u2z;
                        atomicAdd(&gx[e1], g1x.d); atomicAdd(&gy[e1], g1y.d); atomicAdd(&gz[e1], g1z.d);
                        atomicAdd(&gx[e2], g2x.d); atomicAdd(&gy[e2], g2y.d); atomicAdd(&gz[e2], g2z.d);
                        ox += g1x.d + g2x.d; oy += g1y.d + g2y.d; oz += g1z.d + g2z.d;
                    }
                }
                o2 += n2;
            }
            o1 += n1;
        }
        wave_sync();
        // ---- push: every neighbor its sum, the central atom minus the total ----
        float vs[STRAIN ? 9 : 1];   // STRAIN: this lane's part of sum_e d_x g_y, component 3 x + y
#pragma unroll
        for (int c = 0; c < (STRAIN ? 9 : 1); ++c) vs[c] = 0.f;
        for (int e = lane; e < nR; e += WAVE) {
            const size_t jn = (size_t)sj[e];
            atomicAdd(o + 3 * jn, gx[e]);
            atomicAdd(o + 3 * jn + 1, gy[e]);
            atomicAdd(o + 3 * jn + 2, gz[e]);
            if (STRAIN) {
                const float4 d = ent[h.start + e];
                const float dd[3] = {d.x, d.y, d.z}, gg[3] = {gx[e], gy[e], gz[e]};
#pragma unroll
                for (int x = 0; x < 3; ++x)
#pragma unroll
                    for (int y = 0; y < 3; ++y) vs[(STRAIN ? 3 * x + y : 0)] += dd[x] * gg[y];
            }
        }
        if (STRAIN) {   // lane c < 9 keeps the row's component c and adds it to ss[mol][c][row direction]
            float mine = 0.f;
#pragma unroll
            for (int c = 0; c < (STRAIN ? 9 : 1); ++c) {
                const float t = wave_sum(vs[c]);
                if (lane == c) mine = t;
            }
            if (lane < 9) atomicAdd(sa.ss + (size_t)(i / sa.atoms_per_mol) * 81 + 9 * lane + row.slab, (double)mine);
        }
        const float tx = wave_sum(ox), ty = wave_sum(oy), tz = wave_sum(oz);
        if (lane == 0) {
            atomicAdd(o + 3 * i, -tx);
            atomicAdd(o + 3 * i + 1, -ty);
            atomicAdd(o + 3 * i + 2, -tz);
        }
        wave_sync();
    }
}

// every entry point: central atoms (Dense; grid.y = the n_dir directions) or item rows lo <= q < hi
template <Dir M>
static int bwd2_launch(void *stream, const anihip_aev_params *p, const float *table, int64_t n_atoms, int64_t lo, int64_t hi,
                       int64_t n_dir, const int32_t *species, const uint32_t *meta, const float *ent, const float *grad_aev,
                       const float *tangent, const float *dgrad, float *out, const int32_t *row_atom,
                       const int32_t *row_dir, int64_t dir0, int64_t n_slabs, StrainAcc sa)
{
    GenArgs a;
    if (int rc = gen_args(p, &a)) return rc;
    if (hi == lo || n_dir == 0) return 0;
    const int64_t b = std::min<int64_t>((hi - lo + HESS_WPB - 1) / HESS_WPB, M == Dir::Dense ? 1024 : 4096);
    hipLaunchKernelGGL(k_aev_bwd2<M>, dim3((unsigned)b, (unsigned)n_dir), dim3(HESS_WPB * WAVE), 0, (hipStream_t)stream, a,
                       table, n_atoms, lo, hi, species, meta, (const float4 *)ent, grad_aev, tangent, dgrad, out, row_atom,
                       row_dir, dir0, n_slabs, sa);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace anihip

using namespace anihip;

extern "C" int anihip_aev_backward_second(void *stream, const anihip_aev_params *p, const float *table, int64_t n_atoms,
                                          int64_t lo, int64_t hi, const int32_t *species, const uint32_t *meta,
                                          const float *ent, const float *grad_aev, int64_t n_dir, const float *tangent,
                                          const float *dgrad, float *out, uint32_t *status)
{
    ANIHIP_REQUIRE(p && table && species && meta && ent && grad_aev && tangent && dgrad && out, "null pointer argument");
    ANIHIP_REQUIRE(0 <= lo && lo <= hi && hi <= n_atoms, "central range outside 0..n_atoms");
    ANIHIP_REQUIRE(0 <= n_dir && n_dir <= 65535, "n_dir must be 0..65535 (got %lld)", (long long)n_dir);
    (void)status;
    return bwd2_launch<Dir::Dense>(stream, p, table, n_atoms, lo, hi, n_dir, species, meta, ent, grad_aev, tangent, dgrad,
                                   out, nullptr, nullptr, 0, 0, StrainAcc{});
}

extern "C" int anihip_aev_backward_second_items(void *stream, const anihip_aev_params *p, const float *table,
                                                int64_t n_atoms, const int32_t *species, const uint32_t *meta,
                                                const float *ent, const float *grad_aev, int64_t n_rows,
                                                const int32_t *row_atom, const int32_t *row_dir, int64_t dir0,
                                                int64_t n_dir, const float *dgrad, float *out)
{
    ANIHIP_REQUIRE(p && table && species && meta && ent && grad_aev && row_atom && row_dir && dgrad && out,
                   "null pointer argument");
    ANIHIP_REQUIRE(n_atoms >= 0 && n_rows >= 0 && n_dir >= 0, "negative size");
    return bwd2_launch<Dir::Item>(stream, p, table, n_atoms, 0, n_rows, 1, species, meta, ent, grad_aev, nullptr, dgrad, out,
                                  row_atom, row_dir, dir0, n_dir, StrainAcc{});
}

extern "C" int anihip_aev_backward_second_strain_items(void *stream, const anihip_aev_params *p, const float *table,
                                                       int64_t n_atoms, int64_t atoms_per_mol, const int32_t *species,
                                                       const uint32_t *meta, const float *ent, const float *grad_aev,
                                                       int64_t n_rows, const int32_t *row_atom, const int32_t *row_dir,
                                                       const float *dgrad, float *out, double *ss)
{
    ANIHIP_REQUIRE(p && table && species && meta && ent && grad_aev && row_atom && row_dir && dgrad && out && ss,
                   "null pointer argument");
    ANIHIP_REQUIRE(n_atoms >= 0 && n_rows >= 0, "negative size");
    ANIHIP_REQUIRE(atoms_per_mol >= 1 && n_atoms % atoms_per_mol == 0,
                   "atoms_per_mol must be >= 1 and divide n_atoms (got %lld, %lld)", (long long)atoms_per_mol,
                   (long long)n_atoms);
    return bwd2_launch<Dir::Strain>(stream, p, table, n_atoms, 0, n_rows, 1, species, meta, ent, grad_aev, nullptr, dgrad,
                                    out, row_atom, row_dir, 0, 9, StrainAcc{ss, nullptr, atoms_per_mol});
}
