// L-BFGS steps of batches of molecules (torchani_amd.geomopt): ASE's LBFGS without line search, every molecule on its own.
// The inverse-Hessian product uses the compact representation of Byrd, Nocedal and Schnabel (1994):
//
//     H g = gamma g + S t - gamma Y a,   a = R^-1 S^T g,   t = R^-T ((D + gamma Y^T Y) a - gamma Y^T g),   gamma = 1 / alpha
//
// with S, Y [n][m] the stored pairs (oldest first), R the upper triangle of S^T Y and D its diagonal.  R is never factored:
// R^-1 is kept, and it needs no triangular solve -- appending a pair appends a column,
//     R'^-1 = [[R^-1, -R^-1 r / d], [0, 1 / d]]   (r = S^T y_new, d = s_new^T y_new),
// and dropping the oldest pair keeps the trailing block of R^-1, which is the inverse of the trailing block of R.  Every
// product of a step is then a sum over the history with no dependence between its terms.  Four launches per step:
//
//   k_lb_dots       (molecule, chunk of 64 V coordinates, group of LB_SLOTS slots) per wave: the candidate pair s = x - x_prev,
//                   y = f_prev - f (formed in fp64, stored fp32 into the spare slot of the ring) and the fp64 partial sums
//                   s_j.g, y_j.g, s_j.y, y_j.y of every live slot and of the candidate; the chunk's largest |f_i|^2
//   k_lb_solve      one workgroup per molecule: the partial sums reduced in chunk order, the convergence test, the curvature
//                   test s.y > 0, the pair committed (R^-1 column, Y^T Y row and column, oldest dropped beyond `memory`),
//                   then a, the middle vector and t: the coefficients of p = -H g on f and on every stored s and y
//   k_lb_direction  one thread per atom: p_i = gamma f_i - sum_l t_l s_l,i + gamma sum_l a_l y_l,i in fp64, and per wave the
//                   largest |p_i|^2
//   k_lb_update     the largest |p_i| of the molecule, the step scaled to maxstep, coordinates moved, last_step written,
//                   x_prev / f_prev kept for the next pair
//
// The ring holds memory + 1 slots: the candidate pair is written into the spare one, so a rejected pair overwrites nothing.
// No atomics and every sum in a fixed order: trajectories are bit-identical run to run for bit-identical forces.
#include "anihip_common.h"

namespace anihip {

constexpr int LB_SLOTS = 4;        // history slots per wave of k_lb_dots
constexpr int LB_SOLVE = 256;      // threads of k_lb_solve (>= memory + 1)
constexpr int LB_MAX_M1 = ANIHIP_LBFGS_MAX_MEMORY + 1;
static_assert(LB_MAX_M1 <= LB_SOLVE + 1, "one thread per stored pair in k_lb_solve");

static inline size_t lb_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct LbLayout {
    int64_t n, n_pad, V, G, R, NV, Gc, M1;
    size_t state, coef, rinv, rinvt, yy, dd, part, pmax, p, xprev, fprev, s, y, total;
};

// Workspace layout (every region 256-byte aligned, in this order; geomopt.lbfgs_workspace_bytes mirrors it):
//   state int32 [C][4] (head, count, have_prev, -) | coef fp64 [C][2][M1] | rinv, rinvt (its transpose), yy fp64 [C][M1][M1]
//   | dd fp64 [C][M1]
//   part fp64 [C][G][4 M1 + 1] | pmax fp64 [C][Gc] | p fp64 [C][n] | xprev, fprev fp32 [C][n_pad] | S, Y fp32 [C][M1][n_pad]
static LbLayout lb_layout(int64_t C, int64_t A, int64_t memory)
{
    LbLayout L;
    L.n = 3 * A;
    L.n_pad = (L.n + 63) / 64 * 64;
    const int64_t lanes = L.n_pad / 64;
    L.V = 1;
    while (L.V < 16 && L.V < lanes) L.V <<= 1;
    L.G = (L.n_pad + 64 * L.V - 1) / (64 * L.V);
    L.M1 = memory + 1;
    L.R = (L.M1 + LB_SLOTS - 1) / LB_SLOTS;
    L.NV = 4 * L.M1 + 1;
    L.Gc = (A + 63) / 64;
    size_t o = 0;
    L.state = o, o += lb_align((size_t)C * 4 * 4);
    L.coef = o, o += lb_align((size_t)C * 2 * L.M1 * 8);
    L.rinv = o, o += lb_align((size_t)C * L.M1 * L.M1 * 8);
    L.rinvt = o, o += lb_align((size_t)C * L.M1 * L.M1 * 8);
    L.yy = o, o += lb_align((size_t)C * L.M1 * L.M1 * 8);
    L.dd = o, o += lb_align((size_t)C * L.M1 * 8);
    L.part = o, o += lb_align((size_t)C * L.G * L.NV * 8);
    L.pmax = o, o += lb_align((size_t)C * L.Gc * 8);
    L.p = o, o += lb_align((size_t)C * L.n * 8);
    L.xprev = o, o += lb_align((size_t)C * L.n_pad * 4);
    L.fprev = o, o += lb_align((size_t)C * L.n_pad * 4);
    L.s = o, o += lb_align((size_t)C * L.M1 * L.n_pad * 4);
    L.y = o, o += lb_align((size_t)C * L.M1 * L.n_pad * 4);
    L.total = o;
    return L;
}

struct LbArgs {
    int64_t A, n, n_pad, G, R, NV, Gc, M1, memory;
    double gamma, maxstep, damping, fmax;
    const uint8_t *active;
    float *coords;
    const float *forces;
    int32_t *state;
    double *coef, *rinv, *rinvt, *yy, *dd, *part, *pmax, *p;
    float *xprev, *fprev, *S, *Y, *last_step;
    uint8_t *converged;
    int32_t *n_steps;
};

__device__ __forceinline__ double lb_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ double lb_wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

// physical slot of ring position head + l, l < M1 (no integer division in the inner loops)
__device__ __forceinline__ int lb_slot(int head, int l, int M1)
{
    const int p = head + l;
    return p >= M1 ? p - M1 : p;
}

// slot j of the ring holds a stored pair: its logical position (j - head) mod M1 is below count
__device__ __forceinline__ bool lb_live(int64_t j, int64_t head, int64_t count, int64_t M1)
{
    return (j - head + M1) % M1 < count;
}

template <int V>
__global__ __launch_bounds__(WAVE) void k_lb_dots(LbArgs a)
{
    const int64_t w = blockIdx.x;
    const int64_t r = w % a.R, q = (w / a.R) % a.G, c = w / (a.R * a.G);
    if (a.converged[c]) return;
    const int32_t *st = a.state + 4 * c;
    const int64_t head = st[0], count = st[1];
    const bool have = st[2] != 0;
    if (!have && r > 0) return;   // first step: no pair, only the force maximum
    const int lane = lane_id();
    const int64_t d0 = q * 64 * V;
    const int64_t cand = (head + count) % a.M1;
    const float *fc = a.forces + c * a.n;
    const uint8_t *act = a.active + c * a.A;
    float g[V], sn[V], yn[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int64_t d = d0 + lane + 64 * k;
        g[k] = sn[k] = yn[k] = 0.f;
        if (d < a.n && act[d / 3]) {
            const float f = fc[d];
            g[k] = -f;
            if (have) {
                sn[k] = (float)((double)a.coords[c * a.n + d] - (double)a.xprev[c * a.n_pad + d]);
                yn[k] = (float)((double)a.fprev[c * a.n_pad + d] - (double)f);
            }
        }
    }
    if (have) {
        const int64_t j0 = r * LB_SLOTS, j1 = j0 + LB_SLOTS < a.M1 ? j0 + LB_SLOTS : a.M1;
        double *out = a.part + (c * a.G + q) * a.NV;
        for (int64_t j = j0; j < j1; ++j) {
            const bool is_cand = j == cand;
            if (!is_cand && !lb_live(j, head, count, a.M1)) continue;
            float *Sj = a.S + (c * a.M1 + j) * a.n_pad, *Yj = a.Y + (c * a.M1 + j) * a.n_pad;
            double sg = 0.0, yg = 0.0, sy = 0.0, yy = 0.0;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int64_t d = d0 + lane + 64 * k;
                float s = 0.f, y = 0.f;
                if (d < a.n) {
                    if (is_cand) {
                        s = sn[k], y = yn[k];
                        Sj[d] = s;
                        Yj[d] = y;
                    } else {
                        s = Sj[d], y = Yj[d];
                    }
                }
                sg = fma((double)s, (double)g[k], sg);
                yg = fma((double)y, (double)g[k], yg);
                sy = fma((double)s, (double)yn[k], sy);
                yy = fma((double)y, (double)yn[k], yy);
            }
            sg = lb_wave_sum(sg);
            yg = lb_wave_sum(yg);
            sy = lb_wave_sum(sy);
            yy = lb_wave_sum(yy);
            if (lane == 0) {
                out[4 * j + 0] = sg;
                out[4 * j + 1] = yg;
                out[4 * j + 2] = sy;
                out[4 * j + 3] = yy;
            }
        }
    }
    if (r == 0) {   // largest |f_i|^2 over the atoms whose first coordinate lies in this chunk
        const int64_t dend = d0 + 64 * V < a.n ? d0 + 64 * V : a.n;
        double m = 0.0;
        for (int64_t i = (d0 + 2) / 3 + lane; 3 * i < dend; i += 64) {
            if (!act[i]) continue;
            const double fx = fc[3 * i], fy = fc[3 * i + 1], fz = fc[3 * i + 2];
            m = fmax(m, fx * fx + fy * fy + fz * fz);
        }
        m = lb_wave_max(m);
        if (lane == 0) a.part[(c * a.G + q) * a.NV + 4 * a.M1] = m;
    }
}

__global__ __launch_bounds__(LB_SOLVE) void k_lb_solve(LbArgs a)
{
    __shared__ double s_sg[LB_MAX_M1], s_yg[LB_MAX_M1], s_sy[LB_MAX_M1], s_yy[LB_MAX_M1];
    __shared__ double s_a[LB_MAX_M1], s_w[LB_MAX_M1], s_fmax;
    const int64_t c = blockIdx.x;
    if (a.converged[c]) return;
    const int tid = threadIdx.x;
    int32_t *st = a.state + 4 * c;
    int head = st[0], count = st[1];
    const bool have = st[2] != 0;
    const int M1 = (int)a.M1, cand = lb_slot(head, count, M1);
    // partial sums of the live slots and the candidate, reduced in chunk order
    for (int64_t v = tid; v < a.NV; v += LB_SOLVE) {
        const int64_t j = v / 4;
        const bool is_max = v == 4 * M1;
        if (!is_max && !(have && (j == cand || lb_live(j, head, count, M1)))) continue;
        const double *src = a.part + c * a.G * a.NV + v;
        double acc = 0.0;
        if (is_max) {
            for (int64_t q = 0; q < a.G; ++q) acc = fmax(acc, src[q * a.NV]);
            s_fmax = acc;
        } else {
#pragma unroll 8
            for (int64_t q = 0; q < a.G; ++q) acc += src[q * a.NV];
            double *dst = (v & 3) == 0 ? s_sg : (v & 3) == 1 ? s_yg : (v & 3) == 2 ? s_sy : s_yy;
            dst[j] = acc;
        }
    }
    __syncthreads();
    if (sqrt(s_fmax) < a.fmax) {   // converged: frozen from now on
        if (tid == 0) a.converged[c] = 1;
        return;
    }
    // (rows of R^-1 are read from its transpose and rows of Y^T Y as columns: consecutive threads, consecutive addresses)
    double *rinv = a.rinv + c * M1 * M1, *rinvt = a.rinvt + c * M1 * M1, *yy = a.yy + c * M1 * M1, *dd = a.dd + c * M1;
    if (have && s_sy[cand] > 0.0) {   // curvature test (ASE appends unconditionally)
        const double d = s_sy[cand];
        if (count == a.memory) {   // drop the oldest pair: the trailing block of R^-1 stays
            head = lb_slot(head, 1, M1);
            --count;
        }
        if (tid < count) {   // new column of R^-1: -R^-1 r / d, r_k = s_k . y_new
            const int64_t pi = lb_slot(head, tid, M1);
            double acc = 0.0;
#pragma unroll 16
            for (int k = tid; k < count; ++k) {
                const int pk = lb_slot(head, k, M1);
                acc = fma(rinvt[pk * M1 + pi], s_sy[pk], acc);
            }
            rinv[pi * M1 + cand] = rinvt[cand * M1 + pi] = -acc / d;
            yy[pi * M1 + cand] = s_yy[pi];
            yy[cand * M1 + pi] = s_yy[pi];
        }
        if (tid == 0) {
            rinv[cand * M1 + cand] = rinvt[cand * M1 + cand] = 1.0 / d;
            yy[cand * M1 + cand] = s_yy[cand];
            dd[cand] = d;
        }
        ++count;
        __syncthreads();
    }
    const int m = count;
    const double gam = a.gamma;
    double *cs = a.coef + c * 2 * M1, *cy = cs + M1;
    if (tid < m) {   // a = R^-1 S^T g
        const int64_t pi = lb_slot(head, tid, M1);
        double acc = 0.0;
#pragma unroll 16
        for (int j = tid; j < m; ++j) {
            const int pj = lb_slot(head, j, M1);
            acc = fma(rinvt[pj * M1 + pi], s_sg[pj], acc);
        }
        s_a[tid] = acc;
    }
    __syncthreads();
    if (tid < m) {   // w = (D + gamma Y^T Y) a - gamma Y^T g
        const int64_t pi = lb_slot(head, tid, M1);
        double acc = 0.0;
#pragma unroll 16
        for (int j = 0; j < m; ++j) acc = fma(yy[lb_slot(head, j, M1) * M1 + pi], s_a[j], acc);
        s_w[tid] = dd[pi] * s_a[tid] + gam * acc - gam * s_yg[pi];
    }
    __syncthreads();
    if (tid < m) {   // t = R^-T w;  p = -H g = gamma f - S t + gamma Y a
        const int64_t pj = lb_slot(head, tid, M1);
        double acc = 0.0;
#pragma unroll 16
        for (int i = 0; i <= tid; ++i) acc = fma(rinv[(int64_t)lb_slot(head, i, M1) * M1 + pj], s_w[i], acc);
        cs[tid] = -acc;
        cy[tid] = gam * s_a[tid];
    }
    if (tid == 0) {
        st[0] = (int32_t)head;
        st[1] = (int32_t)count;
    }
}

__global__ __launch_bounds__(WAVE) void k_lb_direction(LbArgs a)
{
    const int64_t c = blockIdx.x / a.Gc, b = blockIdx.x % a.Gc;
    if (a.converged[c]) return;
    const int64_t i = b * 64 + lane_id();
    const int32_t *st = a.state + 4 * c;
    const int head = st[0], m = st[1], M1 = (int)a.M1;
    const double *cs = a.coef + c * 2 * M1, *cy = cs + M1;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
    if (i < a.A && a.active[c * a.A + i]) {
        const float *f = a.forces + c * a.n + 3 * i;
        p0 = a.gamma * f[0], p1 = a.gamma * f[1], p2 = a.gamma * f[2];
#pragma unroll 8
        for (int l = 0; l < m; ++l) {
            const int64_t off = (c * M1 + lb_slot(head, l, M1)) * a.n_pad + 3 * i;
            const double ts = cs[l], ay = cy[l];
            const float *s = a.S + off, *y = a.Y + off;
            p0 = fma(ay, (double)y[0], fma(ts, (double)s[0], p0));
            p1 = fma(ay, (double)y[1], fma(ts, (double)s[1], p1));
            p2 = fma(ay, (double)y[2], fma(ts, (double)s[2], p2));
        }
    }
    if (i < a.A) {
        double *p = a.p + c * a.n + 3 * i;
        p[0] = p0, p[1] = p1, p[2] = p2;
    }
    const double mx = lb_wave_max(p0 * p0 + p1 * p1 + p2 * p2);
    if (lane_id() == 0) a.pmax[c * a.Gc + b] = mx;
}

__global__ __launch_bounds__(WAVE) void k_lb_update(LbArgs a)
{
    const int64_t c = blockIdx.x / a.Gc, b = blockIdx.x % a.Gc;
    const int lane = lane_id();
    const int64_t i = b * 64 + lane;
    if (a.converged[c]) {   // frozen: coordinates untouched, no step
        if (i < a.A) {
            float *ls = a.last_step + c * a.n + 3 * i;
            ls[0] = ls[1] = ls[2] = 0.f;
        }
        return;
    }
    double m = 0.0;
    for (int64_t q = lane; q < a.Gc; q += 64) m = fmax(m, a.pmax[c * a.Gc + q]);
    const double longest = sqrt(lb_wave_max(m));
    const double scale = longest >= a.maxstep ? a.maxstep / longest : 1.0;
    if (i < a.A) {
        const bool act = a.active[c * a.A + i] != 0;
        for (int k = 0; k < 3; ++k) {
            const int64_t d = 3 * i + k;
            float *x = a.coords + c * a.n + d;
            const float x0 = *x, f = act ? a.forces[c * a.n + d] : 0.f;
            const float dr = act ? (float)(a.p[c * a.n + d] * scale * a.damping) : 0.f;
            if (act) *x = x0 + dr;
            a.last_step[c * a.n + d] = dr;
            a.xprev[c * a.n_pad + d] = x0;
            a.fprev[c * a.n_pad + d] = f;
        }
    }
    if (b == 0 && lane == 0) {
        a.n_steps[c] += 1;
        a.state[4 * c + 2] = 1;
    }
}

}  // namespace anihip

using namespace anihip;

extern "C" size_t anihip_lbfgs_workspace_bytes(int64_t n_mol, int64_t atoms_per_mol, int32_t memory)
{
    if (n_mol < 1 || atoms_per_mol < 1 || memory < 1 || memory > ANIHIP_LBFGS_MAX_MEMORY) {
        set_error("n_mol and atoms_per_mol must be >= 1 and memory in 1 .. %d", ANIHIP_LBFGS_MAX_MEMORY);
        return 0;
    }
    return lb_layout(n_mol, atoms_per_mol, memory).total;
}

extern "C" int anihip_lbfgs_step(void *stream, const anihip_lbfgs_params *params, const uint8_t *active, float *coords,
                                 const float *forces, void *workspace, size_t workspace_bytes, float *last_step,
                                 uint8_t *converged, int32_t *n_steps)
{
    ANIHIP_REQUIRE(params && active && coords && forces && workspace && last_step && converged && n_steps,
                   "null pointer argument");
    const anihip_lbfgs_params &P = *params;
    ANIHIP_REQUIRE(P.n_mol >= 1 && P.atoms_per_mol >= 1 && (int64_t)P.n_mol * P.atoms_per_mol < ((int64_t)1 << 31),
                   "n_mol and atoms_per_mol must be >= 1, n_mol x atoms_per_mol below 2^31");
    ANIHIP_REQUIRE(1 <= P.memory && P.memory <= ANIHIP_LBFGS_MAX_MEMORY, "memory must be 1 .. %d", ANIHIP_LBFGS_MAX_MEMORY);
    ANIHIP_REQUIRE(P.inv_alpha > 0.0 && P.maxstep > 0.0 && P.damping > 0.0 && P.fmax >= 0.0,
                   "inv_alpha, maxstep and damping must be > 0 and fmax >= 0");
    const int64_t C = P.n_mol, A = P.atoms_per_mol;
    const LbLayout L = lb_layout(C, A, P.memory);
    ANIHIP_REQUIRE(workspace_bytes >= L.total, "workspace holds %zu bytes, %zu needed", workspace_bytes, L.total);
    char *ws = (char *)workspace;
    LbArgs a;
    a.A = A, a.n = L.n, a.n_pad = L.n_pad, a.G = L.G, a.R = L.R, a.NV = L.NV, a.Gc = L.Gc, a.M1 = L.M1, a.memory = P.memory;
    a.gamma = P.inv_alpha, a.maxstep = P.maxstep, a.damping = P.damping, a.fmax = P.fmax;
    a.active = active, a.coords = coords, a.forces = forces;
    a.state = (int32_t *)(ws + L.state);
    a.coef = (double *)(ws + L.coef), a.rinv = (double *)(ws + L.rinv), a.rinvt = (double *)(ws + L.rinvt), a.yy = (double *)(ws + L.yy);
    a.dd = (double *)(ws + L.dd), a.part = (double *)(ws + L.part), a.pmax = (double *)(ws + L.pmax), a.p = (double *)(ws + L.p);
    a.xprev = (float *)(ws + L.xprev), a.fprev = (float *)(ws + L.fprev), a.S = (float *)(ws + L.s), a.Y = (float *)(ws + L.y);
    a.last_step = last_step, a.converged = converged, a.n_steps = n_steps;
    hipStream_t s = (hipStream_t)stream;
    const dim3 gd((unsigned)(C * L.G * L.R)), w(WAVE);
    switch (L.V) {
    case 1: hipLaunchKernelGGL(k_lb_dots<1>, gd, w, 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_lb_dots<2>, gd, w, 0, s, a); break;
    case 4: hipLaunchKernelGGL(k_lb_dots<4>, gd, w, 0, s, a); break;
    case 8: hipLaunchKernelGGL(k_lb_dots<8>, gd, w, 0, s, a); break;
    default: hipLaunchKernelGGL(k_lb_dots<16>, gd, w, 0, s, a); break;
    }
    ANIHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_lb_solve, dim3((unsigned)C), dim3(LB_SOLVE), 0, s, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_lb_direction, dim3((unsigned)(C * L.Gc)), w, 0, s, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_lb_update, dim3((unsigned)(C * L.Gc)), w, 0, s, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}
