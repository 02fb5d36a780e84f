// Reaction paths from saddle points (torchani_amd.geomopt.ReactionPathFollower): the intrinsic reaction coordinate of batches of
// molecules by the local quadratic approximation (LQA, Page & McIver 1988) on a dense model Hessian with Bofill updates, every
// molecule on its own; include/anihip.h has the definition.  The evaluation, the exact Hessian and the symmetric eigensolver
// are the caller's; here are the five launches around them:
//
//   k_irc_basis    one workgroup per molecule: the tables, w = m^-1/2, the orthonormal mass-weighted rigid motions Q (wave 0,
//                  Gram-Schmidt on vectors in LDS), gproj = P W g, then Wq = H_q Q with one wave per row (the row sum of |H_q|
//                  on the way), M = Q^T Wq and B = Wq - Q (M + mu) / 2
//   k_irc_project  blocks of 16 rows: projected = D H_q D + mu (I - D) - Q B^T - B Q^T, a streaming pass over [C][n][n]
//   k_irc_step     one workgroup per molecule: g~ = V^T gproj (one thread per mode), the first point along the direction or
//                  the LQA step (the modes spread over the 256 threads, 16 Gauss-Legendre nodes per panel and one reduction
//                  per panel, a safeguarded Newton iteration in the bracketing panel), then dx = W V alpha with one wave per
//                  row and the move
//   k_irc_commit   one workgroup per molecule: the energy test, the restore or the commit and the append to the path,
//                  xi = D (y - H s) and the three scalars of the Bofill update, the stopping tests
//   k_irc_bofill   blocks of 16 rows: the rank-two update, a streaming pass over [C][n][n]
//
// No atomics and every sum in a fixed order: bit-identical run to run.  A frozen entry (done, or with a status bit) costs an
// early exit in every kernel.
#include "saddle_common.h"

namespace anihip {

constexpr int IRC_NODES = 16;            // Gauss-Legendre nodes of a panel
constexpr int IRC_VALUES = IRC_NODES + 1;   // ... and the speed at one more time, for Newton
constexpr int IRC_PER_THREAD = SD_MAX_N / SD_THREADS;
constexpr int IRC_MAX_PANELS = 600;      // widths grow by sqrt(2): 2^300 times the first one
constexpr int IRC_MAX_NEWTON = 200;
constexpr double IRC_ROOT_TOL = 1e-12;   // |s(t) - step| <= IRC_ROOT_TOL step
constexpr double IRC_LANDING = 40.0;     // T = 40 / min lam: e^-40 of the arc is left beyond

// abscissae and weights of the 16-point Gauss-Legendre rule on [-1, 1] (the positive half)
__constant__ double c_gl_x[8] = {0.0950125098376374401853193, 0.2816035507792589132304605, 0.4580167776572273863424194,
                                 0.6178762444026437484466718, 0.7554044083550030338951012, 0.8656312023878317438804679,
                                 0.9445750230732325760779884, 0.9894009349916499325961542};
__constant__ double c_gl_w[8] = {0.1894506104550684962853967, 0.1826034150449235888667637, 0.1691565193950025381893121,
                                 0.1495959888165767320815017, 0.1246289712555338720524763, 0.0951585116824927848099251,
                                 0.0622535239386478928628438, 0.0271524594117540948517806};

struct IrcLayout {
    int64_t n;
    size_t q, b, gproj, w, disp, xi, xold, scal, total;
};

// Workspace layout (geomopt.irc_workspace_bytes mirrors it)
static IrcLayout irc_layout(int64_t C, int64_t A)
{
    IrcLayout L;
    L.n = 3 * A;
    size_t o = 0;
    L.q = o, o += sd_align((size_t)C * SD_Q * L.n * 8);
    L.b = o, o += sd_align((size_t)C * SD_Q * L.n * 8);
    L.gproj = o, o += sd_align((size_t)C * L.n * 8);
    L.w = o, o += sd_align((size_t)C * L.n * 8);
    L.disp = o, o += sd_align((size_t)C * L.n * 8);
    L.xi = o, o += sd_align((size_t)C * L.n * 8);
    L.xold = o, o += sd_align((size_t)C * L.n * 4);
    L.scal = o, o += sd_align((size_t)C * 8 * 8);
    L.total = o;
    return L;
}

// scalars of a molecule (IC_C1 .. IC_UPDATE in the order sd_bofill_scalars writes them)
enum { IC_MU = 0, IC_DS = 1, IC_ZERO = 2, IC_C1 = 3, IC_C2 = 4, IC_C3 = 5, IC_UPDATE = 6 };

struct IrcArgs {
    int64_t A, n;
    int periodic, bofill;
    int64_t max_points;
    double step, fmax, energy_floor;
    const uint8_t *kind;
    const double *masses;
    float *coords;
    double *energies;
    float *forces;
    double *H;
    const double *direction;
    float *last_step;
    double *arcs;
    int32_t *n_points, *reason, *status;
    float *path_coords;
    double *path_energies, *path_arcs;
    double *q, *b, *gproj, *w, *disp, *xi, *scal;
    float *xold;
    double *projected;         // project
    const double *lam, *V;     // step
    const double *e_new;       // commit
    const float *f_new;
};

__device__ __forceinline__ bool irc_frozen(const IrcArgs &a, int64_t c) { return a.reason[c] != 0 || a.status[c] != 0; }

__global__ __launch_bounds__(SD_THREADS) void k_irc_basis(IrcArgs a)
{
    __shared__ double s_q[SD_Q][SD_MAX_N];
    __shared__ double s_w[SD_MAX_N];
    __shared__ double s_red[SD_WAVES][4];
    __shared__ double s_m[SD_Q][SD_Q];
    __shared__ int s_flags[SD_WAVES][3];
    const int64_t c = blockIdx.x;
    if (irc_frozen(a, c)) return;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE;
    const int64_t A = a.A, n = a.n;
    const uint8_t *kind = a.kind + c * A;
    const double *mass = a.masses + c * A;
    const float *x = a.coords + c * n, *f = a.forces + c * n;

    // the tables and the centre of mass of the free atoms (per-wave partial sums, added in wave order)
    double cx = 0.0, cy = 0.0, cz = 0.0, cnt = 0.0;
    int bad_table = 0, bad_value = 0, has_fixed = 0;
    for (int64_t i = tid; i < A; i += SD_THREADS) {
        const int k = kind[i];
        bad_table |= k > 2;
        has_fixed |= k == 2;
        if (k == 1 || k == 2) {
            const double m = mass[i];
            bad_table |= !(isfinite(m) && m > 0.0);
        }
        if (k != 1) continue;
        const double m = mass[i];
        const double fx = f[3 * i], fy = f[3 * i + 1], fz = f[3 * i + 2];
        const double px = x[3 * i], py = x[3 * i + 1], pz = x[3 * i + 2];
        bad_value |= !(isfinite(fx * fx + fy * fy + fz * fz) && isfinite(px + py + pz));
        cx += m * px, cy += m * py, cz += m * pz, cnt += m;
    }
    cx = sd_wave_sum(cx), cy = sd_wave_sum(cy), cz = sd_wave_sum(cz), cnt = sd_wave_sum(cnt);
    bad_table = __any(bad_table), bad_value = __any(bad_value), has_fixed = __any(has_fixed);
    if (lane == 0) {
        s_red[wave][0] = cx, s_red[wave][1] = cy, s_red[wave][2] = cz, s_red[wave][3] = cnt;
        s_flags[wave][0] = bad_table, s_flags[wave][1] = bad_value, s_flags[wave][2] = has_fixed;
    }
    __syncthreads();
    cx = cy = cz = cnt = 0.0, bad_table = bad_value = has_fixed = 0;
    for (int w = 0; w < SD_WAVES; ++w) {
        cx += s_red[w][0], cy += s_red[w][1], cz += s_red[w][2], cnt += s_red[w][3];
        bad_table |= s_flags[w][0], bad_value |= s_flags[w][1], has_fixed |= s_flags[w][2];
    }
    __syncthreads();
    if (bad_table || bad_value) {
        if (tid == 0) a.status[c] |= bad_table ? ANIHIP_IRC_BAD_TABLE : ANIHIP_IRC_NONFINITE;
        return;
    }
    const bool use_trans = !has_fixed, use_rot = use_trans && !a.periodic;
    if (cnt > 0.0) cx /= cnt, cy /= cnt, cz /= cnt;

    double *gq = a.q + c * SD_Q * n, *gb = a.b + c * SD_Q * n, *gp = a.gproj + c * n, *gw = a.w + c * n;
    if (wave == 0) {
        // raw mass-weighted rigid motions; lane owns coordinates d = lane + 64 m and never looks at another lane's: no barrier
        double g[SD_PER_LANE];
#pragma unroll
        for (int m = 0; m < SD_PER_LANE; ++m) {
            const int64_t d = lane + WAVE * m;
            g[m] = 0.0;
            double v[SD_Q] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w = 0.0;
            if (d < n && kind[d / 3] == 1) {
                const int64_t i = d / 3;
                const int y = (int)(d - 3 * i);
                const double sm = sqrt(mass[i]);
                w = 1.0 / sm;
                g[m] = -(double)f[d] * w;
                const double rx = (double)x[3 * i] - cx, ry = (double)x[3 * i + 1] - cy, rz = (double)x[3 * i + 2] - cz;
                // component y of e_j x r: r_(y + 2) for j = y + 1, -r_(y + 1) for j = y + 2 (indices mod 3), 0 for j = y
                const double up = y == 0 ? rz : y == 1 ? rx : ry, dn = y == 0 ? ry : y == 1 ? rz : rx;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if (use_trans) v[j] = j == y ? sm : 0.0;
                    if (use_rot) v[3 + j] = j == (y + 1) % 3 ? sm * up : j == (y + 2) % 3 ? -sm * dn : 0.0;
                }
            }
#pragma unroll
            for (int j = 0; j < SD_Q; ++j) s_q[j][d] = v[j];
            s_w[d] = w;
            if (d < n) gw[d] = w;
        }
        sd_gram_schmidt(s_q, lane);
        sd_project_gradient(s_q, g, lane, n, gp, gq);   // gproj = P W g
    }
    __syncthreads();

    // Wq = H_q Q, H_q = W H W (w and Q are zero on the inactive coordinates), and the largest row sum of |H_q|
    const double *H = a.H + c * n * n;
    double rowmax = 0.0;
    for (int64_t i = wave; i < n; i += SD_WAVES) {
        const double *Hi = H + i * n;
        const double wi = s_w[i];
        double acc[SD_Q] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ab = 0.0;
        for (int64_t k = lane; k < n; k += WAVE) {
            const double h = Hi[k] * s_w[k];
            ab += fabs(h);
#pragma unroll
            for (int l = 0; l < SD_Q; ++l) acc[l] = fma(h, s_q[l][k], acc[l]);
        }
        ab = sd_wave_sum(ab) * wi;
        rowmax = isfinite(ab) ? fmax(rowmax, ab) : INFINITY;   // (fmax alone would drop a NaN)
#pragma unroll
        for (int l = 0; l < SD_Q; ++l) {
            const double v = sd_wave_sum(acc[l]);
            if (lane == 0) gb[l * n + i] = wi != 0.0 ? wi * v : 0.0;
        }
    }
    if (lane == 0) s_red[wave][0] = rowmax;
    __syncthreads();   // (the workgroup's own global writes of Wq are visible to it from here on)
    rowmax = 0.0;
    for (int w = 0; w < SD_WAVES; ++w) rowmax = fmax(rowmax, s_red[w][0]);
    if (!isfinite(rowmax)) {
        if (tid == 0) a.status[c] |= ANIHIP_IRC_NONFINITE;
        return;
    }
    const double mu = 1.0 + rowmax;
    sd_rank12_correction(s_q, s_m, gb, mu, n, tid, lane, wave);
    if (tid == 0) a.scal[c * 8 + IC_MU] = mu;
}

__global__ __launch_bounds__(SD_THREADS) void k_irc_project(IrcArgs a, int64_t blocks_per_mol)
{
    const int64_t c = blockIdx.x / blocks_per_mol, rb = blockIdx.x % blocks_per_mol;
    if (irc_frozen(a, c)) return;
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const int64_t n = a.n;
    sd_project_rows(a.kind + c * a.A, a.q + c * SD_Q * n, a.b + c * SD_Q * n, a.scal[c * 8 + IC_MU], a.H + c * n * n,
                    a.w + c * n, a.projected + c * n * n, n, rb, lane, wave);
}

// The LQA arc of one molecule: speed(t)^2 = sum_i g2_i e^(-2 lam_i t), the modes of the thread in its registers.
struct IrcArc {
    double g2[IRC_PER_THREAD], lam[IRC_PER_THREAD];
    double (*s_part)[IRC_VALUES];   // [SD_WAVES][IRC_VALUES]
    int lane, wave;

    // integral of the speed over [t0, t1] by the 16-point rule and the speed at tq; every thread calls it (two barriers) and
    // every thread gets the same two numbers: the partial sums of the waves are added in wave order
    __device__ __forceinline__ void panel(double t0, double t1, double tq, double &integral, double &speed_q)
    {
        const double mid = 0.5 * (t0 + t1), half = 0.5 * (t1 - t0);
        double part[IRC_VALUES];
#pragma unroll
        for (int j = 0; j < IRC_VALUES; ++j) {
            const double t = j == IRC_NODES ? tq : j < 8 ? mid - half * c_gl_x[7 - j] : mid + half * c_gl_x[j - 8];
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < IRC_PER_THREAD; ++m)
                if (g2[m] != 0.0) acc += g2[m] * exp(-2.0 * lam[m] * t);
            part[j] = sd_wave_sum(acc);
        }
        __syncthreads();   // (the values of the call before were read)
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < IRC_VALUES; ++j) s_part[wave][j] = part[j];
        }
        __syncthreads();
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < IRC_VALUES; ++j) {
            double v = 0.0;
            for (int w = 0; w < SD_WAVES; ++w) v += s_part[w][j];
            v = sqrt(v);
            if (j == IRC_NODES) speed_q = v;
            else sum += c_gl_w[j < 8 ? 7 - j : j - 8] * v;
        }
        integral = half * sum;
    }
};

__global__ __launch_bounds__(SD_THREADS) void k_irc_step(IrcArgs a)
{
    __shared__ double s_g[SD_MAX_N], s_gt[SD_MAX_N], s_lam[SD_MAX_N], s_al[SD_MAX_N];
    __shared__ double s_part[SD_WAVES][IRC_VALUES];
    __shared__ double s_red[SD_WAVES][4];
    __shared__ int s_bad[SD_WAVES];
    const int64_t c = blockIdx.x;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE;
    const int64_t n = a.n;
    float *ls = a.last_step + c * n;
    double *scal = a.scal + c * 8;
    if (irc_frozen(a, c)) {
        for (int64_t d = tid; d < n; d += SD_THREADS) ls[d] = 0.f;
        return;
    }
    const uint8_t *kind = a.kind + c * a.A;
    const double *V = a.V + c * n * n, *lam = a.lam + c * n, *gw = a.w + c * n;
    const bool first = a.direction != nullptr && a.n_points[c] == 0;
    for (int64_t d = tid; d < SD_MAX_N; d += SD_THREADS) {
        s_g[d] = d < n ? a.gproj[c * n + d] : 0.0;
        s_lam[d] = d < n ? lam[d] : 0.0;
        s_gt[d] = 0.0, s_al[d] = 0.0;
    }
    __syncthreads();
    // g~_k = V_k . gproj: thread k walks down column k
    IrcArc arc;
    arc.s_part = s_part, arc.lane = lane, arc.wave = wave;
    int bad = 0;
    double G2 = 0.0, lmin = INFINITY, lmax = 0.0;
#pragma unroll
    for (int m = 0; m < IRC_PER_THREAD; ++m) {
        const int64_t k = tid + SD_THREADS * m;
        arc.g2[m] = 0.0, arc.lam[m] = 0.0;
        if (k >= n) continue;
        double gt = 0.0;
        for (int64_t i = 0; i < n; ++i) gt = fma(V[i * n + k], s_g[i], gt);
        s_gt[k] = gt;
        const double l = s_lam[k];
        bad |= !(isfinite(l) && isfinite(gt));
        arc.g2[m] = gt * gt, arc.lam[m] = l;
        if (gt != 0.0) G2 += gt * gt, lmin = fmin(lmin, l), lmax = fmax(lmax, fabs(l));
    }
    G2 = sd_wave_sum(G2), lmin = sd_wave_min(lmin), lmax = sd_wave_max(lmax);
    bad = __any(bad);
    // the first point: the sign of V_0 . (M^1/2 direction), summed by wave 0 in a fixed order
    double ov = 0.0;
    if (first && wave == 0) {
        const double *dir = a.direction + c * n;
        for (int64_t i = lane; i < n; i += WAVE) {
            const double w = gw[i];
            if (w != 0.0) ov = fma(V[i * n], dir[i] / w, ov);
        }
        ov = sd_wave_sum(ov);
    }
    if (lane == 0) s_red[wave][0] = G2, s_red[wave][1] = lmin, s_red[wave][2] = lmax, s_red[wave][3] = ov, s_bad[wave] = bad;
    __syncthreads();
    G2 = 0.0, lmin = INFINITY, lmax = 0.0, bad = 0;
    for (int w = 0; w < SD_WAVES; ++w)
        G2 += s_red[w][0], lmin = fmin(lmin, s_red[w][1]), lmax = fmax(lmax, s_red[w][2]), bad |= s_bad[w];
    ov = s_red[0][3];
    int fail = bad ? ANIHIP_IRC_NONFINITE : 0;
    if (!fail && first && !isfinite(ov)) fail = ANIHIP_IRC_NONFINITE;

    // the time t of the arc length `step`, the same in every thread (all of them take every branch below together)
    const double target = a.step;
    double t_end = 0.0, ds = 0.0;
    bool landed = false, zero = false;
    if (fail) {
    } else if (first) {
        ds = target;
    } else if (!(G2 > 0.0) || !isfinite(G2)) {
        zero = G2 == 0.0;
        if (!zero) fail = ANIHIP_IRC_NONFINITE;
    } else {
        const double speed0 = sqrt(G2);
        const double t_land = lmin > 0.0 ? IRC_LANDING / lmin : INFINITY;
        double width = lmax > 0.0 ? fmin(0.01 / lmax, target / speed0) : target / speed0;
        double t0 = 0.0, s0 = 0.0, sp0 = speed0, t1 = 0.0, s1 = 0.0, sp = 0.0;
        bool bracket = false;
        for (int p = 0; p < IRC_MAX_PANELS; ++p) {
            t1 = fmin(t0 + width, t_land);
            double part;
            arc.panel(t0, t1, t1, part, sp);
            s1 = s0 + part;
            if (!(s1 < target)) {   // (a sum that is not finite ends the march too: the test below fails it)
                bracket = true;
                break;
            }
            if (t1 >= t_land) {
                landed = true;
                break;
            }
            t0 = t1, s0 = s1, sp0 = sp, width *= 1.4142135623730951;
        }
        if (landed) {
            ds = s1;
        } else if (!bracket || !isfinite(s1)) {
            fail = ANIHIP_IRC_NO_ROOT;
        } else {
            // s(t) - target on [t0, t1]: negative at t0, not at t1; Newton with the speed in closed form, bisection when it
            // leaves the bracket
            double lo = t0, hi = t1;
            double t = t0 + (target - s0) / sp0;
            if (!(t > lo && t < hi)) t = 0.5 * (lo + hi);
            bool found = false;
            for (int it = 0; it < IRC_MAX_NEWTON; ++it) {
                double part, speed;
                arc.panel(t0, t, t, part, speed);
                const double r = s0 + part - target;
                if (fabs(r) <= IRC_ROOT_TOL * target) {
                    found = true;
                    break;
                }
                if (r < 0.0) lo = t; else hi = t;
                double tn = t - r / speed;
                if (!(tn > lo && tn < hi)) tn = 0.5 * (lo + hi);
                if (!(tn > lo && tn < hi)) break;   // the bracket has collapsed to two neighbours
                t = tn;
            }
            if (!found) {   // accept the collapsed bracket if it is as good as the closed form needs
                double part, speed;
                arc.panel(t0, t, t, part, speed);
                found = fabs(s0 + part - target) <= 1e-9 * target;
            }
            if (found) t_end = t, ds = target;
            else fail = ANIHIP_IRC_NO_ROOT;
        }
    }
    // alpha in the eigenbasis
    double a2 = 0.0;
#pragma unroll
    for (int m = 0; m < IRC_PER_THREAD; ++m) {
        const int64_t k = tid + SD_THREADS * m;
        if (k >= n) continue;
        const double g = s_gt[k], l = s_lam[k];
        double al = 0.0;
        if (fail || zero) al = 0.0;
        else if (first) al = k == 0 ? (ov < 0.0 ? -target : target) : 0.0;
        else if (g == 0.0) al = 0.0;
        else if (landed) al = -g / l;
        else al = l == 0.0 ? -g * t_end : g * expm1(-l * t_end) / l;
        s_al[k] = al;
        a2 = fma(al, al, a2);
    }
    a2 = sd_wave_sum(a2);
    __syncthreads();   // (s_red of the sums above was read)
    if (lane == 0) s_red[wave][0] = a2;
    __syncthreads();
    a2 = 0.0;
    for (int w = 0; w < SD_WAVES; ++w) a2 += s_red[w][0];
    if (!fail && !isfinite(a2)) fail = ANIHIP_IRC_NONFINITE;
    if (fail) {   // left where it is
        if (tid == 0) a.status[c] |= fail;
        for (int64_t d = tid; d < n; d += SD_THREADS) ls[d] = 0.f;
        return;
    }
    // dx = W V alpha, one wave per row; the move
    float *x = a.coords + c * n, *xo = a.xold + c * n;
    double *disp = a.disp + c * n;
    double chord2 = 0.0;   // (lane 0 of a wave: the mass-weighted square of the displacement made, over the wave's rows)
    for (int64_t i = wave; i < n; i += SD_WAVES) {
        double acc = 0.0;
        for (int64_t k = lane; k < n; k += WAVE) acc = fma(V[i * n + k], s_al[k], acc);
        acc = sd_wave_sum(acc);
        if (lane == 0) {
            const float x0 = x[i];
            const float dr = kind[i / 3] == 1 ? (float)(gw[i] * acc) : 0.f;
            const float x1 = x0 + dr;
            const double made = (double)x1 - (double)x0;
            xo[i] = x0;
            x[i] = x1;
            ls[i] = dr;
            disp[i] = made;
            if (dr != 0.f) {
                const double q = made / gw[i];
                chord2 = fma(q, q, chord2);
            }
        }
    }
    // the arc increment is never below the chord between the two fp32 points the path will hold: the rounding of the
    // coordinates can lengthen a straight or a very short step past the arc of the model
    if (lane == 0) s_red[wave][1] = chord2;
    __syncthreads();
    if (tid == 0) {
        chord2 = 0.0;
        for (int w = 0; w < SD_WAVES; ++w) chord2 += s_red[w][1];
        scal[IC_DS] = fmax(ds, sqrt(chord2)), scal[IC_ZERO] = zero ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(SD_THREADS) void k_irc_commit(IrcArgs a)
{
    __shared__ double s_s[SD_MAX_N], s_xi[SD_MAX_N];
    __shared__ double s_fm[SD_WAVES];
    const int64_t c = blockIdx.x;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE;
    const int64_t n = a.n, A = a.A;
    double *scal = a.scal + c * 8;
    // everything thread 0 writes further down (status, reason, energies) is read here by every thread, before the barrier
    const bool frozen = irc_frozen(a, c);
    const double e0 = a.energies[c], e1 = a.e_new[c], ds = scal[IC_DS];
    const bool zero = scal[IC_ZERO] != 0.0;
    const int32_t np = a.n_points[c];
    __syncthreads();
    if (frozen) {
        if (tid == 0) scal[IC_UPDATE] = 0.0;
        return;
    }
    const uint8_t *kind = a.kind + c * A;
    float *x = a.coords + c * n, *f = a.forces + c * n;
    const float *xo = a.xold + c * n, *fn = a.f_new + c * n;
    const bool finite = isfinite(e1);
    const bool full = np < 0 || np >= a.max_points;   // (no slot left: never written beyond the path)
    if (!finite || e1 > e0 + a.energy_floor || full) {
        // restore the coordinates bit for bit; energies and forces still are the old ones, nothing is appended
        for (int64_t d = tid; d < n; d += SD_THREADS) x[d] = xo[d];
        if (tid == 0) {
            scal[IC_UPDATE] = 0.0;
            if (!finite) a.status[c] |= ANIHIP_IRC_NONFINITE;
            else a.reason[c] = e1 > e0 + a.energy_floor ? ANIHIP_IRC_ENERGY_ROSE : ANIHIP_IRC_PATH_FULL;
        }
        return;
    }
    if (a.bofill) {
        for (int64_t d = tid; d < SD_MAX_N; d += SD_THREADS) s_s[d] = d < n ? a.disp[c * n + d] : 0.0, s_xi[d] = 0.0;
        __syncthreads();
        sd_bofill_scalars(kind, a.H + c * n * n, f, fn, s_s, s_xi, a.xi + c * n, scal + IC_C1, n, tid, lane, wave);
    } else if (tid == 0) {
        scal[IC_UPDATE] = 0.0;
    }
    // the new forces, their largest norm over the free atoms, the point appended
    double fm = 0.0;
    for (int64_t i = tid; i < A; i += SD_THREADS) {
        if (kind[i] != 1) continue;
        const double fx = fn[3 * i], fy = fn[3 * i + 1], fz = fn[3 * i + 2];
        const double f2 = fx * fx + fy * fy + fz * fz;
        fm = f2 > fm || !isfinite(f2) ? f2 : fm;   // (a force that is not finite is no minimum: project reports it)
    }
    float *px = a.path_coords + ((int64_t)c * a.max_points + np) * n;
    for (int64_t d = tid; d < n; d += SD_THREADS) {
        f[d] = fn[d];
        px[d] = x[d];
    }
    fm = sd_wave_max(isfinite(fm) ? fm : INFINITY);
    if (lane == 0) s_fm[wave] = fm;
    __syncthreads();
    if (tid == 0) {
        fm = 0.0;
        for (int w = 0; w < SD_WAVES; ++w) fm = fmax(fm, s_fm[w]);
        const double arc = a.arcs[c] + ds;
        a.energies[c] = e1;
        a.arcs[c] = arc;
        a.path_energies[(int64_t)c * a.max_points + np] = e1;
        a.path_arcs[(int64_t)c * a.max_points + np] = arc;
        a.n_points[c] = np + 1;
        if (sqrt(fm) < a.fmax || zero) a.reason[c] = ANIHIP_IRC_MINIMUM;
        else if (np + 1 == a.max_points) a.reason[c] = ANIHIP_IRC_PATH_FULL;
    }
}

__global__ __launch_bounds__(SD_THREADS) void k_irc_bofill(IrcArgs a, int64_t blocks_per_mol)
{
#pragma clang fp contract(off)
    const int64_t c = blockIdx.x / blocks_per_mol, rb = blockIdx.x % blocks_per_mol;
    const double *scal = a.scal + c * 8;
    if (a.status[c] != 0 || scal[IC_UPDATE] == 0.0) return;   // (commit clears the flag of every entry it does not append)
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const int64_t n = a.n;
    sd_bofill_rows(a.H + c * n * n, a.disp + c * n, a.xi + c * n, scal[IC_C1], scal[IC_C2], scal[IC_C3], n, rb, lane, wave);
}

static int irc_args(const anihip_irc *state, IrcArgs &a, int64_t &C)
{
    ANIHIP_REQUIRE(state, "null pointer argument");
    const anihip_irc &S = *state;
    ANIHIP_REQUIRE(S.kind && S.masses && S.coords && S.energies && S.forces && S.hessians && S.last_step && S.arc_lengths &&
                       S.n_points && S.reason && S.status && S.path_coords && S.path_energies && S.path_arcs && S.workspace,
                   "null pointer argument");
    ANIHIP_REQUIRE(S.n_mol >= 1 && S.atoms_per_mol >= 1 && 3 * (int64_t)S.atoms_per_mol <= ANIHIP_SADDLE_MAX_COORDS,
                   "n_mol and atoms_per_mol must be >= 1 and 3 atoms_per_mol <= %d", ANIHIP_SADDLE_MAX_COORDS);
    ANIHIP_REQUIRE(S.step > 0.0 && S.step < INFINITY && S.fmax >= 0.0 && S.energy_floor >= 0.0 && S.max_points >= 1,
                   "step must be finite and > 0, fmax and energy_floor >= 0 and max_points >= 1");
    C = S.n_mol;
    const IrcLayout L = irc_layout(C, S.atoms_per_mol);
    ANIHIP_REQUIRE(C * ((L.n + SD_ROWS - 1) / SD_ROWS) < ((int64_t)1 << 31), "n_mol x 3 atoms_per_mol / %d must be below 2^31",
                   SD_ROWS);
    ANIHIP_REQUIRE(S.workspace_bytes >= L.total, "workspace holds %zu bytes, %zu needed", S.workspace_bytes, L.total);
    char *ws = (char *)S.workspace;
    a.A = S.atoms_per_mol, a.n = L.n;
    a.periodic = S.periodic != 0, a.bofill = 0;
    a.max_points = S.max_points;
    a.step = S.step, a.fmax = S.fmax, a.energy_floor = S.energy_floor;
    a.kind = S.kind, a.masses = S.masses, a.coords = S.coords, a.energies = S.energies, a.forces = S.forces, a.H = S.hessians;
    a.direction = S.direction, a.last_step = S.last_step, a.arcs = S.arc_lengths;
    a.n_points = S.n_points, a.reason = S.reason, a.status = S.status;
    a.path_coords = S.path_coords, a.path_energies = S.path_energies, a.path_arcs = S.path_arcs;
    a.q = (double *)(ws + L.q), a.b = (double *)(ws + L.b), a.gproj = (double *)(ws + L.gproj), a.w = (double *)(ws + L.w);
    a.disp = (double *)(ws + L.disp), a.xi = (double *)(ws + L.xi), a.scal = (double *)(ws + L.scal);
    a.xold = (float *)(ws + L.xold);
    a.projected = nullptr, a.lam = nullptr, a.V = nullptr, a.e_new = nullptr, a.f_new = nullptr;
    return 0;
}

}  // namespace anihip

using namespace anihip;

extern "C" size_t anihip_irc_workspace_bytes(int64_t n_mol, int64_t atoms_per_mol)
{
    if (n_mol < 1 || atoms_per_mol < 1 || 3 * atoms_per_mol > ANIHIP_SADDLE_MAX_COORDS) {
        set_error("n_mol and atoms_per_mol must be >= 1 and 3 atoms_per_mol <= %d", ANIHIP_SADDLE_MAX_COORDS);
        return 0;
    }
    return irc_layout(n_mol, atoms_per_mol).total;
}

extern "C" int anihip_irc_project(void *stream, const anihip_irc *state, double *projected)
{
    IrcArgs a;
    int64_t C;
    if (int rc = irc_args(state, a, C)) return rc;
    ANIHIP_REQUIRE(projected, "null pointer argument");
    a.projected = projected;
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = (a.n + SD_ROWS - 1) / SD_ROWS;
    hipLaunchKernelGGL(k_irc_basis, dim3((unsigned)C), dim3(SD_THREADS), 0, s, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_irc_project, dim3((unsigned)(C * blocks)), dim3(SD_THREADS), 0, s, a, blocks);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_irc_step(void *stream, const anihip_irc *state, const double *eigenvalues, const double *eigenvectors)
{
    IrcArgs a;
    int64_t C;
    if (int rc = irc_args(state, a, C)) return rc;
    ANIHIP_REQUIRE(eigenvalues && eigenvectors, "null pointer argument");
    a.lam = eigenvalues, a.V = eigenvectors;
    hipLaunchKernelGGL(k_irc_step, dim3((unsigned)C), dim3(SD_THREADS), 0, (hipStream_t)stream, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_irc_commit(void *stream, const anihip_irc *state, const double *new_energies, const float *new_forces,
                                 int32_t bofill)
{
    IrcArgs a;
    int64_t C;
    if (int rc = irc_args(state, a, C)) return rc;
    ANIHIP_REQUIRE(new_energies && new_forces, "null pointer argument");
    a.e_new = new_energies, a.f_new = new_forces, a.bofill = bofill != 0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_irc_commit, dim3((unsigned)C), dim3(SD_THREADS), 0, s, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    if (a.bofill) {
        const int64_t blocks = (a.n + SD_ROWS - 1) / SD_ROWS;
        hipLaunchKernelGGL(k_irc_bofill, dim3((unsigned)(C * blocks)), dim3(SD_THREADS), 0, s, a, blocks);
        ANIHIP_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
