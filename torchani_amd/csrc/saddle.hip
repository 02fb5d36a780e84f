// Saddle-point search of batches of molecules (torchani_amd.geomopt.SaddleOptimizer): partitioned rational-function
// optimization on a dense model Hessian with Bofill updates, every molecule on its own; include/anihip.h has the definition.
// The evaluation, the exact Hessian and the symmetric eigensolver are the caller's; here are the five launches around them:
//
//   k_sd_basis    one workgroup per molecule: the convergence test, the orthonormal rigid motions Q (wave 0, Gram-Schmidt on
//                 vectors in LDS, every lane on its own coordinates: no barrier), gproj = P g, then W = H Q with one wave
//                 per row (coalesced fp64 loads, the row sum of |H| on the way), M = Q^T W and B = W - Q (M + mu) / 2
//   k_sd_project  blocks of 16 rows: projected = D H D + mu (I - D) - Q B^T - B Q^T, a streaming pass over [C][n][n]
//   k_sd_step     one workgroup per molecule: g~ = V^T gproj and the overlaps (one thread per mode: consecutive threads read
//                 consecutive addresses of a row of V), the mode, the secular equation and the trust radius by wave 0 on
//                 vectors in LDS, then s = V s~ with one wave per row and the move
//   k_sd_accept   one workgroup per molecule: the ratio test, the restore or the commit, xi = D (y - H s) with one wave per
//                 row and the three scalars of the Bofill update
//   k_sd_bofill   blocks of 16 rows: the rank-two update, a streaming pass over [C][n][n]
//
// No atomics and every sum in a fixed order: bit-identical run to run.  A frozen entry (converged, or with a status bit) costs
// an early exit in every kernel.  The Gram-Schmidt, the rank-12 correction and the two Bofill passes are device functions of
// saddle_common.h, which irc.hip shares.
#include "saddle_common.h"

namespace anihip {

struct SdLayout {
    int64_t n;
    size_t q, b, gproj, disp, xi, xold, scal, total;
};

// Workspace layout (geomopt.saddle_workspace_bytes mirrors it)
static SdLayout sd_layout(int64_t C, int64_t A)
{
    SdLayout L;
    L.n = 3 * A;
    size_t o = 0;
    L.q = o, o += sd_align((size_t)C * SD_Q * L.n * 8);
    L.b = o, o += sd_align((size_t)C * SD_Q * L.n * 8);
    L.gproj = o, o += sd_align((size_t)C * L.n * 8);
    L.disp = o, o += sd_align((size_t)C * L.n * 8);
    L.xi = o, o += sd_align((size_t)C * L.n * 8);
    L.xold = o, o += sd_align((size_t)C * L.n * 4);
    L.scal = o, o += sd_align((size_t)C * 8 * 8);
    L.total = o;
    return L;
}

// scalars of a molecule
enum { SC_MU = 0, SC_PRED = 1, SC_SNORM = 2, SC_C1 = 3, SC_C2 = 4, SC_C3 = 5, SC_UPDATE = 6 };

struct SdArgs {
    int64_t A, n;
    int periodic, follow, bofill;
    double fmax, max_trust, min_trust, energy_floor;
    const uint8_t *kind;
    float *coords;
    double *energies;
    float *forces;
    double *H;
    double *trust, *eigenvalue, *modes;
    float *last_step;
    uint8_t *accepted, *converged;
    int32_t *n_steps, *n_rejected, *status;
    double *q, *b, *gproj, *disp, *xi, *scal;
    float *xold;
    double *projected;         // project
    const double *lam, *V;     // step
    const double *e_new;       // accept
    const float *f_new;
};

__device__ __forceinline__ bool sd_frozen(const SdArgs &a, int64_t c) { return a.converged[c] != 0 || a.status[c] != 0; }

__global__ __launch_bounds__(SD_THREADS) void k_sd_basis(SdArgs a)
{
    __shared__ double s_q[SD_Q][SD_MAX_N];
    __shared__ double s_red[SD_WAVES][4];
    __shared__ double s_m[SD_Q][SD_Q];
    __shared__ int s_flags[SD_WAVES][3];
    const int64_t c = blockIdx.x;
    if (sd_frozen(a, c)) return;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE;
    const int64_t A = a.A, n = a.n;
    const uint8_t *kind = a.kind + c * A;
    const float *x = a.coords + c * n, *f = a.forces + c * n;

    // the convergence test, the table, the centroid (per-wave partial sums, added in wave order)
    double fm = 0.0, cx = 0.0, cy = 0.0, cz = 0.0, cnt = 0.0;
    int bad_table = 0, bad_value = 0, has_fixed = 0;
    for (int64_t i = tid; i < A; i += SD_THREADS) {
        const int k = kind[i];
        bad_table |= k > 2;
        has_fixed |= k == 2;
        if (k != 1) continue;
        const double fx = f[3 * i], fy = f[3 * i + 1], fz = f[3 * i + 2];
        const double px = x[3 * i], py = x[3 * i + 1], pz = x[3 * i + 2];
        const double f2 = fx * fx + fy * fy + fz * fz;
        bad_value |= !(isfinite(f2) && isfinite(px + py + pz));
        fm = fmax(fm, f2);
        cx += px, cy += py, cz += pz, cnt += 1.0;
    }
    fm = sd_wave_max(fm);
    cx = sd_wave_sum(cx), cy = sd_wave_sum(cy), cz = sd_wave_sum(cz), cnt = sd_wave_sum(cnt);
    bad_table = __any(bad_table), bad_value = __any(bad_value), has_fixed = __any(has_fixed);
    if (lane == 0) {
        s_red[wave][0] = cx, s_red[wave][1] = cy, s_red[wave][2] = cz, s_red[wave][3] = cnt;
        s_m[0][wave] = fm;
        s_flags[wave][0] = bad_table, s_flags[wave][1] = bad_value, s_flags[wave][2] = has_fixed;
    }
    __syncthreads();
    fm = 0.0, cx = cy = cz = cnt = 0.0, bad_table = bad_value = has_fixed = 0;
    for (int w = 0; w < SD_WAVES; ++w) {
        fm = fmax(fm, s_m[0][w]);
        cx += s_red[w][0], cy += s_red[w][1], cz += s_red[w][2], cnt += s_red[w][3];
        bad_table |= s_flags[w][0], bad_value |= s_flags[w][1], has_fixed |= s_flags[w][2];
    }
    __syncthreads();
    if (bad_table || bad_value) {
        if (tid == 0) a.status[c] |= bad_table ? ANIHIP_SADDLE_BAD_TABLE : ANIHIP_SADDLE_NONFINITE;
        return;
    }
    if (sqrt(fm) < a.fmax) {   // converged: frozen from now on
        if (tid == 0) a.converged[c] = 1;
        return;
    }
    const bool use_trans = !has_fixed, use_rot = use_trans && !a.periodic;
    if (cnt > 0.0) cx /= cnt, cy /= cnt, cz /= cnt;

    double *gq = a.q + c * SD_Q * n, *gb = a.b + c * SD_Q * n, *gp = a.gproj + c * n;
    if (wave == 0) {
        // raw rigid motions; lane owns coordinates d = lane + 64 m and never looks at another lane's: no barrier
        double g[SD_PER_LANE];
#pragma unroll
        for (int m = 0; m < SD_PER_LANE; ++m) {
            const int64_t d = lane + WAVE * m;
            g[m] = 0.0;
            double v[SD_Q] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (d < n && kind[d / 3] == 1) {
                const int64_t i = d / 3;
                const int y = (int)(d - 3 * i);
                g[m] = -(double)f[d];
                const double rx = (double)x[3 * i] - cx, ry = (double)x[3 * i + 1] - cy, rz = (double)x[3 * i + 2] - cz;
                // component y of e_j x r: r_(y + 2) for j = y + 1, -r_(y + 1) for j = y + 2 (indices mod 3), 0 for j = y
                const double up = y == 0 ? rz : y == 1 ? rx : ry, dn = y == 0 ? ry : y == 1 ? rz : rx;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if (use_trans) v[j] = j == y ? 1.0 : 0.0;
                    if (use_rot) v[3 + j] = j == (y + 1) % 3 ? up : j == (y + 2) % 3 ? -dn : 0.0;
                }
            }
#pragma unroll
            for (int j = 0; j < SD_Q; ++j) s_q[j][d] = v[j];
        }
        sd_gram_schmidt(s_q, lane);
        sd_project_gradient(s_q, g, lane, n, gp, gq);   // gproj = P g
    }
    __syncthreads();

    // W = D H Q (Q is zero on the inactive coordinates, so the columns need no mask) and the largest row sum of |H|
    const double *H = a.H + c * n * n;
    double rowmax = 0.0;
    for (int64_t i = wave; i < n; i += SD_WAVES) {
        const double *Hi = H + i * n;
        double acc[SD_Q] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ab = 0.0;
        for (int64_t k = lane; k < n; k += WAVE) {
            const double h = Hi[k];
            ab += fabs(h);
#pragma unroll
            for (int l = 0; l < SD_Q; ++l) acc[l] = fma(h, s_q[l][k], acc[l]);
        }
        ab = sd_wave_sum(ab);
        rowmax = fmax(rowmax, ab);
        const bool act = kind[i / 3] == 1;
#pragma unroll
        for (int l = 0; l < SD_Q; ++l) {
            const double w = sd_wave_sum(acc[l]);
            if (lane == 0) gb[l * n + i] = act ? w : 0.0;
        }
    }
    if (lane == 0) s_red[wave][0] = rowmax;
    __syncthreads();   // (the workgroup's own global writes of W are visible to it from here on)
    rowmax = 0.0;
    for (int w = 0; w < SD_WAVES; ++w) rowmax = fmax(rowmax, s_red[w][0]);
    if (!isfinite(rowmax)) {
        if (tid == 0) a.status[c] |= ANIHIP_SADDLE_NONFINITE;
        return;
    }
    const double mu = 1.0 + rowmax;
    sd_rank12_correction(s_q, s_m, gb, mu, n, tid, lane, wave);
    if (tid == 0) a.scal[c * 8 + SC_MU] = mu;
}

__global__ __launch_bounds__(SD_THREADS) void k_sd_project(SdArgs a, int64_t blocks_per_mol)
{
    const int64_t c = blockIdx.x / blocks_per_mol, rb = blockIdx.x % blocks_per_mol;
    if (sd_frozen(a, c)) return;
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const int64_t n = a.n;
    const uint8_t *kind = a.kind + c * a.A;
    const double *gq = a.q + c * SD_Q * n, *gb = a.b + c * SD_Q * n;
    const double mu = a.scal[c * 8 + SC_MU];
    const double *H = a.H + c * n * n;
    double *out = a.projected + c * n * n;
    sd_project_rows(kind, gq, gb, mu, H, nullptr, out, n, rb, lane, wave);
}

__global__ __launch_bounds__(SD_THREADS) void k_sd_step(SdArgs a)
{
    __shared__ double s_g[SD_MAX_N], s_gt[SD_MAX_N], s_lam[SD_MAX_N], s_st[SD_MAX_N];
    __shared__ int s_k;
    __shared__ int s_fail;
    const int64_t c = blockIdx.x;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE;
    const int64_t n = a.n;
    float *ls = a.last_step + c * n;
    if (sd_frozen(a, c)) {
        for (int64_t d = tid; d < n; d += SD_THREADS) ls[d] = 0.f;
        return;
    }
    const uint8_t *kind = a.kind + c * a.A;
    const double *V = a.V + c * n * n, *lam = a.lam + c * n;
    double *mode = a.modes + c * n;
    for (int64_t d = tid; d < SD_MAX_N; d += SD_THREADS) {
        s_g[d] = d < n ? a.gproj[c * n + d] : 0.0;
        s_st[d] = d < n ? mode[d] : 0.0;
        s_lam[d] = d < n ? lam[d] : 0.0;
        s_gt[d] = 0.0;
    }
    __syncthreads();
    // g~_k = V_k . gproj and the overlap V_k . mode: thread k walks down column k
    double ov[SD_MAX_N / SD_THREADS];
#pragma unroll
    for (int m = 0; m < SD_MAX_N / SD_THREADS; ++m) {
        const int64_t k = tid + SD_THREADS * m;
        ov[m] = 0.0;
        if (k >= n) continue;
        double gt = 0.0, o = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            const double v = V[i * n + k];
            gt = fma(v, s_g[i], gt);
            o = fma(v, s_st[i], o);
        }
        s_gt[k] = gt;
        ov[m] = fabs(o);
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < SD_MAX_N / SD_THREADS; ++m) s_st[tid + SD_THREADS * m] = ov[m];
    __syncthreads();

    if (wave == 0) {
        const double mu = a.scal[c * 8 + SC_MU];
        int fail = 0;
        // the followed mode
        int kf = 0;
        if (a.follow) {
            double best = -1.0;
            int idx = 0x7fffffff;
            for (int k = lane; k < (int)n; k += WAVE)
                if (s_lam[k] < 0.5 * mu && s_st[k] > best) best = s_st[k], idx = k;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off);
                const int oi = __shfl_xor(idx, off);
                if (ob > best || (ob == best && oi < idx)) best = ob, idx = oi;
            }
            kf = idx < (int)n ? idx : 0;
        }
        double bad = 0.0, G2 = 0.0, lmin = INFINITY;
        for (int k = lane; k < (int)n; k += WAVE) {
            const double l = s_lam[k], g = s_gt[k];
            if (!(isfinite(l) && isfinite(g))) bad = 1.0;
            if (k != kf && g != 0.0) G2 = fma(g, g, G2), lmin = fmin(lmin, l);
        }
        if (sd_wave_max(bad) > 0.0) fail = ANIHIP_SADDLE_NONFINITE;
        G2 = sd_wave_sum(G2);
        lmin = sd_wave_min(lmin);
        double gm = 0.0;
        if (!fail && G2 > 0.0) {
            // f(x) = x + sum g~_i^2 / (lam_i - x) rises from -inf to +inf (or to f(0) > 0) below hi; f(hi - t) < 0 for t > |g~|
            double hi = fmin(0.0, lmin);
            const double G = sqrt(G2);
            double lo = hi - fmax(1.000001 * G, 1e-15 * fabs(hi) + 1e-300);
            auto secular = [&](double x) {
                double acc = 0.0;
                for (int k = lane; k < (int)n; k += WAVE) {
                    const double g = s_gt[k];
                    if (k != kf && g != 0.0) acc += g * g / (s_lam[k] - x);
                }
                return x + sd_wave_sum(acc);
            };
            if (!(lo < hi) || !(secular(lo) < 0.0)) fail = ANIHIP_SADDLE_NO_BRACKET;
            for (int it = 0; it < 1100 && !fail; ++it) {
                const double mid = 0.5 * (lo + hi);
                if (!(mid > lo && mid < hi)) break;
                if (secular(mid) < 0.0) lo = mid; else hi = mid;
            }
            gm = lo;
        }
        // the step in the eigenbasis, the trust radius, the predicted change
        double s2 = 0.0;
        for (int k = lane; k < (int)n; k += WAVE) {
            const double l = s_lam[k], g = s_gt[k];
            double st = 0.0;
            if (g != 0.0) {
                if (k == kf) {   // lam_k - gp = (lam_k - sqrt(lam_k^2 + 4 g^2)) / 2 < 0, without cancellation for lam_k > 0
                    const double root = sqrt(l * l + 4.0 * g * g);
                    st = -g / (l > 0.0 ? -2.0 * g * g / (l + root) : 0.5 * (l - root));
                } else {
                    st = -g / (l - gm);
                }
            }
            s_st[k] = st;
            s2 = fma(st, st, s2);
        }
        s2 = sd_wave_sum(s2);
        double snorm = sqrt(s2);
        if (!fail && !isfinite(snorm)) fail = ANIHIP_SADDLE_NONFINITE;
        const double radius = a.trust[c];
        const double scale = snorm > radius ? radius / snorm : 1.0;
        double pred = 0.0;
        for (int k = lane; k < (int)n; k += WAVE) {
            const double st = s_st[k] * scale;
            s_st[k] = st;
            pred += s_gt[k] * st + 0.5 * s_lam[k] * st * st;
        }
        pred = sd_wave_sum(pred);
        if (snorm > radius) snorm = radius;
        if (lane == 0) {
            s_k = kf, s_fail = fail;
            a.scal[c * 8 + SC_PRED] = pred, a.scal[c * 8 + SC_SNORM] = snorm;
        }
    }
    __syncthreads();
    if (s_fail) {   // left where it is
        if (tid == 0) a.status[c] |= s_fail;
        for (int64_t d = tid; d < n; d += SD_THREADS) ls[d] = 0.f;
        return;
    }
    const int kf = s_k;
    // s = V s~, one wave per row; the move
    float *x = a.coords + c * n, *xo = a.xold + c * n;
    double *disp = a.disp + c * n;
    for (int64_t i = wave; i < n; i += SD_WAVES) {
        double acc = 0.0;
        for (int64_t k = lane; k < n; k += WAVE) acc = fma(V[i * n + k], s_st[k], acc);
        acc = sd_wave_sum(acc);
        if (lane == 0) {
            const float x0 = x[i];
            const float dr = kind[i / 3] == 1 ? (float)acc : 0.f;
            const float x1 = x0 + dr;
            xo[i] = x0;
            x[i] = x1;
            ls[i] = dr;
            disp[i] = (double)x1 - (double)x0;
        }
    }
    for (int64_t d = tid; d < n; d += SD_THREADS) mode[d] = V[d * n + kf];
    if (tid == 0) a.eigenvalue[c] = s_lam[kf];
}

__global__ __launch_bounds__(SD_THREADS) void k_sd_accept(SdArgs a)
{
    __shared__ double s_s[SD_MAX_N], s_xi[SD_MAX_N];
    const int64_t c = blockIdx.x;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE;
    const int64_t n = a.n;
    double *scal = a.scal + c * 8;
    // everything thread 0 writes further down (status, energies, trust) is read here by every thread, before the barrier
    const bool frozen = sd_frozen(a, c);
    const double e0 = a.energies[c], e1 = a.e_new[c], pred = scal[SC_PRED], snorm = scal[SC_SNORM];
    double radius = a.trust[c];
    __syncthreads();
    if (frozen) {
        if (tid == 0) a.accepted[c] = 0, scal[SC_UPDATE] = 0.0;
        return;
    }
    const uint8_t *kind = a.kind + c * a.A;
    float *x = a.coords + c * n, *f = a.forces + c * n;
    const float *xo = a.xold + c * n, *fn = a.f_new + c * n;
    bool ok = true, counted = true;
    if (!isfinite(e1)) {
        ok = false, counted = false;
    } else if (fabs(pred) >= a.energy_floor && pred != 0.0) {
        const double dev = fabs((e1 - e0) / pred - 1.0);
        if (!(dev <= 1.0)) {
            ok = false;
            radius = fmax(0.25 * radius, a.min_trust);
        } else if (dev < 0.25 && snorm >= 0.99 * radius) {
            radius = fmin(2.0 * radius, a.max_trust);
        } else if (dev > 0.75) {
            radius = fmax(0.5 * radius, a.min_trust);
        }
    }
    if (!ok) {   // restore the coordinates bit for bit; energies and forces still are the old ones
        for (int64_t d = tid; d < n; d += SD_THREADS) x[d] = xo[d];
        if (tid == 0) {
            a.accepted[c] = 0, scal[SC_UPDATE] = 0.0;
            if (counted) a.trust[c] = radius, a.n_rejected[c] += 1;
            else a.status[c] |= ANIHIP_SADDLE_NONFINITE;
        }
        return;
    }
    if (a.bofill) {
        for (int64_t d = tid; d < SD_MAX_N; d += SD_THREADS) s_s[d] = d < n ? a.disp[c * n + d] : 0.0, s_xi[d] = 0.0;
        __syncthreads();
        const double *H = a.H + c * n * n;
        sd_bofill_scalars(kind, H, f, fn, s_s, s_xi, a.xi + c * n, scal + SC_C1, n, tid, lane, wave);
    } else if (tid == 0) {
        scal[SC_UPDATE] = 0.0;
    }
    for (int64_t d = tid; d < n; d += SD_THREADS) f[d] = fn[d];
    if (tid == 0) {
        a.energies[c] = e1;
        a.trust[c] = radius;
        a.accepted[c] = 1;
        a.n_steps[c] += 1;
    }
}

__global__ __launch_bounds__(SD_THREADS) void k_sd_bofill(SdArgs a, int64_t blocks_per_mol)
{
#pragma clang fp contract(off)
    const int64_t c = blockIdx.x / blocks_per_mol, rb = blockIdx.x % blocks_per_mol;
    const double *scal = a.scal + c * 8;
    if (sd_frozen(a, c) || scal[SC_UPDATE] == 0.0) return;
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const int64_t n = a.n;
    const double c1 = scal[SC_C1], c2 = scal[SC_C2], c3 = scal[SC_C3];
    const double *s = a.disp + c * n, *xi = a.xi + c * n;
    double *H = a.H + c * n * n;
    sd_bofill_rows(H, s, xi, c1, c2, c3, n, rb, lane, wave);
}

static int sd_args(const anihip_saddle *state, SdArgs &a, int64_t &C)
{
    ANIHIP_REQUIRE(state, "null pointer argument");
    const anihip_saddle &S = *state;
    ANIHIP_REQUIRE(S.kind && S.coords && S.energies && S.forces && S.hessians && S.trust_radii && S.eigenvalues && S.modes &&
                       S.last_step && S.accepted && S.converged && S.n_steps && S.n_rejected && S.status && S.workspace,
                   "null pointer argument");
    ANIHIP_REQUIRE(S.n_mol >= 1 && S.atoms_per_mol >= 1 && 3 * (int64_t)S.atoms_per_mol <= ANIHIP_SADDLE_MAX_COORDS,
                   "n_mol and atoms_per_mol must be >= 1 and 3 atoms_per_mol <= %d", ANIHIP_SADDLE_MAX_COORDS);
    ANIHIP_REQUIRE(S.fmax >= 0.0 && S.min_trust > 0.0 && S.max_trust >= S.min_trust && S.energy_floor >= 0.0,
                   "fmax and energy_floor must be >= 0 and 0 < min_trust <= max_trust");
    C = S.n_mol;
    const SdLayout L = sd_layout(C, S.atoms_per_mol);
    ANIHIP_REQUIRE(C * ((L.n + SD_ROWS - 1) / SD_ROWS) < ((int64_t)1 << 31), "n_mol x 3 atoms_per_mol / %d must be below 2^31",
                   SD_ROWS);
    ANIHIP_REQUIRE(S.workspace_bytes >= L.total, "workspace holds %zu bytes, %zu needed", S.workspace_bytes, L.total);
    char *ws = (char *)S.workspace;
    a.A = S.atoms_per_mol, a.n = L.n;
    a.periodic = S.periodic != 0, a.follow = S.follow != 0, a.bofill = 0;
    a.fmax = S.fmax, a.max_trust = S.max_trust, a.min_trust = S.min_trust, a.energy_floor = S.energy_floor;
    a.kind = S.kind, a.coords = S.coords, a.energies = S.energies, a.forces = S.forces, a.H = S.hessians;
    a.trust = S.trust_radii, a.eigenvalue = S.eigenvalues, a.modes = S.modes, a.last_step = S.last_step;
    a.accepted = S.accepted, a.converged = S.converged;
    a.n_steps = S.n_steps, a.n_rejected = S.n_rejected, a.status = S.status;
    a.q = (double *)(ws + L.q), a.b = (double *)(ws + L.b), a.gproj = (double *)(ws + L.gproj);
    a.disp = (double *)(ws + L.disp), a.xi = (double *)(ws + L.xi), a.scal = (double *)(ws + L.scal);
    a.xold = (float *)(ws + L.xold);
    a.projected = nullptr, a.lam = nullptr, a.V = nullptr, a.e_new = nullptr, a.f_new = nullptr;
    return 0;
}

}  // namespace anihip

using namespace anihip;

extern "C" size_t anihip_saddle_workspace_bytes(int64_t n_mol, int64_t atoms_per_mol)
{
    if (n_mol < 1 || atoms_per_mol < 1 || 3 * atoms_per_mol > ANIHIP_SADDLE_MAX_COORDS) {
        set_error("n_mol and atoms_per_mol must be >= 1 and 3 atoms_per_mol <= %d", ANIHIP_SADDLE_MAX_COORDS);
        return 0;
    }
    return sd_layout(n_mol, atoms_per_mol).total;
}

extern "C" int anihip_saddle_project(void *stream, const anihip_saddle *state, double *projected)
{
    SdArgs a;
    int64_t C;
    if (int rc = sd_args(state, a, C)) return rc;
    ANIHIP_REQUIRE(projected, "null pointer argument");
    a.projected = projected;
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = (a.n + SD_ROWS - 1) / SD_ROWS;
    hipLaunchKernelGGL(k_sd_basis, dim3((unsigned)C), dim3(SD_THREADS), 0, s, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sd_project, dim3((unsigned)(C * blocks)), dim3(SD_THREADS), 0, s, a, blocks);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_saddle_step(void *stream, const anihip_saddle *state, const double *eigenvalues,
                                  const double *eigenvectors)
{
    SdArgs a;
    int64_t C;
    if (int rc = sd_args(state, a, C)) return rc;
    ANIHIP_REQUIRE(eigenvalues && eigenvectors, "null pointer argument");
    a.lam = eigenvalues, a.V = eigenvectors;
    hipLaunchKernelGGL(k_sd_step, dim3((unsigned)C), dim3(SD_THREADS), 0, (hipStream_t)stream, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int anihip_saddle_accept(void *stream, const anihip_saddle *state, const double *new_energies,
                                    const float *new_forces, int32_t bofill)
{
    SdArgs a;
    int64_t C;
    if (int rc = sd_args(state, a, C)) return rc;
    ANIHIP_REQUIRE(new_energies && new_forces, "null pointer argument");
    a.e_new = new_energies, a.f_new = new_forces, a.bofill = bofill != 0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sd_accept, dim3((unsigned)C), dim3(SD_THREADS), 0, s, a);
    ANIHIP_CHECK_HIP(hipGetLastError());
    if (a.bofill) {
        const int64_t blocks = (a.n + SD_ROWS - 1) / SD_ROWS;
        hipLaunchKernelGGL(k_sd_bofill, dim3((unsigned)(C * blocks)), dim3(SD_THREADS), 0, s, a, blocks);
        ANIHIP_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
