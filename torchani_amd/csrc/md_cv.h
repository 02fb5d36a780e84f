#pragma once
// The collective variables of include/anihip.h (ANIHIP_MD_CV_*) with their singularity-free gradients, in fp64: shared by the
// bias of the MD kernels (md_bias.hip) and the constraints of the geometry optimizer (geom_constraints.hip).
#include "anihip_common.h"

namespace anihip {

constexpr double CV_PI = 3.14159265358979323846, CV_TWO_PI = 2.0 * CV_PI;

struct Cv {
    int kind, n;
    int32_t at[4];
    double s, g[4][3];
};

// d less `period` times the number of turns that bring d into [-pi, pi): period = 2 pi wraps a difference of dihedrals, period = 0
// leaves d as it is (a loop over columns of mixed kinds selects by the value, without a branch per column)
__device__ __forceinline__ double cv_wrap_by(double d, double period) { return d - period * floor((d + CV_PI) / CV_TWO_PI); }

// a difference of dihedrals brought into [-pi, pi)
__device__ __forceinline__ double cv_wrap(double d) { return cv_wrap_by(d, CV_TWO_PI); }

__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1], c[1] = a[2] * b[0] - a[0] * b[2], c[2] = a[0] * b[1] - a[1] * b[0];
}

// kind and atoms of row r of the tables (kind [N], atoms [N][4]) for entry c of A atoms: false unless the kind is one of the
// three and the atoms are distinct and inside the entry
__device__ __forceinline__ bool cv_load(const int32_t *kind, const int32_t *atoms, int64_t A, int64_t c, int r, Cv &cv)
{
    cv.kind = kind[r];
    if (cv.kind < ANIHIP_MD_CV_DISTANCE || cv.kind > ANIHIP_MD_CV_DIHEDRAL) return false;
    cv.n = cv.kind + 2;
    int bad = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cv.at[k] = k < cv.n ? atoms[4 * (int64_t)r + k] : -1;
        if (k < cv.n && (cv.at[k] < c * A || cv.at[k] >= (c + 1) * A)) bad = 1;
#pragma unroll
        for (int j = 0; j < k; ++j)
            if (k < cv.n && cv.at[j] == cv.at[k]) bad = 1;
    }
    return !bad;
}

// s and its gradient on every atom at the positions x of the CV's atoms (include/anihip.h has the formulas)
__device__ __forceinline__ void cv_eval(const double (&x)[4][3], Cv &cv)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int d = 0; d < 3; ++d) cv.g[k][d] = 0.0;
    }
    if (cv.kind == ANIHIP_MD_CV_DISTANCE) {
        const double d[3] = {x[0][0] - x[1][0], x[0][1] - x[1][1], x[0][2] - x[1][2]};
        cv.s = sqrt(dot3(d, d));
#pragma unroll
        for (int k = 0; k < 3; ++k) cv.g[0][k] = d[k] / cv.s, cv.g[1][k] = -(d[k] / cv.s);
    } else if (cv.kind == ANIHIP_MD_CV_ANGLE) {
        const double u[3] = {x[0][0] - x[1][0], x[0][1] - x[1][1], x[0][2] - x[1][2]};
        const double v[3] = {x[2][0] - x[1][0], x[2][1] - x[1][1], x[2][2] - x[1][2]};
        double n[3], un[3], nv[3];
        cross3(u, v, n);
        const double nn = sqrt(dot3(n, n));
        cv.s = atan2(nn, dot3(u, v));
        cross3(u, n, un);
        cross3(n, v, nv);
        const double fu = dot3(u, u) * nn, fv = dot3(v, v) * nn;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            cv.g[0][k] = un[k] / fu, cv.g[2][k] = nv[k] / fv;
            cv.g[1][k] = -(cv.g[0][k] + cv.g[2][k]);
        }
    } else {
        const double b1[3] = {x[1][0] - x[0][0], x[1][1] - x[0][1], x[1][2] - x[0][2]};
        const double b2[3] = {x[2][0] - x[1][0], x[2][1] - x[1][1], x[2][2] - x[1][2]};
        const double b3[3] = {x[3][0] - x[2][0], x[3][1] - x[2][1], x[3][2] - x[2][2]};
        double n1[3], n2[3];
        cross3(b1, b2, n1);
        cross3(b2, b3, n2);
        const double L2 = dot3(b2, b2), L = sqrt(L2);
        cv.s = atan2(L * dot3(b1, n2), dot3(n1, n2));
        const double fi = -L / dot3(n1, n1), fl = L / dot3(n2, n2), p = dot3(b1, b2) / L2, q = dot3(b3, b2) / L2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double gi = fi * n1[k], gl = fl * n2[k];
            cv.g[0][k] = gi, cv.g[3][k] = gl;
            cv.g[1][k] = q * gl - (1.0 + p) * gi;
            cv.g[2][k] = p * gi - (1.0 + q) * gl;
        }
    }
}

}  // namespace anihip
