// The direction model of the second-derivative kernels: what a row of k_aev_fwd_gen (JVP), k_aev_bwd2 and k_pair_hvp
// moves along, and the displacement derivative d' of one neighbor entry (d = r_j - r_i, any periodic image) under it.
//
//   Dense   a tangent array t [n_dir][n_atoms][3], one direction per slice (blockIdx.y, or the pair kernel's loop over
//           the directions of a central atom): d' = t_j - t_i.
//   Item    item row q of a block-sparse Hessian: central atom row_atom[q], the implicit unit tangent e_c on atom a
//           (row_dir[q] = 3 a + c), output slab row_dir[q] - dir0: d' = e_c ([j == a] - [i == a]).
//   Strain  strain direction S_ab (3 a + b: item row q of the AEV kernels with row_dir[q] = 3 a + b, or each of the nine
//           directions of a central atom in the pair kernel): every entry moves with its own displacement, d' = d_a e_b,
//           whatever its periodic image.
#pragma once
#include "anihip_common.h"

namespace anihip {

enum class Dir { Dense, Item, Strain };

// the strain mode's outputs: ss [C][9][9], the pair virial [C][9] (or null); molecule = atom / atoms_per_mol
struct StrainAcc {
    double *ss;
    double *virial;
    int64_t atoms_per_mol;
};

// a row: central atom i, output slab, direction 3 a + c (Item: e_c on atom a; Strain: S_ac)
struct DirRow {
    int64_t i, slab;
    int a, c;
};

__device__ __forceinline__ DirRow dir_row(int64_t i, int64_t slab, int r) { return DirRow{i, slab, r / 3, r - 3 * (r / 3)}; }

// item row q (Item, Strain)
__device__ __forceinline__ DirRow dir_item(const int32_t *row_atom, const int32_t *row_dir, int64_t q, int64_t dir0)
{
    const int r = row_dir[q];
    return dir_row((int64_t)row_atom[q], r - dir0, r);
}

// component k of the row's tangent on atom n: Dense the array t (the row's direction slice), Item e_c on atom a
template <Dir M>
__device__ __forceinline__ float dir_tangent(const float *t, const DirRow &row, int64_t n, int k)
{
    if constexpr (M == Dir::Dense) return t[3 * n + k];
    else if constexpr (M == Dir::Item) return n == row.a && k == row.c ? 1.0f : 0.0f;
    else return 0.0f;   // (no tangent array)
}

template <Dir M>
__device__ __forceinline__ float3 dir_tangent3(const float *t, const DirRow &row, int64_t n)
{
    return make_float3(dir_tangent<M>(t, row, n, 0), dir_tangent<M>(t, row, n, 1), dir_tangent<M>(t, row, n, 2));
}

// d' of the entry with displacement d on neighbor j; ti = dir_tangent3(t, row, i) of the central atom i
template <Dir M>
__device__ __forceinline__ float3 dir_dprime(const float *t, const DirRow &row, float3 ti, int64_t j, float3 d)
{
    if constexpr (M == Dir::Strain) {
        const float s = row.a == 0 ? d.x : (row.a == 1 ? d.y : d.z);
        return make_float3(row.c == 0 ? s : 0.f, row.c == 1 ? s : 0.f, row.c == 2 ? s : 0.f);
    } else {
        const float3 tj = dir_tangent3<M>(t, row, j);
        return make_float3(tj.x - ti.x, tj.y - ti.y, tj.z - ti.z);
    }
}

}  // namespace anihip
