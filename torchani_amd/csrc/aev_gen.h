// Shared pieces of the general-grid AEV kernels (aev_generic.hip) and the second-order backward (aev_hess.hip): the grid
// arguments and their host-side validation, the header of a neighbor row, and the pair enumeration of the angular blocks.
#pragma once
#include "anihip_common.h"

namespace anihip {

constexpr int GEN_MAXA = 16, GEN_MAXZ = 16, GEN_MAXR = 32;

struct GenArgs {
    int S, nR, nA, nZ, L, radlen;
    float Rcr, Rca, EtaR, EtaA, Zeta;
    int smooth;
};

struct GenHdr {
    uint32_t start;
    int nA, nF;
    uint64_t pkA, pkF;
};

__device__ __forceinline__ GenHdr gen_hdr(const uint32_t *meta, int64_t i)
{
    const uint32_t *m = meta + (size_t)i * META_W;
    GenHdr h;
    h.start = m[0];
    h.nA = (int)(m[1] & 0xFFFFu);
    h.nF = (int)(m[1] >> 16);
    h.pkA = (uint64_t)m[2] | ((uint64_t)m[3] << 32);
    h.pkF = (uint64_t)m[4] | ((uint64_t)m[5] << 32);
    return h;
}

__device__ __forceinline__ int gen_cnt(uint64_t pk, int t) { return (int)((pk >> (8 * t)) & 255u); }

// (j, k) of the t-th pair of a block: rectangle for two species, row-major upper triangle inside one
__device__ __forceinline__ void gen_pair(bool same, int t, int n1, int n2, int &j, int &k)
{
    if (!same) {
        j = t / n2;
        k = t - j * n2;
    } else {   // t = j (2 n - j - 1) / 2 + (k - j - 1), 0 <= j < k < n
        const float nn = (float)(2 * n1 - 1);
        j = (int)((nn - sqrtf(fmaxf(nn * nn - 8.0f * (float)t, 0.f))) * 0.5f);
        j = max(0, min(j, n1 - 2));
        while (j > 0 && (j * (2 * n1 - j - 1)) / 2 > t) --j;
        while (((j + 1) * (2 * n1 - j - 2)) / 2 <= t) ++j;
        k = j + 1 + (t - (j * (2 * n1 - j - 1)) / 2);
    }
}

__device__ __forceinline__ int gen_triu(int S, int a, int b) { return a * S - (a * (a - 1)) / 2 + (b - a); }

static inline int gen_args(const anihip_aev_params *p, GenArgs *a)
{
    ANIHIP_REQUIRE(p->num_species >= 1 && p->num_species <= MAX_S - 1, "num_species must be 1..7");
    ANIHIP_REQUIRE(p->n_shf_r >= 1 && p->n_shf_r <= GEN_MAXR && p->n_shf_a >= 1 && p->n_shf_a <= GEN_MAXA &&
                       p->n_shf_z >= 1 && p->n_shf_z <= GEN_MAXZ,
                   "symmetry-function grid outside n_shf_r <= 32, n_shf_a <= 16, n_shf_z <= 16 (got %d, %d x %d)",
                   p->n_shf_r, p->n_shf_a, p->n_shf_z);
    a->S = p->num_species;
    a->nR = p->n_shf_r; a->nA = p->n_shf_a; a->nZ = p->n_shf_z;
    a->radlen = a->S * a->nR;
    a->L = a->radlen + (a->S * (a->S + 1) / 2) * a->nA * a->nZ;
    a->Rcr = p->Rcr; a->Rca = p->Rca; a->EtaR = p->EtaR; a->EtaA = p->EtaA; a->Zeta = p->Zeta;
    ANIHIP_REQUIRE(p->cutoff_kind == ANIHIP_CUTOFF_COSINE || p->cutoff_kind == ANIHIP_CUTOFF_SMOOTH,
                   "cutoff_kind must be ANIHIP_CUTOFF_COSINE or ANIHIP_CUTOFF_SMOOTH");
    a->smooth = p->cutoff_kind == ANIHIP_CUTOFF_SMOOTH;
    return 0;
}

}  // namespace anihip
