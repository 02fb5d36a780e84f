/*
 * anihip.h -- C ABI of libanihip.so, the MI355X (gfx950) ANI hot-path engine.
 *
 * One shared object replaces, for the ANI energy+forces path, the three native plug-ins of the
 * reference (paths relative to /root/reference/torchani/):
 *   cuaev.so      csrc/cuaev.cpp:246-294   (cuaev::run, run_with_half_nbrlist, run_with_full_nbrlist,
 *                                           CuaevComputer::{forward,backward}, csrc/aev.cu:1687-2067)
 *   cell_list.so  csrc/cell_list.cpp:342-363 (cell_list::cell_list)
 *   mnp.so        csrc/mnp.cpp:238-280     (mnp::run, MultiNetFunction fwd / input-grad bwd)
 *
 * Conventions:
 *   - plain C: raw device pointers, explicit sizes, no torch types, no exceptions across the ABI;
 *   - every function returns 0 on success, non-zero on error; anihip_last_error() gives the text
 *     (thread-local), replacing the reference's TORCH_CHECK -> RuntimeError (csrc/aev.cu:1693-1710);
 *   - the CALLER owns all device memory (inputs, outputs, workspaces); the library never allocates,
 *     frees or retains device pointers across calls;
 *   - the library creates no streams or events and keeps no state between calls apart from the thread-local error
 *     text: a second stream a call may use is the caller's, handed over in a descriptor (anihip_mlp_desc.aux_stream);
 *   - every call is asynchronous on the given hipStream_t (passed as void*), never synchronises the
 *     host (the reference syncs >= 3 times per forward, csrc/aev.cu:1292,1763-1767);
 *   - capacity overflows are reported through the device-side `status` words (never assert/trap like
 *     csrc/aev.cu:229); the host wrapper reads them when convenient;
 *   - fp32 compute, int32 indices, fp64 energy accumulation.
 *
 * Atoms are the flattened [C*A] array of the reference's (species[C,A], coords[C,A,3]) pair
 * (aev/_computer.py:193-199); species are element indices 0..S-1, padding = -1 (utils.py:67-74).
 */
#ifndef ANIHIP_H
#define ANIHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANIHIP_ABI_VERSION 13

/* status word bits written by the kernels into status[0] */
#define ANIHIP_ST_ENTRY_OVERFLOW 1u   /* neighbor entries exceeded ent_capacity */
#define ANIHIP_ST_ROW_OVERFLOW 2u     /* one atom has > ANIHIP_MAX_ANG / ANIHIP_MAX_RAD neighbors or > 255 of one species */
#define ANIHIP_ST_GRID_OVERFLOW 4u    /* internal: grid coarsened to fit max_cells (not an error) */
#define ANIHIP_STATUS_WORDS 8         /* status[1] = total neighbor entries, status[2] = #cells, status[3] = #cells that
                                         anihip_nbr_build_cell left to its per-atom kernel (stencil of more than 64 bins
                                         or more candidates than the per-bin kernel stages) */

#define ANIHIP_MAX_SPECIES 8
#define ANIHIP_MAX_ANG 128 /* angular neighbors per atom (cuAEV's analogous bound: csrc/aev.cu:11) */
#define ANIHIP_MAX_RAD 256 /* radial neighbors per atom */
#define ANIHIP_META_WORDS 6 /* uint32 words of per-atom neighbor metadata */

/* Cutoff envelopes: cutoffs.py:74-81 (CutoffCosine, 0.5 cos(pi r / Rc) + 0.5) and cutoffs.py:84-101 (CutoffSmooth,
 * order 2, eps 1e-10: exp(1 - 1 / max(eps, 1 - (r/Rc)^2))); the reference's kernels select them with the
 * use_cos_cutoff template flag (csrc/aev.cu:150-178). */
#define ANIHIP_CUTOFF_COSINE 0
#define ANIHIP_CUTOFF_SMOOTH 1

/* Scalar AEV hyper-parameters; replaces the CuaevComputer constructor arguments
 * (csrc/cuaev.cpp:248: Rcr, Rca, EtaR, ShfR, EtaA, Zeta, ShfA, ShfZ, num_species, use_cos_cutoff). */
typedef struct {
    int32_t num_species; /* S <= 7 */
    int32_t n_shf_r;     /* <= 32.  16 with an 8 x 4 (ANI-2x) or 4 x 8 (ANI-1x) angular grid: the tuned kernels, with slab */
    int32_t n_shf_a;     /* <= 16   masks and the forward-mode derivative; any other grid: the general kernels           */
    int32_t n_shf_z;     /* <= 16   (csrc/aev_generic.hip; cuAEV is templated on these lengths, csrc/aev.cu:1687-1777)    */
    float Rcr, Rca;
    float EtaR, EtaA, Zeta;
    int32_t cutoff_kind; /* ANIHIP_CUTOFF_COSINE | ANIHIP_CUTOFF_SMOOTH (use_cos_cutoff = false) */
    int32_t flags;       /* ANIHIP_AEV_*: written by anihip_aev_table_pack from the shift arrays, zero before that */
} anihip_aev_params;

/* flags: the angular radial shifts ShfA are equally spaced and narrow enough for fp32 exponents -- the forward kernel
 * then evaluates its NA Gaussians per neighbor pair by a three-exponential recurrence instead of NA exponentials. */
#define ANIHIP_AEV_UNIFORM_SHFA 1
/* ShfR AND ShfA are equally spaced and every exponent of the chained Gaussians stays inside fp32's range for distances up to
 * the cutoffs: the backward kernel evaluates its 16 radial Gaussians per neighbor from four of them and its NA angular ones per
 * neighbor pair from one (products with exp2(+-2 D x) instead of exponentials; constants in free slots of the table). */
#define ANIHIP_AEV_REC_BWD 2

/* Length in floats of the device constant table consumed by the AEV kernels, and a host-side packer:
 * table = ShfR[32] | ShfA[16] | cos(ShfZ)[16] | sin(ShfZ)[16]  (trig evaluated in double on the
 * fp32-rounded ShfZ) | q_R ShfR[16] | q_A ShfA[16] | cos/2 [16] | sin/2 [16] with
 * q = sqrt(Eta log2 e)  (exp(-Eta x^2) = exp2(-(q x)^2): the kernels keep distances pre-scaled).  The caller uploads
 * it to the device.  For the 16 / 8 x 4 / 4 x 8 grids, slots those grids leave free carry the constants of the backward
 * kernel's Gaussian recurrences (ANIHIP_AEV_REC_BWD; csrc/anihip_common.h TAB_RECR / TAB_RECA / TAB_RECAK): the upper
 * half of the ShfR block (slots 16-25), the ninth slot of the q_A ShfA block (104), and the upper half of the sin/2
 * block (136-143). */
#define ANIHIP_AEV_TABLE_FLOATS 144
int anihip_aev_table_pack(anihip_aev_params *p /* flags are set */, const float *ShfR, const float *ShfA,
                          const float *ShfZ, float *table_out /* host, ANIHIP_AEV_TABLE_FLOATS */);

const char *anihip_last_error(void);
int anihip_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * Neighbor lists.  Output format (shared by all builders and consumed by the AEV kernels):
 *   meta[i*6 + 0]   = first entry of atom i's row
 *   meta[i*6 + 1]   = nA | (nF << 16): #neighbors with r <= Rca, # with Rca < r <= Rcr
 *   meta[i*6 + 2,3] = 8 x uint8: per-species counts of the nA angular-range neighbors
 *   meta[i*6 + 4,5] = 8 x uint8: per-species counts of the nF far neighbors
 *   ent[row..]      = float4 {dx, dy, dz, bits(j | species_j << 28)}, d = r_j (+ image shift) - r_i,
 *                     angular-range neighbors first, each group ordered by species then by discovery.
 * It is a FULL list (both directions), like cuAEV's internal lists (csrc/aev.cu:975-1039).
 * Only central atoms lo <= i < hi get rows (the data-parallel shard of this rank); all atoms are
 * neighbor candidates.
 */

/* Workspace bytes for anihip_nbr_build_batch / anihip_nbr_build_cell (two-call pattern like
 * csrc/cuaev_cub.cuh:10-17). */
size_t anihip_nbr_workspace_bytes(int64_t n_atoms, int64_t max_cells);

/* Batched molecules, all pairs inside each molecule: replaces pairwiseDistance + postProcessNbrList1
 * (csrc/aev.cu:180-249,975-1039) and neighbors.py:187-275 (all_pairs incl. PBC images).
 * cell: device float[9] (rows = lattice vectors) or NULL; pbc_mask bit k = periodic along vector k.
 * anihip_nbr_build_batch and anihip_nbr_build_cell reset the ANIHIP_STATUS_WORDS status words themselves (their first
 * kernel does); the conversions below (from_half / from_full / refresh) and the AEV calls OR into what they are given. */
int anihip_nbr_build_batch(void *stream, const anihip_aev_params *p, int32_t n_mol, int32_t n_atoms_per_mol,
                           const int32_t *species, const float *coords, const float *cell,
                           int32_t pbc_mask, int64_t lo, int64_t hi, void *workspace,
                           size_t workspace_bytes, uint32_t *meta, float *ent, int64_t ent_capacity,
                           uint32_t *status);

/* One large system through a cell grid (O(N)): replaces cell_list::cell_list
 * (csrc/cell_list.cpp:342-354, neighbors.py:366-507) + postProcessExternalHalfNbrList
 * (csrc/aev.cu:1128-1208).  Without pbc the grid spans the bounding box (neighbors.py:389-394). */
int anihip_nbr_build_cell(void *stream, const anihip_aev_params *p, int64_t n_atoms,
                          const int32_t *species, const float *coords, const float *cell,
                          int32_t pbc_mask, int64_t lo, int64_t hi, int64_t max_cells, void *workspace,
                          size_t workspace_bytes, uint32_t *meta, float *ent, int64_t ent_capacity,
                          uint32_t *status);

/* Rows from an externally supplied HALF neighbor list (LAMMPS / Amber style drivers, the reference's
 * AEVComputer.compute_from_neighbors, aev/_computer.py:251-272, and cuaev::run_with_half_nbrlist ->
 * postProcessExternalHalfNbrList, csrc/cuaev.cpp:205-224, csrc/aev.cu:1128-1208).  Pair p joins the
 * flattened atom indices idx[p] and idx[n_pairs + p] (int64 like Neighbors.indices, neighbors.py:22-29) with
 * diff[p] = r_idx0 - r_idx1 (+ image shift) as produced by narrow_down (neighbors.py:105-112).  Pairs longer
 * than Rcr or touching a padding atom are dropped; every other pair is entered in both rows.  Rows come out
 * in the same format (and a canonical order) as those of the builders above. */
size_t anihip_nbr_half_workspace_bytes(int64_t n_central);
int anihip_nbr_from_half(void *stream, const anihip_aev_params *p, int64_t n_atoms, const int32_t *species,
                         int64_t n_pairs, const int64_t *idx, const float *diff, int64_t lo, int64_t hi,
                         void *workspace, size_t workspace_bytes, uint32_t *meta, float *ent,
                         int64_t ent_capacity, uint32_t *status);

/* The reverse direction: the reference's half-list format from neighbor rows -- what cell_list::cell_list returns
 * (csrc/cell_list.cpp:342-354: idx [2, P] i64, dist [P], diff [P, 3], every pair once; call site neighbors.py:285-294), so
 * that anihip_nbr_build_cell + this call replace torch.ops.cell_list.cell_list for FastCellList / model.neighborlist
 * consumers.  Rows lo..hi emit their pairs with j > i (and one of each +-image pair of an atom with itself), in row order:
 * deterministic.  diff = r_i - r_j (+ image shift), the reference's sign (neighbors.py:105-112).  lo = 0, hi = n_atoms
 * gives the complete list.  idx is [2][capacity]; *n_pairs (device) receives the number of pairs whatever the capacity
 * (call with capacity 0 to size the outputs).  Workspace: anihip_nbr_rows_to_half_workspace_bytes(hi - lo). */
size_t anihip_nbr_rows_to_half_workspace_bytes(int64_t n_central);
int anihip_nbr_rows_to_half(void *stream, int64_t n_atoms, int64_t lo, int64_t hi, const uint32_t *meta, const float *ent,
                            void *workspace, size_t workspace_bytes, int64_t capacity, int64_t *idx, float *dist,
                            float *diff, int64_t *n_pairs /* device */);

/* Rows from an externally supplied FULL neighbor list in the LAMMPS convention (local + ghost atoms, every ghost
 * with its own coordinates; cuaev::run_with_full_nbrlist -> postProcessNbrList2, csrc/cuaev.cpp:226-244,
 * csrc/aev.cu:1048-1126, call site aev/_computer.py:420-438): listed atom ilist[g] has the numneigh[g] neighbors
 * jlist[start[g] .. start[g] + numneigh[g]) (start = exclusive prefix sum of numneigh, int64).  Displacements are
 * r_j - r_i from coords [n_atoms, 3]; neighbors beyond Rcr, padding atoms and j == i are dropped.  Atoms that are
 * not listed get empty rows (zero AEVs).  ent_capacity = n_atoms * row capacity.
 * Indices outside 0 .. n_atoms: a jlist entry is skipped like a neighbor beyond the cutoff (no flag: the row is what it
 * would be without it); an ilist entry sets ANIHIP_ST_ENTRY_OVERFLOW and that list entry is skipped, every other listed
 * atom gets its row.  A neighbor named twice in one atom's list is entered twice.  The rows are NOT symmetric (a ghost
 * has no row): consumers must push (no ANIHIP_BWD_SYMMETRIC, ANIHIP_PAIR_PUSH). */
int anihip_nbr_from_full(void *stream, const anihip_aev_params *p, int64_t n_atoms, const int32_t *species,
                         const float *coords, int64_t n_listed, const int32_t *ilist, const int32_t *numneigh,
                         const int64_t *start, const int32_t *jlist, uint32_t *meta, float *ent,
                         int64_t ent_capacity, uint32_t *status);

/* Verlet-skin reuse (VerletCellList, neighbors.py:759-884): verlet_meta / verlet_ent are rows produced by one of the
 * builders above from coords_build with an ENLARGED radial cutoff (Rcr + skin; the caller passes a copy of the
 * parameters with Rcr raised -- and Rca lowered to ~0 so that all of a row counts against the 256-entry radial
 * limit).  While no atom has moved more than skin / 2 since then, the rows for the current coordinates follow
 * without a pair search: every stored displacement is updated with the motion of its two atoms, screened against
 * the real Rcr of p and re-sorted (the narrow_down step, neighbors.py:64-113).  coords and coords_build must be the
 * same unwrapped trajectory (an atom re-wrapped by a lattice vector in between looks like a large move: rebuild).
 * Rows come out for lo <= i < hi in the standard format; ent_capacity = (hi - lo) * row capacity. */
int anihip_nbr_refresh(void *stream, const anihip_aev_params *p, int64_t n_atoms, int64_t lo, int64_t hi,
                       const int32_t *species, const float *coords, const float *coords_build,
                       const uint32_t *verlet_meta, const float *verlet_ent, uint32_t *meta, float *ent,
                       int64_t ent_capacity, uint32_t *status);

/* ---------------------------------------------------------------------------------------------
 * AEV forward / backward: replace cuRadialAEVs + cuAngularAEVs (csrc/aev.cu:768-834,323-472) and their
 * backward kernels (csrc/aev.cu:837-967,474-766).  aev / grad_aev are [n_atoms, L] row-major with
 * L = S*16 + S(S+1)/2*32, layout [radial | angular] (aev/_computer.py:298).  Rows of atoms outside
 * [lo,hi) are not touched; padding atoms inside the range get zero rows.
 * grad_coords [n_atoms,3] is ACCUMULATED into (caller zeroes it), i.e.
 * grad_coords += d(sum grad_aev * aev)/d coords  (csrc/aev.cu:1958-1984).  The radial part of a pair is finished by
 * each of its two atoms for itself -- atom i gathers the 16-float block grad_aev[j][species(i)*16 ..] of every
 * neighbor row j that this call may read, i.e. lo <= j < hi (and, with slab_mask, flagged there) -- so only the
 * angular part and pairs whose partner row belongs to another shard travel through float atomics.  That needs
 * SYMMETRIC rows (j in row i <=> i in row j), which every builder of this library produces except
 * anihip_nbr_from_full (a LAMMPS list names ghost atoms that have no row of their own): leave ANIHIP_BWD_SYMMETRIC out
 * of `flags` for those rows and every pair term is pushed to its neighbor instead.
 * ANIHIP_BWD_FIXED_POINT: grad_coords is then int64_t[n_atoms][3] (caller zeroes it) in units of 2^-32; contributions are
 * added with 64-bit integer atomics, so the result is bit-identical from run to run whatever the order of the waves
 * (the reference's cuAEV backward is not: float atomics, csrc/aev.cu:700-704).  The caller converts: g = acc * 2^-32.
 *
 * slab_mask (optional, may be NULL; needs ceil(S/2) + S(S+1)/2 <= 32): slab_mask[i] flags the 32-wide
 * "slabs" of row i that can be non-zero -- bit j < ceil(S/2): radial blocks of species 2j, 2j+1; bit
 * ceil(S/2) + P: angular block of species pair P.  An AEV block is identically zero when atom i has no
 * neighbor (pair) of that species inside the cutoff; anihip_mlp_forward_backward skips those slabs.
 * anihip_aev_backward(slab_mask != NULL) reads grad_aev only inside flagged slabs (of the rows lo..hi); with
 * slab_mask == NULL every entry of the rows lo..hi must be valid.
 * Any OTHER grid (n_shf_r <= 32, n_shf_a, n_shf_z <= 16: the general kernels; rows of at most 1024 columns): the flags
 * are those of the PLAIN 32-column slabs of the row -- bit j <=> columns 32 j .. 32 j + 31 can be non-zero (a block of a
 * present species or species pair flags every slab it overlaps) -- which is the order anihip_mlp_pack gives the layer-0
 * planes of such networks (aev_radial_len = 0).  The general backward reads only blocks of present species and takes
 * no flags.  anihip_aev_jvp serves every grid as well (ABI 9). */
#define ANIHIP_BWD_SYMMETRIC 1   /* rows are symmetric: gather the radial partner blocks instead of pushing */
#define ANIHIP_BWD_FIXED_POINT 2 /* grad_coords is an int64 fixed-point accumulator (2^-32): reproducible sums */
int anihip_aev_forward(void *stream, const anihip_aev_params *p, const float *table, int64_t n_atoms,
                       int64_t lo, int64_t hi, const int32_t *species, const uint32_t *meta,
                       const float *ent, float *aev, uint32_t *slab_mask, uint32_t *status);
/* The same rows UPDATED IN PLACE (ABI 9; the 16 / 8x4 / 4x8 grids): aev is the buffer of the previous call (any system
 * of the same n_atoms -- which atom a row described does not matter), prev_mask[i] = the slabs of row i that may hold
 * non-zero data (the slab_mask that call wrote; the caller alternates between two flag buffers: prev_mask is only read,
 * slab_mask only written, they must not be the same buffer).  Only those slabs and the ones flagged now are written: an atom of a water box flags
 * 4-5 of its 32 slabs step after step, so an MD loop writes 0.6 KB of each 4 KB row instead of all of it (the rest is
 * zeros nobody has to write again).  The rows are complete afterwards, exactly as anihip_aev_forward leaves them.
 * First use: aev zero-filled, prev_mask zero-filled (or: aev anything, prev_mask all ones).  No reference counterpart
 * (csrc/aev.cu:1732 allocates and zero-fills a fresh tensor per call). */
int anihip_aev_forward_update(void *stream, const anihip_aev_params *p, const float *table, int64_t n_atoms,
                              int64_t lo, int64_t hi, const int32_t *species, const uint32_t *meta,
                              const float *ent, float *aev, const uint32_t *prev_mask, uint32_t *slab_mask,
                              uint32_t *status);
int anihip_aev_backward(void *stream, const anihip_aev_params *p, const float *table, int64_t n_atoms,
                        int64_t lo, int64_t hi, const int32_t *species, const uint32_t *meta,
                        const float *ent, const float *grad_aev, const uint32_t *slab_mask, int32_t flags,
                        float *grad_coords, uint32_t *status);

/* Forward-mode derivative of the AEV rows along a coordinate-space direction: daev[i] = sum_k (d aev[i] / d r_k) .
 * tangent[k]  (tangent: [n_atoms][3]).  This is the reference's cuaev double backward (csrc/aev.cu:1986-2015,
 * cuaev_double_backward, with the is_double_backward kernel variants :474-766,837-967): training on forces
 * differentiates grad_coords = J^T grad_aev with respect to grad_aev, and the gradient arriving at the forces is the
 * direction.  Rows lo <= i < hi of daev are written (rows of padding atoms zeroed). */
int anihip_aev_jvp(void *stream, const anihip_aev_params *p, const float *table, int64_t n_atoms, int64_t lo,
                   int64_t hi, const int32_t *species, const uint32_t *meta, const float *ent,
                   const float *tangent, float *daev, uint32_t *status);

/* anihip_aev_jvp for n_dir directions in one launch (direction = a grid dimension): tangent [n_dir][n_atoms][3] ->
 * daev [n_dir][n_atoms][L], rows lo <= i < hi of every direction written.  Same grids and kernels as anihip_aev_jvp.
 * n_dir <= 65535. */
int anihip_aev_jvp_batched(void *stream, const anihip_aev_params *p, const float *table, int64_t n_atoms, int64_t lo,
                           int64_t hi, const int32_t *species, const uint32_t *meta, const float *ent, int64_t n_dir,
                           const float *tangent, float *daev, uint32_t *status);

/* Second-order AEV backward, for Hessians with respect to the coordinates: for n_dir directions t[k],
 *   out[k] += J^T dgrad[k] + (D_{t[k]} J^T) grad_aev
 * (J = d aev / d coords over the central atoms lo <= i < hi; D_t J^T = the derivative of the backward along the motion t with
 * grad_aev held fixed).  grad_aev [n_atoms][L], dgrad [n_dir][n_atoms][L], tangent [n_dir][n_atoms][3], out [n_dir][n_atoms][3]
 * (accumulated with float atomics: not bit-reproducible).  An entry's displacement moves with t_j - t_i whatever its periodic
 * image.  Any grid of the general kernels (the tuned ones included), both cutoff functions; symmetric rows (the library's
 * builders).  n_dir <= 65535. */
int anihip_aev_backward_second(void *stream, const anihip_aev_params *p, const float *table, int64_t n_atoms, int64_t lo,
                               int64_t hi, const int32_t *species, const uint32_t *meta, const float *ent,
                               const float *grad_aev, int64_t n_dir, const float *tangent, const float *dgrad, float *out,
                               uint32_t *status);

/* ---------------------------------------------------------------------------------------------
 * Block-sparse Hessians (grad.energies_forces_and_sparse_hessians).  The AEV of atom i depends on R(i) = {i} U its row
 * (periodic images folded onto atom indices), so d^2 E / d r_a d r_j is non-zero only for j in P(a) = U_{i in R(a)} R(i).
 * A unit direction (atom a, component c) is worked as ITEM ROWS (direction 3 a + c, central atom i) for i in R(a): the
 * tangent e_c on atom a is implicit; row_dir[q] = 3 a + c (flattened atom index a), row_atom[q] = i.  Symmetric rows only.
 *
 * R lists, two calls: roff NULL -> rcnt[a] = |R(a)| (0 for padding); then, with roff [n_atoms + 1] = the exclusive scan of
 * rcnt, rlist[roff[a] ..] = a followed by the other atoms of R(a) (each once). */
int anihip_hess_sparse_rlist(void *stream, int64_t n_atoms, const int32_t *species, const uint32_t *meta, const float *ent,
                             const int64_t *roff, int32_t *rcnt, int32_t *rlist);

/* The block pattern, two calls: poff NULL -> pcnt[a] = |P(a)|; then, with poff [n_atoms + 1] the exclusive scan of pcnt and
 * nnz = poff[n_atoms], index (int64 [2][nnz]) gets the pattern BY COLUMNS: for p in poff[a] .. poff[a + 1],
 * index[1][p] = a and index[0][p] runs over P(a) ascending.  The pattern is symmetric.  |P(a)| above 4096 (far beyond
 * rows of ANIHIP_MAX_RAD entries) sets bit 0 of *status. */
int anihip_hess_sparse_pattern(void *stream, int64_t n_atoms, const int64_t *roff, const int32_t *rlist, const int64_t *poff,
                               int64_t nnz, int32_t *pcnt, int64_t *index, uint32_t *status);

/* The item rows of the direction atoms n0 <= a < n1: 3 sum_a |R(a)| rows written to row_atom / row_dir, the items (a, i)
 * ordered by the species of i (rows of a species contiguous, species ascending), three rows (c = 0, 1, 2) per item.
 * scratch: num_species (n1 - n0) + 1 ints.  One launch, one block. */
int anihip_hess_sparse_items(void *stream, int32_t num_species, int64_t n0, int64_t n1, const int32_t *species,
                             const int64_t *roff, const int32_t *rlist, int32_t *scratch, int32_t *row_atom, int32_t *row_dir);

/* anihip_aev_jvp over item rows: daev [n_rows][L], row q = d aev_{row_atom[q]} along the unit tangent of row_dir[q].  Every
 * grid through the general kernel (the tuned grids included), both cutoff functions. */
int anihip_aev_jvp_items(void *stream, const anihip_aev_params *p, const float *table, int64_t n_atoms,
                         const int32_t *species, const uint32_t *meta, const float *ent, int64_t n_rows,
                         const int32_t *row_atom, const int32_t *row_dir, float *daev);

/* anihip_aev_backward_second over item rows: out[row_dir[q] - dir0] += J_i^T dgrad[q] + (D_t J_i^T) grad_aev for the central
 * atom i = row_atom[q] and the unit tangent t of row_dir[q]; dgrad [n_rows][L], out [n_dir][n_atoms][3] (float atomics);
 * rows whose slab falls outside 0 .. n_dir are skipped. */
int anihip_aev_backward_second_items(void *stream, const anihip_aev_params *p, const float *table, int64_t n_atoms,
                                     const int32_t *species, const uint32_t *meta, const float *ent, const float *grad_aev,
                                     int64_t n_rows, const int32_t *row_atom, const int32_t *row_dir, int64_t dir0,
                                     int64_t n_dir, const float *dgrad, float *out);

/* Pattern blocks of the entries p0 <= p < p1 (the columns of a chunk's direction atoms) out of the scratch
 * [n_dir][n_atoms][3] whose slab 3 a + c - dir0 holds column (a, c) of H:  blocks[p][y][c] = scratch[3 a + c - dir0][j][y]
 * for j = index[0][p], a = index[1][p]; those scratch positions are written back to zero (the caller zeroes the scratch
 * once, never per chunk). */
int anihip_hess_sparse_extract(void *stream, int64_t n_atoms, int64_t p0, int64_t p1, const int64_t *index, int64_t nnz,
                               int64_t dir0, int64_t n_dir, float *scratch, float *blocks);

/* ---------------------------------------------------------------------------------------------
 * Strain second derivatives (grad.energies_forces_and_strain_hessians).  Coordinates are row vectors; the system is strained
 * by a 3 x 3 matrix S as x -> x S, cell -> cell S, so every pair displacement d (any periodic image) becomes d S.  At S = I,
 * for strain direction k = 3 a + b the tangent of every entry is d' = d_a e_b (it replaces t_j - t_i of a coordinate
 * direction), and
 *   strain_hessians[c][a][b][p][q] = d^2 E_c / d S_ab d S_pq = sum over the rows of molecule c and their pairs of
 *                                    d_a ((d E_i / d d)')_b along the tangent of (p, q),
 *   internal_strain[c][i][y][a][b] = d^2 E_c / d x_iy d S_ab = K_k[i][y] + delta_ya (d E / d x_i)_b,
 * where K_k = J^T (H_net J d') + (D_d' J^T) g is the mixed derivative with the displacements taken in the strained frame
 * (what these entry points scatter); the force term is the caller's.  Strain item rows: row_dir[q] = k in 0 .. 8, row_atom[q] =
 * the central atom i.  ss is double [n_atoms / atoms_per_mol][9][9] (ss[c][3 a + b][3 p + q]), accumulated with fp64
 * atomics; out is float [9][n_atoms][3].  Symmetric rows only.
 *
 * anihip_aev_jvp over strain item rows: daev [n_rows][L], row q = d aev_{row_atom[q]} / d S_k.  Every grid through the
 * general kernel, both cutoff functions. */
int anihip_aev_jvp_strain_items(void *stream, const anihip_aev_params *p, const float *table, int64_t n_atoms,
                                const int32_t *species, const uint32_t *meta, const float *ent, int64_t n_rows,
                                const int32_t *row_atom, const int32_t *row_dir, float *daev);

/* anihip_aev_backward_second over strain item rows: out[k][.] += K_k of the central atom i = row_atom[q] (float atomics, as
 * the item rows of block-sparse Hessians), dgrad [n_rows][L] = H_net J d' of the row; and
 * ss[i / atoms_per_mol][3 x + y][k] += sum_e d_{e,x} ((d E_i / d d_e)')_y (one fp64 atomic per component and row).  Rows with
 * row_dir outside 0 .. 8 are skipped.  atoms_per_mol divides n_atoms. */
int anihip_aev_backward_second_strain_items(void *stream, const anihip_aev_params *p, const float *table, int64_t n_atoms,
                                            int64_t atoms_per_mol, const int32_t *species, const uint32_t *meta,
                                            const float *ent, const float *grad_aev, int64_t n_rows, const int32_t *row_atom,
                                            const int32_t *row_dir, const float *dgrad, float *out, double *ss);

/* anihip_pair_analytic_hvp along the 9 strain directions, over the central atoms lo <= i < hi (same kind, rows, tables,
 * cutoff and flags as anihip_pair_analytic):  out[k][i] += -sum_j B_ij d'_ij  (B = d^2 e / d d^2 of the pair; no atomics),
 * ss[mol][3 x + y][3 p + q] += sum_pairs d_x (B d'_pq)_y / 2 (each row owns half of each of its pairs), and, when virial is
 * not NULL, virial[mol][3 x + y] += sum_pairs (d e / d d)_y d_x / 2 = d E / d S_xy; mol = i / atoms_per_mol.  A periodic
 * image of atom i itself does contribute here.  Symmetric rows only. */
int anihip_pair_analytic_hvp_strain(void *stream, int32_t kind, int64_t n_atoms, int64_t atoms_per_mol, int64_t lo,
                                    int64_t hi, const int32_t *species, const uint32_t *meta, const float *ent,
                                    const float *pair_table, const float *extra, float cutoff, int32_t cutoff_kind,
                                    int32_t flags, float *out, double *ss, double *virial);

/* Lowest normal modes of block-sparse Hessians (grad.sparse_vibrational_analysis): the operator
 *   A = M^-1/2 ((H + H^T) / 2) M^-1/2
 * of a tuples.BlockHessian in a layout of its own (csrc/hess_modes.hip).
 *
 * anihip_block_hessian_prepare, once per call.  index int64 [2][nnz] BY COLUMNS (index[1] non-decreasing, index[0] strictly
 * ascending inside a column), blocks fp32 [nnz][3][3] (blocks[p][x][y] = d^2 E / d r_{index[0][p], x} d r_{index[1][p], y}),
 * masses fp64 [n_atoms] (amu; read only for atoms that hold blocks).  Writes coff int64 [n_atoms + 1] (the entries of column
 * a are coff[a] .. coff[a + 1]), rows int32 [nnz] = index[0], partner int64 [nnz] (the entry of the transposed block),
 * ablocks fp32 [nnz][3][3] = (B_ja + B_aj^T) / (2 sqrt(m_j m_a)) for the entry p = (row j, column a), diag int64 [n_atoms]
 * (the entry of atom a's diagonal block, -1 if it has none: a padding atom) and gersh fp64 [n_atoms] (the largest of the
 * Gershgorin row sums sum_{j, y} |A_{(a x), (j y)}| of atom a's three rows).  *status (zeroed by the caller) gets
 * ANIHIP_BLOCK_HESSIAN_BAD_INDEX for an index out of 0 .. n_atoms or not sorted by columns, ANIHIP_BLOCK_HESSIAN_NO_PARTNER
 * for a block whose transpose is not stored and ANIHIP_BLOCK_HESSIAN_NO_DIAGONAL for an atom with blocks but no diagonal
 * block; the affected outputs are zero.  The index is not read by anihip_block_hessian_spmm.
 *
 * anihip_block_hessian_spmm: y = A x for m vectors, 1 <= m <= ANIHIP_BLOCK_HESSIAN_MAX_VECTORS; x, y fp32 [n_atoms][3][m]
 * (vector index fastest), y OVERWRITTEN (rows of atoms without blocks are zero).  Row a of y is a sum over column a's blocks
 * (A is symmetric) in fp64, written once: no atomics, bit-identical run to run. */
#define ANIHIP_BLOCK_HESSIAN_MAX_VECTORS 64
#define ANIHIP_BLOCK_HESSIAN_BAD_INDEX 1u
#define ANIHIP_BLOCK_HESSIAN_NO_PARTNER 2u
#define ANIHIP_BLOCK_HESSIAN_NO_DIAGONAL 4u
int anihip_block_hessian_prepare(void *stream, int64_t n_atoms, int64_t nnz, const int64_t *index, const float *blocks,
                                 const double *masses, int64_t *coff, int32_t *rows, int64_t *partner, float *ablocks,
                                 double *gersh, int64_t *diag, uint32_t *status);
int anihip_block_hessian_spmm(void *stream, int64_t n_atoms, int32_t m, const int64_t *coff, const int32_t *rows,
                              const float *ablocks, const float *x, float *y);

/* Phonons from the block-sparse Hessian of a supercell (csrc/phonons.hip, torchani_amd/phonons.py).  The supercell is
 * r1 x r2 x r3 copies of a primitive cell of n_basis atoms in cell-major order: atom ((l1 r2 + l2) r3 + l3) n_basis + b.
 * All three functions compute in fp64, write every output element once without atomics (two calls give the same bits) and
 * read nothing on the host.
 *
 * anihip_phonon_fold: the compact force constants.  coff, rows, ablocks are the outputs of anihip_block_hessian_prepare
 * called with unit masses.  Compact entry e < m is (ent_b[e], ent_j[e]): basis atom b and the supercell atom j of a block of
 * the home cell's column of b, i.e. the pair (b; b' = j mod n_basis, cell of j).  phi fp64 [m][3][3] gets
 * phi[e][x][y] = mean over the r1 r2 r3 translations t (t3 fastest, summed in that order) of the symmetrized block
 * d^2 E / d r_(b, t) x  d r_(b', cell of j + t mod repeats) y, each found by a binary search in its column's sorted rows;
 * missing int32 [m] counts the translations whose block is not stored (they count as zero), defect fp64 [m] is the
 * largest |block - mean| over translations and components.  An entry with ent_b or ent_j out of range gets zeros and
 * missing = r1 r2 r3.  With boff int32 [n_basis + 1] (the entries of basis atom b are boff[b] .. boff[b + 1]) and diag_entry
 * int32 [n_basis] (the entry (b; b, 0), -1: none) a second launch imposes the acoustic sum rule:
 * phi[diag_entry[b]] = -(S + S^T) / 2, S the sum of b's other entries.  Both NULL: no sum rule.
 *
 * anihip_phonon_dynmat: D(q)_(3b+x),(3b'+y) = (m_b m_b')^-1/2 sum_e phi[e][x][y] exp(2 pi i q . nvec[e]) over the entries of
 * (b, b'), which must be contiguous: poff int32 [n_basis^2 + 1] holds the run of pair b n_basis + b'.  q fp64 [n_q][3] in
 * fractional reciprocal coordinates, nvec int32 [m][3] the lattice vector of each entry, masses fp64 [n_basis] (amu).  dmat:
 * n_q x 3 n_basis x 3 n_basis complex numbers as interleaved (re, im) fp64 pairs.  dderiv (may be NULL), [n_q][3] such
 * matrices: the derivatives with respect to the Cartesian wave vector (rad / Angstrom), each term times i rvec[e][a],
 * rvec fp64 [m][3] = nvec times the primitive lattice (Angstrom).  The phase is sincospi(2 frac(q . nvec)).
 *
 * anihip_phonon_dos: dos[k] = sum_i weights[i] G_sigma(f_first + k df - freqs[i]), k < bins, G_sigma the unit-area Gaussian;
 * freqs, weights fp64 [n_modes]. */
int anihip_phonon_fold(void *stream, int32_t n_basis, int32_t r1, int32_t r2, int32_t r3, const int64_t *coff,
                       const int32_t *rows, const float *ablocks, int32_t m, const int32_t *ent_b, const int32_t *ent_j,
                       const int32_t *boff, const int32_t *diag_entry, double *phi, int32_t *missing, double *defect);
int anihip_phonon_dynmat(void *stream, int32_t n_basis, int64_t n_q, const int32_t *poff, const int32_t *nvec,
                         const double *phi, const double *rvec, const double *masses, const double *q, double *dmat,
                         double *dderiv);
int anihip_phonon_dos(void *stream, int64_t n_modes, const double *freqs, const double *weights, double f_first, double df,
                      double sigma, int32_t bins, double *dos);

/* L-BFGS geometry optimization of a batch of molecules (torchani_amd.geomopt, csrc/lbfgs.hip): one step of ASE's LBFGS
 * without line search for every molecule c of [n_mol][atoms_per_mol] that has not converged.  active uint8 [C][A] (0: padding
 * or fixed atom: its force is taken as zero, it never moves), coords fp32 [C][A][3] (x_k, moved IN PLACE to x_k+1), forces
 * fp32 [C][A][3] (f_k at coords).  Per molecule:  converged[c] |= max_i |f_i| < fmax, and a converged molecule is left
 * untouched (last_step zero, n_steps unchanged); else the pair (x_k - x_k-1, f_k-1 - f_k) is stored if its curvature s.y
 * (fp64) is positive, the oldest pair dropped beyond `memory`, p = -H f-gradient with H0 = inv_alpha I, scaled to the
 * longest atom step maxstep, and x_k+1 = x_k + damping p; last_step fp32 [C][A][3] = the displacement applied,
 * n_steps[c] += 1.  workspace: anihip_lbfgs_workspace_bytes(n_mol, atoms_per_mol, memory) bytes, ZERO-FILLED before the
 * first step and kept between steps (it holds the history); converged uint8 [C] and n_steps int32 [C] are caller state
 * too.  Four launches, whatever memory, n_mol and atoms_per_mol; no atomics: bit-identical run to run. */
#define ANIHIP_LBFGS_MAX_MEMORY 256
typedef struct {
    int32_t n_mol, atoms_per_mol;
    int32_t memory;   /* stored pairs, 1 .. ANIHIP_LBFGS_MAX_MEMORY */
    int32_t flags;    /* 0 */
    double inv_alpha; /* H0 = inv_alpha I (Angstrom^2 / Hartree) */
    double maxstep;   /* Angstrom */
    double damping;
    double fmax;      /* Hartree / Angstrom */
} anihip_lbfgs_params;
size_t anihip_lbfgs_workspace_bytes(int64_t n_mol, int64_t atoms_per_mol, int32_t memory);   /* 0 + anihip_last_error() */
int anihip_lbfgs_step(void *stream, const anihip_lbfgs_params *params, const uint8_t *active, float *coords,
                      const float *forces, void *workspace, size_t workspace_bytes, float *last_step, uint8_t *converged,
                      int32_t *n_steps);

/* Molecular dynamics of a batch of molecules (torchani_amd.md.BatchedDynamics, csrc/md.hip): velocity Verlet (NVE) and
 * Langevin dynamics in the BAOAB splitting, layout [n_mol][atoms_per_mol] = [C][A].  Units: Angstrom, fs, amu, Hartree;
 * ANIHIP_MD_ACC_UNIT = (Hartree / Angstrom) / amu in Angstrom / fs^2.  A step of the caller is anihip_md_drift, the forces at
 * the new coordinates, anihip_md_kick.  active uint8 [C][A]: 0 = a padding or fixed atom, which never moves and whose velocity
 * is set to zero; 1 = a free atom; 2 (ANIHIP_MD_ATOM_CLUSTER) = an atom owned by a cluster of bond-length constraints (below),
 * which drift and the kick of anihip_md_kick leave alone and the sums count.  One thread per atom, no atomics, every sum in
 * a fixed order: bit-identical run to run.
 *
 * anihip_md_drift, per active atom:  v += dt/2 f inv_mass;  NVE: x += dt v;  Langevin (flags & ANIHIP_MD_LANGEVIN):
 * x += dt/2 v,  v = c1 v + sqrt(kT_c (1 - c1^2) inv_mass) xi,  x += dt/2 v,  c1 = exp(-friction_c dt).  inv_mass fp32 [C][A] =
 * ANIHIP_MD_ACC_UNIT / m (m in amu), kT fp32 [C] = k_B T_c in HARTREE (so kT inv_mass is a velocity squared), friction fp32 [C]
 * in 1 / fs; both may be NULL for NVE.  The position of an atom is the pair coords + coords_lo (fp32 [C][A][3] each; the
 * caller zero-fills coords_lo once): every `x +=` is a two-sum, after which coords -- what the engine reads -- is the fp32
 * nearest to the pair.  velocities fp32 [C][A][3] (Angstrom / fs), forces fp32 [C][A][3] (Hartree / Angstrom).
 *
 * Noise: xi = anihip_md_noise(seed, step, ...), a pure function of (seed, step, replica id, atom index within the molecule).
 * Philox4x32-10 with key (seed low, seed high) and counter (atom index, replica_ids[c] -- int64 [C], values below 2^32 -- or
 * c when NULL, step low, step high) gives u0..u3; with p(u) = ((u >> 9) + 0.5) 2^-23:
 *   xi_x = sqrt(-2 ln p(u0)) cos(2 pi p(u1)),  xi_y = sqrt(-2 ln p(u0)) sin(2 pi p(u1)),  xi_z = sqrt(-2 ln p(u2)) cos(2 pi p(u3)).
 * The caller advances `step` by one per drift.  anihip_md_noise writes out fp32 [C][A][3] for every atom, active or not.
 *
 * anihip_md_kick: v += dt/2 f ANIHIP_MD_ACC_UNIT / mass (mass fp32 [C][A], amu), then kinetic[c] (fp64, Hartree) =
 * 1/2 sum m v^2 / ANIHIP_MD_ACC_UNIT over the active atoms.  anihip_md_remove_drift: v -= sum m v / sum m over the active atoms
 * of each molecule.  Both sum per 256-atom chunk and, for molecules of more than one chunk, per molecule in a second launch;
 * workspace: anihip_md_workspace_bytes(n_mol, atoms_per_mol) bytes of scratch, no state.  Launches: drift 1, kick 1 or 2,
 * remove_drift 2 or 3, noise 1. */
#define ANIHIP_MD_ACC_UNIT 0.26254996403871417
#define ANIHIP_MD_LANGEVIN 1
typedef struct {
    int32_t n_mol, atoms_per_mol;
    int32_t flags;      /* ANIHIP_MD_LANGEVIN or 0 (NVE) */
    int32_t reserved;   /* 0 */
    double dt;          /* fs, > 0 */
    uint64_t seed;      /* Philox key */
    uint64_t step;      /* Philox counter words 2 and 3 */
} anihip_md_params;
size_t anihip_md_workspace_bytes(int64_t n_mol, int64_t atoms_per_mol);   /* 0 + anihip_last_error() */
int anihip_md_drift(void *stream, const anihip_md_params *params, const uint8_t *active, const float *inv_mass,
                    const float *kT, const float *friction, const int64_t *replica_ids, float *coords, float *coords_lo,
                    float *velocities, const float *forces);
int anihip_md_kick(void *stream, const anihip_md_params *params, const uint8_t *active, const float *mass, float *velocities,
                   const float *forces, double *kinetic, void *workspace, size_t workspace_bytes);
int anihip_md_remove_drift(void *stream, const anihip_md_params *params, const uint8_t *active, const float *mass,
                           float *velocities, void *workspace, size_t workspace_bytes);
int anihip_md_noise(void *stream, uint64_t seed, uint64_t step, int64_t n_mol, int64_t atoms_per_mol,
                    const int64_t *replica_ids, float *out);

/* Bond-length constraints (SHAKE / RATTLE) of the integrator above.  A constraint k holds |x_i - x_j| = d_k for two atoms of
 * one molecule; the difference is the plain one of the unwrapped coordinates, no minimum image is taken.  Constraints that
 * share atoms form a cluster, a connected component of the constraint graph, of at most ANIHIP_MD_CLUSTER_ATOMS atoms and
 * ANIHIP_MD_CLUSTER_BONDS constraints (X-H stars, rigid three-site waters, short chains).  There are no angle constraints and
 * no SETTLE.  w_i = inv_mass_i for an active atom and 0 for a fixed atom, which may anchor a constraint; a constraint between
 * two atoms of w = 0 or on a padding atom is the caller's error.  Two operations, per cluster in fp64 on x = coords + coords_lo
 * read exactly:
 *   project_v(x, v): the v' = v - W J^T mu with r_ij . (v'_i - v'_j) = 0 for every constraint (r_ij = x_i - x_j; RATTLE's
 *     velocity stage), a projector at fixed x.  Gauss-Seidel over the constraints in their stored order, mu_k = r.dv /
 *     ((w_i + w_j) r.r); a constraint is converged at |r.dv| <= tolerance d_k v_scale, v_scale = the largest |v| component
 *     of the cluster's atoms when the projection starts.
 *   move(x, v, h): x' = x + h v + W J(x)^T lambda with |x'_i - x'_j| = d_k, the correction directions r_ij taken at the START
 *     of the move (SHAKE); then v' = (x' - x) / h.  Gauss-Seidel, lambda_k = (|s|^2 - d_k^2) / (2 (w_i + w_j) s.r) with
 *     s = x'_i - x'_j; a constraint is converged at | |s|^2 - d_k^2 | <= 2 tolerance d_k^2.
 * An iteration count is the number of sweeps that corrected a constraint, at most max_iterations; a cluster that reaches
 * max_iterations has not converged.  The step is geodesic BAOAB with one RATTLE per sub-step (Leimkuhler and Matthews 2016,
 * K_r = 1), the projections that a later one at the same x makes redundant left out (move(x, v, h) = move(x, project_v(x, v), h)):
 *   anihip_md_constrain_drift:   B v += dt/2 f w;  NVE move(dt);  Langevin move(dt/2), O v = c1 v + sqrt(kT (1 - c1^2) w) xi,
 *     move(dt/2), with c1 and xi those of anihip_md_drift at the atom's own index, all in fp64; writes coords = (float)x,
 *     coords_lo = (float)(x - coords), the fp32 velocities and iterations[q][0] (the larger count of the two moves).
 *   anihip_md_constrain_kick:    B, project_v; writes the velocities and iterations[q][1].  It runs BEFORE anihip_md_kick, which
 *     adds the kinetic energy of the projected velocities.
 *   anihip_md_project_velocities: project_v alone; writes the velocities and iterations[q][1].
 * All three touch only the atoms of clusters with w != 0 (marked 2 in `active`); one thread per cluster, the cluster staged
 * in LDS, no atomics, one launch each.  A cluster whose table entries are out of range moves nothing and reports
 * max_iterations.  Tables (device memory, built once by the caller, Q = n_clusters):
 *   atoms int32 [Q][8]      global atom index c A + i of each slot (one molecule per cluster), slots past count[q][0] unused
 *   count int32 [Q][2]      atoms (2..8) and constraints (1..12) of the cluster
 *   bonds uint8 [Q][12][2]  the slots (a, b) of each constraint
 *   d2    fp64  [Q][12]     d_k^2, Angstrom^2
 *   w     fp64  [Q][8]      w of each slot (ANIHIP_MD_ACC_UNIT / m, 0 for a fixed atom)
 *   iterations int32 [Q][2] OUT: position and velocity iteration counts of the last call that wrote them
 * Two kernel instances: tables whose largest cluster has at most 4 atoms and 4 constraints (max_atoms, max_bonds below) run one
 * with 24 KB of LDS per 64 clusters, any other the 8 / 12 instance with 52 KB.  Measured on one MI355X at tolerance 1e-8
 * (profiles/md_constraints_bench.txt): 778 688 rigid waters add 0.59 ms to a 31.7 ms Langevin step (19 position and 29
 * velocity sweeps per cluster at dt 0.5 fs, 24 and 31 at 2 fs); 524 clusters of X-H bonds add 0.06 ms to a 0.24 ms step (2 sweeps). */
#define ANIHIP_MD_ATOM_CLUSTER 2
#define ANIHIP_MD_CLUSTER_ATOMS 8
#define ANIHIP_MD_CLUSTER_BONDS 12
typedef struct {
    int64_t n_clusters;
    const int32_t *atoms, *count;
    const uint8_t *bonds;
    const double *d2, *w;
    int32_t *iterations;
    double tolerance;         /* > 0 */
    int32_t max_iterations;   /* >= 1 */
    int32_t max_atoms, max_bonds;   /* the largest count[q][0] and count[q][1] of the tables, or 0, 0 if not known: tables of
                                       clusters of at most 4 atoms and 4 constraints run a kernel instance with less LDS */
    int32_t reserved;         /* 0 */
} anihip_md_clusters;
int anihip_md_constrain_drift(void *stream, const anihip_md_params *params, const anihip_md_clusters *clusters,
                              const float *kT, const float *friction, const int64_t *replica_ids, float *coords,
                              float *coords_lo, float *velocities, const float *forces);
int anihip_md_constrain_kick(void *stream, const anihip_md_params *params, const anihip_md_clusters *clusters,
                             const float *coords, const float *coords_lo, float *velocities, const float *forces);
int anihip_md_project_velocities(void *stream, const anihip_md_params *params, const anihip_md_clusters *clusters,
                                 const float *coords, const float *coords_lo, float *velocities);

/* Isotropic stochastic cell rescaling (Bernetti and Bussi 2020) of the integrator above: a first-order barostat that samples
 * the NPT ensemble from the virial alone, without trial energies or an accept / reject step.  Per molecule c, with
 * eps = ln V and V = |det(cell_c)|, one move is
 *   P_int = (2 K_c - tr W_c) / (3 V)
 *   d eps = -(beta_T / tau_p) (P0_c - P_int) dt  +  sqrt(2 kT_c beta_T dt / (V tau_p)) xi_b
 *   mu    = exp(d eps / 3)
 *   x <- mu x,   v <- v / mu,   cell <- mu cell,   K_c <- K_c / mu^2
 * all in fp64.  kinetic fp64 [C] (Hartree; what anihip_md_kick left, UPDATED), virial fp64 [C][9] (Hartree, dE/d strain of
 * the last force evaluation, row-major), kT fp32 [C] (Hartree, the thermostat's), pressure fp64 [C] (P0, Hartree / Angstrom^3),
 * beta_T the isothermal compressibility in Angstrom^3 / Hartree, tau_p the barostat time in fs.  By Ito's formula the equation
 * in eps carries no kT / V term.  x is the pair coords + coords_lo: the sum is formed in fp64 (exactly), multiplied by mu and
 * stored as coords = (float)x, coords_lo = (float)(x - coords).  cell64 fp64 [C][9] is the master copy of the cell (rows are the
 * cell vectors), cell32 fp32 [C][9] = (float)cell64 is written for the neighbor builders.  scale fp64 [C] OUT: mu of this move.
 * xi_b is the xi_x of anihip_md_noise, widened to fp64, at atom index 0 with the molecule's replica id (replica_ids may be
 * NULL as above) and the step word ANIHIP_MD_BAROSTAT_STEP | params->step: drift steps stay below 2^62 and the Maxwell-
 * Boltzmann draws of the Python layer have bit 63 set, so the three streams are disjoint.  Atoms with active != 0 are scaled;
 * padding and fixed atoms are not touched.  The caller runs it between anihip_md_drift and the force evaluation with the
 * params->step of that drift: it uses the virial of the previous evaluation and the kinetic energy of the previous kick, and
 * the forces that anihip_md_kick then reads belong to the rescaled coordinates.  Requires dt, beta_T, tau_p > 0, the
 * ANIHIP_MD_LANGEVIN flag (the noise needs kT) and step < 2^62.  Two launches, one thread per molecule and then one per atom;
 * no atomics, no host synchronization, bit-identical run to run. */
#define ANIHIP_MD_BAROSTAT_STEP (1ull << 62)
int anihip_md_barostat(void *stream, const anihip_md_params *params, double beta_T, double tau_p, const uint8_t *active,
                       const float *kT, const double *pressure, const int64_t *replica_ids, const double *virial,
                       double *kinetic, double *cell64, float *cell32, float *coords, float *coords_lo, float *velocities,
                       double *scale);

/* Molecular cell rescaling: the barostat above for a system with bond-length constraints.  Atomic scaling x <- mu x would
 * change every constrained length by mu, and the multipliers of a geodesic BAOAB step have no single virial; instead every
 * SCALING GROUP is moved as a rigid body by rescaling its centre of mass.  The groups of molecule c are the clusters of the
 * anihip_md_clusters tables and, each on its own, the free atoms (active == 1).  A cluster with a slot of w = 0 (a fixed
 * anchor) neither moves nor enters any sum.  For a cluster q, with m_i = mass[at] (fp32, amu, as anihip_md_kick reads it),
 * M_q = sum m_i and x = coords + coords_lo read exactly, all in fp64:
 *   X_q = sum m_i x_i / M_q        V_q = sum m_i v_i / M_q
 *   K_mol,c = sum over free atoms of 1/2 m v^2 / ANIHIP_MD_ACC_UNIT  +  sum_q 1/2 M_q |V_q|^2 / ANIHIP_MD_ACC_UNIT
 *   G_c     = sum_q sum_{i in q} f_i . (x_i - X_q)
 * tr W + G is the derivative of the energy under a strain of the cell and of the group centres with the groups translated
 * rigidly (W the atomic dE/d strain, f the forces of the same evaluation at the same coordinates); constraint forces are
 * internal to a group and drop out of it exactly.
 *
 * anihip_md_group_terms writes kinetic_mol fp64 [C] = K_mol (Hartree) and virial_mol fp64 [C] = G (Hartree).  They belong to
 * the state after anihip_md_kick, when x, the projected v and f are those of one evaluation: the caller runs it then (or after
 * setting velocities), not after the drift, whose coordinates the forces held no longer match.  scratch: caller-owned,
 * ANIHIP_MD_GROUP_SCRATCH_BYTES(n_mol, atoms_per_mol) bytes, no state: fp64 [C][A][2], where each cluster leaves its two terms
 * at the atom of slot 0 and zeros at its other atoms, then fp64 [C][ceil(A / 256)][2] sums of 256-atom chunks.  One thread per
 * cluster, then one per atom; 2 launches for A <= 256 and 3 beyond (one less without clusters).  A cluster whose table entries
 * are out of range is skipped (its atoms then read unset scratch: the tables are the caller's to get right).
 *
 * anihip_md_barostat_groups is anihip_md_barostat with
 *   P_int = (2 K_mol - (tr W + G)) / (3 V),   d eps and mu as above (the same xi_b, the same step word)
 *   free atom:     x <- mu x,                   v <- v / mu
 *   cluster atom:  x_i <- x_i + (mu - 1) X_q,   v_i <- v_i + (1 / mu - 1) V_q
 *   cell <- mu cell,   kinetic <- kinetic - (1 - mu^-2) K_mol (formed as (kinetic - K_mol) + K_mol / mu^2),   K_mol <- K_mol / mu^2
 * Bond vectors and relative velocities are those of before the move (up to the rounding of the two-float pair and of fp32),
 * so the constraints hold without another solver pass.  kinetic_mol is UPDATED, virial_mol is read.  With n_clusters = 0,
 * kinetic_mol = kinetic and virial_mol = 0 the result is that of anihip_md_barostat bit for bit.  Three launches (two without
 * clusters): one thread per molecule, per atom, per cluster.  Both entry points: no atomics, every sum in a fixed order, no
 * host synchronization, bit-identical run to run; the clusters need not be sorted by molecule; tolerance, max_iterations and
 * iterations of the tables are not used. */
#define ANIHIP_MD_GROUP_SCRATCH_BYTES(n_mol, atoms_per_mol) \
    ((size_t)(n_mol) * ((size_t)(atoms_per_mol) + ((size_t)(atoms_per_mol) + 255) / 256) * 2 * sizeof(double))
int anihip_md_group_terms(void *stream, const anihip_md_params *params, const anihip_md_clusters *clusters,
                          const uint8_t *active, const float *mass, const float *coords, const float *coords_lo,
                          const float *velocities, const float *forces, double *scratch, double *kinetic_mol,
                          double *virial_mol);
int anihip_md_barostat_groups(void *stream, const anihip_md_params *params, double beta_T, double tau_p, const uint8_t *active,
                              const float *kT, const double *pressure, const int64_t *replica_ids, const double *virial,
                              double *kinetic, double *cell64, float *cell32, float *coords, float *coords_lo,
                              float *velocities, double *scale, const anihip_md_clusters *clusters, const float *mass,
                              double *kinetic_mol, const double *virial_mol);

/* Ring polymers: path-integral MD over the beads of a batch (torchani_amd.md.RingPolymerDynamics).  The batch has
 * C = R P entries; entries r P .. r P + P - 1 are the beads j = 0 .. P - 1 of ring polymer r, and all beads of a polymer have
 * the same species, masses and active mask (those of the first bead are read).  With the physical temperature T_r the beads
 * are sampled at P T_r (the convention of Ceriotti et al., J. Chem. Phys. 133, 124104 (2010)):
 *   H_P = sum_j [ sum_i 1/2 m_i v_ij^2 + V(q_j) ] + sum_j sum_i 1/2 m_i w_P^2 (q_ij - q_i,j+1)^2,  w_P = P k_B T_r / hbar,
 * bead P being bead 0.  Normal modes k = 0 .. P - 1 of a bead vector y_j:  y = C u, C real and orthogonal,
 *   C_jk = 1 / sqrt(P) (k = 0),  sqrt(2 / P) cos(2 pi j k / P) (0 < k < P / 2),  (-1)^j / sqrt(P) (k = P / 2, P even),
 *   sqrt(2 / P) sin(2 pi j k / P) (k > P / 2),  with  w_k = 2 w_P sin(k pi / P).
 * A step is BAOAB with an exact A (the "BAOAB-PILE" of Liu, Li and Liu 2016), in the shape of the classical one: the ring-
 * polymer drift, the forces of all beads at the new coordinates, anihip_md_kick (unchanged: the closing B and the kinetic
 * energy of every bead).  The drift, per active atom and Cartesian component of a polymer:
 *   B        v_j += dt/2 f_j inv_mass
 *            (u_k, w_k) = the modes of (q_j, v_j)
 *   A(h)     k = 0: u += h w;  k > 0: (u, w) <- (u cos w_k h + (w / w_k) sin w_k h,  -u w_k sin w_k h + w cos w_k h)
 *   O        w_k = c_k w_k + sqrt(P kT_r (1 - c_k^2) inv_mass) xi_k,  c_k = exp(-gamma_k dt),  gamma_0 = friction_r (0 leaves the
 *            centroid without a thermostat),  gamma_k = 2 pile_lambda w_k for k > 0 (pile_lambda 1: PIMD, 0.5: TRPMD)
 *   A(h)     and back to beads.
 * With ANIHIP_MD_LANGEVIN h = dt/2; without it (RPMD) there is no O and one A(dt).  xi_k is the value of anihip_md_noise at
 * (atom i, the replica id of batch entry r P + k, step): the noise tensor of a step is used row for row, row r P + k driving
 * mode k.  kT fp32 [C] = k_B T in Hartree of the PHYSICAL temperature and friction fp32 [C] are read at the polymer's first
 * bead; kT is needed without the thermostat too (w_P), friction may then be NULL.  Velocities are written as fp32, positions
 * as the two-float pair with coords the fp32 nearest to it.  Inactive atoms keep their coordinates bit for bit and get v = 0.
 * Atoms of constraint clusters (active == 2) are not supported: the kernel has no error channel and leaves them untouched,
 * and RingPolymerDynamics refuses constraints.  Requires 2 <= beads <= ANIHIP_MD_RP_MAX_BEADS and n_mol a multiple of beads.
 *
 * Precision: c_k, 1 - c_k^2 (expm1), sin and cos of w_k h and the matrix C are formed in fp64 once per workgroup.  The centroid
 * is the fp64 mean of the pairs and moves in fp64; modes k > 0 are formed from the offsets from the centroid (and from the
 * mean velocity), in fp64: equal beads have modes that are exactly zero and stay equal bit for bit.  One launch, one thread
 * per (mode, atom, component), the beads and modes of 1024 / beads consecutive floats staged in LDS; one instance for every
 * P, which is read at run time.
 *
 * anihip_md_rp_estimators writes, in fp64 and with every sum in a fixed order (no atomics, bit-identical run to run):
 *   estimators[r][0] = S_r = sum_j sum_i 1/2 m_i w_P^2 |q_ij - q_i,j+1|^2 / ANIHIP_MD_ACC_UNIT   (the spring energy, Hartree)
 *   estimators[r][1] = W_r = sum_j sum_i (q_ij - qbar_i) . f_ij                                  (the centroid-virial sum, Hartree)
 *   centroids[r][i]  = qbar_i = sum_j q_ij / P  of every atom, active or not (fp64 [R][A][3])
 * S and W run over the active atoms; mass fp32 [C][A] in amu, forces those of the coordinates held.  workspace: the
 * anihip_md_workspace_bytes of (n_mol, atoms_per_mol), no state.  One launch, two for polymers of more than 256 atoms. */
#define ANIHIP_MD_HBAR 0.024188843265857   /* Hartree fs */
#define ANIHIP_MD_RP_MAX_BEADS 64
int anihip_md_rp_drift(void *stream, const anihip_md_params *params, int32_t beads, double pile_lambda, const uint8_t *active,
                       const float *inv_mass, const float *kT, const float *friction, const int64_t *replica_ids,
                       float *coords, float *coords_lo, float *velocities, const float *forces);
int anihip_md_rp_estimators(void *stream, const anihip_md_params *params, int32_t beads, const uint8_t *active,
                            const float *mass, const float *kT, const float *coords, const float *coords_lo,
                            const float *forces, double *estimators, double *centroids, void *workspace,
                            size_t workspace_bytes);

/* Temperature replica exchange (parallel tempering) between the entries of a batch (torchani_amd.md.ReplicaExchangeDynamics).
 * TEMPERATURES are swapped, not coordinates: forces, neighbor state, the two-float coordinates and the noise streams stay with
 * the batch entry, only [C]-sized state and a velocity rescale move, and nothing is evaluated again.  A batch of C entries
 * holds L ladders of at most K rungs (all of one ladder the same system).  State, device memory:
 *   slot        int32 [L][K]    the batch entry at rung k; -1 in the unused tail of a shorter ladder            UPDATED
 *   count       int32 [L]       the rungs of each ladder, 0 .. K (clamped); rungs k >= count[l] are not read
 *   rung_of     int32 [C]       the rung of each entry, -1 for an entry in no ladder                            UPDATED
 *   rung_kT     fp32  [L][K]    k_B T of each rung in HARTREE, strictly increasing along a ladder
 *   ladder_ids  int64 [L]       the Philox stream of each ladder (values below 2^32), or NULL for l: a ladder draws the same
 *                               decisions wherever it sits
 *   attempts, accepts  int64 [L][K - 1]   per pair (k, k + 1), ADDED TO
 *   direction   int8  [C], round_trips int32 [C]   the round-trip state below                                   UPDATED
 *   scale       fp64  [C]       OUT: the velocity factor of this attempt for every entry of a ladder (1: the rung is kept)
 *   energies    fp64  [C]       potential energies at the coordinates held (Hartree)
 *   kinetic     fp64  [C]       what anihip_md_kick left, UPDATED;   velocities fp32 [C][A][3], UPDATED
 * (The caller also keeps ladder_of int32 [C], the ladder of each entry, to gather temperatures through rung_of; no kernel
 * reads it.)  Attempt n = params->step pairs the rungs (k, k + 1) with k = n (mod 2) in every ladder; an unpaired top rung, or
 * rung 0 at odd n, sits the attempt out.  For a = slot[l][k] and b = slot[l][k + 1], all in fp64:
 *   arg = (1 / kT_k - 1 / kT_{k+1}) (E_a - E_b)
 *   u   = p(u0) of Philox4x32-10 with key (seed low, seed high) and counter (k, ladder id, step low, step high),
 *         step = ANIHIP_MD_EXCHANGE_STEP | n, p the uniform of anihip_md_noise
 *   accept iff ln u < arg
 * Bit 61 keeps the stream apart from the drifts', the barostat's (bit 62) and the Maxwell-Boltzmann draws' (bit 63): drift
 * steps and attempts stay below 2^61.  On accept the two slot entries and the two rung_of values are swapped; entry a gets
 * v <- v (float)sqrt(kT_{k+1} / kT_k) on every atom with active != 0 and kinetic[a] *= kT_{k+1} / kT_k, entry b the inverse
 * ratio; attempts and accepts are added to by the one thread that owns the pair; an entry that reaches the top rung
 * (count[l] - 1) gets direction -1, one that reaches rung 0 gets round_trips += 1 if its direction was -1 and then direction
 * +1.  (The caller starts with direction +1 at rung 0, -1 at the top rung and 0 between.)  A uniform velocity scale keeps
 * r_ij . (v_i - v_j) = 0, so constrained velocities need no projection.  Friction stays with the entry.  Entries in no ladder,
 * unpaired rungs and rejected pairs are not written at all: their velocities and kinetic energies stay bit-identical.  The
 * caller then sets the thermostat's kT of entry c to rung_kT[ladder_of[c]][rung_of[c]].
 *
 * Two launches: one thread per pair writes the tables, kinetic and scale; one thread per atom, in 256-atom chunks, rescales
 * the velocities where scale is not exactly 1.  No atomics, no host synchronization, bit-identical run to run.  Requires
 * max_rungs >= 2, the ANIHIP_MD_LANGEVIN flag and step < 2^61.  A slot must lie in -1 .. n_mol - 1.  WITHOUT
 * ANIHIP_MD_LADDERS_CHECK THE CALL RETURNS 0 FOR A TABLE THAT BREAKS THIS: it reads nothing on the host and cannot see it.  The
 * kernel then leaves a pair with a slot out of range undecided: nothing is counted, and the member whose slot is in range keeps
 * its rung, its velocities and its kinetic energy (scale 1).  An entry that no slot names although its rung_of is >= 0 -- the
 * one that the bad value displaced -- gets no scale from the attempt, and its velocities are multiplied by what scale[c] held
 * before the call: such a table is outside the contract.  With ANIHIP_MD_LADDERS_CHECK in flags the call first copies slot to
 * the host -- the one synchronization, for a caller that did not build the table itself -- and returns nonzero for such a
 * slot before anything is launched. */
#define ANIHIP_MD_EXCHANGE_STEP (1ull << 61)
#define ANIHIP_MD_LADDERS_CHECK 1
typedef struct {
    int32_t n_ladders, max_rungs;   /* L >= 1, K >= 2 */
    int32_t flags;                  /* ANIHIP_MD_LADDERS_CHECK or 0 */
    int32_t reserved;               /* 0 */
    int32_t *slot;
    const int32_t *count;
    int32_t *rung_of;
    const float *rung_kT;
    const int64_t *ladder_ids;      /* or NULL */
    int64_t *attempts, *accepts;
    int8_t *direction;
    int32_t *round_trips;
    double *scale;
} anihip_md_ladders;
int anihip_md_exchange(void *stream, const anihip_md_params *params, const anihip_md_ladders *ladders, const double *energies,
                       const uint8_t *active, float *velocities, double *kinetic);

/* Biased MD (torchani_amd.md.BatchedDynamics(bias=...)): restraints on collective variables (CVs) and metadynamics, added to
 * the forces held between the evaluation and the kick.  A CV lives on atoms of ONE batch entry; differences are the plain
 * ones of the unwrapped coordinates (no minimum image), and all arithmetic is fp64 on x = coords + coords_lo, read exactly.
 *   ANIHIP_MD_CV_DISTANCE  i-j       s = |x_i - x_j|                                           grad_i = (x_i - x_j) / s = -grad_j
 *   ANIHIP_MD_CV_ANGLE     i-j-k     a = x_i - x_j, b = x_k - x_j, n = a x b, s = atan2(|n|, a.b) in [0, pi]
 *                                    grad_i = a x n / (|a|^2 |n|), grad_k = n x b / (|b|^2 |n|), grad_j = -(grad_i + grad_k):
 *                                    the form through a x b, finite up to a straight angle, no 1 / sin
 *   ANIHIP_MD_CV_DIHEDRAL  i-j-k-l   b1 = x_j - x_i, b2 = x_k - x_j, b3 = x_l - x_k, n1 = b1 x b2, n2 = b2 x b3,
 *                                    s = atan2(|b2| b1.n2, n1.n2) in (-pi, pi], trans = pi; Blondel and Karplus (1996):
 *                                    grad_i = -|b2| n1 / |n1|^2, grad_l = |b2| n2 / |n2|^2, p = b1.b2 / |b2|^2, q = b3.b2 / |b2|^2,
 *                                    grad_j = q grad_l - (1 + p) grad_i, grad_k = p grad_i - (1 + q) grad_l
 * wrap(d) = d - 2 pi floor((d + pi) / (2 pi)) brings a difference of dihedrals into [-pi, pi).
 *
 * Restraint of CV r, restraint[r] = (center, k, half_width), k in Hartree / Angstrom^2 or Hartree / rad^2, k = 0: none:
 *   d = s - center (wrapped for a dihedral),  e = max(0, |d| - half_width),  E = k e^2 / 2,  dE/ds = k e sign(d)
 * Metadynamics: entry c with list[c] = g >= 0 carries the bias of the hills h < used[g] of list g on its one or two CVs
 * meta_cv[c][d] (positions within the entry's CVs, -1: no second one), with the difference wrapped for a dihedral:
 *   V_c = sum_h heights[g][h] exp(-1/2 sum_d inv_sigma2[c][d] (s_d - centers[g][d][h])^2)
 * No truncation.  Entries that share a list are the walkers of multiple-walker metadynamics; they must agree in the kinds of
 * their CVs and in inv_sigma2 (anihip_md_bias_hills reads both from list_entry[g], any member of the list).
 *
 * Tables, device memory unless marked HOST (C = params->n_mol, A = params->atoms_per_mol, G = n_lists, Ncv = n_cvs):
 *   cv_offset    int32 [C + 1]   CSR: entry c owns the CVs cv_offset[c] .. cv_offset[c + 1] - 1, at most ANIHIP_MD_BIAS_MAX_CVS
 *   kind         int32 [Ncv]     ANIHIP_MD_CV_*
 *   atoms        int32 [Ncv][4]  global atom index c A + i of i, j(, k(, l)), distinct, all inside entry c; unused slots -1
 *   restraint    fp64  [Ncv][3]  (center, k >= 0, half_width >= 0)
 *   meta_cv      int32 [C][2]    see above;  inv_sigma2 fp64 [C][2] 1 / sigma_d^2;  height fp64 [C] Hartree
 *   list         int32 [C]       g, or -1: no metadynamics;   rank_in_list int32 [C]  0 .. members[g] - 1, distinct within a list
 *   members      int32 [G]       entries of each list;   list_entry int32 [G] one of them
 *   bias_factor  fp64  [G]       gamma > 1 (well-tempered), or 0 (plain)
 *   used         int32 [G]       hills held, UPDATED by the deposit;   dropped int32 [G]  ADDED TO by a deposit that did not fit
 *   centers      fp64  [G][2][capacity], heights fp64 [G][capacity]   the hills, a structure of arrays; APPENDED TO
 *   status       int32 [C]       OUT of anihip_md_bias_apply: 0, or ANIHIP_MD_BIAS_BAD_* bits of an entry whose tables are out
 *                                of range -- such an entry moves nothing: its forces, energies and CV values are not written
 *   capacity (HOST) hills per list; hills_bound (HOST) the caller's upper bound of every used[g], which sizes the grid of the
 *   hills kernel (hills past it are not summed), or 0 for capacity.
 *
 * anihip_md_bias_apply: forces fp32 [C][A][3] UPDATED, bias_energies fp64 [C] OUT (restraints + V_c), meta_energies fp64 [C]
 * OUT (V_c), cv_values fp64 [Ncv] OUT.  With n_lists = 0 one launch, else two:
 *   hills kernel   one workgroup per (entry, chunk of ANIHIP_MD_BIAS_CHUNK hills), those of entries without a list and of
 *                  chunks past used[g] leaving at once: thread t adds the hills t, t + 256, ... of the chunk in that order, the workgroup sum (lanes, then waves, in a fixed order) of V,
 *                  dV/ds_0 and dV/ds_1 goes to workspace[c][chunk][3]
 *   apply kernel   one workgroup per entry: the chunk sums added in chunk order; one thread per CV evaluates it, its gradient
 *                  and dE/ds (restraint, plus dV/ds_d on the CVs of the metadynamics); one thread per atom of a CV adds
 *                  f = sum over the entry's CVs that hold the atom, in CV order from 0, of -dE/ds grad, and writes
 *                  forces = (float)((double)forces + f) once; bias_energies = (sum of E in CV order) + V_c
 * No atomics on memory: two calls on the same input are bit-identical, and an entry gives the same bits wherever it sits in
 * the batch.  Forces land on fixed atoms too; the integrator ignores them there.
 *
 * anihip_md_bias_deposit (after anihip_md_bias_apply, on its cv_values and meta_energies): every entry with a list appends
 * one hill at h = used[g] + rank_in_list[c]: centers[g][d][h] = its CV d (0 for a missing second one), heights[g][h] =
 * height[c], times exp(-V_c / ((bias_factor[g] - 1) kT_c)) for bias_factor[g] > 0, with kT fp32 [C] in Hartree (NULL: every
 * list deposits the plain height) and V_c = meta_energies[c]: every walker sees the bias of before this round.  Then used[g] +=
 * members[g].  A list with used[g] + members[g] > capacity deposits nothing, keeps used[g] and adds members[g] to dropped[g];
 * nothing is ever written past capacity.  An entry whose status is not 0 appends nothing: the slot that the round reserves
 * for it keeps what it held.  Two launches (one thread per entry, then one per list).
 *
 * anihip_md_bias_hills: V (out_V fp64 [n_points]) and dV/ds (out_dV fp64 [n_points][2]) of list `list` at values fp64
 * [n_points][2], the second column ignored for a list of one CV: one workgroup per point, the chunks summed exactly as
 * above, so a point at a walker's CV values gives the bits of its meta_energies.  The readout for free energies.  A list
 * whose list_entry or CV tables are out of range gives NaN.
 *
 * anihip_md_bias_workspace_bytes: 0 for n_lists = 0, else C ceil(capacity / ANIHIP_MD_BIAS_CHUNK) 3 doubles.
 * All of them return nonzero for what the host can see (null pointers, negative counts, a short workspace, a list index
 * outside 0 .. G - 1); what lives in device memory is checked by the kernels and reported in status. */
#define ANIHIP_MD_BIAS_MAX_CVS 16
#define ANIHIP_MD_BIAS_CHUNK 1024
#define ANIHIP_MD_CV_DISTANCE 0
#define ANIHIP_MD_CV_ANGLE 1
#define ANIHIP_MD_CV_DIHEDRAL 2
#define ANIHIP_MD_BIAS_BAD_OFFSET 1   /* cv_offset outside 0 .. Ncv, falling, or more than ANIHIP_MD_BIAS_MAX_CVS CVs */
#define ANIHIP_MD_BIAS_BAD_CV 2       /* a kind that is none of the three, an atom outside the entry or given twice */
#define ANIHIP_MD_BIAS_BAD_LIST 4     /* list, rank_in_list or meta_cv out of range */
typedef struct {
    int32_t n_cvs, n_lists, capacity, hills_bound, reserved;
    int32_t n_entries;   /* C, equal to params->n_mol (anihip_md_bias_hills takes no params) */
    const int32_t *cv_offset, *kind, *atoms;
    const double *restraint;
    const int32_t *meta_cv;
    const double *inv_sigma2, *height;
    const int32_t *list, *rank_in_list, *members, *list_entry;
    const double *bias_factor;
    int32_t *used, *dropped;
    double *centers, *heights;
    int32_t *status;
} anihip_md_bias;
size_t anihip_md_bias_workspace_bytes(const anihip_md_params *params, const anihip_md_bias *bias);
int anihip_md_bias_apply(void *stream, const anihip_md_params *params, const anihip_md_bias *bias, const float *coords,
                         const float *coords_lo, float *forces, double *bias_energies, double *meta_energies,
                         double *cv_values, void *workspace, size_t workspace_bytes);
int anihip_md_bias_deposit(void *stream, const anihip_md_params *params, const anihip_md_bias *bias, const float *kT,
                           const double *cv_values, const double *meta_energies);
int anihip_md_bias_hills(void *stream, const anihip_md_bias *bias, int32_t list, int64_t n_points, const double *values,
                         double *out_V, double *out_dV);

/* Group CVs of biased MD (torchani_amd.md.center, md.coordination; csrc/md_sites.hip): centres of groups of atoms and
 * coordination numbers reach the kernels above as SITES, pseudo-atoms appended to every entry.  Entry c of A atoms becomes an
 * extended entry of A' = A + V atoms, V = max_sites <= ANIHIP_MD_SITES_MAX: the extended arrays coords_ext, coords_lo_ext and
 * forces_ext are fp32 [C][A'][3], site v of entry c is their atom c A' + A + v, and the CV tables of anihip_md_bias name it
 * like any atom.  One evaluation is
 *   anihip_md_sites_gather  ->  anihip_md_bias_apply(params with atoms_per_mol = A', the extended arrays)  ->  anihip_md_sites_spread
 * and both calls here take params with atoms_per_mol = A.  All arithmetic is fp64 on x = coords + coords_lo, read exactly.
 *
 * Sites (site_kind):
 *   ANIHIP_MD_SITE_CENTER  x_v = sum_i w_i x_i over group site_ref, plain unwrapped coordinates (no minimum image); the weights
 *                          are the host's, fp64, summing to 1 (m_i / sum m, or 1 / n).  Stored as a two-float pair per
 *                          component: hi = (float)x, lo = (float)(x - hi).
 *   ANIHIP_MD_SITE_VALUE   carries the coordination number s >= 0 of row site_ref of the coordination tables as a DISTANCE:
 *   ANIHIP_MD_SITE_ANCHOR  the anchor in slot v - 1 sits at exactly (0, 0, 0) and the value site in slot v at (s', 0, 0), s' =
 *                          max(s, 2^-64) as a two-float pair.  ANIHIP_MD_CV_DISTANCE on (value, anchor) then returns
 *                          sqrt(s' s') = s' exactly with the gradient exactly (+1, 0, 0) on the value site, so after
 *                          anihip_md_bias_apply forces_ext[value].x = -dE/ds, rounded to fp32 by that kernel.  The floor keeps
 *                          the gradient finite at s = 0 and lo out of the fp32 subnormals (the pair holds s to 2^-48 relative).
 *                          This representation is internal to the three calls.
 * Every site gets zero force in forces_ext; the real atoms carry the forces given.  Slots of kind ANIHIP_MD_SITE_NONE are not
 * written.
 *
 * Coordination number of row q = (entry, group A, group B, slot of the value site, n) with coord_params[q] = (r0, d0, r_max, b):
 *   s = sum_{i in A} sum_{j in B, j != i} sw(r_ij),   r_ij = |x_i - x_j| (minimum image along the directions with pbc != 0)
 *   x = max(r - d0, 0) / r0,  base(r) = 1 / (1 + x^n), x^n by repeated multiplication, n an integer in 2 .. 32
 *   sw(r) = (base(r) - b) / (1 - b) for r < r_max, 0 for r >= r_max;  b = base(r_max), or b = 0 with r_max = infinity
 *   dsw/dr = -n x^(n-1) / (r0 (1 + x^n)^2) / (1 - b), 0 for r <= d0 and for r >= r_max
 * A and B may overlap or coincide: the same atom on both sides is skipped, ordered pairs are counted as written.  Minimum image,
 * rows of cell the lattice vectors:  d <- d - (rint(d cell^-1) masked by pbc) cell; the caller keeps r_max within half the
 * smallest perpendicular width over the periodic directions, so the rounded image is the nearest wherever sw != 0.
 *
 * Tables, device memory unless marked HOST (C = n_entries, V = max_sites, Ng = n_groups, Nq = n_coord, Nm = n_members):
 *   site_kind     int32 [C][V]      ANIHIP_MD_SITE_*;   site_ref int32 [C][V]  a group (centre) or a coordination row (anchor, value)
 *   group_offset  int32 [Ng + 1]    CSR: group g owns group_atoms[group_offset[g] .. group_offset[g + 1] - 1]
 *   group_atoms   int32 [n_group_atoms]  global atom indices c A + i, ascending within a group, all inside the entry of the site
 *   group_weights fp64  [n_group_atoms]  w_i of a centre's group (not read for coordination groups)
 *   coord         int32 [Nq][5]     (entry, group A, group B, slot v >= 1 of the value site, n);   coord_params fp64 [Nq][4]
 *   member_offset int32 [C A + 1]   the inverse CSR: atom c A + i owns the rows member_offset[c A + i] .. member_offset[c A + i + 1] - 1
 *   member_site   int32 [Nm][2]     (slot v, ANIHIP_MD_SITE_ROLE_*), in ascending slot order, side A before side B
 *   member_weight fp64  [Nm]        w_i for ANIHIP_MD_SITE_ROLE_CENTER, else 0
 *   status        int32 [C]         OUT of anihip_md_sites_gather: 0, or ANIHIP_MD_SITES_BAD_* bits
 *   pbc, cell, inv_cell (HOST)      by value; cell and inv_cell row-major, not read without a periodic direction
 *
 * anihip_md_sites_gather, at most two launches:
 *   coordination kernel  (only with Nq > 0) one workgroup per (row q, chunk of 256 atoms of A, tile of 256 atoms of B): one
 *                        thread per atom of A loops over the tile in ascending order, the tile staged in LDS; the workgroup sum
 *                        (lanes, then waves, in a fixed order) goes to workspace[q][chunk][tile]
 *   gather kernel        per entry one workgroup per chunk of 256 real atoms, which copies coords, coords_lo and forces into
 *                        the extended arrays, and one more for the sites: it checks every table the entry names (below), then
 *                        writes the sites in slot order -- a centre by one sum (thread t adds the atoms t, t + 256, ... of the
 *                        group in that order, then lanes and waves in a fixed order), a value site by its partial sums, the
 *                        chunks in order and within a chunk the tiles in order
 * anihip_md_sites_spread, one launch, one workgroup per (entry, chunk of 64 atoms), each atom i written once:
 *   acc = (double)forces_ext[i]; through the atom's rows of the inverse CSR in order: a centre v adds w_i (double)forces_ext[v];
 *   a coordination row with G = (double)forces_ext[value].x adds G sum_{j in the other group, j != i} dsw/dr(r_ij) (x_i - x_j)_mic
 *   / r_ij, terms with dsw/dr = 0 left out (r = 0 is never divided by); an atom on both sides has a row for each.  The other
 *   group is staged through LDS in tiles of 256 atoms and an atom has four threads, one for each quarter of every tile: each
 *   adds its quarters in ascending order from 0 over all tiles, and the sum is (q0 + q1) + (q2 + q3).  forces[i] = (float)acc.
 *   Atoms without rows get forces_ext[i] bit for bit.
 * No atomics on memory: two calls on the same input are bit-identical, and an entry gives the same bits wherever it sits in
 * the batch.
 *
 * Checks: the kernels range-check every index they follow.  An entry whose site table (a kind outside the four, a group or
 * row out of range, a falling or overlong CSR offset, an anchor without its value site or the reverse, a row that names another
 * entry or slot, n or the parameters out of range: ANIHIP_MD_SITES_BAD_SITE), group atoms (outside the entry:
 * ANIHIP_MD_SITES_BAD_GROUP) or inverse table (ANIHIP_MD_SITES_BAD_MEMBER) is broken gets the bits in status; its sites are
 * then placed at (v + 1, 0, 0) Angstrom so that the bias kernels see finite positions, and anihip_md_sites_spread, which reads
 * status as the gather left it, leaves that entry's forces as they were: the model's.  Other entries proceed.  What the host
 * can see (null pointers, V outside 1 .. ANIHIP_MD_SITES_MAX, a short workspace) returns nonzero before any launch.
 * anihip_md_sites_workspace_bytes: Nq ceil(A / 256)^2 doubles. */
#define ANIHIP_MD_SITES_MAX 64
#define ANIHIP_MD_SITE_NONE 0
#define ANIHIP_MD_SITE_CENTER 1
#define ANIHIP_MD_SITE_ANCHOR 2
#define ANIHIP_MD_SITE_VALUE 3
#define ANIHIP_MD_SITE_ROLE_CENTER 0
#define ANIHIP_MD_SITE_ROLE_A 1
#define ANIHIP_MD_SITE_ROLE_B 2
#define ANIHIP_MD_SITES_BAD_SITE 1
#define ANIHIP_MD_SITES_BAD_GROUP 2
#define ANIHIP_MD_SITES_BAD_MEMBER 4
typedef struct {
    int32_t n_entries, max_sites, n_groups, n_group_atoms, n_coord, n_members;
    int32_t pbc[3];
    int32_t reserved;   /* 0 */
    double cell[9], inv_cell[9];
    const int32_t *site_kind, *site_ref, *group_offset, *group_atoms;
    const double *group_weights;
    const int32_t *coord;
    const double *coord_params;
    const int32_t *member_offset, *member_site;
    const double *member_weight;
    int32_t *status;
} anihip_md_sites;
size_t anihip_md_sites_workspace_bytes(const anihip_md_params *params, const anihip_md_sites *sites);
int anihip_md_sites_gather(void *stream, const anihip_md_params *params, const anihip_md_sites *sites, const float *coords,
                           const float *coords_lo, const float *forces, float *coords_ext, float *coords_lo_ext,
                           float *forces_ext, void *workspace, size_t workspace_bytes);
int anihip_md_sites_spread(void *stream, const anihip_md_params *params, const anihip_md_sites *sites, const float *coords,
                           const float *coords_lo, const float *forces_ext, float *forces);

/* Observables accumulated along a trajectory on the device (torchani_amd.md.RadialDistribution, MeanSquaredDisplacement,
 * VelocityAutocorrelation; csrc/md_observe.hip).  Neither call reads on the host.
 *
 * anihip_md_rdf_accumulate adds one sample of a pair-distance histogram to `counts` from neighbor rows (meta, ent: the format
 * above, lo = 0, of all N = n_mol atoms_per_mol atoms; ent_capacity = float4 entries that `ent` holds).  With
 * r = sqrt(dx^2 + dy^2 + dz^2) taken in fp64 from the fp32 row entry,
 *   counts[c][p][b] += #{row entries (i -> j): i in entry c, species[i] = a_p, species_j = b_p, r < r_max,
 *                        floor(r (bins / r_max)) = b}
 * (b = bins - 1 if rounding carries the product to bins), c = 0 for per_entry = 0, where the counters are [n_pairs][bins], and
 * c = i / atoms_per_mol for per_entry = 1, [n_mol][n_pairs][bins].  pair_slot (HOST, 64 x int8) maps 8 s_i + s_j to the pair p
 * or to -1; species (int32 [N], element indices 0 .. 7 as the rows carry them; < 0: padding, skipped).  Ordered pairs and
 * periodic images, an atom's own image included, count once each, as the rows hold them.  n_pairs in 1 .. 8, bins in
 * 1 .. 1024, n_pairs bins <= 8192.  One wave per central atom, lanes over its row, a histogram of uint32 in LDS per
 * workgroup, added to `counts` (uint64) with integer atomics, non-zero bins only, whenever the workgroup's entry changes
 * (per_entry) and at its end: integer sums, so the result does not depend on the order of arrival.  A row that the builder
 * zeroed for overflow contributes nothing; the builder's status word says so.
 *
 * anihip_md_corr_accumulate takes sample k = `sample` (0, 1, ...) of a multiple-time-origin correlation over a ring of the
 * last M = lags samples.  The atoms are named by a gather table: gather int32 [n_mol][G] (G = max_atoms), the index within
 * its entry of the g-th atom, -1 past the entry's atoms; gather_species int32 [n_mol][G] in 0 .. n_species - 1 (anything else:
 * the slot is skipped), sorted by species within an entry for speed, not for correctness.
 *   ANIHIP_MD_CORR_MSD   y = (double)x[i] + (double)x_lo[i]  (x_lo NULL: 0), ring of double [M][n_mol][3][G]
 *   ANIHIP_MD_CORR_VACF  y = x[i], ring of float [M][n_mol][3][G]
 * The call writes y into slot k mod M and then, for every lag l = 0 .. min(k, M - 1), with y' of slot (k - l) mod M,
 *   MSD   S[c][s][l] += sum_{g of entry c, species s} |y - y'|^2
 *   VACF  S[c][s][l] += sum_{g of entry c, species s} y . y'        (S: double [n_mol][n_species][M], products in fp64)
 * No atomics: one thread per gather slot, workgroups of 256 slots; per lag the terms of a species are summed over the 64
 * lanes of a wave by a butterfly, then over the four waves in order, to workspace[c][chunk][s][l]; a second launch adds the
 * chunks in ascending order to S.  Two calls on the same input give the same bits.  A gather index outside
 * 0 .. atoms_per_mol - 1 is skipped.  lags in 1 .. 65536, n_species in 1 .. 8.
 * anihip_md_corr_workspace_bytes: n_mol ceil(G / 256) n_species M doubles. */
#define ANIHIP_MD_CORR_MSD 0
#define ANIHIP_MD_CORR_VACF 1
#define ANIHIP_MD_RDF_MAX_PAIRS 8
#define ANIHIP_MD_RDF_MAX_BINS 1024
int anihip_md_rdf_accumulate(void *stream, const anihip_md_params *params, int32_t n_pairs, int32_t bins, double r_max,
                             int32_t per_entry, const int8_t *pair_slot, const int32_t *species, const uint32_t *meta,
                             const float *ent, int64_t ent_capacity, uint64_t *counts);
size_t anihip_md_corr_workspace_bytes(int64_t n_mol, int64_t max_atoms, int64_t lags, int64_t n_species);
int anihip_md_corr_accumulate(void *stream, const anihip_md_params *params, int32_t kind, int32_t lags, int32_t n_species,
                              int32_t max_atoms, int64_t sample, const int32_t *gather, const int32_t *gather_species,
                              const float *x, const float *x_lo, void *ring, double *S, void *workspace,
                              size_t workspace_bytes);

/* Holonomic constraints on internal coordinates for anihip_lbfgs_step (torchani_amd.geomopt.GeometryOptimizer(constraints=),
 * csrc/geom_constraints.hip): the CVs above (ANIHIP_MD_CV_*, csrc/md_cv.h) held at targets, the way ASE's FixInternals works
 * with its LBFGS.  Relaxed scans: every grid point is an entry of the batch with its own target.  Everything is fp64 on the
 * fp32 coords read exactly (the optimizer has no low word).  Per entry c with its n <= ANIHIP_GEOM_MAX_CONSTRAINTS constraints:
 *   w_i = 1 for active[i] != 0, else 0;  J_k = d s_k / d x with the columns of atoms of w = 0 zeroed (a constraint may sit on
 *   a fixed atom, which anchors it);  G = J J^T, solved by Cholesky in the stored order; a pivot <= 1e-12 x the largest diagonal
 *   element of G (or one that is not finite) is SINGULAR: a redundant pair of constraints, a constraint whose atoms are all
 *   fixed, collinear atoms of an angle or dihedral.
 * Tables, device memory (C = n_mol, A = atoms_per_mol, N = n_constraints):
 *   offset       int32 [C + 1]  CSR: entry c owns the constraints offset[c] .. offset[c + 1] - 1
 *   kind         int32 [N]      ANIHIP_MD_CV_*
 *   atoms        int32 [N][4]   global atom index c A + i, distinct, all inside entry c; unused slots -1
 *   target       fp64  [N]      Angstrom or rad
 *   values       fp64  [N]      OUT: s_k;   multipliers fp64 [N]  OUT of the projection: lambda_k
 *   iterations   int32 [C]      OUT of the restore
 *   status       int32 [C]      ANIHIP_GEOM_* bits, OR-ed in and never cleared by the kernels
 *   tolerance (HOST, > 0) and max_iterations (HOST, >= 1) of the restore.
 *
 * anihip_geom_constraints_project: solves G lambda = J f and writes, for every atom named by a constraint,
 *   forces[i] = (float)((double)f_i - sum_k lambda_k J_k,i), the sum over k in constraint order (the first slot that names the
 *   atom writes it); multipliers[k] = lambda_k, values[k] = s_k.  Atoms in no constraint are not written.  At a constrained
 *   minimum f = J^T lambda, so the slope of the relaxed energy along a target is dE* / dt_k = -lambda_k (the torque of a
 *   torsion profile).
 * anihip_geom_constraints_restore: Newton iteration back onto the targets by the minimum-norm correction.  Loop: s and J at
 *   x, r_k = s_k - t_k (wrapped into [-pi, pi) for a dihedral); stop when max |r| <= tolerance; else G mu = r,
 *   x_i <- x_i - sum_k mu_k J_k,i, one iteration counted, at most max_iterations of them (then ANIHIP_GEOM_NOT_CONVERGED).
 *   coords = (float)x for the atoms named, only if an iteration moved them; values[k] = s_k at the fp32 coordinates written
 *   (the residual the caller can trust); iterations[c].
 * One wave per entry, constraint k on lane k, G one element per lane, gradients and multipliers in LDS.  No atomics on memory
 * and every sum in a fixed order: bit-identical run to run and wherever the entry sits in the batch.  An entry with a broken
 * table (an offset that falls, leaves 0 .. N or spans more than 8 constraints; a kind outside the three; an atom outside the
 * entry, repeated within a constraint, or missing) sets ANIHIP_GEOM_BAD_TABLE and writes nothing else; a singular entry sets
 * ANIHIP_GEOM_SINGULAR and writes nothing else; one that does not converge sets its bit and is left unmoved.  Other entries
 * proceed; entries without constraints return at once, and N = 0 launches nothing.  Null pointers, tolerance <= 0 and
 * max_iterations < 1 return nonzero before any launch. */
#define ANIHIP_GEOM_MAX_CONSTRAINTS 8
#define ANIHIP_GEOM_BAD_TABLE 1
#define ANIHIP_GEOM_SINGULAR 2
#define ANIHIP_GEOM_NOT_CONVERGED 4
typedef struct {
    int32_t n_constraints, max_iterations;
    double tolerance;
    const int32_t *offset, *kind, *atoms;
    const double *target;
    double *values, *multipliers;
    int32_t *iterations, *status;
} anihip_geom_constraints;
int anihip_geom_constraints_project(void *stream, int64_t n_mol, int64_t atoms_per_mol, const anihip_geom_constraints *tables,
                                    const uint8_t *active, const float *coords, float *forces);
int anihip_geom_constraints_restore(void *stream, int64_t n_mol, int64_t atoms_per_mol, const anihip_geom_constraints *tables,
                                    const uint8_t *active, float *coords);

/* Saddle-point search of a batch of molecules (torchani_amd.geomopt.SaddleOptimizer, csrc/saddle.hip): partitioned
 * rational-function optimization (P-RFO, Baker 1986) on a dense model Hessian that the caller replaces by the exact one every
 * few steps and that the Bofill formula updates in between.  Everything is fp64 on the fp32 coords and forces read exactly;
 * every molecule c of [n_mol][atoms_per_mol] = [C][A] on its own, n = 3 A.  A step of the caller is: project, a symmetric
 * eigensolver on `projected` (eigenvalues ascending, eigenvectors in the columns), step, the energies and forces at the moved
 * coords, accept.
 *
 * kind uint8 [C][A]: 0 = padding, 1 = a free atom, 2 = a fixed atom (real, never moves); a coordinate is ACTIVE when its atom
 * is free, and g = -forces on the active coordinates, 0 elsewhere.  An entry is FROZEN when converged[c] != 0 or
 * status[c] != 0: the three entry points leave it alone (its coords stay bit-identical, its last_step is zero).
 *
 * project: converged[c] |= max over the free atoms of |f_i| < fmax (then frozen).  Else the rigid motions of the entry are
 *   orthonormalized (Gram-Schmidt, twice) into q_1 .. q_r, r <= 6: the three translations of the free atoms when the entry
 *   has no fixed atom, and the three rotations about the free atoms' centroid when in addition periodic == 0; a vector whose
 *   remainder falls to 1e-8 of its length is dropped (linear and one-atom entries).  With D the 0 / 1 diagonal of the active
 *   coordinates, Q = [q_1 .. q_r], P = D - Q Q^T and mu = 1 + the largest row sum of |hessians[c]|:
 *     gproj = P g  (kept in the workspace),  projected[c] = P H P + mu (I - P)   (H = hessians[c], taken as symmetric).
 *   Every eigenvalue of the part that matters is below mu - 1; the inactive coordinates and the rigid motions sit at mu.
 * step: g~ = V^T gproj.  The followed mode k is the lowest eigenvalue (follow == 0) or, for follow == 1, the mode with
 *   the largest |V_k . modes[c]| among the eigenvalues below mu / 2 (ties: the lowest index).  Along k the step maximizes,
 *   s~_k = -g~_k / (lam_k - gp), gp = (lam_k + sqrt(lam_k^2 + 4 g~_k^2)) / 2; along every other mode it minimizes,
 *   s~_i = -g~_i / (lam_i - gm), gm the lowest root of gm = sum_{i != k} g~_i^2 / (gm - lam_i), which lies below
 *   min(0, the smallest lam_i with g~_i != 0) and is found by bisection from the bracket [hi - 1.000001 |g~|, hi]; a mode with
 *   g~_i == 0 gets s~_i = 0.  If |s~| > trust_radii[c] it is scaled to it; predicted = sum g~_i s~_i + lam_i s~_i^2 / 2.
 *   s = V s~; on the active coordinates coords += (float)s, last_step = (float)s; the old coords are kept for accept, and so is
 *   the displacement (new - old coords, exact in fp64) for the Bofill update.  eigenvalues[c] = lam_k, modes[c] = V_k.
 * accept: e', f' = new_energies, new_forces (at the moved coords); energies and forces still hold those of the old coords.
 *   |predicted| < energy_floor: accepted, the radius unchanged.  Else rho = (e' - e) / predicted; |rho - 1| > 1: REJECTED --
 *   coords restored bit for bit, energies and forces left as they are, radius <- max(radius / 4, min_trust),
 *   n_rejected[c] += 1.  Otherwise accepted, n_steps[c] += 1, and radius <- min(2 radius, max_trust) if |rho - 1| < 0.25 and
 *   |s~| >= 0.99 radius, radius <- max(radius / 2, min_trust) if |rho - 1| > 0.75.  An accepted entry takes e', f' into
 *   energies, forces.  With bofill != 0 its model Hessian is first updated in place, s the displacement, y = g' - g on the
 *   active coordinates, xi = D (y - H s), phi = (xi.s)^2 / ((xi.xi) (s.s)) (0 when xi.s == 0):
 *     H += phi xi xi^T / (xi.s) + (1 - phi) ((xi s^T + s xi^T) / (s.s) - (xi.s) s s^T / (s.s)^2),
 *   skipped when xi.xi or s.s is zero; the update is symmetric bit for bit.
 *
 * status int32 [C], OR-ed in and never cleared: ANIHIP_SADDLE_BAD_TABLE (a kind above 2), ANIHIP_SADDLE_NONFINITE (a force,
 * Hessian row, eigenvalue or new energy that is not finite), ANIHIP_SADDLE_NO_BRACKET (the bracket of gm did not hold).  The
 * entry that sets a bit in step or accept is left at its old coords.
 * workspace: anihip_saddle_workspace_bytes(n_mol, atoms_per_mol) bytes, 256-byte aligned regions in this order:
 *   q, b fp64 [C][6][n] | gproj, displacement, xi fp64 [C][n] | old coords fp32 [C][n] | scalars fp64 [C][8]
 * kept between the three calls of a step.  n <= ANIHIP_SADDLE_MAX_COORDS: one workgroup per molecule holds the six rigid
 * vectors (project) or four vectors of n (step) in its LDS.  project and accept are two launches each (one workgroup per
 * molecule, then a streaming pass over [C][n][n] by blocks of 16 rows), step is one; no allocation, no atomics, every sum
 * in a fixed order: bit-identical run to run.  Null pointers and sizes out of range return nonzero before any launch. */
#define ANIHIP_SADDLE_MAX_COORDS 768
#define ANIHIP_SADDLE_BAD_TABLE 1
#define ANIHIP_SADDLE_NONFINITE 2
#define ANIHIP_SADDLE_NO_BRACKET 4
typedef struct {
    int32_t n_mol, atoms_per_mol;
    int32_t periodic;   /* != 0: the rotations are not projected out */
    int32_t follow;     /* 0: the lowest mode; 1: the largest overlap with modes[c] */
    double fmax;        /* Hartree / Angstrom */
    double max_trust, min_trust; /* Angstrom */
    double energy_floor;         /* Hartree */
    const uint8_t *kind;         /* [C][A] */
    float *coords;               /* [C][A][3], moved in place */
    double *energies;            /* [C] */
    float *forces;               /* [C][A][3] */
    double *hessians;            /* [C][n][n], the model Hessian */
    double *trust_radii;         /* [C] */
    double *eigenvalues;         /* [C] */
    double *modes;               /* [C][n] */
    float *last_step;            /* [C][A][3] */
    uint8_t *accepted, *converged; /* [C] */
    int32_t *n_steps, *n_rejected, *status; /* [C] */
    void *workspace;
    size_t workspace_bytes;
} anihip_saddle;
size_t anihip_saddle_workspace_bytes(int64_t n_mol, int64_t atoms_per_mol);   /* 0 + anihip_last_error() */
int anihip_saddle_project(void *stream, const anihip_saddle *state, double *projected);
int anihip_saddle_step(void *stream, const anihip_saddle *state, const double *eigenvalues, const double *eigenvectors);
int anihip_saddle_accept(void *stream, const anihip_saddle *state, const double *new_energies, const float *new_forces,
                         int32_t bofill);

/* Reaction paths of a batch of molecules (torchani_amd.geomopt.ReactionPathFollower, csrc/irc.hip): the intrinsic reaction
 * coordinate, the steepest-descent path in mass-weighted coordinates q = M^1/2 x, integrated by the local quadratic
 * approximation (LQA, Page & McIver 1988) on a dense Cartesian model Hessian as the saddle search keeps it (exact every few
 * points, Bofill-updated in between).  Everything is fp64 on the fp32 coords and forces read exactly; every molecule c of [C][A] on its
 * own, n = 3 A <= ANIHIP_SADDLE_MAX_COORDS.  A point of the caller is: project, a symmetric eigensolver on `projected`
 * (eigenvalues ascending, eigenvectors in the columns), step, the energies and forces at the moved coords, commit.
 *
 * kind as in anihip_saddle; masses fp64 [C][A] in amu.  w = m^-1/2 on the active coordinates and 0 elsewhere, W = diag(w),
 * g = -forces on the active coordinates.  An entry is FROZEN when reason[c] != 0 (done) or status[c] != 0: the three entry
 * points leave it alone (coords, energies, forces, hessians, counters and path stay bit-identical, its last_step is zero).
 *
 * project: the rigid motions of the entry in mass-weighted coordinates, sqrt(m_i) e_a (when the entry has no fixed atom) and
 *   sqrt(m_i) e_a x (x_i - x_com) about the centre of mass of the free atoms (when in addition periodic == 0), are
 *   orthonormalized as in anihip_saddle_project (Gram-Schmidt twice, a vector dropped when its remainder falls to 1e-8 of its
 *   length) into Q.  With H_q = W H W, D the 0 / 1 diagonal of the active coordinates, P = D - Q Q^T and mu = 1 + the largest
 *   row sum of |H_q|:
 *     gproj = P W g  (kept in the workspace),  projected[c] = P H_q P + mu (I - P).
 *   A mass of a real atom (kind 1 or 2) that is not finite and positive sets ANIHIP_IRC_BAD_TABLE.
 * step: g~ = V^T gproj.
 *   The first point from a saddle, n_points[c] == 0 and direction != NULL: dq = +-step V_0 (the lowest eigenvector), the sign
 *   that of V_0 . (M^1/2 direction[c]) over the active coordinates, + when that overlap is zero; the arc increment is step.
 *   Otherwise the path of the quadratic model through the point, dq/dt = -(gproj + H' dq): q(t) = q_0 + V alpha(t),
 *     alpha_i(t) = -g~_i (1 - e^(-lam_i t)) / lam_i   (-g~_i t for lam_i == 0),   ds/dt = (sum g~_i^2 e^(-2 lam_i t))^1/2,
 *   followed to the time t with s(t) = step, |s(t) - step| <= 1e-9 step.  A mode with g~_i == 0 does not move; if none moves
 *   the step and the arc increment are zero.  If every moving mode has lam_i > 0 and s(T) < step at T = 40 / min lam_i, the
 *   step LANDS on the minimum of the model: alpha_i = -g~_i / lam_i and the arc increment is s(T).  s is integrated by 16-point
 *   Gauss-Legendre panels whose widths grow by sqrt(2) from min(0.01 / max |lam_i|, step / |g~|) (over the moving modes), t is
 *   found by Newton's iteration on s(t) - step inside the bracketing panel, bisection when it leaves the bracket.
 *   dx = W V alpha; on the active coordinates coords += (float)dx, last_step = (float)dx; the old coords are kept for commit,
 *   and so is the displacement (new - old coords, exact in fp64) for the Bofill update.  The arc increment handed to commit
 *   is the larger of the one above and the mass-weighted length of that displacement, |M^1/2 (new - old coords)|: the
 *   rounding of the fp32 coordinates can lengthen a straight or a very short step by an ulp of a coordinate, and the arc
 *   lengths of a path are never shorter than the chords between its stored points.
 * commit: e', f' = new_energies, new_forces (at the moved coords); energies and forces still hold those of the old coords.
 *   e' > e + energy_floor: the coords are restored bit for bit, nothing is appended, reason[c] = ANIHIP_IRC_ENERGY_ROSE.
 *   Otherwise, with bofill != 0 the model Hessian is updated in place by the formula of anihip_saddle_accept (s the Cartesian
 *   displacement, y = g' - g on the active coordinates, the same skips, symmetric bit for bit); then e', f' are taken into
 *   energies, forces, arc_lengths[c] grows by the arc increment, and the point is appended: path_coords[c][k] = coords,
 *   path_energies[c][k] = e', path_arcs[c][k] = arc_lengths[c] at k = n_points[c]++.  Then reason[c] = ANIHIP_IRC_MINIMUM when
 *   max over the free atoms of |f'_i| < fmax or the step was zero, else ANIHIP_IRC_PATH_FULL when n_points[c] == max_points.
 *
 * status int32 [C], OR-ed in and never cleared: ANIHIP_IRC_BAD_TABLE (a kind above 2, a bad mass), ANIHIP_IRC_NONFINITE (a
 * force, coordinate, Hessian row, eigenvalue, step or new energy that is not finite), ANIHIP_IRC_NO_ROOT (no bracket of t, or
 * the iteration did not reach the tolerance).  The entry that sets a bit in step or commit is left at its old coords.
 * workspace: anihip_irc_workspace_bytes(n_mol, atoms_per_mol) bytes, 256-byte aligned regions in this order:
 *   q, b fp64 [C][6][n] | gproj, w, displacement, xi fp64 [C][n] | old coords fp32 [C][n] | scalars fp64 [C][8]
 * kept between the three calls of a point; commit must follow a step on the same state.  project and commit are two launches
 * each (one workgroup of 256 threads per molecule, then a streaming pass over [C][n][n] by blocks of 16 rows), step is one; no
 * allocation, no atomics, every sum in a fixed order: bit-identical run to run.  Null pointers (direction excepted) and sizes
 * out of range return nonzero before any launch. */
#define ANIHIP_IRC_BAD_TABLE 1
#define ANIHIP_IRC_NONFINITE 2
#define ANIHIP_IRC_NO_ROOT 4
#define ANIHIP_IRC_MINIMUM 1
#define ANIHIP_IRC_ENERGY_ROSE 2
#define ANIHIP_IRC_PATH_FULL 3
typedef struct {
    int32_t n_mol, atoms_per_mol;
    int32_t periodic;   /* != 0: the rotations are not projected out */
    int32_t max_points; /* the capacity of the path of an entry */
    double step;        /* Angstrom amu^1/2: the arc length of a point */
    double fmax;        /* Hartree / Angstrom */
    double energy_floor;         /* Hartree */
    const uint8_t *kind;         /* [C][A] */
    const double *masses;        /* [C][A], amu */
    float *coords;               /* [C][A][3], moved in place */
    double *energies;            /* [C] */
    float *forces;               /* [C][A][3] */
    double *hessians;            /* [C][n][n], the Cartesian model Hessian */
    const double *direction;     /* [C][n] or NULL */
    float *last_step;            /* [C][A][3] */
    double *arc_lengths;         /* [C], cumulative */
    int32_t *n_points, *reason, *status; /* [C] */
    float *path_coords;          /* [C][max_points][A][3] */
    double *path_energies, *path_arcs;   /* [C][max_points] */
    void *workspace;
    size_t workspace_bytes;
} anihip_irc;
size_t anihip_irc_workspace_bytes(int64_t n_mol, int64_t atoms_per_mol);   /* 0 + anihip_last_error() */
int anihip_irc_project(void *stream, const anihip_irc *state, double *projected);
int anihip_irc_step(void *stream, const anihip_irc *state, const double *eigenvalues, const double *eigenvectors);
int anihip_irc_commit(void *stream, const anihip_irc *state, const double *new_energies, const float *new_forces,
                      int32_t bofill);

/* anihip_aev_backward plus the virial of the back-propagated scalar,
 *   virial[3a + b] = sum over central atoms lo <= i < hi and their neighbors j of (d E_i / d d_ij)[a] * d_ij[b]
 * (fp64 [9], OVERWRITTEN; d_ij = the displacement stored in the row): the reference's "fdotr" virial
 * (ase.py:164-168, dE/d(diff_vectors)^T @ diff_vectors), which under periodic boundary conditions equals the
 * derivative of the energy with respect to a strain of coordinates and cell (ase.py:170-173); stress = virial /
 * volume.  It needs neither the cell nor whole molecules, so shards / domains simply add their partial virials. */
int anihip_aev_backward_virial(void *stream, const anihip_aev_params *p, const float *table, int64_t n_atoms,
                               int64_t lo, int64_t hi, const int32_t *species, const uint32_t *meta,
                               const float *ent, const float *grad_aev, const uint32_t *slab_mask,
                               int32_t flags, float *grad_coords, double *virial, uint32_t *status);

/* The heat flux of a strictly local potential, E = sum_i E_i with E_i a function of the displacements of row i alone.  With
 * eps_i = 1/2 m_i |v_i|^2 + e_i, differentiating sum_i r_i eps_i along the equations of motion gives
 *   J = sum_i eps_i v_i - sum_i q_i,   q_i = sum_{j in row i} d_ij (g_ij . v_j),   g_ij = d E_i / d d_ij
 * (d_ij = the displacement stored in the row; the product does not depend on its sign convention, and no absolute position
 * enters, so it holds under periodic boundaries).  anihip_aev_backward_flux is the AEV backward with that contraction in place
 * of the scatter into forces: flux_atoms fp32 [n_atoms][3], the rows lo <= i < hi OVERWRITTEN with q_i (zero for an atom
 * without neighbors or with species < 0), every other row untouched; vectors fp32 [n_atoms][3] are gathered by neighbor index.
 * grad_aev is d (sum_i E_i) / d aev as for anihip_aev_backward.  Every term is evaluated as an own term of row i: flags and
 * slab_mask are accepted for the siblings' signature and not used (ANIHIP_BWD_SYMMETRIC would fold a neighbor's share, which
 * multiplies another vector, into the pair).  No global atomics and nothing pushed to other atoms.  On the 16 / 8x4 / 4x8 grids
 * every sum has a fixed order and two calls on the same input are bit-identical by construction.  On any other grid the general
 * kernel adds the angular terms of a row into LDS with float atomics of the one wave that owns the row, as its force variant
 * does: the order is the hardware's order of the lanes of one instruction, which was observed to repeat, not guaranteed to. */
int anihip_aev_backward_flux(void *stream, const anihip_aev_params *p, const float *table, int64_t n_atoms, int64_t lo,
                             int64_t hi, const int32_t *species, const uint32_t *meta, const float *ent,
                             const float *grad_aev, const uint32_t *slab_mask, int32_t flags, const float *vectors,
                             float *flux_atoms, uint32_t *status);

/* The three sums of J per entry: flux fp64 [C][3][3], OVERWRITTEN, in Hartree Angstrom / fs,
 *   flux[c][0] = sum_i 1/2 m_i |v_i|^2 v_i / ANIHIP_MD_ACC_UNIT   (kinetic convective)
 *   flux[c][1] = sum_i e_i v_i                                     (potential convective)
 *   flux[c][2] = - sum_i q_i                                       (virial term)
 * over the atoms with species >= 0.  masses fp32 [C][A] (amu), atomic_energies fp64 [C][A] (Hartree), species int32 [C][A],
 * velocities and flux_atoms fp32 [C][A][3].  fp64 sums in a fixed order, no atomics.  workspace:
 * anihip_md_heat_flux_workspace_bytes(n_mol, atoms_per_mol) bytes of scratch (needed for atoms_per_mol > 256). */
size_t anihip_md_heat_flux_workspace_bytes(int64_t n_mol, int64_t atoms_per_mol);   /* 0 + anihip_last_error() */
int anihip_md_heat_flux(void *stream, const anihip_md_params *params, const float *masses, const double *atomic_energies,
                        const int32_t *species, const float *velocities, const float *flux_atoms, double *flux,
                        void *workspace, size_t workspace_bytes);

/* The multistate Bennett acceptance ratio estimator (MBAR; binless WHAM is the same equations) on recorded series
 * (torchani_amd.md.MBAR; csrc/mbar.hip).  K thermodynamic states, N samples pooled from all of them, N_k of them drawn in state
 * k (N_k = 0: a state that was not sampled, a target).  In the STRUCTURED mode a state is an inverse temperature and one
 * restraint row per CV column, a sample its potential energy E_n and its CV values s_nr, and the reduced potential is
 *   u_k(x_n) = beta_k (E_n + sum_r 1/2 k_kr e^2),   e = max(0, |d| - hw_kr),   d = s_nr - c_kr
 * with d wrapped into [-pi, pi) for a column of kind ANIHIP_MD_CV_DIHEDRAL, the sum over r in ascending order from 0: the
 * restraint energy of anihip_md_bias_apply, operation for operation.  In the DENSE mode (u_kn not null) u_k(x_n) = u_kn[k][n].
 * The N x K matrix never exists in the structured mode.  The fields of the struct, device pointers unless marked HOST:
 *   n_samples (HOST) N >= 1;  n_states (HOST) K >= 1;  n_cvs (HOST) R in 0 .. ANIHIP_MD_BIAS_MAX_CVS
 *   beta       fp64 [K]        1 / Hartree                  n_k     fp64 [K]   counts >= 0, at least one > 0
 *   restraint  fp64 [K][R][3]  (center, k >= 0, half_width >= 0)       cv_kind int32 [R]  ANIHIP_MD_CV_*
 *   energy     fp64 [N] or NULL (zeros)                     cv      fp64 [N][R]
 *   u_kn       fp64 [K][N] or NULL; when given, beta, restraint, cv_kind, energy and cv are not read
 *   status     int32 [1]  OUT: 0, or ANIHIP_MBAR_BAD_* bits.  anihip_mbar_iterate and anihip_mbar_log_weights first check what
 *              they are about to read (every table, and the samples of the call) and rewrite status; a call that leaves it
 *              non-zero writes NOTHING else to its outputs.
 *
 * anihip_mbar_iterate runs n_iter >= 1 self-consistent iterations from f_in fp64 [K] without a host read, three launches
 * each, and leaves the last f in f_out fp64 [K] (may be f_in) and max_k |f' - f| of the last iteration in delta fp64 [1]:
 *   launch 1   d_n = lse over the states with N_j > 0 of (ln N_j + f_j - u_j(x_n)), for every n.  Two samples per thread; the
 *              state table is staged in LDS in tiles of at most 32 KB (sized from the LDS of a CU, not from K) and read by
 *              broadcast; one running (max, sum) pair per sample, one exp per (state, sample)
 *   launch 2   a workgroup owns the samples c S .. c S + S - 1 of chunk c, S = min(2048, 64 floor(6144 / (2 + R') / 64)) with R' = R rounded up to 0, 1, 2, 4, 8 or 16, staged in
 *              LDS; its waves deal the states, a wave holds a state's row in registers and walks the chunk twice: the
 *              maximum m of -u_k(x_n) - d_n, then the sum s of exp(. - m), lane l taking the samples l, l + 64, ... and the
 *              lanes reduced by xor butterflies.  (m, s) goes to workspace[c][k]
 *   launch 3   one workgroup: M_k = max_c m, f'_k = -(M_k + ln sum_c s exp(m - M_k)) with c ascending, then f'_k - f'_0
 * fp64 throughout, every log-sum-exp against a maximum, no floating-point atomics, every sum in a fixed order: two calls on
 * the same input give the same bits.
 *
 * anihip_mbar_log_weights with target = a state index, or ANIHIP_MBAR_TARGET_EXTERNAL and the state given as target_beta fp64 [1]
 * and target_restraint fp64 [R][3] (dense mode: its row target_u fp64 [N]): out fp64 [n_count] = -u_t(x_n) - d_n - ln Z for
 * n_first <= n < n_first + n_count, with d_n from f as in launch 1 and ln Z the log-sum-exp over ALL N samples (chunks of 1024,
 * combined in chunk order): the log-sum-exp of the N log weights is 0 whatever f.  With ANIHIP_MBAR_TARGET_ALL: out fp64
 * [n_count][K] = f_k - u_k(x_n) - d_n for every state, normalized when f is self-consistent; only the slab is evaluated (the
 * host accumulates W^T W over slabs).  workspace: anihip_mbar_workspace_bytes bytes (0 + anihip_last_error() for a bad problem),
 * the same for both.
 *
 * anihip_mbar_histogram: log weights fp64 [N] binned along one or two columns (HOST: columns, lo, hi, bins, one per column)
 * of cv fp64 [N][cv_stride].  A sample is in range when lo <= s < hi in every column, its bin min(bins - 1, (int)((s - lo) bins
 * / (hi - lo))), the first column the slow index; a NaN weight is out of range.  out fp64 [bins_0 bins_1] = lse of the log weights
 * of the bin (-inf when empty), counts int64 the samples per bin; both OVERWRITTEN.  Bin maxima by integer atomics on an
 * order-preserving key, then sums against them per chunk of samples, the chunks added in ascending order: the same bits at
 * every call.  At most ANIHIP_MBAR_MAX_BINS bins in all. */
#define ANIHIP_MBAR_BAD_COUNTS 1    /* a count that is negative or not finite, or no count above 0 */
#define ANIHIP_MBAR_BAD_SAMPLES 2   /* an energy, a CV value or a dense u that is not finite */
#define ANIHIP_MBAR_BAD_STATES 4    /* beta or a restraint row not finite, k or half_width < 0, a kind that is none of the three */
#define ANIHIP_MBAR_TARGET_EXTERNAL (-1)
#define ANIHIP_MBAR_TARGET_ALL (-2)
#define ANIHIP_MBAR_MAX_BINS 4096
typedef struct {
    int64_t n_samples;
    int32_t n_states, n_cvs;
    const double *beta, *n_k, *restraint;
    const int32_t *cv_kind;
    const double *energy, *cv, *u_kn;
    int32_t *status;
} anihip_mbar;
size_t anihip_mbar_workspace_bytes(const anihip_mbar *problem);
int anihip_mbar_iterate(void *stream, const anihip_mbar *problem, const double *f_in, int32_t n_iter, double *f_out,
                        double *delta, void *workspace, size_t workspace_bytes);
int anihip_mbar_log_weights(void *stream, const anihip_mbar *problem, const double *f, int32_t target, const double *target_beta,
                            const double *target_restraint, const double *target_u, int64_t n_first, int64_t n_count,
                            double *out, void *workspace, size_t workspace_bytes);
size_t anihip_mbar_histogram_workspace_bytes(int64_t n_samples, int32_t n_bins);
int anihip_mbar_histogram(void *stream, int64_t n_samples, const double *log_weights, const double *cv, int32_t cv_stride,
                          int32_t n_columns, const int32_t *columns, const double *lo, const double *hi, const int32_t *bins,
                          double *out, int64_t *counts, void *workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * Per-species MLP ensemble: replaces mnp::run (csrc/mnp.cpp:238-265; forward :32-136, input-gradient
 * backward :138-232) and BmmEnsemble (nn/_infer.py:61-216).
 *
 * Packed parameter layout (host code packs once per model, cf. BmmAtomicNetwork nn/_infer.py:141-161).
 * M = ensemble members, widths padded up to multiples of 32 with zeros (Hp):
 *   layer 0 : w [K0][M*H1p]  (column m*H1p+o = member m, unit o)   wt [M*H1p][K0p]  bias [M*H1p]
 *   layer l : w [M][Hlp][H(l+1)p]   wt [M][H(l+1)p][Hlp]   bias [M][H(l+1)p]      (hidden layers)
 *   final   : w [M][Hlastp]  bias [M]
 * K0 = AEV length (multiple of 16), K0p = K0 rounded up to a multiple of 32.
 *
 * Slab order of the layer-0 fp16 planes (desc.aev_radial_len = R > 0, needs (K0 - R) % 32 == 0): the AEV
 * index of wh[0] / wth[0] runs over [radial part zero-padded to a multiple of 32 | angular part], so that
 * every 32-deep slab holds whole species blocks of the AEV (two radial blocks or one angular block) and
 * K0p = 32 * (ceil(R/32) + (K0 - R)/32).  With R = 0 the planes are in plain AEV order.
 */
#define ANIHIP_MAX_LAYERS 4 /* Linear layers per network incl. the final one */
typedef struct {
    int32_t n_layers;                      /* Linear layers incl. final (ANI: 4) */
    int32_t dims[ANIHIP_MAX_LAYERS + 1];   /* padded widths: K0, H1p, H2p, H3p, 1 */
    const float *w[ANIHIP_MAX_LAYERS];     /* device pointers, layouts above */
    const float *wt[ANIHIP_MAX_LAYERS];    /* transposed copies (unused for the final layer) */
    const float *bias[ANIHIP_MAX_LAYERS];
    /* precision == ANIHIP_MLP_F16X3 only: the same hidden-layer matrices as two fp16 planes {hi, lo}
     * with hi + lo = w * wh_scale (power of two), stored [2][rows = output index][cols = reduction index]:
     * wh[l] has the shape of wt[l] (forward GEMMs), wth[l] the shape of w[l] (backward GEMMs; layer 0
     * padded to K0p rows).  Layer 0 uses the slab order described above when aev_radial_len > 0. */
    const void *wh[ANIHIP_MAX_LAYERS];
    const void *wth[ANIHIP_MAX_LAYERS];
    float wh_scale[ANIHIP_MAX_LAYERS];
    /* optional: the same planes re-ordered into MFMA fragment order
     * [member][N/32][K/16][2 planes][64 lanes][8 halves] (lane l <-> output n = 32 cb + (l & 31),
     * k = 16 ks + 8 (l >> 5) + j) for the fused network kernel, which streams them straight into
     * registers: whf[l] for layers 0..n_layers-2 (layer 0 per member: N = H1p, K = K0p in the order of
     * wh[0]), wthf[l] for layers 1..n_layers-2, and (4-layer networks) wthf[0] = layer 0 transposed, per member: N = K0p
     * in the order of wh[0] (a column block = one AEV slab), K = H1p -- the layer-0 backward inside the fused kernel.
     * whf / wthf[1..] NULL disables the fused kernel, wthf[0] NULL its layer-0 backward phase. */
    const void *whf[ANIHIP_MAX_LAYERS];
    const void *wthf[ANIHIP_MAX_LAYERS];
    /* optional, fused kernel of 4-layer networks: per member 8 floats ([5..7] = 0) that bound the operands
     * of the inner GEMMs so their fp16 split scales need no reduction over the tile:
     *   [0] max_j sum_k |W1[j][k]|   [1] max_j |b1[j]|   [2] max_j |w3[j]| / M
     *   [3] [2] * max_k sum_j |W2[j][k]|   [4] [3] * max_k sum_j |W1[j][k]|
     * (|act1| <= max|act0| * [0] + [1], |d act2| <= [2], |d act1| <= [3], |d act0| <= [4]).
     * NULL disables the fused kernel. */
    const float *fused_bounds;
} anihip_species_net;

/* GEMM arithmetic of the hidden layers.
 *   FP32  : v_mfma_f32_32x32x2_f32, exact fp32 products.
 *   F16X3 : every fp32 operand x is split on the fly into two fp16 numbers hi + lo = x * 2^e (e chosen per
 *           tensor from a device-side running max so nothing overflows); a product is evaluated as
 *           hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation: relative error
 *           ~4e-7 per product (fp32: 6e-8) at 16/3 of the fp32-MFMA rate.  Layer-0 inputs use the static
 *           scale 4, valid for |x| < 16376 -- above the largest value an AEV element can take with the
 *           row limits of this library (2 * C(128,2) = 16256). */
#define ANIHIP_ACT_CELU 0
#define ANIHIP_ACT_GELU 1
#define ANIHIP_MLP_FP32 0
#define ANIHIP_MLP_F16X3 1
/* anihip_mlp_desc.flags: algorithm choices of anihip_mlp_forward_backward that the library otherwise makes from the
 * problem size (tests and benchmarks pin them; results agree to rounding whatever is chosen) */
#define ANIHIP_MLP_FLAG_NO_FUSED 1u       /* layer-by-layer GEMMs instead of the fused network kernel */
#define ANIHIP_MLP_FLAG_BIG_TILES 2u      /* 256 x 256 layer-0 tiles (default from 16384 atoms) even for few atoms */
#define ANIHIP_MLP_FLAG_SMALL_TILES 4u    /* 128 x 128 layer-0 tiles whatever the size */
#define ANIHIP_MLP_FLAG_NO_SLAB_MASK 8u   /* ignore slab_mask: multiply every AEV slab */
/* (16, 64, 128, 256: development switches of rounds 1-4 -- 32-atom tiles, separate preparation launches, the 4-wave
 * layer-0 backward, tile-owner order without phase 5 -- retired in ABI 11; setting them changes nothing) */
#define ANIHIP_MLP_FLAG_D0_ROWS 32u       /* d E/d act0 handed to the layer-0 backward row-major, not tile-major */
#define ANIHIP_MLP_FLAG_FUSED_L0B 512u    /* layer-0 backward inside the fused kernel whatever the size (default: from 24000 atoms) */
#define ANIHIP_MLP_FLAG_NO_FUSED_L0B 1024u /* ... never: d E/d act0 through HBM + a layer-0 backward GEMM launch */
#define ANIHIP_MLP_FLAG_SHAPED 4096u       /* with the layer-0 backward inside the fused kernel: ONE LAUNCH PER SPECIES, restricted to its tiles, with the
                                             * network widths as compile-time constants where an instantiation exists (every ANI-2x network) -- 5-6 % faster
                                             * per tile.  Below four rounds of tiles these are plain launches on the caller's stream, each ending with a
                                             * partly filled last round of the CUs (a species of a handful of atoms still costs a tile through all members);
                                             * from four rounds on, IF THE CALLER HANDS OVER A SECOND STREAM in the descriptor (aux_stream, fork_event,
                                             * join_event below), the launches draw their tiles from a queue per species and alternate between the
                                             * caller's stream and that second one (forked from and joined to the caller's stream with the two
                                             * events, so the call stays stream-ordered for the caller).  Without the handles, and inside a stream
                                             * capture, the launches stay on the caller's stream in static tile order.  Whether it pays depends on the
                                             * composition: the Python host prices both schemes (models.ANI._per_species_launches_pay) -- 2.3 M-atom water box: yes; 46 k-atom solvated protein: no */
#define ANIHIP_MLP_FLAG_BWD_TWO_PRODUCTS 2048u /* OFF by default.  With the layer-0 backward inside the fused kernel (>= 24000 atoms,
                                                 * CELU): its backward GEMMs leave out (weight lo) x (gradient hi), i.e. use the weights
                                                 * rounded to fp16 -- energies unchanged, d E/d AEV and the forces differ from the default's
                                                 * by ~1e-6 Ha/A (inside the 1e-4 Ha/A gate of the parity tests, OUTSIDE their 5e-6 regression
                                                 * gate), a sixth fewer MFMAs */
typedef struct {
    int32_t num_species;
    int32_t n_members;
    int32_t aev_len;
    float celu_alpha;
    int32_t precision; /* ANIHIP_MLP_FP32 or ANIHIP_MLP_F16X3 */
    int32_t aev_radial_len; /* R of the slab order of wh[0] / wth[0] (0 = plain order) */
    int32_t flags;          /* ANIHIP_MLP_FLAG_* (0 = let the library choose); the library reads no environment */
    int32_t activation;     /* ANIHIP_ACT_CELU (celu_alpha) or ANIHIP_ACT_GELU (torch.nn.GELU(), exact; energies and
                             * input gradients through the fused network kernel only: 3 hidden layers <= 256 wide whose
                             * 64-atom tile fits the 160 KB of LDS: padded widths with H2 + max(H1, H3) <= 448.  256 / 192 / 256
                             * fits, 256 / 256 / 256 does not: a CELU pack with such a species runs layer by layer, all of it) */
    anihip_species_net net[ANIHIP_MAX_SPECIES];
    /* (ABI 13) second stream of the per-species launches (ANIHIP_MLP_FLAG_SHAPED) with the events that fork it from and
     * join it to the stream of the call: created and destroyed by the CALLER, on the device of the call; all three set
     * or all three NULL (NULL: every launch on the stream of the call; anihip_mlp_pack writes NULL).  aux_stream must
     * differ from the stream of the call.  Read by anihip_mlp_forward_backward only.  Like a workspace, the handles of
     * one descriptor may be in use by one call at a time: concurrent callers bring a set each.  Should the join fail after
     * the launches, the call waits for aux_stream on the host before it returns the error (the one place where a call
     * synchronises): no kernel of a failed call is left running that nothing orders before the caller's next step. */
    void *aux_stream; /* hipStream_t */
    void *fork_event; /* hipEvent_t */
    void *join_event; /* hipEvent_t */
} anihip_mlp_desc;

/* Packing a model behind the ABI (replaces what BmmEnsemble / MNPNetworks do at construction, nn/_infer.py:141-161,
 * 263-372: stacking the members' Linear parameters for the batched kernels; mnp::run takes them as Tensor lists,
 * csrc/mnp.cpp:238-248).  The caller describes the networks, asks for the buffer size, and hands over the parameters of
 * every (member m, species s, layer l) as torch.nn.Linear lays them out: weights[(m * S + s) * n_layers + l] -> float
 * [out][in] (in = aev_len for l = 0, else out_dims[s][l - 1]), biases[...] -> float [out]; device or host pointers.
 * anihip_mlp_pack fills out_buffer (device memory, or host memory with dst_on_device = 0 -- then nothing touches a GPU)
 * with every layout above -- fp32 arrays, transposed copies, {hi, lo} fp16 planes in slab order, MFMA fragment order,
 * fused_bounds -- and writes the descriptor whose pointers refer to out_buffer.  The buffer must stay alive and
 * unchanged while the descriptor is in use; the call synchronises the stream once (model load, not the hot path). */
typedef struct {
    int32_t n_members, num_species, n_layers;   /* n_layers = Linear layers per network incl. the final one (2..4) */
    int32_t aev_len;
    int32_t aev_radial_len; /* R of the slab order; -1: 16 S when aev_len has the ANI form 16 S + 32 S (S + 1) / 2, else 0 */
    int32_t precision;      /* ANIHIP_MLP_FP32 | ANIHIP_MLP_F16X3 */
    int32_t activation;     /* ANIHIP_ACT_CELU | ANIHIP_ACT_GELU */
    float celu_alpha;
    int32_t out_dims[ANIHIP_MAX_SPECIES][ANIHIP_MAX_LAYERS]; /* unpadded output width of every layer; the last is 1 */
} anihip_mlp_shape;
size_t anihip_mlp_pack_bytes(const anihip_mlp_shape *shape);   /* 0 + anihip_last_error() for a shape the kernels refuse */
int anihip_mlp_pack(void *stream, const anihip_mlp_shape *shape, const float *const *weights, const float *const *biases,
                    int32_t src_on_device, void *out_buffer, size_t out_bytes, int32_t dst_on_device,
                    anihip_mlp_desc *out_desc);

/* Workspace for n central atoms (activations of every hidden layer for all members, species-sorted
 * index lists): enough for every entry point below that takes a workspace. */
size_t anihip_mlp_workspace_bytes(const anihip_mlp_desc *d, int64_t n_central);
/* What ONE anihip_mlp_forward_backward call over n_central atoms with this descriptor (its flags included) touches
 * (ABI 10): the fused network kernel keeps the activations in LDS, so its calls need the index lists, the tile table and
 * the per-member energies (~100 B per atom) plus -- below 65536 atoms, where the layer-0 backward is a GEMM of its own --
 * d E / d act0 (8 KB per atom for ANI-2x); want_grad = (grad_aev != NULL).  Never more than anihip_mlp_workspace_bytes. */
size_t anihip_mlp_forward_backward_workspace_bytes(const anihip_mlp_desc *d, int64_t n_central, int32_t want_grad);

/* atomic_e[i] = mean over members of net_{m,species(i)}(aev[i]) for lo <= i < hi (0 for padding);
 * if grad_aev != NULL also grad_aev[i] = d atomic_e[i] / d aev[i] (rows of padding atoms zeroed).
 * member_e (optional) = [M, n_atoms] per-member energies (ensemble_values, nn/_containers.py:638-651).
 * slab_mask (optional; F16X3 with aev_radial_len > 0 only, otherwise ignored): the per-atom slab flags
 * written by anihip_aev_forward.  Slabs that no atom of a row tile flags are skipped in the layer-0
 * GEMMs (their AEV entries are exactly zero, so energies are unchanged); the matching entries of
 * grad_aev are then NOT written -- the caller must only consume grad_aev inside the flagged slabs
 * (anihip_aev_backward does) or pre-zero it. */
int anihip_mlp_forward_backward(void *stream, const anihip_mlp_desc *d, int64_t n_atoms, int64_t lo,
                                int64_t hi, const int32_t *species, const float *aev,
                                const uint32_t *slab_mask, void *workspace, size_t workspace_bytes,
                                float *atomic_e, float *grad_aev, float *member_e);

/* ---------------------------------------------------------------------------------------------
 * Training pass: gradients with respect to every weight and bias.  The reference gets them from torch autograd
 * through nn/_core.py:146-149 + nn/_containers.py:377-421,608-636 (its native MNP path has no weight gradients,
 * csrc/mnp.cpp:138-232); the loop this serves is tools/training-aev-benchmark.py:120-135 (BASELINE config 5).
 *
 * For  Loss = sum_i grad_atomic_e[i] * atomic_e[i]  (the caller folds d Loss / d E_molecule into per-atom factors;
 * atomic_e = ensemble mean as above):
 *   grads[s].gw[l]    = d Loss / d weight of layer l of species s as [M][out_p][in_p] (in_p = K0 for layer 0, [M][Hp]
 *                       for the output layer): per member torch.nn.Linear's [out][in] layout at the padded widths, so
 *                       unpadded networks (ANI-2x) read their gradients in place
 *   grads[s].gbias[l] = d Loss / d bias[l] of species s, same shape as bias[l]
 * (padded rows/columns come out zero).  The gradient arrays are OVERWRITTEN, or -- accumulate != 0 -- ADDED to (the caller
 * zeroes them: gradient accumulation over several calls, optimizers that own one flat gradient buffer).  atomic_e is written
 * as in anihip_mlp_forward_backward; grad_aev (optional) = d Loss / d aev rows, i.e. already scaled by grad_atomic_e.
 * Arithmetic, by descriptor (sums over atoms use float atomics either way: the last bits depend on the execution order):
 *   ANIHIP_MLP_FP32 (any shape, CELU or GELU): exact fp32 on v_mfma_f32_32x32x2_f32, layer by layer; only w / wt / bias are read.
 *   ANIHIP_MLP_F16X3, CELU, three hidden layers <= 256 wide with H2 + max(H1, H3) <= 448 (the fused kernel's LDS budget, see
 *     anihip_mlp_desc.activation; ANI-1x / ANI-2x) -- the FAST training path (round 5): the forward
 *     and the backward down to d e / d z0 run as ONE launch of the fused network kernel (split-fp16 MFMA, the arithmetic of
 *     inference: per-atom energies within 1e-7 Ha of fp64) for a unit upstream gradient, leaving activations and d e / d z in
 *     the workspace; the weight gradients dW_l = sum_atoms g_a (d e / d z_l)^T x_{l-1} are one launch per layer on
 *     v_mfma_f32_32x32x16_f16 with both operands split into two fp16 planes on the fly (three products: 2^-22 relative; the
 *     power-of-two operand scales come from fused_bounds, max |g_a| and the largest |act0| the forward recorded -- round 6), or,
 *     for a pack without fused_bounds, on v_mfma_f32_32x32x16_bf16 with three-way bf16 splits (six products, no scales); the
 *     bias gradients one column reduction per layer.  A call that asks for grad_aev takes the exact-fp32 backward instead (on
 *     the activations of whichever forward ran).
 * member_stride (fast path only; 0 = the packed [M][...] arrays above): gw[l] / gbias[l] point at MEMBER 0's arrays and
 * member m's lie member_stride floats further on each -- the layout of a flat parameter buffer in torch's parameter order
 * (member -> species -> layer -> weight, bias), so an optimizer that owns ONE flat gradient buffer receives the gradients
 * where its update kernel reads them (needs accumulate != 0 and unpadded widths).
 */
typedef struct {
    float *gw[ANIHIP_MAX_LAYERS];
    float *gbias[ANIHIP_MAX_LAYERS];
    int64_t member_stride;
    int32_t accumulate;
} anihip_species_grads;

size_t anihip_mlp_train_workspace_bytes(const anihip_mlp_desc *d, int64_t n_central);
/* 1 if the training passes of this descriptor take the FAST path above, else 0 (also for a NULL or invalid descriptor): the
 * library's own rule -- ANIHIP_MLP_F16X3, CELU, the shape the fused network kernel covers (the test anihip_mlp_forward_backward
 * applies before its flags: depth, widths and LDS budget, at most 32 AEV slabs, every fragment-ordered plane and fused_bounds
 * present).  Reads the descriptor only and makes no device call: valid for a descriptor packed into host memory.  A caller that
 * refreshes only the fused layouts of a pack (anihip_mlp_repack, ANIHIP_REPACK_FUSED_ONLY) asks this before it lets a pass read them. */
int anihip_mlp_fast_training(const anihip_mlp_desc *d);
int anihip_mlp_weight_grads(void *stream, const anihip_mlp_desc *d, int64_t n_atoms, int64_t lo, int64_t hi,
                            const int32_t *species, const float *aev, const float *grad_atomic_e,
                            void *workspace, size_t workspace_bytes, const anihip_species_grads *grads /* [num_species] */,
                            float *atomic_e, float *grad_aev, int32_t forward_done);

/* The two halves of a training step as autograd needs them (forward now, backward later): the forward that leaves the
 * species buckets and every hidden activation (fast path: also d e / d z of every layer) in the workspace
 * (anihip_mlp_train_workspace_bytes), writing atomic_e -- exact fp32 layer by layer, or the fused split-fp16 kernel, by
 * descriptor as above.  A later anihip_mlp_weight_grads call with forward_done != 0 and the SAME descriptor, range,
 * species, aev and (untouched) workspace skips its own forward. */
int anihip_mlp_train_forward(void *stream, const anihip_mlp_desc *d, int64_t n_atoms, int64_t lo, int64_t hi,
                             const int32_t *species, const float *aev, void *workspace, size_t workspace_bytes,
                             float *atomic_e);

/* Second-order pass for training on forces.  For per-atom tangents (tangent: [n_atoms][aev_len]) let
 *     S = sum_i tangent[i] . d atomic_e[i] / d aev[i]
 * (with tangent = -J t, J t from anihip_aev_jvp, S = sum_k t_k . F_k for the forces F = -dE/dr: the part of a force
 * loss that the reference back-propagates through torch.autograd.grad(E, coords, create_graph=True),
 * tools/training-aev-benchmark.py:136-150).  grads = d S / d (weights, biases) in the layouts of
 * anihip_mlp_weight_grads (OVERWRITTEN); datomic_e[i] = tangent[i] . d atomic_e[i] / d aev[i] (the directional
 * derivative of the energies; entries of padding atoms zeroed).  Exact fp32: forward-over-reverse with the
 * activations a_l, their tangents and both adjoint streams kept in the workspace. */
size_t anihip_mlp_tangent_workspace_bytes(const anihip_mlp_desc *d, int64_t n_central);
int anihip_mlp_tangent_weight_grads(void *stream, const anihip_mlp_desc *d, int64_t n_atoms, int64_t lo, int64_t hi,
                                    const int32_t *species, const float *aev, const float *tangent,
                                    void *workspace, size_t workspace_bytes, const anihip_species_grads *grads,
                                    float *datomic_e);

/* Input-space Hessian-vector products of the ensemble-mean atomic energies, for Hessians with respect to the coordinates:
 *   out[k][i] = (1/M) sum_m H_m(aev[i]) . tangent[k][i],   H_m(x) = d^2 e_m / d aev^2 at x,
 * for n_dir directions k and every atom i (tangent, out: [n_dir][n_atoms][aev_len]; rows of padding atoms zeroed).  It is the
 * input gradient of S = tangent . d e / d aev: the tangent pass of anihip_mlp_tangent_weight_grads over the (direction, atom)
 * rows, without the weight gradients, plus the layer-0 input adjoint.  The forward activations are computed once per atom and
 * gathered per row.  Exact fp32; reads the fp32 arrays (w, wt) of any pack, ANIHIP_MLP_F16X3 packs included.
 * n_atoms * n_dir < 2^31. */
size_t anihip_mlp_input_hvp_workspace_bytes(const anihip_mlp_desc *d, int64_t n_atoms, int64_t n_dir);
int anihip_mlp_input_hvp(void *stream, const anihip_mlp_desc *d, int64_t n_atoms, const int32_t *species, const float *aev,
                         int64_t n_dir, const float *tangent, void *workspace, size_t workspace_bytes, float *out);

/* anihip_mlp_input_hvp over explicit rows (block-sparse Hessians): out[q] = (1/M) sum_m H_m(aev[row_atom[q]]) . tangent[q]
 * (tangent, out: [n_rows][aev_len]).  The rows must be ordered so that the rows of a species are contiguous, species
 * ascending (anihip_hess_sparse_items).  anihip_mlp_rows_hvp_prepare runs the exact-fp32 forward over the atoms once and
 * keeps the activations in the workspace; anihip_mlp_rows_hvp then serves any number of row sets of at most n_rows rows
 * (the workspace size of the largest) from the same workspace.  n_rows < 2^31. */
size_t anihip_mlp_rows_hvp_workspace_bytes(const anihip_mlp_desc *d, int64_t n_atoms, int64_t n_rows);
int anihip_mlp_rows_hvp_prepare(void *stream, const anihip_mlp_desc *d, int64_t n_atoms, const int32_t *species,
                                const float *aev, void *workspace, size_t workspace_bytes);
int anihip_mlp_rows_hvp(void *stream, const anihip_mlp_desc *d, int64_t n_atoms, const int32_t *species, int64_t n_rows,
                        const int32_t *row_atom, const float *tangent, void *workspace, size_t workspace_bytes, float *out);

/* Refresh the packed parameter arrays of a descriptor IN PLACE (padding stays zero) from the torch.nn.Linear tensors after
 * an optimizer step -- one or two launches instead of re-packing on the host (cf. BmmAtomicNetwork packing once per model,
 * nn/_infer.py:141-161).  ANIHIP_MLP_FP32: w / wt / bias.  ANIHIP_MLP_F16X3 (round 5): every layout anihip_mlp_pack derives
 * -- w / wt / bias, the {hi, lo} fp16 planes wh / wth, their fragment orders whf / wthf, fused_bounds -- with the
 * power-of-two weight scales the pack was built with (wh_scale is not changed): should a weight have outgrown the fp16
 * range of its layer's scale, bit 0 of *status (device int32, optional, never cleared here) is set and the caller packs
 * again on the host.
 * src: DEVICE array of 2 * M * S * n_layers pointers ordered member, species, layer, {weight [out][in] row-major,
 * bias [out]}; out_in: HOST array [S][n_layers][2] with the (out, in) widths of the source tensors. */
#define ANIHIP_REPACK_FUSED_ONLY 1   /* F16X3: only what the fused network kernel and the fast training pass read -- bias, output
                                        layer, whf, wthf of the hidden layers, fused_bounds; w / wt / wh / wth / wthf[0] go stale */
int anihip_mlp_repack(void *stream, const anihip_mlp_desc *d, const void *const *src, const int32_t *out_in,
                      int32_t *status, int32_t flags);

/* One Adam update over flat buffers (torch.optim.Adam with amsgrad = False, maximize = False: the optimizer of the
 * reference's training recipe, tools/training-aev-benchmark.py:88; weight_decay is torch's L2 form, grad += wd * param):
 *   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  param -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * with t = *step + 1; *step (DEVICE int32: updates done so far) is incremented behind the update, so a captured HIP graph
 * of a training step advances it on every replay.  One launch over n parameters (28 bytes of traffic each) instead of a
 * dozen foreach launches over the model's 448 tensors; buffers 16-byte aligned.  zero_grads != 0: the gradients are zeroed
 * behind the update (the weight-gradient kernels of the next step ADD into them: no memset launch per step).
 * The hyper-parameters are doubles (ABI 12), as torch.optim.Adam holds them: 1 - beta2 taken from the fp32-rounded 0.999 is
 * 1.3e-5 off, and exp_avg_sq then differs from torch's by that factor. */
int anihip_adam_step(void *stream, float *params, float *grads, float *exp_avg, float *exp_avg_sq, int64_t n,
                     double lr, double beta1, double beta2, double eps, double weight_decay, int32_t *step, int32_t zero_grads);

/* ---------------------------------------------------------------------------------------------
 * Pair potentials on the neighbor rows: the xTB repulsion term of the reference's ANI-2xr / ANI-2dr models
 * (potentials/xtb.py:17-77 RepulsionXTB, envelope and per-atom halves of potentials/core.py:155-207):
 *   e_ij = y_ab / d * exp(-sqrt(alpha_ab) d^k_ab) * fc(r_ij, cutoff),  d = r_ij in Bohr (r clamped to >= 1e-7 A);
 * pair_table: device float[8][8][4] = {y_ab, sqrt(alpha_ab), k_ab, 0} indexed [species_i][species_j].
 * atomic_e[i] += sum_j e_ij / 2 for lo <= i < hi (may be NULL); grad_coords [n_atoms][3] += d(sum of those) / d r (may be
 * NULL); virial [9] fp64 += sum (dE_i / d d_ij) (x) d_ij (may be NULL).  cutoff must not exceed the radial cutoff the rows
 * were built with.  Symmetric rows (every builder except anihip_nbr_from_full): no atomics, each atom completes its own
 * entries, deterministic; pass ANIHIP_PAIR_PUSH for asymmetric rows. */
#define ANIHIP_PAIR_PUSH 1
int anihip_pair_xtb_repulsion(void *stream, int64_t n_atoms, int64_t lo, int64_t hi, const int32_t *species,
                              const uint32_t *meta, const float *ent, const float *pair_table, float cutoff,
                              int32_t cutoff_kind, int32_t flags, float *atomic_e, float *grad_coords, double *virial);

/* The other closed-form pair potentials of torchani.potentials on the same rows, same outputs and flags; pair_table:
 * device float[8][8][4] per [species_i][species_j]; distances d in Bohr, r in Angstrom (r clamped to >= 1e-7 A unless
 * ANIHIP_PAIR_NO_CLAMP, core.py:138-139):
 *   ANIHIP_PAIR_XTB      {y_ab, sqrt(alpha_ab), k_ab, -}        y / d exp(-sqrt(alpha) d^k)              (xtb.py:17-77)
 *   ANIHIP_PAIR_ZBL      {Za Zb, (Za^kz + Zb^kz) / k, -, -}     Za Zb / d sum_i c_i exp(-b_i d s)        (zbl.py:10-81)
 *                        extra: float[8] = c_0..3, b_0..3 (host memory)
 *   ANIHIP_PAIR_LJ       {4 eps_ab, sigma_ab, c12, c6}          4 eps (c12 x^12 + c6 x^6), x = sigma / r (lj.py:42-108)
 *   ANIHIP_PAIR_COULOMB  {q_a q_b / dielectric, 1 / eta_ab, -, -}   qq / sqrt(d^2 + 1 / eta^2)   (fixed_coulomb.py:8-75;
 *                        1 / eta = 0: FixedCoulomb, clamped; FixedMNOK: 2 / (eta_a + eta_b), ANIHIP_PAIR_NO_CLAMP) */
#define ANIHIP_PAIR_XTB 0
#define ANIHIP_PAIR_ZBL 1
#define ANIHIP_PAIR_LJ 2
#define ANIHIP_PAIR_COULOMB 3
#define ANIHIP_PAIR_NO_CLAMP 2
int anihip_pair_analytic(void *stream, int32_t kind, int64_t n_atoms, int64_t lo, int64_t hi, const int32_t *species,
                         const uint32_t *meta, const float *ent, const float *pair_table, const float *extra,
                         float cutoff, int32_t cutoff_kind, int32_t flags, float *atomic_e, float *grad_coords,
                         double *virial);

/* Hessian-vector products of anihip_pair_analytic's energy, for Hessians with respect to the coordinates: for n_dir
 * directions t[k],  out[k] += H t[k]  over the central atoms lo <= i < hi, with H = d^2 E / d coords^2 of the pair energies
 * of those rows.  Same kind, rows, pair_table, extra, cutoff, cutoff_kind and ANIHIP_PAIR_NO_CLAMP as anihip_pair_analytic;
 * tangent and out are device float [n_dir][n_atoms][3].  Per pair, with d = r_j - r_i, r = |d|, u = d / r and
 * e(r) = base(r) fc(r):  (H t)_i = sum_{j in row i} (e''(r) u u^T + e'(r) / r (I - u u^T)) (t_i - t_j)  -- a periodic
 * image of atom i itself contributes nothing.  Symmetric rows only (ANIHIP_PAIR_PUSH is refused); no atomics,
 * deterministic. */
int anihip_pair_analytic_hvp(void *stream, int32_t kind, int64_t n_atoms, int64_t lo, int64_t hi, const int32_t *species,
                             const uint32_t *meta, const float *ent, const float *pair_table, const float *extra,
                             float cutoff, int32_t cutoff_kind, int32_t flags, int64_t n_dir, const float *tangent,
                             float *out);

/* anihip_pair_analytic_hvp over item rows (block-sparse Hessians): out[row_dir[q] - dir0][i] += (H t)_i for the central atom
 * i = row_atom[q] and the unit tangent t of row_dir[q] (out [n_dir][n_atoms][3]; an item row names each (direction, atom)
 * once: no atomics).  The pair cutoff must not exceed the radial cutoff the rows were built with; rows whose slab falls
 * outside 0 .. n_dir are skipped. */
int anihip_pair_analytic_hvp_items(void *stream, int32_t kind, int64_t n_atoms, const int32_t *species, const uint32_t *meta,
                                   const float *ent, const float *pair_table, const float *extra, float cutoff,
                                   int32_t cutoff_kind, int32_t flags, int64_t n_rows, const int32_t *row_atom,
                                   const int32_t *row_dir, int64_t dir0, int64_t n_dir, float *out);

/* DFT-D3(BJ) two-body dispersion (potentials/dftd3.py:113-330 TwoBodyDispersionD3, damping :44-110 BeckeJohnsonDamp;
 * envelope and per-atom halves as above), distances in Bohr:
 *   CN_i   = sum_j 1 / (1 + exp(-16 (4/3 (Rcov_a + Rcov_b) / d_ij - 1)))                     (all neighbors of the row)
 *   C6_ij  = sum_ref c6ref L / sum_ref L,  L = exp(-4 ((CN_i - cn_a)^2 + (CN_j - cn_b)^2)) over the references with c6ref > 0
 *   e_ij   = -(s6 C6 / (d^6 + R^6) + s8 3 C6 q_a q_b / (d^8 + R^8)) fc(r_ij),  R = a1 sqrt(3 q_a q_b) + a2
 * c6_table: device float[8][8][25][4] = {c6ref, cn_a, cn_b, -} per [species_i][species_j]: the reference pairs with
 * c6ref > 0 first (any order), their number in the 4th float of entry 0 (missing references are -1 in Grimme's table).
 * The rows must hold ALL atoms 0 .. n_atoms (coordination numbers of every neighbor are needed) and be symmetric;
 * lo / hi select the central atoms whose energies / gradient rows are accumulated (atomic_e[i] += sum_j e_ij / 2,
 * grad_coords[i] += d E / d r_i, both complete for i in lo .. hi: nothing is pushed to other atoms, no atomics,
 * deterministic).  The gradient includes the dependence of C6 on the coordination numbers (the reference gets it from
 * autograd).  cn, gcn: caller-provided scratch, n_atoms floats each.  virial as above (may be NULL);
 * it includes the coordination-number term whether or not grad_coords is given. */
typedef struct anihip_d3_params {
    float s6, s8, a1, a2;
    float cov_radius_bohr[8];   /* per species index */
    float sqrt_q[8];            /* sqrt of the empirical charge, per species index */
} anihip_d3_params;
int anihip_pair_d3(void *stream, int64_t n_atoms, int64_t lo, int64_t hi, const int32_t *species,
                   const uint32_t *meta, const float *ent, const float *c6_table, const anihip_d3_params *params,
                   float cutoff, int32_t cutoff_kind, float *cn, float *gcn, float *atomic_e, float *grad_coords,
                   double *virial);

/* mol_e[c] (fp64) = sum_a atomic_e[c,a] + sae[species[c,a]] over the atoms lo <= c*A+a < hi; padding
 * contributes nothing (sae.py:54-64).  sae may be NULL.  mol_e is overwritten. */
int anihip_energy_reduce(void *stream, int32_t n_mol, int32_t n_atoms_per_mol, int64_t lo, int64_t hi,
                         const int32_t *species, const float *atomic_e, const double *sae, double *mol_e);

/* The last launch of an energies-and-forces step: anihip_energy_reduce, and grad_coords[0 .. n_grad) (the d E / d coords
 * that anihip_aev_backward and the pair terms accumulated) negated in place into forces (grad.py:283-290); one launch for
 * batches of small molecules, where a step is bound by the number of launches. */
int anihip_energy_forces_finish(void *stream, int32_t n_mol, int32_t n_atoms_per_mol, int64_t lo, int64_t hi,
                                const int32_t *species, const float *atomic_e, const double *sae, double *mol_e,
                                float *grad_coords, int64_t n_grad);

#ifdef __cplusplus
}
#endif
#endif /* ANIHIP_H */
