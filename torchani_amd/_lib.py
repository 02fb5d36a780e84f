"""Loader and ctypes prototypes of libanihip.so (the C ABI declared in include/anihip.h).

The product path has NO CPU fallback: if the library is missing or there is no GPU the calls raise.
``build()`` compiles the HIP sources in-tree with plain ``hipcc --offload-arch=gfx950`` (no hipify, no
torch cpp_extension), so the resulting .so travels with the repository snapshot to the GPU box.
"""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import typing as tp

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TORCHANI_AMD_LIB") or os.path.join(_HERE, "libanihip.so")
SOURCES = ["api.hip", "nbr.hip", "aev.hip", "aev_generic.hip", "aev_hess.hip", "mlp.hip", "mlp_fused.hip", "mlp_prep.hip", "pair.hip", "pack.hip", "train.hip", "hess_sparse.hip", "hess_modes.hip", "lbfgs.hip", "md.hip", "md_bias.hip", "md_sites.hip", "md_observe.hip", "geom_constraints.hip", "saddle.hip", "irc.hip", "phonons.hip", "mbar.hip"]
HEADERS = ["anihip_common.h", "aev_gen.h", "hess_rows.h", "train.h", "mlp_fused.h", "mlp_prep.h", "md_sums.h", "md_cv.h", "saddle_common.h", os.path.join("..", "..", "include", "anihip.h")]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-fPIC", "-shared"]

MAX_SPECIES = 8
MAX_LAYERS = 4
META_WORDS = 6
STATUS_WORDS = 8
MAX_ANG = 128
MAX_RAD = 256
TABLE_FLOATS = 144
ST_ENTRY_OVERFLOW, ST_ROW_OVERFLOW, ST_GRID_OVERFLOW = 1, 2, 4
MLP_FP32, MLP_F16X3 = 0, 1
BWD_SYMMETRIC, BWD_FIXED_POINT = 1, 2   # flags of anihip_aev_backward
PAIR_PUSH = 1
PAIR_NO_CLAMP = 2
PAIR_XTB, PAIR_ZBL, PAIR_LJ, PAIR_COULOMB = 0, 1, 2, 3
ACT_CELU, ACT_GELU = 0, 1
# anihip_mlp_desc.flags (ANIHIP_MLP_FLAG_*)
MLP_FLAG_NO_FUSED, MLP_FLAG_BIG_TILES, MLP_FLAG_SMALL_TILES, MLP_FLAG_NO_SLAB_MASK, MLP_FLAG_D0_ROWS = 1, 2, 4, 8, 32
MLP_FLAG_FUSED_L0B, MLP_FLAG_NO_FUSED_L0B = 512, 1024
MLP_FLAG_SHAPED = 4096   # one fused launch per species with compile-time network widths (include/anihip.h)
MLP_FLAG_BWD_TWO_PRODUCTS = 2048   # off by default: two-product backward GEMMs of the large-system path (include/anihip.h)
ABI_VERSION = 13
REPACK_FUSED_ONLY = 1
BLOCK_HESSIAN_MAX_VECTORS = 64   # ANIHIP_BLOCK_HESSIAN_MAX_VECTORS
BLOCK_HESSIAN_BAD_INDEX, BLOCK_HESSIAN_NO_PARTNER, BLOCK_HESSIAN_NO_DIAGONAL = 1, 2, 4
LBFGS_MAX_MEMORY = 256   # ANIHIP_LBFGS_MAX_MEMORY
MD_LANGEVIN = 1   # ANIHIP_MD_LANGEVIN
MD_ATOM_CLUSTER, MD_CLUSTER_ATOMS, MD_CLUSTER_BONDS = 2, 8, 12   # ANIHIP_MD_ATOM_CLUSTER, ANIHIP_MD_CLUSTER_*
MD_BAROSTAT_STEP = 1 << 62   # ANIHIP_MD_BAROSTAT_STEP
MD_HBAR = 0.024188843265857   # ANIHIP_MD_HBAR, Hartree fs
MD_RP_MAX_BEADS = 64   # ANIHIP_MD_RP_MAX_BEADS
MD_EXCHANGE_STEP = 1 << 61   # ANIHIP_MD_EXCHANGE_STEP
MD_LADDERS_CHECK = 1   # ANIHIP_MD_LADDERS_CHECK
MD_BIAS_MAX_CVS = 16   # ANIHIP_MD_BIAS_MAX_CVS
MD_BIAS_CHUNK = 1024   # ANIHIP_MD_BIAS_CHUNK: hills per workgroup of the hills kernel
MD_CV_DISTANCE, MD_CV_ANGLE, MD_CV_DIHEDRAL = 0, 1, 2   # ANIHIP_MD_CV_*
MD_BIAS_BAD_OFFSET, MD_BIAS_BAD_CV, MD_BIAS_BAD_LIST = 1, 2, 4   # ANIHIP_MD_BIAS_BAD_*
MD_SITES_MAX = 64   # ANIHIP_MD_SITES_MAX
MD_SITE_NONE, MD_SITE_CENTER, MD_SITE_ANCHOR, MD_SITE_VALUE = 0, 1, 2, 3   # ANIHIP_MD_SITE_*
MD_SITE_ROLE_CENTER, MD_SITE_ROLE_A, MD_SITE_ROLE_B = 0, 1, 2   # ANIHIP_MD_SITE_ROLE_*
MD_SITES_BAD_SITE, MD_SITES_BAD_GROUP, MD_SITES_BAD_MEMBER = 1, 2, 4   # ANIHIP_MD_SITES_BAD_*
MD_CORR_MSD, MD_CORR_VACF = 0, 1   # ANIHIP_MD_CORR_*
MD_RDF_MAX_PAIRS, MD_RDF_MAX_BINS = 8, 1024   # ANIHIP_MD_RDF_MAX_*
GEOM_MAX_CONSTRAINTS = 8   # ANIHIP_GEOM_MAX_CONSTRAINTS
GEOM_BAD_TABLE, GEOM_SINGULAR, GEOM_NOT_CONVERGED = 1, 2, 4   # ANIHIP_GEOM_*
SADDLE_MAX_COORDS = 768   # ANIHIP_SADDLE_MAX_COORDS
SADDLE_BAD_TABLE, SADDLE_NONFINITE, SADDLE_NO_BRACKET = 1, 2, 4   # ANIHIP_SADDLE_*
IRC_BAD_TABLE, IRC_NONFINITE, IRC_NO_ROOT = 1, 2, 4   # ANIHIP_IRC_* (status bits)
IRC_RUNNING, IRC_MINIMUM, IRC_ENERGY_ROSE, IRC_PATH_FULL = 0, 1, 2, 3   # ANIHIP_IRC_* (reasons; 0: not done)
MBAR_BAD_COUNTS, MBAR_BAD_SAMPLES, MBAR_BAD_STATES = 1, 2, 4   # ANIHIP_MBAR_BAD_*
MBAR_TARGET_EXTERNAL, MBAR_TARGET_ALL = -1, -2   # ANIHIP_MBAR_TARGET_*
MBAR_MAX_BINS = 4096   # ANIHIP_MBAR_MAX_BINS


def md_group_scratch_bytes(n_mol: int, atoms_per_mol: int) -> int:
    """ANIHIP_MD_GROUP_SCRATCH_BYTES: the scratch of anihip_md_group_terms."""
    return n_mol * (atoms_per_mol + (atoms_per_mol + 255) // 256) * 2 * 8


class AevParams(C.Structure):
    _fields_ = [
        ("num_species", C.c_int32),
        ("n_shf_r", C.c_int32),
        ("n_shf_a", C.c_int32),
        ("n_shf_z", C.c_int32),
        ("Rcr", C.c_float),
        ("Rca", C.c_float),
        ("EtaR", C.c_float),
        ("EtaA", C.c_float),
        ("Zeta", C.c_float),
        ("cutoff_kind", C.c_int32),
        ("flags", C.c_int32),   # ANIHIP_AEV_*: set by anihip_aev_table_pack
    ]


CUTOFF_KINDS = {"cosine": 0, "smooth": 1}  # ANIHIP_CUTOFF_*


class SpeciesNet(C.Structure):
    _fields_ = [
        ("n_layers", C.c_int32),
        ("dims", C.c_int32 * (MAX_LAYERS + 1)),
        ("w", C.c_void_p * MAX_LAYERS),
        ("wt", C.c_void_p * MAX_LAYERS),
        ("bias", C.c_void_p * MAX_LAYERS),
        ("wh", C.c_void_p * MAX_LAYERS),
        ("wth", C.c_void_p * MAX_LAYERS),
        ("wh_scale", C.c_float * MAX_LAYERS),
        ("whf", C.c_void_p * MAX_LAYERS),
        ("wthf", C.c_void_p * MAX_LAYERS),
        ("fused_bounds", C.c_void_p),
    ]


class SpeciesGrads(C.Structure):
    _fields_ = [
        ("gw", C.c_void_p * MAX_LAYERS),
        ("gbias", C.c_void_p * MAX_LAYERS),
        ("member_stride", C.c_int64),
        ("accumulate", C.c_int32),
    ]


class D3Params(C.Structure):
    """anihip_d3_params (include/anihip.h)."""
    _fields_ = [("s6", C.c_float), ("s8", C.c_float), ("a1", C.c_float), ("a2", C.c_float),
                ("cov_radius_bohr", C.c_float * 8), ("sqrt_q", C.c_float * 8)]


class MlpDesc(C.Structure):
    _fields_ = [
        ("num_species", C.c_int32),
        ("n_members", C.c_int32),
        ("aev_len", C.c_int32),
        ("celu_alpha", C.c_float),
        ("precision", C.c_int32),
        ("aev_radial_len", C.c_int32),
        ("flags", C.c_int32),
        ("activation", C.c_int32),
        ("net", SpeciesNet * MAX_SPECIES),
        ("aux_stream", C.c_void_p),   # hipStream_t / hipEvent_t of the caller (NULL: none), see include/anihip.h
        ("fork_event", C.c_void_p),
        ("join_event", C.c_void_p),
    ]


class LbfgsParams(C.Structure):
    """anihip_lbfgs_params (include/anihip.h)."""
    _fields_ = [("n_mol", C.c_int32), ("atoms_per_mol", C.c_int32), ("memory", C.c_int32), ("flags", C.c_int32),
                ("inv_alpha", C.c_double), ("maxstep", C.c_double), ("damping", C.c_double), ("fmax", C.c_double)]


class MdParams(C.Structure):
    """anihip_md_params (include/anihip.h)."""
    _fields_ = [("n_mol", C.c_int32), ("atoms_per_mol", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
                ("dt", C.c_double), ("seed", C.c_uint64), ("step", C.c_uint64)]


class MdClusters(C.Structure):
    """anihip_md_clusters (include/anihip.h)."""
    _fields_ = [("n_clusters", C.c_int64), ("atoms", C.c_void_p), ("count", C.c_void_p), ("bonds", C.c_void_p),
                ("d2", C.c_void_p), ("w", C.c_void_p), ("iterations", C.c_void_p), ("tolerance", C.c_double),
                ("max_iterations", C.c_int32), ("max_atoms", C.c_int32), ("max_bonds", C.c_int32), ("reserved", C.c_int32)]


class MdLadders(C.Structure):
    """anihip_md_ladders (include/anihip.h)."""
    _fields_ = [("n_ladders", C.c_int32), ("max_rungs", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
                ("slot", C.c_void_p), ("count", C.c_void_p), ("rung_of", C.c_void_p), ("rung_kT", C.c_void_p),
                ("ladder_ids", C.c_void_p), ("attempts", C.c_void_p), ("accepts", C.c_void_p), ("direction", C.c_void_p),
                ("round_trips", C.c_void_p), ("scale", C.c_void_p)]


class MdBias(C.Structure):
    """anihip_md_bias (include/anihip.h)."""
    _fields_ = [("n_cvs", C.c_int32), ("n_lists", C.c_int32), ("capacity", C.c_int32), ("hills_bound", C.c_int32),
                ("reserved", C.c_int32), ("n_entries", C.c_int32),
                ("cv_offset", C.c_void_p), ("kind", C.c_void_p), ("atoms", C.c_void_p), ("restraint", C.c_void_p),
                ("meta_cv", C.c_void_p), ("inv_sigma2", C.c_void_p), ("height", C.c_void_p), ("list", C.c_void_p),
                ("rank_in_list", C.c_void_p), ("members", C.c_void_p), ("list_entry", C.c_void_p), ("bias_factor", C.c_void_p),
                ("used", C.c_void_p), ("dropped", C.c_void_p), ("centers", C.c_void_p), ("heights", C.c_void_p),
                ("status", C.c_void_p)]


class MdSites(C.Structure):
    """anihip_md_sites (include/anihip.h)."""
    _fields_ = [("n_entries", C.c_int32), ("max_sites", C.c_int32), ("n_groups", C.c_int32), ("n_group_atoms", C.c_int32),
                ("n_coord", C.c_int32), ("n_members", C.c_int32), ("pbc", C.c_int32 * 3), ("reserved", C.c_int32),
                ("cell", C.c_double * 9), ("inv_cell", C.c_double * 9),
                ("site_kind", C.c_void_p), ("site_ref", C.c_void_p), ("group_offset", C.c_void_p), ("group_atoms", C.c_void_p),
                ("group_weights", C.c_void_p), ("coord", C.c_void_p), ("coord_params", C.c_void_p),
                ("member_offset", C.c_void_p), ("member_site", C.c_void_p), ("member_weight", C.c_void_p),
                ("status", C.c_void_p)]


class GeomConstraints(C.Structure):
    """anihip_geom_constraints (include/anihip.h)."""
    _fields_ = [("n_constraints", C.c_int32), ("max_iterations", C.c_int32), ("tolerance", C.c_double),
                ("offset", C.c_void_p), ("kind", C.c_void_p), ("atoms", C.c_void_p), ("target", C.c_void_p),
                ("values", C.c_void_p), ("multipliers", C.c_void_p), ("iterations", C.c_void_p), ("status", C.c_void_p)]


class Saddle(C.Structure):
    """anihip_saddle (include/anihip.h)."""
    _fields_ = [("n_mol", C.c_int32), ("atoms_per_mol", C.c_int32), ("periodic", C.c_int32), ("follow", C.c_int32),
                ("fmax", C.c_double), ("max_trust", C.c_double), ("min_trust", C.c_double), ("energy_floor", C.c_double),
                ("kind", C.c_void_p), ("coords", C.c_void_p), ("energies", C.c_void_p), ("forces", C.c_void_p),
                ("hessians", C.c_void_p), ("trust_radii", C.c_void_p), ("eigenvalues", C.c_void_p), ("modes", C.c_void_p),
                ("last_step", C.c_void_p), ("accepted", C.c_void_p), ("converged", C.c_void_p), ("n_steps", C.c_void_p),
                ("n_rejected", C.c_void_p), ("status", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class Irc(C.Structure):
    """anihip_irc (include/anihip.h)."""
    _fields_ = [("n_mol", C.c_int32), ("atoms_per_mol", C.c_int32), ("periodic", C.c_int32), ("max_points", C.c_int32),
                ("step", C.c_double), ("fmax", C.c_double), ("energy_floor", C.c_double),
                ("kind", C.c_void_p), ("masses", C.c_void_p), ("coords", C.c_void_p), ("energies", C.c_void_p),
                ("forces", C.c_void_p), ("hessians", C.c_void_p), ("direction", C.c_void_p), ("last_step", C.c_void_p),
                ("arc_lengths", C.c_void_p), ("n_points", C.c_void_p), ("reason", C.c_void_p), ("status", C.c_void_p),
                ("path_coords", C.c_void_p), ("path_energies", C.c_void_p), ("path_arcs", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class Mbar(C.Structure):
    """anihip_mbar (include/anihip.h)."""
    _fields_ = [("n_samples", C.c_int64), ("n_states", C.c_int32), ("n_cvs", C.c_int32),
                ("beta", C.c_void_p), ("n_k", C.c_void_p), ("restraint", C.c_void_p), ("cv_kind", C.c_void_p),
                ("energy", C.c_void_p), ("cv", C.c_void_p), ("u_kn", C.c_void_p), ("status", C.c_void_p)]


class MlpShape(C.Structure):
    """anihip_mlp_shape (include/anihip.h): what anihip_mlp_pack needs to know about the networks."""
    _fields_ = [("n_members", C.c_int32), ("num_species", C.c_int32), ("n_layers", C.c_int32), ("aev_len", C.c_int32),
                ("aev_radial_len", C.c_int32), ("precision", C.c_int32), ("activation", C.c_int32),
                ("celu_alpha", C.c_float), ("out_dims", (C.c_int32 * MAX_LAYERS) * MAX_SPECIES)]


def _stale() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(_HERE, "csrc", s) for s in SOURCES + HEADERS]
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile libanihip.so for gfx950 if it is missing or older than its sources."""
    if not force and not _stale():
        return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libanihip.so")
    cmd = [hipcc] + HIPCC_FLAGS + ["-o", LIB_PATH] + [os.path.join(_HERE, "csrc", s) for s in SOURCES]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


_lib: tp.Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """The loaded library.  torch must be imported first so that both share one HIP runtime."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (loads torch's libamdhip64.so.7 first; ours resolves to the same soname)

    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP engine is not built. Run `python -c 'import "
            "__graft_entry__ as g; g.build()'` (there is no CPU fallback)."
        )
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    L.anihip_last_error.restype = C.c_char_p
    L.anihip_abi_version.restype = C.c_int
    L.anihip_aev_table_pack.argtypes = [C.POINTER(AevParams), vp, vp, vp, vp]
    L.anihip_nbr_workspace_bytes.restype = sz
    L.anihip_nbr_workspace_bytes.argtypes = [i64, i64]
    L.anihip_nbr_build_batch.argtypes = [vp, C.POINTER(AevParams), i32, i32, vp, vp, vp, i32, i64, i64, vp,
                                         sz, vp, vp, i64, vp]
    L.anihip_nbr_build_cell.argtypes = [vp, C.POINTER(AevParams), i64, vp, vp, vp, i32, i64, i64, i64, vp,
                                        sz, vp, vp, i64, vp]
    L.anihip_nbr_half_workspace_bytes.restype = sz
    L.anihip_nbr_half_workspace_bytes.argtypes = [i64]
    L.anihip_nbr_from_half.argtypes = [vp, C.POINTER(AevParams), i64, vp, i64, vp, vp, i64, i64, vp, sz, vp, vp,
                                       i64, vp]
    L.anihip_nbr_rows_to_half_workspace_bytes.restype = sz
    L.anihip_nbr_rows_to_half_workspace_bytes.argtypes = [i64]
    L.anihip_nbr_rows_to_half.restype = C.c_int
    L.anihip_nbr_rows_to_half.argtypes = [vp, i64, i64, i64, vp, vp, vp, sz, i64, vp, vp, vp, vp]
    L.anihip_nbr_from_full.argtypes = [vp, C.POINTER(AevParams), i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, vp]
    L.anihip_nbr_refresh.argtypes = [vp, C.POINTER(AevParams), i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, i64, vp]
    L.anihip_aev_forward.argtypes = [vp, C.POINTER(AevParams), vp, i64, i64, i64, vp, vp, vp, vp, vp, vp]
    L.anihip_aev_forward_update.argtypes = [vp, C.POINTER(AevParams), vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp]
    L.anihip_aev_backward.argtypes = [vp, C.POINTER(AevParams), vp, i64, i64, i64, vp, vp, vp, vp, vp, i32, vp, vp]
    L.anihip_aev_jvp.argtypes = [vp, C.POINTER(AevParams), vp, i64, i64, i64, vp, vp, vp, vp, vp, vp]
    L.anihip_aev_jvp_batched.argtypes = [vp, C.POINTER(AevParams), vp, i64, i64, i64, vp, vp, vp, i64, vp, vp, vp]
    L.anihip_aev_jvp_batched.restype = C.c_int
    L.anihip_aev_backward_second.argtypes = [vp, C.POINTER(AevParams), vp, i64, i64, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp]
    L.anihip_aev_backward_second.restype = C.c_int
    L.anihip_mlp_input_hvp_workspace_bytes.restype = sz
    L.anihip_mlp_input_hvp_workspace_bytes.argtypes = [C.POINTER(MlpDesc), i64, i64]
    L.anihip_mlp_input_hvp.argtypes = [vp, C.POINTER(MlpDesc), i64, vp, vp, i64, vp, vp, sz, vp]
    L.anihip_mlp_input_hvp.restype = C.c_int
    L.anihip_aev_backward_virial.argtypes = [vp, C.POINTER(AevParams), vp, i64, i64, i64, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.anihip_aev_backward_flux.argtypes = [vp, C.POINTER(AevParams), vp, i64, i64, i64, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.anihip_aev_backward_flux.restype = C.c_int
    L.anihip_md_heat_flux_workspace_bytes.restype = sz
    L.anihip_md_heat_flux_workspace_bytes.argtypes = [i64, i64]
    L.anihip_md_heat_flux.argtypes = [vp, C.POINTER(MdParams), vp, vp, vp, vp, vp, vp, vp, sz]
    L.anihip_md_heat_flux.restype = C.c_int
    L.anihip_mlp_workspace_bytes.restype = sz
    L.anihip_mlp_workspace_bytes.argtypes = [C.POINTER(MlpDesc), i64]
    L.anihip_mlp_forward_backward_workspace_bytes.restype = sz
    L.anihip_mlp_forward_backward_workspace_bytes.argtypes = [C.POINTER(MlpDesc), i64, C.c_int32]
    L.anihip_mlp_pack_bytes.restype = sz
    L.anihip_mlp_pack_bytes.argtypes = [C.POINTER(MlpShape)]
    L.anihip_mlp_pack.restype = C.c_int
    L.anihip_mlp_pack.argtypes = [vp, C.POINTER(MlpShape), vp, vp, i32, vp, sz, i32, C.POINTER(MlpDesc)]
    L.anihip_mlp_forward_backward.argtypes = [vp, C.POINTER(MlpDesc), i64, i64, i64, vp, vp, vp, vp, sz, vp,
                                              vp, vp]
    L.anihip_mlp_train_workspace_bytes.restype = sz
    L.anihip_mlp_train_workspace_bytes.argtypes = [C.POINTER(MlpDesc), i64]
    L.anihip_mlp_fast_training.restype = C.c_int
    L.anihip_mlp_fast_training.argtypes = [C.POINTER(MlpDesc)]
    L.anihip_mlp_weight_grads.argtypes = [vp, C.POINTER(MlpDesc), i64, i64, i64, vp, vp, vp, vp, sz,
                                          C.POINTER(SpeciesGrads), vp, vp, i32]
    L.anihip_mlp_tangent_workspace_bytes.restype = sz
    L.anihip_mlp_tangent_workspace_bytes.argtypes = [C.POINTER(MlpDesc), i64]
    L.anihip_mlp_tangent_weight_grads.argtypes = [vp, C.POINTER(MlpDesc), i64, i64, i64, vp, vp, vp, vp, sz,
                                                  C.POINTER(SpeciesGrads), vp]
    L.anihip_mlp_train_forward.argtypes = [vp, C.POINTER(MlpDesc), i64, i64, i64, vp, vp, vp, sz, vp]
    L.anihip_mlp_repack.argtypes = [vp, C.POINTER(MlpDesc), vp, vp, vp, i32]
    L.anihip_adam_step.argtypes = [vp, vp, vp, vp, vp, i64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, vp, i32]
    L.anihip_adam_step.restype = C.c_int
    L.anihip_energy_reduce.argtypes = [vp, i32, i32, i64, i64, vp, vp, vp, vp]
    L.anihip_energy_forces_finish.argtypes = [vp, i32, i32, i64, i64, vp, vp, vp, vp, vp, i64]
    L.anihip_energy_forces_finish.restype = C.c_int
    L.anihip_pair_xtb_repulsion.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, C.c_float, i32, i32, vp, vp, vp]
    L.anihip_pair_xtb_repulsion.restype = C.c_int
    L.anihip_pair_analytic.argtypes = [vp, i32, i64, i64, i64, vp, vp, vp, vp, vp, C.c_float, i32, i32, vp, vp, vp]
    L.anihip_pair_analytic.restype = C.c_int
    L.anihip_pair_analytic_hvp.argtypes = [vp, i32, i64, i64, i64, vp, vp, vp, vp, vp, C.c_float, i32, i32, i64, vp, vp]
    L.anihip_pair_analytic_hvp.restype = C.c_int
    L.anihip_hess_sparse_rlist.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp]
    L.anihip_hess_sparse_pattern.argtypes = [vp, i64, vp, vp, vp, i64, vp, vp, vp]
    L.anihip_hess_sparse_items.argtypes = [vp, i32, i64, i64, vp, vp, vp, vp, vp, vp]
    L.anihip_hess_sparse_extract.argtypes = [vp, i64, i64, i64, vp, i64, i64, i64, vp, vp]
    L.anihip_aev_jvp_items.argtypes = [vp, C.POINTER(AevParams), vp, i64, vp, vp, vp, i64, vp, vp, vp]
    L.anihip_aev_backward_second_items.argtypes = [vp, C.POINTER(AevParams), vp, i64, vp, vp, vp, vp, i64, vp, vp, i64, i64,
                                                   vp, vp]
    L.anihip_mlp_rows_hvp_workspace_bytes.restype = sz
    L.anihip_mlp_rows_hvp_workspace_bytes.argtypes = [C.POINTER(MlpDesc), i64, i64]
    L.anihip_mlp_rows_hvp_prepare.argtypes = [vp, C.POINTER(MlpDesc), i64, vp, vp, vp, sz]
    L.anihip_mlp_rows_hvp.argtypes = [vp, C.POINTER(MlpDesc), i64, vp, i64, vp, vp, vp, sz, vp]
    L.anihip_pair_analytic_hvp_items.argtypes = [vp, i32, i64, vp, vp, vp, vp, vp, C.c_float, i32, i32, i64, vp, vp, i64, i64,
                                                 vp]
    for name in ("anihip_hess_sparse_rlist", "anihip_hess_sparse_pattern", "anihip_hess_sparse_items",
                 "anihip_hess_sparse_extract", "anihip_aev_jvp_items", "anihip_aev_backward_second_items",
                 "anihip_mlp_rows_hvp_prepare", "anihip_mlp_rows_hvp", "anihip_pair_analytic_hvp_items"):
        getattr(L, name).restype = C.c_int
    L.anihip_aev_jvp_strain_items.argtypes = [vp, C.POINTER(AevParams), vp, i64, vp, vp, vp, i64, vp, vp, vp]
    L.anihip_aev_backward_second_strain_items.argtypes = [vp, C.POINTER(AevParams), vp, i64, i64, vp, vp, vp, vp, i64, vp, vp,
                                                          vp, vp, vp]
    L.anihip_pair_analytic_hvp_strain.argtypes = [vp, i32, i64, i64, i64, i64, vp, vp, vp, vp, vp, C.c_float, i32, i32, vp, vp,
                                                  vp]
    for name in ("anihip_aev_jvp_strain_items", "anihip_aev_backward_second_strain_items",
                 "anihip_pair_analytic_hvp_strain"):
        getattr(L, name).restype = C.c_int
    L.anihip_block_hessian_prepare.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.anihip_block_hessian_prepare.restype = C.c_int
    L.anihip_block_hessian_spmm.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp]
    L.anihip_block_hessian_spmm.restype = C.c_int
    L.anihip_lbfgs_workspace_bytes.restype = sz
    L.anihip_lbfgs_workspace_bytes.argtypes = [i64, i64, i32]
    L.anihip_lbfgs_step.argtypes = [vp, C.POINTER(LbfgsParams), vp, vp, vp, vp, sz, vp, vp, vp]
    L.anihip_lbfgs_step.restype = C.c_int
    L.anihip_md_workspace_bytes.restype = sz
    L.anihip_md_workspace_bytes.argtypes = [i64, i64]
    L.anihip_md_drift.argtypes = [vp, C.POINTER(MdParams), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.anihip_md_kick.argtypes = [vp, C.POINTER(MdParams), vp, vp, vp, vp, vp, vp, sz]
    L.anihip_md_remove_drift.argtypes = [vp, C.POINTER(MdParams), vp, vp, vp, vp, sz]
    L.anihip_md_noise.argtypes = [vp, C.c_uint64, C.c_uint64, i64, i64, vp, vp]
    L.anihip_md_constrain_drift.argtypes = [vp, C.POINTER(MdParams), C.POINTER(MdClusters), vp, vp, vp, vp, vp, vp, vp]
    L.anihip_md_constrain_kick.argtypes = [vp, C.POINTER(MdParams), C.POINTER(MdClusters), vp, vp, vp, vp]
    L.anihip_md_project_velocities.argtypes = [vp, C.POINTER(MdParams), C.POINTER(MdClusters), vp, vp, vp]
    L.anihip_md_barostat.argtypes = [vp, C.POINTER(MdParams), C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                     vp, vp]
    L.anihip_md_group_terms.argtypes = [vp, C.POINTER(MdParams), C.POINTER(MdClusters), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.anihip_md_barostat_groups.argtypes = [vp, C.POINTER(MdParams), C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                            vp, vp, vp, C.POINTER(MdClusters), vp, vp, vp]
    L.anihip_md_rp_drift.argtypes = [vp, C.POINTER(MdParams), i32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.anihip_md_rp_estimators.argtypes = [vp, C.POINTER(MdParams), i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz]
    L.anihip_md_exchange.argtypes = [vp, C.POINTER(MdParams), C.POINTER(MdLadders), vp, vp, vp, vp]
    L.anihip_md_bias_workspace_bytes.restype = sz
    L.anihip_md_bias_workspace_bytes.argtypes = [C.POINTER(MdParams), C.POINTER(MdBias)]
    L.anihip_md_bias_apply.argtypes = [vp, C.POINTER(MdParams), C.POINTER(MdBias), vp, vp, vp, vp, vp, vp, vp, sz]
    L.anihip_md_bias_deposit.argtypes = [vp, C.POINTER(MdParams), C.POINTER(MdBias), vp, vp, vp]
    L.anihip_md_bias_hills.argtypes = [vp, C.POINTER(MdBias), i32, i64, vp, vp, vp]
    for name in ("anihip_md_bias_apply", "anihip_md_bias_deposit", "anihip_md_bias_hills"):
        getattr(L, name).restype = C.c_int
    L.anihip_md_sites_workspace_bytes.restype = sz
    L.anihip_md_sites_workspace_bytes.argtypes = [C.POINTER(MdParams), C.POINTER(MdSites)]
    L.anihip_md_sites_gather.argtypes = [vp, C.POINTER(MdParams), C.POINTER(MdSites), vp, vp, vp, vp, vp, vp, vp, sz]
    L.anihip_md_sites_spread.argtypes = [vp, C.POINTER(MdParams), C.POINTER(MdSites), vp, vp, vp, vp]
    for name in ("anihip_md_sites_gather", "anihip_md_sites_spread"):
        getattr(L, name).restype = C.c_int
    L.anihip_md_rdf_accumulate.argtypes = [vp, C.POINTER(MdParams), i32, i32, C.c_double, i32, vp, vp, vp, vp, i64, vp]
    L.anihip_md_corr_workspace_bytes.restype = sz
    L.anihip_md_corr_workspace_bytes.argtypes = [i64, i64, i64, i64]
    L.anihip_md_corr_accumulate.argtypes = [vp, C.POINTER(MdParams), i32, i32, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, sz]
    for name in ("anihip_md_rdf_accumulate", "anihip_md_corr_accumulate"):
        getattr(L, name).restype = C.c_int
    L.anihip_geom_constraints_project.argtypes = [vp, i64, i64, C.POINTER(GeomConstraints), vp, vp, vp]
    L.anihip_geom_constraints_restore.argtypes = [vp, i64, i64, C.POINTER(GeomConstraints), vp, vp]
    for name in ("anihip_geom_constraints_project", "anihip_geom_constraints_restore"):
        getattr(L, name).restype = C.c_int
    L.anihip_saddle_workspace_bytes.restype = sz
    L.anihip_saddle_workspace_bytes.argtypes = [i64, i64]
    L.anihip_saddle_project.argtypes = [vp, C.POINTER(Saddle), vp]
    L.anihip_saddle_step.argtypes = [vp, C.POINTER(Saddle), vp, vp]
    L.anihip_saddle_accept.argtypes = [vp, C.POINTER(Saddle), vp, vp, i32]
    for name in ("anihip_saddle_project", "anihip_saddle_step", "anihip_saddle_accept"):
        getattr(L, name).restype = C.c_int
    L.anihip_irc_workspace_bytes.restype = sz
    L.anihip_irc_workspace_bytes.argtypes = [i64, i64]
    L.anihip_irc_project.argtypes = [vp, C.POINTER(Irc), vp]
    L.anihip_irc_step.argtypes = [vp, C.POINTER(Irc), vp, vp]
    L.anihip_irc_commit.argtypes = [vp, C.POINTER(Irc), vp, vp, i32]
    for name in ("anihip_irc_project", "anihip_irc_step", "anihip_irc_commit"):
        getattr(L, name).restype = C.c_int
    L.anihip_phonon_fold.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.anihip_phonon_dynmat.argtypes = [vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.anihip_phonon_dos.argtypes = [vp, i64, vp, vp, C.c_double, C.c_double, C.c_double, i32, vp]
    for name in ("anihip_phonon_fold", "anihip_phonon_dynmat", "anihip_phonon_dos"):
        getattr(L, name).restype = C.c_int
    L.anihip_mbar_workspace_bytes.restype = sz
    L.anihip_mbar_workspace_bytes.argtypes = [C.POINTER(Mbar)]
    L.anihip_mbar_iterate.argtypes = [vp, C.POINTER(Mbar), vp, i32, vp, vp, vp, sz]
    L.anihip_mbar_log_weights.argtypes = [vp, C.POINTER(Mbar), vp, i32, vp, vp, vp, i64, i64, vp, vp, sz]
    L.anihip_mbar_histogram_workspace_bytes.restype = sz
    L.anihip_mbar_histogram_workspace_bytes.argtypes = [i64, i32]
    L.anihip_mbar_histogram.argtypes = [vp, i64, vp, vp, i32, i32, C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(i32), vp, vp, vp, sz]
    for name in ("anihip_mbar_iterate", "anihip_mbar_log_weights", "anihip_mbar_histogram"):
        getattr(L, name).restype = C.c_int
    for name in ("anihip_md_drift", "anihip_md_kick", "anihip_md_remove_drift", "anihip_md_noise",
                 "anihip_md_constrain_drift", "anihip_md_constrain_kick", "anihip_md_project_velocities",
                 "anihip_md_barostat", "anihip_md_group_terms", "anihip_md_barostat_groups", "anihip_md_rp_drift",
                 "anihip_md_rp_estimators", "anihip_md_exchange"):
        getattr(L, name).restype = C.c_int
    L.anihip_pair_d3.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, C.POINTER(D3Params), C.c_float, i32, vp, vp, vp, vp, vp]
    L.anihip_pair_d3.restype = C.c_int
    for name in ("anihip_aev_table_pack", "anihip_nbr_build_batch", "anihip_nbr_build_cell", "anihip_nbr_from_half",
                 "anihip_nbr_from_full", "anihip_nbr_refresh",
                 "anihip_aev_forward", "anihip_aev_forward_update", "anihip_aev_backward", "anihip_aev_backward_virial", "anihip_aev_jvp", "anihip_mlp_forward_backward",
                 "anihip_mlp_weight_grads", "anihip_mlp_tangent_weight_grads", "anihip_mlp_train_forward", "anihip_mlp_repack", "anihip_energy_reduce"):
        getattr(L, name).restype = C.c_int
    if L.anihip_abi_version() != ABI_VERSION:
        raise RuntimeError("libanihip.so ABI version mismatch: rebuild it")
    _lib = L
    return L


EXPORTED_SYMBOLS = [
    "anihip_last_error", "anihip_abi_version", "anihip_aev_table_pack", "anihip_nbr_workspace_bytes",
    "anihip_nbr_build_batch", "anihip_nbr_build_cell", "anihip_nbr_half_workspace_bytes", "anihip_nbr_from_half", "anihip_nbr_from_full",
    "anihip_nbr_refresh", "anihip_aev_forward", "anihip_aev_forward_update", "anihip_aev_backward", "anihip_aev_backward_virial", "anihip_aev_jvp",
    "anihip_mlp_workspace_bytes", "anihip_mlp_forward_backward_workspace_bytes", "anihip_mlp_forward_backward", "anihip_mlp_train_workspace_bytes",
    "anihip_mlp_fast_training",
    "anihip_mlp_weight_grads", "anihip_mlp_train_forward", "anihip_mlp_repack", "anihip_adam_step", "anihip_energy_reduce",
    "anihip_mlp_tangent_workspace_bytes", "anihip_mlp_tangent_weight_grads", "anihip_pair_xtb_repulsion",
    "anihip_pair_d3", "anihip_pair_analytic", "anihip_energy_forces_finish", "anihip_mlp_pack_bytes", "anihip_mlp_pack",
    "anihip_nbr_rows_to_half_workspace_bytes", "anihip_nbr_rows_to_half",
    "anihip_aev_jvp_batched", "anihip_aev_backward_second", "anihip_mlp_input_hvp_workspace_bytes", "anihip_mlp_input_hvp",
    "anihip_pair_analytic_hvp",
    "anihip_hess_sparse_rlist", "anihip_hess_sparse_pattern", "anihip_hess_sparse_items", "anihip_hess_sparse_extract",
    "anihip_aev_jvp_items", "anihip_aev_backward_second_items", "anihip_mlp_rows_hvp_workspace_bytes",
    "anihip_mlp_rows_hvp_prepare", "anihip_mlp_rows_hvp", "anihip_pair_analytic_hvp_items",
    "anihip_block_hessian_prepare", "anihip_block_hessian_spmm",
    "anihip_aev_jvp_strain_items", "anihip_aev_backward_second_strain_items", "anihip_pair_analytic_hvp_strain",
    "anihip_lbfgs_workspace_bytes", "anihip_lbfgs_step",
    "anihip_md_workspace_bytes", "anihip_md_drift", "anihip_md_kick", "anihip_md_remove_drift", "anihip_md_noise",
    "anihip_md_constrain_drift", "anihip_md_constrain_kick", "anihip_md_project_velocities", "anihip_md_barostat",
    "anihip_md_group_terms", "anihip_md_barostat_groups", "anihip_md_rp_drift", "anihip_md_rp_estimators",
    "anihip_md_exchange",
    "anihip_md_bias_workspace_bytes", "anihip_md_bias_apply", "anihip_md_bias_deposit", "anihip_md_bias_hills",
    "anihip_md_sites_workspace_bytes", "anihip_md_sites_gather", "anihip_md_sites_spread",
    "anihip_md_rdf_accumulate", "anihip_md_corr_workspace_bytes", "anihip_md_corr_accumulate",
    "anihip_geom_constraints_project", "anihip_geom_constraints_restore",
    "anihip_saddle_workspace_bytes", "anihip_saddle_project", "anihip_saddle_step", "anihip_saddle_accept",
    "anihip_irc_workspace_bytes", "anihip_irc_project", "anihip_irc_step", "anihip_irc_commit",
    "anihip_aev_backward_flux", "anihip_md_heat_flux_workspace_bytes", "anihip_md_heat_flux",
    "anihip_phonon_fold", "anihip_phonon_dynmat", "anihip_phonon_dos",
    "anihip_mbar_workspace_bytes", "anihip_mbar_iterate", "anihip_mbar_log_weights", "anihip_mbar_histogram_workspace_bytes",
    "anihip_mbar_histogram",
]


def check(rc: int) -> None:
    """Map a non-zero status of the C ABI to RuntimeError (the reference raises c10::Error ->
    RuntimeError from TORCH_CHECK, csrc/aev.cu:1693-1710)."""
    if rc != 0:
        raise RuntimeError("libanihip: " + lib().anihip_last_error().decode())
