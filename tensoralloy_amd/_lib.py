"""
ctypes binding of `libtensoralloy_amd.so` (C ABI: include/tensoralloy_amd.h).

The library is the product: if it is missing or cannot be loaded this module
raises — there is no Python/NumPy fallback for the hot path.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
REPO_DIR = PKG_DIR.parent
CSRC_DIR = PKG_DIR / "csrc"
INCLUDE_DIR = REPO_DIR / "include"
LIB_PATH = PKG_DIR / "libtensoralloy_amd.so"

SOURCES = ["ta_api.hip", "ta_api_train.hip", "ta_api_md.hip", "ta_api_relax.hip", "ta_api_phonon.hip", "ta_resident.hip", "ta_kernels.hip", "ta_kernels_v2.hip", "ta_mlp.hip", "ta_eam.hip",
           "ta_nlist.hip", "ta_grap.hip", "ta_train.hip", "ta_hvp.hip", "ta_neighbor.cpp", "ta_td.hip",
           "ta_td_train.hip", "ta_md.hip", "ta_md_mtk.hip", "ta_md_corr.hip", "ta_md_rdf.hip", "ta_md_adf.hip", "ta_md_order.hip", "ta_md_cluster.hip", "ta_md_cna.hip", "ta_md_sq.hip", "ta_md_flux.hip", "ta_relax.hip", "ta_neb.hip",
           "ta_phonon.hip", "ta_options.cpp"]
OBJ_DIR = CSRC_DIR / "build"

TA_OK = 0
TA_ERR_INVALID, TA_ERR_UNSUPPORTED, TA_ERR_HIP, TA_ERR_NOMEM = -1, -2, -3, -4
TA_WANT_ENERGY, TA_WANT_FORCES, TA_WANT_VIRIAL, TA_WANT_ATOMIC, TA_WANT_DESCRIPTORS = 1, 2, 4, 8, 16
TA_WANT_REUSE_DESCRIPTORS = 32
TA_MODEL_SF_MLP, TA_MODEL_EAM_ALLOY, TA_MODEL_EAM_ADP, TA_MODEL_GRAP_MLP, TA_MODEL_EAM_FS = 1, 2, 3, 4, 5
TA_CUTOFF = {"cosine": 0, "polynomial": 1}
TA_ACT = {"relu": 0, "softplus": 1, "tanh": 2, "squareplus": 3, "leaky_relu": 4,
          "sigmoid": 5, "softsign": 6, "elu": 7}
TA_N_KERNEL_SLOTS = 10
# ta_mlp_launch_info: info[0] (family) and info[7] (where act' lived)
TA_MLP_FAMILY = {0: "none", 1: "tile", 2: "tile_all", 3: "wave", 4: "wave_all", 5: "quad", 6: "quad_all", 7: "td"}
TA_MLP_DA = {0: "registers", 1: "lds", 2: "global"}
TA_MLP_BODY = {0: "none", 1: "generic", 2: "scalar", 3: "mixed"}  # ta_mlp_tile_body
# ta_model_desc.finite_temperature: bit 0 = temperature-dependent, bit 1 = Sommerfeld, bits 8-15 = H activation
TA_TD_ON, TA_TD_SOMMERFELD, TA_TD_ACT_SHIFT = 1, 2, 8
TA_LIST_VIEW = {"resident": 0, "kernel": 1}  # ta_list_info / ta_get_list
TA_LIST_BUILDER = {0: "host", 1: "one_pass", 2: "two_pass"}
TA_ABI_VERSION = 5  # include/tensoralloy_amd.h: TA_ABI_VERSION
KERNEL_SLOTS = ["pair_geometry", "g4_forward", "descriptor_reduce", "mlp", "backward",
                "force_gather", "frame_reduce", "eam", "neighbor_update", "grap_forward"]

# every symbol include/tensoralloy_amd.h declares
EXPORTED_SYMBOLS = [
    "ta_device_count", "ta_create", "ta_destroy", "ta_last_error", "ta_set_frames",
    "ta_compute", "ta_get_results", "ta_eval", "ta_set_stream", "ta_synchronize", "ta_time_compute",
    "ta_batch_energy_device_ptr", "ta_copy_batch_energy", "ta_get_pairs", "ta_neighbor_list", "ta_free",
    "ta_eam_tabulate", "ta_set_batch_energy_target", "ta_param_count", "ta_update_weights",
    "ta_energy_gradient", "ta_measure_hbm_copy", "ta_set_skin", "ta_update_positions", "ta_list_stats",
    "ta_count_contributing_triples", "ta_loss_gradient", "ta_constant_count", "ta_get_constants", "ta_update_constants",
    "ta_constant_gradient", "ta_list_sizes", "ta_abi_version", "ta_model_desc_size", "ta_set_nn_tables", "ta_step", "ta_hessian_vectors", "ta_view_results", "ta_step_view",
    "ta_set_electron_temperatures", "ta_get_td_results", "ta_td_loss_gradient",
    "ta_set_triangles", "ta_backward_variant", "ta_mlp_launch_info", "ta_mlp_tile_body", "ta_count_owned_triangles", "ta_triangle_owner",
    "ta_filter_param_count", "ta_update_filter_weights", "ta_grap_loss_gradient",
    "ta_set_filter_tables", "ta_filter_table_knots",
    "ta_md_init", "ta_md_set_thermostat", "ta_md_run", "ta_md_get_state",
    "ta_md_set_langevin", "ta_md_noise",
    "ta_md_set_barostat", "ta_md_get_cell", "ta_md_get_records",
    "ta_md_set_nose_hoover", "ta_md_get_chain", "ta_md_set_chain", "ta_md_get_chain_records",
    "ta_md_set_mtk_barostat", "ta_md_get_mtk_state", "ta_md_set_mtk_state", "ta_md_get_mtk_records",
    "ta_md_set_sampling", "ta_md_get_correlations", "ta_md_get_samples",
    "ta_md_set_rdf", "ta_md_get_rdf",
    "ta_md_set_adf", "ta_md_get_adf",
    "ta_md_set_order", "ta_md_get_order", "ta_md_get_order_atoms",
    "ta_md_set_clusters", "ta_md_get_clusters", "ta_md_get_cluster_atoms",
    "ta_md_set_cna", "ta_md_get_cna", "ta_md_get_cna_atoms",
    "ta_md_set_sq", "ta_md_get_sq", "ta_md_get_sq_amplitudes",
    "ta_md_set_flux", "ta_md_get_flux", "ta_md_get_flux_rows",
    "ta_relax_init", "ta_relax_run", "ta_relax_get_state",
    "ta_relax_set_cell", "ta_relax_get_cell",
    "ta_relax_set_band", "ta_relax_get_band",
    "ta_list_info", "ta_get_list",
    "ta_phonon_set_cell", "ta_phonon_force_constants", "ta_phonon_load_force_constants",
    "ta_phonon_frequencies", "ta_phonon_dos", "ta_phonon_eigh", "ta_phonon_eigh_group",
]

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class ModelDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("n_elements", C.c_int32),
        ("rcut", C.c_double), ("acut", C.c_double),
        ("angular", C.c_int32), ("cutoff_function", C.c_int32),
        ("n_eta", C.c_int32), ("n_omega", C.c_int32), ("n_beta", C.c_int32),
        ("n_gamma", C.c_int32), ("n_zeta", C.c_int32),
        ("eta", _dp), ("omega", _dp), ("beta", _dp), ("gamma", _dp), ("zeta", _dp),
        ("activation", C.c_int32), ("use_resnet_dt", C.c_int32), ("minmax_scale", C.c_int32),
        ("n_layers", _ip), ("layer_sizes", _ip), ("weights", _dp),
        ("xlo", _dp), ("xhi", _dp),
        ("n_eam_params", C.c_int32), ("eam_params", _dp),
        ("eps", C.c_double),
        ("n_grap_params", C.c_int32), ("grap_params", _dp),
        ("n_eam_nets", C.c_int32),
        ("eam_table_n", _ip), ("eam_table_dx", _dp), ("eam_table_coef", _dp),
        ("safe_pow", C.c_int32),
        ("finite_temperature", C.c_int32),
    ]


class Frame(C.Structure):
    _fields_ = [("n_atoms", C.c_int32), ("species", _ip), ("positions", _dp),
                ("cell", _dp), ("pbc", _ip)]


class BatchInfo(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("n_atoms", C.c_int64), ("n_pairs", C.c_int64),
                ("n_triples", C.c_int64), ("nnl_max", C.c_int32), ("descriptor_dim", C.c_int32),
                ("nl_on_device", C.c_int32), ("reserved_", C.c_int32),
                ("nl_ms", C.c_double), ("set_frames_ms", C.c_double)]


class FireParams(C.Structure):
    _fields_ = [("dt", C.c_double), ("dtmax", C.c_double), ("maxstep", C.c_double), ("finc", C.c_double),
                ("fdec", C.c_double), ("astart", C.c_double), ("fa", C.c_double), ("nmin", C.c_int32)]


class MdBarostatParams(C.Structure):
    _fields_ = [("pressure", C.c_double), ("taup", C.c_double), ("compressibility", C.c_double),
                ("mask", C.c_int32 * 3), ("isotropic", C.c_int32)]


TA_MD_MAX_CHAIN = 8  # include/tensoralloy_amd.h: TA_MD_MAX_CHAIN


class MdNhcParams(C.Structure):
    _fields_ = [("kT0", C.c_double), ("tau", C.c_double), ("chain", C.c_int32), ("loops", C.c_int32),
                ("dof_removed", C.c_int32)]


class MdMtkParams(C.Structure):
    _fields_ = [("pressure", C.c_double), ("tau_p", C.c_double), ("chain", C.c_int32), ("loops", C.c_int32),
                ("mask", C.c_int32 * 3), ("isotropic", C.c_int32)]


TA_MD_MAX_LAGS = 4096  # include/tensoralloy_amd.h: TA_MD_MAX_LAGS


class MdSamplingParams(C.Structure):
    _fields_ = [("n_lags", C.c_int32), ("sample_every", C.c_int32)]


TA_MD_MAX_BINS = 4096  # include/tensoralloy_amd.h: TA_MD_MAX_BINS
TA_MD_ORDER_MAX_DEGREES, TA_MD_ORDER_MAX_L, TA_MD_ORDER_MAX_CONN = 4, 12, 31  # include/tensoralloy_amd.h


class MdRdfParams(C.Structure):
    _fields_ = [("r_max", C.c_double), ("n_bins", C.c_int32), ("sample_every", C.c_int32)]


class MdAdfParams(C.Structure):
    _fields_ = [("r_bond", C.c_double), ("n_bins", C.c_int32), ("sample_every", C.c_int32)]


class MdOrderParams(C.Structure):
    _fields_ = [("r_bond", C.c_double), ("solid_threshold", C.c_double), ("n_bins", C.c_int32),
                ("sample_every", C.c_int32), ("n_degrees", C.c_int32), ("degrees", C.c_int32 * 4),
                ("solid_degree", C.c_int32)]


TA_MD_CLUSTER_MAX_SERIES = 1048576  # include/tensoralloy_amd.h


class MdClusterParams(C.Structure):
    _fields_ = [("r_link", C.c_double), ("n_min", C.c_int32), ("species_mask", C.c_int32), ("n_bins", C.c_int32),
                ("n_series", C.c_int32), ("sample_every", C.c_int32)]


TA_MD_CNA_ADAPTIVE, TA_MD_CNA_FIXED, TA_MD_CNA_TYPES = 0, 1, 5  # include/tensoralloy_amd.h


class MdCnaParams(C.Structure):
    _fields_ = [("r_cut", C.c_double), ("r_max", C.c_double), ("mode", C.c_int32), ("n_series", C.c_int32),
                ("sample_every", C.c_int32)]


TA_MD_SQ_MAX_Q, TA_MD_SQ_MAX_INDEX = 4096, 64  # include/tensoralloy_amd.h


class MdSqParams(C.Structure):
    _fields_ = [("n_q", C.c_int32), ("n_lags", C.c_int32), ("sample_every", C.c_int32), ("currents", C.c_int32)]


TA_MD_FLUX_ROW = 18  # include/tensoralloy_amd.h: J_conv[3], J_pot[3], K[6], W[6]


class MdFluxParams(C.Structure):
    _fields_ = [("n_lags", C.c_int32), ("sample_every", C.c_int32)]


class RelaxCellParams(C.Structure):
    _fields_ = [("cell_factor", C.c_double), ("pressure", C.c_double), ("mask", C.c_int32 * 6),
                ("hydrostatic", C.c_int32), ("reserved_", C.c_int32)]


class BandParams(C.Structure):
    _fields_ = [("k", C.c_double), ("climb", C.c_int32), ("reserved_", C.c_int32)]


TA_PHONON_MAX_ORDER = 48  # include/tensoralloy_amd.h: the eigensolver's largest matrix
TA_PHONON_THZ = 1000.0 * 0.09822694788464063 / (2.0 * 3.141592653589793)  # include/tensoralloy_amd.h


class PhononParams(C.Structure):
    _fields_ = [("n_basis", C.c_int32), ("q_chunk", C.c_int32)]


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def _compile_flags():
    return ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", f"-I{INCLUDE_DIR}",
            f"-I{CSRC_DIR}"] + os.environ.get("TA_EXTRA_HIPCC_FLAGS", "").split()


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile every HIP source for gfx950 into the in-tree shared library: one object per
    translation unit, compiled in parallel (only the stale ones), then one link."""
    srcs = [CSRC_DIR / s for s in SOURCES]
    headers = list(CSRC_DIR.glob("*.h")) + [INCLUDE_DIR / "tensoralloy_amd.h"]
    deps = srcs + headers
    stamp = OBJ_DIR / "flags.txt"
    flags_same = stamp.exists() and stamp.read_text() == " ".join(_compile_flags())
    if not force and flags_same and LIB_PATH.exists():
        newest = max(p.stat().st_mtime for p in deps)
        if LIB_PATH.stat().st_mtime >= newest:
            return LIB_PATH
    # several ranks may get here at once (torchrun): one builds, the others wait for the lock and
    # then find the library up to date; the output appears atomically
    import fcntl
    from concurrent.futures import ThreadPoolExecutor
    lock_path = str(LIB_PATH) + ".lock"
    with open(lock_path, "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            OBJ_DIR.mkdir(exist_ok=True)
            flags = _compile_flags()
            flags_same = stamp.exists() and stamp.read_text() == " ".join(flags)
            if not force and flags_same and LIB_PATH.exists() and \
                    LIB_PATH.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
                return LIB_PATH
            if not flags_same:
                force = True
            hdr_time = max(p.stat().st_mtime for p in headers)

            def compile_one(src):
                obj = OBJ_DIR / (src.stem + ".o")
                if not force and obj.exists() and obj.stat().st_mtime >= max(src.stat().st_mtime, hdr_time):
                    return obj
                cmd = [hipcc_path()] + flags + ["-c", str(src), "-o", str(obj)]
                if verbose:
                    print(" ".join(cmd))
                subprocess.run(cmd, check=True)
                return obj

            try:
                jobs = max(1, min(len(srcs), len(os.sched_getaffinity(0))))
            except AttributeError:
                jobs = 4
            with ThreadPoolExecutor(max_workers=jobs) as pool:
                objs = list(pool.map(compile_one, srcs))
            stamp.write_text(" ".join(flags))
            tmp = str(LIB_PATH) + f".tmp{os.getpid()}"
            cmd = [hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + \
                  [str(o) for o in objs] + ["-o", tmp]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
            os.replace(tmp, LIB_PATH)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB_PATH


_lib = None


def load():
    """Load the shared library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # TA_LIB_AB=<path of another build of the same ABI>: kernel A/B runs inside one GPU session
    # (box-to-box differences of ~5 % otherwise hide a 2 % kernel change). Never silent, and only a
    # library that reports this binding's ABI version (struct layouts included) is accepted.
    path = os.environ.get("TA_LIB_AB") or str(LIB_PATH)
    if path != str(LIB_PATH):
        import sys
        sys.stderr.write(f"tensoralloy_amd: TA_LIB_AB is set, loading {path} instead of {LIB_PATH}\n")
    lib = C.CDLL(path)
    try:
        lib.ta_abi_version.restype = C.c_int
        version, desc_size = lib.ta_abi_version(), lib.ta_model_desc_size()
    except AttributeError:
        version, desc_size = -1, -1
    if version != TA_ABI_VERSION or desc_size != C.sizeof(ModelDesc):
        raise ImportError(f"{path}: ABI version {version} / ta_model_desc of {desc_size} bytes, this binding "
                          f"is version {TA_ABI_VERSION} / {C.sizeof(ModelDesc)} bytes: rebuild the library")
    H = C.c_void_p
    lib.ta_device_count.restype = C.c_int
    lib.ta_create.argtypes = [C.POINTER(ModelDesc), C.c_int, C.POINTER(H)]
    lib.ta_destroy.argtypes = [H]
    lib.ta_last_error.argtypes = [H]
    lib.ta_last_error.restype = C.c_char_p
    lib.ta_set_frames.argtypes = [H, C.c_int32, C.POINTER(Frame), C.POINTER(BatchInfo)]
    lib.ta_compute.argtypes = [H, C.c_uint32]
    lib.ta_get_results.argtypes = [H, _dp, _dp, _dp, _dp, _dp]
    lib.ta_eval.argtypes = [H, C.c_int32, C.POINTER(Frame), C.c_uint32, _dp, _dp, _dp, _dp]
    lib.ta_synchronize.argtypes = [H]
    lib.ta_set_stream.argtypes = [H, C.c_void_p]
    lib.ta_time_compute.argtypes = [H, C.c_uint32, C.c_int32, C.c_int32, _dp, _dp]
    lib.ta_measure_hbm_copy.argtypes = [H, C.c_int64, C.c_int32, _dp]
    lib.ta_batch_energy_device_ptr.argtypes = [H, C.POINTER(C.c_void_p)]
    lib.ta_copy_batch_energy.argtypes = [H, C.c_void_p]
    lib.ta_set_batch_energy_target.argtypes = [H, C.c_void_p]
    lib.ta_param_count.argtypes = [H, C.POINTER(C.c_int64)]
    lib.ta_update_weights.argtypes = [H, _dp, C.c_int64]
    lib.ta_energy_gradient.argtypes = [H, _dp, _dp, C.c_int64]
    lib.ta_loss_gradient.argtypes = [H, _dp, _dp, _dp, _dp, C.c_int64, _dp]
    lib.ta_td_loss_gradient.argtypes = [H, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int64, _dp]
    lib.ta_filter_param_count.argtypes = [H, C.POINTER(C.c_int64)]
    lib.ta_update_filter_weights.argtypes = [H, _dp, C.c_int64]
    lib.ta_grap_loss_gradient.argtypes = [H, _dp, _dp, _dp, _dp, C.c_int64]
    lib.ta_constant_count.argtypes = [H, C.POINTER(C.c_int64)]
    lib.ta_get_constants.argtypes = [H, _dp, C.c_int64]
    lib.ta_update_constants.argtypes = [H, _dp, C.c_int64]
    lib.ta_constant_gradient.argtypes = [H, _dp, _dp, _dp, _dp, C.c_int64]
    lib.ta_get_pairs.argtypes = [H, _ip, _ip, _ip]
    lib.ta_list_info.argtypes = [H, C.c_int32, C.POINTER(C.c_int64)]
    lib.ta_get_list.argtypes = [H, C.c_int32, _ip, _ip, _ip, _ip, _ip, _ip, _ip, _ip]
    lib.ta_neighbor_list.argtypes = [C.POINTER(Frame), C.c_int32, C.c_double,
                                     C.POINTER(C.c_int64), C.POINTER(_ip), C.POINTER(_ip),
                                     C.POINTER(_ip), C.POINTER(_ip)]
    lib.ta_count_contributing_triples.argtypes = [H, C.POINTER(C.c_int64)]
    lib.ta_set_skin.argtypes = [H, C.c_double]
    lib.ta_update_positions.argtypes = [H, _dp, _dp, _ip]
    lib.ta_list_stats.argtypes = [H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.ta_list_sizes.argtypes = [H, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.ta_set_nn_tables.argtypes = [H, C.c_int]
    lib.ta_set_filter_tables.argtypes = [H, C.c_int, C.c_int32]
    lib.ta_filter_table_knots.argtypes = [H, C.POINTER(C.c_int32)]
    lib.ta_set_triangles.argtypes = [H, C.c_int]
    lib.ta_backward_variant.argtypes = [H, C.POINTER(C.c_int32)]
    lib.ta_mlp_launch_info.argtypes = [H, C.POINTER(C.c_int64)]
    lib.ta_mlp_tile_body.argtypes = [H, _ip]
    lib.ta_count_owned_triangles.argtypes = [H, C.POINTER(C.c_int64)]
    lib.ta_triangle_owner.argtypes = [C.c_int64, _ip, _ip]
    lib.ta_hessian_vectors.argtypes = [H, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp]
    lib.ta_step.argtypes = [H, _dp, _dp, C.c_uint32, _dp, _dp, _dp, _dp, _ip]
    _dpp = C.POINTER(_dp)
    lib.ta_view_results.argtypes = [H, C.c_uint32, _dpp, _dpp, _dpp, _dpp]
    lib.ta_step_view.argtypes = [H, _dp, _dp, C.c_uint32, _dpp, _dpp, _dpp, _dpp, _ip]
    lib.ta_free.argtypes = [C.c_void_p]
    lib.ta_eam_tabulate.argtypes = [H, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp]
    lib.ta_free.restype = None
    lib.ta_set_electron_temperatures.argtypes = [H, C.c_int32, _dp]
    lib.ta_get_td_results.argtypes = [H, _dp, _dp, _dp, _dp]
    lib.ta_md_init.argtypes = [H, _dp, _dp]
    lib.ta_md_set_thermostat.argtypes = [H, C.c_double, C.c_double]
    lib.ta_md_run.argtypes = [H, C.c_int32, C.c_double, C.c_uint32, C.c_int32, _dp, _dp, _ip]
    lib.ta_md_get_state.argtypes = [H, _dp, _dp]
    lib.ta_md_set_langevin.argtypes = [H, C.c_double, C.c_double, C.c_uint64]
    lib.ta_md_noise.argtypes = [H, C.c_int64, _dp, _dp]
    lib.ta_md_set_barostat.argtypes = [H, C.POINTER(MdBarostatParams)]
    lib.ta_md_get_cell.argtypes = [H, _dp]
    lib.ta_md_get_records.argtypes = [H, _dp, _dp]
    lib.ta_md_set_nose_hoover.argtypes = [H, C.POINTER(MdNhcParams)]
    lib.ta_md_get_chain.argtypes = [H, _dp, _dp]
    lib.ta_md_set_chain.argtypes = [H, _dp, _dp]
    lib.ta_md_get_chain_records.argtypes = [H, _dp]
    lib.ta_md_set_mtk_barostat.argtypes = [H, C.POINTER(MdMtkParams)]
    lib.ta_md_get_mtk_state.argtypes = [H, _dp, _dp, _dp]
    lib.ta_md_set_mtk_state.argtypes = [H, _dp, _dp, _dp]
    lib.ta_md_get_mtk_records.argtypes = [H, _dp]
    lib.ta_md_set_sampling.argtypes = [H, C.POINTER(MdSamplingParams)]
    lib.ta_md_get_correlations.argtypes = [H, _dp, _dp, C.POINTER(C.c_int64)]
    lib.ta_md_get_samples.argtypes = [H, C.c_int32, C.c_int32, _dp, _dp, C.POINTER(C.c_int64)]
    lib.ta_md_set_rdf.argtypes = [H, C.POINTER(MdRdfParams)]
    lib.ta_md_get_rdf.argtypes = [H, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _dp]
    lib.ta_md_set_adf.argtypes = [H, C.POINTER(MdAdfParams), _dp]
    lib.ta_md_get_adf.argtypes = [H, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _dp]
    lib.ta_md_set_order.argtypes = [H, C.POINTER(MdOrderParams), _dp]
    lib.ta_md_get_order.argtypes = [H, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int64), _dp]
    lib.ta_md_get_order_atoms.argtypes = [H, _dp, _dp, _ip, _ip, _dp]
    lib.ta_md_set_clusters.argtypes = [H, C.POINTER(MdClusterParams), _dp]
    lib.ta_md_get_clusters.argtypes = [H, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int64), _dp]
    lib.ta_md_get_cluster_atoms.argtypes = [H, _ip, _ip]
    lib.ta_md_set_cna.argtypes = [H, C.POINTER(MdCnaParams)]
    lib.ta_md_get_cna.argtypes = [H, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int64)]
    lib.ta_md_get_cna_atoms.argtypes = [H, _ip, _dp]
    lib.ta_md_set_sq.argtypes = [H, C.POINTER(MdSqParams), _ip]
    lib.ta_md_get_sq.argtypes = [H, _dp, _dp, _dp, C.POINTER(C.c_int64), _ip]
    lib.ta_md_get_sq_amplitudes.argtypes = [H, C.c_int32, C.c_int32, _dp, _dp, C.POINTER(C.c_int64)]
    lib.ta_md_set_flux.argtypes = [H, C.POINTER(MdFluxParams)]
    lib.ta_md_get_flux.argtypes = [H, _dp, _dp, _dp, C.POINTER(C.c_int64)]
    lib.ta_md_get_flux_rows.argtypes = [H, C.c_int32, C.c_int32, _dp, C.POINTER(C.c_int64)]
    lib.ta_relax_init.argtypes = [H, C.POINTER(FireParams), C.POINTER(C.c_uint8)]
    lib.ta_relax_run.argtypes = [H, C.c_int32, C.c_double, C.c_uint32, _ip, _ip, _dp, _ip]
    lib.ta_relax_get_state.argtypes = [H, _dp, _dp, _dp, _dp, _ip]
    lib.ta_relax_set_cell.argtypes = [H, C.c_int, C.POINTER(RelaxCellParams)]
    lib.ta_relax_get_cell.argtypes = [H, _dp, _dp, _dp, _dp]
    lib.ta_relax_set_band.argtypes = [H, C.c_int, C.POINTER(BandParams)]
    lib.ta_relax_get_band.argtypes = [H, _dp, _dp, _dp, _ip]
    _i64p, _u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    lib.ta_phonon_set_cell.argtypes = [H, C.POINTER(PhononParams), _ip, _dp, _ip, _dp]
    lib.ta_phonon_force_constants.argtypes = [H, _dp]
    lib.ta_phonon_load_force_constants.argtypes = [H, _dp]
    lib.ta_phonon_frequencies.argtypes = [H, C.c_int64, _dp, _dp, _dp, _i64p]
    lib.ta_phonon_dos.argtypes = [H, C.c_int64, _dp, C.c_int32, C.c_double, C.c_double, _u64p, _dp, _i64p]
    lib.ta_phonon_eigh.argtypes = [H, C.c_int32, C.c_int64, _dp, _dp, _dp, _i64p]
    lib.ta_phonon_eigh_group.argtypes = [C.c_int32]
    _lib = lib
    return lib


def check(lib, handle, rc):
    """Map C error codes to the exceptions the reference raises for this path."""
    if rc == TA_OK:
        return
    msg = lib.ta_last_error(handle)
    msg = msg.decode("utf-8", "replace") if msg else f"error {rc}"
    if rc in (TA_ERR_INVALID, TA_ERR_UNSUPPORTED):
        raise ValueError(msg)
    if rc == TA_ERR_NOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def as_dp(a: np.ndarray):
    return a.ctypes.data_as(_dp)


def as_ip(a: np.ndarray):
    return a.ctypes.data_as(_ip)


class FrameArrays:
    """Keeps the NumPy arrays behind a `Frame` alive."""

    def __init__(self, species, positions, cell, pbc):
        self.species = np.ascontiguousarray(species, dtype=np.int32)
        self.positions = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        self.cell = np.ascontiguousarray(cell, dtype=np.float64).reshape(3, 3)
        self.pbc = np.ascontiguousarray(np.asarray(pbc).astype(bool), dtype=np.int32).reshape(3)
        if len(self.species) != len(self.positions):
            raise ValueError("species and positions disagree on the number of atoms")

    def as_struct(self) -> Frame:
        return Frame(len(self.species), as_ip(self.species), as_dp(self.positions),
                     as_dp(self.cell), as_ip(self.pbc))


def neighbor_list(species, positions, cell, pbc, n_elements, rc):
    """Host-only neighbour list of the library (no GPU needed)."""
    lib = load()
    fa = FrameArrays(species, positions, cell, pbc)
    fr = fa.as_struct()
    n = C.c_int64(0)
    pi, pj, ps, pr = _ip(), _ip(), _ip(), _ip()
    rc_ = lib.ta_neighbor_list(C.byref(fr), n_elements, float(rc), C.byref(n), C.byref(pi),
                               C.byref(pj), C.byref(ps), C.byref(pr))
    check(lib, None, rc_)
    P = n.value
    try:
        i = np.ctypeslib.as_array(pi, shape=(max(P, 1),))[:P].copy()
        j = np.ctypeslib.as_array(pj, shape=(max(P, 1),))[:P].copy()
        s = np.ctypeslib.as_array(ps, shape=(max(3 * P, 1),))[:3 * P].copy().reshape(-1, 3)
        r = np.ctypeslib.as_array(pr, shape=(max(P, 1),))[:P].copy()
    finally:
        for p in (pi, pj, ps, pr):
            lib.ta_free(p)
    return i, j, s, r
