"""Host-side mirror of MendelIHT.jl's hot-path API over the C ABI (ctypes).

Names, keyword arguments, defaults and error behaviour follow the reference:
  fit_iht   src/fit.jl:60-118          cv_iht          src/cross_validation.jl:60-131
  iht       src/wrapper.jl:52-120      cross_validate  src/wrapper.jl:301-349
  project_k! / project_group_sparse!   src/utilities.jl:553-559, 613-679
  SnpLinAlg (SnpArrays.jl)             constructed as in src/wrapper.jl:68-69
All numerics run in libmendeliht_hip.so on the GPU; this file only marshals.
"""
import collections
import ctypes as C
import math
import os
import sys
import time
import warnings

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBNAME = "libmendeliht_hip.so"
# the measurement build of the same sources (-DMIH_PROBES: launch-shape sweeps, round-1 kernel families, timing probes, the
# MENDELIHT_* A/B switches).  tools/ and the "this switch changes nothing" tests select it with MENDELIHT_HIP_PROBES=1 in the
# environment (read once, at the first lib() call); the product never does.
_PROBES_LIBNAME = "libmendeliht_hip_probes.so"


class MendelIHTError(RuntimeError):
    """Base class for errors reported by the HIP library."""


class DimensionMismatch(MendelIHTError, ValueError):
    pass


class ArgumentError(MendelIHTError, ValueError):
    pass


_STATUS = {1: DimensionMismatch, 2: ArgumentError, 3: ArgumentError, 4: MendelIHTError, 5: MendelIHTError,
           6: MendelIHTError, 7: MemoryError, 8: MendelIHTError}


def library_path():
    return os.path.join(_HERE, _LIBNAME)


def probes_library_path():
    return os.path.join(_HERE, _PROBES_LIBNAME)


def using_probes():
    e = os.environ.get("MENDELIHT_HIP_PROBES", "")
    return e not in ("", "0")


class _FitParams(C.Structure):
    _fields_ = [("k", C.c_int64), ("J", C.c_int64), ("dist", C.c_int32), ("link", C.c_int32),
                ("nb_r", C.c_double), ("tol", C.c_double),
                ("max_iter", C.c_int32), ("min_iter", C.c_int32), ("max_step", C.c_int32), ("est_r", C.c_int32),
                ("zkeep", C.c_void_p), ("weight", C.c_void_p), ("group", C.c_void_p), ("ks", C.c_void_p),
                ("nks", C.c_int64), ("progress", C.c_void_p), ("progress_user", C.c_void_p),
                ("init_beta", C.c_int32), ("comm", C.c_void_p), ("debias", C.c_int32), ("xtv_digits", C.c_int32),
                ("choose", C.c_void_p), ("choose_user", C.c_void_p), ("cv_threads", C.c_int32), ("step_mode", C.c_int32)]


class _Comm(C.Structure):
    """mih_comm (include/mendeliht_hip.h): the exchange callbacks of a column-sharded fit."""
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("col_offset", C.c_int64), ("p_global", C.c_int64),
                ("allreduce", C.c_void_p), ("allgather", C.c_void_p), ("user", C.c_void_p)]


_CHOOSE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int64, C.c_int64, C.POINTER(C.c_int64))
CHOOSE_SAMPLE, CHOOSE_SHUFFLE_B, CHOOSE_SHUFFLE_C = 0, 1, 2      # mih_fit_params::choose kinds (include/mendeliht_hip.h)


def _choose_callback(fn):
    """mih_fit_params::choose from a Python callable fn(kind, list, excess) -> positions: the caller's stand-in for the
    reference's RNG draw in _choose! (`sample(non_zero_idx, excess, replace=false)`, src/utilities.jl:453; `shuffle!`,
    src/multivariate.jl:336-337).  kind CHOOSE_SAMPLE: return `excess` distinct entries of list; CHOOSE_SHUFFLE_*: return
    the whole list in shuffled order."""
    def cb(_user, kind, lst, n, excess, out):
        try:
            got = np.asarray(fn(int(kind), np.array(lst[:n], dtype=np.int64), int(excess)), dtype=np.int64).ravel()
            want = excess if kind == CHOOSE_SAMPLE else n
            if got.size != want:
                return 1
            for t in range(want):
                out[t] = int(got[t])
            return 0
        except Exception:       # an exception must not unwind through the C frames
            return 1
    return _CHOOSE(cb)


_ALLREDUCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32)
_ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)


class _FitResult(C.Structure):
    _fields_ = [("time", C.c_double), ("logl", C.c_double), ("iter", C.c_int64), ("pve", C.c_double),
                ("nb_r", C.c_double), ("choose_fired", C.c_int32), ("n_trace", C.c_int32),
                ("beta", C.c_void_p), ("c", C.c_void_p), ("logl_trace", C.c_void_p), ("tol_trace", C.c_void_p),
                ("bt_trace", C.c_void_p), ("mu", C.c_void_p)]


class _MvResult(C.Structure):
    _fields_ = [("time", C.c_double), ("logl", C.c_double), ("iter", C.c_int64),
                ("choose_fired", C.c_int32), ("n_trace", C.c_int32),
                ("B", C.c_void_p), ("C", C.c_void_p), ("Sigma", C.c_void_p), ("pve", C.c_void_p),
                ("logl_trace", C.c_void_p), ("tol_trace", C.c_void_p), ("bt_trace", C.c_void_p)]


class _PassRecord(C.Structure):
    """mih_pass_record: one launch of the dominant X'r kernel as the measurement hook of a matrix recorded it."""
    _fields_ = [("start_ms", C.c_double), ("ms", C.c_double), ("residuals", C.c_int32), ("operands", C.c_int32),
                ("stream_tag", C.c_int32), ("reserved", C.c_int32), ("kernel", C.c_char * 48)]


PROFILE_COUNTERS = ("lanes", "max_in_flight", "handovers", "shared_init", "rounds", "fits", "scores", "max_lane_slots", "init_scores",
                    "resident_steps", "resident_attempts", "resident_handbacks", "resident_direct", "resident_redos", "skipped_last_scores", "residuals_43bit",
                    "peeled_residuals")

_PROGRESS = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double)

# The ctypes argument types of every function include/mendeliht_hip.h declares (all return int).  lib() applies them, and
# exported_symbols() is this table's keys: tests/test_abi_cpu.py holds them against the header, so a declared function without a
# signature fails there.
_vp, _i64, _i32, _dbl = C.c_void_p, C.c_int64, C.c_int32, C.c_double
_SIGNATURES = {
    "mih_device_count": [C.POINTER(C.c_int)],
    "mih_last_error": [C.c_char_p, C.c_size_t],
    "mih_version": [C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "mih_snp_create": [_vp, _i64, _i64, _i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)],
    "mih_snp_create_synthetic": [_i64, _i64, C.c_uint64, _dbl, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)],
    "mih_snp_create_synthetic_shard": [_i64, _i64, _i64, C.c_uint64, _dbl, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)],
    "mih_dense_create": [_vp, _i64, _i64, C.c_int, C.POINTER(_vp)],
    "mih_dense_create_synthetic": [_i64, _i64, C.c_uint64, C.c_int, C.POINTER(_vp)],
    "mih_dense_create_f32": [_vp, _i64, _i64, C.c_int, C.POINTER(_vp)],
    "mih_dosage_create": [_vp, _i64, _i64, _i64, _i32, C.c_int, C.POINTER(_vp)],
    "mih_dosage_create_synthetic": [_i64, _i64, C.c_uint64, _i32, _dbl, C.c_int, C.POINTER(_vp)],
    "mih_dosage_export": [_vp, _i64, _i64, _vp],
    "mih_dosage_create_bgen": [C.c_char_p, _i64, _i64, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i64),
                               C.POINTER(_i32)],
    "mih_vcf_open": [C.c_char_p, C.c_int, _i64, C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_i32)],
    "mih_vcf_info": [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i32), C.POINTER(_i64)],
    "mih_vcf_header": [_vp, C.c_char_p, _i64, C.POINTER(_i64)],
    "mih_dosage_create_vcf": [_vp, C.c_int, _i64, _i64, C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i32)],
    "mih_vcf_meta": [_vp, C.c_char_p, _i64, C.POINTER(_i64)],
    "mih_vcf_inflate": [_vp, C.c_int, C.POINTER(_i64)],
    "mih_vcf_close": [_vp],
    "mih_dosage_regrid": [_vp, _i32],
    "mih_snp_builder_create": [_i64, _i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)],
    "mih_snp_builder_add": [_vp, _i64, _vp, C.POINTER(_i64)],
    "mih_snp_builder_finish": [_vp, C.POINTER(_vp)],
    "mih_snp_builder_destroy": [_vp],
    "mih_snp_create_dosage": [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(_i64)],
    "mih_snp_create_vcf": [_vp, C.c_int, _i64, _i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(_i64),
                           C.POINTER(_i32)],
    "mih_mat_destroy": [_vp],
    "mih_mat_dims": [_vp, C.POINTER(_i64), C.POINTER(_i64)],
    "mih_mat_reserve": [_vp, _i64],
    "mih_mat_score_image": [_vp, C.c_int, _dbl, C.POINTER(_i64), C.POINTER(_i64)],
    "mih_device_trim": [C.c_int, C.POINTER(_i64)],
    "mih_snp_mu_sigma": [_vp, _vp, _vp],
    "mih_snp_export_bed": [_vp, _vp],
    "mih_snp_counts": [_vp, _vp, _vp, _vp, _vp],
    "mih_snp_subset": [_vp, _vp, _i64, _vp, _i64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)],
    "mih_snp_transpose": [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _i64, C.POINTER(_vp)],
    "mih_grm": [_vp, _vp, C.c_int, _i64, _vp],
    "mih_grm_pairs": [_vp, _vp, C.c_int, _i64, _dbl, _i64, _vp, _vp, _vp, C.POINTER(_i64), _vp],
    "mih_grm_eig": [_vp, _vp, C.c_int, _i64, _i32, _i32, _dbl, _i32, C.c_uint64, _vp, _vp, _vp, C.POINTER(_i32), C.POINTER(_i32)],
    "mih_grm_solve": [_vp, _vp, C.c_int, _i64, _dbl, _dbl, _vp, _i32, _dbl, _i32, _vp, _vp, _vp, _vp],
    "mih_lmm_null": [_vp, _vp, C.c_int, _i64, _vp, _vp, _i32, _i32, C.c_uint64, _vp, _i32, _dbl, _i32, _dbl, _i32, _vp, _vp, _vp, C.POINTER(_dbl), _vp, _vp,
                     C.POINTER(_dbl), _vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_dbl)],
    "mih_neglog10p": [_vp, _i64, _vp],
    "mih_ld_band": [_vp, _i64, _i64, _i64, _vp, _vp, _vp],
    "mih_ld_pairs": [_vp, _i64, _dbl, _i64, _i64, _i64, _vp, _vp, _vp, C.POINTER(_i64)],
    "mih_ld_prune": [_vp, _i64, _i64, _dbl, _i64, _i64, _vp, C.POINTER(_i64)],
    "mih_assoc_score": [_vp, _vp, _i32, _vp, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp],
    "mih_assoc_score_spa": [_vp, _vp, _vp, _vp, _i32, _vp, _dbl, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mih_assoc_score_firth": [_vp, _vp, _vp, _vp, _i32, _vp, _dbl, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mih_assoc_sets": [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mih_assoc_sets_skato": [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                             _vp, _vp, _vp, _vp, _vp],
    "mih_snp_naive_impute": [_vp, _vp],
    "mih_xtv": [_vp, _vp, _vp],
    "mih_xtv_batched": [_vp, _vp, C.c_int, _vp],
    "mih_xtv_batched_fmt": [_vp, _vp, C.c_int, C.c_int, _vp],
    "mih_xv_sparse": [_vp, _vp, _vp, _i64, _vp],
    "mih_xb_dense": [_vp, _vp, _vp, _i32, C.c_int, C.c_int, C.c_int, C.c_int, _vp],
    "mih_project_topk": [_vp, _i64, _i64, C.POINTER(_i64)],
    "mih_project_group_sparse": [_vp, _vp, _i64, _i64, _vp, C.c_int],
    "mih_fit_iht": [_vp, C.POINTER(_FitParams), _vp, _vp, _i64, _vp, C.POINTER(_FitResult)],
    "mih_cv_iht": [_vp, C.POINTER(_FitParams), _vp, _vp, _i64, _vp, _i32, _vp, _i64, _i32, _i32, _vp],
    "mih_cv_meanloss": [_vp, _vp, _i64, _i32, _i64, _vp],
    "mih_cv_assignment": [_vp, _i64, _i32, _i32, _vp],
    "mih_fit_iht_path": [_vp, C.POINTER(_FitParams), _vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp],
    "mih_cv_iht_multi": [_vp, _i32, C.POINTER(_FitParams), _vp, _vp, _i64, _vp, _i32, _vp, _i64, _vp],
    "mih_fit_mv": [_vp, C.POINTER(_FitParams), _vp, _i64, _vp, _i64, _vp, C.POINTER(_MvResult)],
    "mih_cv_mv": [_vp, C.POINTER(_FitParams), _vp, _i64, _vp, _i64, _vp, _i32, _vp, _i64, _i32, _i32, _vp],
    "mih_bench_xtv": [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_float), C.POINTER(_dbl)],
    "mih_xtv_algorithmic_bytes": [_vp, C.c_int, C.POINTER(_dbl)],
    "mih_abi_sizes": [_vp, _i32],
    "mih_session_create": [_vp, C.POINTER(_FitParams), _vp, _vp, _i64, _vp, C.POINTER(_vp)],
    "mih_session_step": [_vp, C.POINTER(_dbl), C.POINTER(_i32), C.POINTER(_dbl)],
    "mih_session_run": [_vp, _i64, C.POINTER(_dbl), C.POINTER(_i64), C.POINTER(_dbl)],
    "mih_session_model": [_vp, _vp, _vp],
    "mih_session_destroy": [_vp],
    "mih_rccl_unique_id": [_vp],
    "mih_comm_create_rccl": [_vp, _i32, _i32, _i32, _i64, _i64, C.POINTER(_vp)],
    "mih_comm_destroy_rccl": [_vp],
    "mih_comm_info": [_vp, C.POINTER(_i32), _vp, _i64],
    "mih_cv_allgather": [_vp, _vp, _i64],
    "mih_profile_enable": [_vp, C.c_int],
    "mih_profile_read": [_vp, C.POINTER(_dbl), C.POINTER(_i64), C.c_int],
    "mih_profile_passes": [_vp, C.POINTER(_PassRecord), _i64, C.POINTER(_i64), C.c_int],
    "mih_profile_counters": [_vp, C.POINTER(_i64), C.c_int],
    "mih_profile_exchange": [_vp, C.POINTER(_dbl), C.POINTER(_i64), C.c_int],
}
# include/mendeliht_hip_probes.h: exported by the measurement build only
_PROBE_SIGNATURES = {
    "mih_probe_set_xtv_variant": [C.c_int], "mih_probe_set_xtv_multi_variant": [C.c_int],
    "mih_probe_set_max_fused": [C.c_int],
    "mih_probe_xtv_sequence": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "mih_probe_xv_sequence": [_vp, _i64, _i64, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mih_probe_debias_glm": [_vp, _vp, _i64, _vp, C.c_int, C.c_int, _dbl, _vp, _vp, _vp, _vp, _vp],
    "mih_probe_init_beta": [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]
}

_lib = None


def lib():
    """Load the HIP library; fails loudly when it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = probes_library_path() if using_probes() else library_path()
    path = os.environ.get("MENDELIHT_HIP_LIB", path)          # an explicit build of the library (the Julia glue reads the same variable)
    if not os.path.exists(path):
        raise MendelIHTError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for this path.")
    L = C.CDLL(path)
    sig = dict(_SIGNATURES)
    if using_probes():
        sig.update(_PROBE_SIGNATURES)
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = C.c_int
    _lib = L
    return L


def exported_symbols():
    """Every symbol include/mendeliht_hip.h declares (checked by the CPU test-suite)."""
    return list(_SIGNATURES)


def probe_symbols():
    """What include/mendeliht_hip_probes.h declares: exported by the measurement build only."""
    return list(_PROBE_SIGNATURES)


def _check(rc):
    if rc == 0:
        return
    buf = C.create_string_buffer(512)
    lib().mih_last_error(buf, 512)
    raise _STATUS.get(rc, MendelIHTError)(f"[mih status {rc}] {buf.value.decode(errors='replace')}")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def device_count():
    n = C.c_int(0)
    _check(lib().mih_device_count(C.byref(n)))
    return n.value


def device_trim(device=0):
    """Releases every score image on the device that no live fit or session uses (mih_device_trim); the bytes released."""
    nbytes = C.c_int64(0)
    _check(lib().mih_device_trim(int(device), C.byref(nbytes)))
    return nbytes.value


# ---- distributions and links (Distributions.jl / GLM.jl names) -----------------------
class _Dist:
    code = 0
    name = "Normal"

    def __repr__(self):
        return f"{self.name}()"


class Normal(_Dist):
    code, name = 0, "Normal"


class Bernoulli(_Dist):
    code, name = 1, "Bernoulli"


class Poisson(_Dist):
    code, name = 2, "Poisson"


class NegativeBinomial(_Dist):
    code, name = 3, "NegativeBinomial"

    def __init__(self, r=1.0, p=0.5):
        self.r, self.p = float(r), float(p)

    def __repr__(self):
        return f"NegativeBinomial(r={self.r}, p={self.p})"


class Gamma(_Dist):
    """loglik_obs(::Gamma, ...) src/utilities.jl:34 (shape 1/phi, scale mu*phi); use with LogLink or InverseLink."""
    code, name = 4, "Gamma"


class InverseGaussian(_Dist):
    """loglik_obs(::InverseGaussian, ...) src/utilities.jl:35."""
    code, name = 5, "InverseGaussian"


class MvNormal(_Dist):
    code, name = -1, "MvNormal"


class IdentityLink:
    code = 0

    def __repr__(self):
        return "IdentityLink()"


class LogitLink:
    code = 1

    def __repr__(self):
        return "LogitLink()"


class LogLink:
    code = 2

    def __repr__(self):
        return "LogLink()"


def _link(name, code):
    return type(name, (), {"code": code, "__repr__": lambda self: f"{name}()"})


# the remaining GLM.jl Link types a caller may pass as `l` (linkinv / mueta closed forms in csrc/fit_common.h)
ProbitLink = _link("ProbitLink", 3)
CloglogLink = _link("CloglogLink", 4)
CauchitLink = _link("CauchitLink", 5)
InverseLink = _link("InverseLink", 6)
InverseSquareLink = _link("InverseSquareLink", 7)
SqrtLink = _link("SqrtLink", 8)


def canonicallink(d):
    """GLM.canonicallink (default `l` of cv_iht / iht_run_many_models, cross_validation.jl:237)."""
    d = _inst(d)
    return {0: IdentityLink, 1: LogitLink, 2: LogLink, 3: LogLink, 4: InverseLink, 5: InverseSquareLink}[max(d.code, 0)]()


def _inst(x):
    return x() if isinstance(x, type) else x


# ---- design matrices -------------------------------------------------------------------
def read_bed(path, n):
    """PLINK .bed (SNP-major, header 6c 1b 01) -> (p, ceil(n/4)) uint8 column bytes.  The file is memory-mapped
    (as SnpArrays.jl does): a 125 GB .bed is never copied into Python memory, its pages stream through the
    upload pipeline of mih_snp_create."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        magic = f.read(3)
    if size < 3 or magic != b"\x6c\x1b\x01":
        raise ArgumentError(f"{path} is not a SNP-major PLINK .bed file")
    stride = (n + 3) // 4
    if (size - 3) % stride:
        raise DimensionMismatch(f"{path}: size does not match n={n}")
    if size == 3:
        return np.zeros((0, stride), dtype=np.uint8)
    return np.memmap(path, dtype=np.uint8, mode="r", offset=3, shape=((size - 3) // stride, stride))


def _scan_args(n, A, w, Z, eta=None, traits=False):
    """The arrays of a score_test* / set_test call on a matrix of n rows, as ctypes takes them: (A, w, Z, eta), float64.
    traits=True (score_test): A is n, or n x t, and goes in as n x t in Fortran order; a fifth value says whether it was 1-D.
    Otherwise A is one contiguous trait (n,).  Z (None: an intercept; 1-D: reshaped to n rows) is n x c in Fortran order.  w is
    (n,), or None for unit weights.  With eta (the saddlepoint and Firth calls) w and eta are both required, (n,): a None among
    them is refused for its shape like any other.  A wrong shape is a DimensionMismatch that names the argument."""
    def vec(name, v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.shape != (n,):
            raise DimensionMismatch(f"{name} has shape {v.shape}, expected ({n},)")
        return v
    if traits:
        A = np.asarray(A, dtype=np.float64)
        one = A.ndim == 1
        A = np.asfortranarray(A[:, None] if one else A)
        if A.ndim != 2 or A.shape[0] != n:
            raise DimensionMismatch(f"A has shape {A.shape}, expected {n} rows")
    else:
        A = vec("A", A)
    if eta is not None:
        w, eta = vec("w", w), vec("eta", eta)
    Z = np.ones((n, 1)) if Z is None else np.asarray(Z, dtype=np.float64)
    Z = np.asfortranarray(Z.reshape(n, -1) if Z.ndim == 1 else Z)
    if Z.ndim != 2 or Z.shape[0] != n:
        raise DimensionMismatch(f"Z has shape {Z.shape}, expected {n} rows")
    if eta is None and w is not None:
        w = vec("w", w)
    return (A, w, Z, eta, one) if traits else (A, w, Z, eta)


def _plain_out(p):
    """z, beta, se and neglog10p of a one-trait scan, for the library to fill"""
    return [np.empty(p) for _ in range(4)]


def _spa_out(p, on=True):
    """the saddlepoint outputs by their AssocResult names, in the order the library takes them (on=False: not asked for)"""
    return {"neglog10p_spa": np.empty(p) if on else None, "spa_state": np.empty(p, dtype=np.uint8) if on else None,
            "t_hat": np.empty((p, 2), order="F") if on else None}


def _null_scores(y, zc, d, l):
    """The null model of y ~ zc (fit_null) and what the score test takes of it: (null, A, w, rt).  A Normal trait with the
    identity link goes in with unit weights (w None), scaled by 1 / sqrt(phi): z is exact this way, and beta and se take the
    trait's rt = sqrt(phi) afterwards; null is then a list with one model per column of y, A is n x t and rt has t entries.
    Otherwise rt is None."""
    from .assoc import fit_null
    if isinstance(d, Normal) and (l is None or _inst(l).code == 0):
        cols = y.T if y.ndim == 2 else [y]
        nulls = [fit_null(col, zc, d, l) for col in cols]
        rt = np.sqrt(np.array([m.phi for m in nulls]))
        return nulls, np.stack([(col - m.mu) / r for col, m, r in zip(cols, nulls, rt)], axis=1), None, rt
    null = fit_null(y, zc, d, l)
    return null, null.A, null.w, None


def neglog10p(z):
    """-log10 of the two-sided normal p-value of every z, by the tail function of the library's scans (mih_neglog10p): finite
    far beyond where p underflows, NaN for a NaN."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    out = np.empty_like(z)
    _check(lib().mih_neglog10p(_p(z), z.size, _p(out)))
    return out


class _Mat:
    def __init__(self):
        self._h = C.c_void_p(None)
        self.n = self.p = 0

    def __del__(self):
        try:
            if self._h:
                lib().mih_mat_destroy(self._h)
                self._h = C.c_void_p(None)
        except Exception:
            pass

    @property
    def shape(self):
        return (self.n, self.p)

    def _dims(self):
        n, p = C.c_int64(0), C.c_int64(0)
        _check(lib().mih_mat_dims(self._h, C.byref(n), C.byref(p)))
        self.n, self.p = n.value, p.value

    # mul!(out, Transpose(x), r)
    def xtv(self, r, xtv_digits=None):
        r = np.asarray(r, dtype=np.float64)
        dg = _digits(xtv_digits)
        if r.ndim == 1:
            if r.size != self.n:
                raise DimensionMismatch(f"r has length {r.size}, expected {self.n}")
            r = np.ascontiguousarray(r)
            out = np.empty(self.p)
            if dg == 0:
                _check(lib().mih_xtv(self._h, _p(r), _p(out)))
            else:
                _check(lib().mih_xtv_batched_fmt(self._h, _p(r), 1, dg, _p(out)))
            return out
        if r.shape[0] != self.n:
            raise DimensionMismatch(f"R has {r.shape[0]} rows, expected {self.n}")
        R = np.asfortranarray(r)
        out = np.empty((self.p, R.shape[1]), order="F")
        _check(lib().mih_xtv_batched_fmt(self._h, _p(R), R.shape[1], dg, _p(out)))
        return out

    def score_test(self, A, w=None, Z=None, slice_rows=0, wsum=False):
        """The score test of every column given score residuals A (n or n x t), working weights w (None: ones) and covariates Z
        (None: an intercept) -- mih_assoc_score as it is.  Returns an AssocResult; wsum=True also keeps the class-weight sums
        W1, W2, Wm (p x 3) of a 2-bit matrix."""
        from .assoc import AssocResult
        A, w, Z, _, one = _scan_args(self.n, A, w, Z, traits=True)
        t, c = A.shape[1], Z.shape[1]
        z = np.empty((self.p, t), order="F"); beta = np.empty((self.p, t), order="F"); nlp = np.empty((self.p, t), order="F")
        se = np.empty(self.p)
        ws = np.empty((self.p, 3)) if wsum else None
        _check(lib().mih_assoc_score(self._h, _p(A), t, _p(w), _p(Z), c, int(slice_rows), _p(z), _p(beta), _p(se), _p(nlp), _p(ws)))
        if one:
            z, beta, nlp = z[:, 0].copy(), beta[:, 0].copy(), nlp[:, 0].copy()
        return AssocResult(z, beta, se, nlp, wsum=ws)

    def score_test_spa(self, A, w, Z, eta, cutoff=2.0, slice_rows=0):
        """The score test of every column for one Bernoulli trait with the logit link, with the saddlepoint p-value beside the
        normal one -- mih_assoc_score_spa as it is: A = y - mu, w = mu (1 - mu) and eta of the null fit, covariates Z (None: an
        intercept); columns with |z| >= cutoff are tried (inf: none).  Returns an AssocResult with neglog10p_spa, spa_state
        (0 not tried, 1 saddlepoint, 2 refused: the normal value) and t_hat (p x 2)."""
        from .assoc import AssocResult
        A, w, Z, eta = _scan_args(self.n, A, w, Z, eta=np.asarray(eta, dtype=np.float64))
        z, beta, se, nlp = _plain_out(self.p)
        sp = _spa_out(self.p)
        _check(lib().mih_assoc_score_spa(self._h, _p(A), _p(w), _p(Z), Z.shape[1], _p(eta), float(cutoff), int(slice_rows),
                                         _p(z), _p(beta), _p(se), _p(nlp), *map(_p, sp.values())))
        return AssocResult(z, beta, se, nlp, **sp)

    def score_test_firth(self, A, w, Z, eta, cutoff=2.0, slice_rows=0, spa=False):
        """The score test of every column for one Bernoulli trait with the logit link, with the Firth-penalised effect size and
        likelihood-ratio p-value of the columns with |z| >= cutoff beside it -- mih_assoc_score_firth as it is; the arguments are
        those of score_test_spa.  Returns an AssocResult with beta_firth, se_firth, neglog10p_firth, firth_state (0 not tried,
        1 penalised-likelihood values, 2 refused: the plain values) and firth_evals; spa=True runs the saddlepoint pass on the
        same selection in the same call and fills neglog10p_spa, spa_state and t_hat as score_test_spa does."""
        from .assoc import AssocResult
        A, w, Z, eta = _scan_args(self.n, A, w, Z, eta=np.asarray(eta, dtype=np.float64))
        z, beta, se, nlp = _plain_out(self.p)
        bf = np.empty(self.p); sf = np.empty(self.p); nf = np.empty(self.p)
        fstate = np.empty(self.p, dtype=np.uint8)
        fevals = np.empty(self.p, dtype=np.int32)
        sp = _spa_out(self.p, on=spa)
        _check(lib().mih_assoc_score_firth(self._h, _p(A), _p(w), _p(Z), Z.shape[1], _p(eta), float(cutoff), int(slice_rows),
                                           _p(z), _p(beta), _p(se), _p(nlp), _p(bf), _p(sf), _p(nf), _p(fstate), _p(fevals),
                                           *map(_p, sp.values())))
        return AssocResult(z, beta, se, nlp, beta_firth=bf, se_firth=sf, neglog10p_firth=nf, firth_state=fstate, firth_evals=fevals, **sp)

    def assoc(self, y, z=None, *, d=None, l=None, slice_rows=0, spa=False, spa_cutoff=2.0, firth=False, firth_cutoff=2.0, kinship=None):
        """The marginal association scan: the null model y ~ z (fit_null; z=None: an intercept) and the score test of every column
        against it.  y may be n x t for Normal traits: they share the weights, and each trait's dispersion scales its own
        statistics.  Returns an AssocResult whose `null` is the NullModel (a list of them for several traits).  spa=True (one
        Bernoulli trait, logit link): the saddlepoint p-value of the columns with |z| >= spa_cutoff beside the normal one
        (score_test_spa).  firth=True (likewise): the Firth-penalised effect size and likelihood-ratio p-value of the columns with
        |z| >= firth_cutoff (score_test_firth); with spa=True too both run in one call, on one selection: spa_cutoff must then
        equal firth_cutoff.
        kinship (a SnpLinAlg or DosageMatrix, one Normal trait with the identity link, neither spa nor firth): the mixed-model
        scan, which keeps relatives in the sample.  True fits the variance-component null model on the kinship matrix of this
        matrix's columns (lmm_null(y, z)); an LmmNull reuses one -- the usual case, Phi from pruned markers and the scan over
        all columns.  The scan is score_test(null.Py, None, z) as it is, then, in this order, z / sqrt(gamma), beta / gamma,
        se / sqrt(gamma) with the variance ratio gamma of the null model (GRAMMAR-Gamma, SAIGE), and -log10 p recomputed from
        the rescaled z (neglog10p).  `null` of the result is the LmmNull."""
        d = Normal() if d is None else _inst(d)
        if kinship is not None and kinship is not False:
            return self._assoc_kinship(y, z, d, l, slice_rows, spa, firth, kinship)
        opt = "firth=True" if firth else "spa=True" if spa else None
        if opt:
            if not isinstance(d, Bernoulli) or (l is not None and _inst(l).code != 1):
                raise ArgumentError(f"{opt} is offered for a Bernoulli trait with the logit link only, got "
                                    f"{type(d).__name__}" + ("" if l is None else f" with {type(_inst(l)).__name__}"))
            if spa and firth and float(spa_cutoff) != float(firth_cutoff):
                raise ArgumentError(f"spa=True with firth=True runs both passes on one selection: spa_cutoff ({spa_cutoff}) "
                                    f"must equal firth_cutoff ({firth_cutoff})")
        y, zc = self._trait_args(y, z, d, opt)
        null, A, w, rt = _null_scores(y, zc, d, l)
        if firth:
            res = self.score_test_firth(A, w, zc, null.eta, firth_cutoff, slice_rows, spa=bool(spa))
        elif spa:
            res = self.score_test_spa(A, w, zc, null.eta, spa_cutoff, slice_rows)
        else:
            res = self.score_test(A, w, zc, slice_rows)
        if rt is not None:
            res.beta = res.beta * rt[None, :]
            res.se = res.se[:, None] * rt[None, :]
            if y.ndim == 1:
                null = null[0]
                res.z, res.beta, res.se, res.neglog10p = res.z[:, 0].copy(), res.beta[:, 0].copy(), res.se[:, 0].copy(), res.neglog10p[:, 0].copy()
        res.null = null
        return res

    def _assoc_kinship(self, y, z, d, l, slice_rows, spa, firth, kinship):
        from .assoc import LmmNull
        if not isinstance(self, _Kinship):
            raise ArgumentError("kinship= needs a genotype matrix (SnpLinAlg or DosageMatrix), not a DenseMatrix")
        if not isinstance(d, Normal) or (l is not None and _inst(l).code != 0):
            raise ArgumentError(f"kinship= is offered for a Normal trait with the identity link only, got {type(d).__name__}"
                                + ("" if l is None else f" with {type(_inst(l)).__name__}"))
        if spa or firth:
            raise ArgumentError("kinship= takes neither spa=True nor firth=True: they belong to Bernoulli traits")
        y, zc = self._trait_args(y, z, d, "kinship=")
        if kinship is True:
            null = self.lmm_null(y, zc)
        elif isinstance(kinship, LmmNull):
            null = kinship
            if null.Py.shape[0] != self.n:
                raise DimensionMismatch(f"the null model has {null.Py.shape[0]} samples, expected {self.n}")
        else:
            raise ArgumentError(f"kinship must be True or an LmmNull, got {type(kinship).__name__}")
        res = self.score_test(null.Py, None, zc, slice_rows)
        res.z = res.z / np.sqrt(null.gamma)
        res.beta = res.beta / null.gamma
        res.se = res.se / np.sqrt(null.gamma)
        res.neglog10p = neglog10p(res.z)
        res.null = null
        return res

    def _trait_args(self, y, z, d, one=None):
        """y (n, or n x t for Normal traits; one: the caller or option that takes one trait only) and the covariates (None: an
        intercept) as fit_null takes them."""
        y = np.asarray(y, dtype=np.float64)
        if one is not None and y.ndim != 1:
            raise ArgumentError(f"{one} takes one trait")
        if y.ndim == 2 and not isinstance(d, Normal):
            raise ArgumentError("several traits at once are offered for Normal traits only")
        if y.shape[0] != self.n:
            raise DimensionMismatch(f"y has {y.shape[0]} rows, expected {self.n}")
        return y, np.ones((self.n, 1)) if z is None else np.asarray(z, dtype=np.float64).reshape(self.n, -1)

    def set_test(self, A, w, Z, sets, omega=None, slice_rows=0, cov=False, skato=False, rho=None):
        """Burden and SKAT tests of sets of columns on top of the score test of every column -- mih_assoc_sets as it is: score
        residuals A (n: one trait), working weights w (None: ones) and covariates Z (None: an intercept) as score_test takes
        them.  sets: a list of index arrays (0-based columns, strictly ascending within a set, at most 128), or the pair
        (set_ptr, set_col); omega: one weight >= 0 per entry, as a list of arrays like sets or one flat array (None: ones).
        Returns a SetResult; cov=True also keeps every set's covariance K of the scores (a list of m_s x m_s arrays over the
        entries, NaN in the rows and columns of entries that are not members).  skato=True adds SKAT-O, the optimal combination
        of the two tests over the grid rho (ascending values in [0, 1], at most 16; None: SKAT's 0, 0.01, 0.04, 0.09, 0.16, 0.25,
        0.5, 1) -- mih_assoc_sets_skato as it is: the SetResult then has neglog10p_skato, skato_rho, skato_state, neglog10p_rho
        and lambda_rho; every other output is the same bits as without it."""
        from .assoc import AssocResult, SetResult
        if rho is not None and not skato:
            raise ArgumentError("rho is the grid of SKAT-O: give skato=True with it")
        A, w, Z, _ = _scan_args(self.n, A, w, Z)
        if isinstance(sets, tuple):                     # a tuple is (set_ptr, set_col), a list is a list of sets
            if len(sets) != 2:
                raise ArgumentError("sets as a tuple must be (set_ptr, set_col)")
            ptr = np.ascontiguousarray(sets[0], dtype=np.int64)
            col = np.ascontiguousarray(sets[1], dtype=np.int32)
        else:
            parts = [np.asarray(s, dtype=np.int64).reshape(-1) for s in sets]
            ptr = np.zeros(len(parts) + 1, dtype=np.int64)
            if parts:
                ptr[1:] = np.cumsum([q.size for q in parts])
            col = (np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64))
            if col.size and (col.min() < -2 ** 31 or col.max() >= 2 ** 31):
                raise ArgumentError("a set names a column outside the int32 range")
            col = np.ascontiguousarray(col, dtype=np.int32)
        ns = ptr.size - 1
        if ptr.ndim != 1 or col.ndim != 1 or ptr.size < 1 or int(ptr[-1]) != col.size:
            raise ArgumentError(f"set_ptr must hold nsets + 1 offsets ending at the {col.size} entries of set_col")
        if omega is None:
            om = np.ones(col.size)
        elif isinstance(omega, (list, tuple)) and len(omega) and np.ndim(omega[0]) >= 1:
            om = np.concatenate([np.asarray(o, dtype=np.float64).reshape(-1) for o in omega])
        else:
            om = np.ascontiguousarray(omega, dtype=np.float64).reshape(-1)
        om = np.ascontiguousarray(om, dtype=np.float64)
        if om.size != col.size:
            raise DimensionMismatch(f"omega has {om.size} entries, the sets have {col.size}")
        z, beta, se, nlp = _plain_out(self.p)
        k = max(ns, 0)
        m_used = np.empty(k, dtype=np.int32); state = np.empty(k, dtype=np.uint8)
        bz = np.empty(k); bn = np.empty(k); sq = np.empty(k); sn = np.empty(k)
        lam = np.empty(col.size)
        sizes = np.diff(ptr)
        cv = np.empty(int((sizes * sizes).sum())) if cov else None
        extra = None
        if skato:
            grid = None if rho is None else np.ascontiguousarray(rho, dtype=np.float64).reshape(-1)
            nr = 8 if grid is None else grid.size
            if not 1 <= nr <= 16:
                raise ArgumentError(f"rho must hold 1 to 16 grid values, got {nr}")
            so = np.empty(k); sr = np.empty(k); ss = np.empty(k, dtype=np.uint8); pr = np.empty((k, nr)); lr = np.empty((nr + 1, col.size))
            _check(lib().mih_assoc_sets_skato(self._h, _p(A), _p(w), _p(Z), Z.shape[1], int(slice_rows), ns, _p(ptr), _p(col), _p(om), nr, _p(grid),
                                              _p(z), _p(beta), _p(se), _p(nlp), _p(m_used), _p(bz), _p(bn), _p(sq), _p(sn), _p(state), _p(lam), _p(cv),
                                              _p(so), _p(sr), _p(ss), _p(pr), _p(lr)))
            extra = (so, sr, ss, pr, lr)
        else:
            _check(lib().mih_assoc_sets(self._h, _p(A), _p(w), _p(Z), Z.shape[1], int(slice_rows), ns, _p(ptr), _p(col), _p(om),
                                        _p(z), _p(beta), _p(se), _p(nlp), _p(m_used), _p(bz), _p(bn), _p(sq), _p(sn), _p(state), _p(lam), _p(cv)))
        covs = None
        if cov:
            off = np.concatenate([[0], np.cumsum(sizes * sizes)]).astype(np.int64)
            covs = [cv[off[s]:off[s + 1]].reshape(sizes[s], sizes[s]).copy() for s in range(ns)]
        return SetResult(ptr, col, om, m_used, bz, bn, sq, sn, state, lam, covs, AssocResult(z, beta, se, nlp), skato=extra)

    def assoc_sets(self, y, z, sets, *, d=None, l=None, weights="beta", beta=(1, 25), max_maf=None, slice_rows=0, cov=False, skato=False, rho=None):
        """Gene-based burden and SKAT tests: the null model y ~ z (fit_null, as assoc fits it; z=None: an intercept; a Normal
        trait is scaled by 1 / sqrt(phi) as in assoc) and set_test against it.  weights="beta": omega_j is the Beta(a, b) density
        at the minor allele frequency of column j, beta = (a, b) -- SKAT's default (1, 25) -- divided by sinv_j on a scaled
        handle.  The argument: on a scaled handle the column is x~_j = (g_j - mu_j) sinv_j; with an intercept in z the centring is
        projected out, so U~_j = sinv_j U_j and K~_jk = sinv_j sinv_k K_jk for the raw genotypes' U and K, and omega_j / sinv_j
        on the scaled column gives omega_j U_j and omega_j omega_k K_jk: SKAT's weighting of the raw genotypes, whatever the
        flags of the handle.  weights may be an array of p weights instead (used as they are; a DenseMatrix, which has no allele
        frequencies, takes only that).  max_maf: entries whose minor allele frequency is above it (or not a number) are dropped
        from their sets.  skato, rho: SKAT-O as set_test offers it.  Returns a SetResult whose `assoc.null` is the NullModel."""
        d = Normal() if d is None else _inst(d)
        y, zc = self._trait_args(y, z, d, "assoc_sets")
        parts = [np.asarray(s, dtype=np.int64).reshape(-1) for s in sets]
        for q in parts:
            if q.size and (q.min() < 0 or q.max() >= self.p):
                raise ArgumentError(f"a set names column {int(q.min() if q.min() < 0 else q.max())}, outside [0, {self.p})")
        has_maf = hasattr(self, "_allele_maf")
        maf = self._allele_maf() if has_maf else None
        if isinstance(weights, str):
            if weights != "beta":
                raise ArgumentError(f"weights must be \"beta\" or an array of {self.p} weights, got {weights!r}")
            if not has_maf:
                raise ArgumentError("a DenseMatrix has no allele frequencies: give weights as an array")
            a, b = float(beta[0]), float(beta[1])
            with np.errstate(all="ignore"):
                lg = math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b)
                om = np.exp(lg + (a - 1.0) * np.log(maf) + (b - 1.0) * np.log1p(-maf))
            if a == 1.0:
                om = np.where(maf == 0.0, np.exp(lg), om)
            scaled = isinstance(self, DosageMatrix) or bool(getattr(self, "scale", False))
            if scaled:
                om = om / self.mu_sigma()[1]
            om = np.where(np.isfinite(om), om, 0.0)
        else:
            om = np.asarray(weights, dtype=np.float64)
            if om.shape != (self.p,):
                raise DimensionMismatch(f"weights has shape {om.shape}, expected ({self.p},)")
        if max_maf is not None:
            if not has_maf:
                raise ArgumentError("a DenseMatrix has no allele frequencies: max_maf cannot be applied")
            parts = [q[maf[q] <= float(max_maf)] for q in parts]
        null, A, w, rt = _null_scores(y, zc, d, l)
        if rt is not None:
            null, A, rt = null[0], A[:, 0], rt[0]
        res = self.set_test(A, w, zc, parts, [om[q] for q in parts], slice_rows=slice_rows, cov=cov, skato=skato, rho=rho)
        if rt is not None:
            res.assoc.beta, res.assoc.se = res.assoc.beta * rt, res.assoc.se * rt
        res.assoc.null = null
        return res

    # mul!(out, x, B) for a dense B: offered by the 2-bit matrix (SnpLinAlg.xb); the other kinds say so
    def xb(self, B, xtv_digits=None, center=None, scale=None, impute=None):
        raise ArgumentError(f"xb (the dense product X B) is offered for the 2-bit matrix (SnpLinAlg) only, not for {type(self).__name__}")

    def score(self, weights, cols=None, average=False):
        raise ArgumentError(f"score is offered for the 2-bit matrix (SnpLinAlg) only, not for {type(self).__name__}")

    def xv_sparse(self, idx, val):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        val = np.ascontiguousarray(val, dtype=np.float64)
        out = np.empty(self.n)
        _check(lib().mih_xv_sparse(self._h, _p(idx), _p(val), idx.size, _p(out)))
        return out

    def bench_xtv(self, variant=-1, iters=10, warmup=2, seed=1, xtv_digits=None):
        """ms per single-residual pass (the workspace of a single fit) and a checksum of the result."""
        return self.bench_xtv_batched(1, variant=variant, iters=iters, warmup=warmup, seed=seed, xtv_digits=xtv_digits)

    def bench_xtv_batched(self, m, max_fused=4, variant=-1, iters=5, warmup=1, seed=1, xtv_digits=None):
        """`variant` / `max_fused` other than the defaults are knobs of the measurement build (MENDELIHT_HIP_PROBES=1)."""
        if variant != -1 or max_fused != 4 or using_probes():
            probe_set(variant=variant, max_fused=max_fused)
        ms, cs = C.c_float(0), C.c_double(0)
        try:
            _check(lib().mih_bench_xtv(self._h, _digits(xtv_digits), m, iters, warmup, seed, C.byref(ms), C.byref(cs)))
        finally:
            if using_probes():
                probe_set(variant=-1, max_fused=4)
        return ms.value, cs.value

    def algorithmic_bytes(self, m=1):
        b = C.c_double(0)
        _check(lib().mih_xtv_algorithmic_bytes(self._h, m, C.byref(b)))
        return b.value


# The `reserve` argument of SnpLinAlg when the caller leaves it out.  False: the library's own policy (a 2-bit matrix of 4 GiB or
# more keeps a reserve of device memory for its fits, smaller ones allocate per fit).  True: every matrix asks for a reserve
# (mih_mat_reserve) -- tests/conftest.py sets it so that small test matrices run the pool / arena code of a 125 GB matrix.
RESERVE_BY_DEFAULT = False


_GRM_METHODS = {"GRM": 0, "Robust": 1}

PcaResult = collections.namedtuple("PcaResult", "values vectors residuals iters converged")
SolveResult = collections.namedtuple("SolveResult", "x iters converged residuals")


class _Kinship:
    """grm / related_pairs / pca of the genotype handles (csrc/grm.hip: mih_grm, mih_grm_pairs; csrc/pca.hip: mih_grm_eig)."""

    def _grm_args(self, method, minmaf, cols):
        if isinstance(method, str):
            if method not in _GRM_METHODS:
                raise ArgumentError(f"method must be 'GRM' or 'Robust', got {method!r}"
                                    + (" (MoM is not offered)" if method == "MoM" else ""))
            method = _GRM_METHODS[method]
        if cols is None:
            with np.errstate(invalid="ignore"):
                ck = (self._allele_maf() >= minmaf).astype(np.uint8)              # (NaN fails)
        else:
            ck = SnpLinAlg._sel_mask(cols, self.p, "column")
        return int(method), ck

    def grm(self, method="GRM", minmaf=0.01, cols=None, panel_cols=0):
        """SnpArrays.grm(x; method, minmaf): the (n, n) float64 kinship matrix of the samples, made on the device (mih_grm).
        With mu_j and sinv_j of mu_sigma() and c_ij = g_ij - mu_j (0 for a missing genotype: imputed by the mean),
        method "GRM" is Phi = X X' / (2 m) over the m kept columns with x_ij = c_ij sinv_j, the matrix a fit sees, and "Robust"
        is Phi = C C' / (2 sum_j mu_j (1 - mu_j / 2)).  SnpArrays' third method, "MoM", is out of scope and refused.
        cols: a boolean mask or a strictly increasing index array of the columns to use; None keeps the columns with
        maf >= minmaf (a NaN maf fails), SnpArrays' default -- for a DosageMatrix the same rule on min(mu / 2, 1 - mu / 2).
        panel_cols: kept columns decoded at a time, 0 = the library's rule.  Float64 on the f64 matrix pipe, every entry summed
        over the columns in ascending order: Phi equals its transpose and a second call bit for bit.  The device needs
        8 n^2 bytes for the call; MemoryError names the need and what is free."""
        method, ck = self._grm_args(method, minmaf, cols)
        try:
            phi = np.empty((self.n, self.n))
        except MemoryError:
            phi = None                       # the library refuses first, with its byte counts, if the device cannot hold it either
        rc = lib().mih_grm(self._h, _p(ck), method, int(panel_cols), _p(phi))
        if phi is None and rc == 2:
            raise MemoryError(f"the host cannot hold the {self.n} x {self.n} matrix: use related_pairs")
        _check(rc)
        return phi

    def related_pairs(self, threshold=0.125, method="GRM", minmaf=0.01, cols=None, panel_cols=0, cap=None, _first_cap=None):
        """The pairs of samples with Phi_ik > threshold (strictly) of grm(method, minmaf, cols), found on the device so that no
        n x n array reaches the host (mih_grm_pairs): (i, k, phi, diag) with i < k in the order (i, k), phi bit-equal to the
        entries of grm(), and diag the n values Phi_ii.  cap: the most pairs to return; None starts with room for
        max(1024, 4 n) and calls once more with the count found if that was too small.
        The screen of manuscript/UKBB_metabolomic/data_process.jl:84-101 is then
            i, k, _, _ = x.related_pairs(0.125); mask = np.zeros(x.n, dtype=bool); mask[k] = True
            x = x.subset(rows=~mask)"""
        method, ck = self._grm_args(method, minmaf, cols)
        room = int(cap) if cap is not None else int(_first_cap) if _first_cap is not None else max(1024, 4 * self.n)
        diag = np.empty(self.n)
        for _ in range(2):
            i, k, phi = np.empty(max(room, 1), dtype=np.int64), np.empty(max(room, 1), dtype=np.int64), np.empty(max(room, 1))
            count = C.c_int64(0)
            _check(lib().mih_grm_pairs(self._h, _p(ck), method, int(panel_cols), float(threshold), room, _p(i), _p(k), _p(phi),
                                       C.byref(count), _p(diag)))
            if cap is not None or count.value <= room:
                break
            room = count.value
        got = min(count.value, room)
        return i[:got], k[:got], phi[:got], diag

    def pca(self, k, method="GRM", minmaf=0.01, cols=None, panel_cols=0, tol=1e-10, max_iter=500, block=0, seed=0):
        """The k leading principal components of the samples: the k largest eigenvalues of grm(method, minmaf, cols) and their
        eigenvectors, extracted on the device without the n x n matrix leaving it (mih_grm_eig) -- what PLINK and GCTA compute,
        and the step after related_pairs in manuscript/UKBB_metabolomic/data_process.jl:103-110.  As covariates of a fit:
            z = np.column_stack([np.ones(x.n), x.pca(10).vectors])
        Returns PcaResult(values (k,) descending, vectors (n, k), residuals (k,), iters, converged): vectors[:, i] is the unit
        eigenvector of values[i] with its entry of largest magnitude (the lowest index on a tie) positive; residuals[i] is
        |Phi u_i - lambda_i u_i|_2 as the device evaluated it; converged says max(residuals) <= tol * values[0].  Reaching
        max_iter is not an error: the last Ritz pairs come back with converged=False and their residuals.
        method, minmaf, cols, panel_cols: those of grm().  1 <= k <= min(n, 64).  block: the columns of the blocked subspace
        iteration, 0 = round_up(max(2 k, k + 8), 16), else k <= block <= 128; seed: of the hashed start block.  The same
        arguments give the same bits, whatever panel_cols; another seed or block agrees within the tolerance.  A matrix of
        numerical rank below k raises ArgumentError naming the rank.  The device needs 8 n^2 bytes for the call, like grm():
        about 170 000 samples on a 288 GB device; MemoryError names the need and what is free."""
        method, ck = self._grm_args(method, minmaf, cols)
        k = int(k)
        values, vectors, residuals = np.empty(max(k, 0)), np.empty((max(k, 0), self.n)), np.empty(max(k, 0))
        iters, converged = C.c_int32(0), C.c_int32(0)
        _check(lib().mih_grm_eig(self._h, _p(ck), method, int(panel_cols), k, int(block), float(tol), int(max_iter),
                                 int(seed) & 0xFFFFFFFFFFFFFFFF, _p(values), _p(vectors), _p(residuals), C.byref(iters), C.byref(converged)))
        return PcaResult(values, vectors.T, residuals, iters.value, bool(converged.value))

    def kinship_solve(self, B, tau_e, tau_g, method="GRM", minmaf=0.01, cols=None, panel_cols=0, tol=1e-10, max_iter=500):
        """X ~ V^-1 B with V = tau_e I + tau_g Phi, Phi = grm(method, minmaf, cols): the linear solves of a mixed model on the
        kinship matrix -- what SAIGE, fastGWA and GMMAT run inside their variance-component null model -- made on the device
        without Phi leaving it and without an n x n factorisation (mih_grm_solve).  B: (n,) or (n, m), 1 <= m <= 128;
        tau_e > 0, tau_g >= 0.  Returns SolveResult(x like B, iters (m,), converged (m,) bool, residuals (m,)): a conjugate
        gradient with the Jacobi preconditioner diag V from x = 0, every column with its own scalars; column c stops when its
        recurrence residual reaches |r|_2 <= tol |b|_2, and residuals[c] is the true |b - V x|_2, formed with one more product.
        Reaching max_iter is not an error: converged[c] is False and the last iterate comes back with its residual.  A zero
        column gives x = 0 after 0 iterations, converged.  A column of x is bit for bit the same whatever the other columns of
        B, whatever panel_cols, and on a second call.  method, minmaf, cols, panel_cols: those of grm().  The device needs
        8 n^2 bytes for the call, like grm(), plus six blocks of n x m; MemoryError names the need and what is free."""
        method, ck = self._grm_args(method, minmaf, cols)
        B = np.asarray(B, dtype=np.float64)
        if B.ndim not in (1, 2) or B.shape[0] != self.n:
            raise ArgumentError(f"B must be ({self.n},) or ({self.n}, m), got {B.shape}")
        m = 1 if B.ndim == 1 else B.shape[1]
        b = np.ascontiguousarray(B.reshape(self.n, m).T)                          # (m, n) row-major = n x m column-major
        x, iters, conv, res = np.empty((max(m, 1), self.n)), np.zeros(max(m, 1), dtype=np.int32), np.zeros(max(m, 1), dtype=np.int32), np.empty(max(m, 1))
        _check(lib().mih_grm_solve(self._h, _p(ck), method, int(panel_cols), float(tau_e), float(tau_g), _p(b), m, float(tol), int(max_iter),
                                   _p(x), _p(iters), _p(conv), _p(res)))
        return SolveResult(x[0].copy() if B.ndim == 1 else np.ascontiguousarray(x.T), iters, conv.astype(bool), res)

    def lmm_markers(self, markers=30, min_mac=20, seed=0):
        """The columns whose variance ratios calibrate the mixed-model scan: among the columns with a minor-allele count of at
        least min_mac, min(markers, their number) drawn without replacement by numpy's default_rng(seed), in ascending order."""
        cand = np.flatnonzero(self._minor_allele_counts() >= float(min_mac))
        if cand.size == 0:
            raise ArgumentError(f"no column has a minor-allele count of at least {min_mac}")
        take = min(int(markers), cand.size)
        if take < 1 or take > 128:
            raise ArgumentError(f"markers must be between 1 and 128, got {markers}")
        return np.sort(np.random.default_rng(int(seed)).choice(cand, size=take, replace=False))

    def lmm_null(self, y, z=None, *, method="GRM", minmaf=0.01, cols=None, panel_cols=0, probes=30, markers=30, min_mac=20, seed=0,
                 tol=1e-5, max_iter=50, cg_tol=1e-10, cg_max_iter=500, G=None):
        """The variance-component null model of a mixed-model association scan for one Normal trait: y = z alpha + g + e with
        g ~ N(0, tau_g Phi), Phi = grm(method, minmaf, cols), and e ~ N(0, tau_e I), fitted on the device by average-information
        REML with Hutchinson traces on `probes` Rademacher vectors (mih_lmm_null; the relatives stay in the sample, as in SAIGE,
        fastGWA and GMMAT).  z: the covariates with the intercept among them, None = an intercept.  Returns an LmmNull: tau
        (tau_e, tau_g), h2, alpha, Py (the scan's score residuals), gamma (the variance ratio that calibrates the scan) with its
        ratios and their coefficient of variation ratio_cv, trace, tau_path (every iterate), iters, state (1 converged, 2 on the
        boundary tau_g = 0, 0 max_iter reached: not an error), cg_iters and worst_residual (the largest relative true residual
        of any solve).  The variance ratios are taken on the columns lmm_markers(markers, min_mac, seed), decoded on the host
        and imputed by the mean; G (n x R, R <= 128) gives the columns instead.  tol, max_iter: of the REML iteration;
        cg_tol, cg_max_iter: of its solves (kinship_solve).  The same arguments give the same bits, whatever panel_cols.  Usually
        Phi comes from pruned markers and the scan runs over all: null = x.lmm_null(y, z, cols=pruned); x.assoc(y, z, kinship=null)."""
        from .assoc import LmmNull
        method, ck = self._grm_args(method, minmaf, cols)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.ndim != 1:
            raise ArgumentError("lmm_null takes one trait")
        if y.shape[0] != self.n:
            raise DimensionMismatch(f"y has {y.shape[0]} rows, expected {self.n}")
        zc = np.ones((self.n, 1)) if z is None else np.asarray(z, dtype=np.float64).reshape(self.n, -1)
        if G is None:
            marker_cols = self.lmm_markers(markers, min_mac, seed)
            G = self._marker_genotypes(marker_cols)
        else:
            marker_cols, G = None, np.asarray(G, dtype=np.float64).reshape(self.n, -1)
        c, R, probes, max_iter = zc.shape[1], G.shape[1], int(probes), int(max_iter)
        if max_iter < 1:
            raise ArgumentError(f"max_iter must be at least 1, got {max_iter}")
        zf, gf = np.ascontiguousarray(zc.T), np.ascontiguousarray(G.T)          # column-major
        tau, alpha, py, ratios, trace = np.empty(2), np.empty(max(c, 1)), np.empty(self.n), np.empty(max(R, 1)), np.empty(2)
        path = np.full((max_iter + 1, 2), np.nan)
        gamma, dbar, worst = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
        iters, state, cg = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        _check(lib().mih_lmm_null(self._h, _p(ck), method, int(panel_cols), _p(y), _p(zf), c, probes, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                  _p(gf), R, float(tol), max_iter, float(cg_tol), int(cg_max_iter), _p(tau), _p(alpha), _p(py), C.byref(gamma),
                                  _p(ratios), _p(trace), C.byref(dbar), _p(path), C.byref(iters), C.byref(state), C.byref(cg), C.byref(worst)))
        return LmmNull(tau, alpha[:c], py, gamma.value, ratios[:R], trace, dbar.value, path[:iters.value + 1], iters.value, state.value,
                       cg.value, worst.value, marker_cols, zc)


class SnpLinAlg(_Mat, _Kinship):
    """SnpLinAlg{Float64}(s::SnpArray; model=ADDITIVE_MODEL, center, scale, impute) on the GPU."""

    def _reserve(self, reserve):
        if reserve:
            _check(lib().mih_mat_reserve(self._h, 0))
        elif reserve is None and RESERVE_BY_DEFAULT:
            lib().mih_mat_reserve(self._h, 0)          # best effort: a crowded device keeps the per-fit allocations

    def __init__(self, bed, n=None, center=False, scale=False, impute=True, device=0, _handle=None, dtype=np.float64, reserve=None):
        """dtype: the element type T of SnpLinAlg{T} (np.float64 or np.float32, src/MendelIHT.jl:39).  The device arithmetic is
        the same for both (exact fixed point + Float64); with float32 the models fit_iht / cv_iht return are cast to float32.
        reserve: True asks for the reserve of device memory a large matrix keeps for its fits (mih_mat_reserve), None = RESERVE_BY_DEFAULT."""
        super().__init__()
        self.center, self.scale, self.impute = bool(center), bool(scale), bool(impute)
        self.device = device
        self.dtype = np.dtype(dtype).type
        if self.dtype not in (np.float64, np.float32):
            raise ArgumentError("SnpLinAlg{T}: T must be Float64 or Float32")
        if _handle is not None:
            self._h = _handle
            self._dims()
            return
        if isinstance(bed, (str, os.PathLike)):
            if n is None:
                raise ArgumentError("n (number of samples) is required with a .bed path")
            bed = read_bed(bed, n)
        cols = np.ascontiguousarray(bed, dtype=np.uint8)
        if cols.ndim != 2:
            raise DimensionMismatch("bed columns must be a (p, stride) uint8 array")
        if n is None:
            raise ArgumentError("n (number of samples) is required")
        h = C.c_void_p(None)
        _check(lib().mih_snp_create(_p(cols), n, cols.shape[0], cols.shape[1], int(center), int(scale),
                                    int(impute), 32 if self.dtype is np.float32 else 64, device, C.byref(h)))
        self._h = h
        self._dims()
        self._reserve(reserve)

    @classmethod
    def synthetic(cls, n, p, seed=2024, missing_rate=0.0, center=True, scale=True, impute=True, device=0,
                  col_offset=0, reserve=None):
        """Columns [col_offset, col_offset + p) of the seeded synthetic SnpArray (col_offset > 0: one shard)."""
        h = C.c_void_p(None)
        _check(lib().mih_snp_create_synthetic_shard(n, p, int(col_offset), seed, float(missing_rate), int(center),
                                                    int(scale), int(impute), device, C.byref(h)))
        x = cls(None, center=center, scale=scale, impute=impute, device=device, _handle=h)
        x._reserve(reserve)
        return x

    def score_image(self, mode="query", max_hom_fraction=0.0):
        """The score image of the matrix (mih_mat_score_image): a derived image only the single-residual X'r pass of a fit reads
        (residual format 428), with the columns that hold at most max_hom_fraction * n dosage-2 entries at one bit per genotype.
        mode "build" (max_hom_fraction <= 0: the library's default), "release" or "query"; returns (bytes, one-bit columns) of the
        image the matrix has afterwards, (0, 0) if none.  Results are bit for bit those of the 2-bit pass."""
        code = {"query": 0, "build": 1, "release": 2}[mode]
        nbytes, c1 = C.c_int64(0), C.c_int64(0)
        _check(lib().mih_mat_score_image(self._h, code, float(max_hom_fraction), C.byref(nbytes), C.byref(c1)))
        return nbytes.value, c1.value

    def mu_sigma(self):
        mu, s = np.empty(self.p), np.empty(self.p)
        _check(lib().mih_snp_mu_sigma(self._h, _p(mu), _p(s)))
        return mu, s

    def export_bed(self):
        out = np.empty((self.p, (self.n + 3) // 4), dtype=np.uint8)
        _check(lib().mih_snp_export_bed(self._h, _p(out)))
        return out

    # ---- quality control and sample selection on the device (csrc/qc.hip) ----
    @staticmethod
    def _sel_indices(sel, length, what):
        """A boolean mask or an index array as int64 indices (None: everything).  The order and range of an index array are
        left to whoever takes it."""
        if sel is None:
            return None
        sel = np.asarray(sel)
        if sel.dtype == np.bool_:
            if sel.shape != (length,):
                raise DimensionMismatch(f"the {what} mask has shape {sel.shape}, expected ({length},)")
            return np.flatnonzero(sel).astype(np.int64)
        if sel.ndim != 1 or not (np.issubdtype(sel.dtype, np.integer) or sel.size == 0):
            raise ArgumentError(f"the {what} selection must be a boolean mask or a one-dimensional array of indices")
        return np.ascontiguousarray(sel, dtype=np.int64)

    @classmethod
    def _sel_mask(cls, sel, length, what):
        """The same selection as a byte mask for mih_snp_counts (None: everything)."""
        idx = cls._sel_indices(sel, length, what)
        if idx is None:
            return None
        if idx.size and (idx.min() < 0 or idx.max() >= length):
            raise ArgumentError(f"a {what} index is outside 0 .. {length - 1}")
        if np.any(np.diff(idx) <= 0):
            raise ArgumentError(f"the {what} indices must be strictly increasing")
        mask = np.zeros(length, dtype=np.uint8)
        mask[idx] = 1
        return mask

    def counts(self, rows=None, cols=None):
        """(col_counts (p, 4) int32: n0, n1, n2, nmiss of every kept column over the kept rows, zeros for a column that is not
        kept; row_missing (n,) int32: the missing genotypes of every kept row among the kept columns, 0 for a row that is not
        kept).  rows, cols: boolean masks or strictly increasing index arrays, None = all.  Counted on the device
        (mih_snp_counts); the integers are exact."""
        rk, ck = self._sel_mask(rows, self.n, "row"), self._sel_mask(cols, self.p, "column")
        col_counts, row_missing = np.empty((self.p, 4), dtype=np.int32), np.empty(self.n, dtype=np.int32)
        _check(lib().mih_snp_counts(self._h, _p(rk), _p(ck), _p(col_counts), _p(row_missing)))
        return col_counts, row_missing

    def maf(self, rows=None):
        """SnpArrays.maf over the kept rows: min(f, 1 - f) with f the frequency of allele 2 among the non-missing genotypes
        (NaN for a column with none)."""
        return _maf_of(self.counts(rows=rows)[0])

    def _allele_maf(self):
        return self.maf()

    def _minor_allele_counts(self):
        cnt = self.counts()[0].astype(np.float64)
        return np.minimum(cnt[:, 1] + 2.0 * cnt[:, 2], cnt[:, 1] + 2.0 * cnt[:, 0])

    def _marker_genotypes(self, cols):
        """The allele counts of a few columns (n x len(cols)), decoded on the host, a missing one imputed by the column's mean."""
        bed = self.subset(cols=cols).export_bed()
        two = np.stack([(bed >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(bed.shape[0], -1)[:, :self.n]
        g = np.array([0.0, np.nan, 1.0, 2.0])[two].T
        with np.errstate(invalid="ignore"):
            mean = np.nanmean(g, axis=0)
        return np.where(np.isnan(g), np.where(np.isnan(mean), 0.0, mean)[None, :], g)

    def missing_rate(self, axis):
        """The share of missing genotypes per column (axis = 0: over the rows, length p) or per row (axis = 1, length n)."""
        if axis not in (0, 1):
            raise ArgumentError("axis must be 0 (per column) or 1 (per row)")
        if axis == 0:
            return self.counts()[0][:, 3] / float(self.n)
        row_missing = np.empty(self.n, dtype=np.int32)
        _check(lib().mih_snp_counts(self._h, None, None, None, _p(row_missing)))      # from the missing lists alone
        return row_missing / float(self.p)

    # ---- linkage disequilibrium and pruning on the device (csrc/ld.hip) ----
    def _ld_window(self, window):
        return max(min(int(window), self.p), 1)

    def ld(self, window, stats=False, panel_cols=0, slice_rows=0):
        """The correlation r of every pair of columns j < k with k - j < window (clamped to p), made on the device (mih_ld_band):
        a (p, w - 1) float64 array with r[j, d - 1] = r_{j, j + d} and NaN where j + d >= p.  r is the correlation of the
        mean-imputed columns (the c_ij of grm()): without missing genotypes in either column what `plink --indep-pairwise`
        thresholds; with missing genotypes PLINK takes the pairwise-complete samples, and this library imputes by the mean.
        A column without an observed genotype, or monomorphic among its observed ones, has r = 0 with every column.
        stats=True: (r, stats, diag) with stats (p, w - 1, 4) int64 -- D_jk, A_jk, A_kj, M_jk of tests/ld_spec.py -- and diag
        (p,) int64, D_jj.  panel_cols: the columns whose band is on the device at a time; slice_rows: the rows one f32
        accumulator covers; 0 = the library's rules.  The bits do not depend on either, nor on the call."""
        w = self._ld_window(window)
        r = np.empty((self.p, w - 1))
        st = np.empty((self.p, w - 1, 4), dtype=np.int64) if stats else None
        dg = np.empty(self.p, dtype=np.int64) if stats else None
        _check(lib().mih_ld_band(self._h, int(window), int(panel_cols), int(slice_rows), _p(r), _p(st), _p(dg)))
        return (r, st, dg) if stats else r

    def ld_pairs(self, window, threshold, cap=None, panel_cols=0, slice_rows=0):
        """The pairs of columns j < k, k - j < window, with r_jk^2 > threshold (strictly) of ld(window), found on the device so
        that no p x window array reaches the host (mih_ld_pairs): (j, k, r) in the order (j, k), r bit-equal to the entries of
        ld().  cap: the most pairs to return; None starts with room for max(1024, 4 p) and calls once more with the count
        found if that was too small."""
        room = int(cap) if cap is not None else _ld_first_room(self.p)
        for _ in range(2):
            j, k, r = np.empty(max(room, 1), dtype=np.int64), np.empty(max(room, 1), dtype=np.int64), np.empty(max(room, 1))
            count = C.c_int64(0)
            _check(lib().mih_ld_pairs(self._h, int(window), float(threshold), int(panel_cols), int(slice_rows), room, _p(j), _p(k), _p(r),
                                      C.byref(count)))
            if cap is not None or count.value <= room:
                break
            room = count.value
        got = min(count.value, room)
        return j[:got], k[:got], r[:got]

    def ld_prune(self, window=50, step=5, r2=0.2, panel_cols=0, slice_rows=0):
        """`plink --indep-pairwise window step r2` on the device's pair list (mih_ld_prune): a boolean mask over the columns.
        Degenerate columns are dropped first; then the window [s, s + window) moves by step, and of every pair of kept columns
        inside it with r^2 > r2 the one with the smaller maf goes (a tie keeps the earlier column).  The r is ld()'s.  The step
        of manuscript/NFBC_sim/NFBC_data_qc.jl:18-33 between filter and the kinship matrix is then
            keep = x.ld_prune(50, 5, 0.2); pcs = x.pca(10, cols=keep)"""
        keep = np.empty(self.p, dtype=np.uint8)
        _check(lib().mih_ld_prune(self._h, int(window), int(step), float(r2), int(panel_cols), int(slice_rows), _p(keep), None))
        return keep.astype(np.bool_)

    def subset(self, rows=None, cols=None, center=None, scale=None, impute=None, dtype=None, reserve=None):
        """x[rows, cols] as a new SnpLinAlg, made on the device (mih_snp_subset): bit for bit the SnpLinAlg of the .bed encoding
        of the selected genotypes, with mu and 1/sigma over the kept rows.  rows, cols: boolean masks or strictly increasing
        index arrays, None = all; the flags default to this matrix's; reserve as in the constructor.  This matrix is unchanged."""
        center = self.center if center is None else bool(center)
        scale = self.scale if scale is None else bool(scale)
        impute = self.impute if impute is None else bool(impute)
        dtype = self.dtype if dtype is None else _snp_dtype(dtype)
        ridx, cidx = self._sel_indices(rows, self.n, "row"), self._sel_indices(cols, self.p, "column")
        for what, idx in (("rows", ridx), ("columns", cidx)):
            if idx is not None and idx.size == 0:              # (an empty array has no address to hand over)
                raise ArgumentError(f"the selection of {what} is empty")
        h = C.c_void_p(None)
        _check(lib().mih_snp_subset(self._h, _p(ridx), 0 if ridx is None else ridx.size, _p(cidx), 0 if cidx is None else cidx.size,
                                    int(center), int(scale), int(impute), 32 if dtype is np.float32 else 64, C.byref(h)))
        x = SnpLinAlg(None, center=center, scale=scale, impute=impute, device=self.device, _handle=h, dtype=dtype)
        x._reserve(reserve)
        return x

    # ---- the transposed image and the dense forward product (csrc/transpose.hip, csrc/xb.hip) ----
    def transpose(self, center=None, scale=None, impute=None, dtype=None, reserve=None):
        """The 2-bit matrix of the transposed genotypes (SNPs as rows, samples as columns) as a new SnpLinAlg of shape (p, n), made
        on the device (mih_snp_transpose): bit for bit the SnpLinAlg of the .bed encoding of the transposed code matrix, with mu
        and 1/sigma per sample.  The flags default to this matrix's, like subset; reserve as in the constructor, and -1: no reserve
        of device memory for fits whatever the size.  This matrix is unchanged."""
        center = self.center if center is None else bool(center)
        scale = self.scale if scale is None else bool(scale)
        impute = self.impute if impute is None else bool(impute)
        dtype = self.dtype if dtype is None else _snp_dtype(dtype)
        none = reserve is not None and reserve is not True and reserve is not False and int(reserve) < 0
        h = C.c_void_p(None)
        _check(lib().mih_snp_transpose(self._h, int(center), int(scale), int(impute), 32 if dtype is np.float32 else 64,
                                       -1 if none else 0, C.byref(h)))
        x = SnpLinAlg(None, center=center, scale=scale, impute=impute, device=self.device, _handle=h, dtype=dtype)
        if not none:
            x._reserve(reserve)
        return x

    def row_image(self, build=True):
        """The row image xb() reads: the transposed matrix, kept on this object as self._rows (the library has no hidden cache
        and no process-wide state).  build=True makes it if it is not there (reserve=-1: it only serves products), build=False
        drops it.  Returns the bytes of device memory its tiles take afterwards (0: none)."""
        if not build:
            self._rows = None
            return 0
        if getattr(self, "_rows", None) is None:
            self._rows = self.transpose(center=False, scale=False, impute=False, reserve=-1)
        r = self._rows
        return ((r.p + 31) // 32) * ((r.n + 127) // 128) * 1024

    def xb(self, B, xtv_digits=None, center=None, scale=None, impute=None, rows=None):
        """mul!(out, x, B) for a dense B of length p (-> n) or shape p x t (-> n x t): X B with X as this SnpLinAlg presents it,
        or with the flags overridden (mih_xb_dense).  The product is the X'r pass over the row image -- exact fixed point, any t,
        19 columns a pass; a column of the result depends on its column of B alone, bit for bit.  The row image is built on the
        first call (row_image()) and kept; rows: another SnpLinAlg made by x.transpose() to read instead.  A NaN or Inf in a
        column of B makes that column of the result NaN."""
        B = np.asarray(B, dtype=np.float64)
        if B.ndim not in (1, 2) or B.shape[0] != self.p:
            raise DimensionMismatch(f"B has shape {B.shape}, expected ({self.p},) or ({self.p}, t)")
        if B.ndim == 2 and B.shape[1] == 0:
            raise DimensionMismatch(f"B has shape {B.shape}: no column")
        if rows is None:
            self.row_image(True)
            rows = self._rows
        t = 1 if B.ndim == 1 else B.shape[1]
        Bf = np.asfortranarray(B.reshape(self.p, t))
        out = np.empty((self.n, t), order="F")
        flag = lambda f: -1 if f is None else int(bool(f))      # noqa: E731
        _check(lib().mih_xb_dense(self._h, rows._h, _p(Bf), t, flag(center), flag(scale), flag(impute), _digits(xtv_digits), _p(out)))
        return out[:, 0].copy() if B.ndim == 1 else out

    def score(self, weights, cols=None, average=False):
        """`plink --score`: the polygenic score sum_j w_j g_ij of every sample, whatever this handle's flags: raw allele counts
        (the counted allele is the one the dosages count), a missing genotype imputed by the SNP's mean dosage mu_j -- xb with
        center 0, scale 0, impute 1.  weights: one per SNP, or one per entry of cols, an index array or boolean mask of the SNPs
        they belong to (the others get weight 0).  average=False is the SCORESUM column of `plink --score ... sum` (SCORE1_SUM
        of plink2); average=True divides by 2 x the number of scored SNPs: the SCORE column of PLINK 1.9's default .profile
        (SCORE1_AVG of plink2), whose denominator under its default mean imputation is the allele count of all scored variants.
        PLINK imputes a missing genotype by the allele frequency of the scored file, which is mu_j / 2 of this matrix: the same
        thing when the matrix is the scored file (and not when frequencies come from elsewhere, --read-freq); its
        `no-mean-imputation` (missing genotypes dropped from sum and denominator) is not offered."""
        w = np.asarray(weights, dtype=np.float64)
        if w.ndim != 1:
            raise DimensionMismatch(f"weights has shape {w.shape}, expected one dimension")
        if cols is None:
            if w.size != self.p:
                raise DimensionMismatch(f"weights has length {w.size}, expected {self.p}")
            full, scored = w, self.p
        else:
            idx = self._sel_indices(cols, self.p, "column")
            if idx.size != w.size:
                raise DimensionMismatch(f"weights has length {w.size}, cols selects {idx.size} SNPs")
            if idx.size and (idx.min() < 0 or idx.max() >= self.p):
                raise ArgumentError(f"a column index is outside 0 .. {self.p - 1}")
            full, scored = np.zeros(self.p), idx.size
            full[idx] = w
        s = self.xb(full, center=False, scale=False, impute=True)
        return s / (2.0 * scored) if average else s

    def filter(self, min_success_rate_per_row=0.98, min_success_rate_per_col=0.98, min_maf=0.01, maxiters=5):
        """SnpArrays.filter (without the Hardy-Weinberg test): boolean masks (rmask, cmask) of the rows and columns that are left
        when rows and columns below the success rates, and columns below min_maf, are dropped in turn until nothing changes or
        maxiters rounds have run (then a warning).  Each round counts on the device under the current masks (mih_snp_counts),
        both counts before either mask changes; the thresholds are applied on the host in float64."""
        rmask, cmask = np.ones(self.n, dtype=np.bool_), np.ones(self.p, dtype=np.bool_)
        rmiss, cmiss = 1.0 - float(min_success_rate_per_row), 1.0 - float(min_success_rate_per_col)
        for _ in range(int(maxiters)):
            col_counts, row_missing = self.counts(rmask, cmask)
            rows, cols = int(np.count_nonzero(rmask)), int(np.count_nonzero(cmask))
            ckeep = cmask & (col_counts[:, 3] < cmiss * rows)
            if min_maf > 0:
                with np.errstate(invalid="ignore"):
                    ckeep &= _maf_of(col_counts) >= min_maf                    # (NaN fails)
            rkeep = rmask & (row_missing < rmiss * cols)
            changed = int(np.count_nonzero(rkeep)) != rows or int(np.count_nonzero(ckeep)) != cols
            rmask, cmask = rkeep, ckeep
            if not changed:
                return rmask, cmask
        warnings.warn(f"filter: maxiters = {maxiters} reached, the success rates may not be satisfied", stacklevel=2)
        return rmask, cmask


def _ld_first_room(p):
    """The pairs ld_pairs(cap=None) makes room for before it knows their number."""
    return max(1024, 4 * p)


def _maf_of(col_counts):
    n0, n1, n2 = (col_counts[:, k].astype(np.float64) for k in range(3))
    with np.errstate(invalid="ignore", divide="ignore"):
        f = (n1 + 2.0 * n2) / (2.0 * (n0 + n1 + n2))
    return np.minimum(f, 1.0 - f)


def _snp_dtype(dtype):
    dtype = np.dtype(dtype).type
    if dtype not in (np.float64, np.float32):
        raise ArgumentError("SnpLinAlg{T}: T must be Float64 or Float32")
    return dtype


class SnpBuilder:
    """A SnpLinAlg built on the device from hard-call DosageMatrix panels (mih_snp_builder_*): add(col0, panel) packs the
    panel's columns into columns col0 .. of the 2-bit image -- in any order, at any col0 -- and finish() returns the SnpLinAlg
    once every column is there.  Device memory holds the 2-bit image and the panel in hand, never n x p numerators."""

    def __init__(self, n, p, center=True, scale=True, impute=True, dtype=np.float64, device=0):
        self._b = C.c_void_p(None)
        self.n, self.p, self.device = int(n), int(p), device
        self._flags = (bool(center), bool(scale), bool(impute), _snp_dtype(dtype))
        self.bad_col = -1
        _check(lib().mih_snp_builder_create(self.n, self.p, int(center), int(scale), int(impute),
                                            32 if self._flags[3] is np.float32 else 64, device, C.byref(self._b)))

    def add(self, col0, panel):
        """Columns [col0, col0 + panel.p) from a DosageMatrix whose entries are all 0, 1, 2 or missing."""
        if not isinstance(panel, DosageMatrix):
            raise ArgumentError("a panel must be a DosageMatrix")
        if not self._b:
            raise ArgumentError("the builder is closed")
        bad = C.c_int64(-1)
        rc = lib().mih_snp_builder_add(self._b, int(col0), panel._h, C.byref(bad))
        self.bad_col = bad.value            # the least column (0-based, of the whole matrix) a refusal names, else -1
        _check(rc)
        return self

    def finish(self, reserve=None):
        if not self._b:
            raise ArgumentError("the builder is closed")
        h = C.c_void_p(None)
        try:
            _check(lib().mih_snp_builder_finish(self._b, C.byref(h)))
        finally:
            if h:
                self.close()
        center, scale, impute, dtype = self._flags
        x = SnpLinAlg(None, center=center, scale=scale, impute=impute, device=self.device, _handle=h, dtype=dtype)
        x._reserve(reserve)
        return x

    def close(self):
        if self._b:
            lib().mih_snp_builder_destroy(self._b)
            self._b = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def naive_impute(x, destination, n=None):
    """naive_impute(x::SnpArray, destination) -- src/utilities.jl:862-899: writes `destination` (.bed) with every missing
    genotype of `x` replaced by the mode of its SNP.  `x` is a PLINK .bed path or the (p, ceil(n/4)) column bytes (then
    `n` is required), or a SnpLinAlg already on the GPU."""
    if isinstance(x, SnpLinAlg):
        mat = x
    else:
        if n is None:
            raise ArgumentError("naive_impute needs the number of samples n with a .bed path or raw columns")
        cols = read_bed(x, n) if isinstance(x, (str, os.PathLike)) else x
        mat = SnpLinAlg(cols, n)
    out = np.empty((mat.p, (mat.n + 3) // 4), dtype=np.uint8)
    _check(lib().mih_snp_naive_impute(mat._h, _p(out)))
    if not str(destination).endswith(".bed"):
        destination = str(destination) + ".bed"
    with open(destination, "wb") as f:
        f.write(b"\x6c\x1b\x01")
        f.write(out.tobytes())
    return None


class DenseMatrix(_Mat):
    """The reference's `x::Matrix{Float64}` / `x::Matrix{Float32}` design matrix, resident in HBM.  A float32 input
    is stored as Float32 on the device (half the memory traffic); all arithmetic stays Float64."""

    def __init__(self, x, device=0, _handle=None):
        super().__init__()
        self.device = device
        self.dtype = np.float64
        if _handle is not None:
            self._h = _handle
            self._dims()
            return
        x = np.asarray(x)
        if x.ndim != 2:
            raise DimensionMismatch("x must be a matrix")
        h = C.c_void_p(None)
        if x.dtype == np.float32:
            x = np.asfortranarray(x)
            self.dtype = np.float32
            _check(lib().mih_dense_create_f32(_p(x), x.shape[0], x.shape[1], device, C.byref(h)))
        else:
            x = np.asfortranarray(x, dtype=np.float64)
            _check(lib().mih_dense_create(_p(x), x.shape[0], x.shape[1], device, C.byref(h)))
        self._h = h
        self._dims()

    @classmethod
    def synthetic(cls, n, p, seed=2024, device=0):
        h = C.c_void_p(None)
        _check(lib().mih_dense_create_synthetic(n, p, seed, device, C.byref(h)))
        return cls(None, device=device, _handle=h)


class DosageMatrix(_Mat, _Kinship):
    """Genotype dosages d = num / denom in [0, 2] (VCF DS / GT, BGEN), resident in HBM as 16-bit numerators: 4x less memory
    and X'r traffic than the reference's Matrix{Float64} of the same values.  `num` is n x p, 0xFFFF marks a missing entry,
    1 <= denom <= 32767.  The matrix every fit sees is the STANDARDIZED one of standardize_genotypes! (src/wrapper.jl:406-423)
    -- mu_j the mean of the non-missing d, sigma_j = sqrt(mu_j (1 - mu_j / 2)), x_ij = (d_ij - mu_j) / sigma_j (d_ij - mu_j
    where sigma_j = 0), missing entries imputed by the mean (0), all-missing columns zero -- which is SnpLinAlg(center=true,
    scale=true, impute=true) on these values.  (The reference's own function throws on any missing entry: wrapper.jl:411 reads
    an undefined `t`.)"""

    def __init__(self, num, denom, device=0, _handle=None):
        super().__init__()
        self.device = device
        self.denom = int(denom)
        self.dtype = np.float64
        if _handle is not None:
            self._h = _handle
            self._dims()
            return
        num = np.asarray(num)
        if num.ndim != 2:
            raise DimensionMismatch("num must be a matrix")
        if num.dtype != np.uint16:
            raise ArgumentError(f"num must be uint16 (0xFFFF = missing), got {num.dtype}")
        num = np.asfortranarray(num)
        h = C.c_void_p(None)
        _check(lib().mih_dosage_create(_p(num), num.shape[0], num.shape[1], num.shape[0], self.denom, device, C.byref(h)))
        self._h = h
        self._dims()

    @classmethod
    def from_dosages(cls, d, device=0):
        """Dosages as floats (NaN = missing); the grid num / denom is detected (hard calls, up to 4 decimals, B <= 15 bit
        probabilities) and reduced by the gcd.  ArgumentError if the values sit on no grid with denom <= 32767."""
        from .genotypes import dosage_grid
        num, denom = dosage_grid(np.asarray(d, dtype=np.float64))
        return cls(num, denom, device=device)

    @classmethod
    def synthetic(cls, n, p, seed=2024, denom=255, missing_rate=0.0, device=0):
        """A seeded n x p dosage matrix generated on the device: hard calls Binomial(2, rho_j), rho_j ~ U(0, 0.5), moved by up
        to +-0.1 on the grid 1/denom and clamped to [0, 2]."""
        h = C.c_void_p(None)
        _check(lib().mih_dosage_create_synthetic(n, p, seed, int(denom), float(missing_rate), device, C.byref(h)))
        return cls(None, denom, device=device, _handle=h)

    def mu_sigma(self):
        """mu_j (dosage units) and 1/sigma_j (1 where sigma_j = 0)."""
        mu, s = np.empty(self.p), np.empty(self.p)
        _check(lib().mih_snp_mu_sigma(self._h, _p(mu), _p(s)))
        return mu, s

    def _allele_maf(self):
        f = self.mu_sigma()[0] / 2.0
        return np.minimum(f, 1.0 - f)

    def _minor_allele_counts(self):
        return 2.0 * self.n * self._allele_maf()                     # (expected counts: dosages are not integers)

    def _marker_genotypes(self, cols):
        """The dosages of a few columns (n x len(cols)), decoded on the host, a missing one imputed by the column's mean."""
        g = np.column_stack([self.export(int(j), 1)[:, 0] for j in cols]).astype(np.float64)
        g = np.where(g == 0xFFFF, np.nan, g / float(self.denom))
        with np.errstate(invalid="ignore"):
            mean = np.nanmean(g, axis=0)
        return np.where(np.isnan(g), np.where(np.isnan(mean), 0.0, mean)[None, :], g)

    def regrid(self, denom):
        """The same matrix over the finer grid 1 / denom (a multiple of self.denom, at most 32767): every numerator times
        denom / self.denom, the column statistics recomputed.  Column shards agree on one denominator this way."""
        _check(lib().mih_dosage_regrid(self._h, int(denom)))
        self.denom = int(denom)
        return self

    def to_snp(self, center=True, scale=True, impute=True, dtype=np.float64, reserve=None):
        """The SnpLinAlg of a matrix of hard calls -- every entry 0, 1, 2 or missing, whatever the denominator -- packed on the
        device (mih_snp_create_dosage): bit for bit the SnpLinAlg of the .bed encoding of the same genotypes (ALT counted as
        allele 2), at a quarter of a byte per genotype.  ArgumentError naming the first column that holds anything else."""
        dtype = _snp_dtype(dtype)
        h = C.c_void_p(None)
        _check(lib().mih_snp_create_dosage(self._h, int(center), int(scale), int(impute), 32 if dtype is np.float32 else 64,
                                           C.byref(h), None))
        x = SnpLinAlg(None, center=center, scale=scale, impute=impute, device=self.device, _handle=h, dtype=dtype)
        x._reserve(reserve)
        return x

    def export(self, col0=0, ncols=None):
        """Numerators of columns [col0, col0 + ncols) as an n x ncols uint16 array (0xFFFF = missing)."""
        ncols = self.p - col0 if ncols is None else ncols
        out = np.empty((ncols, self.n), dtype=np.uint16)
        _check(lib().mih_dosage_export(self._h, int(col0), int(ncols), _p(out)))
        return out.T


def _as_mat(x):
    if isinstance(x, _Mat):
        return x
    if isinstance(x, np.ndarray):
        if x.dtype == np.uint8:
            raise ArgumentError("x is a SnpArray! Please convert it to a SnpLinAlg first!")
        return DenseMatrix(x)
    raise ArgumentError(f"unsupported design matrix type {type(x)}")


# ---- projections ---------------------------------------------------------------------------
def project_k(x, k):
    """project_k!(x, k): keep the k largest |x_i| (ties kept); returns the projected copy."""
    if k < 0:
        raise ArgumentError(f"DomainError: Attempted to project to sparsity level {k}")
    x = np.array(x, dtype=np.float64).ravel()
    kept = C.c_int64(0)
    _check(lib().mih_project_topk(_p(x), x.size, int(k), C.byref(kept)))
    return x


def project_group_sparse(y, group, J, k):
    y = np.array(y, dtype=np.float64).ravel()
    group = np.ascontiguousarray(group, dtype=np.int64)
    if group.size != y.size:
        raise DimensionMismatch("group must have the length of y")
    kv = np.ascontiguousarray(np.atleast_1d(k), dtype=np.int64)
    if np.ndim(k) > 0 and group.size and kv.size < group.max():      # the library reads k[0 .. G-1], G = max(group)
        raise DimensionMismatch("k (vector) must have one entry per group")
    _check(lib().mih_project_group_sparse(_p(y), _p(group), y.size, int(J), _p(kv), int(np.ndim(k) > 0)))
    return y


def standardize(z):
    """standardize!(z) (src/utilities.jl:494-530): column-wise (z - mean) * 1/sample-sd."""
    z = np.array(z, dtype=np.float64)
    mu = z.mean(axis=0)
    sd = np.sqrt(((z - mu) ** 2).sum(axis=0) / (z.shape[0] - 1))
    return (z - mu) / sd


# ---- results -------------------------------------------------------------------------------
class IHTResult:
    """IHTResult (src/data_structures.jl:245-256)."""

    def __init__(self, time, logl, iter, beta, c, J, k, group, d, sigma_g, trace=None, choose_fired=False, mu=None):
        self.time, self.logl, self.iter = time, logl, iter
        self.beta, self.c, self.J, self.k, self.group, self.d = beta, c, J, k, group, d
        self.σg = self.sigma_g = sigma_g
        self.trace = trace or {}
        self.choose_fired = choose_fired
        self.mu = mu

    def predict_eta(self, x, z=None):
        """The linear predictor of this model on a cohort: x.xb(beta) + z @ c (z None: the intercept column of a fit without
        covariates).  x: a SnpLinAlg with the flags of the fitted one.  The mean is the link's inverse of it."""
        z = np.ones((x.n, 1)) if z is None else np.asarray(z, dtype=np.float64).reshape(x.n, -1)
        return x.xb(np.asarray(self.beta, dtype=np.float64)) + z @ np.asarray(self.c, dtype=np.float64)

    def __repr__(self):
        nz = np.flatnonzero(self.beta)
        cz = np.flatnonzero(self.c)
        lines = ["", f"IHT estimated {nz.size} nonzero SNP predictors and {cz.size} non-genetic predictors.", "",
                 f"Compute time (sec):     {self.time}", f"Final loglikelihood:    {self.logl}",
                 f"SNP PVE:                {self.σg}", f"Iterations:             {self.iter}", "",
                 "Selected genetic predictors:", " Position  Estimated_β"]
        lines += [f" {j + 1:8d}  {self.beta[j]: .6g}" for j in nz]
        lines += ["", "Selected nongenetic predictors:", " Position  Estimated_β"]
        lines += [f" {j + 1:8d}  {self.c[j]: .6g}" for j in cz]
        return "\n".join(lines)


class mIHTResult:
    """mIHTResult (src/data_structures.jl:263-273)."""

    def __init__(self, time, logl, iter, beta, c, k, traits, Sigma, sigma_g, trace=None, choose_fired=False):
        self.time, self.logl, self.iter, self.beta, self.c = time, logl, iter, beta, c
        self.k, self.traits, self.Σ, self.σg = k, traits, Sigma, sigma_g
        self.Sigma, self.sigma_g = Sigma, sigma_g
        self.trace = trace or {}
        self.choose_fired = choose_fired

    def predict_eta(self, x, z=None):
        """The r x n linear predictors of this model on a cohort: (x.xb(beta')) ' + c z, beta r x p, c r x q, z q x n (None: the
        row of ones of a fit without covariates)."""
        z = np.ones((1, x.n)) if z is None else np.asarray(z, dtype=np.float64).reshape(-1, x.n)
        return x.xb(np.asarray(self.beta, dtype=np.float64).T).T + np.asarray(self.c, dtype=np.float64) @ z


class IHTSession:
    """An IHTVariable kept alive on the GPU: `initialize` once, then `step()` = one iht_one_step!."""

    def __init__(self, y, x, z=None, *, k=10, J=1, d=None, l=None, zkeep=None, weight=None, max_step=3, train=None,
                 comm=None, xtv_digits=None, step_mode=None):
        x = _as_mat(x)
        d = _inst(d) if d is not None else Normal()
        l = _inst(l) if l is not None else IdentityLink()
        self.x = x
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).ravel())
        z = np.ones((x.n, 1)) if z is None else np.asarray(z, dtype=np.float64)
        z = np.asfortranarray(z.reshape(z.shape[0], -1))
        if not (y.size == x.n == z.shape[0]):
            raise DimensionMismatch(f"row dimension of y, x, and z ({y.size}, {x.n}, {z.shape[0]}) are not equal")
        self.q = z.shape[1]
        self._keep = [y, z]
        prm = _params(k, J, d, l, 1e-4, 1 << 30, 5, max_step, "None", zkeep, weight, None, self.q, x.p, self._keep,
                      comm=comm, xtv_digits=xtv_digits, step_mode=step_mode)
        tr = None if train is None else np.ascontiguousarray(train, dtype=np.uint8)
        self._h = C.c_void_p(None)
        _check(lib().mih_session_create(x._h, C.byref(prm), _p(y), _p(z), self.q, _p(tr), C.byref(self._h)))

    def step(self):
        logl, bt, tol = C.c_double(0), C.c_int32(0), C.c_double(0)
        _check(lib().mih_session_step(self._h, C.byref(logl), C.byref(bt), C.byref(tol)))
        return logl.value, bt.value, tol.value

    def run(self, nsteps):
        """`nsteps` iterations in one library call; returns (logl, total backtracks, tol) of the last one."""
        logl, bt, tol = C.c_double(0), C.c_int64(0), C.c_double(0)
        _check(lib().mih_session_run(self._h, int(nsteps), C.byref(logl), C.byref(bt), C.byref(tol)))
        return logl.value, bt.value, tol.value

    def model(self):
        beta, c = np.zeros(self.x.p), np.zeros(self.q)
        _check(lib().mih_session_model(self._h, _p(beta), _p(c)))
        return beta, c

    def close(self):
        if self._h:
            lib().mih_session_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_XTV_FORMATS = (0, -1, 4910, 4908, 1316, 1308, 428)
_default_digits = 0


def set_xtv_digits(digits=0):
    """Default of the `xtv_digits=` keyword of this mirror's calls (fit_iht, cv_iht, iht_run_many_models, IHTSession,
    SnpLinAlg.xtv, ...): the fixed-point format of the residual in X'r, id = base * 100 + digits -- 0 = library default =
    4910 (10 base-49 FP6 digits, 54-bit, 19 residuals in the six operands of a full pass) for fused passes and 428 (28 base-4 digits) for
    a single fit; 1316 (16 base-13 FP4 digits, 57-bit, two per operand); 4908 (43-bit, four per operand: the opt-in fast
    mode for fused multi-RHS passes); 1308 (27-bit, four per operand).  The LIBRARY has no such global: the format travels
    with every call (mih_fit_params::xtv_digits, mih_xtv_batched_fmt), so concurrent calls may differ."""
    global _default_digits
    if int(digits) not in _XTV_FORMATS:
        raise ArgumentError("residual format must be 0 (default), -1 (auto), 4910, 4908, 1316, 1308 or 428")
    _default_digits = int(digits)


def _digits(xtv_digits=None):
    d = _default_digits if xtv_digits is None else int(xtv_digits)
    if d not in _XTV_FORMATS:
        raise ArgumentError("residual format must be 0 (default), -1 (auto), 4910, 4908, 1316, 1308 or 428")
    return d


def probe_set(variant=None, multi_variant=None, max_fused=None):
    """Knobs of the measurement build (libmendeliht_hip_probes.so, MENDELIHT_HIP_PROBES=1): the per-wave single-operand
    kernel shapes, the launch shape / probe id of the LDS-shared and ring kernels, operands fused per register-staged pass."""
    if not using_probes():
        if (variant in (None, -1)) and (multi_variant in (None, 0)) and (max_fused in (None, 4)):
            return
        raise MendelIHTError("kernel-shape knobs exist in the measurement build only: set MENDELIHT_HIP_PROBES=1 before "
                             "the first call (the product library has one kernel per format and operand count)")
    L = lib()
    if variant is not None:
        _check(L.mih_probe_set_xtv_variant(int(variant)))
    if multi_variant is not None:
        _check(L.mih_probe_set_xtv_multi_variant(int(multi_variant)))
    if max_fused is not None:
        _check(L.mih_probe_set_max_fused(int(max_fused)))


def profile_enable(x, on=True):
    """Measurement hook of matrix `x` (mih_profile_*): record every launch of the dominant X'r kernel on it."""
    _check(lib().mih_profile_enable(_as_mat(x)._h, int(on)))


def profile_read(x, reset=True):
    """(total kernel ms, launches) since the last reset."""
    ms, n = C.c_double(0), C.c_int64(0)
    _check(lib().mih_profile_read(_as_mat(x)._h, C.byref(ms), C.byref(n), int(reset)))
    return ms.value, n.value


def profile_passes(x, reset=True):
    """The recorded launches, oldest first: dicts with kernel, residuals, operands, stream_tag, start_ms, ms."""
    h = _as_mat(x)._h
    n = C.c_int64(0)
    _check(lib().mih_profile_passes(h, None, 0, C.byref(n), 0))
    buf = (_PassRecord * max(n.value, 1))()
    _check(lib().mih_profile_passes(h, buf, n.value, C.byref(n), int(reset)))
    return [dict(kernel=buf[i].kernel.decode(), residuals=buf[i].residuals, operands=buf[i].operands,
                 stream_tag=buf[i].stream_tag, start_ms=buf[i].start_ms, ms=buf[i].ms) for i in range(n.value)]


def profile_counters(x, reset=True):
    """What the lock-step drivers did on `x` while its hook was on (PROFILE_COUNTERS)."""
    out = (C.c_int64 * len(PROFILE_COUNTERS))()
    _check(lib().mih_profile_counters(_as_mat(x)._h, out, int(reset)))
    return dict(zip(PROFILE_COUNTERS, [int(v) for v in out]))


EXCHANGE_KINDS = ("allreduce_n_plus_1", "allreduce_n", "allgather_candidates", "host_scalars")


def profile_exchange(x, reset=True):
    """Exchanges of the column-sharded fits on `x` while its hook was on (mih_profile_exchange): {kind: (count, summed ms)}."""
    ms, cnt = (C.c_double * 4)(), (C.c_int64 * 4)()
    _check(lib().mih_profile_exchange(_as_mat(x)._h, ms, cnt, int(reset)))
    return {kk: dict(count=int(cnt[i]), ms=float(ms[i])) for i, kk in enumerate(EXCHANGE_KINDS)}


def busy_union_ms(passes):
    """Time during which at least one of the recorded launches was running (launches of different lanes overlap)."""
    iv = sorted((q["start_ms"], q["start_ms"] + q["ms"]) for q in passes)
    tot, cur_a, cur_b = 0.0, None, None
    for a, b in iv:
        if cur_b is None or a > cur_b:
            if cur_b is not None:
                tot += cur_b - cur_a
            cur_a, cur_b = a, b
        else:
            cur_b = max(cur_b, b)
    if cur_b is not None:
        tot += cur_b - cur_a
    return tot


def cv_assignment(path, q, world):
    """rank_of[fold, ik] of the library's sharding rule for cv_iht (mih_cv_assignment): a (q, len(path)) int32 array."""
    path = np.ascontiguousarray(list(path), dtype=np.int64)
    out = np.zeros((int(q), path.size), dtype=np.int32)
    _check(lib().mih_cv_assignment(_p(path), path.size, int(q), int(world), _p(out)))
    return out


def hash_folds(n, q, seed=2026):
    """folds_i = 1 + (hash(seed, i) mod q): explicit, RNG-free fold labels for benchmarks and tests (the
    reference's default is rand(1:q, n), cross_validation.jl:72)."""
    i = np.arange(n, dtype=np.uint64)
    x = (i + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(31)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(29)
    return (1 + (x % np.uint64(q))).astype(np.int32)


def _is_multivariate(y):
    y = np.asarray(y)
    return y.ndim == 2 and y.shape[0] > 1 and y.shape[1] > 1


def _print_signature(io):
    print("****                   MendelIHT (mendeliht.jl_amd, MI355X)         ****", file=io)
    print("****     hot path of OpenMendel/MendelIHT.jl v1.4.11 on gfx950      ****", file=io)
    print("", file=io)


def _print_parameters(io, k, d, l, use_maf, group, debias, tol, max_iter, min_iter):
    reg = {"Normal": "linear", "Bernoulli": "logistic", "Poisson": "Poisson", "NegativeBinomial": "NegativeBinomial",
           "MvNormal": "Multivariate Gaussian"}.get(d.name, "unknown")
    print(f"Running sparse {reg} regression", file=io)
    print(f"Link functin = {l}", file=io)
    if np.ndim(k) == 0:
        print(f"Sparsity parameter (k) = {k}", file=io)
    else:
        print("Sparsity parameter (k) = using group membership specified in k", file=io)
    print(f"Prior weight scaling = {'on' if use_maf else 'off'}", file=io)
    print(f"Doubly sparse projection = {'on' if group is not None and len(group) > 0 else 'off'}", file=io)
    print(f"Debias = {'on' if debias else 'off'}", file=io)
    print(f"Max IHT iterations = {max_iter}", file=io)
    print(f"Converging when tol < {tol} and iteration ≥ {min_iter}:\n", file=io)


_default_step_mode = 0


def set_step_mode(mode=0):
    """Default of the `step_mode=` keyword (mih_fit_params::step_mode): 0 = iht_one_step! resident on the device wherever the fit
    allows it, 1 = every step host-driven (the path of rounds 1-4).  Same results bit for bit; the switch exists for A/B runs."""
    global _default_step_mode
    if int(mode) not in (0, 1):
        raise ArgumentError("step_mode must be 0 (device-resident steps) or 1 (host-driven steps)")
    _default_step_mode = int(mode)


def _params(k, J, d, l, tol, max_iter, min_iter, max_step, est_r, zkeep, weight, group, q, p, keep, progress=None,
            init_beta=False, comm=None, debias=False, xtv_digits=None, choose=None, step_mode=None):
    prm = _FitParams()
    prm.step_mode = _default_step_mode if step_mode is None else int(step_mode)
    if choose is not None:
        ccb = _choose_callback(choose)
        prm.choose = C.cast(ccb, C.c_void_p)
        keep.append(ccb)
    prm.debias = int(bool(debias))
    prm.xtv_digits = _digits(xtv_digits)
    if comm is not None:            # column-sharded fit: mendeliht.jl_amd.dist.ColumnComm
        prm.comm = comm.pointer()
        keep.append(comm)
    ks = None
    if np.ndim(k) > 0:
        ks = np.ascontiguousarray(k, dtype=np.int64)
        if group is None or len(group) <= 1:
            raise ArgumentError("Doubly sparse projection specified (since k is a vector) but there are no group information.")
        prm.k = 0
    else:
        if k < 0:
            raise ArgumentError("Value of k (max predictors per group) must be nonnegative!")
        prm.k = int(k)
    prm.J = int(J)
    prm.dist = max(d.code, 0)
    prm.link = l.code
    prm.nb_r = getattr(d, "r", 1.0)
    prm.tol = float(tol)
    prm.max_iter, prm.min_iter, prm.max_step = int(max_iter), int(min_iter), int(max_step)
    er = est_r if isinstance(est_r, str) else ("None" if est_r is None else str(est_r))
    er = er.lstrip(":").lower()
    if er not in ("none", "mm", "newton"):
        raise ArgumentError(f"Only support method is Newton or MM, but got {est_r}")
    prm.est_r = {"none": 0, "mm": 1, "newton": 2}[er]
    zk = None
    if zkeep is not None:
        zk = np.ascontiguousarray(zkeep, dtype=np.uint8)
        if zk.size != q:
            raise DimensionMismatch(f"zkeep must have length {q} but was {zk.size}")
    w = None
    if weight is not None and len(weight) > 0:
        w = np.ascontiguousarray(weight, dtype=np.float64)
        if w.size != p:
            raise DimensionMismatch(f"weight must have length {p} but was {w.size}")
    g = None
    if group is not None and len(group) > 0:
        g = np.ascontiguousarray(group, dtype=np.int64)
        if g.size != p:
            raise DimensionMismatch(f"group must have length {p} but was {g.size}")
    prm.zkeep, prm.weight, prm.group, prm.ks = _p(zk), _p(w), _p(g), _p(ks)
    prm.nks = 0 if ks is None else ks.size
    prm.init_beta = int(bool(init_beta))
    cb = None
    if progress is not None:
        cb = _PROGRESS(progress)
        prm.progress = C.cast(cb, C.c_void_p)
    keep.extend([zk, w, g, ks, cb])
    return prm


def fit_iht(y, x, z=None, *, k=10, J=1, d=None, l=None, group=None, weight=None, zkeep=None, est_r="None",
            use_maf=False, debias=False, verbose=True, tol=1e-4, max_iter=200, min_iter=5, max_step=3,
            io=None, init_beta=False, memory_efficient=True, train=None, comm=None, xtv_digits=None, choose=None, step_mode=None):
    """fit_iht(y, x, z; k, J, d, l, ...) -- src/fit.jl:60-118.

    step_mode (no reference counterpart): how iht_one_step! is driven (set_step_mode); None = the mirror's default.

    choose (no keyword in the reference, which draws from the global RNG): fn(kind, list, excess) making the random draw of
    _choose! (src/utilities.jl:444-458, src/multivariate.jl:310-351) when a projection leaves exact ties -- see
    _choose_callback; None = the library's deterministic rule, flagged by result.choose_fired.

    xtv_digits (no reference counterpart): fixed-point format of the residual in this call's X'r passes (set_xtv_digits).

    comm: a `dist.ColumnComm` when x holds only this process's block of SNP columns (column-sharded fit
    over several GPUs; beta in the result then covers the local columns -- see dist.fit_iht_sharded).

    Univariate: y (n,), x SnpLinAlg/DenseMatrix (n x p), z (n, q) with a leading column of ones.
    Multivariate (d=MvNormal or y 2-D): y (r, n), z (q, n), x is the same SnpLinAlg (its transpose is implied).
    """
    io = io or sys.stdout
    x = _as_mat(x)
    mv = _is_multivariate(y)
    d = _inst(d) if d is not None else (MvNormal() if mv else Normal())
    l = _inst(l) if l is not None else IdentityLink()
    if debias and mv:
        raise ArgumentError("debias is disabled for multivariate traits (multivariate.jl:569-570)")
    if init_beta and not isinstance(d, (Normal, MvNormal)):
        raise ArgumentError("Intializing beta values only work for Gaussian phenotypes! Sorry!")
    if not memory_efficient:
        raise ArgumentError("the GPU path is always memory_efficient=true")
    if isinstance(x, SnpLinAlg):
        if not x.center:
            raise ArgumentError("x is not centered! Please construct SnpLinAlg{Float64}(::SnpArray, center=true, scale=true)")
        if not x.scale:
            print("Warning: x is not scaled! We highly recommend `scale=true` in `SnpLinAlg` constructor", file=sys.stderr)
        if not x.impute:
            print("Warning: x does not have impute flag! We highly recommend `impute=true` in `SnpLinAlg` constructor", file=sys.stderr)
    if verbose:
        _print_signature(io)
    if mv:
        return _fit_mv(y, x, z, k, d, l, zkeep, verbose, tol, max_iter, min_iter, max_step, io, train, init_beta, xtv_digits, choose, comm)
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).ravel())
    n = x.n
    z = np.ones((n, 1)) if z is None else np.asarray(z, dtype=np.float64)
    z = np.asfortranarray(z.reshape(z.shape[0], -1))
    if not (y.size == n == z.shape[0]):
        raise DimensionMismatch(f"row dimension of y, x, and z ({y.size}, {n}, {z.shape[0]}) are not equal")
    _checky(y, d)
    q = z.shape[1]
    lines = []

    def progress(_user, it, logl, bt, tl):
        line = f"Iteration {it}: loglikelihood = {logl!r}, backtracks = {bt}, tol = {tl!r}"
        lines.append(line)
        print(line, file=io)

    # the per-iteration callback only when its lines are printed as they come (verbose): a fit whose steps the HOST drives waits
    # for it between two steps (tens of microseconds of interpreter per iteration); a quiet fit gets the same lines from the trace
    keep = []
    prm = _params(k, J, d, l, tol, max_iter, min_iter, max_step, est_r, zkeep, weight, group, q, x.p, keep, progress if verbose else None,
                  init_beta=init_beta, comm=comm, debias=debias, xtv_digits=xtv_digits, choose=choose, step_mode=step_mode)
    if verbose:
        _print_parameters(io, k, d, l, use_maf, group, debias, tol, max_iter, min_iter)
    tr = None if train is None else np.ascontiguousarray(train, dtype=np.uint8)
    beta, c, mu = np.zeros(x.p), np.zeros(q), np.zeros(n)
    nt = max(int(max_iter), 1)
    lt, tt, bt = np.zeros(nt), np.zeros(nt), np.zeros(nt, dtype=np.int32)
    res = _FitResult()
    res.beta, res.c, res.mu = _p(beta), _p(c), _p(mu)
    res.logl_trace, res.tol_trace, res.bt_trace = _p(lt), _p(tt), _p(bt)
    _check(lib().mih_fit_iht(x._h, C.byref(prm), _p(y), _p(z), q, _p(tr), C.byref(res)))
    m = res.n_trace
    if not verbose:
        lines = _trace_lines(lt, bt, tt, m)
    if verbose and res.iter >= max_iter:
        print(f"Did not converge after {max_iter} iterations! IHT run time was {res.time} seconds", file=io)
    dd = NegativeBinomial(res.nb_r) if isinstance(d, NegativeBinomial) else d
    if getattr(x, "dtype", np.float64) is np.float32:          # SnpLinAlg{Float32}: the model comes back in the caller's T
        beta, c, mu = beta.astype(np.float32), c.astype(np.float32), mu.astype(np.float32)
    return IHTResult(res.time, res.logl, res.iter, beta, c, J, k, np.array([] if group is None else group), dd, res.pve,
                     trace=dict(logl=lt[:m].copy(), tol=tt[:m].copy(), backtracks=bt[:m].copy(), lines=lines),
                     choose_fired=bool(res.choose_fired), mu=mu)


def _trace_lines(lt, bt, tt, m):
    """the lines the progress callback prints, from the trace arrays of a quiet fit"""
    return [f"Iteration {i + 1}: loglikelihood = {float(lt[i])!r}, backtracks = {int(bt[i])}, tol = {float(tt[i])!r}" for i in range(m)]


def _checky(y, d):
    if isinstance(d, Bernoulli) and not np.all((y == 0) | (y == 1)):
        raise ArgumentError("Bernoulli data y must be 1 or 0 only")
    if isinstance(d, (Poisson, NegativeBinomial)) and (np.any(y < 0) or np.any(y != np.floor(y))):
        raise ArgumentError("Poisson/NegativeBinomial data must be nonnegative integers")
    if isinstance(d, (Gamma, InverseGaussian)) and np.any(y <= 0):
        raise ArgumentError("Gamma/InverseGaussian data must be positive")


def _fit_mv(Y, x, Z, k, d, l, zkeep, verbose, tol, max_iter, min_iter, max_step, io, train, init_beta=False, xtv_digits=None,
            choose=None, comm=None):
    Y = np.asfortranarray(np.asarray(Y, dtype=np.float64))
    r, n = Y.shape
    Z = np.ones((1, n)) if Z is None else np.asarray(Z, dtype=np.float64)
    Z = np.asfortranarray(Z.reshape(-1, Z.shape[-1]) if Z.ndim > 1 else Z.reshape(1, -1))
    if not (n == x.n == Z.shape[1]):
        raise DimensionMismatch(f"number of samples in y, x, and z = {n}, {x.n}, {Z.shape[1]} are not equal")
    if np.ndim(k) > 0:
        raise ArgumentError("multivariate IHT takes an integer k")
    q = Z.shape[0]
    lines = []

    def progress(_user, it, logl, bt, tl):
        line = f"Iteration {it}: loglikelihood = {logl!r}, backtracks = {bt}, tol = {tl!r}"
        lines.append(line)
        print(line, file=io)

    keep = []
    prm = _params(k, 1, Normal(), l, tol, max_iter, min_iter, max_step, "None", zkeep, None, None, q, x.p, keep, progress if verbose else None,
                  init_beta=init_beta, xtv_digits=xtv_digits, choose=choose, comm=comm)
    if verbose:
        _print_parameters(io, k, MvNormal(), l, False, None, False, tol, max_iter, min_iter)
    tr = None if train is None else np.ascontiguousarray(train, dtype=np.uint8)
    B, Cm = np.zeros((r, x.p), order="F"), np.zeros((r, q), order="F")
    S, pve = np.zeros((r, r), order="F"), np.zeros(r)
    nt = max(int(max_iter), 1)
    lt, tt, bt = np.zeros(nt), np.zeros(nt), np.zeros(nt, dtype=np.int32)
    res = _MvResult()
    res.B, res.C, res.Sigma, res.pve = _p(B), _p(Cm), _p(S), _p(pve)
    res.logl_trace, res.tol_trace, res.bt_trace = _p(lt), _p(tt), _p(bt)
    _check(lib().mih_fit_mv(x._h, C.byref(prm), _p(Y), r, _p(Z), q, _p(tr), C.byref(res)))
    m = res.n_trace
    if not verbose:
        lines = _trace_lines(lt, bt, tt, m)
    return mIHTResult(res.time, res.logl, res.iter, B, Cm, k, r, S, pve,
                      trace=dict(logl=lt[:m].copy(), tol=tt[:m].copy(), backtracks=bt[:m].copy(), lines=lines),
                      choose_fired=bool(res.choose_fired))


def cv_iht(y, x, z=None, *, d=None, l=None, path=range(1, 21), q=5, est_r="None", group=None, weight=None,
           zkeep=None, folds=None, debias=False, verbose=True, max_iter=100, min_iter=5, init_beta=False,
           memory_efficient=True, tol=1e-4, max_step=3, rank=0, world=1, reduce=None, return_raw=False, xtv_digits=None,
           cv_threads=0):
    """cv_iht(y, x, z; path, q, folds, ...) -- src/cross_validation.jl:60-131.

    `x` may be a list of replicas of the matrix (one per GPU): the combinations are then spread over them
    from this one process (mih_cv_iht_multi), as the reference spreads them over its threads.
    `rank`/`world` shard the (fold, k) combinations over processes (one GPU each); `reduce`
    is a callable that sum-reduces the raw q x len(path) loss matrix across ranks (see
    mendeliht.jl_amd.dist.cv_iht_distributed for the torch.distributed/RCCL version).
    `cv_threads` (est_r only): the reference re-uses one IHTVariable per Julia thread, so the NegBin r of one fit is the starting
    value of that thread's next fit (cross_validation.jl:91,100-110) and its losses depend on Threads.nthreads(); the library
    follows the chains of `cv_threads` threads in lock-step.  0 (the default) = 1 = one chain over the whole grid = the reference at
    its default Threads.nthreads() == 1 -- the same meaning in mih_fit_params, the CPU checker of the tests and the Julia glue (which passes
    Threads.nthreads()); cv_threads=q gives one chain per fold (faster, but not a default reference run's losses).
    """
    replicas = None
    if isinstance(x, (list, tuple)):                 # one replica of the matrix per GPU, driven from this process
        replicas = [_as_mat(r) for r in x]
        if not replicas:
            raise ArgumentError("empty list of matrix replicas")
        x = replicas[0]
        if world != 1:
            raise ArgumentError("pass either a list of replicas (one process, several GPUs) or rank/world (one process per GPU)")
    x = _as_mat(x)
    mv = _is_multivariate(y)
    d = _inst(d) if d is not None else (MvNormal() if mv else Normal())
    l = _inst(l) if l is not None else IdentityLink()
    if not memory_efficient:
        raise ArgumentError("the GPU path is always memory_efficient=true")
    if debias and mv:
        raise ArgumentError("debias is disabled for multivariate traits (multivariate.jl:569-570)")
    if replicas is not None and mv:
        raise ArgumentError("replica lists are supported for univariate cross-validation")
    if init_beta and not isinstance(d, (Normal, MvNormal)):
        raise ArgumentError("Intializing beta values only work for Gaussian phenotypes! Sorry!")
    path = np.ascontiguousarray(list(path), dtype=np.int64)
    n = x.n
    if path.size == 0:
        raise ArgumentError("path is empty")
    if path.max() > x.p:
        raise ArgumentError("Sparsity level in `path` cannot be larger than total number of variables")
    if folds is None:
        folds = np.random.randint(1, q + 1, size=n)      # rand(1:q, n) (cross_validation.jl:72)
    folds = np.ascontiguousarray(folds, dtype=np.int32)
    if folds.size != n:
        raise DimensionMismatch("folds must have one label per sample")
    raw = np.zeros((q, path.size))
    keep = []
    if mv:
        Y = np.asfortranarray(np.asarray(y, dtype=np.float64))
        r = Y.shape[0]
        Z = np.ones((1, n)) if z is None else np.asarray(z, dtype=np.float64)
        Z = np.asfortranarray(Z.reshape(-1, Z.shape[-1]) if Z.ndim > 1 else Z.reshape(1, -1))
        prm = _params(1, 1, Normal(), l, tol, max_iter, min_iter, max_step, "None", zkeep, None, None, Z.shape[0], x.p, keep,
                      init_beta=init_beta, xtv_digits=xtv_digits)
        _check(lib().mih_cv_mv(x._h, C.byref(prm), _p(Y), r, _p(Z), Z.shape[0], _p(folds), q, _p(path), path.size,
                               rank, world, _p(raw)))
    else:
        yv = np.ascontiguousarray(np.asarray(y, dtype=np.float64).ravel())
        zz = np.ones((n, 1)) if z is None else np.asarray(z, dtype=np.float64)
        zz = np.asfortranarray(zz.reshape(zz.shape[0], -1))
        if not (yv.size == n == zz.shape[0]):
            raise DimensionMismatch(f"row dimension of y, x, and z ({yv.size}, {n}, {zz.shape[0]}) are not equal")
        _checky(yv, d)
        prm = _params(1, 1, d, l, tol, max_iter, min_iter, max_step, est_r, zkeep, weight, group, zz.shape[1], x.p, keep,
                      init_beta=init_beta, debias=debias, xtv_digits=xtv_digits)
        prm.cv_threads = int(cv_threads)
        if replicas is not None:
            hs = (C.c_void_p * len(replicas))(*[r._h for r in replicas])
            _check(lib().mih_cv_iht_multi(hs, len(replicas), C.byref(prm), _p(yv), _p(zz), zz.shape[1], _p(folds), q,
                                          _p(path), path.size, _p(raw)))
        else:
            _check(lib().mih_cv_iht(x._h, C.byref(prm), _p(yv), _p(zz), zz.shape[1], _p(folds), q, _p(path), path.size,
                                    rank, world, _p(raw)))
    if reduce is not None:
        raw = reduce(raw)
    mse = np.zeros(path.size)
    _check(lib().mih_cv_meanloss(_p(np.ascontiguousarray(raw)), _p(folds), n, q, path.size, _p(mse)))
    if verbose and rank == 0:
        print("\n\nCrossvalidation Results:\n\tk\tMSE")
        for kk, m in zip(path, mse):
            print(f"\t{kk}\t{m}")
        print(f"\nBest k = {path[int(np.argmin(mse))]}\n")
    return (mse, raw) if return_raw else mse


# ---- simulation helpers (src/simulate_utilities.jl) ---------------------------------------------------
def simulate_random_snparray(n, p, seed=2024, missing_rate=0.0, device=0):
    """simulate_random_snparray (simulate_utilities.jl:33-47): maf_j ~ U(0, 0.5), g_ij ~ Binomial(2, maf_j), generated
    on the device with a counter-based generator (not Julia's RNG stream); returned ready for fit_iht, i.e. as
    SnpLinAlg{Float64}(x, center=true, scale=true, impute=true)."""
    return SnpLinAlg.synthetic(n, p, seed=seed, missing_rate=missing_rate, center=True, scale=True, impute=True, device=device)


def simulate_random_response(x, k, d, l=None, *, r=10, alpha=1.0, Zu=None, seed=None):
    """simulate_random_response(x, k, d, l; r, α, Zu) -- simulate_utilities.jl:205-244: k effects at random positions
    (N(0,1); N(0,0.3²) for Poisson / Gamma / NegativeBinomial), eta = x*beta + Zu computed on the GPU, y ~ d(linkinv(eta)).
    Returns (y, true_b, correct_position) with 0-based positions."""
    x = _as_mat(x)
    d = _inst(d)
    l = _inst(l) if l is not None else canonicallink(d)
    if isinstance(d, (NegativeBinomial, Gamma)) and not isinstance(l, LogLink):
        raise ArgumentError(f"Distribution {d!r} must use LogLink!")
    rng = np.random.default_rng(seed)
    n, p = x.n, x.p
    small = isinstance(d, (Poisson, Gamma, NegativeBinomial))
    pos = np.sort(rng.choice(p, size=k, replace=False))
    val = rng.normal(0.0, 0.3 if small else 1.0, size=k)
    true_b = np.zeros(p)
    true_b[pos] = val
    eta = x.xv_sparse(pos, val) + (0.0 if Zu is None else np.asarray(Zu, dtype=np.float64).ravel())
    inv = {0: lambda e: e, 1: lambda e: 1 / (1 + np.exp(-e)), 2: np.exp}
    if l.code not in inv:
        raise ArgumentError("simulate_random_response supports the Identity, Logit and Log links")
    mu = np.clip(inv[l.code](eta), -20, 20)
    if isinstance(d, Normal):
        y = mu + rng.standard_normal(n)
    elif isinstance(d, Bernoulli):
        y = (rng.random(n) < mu).astype(np.float64)
    elif isinstance(d, Poisson):
        y = rng.poisson(mu).astype(np.float64)
    elif isinstance(d, NegativeBinomial):
        y = rng.negative_binomial(r, 1.0 / (1.0 + mu / r)).astype(np.float64)
    elif isinstance(d, Gamma):
        y = rng.gamma(alpha, mu / alpha)                 # shape α, rate 1/μ as in the reference
    else:
        raise ArgumentError(f"unsupported distribution {d!r}")
    return y, true_b, pos


def maf_weights(x, max_weight=np.inf):
    """maf_weights(x::SnpArray; max_weight) -- src/utilities.jl:682-697: prior weights 1 / (2 sqrt(p (1 - p)))
    from the minor allele frequencies (SnpArrays.maf: over the non-missing genotypes), clamped to [1, max_weight]."""
    if not isinstance(x, SnpLinAlg):
        raise ArgumentError("maf_weights needs a SnpLinAlg (2-bit genotypes)")
    mu, _ = x.mu_sigma()
    f = mu / 2.0
    maf = np.minimum(f, 1.0 - f)
    with np.errstate(divide="ignore"):
        w = 1.0 / (2.0 * np.sqrt(maf * (1.0 - maf)))
    return np.clip(w, 1.0, max_weight)


def iht_run_many_models(y, x, z=None, *, d=None, l=None, path=range(1, 21), est_r="None", group=None, weight=None,
                        use_maf=False, debias=False, verbose=True, parallel=False, max_iter=100, rank=0, world=1,
                        reduce=None, xtv_digits=None):
    """iht_run_many_models(y, x, z; path, ...) -- src/cross_validation.jl:232-273: fit_iht on the FULL data
    for every model size in `path` (no hold-out), returns the loglikelihoods.  `parallel` (pmap in the
    reference) is accepted and ignored: the fits of one process run back to back on its GPU; `rank` /
    `world` shard `path` over processes and `reduce` sums the loglikelihood vector across them."""
    x = _as_mat(x)
    if _is_multivariate(y):
        raise ArgumentError("iht_run_many_models on the GPU path takes a univariate response")
    d = _inst(d) if d is not None else Normal()
    l = _inst(l) if l is not None else canonicallink(d)          # cross_validation.jl:237
    path = np.ascontiguousarray([int(k) for k in path], dtype=np.int64)
    yv = np.ascontiguousarray(np.asarray(y, dtype=np.float64).ravel())
    n = x.n
    zz = np.ones((n, 1)) if z is None else np.asarray(z, dtype=np.float64)
    zz = np.asfortranarray(zz.reshape(zz.shape[0], -1))
    if not (yv.size == n == zz.shape[0]):
        raise DimensionMismatch(f"row dimension of y, x, and z ({yv.size}, {n}, {zz.shape[0]}) are not equal")
    _checky(yv, d)
    keep = []
    prm = _params(1, 1, d, l, 1e-4, max_iter, 5, 3, est_r, None, weight, group, zz.shape[1], x.p, keep, debias=debias,
                  xtv_digits=xtv_digits)
    logl = np.zeros(path.size)
    _check(lib().mih_fit_iht_path(x._h, C.byref(prm), _p(yv), _p(zz), zz.shape[1], _p(path), path.size, rank, world,
                                  _p(logl), None, None, None))
    if reduce is not None:
        logl = reduce(logl)
    if verbose and rank == 0:
        print("\n\nResults of running many models:\n\tk\tloglikelihood")
        for k, v in zip(path, logl):
            print(f"\t{k}\t{v}")
    return logl


# ---- file-level wrappers (src/wrapper.jl) ----------------------------------------------------
def _phenotype_is_missing(tok):
    return tok in ("-9", "NA")                                   # wrapper.jl:251-253


def _fam_column(prefix, col, d, n):
    """parse_phenotypes(x::SnpData, col, d) -- wrapper.jl:171-214: column `col` (1-based) of the .fam file; missing ("-9", "NA")
    phenotypes are imputed by the mean of the observed ones for quantitative traits and refused for binary / count traits."""
    toks = []
    with open(prefix + ".fam") as f:
        for line in f:
            parts = line.split()
            if parts:
                toks.append(parts[col - 1])
    if len(toks) != n:
        raise DimensionMismatch(f"{prefix}.fam has {len(toks)} samples, expected {n}")
    miss = np.array([_phenotype_is_missing(t) for t in toks])
    if miss.any() and not isinstance(d, (Normal, MvNormal)):
        i = int(np.flatnonzero(miss)[0]) + 1
        raise ArgumentError(f"Missing phenotype detected for sample {i}. Automatic phenotype imputation are only possible for "
                            "quantitative traits. Please exclude missing phenotypes or impute them first.")
    y = np.array([0.0 if m_ else float(t) for t, m_ in zip(toks, miss)])
    if miss.any():
        y[miss] = y[~miss].sum() / (n - miss.sum())
    return y


def _count_lines(path):
    with open(path) as f:
        return sum(1 for line in f if line.strip())


def parse_phenotypes(plinkfile, phenotypes, d, n):
    """parse_phenotypes (wrapper.jl:136-224): .fam column(s) or a comma-separated file, one sample per row."""
    if isinstance(phenotypes, (int, np.integer)):
        if isinstance(d, MvNormal):
            raise ArgumentError("Multivariate analysis requires multiple phenotypes! Please specify e.g. phenotypes=[6, 7] or save each "
                                "sample's phenotypes in a comma-separated file where each sample occupies a different row and each "
                                "phenotype is separated by a single comma.")
        return _fam_column(plinkfile, int(phenotypes), d, n)
    if isinstance(phenotypes, (list, tuple, np.ndarray)):
        return np.stack([_fam_column(plinkfile, int(c), MvNormal(), n) for c in phenotypes])      # r x n
    y = np.loadtxt(phenotypes, delimiter=",", ndmin=2)                                            # readdlm(file, ',', Float64)
    return y.T.copy() if y.shape[1] > 1 else y[:, 0].copy()


def parse_covariates(filename, exclude_std_idx=(), standardize_columns=True):
    """parse_covariates (wrapper.jl:226-249): comma-separated, one sample per row, first column the intercept; every column not in
    exclude_std_idx (1-based indices or a boolean mask) is standardized, the intercept never."""
    z = np.loadtxt(filename, delimiter=",", ndmin=2)
    ex = np.asarray(list(exclude_std_idx))
    std = np.ones(z.shape[1], dtype=bool)
    if ex.dtype == bool:
        std = ~ex
    elif ex.size:
        std[ex.astype(int) - 1] = False
    if np.all(z[:, 0] == 1):
        std[0] = False
    else:
        print("Warning: Covariate file provided but did not detect an intercept. An intercept will NOT be included in IHT!", file=sys.stderr)
    if standardize_columns and std.any():
        z[:, std] = standardize(z[:, std])
    return z


def _read_bim(prefix):
    """chromosome, SNP id, position, allele1, allele2 of the .bim file (what SnpData.snp_info holds, wrapper.jl:451-485)."""
    chrom, ids, pos, a1, a2 = [], [], [], [], []
    with open(prefix + ".bim") as f:
        for line in f:
            t = line.split()
            if not t:
                continue
            chrom.append(t[0]); ids.append(t[1]); pos.append(t[3]); a1.append(t[4]); a2.append(t[5])
    return chrom, pos, ids, a1, a2


def _parse_inputs(plinkfile, phenotypes, covariates, d, exclude_std_idx=(), dosage=False, device=0, two_bit=False):
    """x, y, z and the variants' (chr, pos, SNPid, ref, alt) of iht / cross_validate (wrapper.jl:64-79).  two_bit: a VCF or
    BGEN file of hard calls becomes a SnpLinAlg (parse_genotypes)."""
    if str(plinkfile).endswith((".vcf", ".vcf.gz", ".bgen")):
        from .genotypes import parse_genotypes
        if not isinstance(phenotypes, (str, os.PathLike)):
            raise ArgumentError("VCF / BGEN inputs carry no phenotypes: give `phenotypes` as a comma-separated file, one sample "
                                "per row (wrapper.jl:210-224)")
        x, _ids, chrom, pos, snpid, ref, alt = parse_genotypes(plinkfile, dosage=dosage, device=device, two_bit=two_bit)
        y = parse_phenotypes(plinkfile, phenotypes, d, x.n)
        if np.shape(y)[-1] != x.n:
            raise DimensionMismatch(f"{phenotypes} has {np.shape(y)[-1]} samples, {plinkfile} has {x.n}")
        z = parse_covariates(covariates, exclude_std_idx) if covariates else np.ones((x.n, 1))
        return x, y, z, (chrom, pos, snpid, ref, alt)
    for ext in (".bed", ".bim", ".fam"):
        if not os.path.exists(plinkfile + ext):
            raise ArgumentError(f"{plinkfile}{ext} not found: binary PLINK files should exclude .bim/.bed/.fam trailings and the trio "
                                "must be present in the same directory")
    n = _count_lines(plinkfile + ".fam")
    x = SnpLinAlg(plinkfile + ".bed", n, center=True, scale=True, impute=True, device=device)     # wrapper.jl:68-69
    y = parse_phenotypes(plinkfile, phenotypes, d, n)
    z = parse_covariates(covariates, exclude_std_idx) if covariates else np.ones((n, 1))
    return x, y, z, _read_bim(plinkfile)


def _show_result(io, res):
    """show(io, ::IHTResult / ::mIHTResult) -- data_structures.jl:280-325 (the tables are DataFrames in the reference)."""
    if isinstance(res, IHTResult):
        io.write(repr(res) + "\n")
        return
    r = res.traits
    io.write(f"\nCompute time (sec):     {res.time}\nFinal loglikelihood:    {res.logl}\nIterations:             {res.iter}\n")
    for t in range(r):
        io.write(f"Trait {t + 1}'s SNP PVE:      {res.σg[t]}\n")
    io.write("\nEstimated trait covariance:\n")
    io.write("\t".join(f"trait{t + 1}" for t in range(r)) + "\n")
    for row in np.asarray(res.Σ):
        io.write("\t".join(repr(float(v)) for v in row) + "\n")
    for t in range(r):
        for what, arr in (("nonzero SNP predictors", res.beta[t]), ("non-genetic predictors", res.c[t])):
            nz = np.flatnonzero(arr)
            io.write(f"\nTrait {t + 1}: IHT estimated {nz.size} {what}\n Position  Estimated_β\n")
            for j in nz:
                io.write(f" {j + 1:8d}  {arr[j]: .6g}\n")


def iht(plinkfile, k, d, *, phenotypes=6, covariates="", summaryfile="iht.summary.txt", betafile="iht.beta.txt",
        covariancefile="iht.cov.txt", exclude_std_idx=(), dosage=False, device=0, two_bit=False, **kwargs):
    """iht(filename, k, d; phenotypes, covariates, summaryfile, betafile, covariancefile, exclude_std_idx, dosage, kwargs...) --
    src/wrapper.jl:52-120 for binary PLINK input: SnpLinAlg{Float64}(center=true, scale=true, impute=true) on the GPU, the
    reference's phenotype / covariate parsing, fit_iht with the canonical link (LogLink for NegativeBinomial, wrapper.jl:87),
    the summary file (the fit's log + show(result)) and the beta file `chr pos SNPid ref alt Estimated_beta` (one row per SNP,
    tab-separated; `beta_1 .. beta_r` columns and the covariance file for multivariate traits, wrapper.jl:100-116).  (v1.4.11
    then overwrites the beta file with an empty CSV header, wrapper.jl:117 `CSV.write(betafile, df)` on an empty DataFrame;
    that accident is not reproduced.)  two_bit=True: a VCF or BGEN file of hard calls is packed into the 2-bit SnpLinAlg and
    fitted exactly as the PLINK trio of the same genotypes; a file that holds anything else is an ArgumentError."""
    d = _inst(d)
    x, y, z, info = _parse_inputs(plinkfile, phenotypes, covariates, d, exclude_std_idx, dosage, device, two_bit)
    mv = _is_multivariate(y)
    user_io = kwargs.pop("io", None)
    with open(summaryfile, "w") if summaryfile else open(os.devnull, "w") as io:
        if mv:
            result = fit_iht(y, x, z.T, k=k, d=MvNormal(), io=io, **kwargs)
        else:
            l = kwargs.pop("l", None) or (LogLink() if isinstance(d, NegativeBinomial) else canonicallink(d))     # wrapper.jl:87
            result = fit_iht(y, x, z, k=k, d=d, l=l, io=io, **kwargs)
        _show_result(io, result)
    if user_io is not None:
        _show_result(user_io, result)
    if betafile:
        chrom, pos, ids, a1, a2 = info
        with open(betafile, "w") as f:
            if mv:
                f.write("chr\tpos\tSNPid\tref\talt" + "".join(f"\tbeta_{t + 1}" for t in range(y.shape[0])) + "\n")
                for j in range(x.p):
                    f.write(f"{chrom[j]}\t{pos[j]}\t{ids[j]}\t{a1[j]}\t{a2[j]}\t" + "\t".join(repr(float(v)) for v in result.beta[:, j]) + "\n")
            else:
                f.write("chr\tpos\tSNPid\tref\talt\tEstimated_beta\n")
                for j in range(x.p):
                    f.write(f"{chrom[j]}\t{pos[j]}\t{ids[j]}\t{a1[j]}\t{a2[j]}\t{float(result.beta[j])!r}\n")
    if covariancefile and mv:
        np.savetxt(covariancefile, np.asarray(result.Σ), delimiter="\t")          # writedlm(covariancefile, result.Σ)
    return result


def gwas(plinkfile, d, *, phenotypes=6, covariates="", outfile="gwas.txt", exclude_std_idx=(), dosage=False, device=0,
         two_bit=False, l=None, slice_rows=0, spa=False, spa_cutoff=2.0, firth=False, firth_cutoff=2.0, lmm=False):
    """The single-SNP association scan of a file, beside iht(): the inputs are parsed as iht parses them, the null model of the
    covariates is fitted (fit_null) and every SNP gets its score test (x.assoc).  outfile: `chr pos SNPid ref alt z beta se
    neglog10p`, one row per SNP, tab-separated; spa=True (Bernoulli, logit link) adds the columns `neglog10p_spa spa_state`,
    firth=True (likewise) appends `beta_firth se_firth neglog10p_firth firth_state`.  lmm=True (a Normal trait): the mixed-model
    scan on the kinship matrix of the file's own SNPs, which keeps relatives in the sample (x.assoc(kinship=True)); the columns
    are the same, `null` of the result is the LmmNull.  Returns the AssocResult."""
    d = _inst(d)
    x, y, z, info = _parse_inputs(plinkfile, phenotypes, covariates, d, exclude_std_idx, dosage, device, two_bit)
    if _is_multivariate(y):
        raise ArgumentError("gwas scans one phenotype at a time")
    if l is None:
        l = LogLink() if isinstance(d, NegativeBinomial) else canonicallink(d)
    res = x.assoc(y, z, d=d, l=l, slice_rows=slice_rows, spa=bool(spa), spa_cutoff=spa_cutoff, firth=bool(firth), firth_cutoff=firth_cutoff,
                  kinship=True if lmm else None)
    if outfile:
        chrom, pos, ids, a1, a2 = info
        with open(outfile, "w") as f:
            f.write("chr\tpos\tSNPid\tref\talt\tz\tbeta\tse\tneglog10p" + ("\tneglog10p_spa\tspa_state" if spa else "")
                    + ("\tbeta_firth\tse_firth\tneglog10p_firth\tfirth_state" if firth else "") + "\n")
            for j in range(x.p):
                f.write(f"{chrom[j]}\t{pos[j]}\t{ids[j]}\t{a1[j]}\t{a2[j]}\t{float(res.z[j])!r}\t{float(res.beta[j])!r}\t"
                        f"{float(res.se[j])!r}\t{float(res.neglog10p[j])!r}"
                        + (f"\t{float(res.neglog10p_spa[j])!r}\t{int(res.spa_state[j])}" if spa else "")
                        + (f"\t{float(res.beta_firth[j])!r}\t{float(res.se_firth[j])!r}\t{float(res.neglog10p_firth[j])!r}\t{int(res.firth_state[j])}"
                           if firth else "") + "\n")
    return res


def gwas_sets(plinkfile, d, setfile, *, phenotypes=6, covariates="", outfile="gwas_sets.txt", exclude_std_idx=(), device=0, l=None,
              weights="beta", beta=(1, 25), max_maf=None, slice_rows=0, skato=False, rho=None):
    """The gene-based tests of a file, beside gwas(): the inputs are parsed as gwas parses them; setfile has two
    whitespace-separated columns `set_id snp_id` (lines starting with # are skipped), the SNP ids are those of the .bim; a set is
    the SNPs of its id in .bim order, in the order the ids first appear.  An id the .bim does not have, and a set of more than
    128 SNPs, are ArgumentErrors naming the first.  x.assoc_sets does the rest.  outfile: `set_id n_snps m_used burden_z
    neglog10p_burden skat_q neglog10p_skat skat_state`, one row per set, tab-separated; skato=True (with the grid rho, as set_test
    takes it) appends `neglog10p_skato skato_rho skato_state`.  Returns (set ids, SetResult)."""
    d = _inst(d)
    x, y, z, info = _parse_inputs(plinkfile, phenotypes, covariates, d, exclude_std_idx, False, device, False)
    if _is_multivariate(y):
        raise ArgumentError("gwas_sets tests one phenotype at a time")
    if l is None:
        l = LogLink() if isinstance(d, NegativeBinomial) else canonicallink(d)
    index = {}
    for j, name in enumerate(info[2]):
        index.setdefault(str(name), j)
    members = {}
    with open(setfile) as f:
        for ln, line in enumerate(f, 1):
            tok = line.split()
            if not tok or tok[0].startswith("#"):
                continue
            if len(tok) < 2:
                raise ArgumentError(f"{setfile}, line {ln}: expected `set_id snp_id`")
            if tok[1] not in index:
                raise ArgumentError(f"{setfile}, line {ln}: SNP {tok[1]} of set {tok[0]} is not in {plinkfile}.bim")
            members.setdefault(tok[0], set()).add(index[tok[1]])
    ids = list(members)
    sets = [np.array(sorted(members[k]), dtype=np.int64) for k in ids]
    for k, s in zip(ids, sets):
        if s.size > 128:
            raise ArgumentError(f"set {k} has {s.size} SNPs, at most 128 are supported")
    res = x.assoc_sets(y, z, sets, d=d, l=l, weights=weights, beta=beta, max_maf=max_maf, slice_rows=slice_rows, skato=skato, rho=rho)
    if outfile:
        with open(outfile, "w") as f:
            f.write("set_id\tn_snps\tm_used\tburden_z\tneglog10p_burden\tskat_q\tneglog10p_skat\tskat_state" +
                    ("\tneglog10p_skato\tskato_rho\tskato_state" if skato else "") + "\n")
            for k, name in enumerate(ids):
                more = f"\t{float(res.neglog10p_skato[k])!r}\t{float(res.skato_rho[k])!r}\t{int(res.skato_state[k])}" if skato else ""
                f.write(f"{name}\t{int(res.set_ptr[k + 1] - res.set_ptr[k])}\t{int(res.m_used[k])}\t{float(res.burden_z[k])!r}\t"
                        f"{float(res.neglog10p_burden[k])!r}\t{float(res.skat_q[k])!r}\t{float(res.neglog10p_skat[k])!r}\t{int(res.skat_state[k])}{more}\n")
    return ids, res


def print_cv_results(io, errors, path, k):
    """print_cv_results (data_structures.jl:327-335)."""
    io.write("\n\nCrossvalidation Results:\n\tk\tMSE\n")
    for kk, e in zip(path, errors):
        io.write(f"\t{int(kk)}\t{float(e)!r}\n")
    io.write(f"\nBest k = {int(k)}\n\n")


def cross_validate(plinkfile, d, *, path=range(1, 21), q=5, phenotypes=6, covariates="",
                   cv_summaryfile="cviht.summary.txt", exclude_std_idx=(), dosage=False, device=0, two_bit=False, **kwargs):
    """cross_validate(filename, d; path, phenotypes, covariates, cv_summaryfile, q, exclude_std_idx, dosage, kwargs...) --
    src/wrapper.jl:301-349 for binary PLINK input; the summary file is print_cv_results + the total time, as the reference's.
    two_bit: as iht."""
    t0 = time.time()
    d = _inst(d)
    x, y, z, _info = _parse_inputs(plinkfile, phenotypes, covariates, d, exclude_std_idx, dosage, device, two_bit)
    path = list(path)
    if _is_multivariate(y):
        mse = cv_iht(y, x, z.T, d=MvNormal(), path=path, q=q, **kwargs)
    else:
        l = kwargs.pop("l", None) or (LogLink() if isinstance(d, NegativeBinomial) else canonicallink(d))
        mse = cv_iht(y, x, z, d=d, l=l, path=path, q=q, **kwargs)
    if cv_summaryfile:
        with open(cv_summaryfile, "w") as io:
            print_cv_results(io, mse, path, path[int(np.argmin(mse))])
            io.write(f"Total cross validation time = {time.time() - t0} seconds\n")
    return mse
