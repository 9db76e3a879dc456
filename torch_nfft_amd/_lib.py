"""Loader for the two native libraries: the C-ABI library ``libnfft_hip.so`` (declared in
``include/nfft_hip.h``; bound here with ctypes for the stage-level entry points, the timers and non-torch style
tests) and the torch operator registry ``core.so`` built on top of it (``csrc/core.cpp``), which is loaded with
``torch.ops.load_library`` like the reference's (``torch_nfft/__init__.py:11``).

The product path has no CPU fallback: if a library is missing or lacks a symbol the import fails loudly.
"""
import collections
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NFFT_HIP_LIB") or os.path.join(_HERE, "libnfft_hip.so")
CORE_PATH = os.path.join(_HERE, "core.so")

ABI_VERSION = 7
POINTS_IN_QUARTER_BALL = 1

# every symbol include/nfft_hip.h declares
SYMBOLS = (
    "nfft_hip_abi_version",
    "nfft_hip_last_error",
    "nfft_hip_check_status",
    "nfft_hip_adjoint_workspace_bytes",
    "nfft_hip_forward_workspace_bytes",
    "nfft_hip_adjoint",
    "nfft_hip_forward",
    "nfft_hip_adjoint_planned",
    "nfft_hip_forward_planned",
    "nfft_hip_forward_grad_workspace_bytes",
    "nfft_hip_forward_grad_points_planned",
    "nfft_hip_forward_value_grad_points_planned",
    "nfft_hip_forward_grad_points_backward_workspace_bytes",
    "nfft_hip_forward_grad_points_backward_planned",
    "nfft_hip_plan_bytes",
    "nfft_hip_plan_points",
    "nfft_hip_plan_verify",
    "nfft_hip_spread_scratch_bytes",
    "nfft_hip_spread",
    "nfft_hip_interpolate",
    "nfft_hip_spectral_multiply",
    "nfft_hip_fastsum_workspace_bytes",
    "nfft_hip_fastsum",
    "nfft_hip_fastsum_planned",
    "nfft_hip_fastsum_band",
    "nfft_hip_fastsum_band_planned",
    "nfft_hip_fastsum_grad_workspace_bytes",
    "nfft_hip_fastsum_backward_planned",
    "nfft_hip_toeplitz_kernel_workspace_bytes",
    "nfft_hip_toeplitz_kernel",
    "nfft_hip_toeplitz_workspace_bytes",
    "nfft_hip_toeplitz_apply",
    "nfft_hip_nearfield_cells",
    "nfft_hip_nearfield_workspace_bytes",
    "nfft_hip_nearfield",
    "nfft_hip_nearfield_gradient_workspace_bytes",
    "nfft_hip_nearfield_gradient",
    "nfft_hip_nearfield_point_gradient_workspace_bytes",
    "nfft_hip_nearfield_point_gradient",
    "nfft_hip_ewald_near_cells",
    "nfft_hip_ewald_near_workspace_bytes",
    "nfft_hip_ewald_near",
    "nfft_hip_ewald_box_cells",
    "nfft_hip_ewald_near_box_workspace_bytes",
    "nfft_hip_ewald_near_box",
    "nfft_hip_ewald_dispersion_near",
    "nfft_hip_ewald_dispersion_near_box",
    "nfft_hip_ewald_virial_near_workspace_bytes",
    "nfft_hip_ewald_virial_near",
    "nfft_hip_ewald_virial_far_workspace_bytes",
    "nfft_hip_ewald_virial_far",
    "nfft_hip_ewald_dispersion_virial_near",
    "nfft_hip_ewald_dispersion_virial_far",
    "nfft_hip_ewald_step_near_workspace_bytes",
    "nfft_hip_ewald_step_near",
    "nfft_hip_ewald_step_spectral_workspace_bytes",
    "nfft_hip_ewald_step_spectral",
    "nfft_hip_ewald_lj_step_near_workspace_bytes",
    "nfft_hip_ewald_lj_step_near",
    "nfft_hip_ewald_lj_step_spectral_workspace_bytes",
    "nfft_hip_ewald_lj_step_spectral",
    "nfft_hip_ewald_lj_excl_near_workspace_bytes",
    "nfft_hip_ewald_lj_excl_near",
    "nfft_hip_ewald_lj_excl_list_workspace_bytes",
    "nfft_hip_ewald_lj_excl_list",
    "nfft_hip_ewald_lj_table_near_workspace_bytes",
    "nfft_hip_ewald_lj_table_near",
    "nfft_hip_ewald_bmh_table_near_workspace_bytes",
    "nfft_hip_ewald_bmh_table_near",
    "nfft_hip_ewald_dipole_near",
    "nfft_hip_ewald_dipole_near_box",
    "nfft_hip_ewald_dipole_spectral",
    "nfft_hip_ewald_stokeslet_near",
    "nfft_hip_ewald_stokeslet_near_box",
    "nfft_hip_ewald_stokeslet_spectral",
    "nfft_hip_ewald_rpy_near",
    "nfft_hip_ewald_rpy_near_box",
    "nfft_hip_ewald_excl",
    "nfft_hip_ewald_excl_box",
    "nfft_hip_ewald_excl_virial_workspace_bytes",
    "nfft_hip_ewald_excl_virial",
    "nfft_hip_ewald_yukawa_near",
    "nfft_hip_ewald_yukawa_near_box",
    "nfft_hip_ewald_yukawa_virial_near",
    "nfft_hip_gaussian_analytic_coeffs",
    "nfft_hip_interpolation_grid",
    "nfft_hip_coeffs_workspace_bytes",
    "nfft_hip_gaussian_interpolated_coeffs",
    "nfft_hip_interpolated_kernel_coeffs",
    "nfft_hip_plan_needed",
    "nfft_hip_profile_enable",
    "nfft_hip_profile_stages",
    "nfft_hip_profile_collect",
)
STAGES = ("plan", "gather", "zero", "spread", "fft", "rolloff", "interp", "multiply")

OK, EINVAL, EWORKSPACE, EFFT, EHIP, EKERNEL = 0, 1, 2, 3, 4, 5


class Problem(ctypes.Structure):
    """``nfft_hip_problem`` of include/nfft_hip.h."""
    _fields_ = [
        ("dim", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("num_points", ctypes.c_int64),
        ("num_columns", ctypes.c_int64),
        ("batch_size", ctypes.c_int64),
        ("N", ctypes.c_int64),
        ("m", ctypes.c_int64),
    ]


    def __init__(self, dim=0, num_points=0, num_columns=0, batch_size=1, N=0, m=0, flags=0):
        super().__init__(dim, flags, num_points, num_columns, batch_size, N, m)


class NearfieldProblem(ctypes.Structure):
    """``nfft_hip_nearfield_problem`` of include/nfft_hip.h."""
    _fields_ = [
        ("dim", ctypes.c_int32),
        ("kernel", ctypes.c_int32),
        ("poly_terms", ctypes.c_int32),
        ("cells_per_axis", ctypes.c_int32),
        ("num_sources", ctypes.c_int64),
        ("num_targets", ctypes.c_int64),
        ("num_columns", ctypes.c_int64),
        ("batch_size", ctypes.c_int64),
        ("c", ctypes.c_double),
        ("eps_I", ctypes.c_double),
        ("poly", ctypes.c_double * 8),
    ]


class EwaldProblem(ctypes.Structure):
    """``nfft_hip_ewald_problem`` of include/nfft_hip.h."""
    _fields_ = [
        ("cells_per_axis", ctypes.c_int32),
        ("with_field", ctypes.c_int32),
        ("num_points", ctypes.c_int64),
        ("num_columns", ctypes.c_int64),
        ("batch_size", ctypes.c_int64),
        ("alpha", ctypes.c_double),
        ("r_cut", ctypes.c_double),
    ]


class EwaldBoxProblem(ctypes.Structure):
    """``nfft_hip_ewald_box_problem`` of include/nfft_hip.h."""
    _fields_ = [
        ("cells", ctypes.c_int32 * 3),
        ("with_field", ctypes.c_int32),
        ("num_points", ctypes.c_int64),
        ("num_columns", ctypes.c_int64),
        ("batch_size", ctypes.c_int64),
        ("alpha", ctypes.c_double),
        ("r_cut", ctypes.c_double),
        ("box", ctypes.c_double * 6),
    ]


EXCL_COULOMB, EXCL_DISPERSION = 0, 1


class EwaldExclProblem(ctypes.Structure):
    """``nfft_hip_ewald_excl_problem`` of include/nfft_hip.h."""
    _fields_ = [
        ("kind", ctypes.c_int32),
        ("with_field", ctypes.c_int32),
        ("num_points", ctypes.c_int64),
        ("num_columns", ctypes.c_int64),
        ("num_entries", ctypes.c_int64),
        ("batch_size", ctypes.c_int64),
        ("alpha", ctypes.c_double),
        ("box", ctypes.c_double * 6),
    ]


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    # torch first: it brings its own libamdhip64, and the library must bind to THAT runtime (the one that owns the
    # tensors' device context).  Loaded the other way round, libnfft_hip.so pulls in the system ROCm runtime and its
    # first HIP call fails ("hipGetDevice failed").
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "torch_nfft_amd: %s is missing -- build it with `python torch_nfft_amd/build.py` "
            "(there is no CPU fallback)" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name in SYMBOLS:
        if not hasattr(lib, name):
            raise ImportError("torch_nfft_amd: %s does not export %s" % (LIB_PATH, name))
    P = ctypes.POINTER(Problem)
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.nfft_hip_abi_version.restype = ci
    lib.nfft_hip_last_error.restype = ctypes.c_char_p
    lib.nfft_hip_check_status.argtypes = [vp, ci]
    lib.nfft_hip_check_status.restype = ci
    for f in (lib.nfft_hip_adjoint_workspace_bytes, lib.nfft_hip_forward_workspace_bytes):
        f.argtypes = [P, ci, ci]
        f.restype = i64
    for f in (lib.nfft_hip_adjoint, lib.nfft_hip_forward):
        f.argtypes = [P, vp, vp, ci, vp, ci, vp, vp, i64, vp]
        f.restype = ci
    for f in (lib.nfft_hip_adjoint_planned, lib.nfft_hip_forward_planned):
        f.argtypes = [P, vp, vp, ci, ci, vp, vp, i64, vp]
        f.restype = ci
    lib.nfft_hip_forward_grad_workspace_bytes.argtypes = [P, ci, ci]
    lib.nfft_hip_forward_grad_workspace_bytes.restype = i64
    lib.nfft_hip_forward_grad_points_planned.argtypes = [P, vp, vp, ci, ci, vp, vp, vp, i64, vp]
    lib.nfft_hip_forward_grad_points_planned.restype = ci
    lib.nfft_hip_forward_value_grad_points_planned.argtypes = [P, vp, vp, ci, ci, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_forward_value_grad_points_planned.restype = ci
    lib.nfft_hip_forward_grad_points_backward_workspace_bytes.argtypes = [P, ci, ci]
    lib.nfft_hip_forward_grad_points_backward_workspace_bytes.restype = i64
    lib.nfft_hip_forward_grad_points_backward_planned.argtypes = [P, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_forward_grad_points_backward_planned.restype = ci
    lib.nfft_hip_plan_needed.argtypes = [P]
    lib.nfft_hip_plan_needed.restype = ci
    lib.nfft_hip_plan_bytes.argtypes = [P]
    lib.nfft_hip_plan_bytes.restype = i64
    lib.nfft_hip_plan_points.argtypes = [P, vp, vp, vp, i64, vp]
    lib.nfft_hip_plan_points.restype = ci
    lib.nfft_hip_spread_scratch_bytes.argtypes = [P, i64]
    lib.nfft_hip_spread_scratch_bytes.restype = i64
    lib.nfft_hip_spread.argtypes = [P, vp, vp, i64, vp, vp, vp]
    lib.nfft_hip_spread.restype = ci
    lib.nfft_hip_plan_verify.argtypes = [P, vp, vp, vp, vp]
    lib.nfft_hip_plan_verify.restype = ci
    lib.nfft_hip_interpolate.argtypes = [P, vp, vp, i64, vp, vp]
    lib.nfft_hip_interpolate.restype = ci
    lib.nfft_hip_spectral_multiply.argtypes = [vp, vp, ci, i64, i64, i64, vp]
    lib.nfft_hip_spectral_multiply.restype = ci
    lib.nfft_hip_fastsum_workspace_bytes.argtypes = [P, P, ci, ci, ci]
    lib.nfft_hip_fastsum_workspace_bytes.restype = i64
    lib.nfft_hip_fastsum.argtypes = [P, vp, vp, P, vp, vp, vp, ci, vp, ci, vp, vp, i64, vp]
    lib.nfft_hip_fastsum.restype = ci
    lib.nfft_hip_fastsum_planned.argtypes = [P, vp, P, vp, vp, ci, vp, ci, vp, vp, i64, vp]
    lib.nfft_hip_fastsum_planned.restype = ci
    lib.nfft_hip_fastsum_band.argtypes = [P, vp, vp, P, vp, vp, vp, ci, vp, ci, vp, vp, vp, i64, vp]
    lib.nfft_hip_fastsum_band.restype = ci
    lib.nfft_hip_fastsum_band_planned.argtypes = [P, vp, P, vp, vp, ci, vp, ci, vp, vp, vp, i64, vp]
    lib.nfft_hip_fastsum_band_planned.restype = ci
    lib.nfft_hip_fastsum_grad_workspace_bytes.argtypes = [P, P, ci]
    lib.nfft_hip_fastsum_grad_workspace_bytes.restype = i64
    lib.nfft_hip_fastsum_backward_planned.argtypes = [P, vp, P, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_fastsum_backward_planned.restype = ci
    for f in (lib.nfft_hip_toeplitz_kernel_workspace_bytes, lib.nfft_hip_toeplitz_workspace_bytes):
        f.argtypes = [P]
        f.restype = i64
    lib.nfft_hip_toeplitz_kernel.argtypes = [P, vp, vp, vp, i64, vp]
    lib.nfft_hip_toeplitz_kernel.restype = ci
    lib.nfft_hip_toeplitz_apply.argtypes = [P, vp, vp, ci, vp, vp, i64, vp]
    lib.nfft_hip_toeplitz_apply.restype = ci
    lib.nfft_hip_nearfield_cells.argtypes = [ctypes.c_int32, ctypes.c_double, i64]
    lib.nfft_hip_nearfield_cells.restype = i64
    lib.nfft_hip_nearfield_workspace_bytes.argtypes = [ctypes.POINTER(NearfieldProblem)]
    lib.nfft_hip_nearfield_workspace_bytes.restype = i64
    lib.nfft_hip_nearfield.argtypes = [ctypes.POINTER(NearfieldProblem), vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_nearfield.restype = ci
    lib.nfft_hip_nearfield_gradient_workspace_bytes.argtypes = [ctypes.POINTER(NearfieldProblem)]
    lib.nfft_hip_nearfield_gradient_workspace_bytes.restype = i64
    lib.nfft_hip_nearfield_gradient.argtypes = [ctypes.POINTER(NearfieldProblem), ctypes.c_int32, vp,
                                                vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_nearfield_gradient.restype = ci
    lib.nfft_hip_nearfield_point_gradient_workspace_bytes.argtypes = [ctypes.POINTER(NearfieldProblem)]
    lib.nfft_hip_nearfield_point_gradient_workspace_bytes.restype = i64
    lib.nfft_hip_nearfield_point_gradient.argtypes = [ctypes.POINTER(NearfieldProblem), ctypes.c_int32, vp,
                                                      vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_nearfield_point_gradient.restype = ci
    lib.nfft_hip_ewald_near_cells.argtypes = [ctypes.c_double, i64]
    lib.nfft_hip_ewald_near_cells.restype = i64
    lib.nfft_hip_ewald_near_workspace_bytes.argtypes = [ctypes.POINTER(EwaldProblem)]
    lib.nfft_hip_ewald_near_workspace_bytes.restype = i64
    lib.nfft_hip_ewald_near.argtypes = [ctypes.POINTER(EwaldProblem), vp, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_ewald_near.restype = ci
    lib.nfft_hip_ewald_box_cells.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_double, i64,
                                             ctypes.POINTER(ctypes.c_int32)]
    lib.nfft_hip_ewald_box_cells.restype = i64
    lib.nfft_hip_ewald_near_box_workspace_bytes.argtypes = [ctypes.POINTER(EwaldBoxProblem)]
    lib.nfft_hip_ewald_near_box_workspace_bytes.restype = i64
    lib.nfft_hip_ewald_near_box.argtypes = [ctypes.POINTER(EwaldBoxProblem), vp, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_ewald_near_box.restype = ci
    lib.nfft_hip_ewald_dispersion_near.argtypes = [ctypes.POINTER(EwaldProblem), vp, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_ewald_dispersion_near.restype = ci
    lib.nfft_hip_ewald_dispersion_near_box.argtypes = [ctypes.POINTER(EwaldBoxProblem), vp, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_ewald_dispersion_near_box.restype = ci
    lib.nfft_hip_ewald_virial_near_workspace_bytes.argtypes = [ctypes.POINTER(EwaldBoxProblem)]
    lib.nfft_hip_ewald_virial_near_workspace_bytes.restype = i64
    lib.nfft_hip_ewald_virial_near.argtypes = [ctypes.POINTER(EwaldBoxProblem), vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_ewald_virial_near.restype = ci
    lib.nfft_hip_ewald_virial_far_workspace_bytes.argtypes = [i64, i64, i64]
    lib.nfft_hip_ewald_virial_far_workspace_bytes.restype = i64
    lib.nfft_hip_ewald_virial_far.argtypes = [i64, i64, i64, vp, vp, ctypes.POINTER(ctypes.c_double), ctypes.c_double, vp,
                                              vp, i64, vp]
    lib.nfft_hip_ewald_virial_far.restype = ci
    lib.nfft_hip_ewald_dispersion_virial_near.argtypes = [ctypes.POINTER(EwaldBoxProblem), vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_ewald_dispersion_virial_near.restype = ci
    lib.nfft_hip_ewald_dispersion_virial_far.argtypes = [i64, i64, i64, vp, vp, vp, ctypes.POINTER(ctypes.c_double), vp, vp,
                                                         i64, vp]
    lib.nfft_hip_ewald_dispersion_virial_far.restype = ci
    lib.nfft_hip_ewald_step_near_workspace_bytes.argtypes = [ctypes.POINTER(EwaldBoxProblem)]
    lib.nfft_hip_ewald_step_near_workspace_bytes.restype = i64
    lib.nfft_hip_ewald_step_near.argtypes = [ctypes.POINTER(EwaldBoxProblem), vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_ewald_step_near.restype = ci
    lib.nfft_hip_ewald_step_spectral_workspace_bytes.argtypes = [i64, i64, i64]
    lib.nfft_hip_ewald_step_spectral_workspace_bytes.restype = i64
    lib.nfft_hip_ewald_step_spectral.argtypes = [i64, i64, i64, vp, vp, ctypes.POINTER(ctypes.c_double), ctypes.c_double, vp, vp,
                                                 vp, i64, vp]
    lib.nfft_hip_ewald_step_spectral.restype = ci
    lib.nfft_hip_ewald_lj_step_near_workspace_bytes.argtypes = [ctypes.POINTER(EwaldBoxProblem), ctypes.c_double]
    lib.nfft_hip_ewald_lj_step_near_workspace_bytes.restype = i64
    lib.nfft_hip_ewald_lj_step_near.argtypes = [ctypes.POINTER(EwaldBoxProblem), ctypes.c_double, vp, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_ewald_lj_step_near.restype = ci
    lib.nfft_hip_ewald_lj_step_spectral_workspace_bytes.argtypes = [i64, i64]
    lib.nfft_hip_ewald_lj_step_spectral_workspace_bytes.restype = i64
    lib.nfft_hip_ewald_lj_step_spectral.argtypes = [i64, i64, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_double), ctypes.c_double, vp,
                                                    vp, vp, i64, vp]
    lib.nfft_hip_ewald_lj_step_spectral.restype = ci
    for f in (lib.nfft_hip_ewald_lj_excl_near_workspace_bytes, lib.nfft_hip_ewald_lj_excl_list_workspace_bytes):
        f.argtypes = [ctypes.POINTER(EwaldBoxProblem), ctypes.c_double]
        f.restype = i64
    lib.nfft_hip_ewald_lj_excl_near.argtypes = [ctypes.POINTER(EwaldBoxProblem), ctypes.c_double, i64, vp, vp, vp, vp, vp, vp, vp, vp,
                                                vp, vp, vp, i64, vp]
    lib.nfft_hip_ewald_lj_excl_near.restype = ci
    lib.nfft_hip_ewald_lj_excl_list.argtypes = [ctypes.POINTER(EwaldBoxProblem), ctypes.c_double, i64, vp, vp, vp, vp, vp, vp, vp, vp,
                                                vp, vp, i64, vp]
    lib.nfft_hip_ewald_lj_excl_list.restype = ci
    lib.nfft_hip_ewald_lj_table_near_workspace_bytes.argtypes = [ctypes.POINTER(EwaldBoxProblem), ctypes.c_double]
    lib.nfft_hip_ewald_lj_table_near_workspace_bytes.restype = i64
    lib.nfft_hip_ewald_lj_table_near.argtypes = [ctypes.POINTER(EwaldBoxProblem), ctypes.c_double, i64, i64, vp, vp, vp, vp, vp, vp,
                                                 vp, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_ewald_lj_table_near.restype = ci
    lib.nfft_hip_ewald_bmh_table_near_workspace_bytes.argtypes = [ctypes.POINTER(EwaldBoxProblem), ctypes.c_double]
    lib.nfft_hip_ewald_bmh_table_near_workspace_bytes.restype = i64
    lib.nfft_hip_ewald_bmh_table_near.argtypes = [ctypes.POINTER(EwaldBoxProblem), ctypes.c_double, i64, i64, vp, vp, vp, vp, vp, vp,
                                                  vp, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_ewald_bmh_table_near.restype = ci
    lib.nfft_hip_ewald_dipole_near.argtypes = [ctypes.POINTER(EwaldProblem), vp, vp, vp, vp, ctypes.c_int32, vp, vp, i64, vp]
    lib.nfft_hip_ewald_dipole_near.restype = ci
    lib.nfft_hip_ewald_dipole_near_box.argtypes = [ctypes.POINTER(EwaldBoxProblem), vp, vp, vp, vp, ctypes.c_int32, vp, vp, i64, vp]
    lib.nfft_hip_ewald_dipole_near_box.restype = ci
    lib.nfft_hip_ewald_dipole_spectral.argtypes = [i64, i64, i64, ctypes.c_int32, vp, vp, ctypes.POINTER(ctypes.c_double), vp, vp]
    lib.nfft_hip_ewald_dipole_spectral.restype = ci
    lib.nfft_hip_ewald_stokeslet_near.argtypes = [ctypes.POINTER(EwaldProblem), vp, vp, vp, vp, ctypes.c_int32, vp, vp, i64, vp]
    lib.nfft_hip_ewald_stokeslet_near.restype = ci
    lib.nfft_hip_ewald_stokeslet_near_box.argtypes = [ctypes.POINTER(EwaldBoxProblem), vp, vp, vp, vp, ctypes.c_int32, vp, vp, i64, vp]
    lib.nfft_hip_ewald_stokeslet_near_box.restype = ci
    lib.nfft_hip_ewald_stokeslet_spectral.argtypes = [i64, i64, i64, ctypes.c_int32, vp, vp, ctypes.POINTER(ctypes.c_double), vp, vp]
    lib.nfft_hip_ewald_stokeslet_spectral.restype = ci
    lib.nfft_hip_ewald_rpy_near.argtypes = [ctypes.POINTER(EwaldProblem), vp, vp, vp, vp, ctypes.c_int32, ctypes.c_double, vp, vp, i64, vp]
    lib.nfft_hip_ewald_rpy_near.restype = ci
    lib.nfft_hip_ewald_rpy_near_box.argtypes = [ctypes.POINTER(EwaldBoxProblem), vp, vp, vp, vp, ctypes.c_int32, ctypes.c_double, vp, vp, i64, vp]
    lib.nfft_hip_ewald_rpy_near_box.restype = ci
    for f in (lib.nfft_hip_ewald_excl, lib.nfft_hip_ewald_excl_box):
        f.argtypes = [ctypes.POINTER(EwaldExclProblem), vp, vp, vp, vp, vp, vp, vp, vp]
        f.restype = ci
    lib.nfft_hip_ewald_excl_virial_workspace_bytes.argtypes = [ctypes.POINTER(EwaldExclProblem)]
    lib.nfft_hip_ewald_excl_virial_workspace_bytes.restype = i64
    lib.nfft_hip_ewald_excl_virial.argtypes = [ctypes.POINTER(EwaldExclProblem), vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.nfft_hip_ewald_excl_virial.restype = ci
    lib.nfft_hip_ewald_yukawa_near.argtypes = [ctypes.POINTER(EwaldProblem), vp, vp, vp, vp, ctypes.c_double, vp, vp, vp, i64, vp]
    lib.nfft_hip_ewald_yukawa_near.restype = ci
    lib.nfft_hip_ewald_yukawa_near_box.argtypes = [ctypes.POINTER(EwaldBoxProblem), vp, vp, vp, vp, ctypes.c_double, vp, vp, vp, i64, vp]
    lib.nfft_hip_ewald_yukawa_near_box.restype = ci
    lib.nfft_hip_ewald_yukawa_virial_near.argtypes = [ctypes.POINTER(EwaldBoxProblem), vp, vp, vp, ctypes.c_double, vp, vp, i64, vp]
    lib.nfft_hip_ewald_yukawa_virial_near.restype = ci
    lib.nfft_hip_gaussian_analytic_coeffs.argtypes = [ctypes.c_double, i64, ctypes.c_int32, vp, vp]
    lib.nfft_hip_gaussian_analytic_coeffs.restype = ci
    lib.nfft_hip_interpolation_grid.argtypes = [i64, ctypes.c_int32, ci, vp, vp]
    lib.nfft_hip_interpolation_grid.restype = ci
    lib.nfft_hip_coeffs_workspace_bytes.argtypes = [i64, ctypes.c_int32]
    lib.nfft_hip_coeffs_workspace_bytes.restype = i64
    lib.nfft_hip_gaussian_interpolated_coeffs.argtypes = [ctypes.c_double, i64, ctypes.c_int32, i64, ctypes.c_double,
                                                          vp, vp, i64, vp]
    lib.nfft_hip_gaussian_interpolated_coeffs.restype = ci
    lib.nfft_hip_interpolated_kernel_coeffs.argtypes = [vp, ci, i64, ctypes.c_int32, vp, vp, i64, vp]
    lib.nfft_hip_interpolated_kernel_coeffs.restype = ci
    lib.nfft_hip_profile_enable.argtypes = [ci]
    lib.nfft_hip_profile_enable.restype = None
    lib.nfft_hip_profile_stages.argtypes = [ctypes.c_uint]
    lib.nfft_hip_profile_stages.restype = None
    lib.nfft_hip_profile_collect.argtypes = [vp, vp, ci]
    lib.nfft_hip_profile_collect.restype = ci
    # test entry of csrc/selftest.hip (not part of the C ABI: a library built from an older tree may lack it)
    if hasattr(lib, "nfft_dbg_wave_reduce"):
        lib.nfft_dbg_wave_reduce.argtypes = [ci, i64, vp, vp, vp]
        lib.nfft_dbg_wave_reduce.restype = ci
    # test entries of csrc/api.hip (not part of the C ABI either)
    if hasattr(lib, "nfft_dbg_route"):
        lib.nfft_dbg_route.argtypes = [P, i64, vp]
        lib.nfft_dbg_route.restype = ci
    if hasattr(lib, "nfft_dbg_plan_layout"):
        lib.nfft_dbg_plan_layout.argtypes = [P, i64, vp, vp]
        lib.nfft_dbg_plan_layout.restype = ci
    if hasattr(lib, "nfft_dbg_work_list"):
        lib.nfft_dbg_work_list.argtypes = [P, vp, ci, vp, vp, vp, i64, vp]
        lib.nfft_dbg_work_list.restype = ci
    if hasattr(lib, "nfft_dbg_fft_route"):
        lib.nfft_dbg_fft_route.argtypes = [P, ci, ci, ci, i64, vp]
        lib.nfft_dbg_fft_route.restype = ci
    if hasattr(lib, "nfft_dbg_fft_stage"):
        lib.nfft_dbg_fft_stage.argtypes = [P, ci, ci, ci, vp, vp, vp, ci, vp, i64, vp]
        lib.nfft_dbg_fft_stage.restype = ci
    if lib.nfft_hip_abi_version() != ABI_VERSION:
        raise ImportError("torch_nfft_amd: ABI version mismatch in %s" % LIB_PATH)
    _lib = lib
    return lib


_core_loaded = False


def load_core():
    """Registers ``torch.ops.torch_nfft.*`` from ``core.so`` (after libnfft_hip.so, which it links against: the
    library loaded above is the instance it binds to)."""
    global _core_loaded
    if _core_loaded:
        return
    load()
    import torch
    if not os.path.exists(CORE_PATH):
        raise ImportError(
            "torch_nfft_amd: %s is missing -- build it with `python torch_nfft_amd/build.py`" % CORE_PATH)
    try:
        torch.ops.load_library(CORE_PATH)
    except Exception as e:  # a second provider of the torch_nfft namespace, or an unresolved symbol
        raise ImportError("torch_nfft_amd: cannot load %s: %s" % (CORE_PATH, e)) from e
    _core_loaded = True


def profile_enable(on, stages=None):
    """Stage timers on / off; ``stages`` = names of the stages to time (default: all of STAGES)."""
    mask = 0xFFFFFFFF if stages is None else sum(1 << STAGES.index(s) for s in stages)
    load().nfft_hip_profile_stages(mask)
    load().nfft_hip_profile_enable(1 if on else 0)


def profile_collect():
    """{stage: (total_ms, launches)} since the last collect (waits for the recorded events)."""
    n = len(STAGES)
    ms = (ctypes.c_double * n)()
    cnt = (ctypes.c_int64 * n)()
    check(load().nfft_hip_profile_collect(ms, cnt, n))
    return {STAGES[i]: (float(ms[i]), int(cnt[i])) for i in range(n)}


def wave_reduce(kind, values):
    """Test entry ``nfft_dbg_wave_reduce``: ``values`` is a 4-byte CUDA tensor of 64 * waves elements; wave w reduces
    elements 64 w ... 64 w + 63 with ``wave_max_f32`` (kind "max_f32") or ``wave_min_i32`` (kind "min_i32") of
    csrc/wave_reduce.h.  Returns one element per wave, same dtype."""
    import torch
    assert values.is_cuda and values.is_contiguous() and values.element_size() == 4 and values.numel() % 64 == 0
    out = torch.empty(values.numel() // 64, dtype=values.dtype, device=values.device)
    stream = torch.cuda.current_stream().cuda_stream
    check(load().nfft_dbg_wave_reduce({"max_f32": 0, "min_i32": 1}[kind], values.numel() // 64,
                                       ctypes.c_void_p(values.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                       ctypes.c_void_p(stream)))
    return out


SPREAD_MODES = ("lds", "mfma", "reg")               # csrc/common.h SpreadMode
GATHER_KERNELS = ("cols", "stream", "ring", "lanes")  # csrc/api.hip GatherKernel
Route = collections.namedtuple("Route", "wide owned pair spread x_through_plan gather column_groups small_grid")


def route(problem, real_columns):
    """Test entry ``nfft_dbg_route``: the route csrc/api.hip plan_route gives ``problem`` (a Problem) for calls with
    ``real_columns`` real planes per point set -- the tiling (wide, owned, pair: booleans), the spreading kernel
    ("lds" / "mfma" / "reg"), whether it reads x through the plan, the gather ("cols": wave per column, "stream", "ring",
    "lanes": lane per point), the column groups of the plan (1 or 3), and whether a call WITHOUT a plan would take the
    one-kernel small-grid path instead of all this.  Host code only; the process's NFFT_HIP_* switches apply."""
    out = (ctypes.c_int32 * 8)()
    check(load().nfft_dbg_route(ctypes.byref(problem), real_columns, out))
    return Route(bool(out[0]), bool(out[1]), bool(out[2]), SPREAD_MODES[out[3]], bool(out[4]), GATHER_KERNELS[out[5]],
                 int(out[6]), bool(out[7]))


PLAN_SCANS = ("none", "small4", "small16", "hipcub")  # csrc/kernels.h PlanDecisions::scan_kind
PlanLayout = collections.namedtuple(
    "PlanLayout",
    "dim m M W Ta1 Ta2 nta1 nta2 np0 bin0 SB sb2 CG wide owned pair pstride tiles_per_batch "
    "ntiles cap l1bins l1seg npencils block_points nblocks two_level grouped "
    "off_offsets off_cursor off_seal off_perm off_spos off_groups off_own "
    "one_level local_scan fuse scan_items scan")
_PLAN_LAYOUT_FLAGS = ("wide", "owned", "pair", "two_level", "grouped", "one_level", "local_scan", "fuse")


def plan_layout(problem, real_columns=0):
    """Test entry ``nfft_dbg_plan_layout``: (main, owned) -- geometry, layout and host decisions of the point plan that
    csrc/api.hip plan_route gives ``problem`` for calls with ``real_columns`` real planes per point set, and of the owned
    plan behind it (None when the route has none).  The ``off_*`` table offsets count from the plan's own start, which
    is ``off_own`` bytes into the plan buffer (0 for the main plan); ``scan`` names the scan between the two first-level
    passes ("none": the scatter pass scans the counts itself).  Host code only; the process's NFFT_HIP_* switches apply."""
    nf = len(PlanLayout._fields) + 1
    main, own = (ctypes.c_int64 * nf)(), (ctypes.c_int64 * nf)()
    check(load().nfft_dbg_plan_layout(ctypes.byref(problem), real_columns, main, own))

    def record(a):
        v = dict(zip(PlanLayout._fields, (int(a[i]) for i in range(nf - 1))))
        for k in _PLAN_LAYOUT_FLAGS:
            v[k] = bool(v[k])
        v["scan"] = PLAN_SCANS[v["scan"]]
        return PlanLayout(**v)
    return record(main), (record(own) if main[nf - 1] else None)


FFT_ROUTES = ("full", "roc_rows", "own_planar", "own_ci")  # csrc/api.hip FftRoute
FftRouteRecord = collections.namedtuple(
    "FftRouteRecord", "fft ci chunk_planes total_planes chunk_fft nc_axis1 nc_axis0 nc_forward specialised")


def fft_route(problem, adjoint, x_is_complex, real_output, chunk_np=0):
    """Test entry ``nfft_dbg_fft_route``: what csrc/api.hip make_route decides for the FFT stage of an adjoint
    (``adjoint`` true) or a forward transform of ``problem`` -- ``fft`` ("full": rocFFT + the roll-off kernel, "roc_rows":
    rocFFT rows + column passes, "own_planar": own rows + planar column passes), ``ci`` (chunks of >= 32 planes go
    column-innermost), the chunk size and plane count, and for a chunk of ``chunk_np`` planes (0: a full chunk) its route
    ``chunk_fft`` ("own_ci" where it goes column-innermost) and the tile widths make_col_geom gives its launches:
    ``nc_axis1`` / ``nc_axis0`` for an adjoint, ``nc_forward`` for a forward transform, 0 where no such launch runs;
    ``specialised``: one flag per launch kind (axis1, axis0, forward), true where col_dispatch takes a compile-time
    instantiation.  Host code only; NFFT_HIP_CHUNK_BYTES and NFFT_HIP_NO_COLFFT apply as in the calls."""
    out = (ctypes.c_int64 * 11)()
    check(load().nfft_dbg_fft_route(ctypes.byref(problem), 1 if adjoint else 0, 1 if x_is_complex else 0,
                                     1 if real_output else 0, chunk_np, out))
    return FftRouteRecord(FFT_ROUTES[out[0]], bool(out[1]), int(out[2]), int(out[3]), FFT_ROUTES[out[4]], int(out[5]),
                          int(out[7]), int(out[9]), (bool(out[6]), bool(out[8]), bool(out[10])))


def fft_stage(problem, adjoint, x_is_complex, real_output, planes, band, mult=None):
    """Test entry ``nfft_dbg_fft_stage``: the FFT stage alone, through make_route and the chunk loop of the operators.
    ``planes``: float32 CUDA tensor [B * C * ppc, (2N)^d] (ppc = 2 for a complex x of an adjoint / a complex y of a
    forward transform, (re, im) adjacent); ``band``: [B, N^d, C] float32 or complex64.  Adjoint: planes -> band (times the
    per-frequency factor ``mult`` [N^d], float32 or complex64, if given); forward: band -> planes.  Writes in place."""
    import torch
    assert planes.is_cuda and planes.is_contiguous() and planes.dtype == torch.float32
    assert band.is_cuda and band.is_contiguous()
    if adjoint:
        assert band.dtype == (torch.float32 if real_output else torch.complex64)
    else:
        assert band.dtype == (torch.complex64 if x_is_complex else torch.float32)
    ppc = (2 if x_is_complex else 1) if adjoint else (1 if real_output else 2)
    columns = problem.batch_size * problem.num_columns
    assert planes.numel() == columns * ppc * (2 * problem.N) ** problem.dim
    assert band.numel() == columns * problem.N ** problem.dim
    assert mult is None or mult.numel() == problem.N ** problem.dim
    lib = load()
    need = (lib.nfft_hip_adjoint_workspace_bytes if adjoint else lib.nfft_hip_forward_workspace_bytes)(
        ctypes.byref(problem), 1 if x_is_complex else 0, 1 if real_output else 0)
    if need < 0:
        check(EINVAL)
    ws = torch.empty(need, dtype=torch.uint8, device=planes.device)
    kind = 0
    if mult is not None:
        assert adjoint and mult.is_cuda and mult.is_contiguous()
        kind = {torch.float32: 1, torch.complex64: 2}[mult.dtype]
    stream = torch.cuda.current_stream().cuda_stream
    check(lib.nfft_dbg_fft_stage(ctypes.byref(problem), 1 if adjoint else 0, 1 if x_is_complex else 0,
                                 1 if real_output else 0, ctypes.c_void_p(planes.data_ptr()),
                                 ctypes.c_void_p(band.data_ptr()), ctypes.c_void_p(mult.data_ptr() if kind else None),
                                 kind, ctypes.c_void_p(ws.data_ptr()), need, ctypes.c_void_p(stream)))
    check_status()


def check_status(stream=None, synchronize=True):
    """Raise if a kernel on the current device has reported a fault (``nfft_hip_check_status``); with ``synchronize``
    the stream (default: torch's current one) is drained first, so that work just enqueued is covered."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    check(load().nfft_hip_check_status(ctypes.c_void_p(stream), 1 if synchronize else 0))


def last_error():
    return load().nfft_hip_last_error().decode("utf-8", "replace")


def check(rc):
    """Map a C-ABI return code onto the exceptions the reference raises (RuntimeError)."""
    if rc == OK:
        return
    msg = last_error()
    if rc == EINVAL and not msg.startswith("Input mismatch"):
        msg = "Input mismatch: " + msg
    raise RuntimeError(msg)
