"""torch_nfft_amd -- MI355X-native NFFT behind the torch_nfft API.

Importing the package loads the HIP C-ABI library ``libnfft_hip.so`` and, with ``torch.ops.load_library``, the
native operator registry ``core.so`` that exports ``torch.ops.torch_nfft.*`` (the reference loads its ``core.so``
the same way, ``torch_nfft/__init__.py:11``).  There is no CPU fallback: a missing library is an ImportError.
"""
from . import _lib

_lib.load()
_lib.load_core()

from . import ops  # noqa: E402
from .nfft import (nfft_adjoint, nfft_forward, nfft_fastsum, NfftAdjointFunction, NfftForwardFunction,  # noqa: E402
                   NfftFastsumFunction)
from .toeplitz import nfft_toeplitz_kernel, nfft_normal, nfft_inverse, NfftNormalFunction  # noqa: E402
from .ndft import ndft_forward, ndft_adjoint, ndft_fastsum, exact_trigonometric_matrix, exact_gaussian_matrix  # noqa: E402
from .coeffs import (gaussian_analytic_coeffs, gaussian_interpolated_coeffs, interpolation_grid,  # noqa: E402
                     radial_interpolation_grid, interpolated_kernel_coeffs)
from .nearfield import (RegularizedKernel, nfft_nearfield, nfft_fastsum_nearfield, NfftNearfieldFunction,  # noqa: E402
                        nfft_nearfield_gradient, nfft_fastsum_nearfield_gradient, NfftNearfieldGradientFunction,
                        NfftNearfieldPointsFunction)
from .ewald import (EwaldSplitting, nfft_ewald, nfft_ewald_energy, NfftEwaldFunction, nfft_ewald_virial,  # noqa: E402
                    nfft_ewald_step, virial_to_box_gradient)
from .dispersion import (DispersionSplitting, nfft_ewald_dispersion, nfft_ewald_dispersion_energy,  # noqa: E402
                         NfftEwaldDispersionFunction, nfft_ewald_dispersion_virial)
from .dipole import nfft_ewald_dipole, nfft_ewald_dipole_energy, NfftEwaldDipoleFunction  # noqa: E402
from .stokeslet import (nfft_ewald_stokeslet, nfft_ewald_stokeslet_power, stokeslet_splitting,  # noqa: E402
                        NfftEwaldStokesletFunction)
from .rpy import nfft_ewald_rpy, nfft_ewald_rpy_power, rpy_coeffs, rpy_splitting, NfftEwaldRpyFunction  # noqa: E402
from .exclusions import ExclusionList  # noqa: E402
from .yukawa import (YukawaSplitting, nfft_ewald_yukawa, nfft_ewald_yukawa_energy, NfftEwaldYukawaFunction,  # noqa: E402
                     nfft_ewald_yukawa_virial)
from .lj import LJPairTable, lj_coefficients, nfft_ewald_lj_step, nfft_ewald_lj_excl_step, nfft_ewald_lj_table_step  # noqa: E402
from .bmh import BMHPairTable, nfft_ewald_bmh_table_step  # noqa: E402
from .matrices import GramMatrix, AdjacencyMatrix  # noqa: E402
from .kernel import GaussianKernel  # noqa: E402
from . import utils  # noqa: E402


__all__ = ["nfft_adjoint", "nfft_forward", "nfft_fastsum", "nfft_toeplitz_kernel", "nfft_normal", "nfft_inverse",
           "NfftNormalFunction", "RegularizedKernel", "nfft_nearfield", "nfft_fastsum_nearfield",
           "NfftNearfieldFunction", "nfft_nearfield_gradient", "nfft_fastsum_nearfield_gradient",
           "NfftNearfieldGradientFunction", "NfftNearfieldPointsFunction", "EwaldSplitting", "nfft_ewald",
           "nfft_ewald_energy", "NfftEwaldFunction", "nfft_ewald_virial", "nfft_ewald_step", "virial_to_box_gradient",
           "DispersionSplitting",
           "nfft_ewald_dispersion", "nfft_ewald_dispersion_energy", "NfftEwaldDispersionFunction",
           "nfft_ewald_dispersion_virial", "nfft_ewald_dipole", "nfft_ewald_dipole_energy", "NfftEwaldDipoleFunction",
           "nfft_ewald_stokeslet", "nfft_ewald_stokeslet_power", "stokeslet_splitting", "NfftEwaldStokesletFunction",
           "nfft_ewald_rpy", "nfft_ewald_rpy_power", "rpy_coeffs", "rpy_splitting", "NfftEwaldRpyFunction", "ExclusionList",
           "YukawaSplitting", "nfft_ewald_yukawa", "nfft_ewald_yukawa_energy", "NfftEwaldYukawaFunction",
           "nfft_ewald_yukawa_virial", "lj_coefficients", "nfft_ewald_lj_step",
           "nfft_ewald_lj_excl_step", "LJPairTable", "nfft_ewald_lj_table_step",
           "BMHPairTable", "nfft_ewald_bmh_table_step",
           "ndft_forward", "ndft_adjoint", "ndft_fastsum",
           "exact_trigonometric_matrix", "exact_gaussian_matrix", "NfftAdjointFunction", "NfftForwardFunction",
           "NfftFastsumFunction", "gaussian_analytic_coeffs", "gaussian_interpolated_coeffs", "interpolation_grid",
           "radial_interpolation_grid", "interpolated_kernel_coeffs", "GramMatrix", "AdjacencyMatrix",
           "GaussianKernel", "utils"]
