"""Developer tool: times the spectral reductions of spectral_frame.h at the column counts that scripts/bench_ewald.py does not
reach (its forms run one column): nfft_ewald_step_spectral, nfft_ewald_virial_far and nfft_ewald_dispersion_virial_far at 1,
2, 4 and 5 columns (the three instantiations CC = 1, 2, 4 and a second column pass) and nfft_ewald_lj_step_spectral, on one
point set at N = 160 in a triclinic box.  Device-event times of 20 calls after three warm-up calls; one JSON line with
[median, minimum, maximum] in ms per timer.  NFFT_HIP_LIB names the library to load, as for pair_kernel_digest.py
(profiles/r21_reduction_frames.md)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_nfft_amd as tn  # noqa: E402
from torch_nfft_amd import ops  # noqa: E402


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return [round(float(np.median(t)), 4), round(min(t), 4), round(max(t), 4)]


if __name__ == "__main__":
    N = 160
    tilted3 = np.array([[1.0, 0.0, 0.0], [0.2, 1.1, 0.0], [0.1, -0.3, 1.3]])
    sc = tn.EwaldSplitting(10.0, 0.3, N, box=tilted3)
    sd = tn.DispersionSplitting(11.5, 0.3, N, box=tilted3)
    strain = sd.strain_coeffs()
    out = {"bench": "spectral_columns", "N": N}
    gen = torch.Generator(device="cuda").manual_seed(1)
    for cols in (1, 2, 4, 5):
        band = torch.view_as_complex(torch.randn((1, N, N, N, cols, 2), device="cuda", generator=gen))
        out["step_spectral_C%d" % cols] = timed(lambda: ops.nfft_ewald_step_spectral(band, sc.coeffs, sc.box6, 10.0))
        out["virial_far_C%d" % cols] = timed(lambda: ops.nfft_ewald_virial_far(band, sc.coeffs, sc.box6, 10.0))
        out["disp_virial_far_C%d" % cols] = timed(lambda: ops.nfft_ewald_dispersion_virial_far(band, sd.coeffs, strain, sd.box6))
    band = torch.view_as_complex(torch.randn((1, N, N, N, 2, 2), device="cuda", generator=gen))
    out["lj_step_spectral"] = timed(lambda: ops.nfft_ewald_lj_step_spectral(band, sc.coeffs, sd.coeffs, strain, sc.box6, 10.0))
    ops.check_status()
    print(json.dumps(out))
