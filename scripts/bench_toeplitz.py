"""Developer tool: cost of the Toeplitz normal operator A^H W A.  For each shape, device-event
medians (after warm-up) of
  normal_fused     one nfft_normal on the route api.hip picks (row passes and the product with K in one kernel where the
                   planar route with its own row passes runs; elsewhere the same as normal_unfused)
  normal_unfused   the same with NFFT_HIP_TOEPLITZ_FUSED=0: forward FFT stage, toeplitz_multiply_kernel, adjoint FFT stage
  composition      nfft_adjoint(w * nfft_forward(x)) on a cached point plan: the only way before this operator existed
  setup            nfft_toeplitz_kernel (the bandwidth-2N adjoint of the weights, its plan included, and one real FFT)
  multiply         toeplitz_multiply_kernel alone (the library's "multiply" stage timer) and bytes moved / time: per cell 4 B of K
                   and, for each of the two planes of a column, 4 B read and 4 B written
Shapes: C3 (3-D N = 256, m = 4, 10^7 points, one column) and the reference's 2-D N = 16 shape (64 sets of 1 000 points).
Usage: python scripts/bench_toeplitz.py [--reps K] [--only c3|ref]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import torch_nfft_amd as tn  # noqa: E402
from torch_nfft_amd import _lib  # noqa: E402
from bench_pos_grad import SHAPES, timed  # noqa: E402


def run(name, d, N, m, n, B, reps):
    gen = torch.Generator(device="cuda").manual_seed(1)
    pos = torch.rand((n, d), generator=gen, device="cuda") - 0.5
    batch = (torch.arange(n, device="cuda") * B) // n if B > 1 else None
    w = torch.rand(n, generator=gen, device="cuda") + 0.5
    xhat = torch.randn((B,) + (N,) * d, generator=gen, device="cuda", dtype=torch.complex64)
    out = {"shape": name, "d": d, "N": N, "m": m, "n": n, "B": B}

    def setup():
        return tn.nfft_toeplitz_kernel(pos, batch, w, bandwidth=N, cutoff=m)

    out["setup_ms"] = round(timed(setup, max(3, reps // 3), warmup=1), 4)
    K = setup()
    torch.cuda.empty_cache()

    def normal():
        tn.nfft_normal(xhat, K)

    def composition():
        with torch.no_grad():
            tn.nfft_adjoint(tn.nfft_forward(xhat, pos, batch, cutoff=m) * w, pos, batch, bandwidth=N, cutoff=m)

    out["normal_fused_ms"] = round(timed(normal, reps), 4)
    os.environ["NFFT_HIP_TOEPLITZ_FUSED"] = "0"
    try:
        out["normal_unfused_ms"] = round(timed(normal, reps), 4)
        _lib.profile_enable(True, stages=["multiply"])
        for _ in range(reps):
            normal()
        ms, launches = _lib.profile_collect()["multiply"]
        _lib.profile_enable(False)
    finally:
        del os.environ["NFFT_HIP_TOEPLITZ_FUSED"]
    out["multiply_ms"] = round(ms / max(launches, 1), 4)
    cells = B * (2 * N) ** d
    out["multiply_bytes"] = cells * 4 * 5
    out["multiply_TBps"] = round(out["multiply_bytes"] / (out["multiply_ms"] * 1e-3) / 1e12, 3)
    out["composition_ms"] = round(timed(composition, reps), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=sorted(SHAPES))
    a = ap.parse_args()
    for name, sh in SHAPES.items():
        if a.only and name != a.only:
            continue
        print(json.dumps(run(name, reps=a.reps, **sh)), flush=True)


if __name__ == "__main__":
    main()
