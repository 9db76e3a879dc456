"""Developer tool: cost of the gradient of nfft_fastsum with respect to its points.  For each shape and coefficient kind,
device-event medians (after warm-up) of
  fwd       y = nfft_fastsum(x, c, sources, targets)
  fwd+bx    the same plus backward for x only
  fwd+bxp   the same plus backward for x, sources and targets
  compose   the same three gradients through nfft_forward(c * nfft_adjoint(x, sources), targets)
Shapes: C5 (3-D N = 256, m = 4, 10^6 sources and 10^6 targets in the quarter ball, one column) and the reference's 2-D
N = 16 shape (m = 3, 1 000 points per set, 64 sets).  Coefficients: real (gaussian_analytic_coeffs) and complex
(gaussian_interpolated_coeffs).  Usage: python scripts/bench_fastsum_grad.py [--reps K] [--only c5|ref] [--once]
(--once: one fwd+bxp and one compose step per case after warm-up each, for a kernel trace)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import torch_nfft_amd as tn  # noqa: E402

SHAPES = {
    "c5": dict(d=3, N=256, m=4, ns=10 ** 6, nt=10 ** 6, B=1),
    "ref": dict(d=2, N=16, m=3, ns=64 * 1000, nt=64 * 1000, B=64),
}


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    times.sort()
    return times[len(times) // 2]


def ball(n, d, gen):
    """n points in the ball of radius 1/4 (fastsum's domain)."""
    p = torch.randn((n, d), generator=gen, device="cuda")
    r = torch.rand((n, 1), generator=gen, device="cuda") ** (1.0 / d)
    return 0.25 * r * p / p.norm(dim=1, keepdim=True)


def run(name, coeff_kind, d, N, m, ns, nt, B, reps, once):
    gen = torch.Generator(device="cuda").manual_seed(1)
    src, tgt = ball(ns, d, gen), ball(nt, d, gen)
    sb = (torch.arange(ns, device="cuda") * B) // ns if B > 1 else None
    tb = (torch.arange(nt, device="cuda") * B) // nt if B > 1 else None
    x = torch.randn((ns, 1), generator=gen, device="cuda")
    dy = torch.randn((nt, 1), generator=gen, device="cuda")
    c = (tn.gaussian_analytic_coeffs(0.1, d, N) if coeff_kind == "real" else
         tn.gaussian_interpolated_coeffs(0.1, d, N, 0, 0.0))
    x_leaf, s_leaf, t_leaf = x.clone().requires_grad_(True), src.clone().requires_grad_(True), tgt.clone().requires_grad_(True)
    cshape = (1,) + (N,) * d + (1,)

    def fwd():
        with torch.no_grad():
            tn.nfft_fastsum(x, c, src, tgt, sb, tb, cutoff=m)

    def fwd_bx():
        tn.nfft_fastsum(x_leaf, c, src, tgt, sb, tb, cutoff=m).backward(dy)

    def fwd_bxp():
        tn.nfft_fastsum(x_leaf, c, s_leaf, t_leaf, sb, tb, cutoff=m).backward(dy)

    def compose():
        band = tn.nfft_adjoint(x_leaf, s_leaf, sb, bandwidth=N, cutoff=m)
        tn.nfft_forward(band * c.reshape(cshape), t_leaf, tb, cutoff=m, real_output=True).backward(dy)

    out = {"shape": name, "coeffs": coeff_kind, "d": d, "N": N, "m": m, "ns": ns, "nt": nt, "B": B}
    if once:
        timed(fwd_bxp, 1)
        timed(compose, 1)
        return out
    for key, fn in (("fwd_ms", fwd), ("fwd_bx_ms", fwd_bx), ("fwd_bxp_ms", fwd_bxp), ("compose_ms", compose)):
        out[key] = round(timed(fn, reps), 4)
    out["points_grad_ms"] = round(out["fwd_bxp_ms"] - out["fwd_bx_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=sorted(SHAPES))
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    for name, sh in SHAPES.items():
        if a.only and name != a.only:
            continue
        for kind in ("real", "complex"):
            print(json.dumps(run(name, kind, reps=a.reps, once=a.once, **sh)), flush=True)


if __name__ == "__main__":
    main()
