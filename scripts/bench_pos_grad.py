"""Developer tool: cost of the gradient with respect to the points.  For each shape, device-event times (after warm-up) of
  fwd       y = nfft_forward(xhat, pos)
  fwd+bx    the same plus backward for xhat only
  fwd+bxp   the same plus backward for xhat and pos
Shapes: C3 (3-D N = 256, m = 4, 10^7 points, complex, one column) and the reference's 2-D N = 16 shape (m = 3, 1 000 points
per set, 64 sets).  Usage: python scripts/bench_pos_grad.py [--reps K] [--only c3|ref]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import torch_nfft_amd as tn  # noqa: E402

SHAPES = {
    "c3": dict(d=3, N=256, m=4, n=10 ** 7, B=1),
    "ref": dict(d=2, N=16, m=3, n=64 * 1000, B=64),
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


def run(name, d, N, m, n, B, reps):
    gen = torch.Generator(device="cuda").manual_seed(1)
    pos = torch.rand((n, d), generator=gen, device="cuda") - 0.5
    batch = (torch.arange(n, device="cuda") * B) // n if B > 1 else None
    xhat = torch.randn((B,) + (N,) * d, generator=gen, device="cuda", dtype=torch.complex64)
    dy = torch.randn(n, generator=gen, device="cuda", dtype=torch.complex64)
    x_leaf = xhat.clone().requires_grad_(True)
    p_leaf = pos.clone().requires_grad_(True)

    def fwd():
        with torch.no_grad():
            tn.nfft_forward(xhat, pos, batch, cutoff=m)

    def fwd_bx():
        tn.nfft_forward(x_leaf, pos, batch, cutoff=m).backward(dy)

    def fwd_bxp():
        tn.nfft_forward(x_leaf, p_leaf, batch, cutoff=m).backward(dy)

    out = {"shape": name, "d": d, "N": N, "m": m, "n": n, "B": B}
    for key, fn in (("fwd_ms", fwd), ("fwd_bx_ms", fwd_bx), ("fwd_bxp_ms", fwd_bxp)):
        out[key] = round(timed(fn, reps), 4)
    out["pos_grad_ms"] = round(out["fwd_bxp_ms"] - out["fwd_bx_ms"], 4)
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
