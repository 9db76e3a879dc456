"""Developer tool: cost of the second derivatives with respect to the points.  For each shape, device-event times (after
warm-up) of
  fwd+bxp   y = nfft_forward(xhat, pos) plus backward for xhat and pos (first order, as scripts/bench_pos_grad.py)
  hvp       the same with create_graph=True, then the Hessian-vector product: backward of <u, dpos> to pos and xhat
  composed  the same second-order quantities from spectral multipliers of plain transforms: d + d(d+1)/2 forwards of
            i k_a xhat, i^2 k_a k_b xhat and d adjoints of omega u_a (no forward, no first-order backward: not the work of
            hvp)
  dxhat     the native backward of the point gradient asked for dxhat only, on the route api.hip picks (the derivative
            spreading on narrow tilings), and with NFFT_HIP_DXHAT=compose (d adjoints of omega u_a): the choice of DESIGN.md 7b
Shapes: C3 (3-D N = 256, m = 4, 10^7 points, complex, one column) and the reference's 2-D N = 16 shape (m = 3, 1 000 points
per set, 64 sets).  Usage: python scripts/bench_pos_hvp.py [--reps K] [--only c3|ref]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import torch_nfft_amd as tn  # noqa: E402
from torch_nfft_amd import ops  # noqa: E402
from bench_pos_grad import SHAPES, timed  # noqa: E402


def run(name, d, N, m, n, B, reps):
    gen = torch.Generator(device="cuda").manual_seed(1)
    pos = torch.rand((n, d), generator=gen, device="cuda") - 0.5
    batch = (torch.arange(n, device="cuda") * B) // n if B > 1 else None
    xhat = torch.randn((B,) + (N,) * d, generator=gen, device="cuda", dtype=torch.complex64)
    dy = torch.randn(n, generator=gen, device="cuda", dtype=torch.complex64)
    u = torch.randn((n, d), generator=gen, device="cuda")
    x_leaf = xhat.clone().requires_grad_(True)
    p_leaf = pos.clone().requires_grad_(True)
    k = torch.arange(-N // 2, N // 2, device="cuda", dtype=torch.float32) * (2 * math.pi)
    ks = [k.reshape((1,) + tuple(N if b == a else 1 for b in range(d))) for a in range(d)]
    first = [-1j * ks[a] * xhat for a in range(d)]                                   # d/dpos_a
    second = [-ks[a] * ks[b] * xhat + 0j for a in range(d) for b in range(a, d)]     # d^2/dpos_a dpos_b

    def fwd_bxp():
        tn.nfft_forward(x_leaf, p_leaf, batch, cutoff=m).backward(dy)

    def hvp():
        y = tn.nfft_forward(x_leaf, p_leaf, batch, cutoff=m)
        (g,) = torch.autograd.grad(y, p_leaf, dy, create_graph=True)
        (g * u).sum().backward()

    def composed():
        with torch.no_grad():
            for s in first + second:
                tn.nfft_forward(s, pos, batch, cutoff=m)
            for a in range(d):
                tn.nfft_adjoint(dy * u[:, a], pos, batch, bandwidth=N, cutoff=m)

    w = torch.view_as_real(dy).reshape(n, 2).contiguous()

    def dxhat():
        ops.nfft_forward_grad_points_backward(pos, xhat, batch, m, False, w, u, True, False, False)

    out = {"shape": name, "d": d, "N": N, "m": m, "n": n, "B": B}
    for key, fn in (("fwd_bxp_ms", fwd_bxp), ("hvp_ms", hvp), ("composed_ms", composed), ("dxhat_ms", dxhat)):
        out[key] = round(timed(fn, reps), 4)
    os.environ["NFFT_HIP_DXHAT"] = "compose"
    try:
        out["dxhat_composed_ms"] = round(timed(dxhat, reps), 4)
    finally:
        del os.environ["NFFT_HIP_DXHAT"]
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
