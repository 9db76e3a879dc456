"""Developer tool: what the host layer of the library decides, one line per query, for comparing two builds with `diff`.

  python scripts/dump_host_layer.py routes OUT   nfft_dbg_route and nfft_dbg_fft_route (host code only: no device needed)
  python scripts/dump_host_layer.py sizes OUT    nfft_hip_plan_bytes, nfft_hip_spread_scratch_bytes and every transform-family
                                                 nfft_hip_*_workspace_bytes (these make rocFFT plans: a device is needed)

NFFT_HIP_LIB selects the library, NFFT_HIP_CHUNK_BYTES the chunk budget, as for every process that loads it.  The problems:
dim 1-3, N in {16, 32, 64, 128}, m in {2, 4, 8}, 1 / 2 / 4 columns, 1 / 3 / 16 point sets, 0 / 10^3 / 10^5 / 10^6 points, real
and complex."""
import ctypes
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_nfft_amd import _lib  # noqa: E402


def problems():
    for dim, N, m, C, B, n in itertools.product((1, 2, 3), (16, 32, 64, 128), (2, 4, 8), (1, 2, 4), (1, 3, 16),
                                                (0, 1000, 100_000, 1_000_000)):
        if 2 * m + 2 <= 2 * N:
            yield "d%d N%d m%d C%d B%d n%d" % (dim, N, m, C, B, n), _lib.Problem(dim, n, C, B, N, m)


def routes(lib, out):
    for tag, p in problems():
        P = ctypes.byref(p)
        for Cr in (p.num_columns, 2 * p.num_columns):
            r = (ctypes.c_int32 * 8)()
            rc = lib.nfft_dbg_route(P, Cr, r)
            out.write("%s route Cr%d: %d %s\n" % (tag, Cr, rc, list(r)))
        for adjoint, cplx, real in itertools.product((0, 1), (0, 1), (0, 1)):
            r = (ctypes.c_int64 * 11)()
            rc = lib.nfft_dbg_fft_route(P, adjoint, cplx, real, 0, r)
            tail = (ctypes.c_int64 * 11)()
            rem = r[3] % r[2] if rc == 0 and r[2] > 0 else 0
            if rem:  # the remainder chunk's route
                lib.nfft_dbg_fft_route(P, adjoint, cplx, real, rem, tail)
            out.write("%s fft a%d c%d r%d: %d %s rem %d %s\n" % (tag, adjoint, cplx, real, rc, list(r), rem, list(tail)[4:]))


def sizes(lib, out):
    seen = set()
    for tag, p in problems():
        P = ctypes.byref(p)
        row = [("plan", lib.nfft_hip_plan_bytes(P))]
        row += [("scratch%d" % k, lib.nfft_hip_spread_scratch_bytes(P, k * p.num_columns)) for k in (1, 2)]
        for cplx, real in itertools.product((0, 1), (0, 1)):
            v = "c%dr%d" % (cplx, real)
            row += [("adjoint " + v, lib.nfft_hip_adjoint_workspace_bytes(P, cplx, real)),
                    ("forward " + v, lib.nfft_hip_forward_workspace_bytes(P, cplx, real)),
                    ("forward_grad " + v, lib.nfft_hip_forward_grad_workspace_bytes(P, cplx, real)),
                    ("grad_backward " + v, lib.nfft_hip_forward_grad_points_backward_workspace_bytes(P, cplx, real))]
        for cplx in (0, 1):
            row += [("fastsum c%d s%d p%d" % (cplx, shared, planned),
                     lib.nfft_hip_fastsum_workspace_bytes(P, P, cplx, shared, planned))
                    for shared, planned in itertools.product((0, 1), (0, 1))]
            row.append(("fastsum_grad c%d" % cplx, lib.nfft_hip_fastsum_grad_workspace_bytes(P, P, cplx)))
        row += [("toeplitz_kernel", lib.nfft_hip_toeplitz_kernel_workspace_bytes(P)),
                ("toeplitz", lib.nfft_hip_toeplitz_workspace_bytes(P))]
        if (p.N, p.dim) not in seen:
            seen.add((p.N, p.dim))
            row.append(("coeffs", lib.nfft_hip_coeffs_workspace_bytes(p.N, p.dim)))
        for name, value in row:
            out.write("%s %s: %d\n" % (tag, name, value))
        out.flush()


if __name__ == "__main__":
    mode, path = sys.argv[1], sys.argv[2]
    with open(path, "w") as f:
        f.write("chunk budget %s\n" % (os.environ.get("NFFT_HIP_CHUNK_BYTES") or "default"))
        {"routes": routes, "sizes": sizes}[mode](_lib.load(), f)
