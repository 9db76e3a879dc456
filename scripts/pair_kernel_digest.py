"""Developer tool: SHA-256 of the raw output bytes of the six pair kernels (nearfield.hip, nearfield_grad.hip,
nearfield_pgrad.hip, ewald_near.hip in both geometries, the pair reduction of ewald_virial.hip) and of that file's spectral
reduction on seeded inputs, one line per case.  The kernels have no atomics and add in a fixed order, so two builds that do the same arithmetic print the
same lines: run it once per library (NFFT_HIP_LIB names the one to load, each in a fresh process) and compare, e.g.

    NFFT_HIP_LIB=/path/to/parent/libnfft_hip.so python scripts/pair_kernel_digest.py > parent.txt
    python scripts/pair_kernel_digest.py > new.txt && cmp parent.txt new.txt

The digests pin the compiler's erfcf, expf and logf as much as this code: compare builds of one toolchain, do not store them.
Cases (profiles/r16_pair_frame.md): real columns 1, 2, 3 (the tail predicate of CC = 4) and 5 (a second column pass); two
point sets of 1 500 and 40 points (cells of the small one are empty) and 400 points crowded into one cell of the first
(several work items per cell, a second LDS tile per range); near field in dim 1, 2, 3, all eight kernels at dim 3, Horner
forms of up to 4 and of more terms, shared and separate targets; Ewald with r_c = 1/3 (G = 3: two of three cells of a row on
the split path) and 0.2, with and without the field, an orthorhombic box of 3 x 4 x 6 cells and a triclinic one."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_nfft_amd as tn  # noqa: E402
from torch_nfft_amd import ops  # noqa: E402

SHAPE_C = {"multiquadric": 0.01, "inverse_multiquadric": 0.01, "gaussian": 0.02, "laplacian_rbf": 0.02}
KERNEL_NAMES = ["one_over_modulus", "one_over_square", "logarithm", "thinplate_spline", "multiquadric", "inverse_multiquadric",
                "gaussian", "laplacian_rbf"]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def report(label, *tensors):
    h = hashlib.sha256()
    mass = 0.0
    for t in tensors:
        a = t.detach().cpu().contiguous().numpy()
        h.update(a.tobytes())
        mass += float(np.abs(a.astype(np.float64)).sum())
    assert np.isfinite(mass) and mass > 0.0, label  # (a sum of nothing would compare equal too)
    print("%-58s %s  |sum| %.6e" % (label, h.hexdigest(), mass), flush=True)


def ball_sets(rng, dim, radius, sizes, crowd):
    """points in the ball, `sizes` per point set, and `crowd` more of set 0 inside one cell; (points, batch), by set"""
    n = sum(sizes)
    d = rng.standard_normal((n, dim))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = d * (radius * rng.random((n, 1)) ** (1.0 / dim))
    batch = np.repeat(np.arange(len(sizes)), sizes)
    knot = 0.03 + 0.02 * rng.random((crowd, dim))  # inside the cell [0, 1/8)^dim of every grid used here
    p = np.concatenate([knot, p])
    batch = np.concatenate([np.zeros(crowd, dtype=np.int64), batch])
    return p.astype(np.float32), batch.astype(np.int64)


def near_field_cases():
    # (dim, kernel, p, real columns, shared points): every kernel at dim 3; p = 4 gives Horner forms of 4 and 3 terms (PT = 4),
    # p = 8 of 8 and 7 (PT = 8); every number of columns meets both PT and both layouts
    cases = [(3, KERNEL_NAMES[i], 4 if i in (0, 3, 5, 6) else 8, (1, 2, 3, 5)[i % 4], i in (0, 1, 6, 7)) for i in range(8)]
    cases += [(1, "logarithm", 4, 2, True), (2, "one_over_modulus", 8, 3, False)]
    for dim, name, p, cols, shared in cases:
        rng = np.random.default_rng(1000 * dim + 10 * p + cols)
        kern = tn.RegularizedKernel(name, c=SHAPE_C.get(name, 1.0), dim=dim, bandwidth=64, p=p, eps_I=0.125, eps_B=0.125,
                                    device="cpu")
        s, sb = ball_sets(rng, dim, kern.max_radius, (1500, 40), 400)
        t, tb = (s, sb) if shared else ball_sets(rng, dim, kern.max_radius, (900, 60), 300)
        x = rng.standard_normal((len(s), cols)).astype(np.float32)
        dy = rng.standard_normal((len(t), cols)).astype(np.float32)
        v = rng.standard_normal((len(t), dim, cols)).astype(np.float32)
        sd, sbd = cuda(s), cuda(sb)
        td, tbd = (sd, sbd) if shared else (cuda(t), cuda(tb))
        label = "dim %d %s p %d Cr %d %s" % (dim, name, p, cols, "shared" if shared else "separate")
        args = (kern.kernel_id, kern.c, kern.eps_I)
        gpoly = kern.near_gradient_poly.tolist()
        report("value     " + label, ops.nfft_nearfield(sd, td, cuda(x), sbd, tbd, *args, kern.near_poly.tolist()))
        report("gradient  " + label, ops.nfft_nearfield_gradient(sd, td, cuda(x), sbd, tbd, *args, gpoly, False))
        report("transpose " + label, ops.nfft_nearfield_gradient(sd, td, cuda(v), sbd, tbd, *args, gpoly, True))
        # shared points with both sides needed: the symmetric sweep; otherwise one one-sided sweep per side
        report("points    " + label, *ops.nfft_nearfield_point_gradient(sd, td, cuda(x), cuda(dy), sbd, tbd, *args, gpoly, True, True))
        if shared:
            report("points/s  " + label, *ops.nfft_nearfield_point_gradient(sd, td, cuda(x), cuda(dy), sbd, tbd, *args, gpoly, True, False))
        ops.check_status()


def torus_sets(rng, sizes, crowd):
    """points of [-1/2, 1/2)^3, `sizes` per point set, and `crowd` more of set 0 in the corner cell (0, 0, 0)"""
    p = rng.random((sum(sizes), 3)) - 0.5
    knot = -0.5 + 0.05 * rng.random((crowd, 3))
    batch = np.concatenate([np.zeros(crowd, dtype=np.int64), np.repeat(np.arange(len(sizes)), sizes)])
    return np.concatenate([knot, p]).astype(np.float32), batch


def ewald_cases():
    unit = [1.0, 0.0, 1.0, 0.0, 0.0, 1.0]
    ortho = [1.0, 0.0, 1.4, 0.0, 0.0, 2.0]       # 3 x 4 x 6 cells at r_c = 0.3
    tilted = [1.0, 0.2, 1.1, 0.1, -0.3, 1.3]     # perpendicular widths 0.977, 1.072, 1.3: 3 x 3 x 4 cells at r_c = 0.3
    rng = np.random.default_rng(7)
    pos, batch = torus_sets(rng, (1500, 40), 400)
    pd, bd = cuda(pos), cuda(batch)
    charges = {cols: cuda(rng.standard_normal((len(pos), cols)).astype(np.float32)) for cols in (1, 2, 3, 5)}
    alpha = 10.0
    for r_c, cols, field in ((1.0 / 3.0, 1, True), (0.2, 3, False), (1.0 / 3.0, 5, False), (0.2, 2, True)):
        report("ewald cubic r_c %.3f Cr %d field %d" % (r_c, cols, field), *ops.nfft_ewald_near(pd, charges[cols], bd, alpha, r_c, field)[:1 + field])
    for name, box, cols, field in (("ortho", ortho, 2, True), ("tilted", tilted, 5, True), ("ortho", ortho, 3, False),
                                   ("tilted", tilted, 1, False), ("unit", unit, 3, True)):
        report("ewald box %s Cr %d field %d" % (name, cols, field), *ops.nfft_ewald_near_box(pd, charges[cols], bd, box, alpha, 0.3, field)[:1 + field])
    for name, box, r_c, cols in (("ortho", ortho, 0.3, 1), ("tilted", tilted, 0.3, 3), ("unit", unit, 1.0 / 3.0, 5), ("tilted", tilted, 0.2, 2)):
        report("virial near %s r_c %.3f Cr %d" % (name, r_c, cols), ops.nfft_ewald_virial_near(pd, charges[cols], bd, box, alpha, r_c))
    # the spectral reduction of the same file (its workgroup sum is the pair reduction's): a grid of one cell per thread and
    # one of several, the 16-byte loads of two and four columns, the tail predicate and a second column pass
    tilted3 = np.array([[1.0, 0.0, 0.0], [0.2, 1.1, 0.0], [0.1, -0.3, 1.3]])
    for N, cols in ((12, 3), (12, 5), (72, 2), (72, 1), (12, 4)):
        sp = tn.EwaldSplitting(alpha, 0.3, N, box=tilted3)
        band = rng.standard_normal((2, N, N, N, cols, 2)).astype(np.float32)
        band = torch.view_as_complex(cuda(band))
        report("virial far N %d C %d" % (N, cols), ops.nfft_ewald_virial_far(band, sp.coeffs, sp.box6, alpha))
    ops.check_status()


if __name__ == "__main__":
    print("library:", os.environ.get("NFFT_HIP_LIB", "the package's own"), file=sys.stderr)
    with open("/proc/self/maps") as maps:  # (what the process really runs: one libnfft_hip, under the one core.so)
        print("mapped:", sorted({line.split()[-1] for line in maps if "libnfft_hip" in line}), file=sys.stderr, flush=True)
    near_field_cases()
    ewald_cases()
