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
the split path) and 0.2, with and without the field, an orthorhombic box of 3 x 4 x 6 cells and a triclinic one.
The step walks (step_frame.h; profiles/r20_step_frame.md) run on the same layout of points in the unit box at r_c = 1/3 and
in the two other boxes: the product law without a list, with an empty one and with one (bonded_list), the two table laws
in all three ways at T = 1, 2 and 32, the Buckingham table with and without a coefficient on the grid, and the list kernel."""
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
        mass += float(np.abs(a).astype(np.float64).sum())  # (a complex entry by its modulus)
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


def bonded_list(pos, batch, G):
    """pairs of `pos` (set 0 apart from its crowd, and the crowd) with their two scales: chains of three near neighbours
    (the triples), one pair across a border of the G^3 cells, one across the torus seam, four pairs inside the crowd's cell
    that share a point (a row of several entries) and one pair beyond every r_c used here.  The scales cycle through
    (0, 0), (0, 0.5), (1, 1), (0.5, 0): the first is the walk's early return"""
    first = int(np.flatnonzero(batch == 0)[-1]) + 1 - 1500  # set 0 after its crowd
    s = pos[first:first + 1500].astype(np.float64)
    raw = s[:, None, :] - s[None, :, :]
    r = np.linalg.norm(raw - np.rint(raw), axis=2)
    np.fill_diagonal(r, 9.0)
    cell = np.floor((s + 0.5) * G).astype(np.int64).clip(0, G - 1)
    seam = (np.abs(raw) > 0.5).any(2)
    border = (cell[:, None, :] != cell[None, :, :]).any(2) & ~seam
    pairs, used = [], set()

    def add(i, j):
        key = (min(i, j), max(i, j))
        if i != j and key not in used:
            used.add(key)
            pairs.append((first + key[0], first + key[1]))

    for mask in (seam, border):
        i, j = np.unravel_index(np.argmin(np.where(mask, r, 9.0)), r.shape)
        assert r[i, j] < 0.2, "no short pair across the seam or a border"
        add(int(i), int(j))
    for i in range(0, 1500, 50):  # triples: i, its nearest neighbour, and that one's
        j = int(np.argmin(r[i]))
        k = int(np.argsort(r[j])[1]) if int(np.argmin(r[j])) == i else int(np.argmin(r[j]))
        add(i, j), add(j, k), add(i, k)
    i, j = np.unravel_index(np.argmax(np.where(r < 9.0, r, 0.0)), r.shape)
    add(int(i), int(j))  # (beyond the cut: only the list kernel sees it)
    pairs += [(7, k) for k in (3, 11, 200, 399)]  # (the crowd comes first)
    scales = np.array([(0.0, 0.0), (0.0, 0.5), (1.0, 1.0), (0.5, 0.0)])[np.arange(len(pairs)) % 4]
    return np.array(pairs), scales[:, 0], scales[:, 1]


def step_cases():
    """the walks of the nonbonded steps (step_frame.h) and, as a control that shares nothing with them, the list kernel"""
    boxes = (("unit", [1.0, 0.0, 1.0, 0.0, 0.0, 1.0], 1.0 / 3.0), ("ortho", [1.0, 0.0, 1.4, 0.0, 0.0, 2.0], 0.3),
             ("tilted", [1.0, 0.2, 1.1, 0.1, -0.3, 1.3], 0.3))
    rng = np.random.default_rng(11)
    pos, batch = torus_sets(rng, (1500, 40), 400)
    n = len(pos)
    pd, bd = cuda(pos), cuda(batch)
    pairs, sc, sl = bonded_list(pos, batch, 3)
    lists = {"list": tn.ExclusionList(pairs, n, coulomb_scale=sc, dispersion_scale=sl, batch=batch),
             "empty": tn.ExclusionList(np.zeros((0, 2), np.int64), n, batch=batch)}
    csr = {k: (ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight) for k, ex in lists.items()}
    csr["none"] = (None, None, None, None)
    # sigma between 0.02 and 0.03 and epsilon between 0.5 and 1.5, as the steps' tests have them: the closest pair of the crowd
    # (7e-4) stays far inside float32
    q = rng.standard_normal(n).astype(np.float32)
    alpha_c, alpha_d = 10.0, 11.5
    sigma, eps = 0.02 + 0.01 * rng.random(n), 0.5 + rng.random(n)
    c, a = (t.float().cuda() for t in tn.lj_coefficients(torch.from_numpy(sigma), torch.from_numpy(eps)))
    xs3 = torch.stack([cuda(q), c, a], 1)
    for name, box, r_c in boxes:
        walk = (box, alpha_c, alpha_d, r_c)
        report("lj_step_near %s" % name, *ops.nfft_ewald_lj_step_near(pd, xs3, bd, *walk))
        for k in ("empty", "list"):
            report("lj_excl_near %s %s" % (name, k), *ops.nfft_ewald_lj_excl_near(pd, xs3, bd, *csr[k], *walk))
        report("lj_excl_list %s" % name, *ops.nfft_ewald_lj_excl_list(pd, xs3, bd, *csr["list"], *walk))
    for T in (1, 2, 32):
        types = (np.arange(n) % T).astype(np.int32)  # (all types present)
        rng.shuffle(types)
        ts, te = 0.02 + 0.01 * rng.random(T), 0.5 + rng.random(T)
        lj = tn.LJPairTable.lorentz_berthelot(ts, te, cuda(types))
        # exp-6: the minimum at r_m = sigma_ij with depth eps_ij, steepness 12 to 14, and a C8 of a tenth of C6 r_m^2
        rm = 0.5 * (ts[:, None] + ts[None, :])
        e = np.sqrt(te[:, None] * te[None, :])
        steep = 12.0 + 2.0 * rng.random((T, T))
        steep = 0.5 * (steep + steep.T)
        A, B, c6 = e * 6.0 / (steep - 6.0) * np.exp(steep), steep / rm, e * steep / (steep - 6.0) * rm ** 6
        bmh = {"grid": tn.BMHPairTable(A, B, c6, 0.1 * c6 * rm * rm, cuda(types)),
               "nogrid": tn.BMHPairTable(A, B, c6, 0.1 * c6 * rm * rm, cuda(types), grid_c=torch.zeros(T))}
        for name, box, r_c in boxes:
            walk = (box, alpha_c, alpha_d, r_c)
            for k in ("none", "empty", "list"):
                label = "T %d %s %s" % (T, name, k)
                report("lj_table_near " + label,
                       *ops.nfft_ewald_lj_table_near(pd, torch.stack([cuda(q), lj.c], 1), lj.types, lj.table, bd, *csr[k], *walk))
                for grid, tab in bmh.items():
                    report("bmh_table_near %s " % grid + label,
                           *ops.nfft_ewald_bmh_table_near(pd, torch.stack([cuda(q), tab.c], 1), tab.types, tab.table, bd, *csr[k], *walk))
    ops.check_status()


def band_at(rng, shape, offset):
    """a seeded complex64 band of `shape` that starts `offset` (0 or 8) bytes past a 16-byte boundary of its storage"""
    flat = rng.standard_normal((int(np.prod(shape)) + 1, 2)).astype(np.float32)
    band = torch.view_as_complex(cuda(flat))[offset // 8:][:int(np.prod(shape))].view(shape)
    assert band.is_contiguous() and band.data_ptr() % 16 == offset
    return band


def reduction_cases():
    """the reductions on virial_frame.h and the spectral kernels on spectral_frame.h (DESIGN.md section 7w;
    profiles/r21_reduction_frames.md): the pair reductions on the layout of ewald_cases() at every CC, its tail and a second
    column pass; the strided sweeps at one cell per thread at most (N = 12) and at several with both carries (N = 72), the
    one-thread-per-element kernels at N = 12 and 16; bands on and 8 bytes off a 16-byte boundary"""
    boxes = (("ortho", [1.0, 0.0, 1.4, 0.0, 0.0, 2.0], 0.3), ("tilted", [1.0, 0.2, 1.1, 0.1, -0.3, 1.3], 0.3),
             ("unit", [1.0, 0.0, 1.0, 0.0, 0.0, 1.0], 1.0 / 3.0))
    rng = np.random.default_rng(7)
    pos, batch = torus_sets(rng, (1500, 40), 400)
    pd, bd = cuda(pos), cuda(batch)
    charges = {cols: cuda(rng.standard_normal((len(pos), cols)).astype(np.float32)) for cols in (1, 2, 3, 5)}
    alpha = 10.0
    for name, box, r_c in boxes:
        for cols in (1, 2, 3, 5):
            label = "%s r_c %.3f Cr %d" % (name, r_c, cols)
            walk = (pd, charges[cols], bd, box, alpha, r_c)
            report("disp virial near " + label, ops.nfft_ewald_dispersion_virial_near(*walk))
            report("yukawa virial near " + label, ops.nfft_ewald_yukawa_virial_near(*walk, 1.0 / r_c))
            report("step near " + label, *ops.nfft_ewald_step_near(*walk))
    ops.check_status()
    tilted3 = np.array([[1.0, 0.0, 0.0], [0.2, 1.1, 0.0], [0.1, -0.3, 1.3]])
    for N in (12, 72):
        sc = tn.EwaldSplitting(alpha, 0.3, N, box=tilted3)
        sd = tn.DispersionSplitting(11.5, 0.3, N, box=tilted3)
        strain = sd.strain_coeffs()
        for cols, offset in ((1, 0), (2, 0), (4, 0), (3, 0), (5, 0), (1, 8), (2, 8), (4, 8)):
            band = band_at(rng, (2, N, N, N, cols), offset)
            label = "N %d C %d band +%d" % (N, cols, offset)
            if offset:  # (ewald_cases() has the aligned bands of this one)
                report("virial far " + label, ops.nfft_ewald_virial_far(band, sc.coeffs, sc.box6, alpha))
            report("disp virial far " + label, ops.nfft_ewald_dispersion_virial_far(band, sd.coeffs, strain, sd.box6))
            report("step spectral " + label, *ops.nfft_ewald_step_spectral(band, sc.coeffs, sc.box6, alpha))
        for offset in (0, 8):
            band = band_at(rng, (2, N, N, N, 2), offset)
            report("lj step spectral N %d band +%d" % (N, offset),
                   *ops.nfft_ewald_lj_step_spectral(band, sc.coeffs, sd.coeffs, strain, sc.box6, alpha))
    for N in (12, 16):
        sc = tn.EwaldSplitting(alpha, 0.3, N, box=tilted3)
        for order in (1, 2):
            for cols in (1, 2, 4, 3):
                label = "N %d C %d order %d" % (N, cols, order)
                report("dipole spectral " + label,
                       ops.nfft_ewald_dipole_spectral(band_at(rng, (2, N, N, N, 4, cols), 0), sc.coeffs, sc.box6, order))
                report("stokeslet spectral " + label,
                       ops.nfft_ewald_stokeslet_spectral(band_at(rng, (2, N, N, N, 3, cols), 0), sc.stokeslet_coeffs, sc.box6, order))
    ops.check_status()


if __name__ == "__main__":
    print("library:", os.environ.get("NFFT_HIP_LIB", "the package's own"), file=sys.stderr)
    with open("/proc/self/maps") as maps:  # (what the process really runs: one libnfft_hip, under the one core.so)
        print("mapped:", sorted({line.split()[-1] for line in maps if "libnfft_hip" in line}), file=sys.stderr, flush=True)
    near_field_cases()
    ewald_cases()
    step_cases()
    reduction_cases()
