"""Times nfft_ewald and its wrapped pair sweep:

    python scripts/bench_ewald.py [--points 100000 1000000] [--neighbours 100] [--tol 1e-5] [--reps 10]

Charges uniform in the unit box, one real column, cutoff m = 4.  r_c is chosen for `neighbours` charges inside the sphere
of radius r_c around a charge, n (4/3) pi r_c^3 = neighbours, and alpha and N by EwaldSplitting.from_tolerance(tol, r_c).
Device-event medians of `reps` calls after two warm-up calls:
  whole sum     nfft_ewald without and with the field
  far field     nfft_fastsum with the splitting's coefficients (the value's far part)
  near sweep    ops.nfft_ewald_near as a whole, without and with the field, and its pair loop on its own
                (nfft_hip_ewald_near through the C ABI on the arrays that the operator's plumbing made, restated here)
  yardstick     the existing 1/r value loop (nfft_hip_nearfield, kernel one_over_modulus, p = 4) on the same points
                scaled into [-1/4, 1/4)^3 with eps_I = r_c / 2 and the same number of cells per axis: the same cells and
                pairs except that its walk does not wrap
  pairs         distance tests per call = sum over targets of the sources in the 27 cells around it (wrapped for the
                Ewald sweep, clipped for the yardstick), and nanoseconds per tested pair for each loop
One JSON line per problem size.

    python scripts/bench_ewald.py --box a,b,c | --box A00,A10,A11,A20,A21,A22 [...]

times the same in an orthorhombic or triclinic box: charges uniform in the box (fractional
positions), n (4/3) pi r_c^3 = neighbours V, EwaldSplitting.from_tolerance(tol, r_c, box=...); the whole sum, the far field,
the near operator ops.nfft_ewald_near_box and its pair loop on its own (nfft_hip_ewald_near_box on restated plumbing), with
the pairs tested and picoseconds per tested pair.  On the identity box (--box 1,1,1) the unit-cube pair loop runs on the same
points as well: the same cells and pairs, three products and three FMAs fewer per tested pair.  No 1/r yardstick here.

    python scripts/bench_ewald.py --virial [--box ...] [...]

adds, after each of the rows above and in the same process, a row for the virial tensor in the same
box (the identity box without --box) on the same charges: nfft_ewald_virial beside nfft_ewald(field=True); the pair loop of
the virial kernel (nfft_hip_ewald_virial_near on restated plumbing, its second-level sum included) beside the field loop,
in picoseconds per tested pair; and the far reduction (ops.nfft_ewald_virial_far) beside the torch composition
((band.abs() ** 2)[..., None] * coef7).sum(...) on the same band, with the bytes of band per second that each reaches.

    python scripts/bench_ewald.py --dispersion [...]

times the dispersion sum 1/r^6 in the unit cube instead: the same points and r_c, coefficients in
[0.5, 1.5), alpha and N by DispersionSplitting.from_tolerance(tol, r_c); nfft_ewald_dispersion without and with the field, its
far field, the near operator ops.nfft_ewald_dispersion_near and its pair loop on its own (nfft_hip_ewald_dispersion_near
on restated plumbing), and beside it, in the same run on the same sorted points, cells and r_c, the Coulomb pair loop
(nfft_hip_ewald_near with the alpha of EwaldSplitting.from_tolerance): the same pairs are tested and the same pass the cut,
what differs is the pair weight.

    python scripts/bench_ewald.py --dispersion --virial [...]

adds the row of --virial for the dispersion sum's virial tensor after each of those, in the identity
box on the same points and coefficients: nfft_ewald_dispersion_virial beside nfft_ewald_dispersion(field=True); the pair loop
of nfft_hip_ewald_dispersion_virial_near beside the dispersion field loop (nfft_hip_ewald_dispersion_near_box), in
picoseconds per tested pair; and the far reduction (ops.nfft_ewald_dispersion_virial_far) beside the torch composition on
the same band, with its agreement with it.

    python scripts/bench_ewald.py --dipole [...]

times the sum of charges and point dipoles in the unit cube on the same points, r_c, alpha and N:
nfft_ewald_dipole of order 1 and 2 beside nfft_ewald with its field; the near operator; the spectral kernel beside the
torch composition on the same band; and the dipole pair loops of order 1 and 2 (nfft_hip_ewald_dipole_near on restated
plumbing) beside the Coulomb pair loop with its field (nfft_hip_ewald_near) on the same sorted points and cells.  The calls
of a group are timed in turn (a, b, c, a, b, c, ...), median, minimum and maximum of `reps` each.

    python scripts/bench_ewald.py --stokeslet [...]

times the periodic Stokeslet sum in the unit cube on the same points, r_c, alpha and N, in the same way:
nfft_ewald_stokeslet for u and for (u, G) beside nfft_ewald with its field; the near operator; the spectral kernel beside the
torch composition on the same band; and the Stokeslet pair loops of order 1 and 2 (nfft_hip_ewald_stokeslet_near on restated
plumbing) beside the Coulomb pair loop with its field on the same sorted points and cells.

    python scripts/bench_ewald.py --rpy [--phi 0.1] [...]

times the periodic Rotne-Prager-Yamakawa sum in the same way on the same points, r_c, alpha and N, for
spheres of the volume fraction phi, n (4/3) pi a^3 = phi (the points are uniform, not a hard-sphere configuration: the share
(2 a / r_c)^3 of the pairs inside the cut overlap and take the second branch; that expected share is reported, not counted): nfft_ewald_rpy for
u and for (u, G) beside nfft_ewald with its field and nfft_ewald_stokeslet; the near operator; and the pair loops of order
1 and 2 (nfft_hip_ewald_rpy_near on restated plumbing) beside the Stokeslet loops and the Coulomb loop with its field.  The
far part is the Stokeslet sum's with another table and is not timed again.

    python scripts/bench_ewald.py --exclusions [--box ...] [...]

times the bonded-pair correction of the Coulomb sum on rigid triples with three listed pairs each (a
water model) in the unit cube or in the box: the list kernel alone (nfft_hip_ewald_excl / _box on restated plumbing) and the
operator around it beside the pair sweep with its field and beside the whole nfft_ewald(field=True) with and without the
list, and the bytes the list kernel must move (row_start, col, weights, the gathered positions and values, the outputs) as a
share of the HBM's specified rate.

    python scripts/bench_ewald.py --step [--box ...] [--exclusions] [...]

times the fused step in the box (the identity box without --box) on uniform charges, one row per point
count: nfft_ewald(field=True), nfft_ewald_virial, their sum and nfft_ewald_step; the two pair loops and the fused one on their
own (nfft_hip_ewald_near_box, nfft_hip_ewald_virial_near and nfft_hip_ewald_step_near on restated plumbing, in picoseconds per
tested pair); and the torch product with field_coeffs() plus ops.nfft_ewald_virial_far beside ops.nfft_ewald_step_spectral on
the same band.  All are timed in turn, median, minimum and maximum of `reps` each.  With --exclusions the three public calls
carry a list of the n / 2 pairs (2 i, 2 i + 1).

    python scripts/bench_ewald.py --lj-step [--box ...] [...]

times the Lennard-Jones + Coulomb step on a jittered lattice with sigma = 0.8 x its spacing, one row per
point count: nfft_ewald_step, nfft_ewald_dispersion(field=True) and nfft_ewald_dispersion_virial (each with the splitting that
from_tolerance gives it, the bandwidth raised to the next size with prime factors <= 7 unless --bandwidth-as-is), their sum and
nfft_ewald_lj_step (one bandwidth for both sums, the larger of the two); the three pair
loops and the new one on restated plumbing; the three spectral passes and the new one on the same band.  All are timed in turn,
median, minimum and maximum of `reps` each.

    python scripts/bench_ewald.py --lj-step --exclusions [--box ...] [...]

times the step with bonded-pair exclusions on n / 3 rigid triples (the water model of --exclusions:
charges -0.834, 0.417, 0.417, the bond 0.3 of the molecules' spacing, 104.5 degrees, Lennard-Jones on the first atom of each)
on a jittered lattice with their three listed pairs each at scale 0, one row per point count: nfft_ewald_lj_excl_step beside
nfft_ewald_lj_step on the same points (what the masking costs) and beside nfft_ewald_step, nfft_ewald_dispersion(field=True)
and nfft_ewald_dispersion_virial with exclusions= (the yardstick of section 7r); and the masked walk, the unmasked walk and
the list kernel as operators.  All are timed in turn, median, minimum and maximum of `reps` each.

    python scripts/bench_ewald.py --lj-step --table [--exclusions] [--types 2 32] [--box ...] [...]

times the step with per-type-pair parameters, one row per point count and type count T, Lorentz-Berthelot
tables with sigma between 0.5 and 0.8 of the spacing: the new pair operator beside _nfft_ewald_lj_step_near on the same points
(the jittered lattice of --lj-step) or, with --exclusions, beside _nfft_ewald_lj_excl_near (the rigid triples of --lj-step
--exclusions; the oxygens take the first T / 2 types, the hydrogens the others with epsilon = 0), and nfft_ewald_lj_table_step
beside nfft_ewald_lj_step / nfft_ewald_lj_excl_step.  The yardsticks take geometric (c, a) of the same sigma and epsilon: other
numbers, the same work.  All are timed in turn, median, minimum and maximum of `reps` each.

    python scripts/bench_ewald.py --lj-step --bmh [--exclusions] [--types 2 32] [--box ...] [...]

times the Buckingham / Born-Mayer-Huggins + Coulomb step, one row per point count and type count T,
exp-6 tables with r_m between 0.7 and 1.0 of the spacing and a C8 term: the new pair operator beside the untouched
_nfft_ewald_lj_table_near and nfft_ewald_bmh_table_step beside the untouched nfft_ewald_lj_table_step, on the same points, types
and list in the same process (the points of --lj-step --table; the yardsticks take a Lorentz-Berthelot table of the same sizes:
other numbers, the same frame), and nfft_ewald_bmh_table_step(dispersion=None) with nothing on the grid.  All are timed in turn,
median, minimum and maximum of `reps` each.

    python scripts/bench_ewald.py --yukawa [--virial] [--screening 1.0] [...]

times the screened Coulomb sum e^(-lambda r) / r in the unit cube on the same points, r_c, alpha and N,
lambda = screening / r_c: nfft_ewald_yukawa without and with the field beside nfft_ewald; the near operator; and the pair
loops (nfft_hip_ewald_yukawa_near on restated plumbing) beside the Coulomb pair loops on the same sorted points and cells,
timed in turn.  With --virial a second row in the identity box: nfft_ewald_yukawa_virial beside nfft_ewald_yukawa(field=True),
and the pair loop of nfft_hip_ewald_yukawa_virial_near beside the field loop and beside the Coulomb virial loop.
"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_nfft_amd as tn  # noqa: E402
from torch_nfft_amd import _lib  # noqa: E402


def median_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def cell_order(pos, G, offset, scale):
    """what core.so's cell orders do for one point set without a batch vector: cell = floor((pos + offset) * scale)"""
    cell = ((pos + offset) * float(scale)).floor().clamp(0, G - 1).to(torch.int64)
    key = cell[:, 0] + cell[:, 1] * G + cell[:, 2] * (G * G)
    skey, order = torch.sort(key, stable=True)
    start = torch.searchsorted(skey, torch.arange(G ** 3 + 1, device=pos.device), out_int32=True)
    return pos.index_select(0, order), order, start


def pairs_tested(v, G):
    """(wrapped, clipped): targets of a cell x sources of the 27 cells around it, with and without the wrap"""
    cells = np.clip(np.floor((v + np.float32(0.5)) * np.float32(G)), 0, G - 1).astype(np.int64)
    count = np.zeros((G,) * 3, dtype=np.int64)
    np.add.at(count, (cells[:, 0], cells[:, 1], cells[:, 2]), 1)
    shifts = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    wrapped = sum(np.roll(count, s, axis=(0, 1, 2)) for s in shifts)
    pad = np.zeros((G + 2,) * 3, dtype=np.int64)
    pad[1:-1, 1:-1, 1:-1] = count
    clipped = sum(pad[1 + a:G + 1 + a, 1 + b:G + 1 + b, 1 + c:G + 1 + c] for a, b, c in shifts)
    return int((count * wrapped).sum()), int((count * clipped).sum())


def box_cell_order(pos, G):
    """cell_order for fractional positions in [-1/2, 1/2)^3 and a cell count per axis"""
    key, stride = 0, 1
    for a in range(3):
        key = key + ((pos[:, a] + 0.5) * float(G[a])).floor().clamp(0, G[a] - 1).to(torch.int64) * stride
        stride *= G[a]
    skey, order = torch.sort(key, stable=True)
    start = torch.searchsorted(skey, torch.arange(stride + 1, device=pos.device), out_int32=True)
    return pos.index_select(0, order), order, start


def box_pairs_tested(v, G):
    """targets of a cell x sources of the 27 wrapped cells around it, G = (G0, G1, G2)"""
    cells = [np.clip(np.floor((v[:, a] + np.float32(0.5)) * np.float32(G[a])), 0, G[a] - 1).astype(np.int64) for a in range(3)]
    count = np.zeros(tuple(G), dtype=np.int64)
    np.add.at(count, tuple(cells), 1)
    wrapped = sum(np.roll(count, (a, b, c), axis=(0, 1, 2)) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1))
    return int((count * wrapped).sum())


def run_box(lib, n, args):
    m = 4
    box = args.box if len(args.box) == 6 else [args.box[0], 0.0, args.box[1], 0.0, 0.0, args.box[2]]
    A = [[box[0], 0.0, 0.0], [box[1], box[2], 0.0], [box[3], box[4], box[5]]]
    probe = tn.EwaldSplitting(1.0, 1e-3 * min(box[0], box[2], box[5]), 2, box=A, device="cpu")  # (volume and widths)
    r_c = min((3.0 * args.neighbours * probe.volume / (4.0 * math.pi * n)) ** (1.0 / 3.0), min(probe.widths) / 3.0)
    sp = tn.EwaldSplitting.from_tolerance(args.tol, r_c, box=A)
    rng = np.random.default_rng(0)
    v = (rng.random((n, 3)) - 0.5).astype(np.float32)
    v[v >= 0.5] = -0.5  # (rounded up to the face: the same point)
    pos = torch.from_numpy(v).cuda()
    q = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    G = sp.cells
    tested = box_pairs_tested(v, G)
    whole = median_ms(lambda: tn.nfft_ewald(q, pos, splitting=sp, cutoff=m, fractional=True), args.reps)
    whole_f = median_ms(lambda: tn.nfft_ewald(q, pos, splitting=sp, cutoff=m, field=True, fractional=True), args.reps)
    far = median_ms(lambda: tn.nfft_fastsum(q, sp.coeffs, pos, cutoff=m), args.reps)
    near = median_ms(lambda: tn.ops.nfft_ewald_near_box(pos, q, None, box, sp.alpha, r_c, False), args.reps)
    near_f = median_ms(lambda: tn.ops.nfft_ewald_near_box(pos, q, None, box, sp.alpha, r_c, True), args.reps)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    spos, order, start = box_cell_order(pos, G)
    xs = q.index_select(0, order).reshape(n, 1).contiguous()
    z, f = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda")
    loops = {}
    for with_field in (0, 1):
        p = _lib.EwaldBoxProblem(cells=(ctypes.c_int32 * 3)(*G), with_field=with_field, num_points=n, num_columns=1,
                                 batch_size=1, alpha=sp.alpha, r_cut=r_c, box=(ctypes.c_double * 6)(*box))
        nbytes = lib.nfft_hip_ewald_near_box_workspace_bytes(ctypes.byref(p))
        assert nbytes > 0, _lib.last_error()
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def loop():
            _lib.check(lib.nfft_hip_ewald_near_box(ctypes.byref(p), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                                   order.data_ptr(), z.data_ptr(), f.data_ptr(), ws.data_ptr(), nbytes, stream))

        loops[with_field] = median_ms(loop, args.reps)
    zo, fo = tn.ops.nfft_ewald_near_box(pos, q, None, box, sp.alpha, r_c, True)
    assert torch.equal(zo, z[:, 0]) and torch.equal(fo, f), "the restated plumbing must give the operator's bits"
    out = {"bench": "ewald_box", "box": box, "points": n, "neighbours": args.neighbours, "tol": args.tol,
           "r_cut": round(r_c, 5), "alpha": round(sp.alpha, 3), "N": sp.bandwidth, "m": m, "cells": list(G),
           "ewald_ms": round(whole, 4), "ewald_field_ms": round(whole_f, 4), "far_ms": round(far, 4),
           "near_ms": round(near, 4), "near_field_ms": round(near_f, 4),
           "pair_loop_ms": round(loops[0], 4), "pair_loop_field_ms": round(loops[1], 4), "pairs_tested": tested,
           "ps_per_pair": round(loops[0] * 1e9 / tested, 3), "ps_per_pair_field": round(loops[1] * 1e9 / tested, 3)}
    if box == [1.0, 0.0, 1.0, 0.0, 0.0, 1.0] and G[0] == G[1] == G[2] == lib.nfft_hip_ewald_near_cells(r_c, 1):
        # the unit-cube kernel on the same sorted points: the same cells, the same pairs
        cube = {}
        zc, fc = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda")
        for with_field in (0, 1):
            p = _lib.EwaldProblem(cells_per_axis=G[0], with_field=with_field, num_points=n, num_columns=1, batch_size=1,
                                  alpha=sp.alpha, r_cut=r_c)
            nbytes = lib.nfft_hip_ewald_near_workspace_bytes(ctypes.byref(p))
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

            def cube_loop():
                _lib.check(lib.nfft_hip_ewald_near(ctypes.byref(p), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                                   order.data_ptr(), zc.data_ptr(), fc.data_ptr(), ws.data_ptr(), nbytes,
                                                   stream))

            cube[with_field] = median_ms(cube_loop, args.reps)
        out.update({"cube_pair_loop_ms": round(cube[0], 4), "cube_pair_loop_field_ms": round(cube[1], 4),
                    "cube_ps_per_pair": round(cube[0] * 1e9 / tested, 3),
                    "cube_ps_per_pair_field": round(cube[1] * 1e9 / tested, 3),
                    "box_over_cube": round(loops[0] / cube[0], 3), "box_over_cube_field": round(loops[1] / cube[1], 3),
                    "max_abs_difference": float((z - zc).abs().max())})
    tn.ops.check_status()
    print(json.dumps(out))


def run_virial(lib, n, args):
    m = 4
    box = [1.0, 0.0, 1.0, 0.0, 0.0, 1.0] if args.box is None else \
        (args.box if len(args.box) == 6 else [args.box[0], 0.0, args.box[1], 0.0, 0.0, args.box[2]])
    A = [[box[0], 0.0, 0.0], [box[1], box[2], 0.0], [box[3], box[4], box[5]]]
    probe = tn.EwaldSplitting(1.0, 1e-3 * min(box[0], box[2], box[5]), 2, box=A, device="cpu")  # (volume and widths)
    r_c = min((3.0 * args.neighbours * probe.volume / (4.0 * math.pi * n)) ** (1.0 / 3.0), min(probe.widths) / 3.0)
    sp = tn.EwaldSplitting.from_tolerance(args.tol, r_c, box=A)
    rng = np.random.default_rng(0)
    v = (rng.random((n, 3)) - 0.5).astype(np.float32)
    v[v >= 0.5] = -0.5  # (rounded up to the face: the same point)
    pos = torch.from_numpy(v).cuda()
    q = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    G, N = sp.cells, sp.bandwidth
    tested = box_pairs_tested(v, G)
    field = median_ms(lambda: tn.nfft_ewald(q, pos, splitting=sp, cutoff=m, field=True, fractional=True), args.reps)
    virial = median_ms(lambda: tn.nfft_ewald_virial(q, pos, splitting=sp, cutoff=m, fractional=True), args.reps)
    adjoint = median_ms(lambda: tn.nfft_adjoint(q, pos, bandwidth=N, cutoff=m), args.reps)
    near_op = median_ms(lambda: tn.ops.nfft_ewald_virial_near(pos, q, None, box, sp.alpha, r_c), args.reps)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    spos, order, start = box_cell_order(pos, G)
    xs = q.index_select(0, order).reshape(n, 1).contiguous()
    z, f = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda")
    p = _lib.EwaldBoxProblem(cells=(ctypes.c_int32 * 3)(*G), with_field=1, num_points=n, num_columns=1, batch_size=1,
                             alpha=sp.alpha, r_cut=r_c, box=(ctypes.c_double * 6)(*box))
    nbytes = lib.nfft_hip_ewald_near_box_workspace_bytes(ctypes.byref(p))
    vbytes = lib.nfft_hip_ewald_virial_near_workspace_bytes(ctypes.byref(p))
    assert nbytes > 0 and vbytes > 0, _lib.last_error()
    ws, vws = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(vbytes, dtype=torch.uint8, device="cuda")
    seven = torch.zeros(1, 7, 1, dtype=torch.float64, device="cuda")

    def field_loop():
        _lib.check(lib.nfft_hip_ewald_near_box(ctypes.byref(p), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                               order.data_ptr(), z.data_ptr(), f.data_ptr(), ws.data_ptr(), nbytes, stream))

    def virial_loop():
        _lib.check(lib.nfft_hip_ewald_virial_near(ctypes.byref(p), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                                  seven.data_ptr(), vws.data_ptr(), vbytes, stream))

    loop_f, loop_v = median_ms(field_loop, args.reps), median_ms(virial_loop, args.reps)
    assert torch.equal(tn.ops.nfft_ewald_virial_near(pos, q, None, box, sp.alpha, r_c), seven[:, :, 0]), \
        "the restated plumbing must give the operator's bits"
    # the far reduction beside the torch composition on the same band
    band = tn.nfft_adjoint(q, pos, bandwidth=N, cutoff=m)  # [1, N, N, N]
    kappa = sp._kappa()
    k2 = (kappa * kappa).sum(3)
    fac = -2.0 * (1.0 / torch.where(k2 > 0, k2, torch.ones_like(k2)) + (math.pi / sp.alpha) ** 2)
    coef7 = [torch.ones_like(k2)] + [1.0 + fac * kappa[..., a] * kappa[..., a] for a in range(3)] + \
            [fac * kappa[..., a] * kappa[..., b] for a, b in ((1, 2), (0, 2), (0, 1))]
    coef7 = (0.5 * sp._b64.unsqueeze(3) * torch.stack(coef7, 3)).to(torch.float32).cuda()  # [N, N, N, 7]
    far_v = median_ms(lambda: tn.ops.nfft_ewald_virial_far(band, sp.coeffs, box, sp.alpha), args.reps)
    far_t = median_ms(lambda: ((band.abs() ** 2)[..., None] * coef7).sum((1, 2, 3)), args.reps)
    got = tn.ops.nfft_ewald_virial_far(band, sp.coeffs, box, sp.alpha)
    want = ((band.abs() ** 2)[..., None] * coef7).sum((1, 2, 3)).double()
    tn.ops.check_status()
    band_bytes = band.numel() * 8
    print(json.dumps({"bench": "ewald_virial", "box": box, "points": n, "neighbours": args.neighbours, "tol": args.tol,
                      "r_cut": round(r_c, 5), "alpha": round(sp.alpha, 3), "N": N, "m": m, "cells": list(G),
                      "ewald_field_ms": round(field, 4), "ewald_virial_ms": round(virial, 4),
                      "virial_over_field": round(virial / field, 3), "adjoint_ms": round(adjoint, 4),
                      "virial_near_ms": round(near_op, 4), "pair_loop_field_ms": round(loop_f, 4),
                      "pair_loop_virial_ms": round(loop_v, 4), "pairs_tested": tested,
                      "ps_per_pair_field": round(loop_f * 1e9 / tested, 3),
                      "ps_per_pair_virial": round(loop_v * 1e9 / tested, 3),
                      "virial_loop_over_field_loop": round(loop_v / loop_f, 3),
                      "far_reduction_ms": round(far_v, 4), "far_torch_ms": round(far_t, 4),
                      "torch_over_far_reduction": round(far_t / far_v, 2),
                      "far_reduction_GBps": round(band_bytes / far_v * 1e-6, 1),
                      "far_torch_GBps": round(band_bytes / far_t * 1e-6, 1),
                      "far_rel_difference": float((got - want).norm() / want.norm())}))


def run(lib, n, args):
    m = 4
    r_c = min((3.0 * args.neighbours / (4.0 * math.pi * n)) ** (1.0 / 3.0), 1.0 / 3.0)
    sp = tn.EwaldSplitting.from_tolerance(args.tol, r_c)
    rng = np.random.default_rng(0)
    v = (rng.random((n, 3)) - 0.5).astype(np.float32)
    v[v >= 0.5] = -0.5  # (rounded up to the face: the same point)
    pos = torch.from_numpy(v).cuda()
    q = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    G = int(lib.nfft_hip_ewald_near_cells(r_c, 1))
    wrapped, clipped = pairs_tested(v, G)
    whole = median_ms(lambda: tn.nfft_ewald(q, pos, splitting=sp, cutoff=m), args.reps)
    whole_f = median_ms(lambda: tn.nfft_ewald(q, pos, splitting=sp, cutoff=m, field=True), args.reps)
    far = median_ms(lambda: tn.nfft_fastsum(q, sp.coeffs, pos, cutoff=m), args.reps)
    near = median_ms(lambda: tn.ops.nfft_ewald_near(pos, q, None, sp.alpha, r_c, False), args.reps)
    near_f = median_ms(lambda: tn.ops.nfft_ewald_near(pos, q, None, sp.alpha, r_c, True), args.reps)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    # the Ewald pair loop on its own
    spos, order, start = cell_order(pos, G, 0.5, G)
    xs = q.index_select(0, order).reshape(n, 1).contiguous()
    z, f = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda")
    loops = {}
    for with_field in (0, 1):
        p = _lib.EwaldProblem(cells_per_axis=G, with_field=with_field, num_points=n, num_columns=1, batch_size=1,
                              alpha=sp.alpha, r_cut=r_c)
        nbytes = lib.nfft_hip_ewald_near_workspace_bytes(ctypes.byref(p))
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def loop():
            _lib.check(lib.nfft_hip_ewald_near(ctypes.byref(p), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                               order.data_ptr(), z.data_ptr(), f.data_ptr(), ws.data_ptr(), nbytes, stream))

        loops[with_field] = median_ms(loop, args.reps)
    zo, fo = tn.ops.nfft_ewald_near(pos, q, None, sp.alpha, r_c, True)
    assert torch.equal(zo, z[:, 0]) and torch.equal(fo, f), "the restated plumbing must give the operator's bits"

    # the yardstick: the 1/r value loop of nfft_hip_nearfield on the same cells
    kern = tn.RegularizedKernel("one_over_modulus", dim=3, bandwidth=64, p=4, eps_I=r_c / 2, eps_B=1.0 / 16.0, device="cpu")
    half = pos * 0.5
    hpos, horder, hstart = cell_order(half, G, 0.25, 2 * G)
    hx = q.index_select(0, horder).reshape(n, 1).contiguous()
    hz = torch.zeros(n, 1, device="cuda")
    hq = _lib.NearfieldProblem(dim=3, kernel=kern.kernel_id, poly_terms=4, cells_per_axis=G, num_sources=n, num_targets=n,
                               num_columns=1, batch_size=1, c=kern.c, eps_I=kern.eps_I)
    for e, a in enumerate(kern.near_poly.tolist()):
        hq.poly[e] = a
    hbytes = lib.nfft_hip_nearfield_workspace_bytes(ctypes.byref(hq))
    assert hbytes > 0, _lib.last_error()
    hws = torch.empty(hbytes, dtype=torch.uint8, device="cuda")

    def yardstick():
        _lib.check(lib.nfft_hip_nearfield(ctypes.byref(hq), hpos.data_ptr(), hx.data_ptr(), hstart.data_ptr(), hpos.data_ptr(),
                                          horder.data_ptr(), hstart.data_ptr(), hz.data_ptr(), hws.data_ptr(), hbytes, stream))

    yard = median_ms(yardstick, args.reps)
    tn.ops.check_status()
    ns, ns_f, ns_y = loops[0] * 1e6 / wrapped, loops[1] * 1e6 / wrapped, yard * 1e6 / clipped
    print(json.dumps({"bench": "ewald", "points": n, "neighbours": args.neighbours, "tol": args.tol, "r_cut": round(r_c, 5),
                      "alpha": round(sp.alpha, 3), "N": sp.bandwidth, "m": m, "cells_per_axis": G,
                      "ewald_ms": round(whole, 4), "ewald_field_ms": round(whole_f, 4), "far_ms": round(far, 4),
                      "near_ms": round(near, 4), "near_field_ms": round(near_f, 4),
                      "pair_loop_ms": round(loops[0], 4), "pair_loop_field_ms": round(loops[1], 4),
                      "one_over_r_loop_ms": round(yard, 4), "pairs_tested": wrapped, "one_over_r_pairs_tested": clipped,
                      "ns_per_pair": round(ns, 5), "ns_per_pair_field": round(ns_f, 5), "one_over_r_ns_per_pair": round(ns_y, 5),
                      "value_over_one_over_r": round(ns / ns_y, 3), "field_over_one_over_r": round(ns_f / ns_y, 3)}))


def run_dispersion(lib, n, args):
    m = 4
    r_c = min((3.0 * args.neighbours / (4.0 * math.pi * n)) ** (1.0 / 3.0), 1.0 / 3.0)
    sp = tn.DispersionSplitting.from_tolerance(args.tol, r_c)
    coulomb_alpha = math.sqrt(-math.log(args.tol)) / r_c  # (EwaldSplitting.from_tolerance's)
    rng = np.random.default_rng(0)
    v = (rng.random((n, 3)) - 0.5).astype(np.float32)
    v[v >= 0.5] = -0.5  # (rounded up to the face: the same point)
    pos = torch.from_numpy(v).cuda()
    c = torch.from_numpy((rng.random(n) + 0.5).astype(np.float32)).cuda()
    G = int(lib.nfft_hip_ewald_near_cells(r_c, 1))
    wrapped, _ = pairs_tested(v, G)
    whole = median_ms(lambda: tn.nfft_ewald_dispersion(c, pos, splitting=sp, cutoff=m), args.reps)
    whole_f = median_ms(lambda: tn.nfft_ewald_dispersion(c, pos, splitting=sp, cutoff=m, field=True), args.reps)
    far = median_ms(lambda: tn.nfft_fastsum(c, sp.coeffs, pos, cutoff=m), args.reps)
    near = median_ms(lambda: tn.ops.nfft_ewald_dispersion_near(pos, c, None, sp.alpha, r_c, False), args.reps)
    near_f = median_ms(lambda: tn.ops.nfft_ewald_dispersion_near(pos, c, None, sp.alpha, r_c, True), args.reps)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    spos, order, start = cell_order(pos, G, 0.5, G)
    xs = c.index_select(0, order).reshape(n, 1).contiguous()
    z, f = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda")
    zc, fc = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda")
    loops, coulomb = {}, {}
    for with_field in (0, 1):
        p = _lib.EwaldProblem(cells_per_axis=G, with_field=with_field, num_points=n, num_columns=1, batch_size=1,
                              alpha=sp.alpha, r_cut=r_c)
        pc = _lib.EwaldProblem(cells_per_axis=G, with_field=with_field, num_points=n, num_columns=1, batch_size=1,
                               alpha=coulomb_alpha, r_cut=r_c)
        nbytes = lib.nfft_hip_ewald_near_workspace_bytes(ctypes.byref(p))
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def loop():
            _lib.check(lib.nfft_hip_ewald_dispersion_near(ctypes.byref(p), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                                          order.data_ptr(), z.data_ptr(), f.data_ptr(), ws.data_ptr(), nbytes,
                                                          stream))

        def coulomb_loop():
            _lib.check(lib.nfft_hip_ewald_near(ctypes.byref(pc), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                               order.data_ptr(), zc.data_ptr(), fc.data_ptr(), ws.data_ptr(), nbytes, stream))

        loops[with_field] = median_ms(loop, args.reps)
        coulomb[with_field] = median_ms(coulomb_loop, args.reps)
    zo, fo = tn.ops.nfft_ewald_dispersion_near(pos, c, None, sp.alpha, r_c, True)
    assert torch.equal(zo, z[:, 0]) and torch.equal(fo, f), "the restated plumbing must give the operator's bits"
    tn.ops.check_status()
    print(json.dumps({"bench": "ewald_dispersion", "points": n, "neighbours": args.neighbours, "tol": args.tol,
                      "r_cut": round(r_c, 5), "alpha": round(sp.alpha, 3), "N": sp.bandwidth, "m": m, "cells_per_axis": G,
                      "coulomb_alpha": round(coulomb_alpha, 3),
                      "dispersion_ms": round(whole, 4), "dispersion_field_ms": round(whole_f, 4), "far_ms": round(far, 4),
                      "near_ms": round(near, 4), "near_field_ms": round(near_f, 4),
                      "pair_loop_ms": round(loops[0], 4), "pair_loop_field_ms": round(loops[1], 4),
                      "coulomb_pair_loop_ms": round(coulomb[0], 4), "coulomb_pair_loop_field_ms": round(coulomb[1], 4),
                      "pairs_tested": wrapped,
                      "ps_per_pair": round(loops[0] * 1e9 / wrapped, 3), "ps_per_pair_field": round(loops[1] * 1e9 / wrapped, 3),
                      "coulomb_ps_per_pair": round(coulomb[0] * 1e9 / wrapped, 3),
                      "coulomb_ps_per_pair_field": round(coulomb[1] * 1e9 / wrapped, 3),
                      "dispersion_over_coulomb": round(loops[0] / coulomb[0], 3),
                      "dispersion_over_coulomb_field": round(loops[1] / coulomb[1], 3)}))


def run_dispersion_virial(lib, n, args):
    """the row of run_virial for the dispersion sum, in the unit cube as the identity box"""
    m = 4
    box = [1.0, 0.0, 1.0, 0.0, 0.0, 1.0]
    r_c = min((3.0 * args.neighbours / (4.0 * math.pi * n)) ** (1.0 / 3.0), 1.0 / 3.0)
    sp = tn.DispersionSplitting.from_tolerance(args.tol, r_c, box=[1.0, 1.0, 1.0])
    rng = np.random.default_rng(0)
    v = (rng.random((n, 3)) - 0.5).astype(np.float32)
    v[v >= 0.5] = -0.5  # (rounded up to the face: the same point)
    pos = torch.from_numpy(v).cuda()
    c = torch.from_numpy((rng.random(n) + 0.5).astype(np.float32)).cuda()
    G, N = sp.cells, sp.bandwidth
    tested = box_pairs_tested(v, G)
    field = median_ms(lambda: tn.nfft_ewald_dispersion(c, pos, splitting=sp, cutoff=m, field=True, fractional=True), args.reps)
    virial = median_ms(lambda: tn.nfft_ewald_dispersion_virial(c, pos, splitting=sp, cutoff=m, fractional=True), args.reps)
    adjoint = median_ms(lambda: tn.nfft_adjoint(c, pos, bandwidth=N, cutoff=m), args.reps)
    near_op = median_ms(lambda: tn.ops.nfft_ewald_dispersion_virial_near(pos, c, None, box, sp.alpha, r_c), args.reps)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    spos, order, start = box_cell_order(pos, G)
    xs = c.index_select(0, order).reshape(n, 1).contiguous()
    z, f = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda")
    p = _lib.EwaldBoxProblem(cells=(ctypes.c_int32 * 3)(*G), with_field=1, num_points=n, num_columns=1, batch_size=1,
                             alpha=sp.alpha, r_cut=r_c, box=(ctypes.c_double * 6)(*box))
    nbytes = lib.nfft_hip_ewald_near_box_workspace_bytes(ctypes.byref(p))
    vbytes = lib.nfft_hip_ewald_virial_near_workspace_bytes(ctypes.byref(p))
    assert nbytes > 0 and vbytes > 0, _lib.last_error()
    ws, vws = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(vbytes, dtype=torch.uint8, device="cuda")
    seven = torch.zeros(1, 7, 1, dtype=torch.float64, device="cuda")

    def field_loop():
        _lib.check(lib.nfft_hip_ewald_dispersion_near_box(ctypes.byref(p), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                                          order.data_ptr(), z.data_ptr(), f.data_ptr(), ws.data_ptr(), nbytes,
                                                          stream))

    def virial_loop():
        _lib.check(lib.nfft_hip_ewald_dispersion_virial_near(ctypes.byref(p), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                                             seven.data_ptr(), vws.data_ptr(), vbytes, stream))

    loop_f, loop_v = median_ms(field_loop, args.reps), median_ms(virial_loop, args.reps)
    assert torch.equal(tn.ops.nfft_ewald_dispersion_virial_near(pos, c, None, box, sp.alpha, r_c), seven[:, :, 0]), \
        "the restated plumbing must give the operator's bits"
    # the far reduction beside the torch composition on the same band
    band = tn.nfft_adjoint(c, pos, bandwidth=N, cutoff=m)  # [1, N, N, N]
    kappa = sp._kappa()
    b64, t64 = sp._b64, sp.strain_coeffs().double().cpu()
    coef7 = [b64] + [b64 + t64 * kappa[..., a] * kappa[..., a] for a in range(3)] + \
            [t64 * kappa[..., a] * kappa[..., b] for a, b in ((1, 2), (0, 2), (0, 1))]
    coef7 = (0.5 * torch.stack(coef7, 3)).to(torch.float32).cuda()  # [N, N, N, 7]
    strain = sp.strain_coeffs()
    far_v = median_ms(lambda: tn.ops.nfft_ewald_dispersion_virial_far(band, sp.coeffs, strain, box), args.reps)
    far_t = median_ms(lambda: ((band.abs() ** 2)[..., None] * coef7).sum((1, 2, 3)), args.reps)
    got = tn.ops.nfft_ewald_dispersion_virial_far(band, sp.coeffs, strain, box)
    want = ((band.abs() ** 2)[..., None] * coef7).sum((1, 2, 3)).double()
    tn.ops.check_status()
    band_bytes = band.numel() * 8
    print(json.dumps({"bench": "ewald_dispersion_virial", "box": box, "points": n, "neighbours": args.neighbours,
                      "tol": args.tol, "r_cut": round(r_c, 5), "alpha": round(sp.alpha, 3), "N": N, "m": m, "cells": list(G),
                      "dispersion_field_ms": round(field, 4), "dispersion_virial_ms": round(virial, 4),
                      "virial_over_field": round(virial / field, 3), "adjoint_ms": round(adjoint, 4),
                      "virial_near_ms": round(near_op, 4), "pair_loop_field_ms": round(loop_f, 4),
                      "pair_loop_virial_ms": round(loop_v, 4), "pairs_tested": tested,
                      "ps_per_pair_field": round(loop_f * 1e9 / tested, 3),
                      "ps_per_pair_virial": round(loop_v * 1e9 / tested, 3),
                      "virial_loop_over_field_loop": round(loop_v / loop_f, 3),
                      "far_reduction_ms": round(far_v, 4), "far_torch_ms": round(far_t, 4),
                      "torch_over_far_reduction": round(far_t / far_v, 2),
                      "far_reduction_GBps": round(band_bytes / far_v * 1e-6, 1),
                      "far_torch_GBps": round(band_bytes / far_t * 1e-6, 1),
                      "far_rel_difference": float((got - want).norm() / want.norm())}))


def alternating_ms(fns, reps):
    """{name: (median, min, max) ms} of the calls `fns` {name: fn}, timed with device events in turn -- a, b, c, a, b, c, ... --
    after two warm-up calls each, so that what else the machine does falls on all of them alike"""
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return {name: (float(np.median(t)), float(min(t)), float(max(t))) for name, t in times.items()}


def run_dipole(lib, n, args):
    """the sum of charges and point dipoles in the unit cube: the same points, r_c, alpha and N as `run`"""
    m = 4
    r_c = min((3.0 * args.neighbours / (4.0 * math.pi * n)) ** (1.0 / 3.0), 1.0 / 3.0)
    sp = tn.EwaldSplitting.from_tolerance(args.tol, r_c)
    rng = np.random.default_rng(0)
    v = (rng.random((n, 3)) - 0.5).astype(np.float32)
    v[v >= 0.5] = -0.5  # (rounded up to the face: the same point)
    pos = torch.from_numpy(v).cuda()
    q = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    mu = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).cuda()
    packed = torch.cat([q.unsqueeze(1), mu], 1).contiguous()  # [n, 4]
    G, N = int(lib.nfft_hip_ewald_near_cells(r_c, 1)), sp.bandwidth
    wrapped, _ = pairs_tested(v, G)
    whole = alternating_ms({
        "coulomb_field": lambda: tn.nfft_ewald(q, pos, splitting=sp, cutoff=m, field=True),
        "order1": lambda: tn.nfft_ewald_dipole(q, mu, pos, splitting=sp, cutoff=m),
        "order2": lambda: tn.nfft_ewald_dipole(q, mu, pos, splitting=sp, cutoff=m, gradient=True),
        "near_op1": lambda: tn.ops.nfft_ewald_dipole_near(pos, packed, None, (), sp.alpha, r_c, 1),
        "near_op2": lambda: tn.ops.nfft_ewald_dipole_near(pos, packed, None, (), sp.alpha, r_c, 2)}, args.reps)
    # the spectral step beside the torch composition on the same band
    band = tn.nfft_adjoint(packed, pos, bandwidth=N, cutoff=m)  # [1, N, N, N, 4]
    tau = 2.0 * math.pi * sp._kappa()
    row0 = sp._b64.unsqueeze(3) * torch.cat([torch.ones(N, N, N, 1, dtype=torch.complex128), 1j * tau], 3)
    rows = [row0] + [1j * tau[..., a, None] * row0 for a in range(3)] + \
           [(tau[..., a] * tau[..., b]).unsqueeze(3) * row0 for a, b in ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))]
    table = torch.stack(rows, 3).to(torch.complex64).cuda()  # [N, N, N, 10, 4]
    spectral = alternating_ms({
        "kernel": lambda: tn.ops.nfft_ewald_dipole_spectral(band, sp.coeffs, (), 2),
        "torch": lambda: torch.einsum("xyzsr,bxyzr->bxyzs", table, band)}, args.reps)
    got, want = tn.ops.nfft_ewald_dipole_spectral(band, sp.coeffs, (), 2), torch.einsum("xyzsr,bxyzr->bxyzs", table, band)
    # the pair loops on their own, on the same sorted points and cells: the Coulomb loop with its field, the dipole loops
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    spos, order, start = cell_order(pos, G, 0.5, G)
    xq = q.index_select(0, order).reshape(n, 1).contiguous()
    xp = packed.index_select(0, order).contiguous()
    z, f = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda")
    outs = {1: torch.zeros(n, 4, device="cuda"), 2: torch.zeros(n, 10, device="cuda")}
    p = _lib.EwaldProblem(cells_per_axis=G, with_field=1, num_points=n, num_columns=1, batch_size=1, alpha=sp.alpha, r_cut=r_c)
    nbytes = lib.nfft_hip_ewald_near_workspace_bytes(ctypes.byref(p))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def coulomb_loop():
        _lib.check(lib.nfft_hip_ewald_near(ctypes.byref(p), spos.data_ptr(), xq.data_ptr(), start.data_ptr(), order.data_ptr(),
                                           z.data_ptr(), f.data_ptr(), ws.data_ptr(), nbytes, stream))

    def dipole_loop(o):
        _lib.check(lib.nfft_hip_ewald_dipole_near(ctypes.byref(p), spos.data_ptr(), xp.data_ptr(), start.data_ptr(),
                                                  order.data_ptr(), o, outs[o].data_ptr(), ws.data_ptr(), nbytes, stream))

    loops = alternating_ms({"coulomb": coulomb_loop, "order1": lambda: dipole_loop(1), "order2": lambda: dipole_loop(2)}, args.reps)
    assert torch.equal(tn.ops.nfft_ewald_dipole_near(pos, packed, None, (), sp.alpha, r_c, 2), outs[2]), \
        "the restated plumbing must give the operator's bits"
    tn.ops.check_status()
    ms = lambda t: [round(e, 4) for e in t]  # noqa: E731
    print(json.dumps({"bench": "ewald_dipole", "points": n, "neighbours": args.neighbours, "tol": args.tol, "r_cut": round(r_c, 5),
                      "alpha": round(sp.alpha, 3), "N": N, "m": m, "cells_per_axis": G, "reps": args.reps,
                      "median_min_max_ms": {"whole": {k: ms(t) for k, t in whole.items()},
                                            "spectral": {k: ms(t) for k, t in spectral.items()},
                                            "pair_loop": {k: ms(t) for k, t in loops.items()}},
                      "pairs_tested": wrapped,
                      "ps_per_pair": {k: round(t[0] * 1e9 / wrapped, 3) for k, t in loops.items()},
                      "order1_over_coulomb_field_loop": round(loops["order1"][0] / loops["coulomb"][0], 3),
                      "order2_over_coulomb_field_loop": round(loops["order2"][0] / loops["coulomb"][0], 3),
                      "torch_over_spectral_kernel": round(spectral["torch"][0] / spectral["kernel"][0], 2),
                      "spectral_GBps": round((band.numel() + got.numel()) * 8 / spectral["kernel"][0] * 1e-6, 1),
                      "spectral_rel_difference": float((got - want).norm() / want.norm())}))


def run_stokeslet(lib, n, args):
    """the periodic Stokeslet sum in the unit cube: the same points, r_c, alpha and N as `run`"""
    m = 4
    r_c = min((3.0 * args.neighbours / (4.0 * math.pi * n)) ** (1.0 / 3.0), 1.0 / 3.0)
    sp = tn.EwaldSplitting.from_tolerance(args.tol, r_c)
    rng = np.random.default_rng(0)
    v = (rng.random((n, 3)) - 0.5).astype(np.float32)
    v[v >= 0.5] = -0.5  # (rounded up to the face: the same point)
    pos = torch.from_numpy(v).cuda()
    q = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    f = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).cuda()
    G, N = int(lib.nfft_hip_ewald_near_cells(r_c, 1)), sp.bandwidth
    wrapped, _ = pairs_tested(v, G)
    whole = alternating_ms({
        "coulomb_field": lambda: tn.nfft_ewald(q, pos, splitting=sp, cutoff=m, field=True),
        "u": lambda: tn.nfft_ewald_stokeslet(f, pos, splitting=sp, cutoff=m),
        "u_G": lambda: tn.nfft_ewald_stokeslet(f, pos, splitting=sp, cutoff=m, gradient=True),
        "near_op1": lambda: tn.ops.nfft_ewald_stokeslet_near(pos, f, None, (), sp.alpha, r_c, 1),
        "near_op2": lambda: tn.ops.nfft_ewald_stokeslet_near(pos, f, None, (), sp.alpha, r_c, 2)}, args.reps)
    # the spectral step beside the torch composition on the same band
    band = tn.nfft_adjoint(f, pos, bandwidth=N, cutoff=m)  # [1, N, N, N, 3]
    tau = 2.0 * math.pi * sp._kappa()
    t2 = (tau * tau).sum(3)
    P = torch.eye(3, dtype=torch.float64) - tau.unsqueeze(4) * tau.unsqueeze(3) / torch.where(t2 > 0, t2, torch.ones_like(t2))[..., None, None]
    P = (sp.stokeslet_coeffs.double().cpu()[..., None, None] * P).to(torch.complex128)  # [N, N, N, 3, 3]
    table = torch.cat([P, (-1j * P.unsqueeze(4) * tau[..., None, :, None]).reshape(N, N, N, 9, 3)], 3).to(torch.complex64).cuda()
    coeffs = sp.stokeslet_coeffs
    spectral = alternating_ms({
        "kernel": lambda: tn.ops.nfft_ewald_stokeslet_spectral(band, coeffs, (), 2),
        "torch": lambda: torch.einsum("xyzsr,bxyzr->bxyzs", table, band)}, args.reps)
    got, want = tn.ops.nfft_ewald_stokeslet_spectral(band, coeffs, (), 2), torch.einsum("xyzsr,bxyzr->bxyzs", table, band)
    # the pair loops on their own, on the same sorted points and cells: the Coulomb loop with its field, the Stokeslet loops
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    spos, order, start = cell_order(pos, G, 0.5, G)
    xq = q.index_select(0, order).reshape(n, 1).contiguous()
    xf = f.index_select(0, order).contiguous()
    z, e = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda")
    outs = {1: torch.zeros(n, 3, device="cuda"), 2: torch.zeros(n, 12, device="cuda")}
    p = _lib.EwaldProblem(cells_per_axis=G, with_field=1, num_points=n, num_columns=1, batch_size=1, alpha=sp.alpha, r_cut=r_c)
    nbytes = lib.nfft_hip_ewald_near_workspace_bytes(ctypes.byref(p))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def coulomb_loop():
        _lib.check(lib.nfft_hip_ewald_near(ctypes.byref(p), spos.data_ptr(), xq.data_ptr(), start.data_ptr(), order.data_ptr(),
                                           z.data_ptr(), e.data_ptr(), ws.data_ptr(), nbytes, stream))

    def stokeslet_loop(o):
        _lib.check(lib.nfft_hip_ewald_stokeslet_near(ctypes.byref(p), spos.data_ptr(), xf.data_ptr(), start.data_ptr(),
                                                     order.data_ptr(), o, outs[o].data_ptr(), ws.data_ptr(), nbytes, stream))

    loops = alternating_ms({"coulomb": coulomb_loop, "order1": lambda: stokeslet_loop(1), "order2": lambda: stokeslet_loop(2)},
                           args.reps)
    assert torch.equal(tn.ops.nfft_ewald_stokeslet_near(pos, f, None, (), sp.alpha, r_c, 2), outs[2]), \
        "the restated plumbing must give the operator's bits"
    tn.ops.check_status()
    ms = lambda t: [round(e, 4) for e in t]  # noqa: E731
    print(json.dumps({"bench": "ewald_stokeslet", "points": n, "neighbours": args.neighbours, "tol": args.tol, "r_cut": round(r_c, 5),
                      "alpha": round(sp.alpha, 3), "N": N, "m": m, "cells_per_axis": G, "reps": args.reps,
                      "median_min_max_ms": {"whole": {k: ms(t) for k, t in whole.items()},
                                            "spectral": {k: ms(t) for k, t in spectral.items()},
                                            "pair_loop": {k: ms(t) for k, t in loops.items()}},
                      "pairs_tested": wrapped,
                      "ps_per_pair": {k: round(t[0] * 1e9 / wrapped, 3) for k, t in loops.items()},
                      "order1_over_coulomb_field_loop": round(loops["order1"][0] / loops["coulomb"][0], 3),
                      "order2_over_coulomb_field_loop": round(loops["order2"][0] / loops["coulomb"][0], 3),
                      "torch_over_spectral_kernel": round(spectral["torch"][0] / spectral["kernel"][0], 2),
                      "spectral_GBps": round((band.numel() + got.numel()) * 8 / spectral["kernel"][0] * 1e-6, 1),
                      "spectral_rel_difference": float((got - want).norm() / want.norm())}))


def run_rpy(lib, n, args):
    """the periodic Rotne-Prager-Yamakawa sum in the unit cube: the same points, r_c, alpha and N as `run`"""
    m = 4
    r_c = min((3.0 * args.neighbours / (4.0 * math.pi * n)) ** (1.0 / 3.0), 1.0 / 3.0)
    a = min((3.0 * args.phi / (4.0 * math.pi * n)) ** (1.0 / 3.0), 0.5 * r_c)
    sp = tn.EwaldSplitting.from_tolerance(args.tol, r_c)
    rng = np.random.default_rng(0)
    v = (rng.random((n, 3)) - 0.5).astype(np.float32)
    v[v >= 0.5] = -0.5  # (rounded up to the face: the same point)
    pos = torch.from_numpy(v).cuda()
    q = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    f = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).cuda()
    G, N = int(lib.nfft_hip_ewald_near_cells(r_c, 1)), sp.bandwidth
    wrapped, _ = pairs_tested(v, G)
    tn.rpy_coeffs(sp, a)  # (built once, outside the timing)
    whole = alternating_ms({
        "coulomb_field": lambda: tn.nfft_ewald(q, pos, splitting=sp, cutoff=m, field=True),
        "stokeslet_u": lambda: tn.nfft_ewald_stokeslet(f, pos, splitting=sp, cutoff=m),
        "u": lambda: tn.nfft_ewald_rpy(f, pos, splitting=sp, radius=a, cutoff=m),
        "u_G": lambda: tn.nfft_ewald_rpy(f, pos, splitting=sp, radius=a, cutoff=m, gradient=True),
        "near_op1": lambda: tn.ops.nfft_ewald_rpy_near(pos, f, None, (), sp.alpha, r_c, a, 1),
        "near_op2": lambda: tn.ops.nfft_ewald_rpy_near(pos, f, None, (), sp.alpha, r_c, a, 2)}, args.reps)
    # the pair loops on their own, on the same sorted points and cells: the Coulomb loop with its field, the Stokeslet loops, these
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    spos, order, start = cell_order(pos, G, 0.5, G)
    xq = q.index_select(0, order).reshape(n, 1).contiguous()
    xf = f.index_select(0, order).contiguous()
    z, e = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda")
    outs = {1: torch.zeros(n, 3, device="cuda"), 2: torch.zeros(n, 12, device="cuda")}
    souts = {1: torch.zeros(n, 3, device="cuda"), 2: torch.zeros(n, 12, device="cuda")}
    p = _lib.EwaldProblem(cells_per_axis=G, with_field=1, num_points=n, num_columns=1, batch_size=1, alpha=sp.alpha, r_cut=r_c)
    nbytes = lib.nfft_hip_ewald_near_workspace_bytes(ctypes.byref(p))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def coulomb_loop():
        _lib.check(lib.nfft_hip_ewald_near(ctypes.byref(p), spos.data_ptr(), xq.data_ptr(), start.data_ptr(), order.data_ptr(),
                                           z.data_ptr(), e.data_ptr(), ws.data_ptr(), nbytes, stream))

    def stokeslet_loop(o):
        _lib.check(lib.nfft_hip_ewald_stokeslet_near(ctypes.byref(p), spos.data_ptr(), xf.data_ptr(), start.data_ptr(),
                                                     order.data_ptr(), o, souts[o].data_ptr(), ws.data_ptr(), nbytes, stream))

    def rpy_loop(o):
        _lib.check(lib.nfft_hip_ewald_rpy_near(ctypes.byref(p), spos.data_ptr(), xf.data_ptr(), start.data_ptr(), order.data_ptr(),
                                               o, a, outs[o].data_ptr(), ws.data_ptr(), nbytes, stream))

    loops = alternating_ms({"coulomb": coulomb_loop, "stokeslet1": lambda: stokeslet_loop(1), "stokeslet2": lambda: stokeslet_loop(2),
                            "order1": lambda: rpy_loop(1), "order2": lambda: rpy_loop(2)}, args.reps)
    assert torch.equal(tn.ops.nfft_ewald_rpy_near(pos, f, None, (), sp.alpha, r_c, a, 2), outs[2]), \
        "the restated plumbing must give the operator's bits"
    tn.ops.check_status()
    ms = lambda t: [round(e, 4) for e in t]  # noqa: E731
    print(json.dumps({"bench": "ewald_rpy", "points": n, "neighbours": args.neighbours, "tol": args.tol, "r_cut": round(r_c, 5),
                      "radius": round(a, 6), "phi": args.phi, "overlapping_share_of_pairs_in_cut": round((2.0 * a / r_c) ** 3, 5),
                      "alpha": round(sp.alpha, 3), "N": N, "m": m, "cells_per_axis": G, "reps": args.reps,
                      "median_min_max_ms": {"whole": {k: ms(t) for k, t in whole.items()},
                                            "pair_loop": {k: ms(t) for k, t in loops.items()}},
                      "pairs_tested": wrapped,
                      "ps_per_pair": {k: round(t[0] * 1e9 / wrapped, 3) for k, t in loops.items()},
                      "order1_over_coulomb_field_loop": round(loops["order1"][0] / loops["coulomb"][0], 3),
                      "order2_over_coulomb_field_loop": round(loops["order2"][0] / loops["coulomb"][0], 3),
                      "order1_over_stokeslet_loop": round(loops["order1"][0] / loops["stokeslet1"][0], 3),
                      "order2_over_stokeslet_loop": round(loops["order2"][0] / loops["stokeslet2"][0], 3),
                      "u_over_coulomb_field": round(whole["u"][0] / whole["coulomb_field"][0], 3),
                      "u_G_over_coulomb_field": round(whole["u_G"][0] / whole["coulomb_field"][0], 3)}))


HBM_PEAK_GBPS = 8000.0  # the MI355X's HBM3E, as specified


def run_exclusions(lib, n, args):
    """bonded-pair exclusions: n / 3 rigid triples (a water model: charges -0.834, 0.417, 0.417, the
    bond 0.3 of the molecules' mean spacing, 104.5 degrees) with their three listed pairs each, in the unit cube or in --box.
    The correction alone (the operator, and the list kernel on restated plumbing) beside the pair sweep with its field and
    beside the whole nfft_ewald(field=True) with and without the list"""
    m = 4
    n -= n % 3
    mol = n // 3
    box = args.box
    if box is not None and len(box) == 3:
        box = [box[0], 0.0, box[1], 0.0, 0.0, box[2]]
    A = np.eye(3) if box is None else np.array([[box[0], 0, 0], [box[1], box[2], 0], [box[3], box[4], box[5]]])
    V = float(np.linalg.det(A))
    r_c = (3.0 * args.neighbours * V / (4.0 * math.pi * n)) ** (1.0 / 3.0)
    if box is None:
        r_c = min(r_c, 1.0 / 3.0)
    sp = tn.EwaldSplitting.from_tolerance(args.tol, r_c, box=None if box is None else torch.from_numpy(A))
    rng = np.random.default_rng(0)
    bond = 0.3 * (V / mol) ** (1.0 / 3.0)
    centre = (rng.random((mol, 3)) - 0.5) @ A
    # a random orthonormal pair (u, v) per molecule: the two hydrogens at bond (cos, +-sin)(104.5 / 2)
    u = rng.standard_normal((mol, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(u, rng.standard_normal((mol, 3)))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    half = math.radians(104.5 / 2)
    x = np.stack([centre, centre + bond * (math.cos(half) * u + math.sin(half) * v),
                  centre + bond * (math.cos(half) * u - math.sin(half) * v)], 1).reshape(n, 3)
    s = (x @ np.linalg.inv(A)).astype(np.float32)
    q = np.tile(np.array([-0.834, 0.417, 0.417], dtype=np.float32), mol)
    o = 3 * np.arange(mol)
    pairs = np.concatenate([np.stack([o, o + 1], 1), np.stack([o, o + 2], 1), np.stack([o + 1, o + 2], 1)])
    ex = tn.ExclusionList(pairs, n)
    pos, qd = torch.from_numpy(s).cuda(), torch.from_numpy(q).cuda()
    frac = {} if box is None else {"fractional": True}
    box6 = () if box is None else sp.box6
    near = ((lambda: tn.ops.nfft_ewald_near(pos, qd, None, sp.alpha, r_c, True)) if box is None else
            (lambda: tn.ops.nfft_ewald_near_box(pos, qd, None, box6, sp.alpha, r_c, True)))
    # the list kernel alone, on restated plumbing: reduced positions, one real column
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    red = pos - pos.round()
    red = torch.where(red >= 0.5, red - 1.0, red).contiguous()
    xr = qd.reshape(n, 1).contiguous()
    z, e = torch.empty(n, 1, device="cuda"), torch.empty(n, 3, device="cuda")
    p = _lib.EwaldExclProblem(kind=_lib.EXCL_COULOMB, with_field=1, num_points=n, num_columns=1, num_entries=ex.col.numel(),
                              batch_size=1, alpha=sp.alpha,
                              box=(ctypes.c_double * 6)(*(box if box is not None else (1.0, 0.0, 1.0, 0.0, 0.0, 1.0))))
    entry = lib.nfft_hip_ewald_excl if box is None else lib.nfft_hip_ewald_excl_box

    def kernel():
        _lib.check(entry(ctypes.byref(p), red.data_ptr(), xr.data_ptr(), ex.row_start.data_ptr(), ex.col.data_ptr(),
                         ex.coulomb_weight.data_ptr(), z.data_ptr(), e.data_ptr(), stream))

    def operator():
        return tn.ops.nfft_ewald_excl(pos, qd, None, ex.row_start, ex.col, ex.coulomb_weight, box6, sp.alpha, 0, True)

    t = alternating_ms({
        "list_kernel": kernel,
        "correction_op": operator,
        "pair_sweep_field": near,
        "whole_field": lambda: tn.nfft_ewald(qd, pos, splitting=sp, cutoff=m, field=True, **frac),
        "whole_field_with_list": lambda: tn.nfft_ewald(qd, pos, splitting=sp, cutoff=m, field=True, exclusions=ex, **frac)}, args.reps)
    zo, fo = operator()
    assert torch.equal(zo, z.reshape(n)) and torch.equal(fo, e), "the restated plumbing must give the operator's bits"
    tn.ops.check_status()
    entries = ex.col.numel()
    # what the list kernel must move: the CSR arrays, each lane's own position, one gathered position and one gathered value per
    # entry, the value and the three field components out
    nbytes = 4 * (n + 1) + 8 * entries + 12 * n + 12 * entries + 4 * entries + 16 * n
    ms = lambda v: [round(a, 4) for a in v]  # noqa: E731
    gbps = nbytes / t["list_kernel"][0] * 1e-6
    print(json.dumps({"bench": "ewald_exclusions", "points": n, "molecules": mol, "listed_pairs": int(pairs.shape[0]),
                      "box": box, "bond": round(bond, 6), "neighbours": args.neighbours, "tol": args.tol, "r_cut": round(r_c, 5),
                      "alpha": round(sp.alpha, 3), "N": sp.bandwidth, "m": m, "reps": args.reps,
                      "median_min_max_ms": {k: ms(v) for k, v in t.items()},
                      "list_kernel_bytes": nbytes, "list_kernel_GBps": round(gbps, 1),
                      "fraction_of_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4),
                      "list_kernel_over_pair_sweep": round(t["list_kernel"][0] / t["pair_sweep_field"][0], 4),
                      "correction_op_over_whole": round(t["correction_op"][0] / t["whole_field"][0], 4),
                      "with_list_over_without": round(t["whole_field_with_list"][0] / t["whole_field"][0], 4)}))


def run_yukawa(lib, n, args):
    """the screened Coulomb sum in the unit cube: the same points, r_c, alpha and N as `run`, lambda =
    args.screening / r_c; with --virial its virial tensor in the identity box as well"""
    m = 4
    r_c = min((3.0 * args.neighbours / (4.0 * math.pi * n)) ** (1.0 / 3.0), 1.0 / 3.0)
    lam = args.screening / r_c
    sp = tn.YukawaSplitting.from_tolerance(args.tol, r_c, lam)
    ew = tn.EwaldSplitting.from_tolerance(args.tol, r_c)
    rng = np.random.default_rng(0)
    v = (rng.random((n, 3)) - 0.5).astype(np.float32)
    v[v >= 0.5] = -0.5  # (rounded up to the face: the same point)
    pos = torch.from_numpy(v).cuda()
    q = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    G, N = int(lib.nfft_hip_ewald_near_cells(r_c, 1)), sp.bandwidth
    wrapped, _ = pairs_tested(v, G)
    whole = alternating_ms({
        "coulomb": lambda: tn.nfft_ewald(q, pos, splitting=ew, cutoff=m),
        "coulomb_field": lambda: tn.nfft_ewald(q, pos, splitting=ew, cutoff=m, field=True),
        "yukawa": lambda: tn.nfft_ewald_yukawa(q, pos, splitting=sp, cutoff=m),
        "yukawa_field": lambda: tn.nfft_ewald_yukawa(q, pos, splitting=sp, cutoff=m, field=True),
        "near_op": lambda: tn.ops.nfft_ewald_yukawa_near(pos, q, None, (), sp.alpha, r_c, lam, False),
        "near_op_field": lambda: tn.ops.nfft_ewald_yukawa_near(pos, q, None, (), sp.alpha, r_c, lam, True)}, args.reps)
    # the pair loops on their own, on the same sorted points and cells: the same pairs are tested and the same pass the cut
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    spos, order, start = cell_order(pos, G, 0.5, G)
    xs = q.index_select(0, order).reshape(n, 1).contiguous()
    z, f = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda")
    zc, fc = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda")
    ps = {w: _lib.EwaldProblem(cells_per_axis=G, with_field=w, num_points=n, num_columns=1, batch_size=1, alpha=sp.alpha, r_cut=r_c)
          for w in (0, 1)}
    nbytes = lib.nfft_hip_ewald_near_workspace_bytes(ctypes.byref(ps[1]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def yukawa_loop(w):
        _lib.check(lib.nfft_hip_ewald_yukawa_near(ctypes.byref(ps[w]), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                                  order.data_ptr(), lam, z.data_ptr(), f.data_ptr(), ws.data_ptr(), nbytes, stream))

    def coulomb_loop(w):
        _lib.check(lib.nfft_hip_ewald_near(ctypes.byref(ps[w]), spos.data_ptr(), xs.data_ptr(), start.data_ptr(), order.data_ptr(),
                                           zc.data_ptr(), fc.data_ptr(), ws.data_ptr(), nbytes, stream))

    loops = alternating_ms({"coulomb": lambda: coulomb_loop(0), "coulomb_field": lambda: coulomb_loop(1),
                            "yukawa": lambda: yukawa_loop(0), "yukawa_field": lambda: yukawa_loop(1)}, args.reps)
    zo, fo = tn.ops.nfft_ewald_yukawa_near(pos, q, None, (), sp.alpha, r_c, lam, True)
    assert torch.equal(zo, z[:, 0]) and torch.equal(fo, f), "the restated plumbing must give the operator's bits"
    tn.ops.check_status()
    ms = lambda t: [round(e, 4) for e in t]  # noqa: E731
    print(json.dumps({"bench": "ewald_yukawa", "points": n, "neighbours": args.neighbours, "tol": args.tol, "r_cut": round(r_c, 5),
                      "alpha": round(sp.alpha, 3), "N": N, "m": m, "cells_per_axis": G, "screening": round(lam, 4),
                      "screening_r_cut": args.screening, "reps": args.reps,
                      "median_min_max_ms": {"whole": {k: ms(t) for k, t in whole.items()},
                                            "pair_loop": {k: ms(t) for k, t in loops.items()}},
                      "pairs_tested": wrapped,
                      "ps_per_pair": {k: round(t[0] * 1e9 / wrapped, 3) for k, t in loops.items()},
                      "yukawa_over_coulomb_loop": round(loops["yukawa"][0] / loops["coulomb"][0], 3),
                      "yukawa_over_coulomb_field_loop": round(loops["yukawa_field"][0] / loops["coulomb_field"][0], 3),
                      "yukawa_over_coulomb_whole": round(whole["yukawa"][0] / whole["coulomb"][0], 3),
                      "yukawa_over_coulomb_whole_field": round(whole["yukawa_field"][0] / whole["coulomb_field"][0], 3)}))
    if not args.virial:
        return
    box = [1.0, 0.0, 1.0, 0.0, 0.0, 1.0]
    spb = tn.YukawaSplitting.from_tolerance(args.tol, r_c, lam, box=[1.0, 1.0, 1.0])
    Gb = spb.cells
    spos, order, start = box_cell_order(pos, Gb)
    xs = q.index_select(0, order).reshape(n, 1).contiguous()
    pb = _lib.EwaldBoxProblem(cells=(ctypes.c_int32 * 3)(*Gb), with_field=1, num_points=n, num_columns=1, batch_size=1,
                              alpha=spb.alpha, r_cut=r_c, box=(ctypes.c_double * 6)(*box))
    nbytes = lib.nfft_hip_ewald_near_box_workspace_bytes(ctypes.byref(pb))
    vbytes = lib.nfft_hip_ewald_virial_near_workspace_bytes(ctypes.byref(pb))
    assert nbytes > 0 and vbytes > 0, _lib.last_error()
    ws, vws = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(vbytes, dtype=torch.uint8, device="cuda")
    seven = torch.zeros(1, 7, 1, dtype=torch.float64, device="cuda")

    def field_loop():
        _lib.check(lib.nfft_hip_ewald_yukawa_near_box(ctypes.byref(pb), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                                      order.data_ptr(), lam, z.data_ptr(), f.data_ptr(), ws.data_ptr(), nbytes,
                                                      stream))

    def virial_loop():
        _lib.check(lib.nfft_hip_ewald_yukawa_virial_near(ctypes.byref(pb), spos.data_ptr(), xs.data_ptr(), start.data_ptr(), lam,
                                                         seven.data_ptr(), vws.data_ptr(), vbytes, stream))

    def coulomb_virial_loop():
        _lib.check(lib.nfft_hip_ewald_virial_near(ctypes.byref(pb), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                                  seven.data_ptr(), vws.data_ptr(), vbytes, stream))

    t = alternating_ms({
        "yukawa_field": lambda: tn.nfft_ewald_yukawa(q, pos, splitting=spb, cutoff=m, field=True, fractional=True),
        "yukawa_virial": lambda: tn.nfft_ewald_yukawa_virial(q, pos, splitting=spb, cutoff=m, fractional=True),
        "field_loop": field_loop, "coulomb_virial_loop": coulomb_virial_loop, "virial_loop": virial_loop}, args.reps)
    assert torch.equal(tn.ops.nfft_ewald_yukawa_virial_near(pos, q, None, box, spb.alpha, r_c, lam), seven[:, :, 0]), \
        "the restated plumbing must give the operator's bits"
    tn.ops.check_status()
    tested = box_pairs_tested(v, Gb)
    print(json.dumps({"bench": "ewald_yukawa_virial", "box": box, "points": n, "neighbours": args.neighbours, "tol": args.tol,
                      "r_cut": round(r_c, 5), "alpha": round(spb.alpha, 3), "N": spb.bandwidth, "m": m, "cells": list(Gb),
                      "screening": round(lam, 4), "reps": args.reps,
                      "median_min_max_ms": {k: ms(e) for k, e in t.items()}, "pairs_tested": tested,
                      "ps_per_pair_field": round(t["field_loop"][0] * 1e9 / tested, 3),
                      "ps_per_pair_virial": round(t["virial_loop"][0] * 1e9 / tested, 3),
                      "virial_over_field": round(t["yukawa_virial"][0] / t["yukawa_field"][0], 3),
                      "virial_loop_over_field_loop": round(t["virial_loop"][0] / t["field_loop"][0], 3),
                      "virial_loop_over_coulomb_virial_loop": round(t["virial_loop"][0] / t["coulomb_virial_loop"][0], 3)}))


def run_step(lib, n, args):
    """the fused step beside the two calls, the two pair loops and the two spectral passes that it replaces"""
    m = 4
    box = [1.0, 0.0, 1.0, 0.0, 0.0, 1.0] if args.box is None else \
        (args.box if len(args.box) == 6 else [args.box[0], 0.0, args.box[1], 0.0, 0.0, args.box[2]])
    A = [[box[0], 0.0, 0.0], [box[1], box[2], 0.0], [box[3], box[4], box[5]]]
    probe = tn.EwaldSplitting(1.0, 1e-3 * min(box[0], box[2], box[5]), 2, box=A, device="cpu")  # (volume and widths)
    r_c = min((3.0 * args.neighbours * probe.volume / (4.0 * math.pi * n)) ** (1.0 / 3.0), min(probe.widths) / 3.0)
    sp = tn.EwaldSplitting.from_tolerance(args.tol, r_c, box=A)
    rng = np.random.default_rng(0)
    v = (rng.random((n, 3)) - 0.5).astype(np.float32)
    v[v >= 0.5] = -0.5  # (rounded up to the face: the same point)
    pos = torch.from_numpy(v).cuda()
    q = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    G, N = sp.cells, sp.bandwidth
    tested = box_pairs_tested(v, G)
    kw = {"splitting": sp, "cutoff": m, "fractional": True}
    if args.exclusions:
        even = 2 * np.arange(n // 2)
        kw["exclusions"] = tn.ExclusionList(np.stack([even, even + 1], 1), n)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    spos, order, start = box_cell_order(pos, G)
    xs = q.index_select(0, order).reshape(n, 1).contiguous()
    z, f = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda")
    zs, fs = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda")
    p = _lib.EwaldBoxProblem(cells=(ctypes.c_int32 * 3)(*G), with_field=1, num_points=n, num_columns=1, batch_size=1,
                             alpha=sp.alpha, r_cut=r_c, box=(ctypes.c_double * 6)(*box))
    nbytes = lib.nfft_hip_ewald_near_box_workspace_bytes(ctypes.byref(p))
    vbytes = lib.nfft_hip_ewald_virial_near_workspace_bytes(ctypes.byref(p))
    sbytes = lib.nfft_hip_ewald_step_near_workspace_bytes(ctypes.byref(p))
    assert nbytes > 0 and vbytes > 0 and sbytes > 0, _lib.last_error()
    ws, vws, sws = (torch.empty(b, dtype=torch.uint8, device="cuda") for b in (nbytes, vbytes, sbytes))
    seven, seven_s = (torch.zeros(1, 7, 1, dtype=torch.float64, device="cuda") for _ in range(2))

    def field_loop():
        _lib.check(lib.nfft_hip_ewald_near_box(ctypes.byref(p), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                               order.data_ptr(), z.data_ptr(), f.data_ptr(), ws.data_ptr(), nbytes, stream))

    def virial_loop():
        _lib.check(lib.nfft_hip_ewald_virial_near(ctypes.byref(p), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                                  seven.data_ptr(), vws.data_ptr(), vbytes, stream))

    def step_loop():
        _lib.check(lib.nfft_hip_ewald_step_near(ctypes.byref(p), spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                                order.data_ptr(), zs.data_ptr(), fs.data_ptr(), seven_s.data_ptr(),
                                                sws.data_ptr(), sbytes, stream))

    band = tn.nfft_adjoint(q, pos, bandwidth=N, cutoff=m)  # [1, N, N, N]
    fc = sp.field_coeffs().reshape(1, N, N, N, 4)
    t = alternating_ms({
        "ewald_field": lambda: tn.nfft_ewald(q, pos, field=True, **kw),
        "ewald_virial": lambda: tn.nfft_ewald_virial(q, pos, **kw),
        "ewald_step": lambda: tn.nfft_ewald_step(q, pos, **kw),
        "pair_loop_field": field_loop, "pair_loop_virial": virial_loop, "pair_loop_step": step_loop,
        "spectral_product": lambda: band.unsqueeze(4) * fc,
        "spectral_virial_far": lambda: tn.ops.nfft_ewald_virial_far(band, sp.coeffs, box, sp.alpha),
        "spectral_step": lambda: tn.ops.nfft_ewald_step_spectral(band, sp.coeffs, box, sp.alpha)}, args.reps)
    zo, fo, so = tn.ops.nfft_ewald_step_near(pos, q, None, box, sp.alpha, r_c)
    assert torch.equal(zo, zs[:, 0]) and torch.equal(fo, fs) and torch.equal(so, seven_s[:, :, 0]), \
        "the restated plumbing must give the operator's bits"
    spectra, far7 = tn.ops.nfft_ewald_step_spectral(band, sp.coeffs, box, sp.alpha)
    want = band.unsqueeze(4) * fc
    tn.ops.check_status()
    ms = lambda v: [round(a, 4) for a in v]  # noqa: E731
    med = {k: v[0] for k, v in t.items()}
    two_calls = med["ewald_field"] + med["ewald_virial"]
    two_loops = med["pair_loop_field"] + med["pair_loop_virial"]
    two_passes = med["spectral_product"] + med["spectral_virial_far"]
    print(json.dumps({"bench": "ewald_step", "box": box, "points": n, "neighbours": args.neighbours, "tol": args.tol,
                      "r_cut": round(r_c, 5), "alpha": round(sp.alpha, 3), "N": N, "m": m, "cells": list(G), "reps": args.reps,
                      "exclusions": bool(args.exclusions), "median_min_max_ms": {k: ms(v) for k, v in t.items()},
                      "field_plus_virial_ms": round(two_calls, 4), "step_over_field_plus_virial": round(med["ewald_step"] / two_calls, 3),
                      "step_over_field": round(med["ewald_step"] / med["ewald_field"], 3),
                      # (the two calls at their slowest against the step at its fastest, and the other way round)
                      "ratio_range": [round(t["ewald_step"][1] / (t["ewald_field"][2] + t["ewald_virial"][2]), 3),
                                      round(t["ewald_step"][2] / (t["ewald_field"][1] + t["ewald_virial"][1]), 3)],
                      "pairs_tested": tested,
                      "ps_per_pair": {k[10:]: round(med[k] * 1e9 / tested, 3) for k in med if k.startswith("pair_loop_")},
                      "two_pair_loops_ms": round(two_loops, 4), "step_loop_over_two_loops": round(med["pair_loop_step"] / two_loops, 3),
                      "step_loop_over_field_loop": round(med["pair_loop_step"] / med["pair_loop_field"], 3),
                      "two_spectral_passes_ms": round(two_passes, 4),
                      "step_spectral_over_two_passes": round(med["spectral_step"] / two_passes, 3),
                      "step_spectral_GBps": round(band.numel() * 8 * 5 / med["spectral_step"] * 1e-6, 1),  # (one read, four writes)
                      "same_bits_as_the_two_loops": bool(torch.equal(zs, z) and torch.equal(fs, f) and torch.equal(seven_s, seven)),
                      "same_bits_as_virial_far": bool(torch.equal(far7, tn.ops.nfft_ewald_virial_far(band, sp.coeffs, box, sp.alpha))),
                      "spectra_rel_difference": float((spectra - want).norm() / want.norm())}))


def fft_friendly(N):
    """the first even size >= N whose prime factors are 2, 3, 5 and 7"""
    N += N % 2
    while True:
        m = N
        for p in (2, 3, 5, 7):
            while m % p == 0:
                m //= p
        if m == 1:
            return N
        N += 2


def run_lj_step(lib, n, args):
    """the Lennard-Jones + Coulomb step beside the three calls, the three pair loops and the three
    spectral passes that it replaces, on a jittered lattice (r^-12 forbids uniform points).  The three calls get the
    splittings that from_tolerance gives each sum; the step needs one bandwidth for both and takes the larger.  Every
    bandwidth is raised to the next size with small prime factors (from_tolerance may return one like 278 = 2 x 139, at which
    the FFT of every call runs many times slower); --bandwidth-as-is keeps what from_tolerance returns."""
    m = 4
    box = [1.0, 0.0, 1.0, 0.0, 0.0, 1.0] if args.box is None else \
        (args.box if len(args.box) == 6 else [args.box[0], 0.0, args.box[1], 0.0, 0.0, args.box[2]])
    A = [[box[0], 0.0, 0.0], [box[1], box[2], 0.0], [box[3], box[4], box[5]]]
    probe = tn.EwaldSplitting(1.0, 1e-3 * min(box[0], box[2], box[5]), 2, box=A, device="cpu")  # (volume and widths)
    r_c = min((3.0 * args.neighbours * probe.volume / (4.0 * math.pi * n)) ** (1.0 / 3.0), min(probe.widths) / 3.0)
    own_c = tn.EwaldSplitting.from_tolerance(args.tol, r_c, box=A)
    own_d = tn.DispersionSplitting.from_tolerance(args.tol, r_c, box=A)
    if not args.bandwidth_as_is:
        own_c = tn.EwaldSplitting(own_c.alpha, r_c, fft_friendly(own_c.bandwidth), box=A)
        own_d = tn.DispersionSplitting(own_d.alpha, r_c, fft_friendly(own_d.bandwidth), box=A)
    N = max(own_c.bandwidth, own_d.bandwidth)
    spc = tn.EwaldSplitting(own_c.alpha, r_c, N, box=A)
    spd = tn.DispersionSplitting(own_d.alpha, r_c, N, box=A)
    rng = np.random.default_rng(0)
    side = int(math.ceil(n ** (1.0 / 3.0)))
    g = (np.arange(side) + 0.5) / side - 0.5
    v = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    v = (v + (rng.random(v.shape) - 0.5) * (0.4 / side))[rng.permutation(side ** 3)[:n]].astype(np.float32)
    v[v >= 0.5] = -0.5  # (rounded up to the face: the same point)
    pos = torch.from_numpy(v).cuda()
    sigma = 0.8 * probe.volume ** (1.0 / 3.0) / side * (0.95 + 0.1 * rng.random(n))
    cc, aa = tn.lj_coefficients(torch.from_numpy(sigma), torch.from_numpy(0.5 + rng.random(n)))
    q = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    c, a = cc.float().cuda(), aa.float().cuda()
    G = spc.cells
    assert spd.cells == G
    tested = box_pairs_tested(v, G)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    spos, order, start = box_cell_order(pos, G)
    qs, cs = (t.index_select(0, order).reshape(n, 1).contiguous() for t in (q, c))
    xs = torch.stack([q, c, a], 1).index_select(0, order).contiguous()
    z, f, fl = torch.zeros(n, 1, device="cuda"), torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
    pc, pd = (_lib.EwaldBoxProblem(cells=(ctypes.c_int32 * 3)(*G), with_field=1, num_points=n, num_columns=1, batch_size=1,
                                   alpha=alpha, r_cut=r_c, box=(ctypes.c_double * 6)(*box)) for alpha in (spc.alpha, spd.alpha))
    sizes = [lib.nfft_hip_ewald_step_near_workspace_bytes(ctypes.byref(pc)), lib.nfft_hip_ewald_near_box_workspace_bytes(ctypes.byref(pd)),
             lib.nfft_hip_ewald_virial_near_workspace_bytes(ctypes.byref(pd)),
             lib.nfft_hip_ewald_lj_step_near_workspace_bytes(ctypes.byref(pc), spd.alpha)]
    assert min(sizes) > 0, _lib.last_error()
    wss = [torch.empty(b, dtype=torch.uint8, device="cuda") for b in sizes]
    seven_c, seven_d = (torch.zeros(1, 7, 1, dtype=torch.float64, device="cuda") for _ in range(2))
    eight = torch.zeros(1, 8, dtype=torch.float64, device="cuda")

    def coulomb_step_loop():
        _lib.check(lib.nfft_hip_ewald_step_near(ctypes.byref(pc), spos.data_ptr(), qs.data_ptr(), start.data_ptr(), order.data_ptr(),
                                                z.data_ptr(), f.data_ptr(), seven_c.data_ptr(), wss[0].data_ptr(), sizes[0], stream))

    def dispersion_field_loop():
        _lib.check(lib.nfft_hip_ewald_dispersion_near_box(ctypes.byref(pd), spos.data_ptr(), cs.data_ptr(), start.data_ptr(),
                                                          order.data_ptr(), z.data_ptr(), f.data_ptr(), wss[1].data_ptr(), sizes[1], stream))

    def dispersion_virial_loop():
        _lib.check(lib.nfft_hip_ewald_dispersion_virial_near(ctypes.byref(pd), spos.data_ptr(), cs.data_ptr(), start.data_ptr(),
                                                             seven_d.data_ptr(), wss[2].data_ptr(), sizes[2], stream))

    def lj_loop():
        _lib.check(lib.nfft_hip_ewald_lj_step_near(ctypes.byref(pc), spd.alpha, spos.data_ptr(), xs.data_ptr(), start.data_ptr(),
                                                   order.data_ptr(), fl.data_ptr(), eight.data_ptr(), wss[3].data_ptr(), sizes[3], stream))

    band = tn.nfft_adjoint(torch.stack([q, c], 1), pos, bandwidth=N, cutoff=m)  # [1, N, N, N, 2]
    bq, bc = band[..., 0].contiguous(), band[..., 1].contiguous()
    fd = spd.field_coeffs().reshape(1, N, N, N, 4)
    kc, kd = ({"splitting": sp, "cutoff": m, "fractional": True} for sp in (own_c, own_d))
    kl = {"coulomb": spc, "dispersion": spd, "cutoff": m, "fractional": True}
    t = alternating_ms({
        "ewald_step": lambda: tn.nfft_ewald_step(q, pos, **kc),
        "dispersion_field": lambda: tn.nfft_ewald_dispersion(c, pos, field=True, **kd),
        "dispersion_virial": lambda: tn.nfft_ewald_dispersion_virial(c, pos, **kd),
        "lj_step": lambda: tn.nfft_ewald_lj_step(q, c, a, pos, **kl),
        "pair_loop_coulomb_step": coulomb_step_loop, "pair_loop_dispersion_field": dispersion_field_loop,
        "pair_loop_dispersion_virial": dispersion_virial_loop, "pair_loop_lj_step": lj_loop,
        "spectral_coulomb_step": lambda: tn.ops.nfft_ewald_step_spectral(bq, spc.coeffs, box, spc.alpha),
        "spectral_dispersion_product": lambda: bc.unsqueeze(4) * fd,
        "spectral_dispersion_virial_far": lambda: tn.ops.nfft_ewald_dispersion_virial_far(bc, spd.coeffs, spd.strain_coeffs(), box),
        "spectral_lj_step": lambda: tn.ops.nfft_ewald_lj_step_spectral(band, spc.coeffs, spd.coeffs, spd.strain_coeffs(), box, spc.alpha)},
        args.reps)
    fo, eo = tn.ops.nfft_ewald_lj_step_near(pos, torch.stack([q, c, a], 1), None, box, spc.alpha, spd.alpha, r_c)
    assert torch.equal(fo, fl) and torch.equal(eo, eight), "the restated plumbing must give the operator's bits"
    tn.ops.check_status()
    ms = lambda v: [round(e, 4) for e in v]  # noqa: E731
    med = {k: v[0] for k, v in t.items()}
    old = ("ewald_step", "dispersion_field", "dispersion_virial")
    loops = ("pair_loop_coulomb_step", "pair_loop_dispersion_field", "pair_loop_dispersion_virial")
    passes = ("spectral_coulomb_step", "spectral_dispersion_product", "spectral_dispersion_virial_far")
    three = sum(med[k] for k in old)
    print(json.dumps({"bench": "ewald_lj_step", "box": box, "points": n, "neighbours": args.neighbours, "tol": args.tol,
                      "r_cut": round(r_c, 5), "alpha_coulomb": round(spc.alpha, 3), "alpha_dispersion": round(spd.alpha, 3), "N": N,
                      "N_of_the_three_calls": [own_c.bandwidth, own_d.bandwidth], "m": m, "cells": list(G), "reps": args.reps,
                      "median_min_max_ms": {k: ms(v) for k, v in t.items()},
                      "three_calls_ms": round(three, 4), "lj_step_over_three_calls": round(med["lj_step"] / three, 3),
                      # (the three calls at their slowest against the step at its fastest, and the other way round)
                      "ratio_range": [round(t["lj_step"][1] / sum(t[k][2] for k in old), 3),
                                      round(t["lj_step"][2] / sum(t[k][1] for k in old), 3)],
                      "pairs_tested": tested,
                      "ps_per_pair": {k[10:]: round(med[k] * 1e9 / tested, 3) for k in med if k.startswith("pair_loop_")},
                      "three_pair_loops_ms": round(sum(med[k] for k in loops), 4),
                      "lj_loop_over_three_loops": round(med["pair_loop_lj_step"] / sum(med[k] for k in loops), 3),
                      "lj_loop_ratio_range": [round(t["pair_loop_lj_step"][1] / sum(t[k][2] for k in loops), 3),
                                              round(t["pair_loop_lj_step"][2] / sum(t[k][1] for k in loops), 3)],
                      "three_spectral_passes_ms": round(sum(med[k] for k in passes), 4),
                      "lj_spectral_over_three_passes": round(med["spectral_lj_step"] / sum(med[k] for k in passes), 3),
                      "lj_spectral_ratio_range": [round(t["spectral_lj_step"][1] / sum(t[k][2] for k in passes), 3),
                                                  round(t["spectral_lj_step"][2] / sum(t[k][1] for k in passes), 3)],
                      "lj_spectral_GBps": round(N ** 3 * (16 + 48 + 12) / med["spectral_lj_step"] * 1e-6, 1)}))


def run_lj_excl_step(lib, n, args):
    """the Lennard-Jones + Coulomb step with bonded-pair exclusions on rigid triples: the water model
    of run_exclusions on the jittered lattice of run_lj_step (one molecule per site), its three pairs per molecule listed at
    scale 0.  Splittings and bandwidths as run_lj_step chooses them."""
    m = 4
    n -= n % 3
    mol = n // 3
    box = [1.0, 0.0, 1.0, 0.0, 0.0, 1.0] if args.box is None else \
        (args.box if len(args.box) == 6 else [args.box[0], 0.0, args.box[1], 0.0, 0.0, args.box[2]])
    A = np.array([[box[0], 0.0, 0.0], [box[1], box[2], 0.0], [box[3], box[4], box[5]]])
    probe = tn.EwaldSplitting(1.0, 1e-3 * min(box[0], box[2], box[5]), 2, box=A, device="cpu")  # (volume and widths)
    r_c = min((3.0 * args.neighbours * probe.volume / (4.0 * math.pi * n)) ** (1.0 / 3.0), min(probe.widths) / 3.0)
    own_c = tn.EwaldSplitting.from_tolerance(args.tol, r_c, box=A)
    own_d = tn.DispersionSplitting.from_tolerance(args.tol, r_c, box=A)
    if not args.bandwidth_as_is:
        own_c = tn.EwaldSplitting(own_c.alpha, r_c, fft_friendly(own_c.bandwidth), box=A)
        own_d = tn.DispersionSplitting(own_d.alpha, r_c, fft_friendly(own_d.bandwidth), box=A)
    N = max(own_c.bandwidth, own_d.bandwidth)
    spc = tn.EwaldSplitting(own_c.alpha, r_c, N, box=A)
    spd = tn.DispersionSplitting(own_d.alpha, r_c, N, box=A)
    rng = np.random.default_rng(0)
    side = int(math.ceil(mol ** (1.0 / 3.0)))
    g = (np.arange(side) + 0.5) / side - 0.5
    centre = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    centre = (centre + (rng.random(centre.shape) - 0.5) * (0.2 / side))[rng.permutation(side ** 3)[:mol]] @ A
    spacing = probe.volume ** (1.0 / 3.0) / side
    bond = 0.3 * spacing
    u = rng.standard_normal((mol, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(u, rng.standard_normal((mol, 3)))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    half = math.radians(104.5 / 2)
    x = np.stack([centre, centre + bond * (math.cos(half) * u + math.sin(half) * v),
                  centre + bond * (math.cos(half) * u - math.sin(half) * v)], 1).reshape(n, 3)
    pos = torch.from_numpy((x @ np.linalg.inv(A)).astype(np.float32)).cuda()
    q = torch.from_numpy(np.tile(np.array([-0.834, 0.417, 0.417], dtype=np.float32), mol)).cuda()
    sigma = np.zeros(n)
    sigma[0::3] = 0.8 * spacing  # (the hydrogens carry no Lennard-Jones term, as in TIP3P)
    cc, aa = tn.lj_coefficients(torch.from_numpy(sigma), torch.ones(n, dtype=torch.float64))
    c, a = cc.float().cuda(), aa.float().cuda()
    o = 3 * np.arange(mol)
    ex = tn.ExclusionList(np.concatenate([np.stack([o, o + 1], 1), np.stack([o, o + 2], 1), np.stack([o + 1, o + 2], 1)]), n)
    lists = (ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight)
    xs = torch.stack([q, c, a], 1)
    kc, kd = ({"splitting": sp, "cutoff": m, "fractional": True, "exclusions": ex} for sp in (own_c, own_d))
    kl = {"coulomb": spc, "dispersion": spd, "cutoff": m, "fractional": True}
    walk = (box, spc.alpha, spd.alpha, r_c)
    t = alternating_ms({
        "lj_excl_step": lambda: tn.nfft_ewald_lj_excl_step(q, c, a, pos, exclusions=ex, **kl),
        "lj_step": lambda: tn.nfft_ewald_lj_step(q, c, a, pos, **kl),
        "ewald_step": lambda: tn.nfft_ewald_step(q, pos, **kc),
        "dispersion_field": lambda: tn.nfft_ewald_dispersion(c, pos, field=True, **kd),
        "dispersion_virial": lambda: tn.nfft_ewald_dispersion_virial(c, pos, **kd),
        "masked_walk_op": lambda: tn.ops.nfft_ewald_lj_excl_near(pos, xs, None, *lists, *walk),
        "unmasked_walk_op": lambda: tn.ops.nfft_ewald_lj_step_near(pos, xs, None, *walk),
        "list_kernel_op": lambda: tn.ops.nfft_ewald_lj_excl_list(pos, xs, None, *lists, *walk)},
        args.reps)
    tn.ops.check_status()
    ms = lambda v_: [round(e, 4) for e in v_]  # noqa: E731
    med = {k: v_[0] for k, v_ in t.items()}
    old = ("ewald_step", "dispersion_field", "dispersion_virial")
    three = sum(med[k] for k in old)
    print(json.dumps({"bench": "ewald_lj_excl_step", "box": box, "points": n, "listed_pairs": len(ex), "neighbours": args.neighbours,
                      "tol": args.tol, "r_cut": round(r_c, 5), "alpha_coulomb": round(spc.alpha, 3),
                      "alpha_dispersion": round(spd.alpha, 3), "N": N, "N_of_the_three_calls": [own_c.bandwidth, own_d.bandwidth],
                      "m": m, "cells": list(spc.cells), "reps": args.reps, "median_min_max_ms": {k: ms(v_) for k, v_ in t.items()},
                      "lj_excl_step_over_lj_step": round(med["lj_excl_step"] / med["lj_step"], 3),
                      "lj_excl_step_over_lj_step_range": [round(t["lj_excl_step"][1] / t["lj_step"][2], 3),
                                                          round(t["lj_excl_step"][2] / t["lj_step"][1], 3)],
                      "three_calls_with_exclusions_ms": round(three, 4),
                      "lj_excl_step_over_three_calls": round(med["lj_excl_step"] / three, 3),
                      "ratio_range": [round(t["lj_excl_step"][1] / sum(t[k][2] for k in old), 3),
                                      round(t["lj_excl_step"][2] / sum(t[k][1] for k in old), 3)],
                      "masked_over_unmasked_walk_op": round(med["masked_walk_op"] / med["unmasked_walk_op"], 3)}))


def run_lj_table_step(lib, n, args):
    """the Lennard-Jones + Coulomb step with a type-pair table beside the steps of sections 7r and 7s on
    the same points: the jittered lattice of run_lj_step, or with --exclusions the rigid triples of run_lj_excl_step.
    Splittings and bandwidths as run_lj_step chooses them."""
    m = 4
    triples = args.exclusions
    if triples:
        n -= n % 3
    sites = n // 3 if triples else n
    box = [1.0, 0.0, 1.0, 0.0, 0.0, 1.0] if args.box is None else \
        (args.box if len(args.box) == 6 else [args.box[0], 0.0, args.box[1], 0.0, 0.0, args.box[2]])
    A = np.array([[box[0], 0.0, 0.0], [box[1], box[2], 0.0], [box[3], box[4], box[5]]])
    probe = tn.EwaldSplitting(1.0, 1e-3 * min(box[0], box[2], box[5]), 2, box=A, device="cpu")  # (volume and widths)
    r_c = min((3.0 * args.neighbours * probe.volume / (4.0 * math.pi * n)) ** (1.0 / 3.0), min(probe.widths) / 3.0)
    own_c = tn.EwaldSplitting.from_tolerance(args.tol, r_c, box=A)
    own_d = tn.DispersionSplitting.from_tolerance(args.tol, r_c, box=A)
    N = max(own_c.bandwidth, own_d.bandwidth)
    if not args.bandwidth_as_is:
        N = max(fft_friendly(own_c.bandwidth), fft_friendly(own_d.bandwidth))
    spc = tn.EwaldSplitting(own_c.alpha, r_c, N, box=A)
    spd = tn.DispersionSplitting(own_d.alpha, r_c, N, box=A)
    rng = np.random.default_rng(0)
    side = int(math.ceil(sites ** (1.0 / 3.0)))
    g = (np.arange(side) + 0.5) / side - 0.5
    v = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    spacing = probe.volume ** (1.0 / 3.0) / side
    if triples:
        centre = (v + (rng.random(v.shape) - 0.5) * (0.2 / side))[rng.permutation(side ** 3)[:sites]] @ A
        bond = 0.3 * spacing
        u = rng.standard_normal((sites, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        w = np.cross(u, rng.standard_normal((sites, 3)))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        half = math.radians(104.5 / 2)
        x = np.stack([centre, centre + bond * (math.cos(half) * u + math.sin(half) * w),
                      centre + bond * (math.cos(half) * u - math.sin(half) * w)], 1).reshape(n, 3)
        v = (x @ np.linalg.inv(A)).astype(np.float32)
        q = torch.from_numpy(np.tile(np.array([-0.834, 0.417, 0.417], dtype=np.float32), sites)).cuda()
        o = 3 * np.arange(sites)
        ex = tn.ExclusionList(np.concatenate([np.stack([o, o + 1], 1), np.stack([o, o + 2], 1), np.stack([o + 1, o + 2], 1)]), n)
        lists = (ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight)
    else:
        v = (v + (rng.random(v.shape) - 0.5) * (0.4 / side))[rng.permutation(side ** 3)[:n]].astype(np.float32)
        v[v >= 0.5] = -0.5  # (rounded up to the face: the same point)
        q = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
        ex, lists = None, (None,) * 4
    pos = torch.from_numpy(v).cuda()
    kl = {"coulomb": spc, "dispersion": spd, "cutoff": m, "fractional": True}
    walk = (box, spc.alpha, spd.alpha, r_c)
    for T in args.types:
        heavy = max(T // 2, 1) if triples else T  # (the types that carry a Lennard-Jones term)
        sigma, eps = np.zeros(T), np.zeros(T)
        sigma[:heavy], eps[:heavy] = spacing * (0.5 + 0.3 * rng.random(heavy)), 0.5 + rng.random(heavy)
        types = rng.integers(0, heavy, n)
        if triples:
            light = rng.integers(heavy, T, n) if T > heavy else np.zeros(n, dtype=np.int64)
            types = np.where(np.arange(n) % 3 == 0, types, light)
            if T == heavy:  # (one type: every atom is an oxygen)
                types[:] = 0
        table = tn.LJPairTable.lorentz_berthelot(torch.from_numpy(sigma), torch.from_numpy(eps), torch.from_numpy(types).cuda())
        cc, aa = tn.lj_coefficients(torch.from_numpy(sigma[types]), torch.from_numpy(eps[types]))
        c, a = cc.float().cuda(), aa.float().cuda()
        xs2, xs3 = torch.stack([q, table.c], 1), torch.stack([q, c, a], 1)
        fns = {"table_walk_op": lambda: tn.ops.nfft_ewald_lj_table_near(pos, xs2, table.types, table.table, None, *lists, *walk),
               "table_step": lambda: tn.nfft_ewald_lj_table_step(q, table, pos, exclusions=ex, **kl)}
        if triples:
            fns["yardstick_walk_op"] = lambda: tn.ops.nfft_ewald_lj_excl_near(pos, xs3, None, *lists, *walk)
            fns["yardstick_step"] = lambda: tn.nfft_ewald_lj_excl_step(q, c, a, pos, exclusions=ex, **kl)
        else:
            fns["yardstick_walk_op"] = lambda: tn.ops.nfft_ewald_lj_step_near(pos, xs3, None, *walk)
            fns["yardstick_step"] = lambda: tn.nfft_ewald_lj_step(q, c, a, pos, **kl)
        t = alternating_ms(fns, args.reps)
        tn.ops.check_status()
        med = {k: v_[0] for k, v_ in t.items()}
        ratio = lambda new, old: [round(med[new] / med[old], 3), round(t[new][1] / t[old][2], 3), round(t[new][2] / t[old][1], 3)]  # noqa: E731
        print(json.dumps({"bench": "ewald_lj_table_step", "yardstick": "lj_excl" if triples else "lj_step", "box": box, "points": n,
                          "types": T, "table_lds_bytes": 8 * T * (T | 1), "neighbours": args.neighbours, "tol": args.tol,
                          "r_cut": round(r_c, 5), "alpha_coulomb": round(spc.alpha, 3), "alpha_dispersion": round(spd.alpha, 3),
                          "N": N, "m": m, "cells": list(spc.cells), "reps": args.reps,
                          "median_min_max_ms": {k: [round(e, 4) for e in v_] for k, v_ in t.items()},
                          # (median over median; then the new at its fastest over the old at its slowest, and the other way round)
                          "walk_op_over_yardstick": ratio("table_walk_op", "yardstick_walk_op"),
                          "step_over_yardstick": ratio("table_step", "yardstick_step")}))


def run_bmh_table_step(lib, n, args):
    """the Buckingham / Born-Mayer-Huggins + Coulomb step beside the step of section 7t on the same points,
    types and list: the points, splittings and bandwidths of run_lj_table_step, restated."""
    m = 4
    triples = args.exclusions
    if triples:
        n -= n % 3
    sites = n // 3 if triples else n
    box = [1.0, 0.0, 1.0, 0.0, 0.0, 1.0] if args.box is None else \
        (args.box if len(args.box) == 6 else [args.box[0], 0.0, args.box[1], 0.0, 0.0, args.box[2]])
    A = np.array([[box[0], 0.0, 0.0], [box[1], box[2], 0.0], [box[3], box[4], box[5]]])
    probe = tn.EwaldSplitting(1.0, 1e-3 * min(box[0], box[2], box[5]), 2, box=A, device="cpu")  # (volume and widths)
    r_c = min((3.0 * args.neighbours * probe.volume / (4.0 * math.pi * n)) ** (1.0 / 3.0), min(probe.widths) / 3.0)
    own_c = tn.EwaldSplitting.from_tolerance(args.tol, r_c, box=A)
    own_d = tn.DispersionSplitting.from_tolerance(args.tol, r_c, box=A)
    N = max(own_c.bandwidth, own_d.bandwidth)
    if not args.bandwidth_as_is:
        N = max(fft_friendly(own_c.bandwidth), fft_friendly(own_d.bandwidth))
    spc = tn.EwaldSplitting(own_c.alpha, r_c, N, box=A)
    spd = tn.DispersionSplitting(own_d.alpha, r_c, N, box=A)
    rng = np.random.default_rng(0)
    side = int(math.ceil(sites ** (1.0 / 3.0)))
    g = (np.arange(side) + 0.5) / side - 0.5
    v = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    spacing = probe.volume ** (1.0 / 3.0) / side
    if triples:
        centre = (v + (rng.random(v.shape) - 0.5) * (0.2 / side))[rng.permutation(side ** 3)[:sites]] @ A
        bond = 0.3 * spacing
        u = rng.standard_normal((sites, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        w = np.cross(u, rng.standard_normal((sites, 3)))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        half = math.radians(104.5 / 2)
        x = np.stack([centre, centre + bond * (math.cos(half) * u + math.sin(half) * w),
                      centre + bond * (math.cos(half) * u - math.sin(half) * w)], 1).reshape(n, 3)
        v = (x @ np.linalg.inv(A)).astype(np.float32)
        q = torch.from_numpy(np.tile(np.array([-0.834, 0.417, 0.417], dtype=np.float32), sites)).cuda()
        o = 3 * np.arange(sites)
        ex = tn.ExclusionList(np.concatenate([np.stack([o, o + 1], 1), np.stack([o, o + 2], 1), np.stack([o + 1, o + 2], 1)]), n)
        lists = (ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight)
    else:
        v = (v + (rng.random(v.shape) - 0.5) * (0.4 / side))[rng.permutation(side ** 3)[:n]].astype(np.float32)
        v[v >= 0.5] = -0.5  # (rounded up to the face: the same point)
        q = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
        ex, lists = None, (None,) * 4
    pos = torch.from_numpy(v).cuda()
    kl = {"coulomb": spc, "dispersion": spd, "cutoff": m, "fractional": True}
    walk = (box, spc.alpha, spd.alpha, r_c)
    for T in args.types:
        heavy = max(T // 2, 1) if triples else T  # (the types that carry a short-range term)
        size, eps = np.zeros(T), np.zeros(T)
        size[:heavy], eps[:heavy] = spacing * (0.7 + 0.3 * rng.random(heavy)), 0.5 + rng.random(heavy)
        types = rng.integers(0, heavy, n)
        if triples:
            light = rng.integers(heavy, T, n) if T > heavy else np.zeros(n, dtype=np.int64)
            types = np.where(np.arange(n) % 3 == 0, types, light)
            if T == heavy:  # (one type: every atom is an oxygen)
                types[:] = 0
        tt = torch.from_numpy(types).cuda()
        # exp-6: r_m and the steepness (12 .. 14) mixed arithmetically, eps geometrically; light types keep B and lose A, C6, C8
        rm = 0.5 * (size[:, None] + size[None, :])
        rm[rm == 0.0] = spacing
        st = 12.0 + 2.0 * rng.random(T)
        st = 0.5 * (st[:, None] + st[None, :])
        e = np.sqrt(eps[:, None] * eps[None, :])
        C6 = e * st * rm ** 6 / (st - 6.0)
        tabs = [torch.from_numpy(v) for v in (6.0 * e * np.exp(st) / (st - 6.0), st / rm, C6, 0.3 * C6 * rm ** 2)]
        table = tn.BMHPairTable(*tabs, tt)
        bare = tn.BMHPairTable(*tabs, tt, grid_c=torch.zeros(T))
        yard = tn.LJPairTable.lorentz_berthelot(torch.from_numpy(0.7 * size), torch.from_numpy(eps), tt)
        xs, xs0, xsy = torch.stack([q, table.c], 1), torch.stack([q, bare.c], 1), torch.stack([q, yard.c], 1)
        walk0 = (box, spc.alpha, spc.alpha, r_c)
        kl0 = {"coulomb": spc, "dispersion": None, "cutoff": m, "fractional": True}
        fns = {"bmh_walk_op": lambda: tn.ops.nfft_ewald_bmh_table_near(pos, xs, table.types, table.table, None, *lists, *walk),
               "bmh_walk_op_no_grid": lambda: tn.ops.nfft_ewald_bmh_table_near(pos, xs0, bare.types, bare.table, None, *lists, *walk0),
               "yardstick_walk_op": lambda: tn.ops.nfft_ewald_lj_table_near(pos, xsy, yard.types, yard.table, None, *lists, *walk),
               "bmh_step": lambda: tn.nfft_ewald_bmh_table_step(q, table, pos, exclusions=ex, **kl),
               "bmh_step_no_grid": lambda: tn.nfft_ewald_bmh_table_step(q, bare, pos, exclusions=ex, **kl0),
               "yardstick_step": lambda: tn.nfft_ewald_lj_table_step(q, yard, pos, exclusions=ex, **kl)}
        t = alternating_ms(fns, args.reps)
        tn.ops.check_status()
        med = {k: v_[0] for k, v_ in t.items()}
        ratio = lambda new, old: [round(med[new] / med[old], 3), round(t[new][1] / t[old][2], 3), round(t[new][2] / t[old][1], 3)]  # noqa: E731
        print(json.dumps({"bench": "ewald_bmh_table_step", "yardstick": "lj_table", "exclusions": bool(triples), "box": box, "points": n,
                          "types": T, "table_lds_bytes": 16 * T * (T | 1), "yardstick_lds_bytes": 8 * T * (T | 1),
                          "neighbours": args.neighbours, "tol": args.tol, "r_cut": round(r_c, 5),
                          "alpha_coulomb": round(spc.alpha, 3), "alpha_dispersion": round(spd.alpha, 3),
                          "N": N, "m": m, "cells": list(spc.cells), "reps": args.reps,
                          "median_min_max_ms": {k: [round(e_, 4) for e_ in v_] for k, v_ in t.items()},
                          # (median over median; then the new at its fastest over the old at its slowest, and the other way round)
                          "walk_op_over_yardstick": ratio("bmh_walk_op", "yardstick_walk_op"),
                          "walk_op_no_grid_over_yardstick": ratio("bmh_walk_op_no_grid", "yardstick_walk_op"),
                          "step_over_yardstick": ratio("bmh_step", "yardstick_step"),
                          "step_no_grid_over_yardstick": ratio("bmh_step_no_grid", "yardstick_step")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--neighbours", type=float, default=100.0)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--box", type=lambda t: [float(e) for e in t.split(",")], default=None,
                    help="a,b,c (orthorhombic) or A00,A10,A11,A20,A21,A22 (lower triangular, rows = lattice vectors)")
    ap.add_argument("--virial", action="store_true", help="add a row for nfft_ewald_virial and its two reductions")
    ap.add_argument("--dispersion", action="store_true", help="time the dispersion sum 1/r^6 (unit cube) instead")
    ap.add_argument("--dipole", action="store_true", help="time the sum of charges and point dipoles (unit cube) instead")
    ap.add_argument("--stokeslet", action="store_true", help="time the periodic Stokeslet sum (unit cube) instead")
    ap.add_argument("--rpy", action="store_true", help="time the periodic Rotne-Prager-Yamakawa sum (unit cube) instead")
    ap.add_argument("--phi", type=float, default=0.1, help="--rpy: the volume fraction of the spheres, n (4/3) pi a^3")
    ap.add_argument("--exclusions", action="store_true",
                    help="time the bonded-pair correction on rigid triples (the unit cube, or --box) instead")
    ap.add_argument("--yukawa", action="store_true", help="time the screened Coulomb sum (unit cube) instead; with --virial its virial too")
    ap.add_argument("--step", action="store_true",
                    help="time nfft_ewald_step beside the calls, pair loops and spectral passes it replaces (with --box, --exclusions)")
    ap.add_argument("--lj-step", action="store_true",
                    help="time nfft_ewald_lj_step beside the three calls, pair loops and spectral passes it replaces (with --box); "
                         "with --exclusions nfft_ewald_lj_excl_step on rigid triples beside it and beside the three calls")
    ap.add_argument("--table", action="store_true",
                    help="--lj-step: time nfft_ewald_lj_table_step and its pair operator beside nfft_ewald_lj_step, with --exclusions "
                         "beside nfft_ewald_lj_excl_step, for every type count of --types")
    ap.add_argument("--bmh", action="store_true",
                    help="--lj-step: time nfft_ewald_bmh_table_step (also with dispersion=None) and its pair operator beside "
                         "nfft_ewald_lj_table_step and its pair operator, with or without --exclusions, for every type count of --types")
    ap.add_argument("--types", type=int, nargs="+", default=[2, 32], help="--table, --bmh: the type counts T, each in [1, 32]")
    ap.add_argument("--bandwidth-as-is", action="store_true",
                    help="--lj-step: keep the bandwidths of from_tolerance instead of the next sizes with prime factors <= 7")
    ap.add_argument("--screening", type=float, default=1.0, help="--yukawa: lambda r_c, the screening parameter times r_c")
    args = ap.parse_args()
    if args.box is not None and len(args.box) not in (3, 6):
        ap.error("--box takes three or six comma-separated numbers")
    if args.step and (args.virial or args.dispersion or args.dipole or args.stokeslet or args.rpy or args.yukawa):
        ap.error("--step times the Coulomb sum's fused step on its own (with or without --box and --exclusions)")
    if args.lj_step and (args.step or args.virial or args.dispersion or args.dipole or args.stokeslet or args.rpy or args.yukawa):
        ap.error("--lj-step times the Lennard-Jones + Coulomb step on its own (with or without --box and --exclusions)")
    if args.table and not args.lj_step:
        ap.error("--table goes with --lj-step")
    if args.bmh and (not args.lj_step or args.table):
        ap.error("--bmh goes with --lj-step and not with --table")
    if args.yukawa and (args.box is not None or args.dispersion or args.dipole or args.stokeslet or args.rpy or args.exclusions):
        ap.error("--yukawa times the unit cube on its own (with or without --virial)")
    if args.yukawa and not 0.0 < args.screening <= 50.0:
        ap.error("--screening is lambda r_c and must lie in (0, 50]")
    if args.exclusions and (args.dispersion or args.virial or args.dipole or args.stokeslet or args.rpy):
        ap.error("--exclusions times the Coulomb sum's correction on its own (with or without --box)")
    if args.dispersion and args.box is not None:
        ap.error("--dispersion times the unit cube and does not go with --box")
    if args.dipole and (args.box is not None or args.dispersion or args.virial):
        ap.error("--dipole times the unit cube on its own")
    if args.stokeslet and (args.box is not None or args.dispersion or args.virial or args.dipole):
        ap.error("--stokeslet times the unit cube on its own")
    if args.rpy and (args.box is not None or args.dispersion or args.virial or args.dipole or args.stokeslet):
        ap.error("--rpy times the unit cube on its own")
    torch.cuda.set_device(0)
    lib = _lib.load()
    for n in args.points:
        if args.lj_step and args.table:
            run_lj_table_step(lib, n, args)
            continue
        if args.lj_step and args.bmh:
            run_bmh_table_step(lib, n, args)
            continue
        if args.lj_step:
            (run_lj_excl_step if args.exclusions else run_lj_step)(lib, n, args)
            continue
        if args.step:
            run_step(lib, n, args)
            continue
        if args.yukawa:
            run_yukawa(lib, n, args)
            continue
        if args.exclusions:
            run_exclusions(lib, n, args)
            continue
        if args.rpy:
            run_rpy(lib, n, args)
            continue
        if args.stokeslet:
            run_stokeslet(lib, n, args)
            continue
        if args.dipole:
            run_dipole(lib, n, args)
            continue
        if args.dispersion:
            run_dispersion(lib, n, args)
            if args.virial:
                run_dispersion_virial(lib, n, args)
            continue
        (run if args.box is None else run_box)(lib, n, args)
        if args.virial:
            run_virial(lib, n, args)


if __name__ == "__main__":
    main()
