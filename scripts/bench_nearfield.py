"""Times nfft_fastsum_nearfield's two halves (profiles/r09_nearfield.md):

    python scripts/bench_nearfield.py [--points 100000] [--reps 10] [--gradient | --point-gradients]

3-D one_over_modulus, N = 64, p = 4 (eps_I = eps_B = 1/16), cutoff m = 4, shared points uniform in the ball of radius
kern.max_radius, C = 1 and C = 4 real columns.  Device-event medians of `reps` calls after two warm-up calls:
  far field     nfft_fastsum with kern.coeffs
  near field    ops.nfft_nearfield as a whole, and its two parts on their own -- the plumbing (cell keys, one stable
                sort, the start table, the gathers of the points and of x: the torch calls core.so makes, restated here)
                and the pair loop (nfft_hip_nearfield through the C ABI on the arrays the plumbing made)
  pairs         distance tests per call = sum over targets of the sources in the 3^3 cells around it, and per second of
                the pair loop; `in range` counts those with r < eps_I
One JSON line per column count.

--gradient times nfft_fastsum_nearfield_gradient on the same problem instead (DESIGN.md section 7e,
profiles/r10_nearfield_gradient.md): the far gradient (one adjoint, the product with the dim coefficient arrays, one forward
with dim C columns), the near gradient and its transpose as operators, their plumbing, and the three pair loops through
the C ABI on the same sorted arrays -- gradient, transpose and, next to them, the value loop (nfft_hip_nearfield, the
kernel of section 7d unchanged) -- with the ratios gradient / value and transpose / value.

--point-gradients times the gradient of the near field with respect to the points on the same problem (DESIGN.md section
7f, profiles/r10_point_gradients.md).  Pair loops through the C ABI on the same sorted arrays, in one run: the contracting
sweep one-sided (the targets' gradient) and symmetric (both gradients of the shared points), against the same gradients
composed from nfft_hip_nearfield_gradient's sweep(s) and the torch contraction with dy (one sweep and one contraction per
side); the value, gradient and transpose loops alongside; and the operator as a whole, one-sided and symmetric.
"""
import argparse
import ctypes
import json
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


def cell_order(pos, G):
    """what core.so's cell_order does for one point set without a batch vector"""
    cell = ((pos + 0.25) * float(2 * G)).floor().clamp(0, G - 1).to(torch.int64)
    key = cell[:, 0] + cell[:, 1] * G + cell[:, 2] * (G * G)
    skey, order = torch.sort(key, stable=True)
    start = torch.searchsorted(skey, torch.arange(G ** 3 + 1, device=pos.device), out_int32=True)
    return pos.index_select(0, order), order, start


def gradient_mode(args, lib, kern, pos, x, G, m, pairs, in_range):
    from torch_nfft_amd.nearfield import _far_gradient
    n, C = x.shape
    gpoly = kern.near_gradient_poly.tolist()
    v = torch.randn(n, 3, C, device="cuda")
    grad_op = lambda t, transpose: tn.ops.nfft_nearfield_gradient(pos, pos, t, None, None, kern.kernel_id, kern.c, kern.eps_I,  # noqa: E731
                                                                  gpoly, transpose)
    far = median_ms(lambda: _far_gradient(x, kern, pos, pos, None, None, m), args.reps)
    near = median_ms(lambda: grad_op(x, False), args.reps)
    near_t = median_ms(lambda: grad_op(v, True), args.reps)

    def plumbing(t, out_row):
        spos, order, start = cell_order(pos, G)
        return spos, order, start, t.reshape(n, -1).index_select(0, order), torch.zeros(n, out_row, device="cuda")

    plumb = median_ms(lambda: plumbing(x, 3 * C), args.reps)
    plumb_t = median_ms(lambda: plumbing(v, C), args.reps)
    spos, order, start, xs, z = plumbing(x, 3 * C)
    _, _, _, vs, zt = plumbing(v, C)
    zv = torch.zeros(n, C, device="cuda")
    q = _lib.NearfieldProblem(dim=3, kernel=kern.kernel_id, poly_terms=kern.p, cells_per_axis=G, num_sources=n, num_targets=n,
                              num_columns=C, batch_size=1, c=kern.c, eps_I=kern.eps_I)
    for e, a in enumerate(kern.near_poly.tolist()):
        q.poly[e] = a
    gp = (ctypes.c_double * 8)(*gpoly)
    nbytes = lib.nfft_hip_nearfield_gradient_workspace_bytes(ctypes.byref(q))
    assert nbytes == lib.nfft_hip_nearfield_workspace_bytes(ctypes.byref(q))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def loop(transpose, src, out):
        _lib.check(lib.nfft_hip_nearfield_gradient(ctypes.byref(q), transpose, ctypes.cast(gp, ctypes.c_void_p), spos.data_ptr(),
                                                   src.data_ptr(), start.data_ptr(), spos.data_ptr(), order.data_ptr(),
                                                   start.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, stream))

    def value_loop():
        _lib.check(lib.nfft_hip_nearfield(ctypes.byref(q), spos.data_ptr(), xs.data_ptr(), start.data_ptr(), spos.data_ptr(),
                                          order.data_ptr(), start.data_ptr(), zv.data_ptr(), ws.data_ptr(), nbytes, stream))

    value = median_ms(value_loop, args.reps)
    pair = median_ms(lambda: loop(0, xs, z), args.reps)
    pair_t = median_ms(lambda: loop(1, vs, zt), args.reps)
    assert torch.equal(grad_op(x, False), z.reshape(n, 3, C)), "the restated plumbing must give the operator's bits"
    assert torch.equal(grad_op(v, True), zt), "the restated plumbing must give the operator's bits"
    tn.ops.check_status()
    print(json.dumps({"bench": "nearfield_gradient", "kernel": kern.name, "N": kern.bandwidth, "p": kern.p, "m": m, "points": n,
                      "columns": C, "cells_per_axis": G, "far_gradient_ms": round(far, 4), "near_gradient_ms": round(near, 4),
                      "near_transpose_ms": round(near_t, 4), "gradient_plumbing_ms": round(plumb, 4),
                      "transpose_plumbing_ms": round(plumb_t, 4), "gradient_pair_loop_ms": round(pair, 4),
                      "transpose_pair_loop_ms": round(pair_t, 4), "value_pair_loop_ms": round(value, 4),
                      "gradient_over_value": round(pair / value, 3), "transpose_over_value": round(pair_t / value, 3),
                      "pairs_tested": pairs, "pairs_in_range_estimate": in_range,
                      "gradient_pairs_per_second": round(pairs / (pair * 1e-3), 1)}))


def point_gradient_mode(args, lib, kern, pos, x, G, m, pairs, in_range):
    n, C = x.shape
    gpoly = kern.near_gradient_poly.tolist()
    dy = torch.randn(n, C, device="cuda")
    v = torch.randn(n, 3, C, device="cuda")
    op = lambda need_s, need_t: tn.ops.nfft_nearfield_point_gradient(pos, pos, x, dy, None, None, kern.kernel_id, kern.c,  # noqa: E731
                                                                     kern.eps_I, gpoly, need_s, need_t)
    op_sym = median_ms(lambda: op(True, True), args.reps)
    op_one = median_ms(lambda: op(False, True), args.reps)
    spos, order, start = cell_order(pos, G)
    xs, dys, vs = x.index_select(0, order), dy.index_select(0, order), v.reshape(n, -1).index_select(0, order)
    out_one, out_sym = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
    zg, zg2, zt, zv = (torch.zeros(n, 3 * C, device="cuda"), torch.zeros(n, 3 * C, device="cuda"),
                       torch.zeros(n, C, device="cuda"), torch.zeros(n, C, device="cuda"))
    q = _lib.NearfieldProblem(dim=3, kernel=kern.kernel_id, poly_terms=kern.p, cells_per_axis=G, num_sources=n, num_targets=n,
                              num_columns=C, batch_size=1, c=kern.c, eps_I=kern.eps_I)
    for e, a in enumerate(kern.near_poly.tolist()):
        q.poly[e] = a
    gpoly_c = (ctypes.c_double * 8)(*gpoly)
    gp = ctypes.cast(gpoly_c, ctypes.c_void_p)
    nbytes = lib.nfft_hip_nearfield_point_gradient_workspace_bytes(ctypes.byref(q))
    assert nbytes == lib.nfft_hip_nearfield_gradient_workspace_bytes(ctypes.byref(q))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def sweep(symmetric, out):
        _lib.check(lib.nfft_hip_nearfield_point_gradient(ctypes.byref(q), symmetric, gp, spos.data_ptr(), xs.data_ptr(),
                                                         start.data_ptr(), spos.data_ptr(), dys.data_ptr(), order.data_ptr(),
                                                         start.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, stream))

    def grad_loop(transpose, src, out):
        _lib.check(lib.nfft_hip_nearfield_gradient(ctypes.byref(q), transpose, gp, spos.data_ptr(), src.data_ptr(),
                                                   start.data_ptr(), spos.data_ptr(), order.data_ptr(), start.data_ptr(),
                                                   out.data_ptr(), ws.data_ptr(), nbytes, stream))

    def value_loop():
        _lib.check(lib.nfft_hip_nearfield(ctypes.byref(q), spos.data_ptr(), xs.data_ptr(), start.data_ptr(), spos.data_ptr(),
                                          order.data_ptr(), start.data_ptr(), zv.data_ptr(), ws.data_ptr(), nbytes, stream))

    def composed_one():  # dt[i, a] = sum_c dy[i, c] G(x)[i, a, c]
        grad_loop(0, xs, zg)
        return (zg.view(n, 3, C) * dy[:, None, :]).sum(-1)

    def composed_both():  # ... + ds[j, a] = sum_c x[j, c] G(dy)[j, a, c] on the shared points
        grad_loop(0, xs, zg)
        grad_loop(0, dys, zg2)
        return (zg.view(n, 3, C) * dy[:, None, :]).sum(-1) + (zg2.view(n, 3, C) * x[:, None, :]).sum(-1)

    one = median_ms(lambda: sweep(0, out_one), args.reps)
    comp_one = median_ms(composed_one, args.reps)
    sym = median_ms(lambda: sweep(1, out_sym), args.reps)
    comp_both = median_ms(composed_both, args.reps)
    contraction = median_ms(lambda: (zg.view(n, 3, C) * dy[:, None, :]).sum(-1), args.reps)
    value = median_ms(value_loop, args.reps)
    grad = median_ms(lambda: grad_loop(0, xs, zg), args.reps)
    transpose = median_ms(lambda: grad_loop(1, vs, zt), args.reps)
    total, zeros = op(True, True)
    assert torch.equal(total, out_sym) and not bool(zeros.any()), "the restated plumbing must give the operator's bits"
    assert torch.equal(op(False, True)[1], out_one), "the restated plumbing must give the operator's bits"
    rel = lambda a, b: float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))  # noqa: E731
    tn.ops.check_status()
    print(json.dumps({"bench": "nearfield_point_gradients", "kernel": kern.name, "N": kern.bandwidth, "p": kern.p, "m": m,
                      "points": n, "columns": C, "cells_per_axis": G, "operator_symmetric_ms": round(op_sym, 4),
                      "operator_one_sided_ms": round(op_one, 4), "one_sided_pair_loop_ms": round(one, 4),
                      "composed_one_sided_ms": round(comp_one, 4), "symmetric_pair_loop_ms": round(sym, 4),
                      "composed_both_ms": round(comp_both, 4), "torch_contraction_ms": round(contraction, 4),
                      "value_pair_loop_ms": round(value, 4), "gradient_pair_loop_ms": round(grad, 4),
                      "transpose_pair_loop_ms": round(transpose, 4), "one_sided_over_composed": round(one / comp_one, 3),
                      "symmetric_over_composed": round(sym / comp_both, 3), "one_sided_over_value": round(one / value, 3),
                      "symmetric_over_value": round(sym / value, 3),
                      "one_sided_vs_composed_rel_l2": rel(out_one, composed_one()),
                      "symmetric_vs_composed_rel_l2": rel(out_sym, composed_both()),
                      "pairs_tested": pairs, "pairs_in_range_estimate": in_range,
                      "symmetric_pairs_per_second": round(pairs / (sym * 1e-3), 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--gradient", action="store_true")
    ap.add_argument("--point-gradients", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lib = _lib.load()
    N, p, m, n = 64, 4, 4, args.points
    kern = tn.RegularizedKernel("one_over_modulus", dim=3, bandwidth=N, p=p)
    rng = np.random.default_rng(0)
    v = rng.standard_normal((n, 3))
    v *= (kern.max_radius * rng.random((n, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
    pos = torch.from_numpy(v.astype(np.float32)).cuda()
    G = int(lib.nfft_hip_nearfield_cells(3, kern.eps_I, 1))
    # pairs tested: targets of a cell x sources of the 27 cells around it
    cells = np.clip(np.floor((v.astype(np.float32) + 0.25) * (2 * G)), 0, G - 1).astype(np.int64)
    count = np.zeros((G + 2,) * 3, dtype=np.int64)
    np.add.at(count, (cells[:, 0] + 1, cells[:, 1] + 1, cells[:, 2] + 1), 1)
    box = sum(count[1 + a:G + 1 + a, 1 + b:G + 1 + b, 1 + c:G + 1 + c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1))
    pairs = int((count[1:-1, 1:-1, 1:-1] * box).sum())
    sub = rng.choice(n, 2000, replace=False)
    hits = sum(int((np.linalg.norm(v[sub[i:i + 100]][:, None, :] - v[None, :, :], axis=-1) < kern.eps_I).sum())
               for i in range(0, 2000, 100))
    in_range = int(hits * (n / 2000.0))
    for C in (1, 4):
        x = torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)).cuda()
        poly = kern.near_poly.tolist()
        if args.gradient:
            gradient_mode(args, lib, kern, pos, x, G, m, pairs, in_range)
            continue
        if args.point_gradients:
            point_gradient_mode(args, lib, kern, pos, x, G, m, pairs, in_range)
            continue
        far = median_ms(lambda: tn.nfft_fastsum(x, kern.coeffs, pos, cutoff=m), args.reps)
        near = median_ms(lambda: tn.ops.nfft_nearfield(pos, pos, x, None, None, kern.kernel_id, kern.c, kern.eps_I, poly), args.reps)

        def plumbing():
            spos, order, start = cell_order(pos, G)
            return spos, order, start, x.index_select(0, order), torch.zeros(n, C, device="cuda")

        plumb = median_ms(plumbing, args.reps)
        spos, order, start, xs, z = plumbing()
        q = _lib.NearfieldProblem(dim=3, kernel=kern.kernel_id, poly_terms=p, cells_per_axis=G, num_sources=n, num_targets=n,
                                  num_columns=C, batch_size=1, c=kern.c, eps_I=kern.eps_I)
        for e, a in enumerate(poly):
            q.poly[e] = a
        nbytes = lib.nfft_hip_nearfield_workspace_bytes(ctypes.byref(q))
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def loop():
            _lib.check(lib.nfft_hip_nearfield(ctypes.byref(q), spos.data_ptr(), xs.data_ptr(), start.data_ptr(), spos.data_ptr(),
                                              order.data_ptr(), start.data_ptr(), z.data_ptr(), ws.data_ptr(), nbytes, stream))

        pair_loop = median_ms(loop, args.reps)
        full = tn.ops.nfft_nearfield(pos, pos, x, None, None, kern.kernel_id, kern.c, kern.eps_I, poly)
        assert torch.equal(full, z), "the restated plumbing must give the operator's bits"
        tn.ops.check_status()
        print(json.dumps({"bench": "nearfield", "kernel": kern.name, "N": N, "p": p, "m": m, "points": n, "columns": C,
                          "cells_per_axis": G, "far_ms": round(far, 4), "near_ms": round(near, 4),
                          "near_plumbing_ms": round(plumb, 4), "near_pair_loop_ms": round(pair_loop, 4),
                          "pairs_tested": pairs, "pairs_in_range_estimate": in_range,
                          "pairs_per_second": round(pairs / (pair_loop * 1e-3), 1)}))


if __name__ == "__main__":
    main()
