"""GPU tests of the lane-per-point derivative gathers (csrc/interp_grad.hip) at every window width and tiling.

interp_grad_kernel<DIM, W, WIDE, VALUE = false> (the point gradient), its VALUE = true form (the fused value + gradient
gather of the fastsum backward) and interp_hvp_kernel<DIM, W, WIDE> (the second-order gather) are instantiated over
GatherCfg<DIM, W, WIDE> (csrc/lane_gather.h).  A width changes the tile shape, the number of aligned 16-byte reads per
row, the row stride, the steps of the resident-plane slide and the hand-set occupancy floors, so every one of the 31
geometries a call can reach runs here, each with all three kernels:

  geometry     shape               why the shape gets this tiling
  1-D          N = 64,  n = 600    dim 1: one 1 x 256 tile (clipped to M = 128)
  2-D          N = 48,  n = 1500   dim 2: 32 x 32 tiles, three per axis of M = 96; M is no power of two, so split_cell
                                   takes its general path and the FFT stage is the full rocFFT route
  narrow 3-D   N = 16,  n = 2000   common.h make_geom: the wide tiling needs M >= 64, here M = 32.  16 x 32 pencils with
                                   TC = 17 - W planes per chunk for W <= 12, 8 x 32 with TC = 3 at W = 14, 8 x 16 with
                                   TC = 21 - W at W = 16 and 18
  wide 3-D     N = 64,  n = 3000   make_geom: wide for 64 <= M <= 1024 and W <= 16 (m <= 7); api.hip prefer_narrow is
                                   false at N = 64 unless m <= 3, B >= 8 and one column.  (33 - W) x (65 - W) pencils,
                                   TC = 17 - W: every width cuts M = 128 into another ragged set of pencils

B = 2 point sets of unequal size and two complex columns (Cr = 4 real planes) throughout.  The points are uniform float32
draws with a block of placed points, whose cells are worked out in float64 from the table above the way split_cell sees
pos * M:

  edge_lo2 / edge_hi2   the first four and the last four cells of a tile on the last axis (the first and the last cell
                        and their neighbours: the alignment col & 3 of a lane's 16-byte reads is a property of the cell,
                        so all four occur at both ends of a tile), random fractions; two tiles where there are two, one of
                        them the ragged last one
  edge_lo1 / edge_hi1   the first and the last cell of a tile on the axis before it (2-D, 3-D), same tiles rule
  boundary              every coordinate exactly on a cell boundary (fraction 0)
  seam                  one coordinate at -0.5 or at the largest float32 below 0.5
  gaps (3-D)            the whole second point set: axis-0 cells {0, 1, 5, 6, 20, M - 1} only, random cells on the other
                        axes, so that consecutive occupied chunks of a pencil are adjacent, a few chunks apart or more
                        than the resident planes apart -- the three branches of the plane slide

Three legs per geometry against float64 on the same float32 inputs; the float64 grid of xhat is computed once per test:

  gradient   ops.nfft_forward_grad_points        vs test_pos_grad_ref.grad_gather            TR   (test_gpu_pos_grad)
  HVP        ops.nfft_forward_grad_points_backward (dw, dpos)
                                                 vs test_pos_hvp_ref.hvp_gather              TR2  (test_gpu_pos_hvp)
  value + gradient
             ops.nfft_fastsum_backward (dx, dsources; real coefficients that are not even, 150 separate targets)
                                                 vs H = conj(c) nfft_ref.nfft_adjoint(dy, targets): dsources by
                                                    grad_gather(grid_of(H)), dx by interp_f64(grid_of(H))
                                                                                              TRF  (test_gpu_fastsum_grad)

Every output is checked three ways with the same imported tolerance, so that a fault confined to one alignment or one
tile edge is not diluted by the uniform points: relative L2 over all compared points, over each alignment class
col & 3 against its own norm, and over each placed category against its own norm.  All points are compared where the
float64 gather stays under about 1.5e6 window taps per column, else a fixed random subset of 400 points plus every placed
point.  The tolerances are the project's contracts of the three files named above; none is restated here.
"""
import numpy as np
import pytest
import torch

import test_pos_grad_ref as ref1
import test_pos_hvp_ref as ref2
from oracle import nfft_ref
from test_gpu_fastsum_grad import TRF
from test_gpu_pos_grad import TR, dev, host, rel
from test_gpu_pos_hvp import TR2

pytestmark = pytest.mark.gpu

B = 2            # point sets
COLS = 2         # complex columns: Cr = 4 real planes
NT = 150         # targets of the fastsum leg
GAP_CELLS = (0, 1, 5, 6, 20, -1)  # axis-0 cells of the second point set in 3-D (-1: M - 1)
ALL_TAPS = 1.5e6  # compare every point while n (2m+2)^d stays below this
SUBSET = 400

SHAPES = {  # geometry: (d, N, n, wide, size of the second point set)
    "1d": (1, 64, 600, False, 200),
    "2d": (2, 48, 1500, False, 500),
    "narrow3d": (3, 16, 2000, False, 150),
    "wide3d": (3, 64, 3000, True, 150),
}
GEOMETRIES = [(name, m) for name in SHAPES for m in range(1, 8 if SHAPES[name][3] else 9)]


@pytest.fixture(scope="module")
def tn():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import torch_nfft_amd
    return torch_nfft_amd


def tiling(d, N, m, wide):
    """(TC, T1, T2): planes per chunk and the pencil's cross-section, common.h tile_cfg clipped to the grid by make_geom."""
    W, M = 2 * m + 2, 2 * N
    if d == 1:
        t = (1, 1, 256)
    elif d == 2:
        t = (1, 32, 32)
    elif wide:
        assert M >= 64 and W <= 16
        t = (17 - W, 33 - W, 65 - W)
    elif W <= 12:
        t = (17 - W, 16, 32)
    elif W == 14:
        t = (3, 8, 32)
    else:
        t = (21 - W, 8, 16)
    return tuple(min(x, M) for x in t)


def cells_of(pos, M):
    """Cell per coordinate, from the float32 positions in float64: floor(pos * M) mod M (the product is exact)."""
    return np.floor(np.asarray(pos, dtype=np.float32).astype(np.float64) * M).astype(np.int64) % M


def coord(cell, frac, M):
    """Position in [-0.5, 0.5) of (cell + frac) / M on the torus."""
    cell = np.asarray(cell, dtype=np.float64)
    return (cell + frac - np.where(cell >= M // 2, M, 0)) / M


def edge_cells(T, M, offsets):
    """Cells at `offsets` from the first (offsets >= 0) or the last (offsets < 0: -1 is the last) cell of a tile of extent T,
    for a tile inside the grid and the (ragged) last tile."""
    nt = (M + T - 1) // T
    out = []
    for tile in sorted({min(1, nt - 1), nt - 1}):
        lo, hi = tile * T, min(tile * T + T, M)
        out += [lo + o if o >= 0 else hi + o for o in offsets]
    return out


def make_points(rng, d, N, m, n, wide, n1):
    """pos [n, d] float32, batch [n], the placed categories {name: rows} and the alignment class col & 3 of every point."""
    M = 2 * N
    TC, T1, T2 = tiling(d, N, m, wide)
    pos = (rng.random((n, d)) - 0.5).astype(np.float32)
    batch = np.concatenate([np.zeros(n - n1, np.int64), np.ones(n1, np.int64)])
    cats = {}
    row = [0]

    def place(name, axis, cells, per_cell):
        """per_cell points in each of `cells` on `axis` with random fractions; the other coordinates stay uniform."""
        cells = np.repeat(np.asarray(cells), per_cell)
        rows = np.arange(row[0], row[0] + len(cells))
        pos[rows, axis] = coord(cells, rng.uniform(0.05, 0.95, len(cells)), M).astype(np.float32)
        assert np.array_equal(cells_of(pos[rows, axis], M), cells)
        cats[name] = rows
        row[0] += len(cells)

    place("edge_lo2", d - 1, edge_cells(T2, M, (0, 1, 2, 3)), 2)
    place("edge_hi2", d - 1, edge_cells(T2, M, (-1, -2, -3, -4)), 2)
    if d >= 2:
        place("edge_lo1", d - 2, edge_cells(T1, M, (0,)), 8)
        place("edge_hi1", d - 2, edge_cells(T1, M, (-1,)), 8)
    # cell boundaries: k / M that float32 holds exactly (every k for a power of two M, every third at M = 96)
    exact = np.array([k for k in range(M) if float(np.float32(coord(k, 0.0, M))) * M == k - (M if k >= M // 2 else 0)])
    assert len(exact) >= M // 3
    rows = np.arange(row[0], row[0] + 12)
    pos[rows] = coord(rng.choice(exact, (12, d)), 0.0, M).astype(np.float32)
    assert np.all(pos[rows].astype(np.float64) * M == np.round(pos[rows].astype(np.float64) * M))
    cats["boundary"] = rows
    row[0] += 12
    # the torus seam, one axis at a time
    rows = np.arange(row[0], row[0] + 8 * d)
    for a in range(d):
        pos[rows[8 * a:8 * a + 4], a] = -0.5
        pos[rows[8 * a + 4:8 * a + 8], a] = np.nextafter(np.float32(0.5), np.float32(0.0))
    assert np.all(pos < 0.5) and np.all(pos >= -0.5)
    cats["seam"] = rows
    row[0] += 8 * d
    assert row[0] < n - n1  # the placed block lies inside the first point set
    if d == 3:
        rows = np.arange(n - n1, n)
        gap = np.array([c % M for c in GAP_CELLS])[np.arange(n1) % len(GAP_CELLS)]
        pos[rows, 0] = coord(gap, rng.uniform(0.05, 0.95, n1), M).astype(np.float32)
        assert np.array_equal(cells_of(pos[rows, 0], M), gap)
        cats["gaps"] = rows
    c2 = cells_of(pos[:, d - 1], M)
    align = (c2 - c2 // T2 * T2) & 3
    return pos, batch, cats, align


def groups_of(sel, cats, align):
    """{group: positions within sel}: the four alignment classes and the placed categories; every one populated."""
    where = {r: i for i, r in enumerate(sel)}
    groups = {}
    for a in range(4):
        groups["align%d" % a] = np.flatnonzero(align[sel] == a)
        assert len(groups["align%d" % a]) >= 30, (a, len(groups["align%d" % a]))
    for name, rows in cats.items():
        groups[name] = np.array([where[r] for r in rows])
        assert len(groups[name]) >= 8, (name, len(groups[name]))
    return groups


def check(label, got, want, groups, tol):
    """Relative L2 over all rows and over every group against the group's own norm, all below tol; prints every figure."""
    got = np.asarray(got, dtype=np.float64).reshape(len(want), -1)
    want = np.asarray(want).reshape(len(want), -1)
    figures = {"all": rel(got, want)}
    for name, idx in groups.items():
        figures[name] = rel(got[idx], want[idx])
    print("  %-9s tol %.1e  " % (label, tol) + "  ".join("%s %.2e" % kv for kv in figures.items()))
    bad = {k: f for k, f in figures.items() if not f < tol}
    assert not bad, (label, tol, bad)


def real_view(t):
    return host(torch.view_as_real(t)).reshape(t.shape[0], -1)


@pytest.mark.parametrize("geometry,m", GEOMETRIES, ids=["%s-m%d" % gm for gm in GEOMETRIES])
def test_gather_width(tn, geometry, m):
    d, N, n, wide, n1 = SHAPES[geometry]
    W = 2 * m + 2
    rng = np.random.default_rng(1000 * d + 100 * wide + m)
    pos, batch, cats, align = make_points(rng, d, N, m, n, wide, n1)
    if n * W ** d <= ALL_TAPS:
        sel = np.arange(n)
    else:
        placed = np.concatenate(list(cats.values()))
        sel = np.union1d(rng.choice(n, SUBSET, replace=False), placed)
    groups = groups_of(sel, cats, align)
    print("%s m = %d: tile (TC, T1, T2) = %s, %d of %d points compared" % (geometry, m, tiling(d, N, m, wide), len(sel), n))

    shape = (B,) + (N,) * d + (COLS,)
    xhat = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    w = rng.standard_normal((n, 2 * COLS)).astype(np.float32)
    v = rng.standard_normal((n, d)).astype(np.float32)
    post, batcht, xhatt, wt = dev(pos), dev(batch), dev(xhat), dev(w)
    g = ref1.grid_of(xhat, d, m)  # float64 grid, shared by the gradient and the HVP leg

    # gradient
    dp = tn.ops.nfft_forward_grad_points(post, xhatt, batcht, m, False, wt)
    assert dp.shape == (n, d) and dp.dtype == torch.float32 and bool(torch.isfinite(dp).all())
    check("grad", host(dp)[sel], ref1.grad_gather(g, pos[sel], batch[sel], m, False, w[sel]), groups, TR)

    # HVP
    dxh, dw, dp2 = tn.ops.nfft_forward_grad_points_backward(post, xhatt, batcht, m, False, wt, dev(v), False, True, True)
    assert dxh.numel() == 0 and dw.shape == (n, 2 * COLS) and dp2.shape == (n, d)
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(dp2).all())
    rdw, rdp = ref2.hvp_gather(g, pos[sel], batch[sel], m, False, w[sel], v[sel])
    check("hvp dw", host(dw)[sel], rdw, groups, TR2)
    check("hvp dpos", host(dp2)[sel], rdp, groups, TR2)
    del g

    # value + gradient: the fastsum backward at the sources
    tgt = (rng.random((NT, d)) - 0.5).astype(np.float32)
    tb = np.concatenate([np.zeros(NT - NT // 3, np.int64), np.ones(NT // 3, np.int64)])
    x = (rng.standard_normal((n, COLS)) + 1j * rng.standard_normal((n, COLS))).astype(np.complex64)
    dy = (rng.standard_normal((NT, COLS)) + 1j * rng.standard_normal((NT, COLS))).astype(np.complex64)
    coeffs = rng.standard_normal((N,) * d).astype(np.float32)  # real, not even
    dx, ds, dt = tn.ops.nfft_fastsum_backward(post, dev(tgt), dev(x), dev(dy), dev(coeffs), None, batcht, dev(tb), m,
                                              True, True, False)
    assert dt.numel() == 0 and dx.shape == (n, COLS) and dx.dtype == torch.complex64 and ds.shape == (n, d)
    assert bool(torch.isfinite(torch.view_as_real(dx)).all()) and bool(torch.isfinite(ds).all())
    H = nfft_ref.nfft_adjoint(dy, tgt, tb, N=N, m=m) * np.conj(coeffs.astype(np.complex128)).reshape((1,) + coeffs.shape + (1,))
    gH = ref1.grid_of(H, d, m)
    check("fs dsrc", host(ds)[sel], ref1.grad_gather(gH, pos[sel], batch[sel], m, False, ref1.real_columns(x, n)[sel]),
          groups, TRF)
    rdx = np.zeros((len(sel), 2 * COLS))
    for b in range(B):
        of_set = batch[sel] == b
        rdx[of_set] = ref1.interp_f64(gH[b:b + 1], pos[sel][of_set], m, False)
    check("fs dx", real_view(dx)[sel], rdx, groups, TRF)
    tn.ops.check_status()
