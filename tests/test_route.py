"""The route query for tests, nfft_dbg_route (csrc/api.hip; torch_nfft_amd._lib.route), without a GPU: plan_route is host
code, and without a device device_cu_count() falls back to 256 CUs, the MI355X's count.

Pinned here: the route of every leg of tests/test_gpu_value_widths.py at every width under the leg's environment (the
switches are read once per process, so every environment is one child that evaluates all its legs; the leg table is
tests/value_width_legs.py, which imports nothing), and the routes of the
tests of tests/test_gpu_parity.py that name a tiling or a point-side kernel of the 64^3 grid -- api.hip prefer_narrow sends
that grid to the narrow tiling for m <= 3 or at most 30 000 points, where no matrix-core kernel runs, which is why those
tests moved to N = 40 (or set NFFT_HIP_SMALL_NARROW=0 in their child).

Also pinned: the FFT-stage record nfft_dbg_fft_route (torch_nfft_amd._lib.fft_route) -- make_route without rocFFT's
work-area query, so host code as well -- one line per FFT route and column-pass tile width that
tests/test_gpu_fft_stage.py runs, the 2-D plane-count thresholds of the tile width at every M included.
"""
import json
import os
import subprocess
import sys

import pytest

from torch_nfft_amd import _lib
from value_width_legs import GEOMETRY, LEGS, POINT_SETS, env_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (NFFT_HIP_WORK_LIST changes no route: the listed legs are evaluated with the others of their environment)
ENVIRONMENTS = sorted({env_key({k: v for k, v in LEGS[leg][0].items() if k != "NFFT_HIP_WORK_LIST"}) for leg in LEGS})


def route(d, n, C, nsets, N, m, Cr):
    return _lib.route(_lib.Problem(d, n, C, nsets, N, m), Cr)


def leg_routes(key):
    """[(leg, m, Cr, route fields, expected fields)] of the legs whose environment (without the work-list switch) is key."""
    rows = []
    for leg, (env, _, geometry, crs, widths, expect, _, _) in LEGS.items():
        if env_key({k: v for k, v in env.items() if k != "NFFT_HIP_WORK_LIST"}) != key:
            continue
        d, N, n = GEOMETRY[geometry]
        for m in widths:
            for Cr in crs:
                rows.append((leg, m, Cr, route(d, n, Cr, POINT_SETS, N, m, Cr)._asdict(), expect))
    return rows


@pytest.mark.parametrize("key", ENVIRONMENTS, ids=[k or "default" for k in ENVIRONMENTS])
def test_value_width_legs_reach_their_kernels(key):
    if key:
        code = ("import json, sys; sys.path[:0] = [%r, %r]; import test_route as t; "
                "print('ROWS ' + json.dumps(t.leg_routes(%r)))") % (ROOT, os.path.join(ROOT, "tests"), key)
        env = dict(os.environ, **dict(kv.split("=") for kv in key.split()))
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        rows = json.loads([l for l in out.stdout.splitlines() if l.startswith("ROWS ")][0][5:])
    else:
        rows = leg_routes(key)
    assert rows
    for leg, m, Cr, got, expect in rows:
        assert {k: got[k] for k in expect} == expect, (leg, m, Cr, got)


def test_register_tiles_stop_at_cutoff_7():
    """spread_reg_supported admits m + 1 <= 8 cells of reach: under NFFT_HIP_SPREAD=reg the cutoff 8 takes spread_kernel."""
    d, N, n = GEOMETRY["narrow3d"]
    code = ("import sys; sys.path.insert(0, %r); from torch_nfft_amd import _lib; "
            "print('SPREAD', [_lib.route(_lib.Problem(%d, %d, 2, 2, %d, m), 2).spread for m in (7, 8)])") % (ROOT, d, n, N)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NFFT_HIP_SPREAD="reg"), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and "SPREAD ['reg', 'lds']" in out.stdout, out.stdout[-500:] + out.stderr[-2000:]


def test_the_64_cubed_grid_is_narrow_for_few_points_or_narrow_windows():
    """api.hip prefer_narrow, and what the four tests of test_gpu_parity.py ran on before they were moved."""
    for m in range(1, 8):
        assert not route(3, 9003, 5, 4, 32, m, 10).wide                       # test_forward_many_columns_wave_per_column
        assert not route(3, 347, 2, 5, 32, m, 4).wide                         # test_edge_cases_wide_tiling
        assert route(3, 30001, 1, 1, 32, m, 1).wide == (m > 3)
        assert route(3, 30001, 1, 1, 32, m, 1).spread == ("mfma" if m > 3 else "lds")
    assert not route(3, 6000, 1, 1500, 32, 3, 1).wide                         # test_many_small_point_sets_wide_tiling
    for m in (1, 2, 5, 7):
        assert route(3, 3000, 2, 1, 32, m, 4).gather == "lanes"               # test_streamed_gather_and_column_groups_...
    assert not route(3, 9003, 5, 4, 32, 8, 10).wide and route(3, 10 ** 6, 1, 1, 32, 8, 1).gather == "lanes"  # (W = 18)


def test_the_moved_tests_reach_the_wide_tiling():
    """The same problems at N = 40 (M = 80: the smallest grid beyond the special case): wide tiling, matrix-core spreading,
    the wave-per-column gather from 4 real planes up and the plane-ring kernel below."""
    for C, complex_out, m in [(5, True, 4), (3, False, 4), (9, False, 4), (4, True, 4), (6, False, 2), (4, False, 6), (2, True, 7)]:
        Cr = C * (2 if complex_out else 1)
        r = route(3, 9003, C, 4, 40, m, Cr)
        assert r.wide and r.gather == ("cols" if Cr >= 4 else "ring"), (C, complex_out, m, r)
    for m in (4, 2, 7):
        r = route(3, 347, 2, 5, 40, m, 4)
        assert r.wide and r.spread == "mfma" and r.gather == "cols", r
    r = route(3, 6000, 1, 1500, 40, 3, 2)
    assert r.wide and r.spread == "mfma" and r.gather == "ring" and not r.owned, r


def test_route_rejects_what_validate_rejects():
    with pytest.raises(RuntimeError):
        _lib.route(_lib.Problem(4, 10, 1, 1, 16, 3), 1)
    with pytest.raises(RuntimeError):
        _lib.route(_lib.Problem(3, 10, 1, 1, 16, 9), 1)
    r = route(1, 600, 2, 2, 64, 4, 2)
    assert r.small_grid and not r.wide and r.spread == "lds" and r.gather == "lanes" and r.x_through_plan  # (1-D, few taps)
    assert not route(3, 3000, 2, 2, 64, 4, 2).small_grid


def fft_route(d, N, B, C, adjoint, x_is_complex, real_output, chunk_np=0):
    return _lib.fft_route(_lib.Problem(d, 0, C, B, N, 4), adjoint, x_is_complex, real_output, chunk_np)


# (d, N, B, C, x complex) -> fft, then the tile widths (adjoint axis 1, adjoint axis 0, forward) and the launches that take a
# compile-time instantiation (col_dispatch: M = 512 at 8 and 4 columns)
FFT_ROUTES = [
    ((1, 8, 2, 3, True), "full", (0, 0, 0), (False, False, False)),
    ((1, 4096, 2, 3, False), "full", (0, 0, 0), (False, False, False)),
    ((2, 8, 2, 3, True), "full", (0, 0, 0), (False, False, False)),
    ((2, 32, 2, 3, True), "full", (0, 0, 0), (False, False, False)),      # M = 64: below the 2-D column pass
    ((3, 12, 2, 3, True), "full", (0, 0, 0), (False, False, False)),      # M = 24: no power of two
    ((3, 8, 1, 1, True), "roc_rows", (16, 16, 16), (False, False, False)),
    ((3, 32, 2, 3, False), "roc_rows", (16, 16, 16), (False, False, False)),
    ((3, 64, 1, 1, True), "own_planar", (16, 16, 16), (False, False, False)),
    ((3, 128, 1, 1, False), "own_planar", (16, 16, 16), (False, False, False)),
    ((3, 128, 1, 1, True), "own_planar", (16, 8, 16), (False, False, False)),   # two tile buffers of 256 x 16 exceed 32 KB
    ((3, 256, 1, 1, False), "own_planar", (8, 8, 8), (True, True, True)),
    ((3, 256, 1, 1, True), "own_planar", (8, 4, 8), (True, True, True)),
    ((3, 512, 1, 1, False), "own_planar", (8, 8, 8), (False, False, False)),
    ((3, 512, 1, 1, True), "own_planar", (8, 4, 8), (False, False, False)),
]


@pytest.mark.parametrize("shape,fft,nc,special", FFT_ROUTES, ids=["%dd-N%d-B%d-C%d-%s" % (s[0][:4] + ("cx" if s[0][4] else "re",))
                                                                   for s in FFT_ROUTES])
def test_fft_route_record(shape, fft, nc, special, monkeypatch):
    monkeypatch.delenv("NFFT_HIP_CHUNK_BYTES", raising=False)
    monkeypatch.delenv("NFFT_HIP_NO_COLFFT", raising=False)
    d, N, B, C, cx = shape
    a = fft_route(d, N, B, C, True, cx, False)
    f = fft_route(d, N, B, C, False, True, not cx)
    planes = B * C * (2 if cx else 1)
    for r in (a, f):
        assert (r.fft, r.chunk_fft, r.ci, r.total_planes, r.chunk_planes) == (fft, fft, C > 1 and d == 3 and N >= 64, planes, planes), r
    assert (a.nc_axis1, a.nc_axis0, a.nc_forward) == (nc[0], nc[1], 0) and a.specialised == (special[0], special[1], False), a
    assert (f.nc_axis1, f.nc_axis0, f.nc_forward) == (0, 0, nc[2]) and f.specialised == (False, False, special[2]), f


def test_fft_route_2d_tile_width_thresholds(monkeypatch):
    """make_col_geom narrows the 2-D tile from 16 columns (8 at M >= 512, or with two tile buffers at M = 256; 4 with two at
    M >= 512) down to 4 until (column tiles) x (launch planes) reaches 64.  A launch plane is a column in the adjoint pass
    and a real plane in the forward pass."""
    monkeypatch.delenv("NFFT_HIP_CHUNK_BYTES", raising=False)
    monkeypatch.delenv("NFFT_HIP_NO_COLFFT", raising=False)
    # N: [(first launch-plane count, tile width)] with one tile buffer
    one = {64: [(1, 4), (13, 8), (22, 16)], 128: [(1, 4), (8, 8), (13, 16)], 256: [(1, 4), (4, 8)], 512: [(1, 4), (2, 8)]}
    two = {64: [(1, 4), (13, 8), (22, 16)], 128: [(1, 4), (8, 8)], 256: [(1, 4)], 512: [(1, 4)]}

    def width(table, planes):
        return [w for first, w in table if first <= planes][-1]

    for N in one:
        for K in range(1, 40):
            r = fft_route(2, N, K, 1, True, False, False)
            assert (r.fft, r.chunk_fft, r.nc_axis1, r.nc_axis0) == ("own_planar", "own_planar", 0, width(one[N], K)), (N, K, r)
            r = fft_route(2, N, K, 1, True, True, False)
            assert (r.total_planes, r.nc_axis0) == (2 * K, width(two[N], K)), (N, K, r)
            r = fft_route(2, N, K, 1, False, True, True)
            assert (r.total_planes, r.nc_forward) == (K, width(one[N], K)), (N, K, r)
            r = fft_route(2, N, K, 1, False, True, False)
            assert (r.total_planes, r.nc_forward) == (2 * K, width(one[N], 2 * K)), (N, K, r)
            # (M = 512: logNC 3 and 2 are the compile-time instantiations)
            assert r.specialised == (False, False, N == 256), (N, K, r)
    assert [fft_route(2, 64, K, 1, True, False, False).nc_axis0 for K in (12, 13, 21, 22)] == [4, 8, 8, 16]


def test_fft_route_column_innermost_chunks(monkeypatch):
    """Several columns on 3-D grids of M = 128 .. 1024: chunks of >= 32 planes go column-innermost, 16 planes per tile."""
    monkeypatch.delenv("NFFT_HIP_NO_COLFFT", raising=False)
    monkeypatch.delenv("NFFT_HIP_CHUNK_BYTES", raising=False)
    for N, B, C, cx in [(64, 1, 32, False), (64, 1, 16, True), (64, 3, 11, False), (64, 1, 47, False), (128, 5, 7, False)]:
        for adjoint in (True, False):
            r = fft_route(3, N, B, C, adjoint, cx if adjoint else True, False if adjoint else not cx)
            assert r.ci and r.fft == "own_planar" and r.chunk_fft == "own_ci" and r.chunk_planes == r.total_planes, r
            assert (r.nc_axis1, r.nc_axis0, r.nc_forward) == ((16, 16, 0) if adjoint else (0, 0, 16)), r
            assert r.specialised == (False, False, False), r
            # a remainder chunk of 31 planes is planar
            assert fft_route(3, N, B, C, adjoint, cx if adjoint else True, False if adjoint else not cx, 31).chunk_fft == "own_planar"
    assert not fft_route(3, 32, 1, 32, True, False, False).ci and not fft_route(2, 256, 1, 32, True, False, False).ci
    # N = 256: the default budget of 16 GiB holds 14 planes (512 MiB of grid, 0.58 GB of half spectrum and 0.15 GB of scratch
    # each): planar chunks.  Column-innermost chunks at M = 512 exist under a raised budget only.
    r = fft_route(3, 256, 1, 16, True, True, False)
    assert r.ci and (r.chunk_planes, r.total_planes, r.chunk_fft) == (14, 32, "own_planar") and r.specialised[:2] == (True, True), r
    monkeypatch.setenv("NFFT_HIP_CHUNK_BYTES", str(40 << 30))
    for adjoint, cx, ro in [(True, True, False), (True, False, True), (False, True, False), (False, True, True)]:
        r = fft_route(3, 256, 1, 16 if (cx if adjoint else not ro) else 32, adjoint, cx, ro)
        assert (r.chunk_planes, r.total_planes, r.chunk_fft) == (32, 32, "own_ci") and r.specialised == (False,) * 3, r
    # M = 1024: 32 planes need about 300 GB; a budget of 288 GB gives planar chunks
    monkeypatch.setenv("NFFT_HIP_CHUNK_BYTES", str(288 * 10 ** 9))
    r = fft_route(3, 512, 1, 16, True, True, False)
    assert r.ci and r.chunk_planes < 32 and r.chunk_fft == "own_planar", r


def test_fft_route_switch_and_budget(monkeypatch):
    monkeypatch.setenv("NFFT_HIP_NO_COLFFT", "1")
    for d, N in [(2, 64), (3, 32), (3, 64)]:
        r = fft_route(d, N, 2, 3, True, True, False)
        assert (r.fft, r.chunk_fft, r.nc_axis1, r.nc_axis0) == ("full", "full", 0, 0), r
    monkeypatch.delenv("NFFT_HIP_NO_COLFFT")
    # bytes per plane at N = 16 (M = 32): grid + half spectrum + column scratch (M (N + 1) rows of 12 kept columns, padded)
    M, align = 32, lambda v: (v + 255) // 256 * 256
    plane = M ** 3 * 4 + M * M * (M // 2 + 1) * 8 + align(M * 17 * 12 * 8) + align(M * 4)
    for budget, chunk in [(4 * plane + 8, 4), (5 * plane + 8, 4), (4 * plane - 8, 2), (1, 2)]:
        monkeypatch.setenv("NFFT_HIP_CHUNK_BYTES", str(budget))
        r = fft_route(3, 16, 2, 3, True, True, False)
        assert (r.fft, r.total_planes, r.chunk_planes) == ("roc_rows", 12, chunk), (budget, r)
    r = fft_route(3, 16, 2, 3, False, True, True)
    assert (r.total_planes, r.chunk_planes) == (6, 1), r
    with pytest.raises(RuntimeError):
        _lib.fft_route(_lib.Problem(4, 0, 1, 1, 16, 3), True, True, False)
