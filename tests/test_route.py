"""The route query for tests, nfft_dbg_route (csrc/api.hip; torch_nfft_amd._lib.route), without a GPU: plan_route is host
code, and without a device device_cu_count() falls back to 256 CUs, the MI355X's count.

Pinned here: the route of every leg of tests/test_gpu_value_widths.py at every width under the leg's environment (the
switches are read once per process, so every environment is one child that evaluates all its legs; the leg table is
tests/value_width_legs.py, which imports nothing), and the routes of the
tests of tests/test_gpu_parity.py that name a tiling or a point-side kernel of the 64^3 grid -- api.hip prefer_narrow sends
that grid to the narrow tiling for m <= 3 or at most 30 000 points, where no matrix-core kernel runs, which is why those
tests moved to N = 40 (or set NFFT_HIP_SMALL_NARROW=0 in their child).
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
