"""Which kernels do the GPU tests that name a tiling or a point-side kernel reach?  Evaluates csrc/api.hip plan_route through
the test entry nfft_dbg_route (torch_nfft_amd._lib.route) on each test's problem and prints the table of
profiles/r14_value_widths.md.  Host code only: runs without a GPU (256 CUs are assumed then, the MI355X's count).

    python scripts/route_audit.py            # the table; every environment is one child process
    python scripts/route_audit.py --fuzz     # the routes the 60 seeds of tests/test_gpu_fuzz.py reach

A row: test, claim, environment, problem (d, N, m, points, point sets, columns), real planes per point set of the call.
The rows restate the tests' shapes by hand and can fall behind them: what keeps a test on the kernel it names is the route
assertion inside the test (test_gpu_parity.py route_of, the workers of test_gpu_graded_items.py and
test_gpu_value_widths.py); this script is the survey that found where such assertions were missing.
"""
import collections
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SN0 = "NFFT_HIP_SMALL_NARROW=0"
ROWS = [
    # test_gpu_parity.py ------------------------------------------------------------------------------------------------
    ("parity::test_edge_cases_wide_tiling[32-4] (parent)", "matrix-core kernels", "", (3, 32, 4, 347, 5, 2), 4),
    ("parity::test_edge_cases_wide_tiling[32-2] (parent)", "matrix-core kernels", "", (3, 32, 2, 347, 5, 2), 4),
    ("parity::test_edge_cases_wide_tiling[40-4]", "matrix-core kernels", "", (3, 40, 4, 347, 5, 2), 4),
    ("parity::test_edge_cases_wide_tiling[40-2]", "matrix-core kernels", "", (3, 40, 2, 347, 5, 2), 4),
    ("parity::test_edge_cases_wide_tiling[40-7]", "matrix-core kernels", "", (3, 40, 7, 347, 5, 2), 4),
    ("parity::test_edge_cases_wide_tiling[64-5]", "matrix-core kernels", "", (3, 64, 5, 347, 5, 2), 4),
    ("parity::test_many_small_point_sets_wide_tiling (parent, N = 32)", "matrix-core kernels", "", (3, 32, 3, 6000, 1500, 1), 2),
    ("parity::test_many_small_point_sets_wide_tiling (N = 40)", "matrix-core kernels", "", (3, 40, 3, 6000, 1500, 1), 2),
    ("parity::test_forward_many_columns_wave_per_column (parent, N = 32, C = 5 complex)", "wave per column", "", (3, 32, 4, 9003, 4, 5), 10),
    ("parity::test_forward_many_columns_wave_per_column (N = 40, C = 5 complex)", "wave per column", "", (3, 40, 4, 9003, 4, 5), 10),
    ("parity::test_forward_many_columns_wave_per_column (N = 40, C = 3 real)", "below 4 planes: ring", "", (3, 40, 4, 9003, 4, 3), 3),
    ("parity::test_forward_many_columns_wave_per_column (N = 40, C = 2 complex, m = 7)", "wave per column", "", (3, 40, 7, 9003, 4, 2), 4),
    ("parity::test_streamed_gather_...[stream+groups] N = 32 m = 1 (parent), forward", "streamed gather", "NFFT_HIP_STREAM_MIN=1", (3, 32, 1, 3000, 1, 2), 4),
    ("parity::test_streamed_gather_...[stream+groups] N = 64 m = 4 (parent), forward", "streamed gather", "NFFT_HIP_STREAM_MIN=1", (3, 64, 4, 6000, 2, 2), 4),
    ("parity::test_streamed_gather_...[stream+groups] N = 32 m = 1, forward of 2 columns", "wave per column, column groups", "NFFT_HIP_STREAM_MIN=1 " + SN0, (3, 32, 1, 3000, 1, 2), 4),
    ("parity::test_streamed_gather_...[stream+groups] N = 32 m = 1, forward of 1 column", "streamed gather", "NFFT_HIP_STREAM_MIN=1 " + SN0, (3, 32, 1, 3000, 1, 1), 2),
    ("parity::test_streamed_gather_...[stream-nogroups] N = 32 m = 7, forward of 1 column", "streamed gather, no groups", "NFFT_HIP_COLGROUPS=0 NFFT_HIP_STREAM_MIN=1 " + SN0, (3, 32, 7, 2500, 1, 1), 2),
    ("parity::test_streamed_gather_...[separate-permutation] N = 64 m = 3, adjoint", "gather_rows + spreading", SN0, (3, 64, 3, 5000, 1, 3), 3),
    ("parity::test_owned_spreading_stage_tile_borders[4-2]", "owned pair", "", (3, 64, 4, 2080, 3, 2), 2),
    ("parity::test_owned_spreading_stage_tile_borders[4-1]", "owned single", "NFFT_HIP_OWNED=1", (3, 64, 4, 2080, 3, 1), 1),
    ("parity::test_scatter_spreading_stage_dense_128_cubed[scatter]", "scatter", "NFFT_HIP_OWNED=0", (3, 64, 4, 120000, 1, 2), 2),
    ("parity::test_round4_selection_switches_match_oracle[wide-64^3]", "wide 64^3", SN0, (3, 32, 3, 2000, 1, 1), 1),
    ("parity::test_register_tile_spreading_mode_is_deterministic", "register tiles", "NFFT_HIP_SPREAD=reg", (3, 16, 4, 3000, 1, 1), 1),
    ("parity::test_spread_stage_matches_oracle", "narrow stage", "", (3, 16, 4, 500, 2, 2), 2),
    ("parity::test_many_columns_column_innermost_passes[64-1-40]", "wave per column (m = 3)", "", (3, 64, 3, 3000, 1, 40), 40),
    ("stream_staging N = 32 m = 1", "streamed gather", "NFFT_HIP_STREAM_MIN=1 " + SN0, (3, 32, 1, 4000, 1, 1), 2),
    ("stream_staging N = 80 m = 4", "streamed gather", "NFFT_HIP_STREAM_MIN=1 " + SN0, (3, 80, 4, 4000, 1, 1), 2),
    # test_gpu_graded_items.py -------------------------------------------------------------------------------------------
    ("graded_items n64_m4_uniform adjoint", "scatter", "", (3, 64, 4, 60000, 1, 1), 1),
    ("graded_items n64_m4_uniform forward [stream]", "streamed gather", "NFFT_HIP_STREAM_MIN=1", (3, 64, 4, 60000, 1, 1), 2),
    ("graded_items n64_m2_pair adjoint", "owned pair", "", (3, 64, 2, 20000, 1, 2), 2),
    ("graded_items n64_m2_pair forward [stream]", "streamed gather", "NFFT_HIP_STREAM_MIN=1", (3, 64, 2, 20000, 1, 2), 4),
    ("graded_items n64_m2_pair forward, real output [stream]", "streamed gather", "NFFT_HIP_STREAM_MIN=1", (3, 64, 2, 20000, 1, 2), 2),
    ("graded_items n64_m4_two_sets forward [stream]", "streamed gather", "NFFT_HIP_STREAM_MIN=1", (3, 64, 4, 12500, 2, 2), 4),
    ("graded_items n64_m4_two_sets forward, real output [stream]", "streamed gather", "NFFT_HIP_STREAM_MIN=1", (3, 64, 4, 12500, 2, 2), 2),
    ("graded_items n64_m6 forward [default]", "ring", "", (3, 64, 6, 8000, 1, 1), 2),
    ("graded_items n64_m4_six_cols forward", "wave per column", "", (3, 64, 4, 5000, 1, 6), 12),
    ("graded_items n48_m4 forward [stream]", "streamed gather", "NFFT_HIP_STREAM_MIN=1", (3, 48, 4, 20000, 1, 1), 2),
    # test_gpu_large.py ----------------------------------------------------------------------------------------------------
    ("large::test_config_c3_3d_n256_m4_10m forward", "streamed gather", "", (3, 256, 4, 10 ** 7, 1, 1), 2),
    ("large::test_streamed_interpolation_clustered_8m", "streamed gather", "", (3, 128, 4, 8 * 10 ** 6, 1, 1), 2),
    ("large::test_streamed_interpolation_other_cutoffs[2-1]", "streamed gather", "", (3, 128, 2, 6 * 10 ** 6, 1, 1), 2),
    ("large::test_streamed_interpolation_other_cutoffs[5-1]", "streamed gather", "", (3, 128, 5, 6 * 10 ** 6, 1, 1), 2),
    ("large::test_streamed_interpolation_other_cutoffs[4-2]", "streamed gather", "", (3, 128, 4, 12 * 10 ** 6, 2, 1), 2),
    ("large::test_work_list_tickets_in_graph_replays[stream]", "scatter, streamed gather", "NFFT_HIP_OWNED=0", (3, 128, 4, 4 * 10 ** 6, 1, 1), 1),
    ("large::test_work_list_tickets_in_graph_replays[cols]", "scatter, wave per column", "NFFT_HIP_OWNED=0", (3, 128, 4, 4 * 10 ** 6, 1, 2), 4),
    ("large::test_work_list_tickets_in_graph_replays[ring]", "scatter, ring", "NFFT_HIP_GATHER=mfma NFFT_HIP_OWNED=0", (3, 128, 4, 4 * 10 ** 6, 1, 1), 1),
    ("large::test_c3_interpolation_stage_matches_float64_gather", "streamed gather", "", (3, 256, 4, 10 ** 7, 1, 1), 1),
    ("large::test_c3_spread_stage_subvolumes_match_float64_gridding", "scatter", "", (3, 256, 4, 10 ** 7, 1, 1), 1),
    ("large::test_config_c4_stated_shape_one_gpu_share adjoint (64 real columns)", "paired owned / wave per column", "", (3, 128, 4, 400000, 4, 64), 64),
    ("large::test_grid_2d_16384_squared", "narrow tiling", "", (2, 8192, 4, 200000, 1, 1), 1),
    # test_gpu_fastsum_routes.py -------------------------------------------------------------------------------------------
    ("fastsum_routes rocrows-3d-N32-C1-mfma, sources", "matrix-core spreading", "", (3, 32, 6, 31000, 1, 1), 2),
    ("fastsum_routes rocrows-3d-N32-C2, sources", "(narrow)", "", (3, 32, 6, 2000, 2, 2), 2),
]


def describe(r):
    tiling = ("wide" + (", owned pair" if r["pair"] else ", owned" if r["owned"] else "")) if r["wide"] else "narrow"
    return "%s; spread %s%s; gather %s%s%s" % (tiling, r["spread"], "" if r["x_through_plan"] else " behind gather_rows", r["gather"],
                                               ", 3 column groups" if r["column_groups"] == 3 else "",
                                               "; un-planned calls: one-kernel path" if r["small_grid"] else "")


def evaluate(env):
    from torch_nfft_amd import _lib
    out = []
    for name, claim, e, (d, N, m, n, nsets, C), Cr in ROWS:
        if e == env:
            out.append((name, claim, _lib.route(_lib.Problem(d, n, C, nsets, N, m), Cr)._asdict()))
    return out


def fuzz():
    import test_gpu_fuzz
    from torch_nfft_amd import _lib
    seen = collections.Counter()
    for seed in range(60):
        c = test_gpu_fuzz.draw_case(seed)
        C = 1
        for s in c["cols"]:
            C *= s
        complex_x = bool(c["x"].dtype.kind == "c")
        for kind, Cr in (("adjoint", C * (2 if complex_x else 1)), ("forward", C * (1 if c["real_fwd"] else 2))):
            r = _lib.route(_lib.Problem(c["d"], c["n"], C, c["B"], c["N"], c["m"]), Cr)
            what = "one-kernel small grid" if r.small_grid else describe(r._asdict()).split("; ")[0] + "; " + (
                "spread " + r.spread if kind == "adjoint" else "gather " + r.gather)
            seen["%s: %s" % (kind, what)] += 1
    for k in sorted(seen):
        print("%3d  %s" % (seen[k], k))


if __name__ == "__main__":
    if "--fuzz" in sys.argv:
        fuzz()
    elif "--child" in sys.argv:
        print("ROWS " + json.dumps(evaluate(sys.argv[sys.argv.index("--child") + 1])))
    else:
        results = {}
        for env in sorted({r[2] for r in ROWS}):
            child_env = dict(os.environ, **dict(kv.split("=") for kv in env.split()))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", env], env=child_env, capture_output=True,
                                 text=True, check=True)
            for name, claim, r in json.loads([l for l in out.stdout.splitlines() if l.startswith("ROWS ")][0][5:]):
                results[name] = (claim, r)
        print("| test | named route | environment | route of plan_route |\n|---|---|---|---|")
        for name, claim, env, _, Cr in ROWS:
            print("| %s | %s | %s | Cr = %d: %s |" % (name, claim, env or "default", Cr, describe(results[name][1])))
