"""The legs of tests/test_gpu_value_widths.py as a table, without any import: tests/test_route.py pins their routes on a
machine without a GPU and must not depend on what the GPU test modules import.

leg: (environment, "spread" / "gather" / "both", geometry, real planes of each run, cutoffs, expected route fields of
torch_nfft_amd._lib.route, expected info[1] of nfft_dbg_work_list or None, name of the tolerance in tests/test_gpu_parity.py)
"""
# geometry: (d, N, n) of test_gpu_gather_widths.SHAPES (test_gpu_value_widths.py asserts that they agree)
GEOMETRY = {"1d": (1, 64, 600), "2d": (2, 48, 1500), "narrow3d": (3, 16, 2000), "wide3d": (3, 64, 3000)}
POINT_SETS = 2
STREAM = {"NFFT_HIP_STREAM_MIN": "1"}
LISTED = {"NFFT_HIP_WORK_LIST": "1"}

LEGS = {}
for _g in ("1d", "2d", "narrow3d"):
    LEGS["narrow-" + _g] = ({}, "both", _g, (2,), range(1, 9), dict(wide=False, spread="lds", gather="lanes"), None, "T1N")
_SCATTER = dict(wide=True, owned=False, pair=False, spread="mfma")
_RANGE = {
    "scatter": ({}, "spread", (1,), dict(_SCATTER, x_through_plan=True)),
    "scatter-cols": ({"NFFT_HIP_OWNED": "0"}, "spread", (3,), dict(_SCATTER, x_through_plan=False)),
    "owned-pair": ({}, "spread", (2, 3), dict(wide=True, owned=True, pair=True, spread="mfma")),
    "owned-single": ({"NFFT_HIP_OWNED": "1"}, "spread", (1,), dict(wide=True, owned=True, pair=False, spread="mfma",
                                                                     x_through_plan=True)),
    "ring": ({}, "gather", (2,), dict(wide=True, gather="ring")),
    "cols": ({}, "gather", (5,), dict(wide=True, gather="cols")),
    "stream3": (STREAM, "gather", (2,), dict(wide=True, gather="stream", column_groups=3)),
    "stream1": (dict(STREAM, NFFT_HIP_COLGROUPS="0"), "gather", (2,), dict(wide=True, gather="stream", column_groups=1)),
}
for _name, (_env, _kind, _crs, _route) in _RANGE.items():
    LEGS[_name] = (_env, _kind, "wide3d", _crs, range(1, 8), _route, 0, "T1W")
    LEGS[_name + "-listed"] = (dict(_env, **LISTED), _kind, "wide3d", _crs, range(1, 8), _route, 1, "T1W")
LEGS["lanes-wide"] = ({"NFFT_HIP_GATHER": "lds"}, "gather", "wide3d", (2,), range(1, 8), dict(wide=True, gather="lanes"), None, "T1W")
LEGS["reg"] = ({"NFFT_HIP_SPREAD": "reg"}, "spread", "narrow3d", (2,), range(1, 8),
               dict(wide=False, spread="reg", x_through_plan=False), None, "T1N")


def env_key(env):
    return " ".join("%s=%s" % kv for kv in sorted(env.items()))


# (ordered by environment, the default one first: the legs of a child process follow each other)
CASES = sorted([(leg, m) for leg in LEGS for m in LEGS[leg][4]], key=lambda c: env_key(LEGS[c[0]][0]))
