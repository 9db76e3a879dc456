"""GPU tests of the edges of the pair kernels' frame (csrc/pair_frame.h) on every Ewald-type pair
kernel: cells that hold exactly 0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257 and 300 points, so that an item's second wave
turns on at 65, a cell is cut into two items at 129 and into three at 257, a streamed range takes a second LDS tile at 257 and
a third past 512; the same in a second point set behind an empty one (set0 != 0, item slots past the first set's); and for the
Yukawa kernels a second pass over the columns.  tests/pair_frame_ref.py builds the three layouts and tests/test_pair_frame_ref.py
asserts on the CPU that they reach these edges -- and that the older fixtures of the Yukawa and Lennard-Jones kernels reach
none of them.

Every op is compared with the float64 brute force of the same pair sum on the same float32 fractional positions
(rel_l2, for the reduced tensors rel_fro).  For the ops with an output per point the same error is taken again over the points
that each edge computes -- the lanes of an item's second wave, the last and partly idle item of a cut cell, the point set
behind the empty one, and the rest -- and each group meets the gate on its own: a wrong edge is not averaged away by 2000
right points.

Gates.  Each is 4 x the largest figure of the first device run of these cases, written beside it; a figure above 1e-4, or a
group far from the other groups of its op, would have been a bug to find, not a number to record.  Where another file has a
gate for the same op and quantity it is named beside the new one, with whether the counted cases keep it; the counted cells
give a point up to 2000 neighbours inside r_c where the older fixtures give a hundred, so the float32 sums are longer.
"""
import numpy as np
import pytest
import torch

import dipole_ref as dp
import dispersion_ref as dr
import dispersion_virial_ref as dv
import ewald_box_ref as eb
import ewald_ref as er
import ewald_step_ref as es
import ewald_virial_ref as ev
import lj_step_ref as lj
import pair_frame_ref as pf
import rpy_ref as rr
import stokeslet_ref as st
import yukawa_ref as yr
from conftest import rel_l2
from ewald_virial_ref import rel_fro
from test_gpu_lj_step import _coefficients

pytestmark = pytest.mark.gpu

# (op, quantity): 4 x the largest figure of the first device run over the op's cases, the four groups of points (or the two
# point sets) and, for Yukawa, the column passes included.  In brackets: that figure and where it stood, the range of the
# cases' figures over all points, and the older gate of the same op and quantity -- every counted case keeps it.
GATES = {
    ("yukawa_near", "value"): 1.9e-6,  # (4.669e-7: the last items of the cut cells, cube; 3.5e-7 .. 4.0e-7; test_gpu_yukawa 3.6e-6)
    ("yukawa_near", "field"): 1.8e-6,  # (4.309e-7: cube at lambda = 40; 3.7e-7 .. 4.2e-7; test_gpu_yukawa 4.0e-6)
    # (4.379e-7: one column of (5,) alone; 1.7e-7 .. 3.1e-7 over all columns; no older gate: this kernel was never
    # compared with a pair sum on its own)
    ("yukawa_virial_near", "seven"): 1.8e-6,
    ("lj_step_near", "F"): 1.8e-6,     # (4.374e-7: the last items of the cut cells, ragged; 4.0e-7 .. 4.1e-7; test_gpu_lj_step 2.0e-5)
    # (6.746e-6: T, one set -- charges of both signs: U_C is what is left of the +- q_i q_j w; 4.6e-7 .. 3.0e-6 on the others and
    # per point set; test_gpu_lj_step 1.5e-4)
    ("lj_step_near", "U_C"): 2.7e-5,
    ("lj_step_near", "U_LJ"): 2.0e-6,  # (4.851e-7: the cube; 3.6e-7 .. 4.9e-7; test_gpu_lj_step 6.9e-6)
    ("lj_step_near", "W"): 4.1e-7,     # (1.022e-7: T; 4.8e-8 .. 1.0e-7; test_gpu_lj_step 7.3e-6)
    ("ewald_near", "value"): 1.7e-6,   # (4.188e-7; test_gpu_ewald 6.4e-6)
    ("ewald_near", "field"): 1.7e-6,   # (4.144e-7; test_gpu_ewald 8.9e-6)
    ("ewald_near_box", "value"): 1.7e-6,  # (4.157e-7: T; test_gpu_ewald_box 2.0e-6)
    ("ewald_near_box", "field"): 1.7e-6,  # (4.109e-7: O; test_gpu_ewald_box 1.8e-6)
    ("dispersion_near", "value"): 1.7e-6,  # (4.042e-7; test_gpu_dispersion 6.6e-6)
    ("dispersion_near", "field"): 3.3e-6,  # (8.189e-7: the rest of the points, against 6.0e-7 .. 6.7e-7 of the edges' groups; 7.4e-6)
    ("dispersion_near_box", "value"): 1.6e-6,  # (3.860e-7: T; test_gpu_dispersion 6.6e-6)
    ("dispersion_near_box", "field"): 3.4e-6,  # (8.254e-7: the rest of the points in T, as in the cube; 6.4e-7 .. 7.1e-7; 7.4e-6)
    ("virial_near", "seven"): 1.4e-6,  # (3.270e-7: set 0 in T; 2.7e-7 .. 3.2e-7; test_gpu_ewald_virial 8.2e-6)
    ("dispersion_virial_near", "seven"): 4.9e-7,  # (1.223e-7: O; 7.7e-8 .. 1.2e-7; test_gpu_dispersion_virial 7.9e-7)
    ("step_near", "value"): 1.7e-6,    # (4.152e-7: O; the gates of test_gpu_ewald_box and test_gpu_ewald_virial, as above)
    ("step_near", "field"): 1.7e-6,    # (4.159e-7: T)
    ("step_near", "seven"): 2.2e-6,    # (5.450e-7: set 0 in T; 3.9e-7 .. 4.8e-7)
    # (the older gates of the next three ops are max(4 x a float32 emulation, test_gpu_ewald's 6.4e-6 or 8.9e-6): kept)
    ("dipole_near", "phi"): 1.7e-6,    # (4.024e-7: T; 3.8e-7 .. 4.0e-7)
    ("dipole_near", "E"): 1.9e-6,      # (4.646e-7: T; 4.3e-7 .. 4.5e-7)
    ("dipole_near", "T"): 2.3e-6,      # (5.576e-7: T; 4.9e-7 .. 5.2e-7)
    ("stokeslet_near", "u"): 1.7e-6,   # (4.138e-7: O; 3.9e-7 .. 4.0e-7)
    ("stokeslet_near", "G"): 1.7e-6,   # (4.248e-7: T; 4.1e-7 .. 4.2e-7)
    ("rpy_near", "u"): 1.7e-6,         # (4.152e-7: O; 3.9e-7 .. 4.0e-7)
    ("rpy_near", "G"): 1.8e-6,         # (4.335e-7: O; 4.0e-7 .. 4.1e-7)
}
# No group of points of any op stood further than a factor 1.4 from the op's other groups.
WHOLE_GATES = {  # the two public calls on the ragged layout in T, the same rule
    ("lj_step", "F"): 1.7e-6,     # (4.108e-7: the rest of the points; 3.4e-7 .. 3.8e-7 in the edges' groups; test_gpu_lj_step 5.1e-6)
    ("lj_step", "U_C"): 6.8e-6,   # (1.689e-6; test_gpu_lj_step 1.2e-5)
    ("lj_step", "U_LJ"): 1.6e-6,  # (3.999e-7; test_gpu_lj_step 1.5e-6: kept by the figure, not by this gate)
    ("lj_step", "W"): 9.6e-7,     # (2.388e-7; test_gpu_lj_step 1.2e-6)
    ("yukawa", "value"): 1.7e-6,  # (4.168e-7: the rest of the points; 3.7e-7 .. 4.0e-7; test_gpu_yukawa 4.5e-6)
    ("yukawa", "field"): 1.6e-6,  # (3.848e-7: the rest of the points; 3.5e-7 .. 3.8e-7; test_gpu_yukawa 2.0e-6)
}

BOXES = {"cube": None, "T": eb.T, "O": eb.O}
# (alpha, r_c) per grid for the Coulomb-type and for the dispersion-type weights: the splits of the older files
SPLIT = {"coulomb": {"grid3": (12.0, 0.3), "ragged3": (12.0, 0.3), "boxO": (14.0, 0.25)},
         "slow": {"grid3": (5.0, 0.3), "ragged3": (5.0, 0.3), "boxO": (6.0, 0.25)}}


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _six(A):
    A = np.eye(3) if A is None else A
    return [A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2]]


def _box6(A):
    return () if A is None else _six(A)


def _seven(UW):
    return es.seven(*UW)


def _matrix(six):
    M = np.zeros((six.shape[0], 3, 3) + six.shape[2:], six.dtype)
    for e, (a, b) in enumerate(dp.VOIGT):
        M[:, a, b] = M[:, b, a] = six[:, e]
    return M


# ---- the table: one row per op ----------------------------------------------------------------------------------------
# inputs(rng, L, A) -> a dict of float32 arrays; run(tn, s, b, A, x, alpha, r_c) -> device tensors; parts(outputs as numpy)
# -> {quantity: array}, those in POINT per point, the others per point set; ref(L, A, x, alpha, r_c) -> the same in float64

COLS = (2,)


def _normal(rng, L, A):
    return {"x": rng.standard_normal((L.n,) + COLS).astype(np.float32)}


def _positive(rng, L, A):
    return {"x": dv.values(rng, L.n, COLS)}


def _ref_vf(near):
    def ref(L, A, x, alpha, r_c):
        z, f = near(x["x"], L.points, A, L.batch, alpha, r_c)
        return {"value": z, "field": f}
    return ref


def _cube_near(q, s, A, batch, alpha, r_c):
    assert A is None
    return er._near(q, s, batch, alpha, r_c)


def _rpy_radius(L, A):
    """half the lattice spacing: the closer of the nearest neighbours overlap (r < 2 a), nothing else does"""
    return 0.5 * pf.cartesian_spacing(L.cells, A)


def _lj_inputs(rng, L, A):
    A = np.eye(3) if A is None else A
    q, c, a = _coefficients(rng, L.n, A, spacing=pf.cartesian_spacing(L.cells, A))
    return {"x": np.stack([q, c, a], 1)}


def _lj_ref(L, A, x, alpha, r_c):
    A = np.eye(3) if A is None else A
    q, c, a = x["x"].T
    f, eight = lj.near_step(q, c, a, L.points, A, L.batch, alpha, alpha + 1.5, r_c)
    return {"F": f, "U_C": eight[:, 0], "U_LJ": eight[:, 1], "W": eight[:, 2:]}


def _step_ref(L, A, x, alpha, r_c):
    A = np.eye(3) if A is None else A
    z, f = eb._near(x["x"], L.points, A, L.batch, alpha, r_c)
    return {"value": z, "field": f, "seven": _seven(ev.near_virial(x["x"], L.points, A, L.batch, alpha, r_c))}


def _dipole_inputs(rng, L, A):
    return {"q": rng.standard_normal((L.n,) + COLS).astype(np.float32), "mu": rng.standard_normal((L.n, 3) + COLS).astype(np.float32)}


def _dipole_parts(o):
    return {"phi": o[0][:, 0], "E": o[0][:, 1:4], "T": _matrix(o[0][:, 4:])}


def _forces(rng, L, A):
    return {"x": rng.standard_normal((L.n, 3) + COLS).astype(np.float32)}


def _ug_parts(o):
    return {"u": o[0][:, :3], "G": o[0][:, 3:].reshape((o[0].shape[0], 3, 3) + o[0].shape[2:])}


OPS = {
    "ewald_near": dict(  # the unit cube
        kind="coulomb", boxes=("cube",), inputs=_normal, point=("value", "field"),
        run=lambda tn, s, b, A, x, al, rc, **kw: tn.ops.nfft_ewald_near(s, x["x"], b, al, rc, True),
        parts=lambda o: {"value": o[0], "field": o[1]}, ref=_ref_vf(_cube_near)),
    "ewald_near_box": dict(
        kind="coulomb", boxes=("T", "O"), inputs=_normal, point=("value", "field"),
        run=lambda tn, s, b, A, x, al, rc, **kw: tn.ops.nfft_ewald_near_box(s, x["x"], b, _six(A), al, rc, True),
        parts=lambda o: {"value": o[0], "field": o[1]}, ref=_ref_vf(eb._near)),
    "dispersion_near": dict(
        kind="slow", boxes=("cube",), inputs=_positive, point=("value", "field"),
        run=lambda tn, s, b, A, x, al, rc, **kw: tn.ops.nfft_ewald_dispersion_near(s, x["x"], b, al, rc, True),
        parts=lambda o: {"value": o[0], "field": o[1]}, ref=_ref_vf(dr._near)),
    "dispersion_near_box": dict(
        kind="slow", boxes=("T", "O"), inputs=_positive, point=("value", "field"),
        run=lambda tn, s, b, A, x, al, rc, **kw: tn.ops.nfft_ewald_dispersion_near_box(s, x["x"], b, _six(A), al, rc, True),
        parts=lambda o: {"value": o[0], "field": o[1]}, ref=_ref_vf(dr._near)),
    "virial_near": dict(
        kind="coulomb", boxes=("T", "O"), inputs=_normal, point=(),
        run=lambda tn, s, b, A, x, al, rc, **kw: (tn.ops.nfft_ewald_virial_near(s, x["x"], b, _six(A), al, rc),),
        parts=lambda o: {"seven": o[0]},
        ref=lambda L, A, x, al, rc: {"seven": _seven(ev.near_virial(x["x"], L.points, A, L.batch, al, rc))}),
    "dispersion_virial_near": dict(
        kind="slow", boxes=("T", "O"), inputs=_positive, point=(),
        run=lambda tn, s, b, A, x, al, rc, **kw: (tn.ops.nfft_ewald_dispersion_virial_near(s, x["x"], b, _six(A), al, rc),),
        parts=lambda o: {"seven": o[0]},
        ref=lambda L, A, x, al, rc: {"seven": _seven(dv.near_virial(x["x"], L.points, A, L.batch, al, rc))}),
    "step_near": dict(
        kind="coulomb", boxes=("T", "O"), inputs=_normal, point=("value", "field"),
        run=lambda tn, s, b, A, x, al, rc, **kw: tn.ops.nfft_ewald_step_near(s, x["x"], b, _six(A), al, rc),
        parts=lambda o: {"value": o[0], "field": o[1], "seven": o[2]}, ref=_step_ref),
    "lj_step_near": dict(
        kind="coulomb", boxes=("cube", "T", "O"), inputs=_lj_inputs, point=("F",),
        run=lambda tn, s, b, A, x, al, rc, **kw: tn.ops.nfft_ewald_lj_step_near(s, x["x"], b, _six(A), al, al + 1.5, rc),
        parts=lambda o: {"F": o[0], "U_C": o[1][:, 0], "U_LJ": o[1][:, 1], "W": o[1][:, 2:]}, ref=_lj_ref),
    "dipole_near": dict(  # order 2
        kind="slow", boxes=("T", "O"), inputs=_dipole_inputs, point=("phi", "E", "T"),
        run=lambda tn, s, b, A, x, al, rc, **kw: (tn.ops.nfft_ewald_dipole_near(
            s, torch.cat([x["q"][:, None], x["mu"]], 1), b, _box6(A), al, rc, 2),),
        parts=_dipole_parts,
        ref=lambda L, A, x, al, rc: dict(zip(("phi", "E", "T"), dp.near(x["q"], x["mu"], L.points, A, L.batch, al, rc, 2)))),
    "stokeslet_near": dict(  # order 2
        kind="slow", boxes=("T", "O"), inputs=_forces, point=("u", "G"),
        run=lambda tn, s, b, A, x, al, rc, **kw: (tn.ops.nfft_ewald_stokeslet_near(s, x["x"], b, _box6(A), al, rc, 2),),
        parts=_ug_parts,
        ref=lambda L, A, x, al, rc: dict(zip(("u", "G"), st.near(x["x"], L.points, A, L.batch, al, rc, 2)))),
    "rpy_near": dict(  # order 2
        kind="slow", boxes=("T", "O"), inputs=_forces, point=("u", "G"),
        run=lambda tn, s, b, A, x, al, rc, radius=None, **kw: (tn.ops.nfft_ewald_rpy_near(s, x["x"], b, _box6(A), al, rc, radius, 2),),
        parts=_ug_parts,
        ref=lambda L, A, x, al, rc, radius=None: dict(zip(("u", "G"), rr.near(x["x"], L.points, A, L.batch, al, rc, radius, 2)))),
    "yukawa_near": dict(
        kind="slow", boxes=("cube", "T", "O"), inputs=_normal, point=("value", "field"),
        run=lambda tn, s, b, A, x, al, rc, lam=10.0, **kw: tn.ops.nfft_ewald_yukawa_near(s, x["x"], b, _box6(A), al, rc, lam, True),
        parts=lambda o: {"value": o[0], "field": o[1]},
        ref=lambda L, A, x, al, rc, lam=10.0: dict(zip(("value", "field"), yr._near(x["x"], L.points, A, L.batch, al, lam, rc)))),
    "yukawa_virial_near": dict(
        kind="slow", boxes=("cube", "T", "O"), inputs=_normal, point=(),
        run=lambda tn, s, b, A, x, al, rc, lam=10.0, **kw: (tn.ops.nfft_ewald_yukawa_virial_near(s, x["x"], b, _six(A), al, rc, lam),),
        parts=lambda o: {"seven": o[0]},
        ref=lambda L, A, x, al, rc, lam=10.0: {"seven": yr.near_virial(x["x"], L.points, A, L.batch, al, lam, rc)}),
}

# The Yukawa and Lennard-Jones ops, which had no crowded case, on all three layouts (the 3^3 grid in the cube and in T); the
# others on the ragged 3^3 layout (in T, the two cube-only ops in the cube) and on the cells (4, 5, 3) of O where they take a box
CASES = []
for _op in ("yukawa_near", "yukawa_virial_near", "lj_step_near"):
    CASES += [(_op, "grid3", "cube", {}), (_op, "grid3", "T", {}), (_op, "boxO", "O", {}), (_op, "ragged3", "T", {})]
CASES.append(("yukawa_near", "grid3", "cube", {"lam": 40.0}))
for _op in OPS:
    if _op not in ("yukawa_near", "yukawa_virial_near", "lj_step_near"):
        CASES += [(_op, "ragged3" if box != "O" else "boxO", box, {}) for box in OPS[_op]["boxes"]]

_CASE = {}


class Case:
    """the inputs and the float64 pair sums of one row of CASES, computed once and left unchanged"""

    def __init__(self, op, layout, box, extra):
        self.op, self.row, self.L, self.A = op, OPS[op], pf.layout(layout), BOXES[box]
        self.tag = "%s, %s in %s%s" % (op, layout, box, "".join(" %s=%g" % kv for kv in sorted(extra.items())))
        self.alpha, self.r_c = SPLIT[self.row["kind"]][layout]
        self.extra = dict(extra)
        if op == "rpy_near":
            self.extra["radius"] = _rpy_radius(self.L, self.A)
        rng = np.random.default_rng(sum(map(ord, op + layout + box)))
        self.x = self.row["inputs"](rng, self.L, self.A)
        self.ref = self.row["ref"](self.L, self.A, self.x, self.alpha, self.r_c, **self.extra)

    def run(self, tn):
        xd = {k: _cuda(v) for k, v in self.x.items()}
        out = self.row["run"](tn, _cuda(self.L.points), _cuda(self.L.batch), self.A, xd, self.alpha, self.r_c, **self.extra)
        tn.ops.check_status()
        return out


def _case(op, layout, box, extra):
    key = (op, layout, box, tuple(sorted(extra.items())))
    if key not in _CASE:
        _CASE[key] = Case(op, layout, box, extra)
    return _CASE[key]


def _groups(L):
    """the points by the edge that computes them"""
    second, last = pf.point_groups(L.points, L.batch, L.cells)
    behind = L.set_of() == 2
    groups = {"second wave": second, "last item of a cut cell": last}
    if behind.any():
        groups["set 2"] = behind
    groups["the rest"] = ~(second | last | behind)
    return groups


def _gate(op, what):
    return GATES[(op, what)]


@pytest.mark.parametrize("op,layout,box,extra", CASES, ids=["%s-%s-%s%s" % (c[0], c[1], c[2], "-lam40" if c[3] else "") for c in CASES])
def test_counted_cells_against_brute_force(op, layout, box, extra):
    import torch_nfft_amd as tn
    c = _case(op, layout, box, extra)
    L, row = c.L, c.row
    if box != "cube":
        assert tn.EwaldSplitting(c.alpha, c.r_c, 4, box=c.A).cells == L.cells
    else:
        assert tn.EwaldSplitting(c.alpha, c.r_c, 4).cells == L.cells
    if op == "rpy_near":  # some of the counted pairs overlap, most do not
        s64 = L.points[L.set_of() == 0].astype(np.float64)
        ds = s64[:400, None] - s64[None]
        r = np.linalg.norm((ds - np.rint(ds)) @ dr._box(c.A), axis=-1)
        below, inside = int(((r > 0) & (r < 2 * c.extra["radius"])).sum()), int(((r > 0) & (r < c.r_c)).sum())
        print("%s: a = %.4f, %d of the %d pairs of 400 points inside r_c overlap" % (c.tag, c.extra["radius"], below, inside))
        assert below >= 100 and below <= 0.05 * inside
    out, again = c.run(tn), c.run(tn)
    for a, b in zip(out, again):
        assert torch.equal(a, b)  # no atomics: the same bits
    got = row["parts"]([o.cpu().numpy() for o in out])
    assert set(got) == set(c.ref)
    groups = _groups(L)
    errors = {}
    for what, ref in c.ref.items():
        g = got[what]
        assert g.shape == ref.shape and np.isfinite(g).all(), (what, g.shape, ref.shape)
        assert g.dtype == (np.float32 if what in row["point"] else np.float64)  # (the reductions are float64)
        assert np.linalg.norm(ref) > 0
        if what in row["point"]:
            errors[what] = rel_l2(g, ref)
            per = {name: rel_l2(g[rows], ref[rows]) for name, rows in groups.items()}
            print("%s: %s rel_l2 %.3e; %s" % (c.tag, what, errors[what], ", ".join("%s (%d) %.3e" % (k, groups[k].sum(), v)
                                                                                   for k, v in per.items())))
            errors.update({(what, k): v for k, v in per.items()})
        else:
            if L.B == 3:
                assert not g[1].any()  # the empty point set: exact zeros
                assert g[0].any() and g[2].any()
                per = {"set %d" % b: rel_fro(g[b], ref[b]) for b in (0, 2)}
            else:
                per = {}
            errors[what] = rel_fro(g, ref)
            print("%s: %s rel_fro %.3e%s" % (c.tag, what, errors[what], "".join("; %s %.3e" % kv for kv in per.items())))
            errors.update({(what, k): v for k, v in per.items()})
    for key, err in errors.items():
        what = key if isinstance(key, str) else key[0]
        assert err <= _gate(op, what), (key, err, _gate(op, what))


# ---- the second pass over the columns (Yukawa), on the 3^3 layout in T ---------------------------------------------------

def _yukawa_columns(cols, complex_x):
    L = pf.layout("grid3")
    rng = np.random.default_rng(70 + cols[0] + complex_x)
    q = rng.standard_normal((L.n,) + cols)
    if complex_x:
        q = q + 1j * rng.standard_normal((L.n,) + cols)
    return L, q.astype(np.complex64 if complex_x else np.float32)


@pytest.mark.parametrize("cols,complex_x,field", [((5,), False, True), ((8,), False, True), ((3,), True, True), ((5,), False, False)])
def test_yukawa_sweep_column_passes(cols, complex_x, field):
    """more than four real columns: the col0 loop runs again over the same LDS -- (5,): one live column and three masked,
    (8,): a full second pass, complex (3,): six reals, two live -- and a pass does not depend on what follows it"""
    import torch_nfft_amd as tn
    L, q = _yukawa_columns(cols, complex_x)
    alpha, r_c = SPLIT["slow"]["grid3"]
    sd, qd = _cuda(L.points), _cuda(q)
    z, f = tn.ops.nfft_ewald_yukawa_near(sd, qd, None, _six(eb.T), alpha, r_c, 10.0, field)
    z2, f2 = tn.ops.nfft_ewald_yukawa_near(sd, qd, None, _six(eb.T), alpha, r_c, 10.0, field)
    tn.ops.check_status()
    dtype = torch.complex64 if complex_x else torch.float32
    assert z.shape == q.shape and z.dtype == dtype and torch.equal(z, z2) and torch.equal(f, f2)
    zref, fref = yr._near(q, L.points, eb.T, None, alpha, 10.0, r_c)
    z, f = z.cpu().numpy(), f.cpu().numpy()
    groups = _groups(L)
    C = cols[0]
    second_pass = slice(4, C) if not complex_x else slice(2, C)  # (a complex column is two reals)
    for what, g, ref in (("value", z, zref),) + ((("field", f, fref),) if field else ()):
        assert g.shape == ref.shape and np.isfinite(g.view(np.float32)).all()
        err, err2 = rel_l2(g, ref), rel_l2(g[..., second_pass], ref[..., second_pass])
        per = {k: rel_l2(g[rows], ref[rows]) for k, rows in groups.items()}
        print("yukawa_near, grid3 in T, cols=%s complex=%d field=%d: %s rel_l2 %.3e, second pass %.3e; %s"
              % (cols, complex_x, field, what, err, err2, ", ".join("%s %.3e" % kv for kv in per.items())))
        for e in [err, err2] + list(per.values()):
            assert e <= _gate("yukawa_near", what)
    if not field:
        assert f.size == 0
    if cols == (5,) and not complex_x:
        four = _cuda(np.ascontiguousarray(q[:, :4]))
        z4, f4 = tn.ops.nfft_ewald_yukawa_near(sd, four, None, _six(eb.T), alpha, r_c, 10.0, field)
        tn.ops.check_status()
        assert np.array_equal(z4.cpu().numpy(), z[:, :4])
        if field:
            assert np.array_equal(f4.cpu().numpy(), f[:, :, :4])


@pytest.mark.parametrize("cols", [(5,), (8,)])
def test_yukawa_virial_column_passes(cols):
    import torch_nfft_amd as tn
    L, q = _yukawa_columns(cols, False)
    alpha, r_c = SPLIT["slow"]["grid3"]
    sd = _cuda(L.points)
    out = tn.ops.nfft_ewald_yukawa_virial_near(sd, _cuda(q), None, _six(eb.T), alpha, r_c, 10.0)
    out2 = tn.ops.nfft_ewald_yukawa_virial_near(sd, _cuda(q), None, _six(eb.T), alpha, r_c, 10.0)
    tn.ops.check_status()
    assert out.shape == (1, 7) + cols and out.dtype == torch.float64 and torch.equal(out, out2)
    ref = yr.near_virial(q, L.points, eb.T, None, alpha, 10.0, r_c)
    out = out.cpu().numpy()
    assert np.isfinite(out).all() and out.all()
    err, err2 = rel_fro(out, ref), rel_fro(out[..., 4:], ref[..., 4:])
    worst = max(rel_fro(out[..., k], ref[..., k]) for k in range(cols[0]))
    print("yukawa_virial_near, grid3 in T, cols=%s: seven rel_fro %.3e, second pass %.3e, worst column %.3e" % (cols, err, err2, worst))
    assert max(err, err2, worst) <= _gate("yukawa_virial_near", "seven")
    if cols == (5,):
        four = tn.ops.nfft_ewald_yukawa_virial_near(sd, _cuda(np.ascontiguousarray(q[:, :4])), None, _six(eb.T), alpha, r_c, 10.0)
        tn.ops.check_status()
        assert np.array_equal(four.cpu().numpy(), out[..., :4])


# ---- the public calls on the ragged layout in T: the sort and the scatter through `index` of cut cells --------------------

WHOLE = (12.0, 13.0, 0.3, 32)  # alpha_C, alpha_D, r_c, N: WHOLE["T"] of tests/test_gpu_lj_step.py, the 3^3 grid in T


def _whole_gate(key):
    return WHOLE_GATES[key]


def _relative(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def test_whole_lj_step_on_the_ragged_layout():
    """nfft_ewald_lj_step, fractional input, against lj_step_ref.exact_lj_step"""
    import torch_nfft_amd as tn
    L, A = pf.layout("ragged3"), eb.T
    alpha_c, alpha_d, r_c, N = WHOLE
    spc, spd = tn.EwaldSplitting(alpha_c, r_c, N, box=A), tn.DispersionSplitting(alpha_d, r_c, N, box=A)
    assert spc.cells == L.cells
    q, c, a = _coefficients(np.random.default_rng(5), L.n, A, spacing=pf.cartesian_spacing(L.cells, A))
    got = tn.nfft_ewald_lj_step(_cuda(q), _cuda(c), _cuda(a), _cuda(L.points), _cuda(L.batch), coulomb=spc, dispersion=spd,
                                cutoff=4, fractional=True)
    tn.ops.check_status()
    F, UC, ULJ, W = (t.cpu().numpy().astype(np.float64) for t in got)
    assert F.shape == (L.n, 3) and UC.shape == ULJ.shape == (3,) and W.shape == (3, 3, 3) and np.isfinite(F).all()
    assert not UC[1] and not ULJ[1] and not W[1].any()  # the empty set
    ref = lj.exact_lj_step(q, c, a, L.points, A, L.batch, alpha_c, alpha_d, r_c, N)
    live = [0, 2]
    e = {"F": rel_l2(F, ref[0]), "U_C": _relative(UC[live], ref[1][live]), "U_LJ": _relative(ULJ[live], ref[2][live]),
         "W": rel_fro(W[live], ref[3][live])}
    per = {k: rel_l2(F[rows], ref[0][rows]) for k, rows in _groups(L).items()}
    print("nfft_ewald_lj_step, ragged3 in T: %s; F by group: %s" % (" ".join("%s %.3e" % kv for kv in sorted(e.items())),
                                                                  ", ".join("%s %.3e" % kv for kv in per.items())))
    for key, err in e.items():
        assert err <= _whole_gate(("lj_step", key)), (key, err)
    for key, err in per.items():
        assert err <= _whole_gate(("lj_step", "F")), (key, err)


def test_whole_yukawa_on_the_ragged_layout():
    """nfft_ewald_yukawa(field=True), lambda = 10, against yukawa_ref.yukawa.  The splitting is the Coulomb one of the
    Lennard-Jones whole call, (12, 0.3, 32): r_c = 0.25 of tests/test_gpu_yukawa.py would give T the cells (3, 4, 3), not the
    grid whose cells were counted.  Fractional input, as above: the round trip through float32 Cartesian positions moves the
    point on the face -1/2 into the cell across it."""
    import torch_nfft_amd as tn
    L, A = pf.layout("ragged3"), eb.T
    alpha, _, r_c, N = WHOLE
    sp = tn.YukawaSplitting(alpha, r_c, N, 10.0, box=torch.from_numpy(A))
    assert sp.cells == L.cells
    s = L.points
    q = np.random.default_rng(6).standard_normal(L.n).astype(np.float32)
    phi, E = tn.nfft_ewald_yukawa(_cuda(q), _cuda(s), _cuda(L.batch), splitting=sp, cutoff=4, field=True, fractional=True)
    tn.ops.check_status()
    phi, E = phi.cpu().numpy(), E.cpu().numpy()
    assert phi.shape == (L.n,) and E.shape == (L.n, 3) and np.isfinite(phi).all() and np.isfinite(E).all()
    pref, Eref = yr.yukawa(q, s, A, L.batch, alpha, 10.0, r_c, N)
    groups = _groups(L)
    for what, g, ref in (("value", phi, pref), ("field", E, Eref)):
        err = rel_l2(g, ref)
        per = {k: rel_l2(g[rows], ref[rows]) for k, rows in groups.items()}
        print("nfft_ewald_yukawa, ragged3 in T: %s rel_l2 %.3e; %s" % (what, err, ", ".join("%s %.3e" % kv for kv in per.items())))
        for e in [err] + list(per.values()):
            assert e <= _whole_gate(("yukawa", what)), (what, e)
