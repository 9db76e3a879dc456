"""GPU tests of the bonded-pair exclusions: the list kernel and the virial reduction of
csrc/ewald_excl.hip alone against the float64 formulas on the same wrapped float32 positions, and nfft_ewald,
nfft_ewald_dispersion, their energies, backwards and virials with `exclusions=` against tests/exclusions_ref.py.

Tolerances.  EXCL_TOL holds 4 x the largest rel_l2 of the first device run (the figure behind each entry is in its comment),
the project's convention; a first-run figure above 1e-4 would have been a defect.  A whole function is held to the smaller of
its entry and a ceiling that no run decides: the WHOLE_TOL of the same quantity in the tests of the sum without exclusions
plus the cancellation that remains -- the sweep's float32 accumulator has held w |x_j| K(r) of every listed pair before the
correction takes it out, which leaves 2^-24 |(sum_j w |x_j| K(r_ij))_i| / |result| (computed here from the inputs).

One list per geometry (exclusions_ref.bonded_list): chains (i, i + 1) at scale 0 and (i, i + 2) at Coulomb / dispersion scales
0.5 / 0.25 in both point sets, bonded at 0.02 .. 0.05, a hub with 20 partners, a pair across each face, a coincident pair,
and empty rows for everything else.  The float64 algorithm is evaluated once per geometry on two real columns; the other
column layouts and complex values are linear combinations of the two, and so are their references."""
import numpy as np
import pytest
import torch

import dispersion_ref as dr
import exclusions_ref as xr
from conftest import rel_l2
from ewald_box_ref import O, T

pytestmark = pytest.mark.gpu

BOXES = {"cube": None, "T": T, "O": O}
COULOMB_SPLIT = {"cube": (12.0, 0.3, 32), "T": (12.0, 0.3, 32), "O": (14.0, 0.25, 48)}  # (tests/test_gpu_ewald*.py)
DISPERSION_SPLIT = (14.0, 0.25, 32)  # (tests/test_gpu_dispersion.py)
SHIFT = np.array([3.0, -2.0, 1.0])  # lattice vectors

EXCL_TOL = {  # 4 x the largest rel_l2 of the first device run (in brackets)
    "list_value": 1.9e-6,  # (4.74e-7: 1 / r^6 in the cube, one column; 8.7e-8 .. 4.7e-7 on the sixty runs of the list kernel)
    "list_field": 1.9e-6,  # (4.72e-7: the same case; 1.8e-7 .. 4.7e-7)
    "virial": 1.7e-6,  # (4.13e-7: 1 / r^6 in O, three columns; 6.3e-8 .. 4.1e-7 on the twenty-four runs)
    "coulomb_value": 2.1e-6,  # (5.16e-7: T, three columns; dx of the backward 5.06e-7; 3.7e-7 .. 5.2e-7, the moved cases among them)
    "coulomb_field": 1.1e-6,  # (2.72e-7: T, three columns; 2.0e-7 .. 2.7e-7; dpos of the backward 2.3e-7 .. 2.6e-7)
    "dispersion_value": 1.3e-6,  # (3.06e-7: T moved, Cartesian; 1.1e-7 .. 3.1e-7)
    "dispersion_field": 1.7e-6,  # (4.22e-7: the same case; 1.4e-7 .. 4.2e-7)
    "coulomb_W": 1.7e-6,  # (4.17e-7 in T; 3.66e-7 in the cube, 3.30e-7 in O)
    "coulomb_U": 6.6e-6,  # (1.64e-6 in T; 1.57e-6 in O, 1.04e-6 in the cube)
    "dispersion_W": 4.7e-7,  # (1.17e-7 in the cube; 1.13e-7 in T, 1.07e-7 in O)
    "dispersion_U": 3.8e-7,  # (9.43e-8 in T; 8.2e-8 in the cube, 3.3e-8 in O)
}
# The cancellation terms of these lists: 7.9e-8 .. 9.5e-8 of |phi| and 7.2e-8 .. 7.6e-8 of |E| for the Coulomb sum, 2.4e-8 ..
# 2.5e-8 of |psi| and 2.1e-8 .. 2.2e-8 of |G| for the dispersion sum: a twentieth of the ceilings, which the entries above stay
# below anyway.  At the two ends of the tightest bond (r = 0.02) alone the device is off by the figures that
# test_coulomb_whole and test_dispersion_whole print beside 2^-24 |x_j| / r (DESIGN.md section 7o has them).

# column layouts as combinations of the two real reference columns: x = x2 @ M, and so is every linear result
MIX = {
    "()": np.array([[1.0], [0.5]]),
    "(2,)": np.eye(2),
    "(3,)": np.array([[1.0, 0.0, 1.0], [0.0, 1.0, -1.0]]),
    "(5,)": np.array([[1.0, 0.0, 1.0, 2.0, 0.0], [0.0, 1.0, -1.0, 0.0, -1.0]]),
    "complex": np.array([[1.0], [1.0j]]),
    "first": np.array([[1.0], [0.0]]),
    "second": np.array([[0.0], [1.0]]),
}
SCALAR = ("()", "complex", "first", "second")  # layouts without a column axis


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mix(a2, name):
    """the two reference columns (last axis) combined into the layout `name`; float32 / complex64 for inputs"""
    out = a2 @ MIX[name]
    return out[..., 0] if name in SCALAR else out


def _six(A):
    return () if A is None else [A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2]]


def _as_input(a):
    return a.astype(np.complex64 if np.iscomplexobj(a) else np.float32)


def _whole_tol(kind):
    if kind == "coulomb_cube":
        from test_gpu_ewald import WHOLE_TOL
    elif kind == "coulomb_box":
        from test_gpu_ewald_box import WHOLE_TOL
    elif kind == "dispersion":
        from test_gpu_dispersion import WHOLE_TOL
    elif kind == "coulomb_virial":
        from test_gpu_ewald_virial import WHOLE_TOL
    else:
        from test_gpu_dispersion_virial import WHOLE_TOL
    return WHOLE_TOL


def _wrapped(s):
    """the float32 positions as the operators reduce them: p - rint(p), and +1/2 is the point -1/2"""
    s = np.asarray(s, dtype=np.float32)
    red = s - np.rint(s)
    return np.where(red >= 0.5, red - np.float32(1.0), red).astype(np.float32)


class Case:
    """one geometry: fractional float32 points s (which the Cartesian float32 x = s A convert back to), two real columns,
    the list, and on request the float64 algorithm without the listed pairs"""

    def __init__(self, box, kind):
        self.box, self.kind, self.A = box, kind, BOXES[box]
        rng = np.random.default_rng(4)
        if kind == xr.COULOMB:
            n = 300
            s0 = (rng.random((n, 3)) - 0.5).astype(np.float32)
            self.batch = (np.arange(n) >= 140).astype(np.int64)
            self.x2 = rng.standard_normal((n, 2)).astype(np.float32)
            self.split = COULOMB_SPLIT[box]
        else:
            s0 = rng.permutation(dr.jittered_lattice(rng, 7, 1.0 / 7, 0.03).reshape(-1, 3))
            n = s0.shape[0]
            self.batch = (np.arange(n) >= 160).astype(np.int64)
            self.x2 = (rng.random((n, 2)) + 0.5).astype(np.float32)
            self.split = DISPERSION_SPLIT
        s0, self.pairs, self.sc, self.sd = xr.bonded_list(s0, self.A, self.batch, seed=5)
        if self.A is None:
            self.s, self.cart = s0, None
        else:
            self.cart = (s0.astype(np.float64) @ self.A).astype(np.float32)
            self.s = (self.cart.astype(np.float64) @ np.linalg.inv(self.A)).astype(np.float32)
        self.n = n
        self.w = 1.0 - (self.sc if kind == xr.COULOMB else self.sd)
        self._ref = self._virial = None

    def exclusions(self):
        import torch_nfft_amd as tn
        return tn.ExclusionList(self.pairs, self.n, coulomb_scale=self.sc, dispersion_scale=self.sd, batch=self.batch)

    def splitting(self):
        import torch_nfft_amd as tn
        cls = tn.EwaldSplitting if self.kind == xr.COULOMB else tn.DispersionSplitting
        return cls(*self.split, box=None if self.A is None else torch.from_numpy(self.A))

    def positions(self, fractional):
        return self.s if (self.A is None or fractional) else self.cart

    def ref(self, s=None):
        """(value [n, 2], field [n, 3, 2]) of the float64 algorithm without the listed pairs, on the float32 fractional points
        (other points `s`: evaluated there, and not kept)"""
        fn = xr.coulomb_algorithm if self.kind == xr.COULOMB else xr.dispersion_algorithm
        if s is not None:
            return fn(self.x2, s, self.A, self.batch, self.pairs, self.w, *self.split)
        if self._ref is None:
            self._ref = fn(self.x2, self.s, self.A, self.batch, self.pairs, self.w, *self.split)
        return self._ref

    def virial_ref(self):
        if self._virial is None:
            fn = xr.coulomb_virial_algorithm if self.kind == xr.COULOMB else xr.dispersion_virial_algorithm
            self._virial = fn(self.x2, self.s, self.A, self.batch, self.pairs, self.w, *self.split)
        return self._virial

    def cancellation(self, name):
        """2^-24 |(sum_j w |x_j| K(r_ij))_i| for the value and for the field: what the sweep's accumulator has rounded away"""
        z, f = xr.listed_terms(self.kind, np.abs(_mix(self.x2.astype(np.float64), name)), _wrapped(self.s), self.A, self.pairs,
                               self.w, self.split[0])
        d = xr.images(_wrapped(self.s), self.A, self.pairs)
        _, k1 = xr.kernels(self.kind, d, self.split[0])
        g = np.zeros((self.n,) + z.shape[1:])
        mag = (self.w * k1 * np.sqrt((d * d).sum(-1)))
        a = np.abs(_mix(self.x2.astype(np.float64), name))
        np.add.at(g, self.pairs[:, 0], mag.reshape((-1,) + (1,) * (a.ndim - 1)) * a[self.pairs[:, 1]])
        np.add.at(g, self.pairs[:, 1], mag.reshape((-1,) + (1,) * (a.ndim - 1)) * a[self.pairs[:, 0]])
        return 2.0 ** -24 * np.linalg.norm(z), 2.0 ** -24 * np.linalg.norm(g)


_CASES = {}


def _case(box, kind):
    if (box, kind) not in _CASES:
        _CASES[(box, kind)] = Case(box, kind)
    return _CASES[(box, kind)]


def _gate(entry, whole_tol, cancel, norm):
    ceiling = whole_tol + cancel / norm
    return min(EXCL_TOL[entry], ceiling), ceiling


def test_the_list_has_every_case():
    for kind in (xr.COULOMB, xr.DISPERSION):
        for box in BOXES:
            c = _case(box, kind)
            ex = c.exclusions()
            length = np.diff(ex.row_start.cpu().numpy())
            d = xr.images(_wrapped(c.s), c.A, c.pairs)
            r = np.sqrt((d * d).sum(-1))
            raw = np.abs(_wrapped(c.s)[c.pairs[:, 0]] - _wrapped(c.s)[c.pairs[:, 1]])
            print("%s kind %d: %d pairs, rows 0 .. %d, %d empty, r in [%.4f, %.4f], %d coincident, %d across a face"
                  % (box, kind, len(c.pairs), length.max(), int((length == 0).sum()), r[r > 0].min(), r.max(), int((r == 0).sum()),
                     int((raw > 0.5).any(1).sum())))
            assert length.max() >= 20 and (length == 0).sum() > 50 and (r == 0).sum() == 1
            assert 0.019 <= r[r > 0].min() <= 0.021 and r.max() < 0.12
            for a in range(3):
                assert (raw[:, a] > 0.5).any()  # a listed pair whose ends lie on opposite sides of this face
            assert len(np.unique(c.batch[c.pairs[:, 0]])) == 2


@pytest.mark.parametrize("box", ["cube", "T", "O"])
@pytest.mark.parametrize("field", [False, True])
@pytest.mark.parametrize("cols", ["()", "(2,)", "(3,)", "(5,)", "complex"])
def test_list_kernel_alone(box, field, cols):
    """both kinds of the list kernel against the float64 formulas on the same wrapped float32 positions; two calls give the
    same bits, and the value-only instantiation adds the same terms"""
    import torch_nfft_amd as tn
    c = _case(box, xr.COULOMB)
    ex = c.exclusions()
    x = _as_input(_mix(c.x2.astype(np.float64), cols))
    box6 = _six(c.A)
    for kind, weight, alpha in ((xr.COULOMB, ex.coulomb_weight, 12.0), (xr.DISPERSION, ex.dispersion_weight, 14.0)):
        args = (_cuda(c.s), _cuda(x), _cuda(c.batch), ex.row_start, ex.col, weight, box6, alpha, kind)
        z, f = tn.ops.nfft_ewald_excl(*args, field)
        z2, f2 = tn.ops.nfft_ewald_excl(*args, field)
        tn.ops.check_status()
        assert torch.equal(z, z2) and torch.equal(f, f2)
        assert z.shape == x.shape and z.dtype == (torch.complex64 if cols == "complex" else torch.float32)
        w = 1.0 - (c.sc if kind == xr.COULOMB else c.sd)
        zr, fr = xr.listed_terms(kind, x, _wrapped(c.s), c.A, c.pairs, w, alpha)
        e = rel_l2(z.cpu().numpy(), zr)
        print("list kernel %s kind %d cols %s field %d: value rel_l2 %.3e" % (box, kind, cols, field, e))
        assert e <= EXCL_TOL["list_value"]
        if field:
            assert f.shape == (c.n, 3) + x.shape[1:]
            e = rel_l2(f.cpu().numpy(), fr)
            print("list kernel %s kind %d cols %s: field rel_l2 %.3e" % (box, kind, cols, e))
            assert e <= EXCL_TOL["list_field"]
            assert torch.equal(tn.ops.nfft_ewald_excl(*args, False)[0], z)
        else:
            assert f.numel() == 0
        # the rows without a partner are exactly zero, and the r = 0 entry carries its constant
        empty = np.flatnonzero(np.diff(ex.row_start.cpu().numpy()) == 0)
        assert not z.cpu().numpy()[empty].any()


@pytest.mark.parametrize("box", ["cube", "T", "O"])
@pytest.mark.parametrize("cols", ["()", "(2,)", "(3,)", "(5,)"])
def test_virial_kernel_alone(box, cols):
    import torch_nfft_amd as tn
    c = _case(box, xr.COULOMB)
    ex = c.exclusions()
    x = _as_input(_mix(c.x2.astype(np.float64), cols))
    box6 = _six(np.eye(3) if c.A is None else c.A)
    for kind, weight, alpha in ((xr.COULOMB, ex.coulomb_weight, 12.0), (xr.DISPERSION, ex.dispersion_weight, 14.0)):
        args = (_cuda(c.s), _cuda(x), _cuda(c.batch), ex.row_start, ex.col, weight, box6, alpha, kind)
        out = tn.ops.nfft_ewald_excl_virial(*args)
        assert torch.equal(out, tn.ops.nfft_ewald_excl_virial(*args))
        tn.ops.check_status()
        assert out.shape == (2, 7) + x.shape[1:] and out.dtype == torch.float64
        w = 1.0 - (c.sc if kind == xr.COULOMB else c.sd)
        U, W = xr.listed_virial(kind, x, _wrapped(c.s), c.A, c.batch, c.pairs, w, alpha)
        want = np.stack([U, W[:, 0, 0], W[:, 1, 1], W[:, 2, 2], W[:, 1, 2], W[:, 0, 2], W[:, 0, 1]], 1)
        e = rel_l2(out.cpu().numpy(), want)
        print("virial kernel %s kind %d cols %s: rel_l2 %.3e" % (box, kind, cols, e))
        assert e <= EXCL_TOL["virial"]
        if cols == "()":  # one point set and no batch: the same pairs, added up over both sets
            one = tn.ops.nfft_ewald_excl_virial(args[0], args[1], None, *args[3:])
            assert one.shape == (1, 7) and rel_l2(one.cpu().numpy()[0], want.sum(0)) <= EXCL_TOL["virial"]


WHOLE_CASES = [("cube", False, "()", True), ("cube", False, "complex", False), ("T", True, "(3,)", True), ("T", False, "(2,)", True),
               ("O", True, "(5,)", False), ("O", False, "()", True)]


def _run_whole(kind, box, fractional, cols, field, shift=False):
    import torch_nfft_amd as tn
    c = _case(box, kind)
    fn, energy = ((tn.nfft_ewald, tn.nfft_ewald_energy) if kind == xr.COULOMB else
                  (tn.nfft_ewald_dispersion, tn.nfft_ewald_dispersion_energy))
    name = "coulomb" if kind == xr.COULOMB else "dispersion"
    tol = _whole_tol("dispersion" if kind == xr.DISPERSION else ("coulomb_cube" if c.A is None else "coulomb_box"))
    x = _as_input(_mix(c.x2.astype(np.float64), cols))
    pos = c.positions(fractional)
    seen = None
    if shift:  # the reference on the float32 fractional positions that the moved ones stand for
        lattice = SHIFT if (c.A is None or fractional) else SHIFT @ c.A
        pos = (pos.astype(np.float64) + lattice).astype(np.float32)
        seen = pos if (c.A is None or fractional) else (pos.astype(np.float64) @ np.linalg.inv(c.A)).astype(np.float32)
        assert np.abs(_wrapped(seen) - _wrapped(c.s)).max() > 0  # (the move has cost bits)
    kw = dict(splitting=c.splitting(), cutoff=4, exclusions=c.exclusions())
    if c.A is not None:
        kw["fractional"] = fractional
    out = fn(_cuda(x), _cuda(pos), _cuda(c.batch), field=field, **kw)
    tn.ops.check_status()
    phi, E = out if field else (out, None)
    ref = c.ref(seen)
    cv, cf = c.cancellation(cols)
    want = _mix(ref[0], cols)
    e = rel_l2(phi.cpu().numpy(), want)
    gate, ceiling = _gate(name + "_value", tol["value"], cv, np.linalg.norm(want))
    print("%s %s fractional %d cols %s shift %d: value rel_l2 %.3e (gate %.3e, ceiling %.3e of which cancellation %.3e)"
          % (name, box, fractional, cols, shift, e, gate, ceiling, cv / np.linalg.norm(want)))
    assert phi.shape == x.shape and e <= gate
    if cols == "()" and not shift:  # the tightest bond, r = 0.02: its two ends beside what the sweep's accumulator has rounded away
        i, j = c.pairs[0]
        r = float(np.linalg.norm(xr.images(_wrapped(c.s), c.A, c.pairs[:1])))
        k0 = 1.0 / r if kind == xr.COULOMB else 1.0 / r ** 6
        got = phi.cpu().numpy()
        print("%s %s: the bond at r = %.4f: |error| %.3e and %.3e of |value| %.3e and %.3e; 2^-24 |x| K0(r) = %.3e and %.3e"
              % (name, box, r, abs(got[i] - want[i]), abs(got[j] - want[j]), abs(want[i]), abs(want[j]),
                 2.0 ** -24 * abs(x[j]) * k0, 2.0 ** -24 * abs(x[i]) * k0))
    if field:
        want = _mix(ref[1], cols)
        e = rel_l2(E.cpu().numpy(), want)
        gate, ceiling = _gate(name + "_field", tol["field"], cf, np.linalg.norm(want))
        print("%s %s fractional %d cols %s shift %d: field rel_l2 %.3e (gate %.3e, ceiling %.3e of which cancellation %.3e)"
              % (name, box, fractional, cols, shift, e, gate, ceiling, cf / np.linalg.norm(want)))
        assert E.shape == (c.n, 3) + x.shape[1:] and e <= gate
    if not shift and cols != "complex":
        U = energy(_cuda(x), _cuda(pos), _cuda(c.batch), **kw).cpu().numpy()
        want = xr.energy(x, _mix(ref[0], cols), c.batch)
        gate, _ = _gate(name + "_value", tol["value"], cv, np.linalg.norm(_mix(ref[0], cols)))
        for b in (0, 1):  # (a sum of products, each good to the gate of |x| |phi|: Cauchy-Schwarz, per column)
            sel = c.batch == b
            bound = gate * 0.5 * np.linalg.norm(x[sel], axis=0) * np.linalg.norm(_mix(ref[0], cols)[sel], axis=0)
            assert (np.abs(U[b] - want[b]) <= bound).all()


@pytest.mark.parametrize("box,fractional,cols,field", WHOLE_CASES)
def test_coulomb_whole(box, fractional, cols, field):
    _run_whole(xr.COULOMB, box, fractional, cols, field)


@pytest.mark.parametrize("box,fractional,cols,field", WHOLE_CASES)
def test_dispersion_whole(box, fractional, cols, field):
    _run_whole(xr.DISPERSION, box, fractional, cols, field)


@pytest.mark.parametrize("kind", [xr.COULOMB, xr.DISPERSION])
@pytest.mark.parametrize("box,fractional", [("cube", False), ("T", True), ("T", False), ("O", False)])
def test_same_image_after_a_lattice_shift(kind, box, fractional):
    """every position moved by (+3, -2, +1) lattice vectors: the same result within the same gate.  In float32 the moved
    positions have lost bits, and Cartesian ones convert to fractional coordinates that differ in their last bits from the
    unmoved ones: a correction that formed d_ij from the positions as passed, and not from the reduced ones the sweep sees,
    would be off by 6e-8 |pos| / r^2 ~ 1e-4 per unit charge at r = 0.02"""
    _run_whole(kind, box, fractional, "(2,)", True, shift=True)


@pytest.mark.parametrize("kind", [xr.COULOMB, xr.DISPERSION])
@pytest.mark.parametrize("box,fractional", [("cube", False), ("T", True), ("T", False), ("O", True)])
def test_backward(kind, box, fractional):
    """L = sum g phi[x]: dL/dx is the corrected operator on g and dL/dpos_i = -(g_i E[x]_i + x_i E[g]_i), with the bounds of
    tests/test_gpu_ewald.py composed from the gates of the value and of the field"""
    import torch_nfft_amd as tn
    c = _case(box, kind)
    fn = tn.nfft_ewald if kind == xr.COULOMB else tn.nfft_ewald_dispersion
    name = "coulomb" if kind == xr.COULOMB else "dispersion"
    tol = _whole_tol("dispersion" if kind == xr.DISPERSION else ("coulomb_cube" if c.A is None else "coulomb_box"))
    x, g = c.x2[:, 0].copy(), c.x2[:, 1].copy()
    phi2, E2 = c.ref()
    kw = dict(splitting=c.splitting(), cutoff=4, exclusions=c.exclusions())
    if c.A is not None:
        kw["fractional"] = fractional
    xd, pd, gd, bd = _cuda(x).requires_grad_(True), _cuda(c.positions(fractional)).requires_grad_(True), _cuda(g), _cuda(c.batch)
    phi = fn(xd, pd, bd, **kw)
    dx, dpos = torch.autograd.grad((phi * gd).sum(), (xd, pd))
    tn.ops.check_status()
    # dx: the corrected operator applied to g, held to the gate of the value of THAT column
    (cv_x, cf_x), (cv_g, cf_g) = c.cancellation("first"), c.cancellation("second")
    gate_v, _ = _gate(name + "_value", tol["value"], cv_g, np.linalg.norm(phi2[:, 1]))
    e = rel_l2(dx.cpu().numpy(), phi2[:, 1])
    print("%s %s fractional %d: dx rel_l2 %.3e (gate %.3e)" % (name, box, fractional, e, gate_v))
    assert e <= gate_v
    # each field is good to its gate in l2 and is weighted by at most max |g| or max |x|
    want = -(g[:, None] * E2[:, :, 0] + x[:, None] * E2[:, :, 1])
    gate_x, _ = _gate(name + "_field", tol["field"], cf_x, np.linalg.norm(E2[:, :, 0]))
    gate_g, _ = _gate(name + "_field", tol["field"], cf_g, np.linalg.norm(E2[:, :, 1]))
    bound = np.abs(g).max() * gate_x * np.linalg.norm(E2[:, :, 0]) + np.abs(x).max() * gate_g * np.linalg.norm(E2[:, :, 1])
    if c.A is not None and fractional:
        want = want @ c.A.T
        bound *= np.linalg.norm(c.A, 2)
    err = np.linalg.norm(dpos.cpu().numpy() - want)
    print("%s %s fractional %d: dpos |error| %.3e, bound %.3e, rel_l2 %.3e" % (name, box, fractional, err, bound, rel_l2(dpos.cpu().numpy(), want)))
    assert dpos.shape == (c.n, 3) and err <= bound
    with pytest.raises(RuntimeError, match="differentiate twice|once_differentiable"):
        d1, = torch.autograd.grad(fn(xd, pd, bd, **kw).square().sum(), pd, create_graph=True)
        d1.square().sum().backward()


@pytest.mark.parametrize("kind", [xr.COULOMB, xr.DISPERSION])
@pytest.mark.parametrize("box,fractional", [("cube", False), ("T", True), ("O", False)])
def test_virial(kind, box, fractional):
    import torch_nfft_amd as tn
    c = _case(box, kind)
    fn = tn.nfft_ewald_virial if kind == xr.COULOMB else tn.nfft_ewald_dispersion_virial
    name = "coulomb" if kind == xr.COULOMB else "dispersion"
    tol = _whole_tol("coulomb_virial" if kind == xr.COULOMB else "dispersion_virial")
    kw = dict(splitting=c.splitting(), cutoff=4, exclusions=c.exclusions())
    if c.A is not None:
        kw["fractional"] = fractional
    U, W = fn(_cuda(c.x2), _cuda(c.positions(fractional)), _cuda(c.batch), **kw)
    tn.ops.check_status()
    Ur, Wr = c.virial_ref()
    assert U.shape == (2, 2) and W.shape == (2, 3, 3, 2)
    # what cancels here is float64 against float64 (the reductions) and the cast of sums that held the listed pairs
    lU, lW = xr.listed_virial(kind, np.abs(c.x2.astype(np.float64)), _wrapped(c.s), c.A, c.batch, c.pairs, c.w, c.split[0])
    eU, eW = rel_l2(U.cpu().numpy(), Ur), rel_l2(W.cpu().numpy(), Wr)
    gU = min(EXCL_TOL[name + "_U"], tol["U"] + 2.0 ** -24 * np.linalg.norm(lU) / np.linalg.norm(Ur))
    gW = min(EXCL_TOL[name + "_W"], tol["W"] + 2.0 ** -24 * np.linalg.norm(lW) / np.linalg.norm(Wr))
    print("%s virial %s fractional %d: U rel_l2 %.3e (gate %.3e), W rel_l2 %.3e (gate %.3e)" % (name, box, fractional, eU, gU, eW, gW))
    assert eU <= gU and eW <= gW
    # the trace: tr W = U (6 U).  The smooth part of a coincident pair is a constant that no strain moves, in U and not in W:
    # that pair breaks the trace of the sum over every pair, and excluding it fully (as here) mends it
    p = 1.0 if kind == xr.COULOMB else 6.0
    trunc = np.abs(np.trace(Wr, axis1=1, axis2=2) - p * Ur).max()  # (the truncated algorithm's own)
    tr = np.trace(W.cpu().numpy().astype(np.float64), axis1=1, axis2=2)
    err = np.abs(tr - p * U.cpu().numpy()).max()
    print("%s virial %s: |tr W - %g U|_max %.3e (the float64 algorithm's own %.3e)" % (name, box, p, err, trunc))
    assert err <= trunc + 3 * gW * np.linalg.norm(Wr) + p * gU * np.linalg.norm(Ur)


def test_empty_list_is_no_list(monkeypatch):
    """exclusions=None and an empty list give the same bits.  Two calls of nfft_ewald on the same input do NOT, with or
    without a list: the far field's transform spreads with float atomics and the charge of a point set is an index_add_ (the
    first two device runs of this test compared such calls and failed on these alone).  So the transform's result and the
    sums over the point sets are computed once here and handed to both calls -- every other step, the pair sweep, the
    correction and the terms after them, runs twice and must reproduce itself"""
    import torch_nfft_amd as tn
    for kind, fn, module in ((xr.COULOMB, tn.nfft_ewald, tn.ewald), (xr.DISPERSION, tn.nfft_ewald_dispersion, tn.dispersion)):
        c = _case("T", kind)
        sp = c.splitting()
        empty = tn.ExclusionList([], c.n, batch=c.batch)
        xd, pd, bd = _cuda(c.x2), _cuda(c.s), _cuda(c.batch)
        z, f = tn.ops.nfft_ewald_excl(pd, xd, bd, empty.row_start, empty.col, empty.weight(kind), sp.box6, sp.alpha, kind, True)
        assert z.shape == (c.n, 2) and f.shape == (c.n, 3, 2) and not bool(z.any()) and not bool(f.any())
        far = module.nfft_fastsum(xd, sp.coeffs, pd, None, bd, None, cutoff=4)
        calls = []

        def once(*args, **kw):
            calls.append(1)
            return far

        sums, set_sums = [], tn.ewald._set_sums

        def sums_once(q, batch):
            if not sums:
                sums.append(set_sums(q, batch))
            return sums[0]

        monkeypatch.setattr(module, "nfft_fastsum", once)
        monkeypatch.setattr(module, "_set_sums", sums_once)
        a = fn(xd, pd, bd, splitting=sp, fractional=True)
        b = fn(xd, pd, bd, splitting=sp, fractional=True, exclusions=empty)
        tn.ops.check_status()
        assert len(calls) == 2 and torch.equal(a, b)
        monkeypatch.undo()
        # and the seven sums of the virial lose exactly nothing
        out = tn.ops.nfft_ewald_excl_virial(pd, xd, bd, empty.row_start, empty.col, empty.weight(kind), sp.box6, sp.alpha, kind)
        assert out.shape == (2, 7, 2) and not bool(out.any())


def test_close_pair_and_coincident_pair_agree():
    """the coincident listed pair moved apart to r = 1e-6: phi of the whole function agrees with r = 0 within the ceiling of
    THAT list -- at 1e-6 the sweep's accumulator has held |q| / r = 1e6 |q|, so the cancellation term is the whole of it.  (The
    dispersion sum has no such test: 1 / r^6 = 1e36 leaves float32 no digits, and 1 / r^8 overflows below r = 1.6e-5; its
    r = 0 branch is the coincident pair of every case above.)"""
    import torch_nfft_amd as tn
    c = _case("cube", xr.COULOMB)
    d = xr.images(_wrapped(c.s), None, c.pairs)
    t = int(np.flatnonzero((d * d).sum(-1) == 0)[0])
    i, j = c.pairs[t]
    s1 = c.s.copy()
    s1[j] = s1[i] + np.float32(1e-6) * np.array([0.6, -0.64, 0.48], dtype=np.float32)
    r = float(np.linalg.norm(xr.images(_wrapped(s1), None, c.pairs[t:t + 1])))
    assert 0.5e-6 < r < 2e-6
    kw = dict(splitting=c.splitting(), cutoff=4, exclusions=c.exclusions())
    x = c.x2[:, 0].copy()
    phi0 = tn.nfft_ewald(_cuda(x), _cuda(c.s), _cuda(c.batch), **kw).cpu().numpy()
    phi1 = tn.nfft_ewald(_cuda(x), _cuda(s1), _cuda(c.batch), **kw).cpu().numpy()
    tn.ops.check_status()
    z, _ = xr.listed_terms(xr.COULOMB, np.abs(x.astype(np.float64)), _wrapped(s1), None, c.pairs, c.w, 12.0)
    from test_gpu_ewald import WHOLE_TOL
    ceiling = 2 * WHOLE_TOL["value"] + 2.0 ** -24 * np.linalg.norm(z) / np.linalg.norm(phi0)
    e = rel_l2(phi1, phi0)
    print("pair at r = %.2e against r = 0: rel_l2 %.3e, ceiling %.3e; at the pair %.3e and %.3e of |phi| %.3e and %.3e"
          % (r, e, ceiling, abs(phi1[i] - phi0[i]), abs(phi1[j] - phi0[j]), abs(phi0[i]), abs(phi0[j])))
    assert e <= ceiling
    # without the r = 0 constant the two would differ by 2 alpha / sqrt(pi) |q| at both ends
    assert 2 * 12.0 / np.sqrt(np.pi) * min(abs(x[i]), abs(x[j])) > 20 * ceiling * np.linalg.norm(phi0)
