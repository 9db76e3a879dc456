"""GPU tests of the fused Ewald step: the pair kernel and the spectral kernel of csrc/ewald_step.hip
on their own, then nfft_ewald_step as a whole, against the float64 restatements (tests/ewald_box_ref.py,
tests/ewald_virial_ref.py and their composition tests/ewald_step_ref.py) on the same float32 fractional positions, and against
the two public calls that the step replaces.

Tolerances.  The two kernels do the arithmetic of kernels that have measured gates, so they inherit those gates and get none
of their own; the numbers below are restated from the files named beside them, where each is 4 x the largest figure of that
kernel's first device run.  Where two device results are compared, each is within its gate of the float64 algorithm, so they
differ by at most twice that.  What the gates must not hide is wrong by far more: tests/test_ewald_step_ref.py.
"""
import math

import numpy as np
import pytest
import torch

import ewald_box_ref as eb
import ewald_ref as er
import ewald_step_ref as es
import ewald_virial_ref as ev
import exclusions_ref as xr
from conftest import rel_l2

pytestmark = pytest.mark.gpu

NEAR_TOL = {
    "value": 2.0e-6, "field": 1.8e-6, "crowded_value": 6.7e-6, "crowded_field": 8.5e-6,  # NEAR_TOL of tests/test_gpu_ewald_box.py
    "seven": 8.2e-6, "crowded_seven": 2.6e-6,  # NEAR_TOL "seven" and "crowded" of tests/test_gpu_ewald_virial.py
}
FAR_TOL = 3.8e-13  # FAR_TOL of tests/test_gpu_ewald_virial.py: the thread-to-cell mapping is kept, so the order of additions is too
SPECTRA_TOL = 1e-6  # tests/test_gpu_dipole.py::test_spectral_kernel: the same kind of product
WHOLE_TOL = {
    "value": 2.1e-6, "field": 8.3e-7, "fixed_point_value": 8.2e-6,  # WHOLE_TOL of tests/test_gpu_ewald_box.py
    "W": 3.2e-6, "U": 5.5e-5, "fixed_point": 2.0e-5,  # WHOLE_TOL of tests/test_gpu_ewald_virial.py
}
CARTESIAN_TOL = {
    "value": 1.3e-6, "field": 4.6e-6,  # CARTESIAN_TOL of tests/test_gpu_ewald_box.py
    "virial": 2.6e-6,  # WHOLE_TOL["cartesian"] of tests/test_gpu_ewald_virial.py
}

BOXES = {"T": eb.T, "O": eb.O, "S": eb.S, "I": np.eye(3)}


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _six(A):
    return [A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2]]


def _ragged_batch(rng, n):
    """three point sets, the middle one empty"""
    b = np.sort(rng.integers(0, 2, n)) * 2
    b[0], b[-1] = 0, 2
    return b.astype(np.int64)


def _box_points(rng, n):
    """n float32 FRACTIONAL points uniform in the box and, among the first hundred (one point set of the ragged cases),
    every edge case of the wrap (those of tests/test_gpu_ewald_box.py and tests/test_gpu_ewald_virial.py, restated)"""
    x = (rng.random((n, 3)) - 0.5).astype(np.float32)
    x[40:60] = x[0:20]                                    # exact duplicates: r = 0
    below = np.nextafter(np.float32(0.5), np.float32(0))  # the largest float32 below 1/2
    for a in range(3):
        x[60 + a, a] = -0.5                               # exactly on the lower face
        x[63 + a, a] = below
        x[66 + a] = x[60 + a] + np.float32(0.01) * rng.random(3).astype(np.float32)  # ... each with a close neighbour
        x[69 + a] = x[63 + a] - np.float32(0.01) * rng.random(3).astype(np.float32)
    x[63, :] = below                                      # (the upper corner; none in the lower one, see there)
    x[72:80] += np.float32(0.7)                           # given outside the box: must act as their images
    x[80:88] -= np.float32(1.2)
    for a in range(3):                                    # a pair straddling each face
        y = (rng.random(3) - 0.5).astype(np.float32)
        x[88 + 2 * a] = y
        x[89 + 2 * a] = y + np.float32(0.003)
        x[88 + 2 * a, a] = 0.49
        x[89 + 2 * a, a] = -0.49
    return x


# ---- the pair operator ------------------------------------------------------------------------------------------------

# box, alpha, r_c, the cells (NEAR_SPLITS of tests/test_gpu_ewald_virial.py)
NEAR_SPLITS = [("O", 14.0, 0.25, (4, 5, 3)), ("T", 12.0, 0.3, (3, 3, 3)), ("T", 30.0, 0.12, (7, 8, 7)),
               ("S", 16.0, 0.22, (3, 4, 4)), ("I", 12.0, 0.3, (3, 3, 3))]


def _same_bits_as_the_two_sweeps(tn, sd, qd, bd, six, alpha, r_c, z, f, seven):
    """whether (z, f) and seven are, bit for bit, those of the two sweeps that the pair kernel fuses (expected: the
    expressions are the same; reported in section 7q, not required)"""
    z0, f0 = tn.ops.nfft_ewald_near_box(sd, qd, bd, six, alpha, r_c, True)
    s0 = tn.ops.nfft_ewald_virial_near(sd, qd, bd, six, alpha, r_c)
    return torch.equal(z, z0) and torch.equal(f, f0), torch.equal(seven, s0)


@pytest.mark.parametrize("cols", [(), (2,), (3,), (5,)])  # (five columns: the CC = 4 pass twice, the tail masked)
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name,alpha,r_c,cells", NEAR_SPLITS)
def test_pair_operator_against_brute_force(name, alpha, r_c, cells, ragged, cols):
    import torch_nfft_amd as tn
    A = BOXES[name]
    assert tn.EwaldSplitting(alpha, r_c, 4, box=A).cells == cells
    rng = np.random.default_rng(int(alpha) * 100 + len(cols) + 10 * ragged + ord(name))
    n = 700
    s = _box_points(rng, n)
    q = rng.standard_normal((n,) + cols).astype(np.float32)
    batch = _ragged_batch(rng, n) if ragged else None
    if batch is not None:
        assert (batch[:100] == 0).all()  # the edge cases share a point set
    sd, qd, bd = _cuda(s), _cuda(q), _cuda(batch)
    z, f, seven = tn.ops.nfft_ewald_step_near(sd, qd, bd, _six(A), alpha, r_c)
    tn.ops.check_status()
    B = 3 if ragged else 1
    assert z.shape == q.shape and f.shape == (n, 3) + cols and z.dtype == f.dtype == torch.float32
    assert seven.shape == (B, 7) + cols and seven.dtype == torch.float64
    zref, fref = eb.near_sum(q, s, A, batch, alpha, r_c), eb.near_field(q, s, A, batch, alpha, r_c)
    sref = es.seven(*ev.near_virial(q, s, A, batch, alpha, r_c))
    e_z, e_f = rel_l2(z.cpu().numpy(), zref), rel_l2(f.cpu().numpy(), fref)
    e_s = ev.rel_fro(seven.cpu().numpy(), sref)
    same = _same_bits_as_the_two_sweeps(tn, sd, qd, bd, _six(A), alpha, r_c, z, f, seven)
    print("step near, box %s (%g, %g) ragged=%d cols=%s: value %.3e field %.3e seven %.3e; same bits as near_box %s, as "
          "virial_near %s" % (name, alpha, r_c, ragged, cols, e_z, e_f, e_s, same[0], same[1]))
    assert np.linalg.norm(zref) > 0 and np.linalg.norm(fref) > 0
    assert np.linalg.norm(sref[:, 0]) > 0 and np.linalg.norm(sref[:, 4:]) > 0
    assert e_z <= NEAR_TOL["value"] and e_f <= NEAR_TOL["field"] and e_s <= NEAR_TOL["seven"]
    if ragged:
        out = seven.cpu().numpy()
        assert not out[1].any()  # the empty point set: exactly zero
        assert out[0].all() and out[2].all()


@pytest.fixture(scope="module")
def crowded():
    """3000 points in a fractional cube of edge 0.06 centred on the corner (1/2, 1/2, 1/2) of the box T (that of
    tests/test_gpu_ewald_box.py): ~375 in each of the eight corner cells -- more than kNearBlock = 128, so three items per
    cell, the last with idle lanes -- and every neighbouring range holds more than kNearTile = 256, so the sweep takes
    several LDS tiles"""
    rng = np.random.default_rng(7)
    s = (0.5 + (rng.random((3000, 3)) - 0.5) * 0.06).astype(np.float32)
    q = rng.standard_normal(3000).astype(np.float32)
    return s, q


def test_crowded_corner(crowded):
    import torch_nfft_amd as tn
    s, q = crowded
    z, f, seven = tn.ops.nfft_ewald_step_near(_cuda(s), _cuda(q), None, _six(eb.T), 12.0, 0.3)
    tn.ops.check_status()
    zref, fref = eb.near_sum(q, s, eb.T, None, 12.0, 0.3), eb.near_field(q, s, eb.T, None, 12.0, 0.3)
    sref = es.seven(*ev.near_virial(q, s, eb.T, None, 12.0, 0.3))
    e_z, e_f, e_s = rel_l2(z.cpu().numpy(), zref), rel_l2(f.cpu().numpy(), fref), ev.rel_fro(seven.cpu().numpy(), sref)
    print("step near, box T, crowded corner: value %.3e field %.3e seven %.3e" % (e_z, e_f, e_s))
    assert e_z <= NEAR_TOL["crowded_value"] and e_f <= NEAR_TOL["crowded_field"] and e_s <= NEAR_TOL["crowded_seven"]


def test_two_calls_are_bitwise_equal(crowded):
    import torch_nfft_amd as tn
    s, q = crowded
    sd, qd = _cuda(s), _cuda(np.stack([q, -q[::-1], q * q], 1))
    a = tn.ops.nfft_ewald_step_near(sd, qd, None, _six(eb.T), 12.0, 0.3)
    b = tn.ops.nfft_ewald_step_near(sd, qd, None, _six(eb.T), 12.0, 0.3)
    tn.ops.check_status()
    assert a[2].shape == (1, 7, 3)
    for x, y in zip(a, b):
        assert bool(x.all()) and torch.equal(x, y)
    band = torch.randn(2, 12, 12, 12, 3, dtype=torch.complex64, device="cuda")
    sp = tn.EwaldSplitting(12.0, 0.3, 12, box=eb.T)
    a = tn.ops.nfft_ewald_step_spectral(band, sp.coeffs, sp.box6, 12.0)
    b = tn.ops.nfft_ewald_step_spectral(band, sp.coeffs, sp.box6, 12.0)
    tn.ops.check_status()
    assert a[0].shape == (2, 12, 12, 12, 4, 3) and a[1].shape == (2, 7, 3) and bool(a[1].all()) and bool(a[0].any())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_no_points_and_refused_inputs():
    import torch_nfft_amd as tn
    pos = torch.zeros(0, 3, device="cuda")
    z, f, seven = tn.ops.nfft_ewald_step_near(pos, torch.zeros(0, 2, device="cuda"), None, _six(eb.T), 12.0, 0.3)
    assert z.shape == (0, 2) and f.shape == (0, 3, 2) and z.dtype == torch.float32
    assert seven.shape == (1, 7, 2) and seven.dtype == torch.float64 and not bool(seven.any())
    z, f, seven = tn.ops.nfft_ewald_step_near(pos, torch.zeros(0, device="cuda"), None, _six(eb.T), 12.0, 0.3)
    assert z.shape == (0,) and f.shape == (0, 3) and seven.shape == (1, 7)
    sp = tn.EwaldSplitting(12.0, 0.3, 8, box=eb.T)
    spectra, seven = tn.ops.nfft_ewald_step_spectral(torch.zeros(1, 8, 8, 8, 0, dtype=torch.complex64, device="cuda"), sp.coeffs,
                                                     sp.box6, 12.0)
    assert spectra.shape == (1, 8, 8, 8, 4, 0) and seven.shape == (1, 7, 0)
    tn.ops.check_status()
    four = torch.zeros(4, 3, device="cuda")
    with pytest.raises(RuntimeError, match="Input mismatch"):  # real charges only
        tn.ops.nfft_ewald_step_near(four, torch.zeros(4, dtype=torch.complex64, device="cuda"), None, _six(eb.T), 12.0, 0.3)
    with pytest.raises(RuntimeError, match="Input mismatch"):  # r_cut above a third of the smallest width
        tn.ops.nfft_ewald_step_near(four, torch.zeros(4, device="cuda"), None, _six(eb.T), 12.0, 0.31)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_step_spectral(torch.zeros(1, 8, 8, 8, device="cuda"), sp.coeffs, sp.box6, 12.0)


# ---- the spectral operator --------------------------------------------------------------------------------------------

# 32: 128 workgroups per point set; 72 and 80: more cells than the 262144 threads of a point set, so threads take a second
# cell and the index is advanced by the stride with both carries (tests/test_gpu_ewald_virial.py has the digits).  One, two
# and three columns: whole cells in 16-byte pieces, and the four-column pass with a masked tail.
SPECTRAL_CASES = [(N, name, cols) for N in (32, 72, 80) for name in ("I", "O", "T") for cols in ((), (2,), (3,))]


def _spectral_refs(tn, sp, band, A, alpha, cols):
    N = sp.bandwidth
    fc = sp.field_coeffs().reshape([1, N, N, N, 4] + [1] * len(cols))
    return _cuda(band).unsqueeze(4) * fc, es.seven(*ev.far_virial(band, sp.coeffs.cpu().numpy(), A, alpha))


@pytest.mark.parametrize("N,name,cols", SPECTRAL_CASES)
def test_spectral_operator(N, name, cols):
    import torch_nfft_amd as tn
    A = BOXES[name]
    alpha = 40.0 if N >= 64 else 12.0  # (so that the coefficients count out to the grid's edge)
    sp = tn.EwaldSplitting(alpha, 0.25, N, box=A)
    rng = np.random.default_rng(N + len(cols) + ord(name))
    B = 2 if N == 32 else 1
    shape = (B, N, N, N) + cols
    band = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    spectra, seven = tn.ops.nfft_ewald_step_spectral(_cuda(band), sp.coeffs, sp.box6, alpha)
    tn.ops.check_status()
    assert spectra.shape == (B, N, N, N, 4) + cols and spectra.dtype == torch.complex64
    assert seven.shape == (B, 7) + cols and seven.dtype == torch.float64
    want, sref = _spectral_refs(tn, sp, band, A, alpha, cols)
    e_sp = [rel_l2(spectra[:, :, :, :, k].cpu().numpy(), want[:, :, :, :, k].cpu().numpy()) for k in range(4)]
    e_s = ev.rel_fro(seven.cpu().numpy(), sref)
    print("step spectral, N %d box %s cols %s: spectra %s, seven %.3e (|ref| %.3e)"
          % (N, name, cols, " ".join("%.3e" % e for e in e_sp), e_s, np.linalg.norm(sref)))
    assert np.linalg.norm(sref[:, 4:]) > 0 and float(want[:, :, :, :, 1:].abs().min(4).values.max()) > 0
    # (whether the seven sums are, bit for bit, those of the reduction that this kernel replaces: reported in section 7q)
    print("    same bits as virial_far: %s" % torch.equal(seven, tn.ops.nfft_ewald_virial_far(_cuda(band), sp.coeffs, sp.box6, alpha)))
    assert max(e_sp) <= SPECTRA_TOL
    assert e_s <= FAR_TOL


@pytest.mark.parametrize("cols", [(), (2,), (4,)])
def test_spectral_operator_on_a_band_that_is_not_16_byte_aligned(cols):
    """a contiguous view one complex64 into its storage: the cells move in 8-byte pieces, the results are the same bits;
    and where b_k = 0 the spectra are zero whatever the band holds"""
    import torch_nfft_amd as tn
    sp = tn.EwaldSplitting(6.0, 0.25, 8, box=eb.T)
    shape = (2, 8, 8, 8) + cols
    buf = torch.randn(1 + math.prod(shape), dtype=torch.complex64, device="cuda")
    band = buf[1:].view(shape)
    zero = (sp.coeffs == 0).reshape((1, 8, 8, 8) + (1,) * len(cols)).expand(shape)
    assert int(zero.sum()) == 2 * (1 + 8 ** 3 - 7 ** 3) * math.prod(cols)
    band[zero] = complex(float("inf"), float("nan"))
    assert band.is_contiguous() and band.data_ptr() % 16 == 8
    aligned = band.clone()
    assert aligned.data_ptr() % 16 == 0
    a = tn.ops.nfft_ewald_step_spectral(band, sp.coeffs, sp.box6, 6.0)
    b = tn.ops.nfft_ewald_step_spectral(aligned, sp.coeffs, sp.box6, 6.0)
    tn.ops.check_status()
    assert bool(a[1].all()) and bool(torch.isfinite(a[1]).all()) and torch.equal(a[1], b[1])
    assert bool(torch.isfinite(torch.view_as_real(a[0])).all()) and torch.equal(a[0], b[0])
    assert not bool(a[0][zero.unsqueeze(4).expand(a[0].shape)].any())
    clean = torch.where(zero, torch.zeros_like(aligned), aligned)
    want = clean.unsqueeze(4) * sp.field_coeffs().reshape([1, 8, 8, 8, 4] + [1] * len(cols))
    assert rel_l2(a[0].cpu().numpy(), want.cpu().numpy()) <= SPECTRA_TOL
    far = tn.ops.nfft_ewald_virial_far(clean, sp.coeffs, sp.box6, 6.0)  # (float64 against float64, the same order)
    assert ev.rel_fro(a[1].cpu().numpy(), far.cpu().numpy()) <= FAR_TOL


# ---- the whole call ---------------------------------------------------------------------------------------------------

WHOLE = {"T": (12.0, 0.3, 32), "O": (14.0, 0.25, 48)}  # (those of the two files this one sits between)


class Whole:
    """n charges in the box `name`, one point set or two ragged ones: float32 Cartesian positions x and the float32
    fractional positions s that they convert back to (as tests/test_gpu_ewald_box.py does); among the first 72 points of the
    first set thirty bonded pairs at 0.02 .. 0.05 and one coincident pair, listed with the scales 0, 1/2 and 1/1.2; the
    float64 restatement with and without the list, computed once"""

    def __init__(self, n, name, ragged):
        self.n, self.name, self.A = n, name, BOXES[name]
        rng = np.random.default_rng(n + ord(name) + ragged)
        s0 = rng.random((n, 3)) - 0.5
        inv = np.linalg.inv(self.A)
        pairs = []
        for k in range(30):
            e = rng.standard_normal(3)
            s0[2 * k + 1] = s0[2 * k] + (rng.uniform(0.02, 0.05) * e / np.linalg.norm(e)) @ inv
            pairs.append((2 * k + 1, 2 * k) if k % 2 else (2 * k, 2 * k + 1))
        s0[71] = s0[70]  # r = 0
        pairs.append((70, 71))
        self.pairs = np.array(pairs, dtype=np.int64)
        self.scale = np.array([(0.0, 0.5, 1.0 / 1.2)[k % 3] for k in range(30)] + [0.0])
        self.x = (s0.astype(np.float32).astype(np.float64) @ self.A).astype(np.float32)
        self.s = (self.x.astype(np.float64) @ inv).astype(np.float32)
        assert (self.s[70] == self.s[71]).all()
        self.q = rng.standard_normal(n).astype(np.float32)
        self.batch = (np.arange(n) >= int(0.46 * n)).astype(np.int64) if ragged else None
        self.B = 2 if ragged else 1
        self._ref = None

    def ref(self, excl):
        if self._ref is None:
            alpha, r_c, N = WHOLE[self.name]
            self._ref = es.exact_step(self.q, self.s, self.A, self.batch, alpha, r_c, N)
        if not excl:
            return self._ref
        alpha = WHOLE[self.name][0]
        zx, fx = xr.listed_terms(xr.COULOMB, self.q, self.s, self.A, self.pairs, 1.0 - self.scale, alpha)
        Ux, Wx = xr.listed_virial(xr.COULOMB, self.q, self.s, self.A, self.batch, self.pairs, 1.0 - self.scale, alpha)
        phi, E, U, W = self._ref
        return phi - zx, E - fx, U - Ux, W - Wx

    def exclusions(self, tn):
        return tn.ExclusionList(self.pairs, self.n, coulomb_scale=self.scale, batch=self.batch)


_WHOLE = {}


def _whole(n, name, ragged):
    key = (n, name, ragged)
    if key not in _WHOLE:
        _WHOLE[key] = Whole(*key)
    return _WHOLE[key]


def _errors(got, ref):
    """relative errors of (phi, E, U, W) against ref"""
    g = [t.cpu().numpy() for t in got]
    return rel_l2(g[0], ref[0]), rel_l2(g[1], ref[1]), ev.rel_fro(g[2], ref[2]), ev.rel_fro(g[3], ref[3])


@pytest.mark.parametrize("excl", [False, True])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", ["T", "O"])
@pytest.mark.parametrize("n", [300, 700])
def test_whole_step(n, name, ragged, excl):
    """Cartesian and fractional input against the float64 restatement, against each other, against nfft_ewald(field=True)
    and nfft_ewald_virial of the same inputs, and tr W = U"""
    import torch_nfft_amd as tn
    c = _whole(n, name, ragged)
    alpha, r_c, N = WHOLE[name]
    sp = tn.EwaldSplitting(alpha, r_c, N, box=c.A)
    ex = c.exclusions(tn) if excl else None
    qd, xd, sd, bd = _cuda(c.q), _cuda(c.x), _cuda(c.s), _cuda(c.batch)
    ref = c.ref(excl)
    cart = tn.nfft_ewald_step(qd, xd, bd, splitting=sp, cutoff=4, exclusions=ex)
    frac = tn.nfft_ewald_step(qd, sd, bd, splitting=sp, cutoff=4, fractional=True, exclusions=ex)
    phi2, E2 = tn.nfft_ewald(qd, sd, bd, splitting=sp, cutoff=4, field=True, fractional=True, exclusions=ex)
    U2, W2 = tn.nfft_ewald_virial(qd, sd, bd, splitting=sp, cutoff=4, fractional=True, exclusions=ex)
    tn.ops.check_status()
    phi, E, U, W = frac
    assert phi.shape == (n,) and E.shape == (n, 3) and U.shape == (c.B,) and W.shape == (c.B, 3, 3)
    assert phi.dtype == E.dtype == U.dtype == W.dtype == torch.float32
    assert torch.equal(W, W.transpose(1, 2))
    for what, got in (("fractional", frac), ("Cartesian", cart)):
        e = _errors(got, ref)
        print("nfft_ewald_step, %d charges in %s, ragged=%d excl=%d, %s input vs float64: phi %.3e E %.3e U %.3e W %.3e"
              % ((n, name, ragged, excl, what) + e))
        assert e[0] <= WHOLE_TOL["value"] and e[1] <= WHOLE_TOL["field"] and e[2] <= WHOLE_TOL["U"] and e[3] <= WHOLE_TOL["W"]
    e = _errors(cart, [t.cpu().numpy() for t in frac])
    print("    Cartesian vs fractional input: phi %.3e E %.3e U %.3e W %.3e" % e)
    assert e[0] <= CARTESIAN_TOL["value"] and e[1] <= CARTESIAN_TOL["field"] and max(e[2], e[3]) <= CARTESIAN_TOL["virial"]
    e = _errors(frac, [t.cpu().numpy() for t in (phi2, E2, U2, W2)])
    print("    vs nfft_ewald(field=True) and nfft_ewald_virial: phi %.3e E %.3e U %.3e W %.3e" % e)
    assert e[0] <= 2 * WHOLE_TOL["value"] and e[1] <= 2 * WHOLE_TOL["field"]
    assert e[2] <= 2 * WHOLE_TOL["U"] and e[3] <= 2 * WHOLE_TOL["W"]
    # tr W = U for the converged sum: |tr W - U| <= |tr (W - Wa)| + |tr Wa - Ua| + |Ua - U| with the float64 algorithm's
    # (Ua, Wa), whose own tr Wa - Ua is its truncation, and the two gates in place of the device's errors (|tr E| <= sqrt(3) |E|_F)
    Ua, Wa = ref[2], ref[3]
    U, W = U.cpu().numpy().astype(np.float64), W.cpu().numpy().astype(np.float64)
    for b in range(c.B):
        own = abs(np.trace(Wa[b]) - Ua[b])
        bound = math.sqrt(3.0) * WHOLE_TOL["W"] * np.linalg.norm(Wa) + WHOLE_TOL["U"] * np.linalg.norm(Ua) + own
        print("    set %d: tr W - U = %.3e, bound %.3e (the algorithm's own %.1e; U = %.7g)" % (b, np.trace(W[b]) - U[b], bound, own, U[b]))
        assert abs(np.trace(W[b]) - U[b]) <= bound


def test_columns_and_the_unit_cube():
    """two columns in a ragged batch; box=None is the identity box"""
    import torch_nfft_amd as tn
    c = _whole(300, "T", True)
    rng = np.random.default_rng(9)
    q = np.stack([c.q, rng.standard_normal(c.n).astype(np.float32)], 1)
    qd, sd, bd = _cuda(q), _cuda(c.s), _cuda(c.batch)
    cube = tn.EwaldSplitting(12.0, 0.3, 32)
    ident = tn.EwaldSplitting(12.0, 0.3, 32, box=(1, 1, 1))
    a = tn.nfft_ewald_step(qd, sd, bd, splitting=cube, cutoff=4)
    b = tn.nfft_ewald_step(qd, sd, bd, splitting=ident, cutoff=4, fractional=True)
    tn.ops.check_status()
    assert a[0].shape == (300, 2) and a[1].shape == (300, 3, 2) and a[2].shape == (2, 2) and a[3].shape == (2, 3, 3, 2)
    ref = es.exact_step(q, c.s, np.eye(3), c.batch, 12.0, 0.3, 32)
    for what, got in (("box=None", a), ("identity box", b)):
        e = _errors(got, ref)
        print("nfft_ewald_step, two columns, %s vs float64: phi %.3e E %.3e U %.3e W %.3e" % ((what,) + e))
        assert e[0] <= WHOLE_TOL["value"] and e[1] <= WHOLE_TOL["field"] and e[2] <= WHOLE_TOL["U"] and e[3] <= WHOLE_TOL["W"]
    with pytest.raises(ValueError, match="fractional"):
        tn.nfft_ewald_step(qd, sd, bd, splitting=cube, fractional=True)


def test_primitive_rock_salt():
    """two ions in the primitive fcc cell: phi_i = -2 M q_i, U = -2 M, W = (U / 3) I"""
    import torch_nfft_amd as tn
    A, _ = eb.lower_triangular(eb.ROCK_SALT_PRIMITIVE)
    q = np.array([1.0, -1.0], dtype=np.float32)
    s = np.array([[0.0, 0.0, 0.0], [-0.5, -0.5, -0.5]], dtype=np.float32)
    alpha, r_c, N = 21.0, 0.19, 48
    sp = tn.EwaldSplitting(alpha, r_c, N, box=A)
    phi, E, U, W = (t.cpu().numpy() for t in tn.nfft_ewald_step(_cuda(q), _cuda(s), splitting=sp, cutoff=4, fractional=True))
    tn.ops.check_status()
    pa, Ea, Ua, Wa = es.exact_step(q, s, A, None, alpha, r_c, N)
    want = -2.0 * er.MADELUNG_NACL
    own = max(np.abs(pa / q - want).max() / abs(want), abs(Ua[0] - want) / abs(want), np.abs(Wa[0] - want / 3.0 * np.eye(3)).max() / abs(want / 3.0))
    e_phi, e_U, e_W = rel_l2(phi, pa), ev.rel_fro(U, Ua), ev.rel_fro(W, Wa)
    print("primitive rock salt: phi / q = %s, U = %.7f (%.7f), diag W = %s; vs float64 phi %.3e U %.3e W %.3e (its own %.1e)"
          % (phi / q, U[0], want, np.diag(W[0]), e_phi, e_U, e_W, own))
    assert own <= 1e-8
    assert e_phi <= WHOLE_TOL["fixed_point_value"] and max(e_U, e_W) <= WHOLE_TOL["fixed_point"]
    assert np.abs(phi / q - want).max() / abs(want) <= WHOLE_TOL["fixed_point_value"] + own
    assert abs(U[0] - want) / abs(want) <= WHOLE_TOL["fixed_point"] + own
    assert np.abs(W[0] - want / 3.0 * np.eye(3)).max() / abs(want / 3.0) <= math.sqrt(3.0) * WHOLE_TOL["fixed_point"] + own
    assert E.shape == (2, 3)


def test_empty_input_and_autograd():
    import torch_nfft_amd as tn
    sp = tn.EwaldSplitting(12.0, 0.3, 16, box=eb.T)
    pos = torch.zeros(0, 3, device="cuda")
    for fractional in (False, True):
        phi, E, U, W = tn.nfft_ewald_step(torch.zeros(0, 2, device="cuda"), pos, splitting=sp, fractional=fractional)
        assert phi.shape == (0, 2) and E.shape == (0, 3, 2) and U.shape == (1, 2) and W.shape == (1, 3, 3, 2)
        assert phi.dtype == E.dtype == U.dtype == W.dtype == torch.float32
        assert not bool(U.any()) and not bool(W.any())
    # inputs that require grad are accepted; all four outputs are constants to autograd
    c = _whole(300, "T", True)
    qd, xd, bd = _cuda(c.q), _cuda(c.x), _cuda(c.batch)
    sp = tn.EwaldSplitting(*WHOLE["T"], box=eb.T)
    out = tn.nfft_ewald_step(qd.clone().requires_grad_(True), xd.clone().requires_grad_(True), bd, splitting=sp)
    tn.ops.check_status()
    for t in out:
        assert not t.requires_grad and t.grad_fn is None
    e = _errors(out, c.ref(False))
    assert e[0] <= WHOLE_TOL["value"] and e[1] <= WHOLE_TOL["field"] and e[2] <= WHOLE_TOL["U"] and e[3] <= WHOLE_TOL["W"]
    with pytest.raises(ValueError, match="real"):
        tn.nfft_ewald_step(qd.to(torch.complex64), xd, bd, splitting=sp)
    with pytest.raises(AssertionError, match="batch"):
        tn.nfft_ewald_step(qd, xd, torch.zeros(300, device="cuda", requires_grad=True), splitting=sp)
    with pytest.raises(ValueError, match="lists pairs of"):
        tn.nfft_ewald_step(qd, xd, bd, splitting=sp, exclusions=tn.ExclusionList([(0, 1)], 299))
