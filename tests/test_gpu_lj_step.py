"""GPU tests of the Lennard-Jones + Coulomb step: the pair kernel and the spectral kernel of
csrc/ewald_lj_step.hip on their own, then nfft_ewald_lj_step as a whole, against the float64 restatement
(tests/lj_step_ref.py) on the same float32 fractional positions, and with a = None against the public calls it replaces.

Points.  r^-12 forbids uniform random points: one near-coincident pair would be the whole norm and hide every other error.
All point sets are jittered lattices with a stated minimum separation (lj_step_ref.lj_points: 0.064 in fractional terms, the
edge cases of the wrap included, asserted below in each box's metric) and sigma = 0.8 x the lattice spacing, so that the three
parts of the force are of comparable size.

Tolerances.  Each gate is 4 x the largest relative error of the first device run against the float64 restatement, written
beside it; rel_l2 for F, rel_fro for W, the relative error for U.  A first-run figure above 1e-4 would have been a bug to
find, not a tolerance to record; none was (the largest, 3.7e-5, is a pair energy whose terms cancel).  What the gates must
not hide is wrong by far more: tests/test_lj_step_ref.py.
"""
import math

import numpy as np
import pytest
import torch

import dispersion_virial_ref as dv
import ewald_box_ref as eb
import lj_step_ref as lj
from conftest import rel_l2
from ewald_virial_ref import rel_fro

pytestmark = pytest.mark.gpu

NEAR_TOL = {  # the pair kernel against brute force, forty cases of 700 points (the largest first-run figure in brackets)
    "F": 2.0e-5,     # (5.069e-6: T at (12, 0.3), one set, all three species; 1.3e-7 .. 4.6e-6 on the others)
    # (3.710e-5: T at (30, 0.12), one set: seven neighbours per charge, whose +- q_i q_j w sum to 0.015 against terms of the
    # size of one -- what is left of a cancellation; 2.0e-7 .. 2.1e-6 on the four other splits)
    "U_C": 1.5e-4,
    "U_LJ": 6.9e-6,  # (1.719e-6: the unit cube, all three species, where a^2 / r^12 and c^2 w_D are closest in size)
    "W": 7.3e-6,     # (1.816e-6: charges alone in T at (30, 0.12); 3.1e-8 .. 1.1e-6 on the others)
}
# float64 torch against the kernel's float64 sums on the same float32 band and tables: what is left is the order of additions
SPECTRAL_TOL = {  # eighteen cases, N = 32, 72, 80, and the two of the unaligned band
    "spectra": 2.2e-7,  # (5.42e-8: a float32 product against the float64 one)
    "U_C": 6.9e-16,     # (1.73e-16)
    "U_LJ": 1.4e-15,    # (3.37e-16)
    "W": 2.5e-14,       # (6.12e-15: the Coulomb and dispersion weights have opposite signs)
}
WHOLE_TOL = {  # nfft_ewald_lj_step (cutoff = 4) against the float64 restatement: I, T, O, one set and ragged, both inputs
    "F": 5.1e-6,     # (1.287e-6)
    "U_C": 1.2e-5,   # (2.949e-6 in T, ragged; below the 5.5e-5 of nfft_ewald_step's U, made by the same arithmetic)
    "U_LJ": 1.5e-6,  # (3.723e-7)
    "W": 1.2e-6,     # (2.909e-7)
}
# The gates of the kernels whose arithmetic a single species repeats, restated from the files named beside them.  Where two
# device results are compared, each is within its gate of the float64 algorithm, so they differ by at most the two gates' sum.
# Whether the single-species figures of the first run kept them (DESIGN.md section 7r has the table): all did -- the pair
# kernel with charges alone F 1.17e-6 and W 1.82e-6, with c alone F 1.50e-6, U 1.80e-7 and W 2.21e-7; the whole call with
# a = None F 5.05e-7, U_C 2.94e-6, U_LJ 2.31e-7 and W 2.32e-7.
INHERITED = {
    "step_near_field": 1.8e-6, "step_near_seven": 8.2e-6,          # NEAR_TOL of tests/test_gpu_ewald_step.py
    "step_field": 8.3e-7, "step_U": 5.5e-5, "step_W": 3.2e-6,      # WHOLE_TOL of tests/test_gpu_ewald_step.py
    "dispersion_near_field": 7.4e-6, "dispersion_field": 3.0e-6,   # NEAR_TOL, WHOLE_TOL of tests/test_gpu_dispersion.py
    "dispersion_near_seven": 7.9e-7,                               # NEAR_TOL of tests/test_gpu_dispersion_virial.py
    "dispersion_U": 4.3e-6, "dispersion_W": 1.2e-6,                # WHOLE_TOL of tests/test_gpu_dispersion_virial.py
}

BOXES = {"T": eb.T, "O": eb.O, "S": eb.S, "I": np.eye(3)}


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _six(A):
    return [A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2]]


def _relative(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def _coefficients(rng, n, A, spacing=None):
    """(q, c, a) float32: standard normal charges, sigma = 0.8 x the lattice spacing along the box's shortest stretch
    (+- 5 %: at most 1.3 d_min, whatever the box), epsilon in [0.5, 1.5).  spacing: the Cartesian spacing of another lattice
    than lj_points'"""
    if spacing is None:
        spacing = lj.LJ_SPACING * np.linalg.svd(A, compute_uv=False).min()
    sigma, eps = 0.8 * spacing * (0.95 + 0.1 * rng.random(n)), 0.5 + rng.random(n)
    c, a = lj.lj_coefficients(sigma, eps)
    return rng.standard_normal(n).astype(np.float32), c.astype(np.float32), a.astype(np.float32)


def _assert_separated(s, A):
    """on the CPU: no pair other than the exact duplicates is closer than d_min = 0.064 x the box's smallest stretch"""
    d_min = lj.D_MIN_FRACTIONAL * np.linalg.svd(A, compute_uv=False).min()
    got = lj.dr.min_separation(s, A)
    assert got >= d_min * (1 - 1e-6), (got, d_min)
    return d_min


# ---- the pair kernel ---------------------------------------------------------------------------------------------------

# box, alpha_C, r_c, the cells (NEAR_SPLITS of tests/test_gpu_ewald_step.py: the (3, 3, 3) grids split every row, (7, 8, 7)
# none of the inner ones); alpha_D = alpha_C + 1.5
NEAR_SPLITS = [("O", 14.0, 0.25, (4, 5, 3)), ("T", 12.0, 0.3, (3, 3, 3)), ("T", 30.0, 0.12, (7, 8, 7)),
               ("S", 16.0, 0.22, (3, 4, 4)), ("I", 12.0, 0.3, (3, 3, 3))]
SPECIES = {"q": (1, 0, 0), "c": (0, 1, 0), "a": (0, 0, 1), "qca": (1, 1, 1)}
_NEAR = {}


def _near_case(k, ragged):
    """the points, coefficients and float64 pair sums of each species alone for split k, computed once: the sums are
    bilinear in each species and have no cross terms, so all three together is their sum"""
    if (k, ragged) not in _NEAR:
        name, alpha, r_c, _ = NEAR_SPLITS[k]
        A = BOXES[name]
        rng = np.random.default_rng(100 * k + ragged)
        s = lj.lj_points(rng, 700)
        _assert_separated(s, A)
        q, c, a = _coefficients(rng, 700, A)
        batch = dv.ragged_batch(700) if ragged else None  # (three sets, the middle one empty; the edge cases share the first)
        z = np.zeros(700)
        refs = {"q": lj.near_step(q, z, z, s, A, batch, alpha, alpha + 1.5, r_c),
                "c": lj.near_step(z, c, z, s, A, batch, alpha, alpha + 1.5, r_c),
                "a": lj.near_step(z, z, a, s, A, batch, alpha, alpha + 1.5, r_c)}
        refs["qca"] = tuple(sum(refs[k2][e] for k2 in "qca") for e in range(2))
        _NEAR[(k, ragged)] = (s, (q, c, a), batch, refs)
    return _NEAR[(k, ragged)]


@pytest.mark.parametrize("species", list(SPECIES))
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("k", range(len(NEAR_SPLITS)))
def test_pair_kernel_against_brute_force(k, ragged, species):
    import torch_nfft_amd as tn
    name, alpha, r_c, cells = NEAR_SPLITS[k]
    A = BOXES[name]
    assert tn.EwaldSplitting(alpha, r_c, 4, box=A).cells == cells
    s, values, batch, refs = _near_case(k, ragged)
    n, B = 700, 3 if ragged else 1
    xs = np.stack([v if on else np.zeros(n, np.float32) for v, on in zip(values, SPECIES[species])], 1)
    sd, xd, bd = _cuda(s), _cuda(xs), _cuda(batch)
    f, eight = tn.ops.nfft_ewald_lj_step_near(sd, xd, bd, _six(A), alpha, alpha + 1.5, r_c)
    f2, eight2 = tn.ops.nfft_ewald_lj_step_near(sd, xd, bd, _six(A), alpha, alpha + 1.5, r_c)
    tn.ops.check_status()
    assert f.shape == (n, 3) and f.dtype == torch.float32 and eight.shape == (B, 8) and eight.dtype == torch.float64
    assert torch.equal(f, f2) and torch.equal(eight, eight2)  # no atomics: the same bits
    f, eight = f.cpu().numpy().astype(np.float64), eight.cpu().numpy()
    fref, eref = refs[species]
    assert np.isfinite(f).all() and np.isfinite(eight).all()
    e = {"F": rel_l2(f, fref), "W": rel_fro(eight[:, 2:], eref[:, 2:])}
    for key, col, on in (("U_C", 0, SPECIES[species][0]), ("U_LJ", 1, SPECIES[species][1] or SPECIES[species][2])):
        if on:
            e[key] = _relative(eight[:, col], eref[:, col])
        else:
            assert not eight[:, col].any() and not eref[:, col].any()  # an absent species adds exactly zero
    newton = np.abs(f.sum(0)).max() / np.abs(f).sum()
    print("lj near, box %s (%g, %g) ragged=%d species %s: %s; |sum F| / sum |F| %.2e"
          % (name, alpha, r_c, ragged, species, " ".join("%s %.3e" % kv for kv in sorted(e.items())), newton))
    assert np.linalg.norm(fref) > 0 and np.linalg.norm(eref[:, 2:]) > 0
    for key, err in e.items():
        assert err <= NEAR_TOL[key], (key, err)
    # Newton's third law.  A pair's term enters f_i and f_j with opposite signs, each rounded on its own: with about a
    # hundred float32 additions per point the worst case is 100 x 2^-24 = 6e-6 of the sum of the terms' magnitudes, which for
    # charges of both signs exceeds |f_i| by about the root of the neighbour count, 5: 3e-5 (random errors give 1e-8)
    assert newton <= 3e-5
    if ragged:
        assert not eight[1].any()  # the empty point set: exactly zero
        assert eight[0, 2:].all() and eight[2, 2:].all()


def test_pair_kernel_no_points_and_refused_inputs():
    import torch_nfft_amd as tn
    pos = torch.zeros(0, 3, device="cuda")
    f, eight = tn.ops.nfft_ewald_lj_step_near(pos, torch.zeros(0, 3, device="cuda"), None, _six(eb.T), 12.0, 13.0, 0.3)
    assert f.shape == (0, 3) and eight.shape == (1, 8) and eight.dtype == torch.float64 and not bool(eight.any())
    tn.ops.check_status()
    four = torch.zeros(4, 3, device="cuda")
    with pytest.raises(RuntimeError, match="Input mismatch"):  # (q, c, a) per point, nothing else
        tn.ops.nfft_ewald_lj_step_near(four, torch.zeros(4, 2, device="cuda"), None, _six(eb.T), 12.0, 13.0, 0.3)
    with pytest.raises(RuntimeError, match="Input mismatch"):  # r_cut above a third of the smallest width
        tn.ops.nfft_ewald_lj_step_near(four, torch.zeros(4, 3, device="cuda"), None, _six(eb.T), 12.0, 13.0, 0.31)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_lj_step_near(four, torch.zeros(4, 3, device="cuda"), None, _six(eb.T), 12.0, float("nan"), 0.3)
    sp = tn.EwaldSplitting(12.0, 0.3, 8, box=eb.T)
    with pytest.raises(RuntimeError, match="Input mismatch"):  # one column is not (q, c)
        tn.ops.nfft_ewald_lj_step_spectral(torch.zeros(1, 8, 8, 8, 1, dtype=torch.complex64, device="cuda"), sp.coeffs, sp.coeffs,
                                           sp.coeffs, sp.box6, 12.0)


# ---- the spectral kernel -----------------------------------------------------------------------------------------------

def _spectral_reference(sc, sd, band, alpha_c):
    """(spectra, eight) in float64 torch on the device from the same band and the splittings' float32 tables"""
    N = sc.bandwidth
    kap = sc._kappa().to(band.device)  # [N, N, N, 3] float64
    bC, bD, tD = sc.coeffs.double(), sd.coeffs.double(), sd.strain_coeffs().double()
    S = band.to(torch.complex128)
    zero = torch.zeros((), dtype=torch.complex128, device=band.device)
    Rq = torch.where(bC == 0, zero, bC * S[..., 0])  # (a zero in the table: zeros, whatever the band holds)
    Rc = torch.where(bD == 0, zero, bD * S[..., 1])
    tau = 2j * math.pi * kap
    spectra = torch.stack([tau[..., a] * R for R in (Rq, Rc) for a in range(3)], 4)
    pq = torch.where(bC == 0, torch.zeros_like(bC), S[..., 0].real ** 2 + S[..., 0].imag ** 2)
    pc = torch.where(bD == 0, torch.zeros_like(bD), S[..., 1].real ** 2 + S[..., 1].imag ** 2)
    k2 = (kap * kap).sum(3)
    fac = -2.0 * (1.0 / torch.where(k2 > 0, k2, torch.ones_like(k2)) + math.pi ** 2 / alpha_c ** 2)
    UC, UD = 0.5 * (bC * pq).sum((1, 2, 3)), 0.5 * (bD * pc).sum((1, 2, 3))
    six = []
    for a, b in ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)):
        kk = kap[..., a] * kap[..., b]
        w = 0.5 * (bC * fac * kk * pq).sum((1, 2, 3)) - 0.5 * (tD * kk * pc).sum((1, 2, 3))
        six.append(w + (UC - UD if a == b else 0.0))
    return spectra, torch.stack([UC, -UD] + six, 1)


def _spectral_errors(got, want):
    spectra, eight = got
    ws, we = want
    e = {"spectra": max(rel_l2(spectra[..., k].cpu().numpy(), ws[..., k].cpu().numpy()) for k in range(6))}
    eight, we = eight.cpu().numpy(), we.cpu().numpy()
    e["U_C"], e["U_LJ"], e["W"] = _relative(eight[:, 0], we[:, 0]), _relative(eight[:, 1], we[:, 1]), rel_fro(eight[:, 2:], we[:, 2:])
    return e


# N: the sizes of tests/test_gpu_ewald_step.py's spectral test (32: 128 workgroups per point set; 72, not a power of two, and
# 80: threads take a second cell and the index is advanced with both carries)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", ["I", "O", "T"])
@pytest.mark.parametrize("N", [32, 72, 80])
def test_spectral_kernel(N, name, B):
    import torch_nfft_amd as tn
    A = BOXES[name]
    alpha = 40.0 if N >= 64 else 12.0  # (so that the tables count out to the grid's edge)
    sc = tn.EwaldSplitting(alpha, 0.25, N, box=A)
    sd = tn.DispersionSplitting(0.8 * N, 0.25, N, box=A)  # (dispersion_virial_ref.far_alpha)
    rng = np.random.default_rng(N + B + ord(name))
    shape = (B, N, N, N, 2)
    band = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    band[:, N // 2, N // 2, N // 2] *= 8  # (S_0 = sum c of positive coefficients stands above the other cells)
    band = _cuda(band)
    got = tn.ops.nfft_ewald_lj_step_spectral(band, sc.coeffs, sd.coeffs, sd.strain_coeffs(), sc.box6, alpha)
    again = tn.ops.nfft_ewald_lj_step_spectral(band, sc.coeffs, sd.coeffs, sd.strain_coeffs(), sc.box6, alpha)
    tn.ops.check_status()
    assert got[0].shape == (B, N, N, N, 6) and got[0].dtype == torch.complex64
    assert got[1].shape == (B, 8) and got[1].dtype == torch.float64
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    want = _spectral_reference(sc, sd, band, alpha)
    assert float(want[0].abs().min(4).values.max()) > 0 and bool(want[1].all())
    e = _spectral_errors(got, want)
    print("lj spectral, N %d box %s B %d: %s" % (N, name, B, " ".join("%s %.3e" % kv for kv in sorted(e.items()))))
    for key, err in e.items():
        assert err <= SPECTRAL_TOL[key], (key, err)


@pytest.mark.parametrize("B", [1, 3])
def test_spectral_kernel_on_a_band_that_is_not_16_byte_aligned(B):
    """a contiguous view one complex64 into its storage takes the 8-byte path: the same bits; and zeros are written where
    a table is zero, even when the band holds NaN there"""
    import torch_nfft_amd as tn
    N = 8
    sc = tn.EwaldSplitting(6.0, 0.25, N, box=eb.T)
    sd = tn.DispersionSplitting(6.4, 0.25, N, box=eb.T)
    shape = (B, N, N, N, 2)
    gen = torch.Generator(device="cuda").manual_seed(B)  # (the gates are a few units of float64's last place: the same band every run)
    buf = torch.randn(1 + math.prod(shape), dtype=torch.complex64, device="cuda", generator=gen)
    band = buf[1:].view(shape)
    zc, zd = (sc.coeffs == 0), (sd.coeffs == 0)
    assert int(zc.sum()) == 1 + N ** 3 - (N - 1) ** 3 and int(zd.sum()) == N ** 3 - (N - 1) ** 3  # (the dispersion k = 0 counts)
    band[:, zc, 0] = complex(float("inf"), float("nan"))
    band[:, zd, 1] = complex(float("nan"), float("nan"))
    assert band.is_contiguous() and band.data_ptr() % 16 == 8
    aligned = band.clone()
    assert aligned.data_ptr() % 16 == 0
    tables = (sc.coeffs, sd.coeffs, sd.strain_coeffs(), sc.box6, 6.0)
    a = tn.ops.nfft_ewald_lj_step_spectral(band, *tables)
    b = tn.ops.nfft_ewald_lj_step_spectral(aligned, *tables)
    tn.ops.check_status()
    assert bool(a[1].all()) and bool(torch.isfinite(a[1]).all()) and torch.equal(a[1], b[1])
    assert bool(torch.isfinite(torch.view_as_real(a[0])).all()) and torch.equal(a[0], b[0])
    assert not bool(a[0][:, zc, :3].any()) and not bool(a[0][:, zd, 3:].any())
    assert bool(a[0][:, ~zc, :3].any()) and bool(a[0][:, ~zd, 3:].any())
    e = _spectral_errors(a, _spectral_reference(sc, sd, aligned, 6.0))
    print("lj spectral, unaligned band, B %d: %s" % (B, " ".join("%s %.3e" % kv for kv in sorted(e.items()))))
    for key, err in e.items():
        assert err <= SPECTRAL_TOL[key], (key, err)


# ---- the whole call ----------------------------------------------------------------------------------------------------

WHOLE = {"I": (12.0, 13.0, 0.3, 32), "T": (12.0, 13.0, 0.3, 32), "O": (14.0, 15.0, 0.25, 48)}  # alpha_C, alpha_D, r_c, N
_WHOLE = {}


class Whole:
    """700 points of lj_points in the box `name`, one point set or three ragged ones with an empty middle one: float32
    Cartesian positions x and the float32 fractional positions s that they convert back to; the float64 restatement of the
    three species together and of (q, c) without a, computed once"""

    def __init__(self, name, ragged):
        self.name, self.A = name, BOXES[name]
        rng = np.random.default_rng(ord(name) + ragged)
        s0 = lj.lj_points(rng, 700)
        self.x = (s0.astype(np.float64) @ self.A).astype(np.float32)
        self.s = (self.x.astype(np.float64) @ np.linalg.inv(self.A)).astype(np.float32)
        self.d_min = _assert_separated(self.s, self.A)
        self.q, self.c, self.a = _coefficients(rng, 700, self.A)
        self.batch = dv.ragged_batch(700) if ragged else None
        self.B = 3 if ragged else 1
        self._ref = {}

    def ref(self, with_a=True):
        if with_a not in self._ref:
            a = self.a if with_a else np.zeros(700)
            self._ref[with_a] = lj.exact_lj_step(self.q, self.c, a, self.s, self.A, self.batch, *WHOLE[self.name])
        return self._ref[with_a]


def _whole(name, ragged):
    if (name, ragged) not in _WHOLE:
        _WHOLE[(name, ragged)] = Whole(name, ragged)
    return _WHOLE[(name, ragged)]


def _whole_errors(got, ref):
    g = [np.asarray(t.cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float64) for t in got]
    return {"F": rel_l2(g[0], ref[0]), "U_C": _relative(g[1], ref[1]), "U_LJ": _relative(g[2], ref[2]), "W": rel_fro(g[3], ref[3])}


def _splittings(tn, name):
    alpha_c, alpha_d, r_c, N = WHOLE[name]
    box = None if name == "I" else BOXES[name]
    return tn.EwaldSplitting(alpha_c, r_c, N, box=box), tn.DispersionSplitting(alpha_d, r_c, N, box=box)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", ["I", "T", "O"])
def test_whole_call(name, ragged):
    """the unit cube (box=None), a triclinic and an orthorhombic box, Cartesian and fractional positions, against the float64
    restatement; tr W = U_C - 6 U_D + 12 U_R within the gates"""
    import torch_nfft_amd as tn
    w = _whole(name, ragged)
    spc, spd = _splittings(tn, name)
    qd, cd, ad, xd, sd, bd = (_cuda(v) for v in (w.q, w.c, w.a, w.x, w.s, w.batch))
    ref = w.ref()
    cart = tn.nfft_ewald_lj_step(qd, cd, ad, xd, bd, coulomb=spc, dispersion=spd, cutoff=4)
    runs = [("Cartesian", cart)]
    if name != "I":
        runs.append(("fractional", tn.nfft_ewald_lj_step(qd, cd, ad, sd, bd, coulomb=spc, dispersion=spd, fractional=True)))
    tn.ops.check_status()
    F, UC, ULJ, W = cart
    assert F.shape == (700, 3) and UC.shape == (w.B,) and ULJ.shape == (w.B,) and W.shape == (w.B, 3, 3)
    assert F.dtype == UC.dtype == ULJ.dtype == W.dtype == torch.float32
    assert torch.equal(W, W.transpose(1, 2))
    for t in cart:
        assert not t.requires_grad and bool(torch.isfinite(t).all())
    live = [0, 2] if ragged else [0]
    for what, got in runs:
        e = _whole_errors([got[0]] + [t[live] for t in got[1:]], [ref[0]] + [r[live] for r in ref[1:]])
        print("nfft_ewald_lj_step, box %s ragged=%d, %s input vs float64: %s (d_min %.3g)"
              % (name, ragged, what, " ".join("%s %.3e" % kv for kv in sorted(e.items())), w.d_min))
        for key, err in e.items():
            assert err <= WHOLE_TOL[key], (key, err)
        if ragged:
            assert not bool(got[1][1]) and not bool(got[2][1]) and not bool(got[3][1].any())  # the empty set
    # Newton's third law for the whole force: the far field's share is not antisymmetric pair by pair, so only within the gate
    Fn = F.cpu().numpy().astype(np.float64)
    assert np.abs(Fn.sum(0)).max() <= WHOLE_TOL["F"] * math.sqrt(700) * np.linalg.norm(Fn)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", ["I", "T"])
def test_without_repulsion_against_the_calls_it_replaces(name, ragged):
    """a = None: F against q E - c G of nfft_ewald(field=True) and nfft_ewald_dispersion(field=True), U_coulomb and W against
    nfft_ewald_virial and the negated nfft_ewald_dispersion_virial.  Both sides are device results, each within its gate of
    the float64 algorithm: they may differ by the sum of the two gates."""
    import torch_nfft_amd as tn
    w = _whole(name, ragged)
    spc, spd = _splittings(tn, name)
    qd, cd, xd, bd = (_cuda(v) for v in (w.q, w.c, w.x, w.batch))
    F, UC, ULJ, W = tn.nfft_ewald_lj_step(qd, cd, None, xd, bd, coulomb=spc, dispersion=spd)
    e = _whole_errors((F, UC, ULJ, W), w.ref(with_a=False))
    E = tn.nfft_ewald(qd, xd, bd, splitting=spc, field=True)[1]
    G = tn.nfft_ewald_dispersion(cd, xd, bd, splitting=spd, field=True)[1]
    U1, W1 = tn.nfft_ewald_virial(qd, xd, bd, splitting=spc)
    U2, W2 = tn.nfft_ewald_dispersion_virial(cd, xd, bd, splitting=spd)
    tn.ops.check_status()
    live = [0, 2] if ragged else [0]
    print("a = None, box %s ragged=%d vs float64: %s" % (name, ragged, " ".join("%s %.3e" % kv for kv in sorted(e.items()))))
    for key, err in e.items():
        assert err <= WHOLE_TOL[key], (key, err)
    d = _whole_errors((F, UC[live], ULJ[live], W[live]),
                      [t.cpu().numpy().astype(np.float64) for t in (qd[:, None] * E - cd[:, None] * G, U1[live], -U2[live],
                                                                     (W1 - W2)[live])])
    print("    vs the public calls: %s" % " ".join("%s %.3e" % kv for kv in sorted(d.items())))
    assert d["F"] <= WHOLE_TOL["F"] + INHERITED["step_field"] + INHERITED["dispersion_field"]
    assert d["U_C"] <= WHOLE_TOL["U_C"] + INHERITED["step_U"] and d["U_LJ"] <= WHOLE_TOL["U_LJ"] + INHERITED["dispersion_U"]
    assert d["W"] <= WHOLE_TOL["W"] + INHERITED["step_W"] + INHERITED["dispersion_W"]
    # c alone: U_lj and W are the negated nfft_ewald_dispersion_virial
    _, UC0, ULJ0, W0 = tn.nfft_ewald_lj_step(None, cd, None, xd, bd, coulomb=spc, dispersion=spd)
    assert not bool(UC0.any())
    d0 = _relative(ULJ0[live].cpu().numpy(), -U2[live].cpu().numpy().astype(np.float64)), rel_fro(W0[live].cpu().numpy(), -W2[live].cpu().numpy())
    print("    c alone vs -nfft_ewald_dispersion_virial: U_lj %.3e W %.3e (that kernel's gates: %.1e, %.1e)"
          % (d0 + (INHERITED["dispersion_U"], INHERITED["dispersion_W"])))
    assert d0[0] <= WHOLE_TOL["U_LJ"] + INHERITED["dispersion_U"] and d0[1] <= WHOLE_TOL["W"] + INHERITED["dispersion_W"]


def test_empty_input_and_autograd():
    import torch_nfft_amd as tn
    spc, spd = _splittings(tn, "T")
    pos = torch.zeros(0, 3, device="cuda")
    e = torch.zeros(0, device="cuda")
    F, UC, ULJ, W = tn.nfft_ewald_lj_step(e, e, e, pos, coulomb=spc, dispersion=spd)
    assert F.shape == (0, 3) and UC.shape == (1,) and ULJ.shape == (1,) and W.shape == (1, 3, 3)
    assert not bool(UC.any()) and not bool(ULJ.any()) and not bool(W.any())
    w = _whole("T", True)
    qd, cd, ad, xd, bd = (_cuda(v) for v in (w.q, w.c, w.a, w.x, w.batch))
    out = tn.nfft_ewald_lj_step(qd.clone().requires_grad_(True), cd.clone().requires_grad_(True), ad, xd.clone().requires_grad_(True),
                                bd, coulomb=spc, dispersion=spd)
    tn.ops.check_status()
    for t in out:
        assert not t.requires_grad and t.grad_fn is None
    with pytest.raises(ValueError, match="columns are not supported"):
        tn.nfft_ewald_lj_step(qd[:, None], cd, ad, xd, bd, coulomb=spc, dispersion=spd)
    with pytest.raises(ValueError, match="must be real"):
        tn.nfft_ewald_lj_step(qd, cd.to(torch.complex64), ad, xd, bd, coulomb=spc, dispersion=spd)
