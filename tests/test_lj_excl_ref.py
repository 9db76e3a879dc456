"""CPU tests of the Lennard-Jones + Coulomb step with bonded-pair exclusions: the float64 restatement
tests/lj_excl_ref.py against a lattice sum in which the listed image is scaled instead of subtracted, against central
differences of that energy, against itself and against three wrong formulas; the kernel's series against the closed forms
across its switch point; the refusals of nfft_ewald_lj_excl_step before any device work, the operator schemas, the C ABI's
validation and the resource figures of csrc/ewald_lj_excl.hip."""
import ctypes
import math
import re

import mpmath
import numpy as np
import pytest
import torch
from scipy.special import erfc

import ewald_box_ref as eb
import exclusions_ref as xr
import lj_excl_ref as le
import lj_step_ref as lj
from conftest import rel_l2
from ewald_virial_ref import rel_fro

N_POINTS = 44
SPLIT = (13.0, 14.0, 0.3, 40)  # alpha_C, alpha_D, r_c, N: those of tests/test_lj_step_ref.py, whose TRUNCATION applies
TRUNCATION = 1e-5
LARGEST_GPU_TOLERANCE = 1e-4
CONVERGED_ALPHA = (6.0, 3.2)   # of the converged sums in ewald_box_ref and dispersion_ref: they set the r = 0 constants


@pytest.fixture(scope="module")
def system():
    """44 points in the triclinic box T: a chain, two waters, the hub of 21, the face pairs, the coincident pair, the pair
    beyond the cut, two single atoms"""
    rng = np.random.default_rng(21)
    s, pairs, sc, sl, info = le.bonded_points(rng, N_POINTS, eb.T, SPLIT[2])
    q, c, a = le.coefficients(rng, N_POINTS, info)
    q = q.astype(np.float64)
    q -= q.mean()
    return s.astype(np.float64), q, c.astype(np.float64), a.astype(np.float64), pairs, sc, sl, info


def _scaled_energy(q, c, a, s, A, r_c, pairs, sc, sl):
    """U = U_C - U_D + U_R of one point set with the listed image of every listed pair SCALED by s inside the converged sums:
    its r^-12 term (r < r_c) enters the sum times s; its erfc(alpha r) / r and its dispersion pair weight leave the near sums w times, and the far sums
    lose w times the smooth remainder erf(alpha r) / r and 1 / r^6 - w_D(r), which is bounded (at r = 0 the near sums hold
    nothing of the pair and the remainders are 2 alpha / sqrt(pi) and alpha^6 / 6).  No 1 / r, 1 / r^6 or 1 / r^12 is subtracted."""
    ac, ad = CONVERGED_ALPHA
    U = lj.converged_energy(q, c, np.zeros_like(a), s, A, r_c) + le.repulsion_scaled(a, s, A, None, r_c, pairs, sl, nimg=1)[1][0]
    pairs_, wc, wl = le._lists(pairs, sc, sl)
    d = xr.images(s, A, pairs_)
    r = np.sqrt((d * d).sum(-1))
    ok = r > 0
    rs = np.where(ok, r, 1.0)
    SC, _, SD, _ = le.smooth_parts(r, ac, ad)
    a2 = (ad * rs) ** 2
    w6 = np.where(ok, np.exp(-a2) * (1.0 + a2 + 0.5 * a2 * a2) / rs ** 6, 0.0)
    near_c = np.where(ok, erfc(ac * rs) / rs, 0.0)
    i, j = pairs_[:, 0], pairs_[:, 1]
    return U - (wc * q[i] * q[j] * (near_c + SC)).sum() + (wl * c[i] * c[j] * (w6 + SD)).sum()


def test_system_is_what_the_builder_promises(system):
    s, q, c, a, pairs, sc, sl, info = system
    assert s.shape == (N_POINTS, 3) and pairs.shape[0] == 6 + 2 * 3 + 210 + 3 + 1 + 1 + 1
    assert info["sigma"] <= 0.8 * info["d_min"] * (1 + 1e-12)
    rows = np.bincount(pairs.ravel(), minlength=N_POINTS)
    assert rows[info["hub"]] == 20 and rows[0] >= 3
    assert set(np.round(sc[sl > 0], 6)) == {0.5, round(1 / 1.2, 6)} and (s.max() > 0.5 or s.min() < -0.5)


def test_restatement_against_the_scaled_lattice_sum(system):
    s, q, c, a, pairs, sc, sl, info = system
    r_c = SPLIT[2]
    F, UC, ULJ, W = le.exact_lj_excl_step(q, c, a, s, eb.T, None, pairs, sc, sl, *SPLIT)
    # (each side takes the r = 0 constants of its own alphas)
    cF, cUC, cULJ, cW, (_, cUD, cUR) = le.converged_lj_excl_step(q, c, a, s, eb.T, r_c, pairs, sc, sl, *CONVERGED_ALPHA)
    scale = abs(cUD[0]) + abs(cUR[0])
    e = rel_l2(F, cF), abs((UC[0] - cUC[0]) / cUC[0]), abs(ULJ[0] - cULJ[0]) / scale, rel_fro(W, cW)
    print("restatement vs converged sums: F %.3e U_C %.3e U_LJ %.3e W %.3e" % e)
    # (a coincident pair's far part depends on alpha; with w = 1 the correction removes exactly that dependence)
    assert max(e) <= TRUNCATION
    U = _scaled_energy(q, c, a, s, eb.T, r_c, pairs, sc, sl)
    total = cUC[0] + cULJ[0]
    print("scaled lattice sum %.12g, converged sums minus the listed terms %.12g" % (U, total))
    assert abs(U - total) <= 1e-10 * (abs(cUC[0]) + scale)
    # tr W = U_C - 6 U_D + 12 U_R for the corrected converged sums
    tr, want = np.trace(cW[0]), cUC[0] - 6.0 * cUD[0] + 12.0 * cUR[0]
    size = abs(cUC[0]) + 6.0 * abs(cUD[0]) + 12.0 * abs(cUR[0])
    print("tr W %.9g, U_C - 6 U_D + 12 U_R %.9g" % (tr, want))
    assert abs(tr - want) <= 1e-6 * size
    assert np.abs(cW - cW.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(cW).max()
    # Newton's third law
    assert np.abs(F.sum(0)).max() <= 1e-9 * np.abs(F).sum() and np.abs(cF.sum(0)).max() <= 1e-9 * np.abs(cF).sum()


def test_force_and_virial_are_derivatives_of_the_scaled_energy(system):
    """F = -dU/dx and W = -dU/d eps by central differences (h = 1e-5 x the bond) of the scaled lattice sum, at the ends of a
    tight bond, of a 1-4 pair, of the hub, of a face pair, of the pair beyond the cut and of the far-index pair.  The
    coincident pair stays where it is: at r = 0 the energy is continuous but the pair's repulsion is not defined."""
    s, q, c, a, pairs, sc, sl, info = system
    A, r_c = eb.T, SPLIT[2]
    h = 2e-7
    F, _, _, W, _ = le.converged_lj_excl_step(q, c, a, s, A, r_c, pairs, sc, sl, *CONVERGED_ALPHA)
    inv = np.linalg.inv(A)
    amber = pairs[np.isclose(sc, 1 / 1.2)][0]
    probe = sorted({int(v) for v in (*info["tight"][0], *info["tight"][-1], *amber, info["hub"], info["hub"] + 3, *info["beyond"],
                                     *info["far_index"])})
    energy = lambda s_, A_: _scaled_energy(q, c, a, s_, A_, r_c, pairs, sc, sl)
    fd = np.zeros((len(probe), 3))
    for row, i in enumerate(probe):
        for k in range(3):
            dx = np.zeros(3)
            dx[k] = h
            sp, sm = s.copy(), s.copy()
            sp[i] += dx @ inv
            sm[i] -= dx @ inv
            fd[row, k] = -(energy(sp, A) - energy(sm, A)) / (2 * h)
    e = np.abs(F[probe] - fd).max() / np.abs(F).max()
    print("F against central differences at %d points: %.3e of |F|_max %.3g" % (len(probe), e, np.abs(F).max()))
    assert e <= 1e-5
    fw = np.zeros((3, 3))
    hw = 1e-6
    for k in range(3):
        for l in range(3):
            eps = np.zeros((3, 3))
            eps[k, l] = hw
            fw[k, l] = -(energy(s, A @ (np.eye(3) + eps)) - energy(s, A @ (np.eye(3) - eps))) / (2 * hw)
    e = np.abs(W[0] - fw).max() / np.abs(W).max()
    print("W against central differences: %.3e of |W|_max %.3g" % (e, np.abs(W).max()))
    assert e <= 1e-5


def test_a_fully_excluded_pair_is_continuous_at_r_zero(system):
    """one end of the coincident pair moved away by 1e-2 and 3e-3: the energies and the force go to those at r = 0 at least
    in proportion (the point moves in the field of the others; the pair itself adds nothing at first order), and U_C ends
    well inside the 2 alpha / sqrt(pi) |q_i q_j| by which it would stay off without the r = 0 constant.  Not closer:
    c_i c_j / r^6 is 3e10 at 1e-3, and the restatement takes it out of a float64 sum."""
    s, q, c, a, pairs, sc, sl, info = system
    i, j = info["coincident"]
    jump = abs(q[i] * q[j]) * 2 * CONVERGED_ALPHA[0] / math.sqrt(math.pi)
    inv = np.linalg.inv(eb.T)
    ref = le.converged_lj_excl_step(q, c, a, s, eb.T, SPLIT[2], pairs, sc, sl, *CONVERGED_ALPHA)
    last = None
    for dist in (1e-2, 3e-3):
        s2 = s.copy()
        s2[j] += np.array([dist, 0.0, 0.0]) @ inv
        got = le.converged_lj_excl_step(q, c, a, s2, eb.T, SPLIT[2], pairs, sc, sl, *CONVERGED_ALPHA)
        e = abs(got[1][0] - ref[1][0]), abs(got[2][0] - ref[2][0]), np.abs(got[0] - ref[0]).max()
        print("coincident pair moved apart by %g: U_C %.3e U_LJ %.3e F %.3e" % ((dist,) + e))
        if last is not None:
            assert all(now <= 0.5 * before for now, before in zip(e, last))
        last = e
    print("2 alpha / sqrt(pi) |q_i q_j| = %.3e" % jump)
    assert last[0] <= 0.2 * jump


@pytest.mark.parametrize("mutant", ["repulsion_unscaled", "all_images", "constant_sign"])
def test_mutants_are_far_off(system, mutant):
    """each wrong formula is off by at least 100 x the largest tolerance that a GPU test may have"""
    s, q, c, a, pairs, sc, sl, info = system
    F, UC, ULJ, W = le.exact_lj_excl_step(q, c, a, s, eb.T, None, pairs, sc, sl, *SPLIT)
    Fm, UCm, ULJm, Wm = le.exact_lj_excl_step(q, c, a, s, eb.T, None, pairs, sc, sl, *SPLIT, mutant=mutant)
    e = {"F": rel_l2(Fm, F), "U_C": abs(UCm[0] / UC[0] - 1), "U_LJ": abs(ULJm[0] / ULJ[0] - 1), "W": rel_fro(Wm, W)}
    print("mutant %-20s %s" % (mutant, " ".join("%s %.3e" % kv for kv in sorted(e.items()))))
    gate = 100 * LARGEST_GPU_TOLERANCE
    if mutant == "repulsion_unscaled":
        assert min(e["F"], e["U_LJ"], e["W"]) >= gate and e["U_C"] == 0
    elif mutant == "all_images":
        assert e["U_C"] >= gate and e["W"] >= gate
    else:
        assert e["U_LJ"] >= gate and e["F"] == 0 and e["W"] == 0 and e["U_C"] == 0


def test_series_against_closed_forms_across_the_switch_point():
    """the kernel's eight terms below u = 1/8 and the closed forms above, in float64, against 80-digit values (the closed forms lose 32 digits at u = 1e-8); and the two
    against each other around the switch"""
    mpmath.mp.dps = 80
    ac, ad = 13.0, 14.0

    def exact(r):
        r_ = mpmath.mpf(r)
        slope = 2 * mpmath.mpf(ac) / mpmath.sqrt(mpmath.pi)
        SC = mpmath.erf(ac * r_) / r_
        TC = (SC - slope * mpmath.exp(-(ac * r_) ** 2)) / r_ ** 2
        u = (ad * r_) ** 2
        e_ = mpmath.exp(-u)
        h = (1 - e_ * (1 + u + u * u / 2)) / u ** 3
        return [float(v) for v in (SC, TC, mpmath.mpf(ad) ** 6 * h, mpmath.mpf(ad) ** 8 * (6 * h - e_) / u)]

    worst = {"series": 0.0, "closed": 0.0, "both": 0.0}
    for u in np.concatenate([np.geomspace(1e-8, le.SERIES_SWITCH, 25), np.linspace(le.SERIES_SWITCH, 4.0, 25)]):
        for alpha, which in ((ac, (0, 1)), (ad, (2, 3))):
            r = math.sqrt(u) / alpha
            want = exact(r)
            se = le.smooth_series(np.array([r]), ac, ad, le.SERIES_TERMS)
            cl = le.smooth_closed(np.array([r]), ac, ad)
            for k in which:
                if u <= le.SERIES_SWITCH:
                    worst["series"] = max(worst["series"], abs(se[k][0] / want[k] - 1))
                if u >= le.SERIES_SWITCH:
                    worst["closed"] = max(worst["closed"], abs(cl[k][0] / want[k] - 1))
                if 0.5 * le.SERIES_SWITCH <= u <= le.SERIES_SWITCH:
                    worst["both"] = max(worst["both"], abs(se[k][0] / cl[k][0] - 1))
    print("series below the switch %.2e, closed forms above %.2e, one against the other just below %.2e"
          % (worst["series"], worst["closed"], worst["both"]))
    # float32's half unit is 6e-8: both sides of the switch are four digits better
    assert worst["series"] <= 1e-11 and worst["closed"] <= 1e-10 and worst["both"] <= 1e-9
    # the limits at r = 0
    z = le.smooth_series(np.array([0.0]), ac, ad, le.SERIES_TERMS)
    want = (2 * ac / math.sqrt(math.pi), 4 * ac ** 3 / (3 * math.sqrt(math.pi)), ad ** 6 / 6, ad ** 8 / 4)
    assert all(abs(z[k][0] / want[k] - 1) <= 1e-15 for k in range(4))
    # every value is bounded by its limit
    r = np.linspace(1e-4, 0.5, 400)
    for k, v in enumerate(le.smooth_parts(r, ac, ad)):
        assert (v > 0).all() and (v <= want[k]).all()
    # and the list step's reference agrees with the definition: erfc part + smooth part = 1 / r, w_D + S_D = 1 / r^6
    SC, TC, SD, TD = le.smooth_parts(r, ac, ad)
    a2 = (ad * r) ** 2
    w6 = np.exp(-a2) * (1 + a2 + a2 * a2 / 2) / r ** 6
    assert np.abs((erfc(ac * r) / r + SC) * r - 1).max() <= 1e-14 and np.abs((w6 + SD) * r ** 6 - 1).max() <= 1e-12


def test_refusals_without_gpu():
    import torch_nfft
    import torch_nfft_amd as tn
    assert "nfft_ewald_lj_excl_step" in tn.__all__ and torch_nfft.nfft_ewald_lj_excl_step is tn.nfft_ewald_lj_excl_step
    assert tn.nfft_ewald_lj_excl_step is tn.lj.nfft_ewald_lj_excl_step
    spc = tn.EwaldSplitting(12.0, 0.25, 16, box=eb.T, device="cpu")
    spd = tn.DispersionSplitting(11.0, 0.25, 16, box=eb.T, device="cpu")
    q, pos = torch.zeros(5), torch.zeros(5, 3)
    call = tn.nfft_ewald_lj_excl_step
    ex = tn.ExclusionList([[0, 1], [3, 1]], 5, coulomb_scale=[0.0, 0.5], dispersion_scale=0.5, device="cpu")
    with pytest.raises(TypeError, match="nfft_ewald_lj_excl_step: exclusions must be an ExclusionList or None"):
        call(q, q, q, pos, coulomb=spc, dispersion=spd, exclusions=[[0, 1]])
    with pytest.raises(ValueError, match="nfft_ewald_lj_excl_step: exclusions lists pairs of 4 points, pos has 5"):
        call(q, q, q, pos, coulomb=spc, dispersion=spd, exclusions=tn.ExclusionList([[0, 1]], 4, device="cpu"))
    with pytest.raises(TypeError, match="nfft_ewald_lj_excl_step: coulomb must be an EwaldSplitting"):
        call(q, q, q, pos, coulomb=spd, dispersion=spd, exclusions=ex)
    with pytest.raises(TypeError, match="nfft_ewald_lj_excl_step: dispersion must be a DispersionSplitting"):
        call(q, q, q, pos, coulomb=spc, dispersion=spc, exclusions=ex)
    with pytest.raises(ValueError, match="same r_cut"):
        call(q, q, q, pos, coulomb=spc, dispersion=tn.DispersionSplitting(11.0, 0.2, 16, box=eb.T, device="cpu"), exclusions=ex)
    with pytest.raises(ValueError, match="same bandwidth"):
        call(q, q, q, pos, coulomb=spc, dispersion=tn.DispersionSplitting(11.0, 0.25, 18, box=eb.T, device="cpu"), exclusions=ex)
    with pytest.raises(ValueError, match="same box"):
        call(q, q, q, pos, coulomb=spc, dispersion=tn.DispersionSplitting(11.0, 0.25, 16, box=eb.O, device="cpu"), exclusions=ex)
    for k in range(3):
        v = [q, q, q]
        v[k] = torch.zeros(5, 2)
        with pytest.raises(ValueError, match="nfft_ewald_lj_excl_step: %s must be \\[n\\]: columns are not supported" % "qca"[k]):
            call(*v, pos, coulomb=spc, dispersion=spd, exclusions=ex)
        v[k] = q.to(torch.complex64)
        with pytest.raises(ValueError, match="nfft_ewald_lj_excl_step: %s must be real" % "qca"[k]):
            call(*v, pos, coulomb=spc, dispersion=spd, exclusions=ex)
        v[k] = q.double()
        with pytest.raises(ValueError, match="must be float32"):
            call(*v, pos, coulomb=spc, dispersion=spd, exclusions=ex)
    with pytest.raises(ValueError, match="nfft_ewald_lj_excl_step: .*three-dimensional"):
        call(q, q, q, torch.zeros(5, 2), coulomb=spc, dispersion=spd, exclusions=ex)
    with pytest.raises(ValueError, match="nfft_ewald_lj_excl_step: fractional=True needs"):
        call(q, q, q, pos, coulomb=tn.EwaldSplitting(12.0, 0.25, 16, device="cpu"),
             dispersion=tn.DispersionSplitting(11.0, 0.25, 16, device="cpu"), fractional=True)
    with pytest.raises(AssertionError, match="nfft_ewald_lj_excl_step: batch holds point-set indices and must not require grad"):
        call(q, q, q, pos, torch.zeros(5, requires_grad=True), coulomb=spc, dispersion=spd, exclusions=ex)
    for e in (None, ex):
        with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
            call(q, None, None, pos, coulomb=spc, dispersion=spd, exclusions=e)
    # nfft_ewald_lj_step keeps its signature
    with pytest.raises(TypeError):
        tn.nfft_ewald_lj_step(q, q, q, pos, coulomb=spc, dispersion=spd, exclusions=None)
    tail = ("(Tensor pos, Tensor xs, Tensor? batch, Tensor row_start, Tensor col, Tensor weight_coulomb, Tensor weight_lj, "
            "float[] box, float alpha_coulomb, float alpha_dispersion, float r_cut) -> (Tensor, Tensor)")
    lists = (ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight)
    for name in ("_nfft_ewald_lj_excl_near", "_nfft_ewald_lj_excl_list"):
        assert str(getattr(torch.ops.torch_nfft, name).default._schema) == "torch_nfft::" + name + tail
        with pytest.raises(RuntimeError, match=name + " is currently only implemented for GPU tensors"):
            getattr(tn.ops, name[1:])(pos, torch.zeros(5, 3), None, *lists, spc.box6, 12.0, 11.0, 0.25)


def _six(A):
    A = np.asarray(A, dtype=np.float64)
    return (ctypes.c_double * 6)(A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2])


def test_c_abi_validation_without_gpu():
    """the refusals of nfft_hip_ewald_lj_step_near, and the list's own: null list pointers, a negative entry count"""
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7  # (additions only)
    for name in ("nfft_hip_ewald_lj_excl_near_workspace_bytes", "nfft_hip_ewald_lj_excl_near",
                 "nfft_hip_ewald_lj_excl_list_workspace_bytes", "nfft_hip_ewald_lj_excl_list"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)

    def problem(A=eb.O, **kw):
        f = dict(cells=(4, 5, 3), with_field=1, num_points=1000, num_columns=1, batch_size=1, alpha=14.0, r_cut=0.25, box=_six(A))
        f.update(kw)
        f["cells"] = (ctypes.c_int32 * 3)(*f["cells"])
        return _lib.EwaldBoxProblem(**f)

    ok = problem()
    sizes = (lib.nfft_hip_ewald_lj_excl_near_workspace_bytes, lib.nfft_hip_ewald_lj_excl_list_workspace_bytes)
    need = [f(ctypes.byref(ok), 12.0) for f in sizes]
    assert need[0] == lib.nfft_hip_ewald_lj_step_near_workspace_bytes(ctypes.byref(ok), 12.0) and need[1] > 0
    for f in sizes:
        for bad in (problem(cells=(5, 5, 3)), problem(cells=(2, 5, 3)), problem(with_field=2), problem(num_points=-1),
                    problem(num_columns=2), problem(batch_size=0), problem(alpha=float("nan")), problem(r_cut=0.5)):
            assert f(ctypes.byref(bad), 12.0) == -1 and _lib.last_error().startswith("Input mismatch")
        for bad_alpha in (0.0, -1.0, float("inf"), float("nan")):
            assert f(ctypes.byref(ok), bad_alpha) == -1
            assert _lib.last_error() == "Input mismatch: alpha_dispersion must be positive and finite"
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: the checks come first)

    def near(q, alpha_d=12.0, entries=10, ws=null, nbytes=0, points=one, xs=one, start=one, index=one, row_start=one, col=one,
             wc=one, wl=one, f=one, out=one):
        return lib.nfft_hip_ewald_lj_excl_near(ctypes.byref(q), alpha_d, entries, points, xs, start, index, row_start, col, wc, wl,
                                               f, out, ws, nbytes, null)

    def listk(q, alpha_d=12.0, entries=10, ws=null, nbytes=0, points=one, xs=one, row_start=one, col=one, wc=one, wl=one,
              set_start=null, f=one, out=one):
        return lib.nfft_hip_ewald_lj_excl_list(ctypes.byref(q), alpha_d, entries, points, xs, row_start, col, wc, wl, set_start, f,
                                               out, ws, nbytes, null)

    for call, size in ((near, need[0]), (listk, need[1])):
        assert call(ok) == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
        assert call(ok, ws=one, nbytes=size - 1) == _lib.EWORKSPACE
        assert call(ok, entries=0, col=null, wc=null, wl=null) == _lib.EWORKSPACE  # (an empty list needs no arrays but row_start)
        for kw in (dict(row_start=null), dict(col=null), dict(wc=null), dict(wl=null), dict(entries=-1), dict(entries=1 << 31)):
            assert call(ok, **kw) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch"), kw
        for kw in (dict(out=null), dict(points=null), dict(xs=null), dict(f=null), dict(alpha_d=float("nan"))):
            assert call(ok, **kw) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch"), kw
        assert call(problem(cells=(2, 5, 3))) == _lib.EINVAL and call(problem(r_cut=0.5)) == _lib.EINVAL
    assert near(ok, start=null) == _lib.EINVAL and near(ok, index=null) == _lib.EINVAL
    assert listk(problem(batch_size=2)) == _lib.EINVAL  # (two point sets need set_start)
    assert listk(problem(batch_size=2), set_start=one) == _lib.EWORKSPACE


def test_kernel_resource_usage():
    """both kernels of section 7s -- the list kernel of csrc/ewald_lj_excl.hip and the masked walk, step_near_kernel<LjProductLaw,
    true> of csrc/ewald_lj_step.hip: no scratch and no spills, the masked walk with the unmasked one's 8320 bytes of LDS; and
    in the list kernel's file no walk that the resource gate of tests/test_lj_step_ref.py would take for its own (the VGPR and
    SGPR figures are recorded in DESIGN.md sections 7s and 7v, not gated)"""
    from resource_usage import resource_usage
    seen = set()
    for source in ("ewald_lj_excl.hip", "ewald_lj_step.hip"):
        for name, u in sorted(resource_usage(source).items()):
            assert source == "ewald_lj_step.hip" or not re.search(r"step_near_kernel", name)
            m = re.search(r"step_near_kernelI\w*?LjProductLawELb1E|lj_excl_list_kernel", name)
            if not m:
                continue
            key = "lj_excl_list_kernel" if m.group(0) == "lj_excl_list_kernel" else "masked walk"
            seen.add((source, key))
            print(key, "VGPRs %d SGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["TotalSGPRs"], u["Occupancy"], u["LDS Size"]))
            assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
            if key == "masked walk":
                assert u["LDS Size"] == 8320
    assert seen == {("ewald_lj_step.hip", "masked walk"), ("ewald_lj_excl.hip", "lj_excl_list_kernel")}
