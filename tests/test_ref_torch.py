"""CPU tests of oracle/nfft_ref_torch.py: the torch restatement against the numpy one (oracle/nfft_ref.py) and against
test_pos_grad_ref.py's window-derivative gather, relative L2 <= 1e-12 -- both are float64 evaluations of the same
formulas and differ only in the order of a few thousand additions (observed: 2e-16 .. 6e-16)."""
import numpy as np
import pytest
import torch

import test_pos_grad_ref as gref
from conftest import rel_l2
from oracle import nfft_ref, nfft_ref_torch as rt

TOL = 1e-12
BELOW_HALF = np.nextafter(np.float32(0.5), np.float32(0))


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def problem(rng, d, N, n, B, cols, complex_x, empty=()):
    """Points with the edge values of the issue in front: -1/2, 0, the largest float below 1/2, grid nodes, and points
    outside [-1/2, 1/2); point sets of ragged size, the ones listed in ``empty`` without points."""
    pos = (rng.random((n, d)) - 0.5).astype(np.float32)
    edge = [-0.5, 0.0, BELOW_HALF, 3.0 / (2 * N), -5.0 / (2 * N), 0.5, 0.75, -1.25, 1.0 / N]
    for i, v in enumerate(edge[:n]):
        pos[i, i % d] = v
    batch = None
    if B > 1:
        live = [b for b in range(B) if b not in empty]
        batch = np.sort(rng.choice(live, n)).astype(np.int64)
        batch[0], batch[-1] = live[0], live[-1]
    x = rng.standard_normal((n,) + cols)
    if complex_x:
        x = x + 1j * rng.standard_normal((n,) + cols)
    return pos, batch, x.astype(np.complex64 if complex_x else np.float32)


def spectrum(rng, B, d, N, cols, complex_x=True):
    xh = rng.standard_normal((B,) + (N,) * d + cols)
    if complex_x:
        xh = xh + 1j * rng.standard_normal(xh.shape)
    return xh.astype(np.complex64 if complex_x else np.float32)


def check_pair(pos, batch, x, xh, N, m, block=None):
    for ro in (False, True):
        ya = rt.nfft_adjoint(t(x), t(pos), t(batch), N=N, m=m, real_output=ro, block=block)
        ra = nfft_ref.nfft_adjoint(x, pos, batch, N=N, m=m, real_output=ro)
        assert ya.shape == ra.shape and ya.dtype == (torch.float64 if ro else torch.complex128)
        assert rel_l2(ya.numpy(), ra) <= TOL
        yf = rt.nfft_forward(t(xh), t(pos), t(batch), m=m, real_output=ro, block=block)
        rf = nfft_ref.nfft_forward(xh, pos, batch, m=m, real_output=ro)
        assert yf.shape == rf.shape and yf.dtype == (torch.float64 if ro else torch.complex128)
        assert rel_l2(yf.numpy(), rf) <= TOL


# d, N, m, n, B, cols, complex x, empty point sets
CASES = [
    (1, 64, 1, 200, 1, (), False, ()),
    (1, 100, 6, 150, 3, (2,), True, (1,)),
    (1, 12, 8, 50, 1, (), True, ()),
    (2, 16, 2, 150, 3, (), False, (1,)),
    (2, 20, 5, 120, 1, (2, 2), True, ()),
    (2, 48, 4, 200, 4, (3,), False, (2,)),
    (2, 12, 7, 80, 1, (), True, ()),
    (3, 8, 3, 100, 2, (2,), True, ()),
    (3, 12, 4, 80, 4, (), False, (1, 2)),
    (3, 16, 4, 120, 1, (2, 1, 2), False, ()),
    (3, 20, 2, 100, 1, (), True, ()),
    (3, 8, 8, 20, 1, (), False, ()),
]


@pytest.mark.parametrize("d,N,m,n,B,cols,cx,empty", CASES)
def test_adjoint_and_forward_match_numpy_oracle(d, N, m, n, B, cols, cx, empty):
    rng = np.random.default_rng(1000 * d + 10 * N + m)
    pos, batch, x = problem(rng, d, N, n, B, cols, cx, empty)
    check_pair(pos, batch, x, spectrum(rng, B, d, N, cols), N, m)


@pytest.mark.parametrize("d,N,m,block", [(1, 48, 3, 7), (2, 16, 4, 33), (3, 8, 2, 50), (3, 12, 1, 1)])
def test_chunked_paths_with_a_small_block(d, N, m, block):
    """Blocks of a few points: every loop over blocks runs several times, with a last partial block."""
    rng = np.random.default_rng(7 + d)
    n = 101 if block > 1 else 12
    pos, batch, x = problem(rng, d, N, n, 3, (2,), True, (1,))
    xh = spectrum(rng, 3, d, N, (2,))
    check_pair(pos, batch, x, xh, N, m, block=block)
    w = rng.standard_normal((n, 4))
    got = rt.forward_pos_grad(t(xh), t(pos), t(batch), m, False, t(w), block=block)
    assert rel_l2(got.numpy(), gref.pos_grad(xh, pos, batch, m, False, w)) <= TOL


@pytest.mark.parametrize("planes", [1, 2])
def test_column_groups_with_a_partial_last_group(monkeypatch, planes):
    """Columns are processed in groups that fit a memory budget: with room for one and for two planes of this grid,
    three columns run as 1 + 1 + 1 and as 2 + 1."""
    d, N, m, n = 3, 8, 3, 90
    monkeypatch.setattr(rt, "GROUP_BYTES", planes * 3 * (2 * N) ** d * 16)
    rng = np.random.default_rng(21)
    pos, batch, x = problem(rng, d, N, n, 2, (3,), True)
    xh = spectrum(rng, 2, d, N, (3,))
    assert rt._group(3, d, N, torch.float64) == planes
    check_pair(pos, batch, x, xh, N, m, block=40)
    g = rt.spread(t(x), t(pos), t(batch), N, m)
    assert rel_l2(g.numpy(), nfft_ref.spread(x, pos, batch, N, m)) <= TOL
    for ro in (False, True):
        w = rng.standard_normal((n, 3 if ro else 6))
        got = rt.forward_pos_grad(t(xh), t(pos), t(batch), m, ro, t(w), block=40)
        assert rel_l2(got.numpy(), gref.pos_grad(xh, pos, batch, m, ro, w)) <= TOL


def test_empty_point_set_at_the_end():
    """An empty last point set: the adjoint cannot know of it (B = batch[-1] + 1, core_cuda.cu:60), the forward refuses
    the spectrum with one set more ('Input mismatch'), in both restatements alike."""
    rng = np.random.default_rng(5)
    pos, batch, x = problem(rng, 2, 16, 90, 3, (2,), False, (1,))
    ya = rt.nfft_adjoint(t(x), t(pos), t(batch), N=16, m=3)
    assert ya.shape == (3, 16, 16, 2) and float(ya[1].abs().max()) == 0.0
    assert rel_l2(ya.numpy(), nfft_ref.nfft_adjoint(x, pos, batch, N=16, m=3)) <= TOL
    xh = spectrum(rng, 4, 2, 16, (2,))
    with pytest.raises(AssertionError):
        nfft_ref.nfft_forward(xh, pos, batch, m=3)
    with pytest.raises(AssertionError):
        rt.nfft_forward(t(xh), t(pos), t(batch), m=3)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_no_points(d):
    """n = 0: a zero spectrum of the right shape, an empty forward result."""
    N, m = 8, 2
    pos = np.zeros((0, d), np.float32)
    ya = rt.nfft_adjoint(t(np.zeros((0, 2), np.float32)), t(pos), None, N=N, m=m)
    assert ya.shape == (1,) + (N,) * d + (2,) and ya.dtype == torch.complex128 and float(ya.abs().max()) == 0.0
    rng = np.random.default_rng(0)
    xh = spectrum(rng, 1, d, N, (2,))
    yf = rt.nfft_forward(t(xh), t(pos), None, m=m)
    assert yf.shape == (0, 2) and yf.dtype == torch.complex128
    assert rt.forward_pos_grad(t(xh), t(pos), None, m, True, t(np.zeros((0, 2)))).shape == (0, d)


def test_spread_and_taps_match_numpy_oracle():
    rng = np.random.default_rng(3)
    pos, batch, x = problem(rng, 3, 12, 70, 2, (2,), True)
    shift, psi = rt.window_taps(t(pos), 12, 3)
    rshift, rpsi = nfft_ref.window_taps(pos, 12, 3)
    assert np.array_equal(shift.numpy(), rshift) and rel_l2(psi.numpy(), rpsi) <= TOL
    assert rel_l2(rt.phi_hat_inv(12, 3).numpy(), nfft_ref.phi_hat_inv(12, 3)) <= TOL
    g = rt.spread(t(x), t(pos), t(batch), 12, 3, block=16)
    assert rel_l2(g.numpy(), nfft_ref.spread(x, pos, batch, 12, 3)) <= TOL


@pytest.mark.parametrize("d,N,m,n,B,cols,cx,ro", [
    (1, 32, 3, 60, 2, (2,), True, False),
    (2, 16, 4, 80, 3, (), True, True),
    (2, 12, 2, 70, 1, (3,), False, False),
    (3, 8, 3, 60, 2, (2,), True, False),
    (3, 12, 5, 40, 1, (), False, True),
])
def test_forward_pos_grad_matches_window_derivative_gather(d, N, m, n, B, cols, cx, ro):
    rng = np.random.default_rng(40 + d + N)
    pos, batch, _ = problem(rng, d, N, n, B, (), False)
    xh = spectrum(rng, B, d, N, cols, cx)
    C = int(np.prod(cols)) if cols else 1
    w = rng.standard_normal((n, C if ro else 2 * C))
    got = rt.forward_pos_grad(t(xh), t(pos), t(batch), m, ro, t(w))
    assert got.shape == (n, d) and got.dtype == torch.float64
    assert rel_l2(got.numpy(), gref.pos_grad(xh, pos, batch, m, ro, w)) <= TOL


@pytest.mark.parametrize("shared,cx,ccx", [(True, False, False), (False, False, True), (False, True, False), (True, True, True)])
def test_fastsum_matches_numpy_oracle(shared, cx, ccx):
    rng = np.random.default_rng(11)
    d, N, m, ns, nt = 2, 16, 4, 90, 70
    src, sb, x = problem(rng, d, N, ns, 2, (2,), cx)
    tgt, tb, _ = problem(rng, d, N, nt, 2, (), False)
    coeffs = rng.standard_normal((N,) * d)
    if ccx:
        coeffs = coeffs + 1j * rng.standard_normal((N,) * d)
    if shared:
        got = rt.nfft_fastsum(t(x), t(coeffs), t(src), batch=t(sb), m=m)
        ref = nfft_ref.nfft_fastsum(x, coeffs, src, batch=sb, m=m)
    else:
        got = rt.nfft_fastsum(t(x), t(coeffs), t(src), t(tgt), t(sb), t(tb), m=m)
        ref = nfft_ref.nfft_fastsum(x, coeffs, src, tgt, sb, tb, m=m)
    assert got.shape == ref.shape and got.is_complex() == np.iscomplexobj(ref)
    assert rel_l2(got.numpy(), ref) <= TOL


def test_float32_mode_is_the_same_code_in_single_precision():
    """The yardstick mode: float32 / complex64 throughout, and within single-precision distance of the oracle."""
    rng = np.random.default_rng(2)
    pos, batch, x = problem(rng, 3, 16, 300, 2, (2,), True)
    xh = spectrum(rng, 2, 3, 16, (2,))
    ya = rt.nfft_adjoint(t(x), t(pos), t(batch), N=16, m=4, dtype=torch.float32)
    yf = rt.nfft_forward(t(xh), t(pos), t(batch), m=4, dtype=torch.float32)
    gp = rt.forward_pos_grad(t(xh), t(pos), t(batch), 4, True, t(x.real), dtype=torch.float32)
    assert ya.dtype == yf.dtype == torch.complex64 and gp.dtype == torch.float32
    assert 1e-9 < rel_l2(ya.numpy(), nfft_ref.nfft_adjoint(x, pos, batch, N=16, m=4)) < 2e-6
    assert 1e-9 < rel_l2(yf.numpy(), nfft_ref.nfft_forward(xh, pos, batch, m=4)) < 2e-6
    assert 1e-9 < rel_l2(gp.numpy(), gref.pos_grad(xh, pos, batch, 4, True, x.real)) < 4e-6
    with pytest.raises(TypeError):
        rt.nfft_adjoint(t(x), t(pos), t(batch), N=16, m=4, dtype=torch.float16)


def test_peak_bytes_counts_the_grids():
    """Two to three complex128 grids of 1024^3 plus the band and the points: 35 .. 60 GB for the N = 512 cases."""
    peak = rt.peak_bytes(3, 512, 4, 1_000_000)
    assert 2 * 1024 ** 3 * 16 < peak < 3.5 * 1024 ** 3 * 16
    assert rt.peak_bytes(3, 512, 4, 1_000_000, dtype=torch.float32) < 0.55 * peak
    assert rt.peak_bytes(2, 16, 4, 0) > 0
