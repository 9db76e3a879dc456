"""GPU tests of the gradient of nfft_fastsum with respect to its sources and targets.

Every case of test_gpu_fastsum_routes.ROUTES (each asserts its FFT route), with real and complex coefficient arrays that are
not even, is checked against
  (a) the float64 restatement: the grids of oracle.nfft_ref (band = c A_s(x), H = conj(c) A_t(dy)), gathered with the
      window's derivative by test_pos_grad_ref.pos_grad -- relative L2 <= TRF (not on the 3-D grids of 64^3 cells and up,
      where the float64 spreading takes minutes);
  (b) the same gradients through the hand-written composition nfft_forward(c * nfft_adjoint(x, s), t) under autograd,
      whose point gradients test_gpu_pos_grad.py pins: relative L2 <= TC;
  (c) dense float64 autograd of the exact trigonometric sum where N^d (ns + nt) is small: relative L2 <= TE[m].
Tolerances (fp32): TRF and TC are the fastsum's own T1 = 2e-5 of test_gpu_fastsum_routes.py (observed: 4e-7 .. 1.1e-6);
TE = the transforms' TE[m] of test_gpu_pos_grad.py times 5 (two transforms and a spectral product instead of one
transform; observed at m = 6: 1e-6 .. 9e-6).  Where the adjoint spreads with atomics the order of the additions varies
from call to call, so results that depend on a spreading are compared at T_ENTRY, not bit for bit: x.grad against today's
call, y of the band-returning fastsum, and repeated sources' gradients.  The targets' gradient gathers the saved band
without atomics and repeats bit for bit.
"""
import numpy as np
import pytest
import torch

import test_pos_grad_ref as ref
from conftest import rel_l2
from oracle import coeffs_ref, nfft_ref
from test_gpu_fastsum_routes import ROUTES, chunk_env, heavy, make_data, rolloff_launches, route_of
from test_gpu_pos_grad import TE as TE_TRANSFORM

pytestmark = pytest.mark.gpu

TRF = 2e-5
TC = 2e-5
T_ENTRY = 2e-6  # the same arithmetic, only the order of the adjoint's spreading atomics differs (test_gpu_fastsum_routes.py)
TE = {m: 5 * v for m, v in TE_TRANSFORM.items()}


@pytest.fixture(scope="module")
def tn():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import torch_nfft_amd
    return torch_nfft_amd


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def coeff_arrays(rng, d, N):
    """A real array and a complex one, neither even nor Hermitian."""
    cr = rng.standard_normal((N,) * d).astype(np.float32)
    cc = (rng.standard_normal((N,) * d) + 1j * rng.standard_normal((N,) * d)).astype(np.complex64)
    return cr, cc


def upstream(rng, nt, C, cx):
    dy = rng.standard_normal((nt, C))
    if cx:
        dy = dy + 1j * rng.standard_normal((nt, C))
    return dy.astype(np.complex64 if cx else np.float32)


def run(tn, x, coeffs, src, tgt, sb, tb, m, dy, shared, grads=("x", "s", "t")):
    """(x.grad, sources.grad, targets.grad) of <dy, nfft_fastsum(...)>; shared: one tensor for both point sets."""
    xt = dev(x).requires_grad_("x" in grads)
    s = dev(src).requires_grad_("s" in grads or "t" in grads and shared)
    t = s if shared else dev(tgt).requires_grad_("t" in grads)
    batched = sb is not None
    y = tn.nfft_fastsum(xt, dev(coeffs), s, t, dev(sb) if batched else None, dev(tb) if batched else None, cutoff=m)
    y.backward(dev(dy))
    return xt.grad, s.grad, (None if shared else t.grad)


def composition(tn, x, coeffs, src, tgt, sb, tb, m, dy, shared):
    """The same gradients through nfft_forward(c * nfft_adjoint(x, s), t) (the transforms' own point gradients)."""
    N, d = coeffs.shape[0], coeffs.ndim
    xt = dev(x).requires_grad_(True)
    s = dev(src).requires_grad_(True)
    t = s if shared else dev(tgt).requires_grad_(True)
    band = tn.nfft_adjoint(xt, s, dev(sb), bandwidth=N, cutoff=m)
    c = dev(coeffs).reshape((1,) + (N,) * d + (1,) * (band.dim() - 1 - d))
    y = tn.nfft_forward(band * c, t, dev(tb), cutoff=m, real_output=not np.iscomplexobj(x))
    y.backward(dev(dy))
    return xt.grad, s.grad, (None if shared else t.grad)


def restatement(x, coeffs, src, tgt, sb, tb, N, m, dy):
    """(dsources, dtargets) float64: the two weighted window-derivative gathers of the derivation."""
    cx = np.iscomplexobj(x)
    ns, nt = len(src), len(tgt)
    cshape = (1,) + coeffs.shape + (1,)
    x2, dy2 = x.reshape(ns, -1), dy.reshape(nt, -1)
    band = nfft_ref.nfft_adjoint(x2, src, sb, N=N, m=m) * coeffs.astype(np.complex128).reshape(cshape)
    h = nfft_ref.nfft_adjoint(dy2, tgt, tb, N=N, m=m) * np.conj(coeffs.astype(np.complex128)).reshape(cshape)
    dt = ref.pos_grad(band, tgt, tb, m, not cx, ref.real_columns(dy2, nt))
    ds = ref.pos_grad(h, src, sb, m, not cx, ref.real_columns(x2, ns))
    return ds, dt


def dense_exact(x, coeffs, src, tgt, sb, tb, dy):
    """(dsources, dtargets) float64 of <dy, y> for the exact sum y_i = sum_j K(s_j - t_i) x_j (real part for a real x)."""
    N, d = coeffs.shape[0], coeffs.ndim
    k = np.stack(np.meshgrid(*([np.arange(-N // 2, N // 2)] * d), indexing="ij"), -1).reshape(-1, d)
    kt = torch.tensor(k, dtype=torch.float64)
    c = torch.tensor(coeffs.reshape(-1).astype(np.complex128))
    s = torch.tensor(src.astype(np.float64), requires_grad=True)
    t = torch.tensor(tgt.astype(np.float64), requires_grad=True)
    Kst = torch.exp(-2j * np.pi * (t @ kt.T)) @ (c[:, None] * torch.exp(2j * np.pi * (s @ kt.T)).T)  # [nt, ns]
    if sb is not None:
        Kst = Kst * torch.tensor(tb[:, None] == sb[None, :], dtype=torch.float64)
    y = Kst @ torch.tensor(x.reshape(len(src), -1).astype(np.complex128))
    g = torch.tensor(dy.reshape(len(tgt), -1).astype(np.complex128))
    loss = (y.real * g.real + y.imag * g.imag).sum() if np.iscomplexobj(x) else (y.real * g.real).sum()
    loss.backward()
    return s.grad.numpy(), t.grad.numpy()


def combine(ds, dt, shared):
    return ds + dt if shared else ds


# ----------------------------------------------------------------------------- every route, three references

@pytest.mark.parametrize("case", ROUTES, ids=[c.name for c in ROUTES])
def test_fastsum_point_gradients_route(tn, monkeypatch, case):
    """Fails without the feature: nfft_fastsum raised AssertionError as soon as sources or targets required grad."""
    assert route_of(case) == case.route
    if case.chunk is not None:
        monkeypatch.setenv("NFFT_HIP_CHUNK_BYTES", chunk_env(case))
    if case.no_colfft:
        monkeypatch.setenv("NFFT_HIP_NO_COLFFT", "1")
    rng, src, tgt, sb, tb, x = make_data(case, 3000 + ROUTES.index(case))
    sb_, tb_ = (sb, tb) if case.B > 1 else (None, None)
    dy = upstream(rng, case.nt, case.C, case.cx)
    small = case.N ** case.d * (case.ns + case.nt) <= 2e7 and case.C * case.B <= 8
    for coeffs in coeff_arrays(rng, case.d, case.N):
        gx, gs, gt = run(tn, x, coeffs, src, tgt, sb_, tb_, case.m, dy, case.shared)
        assert gs.shape == (case.ns, case.d) and gs.dtype == torch.float32 and bool(torch.isfinite(gs).all())
        cx_, cs, ct = composition(tn, x, coeffs, src, tgt, sb_, tb_, case.m, dy, case.shared)
        e_c = [rel_l2(host(gs), host(cs))] + ([] if case.shared else [rel_l2(host(gt), host(ct))])
        e_x = rel_l2(host(gx), host(cx_)) if not np.iscomplexobj(coeffs) else 0.0
        print(case.name, "complex c" if np.iscomplexobj(coeffs) else "real c", "composition", e_c, "dx", e_x)
        assert max(e_c) < TC and e_x < TC
        if not heavy(case):
            ds, dt = restatement(x, coeffs, src, tgt, sb_, tb_, case.N, case.m, dy)
            e_r = [rel_l2(host(gs), combine(ds, dt, case.shared))] + ([] if case.shared else [rel_l2(host(gt), dt)])
            print("  restatement", e_r)
            assert max(e_r) < TRF
        if small:
            es, et = dense_exact(x, coeffs, src, tgt, sb_, tb_, dy)
            e_e = [rel_l2(host(gs), combine(es, et, case.shared))] + ([] if case.shared else [rel_l2(host(gt), et)])
            print("  exact", e_e)
            assert max(e_e) < TE[case.m]
    tn.ops.check_status()


# ----------------------------------------------------------------------------- x gradient, plans, launches, repeats

def _case(name):
    return next(c for c in ROUTES if c.name == name)


@pytest.mark.parametrize("name", ["fused-2d", "rocrows-3d-N16-C3", "ownplanar-2d-N64-C1"])
def test_dx_unchanged(tn, name):
    """Only x requires grad: x.grad is today's swapped fastsum (the same call: equal up to the order of the spreading
    atomics).  With the points too (real coefficients) dx comes from the fused gather and agrees to 1e-5."""
    case = _case(name)
    rng, src, tgt, sb, tb, x = make_data(case, 77)
    sb_, tb_ = (sb, tb) if case.B > 1 else (None, None)
    dy = upstream(rng, case.nt, case.C, case.cx)
    for coeffs in coeff_arrays(rng, case.d, case.N):
        gx, _, _ = run(tn, x, coeffs, src, tgt, sb_, tb_, case.m, dy, case.shared, grads=("x",))
        s = dev(src)
        t = s if case.shared else dev(tgt)
        today = tn.ops.nfft_fastsum(t, s, dev(dy), dev(coeffs), dev(tb_), dev(sb_), case.m)
        assert torch.equal(gx, today) if case.route == ["fused"] else rel_l2(host(gx), host(today)) < T_ENTRY
        gx2, _, _ = run(tn, x, coeffs, src, tgt, sb_, tb_, case.m, dy, case.shared)
        assert rel_l2(host(gx2), host(today)) < 1e-5


@pytest.mark.parametrize("complex_coeffs", [False, True], ids=["real-c", "complex-c"])
def test_backward_plans_nothing_and_launch_counts(tn, complex_coeffs):
    """Planned route: the backward takes the forward's plans (no miss) and runs one adjoint and two forward FFT stages
    (real c; complex c: two adjoints and three, the swapped fastsum for dx included)."""
    case = _case("rocrows-3d-N16-C3")
    assert case.route == ["rocrows"]
    rng, src, tgt, sb, tb, x = make_data(case, 78)
    dy = upstream(rng, case.nt, case.C, case.cx)
    cr, cc = coeff_arrays(rng, case.d, case.N)
    coeffs = dev(cc if complex_coeffs else cr)
    xt = dev(x).requires_grad_(True)
    s = dev(src).requires_grad_(True)
    t = dev(tgt).requires_grad_(True)
    sb_, tb_, dyt = dev(sb), dev(tb), dev(dy)

    def step():
        y = tn.nfft_fastsum(xt, coeffs, s, t, sb_, tb_, cutoff=case.m)
        before = tn.ops.plan_cache_stats()["misses"]
        y.backward(dyt)
        return before

    step()  # plans for these tensors enter the cache
    m0 = tn.ops.plan_cache_stats()["misses"]
    m1, launches = rolloff_launches(step)
    assert m1 == m0 and tn.ops.plan_cache_stats()["misses"] == m0
    assert launches == 2 + (5 if complex_coeffs else 3)


@pytest.mark.parametrize("name", ["fused-2d", "rocrows-3d-N16-C1", "ownplanar-3d-N64-C1"])
def test_repeated_backward(tn, name):
    """Two backward calls of one graph: the targets' gradient bit for bit (no atomics after the saved band)."""
    case = _case(name)
    rng, src, tgt, sb, tb, x = make_data(case, 79)
    sb_, tb_ = (dev(sb), dev(tb)) if case.B > 1 else (None, None)
    dy = dev(upstream(rng, case.nt, case.C, case.cx))
    coeffs = dev(coeff_arrays(rng, case.d, case.N)[0])
    s = dev(src).requires_grad_(True)
    t = dev(tgt).requires_grad_(True)
    y = tn.nfft_fastsum(dev(x), coeffs, s, t, sb_, tb_, cutoff=case.m)
    gs1, gt1 = torch.autograd.grad(y, (s, t), dy, retain_graph=True)
    gs2, gt2 = torch.autograd.grad(y, (s, t), dy)
    assert torch.equal(gt1, gt2)
    assert rel_l2(host(gs1), host(gs2)) < T_ENTRY


def test_directional_derivative(tn):
    """<grad, delta> against a central difference of the loss in the points (float32, h = 1e-3: relative 1e-2)."""
    rng = np.random.default_rng(80)
    d, N, m, ns, nt = 2, 32, 6, 400, 300
    src = (0.4 * (rng.random((ns, d)) - 0.5)).astype(np.float32)
    tgt = (0.4 * (rng.random((nt, d)) - 0.5)).astype(np.float32)
    coeffs = dev(coeffs_ref.gaussian_analytic_coeffs(0.12, d, N).astype(np.float32))
    x = dev(rng.standard_normal((ns, 2)).astype(np.float32))
    w = dev(rng.standard_normal((nt, 2)).astype(np.float32))
    s = dev(src).requires_grad_(True)
    t = dev(tgt).requires_grad_(True)
    (tn.nfft_fastsum(x, coeffs, s, t, cutoff=m) * w).sum().backward()
    ds, dt = dev(rng.standard_normal((ns, d)).astype(np.float32)), dev(rng.standard_normal((nt, d)).astype(np.float32))
    an = float((s.grad * ds).sum() + (t.grad * dt).sum())
    h = 1e-3

    def loss(sign):
        with torch.no_grad():
            return float((tn.nfft_fastsum(x, coeffs, dev(src) + sign * h * ds, dev(tgt) + sign * h * dt, cutoff=m)
                          * w).double().sum())

    fd = (loss(1) - loss(-1)) / (2 * h)
    assert abs(fd - an) <= 1e-2 * abs(an), (fd, an)


# ----------------------------------------------------------------------------- kernel matrices reach the user's points

def gaussian_pos_grad_exact(pos, batch, X, G, sigma, adjacency=False):
    """d/dpos of <G, M X> in float64, M the dense Gaussian Gram matrix exp(-|p_i - p_j|^2 / sigma^2) of each point set,
    or its sym-normalised adjacency D^-1/2 K D^-1/2 (D = K 1)."""
    p = torch.tensor(pos.astype(np.float64), requires_grad=True)
    out = 0.0
    for b in np.unique(batch):
        sel = torch.tensor(batch == b)
        q = p[sel]
        K = torch.exp(-((q[:, None, :] - q[None, :, :]) ** 2).sum(-1) / sigma ** 2)
        if adjacency:
            r = K.sum(1).rsqrt()
            K = r[:, None] * K * r[None, :]
        out = out + (torch.tensor(G[batch == b].astype(np.float64)) *
                     (K @ torch.tensor(X[batch == b].astype(np.float64)))).sum()
    out.backward()
    return p.grad.numpy()


@pytest.mark.parametrize("analytic", [True, False], ids=["analytic", "interpolated"])
def test_gaussian_kernel_gradient_reaches_points(tn, analytic):
    """GaussianKernel (centring and scaling are torch ops) on a planned 3-D route, as test_gram_matrix_3d_planned:
    pos.grad of <G, kern(pos) @ X> against dense float64 autograd."""
    n, b, dim, diameter, N, m = 150, 2, 3, 10.0, 32, 4
    rng = np.random.default_rng(81)
    pos = (diameter * (rng.random((n * b, dim)) - 0.5)).astype(np.float32)
    batch = np.repeat(np.arange(b), n).astype(np.int64)
    X = rng.standard_normal((n * b, 3)).astype(np.float32)
    G = rng.standard_normal((n * b, 3)).astype(np.float32)
    kern = tn.GaussianKernel(diameter, dim, N, m, shift_by_center=True, max_infinity_norm=diameter / 2, reg_degree=0,
                             analytic=analytic)
    assert kern.coeffs.is_complex() != analytic
    p = dev(pos).requires_grad_(True)
    ((kern(p, batch=dev(batch)) @ dev(X)) * dev(G)).sum().backward()
    e = rel_l2(host(p.grad), gaussian_pos_grad_exact(pos, batch, X, G, diameter))
    print("GaussianKernel", "analytic" if analytic else "interpolated", e)
    assert e < 1e-2


def test_adjacency_sym_gradient_reaches_points(tn):
    """A sym-normalised AdjacencyMatrix: the degrees are a fastsum of the points as well.  (sigma is a quarter of the
    spread: with a kernel that is flat over the point set the normalised gradient is a small difference of large terms.)"""
    n, dim, spread, sigma, N, m = 200, 2, 4.0, 1.0, 64, 6
    rng = np.random.default_rng(82)
    pos = (spread * (rng.random((n, dim)) - 0.5)).astype(np.float32)
    batch = np.zeros(n, dtype=np.int64)
    X = rng.standard_normal((n, 2)).astype(np.float32)
    G = rng.standard_normal((n, 2)).astype(np.float32)
    kern = tn.GaussianKernel(sigma, dim, N, m, shift_by_center=True, max_infinity_norm=spread / 2, reg_degree=0,
                             analytic=True)
    p = dev(pos).requires_grad_(True)
    A = kern.adjacency_matrix(p, normalization="sym")
    ((A @ dev(X)) * dev(G)).sum().backward()
    e = rel_l2(host(p.grad), gaussian_pos_grad_exact(pos, batch, X, G, sigma, adjacency=True))
    print("AdjacencyMatrix sym", e)
    assert e < 1e-2


# ----------------------------------------------------------------------------- edges

@pytest.mark.parametrize("complex_x", [False, True])
def test_empty_sides_and_columns(tn, complex_x):
    rng = np.random.default_rng(83)
    d, N, m = 3, 16, 4
    c = dev(coeff_arrays(rng, d, N)[0])
    for ns, nt, C in ((0, 50, 2), (50, 0, 2), (50, 40, 0), (1500, 1200, 1)):
        s = dev((0.4 * (rng.random((ns, d)) - 0.5)).astype(np.float32)).requires_grad_(True)
        t = dev((0.4 * (rng.random((nt, d)) - 0.5)).astype(np.float32)).requires_grad_(True)
        x = torch.ones((ns, C), dtype=torch.complex64 if complex_x else torch.float32, device="cuda").requires_grad_(True)
        y = tn.nfft_fastsum(x, c, s, t, cutoff=m)
        y.backward(torch.ones_like(y))
        assert s.grad.shape == (ns, d) and t.grad.shape == (nt, d) and x.grad.shape == (ns, C)
        if ns == 0 or nt == 0 or C == 0:
            assert not s.grad.any() and not t.grad.any() and not x.grad.any()
    coeffs = c.clone().requires_grad_(True)
    s = dev((0.4 * (rng.random((30, d)) - 0.5)).astype(np.float32)).requires_grad_(True)
    with pytest.raises(AssertionError):
        tn.nfft_fastsum(torch.ones((30, 1), device="cuda"), coeffs, s, cutoff=m)
    tn.ops.check_status()


def test_band_operator_matches_fastsum(tn):
    """_nfft_fastsum_band: the y of nfft_fastsum (same route; equal up to the order of the spreading atomics),
    band = c * A_s(x)."""
    for name in ("fused-2d", "rocrows-3d-N16-C3", "ownplanar-2d-N64-C3"):
        case = _case(name)
        rng, src, tgt, sb, tb, x = make_data(case, 84)
        for coeffs in coeff_arrays(rng, case.d, case.N):
            s = dev(src)
            t = s if case.shared else dev(tgt)
            sbt = dev(sb)
            args = (s, t, dev(x), dev(coeffs), sbt, sbt if case.shared else dev(tb), case.m)
            y0 = tn.ops.nfft_fastsum(*args)
            y1, band = tn.ops.nfft_fastsum_band(*args)
            assert rel_l2(host(y1), host(y0)) < T_ENTRY
            assert band.shape == (case.B,) + (case.N,) * case.d + (case.C,) and band.dtype == torch.complex64
            ref_band = nfft_ref.nfft_adjoint(x, src, sb, N=case.N, m=case.m) * \
                coeffs.astype(np.complex128).reshape((1,) + coeffs.shape + (1,))
            assert rel_l2(host(band), ref_band) < TRF
