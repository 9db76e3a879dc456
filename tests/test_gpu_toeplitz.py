"""GPU tests of the Toeplitz normal operator A^H W A: nfft_toeplitz_kernel, nfft_normal and
nfft_inverse against the float64 restatement of test_toeplitz_ref.py and the dense float64 normal operator.

Tolerances are the ones of test_gpu_parity.py, by shape class:
  T1   2e-5  fp32 class: the device against the float64 restatement of the same algorithm.  Used for nfft_normal against
             the restatement applied with the device's own K, and as the fp32 floor wherever one is needed.
  T1N  2e-6  the adjoint against oracle.nfft_ref on the sweep sizes (a few hundred points).
  T1W  2e-6  the same for the matrix-core spreading, which 3-D grids of 64^3 cells and more take.
nfft_toeplitz_kernel is an adjoint at bandwidth 2N followed by one FFT, which keeps a relative L2 error, so K is held to
the adjoint's tolerance: T1W where the bandwidth-2N adjoint is 3-D with a grid of 64^3 or more, T1N elsewhere.

The chunk loop keeps the (re, im) planes of a column together by construction (a chunk is a whole number of pairs), so
"a chunk boundary inside a pair" is a budget that would cut a pair and is rounded down; boundaries inside a point set
occur as they are.  There is no switch that forces rocFFT's row transforms: that route is taken by its shapes (3-D grids
of 16^3 ... 64^3), which the cases below cover.

nfft_inverse: the relative error of x after the fixed number of iterations may exceed that of the same conjugate-gradient
run in float64 on the restatement by at most the factor INVERSE_FACTOR = 1.1; measured ratio on an MI355X: 1.000 in
all three cases (one point set, ragged batch, weights with a start vector).
"""
import zlib

import numpy as np
import pytest
import torch

import test_toeplitz_ref as ref
from conftest import rel_l2
from oracle import ndft, nfft_ref
from test_gpu_fastsum_routes import plane_bytes
from test_gpu_parity import T1, T1N, T1W, dev, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tn():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import torch_nfft_amd
    return torch_nfft_amd


def points(rng, d, n, B, ragged=True):
    pos = (rng.random((n, d)) - 0.5).astype(np.float32)
    if B == 1:
        return pos, None
    if ragged:
        batch = np.sort(rng.integers(0, B, n)).astype(np.int64)
        batch[0], batch[-1] = 0, B - 1
    else:
        batch = np.repeat(np.arange(B), n // B + 1)[:n].astype(np.int64)
    return pos, batch


def spectrum(rng, B, d, N, cols, cx):
    shape = (B,) + (N,) * d + cols
    x = rng.standard_normal(shape).astype(np.float32)
    if cx:
        x = (x + 1j * rng.standard_normal(shape)).astype(np.complex64)
    return x


def stage_launches(fn, stage):
    """fn() under the library's stage timers: (its result, launches of the named stage)."""
    from torch_nfft_amd import _lib
    torch.cuda.synchronize()
    _lib.profile_collect()
    _lib.profile_enable(True, [stage])
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    return out, _lib.profile_collect()[stage][1]


def apply_ref(K, x, d):
    """The restatement column by column (bounded memory at 128^3 with 17 columns)."""
    B, N = x.shape[0], x.shape[1]
    x2 = x.reshape((B,) + (N,) * d + (-1,))
    out = np.stack([ref.normal_apply(K, x2[..., c]) for c in range(x2.shape[-1])], axis=-1)
    return out.reshape(x.shape)


# ----------------------------------------------------------------------------- the kernel grid

@pytest.mark.parametrize("m", [2, 4, 8])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("d,N", [(1, 64), (2, 16), (3, 16)])
def test_kernel_against_restatement(tn, d, N, B, weighted, m):
    rng = np.random.default_rng(100 * d + 10 * B + m + (5 if weighted else 0))
    n = 700
    pos, batch = points(rng, d, n, B)
    w = (0.5 + rng.random(n)).astype(np.float32) if weighted else None
    K = tn.nfft_toeplitz_kernel(dev(pos), dev(batch), dev(w), bandwidth=N, cutoff=m)
    assert K.shape == (B,) + (2 * N,) * d and K.dtype == torch.float32
    Kref = ref.kernel_from_lags(ref.lags_nfft(np.ones(n) if w is None else w, pos, batch, N, m))
    assert np.abs(Kref.imag).max() <= 1e-12 * np.abs(Kref.real).max()
    err = rel_l2(host(K), Kref.real)
    tol = T1W if d == 3 and 2 * N >= 32 else T1N
    print("K d=%d N=%d B=%d weighted=%s m=%d: %.2e (tolerance %.0e)" % (d, N, B, weighted, m, err, tol))
    assert err < tol


# ----------------------------------------------------------------------------- one application, every FFT route

ROUTES = [
    # id, d, N, B, cols, complex x, NFFT_HIP_NO_COLFFT
    ("1d-N64", 1, 64, 3, (2,), True, False),
    ("1d-N4096", 1, 4096, 1, (), False, False),
    ("2d-N16-full", 2, 16, 3, (3,), True, False),
    ("2d-N24-full", 2, 24, 2, (), True, False),
    ("2d-N24-full-real-C2", 2, 24, 1, (2,), False, False),
    ("2d-N128-own", 2, 128, 1, (), True, False),
    ("2d-N128-own-C3", 2, 128, 2, (3,), False, False),
    ("3d-N8-rocrows", 3, 8, 2, (2,), True, False),
    ("3d-N32-rocrows", 3, 32, 1, (), False, False),
    ("3d-N32-rocrows-C3", 3, 32, 1, (3,), True, False),
    ("3d-N64-own", 3, 64, 1, (), True, False),
    ("3d-N64-own-real", 3, 64, 2, (), False, False),
    ("3d-N64-own-C2", 3, 64, 1, (2,), False, False),
    ("3d-N64-own-C3", 3, 64, 1, (3,), True, False),
    ("3d-N64-groups-C17", 3, 64, 1, (17,), True, False),
    ("3d-N32-nocolfft", 3, 32, 2, (2,), True, True),
    ("2d-N128-nocolfft", 2, 128, 1, (), True, True),
    ("3d-N64-nocolfft", 3, 64, 1, (), False, True),
]
# (one column at 2-D N = 128 and 3-D N = 64 takes the fused row kernel by default; test_fused_row_route_equals_unfused
# runs the same shapes through the three kernels of the general route)


def kernel_for(tn, rng, d, N, B, m=4, n=3000):
    pos, batch = points(rng, d, n, B)
    w = (0.5 + rng.random(n)).astype(np.float32)
    return tn.nfft_toeplitz_kernel(dev(pos), dev(batch), dev(w), bandwidth=N, cutoff=m)


@pytest.mark.parametrize("case", ROUTES, ids=[c[0] for c in ROUTES])
def test_normal_against_restatement(tn, monkeypatch, case):
    name, d, N, B, cols, cx, no_colfft = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    K = kernel_for(tn, rng, d, N, B)
    x = spectrum(rng, B, d, N, cols, cx)
    if no_colfft:
        monkeypatch.setenv("NFFT_HIP_NO_COLFFT", "1")
    y = tn.nfft_normal(dev(x), K)
    assert y.shape == x.shape and y.dtype == torch.complex64
    err = rel_l2(host(y), apply_ref(host(K).astype(np.float64), x, d))
    print("normal %s: %.2e (tolerance %.0e)" % (name, err, T1))
    assert err < T1
    # no atomics anywhere: a second call gives the same bits
    assert torch.equal(tn.nfft_normal(dev(x), K), y)


CHUNKS = [
    # id, d, N, B, cols, complex x, planes per chunk the budget is set for, NFFT_HIP_NO_COLFFT
    ("rocrows-3d-N16", 3, 16, 3, (3,), True, 5, False),   # 18 planes; 5 cuts a pair -> 4: boundaries inside sets
    ("own-2d-N64", 2, 64, 2, (3,), False, 4, False),      # 12 planes in chunks of 4: inside both sets
    ("own-3d-N64", 3, 64, 2, (), True, 3, False),         # 4 planes; 3 cuts a pair -> 2
    ("full-2d-N24", 2, 24, 3, (2,), True, 7, False),      # 12 planes; 7 -> 6: inside the second set
    ("full-3d-N16", 3, 16, 2, (3,), False, 4, True),      # 12 planes in chunks of 4 through rocFFT's 3-D transform
    ("1d-N256", 1, 256, 3, (5,), True, 9, False),         # 30 planes; 9 -> 8
]


@pytest.mark.parametrize("case", CHUNKS, ids=[c[0] for c in CHUNKS])
def test_chunked_equals_unchunked_bitwise(tn, monkeypatch, case):
    name, d, N, B, cols, cx, chunk, no_colfft = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    K = kernel_for(tn, rng, d, N, B)
    x = dev(spectrum(rng, B, d, N, cols, cx))
    if no_colfft:
        monkeypatch.setenv("NFFT_HIP_NO_COLFFT", "1")
    # the roll-off stage (here with the factor 1) runs once per chunk and direction on every route
    whole, launches = stage_launches(lambda: tn.nfft_normal(x, K), "rolloff")
    assert launches == 2
    monkeypatch.setenv("NFFT_HIP_CHUNK_BYTES", str(chunk * plane_bytes(d, N, no_colfft) + 8))
    parts, launches = stage_launches(lambda: tn.nfft_normal(x, K), "rolloff")
    monkeypatch.delenv("NFFT_HIP_CHUNK_BYTES")
    planes = 2 * B * int(np.prod(cols, dtype=np.int64))
    assert launches == 2 * -(-planes // (chunk - chunk % 2)), "the budget did not cut the planes as the case says"
    err = rel_l2(host(whole), apply_ref(host(K).astype(np.float64), host(x), d))
    print("chunked %s: unchunked error %.2e, equal bits %s" % (name, err, torch.equal(parts, whole)))
    assert err < T1
    assert torch.equal(parts, whole)


def test_chunk_of_column_groups_and_planar_remainder(tn, monkeypatch):
    """40 planes at 128^3: a full chunk of 32 goes through the 16-plane groups, the remainder of 8 planar."""
    rng = np.random.default_rng(77)
    d, N, B, cols = 3, 64, 1, (20,)
    K = kernel_for(tn, rng, d, N, B)
    x = spectrum(rng, B, d, N, cols, True)
    monkeypatch.setenv("NFFT_HIP_CHUNK_BYTES", str(32 * plane_bytes(d, N) + 8))
    y, launches = stage_launches(lambda: tn.nfft_normal(dev(x), K), "multiply")
    assert launches == 2
    err = rel_l2(host(y), apply_ref(host(K).astype(np.float64), x, d))
    print("groups + planar remainder: %.2e" % err)
    assert err < T1


@pytest.mark.parametrize("d,N,B,cx", [(3, 64, 1, True), (3, 128, 1, True), (3, 64, 3, False), (2, 128, 2, True)])
def test_fused_row_route_equals_unfused(tn, monkeypatch, d, N, B, cx):
    """One column on the planar route with the library's own row passes: both row passes and the product with K in one
    kernel (the default) against forward FFT stage, multiply kernel, adjoint FFT stage (NFFT_HIP_TOEPLITZ_FUSED=0)."""
    rng = np.random.default_rng(600 + N + B)
    K = kernel_for(tn, rng, d, N, B, n=20000)
    x = dev(spectrum(rng, B, d, N, (), cx))
    # the multiply kernel runs once per chunk on the unfused route and never on the fused one
    fused, launches = stage_launches(lambda: tn.nfft_normal(x, K), "multiply")
    assert launches == 0, "the default route did not take the fused row kernel"
    assert torch.equal(tn.nfft_normal(x, K), fused)
    monkeypatch.setenv("NFFT_HIP_TOEPLITZ_FUSED", "0")
    unfused, launches = stage_launches(lambda: tn.nfft_normal(x, K), "multiply")
    assert launches == 1
    assert torch.equal(tn.nfft_normal(x, K), unfused)
    err = rel_l2(host(fused), host(unfused).astype(np.complex128))
    print("fused vs unfused d=%d N=%d B=%d: %.2e, equal bits %s" % (d, N, B, err, torch.equal(fused, unfused)))
    assert err < T1
    if N <= 64:
        assert rel_l2(host(unfused), apply_ref(host(K).astype(np.float64), host(x), d)) < T1


# ----------------------------------------------------------------------------- against the dense normal operator

@pytest.mark.parametrize("d,N,m,n,B", [(2, 16, 2, 500, 1), (2, 16, 4, 500, 1), (2, 16, 8, 500, 1), (1, 64, 4, 300, 1),
                                       (3, 8, 4, 400, 1), (2, 32, 4, 20000, 1), (2, 16, 4, 900, 3), (3, 8, 3, 900, 3)])
def test_normal_against_dense_operator(tn, d, N, m, n, B):
    rng = np.random.default_rng(9000 + 100 * d + N + m + B)
    pos, batch = points(rng, d, n, B)
    w = (0.5 + rng.random(n)).astype(np.float32)
    x = spectrum(rng, B, d, N, (), True)
    dense = ref.normal_dense(x, w, pos, batch)
    # the bound verified on the CPU (test_toeplitz_ref.py): the relative gap of the algorithm's bandwidth-2N adjoint
    gap = rel_l2(ref.lags_nfft(w, pos, batch, N, m), ref.lags_exact(w, pos, batch, N))
    K = tn.nfft_toeplitz_kernel(dev(pos), dev(batch), dev(w), bandwidth=N, cutoff=m)
    e_toep = rel_l2(host(tn.nfft_normal(dev(x), K)), dense)
    f = tn.nfft_forward(dev(x), dev(pos), dev(batch), cutoff=m)
    comp = tn.nfft_adjoint(f * dev(w), dev(pos), dev(batch), bandwidth=N, cutoff=m)
    e_comp = rel_l2(host(comp), dense)
    print("dense d=%d N=%d m=%d n=%d B=%d: Toeplitz %.2e, composition %.2e, gap of t %.2e" % (d, N, m, n, B, e_toep, e_comp, gap))
    assert e_toep <= max(gap, T1)
    assert e_toep <= e_comp + T1


# ----------------------------------------------------------------------------- operator properties

@pytest.mark.parametrize("d,N,B,cols", [(2, 32, 2, (2,)), (3, 64, 1, ()), (1, 128, 3, ())])
def test_selfadjoint_and_positive(tn, d, N, B, cols):
    rng = np.random.default_rng(31 + d)
    K = kernel_for(tn, rng, d, N, B, n=8 * N ** min(d, 2))
    a, b = dev(spectrum(rng, B, d, N, cols, True)), dev(spectrum(rng, B, d, N, cols, True))
    Ta, Tb = tn.nfft_normal(a, K), tn.nfft_normal(b, K)
    lhs = torch.vdot(b.flatten(), Ta.flatten()).item()   # <b, T a>
    rhs = torch.vdot(Tb.flatten(), a.flatten()).item()   # <T b, a>
    scale = float(torch.linalg.vector_norm(Ta) * torch.linalg.vector_norm(b))
    print("self-adjoint d=%d: |<b,Ta> - <Tb,a>| / (|Ta| |b|) = %.2e" % (d, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= T1 * scale
    assert torch.vdot(a.flatten(), Ta.flatten()).real.item() >= 0.0


# ----------------------------------------------------------------------------- autograd

@pytest.mark.parametrize("cx", [True, False])
def test_autograd(tn, cx):
    rng = np.random.default_rng(41)
    d, N, B, cols = 2, 32, 2, (2,)
    K = kernel_for(tn, rng, d, N, B)
    x = dev(spectrum(rng, B, d, N, cols, cx)).requires_grad_(True)
    c = dev(spectrum(rng, B, d, N, cols, True)).requires_grad_(True)
    e = dev(spectrum(rng, B, d, N, cols, cx))
    y = tn.nfft_normal(x, K)
    L = (y * c.conj()).real.sum()  # Re <c, T x>
    g, = torch.autograd.grad(L, x, create_graph=True)
    Tc = tn.nfft_normal(c.detach(), K)
    expect = Tc if cx else Tc.real
    assert g.dtype == x.dtype
    assert rel_l2(host(g), host(expect)) < T1
    # double backward: g = T c (its real part) is linear in c, and its backward is the operator once more
    L2 = (g * e.conj()).real.sum() if cx else (g * e).sum()
    gc, = torch.autograd.grad(L2, c)
    assert rel_l2(host(gc), host(tn.nfft_normal(e, K))) < T1
    with pytest.raises(AssertionError, match="kernel requires grad"):
        tn.nfft_normal(x, K.clone().requires_grad_())


# ----------------------------------------------------------------------------- the iterative inverse

# Allowed ratio of the device's relative error of x after the fixed iteration count over that of the same
# conjugate-gradient run in float64 on the restatement.  Measured once on an MI355X: 1.000 for the cases below (device
# 4.376e-04 against 4.376e-04 for one point set, 1.535e-02 against 1.535e-02 for the ragged batch of three; 2.978e-03
# against 2.978e-03 in test_inverse_weights_and_start): after these iterations the error is the truncation of the
# iteration, three orders of magnitude above fp32 rounding, which the margin of 10 % leaves room for.
INVERSE_FACTOR = 1.1


@pytest.mark.parametrize("B", [1, 3])
def test_inverse(tn, B):
    rng = np.random.default_rng(51 + B)
    d, N, m, iterations = 2, 32, 3, 10
    n = 8 * N * N if B == 1 else 3 * 6 * N * N
    pos = (rng.random((n, d)) - 0.5).astype(np.float32)
    batch = None
    if B > 1:  # ragged: 4, 6 and 8 N^2 points
        batch = np.repeat(np.arange(3), [4 * N * N, 6 * N * N, 8 * N * N]).astype(np.int64)
    x_true = rng.standard_normal((B,) + (N,) * d) + 1j * rng.standard_normal((B,) + (N,) * d)
    y = ndft.ndft_forward(x_true, pos, batch)
    x, res = tn.nfft_inverse(dev(y.astype(np.complex64)), dev(pos), dev(batch), bandwidth=N, cutoff=m, iterations=iterations)
    assert x.shape == x_true.shape and x.dtype == torch.complex64
    assert res.shape == (iterations,) and res.is_cuda and res.dtype == torch.float32
    res = host(res).astype(np.float64)
    print("inverse B=%d residuals: %s" % (B, " ".join("%.3e" % r for r in res)))
    assert np.all(np.isfinite(res)) and np.all(res[1:] <= res[:-1])
    # the same iteration in float64 on the restatement
    Kref = ref.kernel_from_lags(ref.lags_nfft(np.ones(n), pos, batch, N, m)).real
    bref = nfft_ref.nfft_adjoint(y, pos, batch, N=N, m=m)
    xref, _ = ref.cg_ref(Kref, bref, iterations)
    e_dev, e_ref = rel_l2(host(x), x_true), rel_l2(xref, x_true)
    print("inverse B=%d: device error %.3e, float64 restatement %.3e, ratio %.3f" % (B, e_dev, e_ref, e_dev / e_ref))
    assert e_dev <= INVERSE_FACTOR * e_ref


def test_inverse_weights_and_start(tn):
    """weights= and x0=: conjugate gradients from x0 are x0 plus the iteration from zero on the residual's system, which
    is how the float64 run is made.  Same comparison and same factor as test_inverse."""
    rng = np.random.default_rng(57)
    d, N, m, iterations = 2, 32, 3, 6
    n = 8 * N * N
    pos = (rng.random((n, d)) - 0.5).astype(np.float32)
    w = (0.5 + rng.random(n)).astype(np.float32)
    x_true = rng.standard_normal((1, N, N)) + 1j * rng.standard_normal((1, N, N))
    x0 = (x_true + 0.3 * (rng.standard_normal((1, N, N)) + 1j * rng.standard_normal((1, N, N)))).astype(np.complex64)
    y = ndft.ndft_forward(x_true, pos, None)
    x, res = tn.nfft_inverse(dev(y.astype(np.complex64)), dev(pos), None, bandwidth=N, cutoff=m, weights=dev(w),
                             iterations=iterations, x0=dev(x0))
    res = host(res).astype(np.float64)
    assert np.all(np.isfinite(res)) and np.all(res[1:] <= res[:-1])
    Kref = ref.kernel_from_lags(ref.lags_nfft(w, pos, None, N, m)).real
    bref = nfft_ref.nfft_adjoint(y * w, pos, None, N=N, m=m)
    step, _ = ref.cg_ref(Kref, bref - ref.normal_apply(Kref, x0), iterations)
    e_dev, e_ref, e_0 = rel_l2(host(x), x_true), rel_l2(x0 + step, x_true), rel_l2(x0, x_true)
    print("inverse weights + x0: start %.3e, device %.3e, float64 restatement %.3e, ratio %.3f" % (e_0, e_dev, e_ref, e_dev / e_ref))
    assert e_ref < e_0
    assert e_dev <= INVERSE_FACTOR * e_ref


# ----------------------------------------------------------------------------- error paths

def test_input_mismatch(tn):
    K = torch.ones(2, 32, 32, device="cuda")
    x = torch.zeros(2, 16, 16, dtype=torch.complex64, device="cuda")
    assert tn.nfft_normal(x, K).shape == x.shape
    for bad_x, bad_K in [(x, torch.ones(2, 16, 16, device="cuda")),                    # kernel of the wrong M
                         (x, torch.ones(2, 64, 64, device="cuda")),
                         (x, torch.ones(3, 32, 32, device="cuda")),                    # wrong batch size
                         (x[:, :, 0], K),                                              # wrong dimension count
                         (x, torch.ones(2, 2, 2, 2, 2, device="cuda")),
                         (torch.zeros(2, 16, 12, dtype=torch.complex64, device="cuda"), K),  # x not cubic
                         (x, torch.ones(2, 32, 30, device="cuda")),
                         (x.to(torch.complex128), K), (x, K.double())]:
        with pytest.raises(RuntimeError, match="Input mismatch"):
            tn.nfft_normal(bad_x, bad_K)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_toeplitz_kernel(torch.zeros(1, 32, 30, dtype=torch.complex64, device="cuda"))
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_toeplitz_kernel(torch.zeros(1, 30, 30, dtype=torch.complex64, device="cuda"))
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.nfft_toeplitz_kernel(torch.zeros(5, 2, device="cuda"), weights=torch.ones(4, device="cuda"))
