"""nfft_fastsum on every FFT route of its adjoint, on chunked plane loops and at the edges.

The fast summation has no kernel of its own: the kernel's Fourier coefficients are multiplied in by whichever kernel
ends the adjoint's FFT stage, and that depends on the route ``make_route`` (csrc/api.hip) picks:

  fused      smallgrid.hip small_adjoint_kernel   (grid in one workgroup's LDS, both point sets few enough taps)
  full       spectral.hip deconv_adjoint_kernel   (rocFFT; 1-D, 2-D below 128^2, non-power-of-two, NO_COLFFT)
  rocrows    colfft.hip adj_axis0_kernel          (3-D, M = 16..64)
  ownplanar  colfft.hip adj_axis0_kernel          (2-D / 3-D, M = 128..1024; 3-D chunks of fewer than 32 planes)
  ownci      colfft.hip adj_axis0_ci_kernel       (3-D, M >= 128, two or more columns, chunks of >= 32 planes)

Each has its own frequency indexing and its own Hermitian-mirror branch.  Every case of ROUTES below states the route
it takes; ``route_of`` restates the rules of ``small_grid_route`` / ``make_route`` / ``Route::chunk_fft`` and the
library confirms what it can see of them (``nfft_hip_plan_needed``; the ``rolloff`` stage's launch count, one per chunk
and direction).  The coefficient arrays are never even (c[k] != c[-k]), so a slip in a mirror branch shows.

References:
  (a) oracle.nfft_ref.nfft_fastsum (float64 restatement of the algorithm) at T1; on the 3-D N = 64 grids one
      (point set, column) at a time, for the first and last column of each chunk.
  (b) closed forms for sparse coefficient arrays (a single frequency; a handful on the k = 0 planes, the Nyquist planes
      k_a = -N/2, the band corner and the mirror half), at every target and column, at T2[m].
  (c) oracle.ndft.ndft_fastsum where N^d (ns + nt) is small, at T2[m].
The closed forms put all weight on a few frequencies, the band edge among them, where the window's error is largest:
at m = 4 a lone corner frequency is off by ~6e-4 > T2[4], at m = 6 by < 1e-5.  The cases therefore run at m = 6.
"""
import collections
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import coeffs_ref, ndft, nfft_ref

pytestmark = pytest.mark.gpu

T1 = 2e-5
T2 = {1: 2e-1, 2: 2e-2, 3: 3e-3, 4: 5e-4, 5: 1e-4, 6: 5e-5, 7: 3e-5, 8: 2e-5}  # test_gpu_parity.py
T_ENTRY = 2e-6  # entry points of the same route: only the order of the spreading atomics differs


@pytest.fixture(scope="module")
def tn():
    import torch_nfft_amd
    return torch_nfft_amd


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------- the route table

Case = collections.namedtuple("Case", "name d N m ns nt B C cx shared chunk no_colfft route")
# shared: the targets are the sources (nt = ns); chunk: planes per chunk of the plane loop (None: one chunk);
# route: the FFT route of each chunk, in order
ROUTES = [
    Case("fused-1d", 1, 8, 6, 300, 200, 2, 3, False, False, None, False, ["fused"]),
    Case("fused-2d", 2, 8, 6, 120, 100, 2, 2, True, False, None, False, ["fused"]),
    Case("fused-3d", 3, 8, 6, 40, 30, 2, 2, False, False, None, False, ["fused"]),
    Case("full-1d-N4096", 1, 4096, 6, 2000, 1500, 2, 2, True, False, None, False, ["full"]),
    Case("full-2d-N48", 2, 48, 6, 600, 600, 2, 3, False, True, None, False, ["full"]),
    Case("full-3d-N12", 3, 12, 6, 500, 400, 2, 2, True, False, None, False, ["full"]),
    Case("full-3d-N20", 3, 20, 6, 800, 700, 1, 1, False, False, None, False, ["full"]),
    Case("full-3d-N16-nocolfft", 3, 16, 6, 600, 500, 2, 3, False, False, None, True, ["full"]),
    Case("rocrows-3d-N16-C1", 3, 16, 6, 1500, 1200, 2, 1, False, False, None, False, ["rocrows"]),
    Case("rocrows-3d-N16-C3", 3, 16, 6, 1500, 1500, 2, 3, True, True, None, False, ["rocrows"]),
    # (more than 30 000 points at m > 3: the 64^3 grid takes the matrix-core spreading kernels)
    Case("rocrows-3d-N32-C1-mfma", 3, 32, 6, 31000, 1500, 1, 1, True, False, None, False, ["rocrows"]),
    Case("rocrows-3d-N32-C2", 3, 32, 6, 2000, 1500, 2, 2, False, False, None, False, ["rocrows"]),
    Case("ownplanar-2d-N64-C1", 2, 64, 6, 3000, 2500, 2, 1, True, False, None, False, ["ownplanar"]),
    Case("ownplanar-2d-N64-C3", 2, 64, 6, 3000, 2500, 2, 3, False, False, None, False, ["ownplanar"]),
    Case("ownplanar-3d-N64-C1", 3, 64, 6, 3000, 2000, 2, 1, False, False, None, False, ["ownplanar"]),
    Case("ownplanar-3d-N64-C4", 3, 64, 6, 3000, 2000, 1, 4, True, False, None, False, ["ownplanar"]),
    Case("ownci-3d-N64-B2-C16-real", 3, 64, 6, 3000, 2000, 2, 16, False, False, None, False, ["ownci"]),
    Case("ownci-3d-N64-B2-C8-cplx", 3, 64, 6, 3000, 3000, 2, 8, True, True, None, False, ["ownci"]),
    # chunked plane loops (NFFT_HIP_CHUNK_BYTES): chunks that start inside a point set / a (re, im) pair
    Case("rocrows-chunked", 3, 16, 6, 1500, 1200, 2, 3, False, False, 4, False, ["rocrows", "rocrows"]),
    Case("ownplanar-chunked", 2, 64, 6, 3000, 2500, 2, 3, True, False, 4, False, ["ownplanar"] * 3),
    # a full chunk of 32 planes goes column-innermost, the remainder of 8 planar
    Case("ownci-chunked", 3, 64, 6, 3000, 2000, 2, 20, False, False, 32, False, ["ownci", "ownplanar"]),
]


def _pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def small_grid(d, N, m, n, B):
    """api.hip small_grid_route + smallgrid.hip small_grid_supported."""
    M = 2 * N
    if not _pow2(M) or M < 4 or M ** d > 4096 or 2 * m + 2 > M or B > 65535:
        return False
    return n * (2 * m + 2) ** d <= 80000 * min(max(B, 1), 8)


def colfft(d, N, no_colfft=False):
    """colfft.hip colfft_supported (and NFFT_HIP_NO_COLFFT)."""
    M = 2 * N
    if no_colfft or not _pow2(M):
        return False
    return (d == 2 and 128 <= M <= 1024) or (d == 3 and 16 <= M <= 1024)


def plane_bytes(d, N, no_colfft=False):
    """make_route's bytes per plane of a chunk: real grid + half spectrum (+ one plane of column-pass scratch)."""
    M = 2 * N
    b = M ** d * 4 + (M // 2 + 1) * M ** (d - 1) * 8
    if colfft(d, N, no_colfft):
        a = 8 if M >= 512 else 4
        ks = (N // 2 + 1 + a - 1) // a * a
        align = lambda v: (v + 255) // 256 * 256
        b += align(M * (1 if d == 2 else N + 1) * ks * 8) + align(M * 4)
    return b


def chunk_env(case):
    """NFFT_HIP_CHUNK_BYTES for `case.chunk` planes per chunk (as test_config_c4_shape_batched_columns_chunked)."""
    return str(case.chunk * plane_bytes(case.d, case.N, case.no_colfft) + 8)


def chunks_of(case):
    """[(first plane, planes)] of the plane loop (make_route's chunk size)."""
    ppc = 2 if case.cx else 1
    total = case.B * case.C * ppc
    chunk = total if case.chunk is None else case.chunk
    chunk -= chunk % ppc
    chunk = min(max(chunk, ppc), total)
    return [(p0, min(chunk, total - p0)) for p0 in range(0, total, chunk)]


def route_of(case):
    """The FFT route of every chunk: small_grid_route (both point sets), make_route, Route::chunk_fft."""
    if small_grid(case.d, case.N, case.m, case.ns, case.B) and small_grid(case.d, case.N, case.m, case.nt, case.B):
        return ["fused"]
    if not colfft(case.d, case.N, case.no_colfft):
        return ["full"] * len(chunks_of(case))
    M = 2 * case.N
    if M < 128:
        return ["rocrows"] * len(chunks_of(case))
    ci = case.C > 1 and case.d == 3
    return ["ownci" if ci and np_ >= 32 else "ownplanar" for _, np_ in chunks_of(case)]


def sample_columns(case):
    """(point set, column) pairs of the first and last column of every chunk."""
    ppc = 2 if case.cx else 1
    cols = set()
    for p0, np_ in chunks_of(case):
        for g in (p0 // ppc, (p0 + np_) // ppc - 1):
            cols.add((g // case.C, g % case.C))
    return sorted(cols)


def problem(d, n, C, B, N, m):
    from torch_nfft_amd import _lib
    return _lib.Problem(d, n, C, B, N, m, flags=_lib.POINTS_IN_QUARTER_BALL)


def plan_needed(d, n, C, B, N, m):
    from torch_nfft_amd import _lib
    return _lib.load().nfft_hip_plan_needed(ctypes.byref(problem(d, n, C, B, N, m)))


# ----------------------------------------------------------------------------- data and references

def batch_vector(rng, n, B):
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    b = np.sort(rng.integers(0, B, n)).astype(np.int64)
    b[0], b[-1] = 0, B - 1
    return b


def make_data(case, seed):
    assert not case.shared or case.nt == case.ns
    rng = np.random.default_rng(seed)
    src = (0.5 * (rng.random((case.ns, case.d)) - 0.5)).astype(np.float32)
    sb = batch_vector(rng, case.ns, case.B)
    if case.shared:
        tgt, tb = src, sb
    else:
        tgt = (0.5 * (rng.random((case.nt, case.d)) - 0.5)).astype(np.float32)
        tb = batch_vector(rng, case.nt, case.B)
    x = rng.standard_normal((case.ns, case.C)).astype(np.float32)
    if case.cx:
        x = (x + 1j * rng.standard_normal((case.ns, case.C))).astype(np.complex64)
    return rng, src, tgt, sb, tb, x


def dense_coeffs(rng, d, N):
    """A real array that is not even and a complex one, both spread over the whole band."""
    cr = rng.standard_normal((N,) * d).astype(np.float32)
    cc = (rng.standard_normal((N,) * d) + 1j * rng.standard_normal((N,) * d)).astype(np.complex64)
    return cr, cc


def sparse_freqs(rng, d, N):
    """(single frequency in the mirror half, handful): signed frequencies [q, d].  The handful holds the zero
    frequency, a point on the k = 0 plane and on the Nyquist plane k_a = -N/2 of every axis, the band corner and two
    points of the mirror half (last axis k < 0), whose partners -k carry no weight."""
    H = N // 2
    single = rng.integers(-H + 1, H, (1, d))
    single[0, -1] = -int(rng.integers(1, H))
    f = [np.full(d, -H), np.zeros(d, dtype=np.int64)]
    for a in range(d):
        for plane in (0, -H):
            k = rng.integers(-H, H, d)
            k[a] = plane
            f.append(k)
    for _ in range(2):
        k = rng.integers(-H, H, d)
        k[-1] = -int(rng.integers(1, H + 1))
        f.append(k)
    return single.astype(np.int64), np.unique(np.array(f, dtype=np.int64), axis=0)


def sparse_coeffs(rng, freqs, N, complex_coeffs):
    d = freqs.shape[1]
    vals = rng.standard_normal(len(freqs)) + 0.5 * np.sign(rng.standard_normal(len(freqs)))
    if complex_coeffs:
        vals = vals + 1j * rng.standard_normal(len(freqs))
    c = np.zeros((N,) * d, dtype=np.complex64 if complex_coeffs else np.float32)
    for k, v in zip(freqs, vals):
        c[tuple(k + N // 2)] = v
    return c, vals


def closed_form(x, freqs, vals, src, tgt, sb, tb, B):
    """y_i = sum_l c_l e^{-2 pi i l.t_i} sum_{j in set(i)} x_j e^{2 pi i l.s_j} in float64; real part for a real x."""
    x2 = np.asarray(x).reshape(x.shape[0], -1).astype(np.complex128)
    y = np.zeros((tgt.shape[0], x2.shape[1]), dtype=np.complex128)
    fr = freqs.astype(np.float64)
    for b in range(B):
        js, it = np.nonzero(sb == b)[0], np.nonzero(tb == b)[0]
        if len(it) == 0 or len(js) == 0:
            continue
        S = np.exp(2j * np.pi * (src[js].astype(np.float64) @ fr.T)).T @ x2[js]  # [q, C]
        y[it] = np.exp(-2j * np.pi * (tgt[it].astype(np.float64) @ fr.T)) @ (vals[:, None] * S)
    return y if np.iscomplexobj(x) else y.real


def oracle_sampled(case, x, coeffs, src, tgt, sb, tb):
    """nfft_ref.nfft_fastsum one (point set, column) at a time over sample_columns: (reference, row and column index)."""
    refs, rows, cols = [], [], []
    for b, c in sample_columns(case):
        js, it = np.nonzero(sb == b)[0], np.nonzero(tb == b)[0]
        refs.append(nfft_ref.nfft_fastsum(x[js, c:c + 1], coeffs, src[js], tgt[it], m=case.m)[:, 0])
        rows.append(it)
        cols.append(np.full(len(it), c))
    return np.concatenate(refs), np.concatenate(rows), np.concatenate(cols)


def heavy(case):
    return case.d == 3 and case.N >= 32


def fastsum(tn, case, x, coeffs, src, tgt, sb, tb):
    batched = case.B > 1
    if case.shared:
        return tn.nfft_fastsum(dev(x), dev(coeffs), dev(src), None, dev(sb) if batched else None, cutoff=case.m)
    return tn.nfft_fastsum(dev(x), dev(coeffs), dev(src), dev(tgt), dev(sb) if batched else None,
                           dev(tb) if batched else None, cutoff=case.m)


def rolloff_launches(fn):
    """fn() under the stage timers: (its result, launches of the roll-off stage -- one per chunk and direction)."""
    from torch_nfft_amd import _lib
    torch.cuda.synchronize()
    _lib.profile_collect()
    _lib.profile_enable(True, ["rolloff"])
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    return out, _lib.profile_collect()["rolloff"][1]


# ----------------------------------------------------------------------------- 1, 2: every route, three references

@pytest.mark.parametrize("case", ROUTES, ids=[c.name for c in ROUTES])
def test_fastsum_route(tn, monkeypatch, case):
    assert route_of(case) == case.route, "the case does not take the route it is named after"
    if case.chunk is not None:
        monkeypatch.setenv("NFFT_HIP_CHUNK_BYTES", chunk_env(case))
    if case.no_colfft:
        monkeypatch.setenv("NFFT_HIP_NO_COLFFT", "1")
    fused = case.route == ["fused"]
    assert (plan_needed(case.d, case.ns, case.C, case.B, case.N, case.m) == 0 and
            plan_needed(case.d, case.nt, case.C, case.B, case.N, case.m) == 0) == fused
    rng, src, tgt, sb, tb, x = make_data(case, 1000 + ROUTES.index(case))
    out_dtype = torch.complex64 if case.cx else torch.float32

    # (a) dense coefficients that are not even, against the float64 restatement
    for coeffs in dense_coeffs(rng, case.d, case.N):
        y, launches = rolloff_launches(lambda: fastsum(tn, case, x, coeffs, src, tgt, sb, tb))
        assert y.shape == (case.nt, case.C) and y.dtype == out_dtype
        assert launches == (0 if fused else 2 * len(case.route)), "roll-off launches: chunks x 2 directions"
        yh = host(y)
        if heavy(case):
            ref, rows, cols = oracle_sampled(case, x, coeffs, src, tgt, sb, tb)
            assert rel_l2(yh[rows, cols], ref) < T1
        else:
            assert rel_l2(yh, nfft_ref.nfft_fastsum(x, coeffs, src, tgt, sb, tb, m=case.m)) < T1
            # (c) the exact trigonometric sum, where it is cheap
            if case.N ** case.d * (case.ns + case.nt) <= 2e7:
                assert rel_l2(yh, ndft.ndft_fastsum(x, coeffs, src, tgt, sb, tb)) < T2[case.m]

    # (b) sparse coefficients against closed forms, every target and column
    single, handful = sparse_freqs(rng, case.d, case.N)
    for freqs in (single, handful):
        for complex_coeffs in (False, True):
            coeffs, vals = sparse_coeffs(rng, freqs, case.N, complex_coeffs)
            y = host(fastsum(tn, case, x, coeffs, src, tgt, sb, tb))
            exact = closed_form(x, freqs, vals, src, tgt, sb, tb, case.B)
            assert rel_l2(y, exact) < T2[case.m], (freqs.tolist(), complex_coeffs)
    tn.ops.check_status()


# ----------------------------------------------------------------------------- 3: edges

@pytest.mark.parametrize("d,N,m", [(2, 8, 4), (3, 16, 4)], ids=["fused", "planned"])
@pytest.mark.parametrize("complex_x", [False, True])
def test_fastsum_no_sources(tn, d, N, m, complex_x):
    """ns = 0 without batch vectors: the band is cleared (hipMemsetAsync), the result is zeros."""
    rng = np.random.default_rng(21)
    tgt = dev((0.5 * (rng.random((60, d)) - 0.5)).astype(np.float32))
    src = torch.zeros((0, d), device="cuda")
    x = torch.zeros((0, 3), dtype=torch.complex64 if complex_x else torch.float32, device="cuda")
    assert plan_needed(d, 60, 3, 1, N, m) == (0 if N == 8 else 1)
    coeffs = dev((rng.standard_normal((N,) * d) + 1j * rng.standard_normal((N,) * d)).astype(np.complex64))
    y = tn.nfft_fastsum(x, coeffs, src, tgt, cutoff=m)
    tn.ops.check_status()
    assert y.shape == (60, 3) and y.dtype == x.dtype
    assert torch.count_nonzero(y) == 0


@pytest.mark.parametrize("d,N,m,n", [(2, 8, 4, 40), (3, 16, 4, 400), (2, 64, 4, 1500)],
                         ids=["fused", "rocrows", "ownplanar"])
def test_fastsum_ragged_sets(tn, d, N, m, n):
    """Four point sets: set 1 has sources but no targets, set 2 (in the middle) targets but no sources -- its rows
    are zero -- sets 0 and 3 have both."""
    rng = np.random.default_rng(22 + d + N)
    src = (0.5 * (rng.random((n, d)) - 0.5)).astype(np.float32)
    tgt = (0.5 * (rng.random((n, d)) - 0.5)).astype(np.float32)
    sb = np.sort(rng.choice([0, 1, 3], n)).astype(np.int64)
    tb = np.sort(rng.choice([0, 2, 3], n)).astype(np.int64)
    sb[0], sb[-1], tb[0], tb[-1] = 0, 3, 0, 3
    for complex_x in (False, True):
        x = rng.standard_normal((n, 2)).astype(np.float32)
        if complex_x:
            x = (x + 1j * rng.standard_normal((n, 2))).astype(np.complex64)
        coeffs = (rng.standard_normal((N,) * d) + 1j * rng.standard_normal((N,) * d)).astype(np.complex64)
        y = host(tn.nfft_fastsum(dev(x), dev(coeffs), dev(src), dev(tgt), dev(sb), dev(tb), cutoff=m))
        tn.ops.check_status()
        assert np.count_nonzero(y[tb == 2]) == 0
        assert rel_l2(y, nfft_ref.nfft_fastsum(x, coeffs, src, tgt, sb, tb, m=m)) < T1


@pytest.mark.parametrize("d,N", [(2, 8), (3, 16)], ids=["fused", "planned"])
def test_fastsum_no_targets_and_no_columns(tn, d, N):
    from torch_nfft_amd import _lib
    rng = np.random.default_rng(23)
    src = dev((0.5 * (rng.random((50, d)) - 0.5)).astype(np.float32))
    coeffs = tn.gaussian_analytic_coeffs(0.2, dim=d, N=N)
    y = tn.nfft_fastsum(torch.randn((50, 2), device="cuda"), coeffs, src, torch.zeros((0, d), device="cuda"), cutoff=4)
    assert y.shape == (0, 2)
    y = tn.nfft_fastsum(torch.randn((50, 0), device="cuda"), coeffs, src, cutoff=4)
    assert y.shape == (50, 0) and y.dtype == torch.float32
    y = tn.nfft_fastsum(torch.randn((50, 0), dtype=torch.complex64, device="cuda"), coeffs, src, cutoff=4)
    assert y.shape == (50, 0) and y.dtype == torch.complex64
    # the C entry point with C = 0 returns without touching y
    lib = _lib.load()
    ps = problem(d, 50, 0, 1, N, 4)
    nbytes = lib.nfft_hip_fastsum_workspace_bytes(ctypes.byref(ps), ctypes.byref(ps), 0, 1, 0)
    assert nbytes > 0, _lib.last_error()
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.nfft_hip_fastsum(ctypes.byref(ps), _p(src), None, ctypes.byref(ps), _p(src), None, None, 0,
                                    _p(coeffs), 0, None, _p(ws), nbytes, _stream()))
    tn.ops.check_status()


def test_fastsum_one_side_fused_eligible(tn):
    """1-D N = 64, m = 4: 500 sources fit the fused path, 20 000 targets do not -- both go through the plans."""
    d, N, m, ns, nt = 1, 64, 4, 500, 20000
    assert plan_needed(d, ns, 2, 1, N, m) == 0 and plan_needed(d, nt, 2, 1, N, m) == 1
    rng = np.random.default_rng(24)
    src = (0.5 * (rng.random((ns, d)) - 0.5)).astype(np.float32)
    tgt = (0.5 * (rng.random((nt, d)) - 0.5)).astype(np.float32)
    for complex_x in (False, True):
        x = rng.standard_normal((ns, 2)).astype(np.float32)
        if complex_x:
            x = (x + 1j * rng.standard_normal((ns, 2))).astype(np.complex64)
        for coeffs in dense_coeffs(rng, d, N):
            y = host(tn.nfft_fastsum(dev(x), dev(coeffs), dev(src), dev(tgt), cutoff=m))
            assert rel_l2(y, nfft_ref.nfft_fastsum(x, coeffs, src, tgt, m=m)) < T1
            assert rel_l2(y, ndft.ndft_fastsum(x, coeffs, src, tgt)) < T2[m]
            # and the reverse: 20 000 sources, 500 targets
            xt = rng.standard_normal((nt, 2)).astype(np.float32)
            y = host(tn.nfft_fastsum(dev(xt), dev(coeffs), dev(tgt), dev(src), cutoff=m))
            assert rel_l2(y, nfft_ref.nfft_fastsum(xt, coeffs, tgt, src, m=m)) < T1
    tn.ops.check_status()


def test_fastsum_batch_size_mismatch(tn):
    src = dev(np.zeros((10, 3), dtype=np.float32))
    tgt = dev(np.zeros((12, 3), dtype=np.float32))
    sb = dev(np.repeat(np.arange(2), 5).astype(np.int64))
    tb = dev(np.repeat(np.arange(3), 4).astype(np.int64))
    coeffs = tn.gaussian_analytic_coeffs(0.2, dim=3, N=16)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.nfft_fastsum(torch.randn(10, device="cuda"), coeffs, src, tgt, sb, tb)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.nfft_fastsum(torch.randn(10, device="cuda"), coeffs, src, tgt, sb, None)
    tn.ops.check_status()


@pytest.mark.parametrize("complex_x", [False, True])
def test_fastsum_points_on_whole_torus(tn, complex_x):
    """fastsum always treats its points as lying in radius 1/4 (NFFT_HIP_POINTS_IN_QUARTER_BALL); the hint may change
    which kernels run, never the result.  10 000 points, 3-D N = 64, two columns: with the hint the plain plan spreads,
    without it (the public transforms) the owner-computes plan."""
    d, N, m, n = 3, 64, 4, 10000
    rng = np.random.default_rng(25)
    pos = (rng.random((n, d)) - 0.5).astype(np.float32)
    x = rng.standard_normal((n, 2)).astype(np.float32)
    if complex_x:
        x = (x + 1j * rng.standard_normal((n, 2))).astype(np.complex64)
    _, cc = dense_coeffs(rng, d, N)
    post, xt, ct = dev(pos), dev(x), dev(cc)
    y = tn.nfft_fastsum(xt, ct, post, cutoff=m)
    tn.ops.check_status()
    ref = nfft_ref.nfft_fastsum(x, cc, pos, m=m)
    assert rel_l2(host(y), ref) < T1
    band = tn.nfft_adjoint(xt, post, bandwidth=N, cutoff=m)
    composed = tn.nfft_forward(band * ct[None, ..., None], post, cutoff=m, real_output=not complex_x)
    assert rel_l2(host(y), host(composed)) < T1


# ----------------------------------------------------------------------------- 4: entry points agree

ENTRY = ["fused-2d", "full-3d-N12", "rocrows-3d-N16-C3", "ownplanar-2d-N64-C3", "ownci-3d-N64-B2-C8-cplx"]


@pytest.mark.parametrize("name", ENTRY)
def test_fastsum_entry_points_agree(tn, name):
    """nfft_hip_fastsum (plans in its workspace) = nfft_hip_fastsum_planned = the operator on a plan-cache miss and
    on a hit.  On the fused route the planned C call runs the planned kernels instead of the fused ones, a different
    summation order in different precision: there it is held to T1."""
    from torch_nfft_amd import _lib
    lib = _lib.load()
    case = next(c for c in ROUTES if c.name == name)
    rng, src, tgt, sb, tb, x = make_data(case, 31)
    _, coeffs = dense_coeffs(rng, case.d, case.N)
    srct, sbt, xt, ct = dev(src), dev(sb), dev(x), dev(coeffs)
    tgtt, tbt = (srct, sbt) if case.shared else (dev(tgt), dev(tb))
    ps = problem(case.d, case.ns, case.C, case.B, case.N, case.m)
    pt = problem(case.d, case.nt, case.C, case.B, case.N, case.m)
    cx = 1 if case.cx else 0
    out_dtype = torch.complex64 if case.cx else torch.float32

    def c_call(planned):
        nbytes = lib.nfft_hip_fastsum_workspace_bytes(ctypes.byref(ps), ctypes.byref(pt), cx, 1 if case.shared else 0,
                                                      1 if planned else 0)
        assert nbytes > 0, _lib.last_error()
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        y = torch.full((case.nt, case.C), float("nan"), dtype=out_dtype, device="cuda")
        if not planned:
            _lib.check(lib.nfft_hip_fastsum(ctypes.byref(ps), _p(srct), _p(sbt), ctypes.byref(pt), _p(tgtt), _p(tbt),
                                            _p(xt), cx, _p(ct), 1, _p(y), _p(ws), nbytes, _stream()))
            return host(y)
        plans = []
        for prob, pos, bt in ((ps, srct, sbt), (pt, tgtt, tbt)):
            pb = lib.nfft_hip_plan_bytes(ctypes.byref(prob))
            assert pb > 0, _lib.last_error()
            plan = torch.empty(pb, dtype=torch.uint8, device="cuda")
            _lib.check(lib.nfft_hip_plan_points(ctypes.byref(prob), _p(pos), _p(bt), _p(plan), pb, _stream()))
            plans.append(plan)
        if case.shared:
            plans[1] = plans[0]
        _lib.check(lib.nfft_hip_fastsum_planned(ctypes.byref(ps), _p(plans[0]), ctypes.byref(pt), _p(plans[1]), _p(xt),
                                                cx, _p(ct), 1, _p(y), _p(ws), nbytes, _stream()))
        return host(y)

    y_c = c_call(False)
    y_p = c_call(True)
    tn.ops.plan_cache_clear()
    s0 = tn.ops.plan_cache_stats()

    def op():
        if case.shared:
            return host(tn.nfft_fastsum(xt, ct, srct, None, sbt, None, cutoff=case.m))
        return host(tn.nfft_fastsum(xt, ct, srct, tgtt, sbt, tbt, cutoff=case.m))

    y_miss = op()
    s1 = tn.ops.plan_cache_stats()
    y_hit = op()
    s2 = tn.ops.plan_cache_stats()
    tn.ops.check_status()
    fused = case.route == ["fused"]
    sides = 1 if case.shared else 2
    assert s1["misses"] - s0["misses"] == (0 if fused else sides) and s1["hits"] == s0["hits"]
    assert s2["hits"] - s1["hits"] == (0 if fused else sides) and s2["misses"] == s1["misses"]
    assert np.isfinite(y_c).all() and np.isfinite(y_p).all()
    assert rel_l2(y_miss, y_c) < T_ENTRY
    assert rel_l2(y_hit, y_miss) < T_ENTRY
    assert rel_l2(y_p, y_c) < (T1 if fused else T_ENTRY)


# ----------------------------------------------------------------------------- 5: autograd against a dense matrix

def dense_kernel_matrix(coeffs, src, tgt):
    """K_ij = sum_l c_l e^{2 pi i l.(s_j - t_i)} in float64."""
    N, d = coeffs.shape[0], coeffs.ndim
    k = np.stack(np.meshgrid(*([np.arange(-N // 2, N // 2)] * d), indexing="ij"), -1).reshape(-1, d).astype(np.float64)
    Es = np.exp(2j * np.pi * (src.astype(np.float64) @ k.T))
    Et = np.exp(-2j * np.pi * (tgt.astype(np.float64) @ k.T))
    return (Et * coeffs.reshape(-1).astype(np.complex128)[None, :]) @ Es.T


@pytest.mark.parametrize("d,N,ns,nt", [(2, 16, 300, 250), (3, 16, 400, 300), (2, 64, 400, 300)],
                         ids=["fused", "rocrows", "ownplanar"])
def test_fastsum_autograd_dense(tn, d, N, ns, nt):
    """x.grad against K^T dy with a dense float64 K.  backward is defined as fastsum with sources and targets swapped
    (the reference's nfft.py:62-88): that is the transpose only for even coefficients, so the dense check uses a
    real, even array (analytic Gaussian coefficients with the unpartnered k_a = -N/2 entries set to zero).  For a
    complex array that is not even only the definition is pinned: backward = the swapped fastsum."""
    m = 6
    fused = small_grid(d, N, m, ns, 1) and small_grid(d, N, m, nt, 1)
    assert fused == (N == 16 and d == 2)
    rng = np.random.default_rng(26 + d + N)
    src = (0.5 * (rng.random((ns, d)) - 0.5)).astype(np.float32)
    tgt = (0.5 * (rng.random((nt, d)) - 0.5)).astype(np.float32)
    ce = coeffs_ref.gaussian_analytic_coeffs(0.15, d, N).astype(np.float32)
    for a in range(d):
        idx = [slice(None)] * d
        idx[a] = 0
        ce[tuple(idx)] = 0.0
    K = dense_kernel_matrix(ce, src, tgt)
    assert np.abs(K.imag).max() < 1e-9 * np.abs(K.real).max()
    K = K.real
    x = torch.randn((ns, 2), device="cuda", requires_grad=True)
    y = tn.nfft_fastsum(x, dev(ce), dev(src), dev(tgt), cutoff=m)
    assert rel_l2(host(y), K @ host(x).astype(np.float64)) < T2[m]
    dy = rng.standard_normal((nt, 2)).astype(np.float32)
    y.backward(dev(dy))
    assert rel_l2(host(x.grad), K.T @ dy.astype(np.float64)) < T2[m]
    # coefficients that are not even: backward is the swapped fastsum, not K^T
    _, cc = dense_coeffs(rng, d, N)
    xc = torch.randn((ns, 2), dtype=torch.complex64, device="cuda", requires_grad=True)
    yc = tn.nfft_fastsum(xc, dev(cc), dev(src), dev(tgt), cutoff=m)
    dyc = (rng.standard_normal((nt, 2)) + 1j * rng.standard_normal((nt, 2))).astype(np.complex64)
    yc.backward(dev(dyc))
    swapped = tn.nfft_fastsum(dev(dyc), dev(cc), dev(tgt), dev(src), cutoff=m)
    assert rel_l2(host(xc.grad), host(swapped)) < 1e-5
    tn.ops.check_status()


# ----------------------------------------------------------------------------- 6: GramMatrix on a planned 3-D route

def test_gram_matrix_3d_planned(tn):
    """GramMatrix @ X from GaussianKernel, 3-D N = 32 (the 64^3 grid, rocFFT rows + pruned column passes), two point
    sets and three columns, against the dense float64 Gaussian matrix: |(K - G) X| <= eps * sum_j |X_j| per point set,
    with eps = T2[m] = 5e-4, a tenth of test_gaussian_kernel_matrices' 5e-3 at the same N and m (the truncated
    Fourier series itself is off by 3e-5 here, the window by T2[m])."""
    n, b, dim, diameter, N, m = 150, 2, 3, 10.0, 32, 4
    assert not small_grid(dim, N, m, n * b, b)
    rng = np.random.default_rng(27)
    pos = (diameter * (rng.random((n * b, dim)) - 0.5)).astype(np.float32)
    batch = np.repeat(np.arange(b), n).astype(np.int64)
    X = rng.standard_normal((n * b, 3)).astype(np.float32)
    kern = tn.GaussianKernel(diameter, dim, N, m, shift_by_center=True, max_infinity_norm=diameter / 2, reg_degree=0)
    Y = host(kern(dev(pos), batch=dev(batch)) @ dev(X))
    tn.ops.check_status()
    assert Y.shape == (n * b, 3)
    exact = np.zeros_like(Y, dtype=np.float64)
    for k in range(b):
        sel = batch == k
        q = pos[sel].astype(np.float64)
        d2 = ((q[:, None, :] - q[None, :, :]) ** 2).sum(-1)
        exact[sel] = np.exp(-d2 / diameter ** 2) @ X[sel].astype(np.float64)
    rowsum = np.zeros_like(exact)
    for k in range(b):
        sel = batch == k
        rowsum[sel] = np.abs(X[sel]).sum(0, keepdims=True)
    assert (np.abs(Y - exact) <= T2[m] * rowsum).all()
