"""Full-size transforms against the dense float64 restatement (oracle/nfft_ref_torch.py) evaluated on the GPU.

tests/test_gpu_large.py checks the full sizes on a few dozen random frequencies and a few thousand sampled points at the
approximation tolerance (5e-4).  Here EVERY output element of the public operators -- all B N^d C spectrum entries of
the adjoint, all n C values of the forward, fastsum and point-gradient results -- is compared with the float64
restatement of the same algorithm, which on the device takes seconds per configuration.

Metrics (float64 on the device; `metrics_adjoint`, `metrics_points`):
  1  rel-L2 per (point set, column); the maximum is reported.
  2  adjoint, d >= 2: for every axis and every index along it, the rel-L2 of that (d-1)-dimensional slice of the band
     relative to the slice's own norm; the maximum over all d N slices.  The faces k = -N/2, k = N/2 - 1 and the slice
     k = 0 are printed separately -- this is where a pruned FFT pass, the Hermitian mirror row and a fused roll-off go wrong.
  3  worst element: max |got - ref| / rms(ref), per (point set, column); the maximum is reported.

Bounds:
  metric 1   the project's contract for the float64 restatement on the route in question, unchanged: 2e-6 for the 2-D
             and 3-D transforms (T1W / T1N of test_gpu_parity.py, T_STAGE of test_gpu_large.py), 2e-5 for the 1-D case
             (T1, test_large_1d_grid), 4e-6 for the point gradient (TR, test_gpu_pos_grad.py), 2e-5 for fastsum (T1,
             test_gpu_fastsum_routes.py).
  metrics 2, 3   no contract exists, so they are measured against the REFERENCE'S arithmetic, not against the library:
             the same restatement in its float32 mode (fp32 atomics, single-precision FFT, fp32 roll-off) on the same
             inputs gives the yardstick -- its own metric 2 and 3 against the float64 run, computed in the same test --
             and the library must stay within YARD = 4 times that.  The factor covers a different summation order
             (radix-8/4 passes against rocFFT's, tiles against atomics) and the ~22-bit matrix-core operands T1W already
             allows for; a lost term, a neighbouring roll-off index or one wrong twiddle is orders of magnitude above.

Every test prints one line per comparison with the library's and the yardstick's figures before it asserts.

Measured on one MI355X (library / float32 yardstick):
  configuration, output               rel-L2             worst slice        worst element
  C3     adjoint                      2.61e-7 / 2.62e-7  9.2e-7  / 9.1e-7   2.92e-4 / 2.92e-4  (x >= 0: the k = 0 entry; it moves with
  C3     forward                      2.64e-7 / 2.67e-7                     1.66e-6 / 2.27e-6   the atomics' order, 1.3e-4 in another run)
  C3     forward real_output          2.64e-7 / 2.67e-7                     2.33e-6 / 3.21e-6
  C3-cl  adjoint                      6.86e-7 / 2.31e-6  3.70e-6 / 6.03e-6  2.00e-4 / 1.02e-3
  C3-cl  forward                      2.70e-7 / 2.66e-7                     2.69e-6 / 2.03e-6
  C3-cl  forward real_output          2.70e-7 / 2.66e-7                     3.63e-6 / 2.79e-6
  N512   adjoint, real x, n = 2e5     2.17e-7 / 2.07e-7  3.26e-7 / 3.12e-7  3.32e-5 / 1.54e-5
  N512   forward, n = 2e5             2.15e-7 / 2.69e-7                     1.06e-6 / 1.80e-6
  N512   adjoint, complex x, n = 1e6  2.22e-7 / 2.10e-7  3.33e-7 / 3.18e-7  1.87e-6 / 1.69e-6
  N512   forward, n = 1e6             2.15e-7 / 2.69e-7                     1.30e-6 / 2.09e-6
  C4     adjoint (both budgets)       2.09e-7 / 1.98e-7  3.13e-7 / 2.90e-7  2.05e-6 / 1.53e-6
  C4     forward real_output (both)   2.02e-7 / 2.61e-7                     1.79e-6 / 3.07e-6
  grad   pos.grad                     7.46e-7 / 2.64e-7                     1.51e-5 / 4.84e-6
The fp32 atomics of the yardstick's spreading lose to the library's tile sums on the clustered input (C3-cl: the yardstick
itself is at 2.3e-6, above the 2e-6 the library is held to).  The whole file takes 44 s on one MI355X (tests/test_gpu_large.py in the
same session: 49 s); the other configurations' figures, and which of these tests fail on three deliberately wrong builds
that test_gpu_large.py passes or nearly passes, are in profiles/r06_dense_oracle.txt.
"""
import ctypes
import time

import pytest
import torch

from oracle import nfft_ref, nfft_ref_torch as rt

pytestmark = pytest.mark.gpu

T_XFORM = 2e-6    # T1W, T1N (tests/test_gpu_parity.py), T_STAGE (tests/test_gpu_large.py)
T_1D = 2e-5       # T1 (tests/test_gpu_parity.py: test_large_1d_grid)
T_GRAD = 4e-6     # TR (tests/test_gpu_pos_grad.py)
T_FASTSUM = 2e-5  # T1 (tests/test_gpu_fastsum_routes.py)
YARD = 4.0


@pytest.fixture(scope="module")
def tn():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import torch_nfft_amd
    return torch_nfft_amd


def free():
    torch.cuda.empty_cache()


def _sets(batch, B):
    return [None] if batch is None else [torch.nonzero(batch == b).squeeze(1) for b in range(B)]


def metrics_adjoint(got, ref, d):
    """got, ref [B, N^d, *cols]: metric 1, metric 2 (with the three named slices) and metric 3, each the maximum over
    point sets and columns."""
    B, N = ref.shape[0], ref.shape[1]
    ref = ref.reshape((B,) + (N,) * d + (-1,))
    got = got.reshape(ref.shape)
    out = {"l2": 0.0, "slice": 0.0, "lo": 0.0, "zero": 0.0, "hi": 0.0, "elem": 0.0}
    space = tuple(range(d))
    for b in range(B):
        r2 = ref[b].abs().square()
        if float(r2.sum()) == 0.0:  # an empty point set: the library must write zeros too
            assert float(got[b].abs().max()) == 0.0
            continue
        d2 = (got[b].to(ref.dtype) - ref[b]).abs().square()
        out["l2"] = max(out["l2"], float((d2.sum(dim=space) / r2.sum(dim=space)).sqrt().max()))
        out["elem"] = max(out["elem"], float((d2.amax(dim=space) / r2.mean(dim=space)).sqrt().max()))
        if d >= 2:
            for a in range(d):
                others = tuple(o for o in space if o != a)
                s = (d2.sum(dim=others) / r2.sum(dim=others)).sqrt()  # [N, C]
                out["slice"] = max(out["slice"], float(s.max()))
                for key, i in (("lo", 0), ("zero", N // 2), ("hi", N - 1)):
                    out[key] = max(out[key], float(s[i].max()))
        del d2, r2
    return out


def metrics_points(got, ref, batch=None, B=1):
    """got, ref [n, *cols] (forward, fastsum) or [n, d] (gradient): metrics 1 and 3, maxima over sets and columns."""
    n = ref.shape[0]
    ref = ref.reshape(n, -1)
    got = got.reshape(n, -1)
    out = {"l2": 0.0, "elem": 0.0}
    for sel in _sets(batch, B):
        r = ref if sel is None else ref[sel]
        g = got if sel is None else got[sel]
        if r.shape[0] == 0:
            continue
        r2 = r.abs().square()
        d2 = (g.to(r.dtype) - r).abs().square()
        out["l2"] = max(out["l2"], float((d2.sum(dim=0) / r2.sum(dim=0)).sqrt().max()))
        out["elem"] = max(out["elem"], float((d2.amax(dim=0) / r2.mean(dim=0)).sqrt().max()))
    return out


class Report:
    """Prints every comparison, collects the violated bounds, asserts at the end of the test."""

    def __init__(self, name):
        self.name, self.bad, self.t0 = name, [], time.time()

    def compare(self, what, lib, yard, l2_bound):
        line = "DENSE %s %s: rel_l2 %.3g (yardstick %.3g, bound %.1g)" % (self.name, what, lib["l2"], yard["l2"], l2_bound)
        keys = ["elem"] + (["slice"] if lib.get("slice") else [])
        for k in keys:
            line += "; %s %.3g (yardstick %.3g)" % ({"elem": "worst element", "slice": "worst slice"}[k], lib[k], yard[k])
        if lib.get("slice"):
            line += "; faces -N/2, 0, N/2-1: %.3g %.3g %.3g (yardstick %.3g %.3g %.3g)" % (
                lib["lo"], lib["zero"], lib["hi"], yard["lo"], yard["zero"], yard["hi"])
        print(line, flush=True)
        if not lib["l2"] <= l2_bound:
            self.bad.append("%s rel_l2 %.3g > %.1g" % (what, lib["l2"], l2_bound))
        for k in keys:
            if not lib[k] <= YARD * yard[k]:
                self.bad.append("%s %s %.3g > %g x %.3g" % (what, k, lib[k], YARD, yard[k]))

    def done(self):
        from torch_nfft_amd import ops
        ops.check_status()
        print("DENSE %s: %.1f s" % (self.name, time.time() - self.t0), flush=True)
        assert not self.bad, (self.name, self.bad)


def check_adjoint(rep, tn, x, pos, batch, N, m, l2_bound=T_XFORM, what="adjoint"):
    d = pos.shape[1]
    got = tn.nfft_adjoint(x, pos, batch, bandwidth=N, cutoff=m)
    free()
    ref = rt.nfft_adjoint(x, pos, batch, N=N, m=m)
    assert got.shape == ref.shape and got.dtype == torch.complex64
    lib = metrics_adjoint(got, ref, d)
    del got
    y32 = rt.nfft_adjoint(x, pos, batch, N=N, m=m, dtype=torch.float32)
    yard = metrics_adjoint(y32, ref, d)
    del y32, ref
    free()
    rep.compare(what, lib, yard, l2_bound)


def check_forward(rep, tn, xh, pos, batch, m, real_outputs=(False, True), l2_bound=T_XFORM, what="forward", extra=None):
    """The restatement is evaluated once; ``extra`` lists callables that change a setting of the library and return a
    label (C4's chunk budgets): the library runs, and is compared, once after each."""
    B = xh.shape[0]
    ref = rt.nfft_forward(xh, pos, batch, m=m)
    y32 = rt.nfft_forward(xh, pos, batch, m=m, dtype=torch.float32)
    free()
    for ro in real_outputs:
        r = ref.real if ro else ref
        yard = metrics_points(y32.real if ro else y32, r, batch, B)
        for label in ([""] if extra is None else extra):
            if callable(label):
                label = label()
            got = tn.nfft_forward(xh, pos, batch, cutoff=m, real_output=ro)
            assert got.shape == r.shape and got.dtype == (torch.float32 if ro else torch.complex64)
            lib = metrics_points(got, r, batch, B)
            del got
            free()
            rep.compare("%s%s%s" % (what, " real_output" if ro else "", label), lib, yard, l2_bound)


def randn_c(shape, gen):
    return torch.complex(torch.randn(shape, generator=gen, device="cuda"), torch.randn(shape, generator=gen, device="cuda"))


def clusters(n, d, gen, sigma=0.05, k=8):
    centres = torch.rand((k, d), generator=gen, device="cuda") - 0.5
    which = torch.randint(0, k, (n,), generator=gen, device="cuda")
    pos = centres[which] + sigma * torch.randn((n, d), generator=gen, device="cuda")
    return pos - torch.floor(pos + 0.5)


# ----------------------------------------------------------------------------- the restatement itself, on this device

@pytest.mark.parametrize("d,N,m,n,B,cols", [(3, 16, 4, 1500, 2, (2,)), (2, 64, 4, 3000, 3, ())])
def test_restatement_on_the_device_matches_numpy_oracle(d, N, m, n, B, cols):
    """oracle/nfft_ref_torch.py on the GPU (float64 atomics, torch.fft in complex128 on this device, a small block so
    that the loops over blocks run) against oracle/nfft_ref.py on the host: <= 1e-12."""
    import numpy as np
    import test_pos_grad_ref as gref
    rng = np.random.default_rng(d)
    pos = (rng.random((n, d)) - 0.5).astype(np.float32)
    pos[0], pos[1], pos[2] = -0.5, np.nextafter(np.float32(0.5), np.float32(0)), 0.0
    batch = np.sort(rng.integers(0, B, n)).astype(np.int64)
    batch[0], batch[-1] = 0, B - 1
    x = (rng.standard_normal((n,) + cols) + 1j * rng.standard_normal((n,) + cols)).astype(np.complex64)
    xh = (rng.standard_normal((B,) + (N,) * d + cols) + 1j * rng.standard_normal((B,) + (N,) * d + cols)).astype(np.complex64)
    C = int(np.prod(cols)) if cols else 1
    w = rng.standard_normal((n, 2 * C))
    dev = lambda a: torch.from_numpy(a).cuda()

    def rel(a, b):
        return float(np.linalg.norm((a.cpu().numpy() - b).ravel()) / np.linalg.norm(b.ravel()))

    ea = rel(rt.nfft_adjoint(dev(x), dev(pos), dev(batch), N=N, m=m, block=700), nfft_ref.nfft_adjoint(x, pos, batch, N=N, m=m))
    ef = rel(rt.nfft_forward(dev(xh), dev(pos), dev(batch), m=m, block=700), nfft_ref.nfft_forward(xh, pos, batch, m=m))
    eg = rel(rt.forward_pos_grad(dev(xh), dev(pos), dev(batch), m, False, dev(w), block=700),
             gref.pos_grad(xh, pos, batch, m, False, w))
    print("DENSE restatement on the device, %d-D: adjoint %.2e forward %.2e gradient %.2e" % (d, ea, ef, eg))
    assert ea <= 1e-12 and ef <= 1e-12 and eg <= 1e-12


# ----------------------------------------------------------------------------- C3 and its relatives

def _c3_inputs(kind):
    n = 10_000_000
    if kind == "uniform":
        gen = torch.Generator(device="cuda").manual_seed(4)
        pos = torch.rand((n, 3), generator=gen, device="cuda") - 0.5
    else:  # the input of test_gpu_large.py: test_config_c3_clustered_10m
        gen = torch.Generator(device="cuda").manual_seed(777)
        pos = clusters(n, 3, gen)
    x = torch.rand((n,), generator=gen, device="cuda")
    return gen, pos, x


@pytest.mark.parametrize("kind", ["uniform", "clustered"], ids=["C3", "C3-cl"])
def test_c3_dense(tn, kind):
    """3-D N=256 m=4, n=10^7, one real column: scatter spreading on the matrix cores, own rows + planar column passes
    at M=512, the streamed gather with column groups; with the clustered input the work list, cut slab ranges and
    ragged streamed items.  Adjoint; forward of a dense complex randn spectrum with both real_outputs."""
    N, m = 256, 4
    gen, pos, x = _c3_inputs(kind)
    rep = Report("C3" if kind == "uniform" else "C3-cl")
    check_adjoint(rep, tn, x, pos, None, N, m)
    del x
    xh = randn_c((1, N, N, N), gen)
    check_forward(rep, tn, xh, pos, None, m)
    rep.done()


def test_c3_complex_columns_two_sets(tn):
    """C3-cx: N=256, n=2*10^6, complex x in 3 columns, two point sets of unequal size: (re, im) plane pairs, 12 real
    planes -- not a multiple of the tile-id permutation's span in column_tile_of_block."""
    N, m, n = 256, 4, 2_000_000
    gen = torch.Generator(device="cuda").manual_seed(41)
    pos = torch.rand((n, 3), generator=gen, device="cuda") - 0.5
    batch = (torch.arange(n, device="cuda") >= n // 3).to(torch.int64)
    x = randn_c((n, 3), gen)
    rep = Report("C3-cx")
    check_adjoint(rep, tn, x, pos, batch, N, m)
    del x
    xh = randn_c((2, N, N, N, 3), gen)
    check_forward(rep, tn, xh, pos, batch, m)
    rep.done()


@pytest.mark.parametrize("m", [2, 5, 7])
def test_c3_other_cutoffs(tn, m):
    """m-var: 3-D N=256, n=6*10^6, m = 2, 5 and 7: the streamed gather's other chunk depths and the widest window of
    the matrix-core path."""
    N, n = 256, 6_000_000
    gen = torch.Generator(device="cuda").manual_seed(90 + m)
    pos = torch.rand((n, 3), generator=gen, device="cuda") - 0.5
    x = torch.randn((n,), generator=gen, device="cuda")
    rep = Report("m-var m=%d" % m)
    check_adjoint(rep, tn, x, pos, None, N, m)
    del x
    xh = randn_c((1, N, N, N), gen)
    check_forward(rep, tn, xh, pos, None, m, real_outputs=(False,))
    rep.done()


# ----------------------------------------------------------------------------- N = 512

@pytest.mark.parametrize("n,complex_x", [(200_000, False), (1_000_000, True)], ids=["real-200k", "complex-1m"])
def test_grid_1024_cubed_dense(tn, n, complex_x):
    """N512: 3-D N=512 m=4 (oversampled grid 1024^3: radix sequence 8, 8, 4, 4, the M=1024 twiddle table, owner-computes
    spreading); n=2*10^5 real x (the input of test_grid_1024_cubed) and n=10^6 complex x; forward of a dense spectrum.
    May skip only when the device has less free memory than the restatement's stated peak plus the library's workspace."""
    from torch_nfft_amd import _lib
    N, m = 512, 4
    prob = _lib.Problem(3, n, 1, 1, N, m)
    lib = _lib.load()
    ws = max(lib.nfft_hip_adjoint_workspace_bytes(ctypes.byref(prob), int(complex_x), 0),
             lib.nfft_hip_forward_workspace_bytes(ctypes.byref(prob), 1, 0))
    peak = rt.peak_bytes(3, N, m, n)
    io = 2 * N ** 3 * 8 + n * 64  # the library's spectrum and the dense input spectrum, complex64, and the points
    free()
    avail = torch.cuda.mem_get_info()[0]
    if avail < peak + max(ws, 0) + io:
        pytest.skip("free device memory %d B < restatement's peak %d B + library workspace %d B + spectra %d B" % (avail, peak, ws, io))
    gen = torch.Generator(device="cuda").manual_seed(9)
    pos = torch.rand((n, 3), generator=gen, device="cuda") - 0.5
    x = randn_c((n,), gen) if complex_x else torch.rand((n,), generator=gen, device="cuda")
    rep = Report("N512 %s" % ("complex n=1e6" if complex_x else "real n=2e5"))
    check_adjoint(rep, tn, x, pos, None, N, m)
    del x
    xh = randn_c((1, N, N, N), gen)
    check_forward(rep, tn, xh, pos, None, m, real_outputs=(False,))
    rep.done()


# ----------------------------------------------------------------------------- C4

def test_c4_stated_shape_dense(tn, monkeypatch):
    """C4: N=128 m=4, B=4 point sets of 10^5 points, C=64 real columns (the input of
    test_config_c4_stated_shape_one_gpu_share): column-innermost passes at full size, chunks that start inside a point
    set, paired owner-computes spreading.  Adjoint and forward with real_output, each under the default chunk budget
    and under NFFT_HIP_CHUNK_BYTES = 3 GiB, against one evaluation of the restatement."""
    N, m, B, C, n_per = 128, 4, 4, 64, 100_000
    n = B * n_per
    gen = torch.Generator(device="cuda").manual_seed(64)
    pos = torch.rand((n, 3), generator=gen, device="cuda") - 0.5
    batch = torch.arange(n, device="cuda") // n_per
    x = torch.randn((n, C), generator=gen, device="cuda")
    rep = Report("C4")

    def budget(gib):
        def set_it():
            if gib is None:
                monkeypatch.delenv("NFFT_HIP_CHUNK_BYTES", raising=False)
                return ""
            monkeypatch.setenv("NFFT_HIP_CHUNK_BYTES", str(gib << 30))
            return " chunk budget %d GiB" % gib
        return set_it

    ref = rt.nfft_adjoint(x, pos, batch, N=N, m=m)
    y32 = rt.nfft_adjoint(x, pos, batch, N=N, m=m, dtype=torch.float32)
    yard = metrics_adjoint(y32, ref, 3)
    del y32
    free()
    for gib in (None, 3):
        label = budget(gib)()
        got = tn.nfft_adjoint(x, pos, batch, bandwidth=N, cutoff=m)
        assert got.shape == (B, N, N, N, C) and got.dtype == torch.complex64
        lib = metrics_adjoint(got, ref, 3)
        del got
        free()
        rep.compare("adjoint" + label, lib, yard, T_XFORM)
    del ref, x
    free()
    xh = randn_c((B, N, N, N, C), gen)
    check_forward(rep, tn, xh, pos, batch, m, real_outputs=(True,), extra=[budget(None), budget(3)])
    monkeypatch.delenv("NFFT_HIP_CHUNK_BYTES", raising=False)
    rep.done()


# ----------------------------------------------------------------------------- 2-D and 1-D

def test_2d_16384_squared_dense(tn):
    """2D: N=8192 m=4 n=2*10^5 (the input of test_grid_2d_16384_squared): index range beyond 2^27 on the narrow tiling."""
    N, m, n = 8192, 4, 200_000
    gen = torch.Generator(device="cuda").manual_seed(611)
    pos = torch.rand((n, 2), generator=gen, device="cuda") - 0.5
    x = torch.rand((n,), generator=gen, device="cuda")
    rep = Report("2D N=8192")
    check_adjoint(rep, tn, x, pos, None, N, m)
    del x
    xh = randn_c((1, N, N), gen)
    check_forward(rep, tn, xh, pos, None, m, real_outputs=(False,))
    rep.done()


def test_2d_n512_four_sets_two_columns_dense(tn):
    """2D: N=512 m=4 n=10^6 in 4 point sets of unequal size, 2 columns: the own 2-D row + column pass at M=1024."""
    N, m, n = 512, 4, 1_000_000
    gen = torch.Generator(device="cuda").manual_seed(612)
    pos = torch.rand((n, 2), generator=gen, device="cuda") - 0.5
    i = torch.arange(n, device="cuda")
    batch = (i >= n // 10).to(torch.int64) + (i >= n // 3).to(torch.int64) + (i >= 3 * n // 4).to(torch.int64)
    x = torch.randn((n, 2), generator=gen, device="cuda")
    rep = Report("2D N=512")
    check_adjoint(rep, tn, x, pos, batch, N, m)
    del x
    xh = randn_c((4, N, N, 2), gen)
    check_forward(rep, tn, xh, pos, batch, m)
    rep.done()


def test_1d_2_to_20_dense(tn):
    """1D: N=2^20 (the largest accepted bandwidth), m=4, n=10^6: the fallback plan and the 1-D kernels with many points
    per tile.  Bound T1 = 2e-5 as test_large_1d_grid."""
    N, m, n = 1 << 20, 4, 1_000_000
    gen = torch.Generator(device="cuda").manual_seed(613)
    pos = torch.rand((n, 1), generator=gen, device="cuda") - 0.5
    x = torch.randn((n,), generator=gen, device="cuda")
    rep = Report("1D N=2^20")
    check_adjoint(rep, tn, x, pos, None, N, m, l2_bound=T_1D)
    del x
    xh = randn_c((1, N), gen)
    check_forward(rep, tn, xh, pos, None, m, l2_bound=T_1D)
    rep.done()


# ----------------------------------------------------------------------------- C5: fastsum

@pytest.mark.parametrize("variant", ["analytic", "interpolated-complex"])
def test_c5_fastsum_dense(tn, variant):
    """C5: Gaussian kernel sums, 3-D N=256 m=4, points in the quarter ball (the input of
    test_config_c5_fastsum_1m_x_1m): all 10^6 targets with the analytic coefficients and a real x; once more with the
    complex interpolated coefficients, a complex x and n_s != n_t.  The coefficients are folded into the adjoint's last
    pass at M=512; shared-flag plans."""
    N, m, sigma = 256, 4, 0.1
    ns, nt = (1_000_000, 1_000_000) if variant == "analytic" else (700_000, 1_000_000)
    gen = torch.Generator(device="cuda").manual_seed(11)

    def ball(k):
        p = torch.rand((k, 3), generator=gen, device="cuda") - 0.5
        return p * (0.25 / torch.linalg.norm(p, dim=1).max())

    src, tgt = ball(ns), ball(nt)
    if variant == "analytic":
        x = torch.rand((ns,), generator=gen, device="cuda")
        coeffs = tn.gaussian_analytic_coeffs(sigma, dim=3, N=N)
    else:
        x = randn_c((ns,), gen)
        coeffs = tn.gaussian_interpolated_coeffs(sigma, dim=3, N=N)
        assert coeffs.is_complex()
    rep = Report("C5 " + variant)
    got = tn.nfft_fastsum(x, coeffs, src, tgt, cutoff=m)
    free()
    ref = rt.nfft_fastsum(x, coeffs, src, tgt, m=m)
    assert got.shape == ref.shape == (nt,) and got.is_complex() == ref.is_complex()
    lib = metrics_points(got, ref)
    yard = metrics_points(rt.nfft_fastsum(x, coeffs, src, tgt, m=m, dtype=torch.float32), ref)
    rep.compare("fastsum", lib, yard, T_FASTSUM)
    rep.done()


# ----------------------------------------------------------------------------- the gradient with respect to the points

def test_c3_pos_grad_dense(tn):
    """grad: pos.grad of nfft_forward at N=256 m=4, n=10^7, dense complex spectrum, random upstream gradient: all
    10^7 x 3 entries (interp_grad_kernel through lane_gather.h on a chunked full-size problem)."""
    N, m, n = 256, 4, 10_000_000
    gen = torch.Generator(device="cuda").manual_seed(5)
    pos = torch.rand((n, 3), generator=gen, device="cuda") - 0.5
    xh = randn_c((1, N, N, N), gen)
    w = torch.randn((n, 2), generator=gen, device="cuda")
    rep = Report("grad")
    p = pos.clone().requires_grad_(True)
    y = tn.nfft_forward(xh, p, None, cutoff=m)
    (torch.view_as_real(y) * w).sum().backward()
    got = p.grad
    del y, p
    free()
    assert got.shape == (n, 3) and got.dtype == torch.float32
    ref = rt.forward_pos_grad(xh, pos, None, m, False, w)
    lib = metrics_points(got, ref)
    del got
    yard = metrics_points(rt.forward_pos_grad(xh, pos, None, m, False, w, dtype=torch.float32), ref)
    rep.compare("pos.grad", lib, yard, T_GRAD)
    rep.done()
