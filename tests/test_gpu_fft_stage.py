"""The FFT stage alone (grids <-> band spectrum, roll-off included) on every route, size and plane layout: rocFFT + the
deconv kernels, rocFFT rows + column passes, own rows + planar column passes (3-D and 2-D), the column-innermost passes,
column_layout_kernel, the chunk loop and the fastsum's per-frequency factor.  No points: the test entry nfft_dbg_fft_stage
(csrc/api.hip; torch_nfft_amd._lib.fft_stage) builds the Route with make_route and walks the chunk loop of adjoint_impl /
forward_impl, calling fft_adjoint_chunk / fft_forward_chunk on the caller's planes.

Reference: oracle/nfft_ref_torch.py _grid_to_band / _band_to_grid in float64 on the device, one column (one plane or one
(re, im) pair) at a time.  Every case asserts its route, the route of each of its chunks and the column-pass tile widths
through nfft_dbg_fft_route, runs both directions, fills every output with NaN beforehand and wants it back finite.

Inputs.  Random planes whose magnitude changes a thousandfold from column to column (scales 1, 1e3, 1e-3, 1, ...), every
plane compared against ITS OWN norm, so a leak of 2e-6 of a loud neighbour into a quiet plane fails; zero columns inside
the layout (in the middle of the first group of 16 planes, the last column, the column after the loudest) whose outputs
must be exactly 0; unit impulses (adjoint: one grid cell; forward: one frequency) compared element by element.

Tolerances.  Rel-L2 per plane: T1N (2-D, 3-D) and T1 (1-D) of tests/test_gpu_parity.py -- the stage gets no more than the
whole transform.  The worst (d-1)-dimensional slice against its own norm, the worst element against the plane's rms and the
impulses' worst element against the amplitude have no contract: their yardstick is the SAME reference code run in float32 /
complex64 on the same input, compared with the float64 run in the same test, and the library must stay within YARD = 4
times that figure (case by case: the worst plane of the library against the worst plane of the yardstick).  Zero columns,
finiteness and chunk splits that keep every plane on its route are exact.

Cost on an MI355X: the small cases take well under a second each; the 3-D N = 256 cases (32 planes column-innermost: 16 GiB
of grids, 18 GB of spectra, 5 GB of scratch, the budget raised to 32 planes) and the 3-D N = 512 cases (4 GiB planes) take
seconds each and are skipped, with both numbers named, where the device lacks the memory.  In the large cases only six
columns carry data (the reference's cost); all others are zero columns, which must come back exactly 0.

Measured on an MI355X (library / float32 yardstick, worst plane of all cases of the route; per size in
profiles/r17_fft_stage.md): rel-L2 full 1.8e-7 / 1.8e-7, rocFFT rows 1.7e-7 / 1.7e-7, planar 3-D 2.0e-7 / 2.2e-7, planar 2-D
1.7e-7 / 1.8e-7, column-innermost 1.9e-7 / 2.1e-7; worst slice <= 3.4e-7 / 4.5e-7 on the 2-D grids N = 8 and 24, <= 2.8e-7 / 2.6e-7 from N = 32 up; worst
element <= 9.2e-6 / 6.3e-6 (3-D N = 64 with the factor); impulses <= 8.8e-6 / 8.1e-6 of the amplitude (3-D N = 128); the
largest library / yardstick ratio of any case is 1.74.  The whole file takes about 52 s.
"""
import collections
import math

import pytest
import torch

from oracle import nfft_ref_torch as rt
from test_gpu_fastsum_routes import plane_bytes
from test_gpu_parity import T1, T1N
from torch_nfft_amd import _lib

pytestmark = pytest.mark.gpu

M_CUT = 4       # window cut-off of every case: the roll-off exponent is pi m k^2 / (3 N^2)
YARD = 4.0      # library figure <= YARD * float32-reference figure (slices, elements, impulses)
SCALES = (1.0, 1e3, 1e-3, 1.0)

# d, N, B (point sets), C (columns), pairs: a column is a (re, im) pair of planes (adjoint: x complex; forward: y complex),
# other: the second flag (adjoint: real_output; forward: xhat complex), budget: NFFT_HIP_CHUNK_BYTES in planes,
# no_colfft: NFFT_HIP_NO_COLFFT=1, fft: Route::fft, chunks: chunk_fft of every chunk in order, nc: (axis-1, axis-0, forward)
# tile widths of the FIRST chunk, sparse: only six columns carry data, dirs: directions run
Case = collections.namedtuple("Case", "d N B C pairs other budget no_colfft fft chunks nc sparse dirs")


def case(d, N, B, C, pairs, other, fft, chunks, nc, budget=None, no_colfft=False, sparse=False, dirs=("adjoint", "forward")):
    return Case(d, N, B, C, pairs, other, budget, no_colfft, fft, tuple(chunks), nc, sparse, dirs)


def case_id(c):
    return "%dd-N%d-B%d-C%d-%s-%s%s%s" % (c.d, c.N, c.B, c.C, "pairs" if c.pairs else "single", "other" if c.other else "plain",
                                          "-chunk%d" % c.budget if c.budget else "", "-nocolfft" if c.no_colfft else "")


COMBOS = [(False, False), (False, True), (True, False), (True, True)]
NONE = (0, 0, 0)


def full_cases():
    out = []
    shapes = [(1, 8, False), (1, 48, False), (1, 4096, False), (2, 8, False), (2, 24, False), (2, 32, False), (3, 12, False),
              (2, 64, True), (3, 32, True)]
    for d, N, nocol in shapes:
        for pairs, other in COMBOS:
            out.append(case(d, N, 2, 3, pairs, other, "full", ["full"], NONE, no_colfft=nocol))
    # one chunk split per dimension (and under the switch): 12 planes in chunks of 4 -- the second starts inside a column set
    for d, N, nocol in [(1, 48, False), (2, 24, False), (3, 12, False), (3, 32, True)]:
        out.append(case(d, N, 2, 3, True, False, "full", ["full"] * 3, NONE, budget=4, no_colfft=nocol))
    return out


def roc_rows_cases():
    out = []
    for N in (8, 16, 32):
        for pairs, other in COMBOS:
            out.append(case(3, N, 1, 1, pairs, other, "roc_rows", ["roc_rows"], (16, 16, 16)))
        out.append(case(3, N, 2, 3, True, False, "roc_rows", ["roc_rows"], (16, 16, 16)))
        out.append(case(3, N, 2, 3, False, True, "roc_rows", ["roc_rows"], (16, 16, 16)))
    # a chunk that starts inside a point set: 2 sets x 3 columns x 2 planes in chunks of 4 and of 8 planes
    out.append(case(3, 16, 2, 3, True, False, "roc_rows", ["roc_rows"] * 3, (16, 16, 16), budget=4))
    out.append(case(3, 32, 2, 3, True, True, "roc_rows", ["roc_rows"] * 2, (16, 16, 16), budget=8))
    out.append(case(3, 8, 2, 3, False, False, "roc_rows", ["roc_rows"] * 3, (16, 16, 16), budget=2))
    return out


def planar_3d_cases():
    # tile widths: 16 columns while M * NC * 8 bytes (* 2 tile buffers for complex x) fit 32 KB (64 KB at M = 1024)
    nc = {64: {False: (16, 16, 16), True: (16, 16, 16)}, 128: {False: (16, 16, 16), True: (16, 8, 16)},
          256: {False: (8, 8, 8), True: (8, 4, 8)}, 512: {False: (8, 8, 8), True: (8, 4, 8)}}
    out = []
    for N in (64, 128, 256, 512):
        for pairs, other in COMBOS:
            out.append(case(3, N, 1, 1, pairs, other, "own_planar", ["own_planar"], nc[N][pairs]))
    for N in (64, 128):
        # C = 3: column_layout_kernel; 12 planes stay below the 32 of the column-innermost passes
        out.append(case(3, N, 2, 3, True, False, "own_planar", ["own_planar"], nc[N][True]))
        out.append(case(3, N, 2, 3, False, True, "own_planar", ["own_planar"], nc[N][False]))
        # a chunk boundary inside a set
        out.append(case(3, N, 2, 3, True, False, "own_planar", ["own_planar"] * 3, nc[N][True], budget=4))
        out.append(case(3, N, 1, 5, False, False, "own_planar", ["own_planar"] * 3, nc[N][False], budget=2))
    return out


def ci_cases():
    ci, pl = "own_ci", "own_planar"
    w = (16, 16, 16)
    out = [
        case(3, 64, 1, 32, False, False, pl, [ci], w),                 # 32 planes
        case(3, 64, 1, 16, True, False, pl, [ci], w),                  # 32
        case(3, 64, 1, 16, True, True, pl, [ci], w),
        case(3, 64, 3, 11, False, True, pl, [ci], w),                  # 33: a group of 1 plane; groups straddle the sets
        case(3, 64, 1, 20, True, True, pl, [ci], w),                   # 40
        case(3, 64, 1, 47, False, False, pl, [ci], w),                 # 47: the last group lacks one plane
        case(3, 64, 3, 8, True, False, pl, [ci], w),                   # 48
        case(3, 64, 3, 16, False, True, pl, [ci], w),                  # 48
        case(3, 64, 3, 8, True, False, pl, [ci, pl], w, budget=32),    # ci chunk + planar remainder of 16 planes
        case(3, 64, 3, 16, False, True, pl, [ci, pl], w, budget=32),
        case(3, 64, 3, 8, True, True, pl, [ci], w, budget=48),         # three groups in one chunk
        case(3, 64, 3, 32, False, False, pl, [ci, ci], w, budget=48),  # 96 planes: two column-innermost chunks
        case(3, 128, 1, 16, True, False, pl, [ci], w),                 # 32
        case(3, 128, 5, 7, False, True, pl, [ci], w),                  # 35
        # N = 256: the default budget of 16 GiB holds 14 planes, so these chunks exist only under a raised budget
        case(3, 256, 1, 16, True, False, pl, [ci], w, budget=32, sparse=True),
        case(3, 256, 1, 32, False, True, pl, [ci], w, budget=32, sparse=True),
    ]
    return out


CASES = full_cases() + roc_rows_cases() + planar_3d_cases() + ci_cases()


def problem(d, N, B, C):
    return _lib.Problem(d, 0, C, B, N, M_CUT)


def set_env(monkeypatch, c, budget):
    if budget:
        monkeypatch.setenv("NFFT_HIP_CHUNK_BYTES", str(budget * plane_bytes(c.d, c.N, c.no_colfft) + 8))
    else:
        monkeypatch.delenv("NFFT_HIP_CHUNK_BYTES", raising=False)
    if c.no_colfft:
        monkeypatch.setenv("NFFT_HIP_NO_COLFFT", "1")
    else:
        monkeypatch.delenv("NFFT_HIP_NO_COLFFT", raising=False)


def flags(c, direction):
    """(x_is_complex, real_output) of the call."""
    return (c.pairs, c.other) if direction == "adjoint" else (c.other, not c.pairs)


def chunk_routes(c, direction):
    """The route record of the call and [(planes, chunk_fft, tile widths)] of its chunks."""
    xc, ro = flags(c, direction)
    p = problem(c.d, c.N, c.B, c.C)
    r = _lib.fft_route(p, direction == "adjoint", xc, ro)
    rows = []
    for p0 in range(0, r.total_planes, r.chunk_planes):
        n = min(r.chunk_planes, r.total_planes - p0)
        q = _lib.fft_route(p, direction == "adjoint", xc, ro, n)
        rows.append((n, q.chunk_fft, (q.nc_axis1, q.nc_axis0, q.nc_forward)))
    return r, rows


def assert_route(c, direction):
    r, rows = chunk_routes(c, direction)
    ppc = 2 if c.pairs else 1
    assert r.total_planes == c.B * c.C * ppc and r.fft == c.fft, (r, c)
    assert [q[1] for q in rows] == list(c.chunks), (rows, c)
    if c.budget:
        assert r.chunk_planes == c.budget - c.budget % ppc, (r, c)
    a1, a0, fw = c.nc
    assert rows[0][2] == ((a1, a0, 0) if direction == "adjoint" else (0, 0, fw)), (rows, c)
    return rows


def need_bytes(c):
    """Device memory of a case: the caller's planes and band, the workspace, and the float64 reference of one column."""
    M = 2 * c.N
    planes = c.B * c.C * (2 if c.pairs else 1)
    chunk = min(planes, c.budget or planes)
    ws = chunk * plane_bytes(c.d, c.N, c.no_colfft) + (1 << 28)
    return planes * M ** c.d * 4 * 2 + c.B * c.C * c.N ** c.d * 8 * 4 + ws + 5 * 16 * M ** c.d


def guard_memory(c):
    need = need_bytes(c)
    if need < (2 << 30):
        return
    avail = torch.cuda.mem_get_info()[0]
    if avail < need:
        pytest.skip("needs %.1f GB of device memory, %.1f GB are free" % (need / 1e9, avail / 1e9))


def column_plan(ncols, ppc, sparse):
    """(scale per column, set of zero columns): zero columns sit in the middle of the first group of 16 planes, at the end
    (the last plane of a partial group) and right after the loudest column (scale 1e3 at column 1)."""
    scale = [SCALES[k % 4] for k in range(ncols)]
    if sparse:
        keep = {0, 1, 14 // ppc, 15 // ppc, 16 // ppc, 17 // ppc, ncols - 2}
        zero = set(range(ncols)) - keep
    elif ncols >= 4:
        zero = {2, 7 // ppc, ncols - 1} & set(range(ncols))
    elif ncols >= 2:
        zero = {ncols - 1}
    else:
        zero = set()
    return scale, zero


def random_planes(c, seed):
    """float32 grids [columns, ppc, M^d]."""
    ppc = 2 if c.pairs else 1
    ncols = c.B * c.C
    scale, zero = column_plan(ncols, ppc, c.sparse)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    M = 2 * c.N
    g = torch.empty((ncols, ppc, M ** c.d), dtype=torch.float32, device="cuda")
    for k in range(ncols):
        if k in zero:
            g[k].zero_()
        else:
            g[k].normal_(generator=gen)
            g[k] *= scale[k]
    return g, zero


def random_band(c, seed):
    """xhat [B, N^d, C] (complex64 if c.other else float32), scaled column by column."""
    ppc = 2 if c.pairs else 1
    ncols = c.B * c.C
    scale, zero = column_plan(ncols, ppc, c.sparse)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    K = c.N ** c.d
    x = torch.zeros((c.B, K, c.C), dtype=torch.complex64 if c.other else torch.float32, device="cuda")
    for k in range(ncols):
        if k in zero:
            continue
        v = torch.randn((K, 2), generator=gen, device="cuda") * scale[k]
        x[k // c.C, :, k % c.C] = torch.view_as_complex(v) if c.other else v[:, 0]
    return x, zero


def ref_adjoint(col, c, dtype, real_output, mult=None):
    """Reference band [N..N] of one column col [ppc, M^d] (float32), in `dtype` arithmetic, returned in float64."""
    rdt, cdt = rt._types(dtype)
    M = 2 * c.N
    g = col.to(rdt)
    g = torch.complex(g[0], g[1] if c.pairs else torch.zeros_like(g[0])).reshape((1,) + (M,) * c.d)
    y = rt._grid_to_band(g, c.N, M_CUT, dtype)[0]
    if mult is not None:
        y = y * mult.reshape(y.shape).to(cdt if mult.is_complex() else rdt)
    y = y.to(torch.complex128)
    return y.real.contiguous() if real_output else y


def ref_forward(xcol, c, dtype):
    """Reference planes [ppc, M..M] of one band column xcol [N^d], in `dtype` arithmetic, returned in float64."""
    _, cdt = rt._types(dtype)
    v = xcol.to(cdt).reshape((1,) + (c.N,) * c.d)
    g = rt._band_to_grid(v, M_CUT, dtype)[0].to(torch.complex128)
    return torch.stack([g.real, g.imag]) if c.pairs else g.real[None].contiguous()


def figures(got, ref, faces=None):
    """rel-L2, worst (d-1)-dimensional slice against its own norm, worst element against the rms; with `faces` (indices)
    also the slice figures of those indices, worst over the axes."""
    e2 = (got - ref).abs().double() ** 2
    n2 = ref.abs().double() ** 2
    d = ref.dim()
    rel = math.sqrt(float(e2.sum()) / float(n2.sum()))
    elem = math.sqrt(float(e2.max()) / float(n2.mean()))
    worst, face = 0.0, [0.0] * len(faces or ())
    if d > 1:
        for a in range(d):
            other = tuple(b for b in range(d) if b != a)
            s = torch.sqrt(e2.sum(dim=other) / n2.sum(dim=other))
            worst = max(worst, float(s.max()))
            for i, f in enumerate(faces or ()):
                face[i] = max(face[i], float(s[f]))
    return rel, worst, elem, face


class Tally:
    """Worst figures of the library and of the float32 yardstick over the planes of a case."""

    def __init__(self):
        self.lib = [0.0, 0.0, 0.0]
        self.yard = [0.0, 0.0, 0.0]
        self.faces = [0.0, 0.0, 0.0]

    def add(self, got, ref32, ref, faces=None):
        f = figures(got, ref, faces)
        y = figures(ref32, ref)
        self.lib = [max(a, b) for a, b in zip(self.lib, f[:3])]
        self.yard = [max(a, b) for a, b in zip(self.yard, y[:3])]
        self.faces = [max(a, b) for a, b in zip(self.faces, f[3])] if faces else self.faces
        return f[0]

    def check(self, label, d):
        print("%s: rel-L2 %.2e (float32 %.2e)  slice %.2e (%.2e)  element %.2e (%.2e)  faces -N/2, 0, N/2-1: %s"
              % (label, self.lib[0], self.yard[0], self.lib[1], self.yard[1], self.lib[2], self.yard[2],
                 " ".join("%.2e" % f for f in self.faces)))
        assert self.lib[0] <= (T1 if d == 1 else T1N), label
        assert self.lib[1] <= YARD * self.yard[1], label
        assert self.lib[2] <= YARD * self.yard[2], label


def run_adjoint(c, planes, mult=None):
    xc, ro = flags(c, "adjoint")
    y = torch.full((c.B, c.N ** c.d, c.C), float("nan"), dtype=torch.float32 if ro else torch.complex64, device="cuda")
    _lib.fft_stage(problem(c.d, c.N, c.B, c.C), True, xc, ro, planes.reshape(-1, planes.shape[-1]), y, mult)
    return y


def run_forward(c, xhat):
    xc, ro = flags(c, "forward")
    ppc = 2 if c.pairs else 1
    g = torch.full((c.B * c.C * ppc, (2 * c.N) ** c.d), float("nan"), dtype=torch.float32, device="cuda")
    _lib.fft_stage(problem(c.d, c.N, c.B, c.C), False, xc, ro, g, xhat)
    return g


def check_adjoint(c, planes, zero, y, label, mult=None):
    assert bool(torch.isfinite(torch.view_as_real(y) if y.is_complex() else y).all()), label
    ro = c.other
    tally = Tally()
    faces = (0, c.N // 2, c.N - 1)
    tol = T1 if c.d == 1 else T1N
    for k in range(c.B * c.C):
        got = y[k // c.C, :, k % c.C].reshape((c.N,) * c.d)
        if k in zero:
            assert not bool(got.count_nonzero()), (label, "zero column", k)
            continue
        ref = ref_adjoint(planes[k], c, torch.float64, ro, mult)
        ref32 = ref_adjoint(planes[k], c, torch.float32, ro, mult)
        rel = tally.add(got.to(ref.dtype), ref32, ref, faces)
        assert rel <= tol, (label, "column", k, rel)
    tally.check(label, c.d)


def check_forward(c, xhat, zero, g, label):
    assert bool(torch.isfinite(g).all()), label
    ppc = 2 if c.pairs else 1
    M = 2 * c.N
    g = g.reshape((c.B * c.C, ppc) + (M,) * c.d)
    tally = Tally()
    tol = T1 if c.d == 1 else T1N
    for k in range(c.B * c.C):
        if k in zero:
            assert not bool(g[k].count_nonzero()), (label, "zero column", k)
            continue
        ref = ref_forward(xhat[k // c.C, :, k % c.C], c, torch.float64)
        ref32 = ref_forward(xhat[k // c.C, :, k % c.C], c, torch.float32)
        for part in range(ppc):
            rel = tally.add(g[k, part].double(), ref32[part], ref[part])
            assert rel <= tol, (label, "column", k, "part", part, rel)
    tally.check(label, c.d)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_random_planes(c, monkeypatch):
    """Both directions on thousandfold-scaled random planes with zero columns inside the layout; the chunked cases also
    against the same call in one chunk -- bit for bit where no plane changes its route."""
    guard_memory(c)
    ran = set()
    for direction in c.dirs:
        label = "%s %s" % (case_id(c), direction)
        set_env(monkeypatch, c, c.budget)
        rows = assert_route(c, direction)
        if direction == "adjoint":
            src, zero = random_planes(c, 11)
            out = run_adjoint(c, src)
            check_adjoint(c, src, zero, out, label)
        else:
            src, zero = random_band(c, 12)
            out = run_forward(c, src)
            check_forward(c, src, zero, out, label)
        if c.budget and not c.sparse:
            set_env(monkeypatch, c, None)
            r, whole = chunk_routes(c, direction)
            assert len(whole) == 1 and r.chunk_planes == r.total_planes, (r, c)
            one = run_adjoint(c, src) if direction == "adjoint" else run_forward(c, src)
            if all(q[1] == whole[0][1] for q in rows):
                assert torch.equal(torch.view_as_real(out) if out.is_complex() else out,
                                   torch.view_as_real(one) if one.is_complex() else one), (label, "chunked != one chunk")
            elif direction == "adjoint":
                check_adjoint(c, src, zero, one, label + " (one chunk)")
            else:
                check_forward(c, src, zero, one, label + " (one chunk)")
        ran.add(direction)
        del src, out
    assert ran == set(c.dirs) == {"adjoint", "forward"}


# ---- the 2-D column pass at every tile width make_col_geom returns ---------------------------------------------------------

def width_steps(N, direction, pairs, other):
    """[(columns, tile width)] at the first column count of every tile width, and the last before each change, from the
    route record."""
    xc, ro = (pairs, other) if direction == "adjoint" else (other, not pairs)
    steps, prev = [], None
    for K in range(1, 65):
        r = _lib.fft_route(problem(2, N, K, 1), direction == "adjoint", xc, ro)
        nc = r.nc_axis0 if direction == "adjoint" else r.nc_forward
        assert r.fft == r.chunk_fft == "own_planar" and nc in (4, 8, 16), r
        if nc != prev:
            if prev is not None:
                steps.append((K - 1, prev))
            steps.append((K, nc))
            prev = nc
    return sorted(set(steps))


@pytest.mark.parametrize("pairs,other", COMBOS)
@pytest.mark.parametrize("N", [64, 128, 256, 512])
def test_2d_column_pass_tile_widths(N, pairs, other, monkeypatch):
    """2-D grids of the own row passes: every tile width of the one column pass, at the plane counts on both sides of every
    step (M = 128: 12 | 13 and 21 | 22 planes).  The columns are point sets of one column (the in-place layout)."""
    base = case(2, N, 1, 1, pairs, other, "own_planar", ["own_planar"], NONE)
    set_env(monkeypatch, base, None)
    seen, listed = {}, {}
    for direction in ("adjoint", "forward"):
        steps = width_steps(N, direction, pairs, other)
        listed[direction] = {nc for _, nc in steps}
        if N == 64:
            # M = 128: 4 columns up to 12 launch planes, 8 for 13 .. 21, 16 above (the adjoint pass launches one plane per
            # column, the forward pass one per real plane)
            per = (2 if pairs else 1) if direction == "forward" else 1
            assert all(nc == (4 if K * per <= 12 else 8 if K * per <= 21 else 16) for K, nc in steps), steps
            assert {nc for _, nc in steps} == {4, 8, 16} and len(steps) == 5, steps
        for K, nc in steps:
            c = case(2, N, K, 1, pairs, other, "own_planar", ["own_planar"],
                     (0, nc, 0) if direction == "adjoint" else (0, 0, nc), dirs=(direction,))
            label = "%s %s NC=%d" % (case_id(c), direction, nc)
            r, rows = chunk_routes(c, direction)
            assert rows == [(r.total_planes, "own_planar", c.nc)], (rows, c)
            if direction == "adjoint":
                src, zero = random_planes(c, 21)
                check_adjoint(c, src, zero, run_adjoint(c, src), label)
            else:
                src, zero = random_band(c, 22)
                check_forward(c, src, zero, run_forward(c, src), label)
            seen.setdefault(direction, set()).add(nc)
    assert set(seen) == {"adjoint", "forward"} and seen == listed, (seen, listed)


def test_2d_three_columns_go_through_the_layout_transposes(monkeypatch):
    """C = 3 on a 2-D grid of the column pass: column_layout_kernel in both directions, float and float2 elements."""
    for pairs, other in [(True, False), (False, True)]:
        c = case(2, 64, 5, 3, pairs, other, "own_planar", ["own_planar"], (0, 8, 16 if pairs else 8))
        set_env(monkeypatch, c, None)
        for direction in ("adjoint", "forward"):
            label = "%s %s" % (case_id(c), direction)
            assert_route(c, direction)
            if direction == "adjoint":
                src, zero = random_planes(c, 31)
                check_adjoint(c, src, zero, run_adjoint(c, src), label)
            else:
                src, zero = random_band(c, 32)
                check_forward(c, src, zero, run_forward(c, src), label)


# ---- unit impulses ------------------------------------------------------------------------------------------------------------

IMPULSE_SHAPES = [(1, 8), (1, 48), (2, 8), (2, 24), (2, 64), (2, 128), (2, 256), (2, 512), (3, 8), (3, 12), (3, 32), (3, 64),
                  (3, 128)]
AMPLITUDE = 3.0


def impulse_cells(d, M):
    cells = [(0, 0, 0), (M - 1, M - 1, M - 1), (M // 2, 0, M - 1), (M // 4 + 1, M // 2 - 3, 5)]
    return [t[3 - d:] for t in cells]


def impulse_frequencies(d, N):
    """Band indices (k + N/2): each face k = -N/2, 0, N/2 - 1 on each axis with interior indices on the others, the three
    corners of equal faces, and one interior frequency."""
    inner = (N // 4 + 1, N // 2 + 2, 3 % N)[3 - d:]
    out = [inner]
    for f in (0, N // 2, N - 1):
        out.append((f,) * d)
        for a in range(d):
            out.append(tuple(f if b == a else inner[b] for b in range(d)))
    return sorted(set(out))


def flat(idx, S):
    k = 0
    for i in idx:
        k = k * S + i
    return k


@pytest.mark.parametrize("d,N", IMPULSE_SHAPES, ids=["%dd-N%d" % s for s in IMPULSE_SHAPES])
def test_unit_impulses(d, N, monkeypatch):
    """One grid cell (adjoint) or one frequency (forward) per column, every column of the call another one, compared
    element by element against float64 relative to the amplitude: a wrong twiddle entry, mirror row, pruned column or
    roll-off index shows in full.  Imaginary impulses in the odd columns."""
    M = 2 * N
    cells, freqs = impulse_cells(d, M), impulse_frequencies(d, N)
    for direction, spots, S in (("adjoint", cells, M), ("forward", freqs, N)):
        monkeypatch.delenv("NFFT_HIP_CHUNK_BYTES", raising=False)
        monkeypatch.delenv("NFFT_HIP_NO_COLFFT", raising=False)
        r = _lib.fft_route(problem(d, N, len(spots), 1), direction == "adjoint", True, False)
        c = case(d, N, len(spots), 1, True, direction == "forward", r.fft, [r.fft], NONE)
        assert r.fft == {1: "full", 2: "own_planar" if N >= 64 else "full",
                         3: "own_planar" if N >= 64 else "full" if N == 12 else "roc_rows"}[d] and r.chunk_fft == r.fft, r
        lib_worst = yard_worst = 0.0
        if direction == "adjoint":
            src = torch.zeros((len(spots), 2, M ** d), dtype=torch.float32, device="cuda")
            for k, cell in enumerate(spots):
                src[k, k & 1, flat(cell, M)] = AMPLITUDE
            out = run_adjoint(c, src)
            assert bool(torch.isfinite(torch.view_as_real(out)).all())
            for k in range(len(spots)):
                ref = ref_adjoint(src[k], c, torch.float64, False)
                ref32 = ref_adjoint(src[k], c, torch.float32, False)
                got = out[k, :, 0].reshape(ref.shape).to(torch.complex128)
                lib_worst = max(lib_worst, float((got - ref).abs().max()) / AMPLITUDE)
                yard_worst = max(yard_worst, float((ref32 - ref).abs().max()) / AMPLITUDE)
        else:
            src = torch.zeros((len(spots), N ** d, 1), dtype=torch.complex64, device="cuda")
            for k, f in enumerate(spots):
                src[k, flat(f, N), 0] = AMPLITUDE * (1j if k & 1 else 1.0)
            out = run_forward(c, src).reshape((len(spots), 2) + (M,) * d)
            assert bool(torch.isfinite(out).all())
            for k in range(len(spots)):
                ref = ref_forward(src[k, :, 0], c, torch.float64)
                ref32 = ref_forward(src[k, :, 0], c, torch.float32)
                lib_worst = max(lib_worst, float((out[k].double() - ref).abs().max()) / AMPLITUDE)
                yard_worst = max(yard_worst, float((ref32 - ref).abs().max()) / AMPLITUDE)
        print("%dd N=%d %s impulses (%s): worst element / amplitude %.2e (float32 %.2e)"
              % (d, N, direction, r.fft, lib_worst, yard_worst))
        assert lib_worst <= YARD * yard_worst, (d, N, direction, lib_worst, yard_worst)


# ---- the fastsum's per-frequency factor ---------------------------------------------------------------------------------------

MULT_CASES = [
    case(1, 48, 2, 3, True, False, "full", ["full"], NONE, dirs=("adjoint",)),
    case(2, 24, 2, 3, True, False, "full", ["full"], NONE, dirs=("adjoint",)),
    case(3, 16, 2, 3, True, False, "roc_rows", ["roc_rows"], (16, 16, 16), dirs=("adjoint",)),
    case(3, 64, 1, 1, True, False, "own_planar", ["own_planar"], (16, 16, 16), dirs=("adjoint",)),
    case(3, 64, 2, 3, False, True, "own_planar", ["own_planar"], (16, 16, 16), dirs=("adjoint",)),
    case(2, 128, 3, 1, True, False, "own_planar", ["own_planar"], (0, 4, 0), dirs=("adjoint",)),
    case(3, 64, 3, 11, False, False, "own_planar", ["own_ci"], (16, 16, 16), dirs=("adjoint",)),
    case(3, 64, 1, 16, True, True, "own_planar", ["own_ci"], (16, 16, 16), dirs=("adjoint",)),
]


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("c", MULT_CASES, ids=case_id)
def test_per_frequency_factor(c, kind, monkeypatch):
    """mult_kind 1 (real) and 2 (complex): y = roll-off * band * factor on every route (adjoint only: the forward stage has
    no factor)."""
    set_env(monkeypatch, c, None)
    assert_route(c, "adjoint")
    gen = torch.Generator(device="cuda").manual_seed(41)
    w = torch.randn((c.N ** c.d, 2), generator=gen, device="cuda") + 0.5
    mult = w[:, 0].contiguous() if kind == 1 else torch.view_as_complex(w).contiguous()
    src, zero = random_planes(c, 42)
    out = run_adjoint(c, src, mult)
    check_adjoint(c, src, zero, out, "%s factor kind %d" % (case_id(c), kind), mult)


def test_column_innermost_rows_at_1024_are_out_of_reach(monkeypatch):
    """row_*_ci_kernel<9> (M = 1024) needs a chunk of 32 planes of 4 GiB with their spectra and scratch, about 300 GB: under
    a budget of the device's whole memory make_route still cuts planar chunks."""
    total = torch.cuda.get_device_properties(0).total_memory
    assert 32 * plane_bytes(3, 512) > total
    monkeypatch.setenv("NFFT_HIP_CHUNK_BYTES", str(total))
    for adjoint in (True, False):
        r = _lib.fft_route(problem(3, 512, 1, 16), adjoint, True, False)
        assert r.ci and r.fft == "own_planar" and r.total_planes == 32 and r.chunk_planes < 32, r
        assert r.chunk_fft == "own_planar", r
