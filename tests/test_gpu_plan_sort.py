"""Point plans at the level of their tables: nfft_hip_plan_points against a torch reimplementation of the binning.

Geometry and table offsets come from the layout entry nfft_dbg_plan_layout, and every plan is also compared exactly with the
numpy reference of tests/plan_ref.py (tests/test_gpu_plan_edges.py has the small cases that stand on the sort's boundaries).
The plan's order inside a plan bin has never been fixed (LDS atomics hand out the slots), so nothing here depends on it:
every point appears once, every entry lies inside the offsets range of the plan bin its coordinates give, the last
offset is the entry count, and -- for plans in column-group order -- the groups inside every slab come in order 0, 1, 2.
The cases cover both second-level paths of the 3-D sort (the one-pass kernel when every first-level bin fits it, eight
parts per bin when a clustered input has bins beyond it), batched 3-D plans, 1-D and 2-D plans (first level only), and
2-D plans with 8 192 first-level bins and a single slice, whose one-pass first level needs more than 64 KB of LDS."""
import ctypes

import numpy as np
import pytest
import torch

import plan_ref
from conftest import rel_l2
from oracle import nfft_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from torch_nfft_amd import _lib
    return _lib.load()


def _plan(lib, d, N, m, pos, batch, B):
    from torch_nfft_amd import _lib
    n = pos.shape[0]
    prob = _lib.Problem(d, n, 1, B, N, m)
    nbytes = lib.nfft_hip_plan_bytes(ctypes.byref(prob))
    plan = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.nfft_hip_plan_points(ctypes.byref(prob), p(pos), p(batch), p(plan), nbytes, s))
    torch.cuda.synchronize()
    _lib.check_status()
    return plan, _lib.plan_layout(prob, 0)[0]


def _check_plan(lib, d, N, m, pos, batch=None, B=1, groups=False):
    """Builds the plan of (pos, batch) and checks its tables: against the binning recomputed here with torch, and exactly
    against the reference of tests/plan_ref.py.  Geometry and table offsets come from the layout entry."""
    n = pos.shape[0]
    M = 2 * N
    plan, L = _plan(lib, d, N, m, pos, batch, B)
    assert (L.dim, L.M, L.cap, L.grouped) == (d, M, n, groups)
    T1, T2, np0, nt2 = L.Ta1, L.Ta2, L.np0, L.nta2
    tiles_per_batch, ntiles = L.tiles_per_batch, L.ntiles
    offsets = plan[L.off_offsets: L.off_offsets + (ntiles + 1) * 4].view(torch.int32).long()
    assert int(offsets[0]) == 0
    assert int(offsets[-1]) == n  # the last offset is the entry count
    assert bool((offsets[1:] >= offsets[:-1]).all())
    if d == 3:
        rec = plan[L.off_spos: L.off_spos + n * 16].view(torch.float32).view(n, 4)
        idx = rec[:, 3].contiguous().view(torch.int32).long()
        coords = rec[:, :3]
    else:
        idx = plan[L.off_perm: L.off_perm + n * 4].view(torch.int32).long()
        coords = plan[L.off_spos: L.off_spos + n * d * 4].view(torch.float32).view(n, d)
    # every point appears once, with its own coordinates
    assert bool(((idx >= 0) & (idx < n)).all())
    assert int(torch.bincount(idx, minlength=n).max()) == 1
    assert torch.equal(coords, pos[idx])
    # (a float64 floor: split_cell's cell for all but coordinates a hair below zero, which these inputs do not have --
    # tests/plan_ref.py cells() is the exact statement, and check_plan below uses it)
    cell = torch.remainder(torch.floor(coords.double() * M).long(), M)
    c0 = cell[:, 0] // L.bin0 if d == 3 else torch.zeros_like(idx)
    c1 = cell[:, d - 2] if d >= 2 else torch.zeros_like(idx)
    c2 = cell[:, d - 1]
    b = batch[idx] if batch is not None else torch.zeros_like(idx)
    j2 = c2 // T2
    tile = b * tiles_per_batch + ((c1 // T1) * nt2 + j2) * np0 + c0
    slot = torch.arange(n, device="cuda")
    # every entry lies in the range of its plan bin
    assert bool((offsets[tile] <= slot).all()) and bool((slot < offsets[tile + 1]).all())
    if groups:
        # column-group order inside every slab: group of the window in the padded 64-column tile
        col = c2 - j2 * T2
        W = 2 * m + 2
        grp = torch.where(col + W <= 32, 0, torch.where(col >= 32, 2, 1))
        same = tile[1:] == tile[:-1]
        assert bool((grp[1:][same] >= grp[:-1][same]).all())
    # ... and exactly: offsets, the points of every bin, bit-equal records, the group words
    plan_ref.check_plan(L, plan_ref.cut_tables(L, plan.cpu().numpy()), pos.cpu().numpy(),
                        batch.cpu().numpy() if batch is not None else None)
    return plan


def _uniform(n, d, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((n, d), generator=gen, device="cuda") - 0.5


def _clustered(n, d, seed, frac=0.6, sigma=0.01):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    pos = torch.rand((n, d), generator=gen, device="cuda") - 0.5
    k = int(n * frac)
    pos[:k] = 0.1 + sigma * torch.randn((k, d), generator=gen, device="cuda")
    pos = pos - torch.floor(pos + 0.5)
    return pos.contiguous()


def test_plan_c3_uniform(lib):
    """The headline's plan: 10^7 uniform points on the 512^3 grid, column-group order, every bin in the one-pass kernel."""
    _check_plan(lib, 3, 256, 4, _uniform(10_000_000, 3, 1), groups=True)


def test_plan_c3_clustered(lib):
    """C3-clustered: 8 Gaussian clusters (sigma 0.05) -- dense bins send the plan to the eight-part second level."""
    n, d = 10_000_000, 3
    gen = torch.Generator(device="cuda").manual_seed(1)
    centres = torch.rand((8, d), generator=gen, device="cuda") - 0.5
    which = torch.randint(0, 8, (n,), generator=gen, device="cuda")
    pos = centres[which] + 0.05 * torch.randn((n, d), generator=gen, device="cuda")
    pos = (pos - torch.floor(pos + 0.5)).contiguous()
    _check_plan(lib, 3, 256, 4, pos, groups=True)


def test_plan_dense_64_cubed_both_paths(lib):
    """1.2 x 10^6 points on the 128^3 grid (short first-level segments): 60 % of them in one tight cluster (bins far
    beyond the one-pass kernel's capacity: eight parts), then uniform (one pass)."""
    _check_plan(lib, 3, 64, 4, _clustered(1_200_000, 3, 5), groups=True)
    _check_plan(lib, 3, 64, 4, _uniform(1_200_000, 3, 6), groups=True)


def test_plan_batched_3d(lib):
    n, B = 800_000, 4
    pos = _uniform(n, 3, 7)
    batch = torch.sort(torch.randint(0, B, (n,), device="cuda")).values
    batch[0], batch[-1] = 0, B - 1
    _check_plan(lib, 3, 64, 4, pos, batch, B)


@pytest.mark.parametrize("d,N,n,B", [(2, 256, 300_000, 1), (2, 64, 50_000, 3), (1, 4096, 200_000, 2)])
def test_plan_1d_2d(lib, d, N, n, B):
    pos = _uniform(n, d, 11)
    batch = None
    if B > 1:
        batch = torch.sort(torch.randint(0, B, (n,), device="cuda")).values
        batch[0], batch[-1] = 0, B - 1
    _check_plan(lib, d, N, 4, pos, batch, B)


def test_plan_8192_first_level_bins_one_slice(lib):
    """2-D N = 512 (1 024 tiles of 32 x 32 per point set) x 8 point sets = 8 192 first-level bins, 1 000 points (one
    slice): the one-level sort's in-kernel scan would need 2 x 8 192 x 4 B + the seal's 128 B of LDS, more than a launch
    gets by default.  The plan, and a transform on it against the oracle."""
    d, N, m, n, B = 2, 512, 4, 1000, 8
    pos = _uniform(n, d, 13)
    batch = torch.sort(torch.randint(0, B, (n,), device="cuda")).values
    batch[0], batch[-1] = 0, B - 1
    _check_plan(lib, d, N, m, pos, batch, B)
    import torch_nfft_amd as tn
    rng = np.random.default_rng(3)
    x = rng.standard_normal((n, 2)).astype(np.float32)
    y = tn.nfft_adjoint(torch.from_numpy(x).cuda(), pos, batch, bandwidth=N, cutoff=m)
    ref = nfft_ref.nfft_adjoint(x, pos.cpu().numpy(), batch.cpu().numpy(), N=N, m=m)
    assert rel_l2(y.cpu().numpy(), ref) < 2e-5


def test_transform_parity_one_pass_second_level(lib):
    """Adjoint + forward on a 3-D plan whose bins all take the one-pass second level, against the oracle."""
    import torch_nfft_amd as tn
    d, N, m, n = 3, 32, 4, 50_000
    rng = np.random.default_rng(17)
    pos = (rng.random((n, d)) - 0.5).astype(np.float32)
    x = rng.standard_normal((n, 2)).astype(np.float32)
    post = torch.from_numpy(pos).cuda()
    _check_plan(lib, d, N, m, post)
    y = tn.nfft_adjoint(torch.from_numpy(x).cuda(), post, None, bandwidth=N, cutoff=m)
    ya = nfft_ref.nfft_adjoint(x, pos, None, N=N, m=m)
    assert rel_l2(y.cpu().numpy(), ya) < 2e-5
    z = tn.nfft_forward(y, post, None, cutoff=m, real_output=True)
    za = nfft_ref.nfft_forward(ya, pos, None, m=m, real_output=True)
    assert rel_l2(z.cpu().numpy(), za) < 2e-5
