"""The case table of tests/test_gpu_plan_edges.py: point sets built to stand on the point plan's capacity boundaries, route
switches and cell borders (csrc/binning.hip, csrc/common.h split_cell).  Imports numpy only.  tests/test_plan_ref.py
asserts without a GPU, from the layout entry and the reference counts, that every case reaches the class it claims.

A case: dimension, bandwidth N, point sets B, coefficient columns C, cutoff m, the NFFT_HIP_* switches of its process
(cases with switches run in a child: they are read once per process), `make()` -> (pos float32 [n, d], batch int64 [n] or
None), and `claims`: facts (plan_ref.facts) the case must show.  Tile extents named here (23 x 55 cells with halo for the
matrix-core tiling at m = 4, 32 x 64 / 32 x 32 owned tiles, 16 x 32 x 7 narrow tiles, 32 x 32 in 2-D, 256 cells in 1-D)
only place points; the claims are checked against the library's own layout.
"""
import zlib

import numpy as np

GROUPED = {"NFFT_HIP_STREAM_MIN": "1"}  # every work item counts as big enough for the streamed gather: column-group order
FORCE_OWNED = {"NFFT_HIP_OWNED": "1"}   # the owner-computes plan for a single column below N = 128
CASES = {}


class Case:
    def __init__(self, name, d, N, B, make, claims, m=4, C=1, env=None, seal=False, consumer=False, borders=False):
        self.name, self.d, self.N, self.B, self.m, self.C = name, d, N, B, m, C
        self.env = dict(env or {})
        self._make, self.claims = make, claims
        self.seal, self.consumer, self.borders = seal, consumer, borders
        assert name not in CASES
        CASES[name] = self

    def make(self):
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        pos, batch = self._make(rng)
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, self.d)
        if batch is not None:
            batch = np.ascontiguousarray(batch, dtype=np.int64)
            assert batch.shape == (pos.shape[0],) and (np.diff(batch) >= 0).all()
            assert batch.size == 0 or (batch[0] >= 0 and batch[-1] < self.B)
        return pos, batch

    @property
    def env_key(self):
        return " ".join("%s=%s" % kv for kv in sorted(self.env.items()))


def coord(c, M, u):
    """float32 coordinate in [-0.5, 0.5) that lies the fraction u (well inside (0, 1)) into cell c of M."""
    v = (np.asarray(c, dtype=np.float64) + u) / M
    return np.where(v >= 0.5, v - 1.0, v).astype(np.float32)


def box(rng, k, M, *ranges):
    return np.stack([coord(rng.integers(lo, hi, k), M, rng.uniform(0.05, 0.95, k)) for lo, hi in ranges], axis=1)


def uniform(rng, n, d):
    return (rng.random((n, d)) - 0.5).astype(np.float32)


def sorted_batch(rng, n, B):
    if B == 1:
        return None
    b = np.sort(rng.integers(0, B, n)).astype(np.int64)
    if n >= 2:
        b[0], b[-1] = 0, B - 1
    return b


def pencil_sets(rng, M, T1, T2, counts, slabs=None, cols=None):
    """Points by (point set, pencil): counts[b][j1 * nt2 + j2] points in pencil (j1, j2) of set b, in random cells of the
    pencil; the fullest pencil of a set takes its axis-0 cells from `slabs` and its columns inside the pencil from `cols`,
    if given.  Returns (pos, batch)."""
    nt1, nt2 = -(-M // T1), -(-M // T2)
    pos, batch = [], []
    for b, row in enumerate(counts):
        assert len(row) == nt1 * nt2
        for p, k in enumerate(row):
            j1, j2 = divmod(p, nt2)
            lo2 = j2 * T2
            r2 = (lo2 + cols[0], lo2 + cols[1]) if cols and k == max(row) else (lo2, min(M, lo2 + T2))
            r0 = slabs if slabs and k == max(row) else (0, M)
            pos.append(box(rng, k, M, r0, (j1 * T1, min(M, j1 * T1 + T1)), r2))
            batch.append(np.full(k, b, dtype=np.int64))
    return np.concatenate(pos), (np.concatenate(batch) if len(counts) > 1 else None)


# ---- capacity of the one-pass second level: 3-D N = 32 on the matrix-core tiling (more than 30 000 points: below that
# the 64^3 grid takes the narrow tiling), 3 x 2 pencils of 64 slabs, one first-level segment; column-group order --------
def _fuse(k, B=1, slabs=None, cols=None):
    other = (31000 - k) // (6 * B - 1)
    rows = [[other] * 6 for _ in range(B)]
    rows[B - 1][0] = k  # pencil (0, 0): columns 0..54, all three column groups
    return lambda rng: pencil_sets(rng, 64, 23, 55, rows, slabs, cols)


for _k in (8192, 8193, 16383, 16384, 16385):
    Case("fuse-%d" % _k, 3, 32, 1, _fuse(_k), dict(wide=True, CG=3, fuse=True, l1bins=128, l1seg=1, npencils=6, max_l1=_k,
                                                  route=int(_k <= 16384)), env=GROUPED, consumer=_k >= 16384)
Case("fuse-16384-one-key", 3, 32, 1, _fuse(16384, slabs=(7, 8), cols=(0, 23)),
     dict(wide=True, CG=3, max_l1=16384, route=1), env=GROUPED)
for _k in (16384, 16385):
    Case("fuse-%d-second-set" % _k, 3, 32, 2, _fuse(_k, B=2), dict(wide=True, CG=3, npencils=12, max_l1=_k, route=int(_k <= 16384)),
         env=GROUPED)

# ---- small bins on the eight parts: one bin beyond the one-pass capacity sends every bin there ------------------------
_SMALL = [[0, 16385, 1, 7, 8, 9], [0, 13700, 0, 1, 7, 8], [9, 0, 1, 7, 8, 0]]
Case("parts-small-bins", 3, 32, 3, lambda rng: pencil_sets(rng, 64, 23, 55, _SMALL),
     dict(wide=True, CG=3, npencils=18, max_l1=16385, route=0, l1_has={0, 1, 7, 8, 9}, l1_first_last_empty=True), env=GROUPED)
Case("parts-small-bins-narrow", 3, 32, 1, lambda rng: pencil_sets(rng, 64, 16, 32, [[0, 16385, 1, 7, 8, 9, 3, 0]]),
     dict(wide=False, CG=1, npencils=8, max_l1=16385, route=0, l1_has={0, 1, 7, 8, 9}, l1_first_last_empty=True))

# ---- first-level segments ----------------------------------------------------------------------------------------------
# (64 slabs: a segment of 128 bins is a partial one; at 60 000 points the one segment of the widest pencil, 31 % of the
# cells, holds more than the one-pass kernel takes -- a uniform input on the eight parts)
for _n, _bins, _seg, _route in ((30001, 128, 1, 1), (60000, 64, 1, 0), (80000, 32, 2, 1), (160000, 16, 4, 1)):
    Case("segments-%d" % _bins, 3, 32, 1, lambda rng, n=_n: (uniform(rng, n, 3), None),
         dict(wide=True, l1bins=_bins, l1seg=_seg, partial_segment=_bins == 128, route=_route))
Case("segments-144", 3, 72, 1, lambda rng: (uniform(rng, 40000, 3), None),
     dict(wide=True, l1bins=128, l1seg=2, partial_segment=True, route=1), consumer=True)
Case("segments-144-all-in-last", 3, 72, 1,
     lambda rng: (np.concatenate([box(rng, 40000, 144, (128, 144)), uniform(rng, 40000, 2)], axis=1), None),
     dict(l1seg=2, partial_segment=True, l1_first_last_empty=False, l1_has={0}))
Case("segments-144-none-in-last", 3, 72, 1,
     lambda rng: (np.concatenate([box(rng, 40000, 144, (0, 128)), uniform(rng, 40000, 2)], axis=1), None),
     dict(l1seg=2, partial_segment=True, l1_has={0}))
Case("segments-80", 3, 40, 1, lambda rng: (uniform(rng, 40000, 3), None),
     dict(wide=True, l1bins=128, l1seg=1, partial_segment=True, route=1))

# ---- narrow 3-D tilings ------------------------------------------------------------------------------------------------
for _N in (16, 24):
    for _B in (1, 3):
        Case("narrow-%d-sets-%d" % (_N, _B), 3, _N, _B, lambda rng, B=_B: (uniform(rng, 5000, 3), sorted_batch(rng, 5000, B)),
             dict(wide=False, two_level=True, one_level=False, fuse=True, route=1))

# ---- one-level plans: 1-D, 256 cells per tile, bins = B * ceil(2N / 256); G threads per bin in the in-kernel scan -------
_BINS_1D = {1: (128, 1, 64), 2: (256, 1, 64), 4: (512, 1, 64), 5: (128, 5, 64), 8: (1024, 1, 64), 9: (384, 3, 32),
            17: (128, 17, 16), 63: (1152, 7, 8), 64: (8192, 1, 8), 65: (1664, 5, 4), 128: (8192, 2, 4), 129: (5504, 3, 2),
            257: (128, 257, 1)}
for _bins, (_N, _B, _G) in _BINS_1D.items():
    for _n in (3000, 1) if _bins in (1, 65) else (3000,):
        Case("line-%d-bins-%d" % (_bins, _n), 1, _N, _B, lambda rng, n=_n, B=_B: (uniform(rng, n, 1), sorted_batch(rng, n, B)),
             dict(one_level=True, local_scan=True, scan="none", npencils=_bins, G=_G))
for _B, _G in ((1, 32), (5, 4)):
    Case("plane-64-sets-%d" % _B, 2, 64, _B, lambda rng, B=_B: (uniform(rng, 3000, 2), sorted_batch(rng, 3000, B)),
         dict(one_level=True, local_scan=True, npencils=16 * _B, G=_G))

# ---- scan thresholds: items = first-level bins x slices + 1 ----------------------------------------------------------------
def _plain(d, n, B):
    return lambda rng: (uniform(rng, n, d), sorted_batch(rng, n, B))


Case("scan-16384-items", 1, 16256, 3, _plain(1, 44032, 3), dict(one_level=True, local_scan=True, scan="none", scan_items=16384))
Case("scan-16385-items", 2, 64, 8, _plain(2, 131072, 8), dict(one_level=True, local_scan=False, scan="small16", scan_items=16385))
Case("scan-65536-items", 1, 384, 257, _plain(1, 87040, 257), dict(one_level=True, local_scan=False, scan="small16", scan_items=65536))
Case("scan-65537-items", 2, 128, 8, _plain(2, 131072, 8), dict(one_level=True, local_scan=False, scan="hipcub", scan_items=65537))
Case("scan-lds-8176-bins", 2, 64, 511, _plain(2, 1000, 511), dict(one_level=True, local_scan=True, npencils=8176, G=1))
Case("scan-lds-8177-bins", 1, 1664, 629, _plain(1, 1000, 629), dict(one_level=True, local_scan=False, npencils=8177, scan="small16"))
Case("scan-4096-items", 3, 8, 315, _plain(3, 13312, 315), dict(two_level=True, one_level=False, scan="small4", scan_items=4096))
Case("scan-4097-items", 3, 8, 256, _plain(3, 16384, 256), dict(two_level=True, one_level=False, scan="small16", scan_items=4097))

# ---- slices ------------------------------------------------------------------------------------------------------------
for _n in (1, 511, 512, 513, 1023, 1024, 1025, 8 * 1024 + 1):
    _last = _n - (_n - 1) // 1024 * 1024
    Case("slices-plane-%d" % _n, 2, 64, 1, _plain(2, _n, 1), dict(one_level=True, block_points=1024, last_slice=_last))
    Case("slices-3d-%d" % _n, 3, 40, 1, _plain(3, _n, 1), dict(wide=True, two_level=True, block_points=1024, last_slice=_last))
for _n, _last in ((68 * 2048 - 1, 2047), (68 * 2048 + 1, 1)):
    Case("slices-2048-%d" % _n, 2, 512, 8, _plain(2, _n, 8),
         dict(two_level=True, one_level=True, npencils=8192, block_points=2048, last_slice=_last, scan="hipcub"))

# ---- single-level sort: more than 8 192 first-level bins, or no points ---------------------------------------------------
for _n in (1, 1000, 100000):
    Case("single-level-%d" % _n, 2, 512, 9, _plain(2, _n, 9), dict(two_level=False, scan="small16", scan_items=9217),
         consumer=_n == 1000)
Case("empty-3d", 3, 40, 1, lambda rng: (np.zeros((0, 3), np.float32), None), dict(two_level=False, entries=0))
Case("empty-plane", 2, 64, 1, lambda rng: (np.zeros((0, 2), np.float32), None), dict(two_level=False, entries=0))


# ---- owned plans: windows placed against the tile borders and the torus seam ----------------------------------------------
def _owned(M, T2, rep=40, filler=6000):
    T1, m = 32, 4
    inside1, inside2 = [T1 + 10, T1 + m, T1 - m - 2, 2 * T1 + 12], [T2 + 10, T2 + m, T2 - m - 2, T2 + 14]
    cross1, cross2 = [T1 - 2, T1 + 1, T1 - m - 1, T1 + m - 1], [T2 - 2, T2 + 1, T2 - m - 1, T2 + m - 1]
    seam1, seam2 = [1, M - 2, 0, M - 1, m - 1, M - m - 1], [2, M - 3, 0, M - 1, m - 1, M - m - 1]

    def make(rng):
        parts = [uniform(rng, filler, 3)]
        for a1, a2 in ((inside1, inside2), (cross1, inside2), (inside1, cross2), (cross1, cross2), (seam1, inside2),
                       (inside1, seam2), (seam1, seam2), (seam1, cross2), (cross1, seam2)):
            c1 = np.repeat(a1, len(a2) * rep)
            c2 = np.tile(np.repeat(a2, rep), len(a1))
            k = c1.size
            parts.append(np.stack([coord(rng.integers(0, M, k), M, rng.uniform(0.05, 0.95, k)),
                                   coord(c1, M, rng.uniform(0.05, 0.95, k)), coord(c2, M, rng.uniform(0.05, 0.95, k))], axis=1))
        pos = np.concatenate(parts)
        return pos[rng.permutation(pos.shape[0])], None
    return make


# (touch_min: at least so many constructed points with windows in 1, 2 and 4 tiles; wrapping_min: across the seam)
Case("owned-64-pair", 3, 64, 1, _owned(128, 32), dict(wide=True, has_owned=True, pair=True, touch_min=(640, 1280, 640), wrapping_min=2000),
     C=2, consumer=True)
Case("owned-96-pair", 3, 96, 1, _owned(192, 32), dict(wide=True, has_owned=True, pair=True, touch_min=(640, 1280, 640), wrapping_min=2000), C=2)
Case("owned-64-single", 3, 64, 1, _owned(128, 64), dict(wide=True, has_owned=True, pair=False, touch_min=(640, 1280, 640), wrapping_min=2000),
     env=FORCE_OWNED)
Case("owned-96-single", 3, 96, 1, _owned(192, 64), dict(wide=True, has_owned=True, pair=False, touch_min=(640, 1280, 640), wrapping_min=2000),
     env=FORCE_OWNED)


# ---- coordinates on cell borders -----------------------------------------------------------------------------------------
def border_values(M, extents):
    """-0.0, +0.0, -0.5, the largest float32 below 0.5, 0.5, -2^-30, -2^-40, and k / M with its two float32 neighbours for
    every tile-border cell k of the tile extents given (0 and M, the first and the last tile's outer borders, included)."""
    f = np.float32
    vals = [f(-0.0), f(0.0), f(-0.5), np.nextafter(f(0.5), f(0)), f(0.5), f(-2.0 ** -30), f(-2.0 ** -40)]
    for T in extents:
        for k in sorted(set(range(0, M, T)) | {M}):
            x = k / M
            c = f(x - 1.0 if x >= 0.5 else x)
            vals += [c, np.nextafter(c, f(-1)), np.nextafter(c, f(1))]
    return np.array(vals, dtype=np.float32)


def _borders(d, M, extents, filler, B=1, rep=2):
    def make(rng):
        parts = [uniform(rng, filler, d)]
        for a in range(d):
            v = np.repeat(border_values(M, extents[a]), rep)
            p = uniform(rng, v.size, d)
            p[:, a] = v
            parts.append(p)
        pos = np.concatenate(parts)
        pos = pos[rng.permutation(pos.shape[0])]
        return pos, sorted_batch(rng, pos.shape[0], B)
    return make


_BORDERS = dict(borders=True)
Case("borders-3d-64", 3, 32, 1, _borders(3, 64, [[1], [23], [55]], 31000), dict(wide=True, CG=3, route=1), env=GROUPED,
     consumer=True, **_BORDERS)
Case("borders-3d-144", 3, 72, 2, _borders(3, 144, [[1, 128], [23], [55]], 6000, B=2), dict(wide=True, l1seg=2), **_BORDERS)
Case("borders-3d-narrow-48", 3, 24, 1, _borders(3, 48, [[7], [16], [32]], 3000), dict(wide=False), **_BORDERS)
Case("borders-plane-128", 2, 64, 2, _borders(2, 128, [[32], [32]], 2000, B=2), dict(one_level=True), **_BORDERS)
Case("borders-plane-144", 2, 72, 1, _borders(2, 144, [[32], [32]], 2000), dict(one_level=True), **_BORDERS)
Case("borders-line-768", 1, 384, 1, _borders(1, 768, [[256]], 2000), dict(one_level=True), **_BORDERS)
Case("borders-line-2048", 1, 1024, 3, _borders(1, 2048, [[256]], 2000, B=3), dict(one_level=True), **_BORDERS)
Case("borders-3d-80", 3, 40, 1, _borders(3, 80, [[1], [23], [55]], 4000), dict(wide=True, partial_segment=True), **_BORDERS)
Case("borders-3d-narrow-32", 3, 16, 3, _borders(3, 32, [[7], [16], [32]], 3000, B=3), dict(wide=False), **_BORDERS)
Case("borders-plane-1024", 2, 512, 9, _borders(2, 1024, [[32], [32]], 2000, B=9), dict(two_level=False), **_BORDERS)
Case("borders-owned-128-single", 3, 64, 1, _borders(3, 128, [[1], [23, 32], [55, 64]], 4000), dict(has_owned=True, pair=False),
     env=FORCE_OWNED, **_BORDERS)
Case("borders-owned-128", 3, 64, 1, _borders(3, 128, [[1], [23, 32], [55, 32]], 4000), dict(has_owned=True, pair=True), C=2, **_BORDERS)
Case("borders-owned-192", 3, 96, 1, _borders(3, 192, [[1], [23, 32], [55, 32]], 4000), dict(has_owned=True, pair=True), C=2, **_BORDERS)

# ---- the seal: one case per formation, the last point alone in its slice ---------------------------------------------------
Case("seal-two-level", 3, 40, 2, _plain(3, 5 * 1024 + 1, 2), dict(two_level=True, one_level=False, last_slice=1), seal=True)
Case("seal-local-scan", 2, 64, 2, _plain(2, 3 * 1024 + 1, 2), dict(one_level=True, local_scan=True, last_slice=1), seal=True)
Case("seal-scanned", 1, 1664, 629, _plain(1, 2 * 1024 + 1, 629), dict(one_level=True, local_scan=False, last_slice=1), seal=True)
Case("seal-single-level", 2, 512, 9, _plain(2, 1024 + 1, 9), dict(two_level=False), seal=True)


# ---- the cases tests/test_gpu_plan_sort.py has had all along (shapes only: their claims say what they do NOT reach) ----------
COMMITTED = [  # (d, N, n, B): uniform or clustered inputs of 5e4 .. 1e7 points
    (3, 256, 10_000_000, 1), (3, 64, 1_200_000, 1), (3, 64, 800_000, 4), (2, 256, 300_000, 1), (2, 64, 50_000, 3),
    (1, 4096, 200_000, 2), (2, 512, 1000, 8), (3, 32, 50_000, 1)]
