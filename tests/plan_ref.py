"""Reference of the point plan (csrc/binning.hip) and the checker of its tables.  Pure numpy, no GPU.

A plan files every point under the plan bin of its cell: (point set, tile in the internal axes 1 and 2, bin along axis 0).
The owned tiling files it under every tile its window [c - m, c + m + 1] touches (1, 2 or 4, wrapped on the torus).  Plans
in column-group order (CG = 3) also order a bin by the group of the point's window in the padded 64-column tile and record
where groups 1 and 2 start.  The order inside a (bin, group) is unspecified, and nothing here depends on it.

`layout` is a record of torch_nfft_amd._lib.plan_layout (anything with those attributes will do); `tables` the raw arrays
cut from a plan buffer by `cut_tables`.
"""
import numpy as np


class PlanError(AssertionError):
    """A plan table disagrees with the reference."""


def cells(pos32, M):
    """Cell of every coordinate as split_cell (csrc/common.h) defines it, in exact arithmetic: with e = x * M (exact in
    float64: 24 bits times an integer below 2^21), the cell is floor(e) mod M -- unless the fraction e - floor(e), rounded
    to float32, is 1.0: split_cell then hands the coordinate to the next cell with fraction 0.  Finite inputs only."""
    pos32 = np.asarray(pos32)
    assert pos32.dtype == np.float32 and M < (1 << 21)
    e = pos32.astype(np.float64) * float(M)
    assert np.isfinite(e).all()
    fl = np.floor(e)
    up = (e - fl).astype(np.float32) == np.float32(1.0)  # (e - fl is exact: e has at most 45 significant bits)
    return np.mod(fl.astype(np.int64) + up, M)


def floor_cells(pos32, M):
    """floor(double(x) * M) mod M: what a float64 floor says, which differs from `cells` just below a cell border."""
    return np.mod(np.floor(np.asarray(pos32).astype(np.float64) * float(M)).astype(np.int64), M)


def column_group(col, W):
    """csrc/common.h column_group: 0 if the window [col, col + W) ends by column 32, 2 if it starts at 32 or later, else 1."""
    return np.where(col + W <= 32, 0, np.where(col >= 32, 2, 1))


class PlanRef:
    """Entries of the reference plan: `index` (point), `tile` (plan bin), `group` (column group, zeros unless CG = 3) and
    `l1` (first-level bin: point set, pencil, segment of l1bins bins along axis 0), one per entry, ordered by (tile, group,
    index); `counts` per plan bin; `touched` tiles per point; `wraps`: the window crosses the torus seam (owned plans)."""

    def __init__(self, index, tile, group, l1, ntiles, touched, wraps):
        order = np.argsort((tile * 3 + group) * max(1, touched.size) + index, kind="stable")  # by (tile, group, index)
        self.index, self.tile, self.group, self.l1 = index[order], tile[order], group[order], l1[order]
        self.counts = np.bincount(self.tile, minlength=ntiles)
        self.offsets = np.concatenate(([0], np.cumsum(self.counts))).astype(np.int64)
        self.touched, self.wraps = touched, wraps

    def l1_counts(self, npencils):
        return np.bincount(self.l1, minlength=npencils)


def plan_ref(layout, pos32, batch, cell_fn=cells):
    """The reference plan of (pos32 [n, dim], batch [n] or None) for `layout`."""
    L = layout
    assert L.SB == 1, "sub-block plans (NFFT_HIP_SPREAD=reg) are not modelled"
    pos32 = np.asarray(pos32, dtype=np.float32).reshape(-1, L.dim)
    n = pos32.shape[0]
    c = cell_fn(pos32, L.M)
    zero = np.zeros(n, dtype=np.int64)
    c0 = c[:, 0] if L.dim == 3 else zero
    c1 = c[:, L.dim - 2] if L.dim >= 2 else zero
    c2 = c[:, L.dim - 1]
    b = zero if batch is None else np.asarray(batch, dtype=np.int64)
    k0 = c0 // L.bin0
    idx = np.arange(n, dtype=np.int64)
    if L.owned:
        a0, a1 = np.mod(c1 - L.m, L.M) // L.Ta1, np.mod(c1 + L.m + 1, L.M) // L.Ta1
        b0, b1 = np.mod(c2 - L.m, L.M) // L.Ta2, np.mod(c2 + L.m + 1, L.M) // L.Ta2
        pens = [(a0 * L.nta2 + b0, np.ones(n, dtype=bool)), (a0 * L.nta2 + b1, b1 != b0),
                (a1 * L.nta2 + b0, a1 != a0), (a1 * L.nta2 + b1, (a1 != a0) & (b1 != b0))]
        index = np.concatenate([idx[live] for _, live in pens])
        pencil = np.concatenate([pen[live] for pen, live in pens])
        touched = sum(live.astype(np.int64) for _, live in pens)
        wraps = (c1 - L.m < 0) | (c1 + L.m + 1 >= L.M) | (c2 - L.m < 0) | (c2 + L.m + 1 >= L.M)
        group = np.zeros(index.size, dtype=np.int64)
    else:
        j2 = c2 // L.Ta2
        index, pencil = idx, (c1 // L.Ta1) * L.nta2 + j2
        touched, wraps = np.ones(n, dtype=np.int64), np.zeros(n, dtype=bool)
        group = column_group(c2 - j2 * L.Ta2, L.W) if L.CG == 3 else zero
    tile = b[index] * L.tiles_per_batch + pencil * L.np0 + k0[index]
    l1 = (b[index] * (L.nta1 * L.nta2) + pencil) * L.l1seg + k0[index] // L.l1bins
    return PlanRef(index, tile, group, l1, L.ntiles, touched, wraps)


def cut_tables(layout, buf):
    """The tables of one plan out of the plan buffer `buf` (uint8 numpy array): offsets [ntiles + 1], index [cap], coords
    [cap, dim] (float32), groups [ntiles, 2] or None, and the word at the start of the cursors (the second level's route)."""
    L = layout
    buf = np.ascontiguousarray(buf[L.off_own:])

    def words(off, count, dtype=np.int32):
        return buf[off: off + 4 * count].view(dtype)
    offsets = words(L.off_offsets, L.ntiles + 1)
    if L.dim == 3:
        rec = words(L.off_spos, L.cap * 4, np.float32).reshape(L.cap, 4)
        index, coords = np.ascontiguousarray(rec[:, 3]).view(np.int32), np.ascontiguousarray(rec[:, :3])
    else:
        index = words(L.off_perm, L.cap)
        coords = words(L.off_spos, L.cap * L.dim, np.float32).reshape(L.cap, L.dim)
    groups = words(L.off_groups, L.ntiles * 2).reshape(L.ntiles, 2) if L.grouped else None
    return dict(offsets=offsets, index=index, coords=coords, groups=groups, route=int(words(L.off_cursor, 1)[0]))


def build_tables(layout, ref, pos32):
    """A correct plan made on the CPU from the reference: the tables `cut_tables` would return."""
    L = layout
    pos32 = np.asarray(pos32, dtype=np.float32).reshape(-1, L.dim)
    entries = ref.index.size
    index = np.zeros(L.cap, dtype=np.int32)
    coords = np.zeros((L.cap, L.dim), dtype=np.float32)
    index[:entries] = ref.index
    coords[:entries] = pos32[ref.index]
    groups = None
    if L.grouped:
        g0 = np.bincount(ref.tile[ref.group == 0], minlength=L.ntiles)
        g1 = np.bincount(ref.tile[ref.group == 1], minlength=L.ntiles)
        groups = np.stack([ref.offsets[:-1] + g0, ref.offsets[:-1] + g0 + g1], axis=1).astype(np.int32)
    return dict(offsets=ref.offsets.astype(np.int32), index=index, coords=coords, groups=groups, route=0)


def _fail(what, *args):
    raise PlanError(what % args)


def check_plan(layout, tables, pos32, batch, ref=None):
    """Asserts, exactly: the offsets are the exclusive prefix sum of the reference counts (all ntiles + 1 of them, the last one
    the entry count, within cap); every bin holds the reference's multiset of point indices (scatter plans: every point
    once; owned plans: once per touched tile and nowhere else); every record's coordinates are bit-equal to pos[index]; and
    for grouped plans both group words of every bin are the reference's, with every entry between two boundaries in that
    group.  Nothing about the order inside a (bin, group).  Returns the reference."""
    L = layout
    pos32 = np.asarray(pos32, dtype=np.float32).reshape(-1, L.dim)
    n = pos32.shape[0]
    ref = ref if ref is not None else plan_ref(L, pos32, batch)
    offsets = np.asarray(tables["offsets"]).astype(np.int64)
    if offsets.shape != (L.ntiles + 1,):
        _fail("offsets table has %d entries, the plan %d bins", offsets.size, L.ntiles)
    bad = np.flatnonzero(offsets != ref.offsets)
    if bad.size:
        t = int(bad[0])
        _fail("offsets[%d] = %d, reference %d (%d of %d entries differ; bin %d holds %d points in the reference)",
              t, offsets[t], ref.offsets[t], bad.size, offsets.size, min(t, L.ntiles - 1), ref.counts[min(t, L.ntiles - 1)])
    entries = int(offsets[-1])
    if entries != ref.index.size or entries > L.cap:
        _fail("offsets[-1] = %d, reference entries %d, cap %d", entries, ref.index.size, L.cap)
    index = np.asarray(tables["index"])[:entries].astype(np.int64)
    bad = np.flatnonzero((index < 0) | (index >= n))
    if bad.size:
        _fail("record %d has index %d outside [0, %d)", bad[0], index[bad[0]], n)
    slot_bin = np.repeat(np.arange(L.ntiles, dtype=np.int64), ref.counts)
    got_keys, ref_keys = np.sort(slot_bin * max(1, n) + index), np.sort(ref.tile * max(1, n) + ref.index)  # (bin, index)
    bad = np.flatnonzero(got_keys != ref_keys)
    if bad.size:
        s = int(bad[0])
        _fail("bin %d holds point %d, the reference has point %d in bin %d there; %d sorted (bin, point) pairs differ",
              got_keys[s] // max(1, n), got_keys[s] % max(1, n), ref_keys[s] % max(1, n), ref_keys[s] // max(1, n), bad.size)
    if not L.owned and np.bincount(index, minlength=n).max(initial=0) > 1:
        _fail("a point appears twice")
    got = np.ascontiguousarray(np.asarray(tables["coords"], dtype=np.float32)[:entries]).view(np.int32)
    bad = np.flatnonzero((got != np.ascontiguousarray(pos32[index]).view(np.int32)).any(axis=1))
    if bad.size:
        s = int(bad[0])
        _fail("record %d (bin %d, index %d) holds coordinates %r, the point has %r", s, slot_bin[s], index[s],
              tables["coords"][s].tolist(), pos32[index[s]].tolist())
    if L.grouped:
        groups = np.asarray(tables["groups"]).astype(np.int64).reshape(L.ntiles, 2)
        want = build_tables(L, ref, pos32)["groups"]
        bad = np.argwhere(groups != want)
        if bad.size:
            t, w = (int(v) for v in bad[0])
            _fail("groups[%d][%d] = %d, reference %d", t, w, groups[t, w], want[t, w])
        slots = np.arange(entries, dtype=np.int64)
        here = (slots >= groups[slot_bin, 0]).astype(np.int64) + (slots >= groups[slot_bin, 1])
        point_group = np.zeros(n, dtype=np.int64)
        point_group[ref.index] = ref.group  # (scatter plan: one entry per point)
        bad = np.flatnonzero(here != point_group[index])
        if bad.size:
            s = int(bad[0])
            _fail("record %d (bin %d, index %d) lies in group %d, its point belongs to group %d", s, slot_bin[s], index[s],
                  here[s], point_group[index[s]])
    return ref


def local_scan_threads(npencils):
    """G of sort1_scatter_kernel's in-kernel scan: threads per first-level bin, a power of two with 2 G bins <= 512, at most 64."""
    G = 1
    while 2 * G * npencils <= 512 and G < 64:
        G *= 2
    return G


FUSE_CAP = 16384  # records of a first-level bin the one-pass second level holds (binning.hip kFuseCap)


def facts(layout, ref, n):
    """What class a case falls into, from the layout entry and the reference counts alone."""
    L = layout
    f = dict(wide=L.wide, owned=L.owned, CG=L.CG, two_level=L.two_level, one_level=L.one_level, local_scan=L.local_scan,
             fuse=L.fuse, scan=L.scan, scan_items=L.scan_items, l1bins=L.l1bins, l1seg=L.l1seg, npencils=L.npencils,
             partial_segment=L.np0 % L.l1bins != 0, block_points=L.block_points, nblocks=L.nblocks,
             last_slice=n - (L.nblocks - 1) * L.block_points if n else 0, entries=int(ref.index.size),
             G=local_scan_threads(L.npencils) if L.local_scan else None)
    second = L.two_level and not L.one_level
    l1 = ref.l1_counts(L.npencils) if L.two_level else np.zeros(1, dtype=np.int64)
    f["max_l1"] = int(l1.max(initial=0))
    f["l1_sizes"] = set(int(v) for v in l1)
    f["l1_first_last_empty"] = bool(l1[0] == 0 and l1[-1] == 0)
    # the word sort2_route_kernel leaves at the start of the cursors: 1 when every first-level bin fits the one-pass kernel
    f["route"] = (1 if f["max_l1"] <= FUSE_CAP else 0) if second and L.fuse else None
    f["touch"] = tuple(int((ref.touched == k).sum()) for k in (1, 2, 4))
    f["wrapping"] = int(ref.wraps.sum())
    return f
