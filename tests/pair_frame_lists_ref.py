"""Exclusion lists laid over the counted layouts of tests/pair_frame_ref.py, so that a listed pair sits on a chosen edge of
the pair kernels' frame and of the list's own search -- TEST INFRASTRUCTURE ONLY, plain NumPy.

``listed_pairs(L, A, r_c, rng)`` returns ``(pairs [m, 2], sc [m], sl [m], classes)``: pairs of caller-order indices, each once,
never across two point sets, with the Coulomb and the Lennard-Jones scale of each, and a dict of named classes, each an int64
array of indices into ``pairs``.  A pair may sit in several classes.  The pairs picked for a class are near neighbours: at most
NEAR = 2 lattice spacings (pair_frame_ref.cartesian_spacing) apart in the box's metric, so that losing one changes the force
on its ends visibly.  Four exceptions: ``beyond`` and ``duplicate`` by their definition; a long row takes its entries from
within ROW_REACH = 3 spacings, where 33 neighbours are; and a point on a face or given outside the box whose own cell, or the
cell across the face, is a sparse one takes its nearest neighbour, less than 0.9 r_c away.  The layouts' own separation
stands: no point is moved.

Classes (pair_frame_ref.pair_streams and point_groups say where a pair is computed):
  ``tile0, tile1, tile2``  in at least one direction the partner is staged in the first, second, third LDS tile of its range
  ``second_wave``          both ends are computed by lanes of their items' second waves
  ``last_item``            an end is in the partly idle last item of a cut cell
  ``set2``                 the pair lies in the point set behind the empty one (ragged3)
  ``wrap``                 the image goes through a face between the cells c_a = 0 and c_a = G_a - 1, one pair per axis at least
  ``face``                 the points exactly on -1/2 and at the largest float32 below 1/2, each with a neighbour across the face
  ``moved``                an end is given one box to the right, or two boxes to the left, of where it acts
  ``duplicate``            the exact duplicate pair (r = 0) at (0, 0); the rows of its two points hold each other only
  ``beyond``               one pair per point set farther apart than r_c, at (1/2, 1/4)
  ``trip2, straddle``      both ends, or exactly one, have an in-set rank of list_blocks(n, B) * 256 or more: the list kernel's
                           second trip of its strided loop (empty where a point set is no larger than that)
  ``row1 .. row33``        per ROW_LENGTHS: a point of a crowded cell (255 points or more) whose row holds exactly that many
                           entries -- its nearest neighbours -- with the scales ROW_SCALES in turn along the row, so that a hit
                           on the wrong entry takes another weight.  All entries are inside r_c, so the first, the last and a
                           middle entry are hits of the walk; an unlisted neighbour inside r_c with an index strictly between
                           the row's first and last column (a miss after a full search) exists for every row of two or more
  ``s(0,0) .. s(1,1)``     per SCALES, every pair with exactly these scales, PER_SCALE of them picked for the class; the four
                           ONE_ZERO classes have exactly one scale equal to zero; (1, 1) is listed with both weights zero

``row_report`` restates the rows of a list, ``unlisted_change`` is the tooth of a class: what the float64 masked walk
(lj_excl_ref.near_step_scaled) loses on the class's ends when its pairs are un-listed, or listed with other scales.
"""
import numpy as np

import dispersion_ref as dr
import lj_excl_ref as le
import pair_frame_ref as pf

ROW_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33)
SCALES = {"s(0,0)": (0.0, 0.0), "s(1/1.2,1/2)": le.AMBER_14, "s(0,1/2)": (0.0, 0.5), "s(1/2,0)": (0.5, 0.0),
          "s(0,1)": (0.0, 1.0), "s(1,0)": (1.0, 0.0), "s(1,1)": (1.0, 1.0)}
ONE_ZERO = ("s(0,1/2)", "s(1/2,0)", "s(0,1)", "s(1,0)")
EDGE_SCALES = ((0.0, 0.0), le.AMBER_14, (0.5, 0.25))
ROW_SCALES = EDGE_SCALES + ((0.25, 0.75),)
BEYOND_SCALES = (0.5, 0.25)
LIST_BLOCK, LIST_BLOCKS = 256, 1024  # kListBlock and kListBlocks of csrc/ewald_lj_excl.hip
NEAR = 2.0       # lattice spacings
ROW_REACH = 3.0  # ... within which a long row finds its 33 entries
PER_CLASS = 8    # pairs picked for an edge class, per point set
PER_SCALE = 6    # ... for a scale class
CROWDED = 255    # points in a cell that holds the centre of a long row
NO_TEETH = ("duplicate", "beyond", "s(1,1)")  # classes whose pairs add nothing to the walk's sums, listed or not


def list_blocks(n, B):
    """list_blocks() of csrc/ewald_lj_excl.hip: workgroups per point set, one per 256 points of an average set"""
    per_set = -(-n // B)
    return max(1, min(-(-per_set // LIST_BLOCK), LIST_BLOCKS))


def _separations(s, A, rows):
    """r [len(rows), n] of the minimum images in the box A, float64 on the float32 positions"""
    s64 = np.asarray(s, dtype=np.float64)
    ds = s64[rows][:, None, :] - s64[None, :, :]
    d = (ds - np.rint(ds)) @ dr._box(A)
    return np.sqrt((d * d).sum(-1))


def _near_pairs(s, A, reach):
    """(i, j, r) of every pair i < j of the point set s no farther apart than `reach`, r = 0 included"""
    out = []
    for r0 in range(0, s.shape[0], 512):
        r = _separations(s, A, np.arange(r0, min(r0 + 512, s.shape[0])))
        ii, jj = np.nonzero(r <= reach)
        keep = ii + r0 < jj
        out.append((ii[keep] + r0, jj[keep], r[ii[keep], jj[keep]]))
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def pair_separation(L, A, pairs):
    """r [m] of the listed images: lj_excl_ref's d_ij = (ds - rint(ds)) A on the float32 positions"""
    s64 = L.points.astype(np.float64)
    ds = s64[pairs[:, 0]] - s64[pairs[:, 1]]
    d = (ds - np.rint(ds)) @ dr._box(A)
    return np.sqrt((d * d).sum(-1))


def _geometry(L, pairs):
    """per pair, where the walk computes it: a dict of bool [m] -- tile0, tile1, tile2, second_wave, last_item, wrap, moved"""
    st = pf.pair_streams(L.points, L.batch, L.cells, pairs)
    second, last = pf.point_groups(L.points, L.batch, L.cells)
    i, j = pairs[:, 0], pairs[:, 1]
    red = pf._reduce(L.points).astype(np.float64)
    cross = np.rint(red[i] - red[j]) != 0  # [m, 3]: the image goes through the face of this axis
    key = pf.cell_of(L.points, L.cells)
    wrap, stride = np.zeros(len(pairs), bool), 1
    for a in range(3):
        ca = (key // stride) % L.cells[a]
        wrap |= cross[:, a] & (np.minimum(ca[i], ca[j]) == 0) & (np.maximum(ca[i], ca[j]) == L.cells[a] - 1)
        stride *= L.cells[a]
    moved = (L.points > 0.5).all(1) | (L.points < -1.5).all(1)
    return {"tile0": (st["tile"] == 0).any(1), "tile1": (st["tile"] == 1).any(1), "tile2": (st["tile"] == 2).any(1),
            "second_wave": second[i] & second[j], "last_item": last[i] | last[j], "wrap": wrap, "moved": moved[i] | moved[j],
            "cross": cross}


def listed_pairs(L, A, r_c, rng):
    """(pairs, sc, sl, classes) over the layout L in the box A (None: the unit cube): see the module's docstring.  Asserted
    here: every class holds what it is named for, no pair spans two point sets or is within 1e-4 r_c of r_c, the rows have
    their lengths and their misses."""
    h = pf.cartesian_spacing(L.cells, A)
    assert ROW_REACH * h < r_c
    below = np.nextafter(np.float32(0.5), np.float32(0))
    red = pf._reduce(L.points)
    key = pf.cell_of(L.points, L.cells)
    K = int(np.prod(L.cells))
    set_of = L.set_of()
    counts = np.bincount(key + set_of * K, minlength=L.B * K)
    second_trip = list_blocks(L.n, L.B) * LIST_BLOCK
    pairs, sc, sl, origin = [], [], [], []

    def add(i, j, scales, name):
        if rng.random() < 0.5:  # (either order)
            i, j = j, i
        pairs.append((int(i), int(j)))
        sc.append(scales[0])
        sl.append(scales[1])
        origin.append(name)

    for b in sorted(L.counts):
        sel = np.flatnonzero(set_of == b)  # (ascending and contiguous: the point-set vector is sorted)
        pts = L.points[sel]
        ci, cj, cr = _near_pairs(pts, A, ROW_REACH * h)
        ci, cj = sel[ci], sel[cj]
        geo = _geometry(L, np.stack([ci, cj], 1))
        rank_i, rank_j = ci - sel[0], cj - sel[0]
        geo["trip2"] = (rank_i >= second_trip) & (rank_j >= second_trip)
        geo["straddle"] = (rank_i >= second_trip) != (rank_j >= second_trip)
        apart = cr > 0
        close = apart & (cr <= NEAR * h)
        used = set()
        by_point = {}
        for t in np.argsort(cr, kind="stable"):  # per point, its candidates by distance
            by_point.setdefault(int(ci[t]), []).append(int(t))
            by_point.setdefault(int(cj[t]), []).append(int(t))

        def other(t, p):
            return int(cj[t]) if int(ci[t]) == p else int(ci[t])

        def pick(mask, count, scales, name):
            got = 0
            for t in rng.permutation(np.flatnonzero(mask & close)):
                i, j = int(ci[t]), int(cj[t])
                if i in used or j in used:
                    continue
                used.update((i, j))
                add(i, j, scales[got % len(scales)], name)
                got += 1
                if got == count:
                    break
            assert got == count, (L.name, b, name, got)

        def nearest(p, name, scales, across=None):
            """the point p with its nearest unused neighbour (across the face of the axis `across`)"""
            for t in by_point.get(p, []):
                o = other(t, p)
                if close[t] and o not in used and (across is None or geo["cross"][t, across]):
                    used.update((p, o))
                    add(p, o, scales, name)
                    return
            # (the point, or the cell across its face, may lie in a sparse cell: then the nearest such point, well inside r_c)
            r = _separations(L.points[sel], A, [p - sel[0]])[0]
            through = np.ones(sel.size, bool)
            if across is not None:
                through = np.rint(red[p].astype(np.float64) - red[sel].astype(np.float64))[:, across] != 0
            for o in sel[np.argsort(r, kind="stable")]:
                o = int(o)
                if through[o - sel[0]] and o not in used and 0 < r[o - sel[0]] < 0.9 * r_c:
                    used.update((p, o))
                    add(p, o, scales, name)
                    return
            raise AssertionError((L.name, b, name, p))

        # the duplicate pair: its two points stay out of everything else
        t = np.flatnonzero(~apart)
        assert t.size == 1
        used.update((int(ci[t[0]]), int(cj[t[0]])))
        add(ci[t[0]], cj[t[0]], (0.0, 0.0), "duplicate")
        # the points on the faces, each with a neighbour across its face (none of them, or of those given outside, is a partner)
        on_face = (red[sel] == np.float32(-0.5)) | (red[sel] == below)
        used.update(int(p) for p in sel[on_face.any(1) | (pts > 0.5).all(1) | (pts < -1.5).all(1)])
        for a in range(3):
            for value in (np.float32(-0.5), below):
                p = sel[np.flatnonzero(red[sel, a] == value)]
                assert p.size == 1
                nearest(int(p[0]), "face", EDGE_SCALES[a], across=a)
        # points given outside the box
        for outside in ((L.points[sel] > 0.5).all(1), (L.points[sel] < -1.5).all(1)):
            given = sel[np.flatnonzero(outside)]
            assert given.size == 4
            for k, p in enumerate(given[:2]):
                nearest(int(p), "moved", EDGE_SCALES[k])
        for a in range(3):
            pick(geo["wrap"] & geo["cross"][:, a], 1, EDGE_SCALES[a:], "wrap")
        # the rows: a centre in a crowded cell and its nearest unused neighbours
        crowded = sel[counts[key[sel] + b * K] >= CROWDED]
        for length in ROW_LENGTHS:
            for p in rng.permutation(crowded):
                p = int(p)
                if p in used:
                    continue
                partners = []
                for t in by_point.get(p, []):
                    o = other(t, p)
                    if cr[t] > 0 and o not in used and o not in partners:
                        partners.append(o)
                    if len(partners) == length:
                        break
                if len(partners) < length:
                    continue
                row = sorted(partners)
                if length >= 2:  # a miss after a full search: an unlisted neighbour inside r_c strictly between lo and hi
                    r = _separations(L.points[sel], A, [p - sel[0]])[0]
                    inside = sel[(r > 0) & (r < r_c)]
                    if not ((inside > row[0]) & (inside < row[-1]) & ~np.isin(inside, row)).any():
                        continue
                used.add(p)
                used.update(row)
                for k, o in enumerate(row):
                    add(p, o, ROW_SCALES[k % len(ROW_SCALES)], "row%d" % length)
                break
            else:
                raise AssertionError((L.name, b, "no centre for a row of", length))
        for name in ("tile2", "tile1", "last_item", "second_wave"):
            pick(geo[name], PER_CLASS, EDGE_SCALES, name)
        if sel.size > second_trip:
            pick(geo["trip2"], PER_CLASS, EDGE_SCALES, "trip2")
            pick(geo["straddle"], PER_CLASS // 2, EDGE_SCALES, "straddle")
        pick((geo["tile0"] & ~geo["tile1"] & ~geo["tile2"]), PER_CLASS, EDGE_SCALES, "tile0")
        for name, scales in SCALES.items():
            pick(cr <= 1.5 * h, PER_SCALE, (scales,), name)
        # one pair beyond the cut
        for p in rng.permutation(sel):
            p = int(p)
            if p in used:
                continue
            r = _separations(L.points[sel], A, [p - sel[0]])[0]
            far = [int(o) for o in sel[(r > 1.1 * r_c) & (r < 1.4 * r_c)] if int(o) not in used]
            if far:
                used.update((p, far[0]))
                add(p, far[0], BEYOND_SCALES, "beyond")
                break
        else:
            raise AssertionError((L.name, b, "beyond"))

    pairs, sc, sl, origin = np.array(pairs, dtype=np.int64), np.array(sc), np.array(sl), np.array(origin)
    m = pairs.shape[0]
    assert (set_of[pairs[:, 0]] == set_of[pairs[:, 1]]).all()
    r = pair_separation(L, A, pairs)
    assert np.abs(r - r_c).min() > 1e-4 * r_c
    # the classes: what a pair was picked for, and every other class whose condition it meets
    geo = _geometry(L, pairs)
    teeth = ~np.isin(origin, NO_TEETH)
    rank = pairs - np.searchsorted(set_of, set_of[pairs[:, 0]])[:, None]
    classes = {name: np.flatnonzero(geo[name] & teeth) for name in ("tile0", "tile1", "tile2", "second_wave", "last_item", "wrap", "moved")}
    if L.B > 1:
        classes["set2"] = np.flatnonzero((set_of[pairs[:, 0]] == 2) & teeth)
    for name in ("face", "duplicate", "beyond"):
        classes[name] = np.flatnonzero(origin == name)
    classes["trip2"] = np.flatnonzero((rank >= second_trip).all(1) & teeth)
    classes["straddle"] = np.flatnonzero(((rank >= second_trip).sum(1) == 1) & teeth)
    for length in ROW_LENGTHS:
        classes["row%d" % length] = np.flatnonzero(origin == "row%d" % length)
    for name, scales in SCALES.items():
        classes[name] = np.flatnonzero((sc == scales[0]) & (sl == scales[1]) & (r > 0) & (r < r_c))
    sets = len(L.counts)
    for name in ("tile0", "tile1", "tile2", "second_wave", "last_item"):
        assert classes[name].size >= PER_CLASS * sets, (name, classes[name].size)
    assert classes["wrap"].size >= 3 * sets and geo["cross"][classes["wrap"]].any(0).all()
    assert classes["face"].size == 6 * sets and geo["wrap"][classes["face"]].all()
    assert classes["moved"].size >= 4 * sets and classes["duplicate"].size == sets and classes["beyond"].size == sets
    assert not r[classes["duplicate"]].any() and (r[classes["beyond"]] > r_c).all()
    assert (np.delete(r, classes["beyond"]) < r_c).all()
    near = np.ones(m, bool)
    near[np.concatenate([classes["duplicate"], classes["beyond"]])] = False
    assert r[near].min() >= 0.8 * h and r[near].max() < 0.9 * r_c
    near[np.isin(origin, ("face", "moved"))] = False
    assert r[near].max() <= ROW_REACH * h
    near[np.char.startswith(origin, "row")] = False
    assert r[near].max() <= NEAR * h
    for name in SCALES:
        assert classes[name].size >= 4 * sets
    report = row_report(L, A, r_c, pairs, classes)
    for length in ROW_LENGTHS:
        assert len(report[length]) == sets and all(row["inside"] and (length < 2 or row["misses"] >= 1) for row in report[length])
    return pairs, sc, sl, classes


def ends(pairs, which):
    """the points of the pairs `which`, ascending"""
    return np.unique(pairs[which])


def row_report(L, A, r_c, pairs, classes):
    """{length: [a dict per row of that length class]}: the centre `point`, its ascending `row` of columns (over the WHOLE
    list, not the class alone), `first`, `last`, `middle` (the columns hit at those entries), `inside` (every column is
    inside r_c, so each is a hit of the walk) and `misses`, the number of unlisted neighbours inside r_c whose index lies
    strictly between the row's first and last column"""
    rows = {}
    for i, j in pairs:
        rows.setdefault(int(i), []).append(int(j))
        rows.setdefault(int(j), []).append(int(i))
    set_of = L.set_of()
    out = {}
    for length in ROW_LENGTHS:
        which = classes["row%d" % length]
        out[length] = []
        points, times = np.unique(pairs[which], return_counts=True)
        centres = points[times == length] if length > 1 else pairs[which][:, 0]
        for p in centres:
            row = sorted(rows[int(p)])
            assert len(row) == length, (length, p, row)
            sel = np.flatnonzero(set_of == set_of[p])
            r = _separations(L.points[sel], A, [int(p) - sel[0]])[0]
            inside = sel[(r > 0) & (r < r_c)]
            misses = int(((inside > row[0]) & (inside < row[-1]) & ~np.isin(inside, row)).sum())
            out[length].append({"point": int(p), "row": row, "first": row[0], "last": row[-1], "middle": row[length // 2],
                                "inside": bool(np.isin(row, inside).all()), "misses": misses, "neighbours": int(inside.size)})
    return out


def row_lengths(pairs, n):
    """entries per row of the symmetrised list"""
    return np.bincount(np.asarray(pairs).ravel(), minlength=n)


def unlisted_change(L, A, x, split, pairs, sc, sl, which, instead=None):
    """(the ends of the pairs `which`, dF [ends, 3]): the force of lj_excl_ref.near_step_scaled with these pairs listed at their
    scales minus the force with them un-listed -- or, with `instead` = (s^C, s^L), listed at those scales.  The walk's sums are
    sums of pair terms and only these pairs' terms change, so the change is that of the sub-system of their ends alone, and is
    taken there.  x [n, 3] holds (q, c, a); split = (alpha_C, alpha_D, r_c)."""
    e = ends(pairs, which)
    local = np.searchsorted(e, pairs[which])
    batch = None if L.batch is None else L.batch[e]
    q, c, a = x[e].T
    args = (q, c, a, L.points[e], dr._box(A), batch)
    f1, _ = le.near_step_scaled(*args, local, sc[which], sl[which], *split)
    if instead is None:
        f0, _ = le.near_step_scaled(*args, np.zeros((0, 2), np.int64), 0.0, 0.0, *split)
    else:
        f0, _ = le.near_step_scaled(*args, local, instead[0], instead[1], *split)
    return e, f1 - f0


def per_set(step, L, pairs, *lists):
    """(f [n, 3], eight [B, 8]) of a brute-force step of lj_excl_ref or lj_table_ref evaluated point set by point set (its n x n
    scale matrices stay small; pairs never span two sets): step(sel, local pairs, *lists of those pairs) -> (f, eight [1, 8])"""
    f, eight = np.zeros((L.n, 3)), np.zeros((L.B, 8))
    set_of = L.set_of()
    for b in sorted(L.counts):
        sel = np.flatnonzero(set_of == b)
        mine = np.flatnonzero(set_of[pairs[:, 0]] == b) if len(pairs) else np.zeros(0, np.int64)
        fb, eb = step(sel, pairs[mine] - sel[0], *(v[mine] for v in lists))
        f[sel], eight[b] = fb, eb[0]
    return f, eight
