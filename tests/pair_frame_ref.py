"""The frame of the pair kernels (csrc/pair_frame.h) restated in plain Python, and point sets with a
chosen number of points in every cell -- TEST INFRASTRUCTURE ONLY.

The frame's edges are set by kNearBlock = 128 (output points per work item), kNearTile = 256 (streamed points per LDS tile)
and the 64-lane wave.  A point set reaches an edge only through how many points its cells hold, so the fixtures here are
built from the counts:

``cell_of``          the cell of every point: the binning of the host layer (``torus_reduce`` and ``cell_order`` of
                     csrc/core.cpp, in float32 as there), restated
``counted_points``   float32 fractional points, exactly ``counts[k]`` of them in cell ``k``, on a jittered lattice with a stated
                     minimum separation, a handful of the wrap's edge cases among them, shuffled
``frame_geometry``   what ``launch_nearfield_items`` and ``WrappedWalk`` make of a point set: the work items as (cell, first,
                     live lanes) and, per item, the lengths of the ranges that it sweeps
``point_groups``     per point, which edge of the frame computes it: the second wave of an item, the last and partly idle item
                     of a cut cell
``pair_streams``     per pair of points and per direction: the item that computes one end, the range of its walk that holds the
                     other, and the LDS tile in which that one is staged (tests/pair_frame_lists_ref.py)
``LAYOUTS``          the three layouts of tests/test_gpu_pair_frame_edges.py, whose coverage tests/test_pair_frame_ref.py asserts

What the walk does on a G0 = 3 grid: the items of the cells c0 = 0 and c0 = 2 sweep every row in two ranges (one cell, then
two), those of c0 = 1 sweep the whole row as one; single cells are swept as ranges only at c0 = 0 and c0 = G0 - 1.
"""
import numpy as np

import dispersion_ref as dr

NEAR_BLOCK, NEAR_TILE, WAVE = 128, 256, 64
NODES = 7        # sub-lattice nodes per axis and cell: up to 343 points per cell
JITTER = 0.08    # of the sub-lattice spacing, per coordinate


def _reduce(points):
    """p modulo 1 in [-1/2, 1/2), in float32: p - rint(p), and what comes out as +1/2 is the point -1/2"""
    p = np.asarray(points, dtype=np.float32)
    red = p - np.rint(p)
    return np.where(red >= np.float32(0.5), red - np.float32(1.0), red).astype(np.float32)


def cell_of(points, cells):
    """c0 + G0 (c1 + G1 c2) with c_a = floor((p_a + 1/2) G_a) clamped to [0, G_a - 1], float32 arithmetic: [n] int64"""
    red = _reduce(points)
    key, stride = np.zeros(red.shape[0], np.int64), 1
    for a in range(3):
        c = np.floor((red[:, a] + np.float32(0.5)) * np.float32(cells[a]))
        key += np.clip(c, 0, cells[a] - 1).astype(np.int64) * stride
        stride *= cells[a]
    return key


def spacing(cells):
    """the sub-lattice spacing per axis, fractional"""
    return 1.0 / (NODES * np.asarray(cells, dtype=np.float64))


def d_min_fractional(cells):
    """no two distinct points of counted_points are closer than this in fractional terms, through the wrap: two nodes differ
    by a whole spacing on some axis, and each is moved by JITTER of it at most"""
    return (1.0 - 2.0 * JITTER) * spacing(cells).min()


def cartesian_spacing(cells, A=None):
    """the smallest distance of two neighbouring nodes of the lattice before the jitter, in the box A"""
    h, A = spacing(cells), dr._box(A)
    e = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)], dtype=np.float64)
    return float(np.linalg.norm((e * h) @ A, axis=1).min())


def counted_points(rng, cells, counts, edge_cases=True):
    """float32 fractional points [sum(counts), 3] in [-1/2, 1/2)^3 (but for those given outside on purpose), counts[k] of
    them in cell k = c0 + G0 (c1 + G1 c2) of the grid `cells`, shuffled.

    The points are nodes of the lattice of NODES G_a nodes per axis -- NODES^3 per cell, half a spacing clear of the cell's
    faces -- each coordinate moved by at most JITTER of the spacing: no node leaves its cell, and no two are closer than
    d_min_fractional(cells), through the wrap too.  The edge cases of the wrap are written over chosen nodes, so they change
    no cell's count:
      * per axis, a point exactly on the lower face -1/2 and one at the largest float32 below 1/2 (its cell index is clamped);
        the node that faces either through the wrap is left out, so the separation holds;
      * four points given one box to the right and four given two boxes to the left of where they act;
      * one exact duplicate pair (r = 0, skipped by every kernel): the second point takes a node's place in the count.
    """
    G = np.asarray(cells, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    K = int(G.prod())
    assert counts.shape == (K,) and counts.min() >= 0 and counts.max() <= NODES ** 3 - 8
    h = spacing(cells)
    coords = np.array([(k % G[0], (k // G[0]) % G[1], k // (G[0] * G[1])) for k in range(K)])
    nodes = np.array([(i, j, l) for i in range(NODES) for j in range(NODES) for l in range(NODES)])

    must, forbidden, special = {}, set(), []  # cell -> [node index]; (global node); (kind, axis, cell, node)
    if edge_cases:
        used = set()  # the global nodes of the hosts

        def host(pred_cell, pred_node, facing=None):
            """a (cell, node) not used before, in a cell that keeps a point to spare; facing(g): the node to leave out"""
            for k in rng.permutation(K):
                if not pred_cell(coords[k]) or len(must.get(k, [])) + 2 > counts[k]:
                    continue
                for m in rng.permutation(NODES ** 3):
                    g = tuple(int(v) for v in coords[k] * NODES + nodes[m])
                    if not pred_node(nodes[m]) or g in forbidden or g in used or (facing and facing(g) in used):
                        continue
                    must.setdefault(k, []).append(m)
                    used.add(g)
                    if facing:
                        forbidden.add(facing(g))
                    return k, m
            raise AssertionError("no cell has room for an edge case")

        def facing_through(a, step):
            return lambda g: tuple((g[b] + (step if b == a else 0)) % (NODES * int(G[b])) for b in range(3))

        for a in range(3):
            for kind, c_a, i_a, step in (("lower", 0, 0, -1), ("below", G[a] - 1, NODES - 1, 1)):
                k, m = host(lambda c: c[a] == c_a, lambda nd: nd[a] == i_a, facing_through(a, step))
                special.append((kind, a, k, m))
        for kind in ("right",) * 4 + ("left",) * 4 + ("duplicate",):
            k, m = host(lambda c: True, lambda nd: True)
            special.append((kind, None, k, m))

    chosen = {}
    for k in range(K):
        fixed = list(must.get(k, []))
        ndup = sum(1 for kind, _, kk, _ in special if kind == "duplicate" and kk == k)
        free = [m for m in range(NODES ** 3) if m not in fixed and tuple(coords[k] * NODES + nodes[m]) not in forbidden]
        take = fixed + list(rng.permutation(free)[:counts[k] - len(fixed) - ndup])
        assert len(take) == counts[k] - ndup
        chosen[k] = take
    out = {}
    for k in range(K):
        n = coords[k][None, :] * NODES + nodes[chosen[k]]  # global node indices [m, 3]
        x = -0.5 + (n + 0.5) * h + (rng.random(n.shape) * 2.0 - 1.0) * JITTER * h
        out[k] = x.astype(np.float32)
    below = np.nextafter(np.float32(0.5), np.float32(0))  # the largest float32 below 1/2
    extra = []
    for kind, a, k, m in special:
        row = chosen[k].index(m)
        if kind == "lower":
            out[k][row, a] = -0.5
        elif kind == "below":
            out[k][row, a] = below
        elif kind == "right":
            out[k][row] += np.float32(1.0)
        elif kind == "left":
            out[k][row] -= np.float32(2.0)
        else:
            extra.append(out[k][row].copy())
    pts = np.concatenate([out[k] for k in range(K)] + ([np.array(extra, dtype=np.float32)] if extra else []))
    pts = pts[rng.permutation(pts.shape[0])].astype(np.float32)
    assert (np.bincount(cell_of(pts, cells), minlength=K) == counts).all()
    return pts


def _sorted(points, batch, cells):
    """(key per point, the order of the stable sort by (point set, cell), the start table over B prod(G) cells)"""
    K = int(np.prod(cells))
    key = cell_of(points, cells)
    B = 1
    if batch is not None:
        batch = np.asarray(batch, dtype=np.int64)
        B = int(batch.max()) + 1 if batch.size else 1
        key = key + batch * K
    order = np.argsort(key, kind="stable")
    start = np.searchsorted(key[order], np.arange(B * K + 1))
    return key, order, start


def _walk(k, start, G0, G1, G2, bounds=False):
    """WrappedWalk of the cell k (counted over all point sets): the lengths of the ranges [first, last) that it hands on;
    with `bounds` the ranges themselves, [m, 2] int64 of (first, last) in the cell order"""
    c0, c1, c2 = k % G0, (k // G0) % G1, (k // (G0 * G1)) % G2
    set0 = k - (c2 * G1 + c1) * G0 - c0  # first cell of the point set
    split = c0 == 0 or c0 == G0 - 1
    lo0 = G0 - 1 if c0 == 0 else (0 if c0 == G0 - 1 else c0 - 1)
    hi0 = G0 if c0 == 0 else (1 if c0 == G0 - 1 else c0 + 2)
    lo1, hi1 = (0, 2) if c0 == 0 else (G0 - 2, G0)
    swept = []
    for d2 in (-1, 0, 1):
        w2 = G2 - 1 if c2 + d2 < 0 else (0 if c2 + d2 >= G2 else c2 + d2)
        for d1 in (-1, 0, 1):
            w1 = G1 - 1 if c1 + d1 < 0 else (0 if c1 + d1 >= G1 else c1 + d1)
            row = set0 + (w2 * G1 + w1) * G0
            swept.append((int(start[row + lo0]), int(start[row + hi0])))
            if split:
                swept.append((int(start[row + lo1]), int(start[row + hi1])))
    swept = np.array(swept, dtype=np.int64)
    return swept if bounds else swept[:, 1] - swept[:, 0]


def frame_geometry(points, batch, cells):
    """(items, ranges): items [m, 3] int64, (cell over all point sets, first output point in cell order, live lanes) of every
    work item in the order of their slots; ranges, a list of m int64 arrays, the lengths last - first of the ranges that the
    item's walk hands to the sweep, in the walk's order (two for each of the nine rows, or one where the row is swept whole)"""
    G0, G1, G2 = (int(g) for g in cells)
    _, _, start = _sorted(points, batch, cells)
    items, ranges = [], []
    for k in range(start.shape[0] - 1):
        ts, te = int(start[k]), int(start[k + 1])
        t = ts
        while t < te:  # launch_nearfield_items: a piece of kNearBlock output points per slot
            items.append((k, t, min(t + NEAR_BLOCK, te) - t))  # pair_lane: tend = min(first + kNearBlock, start[cell + 1])
            ranges.append(_walk(k, start, G0, G1, G2))
            t += NEAR_BLOCK
    return np.array(items, dtype=np.int64).reshape(-1, 3), ranges


def point_groups(points, batch, cells):
    """(second_wave, last_item) bool [n] in the caller's order: the point is computed by a lane of the second wave of its
    item (its place in its cell modulo kNearBlock is 64 or more); it belongs to the last item of a cell that is cut into
    several, and that item has idle lanes.  The sort by cell is stable, so a point's place in its cell is its rank among
    the cell's points in the caller's order."""
    _, order, start = _sorted(points, batch, cells)
    n = order.shape[0]
    cell = np.searchsorted(start, np.arange(n), side="right") - 1  # of the sorted points
    rank = np.arange(n) - start[cell]
    size = (start[1:] - start[:-1])[cell]
    second = np.zeros(n, bool)
    last = np.zeros(n, bool)
    second[order] = rank % NEAR_BLOCK >= WAVE
    last[order] = (size > NEAR_BLOCK) & (size % NEAR_BLOCK != 0) & (rank >= (size // NEAR_BLOCK) * NEAR_BLOCK)
    return second, last


def pair_streams(points, batch, cells, pairs):
    """Where the walk of one end of a pair meets the other end.  `pairs` [m, 2] holds caller-order indices (i, j) of two points
    of one point set; direction 0 is "i is computed, j is streamed", direction 1 the reverse.  Returns a dict of int64 [m, 2]
    arrays, one column per direction:
      ``item``    the work item that computes the output point, an index into frame_geometry's items
      ``range``   which of that item's ranges (in the walk's order) holds the streamed point
      ``first``, ``last``  that range in the cell order
      ``offset``  the streamed point's place in it; ``tile`` = offset // kNearTile, the LDS tile it is staged in
    The 27 cells of a walk are distinct (every G_a >= 3), so at most one range holds the streamed point (asserted); where the
    two cells are no neighbours, or the ends lie in two point sets, the walk never meets it: -1 in every array but ``item``."""
    G0, G1, G2 = (int(g) for g in cells)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    _, order, start = _sorted(points, batch, cells)
    n = order.shape[0]
    place = np.empty(n, np.int64)
    place[order] = np.arange(n)  # the caller's index -> the place in the cell order
    cell = np.searchsorted(start, np.arange(n), side="right") - 1  # of the sorted points
    items_before = np.concatenate([[0], np.cumsum(-(-(start[1:] - start[:-1]) // NEAR_BLOCK))])  # items of the cells before
    out = {k: np.full(pairs.shape, -1, np.int64) for k in ("item", "range", "first", "last", "offset", "tile")}
    walks = {}
    for direction in (0, 1):
        pi, pj = place[pairs[:, direction]], place[pairs[:, 1 - direction]]
        ki = cell[pi]
        out["item"][:, direction] = items_before[ki] + (pi - start[ki]) // NEAR_BLOCK
        for k in np.unique(ki):
            if k not in walks:
                walks[k] = _walk(int(k), start, G0, G1, G2, bounds=True)
            rows = np.flatnonzero(ki == k)
            inside = (pj[rows, None] >= walks[k][None, :, 0]) & (pj[rows, None] < walks[k][None, :, 1])
            assert (inside.sum(1) <= 1).all()
            rows, r = rows[inside.any(1)], inside.argmax(1)[inside.any(1)]
            out["range"][rows, direction] = r
            out["first"][rows, direction], out["last"][rows, direction] = walks[k][r, 0], walks[k][r, 1]
    out["offset"] = np.where(out["first"] >= 0, np.stack([place[pairs[:, 1]], place[pairs[:, 0]]], 1) - out["first"], -1)
    out["tile"] = out["offset"] // NEAR_TILE
    return out


# ---- the three layouts -------------------------------------------------------------------------------------------------

REST3, REST_O = 20, 12


def _counts3(flip):
    """the 3^3 grid, rows r = c1 + 3 c2 of three cells: 0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257 and 300, the rest 20
    (1945 points).  0, 255, 256 and 257 stand at c0 = 0, where the items of c0 = 2 sweep them as single cells; 257 + 300 are
    the two-cell range of the items of c0 = 0.  flip: another assignment -- the rows moved on by four and reversed."""
    rows = {0: (257, 300, REST3), 1: (255, 63, 0), 2: (256, 64, 1), 3: (128, 65, 129), 4: (127, REST3, REST3)}
    counts = np.full((9, 3), REST3, dtype=np.int64)
    for r, row in rows.items():
        counts[(r + 4) % 9 if flip else r] = row[::-1] if flip else row
    return counts.reshape(-1)


def _counts_o():
    """cells (4, 5, 3), rows r = c1 + 5 c2 of four cells: the items of the inner cells c0 = 1, 2 sweep three cells as one
    range -- 100 + 100 + 56 = 256, 100 + 100 + 57 = 257, 300 + 257 + 129 = 686 -- and 0 and 255 stand at the rows' ends, where
    they are swept as single cells; the rest hold 12 (2650 points)"""
    rows = {0: (100, 100, 56, REST_O), 1: (100, 100, 57, REST_O), 2: (300, 257, 129, REST_O), 5: (255, 1, 63, 0),
            6: (256, 64, 65, REST_O), 7: (127, 128, REST_O, REST_O)}
    counts = np.full((15, 4), REST_O, dtype=np.int64)
    for r, row in rows.items():
        counts[r] = row
    return counts.reshape(-1)


class Layout:
    """points [n, 3] float32, batch [n] int64 or None, the cells and the counts per point set"""

    def __init__(self, name, cells, counts_per_set, seed):
        rng = np.random.default_rng(seed)
        self.name, self.cells = name, tuple(cells)
        self.counts = counts_per_set  # {point set: counts}
        sets = sorted(counts_per_set)
        parts = [counted_points(rng, cells, counts_per_set[b]) for b in sets]
        self.points = np.concatenate(parts)
        self.batch = None if sets == [0] else np.concatenate([np.full(p.shape[0], b, np.int64) for b, p in zip(sets, parts)])
        self.B = max(sets) + 1
        self.n = self.points.shape[0]

    def set_of(self):
        return np.zeros(self.n, np.int64) if self.batch is None else self.batch


_LAYOUTS = {}
LAYOUTS = ("grid3", "boxO", "ragged3")


def layout(name):
    """grid3: one point set on the 3^3 grid (the unit cube and the box T at r_c = 0.3); boxO: one point set on the cells
    (4, 5, 3) of the box O at r_c = 0.25; ragged3: three point sets on the 3^3 grid, the middle one empty, the first and the
    last with different assignments of the counts to the cells.  Built once and left unchanged."""
    if name not in _LAYOUTS:
        if name == "grid3":
            _LAYOUTS[name] = Layout(name, (3, 3, 3), {0: _counts3(False)}, 1)
        elif name == "boxO":
            _LAYOUTS[name] = Layout(name, (4, 5, 3), {0: _counts_o()}, 2)
        else:
            _LAYOUTS[name] = Layout(name, (3, 3, 3), {0: _counts3(False), 2: _counts3(True)}, 3)
    return _LAYOUTS[name]
