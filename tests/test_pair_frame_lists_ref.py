"""CPU tests of tests/pair_frame_lists_ref.py and of pair_frame_ref.pair_streams: the exclusion lists of
tests/test_gpu_pair_frame_lists.py reach every class that they name -- asserted here from the restated walk, the restated rows
and the separations, not assumed -- the bonded fixtures of tests/test_gpu_lj_excl.py and tests/test_gpu_lj_table.py reach none of
the new ones, and every class has teeth: un-listing its pairs changes the float64 reference of the masked walk by at least
TEETH = 1e-2 of the force on its ends, and so does taking a pair with exactly one zero scale for a fully excluded one (an
`||` in place of the `&&` of the kernels' early return)."""
import numpy as np
import pytest

import pair_frame_lists_ref as pl
import pair_frame_ref as pf
from test_gpu_lj_excl import Case as BondedCase
from test_gpu_pair_frame_lists import EXCL_CASES, _lists

TEETH = 1e-2
IDS = ["%s-%s" % c for c in EXCL_CASES]


@pytest.mark.parametrize("layout,box", EXCL_CASES, ids=IDS)
def test_pair_streams_restates_the_walk(layout, box):
    """the item, range, offset and tile of pair_streams against frame_geometry and the cell order itself"""
    c = _lists(layout, box)
    L = c.L
    items, ranges = pf.frame_geometry(L.points, L.batch, L.cells)
    _, order, start = pf._sorted(L.points, L.batch, L.cells)
    st = pf.pair_streams(L.points, L.batch, L.cells, c.pairs)
    assert all(v.shape == c.pairs.shape for v in st.values())
    key = pf.cell_of(L.points, L.cells) + L.set_of() * int(np.prod(L.cells))
    for direction in (0, 1):
        out, streamed = c.pairs[:, direction], c.pairs[:, 1 - direction]
        it = items[st["item"][:, direction]]
        assert (it[:, 0] == key[out]).all()  # the item's cell is the output point's
        for t in range(len(c.pairs)):
            first, live = it[t, 1], it[t, 2]
            assert out[t] in order[first:first + live]  # ... and the point is one of its live lanes
            r = st["range"][t, direction]
            if r < 0:  # (the pair beyond the cut on cells (4, 5, 3): the walk never meets the partner)
                assert t in c.classes["beyond"] and st["tile"][t, direction] < 0
                continue
            lengths = ranges[st["item"][t, direction]]
            assert lengths[r] == st["last"][t, direction] - st["first"][t, direction]
            assert 0 <= st["offset"][t, direction] < lengths[r]
            assert order[st["first"][t, direction] + st["offset"][t, direction]] == streamed[t]
            assert st["tile"][t, direction] == st["offset"][t, direction] // 256
    met = st["range"] >= 0
    assert met[np.setdiff1d(np.arange(len(c.pairs)), c.classes["beyond"])].all()


@pytest.mark.parametrize("layout,box", EXCL_CASES, ids=IDS)
def test_the_lists_reach_every_class(layout, box):
    import torch_nfft_amd as tn
    c = _lists(layout, box)
    L, pairs, classes = c.L, c.pairs, c.classes
    sets = len(L.counts)
    set_of = L.set_of()
    print("%s: %d pairs; %s" % (c.tag, len(pairs), ", ".join("%s %d" % (k, v.size) for k, v in classes.items())))
    assert (set_of[pairs[:, 0]] == set_of[pairs[:, 1]]).all()  # never across two point sets
    # where the walk meets the partner, recomputed
    st = pf.pair_streams(L.points, L.batch, L.cells, pairs)
    second, last = pf.point_groups(L.points, L.batch, L.cells)
    for k in (0, 1, 2):
        which = classes["tile%d" % k]
        assert which.size >= 8 * sets and (st["tile"][which] == k).any(1).all()
    assert max(st["last"][classes["tile2"]].max(1) - st["first"][classes["tile2"]].max(1)) > 512
    which = classes["second_wave"]
    assert which.size >= 8 * sets and second[pairs[which]].all()
    which = classes["last_item"]
    assert which.size >= 8 * sets and last[pairs[which]].any(1).all()
    if layout == "ragged3":
        n0 = int((set_of == 0).sum())
        which = classes["set2"]
        assert which.size >= 100 and (pairs[which] >= n0).all()  # caller indices past the first set's size
        for name in ("tile1", "tile2", "second_wave", "last_item", "wrap", "face", "row33", "s(0,1)", "s(1,0)"):
            assert np.intersect1d(which, classes[name]).size, name
        blocks = pl.list_blocks(L.n, L.B)
        assert blocks == 6 and blocks * 256 < min(n0, L.n - n0)
        rank = pairs - np.where(set_of[pairs] == 2, n0, 0)
        for b in (0, 2):
            mine = set_of[pairs[:, 0]] == b
            assert ((rank[classes["trip2"]] >= blocks * 256).all(1) & mine[classes["trip2"]]).sum() >= 8
            assert (((rank[classes["straddle"]] >= blocks * 256).sum(1) == 1) & mine[classes["straddle"]]).sum() >= 4
    else:
        assert "set2" not in classes and not classes["trip2"].size and not classes["straddle"].size
    # through the faces
    red = pf._reduce(L.points).astype(np.float64)
    through = np.rint(red[pairs[:, 0]] - red[pairs[:, 1]]) != 0
    assert classes["wrap"].size >= 3 * sets and through[classes["wrap"]].any(1).all() and through[classes["wrap"]].any(0).all()
    below = np.nextafter(np.float32(0.5), np.float32(0))
    which = classes["face"]
    assert which.size == 6 * sets and through[which].any(1).all()
    on_face = (L.points[pairs[which]] == np.float32(-0.5)) | (L.points[pairs[which]] == below)  # [6 sets, 2, 3]
    assert (on_face.any(1) & through[which]).any(1).all() and on_face.any(1).sum(0).tolist() == [2 * sets] * 3
    right, left = (L.points > 0.5).all(1), (L.points < -1.5).all(1)
    assert right[pairs[classes["moved"]]].any() and left[pairs[classes["moved"]]].any()
    # the separations
    r = pl.pair_separation(L, c.A, pairs)
    h = pf.cartesian_spacing(L.cells, c.A)
    assert np.abs(r - c.r_c).min() > 1e-4 * c.r_c
    assert classes["duplicate"].size == sets and not r[classes["duplicate"]].any()
    assert (c.sc[classes["duplicate"]] == 0).all() and (c.sl[classes["duplicate"]] == 0).all()
    which = classes["beyond"]
    assert which.size == sets and (r[which] > c.r_c).all() and (c.sc[which] == 0.5).all() and (c.sl[which] == 0.25).all()
    others = np.setdiff1d(np.arange(len(pairs)), np.concatenate([classes["duplicate"], which]))
    assert r[others].min() >= 0.8 * h and r[others].max() < 0.9 * c.r_c
    for name in ("tile0", "tile1", "tile2", "second_wave", "last_item", "wrap", "trip2", "straddle") + tuple(pl.SCALES):
        picked = classes[name]
        if picked.size:
            near = r[picked] <= pl.NEAR * h  # (the others: entries of a long row, or the partner of a point on a face)
            assert near.sum() >= min(4 * sets, picked.size) and near.mean() >= 0.5, name
    # the scales
    for name, (s_c, s_l) in pl.SCALES.items():
        which = classes[name]
        assert which.size >= 4 * sets and (c.sc[which] == s_c).all() and (c.sl[which] == s_l).all()
    for name in pl.ONE_ZERO:
        assert ((c.sc[classes[name]] == 0) != (c.sl[classes[name]] == 0)).all()
    # the list itself, and its rows
    ex = tn.ExclusionList(pairs, L.n, coulomb_scale=c.sc, dispersion_scale=c.sl, batch=L.batch, device="cpu")
    row_start, col = ex.row_start.numpy(), ex.col.numpy()
    assert (np.diff(row_start) == pl.row_lengths(pairs, L.n)).all()
    report = pl.row_report(L, c.A, c.r_c, pairs, classes)
    for length in pl.ROW_LENGTHS:
        assert classes["row%d" % length].size == length * sets and len(report[length]) == sets
        for row in report[length]:
            p = row["point"]
            mine = col[row_start[p]:row_start[p + 1]]
            assert mine.size == length and mine.tolist() == row["row"] and (np.diff(mine) > 0).all()
            assert (mine[0], mine[-1], mine[length // 2]) == (row["first"], row["last"], row["middle"])
            assert row["inside"]  # every entry is a neighbour inside r_c: the walk hits the first, the last and a middle entry
            assert length == 1 or row["misses"] >= 1  # an unlisted neighbour inside r_c strictly between lo and hi
            assert row["neighbours"] >= 150  # (a crowded cell: the searches that miss are many)
            w = 1.0 - ex.coulomb_weight.numpy()[row_start[p]:row_start[p + 1]]
            assert length == 1 or (np.abs(np.diff(w)) > 0.1).all()  # neighbouring entries carry different scales
    twins = pl.ends(pairs, classes["duplicate"])
    assert (np.diff(row_start)[twins] == 1).all()  # the rows of a duplicate pair hold each other only


def _bonded_reach(w, cells):
    st = pf.pair_streams(w.s, w.batch, cells, w.pairs)
    rows = set(np.bincount(w.pairs.ravel(), minlength=w.n).tolist()) - {0}
    one_zero = int(((w.sc == 0) != (w.sl == 0)).sum())
    behind = st["tile"][w.batch[w.pairs[:, 0]] == 2] if w.batch is not None else np.zeros((0, 2), np.int64)
    return st["tile"], rows, one_zero, behind


@pytest.mark.parametrize("name", ["I", "T", "O"])
def test_the_bonded_fixtures_reach_none_of_the_new_classes(name):
    """the gap that tests/test_gpu_pair_frame_lists.py closes, as test_the_older_fixtures_reach_none_of_the_edges states it for
    the frame: on lj_excl_ref.bonded_points (the points of tests/test_gpu_lj_excl.py; tests/test_gpu_lj_table.py draws the same
    with another seed) no listed partner is staged in a second or third tile, none in the set behind the empty one with a
    second tile, no pair has exactly one zero scale, and no row has 2^k - 1, 2^k or 2^k + 1 entries beyond 1, 2 and 3"""
    cells = (4, 5, 3) if name == "O" else (3, 3, 3)
    for ragged in (False, True):
        tile, rows, one_zero, behind = _bonded_reach(BondedCase(name, ragged), cells)
        print("bonded_points, box %s ragged=%d: tiles %s, row lengths %s" % (name, ragged, sorted(set(tile.ravel().tolist())), sorted(rows)))
        assert tile.max() == 0 and one_zero == 0 and rows <= {1, 2, 3, 4, 20, 21}
        assert not rows & (set(pl.ROW_LENGTHS) - {1, 2, 3, 4})
        if ragged:
            assert behind.size and behind.max() == 0


def test_what_the_large_bonded_fixture_reaches():
    """Case("I", False, n=4000, G=12, seed=5) of tests/test_gpu_lj_excl.py, the one crowded case before this file.  What it
    reaches is written down here: a share of its listed partners are staged in a second tile (no cell of its 3^3 grid holds
    257 points, but every row of three does); none is staged in a third, it has one point set, no pair with exactly one zero
    scale, and its rows are those of the small fixtures plus the one that spans all indices"""
    w = BondedCase("I", False, n=4000, G=12, seed=5)
    tile, rows, one_zero, _ = _bonded_reach(w, (3, 3, 3))
    share = float((tile == 1).any(1).mean())
    print("bonded_points, 4 000 points: tiles %s, %.0f %% of the pairs with a partner in the second tile, row lengths %s"
          % (sorted(set(tile.ravel().tolist())), 100 * share, sorted(rows)))
    assert tile.max() == 1 and 0.1 < share < 0.3  # reached: the second tile, by 19 % of the pairs; not the third
    assert w.batch is None and one_zero == 0
    assert not rows & (set(pl.ROW_LENGTHS) - {1, 2, 3, 4})


@pytest.mark.parametrize("layout,box", EXCL_CASES, ids=IDS)
def test_every_class_has_teeth(layout, box):
    """un-listing a class's pairs changes lj_excl_ref.near_step_scaled by at least TEETH of |F| over the class's ends; a kernel
    that loses the class loses at least that, a hundred times the gates and more"""
    c = _lists(layout, box)
    fref = c.ref("near")[0]
    shown = []
    for name, which in c.classes.items():
        if name in pl.NO_TEETH or which.size == 0:
            continue
        e, df = pl.unlisted_change(c.L, c.A, c.x, c.split, c.pairs, c.sc, c.sl, which)
        ratio = np.linalg.norm(df) / np.linalg.norm(fref[e])
        shown.append("%s %.2e" % (name, ratio))
        assert ratio >= TEETH, (c.tag, name, ratio)
    print("%s: |dF| / |F| over the ends when a class is un-listed: %s" % (c.tag, ", ".join(shown)))
    shown = []
    for name in pl.ONE_ZERO:  # the `||` mutant: a pair with one zero scale taken for a fully excluded one
        e, df = pl.unlisted_change(c.L, c.A, c.x, c.split, c.pairs, c.sc, c.sl, c.classes[name], instead=(0.0, 0.0))
        ratio = np.linalg.norm(df) / np.linalg.norm(fref[e])
        shown.append("%s %.2e" % (name, ratio))
        assert ratio >= TEETH, (c.tag, name, ratio)
    print("%s: the same when a one-zero pair is taken for fully excluded: %s" % (c.tag, ", ".join(shown)))
    # (1, 1) and the pair beyond the cut add nothing to the walk, listed or not: exactly no change
    for name in ("s(1,1)", "beyond"):
        _, df = pl.unlisted_change(c.L, c.A, c.x, c.split, c.pairs, c.sc, c.sl, c.classes[name])
        assert not df.any()
