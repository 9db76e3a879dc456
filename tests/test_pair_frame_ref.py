"""CPU tests of tests/pair_frame_ref.py: the three counted layouts of tests/test_gpu_pair_frame_edges.py reach every edge of
the pair kernels' frame (csrc/pair_frame.h: kNearBlock = 128, kNearTile = 256, the 64-lane wave) -- asserted here from the
restated item list and walk, not assumed -- and the fixtures of the Yukawa and Lennard-Jones tests reach none of them."""
import numpy as np
import pytest

import dispersion_ref as dr
import lj_step_ref as lj
import pair_frame_ref as pf
import yukawa_ref as yr
from ewald_box_ref import O, T

BOXES = {"grid3": (None, T), "boxO": (O,), "ragged3": (None, T)}


def _edges(points, batch, cells):
    """(the live-lane counts, the cells cut after exactly 128 + 1, the swept range lengths) of a point set"""
    items, ranges = pf.frame_geometry(points, batch, cells)
    live = set(items[:, 2].tolist())
    split = {int(k) for k in np.unique(items[:, 0]) if items[items[:, 0] == k][:, 2].tolist() == [128, 1]}
    return items, live, split, set(np.concatenate(ranges).tolist())


@pytest.mark.parametrize("name", pf.LAYOUTS)
def test_layout_reaches_every_edge(name):
    L = pf.layout(name)
    K = int(np.prod(L.cells))
    key = pf.cell_of(L.points, L.cells) + L.set_of() * K
    counts = np.bincount(key, minlength=L.B * K)
    for b in range(L.B):  # exactly the chosen counts, the empty middle set included
        want = L.counts.get(b, np.zeros(K, np.int64))
        assert (counts[b * K:(b + 1) * K] == want).all()
    items, live, split, swept = _edges(L.points, L.batch, L.cells)
    print("%s: %d points, %d items, live lanes %s, range lengths up to %d"
          % (name, L.n, items.shape[0], sorted(live), max(swept)))
    # the item list is what the counts say: ceil(count / 128) items per cell, none empty, every point in one lane
    assert items[:, 2].min() >= 1 and items[:, 2].max() <= 128 and int(items[:, 2].sum()) == L.n
    assert (np.bincount(items[:, 0], minlength=L.B * K) == -(-counts // 128)).all()
    assert (np.diff(items[:, 0] * (1 << 20) + items[:, 1]) > 0).all()
    assert {1, 63, 64, 65, 127, 128} <= live and split                  # 64/65: the second wave; 128/129: the cut
    assert {0, 255, 256, 257} <= swept and max(swept) > 512             # 256/257: the second tile; a third
    # the groups of tests/test_gpu_pair_frame_edges.py are not empty
    second, last = pf.point_groups(L.points, L.batch, L.cells)
    assert second.sum() > 100 and last.sum() > 30 and (~second & ~last).sum() > 100
    assert int(second.sum()) == int(sum(max(0, int(v) - 64) for v in items[:, 2]))
    cut = [k for k in np.unique(items[:, 0]) if (items[:, 0] == k).sum() > 1 and counts[k] % 128]
    assert int(last.sum()) == int(sum(counts[k] % 128 for k in cut))


def test_ragged_layout_reaches_the_edges_in_its_last_set():
    """set 2 starts at cell 54 and at item slots past those of set 0: a cut cell and a multi-tile range there, and another
    assignment of the counts than set 0's"""
    L = pf.layout("ragged3")
    assert L.B == 3 and 1 not in L.counts and (L.batch != 1).all() and (np.diff(L.batch) >= 0).all()
    assert sorted(L.counts[0]) == sorted(L.counts[2]) and (L.counts[0] != L.counts[2]).any()
    items, ranges = pf.frame_geometry(L.points, L.batch, L.cells)
    own = items[:, 0] >= 54
    assert own.any() and (items[~own, 0] < 27).all()
    n0 = int(L.counts[0].sum())
    assert items[own, 1].min() == n0  # (the first output point of set 2 in cell order)
    cells2 = items[own, 0]
    assert max((cells2 == k).sum() for k in np.unique(cells2)) == 3  # 257 and 300: three items
    assert {1, 63, 64, 65, 127, 128} <= set(items[own, 2].tolist())
    swept = set(np.concatenate([r for r, o in zip(ranges, own) if o]).tolist())
    assert {0, 255, 256, 257} <= swept and max(swept) > 512
    # a set's ranges hold its own points only
    for r, (k, _, _) in zip(ranges, items):
        assert int(r.sum()) == (n0 if k < 27 else L.n - n0)


@pytest.mark.parametrize("name", pf.LAYOUTS)
def test_minimum_separation_and_edge_cases(name):
    """the stated separation in each box's metric, through the wrap (as _assert_separated of tests/test_gpu_lj_step.py), and
    the edge cases of the wrap are there"""
    L = pf.layout(name)
    p = L.points
    for b in sorted(L.counts):
        s = p[L.set_of() == b]
        for A in BOXES[name]:
            Am = dr._box(A)
            d_min = pf.d_min_fractional(L.cells) * np.linalg.svd(Am, compute_uv=False).min()
            got = dr.min_separation(s, Am)
            print("%s set %d box %s: min separation %.4f, stated %.4f, lattice spacing %.4f"
                  % (name, b, "cube" if A is None else "TO"[int(A is O)], got, d_min, pf.cartesian_spacing(L.cells, A)))
            assert got >= d_min * (1 - 1e-6)
            assert got >= 0.8 * pf.cartesian_spacing(L.cells, A)  # (what the r^-12 terms see)
        below = np.nextafter(np.float32(0.5), np.float32(0))
        for a in range(3):
            assert (s[:, a] == np.float32(-0.5)).sum() == 1 and (s[:, a] == below).sum() == 1
        assert ((s > 0.5).all(1)).sum() == 4 and ((s < -1.5).all(1)).sum() == 4
        assert s.shape[0] - np.unique(s, axis=0).shape[0] == 1  # one exact duplicate pair
    # shuffled: the caller's order is not the cell order
    key = pf.cell_of(p, L.cells)[L.set_of() == 0]
    assert (np.diff(key) < 0).sum() > key.shape[0] // 4


def test_cell_of_at_the_faces():
    below = np.nextafter(np.float32(0.5), np.float32(0))
    p = np.array([[-0.5, 0.0, below], [0.5, below, -0.5], [1.25, -2.25, 0.1666], [-0.16, 0.17, 0.1667]], dtype=np.float32)
    c = pf.cell_of(p, (3, 3, 3))
    assert c.tolist() == [0 + 3 * (1 + 3 * 2), 0 + 3 * (2 + 3 * 0), 2 + 3 * (0 + 3 * 1), 1 + 3 * (2 + 3 * 2)]
    assert pf.cell_of(p[:1], (4, 5, 3)).tolist() == [0 + 4 * (2 + 5 * 2)]


@pytest.mark.parametrize("what", ["yukawa", "lj"])
def test_the_older_fixtures_reach_none_of_the_edges(what):
    """the gap that tests/test_gpu_pair_frame_edges.py closes: on every grid of tests/test_gpu_yukawa.py and
    tests/test_gpu_lj_step.py no item has a second wave, no cell is cut and no range fills a tile"""
    if what == "yukawa":
        sets = [(yr.near_points(), b) for b in (None, np.concatenate([np.zeros(230, np.int64), np.full(282, 2, np.int64)]))]
        grids = [(3, 3, 3), (4, 4, 4), (8, 8, 8), (4, 5, 3), (9, 11, 7), (3, 4, 4)]
    else:
        import dispersion_virial_ref as dv
        sets = [(lj.lj_points(np.random.default_rng(k)), b) for k in (0, 101, 400) for b in (None, dv.ragged_batch(700))]
        grids = [(4, 5, 3), (3, 3, 3), (7, 8, 7), (3, 4, 4)]
    for s, batch in sets:
        for cells in grids:
            items, live, split, swept = _edges(s, batch, cells)
            assert max(live) <= 64 and not split and max(swept) < 256, (what, cells, max(live), max(swept))
            assert (np.bincount(items[:, 0]) <= 1).all()
