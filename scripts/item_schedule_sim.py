#!/usr/bin/env python3
"""List scheduling of the matrix-core kernels' work items on the CUs, on the host (no GPU).

How the grading rule of the work list (csrc/common.h: grade_fraction; csrc/binning.hip: segment_split_kernel) was chosen and
how a new shape is checked: the hardware dispatcher hands the workgroups of a launch to the CUs in grid order, one per CU
for these kernels, so a launch over the list in launch order IS list scheduling -- every item goes to the CU that is free
first.  With a cost per item that is simulated with a heap.

Cost model (fitted to profiles/r03_spread_trace.txt, the spreading kernel at uniform C3): an item takes
    us_per_kblock * K-blocks + us_per_item           (0.624 us, 16 us: set-up, flush, workgroup turn-around)
where a K-block is 16 points of one slab.  For an item list that carries points only, K-blocks are estimated as
points / 16 + slabs / 2 (every slab's last K-block is half full on average).

    python scripts/item_schedule_sim.py                       # the graded split against the equal one, uniform C3
    python scripts/item_schedule_sim.py --n 4000000 --N 128   # another shape
    python scripts/item_schedule_sim.py --items list.npy      # a plan's list as nfft_dbg_work_list returns it

Outputs span (us), ideal (sum of the costs / CUs) and utilisation (ideal / span).
"""
import argparse
import heapq
import json

import numpy as np

US_PER_KBLOCK = 0.624
US_PER_ITEM = 16.0
MAX_ITEM_SLABS = 128   # csrc/common.h kItemMaxSlabs
SEG_MAX = 32           # csrc/common.h kSegMax
MAX_ITEM_COUNT = 256   # csrc/common.h kItemMaxCount
GRADE_TAIL = 3         # csrc/common.h kGradeTail


def geometry(N, m):
    """Pencils of the wide tiling: M slabs, tiles of (32 - 2m - 1) rows x (64 - 2m - 1) columns."""
    M = 2 * N
    t1, t2 = 32 - (2 * m + 1), 64 - (2 * m + 1)
    n1, n2 = -(-M // t1), -(-M // t2)
    rows = [min(t1, M - j * t1) for j in range(n1)]
    cols = [min(t2, M - j * t2) for j in range(n2)]
    return M, [(r, c) for r in rows for c in cols]


def seg_target_points(n, nsets, ncu, items_per_cu=5.4):
    return max(2048, int(n / nsets / (items_per_cu * ncu) + 0.5))


def seg_base_runs(n, nsets, pencils, M, ncu, items_per_cu=5.4):
    avg = n / (nsets * pencils)
    r = int(avg / seg_target_points(n, nsets, ncu, items_per_cu) + 0.5)
    lo = (M + 127) // 128
    hi = max(M // 32, lo)
    r = min(max(r, lo), hi)
    while r < hi and nsets * pencils * (r + 1) <= ncu:
        r += 1
    return min(r, SEG_MAX)


def grade_fraction(i, k, graded):
    """Share of a pencil's points in front of item i of k (mirror of common.h grade_fraction): graded, the last three
    items hold 3/4, 1/2 and 1/4 of one of the others."""
    if i <= 0:
        return 0.0
    if i >= k:
        return 1.0
    if not graded:
        return i / k
    big = k - GRADE_TAIL
    total = big + 1.5
    if i <= big:
        return i / total
    return (big + (0.75 if i - big == 1 else 1.25)) / total


def tail_pencils(pencils, runs, M, ncu):
    """Pencils at the end of the grid order that the equal cut gives 2 x runs ranges (mirror of common.h tail_pencils)."""
    if pencils * runs <= ncu or 2 * runs > M // 32 or 2 * runs > 64:
        return 0
    return min((ncu + 2 * runs - 1) // (2 * runs), pencils // 2)


def pencil_items(off, runs, set_pts, pencils, target, grade, fine=False):
    """Items (first slab, end slab, points) of one pencil from its slab offsets `off` (M + 1 ints): mirror of
    segment_split_kernel (csrc/binning.hip)."""
    M = len(off) - 1
    P = int(off[M] - off[0])
    if not grade:  # the equal cut (default): `runs` equal ranges of slabs, a range of >= 1.5 x target points cut on by points
        k = 2 * runs if fine else runs  # (a pencil of the launch's tail: twice as many ranges)
        seg = (M + k - 1) // k
        items = []
        for sb in range(0, M, seg):
            se = min(sb + seg, M)
            pts = int(off[se] - off[sb])
            pieces = min(max((pts + target // 2) // target, 1), 16)
            cuts = [sb] + [int(np.searchsorted(off, off[sb] + pts * p // pieces, side="left")) for p in range(1, pieces)] + [se]
            items += [(a, b, int(off[b] - off[a])) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        return items
    lo = (M + MAX_ITEM_SLABS - 1) // MAX_ITEM_SLABS
    hi = max(M // 32, lo)
    at_rate = min(runs * pencils / max(set_pts, 1) * P + 0.5, hi)
    dense = P / target + 0.5
    k = max(lo, int(min(max(at_rate, dense), MAX_ITEM_COUNT)))
    by_slabs = k == lo
    graded = k >= lo + 2 and k > GRADE_TAIL

    def cut(i):
        if i <= 0:
            return 0
        if i >= k:
            return M
        if by_slabs:
            return min(M, i * ((M + k - 1) // k))
        t = off[0] + int(P * grade_fraction(i, k, graded))
        return int(np.searchsorted(off, t, side="left"))

    items = []
    for i in range(k):
        a, b = cut(i), cut(i + 1)
        if b <= a:
            continue
        parts = -(-(b - a) // MAX_ITEM_SLABS)
        for p in range(parts):
            s, e = a + (b - a) * p // parts, a + (b - a) * (p + 1) // parts
            items.append((s, e, int(off[e] - off[s])))
    return items


def uniform_offsets(n, N, m, seed=0):
    """Slab offsets of every pencil for n uniform points (binomial counts: no point array needed)."""
    M, pencils = geometry(N, m)
    rng = np.random.default_rng(seed)
    p = np.array([r * c for r, c in pencils], dtype=np.float64) / (M * M)
    per_pencil = rng.multinomial(n, p / p.sum())
    offs = []
    for cnt in per_pencil:
        slabs = rng.multinomial(cnt, np.full(M, 1.0 / M))
        offs.append(np.concatenate([[0], np.cumsum(slabs)]))
    return M, offs


def item_cost(points, slabs, kblocks=None):
    kb = kblocks if kblocks is not None else points / 16.0 + slabs / 2.0
    return US_PER_KBLOCK * kb + US_PER_ITEM


def simulate(costs, ncu=256):
    """List scheduling in the given order.  Returns span, ideal, utilisation."""
    costs = [float(c) for c in costs]
    if not costs:
        return 0.0, 0.0, 1.0
    free = [0.0] * ncu
    heapq.heapify(free)
    span = 0.0
    for c in costs:
        t = heapq.heappop(free) + c
        span = max(span, t)
        heapq.heappush(free, t)
    ideal = sum(costs) / ncu
    return span, ideal, ideal / span


def order_by_class(items, classes=16):
    """Launch order of work_order_kernel: 16 size classes (sixteenths of the largest item), biggest first, stable."""
    mx = max(1, max(it[2] for it in items))
    cls = [classes - 1 - min(classes - 1, int(it[2] * classes / mx)) for it in items]
    return [it for _, it in sorted(zip(cls, items), key=lambda t: t[0])]


def simulate_list(entries, ncu=256):
    """entries: rows {pencil, first slab, end slab, points} in launch order (one point set)."""
    return simulate([item_cost(e[3], e[2] - e[1]) for e in entries], ncu)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--items-per-cu", type=float, default=5.4)
    ap.add_argument("--items", help=".npy of int32 [entries, 4] rows {pencil, first slab, end slab, points} in launch order")
    a = ap.parse_args()
    if a.items:
        e = np.load(a.items)
        span, ideal, util = simulate_list(e, a.cus)
        print(json.dumps({"items": int(len(e)), "span_us": round(span, 1), "ideal_us": round(ideal, 1),
                          "span_over_ideal": round(span / ideal, 4), "utilisation": round(util, 4)}))
        return
    M, offs = uniform_offsets(a.n, a.N, a.m)
    target = seg_target_points(a.n, 1, a.cus, a.items_per_cu)
    runs = seg_base_runs(a.n, 1, len(offs), M, a.cus, a.items_per_cu)
    tailp = tail_pencils(len(offs), runs, M, a.cus)
    for name, grade, ordered, tail in (("equal cut, grid order", False, False, 0),
                                       ("... finer last pencils (default)", False, False, tailp),
                                       ("equal cut, biggest first", False, True, 0),
                                       ("graded cut, biggest first", True, True, 0)):
        items = []
        for i, off in enumerate(offs):
            items += pencil_items(off, runs, a.n, len(offs), target, grade, fine=i >= len(offs) - tail)
        if ordered:
            items = order_by_class(items)
        span, ideal, util = simulate([item_cost(p, e - s) for s, e, p in items], a.cus)
        print("%-36s items %5d (%.2f per CU)  span %7.1f us  ideal %7.1f us  span/ideal %.3f  utilisation %.3f"
              % (name, len(items), len(items) / a.cus, span, ideal, span / ideal, util))


if __name__ == "__main__":
    main()
