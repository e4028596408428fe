"""The Verlet rebuild's checkers, proven on the CPU before any GPU run (no GPU needed):

1. tests/verlet_util.py's all_pairs and wall_flags are the reference: equal to the CPU oracle's verlet() (itself pinned to the
   unmodified reference by tests/test_oracle_vs_reference.py).
2. its generators put grains on the thresholds they claim: accepted, rejected and equal pairs on every axis, no pair in
   reach of another pair's grains -- and on a grid whose cell edge is exactly 2 rmax + distVerlet (what the double build
   had) some accepted pairs lie two cells apart, where the 3 x 3 scan never looks; on the padded edge none does.

The counts the search prints (pytest -s) are the ones written down in LABBOOK.md."""
import numpy as np
import pytest

import pyoracle
import samples
import verlet_util as vu
import vib_util

SEARCH_N = 4_000_000   # placements per origin and cell-edge rule; ~3 s each


def oracle_lists(lx, ly, r, x1, x2):
    ora = pyoracle.Oracle(lx, ly, r, x1, x2)
    ora.verlet_rebuild()
    cumul, neigh, _, walls = ora.verlet()
    s = ora.scalars()
    flags = np.zeros(len(r), np.int32)
    for bit, lst in enumerate(walls):
        flags[lst] |= 1 << bit
    return cumul, neigh, flags, s


@pytest.mark.parametrize("case", ["packing_900", "wall_grains"])
def test_restatement_is_the_reference(case):
    if case == "packing_900":
        lx, ly = 512, 384
        r, x1, x2 = samples.to_metres(*samples.row_packing(lx, ly, 900, seed=21))   # test_verlet_pair_set_and_wall_lists' case
    else:
        lx, ly = 128, 96
        r, x1, x2 = vib_util.with_wall_grains(*samples.to_metres(*samples.row_packing(lx, ly, 120, seed=4)), lx, ly)
    cumul_o, neigh_o, flags_o, s = oracle_lists(lx, ly, r, x1, x2)
    cumul, neigh = vu.all_pairs(r, x1, x2)
    assert len(neigh) > (1000 if case == "packing_900" else 40)   # (the cases have lists to compare)
    assert np.array_equal(cumul, cumul_o)
    assert np.array_equal(neigh, neigh_o[:len(neigh)])
    flags = vu.wall_flags(r, x1, x2, s["Mby"], s["Mhy"], s["Mgx"], s["Mdx"])
    assert np.array_equal(flags, flags_o)
    if case == "wall_grains":
        # the oracle's VerletWall has moved the right and top walls out (dtt = 0): candidates of the left wall only; with the
        # walls at the lattice's edges all three pressed grains are candidates
        assert (flags & 4).any()
        near = vu.wall_flags(r, x1, x2, 0.0, 1e-3 * ly / 10, 0.0, 1e-3 * lx / 10)
        assert all((near & b).any() for b in (1, 2, 4, 8))


@pytest.mark.parametrize("origin", vu.ORIGINS)
def test_threshold_pairs_sit_on_the_thresholds(origin):
    rmax, rsmall, lx, ly = 0.15e-3, 0.11e-3, 96, 64
    tp = vu.threshold_pairs(np.random.default_rng(11), rmax, rsmall, lx, ly, origin)
    ncx, ncy = vu.grid_shape(lx, ly, vu.lattice_dx(lx), vu.cell_edge(rmax))
    for axis, which in (("x", 0), ("y", 1), ("d", 2)):
        q = tp[tp["axis"] == axis]
        lhs = vu.pair_lhs(q["ri"], np.nan_to_num(q["xi"]), np.nan_to_num(q["yi"]), q["rj"], np.nan_to_num(q["xj"]),
                          np.nan_to_num(q["yj"]))
        below, equal, above = (lhs[which] < vu.DV).sum(), (lhs[which] == vu.DV).sum(), (lhs[which] > vu.DV).sum()
        print(f"origin {origin} axis {axis}: {len(q)} pairs, {below} below, {equal} on, {above} above the threshold")
        assert below > 0 and equal > 0 and above > 0
        if axis == "d":   # both fabs tests pass: the sqrt decides
            assert (lhs[0] < vu.DV).all() and (lhs[1] < vu.DV).all()
        assert {"last", "first", "mid"} == set(q["place"])
        assert (q["ri"] == q["rj"]).any() and (q["ri"] > q["rj"]).any() and (q["ri"] < q["rj"]).any()
        # i in the last cell and in the first boundary's cells, j on either side of i
        c = vu.grid_cells(q["yi" if axis == "y" else "xi"], origin[axis == "y"], vu.cell_edge(rmax), ncy if axis == "y" else ncx)
        assert c.max() == (ncy if axis == "y" else ncx) - 1 and c.min() <= 1
        d = q["yj"] - q["yi"] if axis == "y" else q["xj"] - q["xi"]
        assert (d > 0).any() and (d < 0).any()
    scenes = vu.pack(tp, rmax, lx, ly, origin)
    assert sum(len(s[0]) for s in scenes) == 2 * len(tp) and len(scenes) <= 24
    acc = far_old = far_new = 0
    for r, x1, x2 in scenes:
        n = len(r)
        assert n <= 300 and r.max() == rmax
        cumul, neigh = vu.all_pairs(r, x1, x2)
        ends = np.concatenate([cumul[:-1], [len(neigh)]])
        i = np.repeat(np.arange(n), np.diff(np.concatenate([[0], ends])))
        assert ((i % 2 == 0) & (neigh == i + 1)).all(), "a grain in reach of another pair's"
        assert 2 * len(neigh) < 8 * n          # the symmetric list under a quarter of the library's 32 n
        a, f0 = vu.straddlers(r, x1, x2, origin, vu.cell_edge(rmax, pad=1.0), lx, ly)
        _, f1 = vu.straddlers(r, x1, x2, origin, vu.cell_edge(rmax), lx, ly)
        acc, far_old, far_new = acc + a, far_old + f0, far_new + f1
    print(f"origin {origin}: {len(scenes)} scenes, {acc} accepted pairs, two cells apart: {far_old} on the edge 2 rmax + dV, "
          f"{far_new} on the padded edge")
    assert acc > 100 and far_new == 0


def test_literal_straddler():
    """the placement of the first CPU search: accepted by the reference, cells 2 and 4 of the unpadded grid at origin 3.3e-4"""
    S = vu.STRADDLER
    r = np.array([S["rmax"]] * 2); x1 = np.array([S["xi"], S["xj"]]); x2 = np.array([2e-3, 2e-3])
    cumul, neigh = vu.all_pairs(r, x1, x2)
    assert cumul.tolist() == [1, 0] and neigh.tolist() == [1]
    assert vu.grid_cells(x1, S["ox"], vu.cell_edge(S["rmax"], pad=1.0), 50).tolist() == [2, 4]
    assert np.ptp(vu.grid_cells(x1, S["ox"], vu.cell_edge(S["rmax"]), 50)) <= 1


@pytest.mark.parametrize("origin", vu.ORIGINS)
def test_search_for_pairs_the_scan_cannot_see(origin):
    """Random placements on the threshold (verlet_util.search_straddlers: both axes, the diagonal down to 1e-9 rad off an
    axis, unequal radii, k up to 400). Edge 2 rmax + distVerlet: at a non-zero origin the search must find accepted pairs two
    cells apart; at origin 0 the count is printed and recorded (LABBOOK.md), nothing is asserted about it. Edge padded by
    1.001, the library's: none anywhere -- the bound in lbmdem_create's comment says there cannot be."""
    found = {}
    for pad in (1.0, vu.CELL_PAD):
        rng = np.random.default_rng(2024)
        acc = far = 0
        for _ in range(SEARCH_N // 1_000_000):
            a, f = vu.search_straddlers(rng, 1_000_000, origin, pad)
            acc, far = acc + a, far + f
        found[pad] = far
        print(f"origin {origin} cell edge x {pad}: {SEARCH_N} placements, {acc} accepted, {far} of them two cells apart")
    if origin != (0.0, 0.0):
        assert found[1.0] > 0
    assert found[vu.CELL_PAD] == 0
