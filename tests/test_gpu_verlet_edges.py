"""The Verlet rebuild (counting sort by cell + k_verlet_scan, dem_kernels.hip) against the reference's all-pairs list at the
places where a uniform grid can go wrong: pairs on the candidate test's threshold across cell boundaries, a grid origin off
zero, grains the grid does not cover, degenerate grids and counts, wall flags on the strict threshold, arrival order.

Expected values come from tests/verlet_util.py (numpy float64 all-pairs restatement, proven against the CPU oracle and the
generators proven on the CPU by tests/test_verlet_host.py). fp64 handles, np.array_equal throughout. List overflow is not
tested here: every case keeps the symmetric list under a quarter of the library's 32 n entries and asserts so."""
import ctypes as C

import numpy as np
import pytest

import verlet_util as vu

pytestmark = pytest.mark.gpu

LX, LY = 96, 64
RMAX, RSMALL = 0.15e-3, 0.11e-3


def check_lists(sim, r, x1, x2, what=""):
    """sim's list, wall flags and pair count against the restatement; -> number of pairs"""
    n = len(r)
    cumul, neigh, wf = sim.verlet()
    ec, en = vu.all_pairs(r, x1, x2, sim.cfg.phys.distVerlet)
    assert 2 * len(en) < 8 * n or n < 3, f"{what}: the case itself is too dense ({len(en)} pairs of {n} grains)"
    assert len(neigh) == len(en), f"{what}: {len(neigh)} pairs, the reference has {len(en)}"
    assert np.array_equal(cumul, ec), f"{what}: cumul"
    assert np.array_equal(neigh, en), f"{what}: neighbours"
    cfg = sim.config()
    assert np.array_equal(wf, vu.wall_flags(r, x1, x2, cfg.Mby, cfg.Mhy, cfg.Mgx, cfg.Mdx, cfg.phys.distVerlet)), f"{what}: wall flags"
    return len(en)


def threshold_scenes(origin):
    tp = vu.threshold_pairs(np.random.default_rng(11), RMAX, RSMALL, LX, LY, origin)
    return vu.pack(tp, RMAX, LX, LY, origin)


def run_threshold_scenes(pkg, origin):
    total = 0
    for k, (r, x1, x2) in enumerate(threshold_scenes(origin)):
        with pkg.LbmDem(LX, LY, r, x1, x2, origin=origin if origin != (0.0, 0.0) else None) as sim:
            sim.initVerlet()
            cfg = sim.config()
            assert (cfg.Mgx, cfg.Mby) == origin
            total += check_lists(sim, r, x1, x2, f"origin {origin} scene {k}")
    assert total > 100     # (accepted pairs; as many again are rejected by an ulp or more)


def test_threshold_pairs_default_origin(pkg):
    """1. accepted, rejected-by-an-ulp and equal pairs along x, y and the diagonal, radii (rmax, rmax) and (rmax, smaller) in
    either order, i at the last double of a cell, the first of the next and mid-cell, boundaries across the lattice incl. the
    last cell, j on either side: the list holds exactly the accepted ones."""
    run_threshold_scenes(pkg, (0.0, 0.0))


def test_threshold_pairs_nonzero_origin(pkg):
    """2. the same with the walls Mgx, Mby off zero. Route: a config handed to lbmdem_create (LbmDem(origin=...)). With the
    placement the CPU search found for a cell edge of exactly 2 rmax + distVerlet: a pair the reference lists, cells 2 and 4
    of that grid -- the library's padded edge keeps it inside the 3 x 3 cells."""
    origin = vu.ORIGINS[1]
    run_threshold_scenes(pkg, origin)
    S = vu.STRADDLER
    rng = np.random.default_rng(3)
    r = np.concatenate([[S["rmax"]] * 2, rng.uniform(0.2e-3, 0.4e-3, 10)])
    x1 = np.concatenate([[S["xi"], S["xj"]], rng.uniform(0.5e-3, 9e-3, 10)])
    x2 = np.concatenate([[2.1e-3, 2.1e-3], rng.uniform(3.5e-3, 6e-3, 10)])
    with pkg.LbmDem(LX, LY, r, x1, x2, origin=(S["ox"], origin[1])) as sim:
        sim.initVerlet()
        cumul, neigh, _ = sim.verlet()
        assert cumul[0] == 1 and neigh[0] == 1, "the straddling pair is missing from the list"
        check_lists(sim, r, x1, x2, "literal straddler")


@pytest.mark.parametrize("origin", vu.ORIGINS)
def test_grains_outside_the_grid(pkg, origin):
    """3. centres left of and below the origin, right of and above the last cell, several cell edges out, in the corners;
    two outside grains close to each other, an outside grain next to an inside one: the clamp into the edge cells loses no
    pair and invents none."""
    lx, ly, R = 64, 48, 0.3e-3
    cs = vu.cell_edge(R)
    W, H = vu.lattice_dx(lx) * (lx - 1), vu.lattice_dx(lx) * (ly - 1)
    ncx, ncy = vu.grid_shape(lx, ly, vu.lattice_dx(lx), cs)
    ox, oy = origin
    rng = np.random.default_rng(17)
    xs = [ox - 0.2 * cs, ox - 1.5 * cs, ox - 5 * cs, ox - 5 * cs + 0.9 * cs, ox - 0.4 * cs, ox + 0.5 * cs,       # left
          ox + ncx * cs + 0.3 * cs, ox + ncx * cs + 4 * cs, ox + ncx * cs + 4.8 * cs, ox + ncx * cs - 0.5 * cs,  # right
          ox + 2 * cs, ox + 2.6 * cs, ox + 2.2 * cs, ox + 2.3 * cs,                                              # above
          ox - 3 * cs, ox - 3.5 * cs, ox + ncx * cs + 3 * cs, ox + ncx * cs + 2.4 * cs]                          # corners
    ys = [oy + 1.3 * cs, oy + 1.3 * cs, oy + 2 * cs, oy + 2.1 * cs, oy + 3 * cs, oy + 3.2 * cs,
          oy + cs, oy + 1.4 * cs, oy + 1.5 * cs, oy + 0.8 * cs,
          oy + ncy * cs + 0.1 * cs, oy + ncy * cs + 0.2 * cs, oy + ncy * cs + 6 * cs, oy + ncy * cs - 0.4 * cs,
          oy - 2 * cs, oy - 2.2 * cs, oy + ncy * cs + 2 * cs, oy + ncy * cs + 2.5 * cs]
    m = 180
    x1 = np.concatenate([xs, ox + rng.uniform(-4 * cs, W + 4 * cs, m)])
    x2 = np.concatenate([ys, oy + rng.uniform(-4 * cs, H + 4 * cs, m)])
    r = np.concatenate([np.full(len(xs), R), rng.uniform(0.5 * R, R, m)])
    outside = (x1 < ox) | (x2 < oy) | (x1 >= ox + ncx * cs) | (x2 >= oy + ncy * cs)
    assert outside.sum() > 60 and (~outside).sum() > 30
    with pkg.LbmDem(lx, ly, r, x1, x2, origin=origin if origin != (0.0, 0.0) else None) as sim:
        sim.initVerlet()
        npairs = check_lists(sim, r, x1, x2, "outside grains")
    _, neigh = vu.all_pairs(r, x1, x2)
    assert npairs > 100 and outside[neigh].sum() > 30   # (pairs with an outside partner are there to be lost)


def test_degenerate_grids_and_counts(pkg):
    """4. a grid of 2 x 2 cells; n = 1 (empty list), n = 2 touching and far apart; 60 small grains in ONE cell of a grid that
    a large grain far away makes coarse; 63 / 64 / 65 grains (a tile of k_tile_halo and k_dem_chain); grains with identical
    coordinates (distance 0, a pair like any other)."""
    rng = np.random.default_rng(23)
    cases = []
    R = 2.6e-3                                   # 37 x 50 nodes = 3.7 x 5 mm, cell edge 5.7 mm: ncx = ncy = 2
    assert vu.grid_shape(37, 50, vu.lattice_dx(37), vu.cell_edge(R)) == (2, 2)
    cases.append(("2x2 grid", 37, 50, np.concatenate([[R], rng.uniform(0.4e-3, 0.9e-3, 15)]),
                  np.concatenate([[1.5e-3], rng.uniform(0.0, 12e-3, 15)]), np.concatenate([[1e-3], rng.uniform(0.0, 12e-3, 15)])))
    cases.append(("n = 1", LX, LY, np.array([0.4e-3]), np.array([3e-3]), np.array([2e-3])))
    cases.append(("n = 2 touching", LX, LY, np.array([0.4e-3, 0.3e-3]), np.array([3e-3, 3.7e-3]), np.array([2e-3, 2e-3])))
    cases.append(("n = 2 apart", LX, LY, np.array([0.4e-3, 0.3e-3]), np.array([3e-3, 7e-3]), np.array([2e-3, 4e-3])))
    # one grain of 1.5 mm: cell edge 3.5 mm; 60 grains of 0.02 mm (reach 0.54 mm) inside cell (1, 0), three of them on one spot
    cs = vu.cell_edge(1.5e-3)
    cx = np.concatenate([[8.5e-3], cs + rng.uniform(0.05, 0.95, 60) * cs]); cy = np.concatenate([[5.5e-3], rng.uniform(0.05, 0.95, 60) * cs])
    cx[5] = cx[40] = cx[17]; cy[5] = cy[40] = cy[17]
    cr = np.concatenate([[1.5e-3], np.full(60, 0.02e-3)])
    assert (vu.grid_cells(cx[1:], 0.0, cs, 4) == 1).all() and (vu.grid_cells(cy[1:], 0.0, cs, 3) == 0).all()
    cases.append(("one crowded cell", LX, LY, cr, cx, cy))
    for n in (63, 64, 65):
        x = 0.4e-3 + 0.14e-3 * np.arange(n)      # a row, every grain with ~3 partners on either side
        cases.append((f"n = {n}", LX, LY, np.full(n, 0.05e-3), x, np.full(n, 2e-3) + 1e-5 * rng.standard_normal(n)))
    for what, lx, ly, r, x1, x2 in cases:
        with pkg.LbmDem(lx, ly, r, x1, x2) as sim:
            sim.initVerlet()
            npairs = check_lists(sim, r, x1, x2, what)
            cumul, neigh, _ = sim.verlet()
        if what in ("n = 1", "n = 2 apart"):
            assert npairs == 0 and not cumul.any() and len(neigh) == 0
        elif what == "n = 2 touching":
            assert cumul.tolist() == [1, 0] and neigh.tolist() == [1]
        elif what == "one crowded cell":
            assert npairs > 100
            _, en = vu.all_pairs(r, x1, x2)
            assert 40 in en and 17 in en          # the coincident grains are partners of each other
        else:
            assert npairs > 2


def wall_threshold_grains(lx, ly, Mby, Mhy, Mgx, Mdx, dV=vu.DV):
    """for each wall grains whose left-hand side of VerletWall's test is below, on and above distVerlet by an ulp or two:
    a sweep of -4 .. +4 ulps of the coordinate around the threshold; the other coordinate mid-box. Dyadic radii: next to a wall
    at 0 the sum r + distVerlet is a double, so the sweep holds a grain exactly on the threshold. (Next to a wall elsewhere
    the left-hand side is a multiple of the coordinate's ulp, which distVerlet = 5e-4 is not: no double sits on it.)"""
    rs, xs, ys = [], [], []
    for wall in range(4):
        for r in (2.0 ** -12, 3 * 2.0 ** -13, 2.0 ** -11):
            M = (Mby, Mhy, Mgx, Mdx)[wall]
            c0 = (M + r) + dV if wall in (0, 2) else (M - r) - dV
            for m in range(-4, 5):
                c = float(vu.ulps(c0, m))
                rs.append(r)
                xs.append(c if wall >= 2 else 0.5 * (Mgx + 1e-4 * lx)); ys.append(c if wall < 2 else 0.5 * (Mby + 1e-4 * ly))
    return np.array(rs), np.array(xs), np.array(ys)


@pytest.mark.parametrize("dtt,origin", [(0.0, vu.ORIGINS[0]), (1.0, vu.ORIGINS[0]), (1.0, vu.ORIGINS[1])])
def test_wall_flags_on_the_strict_threshold(pkg, dtt, origin):
    """5. the four strict `<` of VerletWall (main.c:1563-1593) with grains an ulp below, on and an ulp above distVerlet, at
    the right and top walls the rebuild has just moved: to 1e-3 lx, 1e-3 ly (dtt = 0, the reference's default: ten times the
    lattice away) and to the lattice's edge (nbsteps * dt < dtt); left and bottom walls at 0 and off zero."""
    phys = pkg.Physics()
    pkg.load_library().lbmdem_physics_defaults(C.byref(phys))
    phys.dtt = dtt
    Mdx, Mhy = (1.e-3 * LX / 10, 1.e-3 * LY / 10) if dtt > 0 else (1.e-3 * LX, 1.e-3 * LY)     # main.c:1555-1561
    r, x1, x2 = wall_threshold_grains(LX, LY, origin[1], Mhy, origin[0], Mdx)
    lhs = vu.wall_lhs(r, x1, x2, origin[1], Mhy, origin[0], Mdx)
    for wall in range(4):     # the sweep does straddle the threshold
        own = lhs[wall][wall * 27:(wall + 1) * 27]
        assert (own < vu.DV).any() and (own > vu.DV).any(), wall
        assert (own == vu.DV).any() or (origin[1], Mhy, origin[0], Mdx)[wall] != 0.0, wall
    with pkg.LbmDem(LX, LY, r, x1, x2, physics=phys, origin=origin if origin != (0.0, 0.0) else None) as sim:
        sim.initVerlet()
        cfg = sim.config()
        assert (cfg.Mgx, cfg.Mdx, cfg.Mby, cfg.Mhy) == (origin[0], Mdx, origin[1], Mhy)
        _, _, wf = sim.verlet()
        assert np.array_equal(wf, vu.wall_flags(r, x1, x2, origin[1], Mhy, origin[0], Mdx))
        flagged = [int(((wf >> w) & 1)[w * 27:(w + 1) * 27].sum()) for w in range(4)]
        assert all(0 < f < 27 for f in flagged), flagged


def test_partner_order_does_not_depend_on_arrival(pkg):
    """6. one packing (lists of 6-12 partners) under three numberings, each against all_pairs of the renumbered arrays; a
    second rebuild on the same handle (k_cell_scatter has returned the cell counts to zero); a rebuild after every grain has
    moved to another cell."""
    rng = np.random.default_rng(31)
    n = 300
    r = rng.uniform(0.04e-3, 0.07e-3, n)
    x1, x2 = rng.uniform(0.3e-3, 9.3e-3, n), rng.uniform(0.3e-3, 6.1e-3, n)     # ~5.7 grains per mm^2, reach ~0.61 mm
    for trial in range(3):
        p = rng.permutation(n) if trial else np.arange(n)
        rp, xp, yp = r[p], x1[p], x2[p]
        with pkg.LbmDem(LX, LY, rp, xp, yp) as sim:
            sim.initVerlet()
            npairs = check_lists(sim, rp, xp, yp, f"numbering {trial}")
            assert 6 <= 2 * npairs / n < 8      # (lists of 6 and more, the whole under a quarter of the allocation)
            first = sim.verlet()
            sim.initVerlet()
            again = sim.verlet()
            assert all(np.array_equal(a, b) for a, b in zip(first, again)), "second rebuild differs"
            cs = vu.cell_edge(float(r.max()))
            k = sim.kinematics
            k[:, 0] += 1.7 * cs; k[:, 1] += 1.3 * cs
            k[::2, 0] += 0.31 * cs                     # (not a rigid shift: the list changes)
            sim.kinematics = k
            sim.initVerlet()
            moved = check_lists(sim, rp, k[:, 0], k[:, 1], f"numbering {trial}, moved")
            assert moved != npairs


def test_list_as_the_substep_sees_it(pkg, po):
    """7. the threshold scene of test 1 through its consumers: fluid step, rebuild and 5 sub-steps phase by phase, one launch
    per sub-step, and renderScene(5) with the multi-sub-step kernel on a twin -- bit-equal to each other and to the CPU
    oracle. None of the threshold pairs touches: whether a pair an ulp from the threshold is listed must change nothing."""
    r, x1, x2 = threshold_scenes((0.0, 0.0))[0]
    _, en = vu.all_pairs(r, x1, x2)
    assert len(en) > 10
    a, b, ora = pkg.LbmDem(LX, LY, r, x1, x2), pkg.LbmDem(LX, LY, r, x1, x2), po.Oracle(LX, LY, r, x1, x2)
    a.set_dem_chain(0)
    a.lbm_step(); a.initVerlet()
    check_lists(a, r, x1, x2, "scene 0")
    for _ in range(5):
        a.dem_substep()
    b.renderScene(5)
    ora.steps(5)
    assert b.dem_chain_stats()[0] > 0 and a.dem_chain_stats()[0] == 0
    ka, kb, ko = a.kinematics, b.kinematics, ora.get_grains()[:, :9]
    assert np.array_equal(ka, kb) and np.array_equal(ka, ko)
    assert np.array_equal(a.fhf, b.fhf) and np.array_equal(a.fhf, ora.get_fhf())
    for s in (a, b):
        cumul, neigh, _ = s.verlet()
        co, no, _, _ = ora.verlet()
        assert np.array_equal(cumul, co) and np.array_equal(neigh, no[:len(neigh)])
        s.close()
