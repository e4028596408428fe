"""CPU: the harness of tests/test_gpu_moving_walls.py. The restatement of the Voronoi cells with boxes that do not start at the
origin or reach ten times the lattice (the cells still tile the box), the inequalities that give the device comparisons their teeth
-- evaluated from the restatements, vib_util.VibOracle and lbmdem_vibration_schedule alone --, and the small scenes against what
their docstrings say. No device is touched."""
import numpy as np
import pytest

import contacts_util as cu
import moving_walls_util as mw
import vib_util as vu
import voronoi_util as vo

EPS = float(np.finfo(np.float64).eps)


@pytest.mark.parametrize("box", ["shifted", "tenfold", "both"])
def test_cells_tile_a_box_that_has_moved(box):
    """rcut beyond every distance: every neighbour's line is there, every cell is complete, and the areas add up to W * H. The
    bound: a cell's area is a sum of nverts products of coordinates no larger than W and H, each with a relative error of a few
    eps, so the n areas together stay within n * eps * W * H; the residuals measured are 0 (shifted), 0 (tenfold) and 0.045 (both)
    of that bound."""
    lx, ly = mw.SMALL_SHAPES[1]
    W, H = 1e-3 * lx / 10, 1e-3 * ly / 10
    # twelve grains, three of them touching the left wall at 0: with every other grain for a neighbour no cell passes the 32
    # vertices a cell may have on its way (65 grains, half of them along the walls, do: two cells of small_scene overflow)
    rng = np.random.default_rng(12)
    r = rng.uniform(0.2e-3, 0.5e-3, 12)
    x, y = rng.uniform(0.6e-3, W - 0.6e-3, 12), rng.uniform(0.6e-3, H - 0.6e-3, 12)
    x[:3] = 0.9 * r[:3]
    gx = 0.93e-4 if box != "tenfold" else 0.0
    far = 10.0 if box != "shifted" else 1.0
    b = (gx, far * W + gx, 0.0, far * H)
    R = vo.restate(x, y, r, b, 1.0)
    g = R["grains"]
    assert R["counts"]["complete"] == R["counts"]["cells"] == len(r) and R["counts"]["overflowed"] == R["counts"]["empty"] == 0
    area = (b[1] - b[0]) * (b[3] - b[2])
    total = float(np.sum(g["area"]))
    residual = abs(total - area)
    print("box %s: sum of areas %.17g, W * H %.17g, residual %.3g of the bound" % (box, total, area, residual / (len(r) * EPS * area)))
    assert residual <= len(r) * EPS * area
    assert (g["walls"] & mw.BIT_L > 0).sum() >= 3 and (g["walls"] & mw.BIT_R > 0).sum() >= 1


@pytest.fixture(scope="module")
def shaken(pkg):
    """the shaken scene on the oracle, sub-step by sub-step: the walls of every sub-step, the restated records of the sub-steps
    the device test looks at (with the sub-step's walls, and with the initial left wall), the state behind every piece"""
    lx, ly, r, x1, x2 = mw.shaken_inputs()
    phys = mw.shaken_physics(pkg)
    cfg = pkg.derive(lx, ly, r, physics=phys)
    ora = vu.VibOracle(lx, ly, r, x1, x2, phys=phys)
    sched = pkg.vibration_schedule(cfg, 0, mw.N)
    records, pieces = {}, {}
    ends = set(np.cumsum(mw.PIECES).tolist())
    for s in range(mw.N):
        pre = ora.get_grains()[:, :9].copy()
        ora.vib_steps(1)
        w = ora.walls()
        assert (w["t"], w["Mgx"], w["Mdx"]) == tuple(sched[s, :3]), s      # the schedule is the oracle's walls
        if s in mw.CONTACT_SUBSTEPS:
            cumul, neigh, _, lists = ora.verlet()
            wf = cu.wallflags_of_lists(len(r), lists)
            args = (pkg, cfg, sched[s], w["Mhy"], pre, r, cumul, neigh, wf)
            records[s] = (mw.restated_records(*args)[0], mw.restated_records(*args, Mgx=cfg.Mgx)[0])
        if s + 1 in ends:
            g = ora.get_grains()
            pieces[s + 1] = (g[:, 0].copy(), g[:, 1].copy(), (w["Mgx"], w["Mdx"], w["Mby"], w["Mhy"]))
    return dict(cfg=cfg, r=r, records=records, pieces=pieces, box0=(cfg.Mgx, cfg.Mdx, cfg.Mby, cfg.Mhy))


def test_voronoi_comparison_has_teeth(shaken):
    """test 1's: by the end Mgx has moved by more than dx, five grains or more own a left-wall face and five or more a right-wall
    face, and five cells or more are not those of the initial walls. Measured: 4.74 nodes, 12, 10 and 66 of 174 cells."""
    S = shaken
    x, y, box1 = S["pieces"][mw.N]
    figures = mw.voronoi_teeth(x, y, S["r"], S["box0"], box1, S["cfg"].dx, mw.voronoi_rcut(S["r"]))
    print(figures)
    # ... and the right and the top wall stay at the lattice's edge but for the right wall's drift since the last rebuild
    assert box1[3] == S["box0"][3] and 0 < box1[1] - S["box0"][1] < 3 * S["cfg"].dx
    # every piece ends with walls of its own
    assert len({S["pieces"][k][2] for k in S["pieces"]}) == len(mw.PIECES)


def test_contact_comparison_has_teeth(shaken):
    """test 3's: over the sub-steps looked at, three records or more at each of the left, the right and the top wall, and a
    left-wall dn that the initial Mgx does not give. The sub-steps end on rebuilds (100, 200), on fluid steps (12, 24, 240) and on
    neither. Measured: 32 left, 4 right, 6 top; the left wall's records of sub-steps 200, 240 and 249 differ."""
    S = shaken
    npdem, uv = S["cfg"].npDEM, S["cfg"].phys.updateVerlet
    subs = mw.CONTACT_SUBSTEPS
    assert any(s % uv == 0 for s in subs) and any(s % npdem == 0 for s in subs) and any(s % uv and s % npdem for s in subs)
    assert all(s % S["cfg"].phys.stepFilm for s in subs)                   # none of them takes the film law
    total = dict(left=0, right=0, top=0)
    told_apart = []
    for s in subs:
        rec, rec0 = S["records"][s]
        for name, k in mw.wall_counts(rec).items():
            total[name] += k
        if mw.left_dn_differs(rec, rec0):
            told_apart.append(s)
    print(total, told_apart)
    assert min(total.values()) >= 3, total
    assert len(told_apart) >= 1


@pytest.mark.parametrize("n", mw.SMALL_COUNTS)
@pytest.mark.parametrize("lx,ly", mw.SMALL_SHAPES)
def test_small_scenes_are_what_their_docstring_says(pkg, lx, ly, n):
    r, x, y = mw.small_scene(lx, ly, n)
    W, H = 1e-3 * lx / 10, 1e-3 * ly / 10
    assert len(r) == len(x) == len(y) == n <= 65
    left, right = mw.wall_touchers(r, x, lx)
    nw = (n + 1) // 2
    assert len(left) == (nw + 1) // 2 and len(right) == nw // 2 and sorted(left.tolist() + right.tolist()) == list(range(nw))
    assert mw.overlaps(r, x, y) == 0
    assert (x > 0).all() and (x < W).all() and (y - r > 0).all() and (y + r < H).all()
    # one move by hand: both side walls about a node further, Mgx no multiple of dx, and cells that can tell
    cfg = pkg.derive(lx, ly, r, physics=mw.small_physics(pkg, lx, ly, r))
    row = pkg.vibration_schedule(cfg, 1, 1)[0]          # (sub-step 1: no rebuild resets the right wall in this row)
    shift = row[1] - cfg.Mgx
    assert 0.8 * cfg.dx < shift < 1.2 * cfg.dx and row[2] > cfg.Mdx
    rcut = 10.0 * 2.0 * float(r.mean())
    box0, box1 = (cfg.Mgx, cfg.Mdx, cfg.Mby, cfg.Mhy), (row[1], row[2], cfg.Mby, cfg.Mhy)
    # (a single grain's cell is the box: the same area and faces wherever the box lies, another R2)
    assert len(mw.records_that_differ(vo.restate(x, y, r, box1, rcut), vo.restate(x, y, r, box0, rcut))) >= min(n, 2)


def test_run_scene_case_stays_finite_and_its_walls_move(pkg):
    """test 5's scene (run_scene_inputs, the host driver's --vib-freq 60 --vib-amp 2e-7, dtt = 0) on the oracle through the
    sub-step of the first DEM event: finite, the left wall a node from where it began (measured: 1.08 nodes), Mdx and Mhy at ten
    times the lattice, a contact record at the event (measured: one pair), and cells that are not those of the initial walls"""
    lx, ly, r, x, y = mw.run_scene_inputs()
    assert len(r) <= 65 and mw.overlaps(r, x, y) >= 1            # (some pairs of the row packing touch from the start)
    phys = vu.physics(pkg, freq=60.0, amp=2e-7, dtt=0.0)
    cfg = pkg.derive(lx, ly, r, physics=phys)
    ora = vu.VibOracle(lx, ly, r, x, y, phys=phys)
    ora.vib_steps(3999)
    pre = ora.get_grains()[:, :9].copy()
    ora.vib_steps(1)
    w, g = ora.walls(), ora.get_grains()
    assert np.isfinite(g).all() and np.isfinite(ora.get_f()).all()
    assert w["Mgx"] - cfg.Mgx > cfg.dx and w["Mdx"] > 5 * 1e-4 * lx and w["Mhy"] == 1e-3 * ly
    row = pkg.vibration_schedule(cfg, 0, 4000)[-1]
    assert (w["t"], w["Mgx"]) == tuple(row[:2])
    cumul, neigh, _, lists = ora.verlet()
    rec, _ = mw.restated_records(pkg, cfg, row, w["Mhy"], pre, r, cumul, neigh, cu.wallflags_of_lists(len(r), lists))
    rcut = 5.0 * 2.0 * float(r.mean())
    box0, box1 = (cfg.Mgx, cfg.Mdx, cfg.Mby, cfg.Mhy), (w["Mgx"], w["Mdx"], w["Mby"], w["Mhy"])
    differ = mw.cells_that_differ(vo.restate(g[:, 0], g[:, 1], r, box1, rcut), vo.restate(g[:, 0], g[:, 1], r, box0, rcut))
    print(len(rec), (w["Mgx"] - cfg.Mgx) / cfg.dx, len(differ))
    assert len(rec) >= 1 and len(differ) >= 3
