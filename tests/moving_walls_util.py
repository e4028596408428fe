"""Shared by the tests of the analyses on handles whose walls move (tests/test_moving_walls_host.py on the CPU,
tests/test_gpu_moving_walls.py on the device): the three scenes, the sub-steps that are looked at, and the inequalities that give
the comparisons their teeth, each a function of restatements alone (voronoi_util, contacts_util, vib_util.VibOracle and
lbmdem_vibration_schedule), so that the CPU module can evaluate them without a device.

Scenes
  shaken   the packing of test_gpu_vibration._inputs("G4") (171 grains of G4_coupled_256x200 plus one grain pressed against each of
           the left, right and top walls: 174), 256 x 200, with test_gpu_vibration._shaker's physics: freq * t sweeps 1.4 rad over
           250 sub-steps, the left wall travels about 4 nodes, and dtt = 1 s keeps the right and top walls at the lattice's edge.
  reset    the same packing with the reference's own physics but dtt: 0 (the first rebuild by hand puts Mdx and Mhy at ten times
           the lattice) or RESET_DTT_STEPS sub-steps (the rebuild by hand after RESET_RUN_STEPS sub-steps does the same in mid-run).
  small    small_scene(lx, ly, n): n grains on 65 x 17 or 61 x 59, every other one pressed against the left or the right wall
           (ceil(n / 2) of them, left and right in turn), the rest on a jittered grid between them, no two overlapping. With
           small_physics one lbmdem_move_walls moves both side walls by about one node. Never stepped.
  run      run_scene_inputs(): ten grains on 61 x 59, shaken through the first DEM event (test 5)."""
import math

import numpy as np

import contacts_util as cu
import golden_util as gu
import samples
import vib_util as vu
import voronoi_util as vo

N = 250                                  # >= 3 fluid steps (npDEM = 12) and 3 list rebuilds (0, 100, 200), as test_gpu_vibration's
PIECES = (1, 36, 63, 100, 50)            # test_gpu_vibration's: runs that end on and off fluid steps and rebuilds
assert sum(PIECES) == N == 250
# the last sub-steps whose records are compared (npDEM = 12, updateVerlet = 100 in the shaken scene): a rebuild (100, 200), a fluid
# step (12, 24, 240), neither (5, 31, 249). The grain pressed against the right wall leaves it after sub-step 32 and the one at the
# top wall between 55 and 207, so the early ones are there for those two walls; the left wall reaches the packing from 188 on
CONTACT_SUBSTEPS = (5, 12, 24, 31, 100, 200, 240, 249)
SMALL_SHAPES = ((65, 17), (61, 59))
SMALL_COUNTS = (1, 63, 64, 65)
RESET_DTT_STEPS, RESET_RUN_STEPS = 230, 250   # rebuilds at 0, 100, 200 lie before dtt; the one by hand at 250 behind it
BIT_L, BIT_R = 8, 2                      # lbmdem_voronoi's wall bits: a face on the left (source -4) and on the right wall (-2)


def shaken_inputs():
    """test_gpu_vibration._inputs("G4"), restated here so that nothing on the CPU imports a device test -> lx, ly, r, x1, x2"""
    lx, ly = 256, 200
    r, x1, x2 = gu.inputs_m("G4_coupled_256x200")
    r, x1, x2 = vu.with_wall_grains(r, x1, x2, lx, ly)
    return lx, ly, r, x1, x2


def shaken_physics(pkg, n=N, amp_nodes=4.0):
    """test_gpu_vibration._shaker: freq * t sweeps 1.4 rad over n sub-steps, the left wall moves about amp_nodes nodes"""
    lx, ly, r, _, _ = shaken_inputs()
    dt = pkg.derive(lx, ly, r).dt
    phys = vu.physics(pkg, freq=1.4 / (n * dt), amp=0.0)
    phys.amp = amp_nodes * 1e-4 / (0.5 * n)
    return phys


def voronoi_rcut(r):
    """3.3 mean diameters: the cutoff the Voronoi tests use"""
    return 3.3 * 2.0 * float(np.mean(r))


def small_scene(lx, ly, n, seed=0, press=0.1):
    """-> r, x, y in metres; the first ceil(n / 2) grains touch a side wall (even ones the left, odd ones the right), `press` of
    their radius into it. These scenes are looked at, not stepped: pressed a tenth into the walls the grains are shot off them and
    the state is NaN within 1500 sub-steps on the oracle"""
    W, H = 1e-3 * lx / 10, 1e-3 * ly / 10
    nw = (n + 1) // 2
    per_wall = (nw + 1) // 2
    pitch = H / per_wall
    rw = min(0.3e-3, 0.42 * pitch)
    r, x, y = [], [], []
    for k in range(nw):
        left = k % 2 == 0
        r.append(rw)
        x.append((1.0 - press) * rw if left else W - (1.0 - press) * rw)
        y.append((k // 2 + 0.5) * pitch)
    rest = n - nw
    if rest:
        x0, x1 = 2 * rw + 0.1e-3, W - 2 * rw - 0.1e-3
        cols = max(1, int(math.ceil(math.sqrt(rest * (x1 - x0) / H))))
        rows = -(-rest // cols)
        px, py = (x1 - x0) / cols, H / rows
        rng = np.random.default_rng(seed + 1000 * n + lx)
        for k in range(rest):
            i, j = k % cols, k // cols
            rad = rng.uniform(0.25, 0.4) * min(px, py)
            room = 0.5 * min(px, py) - rad
            r.append(rad)
            x.append(x0 + (i + 0.5) * px + rng.uniform(-1, 1) * 0.9 * room)
            y.append((j + 0.5) * py + rng.uniform(-1, 1) * 0.9 * room)
    return np.array(r), np.array(x), np.array(y)


def small_physics(pkg, lx, ly, r, amp=1.2e-4):
    """freq * dt = 1 rad: the first lbmdem_move_walls moves both side walls by amp * sin(1), about one node; dtt = 1 s keeps the
    right and the top wall at the lattice's edge"""
    dt = pkg.derive(lx, ly, r).dt
    return vu.physics(pkg, freq=1.0 / dt, amp=amp)


def run_scene_inputs():
    """test 5's scene: the 61 x 59 packing of the shape sweep (as test_gpu_pores.shape_scene makes it: ten grains in rows, 0.05 mm
    from the left wall). small_scene is not stepped: its grains start pressed into the walls, are shot off them and are out of
    every contact long before the first DEM event. -> lx, ly, r, x, y in metres"""
    lx, ly = SMALL_SHAPES[1]
    return (lx, ly) + tuple(samples.to_metres(*samples.row_packing(lx, ly, 400, seed=1000 * lx + ly, margin=0.05)))


def wall_touchers(r, x, lx):
    """(grains overlapping the left wall at 0, grains overlapping the right wall at the lattice's edge)"""
    W = 1e-3 * lx / 10
    return np.nonzero(x - r < 0)[0], np.nonzero(W - x - r < 0)[0]


def overlaps(r, x, y):
    d = np.hypot(x[None, :] - x[:, None], y[None, :] - y[:, None]) - (r[None, :] + r[:, None])
    return int((d[~np.eye(len(r), dtype=bool)] < 0).sum()) // 2


# ---- the Voronoi comparison's teeth ----

def cells_that_differ(A, B):
    """grains whose restated cell differs between two restatements: the area's bits or the list of faces"""
    out = []
    for i in range(len(A["grains"])):
        fa = A["fsrc"][A["foff"][i]:A["foff"][i + 1]].tolist()
        fb = B["fsrc"][B["foff"][i]:B["foff"][i + 1]].tolist()
        if fa != fb or not vo.same_bits(A["grains"]["area"][i], B["grains"]["area"][i]):
            out.append(i)
    return out


def records_that_differ(A, B):
    """grains for which two restatements differ in anything: a measure's bits, a count, a flag, a face or its length"""
    out = []
    for i in range(len(A["grains"])):
        a, b = slice(A["foff"][i], A["foff"][i + 1]), slice(B["foff"][i], B["foff"][i + 1])
        if (A["grains"][i].tobytes() != B["grains"][i].tobytes() or A["fsrc"][a].tolist() != B["fsrc"][b].tolist()
                or A["flen"][a].tobytes() != B["flen"][b].tobytes()):
            out.append(i)
    return out


def voronoi_teeth(x, y, r, box0, box1, dx, rcut):
    """the restatement with the final walls box1 against the one with the initial walls box0 -> the figures, after asserting what
    test 1 relies on: Mgx has moved by more than a node, five grains or more own a left-wall face, five or more a right-wall face,
    and five cells or more are not the cells of the initial walls"""
    now, then = vo.restate(x, y, r, box1, rcut), vo.restate(x, y, r, box0, rcut)
    left = int((now["grains"]["walls"] & BIT_L > 0).sum())
    right = int((now["grains"]["walls"] & BIT_R > 0).sum())
    differ = cells_that_differ(now, then)
    figures = dict(shift_nodes=(box1[0] - box0[0]) / dx, left=left, right=right, differ=len(differ))
    assert box1[0] - box0[0] > dx, figures
    assert left >= 5 and right >= 5 and len(differ) >= 5, figures
    return figures


# ---- the contact comparison's teeth ----

def config_with(pkg, cfg, t, Mgx, Mdx, Mhy=None):
    c = pkg.Config.from_buffer_copy(cfg)
    c.phys.t, c.Mgx, c.Mdx = float(t), float(Mgx), float(Mdx)
    if Mhy is not None:
        c.Mhy = float(Mhy)
    return c


def restated_records(pkg, cfg, sched_row, Mhy, pre, r, cumul, neigh, wf, film=False, Mgx=None):
    """the records of the sub-step that started from `pre` with the walls of lbmdem_vibration_schedule's row (t, Mgx, Mdx,
    wallT_vel); Mgx: another left wall, for the teeth"""
    c = config_with(pkg, cfg, sched_row[0], sched_row[1] if Mgx is None else Mgx, sched_row[2], Mhy)
    P = cu.params_of_config(c, wallT_vel=float(sched_row[3]))
    return cu.restate(pre, r, cu.pairs_of_list(cumul, neigh), wf, P, film)


def wall_counts(rec):
    return {name: int((rec["j"] == code).sum()) for name, code in (("left", cu.WALL_L), ("right", cu.WALL_R), ("top", cu.WALL_T))}


def left_dn_differs(rec, rec_initial_wall):
    """a left-wall record whose dn is not the one the same law gives with the initial Mgx (same grain, or no such record there)"""
    a = rec[rec["j"] == cu.WALL_L]
    b = {int(c["i"]): c["dn"] for c in rec_initial_wall[rec_initial_wall["j"] == cu.WALL_L]}
    return any(int(c["i"]) not in b or np.float64(c["dn"]).tobytes() != np.float64(b[int(c["i"])]).tobytes() for c in a)
