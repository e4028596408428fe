"""GPU: the fluid tracers (lbmdem_tracer_*, lbmdem_write_tracers, lbmdem_set_tracer_output; include/lbmdem_hip.h) against their
numpy restatement (tests/tracer_util.py) over the handle's downloads: every position exactly equal, no tolerance."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import samples
import tracer_util as tu

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "golden", "dem_G6_4000steps")
AB_LIB = os.path.join(ROOT, "2d-lbm-dem_amd", "liblbmdem_hip_ab.so")
LX, LY = 256, 200
CLASSES = ("fluid", "one_grain", "mixed", "two_grains", "wall")


def g6():
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    return z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3


def cell_classes(obst, n):
    """-> dict class -> boolean [lx - 1][ly - 1] over the cells, by the owners of a cell's four nodes"""
    c = np.stack([obst[:-1, :-1], obst[1:, :-1], obst[:-1, 1:], obst[1:, 1:]])
    fluid, wall, grain = c == -1, c == n, (c >= 0) & (c < n)
    hi, lo = np.where(grain, c, -1).max(0), np.where(grain, c, n + 1).min(0)
    several = (grain.sum(0) >= 2) & (hi != lo)
    return dict(fluid=fluid.all(0), one_grain=grain.all(0) & (hi == lo), mixed=fluid.any(0) & grain.any(0) & ~wall.any(0) & ~several,
                two_grains=several & ~wall.any(0), wall=wall.any(0))


def class_seeds(obst, n, rng, per_class=64):
    """up to 64 tracers per cell class at random offsets inside their cells -> (xy, dict class -> indices into xy)"""
    xy, where, at = [], {}, 0
    for name, mask in cell_classes(obst, n).items():
        ij = np.argwhere(mask)
        ij = ij[rng.choice(len(ij), min(per_class, len(ij)), replace=False)] if len(ij) else ij
        xy.append(ij + rng.uniform(0.01, 0.99, (len(ij), 2)))
        where[name] = np.arange(at, at + len(ij))
        at += len(ij)
    return np.concatenate(xy), where


def advance_and_compare(sim, uv, times=1):
    """explicit advances, each against the restatement applied to the download taken just before it -> the last positions"""
    for _ in range(times):
        want = tu.advance(uv[0], uv[1], sim.tracers)
        sim.advance_tracers()
        got = sim.tracers
        bad = np.argwhere((got != want).any(1)).ravel()
        assert tu.same(got, want), (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    return got


@pytest.fixture(scope="module")
def coupled(pkg):
    """The G6 packing on 256 x 200 after five fluid periods and three more sub-steps. At that moment no cell of the map holds nodes
    of two different grains (the reduced discs of touching grains stay a node apart), so one grain is then set onto its nearest
    neighbour, 0.8 reduced radii sums from its centre, and the map is rasterised again (obst_construction): the state the
    advances read -- f, this map, these kinematics -- is what the downloads show. -> (sim, (ux, uy) of the restatement)"""
    r, x, y = g6()
    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        sim.renderScene(5 * sim.cfg.npDEM + 3)
        k = sim.kinematics
        d = np.hypot(k[:, 0] - k[0, 0], k[:, 1] - k[0, 1])
        d[0] = np.inf
        b = int(np.argmin(d))
        reach = 0.8 * sim.config().phys.reductionR * (r[0] + r[b])
        k[b, 0] = k[0, 0] + (k[b, 0] - k[0, 0]) / d[b] * reach
        k[b, 1] = k[0, 1] + (k[b, 1] - k[0, 1]) / d[b] * reach
        sim.kinematics = k
        sim.obst_construction()
        yield sim, tu.planes(sim)


def test_coupled_state(coupled):
    sim, uv = coupled
    obst = sim.obst
    rng = np.random.default_rng(41)
    xy, where = class_seeds(obst, sim.n, rng)
    for name in CLASSES:   # a condition on the input, not on the code
        assert len(where[name]) > 0, name
    nodes = np.argwhere(np.ones((LX - 1, LY - 1), bool))
    nodes = nodes[rng.choice(len(nodes), 32, replace=False)].astype(np.float64)   # exactly on nodes: a = b = 0
    on_grain = np.argwhere((obst >= 0) & (obst < sim.n))[:8].astype(np.float64)
    corners = np.array([[0., 0.], [LX - 1., 0.], [0., LY - 1.], [LX - 1., LY - 1.]])
    edge = np.array([[LX - 1 - 5e-13, 77.25], [100.5, LY - 1 - 5e-13]])
    assert edge[0, 0] < LX - 1 and edge[1, 1] < LY - 1
    start = np.concatenate([xy, nodes, on_grain, corners, edge])
    sim.set_tracers(start, automatic=False)
    assert np.array_equal(sim.tracers, start)
    end = advance_and_compare(sim, uv, times=3)
    assert sim.tracer_stats() == {"tracers": len(start), "advances": 3, "hook_advances": 0}
    moved = (end != start).any(1)
    for name in CLASSES[:4]:
        assert moved[where[name]].any(), name
    print(f"{len(start)} tracers, classes {[len(where[c]) for c in CLASSES]}, moved {int(moved.sum())}, "
          f"largest displacement {np.abs(end - start).max():.3e}")
    # the corners sit between lattice-edge walls and the fluid node diagonal to them: they stay inside the domain
    assert (end >= 0).all() and (end[:, 0] <= LX - 1).all() and (end[:, 1] <= LY - 1).all()
    # the sample: the restatement's velocity and the nearest node's owner
    s = sim.tracer_sample()
    want = tu.sample(uv[0], uv[1], obst, end)
    assert np.array_equal(s, want) and set(np.unique(s[:, 2])) >= {-1.0, float(sim.n)}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_tracer_counts(coupled, n):
    sim, uv = coupled
    rng = np.random.default_rng(n)
    start = rng.uniform(0.0, 1.0, (n, 2)) * (LX - 1, LY - 1)
    sim.set_tracers(start, automatic=False)
    assert sim.tracer_stats() == {"tracers": n, "advances": 0, "hook_advances": 0}   # (a new set counts from 0)
    advance_and_compare(sim, uv, times=2)
    assert sim.tracer_sample().shape == (n, 3)


def test_no_tracers_then_some_then_none(coupled):
    sim, uv = coupled
    sim.set_tracers(np.zeros((0, 2)))
    for _ in range(2):
        assert sim.tracers.shape == (0, 2) and sim.tracer_sample().shape == (0, 3)
        assert sim.tracer_stats() == {"tracers": 0, "advances": 0, "hook_advances": 0}
        sim.advance_tracers()   # nothing to do
        assert tuple(sim.tracers_tensor().shape) == (0, 2)
        sim.set_tracers(tu.grid_seeds(LX, LY, 3, 5), automatic=False)
        advance_and_compare(sim, uv)
        sim.set_tracers([])


@pytest.mark.parametrize("name", ["S_127x121", "S_13x61"])
def test_odd_lattices(pkg, name):
    """the short last tile of y, and a lattice narrower than a workgroup: grid seeds, two periods, explicit advances"""
    c = gu.CASES[name]
    a = gu.GpuAdapter(pkg, name)
    try:
        a.set_kinematics(gu.mg.shape_initial_kinematics(c))
        sim = a.sim
        sim.renderScene(2 * sim.cfg.npDEM)
        sim.set_tracers(tu.grid_seeds(sim.lx, sim.ly, 17, 19), automatic=False)
        start = sim.tracers
        end = advance_and_compare(sim, tu.planes(sim), times=2)
        assert (end != start).any()
    finally:
        a.sim.close()


def _plant(f, x, y, ux=0.0, uy=0.0):
    """node (x, y) at rest with rho = 1, then jx = ux and jy = uy exactly representable shifts of two opposite populations"""
    w = np.array([4. / 9] + [1. / 36, 1. / 9] * 4)
    f[x, y, :] = w
    f[x, y, 6] += 0.5 * ux; f[x, y, 2] -= 0.5 * ux   # jx = f5 + f6 + f7 - f1 - f2 - f3
    f[x, y, 8] += 0.5 * uy; f[x, y, 4] -= 0.5 * uy   # jy = f1 + f8 + f7 - f3 - f4 - f5


def test_clamp(pkg):
    """Fluid nodes next to each wall are given a velocity of 100 nodes per step towards it. A tracer a hair inside the far side of
    such a node's cell has a small U0, a midpoint still inside the cell and a large U1: it ends exactly on 0., lx - 1., ly - 1.
    (a tracer whose MIDPOINT is thrown onto the wall sees the wall's +0.0 there and stays: the contract's own consequence, checked
    through the restatement). Then a NaN in the fluid node (1, 1): every tracer whose cell touches it has a NaN U0, the midpoint
    (0, 0) -- whose cell touches it as well -- and ends on (0, 0); every other tracer equals the restatement. A NaN in a node of
    the interior sends the tracers around it to the midpoint (0, 0) and from there on by the corner's velocity: the restatement
    again. Nothing faults: the clamp is the code under test."""
    r, x, y = g6()
    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        sim.renderScene(2)
        f, obst = sim.f, sim.obst
        ys, xs = (150, 151, 152), (120, 121, 122)
        spots = [(1, yy) for yy in ys] + [(LX - 2, yy) for yy in ys] + [(xx, 1) for xx in xs] + [(xx, LY - 2) for xx in xs]
        assert all(obst[p] == -1 for p in spots)
        for yy in ys:
            _plant(f, 1, yy, ux=-100.0)
            _plant(f, LX - 2, yy, ux=100.0)
        for xx in xs:
            _plant(f, xx, 1, uy=-100.0)
            _plant(f, xx, LY - 2, uy=100.0)
        sim.f = f
        uv = tu.planes(sim)
        planted = np.array([uv[0][1, 151], -uv[0][LX - 2, 151], uv[1][121, 1], -uv[1][121, LY - 2]])
        assert (np.abs(planted + 100.0) < 1e-9).all(), planted   # (a condition on the input)
        hair = 2.0 ** -9
        thrown = np.array([[2 - hair, 150.5], [LX - 3 + hair, 151.25], [120.5, 2 - hair], [121.75, LY - 3 + hair]])
        stay = np.array([[1.5, 150.5], [LX - 2.5, 151.5], [121.5, 1.5], [120.5, LY - 2.5]])   # midpoint on the wall: U1 = 0
        rest = np.random.default_rng(7).uniform(0.0, 1.0, (200, 2)) * (LX - 1, LY - 1)
        sim.set_tracers(np.concatenate([thrown, stay, rest]), automatic=False)
        end = advance_and_compare(sim, uv)
        assert end[0, 0] == 0.0 and end[1, 0] == LX - 1.0 and end[2, 1] == 0.0 and end[3, 1] == LY - 1.0
        assert end[4, 0] == 1.5 and end[5, 0] == LX - 2.5 and end[6, 1] == 1.5 and end[7, 1] == LY - 2.5
        # a NaN in the fluid node (1, 1)
        assert obst[1, 1] == -1 and obst[90, 160] == -1
        for node, to_origin in (((1, 1), True), ((90, 160), False)):
            g = sim.f
            g[node[0], node[1], 3] = np.nan
            sim.f = g
            uv = tu.planes(sim)
            assert np.isnan(uv[0][node]) and np.isnan(uv[0]).sum() == (1 if to_origin else 2)
            around = np.array([[node[0] - 0.5, node[1] - 0.5], [node[0] + 0.5, node[1] - 0.5], [node[0] - 0.5, node[1] + 0.5],
                               [node[0] + 0.5, node[1] + 0.5], [float(node[0]), float(node[1])]])
            away = np.array([[node[0] + 1.5, node[1] + 0.5], [node[0] + 0.5, node[1] + 1.5], [node[0] + 1.5, node[1] + 1.5]])
            start = np.concatenate([around, away, rest])
            sim.set_tracers(start, automatic=False)
            end = advance_and_compare(sim, uv)
            if to_origin:
                assert not end[:5].any()
            assert np.array_equal(end[5:8], tu.advance(uv[0], uv[1], away)) and not np.isnan(end).any()
            touched = np.isnan(tu.velocity(uv[0], uv[1], start[:, 0], start[:, 1])[0])
            assert touched[:5].all() and not touched[5:8].any()


def _state(sim):
    return dict(f=sim.f, obst=sim.obst, kinematics=sim.kinematics, fhf=sim.fhf, nbsteps=sim.nbsteps)


def _same_state(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])]


def test_automatic_advance_is_the_advance_by_hand(pkg):
    r, x, y = g6()
    seeds = tu.grid_seeds(LX, LY, 24, 20)
    with pkg.LbmDem(LX, LY, r, x, y) as a, pkg.LbmDem(LX, LY, r, x, y) as b, pkg.LbmDem(LX, LY, r, x, y) as c:
        period = a.cfg.npDEM
        n = 4 * period + 5
        a.set_tracers(seeds, automatic=True)
        a.renderScene(n)
        assert a.dem_chain_stats()[0] > 0   # the multi-sub-step kernel ran
        b.set_tracers(seeds, automatic=False)
        for s in range(n):
            if s % period == 0:
                b.lbm_step()
                b.advance_tracers()
            if s % b.cfg.phys.updateVerlet == 0:
                b.initVerlet()
            b.dem_substep()
        c.renderScene(n)
        ta, tb = a.tracers, b.tracers
        assert tu.same(ta, tb) and (ta != seeds).any()
        assert a.tracer_stats() == {"tracers": len(seeds), "advances": 5, "hook_advances": 5}
        assert b.tracer_stats() == {"tracers": len(seeds), "advances": 5, "hook_advances": 0}
        sa, sb, sc = _state(a), _state(b), _state(c)
        assert _same_state(sa, sb) == [] and _same_state(sa, sc) == []   # tracers change nothing a step reads
        # automatic == 0: steps leave the set alone
        b.renderScene(period)
        assert np.array_equal(b.tracers, tb) and b.tracer_stats()["advances"] == 5


RECOVERY_SCRIPT = r"""
import os, sys
import numpy as np
root = os.getcwd()
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import __graft_entry__ as ge, samples, tracer_util as tu
pkg = ge.load_package()
lx, ly = 256, 160
r, x, y = samples.row_packing(lx, ly, 300, seed=5)
r, x1, x2 = samples.to_metres(r, x, y)
a = pkg.LbmDem(lx, ly, r, x1, x2)
b = pkg.LbmDem(lx, ly, r, x1, x2); b.set_dem_chain(0)
k = a.kinematics
k[:, 3:6] = np.random.default_rng(17).normal(0, 1, (len(k), 3)) * (0.05, 0.05, 30.0)
seeds = tu.grid_seeds(lx, ly, 31, 23)
for s in (a, b):
    s.kinematics = k
    s.set_tracers(seeds, automatic=True)
a.debug_chain_giveup(1)
for n in (37, 1, 12):
    a.renderScene(n); b.renderScene(n)
assert a.dem_chain_stats()[0] > 1 and a.dem_chain_recoveries() == 0, (a.dem_chain_stats(), a.dem_chain_recoveries())
ta, tb = a.tracers, b.tracers            # (the first download settles the handle)
assert a.dem_chain_recoveries() == 1 and b.dem_chain_recoveries() == 0
assert tu.same(ta, tb) and (ta != seeds).any(), int((ta != tb).any(1).sum())
fluid_steps = sum(1 for s in range(50) if s % a.cfg.npDEM == 0)
want = {"tracers": len(seeds), "advances": fluid_steps, "hook_advances": fluid_steps}
assert a.tracer_stats() == want and b.tracer_stats() == want, (a.tracer_stats(), b.tracer_stats(), want)
for what in ("f", "obst", "kinematics", "fhf"):
    assert np.array_equal(getattr(a, what), getattr(b, what)), what
print("recovered: tracers", a.tracer_stats())
"""


def test_give_up_recovery_repeats_the_advances_once():
    """as tests/test_gpu_chain_recovery.py does it, in a process of its own against the experiment build: launch 1 of the
    multi-sub-step kernel gives up on `a` (the library's own cooperative exit, no fault), `b` runs without that kernel, both with
    automatic tracers and runs of (37, 1, 12): one recovery on `a`, positions and counts equal"""
    assert os.path.exists(AB_LIB), "the experiment build (make -C 2d-lbm-dem_amd/csrc AB=1) is not there"
    env = dict(os.environ, LBMDEM_HIP_LIBRARY=AB_LIB)
    out = subprocess.run([sys.executable, "-c", RECOVERY_SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "recovered: tracers" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_rigid_translation(pkg):
    """One grain with v3 = 0 and a tracer deep inside it: every node of the tracer's cells holds u = (fl(v1 / c), fl(v2 / c)) --
    (v1 - (...) * 0) / c is v1 / c exactly, one rounding -- so an advance moves it by (v1, v2) / c.
    Bound, per axis and advance, with eps the spacing of doubles at 1 (unit roundoff eps / 2): a computed weight carries the
    roundings of 1. - a, 1. - b and their product, a term one more, and the three additions of four terms of one sign at most
    three more each: U = u (1 + t) with |t| <= 7 (eps / 2) / (1 - 7 eps / 2) < 4 eps, the true weights summing to 1. The same holds
    for U1 at the midpoint (still deep inside). px' = fl(px + U1) adds (eps / 2) |px'| <= (eps / 2) lx. After k advances
    |px_k - (px_0 + k u)| <= k (4 eps |u| + (eps / 2) lx); the comparison value fl(px_0 + fl(k u)) is off by at most eps lx.
    Nothing is fitted."""
    r, x, y = np.array([1.5e-3]), np.array([12.8e-3]), np.array([10.0e-3])
    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        sim.renderScene(2)
        k = sim.kinematics
        k[0, 3:6] = (0.013, -0.007, 0.0)
        sim.kinematics = k
        cfg = sim.config()
        g = sim.obst == 0
        ij = np.argwhere(g)
        centre = ij.mean(0)
        assert g[int(centre[0]) - 3:int(centre[0]) + 5, int(centre[1]) - 3:int(centre[1]) + 5].all()   # deep inside
        start = np.array([[int(centre[0]) + 0.37, int(centre[1]) + 0.81]])
        sim.set_tracers(start, automatic=False)
        u = np.array([0.013 / cfg.c, -0.007 / cfg.c])
        steps = 5
        assert np.abs(steps * u).max() < 1.0   # (it stays in the cells checked above)
        for _ in range(steps):
            sim.advance_tracers()
        end = sim.tracers
        eps = np.finfo(np.float64).eps
        bound = steps * (4 * eps * np.abs(u) + 0.5 * eps * LX) + eps * LX
        dev = np.abs(end[0] - (start[0] + steps * u))
        print(f"rigid translation: u {u}, deviation {dev}, bound {bound}")
        assert (u != 0).all() and (end[0] != start[0]).all() and (dev <= bound).all()
        assert np.array_equal(sim.tracer_sample()[0, 2:], [0.0])


def test_file_and_scene(pkg, tmp_path):
    r, x, y = g6()
    phys = pkg.derive(LX, LY, r).phys
    phys.stepFilm = 60
    seeds = tu.grid_seeds(LX, LY, 16, 12)
    da, dc, dw = tmp_path / "scene", tmp_path / "off", tmp_path / "one"
    for d in (da, dc, dw):
        d.mkdir()
    with pkg.LbmDem(LX, LY, r, x, y, physics=phys) as a, pkg.LbmDem(LX, LY, r, x, y, physics=phys) as c:
        a.set_tracers(seeds)
        a.set_tracer_output(True)
        _, res = a.run_scene(180, str(da))
        assert res["nfile"] == 3
        c.run_scene(180, str(dc))
        names = ["tracers%06d.vtk" % k for k in range(3)]
        assert sorted(n for n in os.listdir(da) if n.startswith("tracers")) == names
        assert sorted(os.listdir(dc)) == sorted(n for n in os.listdir(da) if not n.startswith("tracers")) and len(os.listdir(dc)) > 0
        for n in os.listdir(dc):   # every other file is what a run without tracers writes
            assert (dc / n).read_bytes() == (da / n).read_bytes(), n
        assert _same_state(_state(a), _state(c)) == []
        # the last frame's file is the present state's; the bytes are the restatement's over positions and sample
        xy, uvo = a.tracers, a.tracer_sample()
        uv = tu.planes(a)
        assert np.array_equal(uvo, tu.sample(uv[0], uv[1], a.obst, xy))
        a.write_tracers(str(dw), 12)
        want = tu.file_bytes(LX, xy, uvo)
        assert (dw / "tracers000012.vtk").read_bytes() == want == (da / names[2]).read_bytes()
        assert (da / names[0]).read_bytes() != (da / names[2]).read_bytes()
        assert a.tracer_stats()["hook_advances"] == len(range(0, 180, a.cfg.npDEM))
        # no tracers: a valid empty file
        c.write_tracers(str(dw), 13)
        assert (dw / "tracers000013.vtk").read_bytes() == tu.file_bytes(LX, np.zeros((0, 2)), np.zeros((0, 3)))
        with pytest.raises(pkg.LbmDemError, match="cannot open"):
            a.write_tracers(str(tmp_path / "not" / "there"), 0)


def test_torch_view_aliases_the_buffer(coupled):
    import torch
    sim, uv = coupled
    start = tu.grid_seeds(LX, LY, 9, 7)
    sim.set_tracers(start, automatic=False)
    t = sim.tracers_tensor()
    assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (len(start), 2)
    assert np.array_equal(t.cpu().numpy(), start)
    sim.advance_tracers()
    sim.sync()
    now = t.cpu().numpy()   # no other call into the library: the tensor IS the buffer
    assert np.array_equal(now, sim.tracers) and tu.same(now, tu.advance(uv[0], uv[1], start)) and (now != start).any()
    sim.set_tracers([])


def test_refusals(pkg, tmp_path):
    r, x, y = samples.to_metres(*samples.row_packing(LX, LY, 65, seed=29))
    L = pkg.load_library()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = tu.grid_seeds(LX, LY, 5, 4)
    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        for k, bad in ((3, np.nan), (0, -1e-9), (7, LX - 1 + 1e-9), (2, np.inf)):
            xy = good.copy()
            xy[k, 0] = bad
            with pytest.raises(pkg.LbmDemError, match=f"tracer {k} ") as e:
                sim.set_tracers(xy)
            assert e.value.code == -1
            xy = good.copy()
            xy[k, 1] = LY - 1 + 1e-9 if bad > 0 else bad
            with pytest.raises(pkg.LbmDemError, match=f"tracer {k} "):
                sim.set_tracers(xy)
        assert sim.tracer_stats()["tracers"] == 0
        with pytest.raises(pkg.LbmDemError, match=r"\(n, 2\)"):
            sim.set_tracers(np.zeros((4, 3)))
        assert L.lbmdem_tracer_set(sim._h, 4, None, 1) == -1 and L.lbmdem_tracer_set(sim._h, -1, vp(good), 1) == -1
        assert L.lbmdem_tracer_set(sim._h, 1 << 40, vp(good), 1) == -1
        sim.set_tracers(good)
        cnt = ctypes.c_long(-1)
        small = np.full((len(good) - 1, 2), 7.0)
        assert L.lbmdem_tracer_download(sim._h, vp(small), len(small), ctypes.byref(cnt)) == -1
        assert cnt.value == len(good) and (small == 7.0).all() and b"buffer holds" in L.lbmdem_last_error()
        small3 = np.full((len(good) - 1, 3), 7.0)
        cnt.value = -1
        assert L.lbmdem_tracer_sample(sim._h, vp(small3), len(small3), ctypes.byref(cnt)) == -1
        assert cnt.value == len(good) and (small3 == 7.0).all()
        assert L.lbmdem_tracer_download(sim._h, vp(small), len(small), None) == -1
        assert L.lbmdem_tracer_download(sim._h, None, 5, ctypes.byref(cnt)) == -1
        assert L.lbmdem_tracer_stats(sim._h, None) == -1 and L.lbmdem_tracer_device(sim._h, None) == -1
        assert L.lbmdem_write_tracers(sim._h, None, 0) == -1
        with pytest.raises(pkg.LbmDemError, match="tracers"):   # distributed grains are enabled at a fluid-step boundary
            sim.dist_enable()
        sim.set_tracers([])
        sim.set_tracer_output(True)
        with pytest.raises(pkg.LbmDemError, match="lbmdem_set_tracer_output"):
            sim.dist_enable()
        sim.set_tracer_output(False)
        sim.dist_enable()
        for call in (lambda: sim.set_tracers(good), sim.advance_tracers, lambda: sim.tracers, sim.tracer_sample, sim.tracer_stats,
                     sim.set_tracer_output, lambda: sim.write_tracers(str(tmp_path), 0)):
            with pytest.raises(pkg.LbmDemError, match="distributed"):
                call()
    with pkg.LbmDem(LX, LY, r, x, y, strip=(128, 256), halo=12) as strip:
        for call in (lambda: strip.set_tracers(good), strip.advance_tracers, lambda: strip.tracers, strip.tracer_sample,
                     strip.tracer_stats, strip.tracers_tensor, strip.set_tracer_output, lambda: strip.write_tracers(str(tmp_path), 0)):
            with pytest.raises(pkg.LbmDemError, match="strip"):
                call()
    with pkg.LbmDem(LX, LY, r, x, y, precision="f32") as sp:
        for call in (lambda: sp.set_tracers(good), sp.advance_tracers, lambda: sp.tracers, sp.tracer_sample, sp.tracer_stats,
                     sp.set_tracer_output, lambda: sp.write_tracers(str(tmp_path), 0)):
            with pytest.raises(pkg.LbmDemError, match="single-precision"):
                call()
    assert os.listdir(tmp_path) == []


def test_checkpoints_do_not_carry_tracers(pkg, tmp_path):
    r, x, y = samples.to_metres(*samples.row_packing(LX, LY, 65, seed=29))
    with pkg.LbmDem(LX, LY, r, x, y) as a, pkg.LbmDem(LX, LY, r, x, y) as b:
        a.set_tracers(tu.grid_seeds(LX, LY, 8, 8))
        a.set_tracer_output(True)
        a.renderScene(30); b.renderScene(30)
        assert a.tracer_stats()["hook_advances"] == len(range(0, 30, a.cfg.npDEM)) > 1
        a.checkpoint_save(str(tmp_path / "a.ckpt")); b.checkpoint_save(str(tmp_path / "b.ckpt"))
        assert (tmp_path / "a.ckpt").read_bytes() == (tmp_path / "b.ckpt").read_bytes()
        assert a.tracer_stats()["tracers"] == 64   # (saving leaves the set alone)
    back = pkg.LbmDem.checkpoint_load(str(tmp_path / "a.ckpt"))
    try:
        assert back.tracer_stats() == {"tracers": 0, "advances": 0, "hook_advances": 0} and back.tracers.shape == (0, 2)
        back.renderScene(12)
        assert back.tracer_stats()["advances"] == 0
    finally:
        back.close()
