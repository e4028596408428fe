"""GPU: the analyses that read the four DEM walls, on handles whose walls move -- inside a run (vibrating side walls: vib_commit
behind a launch of the multi-sub-step kernel, vib_advance in front of a single sub-step), by hand (lbmdem_move_walls) and at a list
rebuild by hand (lbmdem_verlet_rebuild, whose VerletWall puts the right and the top wall at the lattice's edge or at ten times it).
Every output against its restatement fed walls(), integers by array_equal and doubles on the bits; the scenes, the sub-steps looked
at and the inequalities that give the comparisons their teeth are tests/moving_walls_util.py's, and tests/test_moving_walls_host.py
evaluates the same inequalities without a device.

A wall that takes another value outside a sub-step makes stale what was computed with the walls as they were (the handle's
walls_moved stamp): the Voronoi readers, the contact export and the clusters refuse until their next compute or table sub-step; the
structure readers, which read no wall, go on answering; a move that changes no wall's bits changes nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

import coarse_util as co
import contacts_util as cu
import moving_walls_util as mw
import pore_stack_util as ps
import scalar_util as su
import structure_util as st
import tracer_util as tu
import vib_util as vu
import voronoi_util as vo
from test_gpu_clusters import check as cluster_check
from test_gpu_structure import check as structure_check
from test_gpu_voronoi import DOUBLES, INTS, NO_COMPUTE, READERS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
AB_LIB = os.path.join(ROOT, "2d-lbm-dem_amd", "liblbmdem_hip_ab.so")
NO_TABLE = "the last sub-step was no table sub-step"
WALL_MOVED = "%s: a wall has been moved since the last table sub-step (lbmdem_move_walls)"
NO_CLUSTERS = "%s: no lbmdem_cluster_compute has been made for the last table sub-step"


def box_of(sim):
    w = sim.walls()
    return w["Mgx"], w["Mdx"], w["Mby"], w["Mhy"]


def centres(sim):
    k = sim.kinematics
    return k[:, 0], k[:, 1]


def compare_voronoi(sim, R, counts=None):
    """the readers of the last compute (and its counters, where given) against the restatement R"""
    if counts is not None:
        assert counts == R["counts"], (counts, R["counts"])
    g = sim.voronoi_grains()
    for name in INTS:
        assert g[name].dtype == np.int32 and np.array_equal(g[name], R["grains"][name]), (name, np.nonzero(g[name] != R["grains"][name])[0][:5])
    for name in DOUBLES:
        assert vo.same_bits(g[name], R["grains"][name]), (name, np.nonzero(g[name] != R["grains"][name])[0][:5])
    off, src, length = sim.voronoi_faces()
    assert np.array_equal(off, R["foff"]) and np.array_equal(src, R["fsrc"]) and vo.same_bits(length, R["flen"])
    tv = sim.voronoi_tensors()
    for name in vo.VORONOI_DTYPE.names:
        assert np.array_equal(tv[name].cpu().numpy().view(np.uint8), np.ascontiguousarray(g[name]).view(np.uint8)), name


def voronoi_refused(pkg, sim):
    for who, call in zip(READERS, (sim.voronoi_grains, sim.voronoi_tensors, sim.voronoi_faces)):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1 and sim._L.lbmdem_last_error().decode() == NO_COMPUTE % who


def structure_snapshot(sim):
    off, nbr = sim.structure_neighbours()
    return sim.structure_grains().tobytes(), sim.structure_hist().tobytes(), off.tobytes(), nbr.tobytes()


# ---- 1. Voronoi after the walls have moved inside a run ----

@pytest.mark.parametrize("chain", [True, False], ids=["chain", "one_launch_per_substep"])
def test_voronoi_follows_the_walls_of_a_shaken_run(pkg, chain):
    """the shaken scene in test_gpu_vibration's uneven pieces; after each, structure + voronoi and every reader against the
    restatement with box = walls(). chain: the walls come from vib_commit; else from vib_advance"""
    lx, ly, r, x1, x2 = mw.shaken_inputs()
    rcut = mw.voronoi_rcut(r)
    with pkg.LbmDem(lx, ly, r, x1, x2, physics=mw.shaken_physics(pkg)) as sim:
        if not chain:
            sim.set_dem_chain(0)
        sim.set_vibration(True)
        box0 = box_of(sim)
        for n in mw.PIECES:
            sim.renderScene(n)
            x, y = centres(sim)
            compare_voronoi(sim, vo.restate(x, y, r, box_of(sim), rcut), sim.voronoi(rcut))
        # the comparison has teeth: the restatement with the walls the handle started with is another one
        print(mw.voronoi_teeth(x, y, r, box0, box_of(sim), sim.cfg.dx, rcut))
        assert (sim.dem_chain_stats()[0] > 0) == chain


# ---- 2. the guards ----

def guards(pkg, sim, r, rcut, move, tmp_path):
    """structure and Voronoi, then `move`, which changes a wall: every Voronoi reader is refused, the structure readers are not, a new
    compute answers for the new box and lbmdem_write_voronoi writes cells and a box_area of the same walls -> (box before, after)"""
    x, y = centres(sim)
    structure_check(sim, st.Restatement(x, y, r), rcut, 7, 1.2)
    box0 = box_of(sim)
    R0 = vo.restate(x, y, r, box0, rcut)
    compare_voronoi(sim, R0, sim.voronoi())
    listed = structure_snapshot(sim)
    move()
    box1 = box_of(sim)
    assert box1 != box0
    voronoi_refused(pkg, sim)
    assert structure_snapshot(sim) == listed                  # they read no wall: still valid, and the same bytes
    x1, y1 = centres(sim)
    assert vo.same_bits(x1, x) and vo.same_bits(y1, y)        # no grain has moved
    R1 = vo.restate(x, y, r, box1, rcut)
    assert mw.records_that_differ(R1, R0)                     # (the restatement can tell the two boxes apart)
    compare_voronoi(sim, R1, sim.voronoi())                   # the neighbour list is still good: the compute alone
    compare_voronoi(sim, R1, sim.voronoi(rcut))               # ... and behind a fresh structure compute
    sim.write_voronoi(str(tmp_path), 0, rcut)
    want = vo.files_text(R1["grains"], rcut, R1["counts"], sim.nbsteps * sim.cfg.dt, box1[1] - box1[0], box1[3] - box1[2])
    assert (tmp_path / "voronoi000000.dat").read_text() == want[0]
    assert (tmp_path / "voronoi.data").read_text() == vo.DATA_HEADER + want[1]
    compare_voronoi(sim, R1)
    return box0, box1


@pytest.mark.parametrize("n", mw.SMALL_COUNTS)
@pytest.mark.parametrize("lx,ly", mw.SMALL_SHAPES)
def test_guards_after_a_move_by_hand(pkg, tmp_path, lx, ly, n):
    """the small scenes: lbmdem_move_walls moves both side walls by about a node, past the edge of the grains that touch them"""
    r, x, y = mw.small_scene(lx, ly, n)
    with pkg.LbmDem(lx, ly, r, x, y, physics=mw.small_physics(pkg, lx, ly, r)) as sim:
        sim.set_vibration(True)
        box0, box1 = guards(pkg, sim, r, 10.0 * 2.0 * float(r.mean()), sim.move_walls, tmp_path)
        assert 0.8 * sim.cfg.dx < box1[0] - box0[0] < 1.2 * sim.cfg.dx and box1[1] > box0[1]
        assert box1[0] / sim.cfg.dx != round(box1[0] / sim.cfg.dx)          # Mgx is no multiple of dx


@pytest.mark.parametrize("when", ["fresh", "mid_run"])
def test_guards_after_a_rebuild_by_hand(pkg, tmp_path, when):
    """the reset scene: initVerlet() by hand puts Mdx and Mhy at ten times the lattice -- on a fresh default handle (dtt = 0), and in
    mid-run behind dtt. A second rebuild leaves all four where they are, and the results readable"""
    lx, ly, r, x1, x2 = mw.shaken_inputs()
    rcut = mw.voronoi_rcut(r)
    dt = pkg.derive(lx, ly, r).dt
    phys = vu.physics(pkg, freq=5., amp=4.e-4, dtt=0.0 if when == "fresh" else mw.RESET_DTT_STEPS * dt)
    with pkg.LbmDem(lx, ly, r, x1, x2, physics=phys) as sim:
        if when == "mid_run":
            sim.renderScene(mw.RESET_RUN_STEPS)           # rebuilds at 0, 100 and 200, all before dtt: the walls stay
            assert box_of(sim) == (0.0, 1e-3 * lx / 10, 0.0, 1e-3 * ly / 10)
        box0, box1 = guards(pkg, sim, r, rcut, sim.initVerlet, tmp_path)
        assert box1 == (0.0, 1e-3 * lx, 0.0, 1e-3 * ly) and box0 == (0.0, 1e-3 * lx / 10, 0.0, 1e-3 * ly / 10)
        x, y = centres(sim)
        R1 = vo.restate(x, y, r, box1, rcut)
        sim.initVerlet()
        assert box_of(sim) == box1
        compare_voronoi(sim, R1)


def test_a_move_that_changes_no_wall_keeps_the_results(pkg):
    """amp = 0: lbmdem_move_walls advances the clock and leaves the walls; dtt = 1 s: a rebuild by hand puts Mdx and Mhy where
    they are already"""
    lx, ly = mw.SMALL_SHAPES[1]
    r, x, y = mw.small_scene(lx, ly, 65)
    rcut = 10.0 * 2.0 * float(r.mean())
    with pkg.LbmDem(lx, ly, r, x, y, physics=mw.small_physics(pkg, lx, ly, r, amp=0.0)) as sim:
        sim.set_vibration(True)
        R = vo.restate(x, y, r, box_of(sim), rcut)
        compare_voronoi(sim, R, sim.voronoi(rcut))
        t0, box0 = sim.walls()["t"], box_of(sim)
        sim.move_walls()
        assert sim.walls()["t"] > t0 and box_of(sim) == box0
        compare_voronoi(sim, R)
        sim.initVerlet()
        sim.initVerlet()
        assert box_of(sim) == box0
        compare_voronoi(sim, R)


# ---- 3. contact export and clusters at moving walls ----

def export_refused(pkg, sim, tmp_path, text):
    calls = (("lbmdem_download_contacts", sim.download_contacts), ("lbmdem_download_contacts", lambda: sim.write_contacts(str(tmp_path), 7)),
             ("lbmdem_contact_stats", sim.contact_stats), ("lbmdem_cluster_compute", sim.clusters),
             ("lbmdem_cluster_compute", lambda: sim.write_clusters(str(tmp_path), 7)))
    for who, call in calls:
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1 and sim._L.lbmdem_last_error().decode().startswith(text % who), (who, sim._L.lbmdem_last_error())
    for who, call in (("lbmdem_download_cluster_grains", sim.cluster_grains), ("lbmdem_download_clusters", sim.cluster_table)):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1 and sim._L.lbmdem_last_error().decode() == NO_CLUSTERS % who
    assert not os.path.exists(tmp_path / "contacts000007.dat") and not os.path.exists(tmp_path / "clusters000007.dat")


def test_contacts_and_clusters_at_moving_walls(pkg, tmp_path):
    """the shaken scene; the sub-steps of moving_walls_util.CONTACT_SUBSTEPS as table sub-steps, their records against the laws
    evaluated with the walls lbmdem_vibration_schedule gives for that sub-step, the clusters against cluster_util on those records"""
    lx, ly, r, x1, x2 = mw.shaken_inputs()
    with pkg.LbmDem(lx, ly, r, x1, x2, physics=mw.shaken_physics(pkg)) as sim:
        sim.set_vibration(True)
        Mgx0 = sim.walls()["Mgx"]
        total, told_apart = dict(left=0, right=0, top=0), 0
        for s in mw.CONTACT_SUBSTEPS:
            sim.set_diagnostics(False)
            sim.renderScene(s - sim.nbsteps)
            sim.set_diagnostics(True)
            cfg0, pre = sim.config(), sim.kinematics
            row = pkg.vibration_schedule(cfg0, s, 1)[0]
            sim.renderScene(1)
            w = sim.walls()
            assert (w["t"], w["Mgx"], w["Mdx"]) == tuple(row[:3]), s      # the walls that sub-step saw
            cumul, neigh, wf = sim.verlet()
            want, counts = mw.restated_records(pkg, cfg0, row, w["Mhy"], pre, r, cumul, neigh, wf)
            rec = sim.download_contacts()
            assert cu.same_records(rec, want), (s, len(rec), len(want))
            assert sim.contact_stats() == counts, (s, sim.contact_stats(), counts)
            for name, k in mw.wall_counts(want).items():
                total[name] += k
            still, _ = mw.restated_records(pkg, cfg0, row, w["Mhy"], pre, r, cumul, neigh, wf, Mgx=Mgx0)
            told_apart += mw.left_dn_differs(want, still)
            cluster_check(sim, 1.0, True, 2, rec=want)
        print(total, told_apart)
        assert min(total.values()) >= 3, total                 # records at the left, the right and the top wall
        assert told_apart >= 1                                 # ... and a left-wall dn that the initial Mgx does not give
        # a wall moved by hand: the handle's walls are not those of the records any more
        sim.move_walls()
        assert sim.walls()["Mgx"] != w["Mgx"]
        export_refused(pkg, sim, tmp_path, WALL_MOVED)
        # the next sub-step (walls moved once more by its own renderScene) makes them answer again
        cfg0, pre, s = sim.config(), sim.kinematics, sim.nbsteps
        row = pkg.vibration_schedule(cfg0, s, 1)[0]
        sim.renderScene(1)
        cumul, neigh, wf = sim.verlet()
        want, counts = mw.restated_records(pkg, cfg0, row, sim.walls()["Mhy"], pre, r, cumul, neigh, wf)
        assert cu.same_records(sim.download_contacts(), want) and sim.contact_stats() == counts
        cluster_check(sim, 1.0, True, 2, rec=want)
        sim.write_contacts(str(tmp_path), 8)
        sim.write_clusters(str(tmp_path), 8)
        # an ordinary sub-step ends the records' validity as ever, with the sentence it always had
        sim.set_diagnostics(False)
        sim.renderScene(1)
        export_refused(pkg, sim, tmp_path, "%s: " + NO_TABLE)


# ---- 4. everything else on a shifted raster ----

@pytest.fixture
def shifted(pkg):
    """the shaken scene after 250 sub-steps: the raster's origin has moved by more than a node. A handle per test: the second
    test sets tracers and a scalar on it"""
    lx, ly, r, x1, x2 = mw.shaken_inputs()
    with pkg.LbmDem(lx, ly, r, x1, x2, physics=mw.shaken_physics(pkg)) as sim:
        sim.set_vibration(True)
        sim.renderScene(mw.N)
        assert sim.walls()["Mgx"] > sim.cfg.dx
        yield sim, r


STACK = (ps.compute("pores", conn=8), ps.compute("clearance"), ps.compute("network", merge=-1),
         ps.compute("drainage", sides=ps.SIDES[0]), ps.compute("geodesic", sides=ps.SIDES[0], conn=8, min_d2=0),
         ps.compute("netflux", merge=-1, level=0), ps.compute("netsolve", sides=ps.SIDES[0], merge=-1, level=0))


def test_pore_analyses_on_a_shifted_raster(pkg, shifted):
    """the seven pore analyses on the handle's own map, each against its restatement fed obst and f: one pass"""
    sim, _ = shifted
    h = ps.Harness(pkg, sim, tag="shifted raster:")
    for op in STACK:
        h.run(op)                       # (holds the compute's return and its readers to the restatement)
    h.check_all()


def test_coarse_tracers_and_scalar_on_a_shifted_raster(pkg, shifted):
    sim, r = shifted
    lx, ly = sim.lx, sim.ly
    want, outside, valid = co.expected(sim, r, 16, 16)
    cells, got_outside, got_valid = sim.coarse_fields(16, 16)
    assert co.mismatches(cells, want) == [] and (got_outside, got_valid) == (outside, valid)
    assert want["grains"].sum() == sim.n - outside
    ux, uy = tu.planes(sim)             # (flow_util.fields with walls()["Mgx"]: the grains' velocity at nodes of the moved raster)
    obst = sim.obst
    xy = tu.grid_seeds(lx, ly, 16, 12)
    sim.set_tracers(xy, automatic=False)
    s = sim.tracer_sample()
    assert np.array_equal(s, tu.sample(ux, uy, obst, xy)) and (s[:, 2] >= 0).any() and (s[:, 2] == -1).any()
    sim.advance_tracers()
    assert tu.same(sim.tracers, tu.advance(ux, uy, xy))
    sim.set_tracers(np.zeros((0, 2)))
    tau = 0.8
    C0 = np.random.default_rng(41).normal(1.0, 0.5, (lx, ly))
    sim.set_scalar(C0, tau, automatic=False)
    g0, _ = su.initial(C0, obst)
    assert vo.same_bits(sim.scalar, su.conc(g0))
    want_g, want_was, want_C = su.expected_step(sim, 1. / tau, (ux, uy))
    sim.step_scalar()
    g, was = sim.scalar_state()
    assert vo.same_bits(g, want_g) and np.array_equal(was, want_was) and vo.same_bits(sim.scalar, want_C)
    sim.set_scalar(None)


# ---- 5. run_scene and the host driver ----

FREQ, AMP = 60.0, 2e-7
OUTPUTS = dict(fmin=1.0, relative=True, zmin=2, nbins=64, shell=1.2)


def scene_names(directory):
    return sorted(name for name in os.listdir(directory) if name != "stats.data")


def data_lines(path):
    return [l for l in open(path).read().splitlines() if not l.startswith("#")]


def test_run_scene_and_host_driver_while_vibrating(pkg, po, tmp_path):
    """61 x 59, vibrating, with the contacts, clusters, structure and Voronoi outputs on, through one DEM event: lbmdem_run_scene
    and `lbmdem --vib ...` in a child process write, byte for byte, what the same run driven from Python writes with the writers
    called by hand at that event"""
    lx, ly, r, x, y = mw.run_scene_inputs()
    rcut = 5.0 * 2.0 * float(r.mean())
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), r * 1e3, x * 1e3, y * 1e3)
    r, x, y = pkg.read_sample(str(sample))                 # (what the driver reads)
    phys = vu.physics(pkg, freq=FREQ, amp=AMP, dtt=0.0)
    dirs = {name: tmp_path / name for name in ("hand", "scene", "driver")}
    for d in dirs.values():
        d.mkdir()
    with pkg.LbmDem(lx, ly, r, x, y, physics=phys) as sim:
        sim.set_vibration(True)
        Mgx0 = sim.walls()["Mgx"]
        sim.renderScene(4000)
        assert np.isfinite(sim.kinematics).all() and sim.walls()["Mgx"] - Mgx0 > sim.cfg.dx
        hand = str(dirs["hand"])
        sim.write_DEM(hand, 0)
        sim.write_forces(hand, 0)
        sim.write_contacts(hand, 0)
        sim.write_clusters(hand, 0, OUTPUTS["fmin"], OUTPUTS["relative"], OUTPUTS["zmin"])
        sim.write_structure(hand, 0, rcut, OUTPUTS["nbins"], OUTPUTS["shell"])
        sim.write_voronoi(hand, 0, rcut)
        assert len(sim.download_contacts()) > 0
        end = {what: getattr(sim, what) for what in ("f", "obst", "kinematics", "fhf")}
    with pkg.LbmDem(lx, ly, r, x, y, physics=phys) as sim:
        sim.set_vibration(True)
        sim.set_contacts_output(True)
        sim.set_clusters_output(True, OUTPUTS["fmin"], OUTPUTS["relative"], OUTPUTS["zmin"])
        sim.set_structure_output(True, rcut, OUTPUTS["nbins"], OUTPUTS["shell"])
        sim.set_voronoi_output(True, rcut)
        sim.run_scene(4000, str(dirs["scene"]))
        for what in end:
            assert np.array_equal(getattr(sim, what), end[what]), what
    out = subprocess.run([EXE, str(sample), "--lx", str(lx), "--ly", str(ly), "--steps", "4001", "--vib", "--vib-freq", str(FREQ),
                          "--vib-amp", str(AMP), "--contacts", "--clusters", "--structure", repr(rcut), "--voronoi", repr(rcut)],
                         capture_output=True, text=True, cwd=dirs["driver"], timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    names = scene_names(dirs["hand"])
    assert {"contacts000000.dat", "clusters000000.dat", "cluster_table000000.dat", "structure000000.dat", "gr000000.dat",
            "voronoi000000.dat", "voronoi.data", "clusters.data", "structure.data", "DEM000000.dat"} <= set(names)
    for other in ("scene", "driver"):
        assert scene_names(dirs[other]) == names, other
        for name in names:
            assert (dirs[other] / name).read_bytes() == (dirs["hand"] / name).read_bytes(), (other, name)
        assert data_lines(dirs[other] / "stats.data") == data_lines(dirs["hand"] / "stats.data"), other


# ---- 6. recovery ----

RECOVERY_SCRIPT = r"""
import os, sys
import numpy as np
root = os.getcwd()
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "oracle")); sys.path.insert(0, os.path.join(root, "tests"))
import __graft_entry__ as ge
import moving_walls_util as mw, voronoi_util as vo
import test_gpu_moving_walls as tm
pkg = ge.load_package()
lx, ly, r, x1, x2 = mw.shaken_inputs()
rcut = mw.voronoi_rcut(r)
phys = mw.shaken_physics(pkg)
a = pkg.LbmDem(lx, ly, r, x1, x2, physics=phys)
b = pkg.LbmDem(lx, ly, r, x1, x2, physics=phys); b.set_dem_chain(0)
for s in (a, b):
    s.set_vibration(True)
cfg0 = a.config()
box0 = tm.box_of(a)
giveup = 1                                        # in the second fluid period of the second piece
a.debug_chain_giveup(giveup)
done = 0
for i, n in enumerate(mw.PIECES[:3]):
    a.renderScene(n); b.renderScene(n)
    done += n
assert a.dem_chain_stats()[0] > giveup and a.dem_chain_recoveries() == 0     # made, and nothing but runs since
# the first call that settles the handle finds the launch: chain_restore puts Mgx, Mdx, Mhy and t back where the launch found
# them, and the replay moves them on again, one sub-step at a time
w = a.walls()
assert a.dem_chain_recoveries() == 1 and b.dem_chain_recoveries() == 0 and a.nbsteps == b.nbsteps == done == 100
row = pkg.vibration_schedule(cfg0, 0, done)[-1]
assert (w["t"], w["Mgx"], w["Mdx"]) == tuple(row[:3]) and w == b.walls(), (w, row, b.walls())
assert w["Mhy"] == box0[3] and w["Mby"] == box0[2] and w["Mgx"] > box0[0]
ka, kb = a.kinematics, b.kinematics
assert np.isfinite(ka).all() and np.array_equal(ka.view(np.uint64), kb.view(np.uint64))
tm.compare_voronoi(a, vo.restate(ka[:, 0], ka[:, 1], r, tm.box_of(a), rcut), a.voronoi(rcut))
# ... and on, with the kernel back in use: the cells of the final walls, which are not those of the walls it began with
a.set_dem_chain(128)
la = a.dem_chain_stats()[0]
for n in mw.PIECES[3:]:
    a.renderScene(n); b.renderScene(n)
    done += n
    w = a.walls()
    row = pkg.vibration_schedule(cfg0, 0, done)[-1]
    assert (w["t"], w["Mgx"], w["Mdx"]) == tuple(row[:3]) and w == b.walls(), (done, w, row)
    x, y = tm.centres(a)
    tm.compare_voronoi(a, vo.restate(x, y, r, tm.box_of(a), rcut), a.voronoi(rcut))
assert a.dem_chain_stats()[0] > la and a.dem_chain_recoveries() == 1
print(mw.voronoi_teeth(x, y, r, box0, tm.box_of(a), a.cfg.dx, rcut))
a.close(); b.close()
print("recovered: voronoi")
"""


def test_voronoi_after_a_recovered_run():
    """the shaken scene against the experiment build, in a process of its own as tests/test_gpu_chain_recovery.py's cases: launch 1
    of the multi-sub-step kernel gives up (lbmdem_debug_chain_giveup: the library's own cooperative exit, no fault), the first
    walls() finds it. The walls and the clock are those of lbmdem_vibration_schedule and of a twin handle without the kernel, and
    structure + voronoi and the readers are the restatement with box = walls(), there and 150 sub-steps on"""
    assert os.path.exists(AB_LIB), "the experiment build (make -C 2d-lbm-dem_amd/csrc AB=1) is not there"
    env = dict(os.environ, LBMDEM_HIP_LIBRARY=AB_LIB)
    out = subprocess.run([sys.executable, "-c", RECOVERY_SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "recovered: voronoi" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
