"""GPU: write_DEM / write_forces in the background (lbmdem_set_async_dem / lbmdem_write_dem_async / lbmdem_dem_stats) -- the
stats.data line computed on the device against the reference's file and, bit for bit, against the host loop of the
synchronous writer; the files against the synchronous writers' and the reference's; an event that is a snapshot although
the run goes on at once; the loop (lbmdem_run_scene) with either or both background switches; back-pressure with one slot;
the writer's errors; the refusals; a replayed run; checkpoints; the host driver's --async-dem. All comparisons are exact."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import golden_util as gu
import samples
from test_dem_rows_host import REF_DIR, check_against_golden
from test_gpu_async_output import same_dirs, same_state, vtk_names, g4
from test_gpu_run_scene import without_clock
from test_gpu_vibration import _inputs as _vib_inputs, _shaker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
E8 = [8, 15, 16, 18, 17, 19, 20, 21]     # energies8 = stats22[E8]


def g6():
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    return 256, 200, z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3


def packing(n):
    """the G6 grains, or a row packing of exactly n grains (some pairs in contact) on the smallest lattice that holds it"""
    if n == "G6":
        return g6()
    lx, ly = (512, 640) if n > 500 else (256, 200)
    r, x, y = samples.row_packing(lx, ly, n, seed=29)
    assert len(r) == n
    return (lx, ly) + samples.to_metres(r, x, y)


def dem_names(*nfiles):
    return ["DEM%06d.%s" % (k, e) for k in nfiles for e in ("dat", "ps")] + ["stats.data"]


def stats_lines(d):
    return [l.split() for l in (d / "stats.data").read_text().splitlines()]


def host_loop(sim, po):
    """the loop of write_DEM (main.c:340-438) over the downloaded table in Python's doubles, statement for statement: ten
    serial chains in grain order"""
    t, cfg, c = sim.grain_table(), sim.cfg, po.COL
    p = cfg.phys
    col = lambda name: [float(v) for v in t[:, c[name]]]
    x1, x2, v1, v2, v3, r, m, It, pp, ss = (col(k) for k in "x1 x2 v1 v2 v3 r m It p s".split())
    fr, ifr, ice, slip, rw, z, zz = (col(k) for k in "fr ifr ice slip rw z zz".split())
    n = len(r)
    xfront, height, xgrainmax = x1[0] + r[0], x2[0] + r[0], x1[0]
    ex = ey = et = ep = SE = WF = IFR = INCE = TSLIP = TRW = 0.0
    zmean, N = 0.0, [0.0] * 6
    for i in range(n):
        zmean += int(z[i])
        if 0 <= int(z[i]) <= 5:
            N[int(z[i])] += 1
        ex += 0.5 * m[i] * v1[i] * v1[i]
        ey += 0.5 * m[i] * v2[i] * v2[i]
        et += 0.5 * It[i] * v3[i] * v3[i]
        ep += m[i] * p.G * x2[i]
        SE += 0.5 * (((pp[i] * pp[i]) / p.kg) + ((ss[i] * ss[i]) / p.kt))
        WF += fr[i]; IFR += ifr[i]; TSLIP += slip[i]; TRW += rw[i]; INCE += ice[i]
        if x1[i] + r[i] > xgrainmax: xgrainmax = x1[i] + r[i]
        if x2[i] + r[i] > height: height = x2[i] + r[i]
        if zz[i] > 0 and x1[i] + r[i] >= xfront: xfront = x1[i] + r[i]
    return np.array([sim.nbsteps * cfg.dt - p.dtt, xfront, xgrainmax, height, zmean / n, ex, ey, et, ex + ey + et] +
                    [v / n for v in N] + [ep, SE, WF, IFR, INCE, TSLIP, TRW])


# ---- 1. the stats line and the files at the reference's own event ----------------------------------------------------------------

@pytest.fixture(scope="module")
def at4000(pkg):
    """twin handles with the G6 packing after the 4000 sub-steps of the golden files; the tests that share them only read"""
    lx, ly, r, x1, x2 = g6()
    a, b = pkg.LbmDem(lx, ly, r, x1, x2), pkg.LbmDem(lx, ly, r, x1, x2)
    a.renderScene(4000); b.renderScene(4000)
    yield a, b
    a.close(); b.close()


def test_stats_line_matches_the_reference_and_the_synchronous_writer(at4000, tmp_path):
    a, b = at4000
    st = b.dem_stats()
    want = open(os.path.join(REF_DIR, "stats.data")).read().split()
    assert len(want) == 22 and st.shape == (22,)
    for k in range(22):
        assert "%le" % st[k] == want[k], (k, st[k], want[k])
    e8 = a.write_DEM(str(tmp_path), 0)
    assert tuple(st[E8]) == e8
    assert np.array_equal(b.dem_stats(), st)          # asking changes nothing


def test_files_identical_to_the_synchronous_writers_and_the_reference(at4000, tmp_path):
    a, b = at4000
    da, db = tmp_path / "sync", tmp_path / "async"
    da.mkdir(); db.mkdir()
    ea = a.write_DEM(str(da), 0)
    a.write_forces(str(da), 0)
    b.set_async_dem(2)
    eb = b.write_DEM_async(str(db), 0)
    b.output_drain()
    assert ea == eb
    same_dirs(da, db, dem_names(0))
    check_against_golden(db)
    assert stats_lines(db) == [open(os.path.join(REF_DIR, "stats.data")).read().split()]
    st = b.output_stats_dem()
    assert (st["queued"], st["written"], st["failed"], st["slot_waits"]) == (1, 1, 0, 0) and st["ms_io"] > 0.0
    assert np.array_equal(b.dem_stats(), a.dem_stats())      # with the feature on (its scratch) and off (a temporary)
    # without the map: DEM*.dat and the line only
    dc = tmp_path / "nomap"
    dc.mkdir()
    b.write_DEM_async(str(dc), 1, forces=False)
    b.set_async_dem(0)                                       # writes what is queued
    assert sorted(p.name for p in dc.iterdir()) == ["DEM000001.dat", "stats.data"]
    assert (dc / "DEM000001.dat").read_bytes() == (da / "DEM000000.dat").read_bytes()
    assert b.output_stats_dem()["queued"] == 0


# ---- 2. the chains, bit for bit ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ["G6", 1, 63, 65, 1025])
def test_chains_equal_the_host_loop_bit_for_bit(pkg, po, tmp_path, n):
    """after 1, 2, 3, 25 and 100 sub-steps (step 0 is a film step; the early steps have wall contacts). 1, 63, 65, 1025 grains:
    below one wavefront, around one, and across the 128-grain workgroups of the row kernel and the 256-grain chunks of the
    chains with a ragged tail"""
    lx, ly, r, x1, x2 = packing(n)
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    sim.set_diagnostics(True)
    for k, steps in enumerate((1, 1, 1, 22, 75)):
        sim.renderScene(steps)
        st = sim.dem_stats()
        e8 = sim.write_DEM(str(tmp_path), k)
        line = stats_lines(tmp_path)[-1]
        assert tuple(st[E8]) == e8, (sim.nbsteps, st[E8], e8)
        assert ["%le" % v for v in st] == line, sim.nbsteps
        want = host_loop(sim, po)
        assert np.array_equal(st, want), (sim.nbsteps, np.flatnonzero(st != want), st, want)
    assert st[8] > 0.0 and np.isfinite(st).all()      # the grains move
    sim.close()


def test_rows_equal_the_table_and_the_forces(pkg, po, tmp_path):
    """the rows as the file prints them, at sizes around the row kernel's workgroup: every column read back exactly"""
    for n in (1, 129):
        lx, ly, r, x1, x2 = packing(n)
        sim = pkg.LbmDem(lx, ly, r, x1, x2)
        sim.set_diagnostics(True)
        sim.set_async_dem(1)
        sim.renderScene(25)
        sim.write_DEM_async(str(tmp_path), n)
        sim.output_drain()
        t, hf, c = sim.grain_table(), sim.fhf, po.COL
        got = [l.split("\t") for l in (tmp_path / ("DEM%06d.dat" % n)).read_text().splitlines()]
        assert len(got) == n
        names = "r x1 x2 x3 v1 v2 v3 a1 a2 a3".split() + [None] * 3 + ["p", "s", None] + "fr ifr ice slip rw fm M11 M12 M21 M22".split()
        for i, f in enumerate(got):
            assert len(f) == 28 and f[0] == str(i) and f[27] == str(int(t[i, c["z"]]))
            for k, name in enumerate(names):
                if name is not None:
                    assert f[1 + k] == "%le" % t[i, c[name]], (i, name)
            assert f[11:14] == ["%le" % v for v in hf[i]]
        sim.close()


# ---- 3. a snapshot is a snapshot --------------------------------------------------------------------------------------------------

def test_an_event_holds_the_table_it_was_asked_at(pkg, tmp_path):
    lx, ly, r, x1, x2 = g6()
    a, b = pkg.LbmDem(lx, ly, r, x1, x2), pkg.LbmDem(lx, ly, r, x1, x2)
    da, db = tmp_path / "sync", tmp_path / "async"
    da.mkdir(); db.mkdir()
    for s in (a, b):
        s.set_diagnostics(True)
        s.renderScene(30)
    b.set_async_dem(2)
    ea = a.write_DEM(str(da), 0); a.write_forces(str(da), 0)
    then = b.dem_stats()
    eb = b.write_DEM_async(str(db), 0)
    b.renderScene(50)                 # right behind the two kernels: rewrites every array they read
    a.renderScene(50)
    b.output_drain()
    assert ea == eb
    same_dirs(da, db, dem_names(0))
    same_state(a, b)
    assert not np.array_equal(b.dem_stats()[1:], then[1:])
    a.close(); b.close()


# ---- 4. the loop ----------------------------------------------------------------------------------------------------------------------

def test_run_scene_queues_its_tables_and_leaves_the_same_files(pkg, tmp_path):
    lx, ly, r, x1, x2 = g4()
    phys = pkg.derive(lx, ly, r).phys
    phys.stepFilm = 1300
    sims = [pkg.LbmDem(lx, ly, r, x1, x2, physics=phys) for _ in range(3)]
    off, dem, both = sims
    dirs = [tmp_path / k for k in ("off", "dem", "both")]
    for d in dirs:
        d.mkdir()
    dem.set_async_dem(2)
    both.set_async_dem(2); both.set_async_output(2)
    outs = [s.run_scene(4100, outdir=str(d)) for s, d in zip(sims, dirs)]
    sd, sb = dem.output_stats_dem(), both.output_stats_dem()      # taken right after the call: nothing may be pending
    assert (sd["queued"], sd["written"], sd["failed"]) == (1, 1, 0), sd
    assert (sb["queued"], sb["written"], sb["failed"]) == (1, 1, 0), sb
    st = both.output_stats()
    assert (st["queued"], st["written"], st["failed"]) == (3, 3, 0), st
    zeros = dict(queued=0, written=0, failed=0, slot_waits=0, ms_slot_wait=0.0, ms_copy_wait=0.0, ms_io=0.0, ms_drain=0.0)
    assert dem.output_stats() == zeros and off.output_stats() == zeros
    assert off.output_stats_dem() == dict(queued=0, written=0, failed=0, slot_waits=0, ms_slot_wait=0.0, ms_copy_wait=0.0,
                                          ms_io=0.0, ms_stats_wait=0.0)
    expect = sum((vtk_names(k) for k in range(3)), []) + dem_names(3)
    for k in (1, 2):
        assert outs[k][1] == outs[0][1] and outs[0][1]["nfile"] == 3
        assert without_clock(outs[k][0]) == without_clock(outs[0][0])
        same_dirs(dirs[0], dirs[k], expect)
        same_state(sims[0], sims[k])
    assert any(v != 0.0 for v in outs[0][1]["energies8"])
    # a second loop across the next event: the lines of stats.data in order
    outs = [s.run_scene(4000, outdir=str(d)) for s, d in zip(sims, dirs)]
    expect = sum((vtk_names(k) for k in range(6)), []) + dem_names(3, 6)
    for k in (1, 2):
        assert outs[k][1] == outs[0][1] and outs[0][1]["nfile"] == 6
        assert without_clock(outs[k][0]) == without_clock(outs[0][0])
        same_dirs(dirs[0], dirs[k], expect)
    lines = stats_lines(dirs[1])
    assert len(lines) == 2 and float(lines[0][0]) < float(lines[1][0])
    assert dem.output_stats_dem()["written"] == 2
    for s in sims:
        s.close()


# ---- 5. back-pressure -------------------------------------------------------------------------------------------------------------------

def test_one_slot_never_drops_an_event(pkg, tmp_path):
    lx, ly, r, x1, x2 = g6()
    a, b = pkg.LbmDem(lx, ly, r, x1, x2), pkg.LbmDem(lx, ly, r, x1, x2)
    da, db = tmp_path / "sync", tmp_path / "async"
    da.mkdir(); db.mkdir()
    a.set_diagnostics(True); b.set_diagnostics(True)
    b.set_async_dem(1)
    for k in range(4):
        a.renderScene(12); b.renderScene(12)
        ea = a.write_DEM(str(da), k); a.write_forces(str(da), k)
        assert b.write_DEM_async(str(db), k) == ea
    b.output_drain()
    same_dirs(da, db, dem_names(0, 1, 2, 3))
    times = [float(l[0]) for l in stats_lines(db)]
    assert len(times) == 4 and times == sorted(times) and len(set(times)) == 4
    st = b.output_stats_dem()
    assert (st["queued"], st["written"], st["failed"]) == (4, 4, 0)
    assert 0 <= st["slot_waits"] <= 3 and (st["slot_waits"] == 0) == (st["ms_slot_wait"] == 0.0)
    assert st["ms_io"] > 0.0 and st["ms_stats_wait"] > 0.0
    same_state(a, b)
    # a change of the number of slots keeps nothing and loses nothing; frames switched on and off leave the tables alone
    b.set_async_dem(3)
    assert b.output_stats_dem()["queued"] == 0
    b.set_async_output(1)
    b.write_DEM_async(str(db), 4); a.write_DEM(str(da), 4); a.write_forces(str(da), 4)
    b.set_async_output(0)            # drains: the writer is shared
    same_dirs(da, db, dem_names(0, 1, 2, 3, 4))
    assert b.output_stats_dem()["written"] == 1
    b.set_async_dem(0)
    a.close(); b.close()


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------------

def test_a_writer_failure_reaches_the_caller_once_and_the_handle_goes_on(pkg, tmp_path):
    lx, ly, r, x1, x2 = g6()
    a, b = pkg.LbmDem(lx, ly, r, x1, x2), pkg.LbmDem(lx, ly, r, x1, x2)
    a.set_diagnostics(True); b.set_diagnostics(True)
    b.set_async_dem(2)
    gone = tmp_path / "vanishes"
    gone.mkdir(); gone.rmdir()
    a.renderScene(24); b.renderScene(24)
    b.write_DEM_async(str(gone), 0)          # queued: the failure is the writer's
    with pytest.raises(pkg.LbmDemError) as e:
        b.output_drain()
    assert e.value.code == -1 and str(gone) in str(e.value)
    st = b.output_stats_dem()
    assert (st["queued"], st["written"], st["failed"]) == (1, 0, 1)
    b.output_drain()                         # reported once
    # ... or at the next event, which is then not queued
    b.write_DEM_async(str(gone), 1)
    deadline = time.monotonic() + 60
    while b.output_stats_dem()["failed"] < 2 and time.monotonic() < deadline:
        time.sleep(0.01)
    assert b.output_stats_dem()["failed"] == 2
    with pytest.raises(pkg.LbmDemError) as e:
        b.write_DEM_async(str(tmp_path), 2)
    assert str(gone) in str(e.value) and b.output_stats_dem()["queued"] == 2
    # the handle steps and writes a good event
    a.renderScene(24); b.renderScene(24)
    da, db = tmp_path / "sync", tmp_path / "async"
    da.mkdir(); db.mkdir()
    ea = a.write_DEM(str(da), 5); a.write_forces(str(da), 5)
    assert b.write_DEM_async(str(db), 5) == ea
    b.output_drain()
    same_dirs(da, db, dem_names(5))
    same_state(a, b)
    b.write_DEM_async(str(gone), 6)          # an unreported failure does not keep close() from returning
    b.close(); a.close()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["async", "sync"]


def test_destroy_with_jobs_pending_leaves_complete_files(pkg, tmp_path):
    lx, ly, r, x1, x2 = g6()
    a, b = pkg.LbmDem(lx, ly, r, x1, x2), pkg.LbmDem(lx, ly, r, x1, x2)
    da, db = tmp_path / "sync", tmp_path / "async"
    da.mkdir(); db.mkdir()
    a.set_diagnostics(True); b.set_diagnostics(True)
    b.set_async_dem(4)
    for k in range(3):
        a.renderScene(9); b.renderScene(9)
        a.write_DEM(str(da), k); a.write_forces(str(da), k)
        b.write_DEM_async(str(db), k)
    b.close()
    same_dirs(da, db, dem_names(0, 1, 2))
    a.close()


# ---- 7. refusals, and the handles that are allowed -------------------------------------------------------------------------------------

def test_refusals(pkg, tmp_path):
    lx, ly, r, x1, x2 = g6()
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    sim.set_diagnostics(True)
    sim.renderScene(3)
    with pytest.raises(pkg.LbmDemError) as e:
        sim.write_DEM_async(str(tmp_path), 0)              # off by default
    assert e.value.code == -1 and "lbmdem_set_async_dem" in str(e.value)
    for slots in (-1, 5):
        with pytest.raises(pkg.LbmDemError) as e:
            sim.set_async_dem(slots)
        assert e.value.code == -1
    sim.set_async_dem(4)
    sim.set_async_dem(0)
    with pytest.raises(pkg.LbmDemError) as e:
        sim.write_DEM_async(str(tmp_path), 0)
    assert e.value.code == -1
    sim.set_async_dem(1)
    sim.set_diagnostics(False)
    sim.renderScene(1)                                     # the last sub-step left no table
    for call in (lambda: sim.write_DEM_async(str(tmp_path), 0), sim.dem_stats):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1 and "diagnostics" in str(e.value)
    assert sim.output_stats_dem()["queued"] == 0
    with pytest.raises(pkg.LbmDemError) as e:
        sim.dist_enable()
    assert e.value.code == -1 and "lbmdem_set_async_dem" in str(e.value)
    sim.close()
    lx, ly, r, x1, x2 = g4()
    strip = pkg.LbmDem(lx, ly, r, x1, x2, strip=(0, 128), halo=2)
    with pytest.raises(pkg.LbmDemError) as e:
        strip.set_async_dem(2)
    assert e.value.code == -1
    strip.close()
    dist = pkg.LbmDem(lx, ly, r, x1, x2)
    dist.dist_enable()
    with pytest.raises(pkg.LbmDemError) as e:
        dist.set_async_dem(2)
    assert e.value.code == -1
    dist.close()
    sp = pkg.LbmDem(lx, ly, r, x1, x2, precision="f32")   # the float library has no write_DEM
    sp.renderScene(3)
    for call in (lambda: sp.set_async_dem(2), lambda: sp.write_DEM_async(str(tmp_path), 0), sp.dem_stats):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1 and "single-precision" in str(e.value)
    sp.close()
    assert list(tmp_path.iterdir()) == []


def test_a_checkpoint_does_not_carry_the_setting(pkg, tmp_path):
    lx, ly, r, x1, x2 = g6()
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    sim.set_diagnostics(True)
    sim.set_async_dem(2)
    sim.renderScene(12)
    sim.checkpoint_save(str(tmp_path / "ck"))
    back = pkg.LbmDem.checkpoint_load(str(tmp_path / "ck"))
    back.renderScene(1); sim.renderScene(1)
    with pytest.raises(pkg.LbmDemError) as e:
        back.write_DEM_async(str(tmp_path), 0)
    assert "lbmdem_set_async_dem" in str(e.value)
    assert np.array_equal(back.dem_stats(), sim.dem_stats())
    sim.close(); back.close()


def test_vibrating_and_probing_handles_write_the_same_tables(pkg, tmp_path):
    lx, ly, r, x1, x2 = _vib_inputs("G4")
    phys = _shaker(pkg, lx, ly, r)
    for kind in ("vib", "probe"):
        sims = [pkg.LbmDem(lx, ly, r, x1, x2, physics=phys if kind == "vib" else None) for _ in range(2)]
        for s in sims:
            if kind == "vib":
                s.set_vibration(True)
            else:
                s.probe_enable(every=1, capacity=64, pressure_row=2, points=[(5, 5)])
            s.set_diagnostics(True)
        a, b = sims
        da, db = tmp_path / (kind + "_sync"), tmp_path / (kind + "_async")
        da.mkdir(); db.mkdir()
        b.set_async_dem(2)
        for k in range(3):
            a.renderScene(50); b.renderScene(50)
            ea = a.write_DEM(str(da), k); a.write_forces(str(da), k)
            assert b.write_DEM_async(str(db), k) == ea
        b.output_drain()
        same_dirs(da, db, dem_names(0, 1, 2))
        same_state(a, b)
        a.close(); b.close()


# ---- 8. a replayed run ---------------------------------------------------------------------------------------------------------------

GIVEUP_SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import __graft_entry__ as ge, samples
pkg = ge.load_package()
out = sys.argv[1]
lx, ly = 512, 320
r, x, y = samples.row_packing(lx, ly, 700, seed=5)
r, x1, x2 = samples.to_metres(r, x, y)
a = pkg.LbmDem(lx, ly, r, x1, x2)          # the multi-sub-step kernel, one launch made to give up
b = pkg.LbmDem(lx, ly, r, x1, x2); b.set_dem_chain(0)
k = a.kinematics
k[:, 3:6] = np.random.default_rng(17).normal(0, 1, (len(r), 3)) * (0.05, 0.05, 30.0)
for s in (a, b):
    s.kinematics = k
    s.nbsteps = 3800               # the sub-step that reaches 4000 leaves the table
a.set_async_dem(2)
a.debug_chain_giveup(3)            # inside the stretch: the event of step 4000 is the call that finds it
da, db = os.path.join(out, "a"), os.path.join(out, "b")
os.mkdir(da); os.mkdir(db)
a.renderScene(200); b.renderScene(200)
ea = a.write_DEM_async(da, 1)
eb = b.write_DEM(db, 1); b.write_forces(db, 1)
a.output_drain()
assert a.dem_chain_recoveries() == 1 and b.dem_chain_recoveries() == 0
assert ea == eb, (ea, eb)
st = a.output_stats_dem()
assert (st["queued"], st["written"], st["failed"]) == (1, 1, 0), st
names = sorted(os.listdir(da))
assert names == sorted(os.listdir(db)) == ["DEM000001.dat", "DEM000001.ps", "stats.data"], names
for n in names:
    assert open(os.path.join(da, n), "rb").read() == open(os.path.join(db, n), "rb").read(), n
assert np.array_equal(a.f, b.f) and np.array_equal(a.kinematics, b.kinematics) and np.array_equal(a.obst, b.obst)
a.close(); b.close()
print("recovered: tables", len(names))
"""


def test_a_replayed_run_writes_the_tables_of_the_undisturbed_one(tmp_path):
    """A launch of the multi-sub-step DEM kernel that gives up (made to, in the experiment build, as
    tests/test_gpu_async_output.py::test_a_replayed_run_writes_the_frames_of_the_undisturbed_one does) before a DEM event:
    the writer settles the handle first -- the launch is undone, its sub-steps and the table sub-step repeated -- and only
    then takes the table."""
    lib = os.path.join(ROOT, "2d-lbm-dem_amd", "liblbmdem_hip_ab.so")
    assert os.path.exists(lib), "run __graft_entry__.build()"
    env = dict(os.environ, LBMDEM_HIP_LIBRARY=lib)
    out = subprocess.run([sys.executable, "-c", GIVEUP_SCRIPT, str(tmp_path)], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "recovered: tables 3" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 9. the host driver ---------------------------------------------------------------------------------------------------------------

def test_host_driver_async_dem_writes_the_same_files(po, tmp_path):
    c = gu.CASES["G4_coupled_256x200"]
    outs = {}
    for mode, extra in (("sync", []), ("dem", ["--async-dem"]), ("both", ["--async-dem", "1", "--async-output"])):
        d = tmp_path / mode
        d.mkdir()
        sample = d / "packing.data"
        po.write_sample(str(sample), c["r_mm"], c["x_mm"], c["y_mm"])
        cmd = [EXE, str(sample), "--lx", "256", "--ly", "200", "--steps", "8001", "--run-stats"] + extra
        out = subprocess.run(cmd, capture_output=True, text=True, cwd=d, timeout=900)
        assert out.returncode == 0, (out.stdout[-400:], out.stderr[-1200:])
        outs[mode] = out
    expect = ["packing.data"] + vtk_names(0) + dem_names(0, 1)
    same_dirs(tmp_path / "sync", tmp_path / "dem", expect)
    same_dirs(tmp_path / "sync", tmp_path / "both")
    fd = lambda o: re.search(r"^final_density: ([0-9.]+)$", o.stderr, re.M).group(1)
    assert fd(outs["sync"]) == fd(outs["dem"]) == fd(outs["both"])
    assert "async_dem" not in outs["sync"].stderr and "async_output" not in outs["dem"].stderr
    for mode in ("dem", "both"):
        m = re.search(r"^async_dem: queued (\d+) written (\d+) failed (\d+) slot_waits (\d+) ms_slot_wait ([0-9.]+) "
                      r"ms_copy_wait ([0-9.]+) ms_io ([0-9.]+) ms_stats_wait ([0-9.]+)$", outs[mode].stderr, re.M)
        assert m, outs[mode].stderr[-800:]
        assert [int(v) for v in m.groups()[:3]] == [2, 2, 0]
    console = lambda o: [l.split(" Time ")[0] for l in o.stdout.splitlines() if l.startswith(("Iteration Number", "steps "))]
    assert console(outs["sync"]) == console(outs["dem"]) == console(outs["both"]) and len(console(outs["sync"])) >= 80
