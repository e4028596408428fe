"""GPU: VTK frames written in the background (lbmdem_set_async_output / lbmdem_write_vtk_async / lbmdem_output_drain) --
the snapshot kernel against the existing field kernel, the files against the reference's own and against the synchronous
writer's, a frame that is a snapshot although the run goes on at once, the loop (lbmdem_run_scene), back-pressure with one
slot, the writer's errors, the refusals, a replayed run, and the host driver's --async-output. All comparisons are exact."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import golden_util as gu
import samples
from test_gpu_run_scene import without_clock
from test_gpu_vibration import _inputs as _vib_inputs, _shaker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
FIELDS = ("grain_pressure", "grain_velocity", "grain_acceleration", "fluid_pressure", "fluid_velocity")


def vtk_names(nfile):
    return sorted("%s_%06d.vtk" % (f, nfile) for f in FIELDS)


def g4():
    return (256, 200) + tuple(gu.inputs_m("G4_coupled_256x200"))


def image_of_fields(sim):
    """what the existing kernel (k_vtk_fields) gives, put into the image's form: big-endian, the five payloads back to back"""
    return b"".join(np.ascontiguousarray(a).astype(">f4").tobytes() for a in sim.vtk_fields())


def same_dirs(da, db, expect=None):
    names = sorted(p.name for p in da.iterdir())
    assert names == sorted(p.name for p in db.iterdir())
    if expect is not None:
        assert names == sorted(expect), names
    for n in names:
        assert (da / n).read_bytes() == (db / n).read_bytes(), n


def same_state(a, b):
    assert a.nbsteps == b.nbsteps
    assert np.isfinite(a.kinematics).all()
    assert np.array_equal(a.kinematics, b.kinematics)
    assert np.array_equal(a.obst, b.obst)
    assert np.array_equal(a.f, b.f)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------

def check_image(sim):
    got = sim.vtk_image().tobytes()
    want = image_of_fields(sim)
    assert len(got) == 44 * sim.lx * sim.ly == len(want)
    if got != want:
        g, w = np.frombuffer(got, ">f4"), np.frombuffer(want, ">f4")
        bad = np.flatnonzero(g.view(">u4") != w.view(">u4"))
        raise AssertionError(f"{bad.size} of {g.size} floats differ, first at {bad[0]}: {g[bad[0]]!r} vs {w[bad[0]]!r}")
    fp = np.frombuffer(want, ">f4")[7 * sim.lx * sim.ly:8 * sim.lx * sim.ly]
    gp = np.frombuffer(want, ">f4")[:sim.lx * sim.ly]
    assert np.any(fp != 0) and np.any(gp != -1.0)      # fluid nodes and grain nodes both occur


def test_image_equals_the_field_kernel_G4(pkg):
    lx, ly, r, x1, x2 = g4()
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    check_image(sim)              # before the first step: obst as created
    sim.renderScene(60)
    check_image(sim)
    sim.obst_construction()       # a newer map not yet consumed by collide_stream: both kernels take that one
    check_image(sim)
    sim.close()


def test_image_equals_the_field_kernel_a08d83(pkg):
    g = gu.load("real_a08d83_600x500")
    sim = pkg.LbmDem(600, 500, g["r"], g["x1"], g["x2"])
    sim.renderScene(60)
    check_image(sim)
    sim.close()


@pytest.mark.parametrize("lx,ly", [(83, 37), (65, 17), (130, 95)])
def test_image_on_lattices_that_do_not_fill_the_blocks(pkg, lx, ly):
    """lx not a multiple of the kernel's 64 (32) columns, ly not a multiple of 16 (32): the row pitch is not ly; both builds"""
    # a row of grains of 0.5 mm on the floor (a node is 0.1 mm), some in contact
    x1 = np.arange(1.0e-3, lx * 1e-4 - 1.0e-3, 1.02e-3)
    r, x2 = np.full(len(x1), 0.5e-3), np.full(len(x1), 0.75e-3)
    assert len(r) >= 4
    for precision in ("f64", "f32"):
        sim = pkg.LbmDem(lx, ly, r, x1, x2, precision=precision)
        sim.renderScene(40)
        check_image(sim)
        sim.close()


def test_image_equals_the_field_kernel_in_the_float_build(pkg):
    lx, ly, r, x1, x2 = g4()
    sim = pkg.LbmDem(lx, ly, r, x1, x2, precision="f32")
    sim.renderScene(60)
    check_image(sim)
    sim.close()


# ---- 2. the reference's bytes ------------------------------------------------------------------------------------------------

def test_async_files_byte_identical_to_the_reference(pkg, tmp_path):
    """the set-up of test_gpu_golden.py::test_vtk_files_byte_identical_to_the_reference, written in the background"""
    sim = gu.GpuAdapter(pkg, "G5_dem_64x48")
    sim.set_kinematics(gu.mg.dem_initial_kinematics(gu.CASES["G5_dem_64x48"]))
    sim.steps(25)
    sim.sim.set_async_output(2)
    sim.sim.write_vtk_async(str(tmp_path), 3)
    sim.sim.output_drain()
    ref_dir = os.path.join(gu.HERE, "golden", "vtk_G5_25steps")
    names = sorted(os.listdir(ref_dir))
    assert len(names) == 5 and sorted(p.name for p in tmp_path.iterdir()) == names
    for name in names:
        got = open(tmp_path / name, "rb").read()
        want = open(os.path.join(ref_dir, name), "rb").read()
        assert got == want, f"{name}: {len(got)} vs {len(want)} bytes, first diff at " \
                            f"{next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)}"
    st = sim.sim.output_stats()
    assert (st["queued"], st["written"], st["failed"]) == (1, 1, 0)


# ---- 3. a snapshot is a snapshot ----------------------------------------------------------------------------------------------

def test_a_frame_holds_the_state_it_was_asked_at(pkg, tmp_path):
    """1024 x 1024 with grains: the copy and the files (45 MB) take far longer than a coupled step; the run goes on right
    behind the snapshot kernel and must not reach the frame"""
    lx = ly = 1024
    r, x, y = samples.row_packing(lx, ly, 2500, seed=11)
    r, x1, x2 = samples.to_metres(r, x, y)
    a, b = pkg.LbmDem(lx, ly, r, x1, x2), pkg.LbmDem(lx, ly, r, x1, x2)
    k = a.kinematics
    k[:, 3:6] = np.random.default_rng(2).normal(0, 1, (len(r), 3)) * (0.05, 0.05, 30.0)
    a.kinematics = k; b.kinematics = k
    a.renderScene(30); b.renderScene(30)
    da, db = tmp_path / "sync", tmp_path / "async"
    da.mkdir(); db.mkdir()
    b.set_async_output(2)
    a.write_vtk(str(da), 0)
    a.renderScene(240)
    b.write_vtk_async(str(db), 0)
    b.renderScene(240)
    b.output_drain()
    same_dirs(da, db, vtk_names(0))
    same_state(a, b)
    assert not np.array_equal(a.vtk_image(), np.frombuffer(b"".join(
        (da / ("%s_%06d.vtk" % (f, 0))).read_bytes()[-lx * ly * 4 * d:] for f, d in zip(FIELDS, (1, 3, 3, 1, 3))), np.uint8))
    a.close(); b.close()


# ---- 4. the loop ------------------------------------------------------------------------------------------------------------------

def test_run_scene_queues_its_frames_and_leaves_the_same_files(pkg, tmp_path):
    lx, ly, r, x1, x2 = g4()
    phys = pkg.derive(lx, ly, r).phys
    phys.stepFilm = 60
    a, b = (pkg.LbmDem(lx, ly, r, x1, x2, physics=phys) for _ in range(2))
    da, db = tmp_path / "sync", tmp_path / "async"
    da.mkdir(); db.mkdir()
    b.set_async_output(2)
    la, ra = a.run_scene(600, outdir=str(da))
    lb, rb = b.run_scene(600, outdir=str(db))
    st = b.output_stats()            # taken right after the call: nothing may be pending
    assert (st["queued"], st["written"], st["failed"]) == (10, 10, 0), st
    assert ra == rb and ra["nfile"] == 10 and ra["steps_done"] == 600
    assert without_clock(la) == without_clock(lb) and len(la) >= 7
    same_dirs(da, db, sum((vtk_names(k) for k in range(10)), []))
    same_state(a, b)
    assert a.output_stats() == dict(queued=0, written=0, failed=0, slot_waits=0, ms_slot_wait=0.0, ms_copy_wait=0.0, ms_io=0.0,
                                    ms_drain=0.0)
    a.close(); b.close()


def test_run_scene_with_tables_writes_every_file_of_the_schedule(pkg, tmp_path):
    """across a write_DEM / write_forces event (step 4000), which stay synchronous: VTK, DEM*.dat, .ps, stats.data"""
    lx, ly, r, x1, x2 = g4()
    phys = pkg.derive(lx, ly, r).phys
    phys.stepFilm = 1300
    a, b = (pkg.LbmDem(lx, ly, r, x1, x2, physics=phys) for _ in range(2))
    da, db = tmp_path / "sync", tmp_path / "async"
    da.mkdir(); db.mkdir()
    b.set_async_output(2)
    la, ra = a.run_scene(4100, outdir=str(da))
    lb, rb = b.run_scene(4100, outdir=str(db))
    assert ra == rb and ra["nfile"] == 3
    assert without_clock(la) == without_clock(lb)
    same_dirs(da, db, sum((vtk_names(k) for k in range(3)), []) + ["DEM000003.dat", "DEM000003.ps", "stats.data"])
    same_state(a, b)
    st = b.output_stats()
    assert (st["queued"], st["written"], st["failed"]) == (3, 3, 0)
    a.close(); b.close()


# ---- 5. back-pressure ---------------------------------------------------------------------------------------------------------------

def test_one_slot_never_drops_a_frame(pkg, tmp_path):
    lx, ly, r, x1, x2 = g4()
    a, b = pkg.LbmDem(lx, ly, r, x1, x2), pkg.LbmDem(lx, ly, r, x1, x2)
    da, db = tmp_path / "sync", tmp_path / "async"
    da.mkdir(); db.mkdir()
    b.set_async_output(1)
    for k in range(4):
        a.renderScene(12); b.renderScene(12)
        a.write_vtk(str(da), k)
        b.write_vtk_async(str(db), k)
    b.output_drain()
    same_dirs(da, db, sum((vtk_names(k) for k in range(4)), []))
    st = b.output_stats()
    assert (st["queued"], st["written"], st["failed"]) == (4, 4, 0)
    assert 0 <= st["slot_waits"] <= 3 and (st["slot_waits"] == 0) == (st["ms_slot_wait"] == 0.0)
    assert st["ms_io"] > 0.0
    same_state(a, b)
    # a change of the number of slots keeps nothing and loses nothing
    b.set_async_output(3)
    assert b.output_stats()["queued"] == 0
    b.write_vtk_async(str(db), 4); a.write_vtk(str(da), 4)
    b.set_async_output(0)            # drains
    same_dirs(da, db, sum((vtk_names(k) for k in range(5)), []))
    a.close(); b.close()


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------

def test_a_writer_failure_reaches_the_caller_and_the_handle_goes_on(pkg, tmp_path):
    lx, ly, r, x1, x2 = g4()
    a, b = pkg.LbmDem(lx, ly, r, x1, x2), pkg.LbmDem(lx, ly, r, x1, x2)
    b.set_async_output(2)
    missing = str(tmp_path / "not" / "there")
    a.renderScene(24); b.renderScene(24)
    b.write_vtk_async(missing, 0)          # queued: the failure is the writer's
    with pytest.raises(pkg.LbmDemError) as e:
        b.output_drain()
    assert e.value.code == -1 and missing in str(e.value)
    st = b.output_stats()
    assert (st["queued"], st["written"], st["failed"]) == (1, 0, 1)
    b.output_drain()                       # reported once
    # ... or at the next frame, which is then not queued
    b.write_vtk_async(missing, 1)
    deadline = time.monotonic() + 60
    while b.output_stats()["failed"] < 2 and time.monotonic() < deadline:
        time.sleep(0.01)
    assert b.output_stats()["failed"] == 2
    with pytest.raises(pkg.LbmDemError) as e:
        b.write_vtk_async(str(tmp_path), 2)
    assert missing in str(e.value) and b.output_stats()["queued"] == 2
    # the handle steps and writes a good frame
    a.renderScene(24); b.renderScene(24)
    da, db = tmp_path / "sync", tmp_path / "async"
    da.mkdir(); db.mkdir()
    a.write_vtk(str(da), 5); b.write_vtk_async(str(db), 5)
    b.output_drain()
    same_dirs(da, db, vtk_names(5))
    same_state(a, b)
    b.write_vtk_async(missing, 6)          # an unreported failure does not keep close() from returning
    b.close(); a.close()


# ---- 7. refusals, and the handles that are allowed --------------------------------------------------------------------------------

def test_refusals(pkg, tmp_path):
    lx, ly, r, x1, x2 = g4()
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    with pytest.raises(pkg.LbmDemError) as e:
        sim.write_vtk_async(str(tmp_path), 0)              # off by default
    assert e.value.code == -1 and "lbmdem_set_async_output" in str(e.value)
    sim.output_drain()                                     # fine and immediate while off
    for frames in (-1, 5):
        with pytest.raises(pkg.LbmDemError) as e:
            sim.set_async_output(frames)
        assert e.value.code == -1
    sim.set_async_output(4)
    sim.set_async_output(0)
    with pytest.raises(pkg.LbmDemError) as e:
        sim.write_vtk_async(str(tmp_path), 0)
    assert e.value.code == -1
    sim.set_async_output(1)
    with pytest.raises(pkg.LbmDemError) as e:
        sim.dist_enable()
    assert e.value.code == -1
    sim.close()
    strip = pkg.LbmDem(lx, ly, r, x1, x2, strip=(0, 128), halo=2)
    with pytest.raises(pkg.LbmDemError) as e:
        strip.set_async_output(2)
    assert e.value.code == -1
    with pytest.raises(pkg.LbmDemError):
        strip.vtk_image()
    strip.close()
    dist = pkg.LbmDem(lx, ly, r, x1, x2)
    dist.dist_enable()
    with pytest.raises(pkg.LbmDemError) as e:
        dist.set_async_output(2)
    assert e.value.code == -1
    dist.close()
    assert list(tmp_path.iterdir()) == []


def test_a_checkpoint_does_not_carry_the_setting(pkg, tmp_path):
    lx, ly, r, x1, x2 = g4()
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    sim.set_async_output(2)
    sim.renderScene(12)
    sim.checkpoint_save(str(tmp_path / "ck"))
    back = pkg.LbmDem.checkpoint_load(str(tmp_path / "ck"))
    with pytest.raises(pkg.LbmDemError):
        back.write_vtk_async(str(tmp_path), 0)
    sim.close(); back.close()


def test_vibrating_and_probing_handles_write_the_same_frames(pkg, tmp_path):
    lx, ly, r, x1, x2 = _vib_inputs("G4")
    phys = _shaker(pkg, lx, ly, r)
    for kind in ("vib", "probe"):
        sims = [pkg.LbmDem(lx, ly, r, x1, x2, physics=phys if kind == "vib" else None) for _ in range(2)]
        for s in sims:
            if kind == "vib":
                s.set_vibration(True)
            else:
                s.probe_enable(every=1, capacity=64, pressure_row=2, points=[(5, 5)])
        a, b = sims
        da, db = tmp_path / (kind + "_sync"), tmp_path / (kind + "_async")
        da.mkdir(); db.mkdir()
        b.set_async_output(2)
        for k in range(3):
            a.renderScene(50); b.renderScene(50)
            a.write_vtk(str(da), k); b.write_vtk_async(str(db), k)
        b.output_drain()
        same_dirs(da, db, sum((vtk_names(k) for k in range(3)), []))
        same_state(a, b)
        if kind == "probe":
            pa, pb = a.probe_read(), b.probe_read()
            for key in pa:
                assert np.array_equal(pa[key], pb[key]), key
        a.close(); b.close()


def test_the_float_build_writes_the_same_frames(pkg, tmp_path):
    lx, ly, r, x1, x2 = g4()
    a, b = (pkg.LbmDem(lx, ly, r, x1, x2, precision="f32") for _ in range(2))
    da, db = tmp_path / "sync", tmp_path / "async"
    da.mkdir(); db.mkdir()
    b.set_async_output(2)
    for k in range(2):
        a.renderScene(36); b.renderScene(36)
        a.write_vtk(str(da), k); b.write_vtk_async(str(db), k)
    b.output_drain()
    same_dirs(da, db, vtk_names(0) + vtk_names(1))
    a.close(); b.close()


def test_a_dry_run_queues_nothing(pkg, tmp_path):
    lx, ly, r, x1, x2 = g4()
    phys = pkg.derive(lx, ly, r).phys
    phys.stepFilm = 60
    sim = pkg.LbmDem(lx, ly, r, x1, x2, physics=phys)
    sim.set_async_output(2)
    lines, res = sim.run_scene(200, outdir=str(tmp_path), fluid=False)
    assert res["nfile"] == 3 and sim.output_stats()["queued"] == 0
    assert list(tmp_path.iterdir()) == []
    sim.close()


# ---- 8. a replayed run -------------------------------------------------------------------------------------------------------------

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
phys = pkg.derive(lx, ly, r).phys
phys.stepFilm = 90
a = pkg.LbmDem(lx, ly, r, x1, x2, physics=phys)          # the multi-sub-step kernel, one launch made to give up
b = pkg.LbmDem(lx, ly, r, x1, x2, physics=phys); b.set_dem_chain(0)
k = a.kinematics
k[:, 3:6] = np.random.default_rng(17).normal(0, 1, (len(r), 3)) * (0.05, 0.05, 30.0)
a.kinematics = k; b.kinematics = k
a.set_async_output(2)
a.debug_chain_giveup(3)        # inside the first stretch: the frame event of step 90 is the call that finds it
da, db = os.path.join(out, "a"), os.path.join(out, "b")
os.mkdir(da); os.mkdir(db)
la, ra = a.run_scene(345, outdir=da)
lb, rb = b.run_scene(345, outdir=db)
assert a.dem_chain_recoveries() == 1 and b.dem_chain_recoveries() == 0
assert ra == rb and ra["nfile"] == 3
st = a.output_stats()
assert (st["queued"], st["written"], st["failed"]) == (3, 3, 0), st
names = sorted(os.listdir(da))
assert names == sorted(os.listdir(db)) and len(names) == 15, names
for n in names:
    assert open(os.path.join(da, n), "rb").read() == open(os.path.join(db, n), "rb").read(), n
assert np.array_equal(a.f, b.f) and np.array_equal(a.kinematics, b.kinematics) and np.array_equal(a.obst, b.obst)
a.close(); b.close()
print("recovered: frames", len(names))
"""


def test_a_replayed_run_writes_the_frames_of_the_undisturbed_one(tmp_path):
    """A launch of the multi-sub-step DEM kernel that gives up (made to, in the experiment build, as
    tests/test_gpu_probes.py::test_a_replayed_run_records_every_fluid_step_once does) before a frame event: the writer
    settles the handle first -- the launch is undone, its sub-steps repeated -- and only then snapshots."""
    lib = os.path.join(ROOT, "2d-lbm-dem_amd", "liblbmdem_hip_ab.so")
    assert os.path.exists(lib), "run __graft_entry__.build()"
    env = dict(os.environ, LBMDEM_HIP_LIBRARY=lib)
    out = subprocess.run([sys.executable, "-c", GIVEUP_SCRIPT, str(tmp_path)], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "recovered: frames 15" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 9. the host driver ------------------------------------------------------------------------------------------------------------

def test_host_driver_async_output_writes_the_same_files(po, tmp_path):
    c = gu.CASES["G4_coupled_256x200"]
    outs = {}
    for mode, extra in (("sync", []), ("async", ["--async-output"]), ("async3", ["--async-output", "3"])):
        d = tmp_path / mode
        d.mkdir()
        sample = d / "packing.data"
        po.write_sample(str(sample), c["r_mm"], c["x_mm"], c["y_mm"])
        cmd = [EXE, str(sample), "--lx", "256", "--ly", "200", "--steps", "8001", "--run-stats"] + extra
        out = subprocess.run(cmd, capture_output=True, text=True, cwd=d, timeout=900)
        assert out.returncode == 0, (out.stdout[-400:], out.stderr[-1200:])
        outs[mode] = out
    expect = ["packing.data", "stats.data"] + vtk_names(0) + ["DEM%06d.%s" % (k, e) for k in (0, 1) for e in ("dat", "ps")]
    same_dirs(tmp_path / "sync", tmp_path / "async", expect)
    same_dirs(tmp_path / "sync", tmp_path / "async3")
    fd = lambda o: re.search(r"^final_density: ([0-9.]+)$", o.stderr, re.M).group(1)
    assert fd(outs["sync"]) == fd(outs["async"]) == fd(outs["async3"])
    assert "async_output" not in outs["sync"].stderr
    for mode in ("async", "async3"):
        m = re.search(r"^async_output: queued (\d+) written (\d+) failed (\d+) slot_waits (\d+) ms_slot_wait ([0-9.]+) "
                      r"ms_copy_wait ([0-9.]+) ms_io ([0-9.]+) ms_drain ([0-9.]+)$", outs[mode].stderr, re.M)
        assert m, outs[mode].stderr[-800:]
        assert [int(v) for v in m.groups()[:3]] == [1, 1, 0]
    console = lambda o: [l.split(" Time ")[0] for l in o.stdout.splitlines() if l.startswith(("Iteration Number", "steps "))]
    assert console(outs["sync"]) == console(outs["async"]) and len(console(outs["sync"])) >= 80
