"""GPU: lbmdem_run_scene -- the reference's main loop (main.c:1879-1890) as one library call -- against the same loop made
of one-sub-step calls with the writers called from Python at the reference's cadences: same state, same files, same
console lines; the stretches between two output events really reach the multi-sub-step DEM kernel; the stop condition;
and the host driver on top of it (`lbmdem --run-stats`), alone and as two ranks on the one GPU of the test box through
the library's own transport (the stand-in of tests/test_gpu_rccl_shim.py). All comparisons are exact."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util as gu
from test_gpu_rccl_shim import cut_sample, shim_env
from test_gpu_vibration import _inputs as _vib_inputs, _shaker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")


def _inputs(case):
    """G4 256x200 with the grains test_gpu_vibration.py puts against the left, right and top walls (the vibrating runs here
    need them); real_a08d83_600x500 as the golden file has it -- with those extra grains that packing does not stay finite
    beyond a few hundred sub-steps (test_gpu_vibration.py runs 250), and a state of NaNs compares nothing"""
    if case == "G4":
        return _vib_inputs("G4")
    g = gu.load("real_a08d83_600x500")
    return 600, 500, g["r"], g["x1"], g["x2"]


class SteppedByOne:
    """renderScene() one call at a time with everything the reference's loop hangs on the step counter (main.c:1697-1777,
    1880-1890), as the host driver did before the library had the loop"""

    def __init__(self, sim, outdir, fluid=True, duration=-1.0):
        self.sim, self.outdir, self.fluid, self.duration = sim, str(outdir), fluid, duration
        self.energies = (0.0,) * 8
        self.lines = []

    def run(self, n):
        sim, cfg = self.sim, self.sim.cfg
        npDEM, updateVerlet, stepFilm, dt = cfg.npDEM, cfg.phys.updateVerlet, cfg.phys.stepFilm, cfg.dt
        nFile = sim.nbsteps // stepFilm
        first, stopped = sim.nbsteps, False
        for _ in range(n):
            s = sim.nbsteps
            if self.fluid and s % npDEM == 0 and s % 400 == 0:
                if sim.vibrating:
                    sim.move_walls()
                sim.lbm_step()
                self.lines.append("Iteration Number %d, Total density in the system %f\n" % (s, sim.check_density()))
                if s % updateVerlet == 0:
                    sim.initVerlet()
                sim.dem_substep()
            elif self.fluid:
                sim.renderScene(1)
            else:
                sim.renderScene_dry(1)
            s = sim.nbsteps
            if s % stepFilm == 0:
                if self.fluid:
                    sim.write_vtk(self.outdir, nFile)
                nFile += 1
            if s % 4000 == 0:
                self.energies = sim.write_DEM(self.outdir, nFile)
                sim.write_forces(self.outdir, nFile)
            if s % updateVerlet == 0:
                e = self.energies
                self.lines.append("steps %d steps %e KE %e PE %e SE %e WF %e INCE %e SLIP %e RW %e Time " %
                                  (s, s * dt, e[0], e[1], e[2], e[4], e[5], e[6], e[7]))
            if self.duration >= 0 and s * dt > self.duration:
                stopped = True
                break
        return dict(steps_done=sim.nbsteps - first, nfile=nFile, stopped=stopped, energies8=tuple(self.energies))


def without_clock(lines):
    """the "steps" line ends with asctime: cut it off behind "Time " """
    out = []
    for l in lines:
        if l.startswith("steps "):
            assert re.search(r" Time \w{3} \w{3} [ \d]\d \d\d:\d\d:\d\d \d{4}\n \n$", l), repr(l)
            l = l[:l.index(" Time ") + 6]
        out.append(l)
    return out


def same_state(a, b, fluid=True):
    assert a.nbsteps == b.nbsteps
    k = a.kinematics
    assert np.isfinite(k).all()
    assert np.array_equal(k, b.kinematics)
    assert np.array_equal(a.fhf, b.fhf)
    if fluid:
        assert np.array_equal(a.obst, b.obst)
        assert np.array_equal(a.f, b.f)
    assert a.walls() == b.walls()


def same_files(da, db, expect):
    names = sorted(p.name for p in da.iterdir())
    assert names == sorted(p.name for p in db.iterdir())
    assert names == sorted(expect), names
    for n in names:
        assert (da / n).read_bytes() == (db / n).read_bytes(), n


VTK = ["%s_%06d.vtk" % (f, 0) for f in ("fluid_pressure", "fluid_velocity", "grain_acceleration", "grain_pressure", "grain_velocity")]
TABLES = ["DEM000000.dat", "DEM000000.ps", "DEM000001.dat", "DEM000001.ps", "stats.data"]


def pair(pkg, case, tmp_path, vib=False, total=8200):
    lx, ly, r, x1, x2 = _inputs(case)
    phys = _shaker(pkg, lx, ly, r, n=total) if vib else None
    sims = [pkg.LbmDem(lx, ly, r, x1, x2, physics=phys) for _ in range(2)]
    if vib:
        for s in sims:
            s.set_vibration(True)
    dirs = [tmp_path / "scene", tmp_path / "stepped"]
    for d in dirs:
        d.mkdir()
    return sims[0], sims[1], dirs[0], dirs[1]


def check_scene_against_stepped(pkg, tmp_path, case, calls, fluid=True, vib=False):
    total = sum(calls)
    assert total == 8200   # crosses console densities, film-law sub-steps 0 and 8000, table sub-steps 3999 and 7999, one frame
    a, b, da, db = pair(pkg, case, tmp_path, vib=vib, total=total)
    ref = SteppedByOne(b, db, fluid=fluid)
    lines = []
    for n in calls:
        got_lines, got = a.run_scene(n, outdir=str(da), fluid=fluid)
        want = ref.run(n)
        lines += got_lines
        last = got.pop("last_density")
        assert got == want
        same_state(a, b, fluid=fluid)
    assert without_clock(lines) == ref.lines
    assert a.dem_chain_recoveries() == 0
    densities = [l for l in lines if l.startswith("Iteration Number")]
    lcm = math.lcm(a.cfg.npDEM, 400)
    assert len(densities) == ((total - 1) // lcm + 1 if fluid else 0)
    last_step = (total - 1) // lcm * lcm
    if fluid and last_step >= total - calls[-1]:   # (the last call saw it: its result carries the sum)
        assert densities[-1] == "Iteration Number %d, Total density in the system %f\n" % (last_step, last)
    assert sum(l.startswith("steps ") for l in lines) == 82
    same_files(da, db, TABLES + (VTK if fluid else []))
    if vib:
        assert a.walls()["t"] > 0.0 and a.walls()["Mgx"] != a.cfg.Mgx
    a.close(); b.close()


@pytest.mark.parametrize("calls", [(8200,), (3977, 4223), (4100, 4100)], ids=["one_call", "two_calls", "two_calls_energies_kept"])
@pytest.mark.parametrize("case", ["G4", "a08d83"])
def test_coupled_same_state_files_and_lines(pkg, tmp_path, case, calls):
    """(4100 + 4100: the second call's "steps" lines up to 7900 print what the first call's write_DEM left in the handle)"""
    check_scene_against_stepped(pkg, tmp_path, case, calls)


@pytest.mark.parametrize("calls", [(8200,), (3977, 4223)], ids=["one_call", "two_calls"])
def test_without_the_fluid_same_state_files_and_lines(pkg, tmp_path, calls):
    check_scene_against_stepped(pkg, tmp_path, "G4", calls, fluid=False)


@pytest.mark.parametrize("fluid", [True, False], ids=["coupled", "dry"])
def test_vibrating_same_state_files_and_lines(pkg, tmp_path, fluid):
    check_scene_against_stepped(pkg, tmp_path, "G4", (3977, 4223), fluid=fluid, vib=True)


def test_the_fast_path_is_what_ran(pkg):
    """between two output events the sub-steps go to the run loop in one piece: runs of ordinary sub-steps are single launches
    of the multi-sub-step kernel, whose tail rasterises and leaves the change bits the fused fluid kernel uses. (A handle
    stepped by one sub-step per call has all of these counters at 0.)"""
    lx, ly, r, x1, x2 = _inputs("G4")
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    n = 2400
    lines, res = sim.run_scene(n)
    assert res["steps_done"] == n and not res["stopped"] and res["nfile"] == 0
    launches, substeps, _, _ = sim.dem_chain_stats()
    assert substeps >= 0.9 * n, (launches, substeps)
    assert launches <= math.ceil(n / sim.cfg.npDEM) + 24 + 2, (launches, sim.cfg.npDEM)   # one per fluid step, rebuild, special sub-step
    assert sim.dem_chain_paints() > 0
    assert sim.change_mask_stats()[0] > 0
    assert sim.dem_chain_recoveries() == 0
    assert sum(l.startswith("steps ") for l in lines) == 24
    sim.close()


def test_the_host_driver_reaches_the_fast_path(po, tmp_path):
    c = gu.CASES["G4_coupled_256x200"]
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), c["r_mm"], c["x_mm"], c["y_mm"])
    cmd = [EXE, str(sample), "--lx", "256", "--ly", "200", "--steps", "2400"]
    out = subprocess.run(cmd + ["--run-stats"], capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    m = re.search(r"^dem_chain: launches (\d+) substeps (\d+) recoveries (\d+) paints (\d+)$", out.stderr, re.M)
    assert m, out.stderr[-600:]
    launches, substeps, recoveries, paints = map(int, m.groups())
    npDEM = int(re.search(r"npDEM=(\d+)", out.stdout).group(1))
    assert substeps >= 2160 and recoveries == 0 and paints > 0 and 0 < launches <= math.ceil(2400 / npDEM) + 24 + 2
    assert int(re.search(r"dem_steps: (\d+)", out.stderr).group(1)) == 2400
    # without the option: the same lines but that one
    plain = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert plain.returncode == 0 and "dem_chain" not in plain.stderr
    key = lambda o: [l.split(":")[0] for l in o.stderr.splitlines()]
    assert key(out) == key(plain) + ["dem_chain"]
    fd = lambda o: re.search(r"final_density: ([0-9.]+)", o.stderr).group(1)
    assert fd(out) == fd(plain)


@pytest.mark.parametrize("fluid", [True, False], ids=["coupled", "dry"])
def test_stop_in_the_middle_of_a_stretch(pkg, tmp_path, fluid):
    """duration such that the loop's own test, nbsteps * dt > duration after every sub-step, first holds at step 4130 -- 30
    sub-steps into a stretch of 100 without events"""
    a, b, da, db = pair(pkg, "G4", tmp_path)
    want_steps = 4130
    duration = (want_steps - 0.5) * a.cfg.dt
    ref = SteppedByOne(b, db, fluid=fluid, duration=duration)
    lines, got = a.run_scene(8200, outdir=str(da), fluid=fluid, duration=duration)
    want = ref.run(8200)
    got.pop("last_density")
    assert got == want and got["steps_done"] == want_steps and got["stopped"] and got["nfile"] == 0
    same_state(a, b, fluid=fluid)
    assert without_clock(lines) == ref.lines
    same_files(da, db, ["DEM000000.dat", "DEM000000.ps", "stats.data"])
    # a second call starts beyond the stop: the do-while makes one sub-step, then stops again
    lines, got = a.run_scene(50, outdir=str(da), fluid=fluid, duration=duration)
    assert got["steps_done"] == 1 and got["stopped"] and a.nbsteps == want_steps + 1
    a.close(); b.close()


def test_no_outdir_writes_nothing_and_counts_the_frames(pkg, tmp_path):
    lx, ly, r, x1, x2 = _inputs("G4")
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        lines, res = sim.run_scene(8001)
    finally:
        os.chdir(cwd)
    assert list(tmp_path.iterdir()) == []
    assert res["steps_done"] == 8001 and res["nfile"] == 1 and res["energies8"] == (0.0,) * 8
    assert lines[0].startswith("Iteration Number 0,") and sum(l.startswith("steps ") for l in lines) == 80
    sim.close()


def test_float_build_runs_the_loop(pkg, tmp_path):
    """liblbmdem_hip_sp.so: the loop, its lines and the VTK frame as in the double build. (write_DEM / write_forces do not
    exist there: a run that reaches step 4000 with a directory fails with LBMDEM_EINVAL, by their own refusal.)"""
    lx, ly, r, x1, x2 = _inputs("G4")
    phys = pkg.derive(lx, ly, r, precision="f32").phys
    phys.stepFilm = 250
    sim = pkg.LbmDem(lx, ly, r, x1, x2, precision="f32", physics=phys)
    lines, res = sim.run_scene(249, outdir=str(tmp_path))
    assert res["steps_done"] == 249 and res["nfile"] == 0
    assert [l.split(" KE ")[0].split(",")[0] for l in lines] == ["Iteration Number 0", "steps 100 steps %e" % (100 * sim.cfg.dt),
                                                                 "steps 200 steps %e" % (200 * sim.cfg.dt)]
    lines, res = sim.run_scene(250, outdir=str(tmp_path))      # the float build has write_vtk: the frame of step 250
    assert res["steps_done"] == 250 and res["nfile"] == 1 and sim.nbsteps == 499
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(VTK)
    sim.close()


def test_two_ranks_on_one_gpu_write_the_single_gpu_files(po, tmp_path):
    """`lbmdem --gpus 2 --devices 0,0 --run-stats` (lbmdem_run_scene over lbmdem_comm_run on every rank) against `lbmdem`.
    (No chain sub-steps are asserted: with two ranks sharing one GPU the census may rightly find that the tiles of both do
    not fit at once, and one launch per sub-step is then the correct answer.)"""
    lx, ly = 640, 160
    r, x, y, _ = cut_sample(lx, ly, 230, seed=36)
    outs = {}
    for mode, extra in (("single", []), ("two", ["--gpus", "2", "--devices", "0,0"])):
        d = tmp_path / mode
        d.mkdir()
        sample = d / "packing.data"
        po.write_sample(str(sample), r, x, y)
        cmd = [EXE, str(sample), "--lx", str(lx), "--ly", str(ly), "--steps", "8000", "--run-stats"] + extra
        out = subprocess.run(cmd, capture_output=True, text=True, cwd=d, env=shim_env(), timeout=900)
        assert out.returncode == 0, (out.stdout[-400:], out.stderr[-1200:])
        outs[mode] = out
    a, b = tmp_path / "single", tmp_path / "two"
    same_files(a, b, ["packing.data"] + TABLES + VTK)
    fd = lambda o: re.search(r"final_density: ([0-9.]+)", o.stderr).group(1)
    assert fd(outs["single"]) == fd(outs["two"])
    assert "(2 GPUs)" in outs["two"].stderr
    for o in outs.values():
        m = re.search(r"^dem_chain: launches (\d+) substeps (\d+) recoveries (\d+) paints (\d+)$", o.stderr, re.M)
        assert m and int(m.group(3)) == 0, o.stderr[-600:]
    console = lambda o: [l for l in o.stdout.splitlines() if l.startswith(("Iteration Number", "steps "))]
    assert [l.split(" Time ")[0] for l in console(outs["single"])] == [l.split(" Time ")[0] for l in console(outs["two"])]
    assert len(console(outs["single"])) >= 80
