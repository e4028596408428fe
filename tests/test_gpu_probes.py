"""GPU: the probe recorder (lbmdem_probe_*): the series it records every fluid step against goldens made from the unmodified
reference (tests/golden/probes_*.npz), bit for bit, on every path a fluid step is issued from; that it only observes; its
cadence, its full ring, a vibrating box, its refusals, and the host driver's --probes."""
import os
import subprocess

import numpy as np
import pytest

import probe_util as pu
import vib_util as vu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
NAMES = sorted(pu.CASES)


def _sim(pkg, name, **kw):
    case = pu.CASES[name]
    r, x1, x2 = pu.mpg.grains_m(case)
    return case, pkg.LbmDem(case["lx"], case["ly"], r, x1, x2, **kw)


def _steps(case, sim):
    return (case["fluid_steps"] - 1) * sim.cfg.npDEM + 1   # the last one is the sub-step of the last sampled fluid step


@pytest.mark.parametrize("how", ["chain", "one_launch_per_substep", "run_scene", "phases"])
@pytest.mark.parametrize("which_row", [0, 1], ids=["row2", "row_through_grains"])
@pytest.mark.parametrize("name", NAMES)
def test_series_equals_the_reference(pkg, name, which_row, how):
    case, sim = _sim(pkg, name)
    g = pu.golden(name)
    row = case["pressure_rows"][which_row]
    if which_row == 1:   # (the golden itself: this row really crosses grains, the velocity profile too)
        assert np.all(g[f"pressure_solid_{row}"] > 0) and np.all(g["velocity_on_grain"] > 0)
    sim.probe_enable(every=1, capacity=case["fluid_steps"] + 4, pressure_row=row, points=case["points"])
    n = _steps(case, sim)
    if how == "chain":
        sim.renderScene(n)                      # ONE call: the sub-steps between two fluid steps are single launches
        assert sim.dem_chain_stats()[0] > 0
    elif how == "one_launch_per_substep":
        sim.set_dem_chain(0)
        sim.renderScene(n)
        assert sim.dem_chain_stats()[0] == 0
    elif how == "run_scene":
        _, res = sim.run_scene(n)
        assert res["steps_done"] == n
    else:                                       # the phases one by one: the sample follows forces_fluid
        for s in range(n):
            if s % sim.cfg.npDEM == 0:
                sim.obst_construction(); sim.collision_streaming(); sim.forces_fluid()
            if s % sim.cfg.phys.updateVerlet == 0:
                sim.initVerlet()
            sim.dem_substep()
    got = sim.probe_read()
    assert got["dropped"] == 0
    pu.same_series(got, g, row, what=(name, how))
    assert np.array_equal(got["clock"], np.zeros(len(got["step"])))
    again = sim.probe_read()                    # the ring is empty now
    assert len(again["step"]) == 0 and again["dropped"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_the_recorder_only_observes(pkg, name):
    states = []
    for probes in (False, True):
        case, sim = _sim(pkg, name)
        if probes:
            sim.probe_enable(capacity=8, pressure_row=case["pressure_rows"][1], points=case["points"])   # (fills up on the way)
        sim.renderScene(_steps(case, sim) + 5)
        states.append((sim.f, sim.obst, sim.kinematics, sim.fhf, sim.nbsteps))
        if probes:
            got = sim.probe_read()
            assert len(got["step"]) == 8 and got["dropped"] == case["fluid_steps"] - 8
    for a, b in zip(*states):
        assert np.array_equal(a, b)


def test_every_third_fluid_step(pkg):
    name = NAMES[0]
    case, sim = _sim(pkg, name)
    row = case["pressure_rows"][0]
    sim.probe_enable(every=3, capacity=64, pressure_row=row, points=case["points"])
    sim.renderScene(_steps(case, sim))
    got = sim.probe_read()
    pu.same_series(got, pu.golden(name), row, rows=slice(0, None, 3), what="every=3")
    assert len(got["step"]) == (case["fluid_steps"] + 2) // 3 and got["dropped"] == 0


def test_full_ring_drops_and_counts_then_resumes(pkg):
    name = NAMES[0]
    case, sim = _sim(pkg, name)
    g, row, npdem = pu.golden(name), case["pressure_rows"][1], sim.cfg.npDEM
    cap, first = 5, 12
    assert first + cap < case["fluid_steps"]
    sim.probe_enable(every=1, capacity=cap, pressure_row=row, points=case["points"])
    sim.renderScene(first * npdem)              # fluid steps 0 .. first - 1
    got = sim.probe_read()
    assert len(got["step"]) == cap and got["dropped"] == first - cap
    pu.same_series(got, g, row, rows=slice(0, cap), what="the first ones are kept")
    sim.renderScene(3 * npdem)                  # recording resumes: fluid steps first .. first + 2
    got = sim.probe_read()
    assert got["dropped"] == 0
    pu.same_series(got, g, row, rows=slice(first, first + 3), what="after the read")


def test_fields_can_be_switched_off(pkg):
    name = NAMES[0]
    case, sim = _sim(pkg, name)
    g = pu.golden(name)
    sim.probe_enable(capacity=4, pressure_row=None, velocity_row=False, points=(), grain_extent=True)
    sim.renderScene(2 * sim.cfg.npDEM)
    got = sim.probe_read()
    assert sorted(got) == ["clock", "dropped", "height", "step", "time", "xgrainmax"]
    assert np.array_equal(got["xgrainmax"], g["xgrainmax"][:2]) and np.array_equal(got["height"], g["height"][:2])
    sim.probe_enable(capacity=4, pressure_row=2, velocity_row=False, points=case["points"][:1], grain_extent=False)   # replaces it
    sim.renderScene(sim.cfg.npDEM)
    got = sim.probe_read()
    assert sorted(got) == ["clock", "dropped", "point_pressure", "pressure_row", "step", "time"]
    assert np.array_equal(got["pressure_row"], g["pressure_row_2"][2:3])
    assert np.array_equal(got["point_pressure"], g["point_pressure"][2:3, :1])
    sim.probe_disable()
    with pytest.raises(pkg.LbmDemError) as e:
        sim.probe_read()
    assert e.value.code == -1


class _VibAsReference:
    """gives the vibrating oracle the method names make_probe_golden.run_case uses"""

    def __init__(self, ora): self.o = ora
    def scalars(self): return self.o.scalars()
    def get_grains(self): return self.o.get_grains()
    def get_f(self): return self.o.get_f()
    def get_obst(self): return self.o.get_obst()
    def steps(self, n): self.o.vib_steps(n)
    @property
    def nbsteps(self): return self.o.nbsteps


@pytest.mark.parametrize("chain", [True, False], ids=["chain", "one_launch_per_substep"])
def test_vibrating_box_against_the_vibrating_oracle(pkg, chain):
    name = NAMES[0]
    case = dict(pu.CASES[name], fluid_steps=20)
    lx, ly = case["lx"], case["ly"]
    r, x1, x2 = vu.with_wall_grains(*pu.mpg.grains_m(case), lx, ly)
    nsub = 20 * pkg.derive(lx, ly, r).npDEM
    phys = vu.physics(pkg, freq=1.4 / (nsub * pkg.derive(lx, ly, r).dt), amp=4.0 * 1e-4 / (0.5 * nsub))
    sim = pkg.LbmDem(lx, ly, r, x1, x2, physics=phys)
    ora = vu.VibOracle(lx, ly, r, x1, x2, phys=phys)
    row = case["pressure_rows"][1]
    if not chain:
        sim.set_dem_chain(0)
    sim.set_vibration(True)
    sim.probe_enable(capacity=32, pressure_row=row, points=case["points"])
    # the oracle's records, with the clock its walls show after each sampled sub-step's move
    clocks, want = [], []
    adapter = _VibAsReference(ora)
    for _ in range(case["fluid_steps"]):
        want.append(pu.mpg.sample_now(adapter, case))
        clocks.append(ora.walls()["t"])
        ora.vib_steps(sim.cfg.npDEM - 1)
    want = {k: np.array([w[k] for w in want]) for k in want[0]}
    sim.renderScene(case["fluid_steps"] * sim.cfg.npDEM)
    got = sim.probe_read()
    pu.same_series(got, want, row, what="vibrating")
    assert np.array_equal(got["clock"], np.array(clocks)) and clocks[-1] > clocks[0] > 0
    assert sim.walls() == ora.walls() and sim.walls()["Mgx"] > sim.cfg.dx   # the walls moved, by more than a node
    assert np.array_equal(sim.f, ora.get_f())


def test_refusals(pkg):
    name = NAMES[0]
    case = pu.CASES[name]
    r, x1, x2 = pu.mpg.grains_m(case)
    lx, ly = case["lx"], case["ly"]

    def refused(sim, **kw):
        with pytest.raises(pkg.LbmDemError) as e:
            sim.probe_enable(**kw)
        assert e.value.code == -1, e.value
        return str(e.value)

    strip = pkg.LbmDem(lx, ly, r, x1, x2, strip=(0, lx // 2), halo=12)
    assert "strip" in refused(strip)
    dist = pkg.LbmDem(lx, ly, r, x1, x2)
    dist.dist_enable()
    assert "distributed" in refused(dist)
    f32 = pkg.LbmDem(lx, ly, r, x1, x2, precision="f32")
    assert "single-precision" in refused(f32)
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    for pt in ((lx, 0), (0, ly), (-1, 3), (3, -1)):
        assert "outside" in refused(sim, points=[pt])
    assert "outside" in refused(sim, pressure_row=ly)
    refused(sim, every=0)
    refused(sim, capacity=0)
    refused(sim, points=[(1, 1)] * 65)
    assert "MiB" in refused(sim, capacity=2 ** 30)
    sim.probe_enable(capacity=4)
    with pytest.raises(pkg.LbmDemError) as e:    # a probing handle cannot become a distributed one
        sim.dist_enable()
    assert e.value.code == -1
    # checkpoints do not carry probes
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        sim.renderScene(3)
        sim.checkpoint_save(os.path.join(tmp, "c.ckpt"))
        back = pkg.LbmDem.checkpoint_load(os.path.join(tmp, "c.ckpt"))
        with pytest.raises(pkg.LbmDemError):
            back.probe_read()


def test_host_driver_probes(pkg, po, tmp_path):
    """lbmdem <sample> --probes FILE: FILE and the pressure_base files are what probe_read of the same run gives, formatted
    as the driver formats them; every other output file is byte-identical to a run without --probes. Fresh child processes."""
    name = NAMES[0]
    case = pu.CASES[name]
    sample = tmp_path / "sample.data"
    po.write_sample(str(sample), case["r_mm"], case["x_mm"], case["y_mm"])
    r, x1, x2 = po.read_sample(str(sample))
    lx, ly, nsteps = case["lx"], case["ly"], 8001    # one VTK frame, two write_DEM
    pts = case["points"][:3]
    base = [EXE, str(sample), "--lx", str(lx), "--ly", str(ly), "--steps", str(nsteps)]
    flags = ["--probes", "probes.txt", "--probe-every", "7", "--probe-row", "2"]
    for x, y in pts:
        flags += ["--probe-point", f"{x},{y}"]
    outs = {}
    for tag, extra in (("plain", []), ("probes", flags)):
        d = tmp_path / tag
        d.mkdir()
        out = subprocess.run(base + extra, capture_output=True, text=True, cwd=d, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        outs[tag] = out
    drop_time = lambda text: [l for l in text.splitlines() if "Time" not in l and "time" not in l]
    assert drop_time(outs["plain"].stdout) == drop_time(outs["probes"].stdout)
    plain = sorted(os.listdir(tmp_path / "plain"))
    extra_files = sorted(set(os.listdir(tmp_path / "probes")) - set(plain))
    for fn in plain:
        assert (tmp_path / "plain" / fn).read_bytes() == (tmp_path / "probes" / fn).read_bytes(), fn
    # the same run in Python
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    sim.probe_enable(every=7, capacity=4096, pressure_row=2, points=pts)
    sim.run_scene(nsteps)
    got = sim.probe_read()
    n = len(got["step"])
    fluid_steps = (nsteps - 1) // sim.cfg.npDEM + 1
    assert n == (fluid_steps + 6) // 7 and got["dropped"] == 0
    lines = []
    for k in range(n):
        line = "%d %e %e %e" % (got["step"][k], got["time"][k], got["xgrainmax"][k], got["height"][k])
        lines.append(line + "".join(" %e" % v for v in got["point_pressure"][k]))
    assert (tmp_path / "probes" / "probes.txt").read_text().splitlines() == lines
    assert extra_files == sorted(["probes.txt"] + ["pressure_base%06d.dat" % k for k in range(n)])
    pas = 1. / lx
    for k in range(n):
        want = "".join("%e %e\n" % (x * pas, got["pressure_row"][k, x]) for x in range(lx))
        assert (tmp_path / "probes" / ("pressure_base%06d.dat" % k)).read_text() == want, k
    # refused with several GPUs
    out = subprocess.run(base + flags + ["--gpus", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert out.returncode != 0 and "--probes" in out.stderr


GIVEUP_SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import __graft_entry__ as ge, samples
pkg = ge.load_package()
mode = sys.argv[1]
lx, ly = 512, 320
r, x, y = samples.row_packing(lx, ly, 700, seed=5)
r, x1, x2 = samples.to_metres(r, x, y)
a = pkg.LbmDem(lx, ly, r, x1, x2)          # the multi-sub-step kernel, one launch made to give up
b = pkg.LbmDem(lx, ly, r, x1, x2); b.set_dem_chain(0)
k = a.kinematics
k[:, 3:6] = np.random.default_rng(17).normal(0, 1, (len(r), 3)) * (0.05, 0.05, 30.0)
a.kinematics = k; b.kinematics = k
cap = 10 if mode == "full_ring" else 64
for s in (a, b):
    s.probe_enable(every=2, capacity=cap, pressure_row=12, points=[(5, 5), (250, 12), (500, 300)])
a.debug_chain_giveup(9 if mode == "inloop" else 3)
for n in ((345,) if mode == "inloop" else (37, 1, 12, 200, 95)):   # nothing but runs: fluid steps are sampled behind the failed launch
    a.renderScene(n); b.renderScene(n)
ra, rb = a.probe_read(), b.probe_read()
assert a.dem_chain_recoveries() == 1 and b.dem_chain_recoveries() == 0
fluid_steps = (345 - 1) // a.cfg.npDEM + 1
sampled = (fluid_steps + 1) // 2
assert len(rb["step"]) == min(sampled, cap) and rb["dropped"] == sampled - min(sampled, cap), (len(rb["step"]), rb["dropped"])
assert np.array_equal(rb["step"], np.arange(len(rb["step"])) * 2 * a.cfg.npDEM)   # every fluid step once, none twice
assert sorted(ra) == sorted(rb)
for key in ra:
    assert np.array_equal(ra[key], rb[key]), key
assert np.any(rb["pressure_row"] == 0.0) and np.any(rb["velocity_row"] != 0.0)
a.renderScene(40); b.renderScene(40)       # and it goes on recording
ra, rb = a.probe_read(), b.probe_read()
assert len(rb["step"]) > 0
for key in ra:
    assert np.array_equal(ra[key], rb[key]), key
assert np.array_equal(a.f, b.f) and np.array_equal(a.kinematics, b.kinematics)
print("recovered:", mode, len(rb["step"]))
"""


@pytest.mark.parametrize("mode", ["end", "full_ring", "inloop"])
def test_a_replayed_run_records_every_fluid_step_once(mode):
    """A launch of the multi-sub-step DEM kernel that gives up (made to, in the experiment build, as
    tests/test_gpu_dem_chain.py does) is undone and its sub-steps are repeated: the samples queued behind it find the stop
    word and write nothing, the recorder's counts go back with the handle, and the series equals that of a handle that never
    used the kernel -- with a ring that fills on the way, and when the run loop finds the failed launch itself."""
    import sys
    lib = os.path.join(ROOT, "2d-lbm-dem_amd", "liblbmdem_hip_ab.so")
    assert os.path.exists(lib), "run __graft_entry__.build()"
    env = dict(os.environ, LBMDEM_HIP_LIBRARY=lib)
    if mode == "inloop":
        env["LBMDEM_CHAIN_CAP"] = "2"
    out = subprocess.run([sys.executable, "-c", GIVEUP_SCRIPT, mode], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "recovered: " + mode in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
