"""GPU: vibrating side walls (the reference's vib = 1, main.c:1700-1705; lbmdem_set_vibration) against the CPU oracle with
the same block in front of its renderScene (tests/vib_oracle/vib_oracle.c): populations, obstacle map, hydrodynamic forces,
grain kinematics and the walls, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import vib_util as vu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
N = 250   # >= 3 fluid steps (npDEM ~ 12) and 3 Verlet rebuilds (0, 100, 200)


def _inputs(case):
    if case == "G4":
        lx, ly = 256, 200
        r, x1, x2 = gu.inputs_m("G4_coupled_256x200")
    else:
        lx, ly = 600, 500
        g = gu.load("real_a08d83_600x500")
        r, x1, x2 = g["r"], g["x1"], g["x2"]
    r, x1, x2 = vu.with_wall_grains(r, x1, x2, lx, ly)
    return lx, ly, r, x1, x2


def _shaker(pkg, lx, ly, r, n=N, amp_nodes=4.0):
    """freq, amp such that freq * t sweeps ~1.4 rad over n sub-steps and the left wall moves ~amp_nodes nodes to the right"""
    dt = pkg.derive(lx, ly, r).dt
    phys = vu.physics(pkg, freq=1.4 / (n * dt), amp=0.0)
    phys.amp = amp_nodes * 1e-4 / (0.5 * n)
    return phys


def _pair(pkg, case, amp_nodes=4.0):
    lx, ly, r, x1, x2 = _inputs(case)
    phys = _shaker(pkg, lx, ly, r, amp_nodes=amp_nodes)
    sim = pkg.LbmDem(lx, ly, r, x1, x2, physics=phys)
    ora = vu.VibOracle(lx, ly, r, x1, x2, phys=phys)
    return sim, ora


def _same_walls(sim, ora):
    a, b = sim.walls(), ora.walls()
    assert a == b, (a, b)


def _same_state(sim, ora, fluid=True):
    k = sim.kinematics
    assert np.array_equal(k, ora.get_grains()[:, :9]), sim.nbsteps
    assert np.array_equal(sim.fhf, ora.get_fhf()), sim.nbsteps
    if fluid:
        assert np.array_equal(sim.obst, ora.get_obst()), sim.nbsteps
        assert np.array_equal(sim.f, ora.get_f()), sim.nbsteps
    _same_walls(sim, ora)


@pytest.mark.parametrize("chain", [True, False], ids=["chain", "one_launch_per_substep"])
@pytest.mark.parametrize("case", ["G4", "a08d83"])
def test_coupled_vibration_matches_the_oracle(pkg, case, chain):
    sim, ora = _pair(pkg, case)
    cfg = sim.cfg
    assert cfg.npDEM * 3 < N
    if not chain:
        sim.set_dem_chain(0)
    sim.set_vibration(True)
    assert sim.vibrating
    mgx0 = sim.walls()["Mgx"]
    contacts = {"left": 0, "right": 0, "top": 0}
    for n in (1, 36, 63, 100, 50):                   # runs that end on and off fluid steps and rebuilds
        sim.renderScene(n)
        ora.vib_steps_counting(n, contacts)
        _same_walls(sim, ora)
    _same_state(sim, ora)
    assert sim.walls()["Mgx"] - mgx0 > cfg.dx        # the raster really shifted: more than one node
    # the wall laws of all three walls that can be reached really ran, each in many sub-steps (left: with the moving Mgx)
    assert min(contacts.values()) >= 20, contacts
    launches = sim.dem_chain_stats()[0]
    assert (launches > 0) == chain
    sim.close()


def test_change_bits_verified_and_the_chain_used_while_vibrating(pkg):
    """set_change_mask(2) checks every fused launch's bits against both maps: nothing hidden. The multi-sub-step kernel did
    the sub-steps (one launch per fluid step), so the vibrating path is the fast one."""
    sim, ora = _pair(pkg, "G4")
    sim.set_change_mask(2)
    sim.set_vibration(True)
    sim.renderScene(N)
    ora.vib_steps(N)
    _same_state(sim, ora)
    assert sim.change_mask_stats()[1] == 0
    launches, substeps, _, _ = sim.dem_chain_stats()
    assert substeps > N * 0.9
    assert launches <= -(-N // sim.cfg.npDEM) + 3 + 1   # at most one launch per fluid step, rebuild and film sub-step
    sim.close()


def test_dry_vibration_matches_the_oracle(pkg):
    """renderScene_dry (the reference without _FLUIDE_) shaken: the classic vibrated bed"""
    sim, ora = _pair(pkg, "G4")
    sim.set_vibration(True)
    for n in (150, 250):
        sim.renderScene_dry(n)
        ora.vib_steps_dry(n)
        _same_state(sim, ora, fluid=False)
    assert np.all(sim.fhf == 0.0)
    sim.close()


def test_checkpoint_of_a_vibrating_run_goes_on_vibrating(pkg, tmp_path):
    sim, ora = _pair(pkg, "G4")
    sim.set_vibration(True)
    sim.renderScene(130)
    path = str(tmp_path / "vib.ckpt")
    sim.checkpoint_save(path)
    back = pkg.LbmDem.checkpoint_load(path)
    assert back.vibrating
    assert back.walls() == sim.walls()
    sim.renderScene(N - 130)
    back.renderScene(N - 130)
    ora.vib_steps(N)
    _same_state(back, ora)
    _same_state(sim, ora)
    back.close(); sim.close()


def test_zero_amplitude_is_the_still_box(pkg):
    """a vibrating handle with amp = 0 computes what a handle that does not vibrate computes (the default path is untouched)"""
    lx, ly, r, x1, x2 = _inputs("G4")
    phys = _shaker(pkg, lx, ly, r)
    phys.amp = 0.0
    a = pkg.LbmDem(lx, ly, r, x1, x2, physics=phys)
    b = pkg.LbmDem(lx, ly, r, x1, x2, physics=phys)
    a.set_vibration(True)
    a.renderScene(N)
    b.renderScene(N)
    assert np.array_equal(a.f, b.f)
    assert np.array_equal(a.obst, b.obst)
    assert np.array_equal(a.fhf, b.fhf)
    assert np.array_equal(a.kinematics, b.kinematics)
    wa, wb = a.walls(), b.walls()
    assert wa["Mgx"] == wb["Mgx"] and wa["Mdx"] == wb["Mdx"] and wa["t"] > wb["t"]
    a.close(); b.close()


def _lines(path):
    return [l for l in open(path).read().splitlines() if not l.startswith("#")]


@pytest.mark.parametrize("dry", [False, True], ids=["coupled", "dry"])
def test_host_driver_vib_writes_what_the_library_writes(pkg, po, tmp_path, dry):
    """`lbmdem <sample> --vib` (and with --dry): DEM*.dat, stats.data and the VTK frame byte-identical to the same run
    driven from Python and written by the library's writers"""
    c = gu.CASES["G4_coupled_256x200"]
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), c["r_mm"], c["x_mm"], c["y_mm"])
    freq, amp = 60.0, 2e-8
    drv = tmp_path / "driver"
    drv.mkdir()
    cmd = [EXE, str(sample), "--lx", "256", "--ly", "200", "--steps", "8000", "--vib", "--vib-freq", str(freq),
           "--vib-amp", str(amp)] + (["--dry"] if dry else [])
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=drv, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    lib = tmp_path / "library"
    lib.mkdir()
    r, x1, x2 = pkg.read_sample(str(sample))
    phys = vu.physics(pkg, freq=freq, amp=amp, dtt=0.0)
    sim = pkg.LbmDem(256, 200, r, x1, x2, physics=phys)
    sim.set_vibration(True)
    step = sim.renderScene_dry if dry else sim.renderScene
    step(4000)
    sim.write_DEM(str(lib), 0)
    step(4000)
    if not dry:
        sim.write_vtk(str(lib), 0)
    sim.write_DEM(str(lib), 1)
    for name in ("DEM000000.dat", "DEM000001.dat"):
        assert open(drv / name, "rb").read() == open(lib / name, "rb").read(), name
    assert _lines(drv / "stats.data") == _lines(lib / "stats.data")
    vtk = sorted(p.name for p in drv.glob("*.vtk"))
    assert len(vtk) == (0 if dry else 5)
    for name in vtk:
        assert open(drv / name, "rb").read() == open(lib / name, "rb").read(), name
    assert sim.walls()["t"] > 0.0
    sim.close()


def test_vibration_is_refused_on_strips_distributed_grains_and_the_float_build(pkg):
    lx, ly, r, x1, x2 = _inputs("G4")
    strip = pkg.LbmDem(lx, ly, r, x1, x2, strip=(0, 128), halo=2)
    with pytest.raises(pkg.LbmDemError) as e:
        strip.set_vibration(True)
    assert e.value.code == -1
    strip.close()
    dist = pkg.LbmDem(lx, ly, r, x1, x2)
    dist.dist_enable()
    with pytest.raises(pkg.LbmDemError) as e:
        dist.set_vibration(True)
    assert e.value.code == -1
    dist.close()
    vib = pkg.LbmDem(lx, ly, r, x1, x2)
    vib.set_vibration(True)
    with pytest.raises(pkg.LbmDemError) as e:
        vib.dist_enable()
    assert e.value.code == -1
    vib.close()
    sp = pkg.LbmDem(lx, ly, r, x1, x2, precision="f32")
    with pytest.raises(pkg.LbmDemError) as e:
        sp.set_vibration(True)
    assert e.value.code == -1
    sp.close()
