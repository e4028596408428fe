"""GPU: the coarse-grained fields (lbmdem_coarse_fields, lbmdem_write_coarse, lbmdem_set_coarse_output; include/lbmdem_hip.h)
against their numpy restatement (tests/coarse_util.py) over the handle's pinned downloads: every member of every cell exactly
equal, no tolerance."""
import ctypes
import os

import numpy as np
import pytest

import coarse_util as cz
import golden_util as gu
import samples

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(HERE, "golden", "dem_G6_4000steps")
ODD = "S_127x121"   # lx % 8 = 7, ly % 16 = 9


def g6():
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    return z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3


def check(sim, r, cw, ch, table="ask"):
    """the export equals the restatement; -> (cells, outside, contacts_valid)"""
    cells, outside, valid = sim.coarse_fields(cw, ch)
    want, want_outside, want_valid = cz.expected(sim, r, cw, ch, table)
    assert cells.shape == want.shape == cz.grid(sim.lx, sim.ly, cw, ch)
    bad = cz.mismatches(cells, want)
    print(f"{sim.lx}x{sim.ly} cells {cw}x{ch}: members that differ {bad}, outside {outside}/{want_outside}, table {valid}/{want_valid}")
    assert bad == []
    assert (outside, valid) == (want_outside, want_valid)
    assert cells["nodes"].sum() == sim.lx * sim.ly and cells["grains"].sum() + outside == sim.n
    return cells, outside, valid


@pytest.fixture(scope="module")
def coupled(pkg):
    """the G6 packing on 256 x 200 after five fluid periods and three more sub-steps, through the multi-sub-step kernel"""
    r, x, y = g6()
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.renderScene(5 * sim.cfg.npDEM + 3)
        yield sim, r


@pytest.mark.parametrize("cw,ch", [(16, 16), (7, 13), (60, 17), (1, 1), (256, 200), (300, 300), (5, 200), (256, 3)])
def test_coupled_state(coupled, cw, ch):
    sim, r = coupled
    cells, outside, valid = check(sim, r, cw, ch)
    assert valid == 0 and not any(cells[name].any() for name in cz.CONTACT_BLOCK)
    assert cells["grain_nodes"].sum() > 0 and cells["wall_nodes"].sum() > 0
    assert cells["sum_rho"].sum() > 0 and np.abs(cells["sum_fhf2"]).sum() > 0 and np.abs(cells["sum_mv2"]).sum() > 0


@pytest.mark.parametrize("cw,ch", [(16, 16), (9, 31)])
def test_odd_lattice(pkg, cw, ch):
    """127 x 121: the last cell is cut both ways; ch = 16 leaves a last segment of 9 nodes, ch = 31 segments longer than a tile
    of the population layout that begin and end inside one"""
    c = gu.CASES[ODD]
    assert c["lx"] % 8 != 0 and c["ly"] % 16 != 0 and c["lx"] % cw != 0 and c["ly"] % ch != 0
    a = gu.GpuAdapter(pkg, ODD)
    try:
        a.set_kinematics(gu.mg.shape_initial_kinematics(c))
        a.sim.renderScene(2 * a.sim.cfg.npDEM + 1)
        cells, _, _ = check(a.sim, gu.inputs_m(ODD)[0], cw, ch)
        assert cells["nodes"][-1, -1] == (c["lx"] - (cells.shape[0] - 1) * cw) * (c["ly"] - (cells.shape[1] - 1) * ch)
    finally:
        a.sim.close()


@pytest.mark.parametrize("n,cw,ch", [(1025, 128, 64), (1, 64, 64), (63, 64, 64), (64, 64, 64), (65, 64, 64)])
def test_crowded_and_empty_cells(pkg, n, cw, ch):
    r, x, y = samples.to_metres(*samples.row_packing(256, 200, n, rmin=0.2, rmax=0.2))
    assert len(r) == n
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.renderScene(2)
        cells, outside, _ = check(sim, r, cw, ch)
        assert outside == 0 and (cells["grains"] == 0).any()
        if n == 1025:
            assert (cells["grains"] > 256).any()


def test_outside_grains(pkg):
    n = 65
    r, x, y = samples.to_metres(*samples.row_packing(256, 200, n, seed=29))
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.renderScene(2)
        dx = sim.config().dx
        k = sim.kinematics
        k[5, 0] = dx * 256 * 1.5          # beyond the right edge
        k[17, 0] = -1.0e-5                # left of the lattice
        k[40, 1] = dx * 200 * (1 - 1e-9)  # just below the top edge: inside, in the last row of cells
        sim.kinematics = k
        cells, outside, _ = check(sim, r, 16, 16)
        assert outside == 2 and cells["grains"].sum() == n - 2
        assert cells["grains"][:, -1].sum() >= 1


def test_contact_block(pkg):
    n = 65
    r, x, y = samples.to_metres(*samples.row_packing(256, 200, n, seed=29, touch_prob=1.0))
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.renderScene(2)
        sim.set_diagnostics(True)
        sim.dem_substep()
        cells, _, valid = check(sim, r, 16, 16, table=sim.grain_table())
        assert valid == 1 and (cells["sum_z"] > 0).any() and cells["sum_z"].sum() == sim.grain_table()[:, 28].sum()
        assert any(cells[name].any() for name in ("sum_p", "M11", "M22"))
        sim.set_diagnostics(False)
        sim.dem_substep()
        cells, _, valid = check(sim, r, 16, 16, table=None)
        assert valid == 0 and not any(cells[name].any() for name in cz.CONTACT_BLOCK)
        with pytest.raises(pkg.LbmDemError):   # (the restatement had no table to ask for either)
            sim.grain_table()


def test_vibrating_handle(pkg):
    r, x, y = g6()
    phys = pkg.Physics()
    pkg.load_library().lbmdem_physics_defaults(ctypes.byref(phys))
    phys.freq, phys.amp = 900.0, 2.0e-6
    with pkg.LbmDem(256, 200, r, x, y, physics=phys) as sim:
        Mgx0 = sim.walls()["Mgx"]
        sim.set_vibration(True)
        sim.renderScene(300)
        assert sim.walls()["Mgx"] != Mgx0   # the wall the cells are measured from has moved
        check(sim, r, 16, 16)
        check(sim, r, 7, 13)


def test_export_does_not_interfere(pkg):
    r, x, y = g6()
    with pkg.LbmDem(256, 200, r, x, y) as a, pkg.LbmDem(256, 200, r, x, y) as b:
        period = a.cfg.npDEM
        for _ in range(3):
            a.renderScene(period); b.renderScene(period)
            first = a.coarse_fields(16, 16)
            a.coarse_fields(1, 1)
            again = a.coarse_fields(16, 16)   # (behind a finer grid: the scratch has been grown in between)
            assert first[1:] == again[1:] and cz.mismatches(first[0], again[0]) == []
        for what in ("f", "obst", "fhf", "kinematics"):
            assert np.array_equal(getattr(a, what), getattr(b, what)), what
        assert a.nbsteps == b.nbsteps == 3 * period


def test_sizing_and_refusals(pkg, tmp_path):
    L = pkg.load_library()
    r, x, y = samples.to_metres(*samples.row_packing(256, 200, 65, seed=29))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.renderScene(2)
        cnt, info = ctypes.c_long(-1), np.zeros(2, np.int64)
        assert L.lbmdem_coarse_fields(sim._h, 16, 16, None, 0, ctypes.byref(cnt), vp(info)) == 0 and cnt.value == 16 * 13
        small = np.full((16 * 13 - 1, 25), 7.0)
        cnt.value = -1
        assert L.lbmdem_coarse_fields(sim._h, 16, 16, vp(small), len(small), ctypes.byref(cnt), vp(info)) == -1
        assert cnt.value == 16 * 13 and (small == 7.0).all()
        roomy = np.full((16 * 13 + 3, 25), 7.0)
        assert L.lbmdem_coarse_fields(sim._h, 16, 16, vp(roomy), len(roomy), ctypes.byref(cnt), vp(info)) == 0
        assert cnt.value == 16 * 13 and (roomy[16 * 13:] == 7.0).all()
        assert np.array_equal(roomy[:16 * 13].reshape(16, 13, 25), sim.coarse_fields(16, 16)[0].view(np.float64).reshape(16, 13, 25))
        for cw, ch in ((0, 16), (16, 0), (-3, 16)):
            with pytest.raises(pkg.LbmDemError) as e:
                sim.coarse_fields(cw, ch)
            assert e.value.code == -1
            with pytest.raises(pkg.LbmDemError):
                sim.write_coarse(str(tmp_path), 0, cw, ch)
            with pytest.raises(pkg.LbmDemError):
                sim.set_coarse_output(cw, ch)
        assert L.lbmdem_coarse_fields(sim._h, 16, 16, vp(roomy), len(roomy), None, vp(info)) == -1
        assert L.lbmdem_coarse_fields(sim._h, 16, 16, vp(roomy), len(roomy), ctypes.byref(cnt), None) == -1
        assert L.lbmdem_coarse_fields(sim._h, 16, 16, None, 5, ctypes.byref(cnt), vp(info)) == -1
        with pytest.raises(pkg.LbmDemError, match="cannot open"):
            sim.write_coarse(str(tmp_path / "not" / "there"), 0, 16, 16)
        sim.set_coarse_output(0, 0)   # off is always accepted
        sim.write_coarse(str(tmp_path), 3, 60, 17)
        cells, outside, valid = sim.coarse_fields(60, 17)
        assert (tmp_path / "coarse000003.dat").read_text() == cz.file_text(60, 17, cells, outside, valid)
    with pkg.LbmDem(256, 200, r, x, y) as sim:   # (distributed grains are enabled at a fluid-step boundary)
        sim.set_coarse_output(16, 16)
        with pytest.raises(pkg.LbmDemError, match="lbmdem_set_coarse_output"):
            sim.dist_enable()
        sim.set_coarse_output(0, 0)
        sim.dist_enable()
        for call in (lambda: sim.coarse_fields(16, 16), lambda: sim.set_coarse_output(16, 16)):
            with pytest.raises(pkg.LbmDemError, match="distributed"):
                call()
    with pkg.LbmDem(256, 200, r, x, y, strip=(128, 256), halo=12) as strip:
        for call in (lambda: strip.coarse_fields(16, 16), lambda: strip.write_coarse(str(tmp_path), 0, 16, 16),
                     lambda: strip.set_coarse_output(16, 16)):
            with pytest.raises(pkg.LbmDemError, match="strip"):
                call()
    if os.path.exists(pkg.SP_LIB_PATH):
        with pkg.LbmDem(256, 200, r, x, y, precision="f32") as sp:
            for call in (lambda: sp.coarse_fields(16, 16), lambda: sp.write_coarse(str(tmp_path), 0, 16, 16),
                         lambda: sp.set_coarse_output(16, 16)):
                with pytest.raises(pkg.LbmDemError, match="single-precision"):
                    call()


def test_g6_at_4000_through_run_scene(pkg, tmp_path):
    r, x, y = g6()
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.set_coarse_output(16, 16)
        sim.run_scene(4000, str(tmp_path))
        cells, outside, valid = check(sim, r, 16, 16)
        assert valid == 1 and cells["sum_z"].sum() > 0
    text = (tmp_path / "coarse000000.dat").read_text()
    assert text.splitlines()[0].endswith("contacts 1")
    assert text == cz.file_text(16, 16, cells, outside, valid)
    for name in ("DEM000000.dat", "stats.data"):   # everything else the event writes is still the reference's
        assert (tmp_path / name).read_bytes() == open(os.path.join(REF_DIR, name), "rb").read(), name
    assert sorted(os.listdir(tmp_path)) == sorted(["DEM000000.dat", "DEM000000.ps", "stats.data", "coarse000000.dat"])
