"""GPU: the flow fields (lbmdem_flow_fields, lbmdem_flow_fields_device, lbmdem_flow_sums, lbmdem_write_flow,
lbmdem_set_flow_output; include/lbmdem_hip.h) against their numpy restatement (tests/flow_util.py) over the handle's downloads:
every plane and every sum exactly equal, no tolerance."""
import ctypes
import os

import numpy as np
import pytest

import flow_util as fu
import golden_util as gu
import samples

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(HERE, "golden", "dem_G6_4000steps")
ODD = "S_127x121"      # lx % 8 = 7, ly % 16 = 9, a last sum block of 57 columns
NARROW = "S_13x61"     # the narrowest lattice of tests/golden/S_*: the window is wider than the lattice, one short block


def g6():
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    return z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3


def check(sim):
    """all planes and all sums equal the restatement; -> (fields, sums) of the restatement"""
    F, S = fu.expected(sim)
    got = sim.flow_fields()
    assert list(got) == list(fu.NAMES) and all(p.shape == (sim.lx, sim.ly) for p in got.values())
    bad = fu.mismatches(got, F)
    sums = sim.flow_sums()
    bad_sums = [k for k in fu.SUMS if not sums[k] == S[k]]
    print(f"{sim.lx}x{sim.ly}: planes that differ {bad}, sums that differ {bad_sums}; {sums}")
    assert bad == [] and bad_sums == []
    assert sums["n_fluid"] == (sim.obst == -1).sum()
    return F, S


@pytest.fixture(scope="module")
def coupled(pkg):
    """the G6 packing on 256 x 200 after five fluid periods and three more sub-steps"""
    r, x, y = g6()
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.renderScene(5 * sim.cfg.npDEM + 3)
        yield sim, fu.expected(sim)


def test_coupled_state(coupled):
    sim, _ = coupled
    F, S = check(sim)
    for name in ("vort", "gdot", "diss", "div", "nxx", "nxy"):
        assert F[name].any(), name
    assert S["sum_ke"] > 0 and S["sum_diss"] > 0 and S["sum_enstrophy"] > 0 and S["max_gdot"] > 0
    grain = (sim.obst >= 0) & (sim.obst < sim.n)
    assert grain.any() and (F["ux"][grain] != 0).any()   # the grains' own velocity is in the composite


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 16, 32, 64, 128, 2 | 4 | 32 | 128])
def test_masks_give_their_planes_in_bit_order(coupled, mask):
    sim, (F, _) = coupled
    got = sim.flow_fields(mask)
    assert list(got) == fu.plane_names(mask)
    assert fu.mismatches(got, F) == []


@pytest.mark.parametrize("name", [ODD, NARROW])
def test_odd_lattices(pkg, name):
    c = gu.CASES[name]
    a = gu.GpuAdapter(pkg, name)
    try:
        a.set_kinematics(gu.mg.shape_initial_kinematics(c))
        a.sim.renderScene(2 * a.sim.cfg.npDEM + 1)
        F, S = check(a.sim)
        assert F["vort"].any() and S["sum_rho"] > 0
        assert fu.mismatches(a.sim.flow_fields(4 | 8), F) == []
    finally:
        a.sim.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_grain_counts(pkg, n):
    r, x, y = samples.to_metres(*samples.row_packing(256, 200, n, rmin=0.2, rmax=0.2))
    assert len(r) == n
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.renderScene(2)
        check(sim)


def test_spinning_grain(pkg):
    """One grain given a spin: at nodes whose four neighbours belong to the grain the stencil sees a rigid rotation,
    u = (v1 - (Y - x2) v3, v2 + (X - x1) v3) / c with X = x dx + Mgx, so vort = 2 v3 dx / c = 2 v3 dtLB and div = 0.
    Bound, with u = eps / 2 the unit roundoff: uy = fl(fl(v2 + fl(fl(fl(fl(x dx) + Mgx) - x1) v3)) / c) is six roundings. Those of
    x dx and of the sum with Mgx are relative to the node's distance from the WALL, up to Xmax = lx dx + |Mgx|, not to its distance
    from the centre (the subtraction cancels), so the largest |u| of the stencil's own nodes does not bound them; the largest |u|
    the rotation gives anywhere on the lattice does: W = (|v1| + |v2| + (Xmax + Ymax) |v3|) / c bounds |uy|, |g| / c, |e| / c and
    Xmax |v3| / c, so |error(uy)| <= u (4 W + 2 W) = 3 eps W, likewise ux. A difference of two velocities is off by at most
    6 eps W plus its own rounding, < 7 eps W; the halving is exact, each half is off by 3.5 eps W, their sum by 7 eps W plus one
    rounding, < 8 eps W. The comparison value 2 v3 dtLB carries the roundings of dtLB = dx / c and of the product:
    |vort - 2 v3 dtLB| <= 8 eps W + 4 eps |2 v3 dtLB|, |div| <= 8 eps W."""
    r, x, y = np.array([1.5e-3]), np.array([12.8e-3]), np.array([10.0e-3])
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.renderScene(2)
        k = sim.kinematics
        k[0, 3:6] = (0.013, -0.007, 37.0)   # v1, v2, v3
        sim.kinematics = k
        F, _ = check(sim)
        cfg = sim.config()
        g = sim.obst == 0
        inner = np.zeros_like(g)
        inner[1:-1, 1:-1] = g[1:-1, 1:-1] & g[2:, 1:-1] & g[:-2, 1:-1] & g[1:-1, 2:] & g[1:-1, :-2]
        assert inner.sum() > 100
        got = sim.flow_fields()
        want = 2 * 37.0 * cfg.dtLB
        w = sim.walls()
        W = (0.013 + 0.007 + (256 * cfg.dx + abs(w["Mgx"]) + 200 * cfg.dx + abs(w["Mby"])) * 37.0) / cfg.c
        eps = np.finfo(np.float64).eps
        bound = 8 * eps * W + 4 * eps * abs(want)
        print(f"spin: vort {want:.6e}, largest deviation {np.abs(got['vort'][inner] - want).max():.3e}, "
              f"largest |div| {np.abs(got['div'][inner]).max():.3e}, bound {bound:.3e}, W {W:.3e}")
        assert want != 0 and np.abs(got["vort"][inner] - want).max() <= bound
        assert np.abs(got["div"][inner]).max() <= 8 * eps * W
        for name in ("nxx", "nxy", "gdot", "diss"):
            assert not got[name][g].any()


def test_vibrating_handle(pkg):
    r, x, y = g6()
    phys = pkg.Physics()
    pkg.load_library().lbmdem_physics_defaults(ctypes.byref(phys))
    phys.freq, phys.amp = 900.0, 2.0e-6
    with pkg.LbmDem(256, 200, r, x, y, physics=phys) as sim:
        Mgx0 = sim.walls()["Mgx"]
        sim.set_vibration(True)
        sim.renderScene(300)
        k = sim.kinematics
        k[:, 5] += 3.0   # every grain spins: the moved wall enters wall_uy through (x dx + Mgx - x1) v3
        sim.kinematics = k
        w = sim.walls()
        assert w["Mgx"] != Mgx0
        F, _ = check(sim)
        cfg = sim.config()
        stale = fu.fields(sim.f, sim.obst, sim.kinematics, Mgx0, w["Mby"], cfg.dx, cfg.c, cfg.phys.s8, cfg.phys.s9, cfg.nbgrains)
        assert not np.array_equal(stale["uy"], F["uy"])   # (the restatement with the wall where it started is another field)


def test_device_tensors(pkg):
    import torch
    r, x, y = g6()
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.renderScene(2 * sim.cfg.npDEM)
        host = sim.flow_fields()
        dev = sim.flow_fields(device=True)
        sim.sync()
        assert list(dev) == list(fu.NAMES)
        for name, t in dev.items():
            assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (256, 200)
            assert np.array_equal(t.cpu().numpy(), host[name]), name
        one = sim.flow_fields(pkg.FLOW_VORT | pkg.FLOW_GDOT, device=True)
        sim.sync()
        assert list(one) == ["vort", "gdot"] and np.array_equal(one["gdot"].cpu().numpy(), host["gdot"])
        small = torch.full((2 * 256 * 200 - 1,), 7.0, dtype=torch.float64, device="cuda")
        with pytest.raises(pkg.LbmDemError, match="buffer holds") as e:
            sim.flow_fields_into(pkg.FLOW_VORT | pkg.FLOW_GDOT, small)
        assert e.value.code == -1
        sim.sync()
        assert bool((small == 7.0).all())
        with pytest.raises(pkg.LbmDemError):
            sim.flow_fields_into(pkg.FLOW_VORT, small.float())


def test_export_does_not_interfere(pkg, tmp_path):
    r, x, y = g6()
    with pkg.LbmDem(256, 200, r, x, y) as a, pkg.LbmDem(256, 200, r, x, y) as b:
        period = a.cfg.npDEM
        for k in range(3):
            a.renderScene(period); b.renderScene(period)
            first = a.flow_fields()
            a.flow_sums()
            a.write_flow(str(tmp_path), k)
            a.flow_fields(pkg.FLOW_DIV)
            assert fu.mismatches(a.flow_fields(), first) == []
        for what in ("f", "obst", "fhf", "kinematics"):
            assert np.array_equal(getattr(a, what), getattr(b, what)), what
        assert a.nbsteps == b.nbsteps == 3 * period


def test_sizing_and_refusals(pkg, tmp_path):
    L = pkg.load_library()
    r, x, y = samples.to_metres(*samples.row_packing(256, 200, 65, seed=29))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    plane = 256 * 200
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.renderScene(2)
        cnt = ctypes.c_long(-1)
        assert L.lbmdem_flow_fields(sim._h, 255, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == 8 * plane
        assert L.lbmdem_flow_fields(sim._h, 4 | 64, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == 2 * plane
        small = np.full(2 * plane - 1, 7.0)
        cnt.value = -1
        assert L.lbmdem_flow_fields(sim._h, 4 | 64, vp(small), len(small), ctypes.byref(cnt)) == -1
        assert cnt.value == 2 * plane and (small == 7.0).all()
        roomy = np.full(2 * plane + 3, 7.0)
        assert L.lbmdem_flow_fields(sim._h, 4 | 64, vp(roomy), len(roomy), ctypes.byref(cnt)) == 0
        assert cnt.value == 2 * plane and (roomy[2 * plane:] == 7.0).all()
        want = sim.flow_fields(4 | 64)
        assert np.array_equal(roomy[:plane].reshape(256, 200), want["vort"])
        assert np.array_equal(roomy[plane:2 * plane].reshape(256, 200), want["gdot"])
        for mask in (0, 256, -4):
            assert L.lbmdem_flow_fields(sim._h, mask, vp(roomy), len(roomy), ctypes.byref(cnt)) == -1
        assert L.lbmdem_flow_fields(sim._h, 255, vp(roomy), len(roomy), None) == -1
        assert L.lbmdem_flow_fields(sim._h, 255, None, 5, ctypes.byref(cnt)) == -1
        assert L.lbmdem_flow_sums(sim._h, None) == -1
        with pytest.raises(pkg.LbmDemError, match="cannot open"):
            sim.write_flow(str(tmp_path / "not" / "there"), 0)
        sim.set_flow_output(False)   # off is always accepted
    with pkg.LbmDem(256, 200, r, x, y) as sim:   # (distributed grains are enabled at a fluid-step boundary)
        sim.set_flow_output(True)
        with pytest.raises(pkg.LbmDemError, match="lbmdem_set_flow_output"):
            sim.dist_enable()
        sim.set_flow_output(False)
        sim.dist_enable()
        for call in (sim.flow_fields, sim.flow_sums, sim.set_flow_output):
            with pytest.raises(pkg.LbmDemError, match="distributed"):
                call()
    with pkg.LbmDem(256, 200, r, x, y, strip=(128, 256), halo=12) as strip:
        for call in (strip.flow_fields, strip.flow_sums, lambda: strip.write_flow(str(tmp_path), 0), strip.set_flow_output,
                     lambda: strip.flow_fields(device=True)):
            with pytest.raises(pkg.LbmDemError, match="strip"):
                call()
    if os.path.exists(pkg.SP_LIB_PATH):
        with pkg.LbmDem(256, 200, r, x, y, precision="f32") as sp:
            for call in (sp.flow_fields, sp.flow_sums, lambda: sp.write_flow(str(tmp_path), 0), sp.set_flow_output):
                with pytest.raises(pkg.LbmDemError, match="single-precision"):
                    call()
    assert os.listdir(tmp_path) == []


def test_written_file_is_the_host_writer_over_the_planes(pkg, tmp_path):
    c = gu.CASES[ODD]
    a = gu.GpuAdapter(pkg, ODD)
    try:
        a.set_kinematics(gu.mg.shape_initial_kinematics(c))
        a.sim.renderScene(2 * a.sim.cfg.npDEM + 1)
        sims = [a.sim]
        r, x, y = g6()
        with pkg.LbmDem(256, 200, r, x, y) as big:
            big.renderScene(3 * big.cfg.npDEM)
            for k, sim in enumerate(sims + [big]):
                dev, host = tmp_path / f"dev{k}", tmp_path / f"host{k}"
                dev.mkdir(); host.mkdir()
                sim.write_flow(str(dev), 12)
                p = sim.flow_fields()
                pkg.write_flow_files(str(host), 12, p["ux"], p["uy"], p["vort"], p["gdot"], p["diss"])
                got = (dev / "flow000012.vtk").read_bytes()
                assert got == (host / "flow000012.vtk").read_bytes() == fu.file_bytes(p["ux"], p["uy"], p["vort"], p["gdot"], p["diss"])
                assert os.listdir(dev) == ["flow000012.vtk"]
    finally:
        a.sim.close()


def test_g6_at_4000_through_run_scene(pkg, tmp_path):
    r, x, y = g6()
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.set_flow_output(True)
        sim.run_scene(4000, str(tmp_path))
        _, S = check(sim)
        t = sim.nbsteps * sim.cfg.dt
        assert sim.nbsteps == 4000
    for name in ("DEM000000.dat", "stats.data"):   # everything else the event writes is still the reference's
        assert (tmp_path / name).read_bytes() == open(os.path.join(REF_DIR, name), "rb").read(), name
    assert sorted(os.listdir(tmp_path)) == sorted(["DEM000000.dat", "DEM000000.ps", "stats.data", "flow.data"])
    lines = (tmp_path / "flow.data").read_text().splitlines(keepends=True)
    assert lines == [fu.DATA_HEADER, fu.data_line(t, S)]


def test_run_scene_writes_the_frames_a_twin_writes_by_hand(pkg, tmp_path):
    r, x, y = g6()
    phys = pkg.derive(256, 200, r).phys
    phys.stepFilm = 60
    da, db = tmp_path / "scene", tmp_path / "hand"
    da.mkdir(); db.mkdir()
    with pkg.LbmDem(256, 200, r, x, y, physics=phys) as a, pkg.LbmDem(256, 200, r, x, y, physics=phys) as b:
        a.set_flow_output(True)
        _, res = a.run_scene(180, str(da))
        assert res["nfile"] == 3
        for k in range(3):
            b.renderScene(60)
            b.write_flow(str(db), k)
        names = ["flow%06d.vtk" % k for k in range(3)]
        assert sorted(n for n in os.listdir(da) if n.startswith("flow")) == names   # (no DEM event: no flow.data)
        for n in names:
            assert (da / n).read_bytes() == (db / n).read_bytes(), n
        assert (da / names[0]).read_bytes() != (da / names[2]).read_bytes()
        for what in ("f", "obst", "kinematics"):
            assert np.array_equal(getattr(a, what), getattr(b, what)), what
    # off (the default): the same run leaves the frames alone and nothing else
    dc = tmp_path / "off"
    dc.mkdir()
    with pkg.LbmDem(256, 200, r, x, y, physics=phys) as c:
        c.run_scene(180, str(dc))
    assert sorted(os.listdir(dc)) == sorted(n for n in os.listdir(da) if not n.startswith("flow"))
    for n in os.listdir(dc):
        assert (dc / n).read_bytes() == (da / n).read_bytes(), n
