"""GPU: the contact network export (lbmdem_contact_stats, lbmdem_download_contacts, lbmdem_write_contacts,
lbmdem_set_contacts_output; include/lbmdem_hip.h) against the unmodified reference's per-grain sums (tests/golden/contacts_*.npz,
tests/golden/dem_G6_4000steps) and against the numpy restatement of the laws (tests/contacts_util.py), bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import contacts_util as cu
import samples

pytestmark = pytest.mark.gpu
REF_DIR = os.path.join(cu.HERE, "golden", "dem_G6_4000steps")


def table_substep(sim, k9=None, nbsteps=None):
    """one table sub-step from the given kinematics -> (the state it started from, was it a film step)"""
    if nbsteps is not None:
        sim.nbsteps = nbsteps
    if k9 is not None:
        sim.kinematics = k9
    sim.initVerlet()
    sim.set_diagnostics(True)
    pre, film = sim.kinematics, sim.nbsteps % sim.config().phys.stepFilm == 0
    sim.dem_substep()
    return pre, film


def restated(sim, pre, film, **over):
    """the restatement's records and counters for the sub-step that started from `pre`, with the handle's list"""
    cumul, neigh, wf = sim.verlet()
    P = cu.params_of_config(sim.config(), **over)
    return cu.restate(pre, sim.grain_table()[:, 9], cu.pairs_of_list(cumul, neigh), wf, P, film) + (P,)


@pytest.mark.parametrize("name", cu.CASES)
def test_golden_records_add_up_to_the_references_table(pkg, name):
    g = cu.load_case(name)
    lx, ly = (int(v) for v in name.rsplit("_", 1)[1].split("x"))
    n = len(g["r_mm"])
    with pkg.LbmDem(lx, ly, g["r_mm"] * 1e-3, g["x_mm"] * 1e-3, g["y_mm"] * 1e-3) as sim:
        pre, film = table_substep(sim, g["pre"], int(g["nbsteps"]))
        assert film == cu.case_film(g) and np.array_equal(pre, g["pre"])
        rec, stats = sim.download_contacts(), sim.contact_stats()
        P = cu.case_params(g)   # (the reference's scalars, not the handle's)
        bad = cu.table_mismatches(cu.replay(rec, g["table"][:, 0], g["table"][:, 1], n, film, P["dt"], P["mu"]), g["table"])
        assert not bad, (name, bad)
        want, counts = cu.restate(g["pre"], g["r"], cu.pairs_of_list(g["cumul"], g["neigh"]), g["wallflags"], P, film)
        assert cu.same_records(rec, want), name
        assert stats == counts, (name, stats, counts)
        assert np.array_equal(sim.download_contacts(), rec)   # asking again changes nothing


def test_g6_at_4000_through_run_scene(pkg, tmp_path):
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    n = len(z["r_mm"])
    with pkg.LbmDem(256, 200, z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3) as sim:
        sim.set_contacts_output(True)
        sim.run_scene(4000, str(tmp_path))
        rec = sim.download_contacts()
        cfg = sim.config()
    lines = (tmp_path / "contacts000000.dat").read_text().splitlines()
    t = z["grains"]
    # (z counts every record once: a pair at its lower grain, a wall contact at its grain)
    assert lines[0] == "# i j dn nx ny fn ft" and len(lines) == 1 + len(rec) and len(rec) == int(t[:, 28].sum()) > 0
    for l, c in zip(lines[1:], rec):
        assert l == "%d %d %e %e %e %e %e" % (c["i"], c["j"], c["dn"], c["nx"], c["ny"], c["fn"], c["ft"])
    bad = cu.table_mismatches(cu.replay(rec, t[:, 0], t[:, 1], n, False, cfg.dt, cfg.phys.mu), t)
    assert not bad, bad
    ps = (tmp_path / "DEM000000_chains.ps").read_bytes()
    assert ps.count(b"stroke") == int(((rec["j"] >= 0) & (rec["fn"] > 0)).sum())
    # everything else the event writes is still the reference's
    for name in ("DEM000000.dat", "stats.data"):
        assert (tmp_path / name).read_bytes() == open(os.path.join(REF_DIR, name), "rb").read(), name
    got = (tmp_path / "DEM000000.ps").read_bytes().split(b"\n")
    assert [got[0]] + got[4:] == open(os.path.join(REF_DIR, "DEM000000.ps"), "rb").read().split(b"\n")
    assert sorted(os.listdir(tmp_path)) == sorted(["DEM000000.dat", "DEM000000.ps", "stats.data", "contacts000000.dat",
                                                   "DEM000000_chains.ps"])


def shape_packing(n, dense=False):
    """a row packing of exactly n grains, some pairs in contact, every third grain of the bottom row 2 um into the floor, with
    random velocities. dense: small grains, a dozen list entries each -- a workgroup's slice of the list takes several rounds"""
    lx, ly = (512, 640) if n > 160 and not dense else (256, 200)
    kw = dict(rmin=0.2, rmax=0.2) if dense else {}
    r, x, y = samples.to_metres(*samples.row_packing(lx, ly, n, seed=29, **kw))
    assert len(r) == n
    row0 = np.nonzero(y < y.min() + 2e-5)[0][::3]
    y[row0] = r[row0] - 2e-6
    k = np.zeros((n, 9))
    k[:, 0], k[:, 1] = x, y
    rng = np.random.default_rng(n)
    k[:, 3:6] = rng.normal(0, 1, (n, 3)) * [0.05, 0.05, 30.0]
    k[:, 6:9] = rng.normal(0, 1, (n, 3)) * [5.0, 5.0, 3000.0]
    return lx, ly, r, x, y, k


@pytest.mark.parametrize("n,dense,nbsteps", [(1, False, 1), (2, False, 1), (63, False, 1), (64, False, 1), (65, False, 1),
                                             (65, False, 0), (257, False, 1), (1025, False, 1), (1025, True, 1)])
def test_shapes_record_by_record(pkg, n, dense, nbsteps):
    lx, ly, r, x, y, k = shape_packing(n, dense)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        pre, film = table_substep(sim, k, nbsteps)
        assert film == (nbsteps == 0)
        rec, stats = sim.download_contacts(), sim.contact_stats()
        want, counts, _ = restated(sim, pre, film)
        assert cu.same_records(rec, want), (n, len(rec), len(want))
        assert stats == counts, (stats, counts)
        assert counts["wall_contacts"] >= 1
        if n == 1:
            assert counts["candidate_pairs"] == 0 and (rec["j"] < 0).all()
        if n >= 63:
            assert counts["touching_pairs"] >= n // 8
        if dense:   # more than one round of 256 entries per workgroup of 64 grains, records in every round
            cumul, neigh, _ = sim.verlet()
            assert 2 * len(neigh) >= 2 * 256 * ((n + 63) // 64) and counts["touching_pairs"] > 256
        # sizing, and a buffer that is too small
        L, cnt = pkg.load_library(), ctypes.c_long(-1)
        assert L.lbmdem_download_contacts(sim._h, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == len(rec)
        small = np.full(len(rec) - 1, 7, cu.CONTACT_DTYPE) if len(rec) > 1 else None
        if small is not None:
            cnt.value = -1
            assert L.lbmdem_download_contacts(sim._h, small.ctypes.data_as(ctypes.c_void_p), len(small), ctypes.byref(cnt)) == -1
            assert cnt.value == len(rec) and (small["i"] == 7).all()
        assert np.array_equal(sim.download_contacts(), rec)   # the handle stays usable


def test_no_contact_at_all_leaves_the_buffer_alone(pkg):
    r, x, y = samples.to_metres(*samples.row_packing(256, 200, 40, seed=5, touch_prob=0.0))
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        pre, film = table_substep(sim, None, 1)
        out = np.full(8, 7, cu.CONTACT_DTYPE)
        cnt = ctypes.c_long(-1)
        assert pkg.load_library().lbmdem_download_contacts(sim._h, out.ctypes.data_as(ctypes.c_void_p), len(out), ctypes.byref(cnt)) == 0
        assert cnt.value == 0 and (out["i"] == 7).all() and (out["fn"] == 7).all()
        stats = sim.contact_stats()
        assert stats["candidate_pairs"] > 0 and not any(stats[c] for c in cu.COUNTERS[1:])
        assert stats == restated(sim, pre, film)[1]


def test_every_candidate_touches(pkg):
    n = 30   # one row of equal grains, each 0 .. 4 um into the next; the next but one is 0.6 mm away, beyond distVerlet
    r, x, y = samples.to_metres(*samples.row_packing(256, 200, n, seed=11, rmin=0.3, rmax=0.3, touch_prob=1.0))
    assert len(r) == n and np.ptp(y) < 2e-5
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        pre, film = table_substep(sim, None, 1)
        rec, stats = sim.download_contacts(), sim.contact_stats()
        want, counts, _ = restated(sim, pre, film)
        assert stats == counts and stats["candidate_pairs"] == stats["touching_pairs"] == n - 1 == len(rec)
        assert cu.same_records(rec, want)
        assert np.array_equal(rec["i"], np.arange(n - 1)) and np.array_equal(rec["j"], np.arange(1, n))


def test_export_does_not_interfere(pkg, tmp_path):
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    r, x, y = z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3
    with pkg.LbmDem(256, 200, r, x, y) as a, pkg.LbmDem(256, 200, r, x, y) as b:
        for sim in (a, b):
            sim.set_diagnostics(True)
        for piece in (1, 7, 30, 13):
            a.renderScene(piece); b.renderScene(piece)
            a.contact_stats(); a.download_contacts(); a.write_contacts(str(tmp_path), piece)
        a.set_diagnostics(False); b.set_diagnostics(False)
        a.renderScene(40); b.renderScene(40)
        a.set_diagnostics(True); b.set_diagnostics(True)
        a.renderScene(1); b.renderScene(1)
        a.download_contacts()
        assert a.nbsteps == b.nbsteps == 92
        for what in ("f", "obst", "kinematics", "fhf"):
            assert np.array_equal(getattr(a, what), getattr(b, what)), what
        assert np.array_equal(a.grain_table(), b.grain_table())


def test_validity(pkg):
    lx, ly, r, x, y, k = shape_packing(65)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        def refused():
            for call in (sim.contact_stats, sim.download_contacts, lambda: sim.write_contacts("/nowhere", 0)):
                with pytest.raises(pkg.LbmDemError, match="lbmdem_set_diagnostics") as e:
                    call()
                assert e.value.code == -1
        refused()                                # after create
        sim.nbsteps = 1
        sim.kinematics = k
        sim.initVerlet()
        sim.dem_substep()
        refused()                                # after an ordinary sub-step
        sim.set_diagnostics(True)
        sim.dem_substep()
        n0 = len(sim.download_contacts())
        assert n0 > 0
        sim.initVerlet()
        refused()                                # after verlet_rebuild
        sim.dem_substep()
        assert len(sim.download_contacts()) > 0
        sim.kinematics = sim.kinematics
        refused()                                # after upload_kinematics
        sim.set_diagnostics(False)
        sim.renderScene(3)
        refused()                                # after a run of ordinary sub-steps
        sim.set_diagnostics(True)
        pre = sim.kinematics
        sim.dem_substep()                        # valid again after the next table sub-step
        want, counts, _ = restated(sim, pre, False)
        assert cu.same_records(sim.download_contacts(), want) and sim.contact_stats() == counts
        with pytest.raises(pkg.LbmDemError, match="cannot open"):
            sim.write_contacts("/nowhere/at/all", 0)
        assert cu.same_records(sim.download_contacts(), want)


def test_vibrating_top_wall_follows_the_schedule(pkg):
    """the top wall's ft reads wallT_vel = amp freq cos(freq t) of the sub-step's clock (main.c:855)"""
    lx, ly = 64, 48
    r = np.array([0.6e-3, 0.7e-3, 0.5e-3])
    x = np.array([1.5e-3, 3.4e-3, 5.0e-3])
    y = np.array([ly * 1e-3 - r[0] + 3e-6, ly * 1e-3 - r[1] + 2e-6, 2.0e-3])   # two grains pressed into the top wall at 1e-3 ly
    phys = pkg.Physics()
    pkg.load_library().lbmdem_physics_defaults(ctypes.byref(phys))
    phys.freq, phys.amp = 900.0, 2.0e-6
    with pkg.LbmDem(lx, ly, r, x, y, physics=phys) as sim:
        sim.set_vibration(True)
        sim.set_diagnostics(True)
        sim.nbsteps = 1
        k = sim.kinematics
        k[:, 3] = [0.02, -0.03, 0.0]
        sim.kinematics = k
        sim.initVerlet()
        sim.renderScene_dry(5)
        cfg0 = sim.config()
        sched = np.zeros((1, 4))
        pkg.load_library().lbmdem_vibration_schedule(ctypes.byref(cfg0), sim.nbsteps, 1, sched.ctypes.data_as(ctypes.c_void_p))
        pre = sim.kinematics
        sim.renderScene_dry(1)
        rec = sim.download_contacts()
        cfg = sim.config()   # (the walls and the clock the sub-step saw)
        vel = float(sched[0, 3])   # lbmdem_vibration_schedule: t, Mgx, Mdx, wallT_vel of that sub-step
        want, counts, _ = restated(sim, pre, False, wallT_vel=vel)
        top = rec[rec["j"] == cu.WALL_T]
        assert len(top) == 2 and counts["wall_contacts"] >= 2
        assert cu.same_records(rec, want)
        assert sched[0, 0] == cfg.phys.t and sched[0, 1] == cfg.Mgx and sched[0, 2] == cfg.Mdx
        assert abs(vel) > 1e-4 and vel != phys.amp * phys.freq     # the clock has moved: not the value at t = 0
        still, _, _ = restated(sim, pre, False, wallT_vel=phys.amp * phys.freq)
        assert not cu.same_records(rec, still)                     # ... and the records can tell


def test_refusals(pkg):
    lx, ly, r, x, y, k = shape_packing(65)
    if os.path.exists(pkg.SP_LIB_PATH):
        with pkg.LbmDem(lx, ly, r, x, y, precision="f32") as sp:
            for call in (sp.contact_stats, sp.download_contacts, lambda: sp.write_contacts(".", 0), lambda: sp.set_contacts_output(True)):
                with pytest.raises(pkg.LbmDemError, match="single-precision"):
                    call()
    with pkg.LbmDem(lx, ly, r, x, y, strip=(lx // 2, lx), halo=12) as strip:
        for call in (strip.contact_stats, strip.download_contacts, lambda: strip.set_contacts_output(True)):
            with pytest.raises(pkg.LbmDemError, match="strip"):
                call()
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.set_contacts_output(True)
        with pytest.raises(pkg.LbmDemError, match="lbmdem_set_contacts_output"):
            sim.dist_enable()
        sim.set_contacts_output(False)
        sim.dist_enable()
        with pytest.raises(pkg.LbmDemError, match="distributed"):
            sim.set_contacts_output(True)
        with pytest.raises(pkg.LbmDemError, match="distributed"):
            sim.contact_stats()
