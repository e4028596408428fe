"""GPU: the cluster analysis of the contact net (lbmdem_cluster_compute, lbmdem_download_cluster_grains,
lbmdem_cluster_grains_device, lbmdem_download_clusters, lbmdem_write_clusters, lbmdem_set_clusters_output; include/lbmdem_hip.h)
against the restatement over download_contacts() and the table's centres (tests/cluster_util.py): every integer and every box
by array_equal, the threshold on the bits."""
import ctypes
import os

import numpy as np
import pytest

import cluster_util as cl
import contacts_util as cu
import samples

pytestmark = pytest.mark.gpu
REF_DIR = os.path.join(cu.HERE, "golden", "dem_G6_4000steps")
WHOLE = " needs the whole lattice and all grains on this handle (not a strip of a decomposition, no distributed grains)"


def table_substep(sim, k9=None, nbsteps=None):
    """test_gpu_contacts.py's recipe: one table sub-step from the given kinematics"""
    if nbsteps is not None:
        sim.nbsteps = nbsteps
    if k9 is not None:
        sim.kinematics = k9
    sim.initVerlet()
    sim.set_diagnostics(True)
    sim.dem_substep()


def shape_packing(n, dense=False):
    """test_gpu_contacts.py's packing: n grains in rows, some pairs in contact, every third grain of the bottom row 2 um into
    the floor, random velocities"""
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


def check(sim, fmin, relative, zmin, rec=None):
    """one compute against the restatement, every output -> (restatement, counts, rounds)"""
    rec = sim.download_contacts() if rec is None else rec
    t = sim.grain_table()
    R = cl.restate(rec, sim.n, t[:, 0], t[:, 1], fmin, relative, zmin)
    counts, thr = sim.clusters(fmin, relative, zmin)
    what = (fmin, relative, zmin)
    assert cl.same_bits(thr, R["thr"]), (what, thr, R["thr"])
    assert counts == R["counts"], (what, counts, R["counts"])
    g = sim.cluster_grains()
    for name in ("label", "degree", "core", "walls"):
        assert g[name].dtype == np.int32 and np.array_equal(g[name], R[name]), (what, name)
    tab = sim.cluster_table()
    assert cl.same_table(tab, R["table"]), (what, tab, R["table"])
    gt = sim.cluster_grains_tensors()
    for name in ("label", "degree", "core", "walls"):
        assert gt[name].is_cuda and np.array_equal(gt[name].cpu().numpy(), R[name]), (what, name)
    rounds = sim.cluster_rounds()
    assert rounds[1] == R["peel_rounds"] and 0 <= rounds[0] <= sim.n + 1
    assert np.array_equal(sim.download_contacts(), rec)   # the records are still the export's
    return R, counts, rounds


@pytest.mark.parametrize("n,dense", [(1, False), (2, False), (63, False), (64, False), (65, False), (257, False), (1025, False),
                                     (1025, True)])
def test_shapes_against_the_restatement(pkg, n, dense):
    lx, ly, r, x, y, k = shape_packing(n, dense)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        table_substep(sim, k, 1)
        rec = sim.download_contacts()
        assert (rec["j"] < 0).any()
        for fmin, relative, zmin in ((1.0, True, 2), (0.0, False, 0), (0.25, True, 3), (0.5, False, 1)):
            R, counts, _ = check(sim, fmin, relative, zmin, rec)
        R, counts, _ = check(sim, 0.0, False, 2, rec)
        assert counts["selected_pairs"] + counts["selected_walls"] == int((rec["fn"] >= 0).sum())
        if n >= 63:
            assert counts["clusters"] >= n // 16 and counts["largest_size"] >= 3
        if n == 1:
            assert counts["clusters"] == 0 and counts["largest_size"] == 1 and counts["largest_label"] == 0
        if n == 1025:   # several workgroups of records and of grains
            assert (rec["j"] >= 0).sum() > 256
        # sizing, and a buffer that is too small
        L, cnt = pkg.load_library(), ctypes.c_long(-1)
        tab = sim.cluster_table()
        assert L.lbmdem_download_clusters(sim._h, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == len(tab)
        if len(tab) > 1:
            small = np.full(len(tab) - 1, 7, cl.CLUSTER_DTYPE)
            cnt.value = -1
            assert L.lbmdem_download_clusters(sim._h, small.ctypes.data_as(ctypes.c_void_p), len(small), ctypes.byref(cnt)) == -1
            assert cnt.value == len(tab) and (small["label"] == 7).all()
            assert "there are %d entries, the buffer holds %d" % (len(tab), len(small)) in L.lbmdem_last_error().decode()
        assert cl.same_table(sim.cluster_table(), tab)   # the handle stays usable
        # any pointer may be NULL
        deg = np.full(n, -1, np.int32)
        assert L.lbmdem_download_cluster_grains(sim._h, None, deg.ctypes.data_as(ctypes.c_void_p), None, None) == 0
        assert np.array_equal(deg, R["degree"])


def touching_row(order=None, n=30, lx=256, ly=200):
    """test_gpu_contacts.py's row of equal grains that all touch, lifted off the floor; `order`: the grain index of each place"""
    r, x, y = samples.to_metres(*samples.row_packing(lx, ly, n, seed=11, rmin=0.3, rmax=0.3, touch_prob=1.0))
    assert len(r) == n and np.ptp(y) < 2e-5
    if order is not None:
        xs, ys = x.copy(), y.copy()
        x[order], y[order] = xs, ys
    return r, x, y


def test_row_is_one_component_and_peels_from_both_ends(pkg):
    n = 30
    r, x, y = touching_row()
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        table_substep(sim, None, 1)
        rec = sim.download_contacts()
        assert len(rec) == n - 1 and (rec["j"] >= 0).all() and (rec["fn"] > 0).all()
        R, counts, rounds = check(sim, 0.0, False, 2, rec)
        assert counts["clusters"] == 1 and counts["largest_size"] == n and counts["largest_label"] == 0
        assert (R["label"] == 0).all() and counts["spanning"] == 0
        assert rounds[1] == 15 and counts["core_grains"] == 0 and counts["core_pairs"] == 0   # both ends go, round after round
        tab = sim.cluster_table()
        assert len(tab) == 1 and tab[0]["contacts"] == n - 1 and tab[0]["core"] == 0
        for zmin in (0, 3):
            R, counts, rounds = check(sim, 0.0, False, zmin, rec)
            assert counts["core_grains"] == (n if zmin == 0 else 0)
        assert rounds[1] == 1   # no grain of a chain has three contacts
        # a threshold above every fn: singletons, an empty table, the largest size is 1
        R, counts, _ = check(sim, float(rec["fn"].max()) * 2, False, 2, rec)
        assert counts["clusters"] == 0 and counts["largest_size"] == 1 and counts["largest_label"] == 0
        assert counts["isolated_grains"] == n and len(sim.cluster_table()) == 0
        assert np.array_equal(sim.cluster_grains()["label"], np.arange(n))
        # the relative threshold: the mean keeps the stronger part of the chain
        R, counts, _ = check(sim, 1.0, True, 2, rec)
        assert 0 < counts["selected_pairs"] < n - 1


@pytest.mark.parametrize("kind,n,lx", [("descending", 30, 256), ("interleaved", 30, 256), ("descending", 600, 3712), ("interleaved", 600, 3712),
                                       ("shuffled", 2200, 13312)])
def test_labels_travel_against_the_index_order(pkg, kind, n, lx):
    """a long row that all touches, the grain indices permuted along it: the smallest index has to cross the whole chain,
    through records of many workgroups; 2199 pair records are three blocks of the threshold's sum"""
    order = {"descending": np.arange(n)[::-1], "interleaved": np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)[::-1]]),
             "shuffled": np.random.default_rng(3).permutation(n)}[kind]
    r, x, y = touching_row(order, n, lx, 64)
    with pkg.LbmDem(lx, 64, r, x, y) as sim:
        table_substep(sim, None, 1)
        rec = sim.download_contacts()
        assert (rec["j"] >= 0).all()
        R, counts, rounds = check(sim, 0.0, False, 2, rec)
        if n <= 600:
            assert len(rec) == n - 1
            assert counts["clusters"] == 1 and counts["largest_size"] == n and (R["label"] == 0).all()
            assert rounds[1] == n // 2
        else:   # (a metre from the origin a few of the smallest overlaps are lost to rounding: several long chains)
            assert len(rec) > 2 * 1024 and counts["largest_size"] > 256
        R, counts, _ = check(sim, 1.0, True, 1, rec)
        assert counts["clusters"] > 1


def test_no_contact_at_all_and_relative_without_a_positive_force(pkg):
    r, x, y = samples.to_metres(*samples.row_packing(256, 200, 40, seed=5, touch_prob=0.0))
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        table_substep(sim, None, 1)
        assert len(sim.download_contacts()) == 0
        for fmin, relative, zmin in ((1.0, True, 2), (0.0, True, 2), (0.0, False, 0), (3.0, False, 6)):
            R, counts, rounds = check(sim, fmin, relative, zmin)
            assert counts["clusters"] == 0 and counts["largest_size"] == 1 and counts["isolated_grains"] == 40
            assert counts["core_grains"] == (40 if zmin == 0 else 0) and rounds[0] == 0
        assert sim.clusters(1.0, True, 2)[1] == float("inf") and sim.clusters(0.0, True, 2)[1] == 0.0   # m == 0


def test_relative_with_records_but_m_zero(pkg):
    """grains on the floor and no pair: wall records only, so the mean of the pair forces has no term"""
    r, x, y = samples.to_metres(*samples.row_packing(256, 200, 12, seed=5, touch_prob=0.0))
    assert np.ptp(y) < 2e-5   # (one row)
    y[:] = r - 2e-6
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        table_substep(sim, None, 1)
        rec = sim.download_contacts()
        assert len(rec) == 12 and (rec["j"] == cu.WALL_B).all()
        R, counts, _ = check(sim, 1.0, True, 1, rec)
        assert R["thr"] == float("inf") and counts["selected_walls"] == 0
        R, counts, _ = check(sim, 0.0, True, 1, rec)
        assert R["thr"] == 0.0 and counts["selected_walls"] == 12 and counts["core_grains"] == 12 and counts["core_walls"] == 12
        assert (R["walls"] == 1).all() and counts["clusters"] == 0


def test_row_between_both_side_walls_spans(pkg):
    """the records of the top and the right wall carry the reference's fn <= 0 (include/lbmdem_hip.h, the contact network export):
    fn >= thr selects one only at thr == 0 and fn == 0 -- the end grain is leaving the wall fast enough for the law's clamp"""
    lx, ly, d = 256, 200, 2e-6
    with pkg.LbmDem(lx, ly, [5e-4], [3e-3], [3e-3]) as probe:   # where the side walls stand after the first list build
        probe.nbsteps = 1
        probe.initVerlet()
        Mgx, Mdx = probe.config().Mgx, probe.config().Mdx
    W = Mdx - Mgx
    n = int(W / 1.3e-3)
    rr = (W + (n + 1) * d) / (2 * n)         # n equal grains, each d into its neighbours and the end grains d into the walls
    r = np.full(n, rr)
    x = Mgx + rr - d + np.arange(n) * (2 * rr - d)
    y = np.full(n, 3e-3)
    for v_last, span in ((-0.1, 1), (0.0, 0)):
        k = np.zeros((n, 9))
        k[:, 0], k[:, 1] = x, y
        k[n - 1, 3] = v_last
        with pkg.LbmDem(lx, ly, r, x, y) as sim:
            table_substep(sim, k, 1)
            rec = sim.download_contacts()
            assert (rec["j"] == cu.WALL_L).sum() == 1 and (rec["j"] == cu.WALL_R).sum() == 1 and (rec["j"] >= 0).sum() == n - 1
            wr = rec[rec["j"] == cu.WALL_R]["fn"][0]
            assert (wr == 0) if span else (wr < 0)
            R, counts, _ = check(sim, 0.0, False, 2, rec)
            assert counts["spanning"] == span and counts["clusters"] == 1 and counts["largest_size"] == n
            assert R["walls"][0] == 4 and R["walls"][n - 1] == (8 if span else 0)
            assert check(sim, 1e-3, False, 2, rec)[1]["spanning"] == 0


def test_g6_at_4000_through_run_scene(pkg, tmp_path):
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    fmin, relative, zmin = 0.5, True, 2
    with pkg.LbmDem(256, 200, z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3) as sim:
        sim.set_clusters_output(True, fmin, relative, zmin)
        sim.run_scene(4000, str(tmp_path))
        rec, t = sim.download_contacts(), sim.grain_table()
        when = sim.nbsteps * sim.config().dt
        R, counts, _ = check(sim, fmin, relative, zmin, rec)
    assert counts["selected_pairs"] > 0 and counts["clusters"] > 0
    want = cl.files_text(t[:, 9], t[:, 0], t[:, 1], t[:, 18], rec, R, fmin, relative, zmin, when, 256, 200)
    assert (tmp_path / "clusters000000.dat").read_text() == want[0]
    assert (tmp_path / "cluster_table000000.dat").read_text() == want[1]
    assert (tmp_path / "DEM000000_clusters.ps").read_text() == want[2]
    assert (tmp_path / "clusters.data").read_text() == cl.DATA_HEADER + want[3]
    # everything else the event writes is still the reference's
    for name in ("DEM000000.dat", "stats.data"):
        assert (tmp_path / name).read_bytes() == open(os.path.join(REF_DIR, name), "rb").read(), name
    got = (tmp_path / "DEM000000.ps").read_bytes().split(b"\n")
    assert [got[0]] + got[4:] == open(os.path.join(REF_DIR, "DEM000000.ps"), "rb").read().split(b"\n")
    assert sorted(os.listdir(tmp_path)) == sorted(["DEM000000.dat", "DEM000000.ps", "stats.data", "clusters000000.dat",
                                                   "cluster_table000000.dat", "DEM000000_clusters.ps", "clusters.data"])


def test_analysis_does_not_interfere(pkg, tmp_path):
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    r, x, y = z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3
    with pkg.LbmDem(256, 200, r, x, y) as a, pkg.LbmDem(256, 200, r, x, y) as b:
        for sim in (a, b):
            sim.set_diagnostics(True)
        for piece in (1, 7, 30, 13):
            a.renderScene(piece); b.renderScene(piece)
            a.clusters(1.0, True, 2); a.cluster_grains(); a.cluster_table(); a.write_clusters(str(tmp_path), piece, 0.0, False, 3)
        a.set_diagnostics(False); b.set_diagnostics(False)
        a.renderScene(40); b.renderScene(40)
        a.set_diagnostics(True); b.set_diagnostics(True)
        a.renderScene(1); b.renderScene(1)
        a.clusters()
        assert a.nbsteps == b.nbsteps == 92
        for what in ("f", "obst", "kinematics", "fhf"):
            assert np.array_equal(getattr(a, what), getattr(b, what)), what
        assert np.array_equal(a.grain_table(), b.grain_table())
        assert np.array_equal(a.download_contacts(), b.download_contacts())


def test_validity(pkg, tmp_path):
    lx, ly, r, x, y, k = shape_packing(65)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        readers = (("lbmdem_download_cluster_grains", sim.cluster_grains), ("lbmdem_cluster_grains_device", sim.cluster_grains_tensors),
                   ("lbmdem_download_clusters", sim.cluster_table), ("lbmdem_cluster_rounds", sim.cluster_rounds))

        def readers_refused():
            for who, call in readers:
                with pytest.raises(pkg.LbmDemError) as e:
                    call()
                assert e.value.code == -1
                assert sim._L.lbmdem_last_error().decode() == "%s: no lbmdem_cluster_compute has been made for the last table sub-step" % who

        def refused():
            for call in (sim.clusters, lambda: sim.write_clusters(str(tmp_path), 0)):
                with pytest.raises(pkg.LbmDemError, match="lbmdem_cluster_compute: the last sub-step was no table sub-step") as e:
                    call()
                assert e.value.code == -1 and "lbmdem_set_diagnostics" in str(e.value)
            readers_refused()
        refused()                                # after create
        sim.nbsteps = 1
        sim.kinematics = k
        sim.initVerlet()
        sim.dem_substep()
        refused()                                # after an ordinary sub-step
        sim.set_diagnostics(True)
        sim.dem_substep()
        readers_refused()                        # a table sub-step, and no compute yet
        check(sim, 1.0, True, 2)
        sim.dem_substep()
        readers_refused()                        # another table sub-step: the results were the last one's
        check(sim, 1.0, True, 2)
        sim.initVerlet()
        refused()                                # after a list rebuild
        sim.dem_substep()
        check(sim, 0.0, False, 1)
        sim.kinematics = sim.kinematics
        refused()                                # after an upload of kinematics
        sim.dem_substep()
        for bad in (dict(fmin=-1.0), dict(fmin=float("inf")), dict(fmin=float("nan")), dict(zmin=-1), dict(zmin=7)):
            with pytest.raises(pkg.LbmDemError, match="fmin must be finite|zmin must lie in 0 .. 6"):
                sim.clusters(**bad)
        readers_refused()                        # a refused compute is none
        R, _, _ = check(sim, 1.0, True, 2)
        missing = str(tmp_path / "not" / "there")
        with pytest.raises(pkg.LbmDemError) as e:
            sim.write_clusters(missing, 0)
        assert sim._L.lbmdem_last_error().decode() == "cannot open '%s/clusters000000.dat' for writing" % missing
        assert np.array_equal(sim.cluster_grains()["label"], R["label"])
        assert os.listdir(tmp_path) == []


def test_refusals(pkg):
    lx, ly, r, x, y, k = shape_packing(65)
    if os.path.exists(pkg.SP_LIB_PATH):
        with pkg.LbmDem(lx, ly, r, x, y, precision="f32") as sp:
            for call in (sp.clusters, sp.cluster_grains, sp.cluster_grains_tensors, sp.cluster_table, sp.cluster_rounds,
                         lambda: sp.write_clusters(".", 0), lambda: sp.set_clusters_output(True)):
                with pytest.raises(pkg.LbmDemError) as e:
                    call()
                assert e.value.code == -1
                assert sp._L.lbmdem_last_error().decode() == "the cluster analysis is not available in the single-precision build of the library"
    def text(sim, call):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1, e.value
        return sim._L.lbmdem_last_error().decode()
    with pkg.LbmDem(lx, ly, r, x, y, strip=(lx // 2, lx), halo=12) as strip:
        for who, call in (("lbmdem_cluster_compute", strip.clusters), ("lbmdem_download_cluster_grains", strip.cluster_grains),
                          ("lbmdem_download_clusters", strip.cluster_table),
                          ("lbmdem_set_clusters_output", lambda: strip.set_clusters_output(True))):
            assert text(strip, call) == who + WHOLE
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.set_clusters_output(True)
        assert text(sim, sim.dist_enable) == ("the cluster analysis is not available with distributed grains "
                                              "(lbmdem_set_clusters_output(h, 0, 0., 0, 0) first)")
        sim.set_clusters_output(False)
        sim.dist_enable()
        for who, call in (("lbmdem_set_clusters_output", lambda: sim.set_clusters_output(True)), ("lbmdem_cluster_compute", sim.clusters),
                          ("lbmdem_cluster_compute", lambda: sim.write_clusters(".", 0))):
            assert text(sim, call) == who + WHOLE
