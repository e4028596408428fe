"""GPU: the strain analysis (lbmdem_strain_mark, lbmdem_strain_compute and their readers, lbmdem_write_strain,
lbmdem_set_strain_output; include/lbmdem_hip.h) against the restatement over kinematics and strain_reference()
(tests/strain_util.py): every integer by array_equal, every double on the bits."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import contacts_util as cu
import moving_walls_util as mw
import strain_util as su
from test_gpu_clusters import shape_packing, table_substep

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
REF_DIR = os.path.join(cu.HERE, "golden", "dem_G6_4000steps")
WHOLE = " needs the whole lattice and all grains on this handle (not a strip of a decomposition, no distributed grains)"
NO_COMPUTE = "%s: no lbmdem_strain_compute has been made for the mark and the grains where they are now"
NO_MARK = "%s: no lbmdem_strain_mark has been made on this handle"
NO_LIST = "lbmdem_strain_mark: no lbmdem_structure_compute has been made for the grains where they are now"
COUNTS_ONLY = ("lbmdem_strain_mark: the last lbmdem_structure_compute had max_entries == 0: counts and histogram only, and the "
               "mark needs its neighbour list")
READERS = ("lbmdem_download_strain_grains", "lbmdem_strain_grains_device")
REF_KEYS = ("x0", "y0", "th0", "offsets", "nbr", "rc2", "nbsteps")


def restatement_of(sim, ref=None):
    ref = sim.strain_reference() if ref is None else ref
    k = sim.kinematics
    return su.restate(ref["x0"], ref["y0"], ref["th0"], ref["offsets"], ref["nbr"], ref["rc2"], k[:, 0], k[:, 1], k[:, 2])


def compare(sim, R, counts, what=None):
    assert counts == R["counts"], (what, counts, R["counts"])
    g = sim.strain_grains()
    for name in su.INTS:
        assert g[name].dtype == np.int32 and np.array_equal(g[name], R["grains"][name]), (what, name,
                                                                                          np.nonzero(g[name] != R["grains"][name])[0][:5])
    for name in su.DOUBLES:
        assert su.same_bits(g[name], R["grains"][name]), (what, name, np.nonzero(g[name] != R["grains"][name])[0][:5])
    return R


def check(sim, what=None):
    """one compute against the restatement over the handle's mark and kinematics, every output -> the restatement"""
    R = restatement_of(sim)
    return compare(sim, R, sim.strain(), what)


def mark(sim, rcut):
    """structure(rcut, 1, 1.0) and the mark; the mark against the kinematics and the all-pairs list -> strain_reference()"""
    sim.structure(rcut, 1, 1.0)
    k = sim.kinematics
    entries = sim.strain_mark()
    ref = sim.strain_reference()
    off, nbr, rc2 = su.neighbour_list(k[:, 0], k[:, 1], rcut)
    assert entries == len(nbr) == len(ref["nbr"]) and ref["rc2"] == rc2 and ref["nbsteps"] == sim.nbsteps
    assert ref["offsets"].dtype == ref["nbr"].dtype == np.int32
    assert np.array_equal(ref["offsets"], off) and np.array_equal(ref["nbr"], nbr)
    s_off, s_nbr = sim.structure_neighbours()
    assert np.array_equal(s_off, off) and np.array_equal(s_nbr, nbr)
    for key, col in (("x0", 0), ("y0", 1), ("th0", 2)):
        assert su.same_bits(ref[key], k[:, col]), key
    return ref


def same_reference(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8) if isinstance(a[k], np.ndarray) else a[k],
                              np.asarray(b[k]).view(np.uint8) if isinstance(b[k], np.ndarray) else b[k]) for k in REF_KEYS)


def disturbed(k, rcut, seed, m):
    """an affine map of the centres plus noise; grain m two cutoffs away; the last centre NaN"""
    rng = np.random.default_rng(seed)
    n = len(k)
    k = k.copy()
    x, y = k[:, 0].copy(), k[:, 1].copy()
    k[:, 0] = 1.01 * x + 0.02 * y + rng.normal(0, 0.01 * rcut, n)
    k[:, 1] = -0.01 * x + 0.98 * y + rng.normal(0, 0.01 * rcut, n)
    k[:, 2] += rng.normal(0, 0.3, n)
    k[m, 1] += 2.0 * rcut
    k[n - 1, 0] = np.nan
    return k


@pytest.mark.parametrize("cut", [1.1, 3.3])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257, 1025])
def test_shapes_against_the_restatement(pkg, n, cut):
    lx, ly, r, x, y, k = shape_packing(n)
    rcut = cut * 2.0 * float(r.mean())
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        ref = mark(sim, rcut)
        deg = np.diff(ref["offsets"])
        # the restatement first: the small cutoff leaves grains with fewer than two neighbours, the large one none (n = 1, 2 can
        # have nothing else)
        if cut == 1.1 or n <= 2:
            assert (deg < 2).any()
        else:
            assert (deg >= 2).all()
        # the mark against itself
        R = check(sim, (n, cut, "at once"))
        g = R["grains"]
        assert R["counts"]["lost"] == 0 and R["counts"]["few"] == int((deg < 2).sum()) and R["counts"]["entries"] == deg.sum()
        assert not g["ux"].any() and not g["uy"].any() and not g["drot"].any()
        # after sub-steps
        table_substep(sim, k, 1)
        for _ in range(3):
            sim.dem_substep()
        assert same_reference(sim.strain_reference(), ref)
        R = check(sim, (n, cut, "after sub-steps"))
        assert np.abs(R["grains"]["ux"]).max() > 0 and np.abs(R["grains"]["drot"]).max() > 0
        # after an upload
        m = int(np.argmax(deg[:-1] > 0)) if n > 1 else 0          # the first grain that has a neighbour to lose
        sim.kinematics = disturbed(sim.kinematics, rcut, n, m)
        assert same_reference(sim.strain_reference(), ref)
        R = check(sim, (n, cut, "after an upload"))
        g, c = R["grains"], R["counts"]
        assert c["nonfinite_grains"] == 1 and g["flags"][n - 1] == su.NONFINITE
        if n >= 63:          # (a handful of grains have no neighbour to lose and none to fit)
            assert c["lost"] > 0 and g["lost"][m] > 0
            assert c["fitted"] > 0 and c["worst_grain"] >= 0 and g["d2min"][c["worst_grain"]] == g["d2min"].max() > 0
            if cut == 3.3:
                assert c["fitted"] > n // 2
        # the torch views are the downloads
        got = sim.strain_grains()
        tv = sim.strain_tensors()
        for name in su.STRAIN_DTYPE.names:
            assert tv[name].is_cuda and np.array_equal(tv[name].cpu().numpy().view(np.uint8),
                                                       np.ascontiguousarray(got[name]).view(np.uint8)), name
        # any pointer may be NULL; sizing, and a buffer that is one entry short
        L = pkg.load_library()
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        flags, d2 = np.full(n, -1, np.int32), np.full(n, -1.0)
        assert L.lbmdem_download_strain_grains(sim._h, *([None] * 7), vp(d2), None, None, vp(flags)) == 0
        assert np.array_equal(flags, got["flags"]) and su.same_bits(d2, got["d2min"])
        assert L.lbmdem_download_strain_grains(sim._h, *([None] * 11)) == 0
        assert L.lbmdem_strain_grains_device(sim._h, *([None] * 11)) == 0
        cnt, rc2, nbs = ctypes.c_long(-1), ctypes.c_double(-1.0), ctypes.c_long(-1)
        assert L.lbmdem_download_strain_reference(sim._h, None, None, None, None, None, 0, ctypes.byref(cnt), None, None) == 0
        assert cnt.value == len(ref["nbr"])
        if len(ref["nbr"]) > 1:
            only = np.full(len(ref["nbr"]), -9, np.int32)
            assert L.lbmdem_download_strain_reference(sim._h, None, None, None, None, vp(only), len(only), ctypes.byref(cnt),
                                                      ctypes.byref(rc2), ctypes.byref(nbs)) == 0
            assert np.array_equal(only, ref["nbr"]) and rc2.value == ref["rc2"] and nbs.value == ref["nbsteps"]
            small, cnt.value = np.full(len(only) - 1, -7, np.int32), -1
            assert L.lbmdem_download_strain_reference(sim._h, None, None, None, None, vp(small), len(small), ctypes.byref(cnt),
                                                      None, None) == -1
            assert cnt.value == len(only) and (small == -7).all()
            assert "there are %d entries, the buffer holds %d" % (len(only), len(small)) in L.lbmdem_last_error().decode()


def test_the_mark_is_a_copy(pkg):
    lx, ly, r, x, y, k = shape_packing(257)
    D = 2.0 * float(r.mean())
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        table_substep(sim, k, 1)
        ref = mark(sim, 3.3 * D)
        sim.dem_substep()
        R = check(sim)
        before = sim.strain_grains()
        sim.structure(1.7 * D, 9, 1.3)
        assert same_reference(sim.strain_reference(), ref)
        sim.structure(5.0 * D, 3, 1.1, max_entries=0)
        assert same_reference(sim.strain_reference(), ref)
        sim.voronoi(2.2 * D)
        sim.voronoi_faces()
        assert same_reference(sim.strain_reference(), ref)
        assert np.array_equal(sim.strain_grains().view(np.uint8), before.view(np.uint8))      # the result too
        compare(sim, R, sim.strain())
        assert np.array_equal(sim.strain_grains().view(np.uint8), before.view(np.uint8))
        # and the other way round: marks and computes leave the structure and the Voronoi results as they were
        sim.structure(2.5 * D, 5, 1.2)
        sim.voronoi()
        s0, v0, n0 = sim.structure_grains(), sim.voronoi_grains(), sim.structure_neighbours()
        sim.strain_mark()
        sim.strain()
        sim.strain_clear()
        assert np.array_equal(sim.structure_grains().view(np.uint8), s0.view(np.uint8))
        assert np.array_equal(sim.voronoi_grains().view(np.uint8), v0.view(np.uint8))
        assert all(np.array_equal(a, b) for a, b in zip(sim.structure_neighbours(), n0))


def test_validity(pkg):
    lx, ly, r, x, y, k = shape_packing(65)
    rcut = 3.3 * 2.0 * float(np.mean(r))
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        calls = (sim.strain_grains, sim.strain_tensors)

        def text(call):
            with pytest.raises(pkg.LbmDemError) as e:
                call()
            assert e.value.code == -1
            return sim._L.lbmdem_last_error().decode()

        def refused():
            for who, call in zip(READERS, calls):
                assert text(call) == NO_COMPUTE % who

        def unmarked():
            refused()
            assert text(sim.strain) == NO_MARK % "lbmdem_strain_compute"
            assert text(sim.strain_reference) == NO_MARK % "lbmdem_download_strain_reference"
        unmarked()                                    # after create
        assert text(sim.strain_mark) == NO_LIST       # no structure compute yet
        sim.structure(rcut, 7, 1.2, max_entries=0)
        assert text(sim.strain_mark) == COUNTS_ONLY   # a counts-only structure compute
        unmarked()
        ref = mark(sim, rcut)
        refused()                                     # a mark is no compute
        check(sim)
        table_substep(sim, k, 1)
        refused()                                     # after a sub-step
        assert same_reference(sim.strain_reference(), ref)       # the mark survives it
        assert text(sim.strain_mark) == NO_LIST       # the list is stale: refused, and the earlier mark stays
        assert same_reference(sim.strain_reference(), ref)
        check(sim)
        sim.renderScene(2)
        refused()                                     # after coupled steps
        check(sim)
        sim.strain_grains()                           # reading does not invalidate
        sim.kinematics = sim.kinematics
        refused()                                     # after an upload of kinematics
        assert same_reference(sim.strain_reference(), ref)
        check(sim)
        sim.structure(rcut, 7, 1.2, max_entries=0)
        assert text(sim.strain_mark) == COUNTS_ONLY
        sim.strain_grains()                           # a refused mark leaves mark and result as they were
        assert same_reference(sim.strain_reference(), ref)
        ref2 = mark(sim, 0.5 * rcut)
        assert not same_reference(ref2, ref)
        refused()                                     # after a new mark
        check(sim)
        sim.strain_clear()
        unmarked()                                    # after a clear: no result, no mark; a refused compute leaves none either
        mark(sim, rcut)
        check(sim)


def test_a_mark_survives_wall_moves(pkg):
    lx, ly = mw.SMALL_SHAPES[1]
    r, x, y = mw.small_scene(lx, ly, 65)
    rcut = 3.3 * 2.0 * float(r.mean())
    with pkg.LbmDem(lx, ly, r, x, y, physics=mw.small_physics(pkg, lx, ly, r)) as sim:
        sim.set_vibration(True)
        ref = mark(sim, rcut)
        R = check(sim)
        before, walls = sim.strain_grains(), sim.walls()
        sim.move_walls()
        assert not np.array_equal(sim.walls(), walls)
        assert same_reference(sim.strain_reference(), ref)
        assert np.array_equal(sim.strain_grains().view(np.uint8), before.view(np.uint8))      # walls do not enter
        compare(sim, R, sim.strain())
    lx, ly, r, x1, x2 = mw.shaken_inputs()
    with pkg.LbmDem(lx, ly, r, x1, x2, physics=mw.shaken_physics(pkg)) as sim:          # a vibrating handle in a run
        sim.set_vibration(True)
        ref = mark(sim, 10.0 * 2.0 * float(r.mean()))
        for piece in mw.PIECES[:3]:
            sim.renderScene(piece)
            assert same_reference(sim.strain_reference(), ref)
            R = check(sim)
        assert np.abs(R["grains"]["ux"]).max() > 0


def test_refusals(pkg, tmp_path):
    lx, ly, r, x, y, k = shape_packing(65)
    rcut = 2e-3
    if os.path.exists(pkg.SP_LIB_PATH):
        with pkg.LbmDem(lx, ly, r, x, y, precision="f32") as sp:
            for call in (sp.strain_mark, sp.strain_clear, sp.strain, sp.strain_grains, sp.strain_tensors, sp.strain_reference,
                         lambda: sp.write_strain(".", 0, rcut), lambda: sp.set_strain_output(True, rcut)):
                with pytest.raises(pkg.LbmDemError) as e:
                    call()
                assert e.value.code == -1
                assert sp._L.lbmdem_last_error().decode() == "the strain analysis is not available in the single-precision build of the library"

    def text(sim, call):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1, e.value
        return sim._L.lbmdem_last_error().decode()
    with pkg.LbmDem(lx, ly, r, x, y, strip=(lx // 2, lx), halo=12) as strip:
        for who, call in (("lbmdem_strain_mark", strip.strain_mark),
                          ("lbmdem_strain_clear", strip.strain_clear),
                          ("lbmdem_strain_compute", strip.strain),
                          ("lbmdem_download_strain_grains", strip.strain_grains),
                          ("lbmdem_strain_grains_device", strip.strain_tensors),
                          ("lbmdem_download_strain_reference", strip.strain_reference),
                          ("lbmdem_write_strain", lambda: strip.write_strain(".", 0, rcut)),
                          ("lbmdem_set_strain_output", lambda: strip.set_strain_output(True, rcut))):
            assert text(strip, call) == who + WHOLE
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert text(sim, lambda: sim.set_strain_output(True, bad)).startswith("lbmdem_set_strain_output: rcut must be finite and > 0")
            assert text(sim, lambda: sim.write_strain(str(tmp_path), 0, bad)).startswith("lbmdem_write_strain: rcut must be finite and > 0")
        assert text(sim, lambda: sim.write_strain(str(tmp_path / "not" / "there"), 0, rcut)).startswith("cannot open")
        assert os.listdir(tmp_path) == []
        sim.set_strain_output(True, rcut)
        assert text(sim, sim.dist_enable) == ("the strain analysis is not available with distributed grains "
                                              "(lbmdem_set_strain_output(h, 0, 0., 0) first)")
        sim.set_strain_output(False)
        sim.dist_enable()
        for who, call in (("lbmdem_set_strain_output", lambda: sim.set_strain_output(True, rcut)),
                          ("lbmdem_strain_mark", sim.strain_mark),
                          ("lbmdem_strain_compute", sim.strain),
                          ("lbmdem_write_strain", lambda: sim.write_strain(".", 0, rcut))):
            assert text(sim, call) == who + WHOLE


def test_analysis_does_not_interfere(pkg, tmp_path):
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    r, x, y = z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3
    rcut = 3.3 * 2.0 * float(r.mean())
    with pkg.LbmDem(256, 200, r, x, y) as a, pkg.LbmDem(256, 200, r, x, y) as b:
        for piece in (1, 7, 3, 13):
            a.renderScene(piece); b.renderScene(piece)
            a.write_strain(str(tmp_path), piece, rcut, incremental=(piece == 3))
            a.strain(); a.strain_grains(); a.strain_reference()
            if piece == 7:
                a.structure(rcut / 2, 1, 1.0); a.strain_mark(); a.strain()
        assert a.nbsteps == b.nbsteps == 24
        for what in ("f", "obst", "kinematics", "fhf"):
            assert np.array_equal(getattr(a, what), getattr(b, what)), what
        assert sorted(os.listdir(tmp_path)) == sorted(["strain%06d.dat" % p for p in (1, 3, 7, 13)] + ["strain.data"])


STEPS = 12000          # three DEM events


@pytest.fixture(scope="module")
def g6_scene(pkg, tmp_path_factory):
    """the G6 golden through run_scene over three DEM events: without the strain output, with it, with it and incremental; and the
    states at the events, from a handle run event by event (an event's files carry the frame counter of scene_schedule: two events
    between two frames write the same strain%.6i.dat, the later one last)"""
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    r, x, y = z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3
    rcut = 3.3 * 2.0 * float(r.mean())
    dirs = {k: tmp_path_factory.mktemp(k) for k in ("without", "cumulative", "incremental")}
    for kind, d in dirs.items():
        with pkg.LbmDem(256, 200, r, x, y) as sim:
            if kind != "without":
                sim.set_strain_output(True, rcut, incremental=(kind == "incremental"))
            sim.run_scene(STEPS, str(d))
            if kind == "cumulative":
                last = sim.kinematics
    states = []
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        events = [(step, nfile) for kind, step, nfile in pkg.scene_schedule(sim.config(), 0, STEPS) if kind == "DEM"]
        assert len(events) == 3 and events[-1][0] == STEPS
        for step, nfile in events:
            sim.run_scene(step - sim.nbsteps)
            assert sim.nbsteps == step
            states.append(dict(k=sim.kinematics, nbsteps=sim.nbsteps, dt=sim.config().dt, nfile=nfile))
    assert np.array_equal(states[-1]["k"].view(np.uint8), last.view(np.uint8))      # event by event is the same run
    return dict(z=z, rcut=rcut, dirs=dirs, states=states)


def expected_files(S, incremental):
    """strain%.6i.dat of every event and strain.data, from the restatement over the states at the events"""
    states, rcut = S["states"], S["rcut"]
    texts, data = {}, su.DATA_HEADER
    m = 0                                                      # the event of the mark
    for e, now in enumerate(states):
        at = states[m]
        off, nbr, rc2 = su.neighbour_list(at["k"][:, 0], at["k"][:, 1], rcut)
        R = su.restate(at["k"][:, 0], at["k"][:, 1], at["k"][:, 2], off, nbr, rc2, now["k"][:, 0], now["k"][:, 1], now["k"][:, 2])
        a, b = su.files_text(R["grains"], rc2, R["counts"], now["nbsteps"] * now["dt"], at["nbsteps"] * at["dt"])
        texts["strain%06d.dat" % now["nfile"]] = a
        data += b
        if incremental:
            m = e
        if e == len(states) - 1:
            assert R["counts"]["fitted"] > 0 and np.abs(R["grains"]["ux"]).max() > 0 and R["grains"]["d2min"].max() > 0
    texts["strain.data"] = data
    return texts


@pytest.mark.parametrize("kind", ["cumulative", "incremental"])
def test_g6_through_run_scene(g6_scene, kind):
    S = g6_scene
    want = expected_files(S, kind == "incremental")
    others = sorted(os.listdir(S["dirs"]["without"]))
    assert sorted(os.listdir(S["dirs"][kind])) == sorted(others + list(want)) and "DEM%06d.dat" % S["states"][-1]["nfile"] in others
    for name in others:
        assert (S["dirs"][kind] / name).read_bytes() == (S["dirs"]["without"] / name).read_bytes(), name
    for name, text in want.items():
        assert (S["dirs"][kind] / name).read_text() == text, name
    assert expected_files(S, True)["strain.data"] != expected_files(S, False)["strain.data"]      # (the two modes can be told apart)


@pytest.mark.parametrize("kind", ["cumulative", "incremental"])
def test_host_driver_writes_the_strain_files(po, g6_scene, tmp_path, kind):
    """`lbmdem <G6> --steps 12000 --strain RCUT [--strain-incremental]` in a child process"""
    S, z = g6_scene, g6_scene["z"]
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), z["r_mm"], z["x_mm"], z["y_mm"])
    extra = ["--strain-incremental"] if kind == "incremental" else []
    out = subprocess.run([EXE, str(sample), "--lx", "256", "--ly", "200", "--steps", str(STEPS), "--strain",
                          repr(S["rcut"])] + extra, capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    for name in sorted({"strain%06d.dat" % st["nfile"] for st in S["states"]}) + ["strain.data"]:
        assert (tmp_path / name).read_bytes() == (S["dirs"][kind] / name).read_bytes(), name
    if kind == "cumulative":
        refused = subprocess.run([EXE, str(sample), "--strain", "2e-3", "--gpus", "2"], capture_output=True, text=True, cwd=tmp_path,
                                 timeout=120)
        assert refused.returncode != 0 and "--strain is a single-GPU mode" in refused.stderr
