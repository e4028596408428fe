"""GPU: the pore space analysis (lbmdem_pore_compute and its readers, lbmdem_write_pores, lbmdem_set_pores_output;
include/lbmdem_hip.h) against the numpy restatement over obst and f (tests/pore_util.py): every output by array_equal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pore_util as pz
import samples
from test_pore_host import pocket_scene, some_f

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
WHOLE = " needs the whole lattice and all grains on this handle (not a strip of a decomposition, no distributed grains)"
NO_COMPUTE = "%s: no lbmdem_pore_compute has been made for the map and the populations as they are now"
READERS = ("lbmdem_download_pore_labels", "lbmdem_pore_labels_device", "lbmdem_download_pores", "lbmdem_download_pore_grains",
           "lbmdem_pore_grains_device")
GRAINS = ("wet", "pore_min", "pore_max")


def readers_of(sim):
    return (sim.pore_labels, sim.pore_labels_tensor, sim.pore_table, sim.pore_grains, sim.pore_grains_tensors)


def check(sim, conn, M=None, f=None, what=""):
    """one compute against the restatement, every output -> the restatement. M: a caller's map (None: the handle's); f: what the
    handle holds, when the caller knows it"""
    R = pz.restate(sim.obst if M is None else M, sim.f if f is None else f, sim.n, conn)
    what = (what, sim.lx, sim.ly, conn)
    counts = sim.pores(conn, M)
    assert counts == R["counts"], (what, counts, R["counts"])
    label = sim.pore_labels()
    assert label.dtype == np.int32 and np.array_equal(label, R["label"]), (what, np.argwhere(label != R["label"])[:5])
    table = sim.pore_table()
    assert table.dtype == pz.PORE_DTYPE and len(table) == len(R["table"]), what
    for name in pz.PORE_DTYPE.names:
        assert np.array_equal(table[name], R["table"][name]), (what, name, np.nonzero(table[name] != R["table"][name])[0][:5])
    g = sim.pore_grains()
    for name in GRAINS:
        assert g[name].dtype == np.int32 and np.array_equal(g[name], R[name]), (what, name, np.nonzero(g[name] != R[name])[0][:5])
    return R


def shape_scene(lx, ly):
    """the shape sweep's packing (tests/golden/make_golden.py)"""
    r, x, y = samples.row_packing(lx, ly, 400, seed=1000 * lx + ly, margin=0.05)
    if len(r) < 3:       # 13 rows = 1.3 mm: only small grains fit
        r, x, y = samples.row_packing(lx, ly, 400, seed=1000 * lx + ly, margin=0.05, rmin=0.3, rmax=0.45)
    return samples.to_metres(r, x, y)


@pytest.mark.parametrize("lx,ly", [(13, 61), (33, 62), (61, 59), (64, 64), (100, 63), (127, 121), (203, 122), (256, 200)])
def test_rasterised_maps(pkg, lx, ly):
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        for conn in (4, 8):
            R = check(sim, conn, what="rest")
        assert R["counts"]["fluid_nodes"] > 0 and R["counts"]["components"] >= 1 and (R["wet"] > 0).any()
        sim.renderScene(2 * sim.cfg.npDEM + 1)      # two fluid steps: rho differs from node to node
        rho = pz.rho_of(sim.f)[sim.obst == -1]
        assert len(np.unique(rho)) > 10
        for conn in (4, 8):
            check(sim, conn, what="stepped")


def test_pockets_of_a_touching_packing(pkg):
    """reductionR = 1: the discs are rasterised with their full radius and seal the gaps between them"""
    lx, ly, r, x, y = pocket_scene()
    phys = pkg.Physics()
    pkg.load_library().lbmdem_physics_defaults(ctypes.byref(phys))
    phys.reductionR = 1.0
    with pkg.LbmDem(lx, ly, r, x, y, physics=phys) as sim:
        for conn in (4, 8):
            R = check(sim, conn, what="pockets")
            assert R["counts"]["components"] > 1 and R["counts"]["trapped_nodes"] > 0
            assert (R["pore_min"] != R["pore_max"]).any() and R["counts"]["throat_grains"] > 0
        sim.renderScene(sim.cfg.npDEM + 1)
        for conn in (4, 8):
            assert check(sim, conn, what="pockets, stepped")["counts"]["components"] > 1


CALLER_SHAPES = [(65, 17), (17, 65), (127, 121), (121, 127), (257, 513), (513, 257)]


@pytest.mark.parametrize("lx,ly", CALLER_SHAPES)
def test_callers_maps(pkg, lx, ly):
    """every map of pore_util.shape_maps; the second shape of a pair runs the first one's maps transposed, so that the seams along
    both axes are crossed by every shape"""
    transposed = (lx, ly) in CALLER_SHAPES[1::2]
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        n = sim.n
        maps = pz.shape_maps(ly, lx, n) if transposed else pz.shape_maps(lx, ly, n)
        f = some_f(lx, ly, seed=lx)
        sim.f = f
        assert np.array_equal(sim.f.view(np.uint64), f.view(np.uint64))
        own = sim.obst
        for name, M in maps.items():
            M = np.ascontiguousarray(M.T) if transposed else M
            for conn in (4, 8):
                R = check(sim, conn, M, f, what=name)
            c = R["counts"]      # (conn == 8)
            if name in ("all_fluid", "checkerboard", "serpentine", "comb", "u_shape"):
                assert c["components"] == 1, name
            if name == "all_fluid":
                assert c["spanning"] == 3 and c["largest_nodes"] == lx * ly and c["dry_grains"] == n
            if name == "no_fluid":
                assert c["components"] == 0 and c["largest_label"] == -1 and len(sim.pore_table()) == 0
            assert c["unaccumulated"] == int(((M == -1) & ~(np.abs(pz.rho_of(f)) < 2.0 ** 20)).sum())
        # a caller's map leaves the handle's alone
        assert np.array_equal(sim.obst, own)
        check(sim, 8, what="own map after callers' maps")


def test_map_validation(pkg):
    lx, ly = 65, 17
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        n = sim.n
        check(sim, 8)
        for bad in (n + 1, -2):
            M = pz.shape_maps(lx, ly, n)["random_60"]
            M[40, 3] = bad
            M[41, 5] = bad
            with pytest.raises(pkg.LbmDemError) as e:
                sim.pores(8, M)
            assert e.value.code == -1
            text = sim._L.lbmdem_last_error().decode()
            assert text.startswith("lbmdem_pore_compute: map[%d] = %d (node 40, 3)" % (40 * ly + 3, bad)), text
            with pytest.raises(pkg.LbmDemError):      # no result exists after a refused compute
                sim.pore_labels()
            assert sim._L.lbmdem_last_error().decode() == NO_COMPUTE % "lbmdem_download_pore_labels"
        with pytest.raises(pkg.LbmDemError):
            sim.pores(8, np.zeros((ly, lx), np.int32))
        check(sim, 4)


def test_readers_refuse_before_a_compute_and_after_a_change(pkg):
    lx, ly = 100, 63
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim, pkg.LbmDem(lx, ly, r, x, y) as twin:
        def refused():
            for who, call in zip(READERS, readers_of(sim)):
                with pytest.raises(pkg.LbmDemError) as e:
                    call()
                assert e.value.code == -1
                assert sim._L.lbmdem_last_error().decode() == NO_COMPUTE % who
        refused()                                   # after create
        check(sim, 8)
        for call in readers_of(sim):                # reading does not invalidate
            call()
        sim.renderScene(sim.cfg.npDEM + 1); twin.renderScene(twin.cfg.npDEM + 1)
        refused()                                   # after coupled steps
        for what in ("f", "obst", "kinematics", "fhf"):      # ... which the compute has not disturbed
            assert np.array_equal(getattr(sim, what), getattr(twin, what)), what
        check(sim, 4)
        sim.dem_substep(); twin.dem_substep()
        refused()                                   # after a sub-step
        check(sim, 8)
        sim.lbm_step(); twin.lbm_step()
        refused()                                   # after a fluid step
        check(sim, 8)
        sim.f = sim.f; twin.f = twin.f
        refused()                                   # after an upload of f
        check(sim, 8)
        sim.kinematics = sim.kinematics; twin.kinematics = twin.kinematics
        refused()                                   # after an upload of kinematics
        check(sim, 8)
        sim.pores(4, pz.shape_maps(lx, ly, sim.n)["comb"])
        sim.renderScene(3); twin.renderScene(3)
        refused()
        for what in ("f", "obst", "kinematics", "fhf"):
            assert np.array_equal(getattr(sim, what), getattr(twin, what)), what


def test_sizing_and_device_views(pkg):
    lx, ly = 127, 121
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        n = sim.n
        M = pz.shape_maps(lx, ly, n)["random_40"]
        R = check(sim, 4, M)
        L = pkg.load_library()
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        cnt = ctypes.c_long(-1)
        assert L.lbmdem_download_pores(sim._h, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == len(R["table"]) > 10
        short, cnt.value = np.zeros(len(R["table"]) - 1, pz.PORE_DTYPE), -1
        short["label"] = -7
        assert L.lbmdem_download_pores(sim._h, vp(short), len(short), ctypes.byref(cnt)) == -1
        assert cnt.value == len(R["table"]) and (short["label"] == -7).all() and (short["nodes"] == 0).all()
        assert "there are %d components, the buffer holds %d" % (len(R["table"]), len(short)) in L.lbmdem_last_error().decode()
        roomy = np.zeros(len(R["table"]) + 3, pz.PORE_DTYPE)
        assert L.lbmdem_download_pores(sim._h, vp(roomy), len(roomy), ctypes.byref(cnt)) == 0
        assert np.array_equal(roomy[:cnt.value], R["table"]) and (roomy[cnt.value:]["nodes"] == 0).all()
        # any pointer may be NULL
        only = np.full(n, -9, np.int32)
        assert L.lbmdem_download_pore_grains(sim._h, None, vp(only), None) == 0 and np.array_equal(only, R["pore_min"])
        assert L.lbmdem_download_pore_grains(sim._h, None, None, None) == 0
        assert L.lbmdem_pore_grains_device(sim._h, None, None, None) == 0
        assert L.lbmdem_download_pore_labels(sim._h, None) == -1 and L.lbmdem_pore_labels_device(sim._h, None, None) == -1
        assert L.lbmdem_pore_compute(sim._h, 8, None, None) == -1
        # the torch views are the downloads; the label view is indexed through the row pitch
        tv = sim.pore_grains_tensors()
        for name in GRAINS:
            assert tv[name].is_cuda and np.array_equal(tv[name].cpu().numpy(), R[name])
        lt = sim.pore_labels_tensor()
        sy = lt.shape[1]
        assert lt.is_cuda and lt.shape[0] == lx and sy >= ly and sy % 16 == 0
        host = lt.cpu().numpy()
        assert np.array_equal(host[:, :ly], R["label"]) and (host[:, ly:] == -1).all()
        assert int(lt.reshape(-1)[5 * sy + 7]) == R["label"][5, 7]


def test_refusals(pkg, tmp_path):
    lx, ly = 64, 64
    r, x, y = shape_scene(lx, ly)
    calls = lambda s: ([("lbmdem_pore_compute", s.pores)] + list(zip(READERS, readers_of(s))) +
                       [("lbmdem_write_pores", lambda: s.write_pores(str(tmp_path), 0)),
                        ("lbmdem_set_pores_output", lambda: s.set_pores_output(True))])

    def text(sim, call):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1, e.value
        return sim._L.lbmdem_last_error().decode()
    if os.path.exists(pkg.SP_LIB_PATH):
        with pkg.LbmDem(lx, ly, r, x, y, precision="f32") as sp:
            for who, call in calls(sp):
                assert text(sp, call) == "the pore space analysis is not available in the single-precision build of the library", who
    with pkg.LbmDem(lx, ly, r, x, y, strip=(lx // 2, lx), halo=12) as strip:
        for who, call in calls(strip):
            assert text(strip, call) == who + WHOLE
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        for bad in (0, 6, -8, 9):
            assert text(sim, lambda: sim.pores(bad)) == "lbmdem_pore_compute: conn is 4 or 8 (%d)" % bad
            assert text(sim, lambda: sim.set_pores_output(True, bad)) == "lbmdem_set_pores_output: conn is 4 or 8 (%d)" % bad
            assert text(sim, lambda: sim.write_pores(str(tmp_path), 0, bad)) == "lbmdem_pore_compute: conn is 4 or 8 (%d)" % bad
        missing = str(tmp_path / "missing")
        assert text(sim, lambda: sim.write_pores(missing, 0)) == f"cannot open '{missing}/pore_table000000.dat' for writing"
        assert os.listdir(tmp_path) == []
        sim.set_pores_output(True, 4)
        assert text(sim, sim.dist_enable) == ("the pore space analysis is not available with distributed grains "
                                              "(lbmdem_set_pores_output(h, 0, 0, 0) first)")
        sim.set_pores_output(False)
        sim.dist_enable()
        for who, call in calls(sim):
            assert text(sim, call) == who + WHOLE


@pytest.fixture(scope="module")
def scene(pkg, tmp_path_factory):
    """a packing through run_scene over two DEM events, with the pore output on and without"""
    lx, ly = 61, 59
    r, x, y = shape_scene(lx, ly)
    with_dir, without_dir = tmp_path_factory.mktemp("with"), tmp_path_factory.mktemp("without")
    steps = 8000
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.run_scene(steps, str(without_dir))
        end = {what: getattr(sim, what) for what in ("f", "obst", "kinematics", "fhf")}
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.set_pores_output(True, 4, plane=True)
        _, res = sim.run_scene(steps, str(with_dir))
        for what in end:
            assert np.array_equal(getattr(sim, what), end[what]), what
        # the last event is the run's last sub-step: the restatement of the state the run ends in
        R = pz.restate(sim.obst, sim.f, sim.n, 4)
        t = sim.nbsteps * sim.config().dt
    return dict(lx=lx, ly=ly, r=r, x=x, y=y, with_dir=with_dir, without_dir=without_dir, steps=steps, R=R, t=t, nfile=res["nfile"])


def test_run_scene_with_the_pore_output(pkg, scene, tmp_path):
    S = scene
    lx, ly, R, last = S["lx"], S["ly"], S["R"], S["nfile"]
    others = sorted(os.listdir(S["without_dir"]))
    numbers = sorted({int(name[3:9]) for name in others if name.startswith("DEM") and name.endswith(".dat")})
    assert last in numbers
    new = ["pores.data"] + [p % k for k in numbers for p in ("pore_table%06d.dat", "pore_grains%06d.dat", "pores%06d.vtk")]
    assert sorted(os.listdir(S["with_dir"])) == sorted(others + new)
    for name in others:
        assert (S["with_dir"] / name).read_bytes() == (S["without_dir"] / name).read_bytes(), name
    # one line per DEM event, as stats.data has
    lines = (S["with_dir"] / "pores.data").read_text().splitlines()
    events = len((S["with_dir"] / "stats.data").read_text().splitlines())
    assert lines[0] + "\n" == pz.DATA_HEADER and len(lines) == 1 + events and events == 2
    assert R["counts"]["fluid_nodes"] > 0 and len(R["table"]) >= 1
    pkg.write_pore_files(str(tmp_path), last, 4, lx, ly, R["table"], R["wet"], R["pore_min"], R["pore_max"], R["counts"], S["t"],
                         label=R["label"])
    want = pz.files_bytes(4, lx, ly, R, S["t"], nfile=last, plane=True)
    assert lines[-1] + "\n" == want.pop("pores.data").decode()
    for name, data in want.items():
        assert (S["with_dir"] / name).read_bytes() == data == (tmp_path / name).read_bytes(), name


def test_host_driver_writes_the_pore_files(po, scene, tmp_path):
    """`lbmdem <sample> --steps N --pores 4 --pores-plane` in a child process"""
    S = scene
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), S["r"] * 1e3, S["x"] * 1e3, S["y"] * 1e3)
    out = subprocess.run([EXE, str(sample), "--lx", str(S["lx"]), "--ly", str(S["ly"]), "--steps", str(S["steps"] + 1), "--pores", "4",
                          "--pores-plane"], capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    names = [name for name in os.listdir(S["with_dir"]) if name.startswith("pore")]
    assert "pores.data" in names and len(names) >= 4
    for name in names:
        assert (tmp_path / name).read_bytes() == (S["with_dir"] / name).read_bytes(), name
    refused = subprocess.run([EXE, str(sample), "--pores", "--gpus", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "--pores is a single-GPU mode" in refused.stderr
    refused = subprocess.run([EXE, str(sample), "--pores", "6"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "--pores [4|8]" in refused.stderr
