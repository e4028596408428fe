"""GPU: the pore clearance analysis (lbmdem_clearance_compute and its readers, lbmdem_write_clearance, lbmdem_set_clearance_output;
include/lbmdem_hip.h) against the numpy restatement over obst (tests/clearance_util.py): every output by array_equal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import clearance_util as cz
from test_gpu_pores import shape_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
WHOLE = " needs the whole lattice and all grains on this handle (not a strip of a decomposition, no distributed grains)"
NO_COMPUTE = "%s: no lbmdem_clearance_compute has been made for the map as it is now"
READERS = ("lbmdem_download_clearance", "lbmdem_clearance_device", "lbmdem_download_clearance_hist", "lbmdem_download_clearance_owners",
           "lbmdem_clearance_owners_device", "lbmdem_download_throats")


def readers_of(sim):
    return (sim.clearance_planes, sim.clearance_tensors, sim.clearance_hist, sim.clearance_owners, sim.clearance_owner_tensors,
            sim.throat_table)


def compare(sim, R, counts, what):
    assert counts == R["counts"], (what, counts, R["counts"])
    d2, owner = sim.clearance_planes()
    assert d2.dtype == np.int32 and np.array_equal(d2, R["d2"]), (what, np.argwhere(d2 != R["d2"])[:5])
    assert owner.dtype == np.int32 and np.array_equal(owner, R["owner"]), (what, np.argwhere(owner != R["owner"])[:5])
    hist = sim.clearance_hist()
    assert hist.dtype == np.int64 and np.array_equal(hist, R["hist"]), (what, hist, R["hist"])
    g = sim.clearance_owners()
    assert g["owned"].dtype == np.int64 and np.array_equal(g["owned"], R["owned"]), (what, g["owned"], R["owned"])
    assert g["d2max"].dtype == np.int32 and np.array_equal(g["d2max"], R["d2max"]), (what, g["d2max"], R["d2max"])
    table = sim.throat_table()
    assert table.dtype == cz.THROAT_DTYPE and len(table) == len(R["table"]), (what, len(table), len(R["table"]))
    for name in cz.THROAT_DTYPE.names:
        assert np.array_equal(table[name], R["table"][name]), (what, name, np.nonzero(table[name] != R["table"][name])[0][:5])


def check(sim, M=None, what="", max_edges=0):
    """one compute against the restatement, every output -> the restatement. M: a caller's map (None: the handle's)"""
    R = cz.restate(sim.obst if M is None else M, sim.n)
    compare(sim, R, sim.clearance(M, max_edges), (what, sim.lx, sim.ly))
    return R


@pytest.mark.parametrize("lx,ly", [(13, 61), (33, 62), (61, 59), (64, 64), (100, 63), (127, 121), (203, 122), (256, 200)])
def test_rasterised_packings(pkg, lx, ly):
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        R = check(sim, what="rest")
        assert R["counts"]["fluid_nodes"] > 0 and R["counts"]["throats"] >= 1 and R["counts"]["ridge_edges"] > 0
        if (lx, ly) == (256, 200):
            assert R["counts"]["grain_throats"] >= 1 and R["counts"]["narrowest_c"] >= 1
        sim.renderScene(2 * sim.cfg.npDEM + 1)
        check(sim, what="stepped")


CALLER_SHAPES = [(65, 17), (17, 65), (127, 121), (121, 127)]


@pytest.mark.parametrize("lx,ly", CALLER_SHAPES)
def test_callers_maps(pkg, lx, ly):
    """every map of clearance_util.shape_maps; the second shape of a pair runs the first one's maps transposed, so that the walk
    and the scan each meet every shape"""
    transposed = (lx, ly) in CALLER_SHAPES[1::2]
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        n = sim.n
        maps = cz.shape_maps(ly, lx, n) if transposed else cz.shape_maps(lx, ly, n)
        own = sim.obst
        for name, M in maps.items():
            M = np.ascontiguousarray(M.T) if transposed else M
            c = check(sim, M, what=name)["counts"]
            if name == "all_fluid":
                half = (min(lx, ly) + 1) // 2
                assert c["d2_max"] == half * half and c["throats"] == 0 and c["ownerless_grains"] == n
            if name == "no_fluid":
                assert c["fluid_nodes"] == 0 and c["kmax"] == 0 and len(sim.throat_table()) == 0 and len(sim.clearance_hist()) == 1
        # a caller's map leaves the handle's alone
        assert np.array_equal(sim.obst, own)
        check(sim, what="own map after callers' maps")


def test_callers_maps_wider_than_any_tile(pkg):
    """257 x 513: distances above every tile and chunk, walks that cross many workgroups"""
    lx, ly = 257, 513
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        maps = cz.shape_maps(lx, ly, sim.n)
        own = sim.obst
        for name in ("all_fluid", "sparse_seeds", "far_wall", "random_80", "disc_packing"):
            c = check(sim, maps[name], what=name)["counts"]
            if name in ("all_fluid", "sparse_seeds", "far_wall"):
                assert c["kmax"] > 64
        assert np.array_equal(sim.obst, own)
        check(sim, what="own map after callers' maps")


def test_budget(pkg):
    lx, ly = 127, 121
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        M = cz.shape_maps(lx, ly, sim.n)["disc_packing"]
        R = check(sim, M)
        edges = R["counts"]["ridge_edges"]
        assert edges > 10
        with pytest.raises(pkg.LbmDemError) as e:
            sim.clearance(M, max_edges=edges - 1)
        assert e.value.code == -1
        text = sim._L.lbmdem_last_error().decode()
        assert text == "lbmdem_clearance_compute: the ridge has %d edges, max_edges is %d" % (edges, edges - 1), text
        for who, call in zip(READERS, readers_of(sim)):      # no result exists after a refused compute
            with pytest.raises(pkg.LbmDemError):
                call()
            assert sim._L.lbmdem_last_error().decode() == NO_COMPUTE % who
        check(sim, M, what="the exact budget", max_edges=edges)
        with pytest.raises(pkg.LbmDemError):
            sim.clearance(M, max_edges=-1)
        assert "max_edges must lie in 0 .." in sim._L.lbmdem_last_error().decode()


def test_map_validation(pkg):
    lx, ly = 65, 17
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        n = sim.n
        check(sim)
        for bad in (n + 1, -2):
            M = cz.shape_maps(lx, ly, n)["random_60"]
            M[40, 3] = bad
            M[41, 5] = bad
            with pytest.raises(pkg.LbmDemError) as e:
                sim.clearance(M)
            assert e.value.code == -1
            text = sim._L.lbmdem_last_error().decode()
            assert text == ("lbmdem_clearance_compute: map[%d] = %d (node 40, 3) is neither -1 (fluid), a grain (0 .. %d) nor the wall "
                            "(%d)" % (40 * ly + 3, bad, n - 1, n)), text
            with pytest.raises(pkg.LbmDemError):      # no result exists after a refused compute
                sim.clearance_planes()
            assert sim._L.lbmdem_last_error().decode() == NO_COMPUTE % "lbmdem_download_clearance"
        with pytest.raises(pkg.LbmDemError):
            sim.clearance(np.zeros((ly, lx), np.int32))
        check(sim)


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
        check(sim)
        for call in readers_of(sim):                # reading does not invalidate
            call()
        sim.renderScene(sim.cfg.npDEM + 1); twin.renderScene(twin.cfg.npDEM + 1)
        refused()                                   # after coupled steps
        for what in ("f", "obst", "kinematics", "fhf"):      # ... which the compute has not disturbed
            assert np.array_equal(getattr(sim, what), getattr(twin, what)), what
        check(sim)
        sim.dem_substep(); twin.dem_substep()
        refused()                                   # after a sub-step
        check(sim)
        sim.lbm_step(); twin.lbm_step()
        refused()                                   # after a fluid step
        check(sim)
        sim.f = sim.f; twin.f = twin.f
        refused()                                   # after an upload of f
        check(sim)
        sim.kinematics = sim.kinematics; twin.kinematics = twin.kinematics
        refused()                                   # after an upload of kinematics
        check(sim)
        sim.clearance(cz.shape_maps(lx, ly, sim.n)["comb"])
        sim.renderScene(3); twin.renderScene(3)
        refused()
        for what in ("f", "obst", "kinematics", "fhf"):
            assert np.array_equal(getattr(sim, what), getattr(twin, what)), what


def test_sizing_and_device_views(pkg):
    lx, ly = 127, 121
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        n = sim.n
        M = cz.shape_maps(lx, ly, n)["disc_packing"]
        R = check(sim, M)
        L = pkg.load_library()
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        cnt = ctypes.c_long(-1)
        assert L.lbmdem_download_throats(sim._h, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == len(R["table"]) > 3
        short, cnt.value = np.zeros(len(R["table"]) - 1, cz.THROAT_DTYPE), -1
        short["lo"] = -7
        assert L.lbmdem_download_throats(sim._h, vp(short), len(short), ctypes.byref(cnt)) == -1
        assert cnt.value == len(R["table"]) and (short["lo"] == -7).all() and (short["edges"] == 0).all()
        assert "there are %d throats, the buffer holds %d" % (len(R["table"]), len(short)) in L.lbmdem_last_error().decode()
        roomy = np.zeros(len(R["table"]) + 3, cz.THROAT_DTYPE)
        assert L.lbmdem_download_throats(sim._h, vp(roomy), len(roomy), ctypes.byref(cnt)) == 0
        assert np.array_equal(roomy[:cnt.value], R["table"]) and (roomy[cnt.value:]["edges"] == 0).all()
        # the histogram is sized the same way
        bins = len(R["hist"])
        assert L.lbmdem_download_clearance_hist(sim._h, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == bins > 2
        few = np.full(bins - 1, -7, np.int64)
        assert L.lbmdem_download_clearance_hist(sim._h, vp(few), len(few), ctypes.byref(cnt)) == -1 and (few == -7).all()
        assert "there are %d bins, the buffer holds %d" % (bins, bins - 1) in L.lbmdem_last_error().decode()
        more = np.full(bins + 2, -7, np.int64)
        assert L.lbmdem_download_clearance_hist(sim._h, vp(more), len(more), ctypes.byref(cnt)) == 0
        assert np.array_equal(more[:bins], R["hist"]) and (more[bins:] == -7).all()
        # either plane may be NULL, not both; any owners' pointer may be NULL
        only = np.full((lx, ly), -9, np.int32)
        assert L.lbmdem_download_clearance(sim._h, None, vp(only)) == 0 and np.array_equal(only, R["owner"])
        assert L.lbmdem_download_clearance(sim._h, vp(only), None) == 0 and np.array_equal(only, R["d2"])
        assert L.lbmdem_download_clearance(sim._h, None, None) == -1
        one = np.full(n + 1, -9, np.int32)
        assert L.lbmdem_download_clearance_owners(sim._h, None, vp(one)) == 0 and np.array_equal(one, R["d2max"])
        assert L.lbmdem_download_clearance_owners(sim._h, None, None) == 0
        assert L.lbmdem_clearance_owners_device(sim._h, None, None) == 0
        assert L.lbmdem_clearance_device(sim._h, None, None, None) == -1
        assert L.lbmdem_clearance_compute(sim._h, None, 0, None) == -1
        # the torch views are the downloads; the planes are indexed through the row pitch
        tv = sim.clearance_owner_tensors()
        assert tv["owned"].is_cuda and np.array_equal(tv["owned"].cpu().numpy(), R["owned"])
        assert tv["d2max"].is_cuda and np.array_equal(tv["d2max"].cpu().numpy(), R["d2max"])
        pt = sim.clearance_tensors()
        sy = pt["d2"].shape[1]
        assert pt["d2"].is_cuda and pt["owner"].is_cuda and pt["d2"].shape == pt["owner"].shape
        assert pt["d2"].shape[0] == lx and sy >= ly and sy % 16 == 0 and sy > ly
        hd, ho = pt["d2"].cpu().numpy(), pt["owner"].cpu().numpy()
        assert np.array_equal(hd[:, :ly], R["d2"]) and (hd[:, ly:] == 0).all()
        assert np.array_equal(ho[:, :ly], R["owner"]) and (ho[:, ly:] == -1).all()
        assert int(pt["d2"].reshape(-1)[5 * sy + 7]) == R["d2"][5, 7] and int(pt["owner"].reshape(-1)[5 * sy + 7]) == R["owner"][5, 7]


def test_refusals(pkg, tmp_path):
    lx, ly = 64, 64
    r, x, y = shape_scene(lx, ly)
    calls = lambda s: ([("lbmdem_clearance_compute", s.clearance)] + list(zip(READERS, readers_of(s))) +
                       [("lbmdem_write_clearance", lambda: s.write_clearance(str(tmp_path), 0)),
                        ("lbmdem_set_clearance_output", lambda: s.set_clearance_output(True))])

    def text(sim, call):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1, e.value
        return sim._L.lbmdem_last_error().decode()
    if os.path.exists(pkg.SP_LIB_PATH):
        with pkg.LbmDem(lx, ly, r, x, y, precision="f32") as sp:
            for who, call in calls(sp):
                assert text(sp, call) == "the pore clearance analysis is not available in the single-precision build of the library", who
    with pkg.LbmDem(lx, ly, r, x, y, strip=(lx // 2, lx), halo=12) as strip:
        for who, call in calls(strip):
            assert text(strip, call) == who + WHOLE
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        missing = str(tmp_path / "missing")
        assert text(sim, lambda: sim.write_clearance(missing, 0)) == f"cannot open '{missing}/throats000000.dat' for writing"
        assert os.listdir(tmp_path) == []
        sim.set_clearance_output(True)
        assert text(sim, sim.dist_enable) == ("the pore clearance analysis is not available with distributed grains "
                                              "(lbmdem_set_clearance_output(h, 0, 0) first)")
        sim.set_clearance_output(False)
        sim.dist_enable()
        for who, call in calls(sim):
            assert text(sim, call) == who + WHOLE


@pytest.fixture(scope="module")
def scene(pkg, tmp_path_factory):
    """a packing through run_scene over two DEM events, with the clearance output on and without"""
    lx, ly = 61, 59
    r, x, y = shape_scene(lx, ly)
    with_dir, without_dir = tmp_path_factory.mktemp("with"), tmp_path_factory.mktemp("without")
    steps = 8000
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.run_scene(steps, str(without_dir))
        end = {what: getattr(sim, what) for what in ("f", "obst", "kinematics", "fhf")}
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.set_clearance_output(True, plane=True)
        _, res = sim.run_scene(steps, str(with_dir))
        for what in end:
            assert np.array_equal(getattr(sim, what), end[what]), what
        # the last event is the run's last sub-step: the restatement of the state the run ends in
        R = cz.restate(sim.obst, sim.n)
        t = sim.nbsteps * sim.config().dt
        n = sim.n
    return dict(lx=lx, ly=ly, r=r, x=x, y=y, n=n, with_dir=with_dir, without_dir=without_dir, steps=steps, R=R, t=t, nfile=res["nfile"])


NEW_FILES = ("throats%06d.dat", "clearance_hist%06d.dat", "clearance_owners%06d.dat", "clearance%06d.vtk")


def test_run_scene_with_the_clearance_output(pkg, scene, tmp_path):
    S = scene
    lx, ly, R, last = S["lx"], S["ly"], S["R"], S["nfile"]
    others = sorted(os.listdir(S["without_dir"]))
    numbers = sorted({int(name[3:9]) for name in others if name.startswith("DEM") and name.endswith(".dat")})
    assert last in numbers
    new = ["clearance.data"] + [p % k for k in numbers for p in NEW_FILES]
    assert sorted(os.listdir(S["with_dir"])) == sorted(others + new)
    for name in others:
        assert (S["with_dir"] / name).read_bytes() == (S["without_dir"] / name).read_bytes(), name
    # one line per DEM event, as stats.data has
    lines = (S["with_dir"] / "clearance.data").read_text().splitlines()
    events = len((S["with_dir"] / "stats.data").read_text().splitlines())
    assert lines[0] + "\n" == cz.DATA_HEADER and len(lines) == 1 + events and events == 2
    assert R["counts"]["fluid_nodes"] > 0 and len(R["table"]) >= 1
    pkg.write_clearance_files(str(tmp_path), last, lx, ly, R["table"], R["hist"], R["owned"], R["d2max"], R["counts"], S["t"],
                              d2=R["d2"], owner=R["owner"])
    want = cz.files_bytes(lx, ly, S["n"], R, S["t"], nfile=last, plane=True)
    assert lines[-1] + "\n" == want.pop("clearance.data").decode()
    for name, data in want.items():
        assert (S["with_dir"] / name).read_bytes() == data == (tmp_path / name).read_bytes(), name


def test_host_driver_writes_the_clearance_files(po, scene, tmp_path):
    """`lbmdem <sample> --steps N --clearance --clearance-plane` in a child process"""
    S = scene
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), S["r"] * 1e3, S["x"] * 1e3, S["y"] * 1e3)
    out = subprocess.run([EXE, str(sample), "--lx", str(S["lx"]), "--ly", str(S["ly"]), "--steps", str(S["steps"] + 1), "--clearance",
                          "--clearance-plane"], capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    names = [name for name in os.listdir(S["with_dir"]) if name.startswith(("throats", "clearance"))]
    assert "clearance.data" in names and len(names) >= 5
    for name in names:
        assert (tmp_path / name).read_bytes() == (S["with_dir"] / name).read_bytes(), name
    refused = subprocess.run([EXE, str(sample), "--clearance", "--gpus", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "--clearance is a single-GPU mode" in refused.stderr
