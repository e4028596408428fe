"""GPU: the pore network (lbmdem_network_compute and its readers, lbmdem_write_network, lbmdem_set_network_output;
include/lbmdem_hip.h) against the numpy restatement over obst (tests/network_util.py): every output by array_equal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import clearance_util as cz
import network_util as nu
from test_gpu_clearance import compare as compare_clearance
from test_gpu_pores import shape_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
WHOLE = " needs the whole lattice and all grains on this handle (not a strip of a decomposition, no distributed grains)"
NO_COMPUTE = "%s: no lbmdem_network_compute has been made for the map as it is now"
READERS = ("lbmdem_download_network", "lbmdem_network_device", "lbmdem_download_network_bodies", "lbmdem_download_network_groups",
           "lbmdem_download_network_links", "lbmdem_download_network_links")


def readers_of(sim):
    return (sim.network_planes, sim.network_tensors, sim.network_bodies, sim.network_groups, lambda: sim.network_links(0),
            sim.network_links)


def device(sim, counts):
    body, group = sim.network_planes()
    assert body.dtype == np.int32 and group.dtype == np.int32
    out = dict(counts=counts, body=body, group=group, bodies=sim.network_bodies(), groups=sim.network_groups(),
               links0=sim.network_links(0), links1=sim.network_links(1))
    assert out["bodies"].dtype == nu.NET_BODY_DTYPE and out["groups"].dtype == nu.NET_GROUP_DTYPE
    assert out["links0"].dtype == nu.NET_LINK_DTYPE and out["links1"].dtype == nu.NET_LINK_DTYPE
    return out


def check(sim, M=None, merge=-1, what="", max_edges=0):
    """one compute against the restatement, every output -> the restatement. M: a caller's map (None: the handle's)"""
    R = nu.restate(sim.obst if M is None else M, sim.n, merge)
    D = device(sim, sim.network(M, merge, max_edges))
    assert D["counts"] == R["counts"], (what, merge, D["counts"], R["counts"])
    assert nu.same(D, R) is None, (what, merge, sim.lx, sim.ly, nu.same(D, R))
    return R


@pytest.mark.parametrize("lx,ly", [(13, 61), (33, 62), (61, 59), (64, 64), (100, 63), (127, 121), (203, 122), (256, 200)])
def test_rasterised_packings(pkg, lx, ly):
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        for merge in (-1, 1):
            R = check(sim, merge=merge, what="rest")
        assert R["counts"]["fluid_nodes"] > 0 and R["counts"]["bodies"] >= 1
        sim.renderScene(2 * sim.cfg.npDEM + 1)
        for merge in (-1, 1):
            check(sim, merge=merge, what="stepped")


CALLER_SHAPES = [(65, 17), (17, 65), (127, 121), (121, 127)]


@pytest.mark.parametrize("lx,ly", CALLER_SHAPES)
def test_callers_maps(pkg, lx, ly):
    """every map of clearance_util.shape_maps; the second shape of a pair runs the first one's maps transposed: the seams of 16 and
    64 and the ragged last tile along either axis"""
    transposed = (lx, ly) in CALLER_SHAPES[1::2]
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        n = sim.n
        maps = cz.shape_maps(ly, lx, n) if transposed else cz.shape_maps(lx, ly, n)
        own = sim.obst
        for name, M in maps.items():
            M = np.ascontiguousarray(M.T) if transposed else M
            c = check(sim, M, merge=0, what=name)["counts"]
            if name == "all_fluid":
                assert c["bodies"] == 1
            if name == "checkerboard":
                assert c["groups"] == 1 and c["bodies"] > 1
            if name == "disc_packing" and (lx, ly) == (127, 121):
                assert c["bodies"] >= 2 and c["group_links"] >= 1
            if name == "no_fluid":
                assert c["narrowest_saddle"] == -1 and c["fluid_nodes"] == 0
                assert not len(sim.network_bodies()) and not len(sim.network_groups()) and not len(sim.network_links(0))
                assert not len(sim.network_links(1))
        # a caller's map leaves the handle's alone
        assert np.array_equal(sim.obst, own)
        check(sim, merge=0, what="own map after callers' maps")


def test_callers_maps_wider_than_any_tile(pkg):
    """257 x 513: chains and distances longer than any tile"""
    lx, ly = 257, 513
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        maps = cz.shape_maps(lx, ly, sim.n)
        for name in ("all_fluid", "sparse_seeds", "far_wall", "random_80", "disc_packing"):
            for merge in (-1, 3):
                c = check(sim, maps[name], merge=merge, what=name)["counts"]
            if name == "all_fluid":
                assert c["bodies"] == 1 and c["largest_group_nodes"] == lx * ly


def test_reuse_of_the_clearance_result(pkg):
    lx, ly = 100, 63
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim, pkg.LbmDem(lx, ly, r, x, y) as twin:
        Z = cz.restate(sim.obst, sim.n)
        zc = sim.clearance()
        R = check(sim, merge=1, what="after clearance()")          # (reuses the d2 plane)
        compare_clearance(sim, Z, zc, "the clearance result after network()")
        T = device(twin, twin.network(None, 1))                      # (no clearance() before)
        assert nu.same(T, R) is None
        compare_clearance(twin, Z, zc, "the clearance readers are valid after network()")
        # a clearance result of a caller's map is not taken for the handle's
        M = cz.shape_maps(lx, ly, sim.n)["comb"]
        sim.clearance(M)
        check(sim, merge=1, what="after clearance(map)")
        compare_clearance(sim, Z, zc, "network() computed the handle's clearance")
        check(sim, M, merge=1, what="a caller's map")
        compare_clearance(sim, cz.restate(M, sim.n), sim.clearance(M), "a caller's map: the clearance readers")
        assert np.array_equal(sim.obst, twin.obst)


def test_budget(pkg):
    lx, ly = 127, 121
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        M = cz.shape_maps(lx, ly, sim.n)["disc_packing"]
        R = check(sim, M, merge=1)
        edges = R["counts"]["body_edges"]
        assert edges > 10
        with pytest.raises(pkg.LbmDemError) as e:
            sim.network(M, 1, max_edges=edges - 1)
        assert e.value.code == -1
        text = sim._L.lbmdem_last_error().decode()
        assert text == "lbmdem_network_compute: the ridge has %d edges, max_edges is %d" % (edges, edges - 1), text
        for who, call in zip(READERS, readers_of(sim)):      # no result exists after a refused compute
            with pytest.raises(pkg.LbmDemError):
                call()
            assert sim._L.lbmdem_last_error().decode() == NO_COMPUTE % who
        check(sim, M, merge=1, what="the exact budget", max_edges=edges)
        for bad in (-1, 2 ** 31):
            with pytest.raises(pkg.LbmDemError):
                sim.network(M, 1, max_edges=bad)
            assert sim._L.lbmdem_last_error().decode() == "lbmdem_network_compute: max_edges must lie in 0 .. %d (%d)" % (2 ** 31 - 1, bad)


def test_map_validation_and_arguments(pkg):
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
                sim.network(M)
            assert e.value.code == -1
            text = sim._L.lbmdem_last_error().decode()
            assert text == ("lbmdem_network_compute: map[%d] = %d (node 40, 3) is neither -1 (fluid), a grain (0 .. %d) nor the wall "
                            "(%d)" % (40 * ly + 3, bad, n - 1, n)), text
            with pytest.raises(pkg.LbmDemError):      # no result exists after a refused compute
                sim.network_planes()
            assert sim._L.lbmdem_last_error().decode() == NO_COMPUTE % "lbmdem_download_network"
        with pytest.raises(pkg.LbmDemError):
            sim.network(np.zeros((ly, lx), np.int32))
        check(sim)
        with pytest.raises(pkg.LbmDemError) as e:
            sim.network(merge=-2)
        assert e.value.code == -1
        assert sim._L.lbmdem_last_error().decode() == ("lbmdem_network_compute: merge must be -1 (no merging) or a difference of "
                                                       "radii >= 0 (-2)")
        check(sim)
        with pytest.raises(pkg.LbmDemError) as e:
            sim.network_links(2)
        assert e.value.code == -1
        assert sim._L.lbmdem_last_error().decode() == ("lbmdem_download_network_links: level must be 0 (between bodies) or 1 "
                                                       "(between groups) (2)")
        with pytest.raises(pkg.LbmDemError):
            sim.set_network_output(True, merge=-2)
        assert sim._L.lbmdem_last_error().decode() == ("lbmdem_set_network_output: merge must be -1 (no merging) or a difference of "
                                                       "radii >= 0 (-2)")


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
        check(sim, merge=1)
        for call in readers_of(sim):                # reading does not invalidate
            call()
        sim.renderScene(sim.cfg.npDEM + 1); twin.renderScene(twin.cfg.npDEM + 1)
        refused()                                   # after coupled steps
        for what in ("f", "obst", "kinematics", "fhf"):      # ... which the compute has not disturbed
            assert np.array_equal(getattr(sim, what), getattr(twin, what)), what
        check(sim, merge=1)
        sim.dem_substep(); twin.dem_substep()
        refused()                                   # after a sub-step
        check(sim, merge=1)
        sim.lbm_step(); twin.lbm_step()
        refused()                                   # after a fluid step
        check(sim, merge=1)
        sim.kinematics = sim.kinematics; twin.kinematics = twin.kinematics
        refused()                                   # after an upload of kinematics
        sim.network(cz.shape_maps(lx, ly, sim.n)["comb"], 0)
        sim.renderScene(3); twin.renderScene(3)
        refused()
        for what in ("f", "obst", "kinematics", "fhf"):
            assert np.array_equal(getattr(sim, what), getattr(twin, what)), what


def test_sizing_and_device_views(pkg):
    lx, ly = 127, 121
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        M = cz.shape_maps(lx, ly, sim.n)["disc_packing"]
        R = check(sim, M, merge=1)
        L = pkg.load_library()
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        tables = (("lbmdem_download_network_bodies", "bodies", (), R["bodies"]), ("lbmdem_download_network_groups", "groups", (), R["groups"]),
                  ("lbmdem_download_network_links", "links", (0,), R["links0"]), ("lbmdem_download_network_links", "links", (1,), R["links1"]))
        for who, what, lead, want in tables:
            call = getattr(L, who)
            cnt = ctypes.c_long(-1)
            assert call(sim._h, *lead, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == len(want) > 3
            short, cnt.value = np.zeros(len(want) - 1, want.dtype), -1
            short["node"] = -7
            assert call(sim._h, *lead, vp(short), len(short), ctypes.byref(cnt)) == -1
            assert cnt.value == len(want) and (short["node"] == -7).all()
            assert L.lbmdem_last_error().decode() == "%s: there are %d %s, the buffer holds %d" % (who, len(want), what, len(short))
            roomy = np.zeros(len(want) + 3, want.dtype)
            roomy["node"] = -7
            assert call(sim._h, *lead, vp(roomy), len(roomy), ctypes.byref(cnt)) == 0
            assert np.array_equal(roomy[:cnt.value], want) and (roomy[cnt.value:]["node"] == -7).all()
            assert call(sim._h, *lead, None, 0, None) == -1
        # either plane may be NULL, not both
        only = np.full((lx, ly), -9, np.int32)
        assert L.lbmdem_download_network(sim._h, None, vp(only)) == 0 and np.array_equal(only, R["group"])
        assert L.lbmdem_download_network(sim._h, vp(only), None) == 0 and np.array_equal(only, R["body"])
        assert L.lbmdem_download_network(sim._h, None, None) == -1
        assert L.lbmdem_network_device(sim._h, None, None, None) == -1
        assert L.lbmdem_network_compute(sim._h, None, 0, 0, None) == -1
        # the torch views are the downloads; the planes are indexed through the row pitch, the pad columns hold -1
        pt = sim.network_tensors()
        sy = pt["body"].shape[1]
        assert pt["body"].is_cuda and pt["group"].is_cuda and pt["body"].shape == pt["group"].shape
        assert pt["body"].shape[0] == lx and sy > ly and sy % 16 == 0
        hb, hg = pt["body"].cpu().numpy(), pt["group"].cpu().numpy()
        assert np.array_equal(hb[:, :ly], R["body"]) and (hb[:, ly:] == -1).all()
        assert np.array_equal(hg[:, :ly], R["group"]) and (hg[:, ly:] == -1).all()
        assert int(pt["body"].reshape(-1)[5 * sy + 7]) == R["body"][5, 7]


def test_refusals(pkg, tmp_path):
    lx, ly = 64, 64
    r, x, y = shape_scene(lx, ly)
    calls = lambda s: ([("lbmdem_network_compute", s.network)] + list(zip(READERS, readers_of(s))) +
                       [("lbmdem_write_network", lambda: s.write_network(str(tmp_path), 0)),
                        ("lbmdem_set_network_output", lambda: s.set_network_output(True))])

    def text(sim, call):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1, e.value
        return sim._L.lbmdem_last_error().decode()
    if os.path.exists(pkg.SP_LIB_PATH):
        with pkg.LbmDem(lx, ly, r, x, y, precision="f32") as sp:
            for who, call in calls(sp):
                assert text(sp, call) == "the pore network analysis is not available in the single-precision build of the library", who
    with pkg.LbmDem(lx, ly, r, x, y, strip=(lx // 2, lx), halo=12) as strip:
        for who, call in calls(strip):
            assert text(strip, call) == who + WHOLE
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        missing = str(tmp_path / "missing")
        assert text(sim, lambda: sim.write_network(missing, 0)) == f"cannot open '{missing}/network_bodies000000.dat' for writing"
        assert os.listdir(tmp_path) == []
        sim.set_network_output(True, merge=1)
        assert text(sim, sim.dist_enable) == ("the pore network analysis is not available with distributed grains "
                                              "(lbmdem_set_network_output(h, 0, 0, 0) first)")
        sim.set_network_output(False)
        sim.dist_enable()
        for who, call in calls(sim):
            assert text(sim, call) == who + WHOLE


MERGE = 1


@pytest.fixture(scope="module")
def scene(pkg, tmp_path_factory):
    """a packing through run_scene over two DEM events, with the network output on and without"""
    lx, ly = 61, 59
    r, x, y = shape_scene(lx, ly)
    with_dir, without_dir = tmp_path_factory.mktemp("with"), tmp_path_factory.mktemp("without")
    steps = 8000
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.run_scene(steps, str(without_dir))
        end = {what: getattr(sim, what) for what in ("f", "obst", "kinematics", "fhf")}
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.set_network_output(True, merge=MERGE, plane=True)
        _, res = sim.run_scene(steps, str(with_dir))
        for what in end:
            assert np.array_equal(getattr(sim, what), end[what]), what
        # the last event is the run's last sub-step: the restatement of the state the run ends in
        R = nu.restate(sim.obst, sim.n, MERGE)
        t = sim.nbsteps * sim.config().dt
        n = sim.n
    return dict(lx=lx, ly=ly, r=r, x=x, y=y, n=n, with_dir=with_dir, without_dir=without_dir, steps=steps, R=R, t=t, nfile=res["nfile"])


NEW_FILES = ("network_bodies%06d.dat", "network_links%06d.dat", "network_groups%06d.dat", "network%06d.vtk")


def test_run_scene_with_the_network_output(pkg, scene, tmp_path):
    S = scene
    lx, ly, R, last = S["lx"], S["ly"], S["R"], S["nfile"]
    others = sorted(os.listdir(S["without_dir"]))
    numbers = sorted({int(name[3:9]) for name in others if name.startswith("DEM") and name.endswith(".dat")})
    assert last in numbers
    new = ["network.data"] + [p % k for k in numbers for p in NEW_FILES]
    assert sorted(os.listdir(S["with_dir"])) == sorted(others + new)
    for name in others:
        assert (S["with_dir"] / name).read_bytes() == (S["without_dir"] / name).read_bytes(), name
    lines = (S["with_dir"] / "network.data").read_text().splitlines()
    events = len((S["with_dir"] / "stats.data").read_text().splitlines())
    assert lines[0] + "\n" == nu.DATA_HEADER and len(lines) == 1 + events and events == 2
    assert R["counts"]["bodies"] >= 2 and len(R["links0"]) >= 1
    pkg.write_network_files(str(tmp_path), last, lx, ly, S["n"], MERGE, R["bodies"], R["groups"], R["links1"], R["counts"], S["t"],
                            body=R["body"], group=R["group"])
    want = nu.files_bytes(lx, ly, S["n"], MERGE, R, S["t"], nfile=last, plane=True)
    assert lines[-1] + "\n" == want.pop("network.data").decode()
    for name, data in want.items():
        assert (S["with_dir"] / name).read_bytes() == data == (tmp_path / name).read_bytes(), name


def test_host_driver_writes_the_network_files(po, scene, tmp_path):
    """`lbmdem <sample> --steps N --network 1 --network-plane` in a child process"""
    S = scene
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), S["r"] * 1e3, S["x"] * 1e3, S["y"] * 1e3)
    out = subprocess.run([EXE, str(sample), "--lx", str(S["lx"]), "--ly", str(S["ly"]), "--steps", str(S["steps"] + 1), "--network",
                          str(MERGE), "--network-plane"], capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    names = [name for name in os.listdir(S["with_dir"]) if name.startswith("network")]
    assert "network.data" in names and len(names) >= 5
    for name in names:
        assert (tmp_path / name).read_bytes() == (S["with_dir"] / name).read_bytes(), name
    refused = subprocess.run([EXE, str(sample), "--network", "--gpus", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "--network is a single-GPU mode" in refused.stderr
