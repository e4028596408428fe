"""GPU: drainage (lbmdem_drainage_compute and its readers, lbmdem_write_drainage, lbmdem_set_drainage_output;
include/lbmdem_hip.h) against the numpy restatement over obst (tests/drainage_util.py): every integer by array_equal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import clearance_util as cz
import drainage_util as du
import network_util as nu
from test_gpu_network import device as network_device
from test_gpu_pores import shape_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
WHOLE = " needs the whole lattice and all grains on this handle (not a strip of a decomposition, no distributed grains)"
NO_COMPUTE = "%s: no lbmdem_drainage_compute has been made for the map as it is now"
READERS = ("lbmdem_download_drainage", "lbmdem_drainage_device", "lbmdem_download_drainage_bodies", "lbmdem_download_drainage_links",
           "lbmdem_download_drainage_hist", "lbmdem_drainage_rounds")
B, T, L, R = du.SIDE_B, du.SIDE_T, du.SIDE_L, du.SIDE_R


def readers_of(sim):
    return (sim.drainage_plane, sim.drainage_tensor, sim.drainage_bodies, sim.drainage_links, sim.drainage_hist, sim.drainage_rounds)


def device(sim, counts):
    out = dict(counts=counts, access=sim.drainage_plane(), A=sim.drainage_bodies(), passes=sim.drainage_links(), hist=sim.drainage_hist())
    assert out["access"].dtype == np.int32 and out["A"].dtype == np.int32 and out["passes"].dtype == np.int32
    assert out["hist"].dtype == np.int64
    return out


def check(sim, frm, band, to, M=None, what="", N=None, max_edges=0):
    """one compute against the restatement, every output -> the restatement. M: a caller's map (None: the handle's)"""
    W = du.restate(sim.obst if M is None else M, sim.n, frm, band, to, N=N)
    D = device(sim, sim.drainage(frm, band, to, M, max_edges))
    assert D["counts"] == W["counts"], (what, frm, band, to, D["counts"], W["counts"])
    assert du.same(D, W) is None, (what, frm, band, to, sim.lx, sim.ly, du.same(D, W))
    assert sim.drainage_rounds() >= (1 if len(W["passes"]) else 0)
    return W


CASES = ((T, 4, B), (L, 3, R), (B | T | L | R, 1, B | T | L | R))


@pytest.mark.parametrize("lx,ly", [(13, 61), (33, 62), (61, 59), (64, 64), (100, 63), (127, 121), (203, 122), (256, 200)])
def test_rasterised_packings(pkg, lx, ly):
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        N = nu.restate(sim.obst, sim.n, -1)
        W = [check(sim, frm, band, to, what="rest", N=N) for frm, band, to in CASES]
        # (the lattice's edge nodes are wall: a band of 1 holds no fluid, and that is a case too)
        assert W[0]["counts"]["fluid_nodes"] > 0 and max(w["counts"]["reached_nodes"] for w in W) > 0
        sim.renderScene(2 * sim.cfg.npDEM + 1)
        check(sim, T, 4, B, what="stepped")


def test_callers_maps(pkg):
    """maps chosen for what can go wrong, on a lattice whose ly is no multiple of the row pitch"""
    lx, ly = 48, 50
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        n, own = sim.n, sim.obst
        c = check(sim, T, 4, B, np.full((lx, ly), -1, np.int32), "all fluid")
        assert len(c["A"]) == 1 and c["counts"]["reached_nodes"] == lx * ly
        M = du.two_pores(lx, ly)
        c = check(sim, B, 3, T, M, "two pores")
        assert (c["access"][:, ly // 2:] == 0).all() and c["hist"][0] == (M[:, ly // 2:] == -1).sum() > 0
        assert c["counts"]["critical"] == 0 and c["counts"]["critical_node"] == -1 and c["counts"]["outlet_nodes"] > 0
        M = du.chamber_behind_neck(lx, ly)
        c = check(sim, B, 4, 0, M, "a chamber behind a neck")
        assert (c["access"][lx // 2 - 8:lx // 2 + 9, 11:29] == 1).all() and c["counts"]["shielded_nodes"] >= 17 * 18 - 100
        assert c["network"]["d2"][lx // 2, 20] > 1
        M = du.diagonal_passage(lx, ly)
        c = check(sim, B, 4, T, M, "a diagonal step")
        assert c["counts"]["critical"] == 1 and c["counts"]["front_links"] >= 1
        c = check(sim, B, 4, T, du.two_routes(lx, ly), "two routes of equal width")
        assert c["counts"]["critical"] == 4 and c["counts"]["front_links"] == 2
        M = np.full((lx, ly), -1, np.int32)
        M[:, ly - 5:] = n
        c = check(sim, T, 4, B, M, "an inlet band without fluid")
        assert c["counts"]["inlet_nodes"] == 0 and c["counts"]["reached_nodes"] == 0 and c["counts"]["critical"] == 0
        assert c["hist"][0] == c["counts"]["fluid_nodes"] > 0 and not c["access"].any()
        M = du.random_discs(lx, ly, n, 5)
        for band in (max(lx, ly), 10 ** 6, 2 ** 31 - 1):
            c = check(sim, B | T | L | R, band, 0, M, "a band larger than the lattice")
            assert np.array_equal(c["access"], c["network"]["d2"]) and c["counts"]["critical"] == -1
        check(sim, L, 3, L, M, "from equal to to")
        c1, c2 = check(sim, L, 5, T, M, "L to T"), check(sim, T, 5, L, M, "T to L")
        assert c1["counts"]["critical"] == c2["counts"]["critical"]
        # the torch view: the plane through the row pitch, the pad columns hold 0
        t = sim.drainage_tensor()
        sy = t.shape[1]
        assert t.is_cuda and t.shape[0] == lx and sy > ly and sy % 16 == 0
        ht = t.cpu().numpy()
        assert np.array_equal(ht[:, :ly], c2["access"]) and (ht[:, ly:] == 0).all()
        assert int(t.reshape(-1)[5 * sy + 7]) == c2["access"][5, 7]
        assert np.array_equal(sim.obst, own)      # a caller's map leaves the handle's alone
        check(sim, T, 4, B, what="own map after callers' maps")


def test_serpentine(pkg):
    """bodies in series over more links than one workgroup holds: the relaxation crosses chunks"""
    lx, ly = 70, 200
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        M = du.serpentine(lx, ly)
        c = check(sim, B, 4, T, M, "serpentine")
        assert len(c["passes"]) > 256 and c["rounds"] > 100 and c["counts"]["critical"] >= 1
        assert c["counts"]["reached_nodes"] == c["counts"]["fluid_nodes"] and sim.drainage_rounds() >= 1
        check(sim, T, 4, B, M, "serpentine, from the other end")
        check(sim, L, 3, R, M, "serpentine, from the side")


def test_reuse_of_the_network_result(pkg):
    lx, ly = 100, 63
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        L_ = pkg.load_library()
        Nm = nu.restate(sim.obst, sim.n, 1)
        before = network_device(sim, sim.network(None, 1))
        assert nu.same(before, Nm) is None
        planes = sim.network_tensors()
        kept = {k: v.clone() for k, v in planes.items()}
        check(sim, T, 4, B, what="after network(merge=1)")
        after = network_device(sim, before["counts"])          # the readers are still valid and say the same: merge 1's groups
        assert nu.same(after, Nm) is None and after["counts"]["groups"] < after["counts"]["bodies"]
        assert all(bool((planes[k] == kept[k]).all()) for k in kept)
        # a caller's map: a network of that map is made, merge -1
        M = du.random_discs(lx, ly, sim.n, 3)
        check(sim, T, 4, B, M, "a caller's map")
        made = network_device(sim, nu.restate(M, sim.n, -1)["counts"])
        assert nu.same(made, nu.restate(M, sim.n, -1)) is None
        # ... which is not taken for the handle's
        check(sim, T, 4, B, what="the handle's map after a caller's")
        assert nu.same(network_device(sim, nu.restate(sim.obst, sim.n, -1)["counts"]), nu.restate(sim.obst, sim.n, -1)) is None
        # a later network() takes the tables A and pass are aligned with away
        sim.network(None, 0)
        with pytest.raises(pkg.LbmDemError):
            sim.drainage_bodies()
        assert L_.lbmdem_last_error().decode() == NO_COMPUTE % "lbmdem_download_drainage_bodies"


def test_readers_sizing_and_budget(pkg):
    lx, ly = 127, 121
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim, pkg.LbmDem(lx, ly, r, x, y) as twin:
        def refused():
            for who, call in zip(READERS, readers_of(sim)):
                with pytest.raises(pkg.LbmDemError) as e:
                    call()
                assert e.value.code == -1
                assert sim._L.lbmdem_last_error().decode() == NO_COMPUTE % who
        refused()                                   # after create
        M = cz.shape_maps(lx, ly, sim.n)["disc_packing"]
        W = check(sim, T, 4, B, M)
        Lb = pkg.load_library()
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        for who, what, want in (("lbmdem_download_drainage_bodies", "bodies", W["A"]), ("lbmdem_download_drainage_links", "links", W["passes"]),
                                ("lbmdem_download_drainage_hist", "bins", W["hist"])):
            call = getattr(Lb, who)
            cnt = ctypes.c_long(-1)
            assert call(sim._h, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == len(want) > 3
            short, cnt.value = np.full(len(want) - 1, -7, want.dtype), -1
            assert call(sim._h, vp(short), len(short), ctypes.byref(cnt)) == -1
            assert cnt.value == len(want) and (short == -7).all()
            assert Lb.lbmdem_last_error().decode() == "%s: there are %d %s, the buffer holds %d" % (who, len(want), what, len(short))
            roomy = np.full(len(want) + 3, -7, want.dtype)
            assert call(sim._h, vp(roomy), len(roomy), ctypes.byref(cnt)) == 0
            assert np.array_equal(roomy[:cnt.value], want) and (roomy[cnt.value:] == -7).all()
            assert call(sim._h, None, 0, None) == -1
        assert np.array_equal(sim.drainage_hist().shape, sim.clearance_hist().shape)
        assert Lb.lbmdem_download_drainage(sim._h, None) == -1 and Lb.lbmdem_drainage_device(sim._h, None, None) == -1
        assert Lb.lbmdem_drainage_rounds(sim._h, None) == -1 and Lb.lbmdem_drainage_compute(sim._h, None, T, 1, 0, 0, None) == -1
        # the budget is the network's; a refused compute leaves no drainage result
        edges = W["network"]["counts"]["body_edges"]
        assert edges > 10
        with pytest.raises(pkg.LbmDemError) as e:
            sim.drainage(T, 4, B, M, max_edges=edges - 1)
        assert e.value.code == -1
        assert sim._L.lbmdem_last_error().decode() == "lbmdem_network_compute: the ridge has %d edges, max_edges is %d" % (edges, edges - 1)
        refused()
        check(sim, T, 4, B, M, "the exact budget", max_edges=edges)
        for bad in (-1, 2 ** 31):
            with pytest.raises(pkg.LbmDemError):
                sim.drainage(T, 4, B, M, max_edges=bad)
            assert sim._L.lbmdem_last_error().decode() == "lbmdem_drainage_compute: max_edges must lie in 0 .. %d (%d)" % (2 ** 31 - 1, bad)
        refused()
        # arguments
        text = lambda call: (pytest.raises(pkg.LbmDemError, call), sim._L.lbmdem_last_error().decode())[1]
        for bad in (0, 16, -1):
            assert text(lambda: sim.drainage(bad)) == ("lbmdem_drainage_compute: from must be a mask of sides, B 1 | T 2 | L 4 | R 8, "
                                                       "with at least one (%d)" % bad)
        for bad in (16, -1):
            assert text(lambda: sim.drainage(T, 1, bad)) == ("lbmdem_drainage_compute: to must be a mask of sides, B 1 | T 2 | L 4 | R 8, "
                                                             "or 0 for no outlet (%d)" % bad)
        assert text(lambda: sim.drainage(T, 0)) == "lbmdem_drainage_compute: band must be at least 1 node (0)"
        assert text(lambda: sim.set_drainage_output(True, T, 0)) == "lbmdem_set_drainage_output: band must be at least 1 node (0)"
        bad = M.copy()
        bad[40, 3] = sim.n + 1
        assert text(lambda: sim.drainage(T, 1, 0, bad)) == ("lbmdem_drainage_compute: map[%d] = %d (node 40, 3) is neither -1 (fluid), a grain "
                                                            "(0 .. %d) nor the wall (%d)" % (40 * ly + 3, sim.n + 1, sim.n - 1, sim.n))
        with pytest.raises(pkg.LbmDemError):
            sim.drainage(T, 1, 0, np.zeros((ly, lx), np.int32))
        refused()
        # steps invalidate, and the computes have disturbed nothing
        check(sim, T, 4, B)
        for call in readers_of(sim):                # reading does not invalidate
            call()
        sim.renderScene(sim.cfg.npDEM + 1); twin.renderScene(twin.cfg.npDEM + 1)
        refused()                                   # after coupled steps
        check(sim, L, 3, R)
        sim.dem_substep(); twin.dem_substep()
        refused()                                   # after a sub-step
        check(sim, L, 3, R)
        sim.lbm_step(); twin.lbm_step()
        refused()                                   # after a fluid step
        sim.drainage(T, 2, B, M)
        sim.renderScene(3); twin.renderScene(3)
        refused()
        for what in ("f", "obst", "kinematics", "fhf"):
            assert np.array_equal(getattr(sim, what), getattr(twin, what)), what


def test_refusals(pkg, tmp_path):
    lx, ly = 64, 64
    r, x, y = shape_scene(lx, ly)
    calls = lambda s: ([("lbmdem_drainage_compute", lambda: s.drainage(T))] + list(zip(READERS, readers_of(s))) +
                       [("lbmdem_write_drainage", lambda: s.write_drainage(str(tmp_path), 0)),
                        ("lbmdem_set_drainage_output", lambda: s.set_drainage_output(True))])

    def text(sim, call):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1, e.value
        return sim._L.lbmdem_last_error().decode()
    if os.path.exists(pkg.SP_LIB_PATH):
        with pkg.LbmDem(lx, ly, r, x, y, precision="f32") as sp:
            for who, call in calls(sp):
                assert text(sp, call) == "the drainage analysis is not available in the single-precision build of the library", who
    with pkg.LbmDem(lx, ly, r, x, y, strip=(lx // 2, lx), halo=12) as strip:
        for who, call in calls(strip):
            assert text(strip, call) == who + WHOLE
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        missing = str(tmp_path / "missing")
        assert text(sim, lambda: sim.write_drainage(missing, 0)) == f"cannot open '{missing}/drainage_curve000000.dat' for writing"
        assert os.listdir(tmp_path) == []
        sim.set_drainage_output(True, T, 2, B)
        assert text(sim, sim.dist_enable) == ("the drainage analysis is not available with distributed grains "
                                              "(lbmdem_set_drainage_output(h, 0, 0, 0, 0, 0) first)")
        sim.set_drainage_output(False)
        sim.dist_enable()
        for who, call in calls(sim):
            assert text(sim, call) == who + WHOLE


BAND = 3          # (the lattice's edge nodes are wall: a reservoir one node deep holds no fluid)


@pytest.fixture(scope="module")
def scene(pkg, tmp_path_factory):
    """a packing through run_scene over two DEM events, with the drainage output on and without"""
    lx, ly = 61, 59
    r, x, y = shape_scene(lx, ly)
    with_dir, without_dir = tmp_path_factory.mktemp("with"), tmp_path_factory.mktemp("without")
    steps = 8000
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.run_scene(steps, str(without_dir))
        end = {what: getattr(sim, what) for what in ("f", "obst", "kinematics", "fhf")}
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.set_drainage_output(True, T, BAND, B, plane=True)
        _, res = sim.run_scene(steps, str(with_dir))
        for what in end:
            assert np.array_equal(getattr(sim, what), end[what]), what
        # the last event is the run's last sub-step: the restatement of the state the run ends in
        W = du.restate(sim.obst, sim.n, T, BAND, B)
        chist = cz.restate(sim.obst, sim.n)["hist"]
        t = sim.nbsteps * sim.config().dt
        n = sim.n
    return dict(lx=lx, ly=ly, r=r, x=x, y=y, n=n, with_dir=with_dir, without_dir=without_dir, steps=steps, W=W, chist=chist, t=t,
                nfile=res["nfile"])


NEW_FILES = ("drainage_curve%06d.dat", "drainage_bodies%06d.dat", "drainage%06d.vtk")


def test_run_scene_with_the_drainage_output(pkg, scene, tmp_path):
    S = scene
    lx, ly, W, last = S["lx"], S["ly"], S["W"], S["nfile"]
    others = sorted(os.listdir(S["without_dir"]))
    numbers = sorted({int(name[3:9]) for name in others if name.startswith("DEM") and name.endswith(".dat")})
    assert last in numbers
    new = ["drainage.data"] + [p % k for k in numbers for p in NEW_FILES]
    assert sorted(os.listdir(S["with_dir"])) == sorted(others + new)
    for name in others:
        assert (S["with_dir"] / name).read_bytes() == (S["without_dir"] / name).read_bytes(), name
    lines = (S["with_dir"] / "drainage.data").read_text().splitlines()
    events = len((S["with_dir"] / "stats.data").read_text().splitlines())
    assert lines[0] + "\n" == du.DATA_HEADER and len(lines) == 1 + events and events == 2
    assert W["counts"]["reached_nodes"] > 0 and len(W["A"]) >= 2
    pkg.write_drainage_files(str(tmp_path), last, lx, ly, S["n"], T, BAND, B, W["network"]["bodies"], W["A"], W["hist"], S["chist"],
                             W["counts"], S["t"], access=W["access"])
    want = du.files_bytes(lx, ly, S["n"], T, BAND, B, W, S["chist"], S["t"], nfile=last, plane=True)
    assert lines[-1] + "\n" == want.pop("drainage.data").decode()
    for name, data in want.items():
        assert (S["with_dir"] / name).read_bytes() == data == (tmp_path / name).read_bytes(), name


def test_host_driver_writes_the_drainage_files(po, scene, tmp_path):
    """`lbmdem <sample> --steps N --drainage T --drainage-to B --drainage-band 3 --drainage-plane` in a child process"""
    S = scene
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), S["r"] * 1e3, S["x"] * 1e3, S["y"] * 1e3)
    out = subprocess.run([EXE, str(sample), "--lx", str(S["lx"]), "--ly", str(S["ly"]), "--steps", str(S["steps"] + 1), "--drainage", "T",
                          "--drainage-to", "B", "--drainage-band", str(BAND), "--drainage-plane"], capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    names = [name for name in os.listdir(S["with_dir"]) if name.startswith("drainage")]
    assert "drainage.data" in names and len(names) >= 4
    for name in names:
        assert (tmp_path / name).read_bytes() == (S["with_dir"] / name).read_bytes(), name
    refused = subprocess.run([EXE, str(sample), "--drainage", "T", "--gpus", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "--drainage is a single-GPU mode" in refused.stderr
    refused = subprocess.run([EXE, str(sample), "--drainage", "X"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "letters out of BTLR" in refused.stderr
