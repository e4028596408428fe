"""GPU: geodesic (lbmdem_geodesic_compute and its readers, lbmdem_write_geodesic, lbmdem_set_geodesic_output;
include/lbmdem_hip.h) against the numpy restatement over obst (tests/geodesic_util.py): every integer by array_equal."""
import os
import subprocess

import numpy as np
import pytest

import clearance_util as cz
import drainage_util as du
import geodesic_util as gu
from test_gpu_pores import shape_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
WHOLE = " needs the whole lattice and all grains on this handle (not a strip of a decomposition, no distributed grains)"
NO_COMPUTE = "%s: no lbmdem_geodesic_compute has been made for the map as it is now"
NO_CLEARANCE = "%s: no lbmdem_clearance_compute has been made for the map as it is now"
READERS = ("lbmdem_download_geodesic", "lbmdem_geodesic_device", "lbmdem_download_geodesic_profile", "lbmdem_geodesic_rounds")
B, T, L, R = du.SIDE_B, du.SIDE_T, du.SIDE_L, du.SIDE_R
ALL = B | T | L | R


def readers_of(sim):
    return (sim.geodesic_planes, sim.geodesic_tensors, sim.geodesic_profile, sim.geodesic_rounds)


def device(sim, counts):
    out = dict(sim.geodesic_planes(), counts=counts, profile=sim.geodesic_profile())
    assert all(out[k].dtype == np.int32 for k in ("dist", "back", "detour")) and out["profile"].dtype == gu.LEVEL_DTYPE
    return out


def check(sim, frm, band, to=0, conn=8, min_d2=0, M=None, what="", max_edges=0):
    """one compute against the restatement, every output -> the restatement. M: a caller's map (None: the handle's)"""
    W = gu.restate(sim.obst if M is None else M, sim.n, frm, band, to, conn, min_d2)
    D = device(sim, sim.geodesic(frm, band, to, conn, min_d2, M, max_edges))
    print(what, (sim.lx, sim.ly), (frm, band, to, conn, min_d2), D["counts"], "rounds", sim.geodesic_rounds(), "sweeps", W["rounds"])
    assert D["counts"] == W["counts"], (what, frm, band, to, conn, min_d2, D["counts"], W["counts"])
    assert gu.same(D, W) is None, (what, frm, band, to, conn, min_d2, sim.lx, sim.ly, gu.same(D, W))
    fwd, bwd = sim.geodesic_rounds()
    assert (fwd >= 1) == (W["counts"]["inlet_nodes"] > 0) and (bwd >= 1) == (W["counts"]["outlet_nodes"] > 0)
    return W


CASES = ((T, 4, B, 8, 0), (L, 3, R, 4, 4), (ALL, 1, ALL, 8, 0))


@pytest.mark.parametrize("lx,ly", [(13, 61), (33, 62), (61, 59), (64, 64), (100, 63), (127, 121), (203, 122), (256, 200)])
def test_rasterised_packings(pkg, lx, ly):
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        W = [check(sim, *case, what="rest") for case in CASES]
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
        c = check(sim, T, 4, B, M=np.full((lx, ly), -1, np.int32), what="all fluid")
        assert c["counts"]["shortest"] == 215 and c["counts"]["reached_nodes"] == lx * ly
        M = du.two_pores(lx, ly)
        c = check(sim, B, 3, T, M=M, what="two pores")
        assert (c["dist"][:, ly // 2:] == -1).all() and c["counts"]["shortest"] == -1 and c["counts"]["outlet_nodes"] > 0
        assert c["counts"]["reached_nodes"] == (M[:, :ly // 2] == -1).sum() and (c["detour"] == -1).all()
        M = du.chamber_behind_neck(lx, ly)
        c = check(sim, B, 4, 0, 8, 0, M, "a chamber behind a neck")
        assert c["counts"]["reached_nodes"] == c["counts"]["fluid_nodes"]
        c = check(sim, B, 4, 0, 8, 2, M, "a chamber behind a neck a particle does not pass")
        assert (c["counts"]["reached_nodes"], c["counts"]["passable_nodes"]) == (139, 380)
        M = du.diagonal_passage(lx, ly)
        assert check(sim, B, 4, T, 4, 0, M, "a diagonal step, conn 4")["counts"]["shortest"] == -1
        assert check(sim, B, 4, T, 8, 0, M, "a diagonal step, conn 8")["counts"]["shortest"] == 217
        c = check(sim, B, 4, T, M=du.two_routes(lx, ly), what="two routes of equal width")
        assert (c["detour"][6:9, 10] == 0).all() and (c["detour"][lx - 11:lx - 8, 10] == 0).all()
        assert c["counts"]["path_nodes"] == (c["detour"] == 0).sum() > 2 * 3 * (ly - 14)
        M = np.full((lx, ly), -1, np.int32)
        M[:, ly - 5:] = n
        c = check(sim, T, 4, B, M=M, what="an inlet band without fluid")
        assert c["counts"]["inlet_nodes"] == 0 and c["counts"]["reached_nodes"] == 0 and c["counts"]["dist_max"] == -1
        assert all((c[k] == -1).all() for k in ("dist", "detour")) and (c["back"] >= 0).any() and sim.geodesic_rounds()[0] == 0
        c = check(sim, T, 4, 0, M=M, what="an inlet band without fluid, no outlet")
        assert all((c[k] == -1).all() for k in ("dist", "back", "detour")) and sim.geodesic_rounds() == (0, 0)
        M = du.random_discs(lx, ly, n, 5)
        for band in (max(lx, ly), 10 ** 6, 2 ** 31 - 1):
            c = check(sim, ALL, band, 0, M=M, what="a band larger than the lattice")
            assert (c["dist"][M == -1] == 0).all() and c["counts"]["dist_max"] == 0 and c["counts"]["shortest"] == -1
        c = check(sim, L, 3, 0, M=M, what="no outlet")
        assert (c["back"] == -1).all() and (c["detour"] == -1).all() and c["counts"]["outlet_nodes"] == 0
        c = check(sim, L, 3, L, M=M, what="from equal to to")
        assert c["counts"]["shortest"] == 0 and np.array_equal(c["dist"], c["back"])
        c1 = check(sim, L, 5, T, M=M, what="L to T")
        assert c1["counts"]["shortest"] == check(sim, T, 5, L, M=M, what="T to L")["counts"]["shortest"]
        # the torch views: the planes through the row pitch, the pad columns hold -1
        c2 = check(sim, T, 5, L, 4, 4, M, "T to L")
        views = sim.geodesic_tensors()
        for k, t in views.items():
            sy = t.shape[1]
            assert t.is_cuda and t.shape[0] == lx and sy > ly and sy % 16 == 0
            ht = t.cpu().numpy()
            assert np.array_equal(ht[:, :ly], c2[k]) and (ht[:, ly:] == -1).all(), k
            assert int(t.reshape(-1)[5 * sy + 7]) == c2[k][5, 7]
        c = check(sim, T, 4, B, M=np.full((lx, ly), n, np.int32), what="no fluid at all")
        assert c["counts"]["fluid_nodes"] == 0 and (c["dist"] == -1).all() and sim.geodesic_rounds() == (0, 0)
        assert np.array_equal(sim.obst, own)      # a caller's map leaves the handle's alone
        check(sim, T, 4, B, what="own map after callers' maps")


@pytest.mark.parametrize("name", ["comb", "serpentine"])
def test_long_paths(pkg, name):
    """paths that re-enter the same tiles many times and are longer than a tile sweeps in one launch"""
    lx, ly = (48, 50) if name == "comb" else (70, 200)
    M = gu.comb(lx, ly) if name == "comb" else du.serpentine(lx, ly)
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        c = check(sim, B, 4, T, M=M, what=name)
        assert c["counts"]["dist_max"] > 5 * 500 and c["counts"]["shortest"] > 5000 and sim.geodesic_rounds()[0] >= 2
        assert c["counts"]["reached_nodes"] == c["counts"]["passable_nodes"] and sim.geodesic_rounds()[1] >= 2
        check(sim, T, 4, B, 4, 0, M, name + ", from the other end")
        assert sim.geodesic_rounds()[0] >= 2
        check(sim, L, 3, R, M=M, what=name + ", from the side")
        if name == "comb":
            c = check(sim, B, 1, 0, M=M, what="comb, one corridor as inlet")
            assert c["counts"]["dist_max"] > 5 * 500 and c["counts"]["inlet_nodes"] == lx


def test_reuse_of_the_clearance_result(pkg):
    lx, ly = 100, 63
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim, pkg.LbmDem(lx, ly, r, x, y) as fresh:
        L_ = pkg.load_library()
        Cz = cz.restate(sim.obst, sim.n)
        counts = sim.clearance()
        assert counts == Cz["counts"]
        views = sim.clearance_tensors()
        kept = {k: v.clone() for k, v in views.items()}
        check(sim, T, 4, B, 8, 4, what="after clearance()")
        d2, owner = sim.clearance_planes()               # the readers are still valid and say the same
        assert np.array_equal(d2, Cz["d2"]) and np.array_equal(owner, Cz["owner"])
        assert all(bool((views[k] == kept[k]).all()) for k in kept)
        # min_d2 0 needs no clearance and makes none
        check(fresh, T, 4, B, 8, 0, what="a fresh handle")
        with pytest.raises(pkg.LbmDemError):
            fresh.clearance_planes()
        assert L_.lbmdem_last_error().decode() == NO_CLEARANCE % "lbmdem_download_clearance"
        check(fresh, T, 4, B, 8, 1, what="a fresh handle, min_d2 1")
        with pytest.raises(pkg.LbmDemError):
            fresh.clearance_planes()
        # a caller's map: a clearance of that map is made ...
        M = du.random_discs(lx, ly, sim.n, 3)
        check(sim, T, 4, B, 8, 4, M, "a caller's map")
        assert np.array_equal(sim.clearance_planes()[0], cz.restate(M, sim.n)["d2"])
        sim.geodesic_planes()
        # ... which is not taken for the handle's
        check(sim, T, 4, B, 8, 4, what="the handle's map after a caller's")
        assert np.array_equal(sim.clearance_planes()[0], Cz["d2"])
        # a later clearance() takes the d2 the result was made over away; a result made without it stays
        sim.clearance()
        with pytest.raises(pkg.LbmDemError):
            sim.geodesic_planes()
        assert L_.lbmdem_last_error().decode() == NO_COMPUTE % "lbmdem_download_geodesic"
        check(sim, T, 4, B, 8, 0)
        sim.clearance()
        sim.geodesic_planes()
        # the clearance's budget is passed through; a refused compute leaves no result
        edges = Cz["counts"]["ridge_edges"]
        assert edges > 10
        with pytest.raises(pkg.LbmDemError):
            sim.geodesic(T, 4, B, 8, 4, sim.obst, max_edges=edges - 1)
        assert L_.lbmdem_last_error().decode() == "lbmdem_clearance_compute: the ridge has %d edges, max_edges is %d" % (edges, edges - 1)
        with pytest.raises(pkg.LbmDemError):
            sim.geodesic_rounds()
        check(sim, T, 4, B, 8, 4, sim.obst, "the exact budget", max_edges=edges)


def test_readers_and_arguments(pkg):
    lx, ly = 127, 121
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim, pkg.LbmDem(lx, ly, r, x, y) as twin:
        Lb = pkg.load_library()

        def refused():
            for who, call in zip(READERS, readers_of(sim)):
                with pytest.raises(pkg.LbmDemError) as e:
                    call()
                assert e.value.code == -1
                assert sim._L.lbmdem_last_error().decode() == NO_COMPUTE % who
        refused()                                   # after create
        M = cz.shape_maps(lx, ly, sim.n)["disc_packing"]
        W = check(sim, T, 4, B, M=M)
        import ctypes
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        want, cnt = W["profile"], ctypes.c_long(-1)
        call = Lb.lbmdem_download_geodesic_profile
        assert call(sim._h, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == len(want) == ly
        short, cnt.value = np.zeros(len(want) - 1, want.dtype), -1
        short["dmin"] = -7
        assert call(sim._h, vp(short), len(short), ctypes.byref(cnt)) == -1
        assert cnt.value == len(want) and (short["dmin"] == -7).all()
        assert Lb.lbmdem_last_error().decode() == ("lbmdem_download_geodesic_profile: there are %d depths, the buffer holds %d"
                                                   % (len(want), len(short)))
        roomy = np.zeros(len(want) + 3, want.dtype)
        roomy["dmin"] = -7
        assert call(sim._h, vp(roomy), len(roomy), ctypes.byref(cnt)) == 0
        assert np.array_equal(roomy[:cnt.value], want) and (roomy["dmin"][cnt.value:] == -7).all()
        assert call(sim._h, None, 0, None) == -1
        assert Lb.lbmdem_geodesic_device(sim._h, None, None, None, None) == -1 and Lb.lbmdem_geodesic_rounds(sim._h, None, None) == -1
        assert Lb.lbmdem_geodesic_compute(sim._h, None, T, 1, 0, 8, 0, 0, None) == -1
        only = np.full((lx, ly), -9, np.int32)       # any pointer may be NULL
        assert Lb.lbmdem_download_geodesic(sim._h, None, None, vp(only)) == 0 and np.array_equal(only, W["detour"])
        assert Lb.lbmdem_download_geodesic(sim._h, None, None, None) == 0
        # arguments: every refusal's text, and a refused compute leaves no result
        text = lambda call: (pytest.raises(pkg.LbmDemError, call), sim._L.lbmdem_last_error().decode())[1]
        who = "lbmdem_geodesic_compute: "
        for bad in (0, 16, -1):
            assert text(lambda: sim.geodesic(bad)) == who + "from must be a mask of sides, B 1 | T 2 | L 4 | R 8, with at least one (%d)" % bad
        refused()
        for bad in (16, -1):
            assert text(lambda: sim.geodesic(T, 1, bad)) == who + ("to must be a mask of sides, B 1 | T 2 | L 4 | R 8, or 0 for no outlet "
                                                                  "(%d)" % bad)
        assert text(lambda: sim.geodesic(T, 0)) == who + "band must be at least 1 node (0)"
        for bad in (0, 6, 9):
            assert text(lambda: sim.geodesic(T, 1, 0, bad)) == who + "conn must be 4 or 8 (%d)" % bad
        assert text(lambda: sim.geodesic(T, 1, 0, 8, -1)) == who + "min_d2 must not be negative (-1)"
        for bad in (-1, 2 ** 31):
            assert text(lambda: sim.geodesic(T, 4, B, 8, 4, M, max_edges=bad)) == who + "max_edges must lie in 0 .. %d (%d)" % (2 ** 31 - 1, bad)
        assert text(lambda: sim.set_geodesic_output(True, T, 0)) == "lbmdem_set_geodesic_output: band must be at least 1 node (0)"
        assert text(lambda: sim.set_geodesic_output(True, T, 1, 0, 5)) == "lbmdem_set_geodesic_output: conn must be 4 or 8 (5)"
        bad = M.copy()
        bad[40, 3] = sim.n + 1
        assert text(lambda: sim.geodesic(T, 1, 0, 8, 0, bad)) == who + ("map[%d] = %d (node 40, 3) is neither -1 (fluid), a grain "
                                                                        "(0 .. %d) nor the wall (%d)" % (40 * ly + 3, sim.n + 1, sim.n - 1, sim.n))
        with pytest.raises(pkg.LbmDemError):
            sim.geodesic(T, 1, 0, 8, 0, np.zeros((ly, lx), np.int32))
        refused()
        # seeds that end exactly at a tile's border (64 along y, 16 along x): the tile behind it has to be woken by the first round
        fluid = np.full((lx, ly), -1, np.int32)
        for frm, band, to in ((B, 64, T), (T, ly - 64, B), (L, 16, R), (L, 32, 0), (ALL, 16, 0)):
            c = check(sim, frm, band, to, M=fluid, what="a band that ends at a tile's border")
            assert c["counts"]["reached_nodes"] == lx * ly
        # steps invalidate, and the computes have disturbed nothing
        check(sim, T, 4, B)
        for call in readers_of(sim):                # reading does not invalidate
            call()
        sim.renderScene(sim.cfg.npDEM + 1); twin.renderScene(twin.cfg.npDEM + 1)
        refused()                                   # after coupled steps
        check(sim, L, 3, R, 4, 4)
        sim.dem_substep(); twin.dem_substep()
        refused()                                   # after a sub-step
        check(sim, L, 3, R)
        sim.lbm_step(); twin.lbm_step()
        refused()                                   # after a fluid step
        sim.geodesic(T, 2, B, 8, 0, M)
        sim.renderScene(3); twin.renderScene(3)
        refused()
        for what in ("f", "obst", "kinematics", "fhf"):
            assert np.array_equal(getattr(sim, what), getattr(twin, what)), what


def test_refusals(pkg, tmp_path):
    lx, ly = 64, 64
    r, x, y = shape_scene(lx, ly)
    calls = lambda s: ([("lbmdem_geodesic_compute", lambda: s.geodesic(T))] + list(zip(READERS, readers_of(s))) +
                       [("lbmdem_write_geodesic", lambda: s.write_geodesic(str(tmp_path), 0)),
                        ("lbmdem_set_geodesic_output", lambda: s.set_geodesic_output(True))])

    def text(sim, call):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1, e.value
        return sim._L.lbmdem_last_error().decode()
    assert os.path.exists(pkg.SP_LIB_PATH)
    with pkg.LbmDem(lx, ly, r, x, y, precision="f32") as sp:
        for who, call in calls(sp):
            assert text(sp, call) == "the geodesic analysis is not available in the single-precision build of the library", who
    with pkg.LbmDem(lx, ly, r, x, y, strip=(lx // 2, lx), halo=12) as strip:
        for who, call in calls(strip):
            assert text(strip, call) == who + WHOLE
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        missing = str(tmp_path / "missing")
        assert text(sim, lambda: sim.write_geodesic(missing, 0)) == f"cannot open '{missing}/geodesic_profile000000.dat' for writing"
        assert os.listdir(tmp_path) == []
        sim.set_geodesic_output(True, T, 2, B)
        assert text(sim, sim.dist_enable) == ("the geodesic analysis is not available with distributed grains "
                                              "(lbmdem_set_geodesic_output(h, 0, 0, 0, 0, 0, 0, 0) first)")
        sim.set_geodesic_output(False)
        sim.dist_enable()
        for who, call in calls(sim):
            assert text(sim, call) == who + WHOLE


BAND = 3          # (the lattice's edge nodes are wall: a region one node deep holds no fluid)


@pytest.fixture(scope="module")
def scene(pkg, tmp_path_factory):
    """a packing through run_scene over two DEM events, with the geodesic output on and without"""
    lx, ly = 61, 59
    r, x, y = shape_scene(lx, ly)
    with_dir, without_dir = tmp_path_factory.mktemp("with"), tmp_path_factory.mktemp("without")
    steps = 8000
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.run_scene(steps, str(without_dir))
        end = {what: getattr(sim, what) for what in ("f", "obst", "kinematics", "fhf")}
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.set_geodesic_output(True, T, BAND, B, 8, 2, plane=True)
        _, res = sim.run_scene(steps, str(with_dir))
        for what in end:
            assert np.array_equal(getattr(sim, what), end[what]), what
        # the last event is the run's last sub-step: the restatement of the state the run ends in
        W = gu.restate(sim.obst, sim.n, T, BAND, B, 8, 2)
        t = sim.nbsteps * sim.config().dt
        n = sim.n
    return dict(lx=lx, ly=ly, r=r, x=x, y=y, n=n, with_dir=with_dir, without_dir=without_dir, steps=steps, W=W, t=t, nfile=res["nfile"])


NEW_FILES = ("geodesic_profile%06d.dat", "geodesic%06d.vtk")


def test_run_scene_with_the_geodesic_output(pkg, scene, tmp_path):
    S = scene
    lx, ly, W, last = S["lx"], S["ly"], S["W"], S["nfile"]
    others = sorted(os.listdir(S["without_dir"]))
    numbers = sorted({int(name[3:9]) for name in others if name.startswith("DEM") and name.endswith(".dat")})
    assert last in numbers
    new = ["geodesic.data"] + [p % k for k in numbers for p in NEW_FILES]
    assert sorted(os.listdir(S["with_dir"])) == sorted(others + new)
    for name in others:
        assert (S["with_dir"] / name).read_bytes() == (S["without_dir"] / name).read_bytes(), name
    lines = (S["with_dir"] / "geodesic.data").read_text().splitlines()
    events = len((S["with_dir"] / "stats.data").read_text().splitlines())
    assert lines[0] + "\n" == gu.DATA_HEADER and len(lines) == 1 + events and events == 2
    assert W["counts"]["reached_nodes"] > 0
    pkg.write_geodesic_files(str(tmp_path), last, lx, ly, S["n"], T, BAND, B, 8, 2, W["profile"], W["counts"], S["t"],
                             planes=(W["dist"], W["back"], W["detour"]))
    want = gu.files_bytes(lx, ly, S["n"], T, BAND, B, 8, 2, W, S["t"], nfile=last, plane=True)
    assert lines[-1] + "\n" == want.pop("geodesic.data").decode()
    for name, data in want.items():
        assert (S["with_dir"] / name).read_bytes() == data == (tmp_path / name).read_bytes(), name


def test_host_driver_writes_the_geodesic_files(po, scene, tmp_path):
    """`lbmdem <sample> --steps N --geodesic T --geodesic-to B --geodesic-band 3 --geodesic-min-d2 2 --geodesic-plane` in a child
    process"""
    S = scene
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), S["r"] * 1e3, S["x"] * 1e3, S["y"] * 1e3)
    out = subprocess.run([EXE, str(sample), "--lx", str(S["lx"]), "--ly", str(S["ly"]), "--steps", str(S["steps"] + 1), "--geodesic", "T",
                          "--geodesic-to", "B", "--geodesic-band", str(BAND), "--geodesic-conn", "8", "--geodesic-min-d2", "2",
                          "--geodesic-plane"], capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    names = [name for name in os.listdir(S["with_dir"]) if name.startswith("geodesic")]
    assert "geodesic.data" in names and len(names) >= 3
    for name in names:
        assert (tmp_path / name).read_bytes() == (S["with_dir"] / name).read_bytes(), name
    refused = subprocess.run([EXE, str(sample), "--geodesic", "T", "--gpus", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "--geodesic is a single-GPU mode" in refused.stderr
    refused = subprocess.run([EXE, str(sample), "--geodesic", "X"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "letters out of BTLR" in refused.stderr
    refused = subprocess.run([EXE, str(sample), "--geodesic-conn", "8"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "need --geodesic FROM" in refused.stderr
    refused = subprocess.run([EXE, str(sample), "--geodesic", "T", "--geodesic-conn", "6"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "--geodesic-conn 4|8" in refused.stderr
