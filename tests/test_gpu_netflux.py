"""GPU: the pore fluxes (lbmdem_netflux_compute and its readers, lbmdem_write_netflux, lbmdem_set_netflux_output;
include/lbmdem_hip.h) against the numpy restatement over obst and f (tests/netflux_util.py): every integer by array_equal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import drainage_util as du
import netflux_util as fu
import network_util as nu
from test_gpu_network import device as network_device
from test_gpu_pores import shape_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
WHOLE = " needs the whole lattice and all grains on this handle (not a strip of a decomposition, no distributed grains)"
NO_COMPUTE = "%s: no lbmdem_netflux_compute has been made for the map and populations as they are now"
READERS = ("lbmdem_download_netflux_links", "lbmdem_download_netflux_regions", "lbmdem_download_netflux_profile")


def readers_of(sim):
    return (sim.netflux_links, sim.netflux_regions, sim.netflux_profile)


def random_f(lx, ly, seed):
    return np.random.default_rng(seed).uniform(0.01, 0.5, (lx, ly, 9))


def device(sim, counts):
    col, row = sim.netflux_profile()
    out = dict(counts=counts, links=sim.netflux_links(), regions=sim.netflux_regions(), col=col, row=row)
    assert out["links"].dtype == fu.NETFLUX_LINK_DTYPE and out["regions"].dtype == fu.NETFLUX_REGION_DTYPE
    assert col.dtype == np.int64 and row.dtype == np.int64 and len(col) == sim.lx - 1 and len(row) == sim.ly - 1
    return out


def check(sim, merge, level, M=None, what="", N=None, f=None):
    """one compute against the restatement, every output -> the restatement. M: a caller's map (None: the handle's)"""
    W = fu.restate(sim.obst if M is None else M, sim.f if f is None else f, sim.n, merge, level, N=N)
    D = device(sim, sim.netflux(merge, level, M))
    assert D["counts"] == W["counts"], (what, merge, level, D["counts"], W["counts"])
    assert fu.same(D, W) is None, (what, merge, level, sim.lx, sim.ly, fu.same(D, W))
    return W


def at_rest(W):
    c = W["counts"]
    return not (W["col"].any() or W["row"].any() or W["links"]["flux_q32"].any() or W["links"]["exchange_q32"].any() or
                W["regions"]["net_q32"].any() or W["regions"]["through_q32"].any() or c["flowing_links"] or c["largest_imbalance"])


CASES = ((-1, 0), (-1, 1), (1, 0), (1, 1))


@pytest.mark.parametrize("lx,ly", [(13, 61), (33, 62), (61, 59), (64, 64), (100, 63), (127, 121), (203, 122), (256, 200)])
def test_rasterised_packings(pkg, lx, ly):
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        Ns = {m: nu.restate(sim.obst, sim.n, m) for m in (-1, 1)}
        f = sim.f
        for merge, level in CASES:
            W = check(sim, merge, level, what="rest", N=Ns[merge], f=f)
            assert at_rest(W), (merge, level)          # a fluid at rest: every flux is 0
            assert W["counts"]["fluid_nodes"] > 0 and W["counts"]["edges"] > 0 and W["regions"]["mass_q32"].all()
        sim.renderScene(2 * sim.cfg.npDEM + 1)
        Ns = {m: nu.restate(sim.obst, sim.n, m) for m in (-1, 1)}
        f = sim.f
        for merge, level in CASES:
            check(sim, merge, level, what="stepped", N=Ns[merge], f=f)
        f = random_f(lx, ly, lx + ly)
        sim.f = f
        for merge, level in CASES:
            W = check(sim, merge, level, what="random f", N=Ns[merge], f=f)
            # (the lattice's edge nodes are wall: the outermost sections carry nothing)
            assert W["counts"]["flowing_links"] == W["counts"]["links"] and W["col"][1:-1].all() and W["row"][1:-1].all()
            assert not W["col"][0] and not W["col"][-1] and not W["row"][0] and not W["row"][-1]


def one_node_neck(lx, ly):
    M = np.full((lx, ly), -1, np.int32)
    M[lx // 2, :] = 0
    M[lx // 2, ly // 2] = -1
    return M


def callers_maps(sim, what):
    lx, ly, n = sim.lx, sim.ly, sim.n
    own = sim.obst
    f = random_f(lx, ly, 7 * lx + ly)
    sim.f = f
    for merge, level in ((-1, 0), (0, 1)):
        c = check(sim, merge, level, np.full((lx, ly), -1, np.int32), what + "all fluid", f=f)
        assert c["counts"]["regions"] == 1 and c["counts"]["links"] == 0 and c["counts"]["strongest_link"] == -1
        assert c["counts"]["edges"] == lx * (ly - 1) + (lx - 1) * ly + 2 * (lx - 1) * (ly - 1) and c["col"].all() and c["row"].all()
        c = check(sim, merge, level, du.two_pores(lx, ly), what + "two pores", f=f)
        assert c["counts"]["regions"] >= 2
        c = check(sim, merge, level, one_node_neck(lx, ly), what + "a one-node neck", f=f)
        assert c["counts"]["ridge_edges"] >= 1 and c["counts"]["links"] >= 1
        c = check(sim, merge, level, du.diagonal_passage(lx, ly), what + "a diagonal step", f=f)
        c = check(sim, merge, level, np.full((lx, ly), n, np.int32), what + "no fluid", f=f)
        assert c["counts"] == dict(zip(fu.NETFLUX_COUNTERS, (0, 0, 0, 0, 0, 0, 0, 0, -1, 0))) and not c["col"].any() and not c["row"].any()
    # the passage by a diagonal step: a link whose only edge is direction 5 or 7
    c = check(sim, -1, 0, du.diagonal_passage(lx, ly), what + "a diagonal step", f=f)
    assert (c["links"]["edges"] == 1).any()
    assert np.array_equal(sim.obst, own)          # a caller's map leaves the handle's alone
    check(sim, -1, 0, what=what + "own map after callers' maps", f=f)


@pytest.mark.parametrize("lx,ly", [(48, 50), (65, 17), (17, 65)])
def test_callers_maps(pkg, lx, ly):
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        callers_maps(sim, "%d x %d: " % (lx, ly))


def test_a_taller_lattice(pkg):
    """more than one workgroup along y, lanes beyond 256"""
    lx, ly = 257, 513
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        f = random_f(lx, ly, 5)
        sim.f = f
        N = nu.restate(sim.obst, sim.n, 1)
        for level in (0, 1):
            W = check(sim, 1, level, what="tall", N=N, f=f)
        assert W["counts"]["links"] > 0 and W["row"][255:258].all()


def test_special_values(pkg):
    lx, ly = 17, 130
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        M = du.random_discs(lx, ly, sim.n, 11)
        M[0:3, 0:3] = -1
        M[3, 60:70] = -1
        M[4, 60:70] = -1
        M[lx - 1, ly - 1] = -1
        N = nu.restate(M, sim.n, -1)
        body = N["body"]
        f = np.full((lx, ly, 9), 0.25)
        k = 12344
        # a ridge edge in direction 6, (x, y) -> (x + 1, y)
        rx, ry = np.nonzero((body[:-1] >= 0) & (body[1:] >= 0) & (body[:-1] != body[1:]))
        assert len(rx) >= 2
        f[rx[0] + 1, ry[0], 6] = np.nan
        f[rx[1] + 1, ry[1], 6] = 0.25 + (k + 0.5) / 2.0 ** 32       # a tie, to even
        # across the wavefronts' seam, direction 8 from (3, 63) to (3, 64); direction 7 from (3, 63) to (4, 64) and 5 back
        f[3, 64, 8] = 0.25 + (k + 1.5) / 2.0 ** 32
        f[4, 64, 7] = 0.25 + 2.0 ** 20
        f[4, 63, 5] = 0.25 + 2.0 ** 20 - 2.0 ** -20
        f[3, 65, 4] = 0.25 - 2.0 ** 20                               # p's side of an edge: phi = +2^20
        # next to the lattice's edge
        f[0, 0, 3] = np.inf
        f[1, 0, 6] = -np.inf
        f[lx - 1, ly - 1, 0] = 2.0 ** 20                             # rho only
        sim.f = f
        for level in (0, 1):
            W = check(sim, -1, level, M, "special values", N=N, f=f)
        c = W["counts"]
        # edges left out: the NaN, 2^20 twice, the two infinities; nodes: those and the one whose rho alone is 2^20
        assert c["unaccumulated_edges"] == 5 and c["unaccumulated_nodes"] == 6
        assert W["row"][63] == (k + 2) - (2 ** 52 - 2 ** 12)          # the odd tie up, and direction 5 counts towards -y
        assert c["flowing_links"] == 1 and c["largest_imbalance"] == k          # the even tie on a ridge edge, down


def test_reuse_of_the_network_result(pkg):
    lx, ly = 100, 63
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        L_ = pkg.load_library()
        f = random_f(lx, ly, 1)
        sim.f = f
        Nm = nu.restate(sim.obst, sim.n, 1)
        before = network_device(sim, sim.network(None, 1))
        assert nu.same(before, Nm) is None
        planes = sim.network_tensors()
        kept = {k: v.clone() for k, v in planes.items()}
        check(sim, 1, 1, what="after network(merge=1)", N=Nm, f=f)
        after = network_device(sim, before["counts"])          # the network's readers are still valid and say the same
        assert nu.same(after, Nm) is None and all(bool((planes[k] == kept[k]).all()) for k in kept)
        check(sim, 1, 0, what="the other level of the same result", N=Nm, f=f)
        # another merge: the network is made again, and its readers show it
        N0 = nu.restate(sim.obst, sim.n, -1)
        check(sim, -1, 1, what="another merge", N=N0, f=f)
        assert nu.same(network_device(sim, N0["counts"]), N0) is None
        # upload_f: the network is made again and the new populations are read
        f2 = random_f(lx, ly, 2)
        sim.f = f2
        W = check(sim, -1, 0, what="after upload_f", N=N0, f=f2)
        assert nu.same(network_device(sim, N0["counts"]), N0) is None
        # a caller's map: a network of that map is made, which is not taken for the handle's
        M = du.random_discs(lx, ly, sim.n, 3)
        check(sim, -1, 0, M, "a caller's map", f=f2)
        assert nu.same(network_device(sim, nu.restate(M, sim.n, -1)["counts"]), nu.restate(M, sim.n, -1)) is None
        W2 = check(sim, -1, 0, what="the handle's map after a caller's", N=N0, f=f2)
        assert fu.same(W, W2) is None
        # a later network() takes the tables the results are aligned with away
        sim.network(None, -1)
        with pytest.raises(pkg.LbmDemError):
            sim.netflux_links()
        assert L_.lbmdem_last_error().decode() == NO_COMPUTE % "lbmdem_download_netflux_links"


def test_readers_sizing_and_validity(pkg):
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
        f = random_f(lx, ly, 3)
        sim.f = f; twin.f = f
        W = check(sim, -1, 0, f=f)
        Lb = pkg.load_library()
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        for who, what, want in (("lbmdem_download_netflux_links", "links", W["links"]),
                                ("lbmdem_download_netflux_regions", "regions", W["regions"])):
            call = getattr(Lb, who)
            cnt = ctypes.c_long(-1)
            assert call(sim._h, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == len(want) > 3
            short, cnt.value = np.zeros(len(want) - 1, want.dtype), -1
            short.view(np.int64)[:] = -7
            assert call(sim._h, vp(short), len(short), ctypes.byref(cnt)) == -1
            assert cnt.value == len(want) and (short.view(np.int64) == -7).all()
            assert Lb.lbmdem_last_error().decode() == "%s: there are %d %s, the buffer holds %d" % (who, len(want), what, len(short))
            roomy = np.zeros(len(want) + 3, want.dtype)
            assert call(sim._h, vp(roomy), len(roomy), ctypes.byref(cnt)) == 0
            assert np.array_equal(roomy[:cnt.value], want) and not roomy[cnt.value:].view(np.int64).any()
            assert call(sim._h, None, 0, None) == -1
        col, row = np.zeros(lx - 1, np.int64), np.zeros(ly - 1, np.int64)
        assert Lb.lbmdem_download_netflux_profile(sim._h, vp(col), None) == 0 and np.array_equal(col, W["col"])
        assert Lb.lbmdem_download_netflux_profile(sim._h, None, vp(row)) == 0 and np.array_equal(row, W["row"])
        assert Lb.lbmdem_download_netflux_profile(sim._h, None, None) == -1
        assert Lb.lbmdem_netflux_compute(sim._h, None, -1, 0, None) == -1
        # arguments; a refused compute leaves no result
        text = lambda call: (pytest.raises(pkg.LbmDemError, call), sim._L.lbmdem_last_error().decode())[1]
        check(sim, -1, 0, f=f)
        for bad in (-1, 2):
            assert text(lambda: sim.netflux(-1, bad)) == "lbmdem_netflux_compute: level must be 0 (between bodies) or 1 (between groups) (%d)" % bad
        refused()
        assert text(lambda: sim.netflux(-2, 0)) == "lbmdem_netflux_compute: merge must be -1 (no merging) or a difference of radii >= 0 (-2)"
        assert text(lambda: sim.set_netflux_output(True, -2, 0)) == ("lbmdem_set_netflux_output: merge must be -1 (no merging) or a "
                                                                       "difference of radii >= 0 (-2)")
        assert text(lambda: sim.set_netflux_output(True, 0, 3)) == ("lbmdem_set_netflux_output: level must be 0 (between bodies) or 1 "
                                                                      "(between groups) (3)")
        bad = sim.obst.copy()
        bad[40, 3] = sim.n + 1
        assert text(lambda: sim.netflux(-1, 0, bad)) == ("lbmdem_netflux_compute: map[%d] = %d (node 40, 3) is neither -1 (fluid), a grain "
                                                         "(0 .. %d) nor the wall (%d)" % (40 * ly + 3, sim.n + 1, sim.n - 1, sim.n))
        with pytest.raises(pkg.LbmDemError):
            sim.netflux(-1, 0, np.zeros((ly, lx), np.int32))
        refused()
        # steps and uploads invalidate, and the computes have disturbed nothing
        check(sim, -1, 0)
        for call in readers_of(sim):                # reading does not invalidate
            call()
        sim.lbm_step(); twin.lbm_step()
        refused()                                   # after a fluid step
        check(sim, 1, 1)
        sim.f = sim.f; twin.f = twin.f
        refused()                                   # after upload_f
        check(sim, 1, 1)
        sim.kinematics = sim.kinematics; twin.kinematics = twin.kinematics
        refused()                                   # after a grain upload
        check(sim, 1, 0)
        sim.renderScene(sim.cfg.npDEM + 1); twin.renderScene(twin.cfg.npDEM + 1)
        refused()                                   # after coupled steps
        check(sim, -1, 0)
        for what in ("f", "obst", "kinematics", "fhf"):
            assert np.array_equal(getattr(sim, what), getattr(twin, what)), what


def test_refusals(pkg, tmp_path):
    lx, ly = 64, 64
    r, x, y = shape_scene(lx, ly)
    calls = lambda s: ([("lbmdem_netflux_compute", lambda: s.netflux())] + list(zip(READERS, readers_of(s))) +
                       [("lbmdem_write_netflux", lambda: s.write_netflux(str(tmp_path), 0)),
                        ("lbmdem_set_netflux_output", lambda: s.set_netflux_output(True))])

    def text(sim, call):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1, e.value
        return sim._L.lbmdem_last_error().decode()
    if os.path.exists(pkg.SP_LIB_PATH):
        with pkg.LbmDem(lx, ly, r, x, y, precision="f32") as sp:
            for who, call in calls(sp):
                assert text(sp, call) == "the pore flux analysis is not available in the single-precision build of the library", who
    with pkg.LbmDem(lx, ly, r, x, y, strip=(lx // 2, lx), halo=12) as strip:
        for who, call in calls(strip):
            assert text(strip, call) == who + WHOLE
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        missing = str(tmp_path / "missing")
        assert text(sim, lambda: sim.write_netflux(missing, 0)) == f"cannot open '{missing}/netflux_links000000.dat' for writing"
        assert os.listdir(tmp_path) == []
        sim.set_netflux_output(True, 1, 1)
        assert text(sim, sim.dist_enable) == ("the pore flux analysis is not available with distributed grains "
                                              "(lbmdem_set_netflux_output(h, 0, 0, 0) first)")
        sim.set_netflux_output(False)
        sim.dist_enable()
        for who, call in calls(sim):
            assert text(sim, call) == who + WHOLE


MERGE, LEVEL = 1, 1


@pytest.fixture(scope="module")
def scene(pkg, tmp_path_factory):
    """a packing through run_scene over two DEM events, with the pore flux output on and without"""
    lx, ly = 61, 59
    r, x, y = shape_scene(lx, ly)
    with_dir, without_dir = tmp_path_factory.mktemp("with"), tmp_path_factory.mktemp("without")
    steps = 8000
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.run_scene(steps, str(without_dir))
        end = {what: getattr(sim, what) for what in ("f", "obst", "kinematics", "fhf")}
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.set_netflux_output(True, MERGE, LEVEL)
        _, res = sim.run_scene(steps, str(with_dir))
        for what in end:
            assert np.array_equal(getattr(sim, what), end[what]), what
        # the last event is the run's last sub-step: the restatement of the state the run ends in
        W = fu.restate(sim.obst, sim.f, sim.n, MERGE, LEVEL)
        t = sim.nbsteps * sim.config().dt
        n = sim.n
    return dict(lx=lx, ly=ly, r=r, x=x, y=y, n=n, with_dir=with_dir, without_dir=without_dir, steps=steps, W=W, t=t, nfile=res["nfile"])


NEW_FILES = ("netflux_links%06d.dat", "netflux_regions%06d.dat", "netflux_profile%06d.dat")


def test_run_scene_with_the_netflux_output(pkg, scene, tmp_path):
    S = scene
    lx, ly, W, last = S["lx"], S["ly"], S["W"], S["nfile"]
    others = sorted(os.listdir(S["without_dir"]))
    numbers = sorted({int(name[3:9]) for name in others if name.startswith("DEM") and name.endswith(".dat")})
    assert last in numbers
    new = ["netflux.data"] + [p % k for k in numbers for p in NEW_FILES]
    assert sorted(os.listdir(S["with_dir"])) == sorted(others + new)
    for name in others:
        assert (S["with_dir"] / name).read_bytes() == (S["without_dir"] / name).read_bytes(), name
    lines = (S["with_dir"] / "netflux.data").read_text().splitlines()
    events = len((S["with_dir"] / "stats.data").read_text().splitlines())
    assert lines[0] + "\n" == fu.DATA_HEADER and len(lines) == 1 + events and events == 2
    assert W["counts"]["regions"] >= 2 and W["counts"]["flowing_links"] > 0
    pkg.write_netflux_files(str(tmp_path), last, lx, ly, S["n"], MERGE, LEVEL, W["table"], W["links"], W["region_body"], W["region_nodes"],
                            W["regions"], W["col"], W["row"], W["counts"], S["t"])
    want = fu.files_bytes(lx, ly, S["n"], MERGE, LEVEL, W, S["t"], nfile=last)
    assert lines[-1] + "\n" == want.pop("netflux.data").decode()
    for name, data in want.items():
        assert (S["with_dir"] / name).read_bytes() == data == (tmp_path / name).read_bytes(), name


def test_host_driver_writes_the_netflux_files(po, scene, tmp_path):
    """`lbmdem <sample> --steps N --netflux 1 --netflux-merge 1` in a child process"""
    S = scene
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), S["r"] * 1e3, S["x"] * 1e3, S["y"] * 1e3)
    out = subprocess.run([EXE, str(sample), "--lx", str(S["lx"]), "--ly", str(S["ly"]), "--steps", str(S["steps"] + 1), "--netflux", str(LEVEL),
                          "--netflux-merge", str(MERGE)], capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    names = [name for name in os.listdir(S["with_dir"]) if name.startswith("netflux")]
    assert "netflux.data" in names and len(names) >= 4
    for name in names:
        assert (tmp_path / name).read_bytes() == (S["with_dir"] / name).read_bytes(), name
    refused = subprocess.run([EXE, str(sample), "--netflux", "--gpus", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "--netflux is a single-GPU mode" in refused.stderr
    refused = subprocess.run([EXE, str(sample), "--netflux", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "--netflux [LEVEL]" in refused.stderr
    refused = subprocess.run([EXE, str(sample), "--netflux-merge", "1"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "--netflux-merge needs --netflux" in refused.stderr
