"""GPU: the network pressures (lbmdem_netsolve_compute and its readers, lbmdem_write_netsolve, lbmdem_set_netsolve_output;
include/lbmdem_hip.h) against the numpy restatement (tests/netsolve_util.py, pinned by tests/test_netsolve_host.py): every double
array_equal on the bits, counts and sums too."""
import os
import subprocess

import numpy as np
import pytest

import drainage_util as du
import netsolve_util as su
import network_util as nu
from test_gpu_pores import shape_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
WHOLE = " needs the whole lattice and all grains on this handle (not a strip of a decomposition, no distributed grains)"
NO_COMPUTE = "%s: no lbmdem_netsolve_compute has been made for the map as it is now"
READERS = ("lbmdem_download_netsolve_regions", "lbmdem_download_netsolve_links", "lbmdem_netsolve_rounds")
B, T, L, R = du.SIDE_B, du.SIDE_T, du.SIDE_L, du.SIDE_R


def readers_of(sim):
    return (sim.netsolve_regions, sim.netsolve_links, sim.netsolve_rounds)


def device(sim, result):
    out = dict(counts=result[0], sums=result[1], regions=sim.netsolve_regions(), links=sim.netsolve_links())
    assert out["regions"].dtype == su.NETSOLVE_REGION_DTYPE and out["links"].dtype == su.NETSOLVE_LINK_DTYPE
    return out


def check(sim, frm, band, to, merge=-1, level=0, M=None, what="", N=None, **kw):
    """one compute against the restatement, every output -> the restatement. M: a caller's map (None: the handle's)"""
    W = su.restate(sim.obst if M is None else M, sim.n, frm, band, to, merge, level, model=kw.get("model", 0), g_user=kw.get("g"),
                   rtol=kw.get("rtol", 1e-8), max_iter=kw.get("max_iter", 0), N=N)
    D = device(sim, sim.netsolve(frm, band, to, merge, level, map=M, **kw))
    assert D["counts"] == W["counts"], (what, merge, level, D["counts"], W["counts"])
    assert su.same(D, W) is None, (what, merge, level, sim.lx, sim.ly, su.same(D, W), D["sums"], W["sums"])
    # launches: whole batches of 16 iterations, two each, until the launch that makes the last test has run
    c = W["counts"]
    if c["regions"]:
        pairs = c["iterations"] + 1
        assert sim.netsolve_rounds() == 32 * max(1, -(-pairs // 16)), (what, sim.netsolve_rounds(), c)
    return W


CASES = ((-1, 0), (1, 1))


@pytest.mark.parametrize("lx,ly", [(13, 61), (33, 62), (64, 64), (127, 121), (256, 200)])
def test_rasterised_packings(pkg, lx, ly):
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        flowing = 0
        for stepped in (False, True):
            if stepped:
                sim.renderScene(2 * sim.cfg.npDEM + 1)
            Ns = {m: nu.restate(sim.obst, sim.n, m) for m in (-1, 1)}
            for merge, level in CASES:
                for frm, band, to in ((T, 4, B), (L, 3, R)):
                    W = check(sim, frm, band, to, merge, level, what="stepped" if stepped else "rest", N=Ns[merge])
                    flowing += W["counts"]["flowing_links"]
                    assert W["counts"]["status"] == 0 and W["counts"]["regions"] >= 1
        assert flowing > 0 or lx < 20


def test_callers_maps(pkg):
    lx, ly = 48, 50
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        own = sim.obst
        for merge, level in ((-1, 0), (0, 1)):
            W = check(sim, B, 2, T, merge, level, np.full((lx, ly), -1, np.int32), "all fluid")
            assert W["counts"] == dict(zip(su.NETSOLVE_COUNTERS, (1, 0, 1, 0, 1, 0, 0, 0, 0, -1)))
            W = check(sim, B, 3, B, merge, level, du.two_pores(lx, ly), "two pores")
            far = (W["regions"]["flags"] == 0) & (W["regions"]["p"].view(np.int64) == 0)          # exact zeros behind the wall
            assert far.any() and W["counts"]["inlet_regions"] >= 1
            assert not W["links"]["q"][far[W["lo"]] | far[W["hi"]]].view(np.int64).any()
            W = check(sim, B, 5, T, merge, level, du.chamber_behind_neck(lx, ly), "a chamber behind a neck")
            W = check(sim, B, 3, T, merge, level, du.two_routes(lx, ly), "two routes")
            q = W["links"]["q"][W["links"]["q"] != 0]
            if level == 0:          # the two routes: equal on the bits (merged, the halves of one channel may join)
                assert len(q) == 2 and q.view(np.int64)[0] == q.view(np.int64)[1]
            assert len(q) >= 1 and W["sums"]["Q_in"] > 0
            M = du.random_discs(lx, ly, sim.n, 5)
            M[:, :3] = sim.n
            W = check(sim, B, 3, T, merge, level, M, "an empty inlet")
            assert W["counts"]["inlet_regions"] == 0 and W["counts"]["iterations"] == 0 and not W["regions"]["p"].any()
            W = check(sim, B, 3, T, merge, level, np.full((lx, ly), sim.n, np.int32), "no fluid")
            assert W["counts"]["regions"] == 0
            W = check(sim, T, 4, T, merge, level, du.random_discs(lx, ly, sim.n, 2), "from == to")
            assert W["counts"]["shorted_regions"] == W["counts"]["inlet_regions"] >= 1
        # model 1: a seeded random g
        M = du.random_discs(lx, ly, sim.n, 9)
        for merge, level in ((-1, 0), (1, 1)):
            net = nu.restate(M, sim.n, merge)
            g = np.random.default_rng(17).uniform(0.05, 3.0, len(net["links1" if level else "links0"]))
            W = check(sim, L, 3, R, merge, level, M, "model 1", N=net, model=1, g=g, rtol=1e-10)
            assert W["counts"]["links"] >= (3 if level == 0 else 1) and np.array_equal(W["links"]["g"], g)
        assert np.array_equal(sim.obst, own)          # a caller's map leaves the handle's alone
        check(sim, T, 4, B, what="own map after callers' maps")


def test_a_row_longer_than_a_wavefront(pkg):
    M = su.star()
    lx, ly = M.shape
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        W = check(sim, B, 5, T, -1, 0, M, "star")
        assert W["regions"]["degree"].max() > 64 and W["regions"]["flags"][np.argmax(W["regions"]["degree"])] == 0
        assert W["counts"]["inlet_regions"] >= 10 and W["counts"]["outlet_regions"] >= 10 and W["counts"]["status"] == 0
        check(sim, L, 5, R, -1, 1, M, "star, level 1")


def test_three_levels_of_the_reduction(pkg):
    lx = ly = 1301
    M = su.chambers(lx, ly)
    r, x, y = shape_scene(lx, ly)          # (the map is the caller's)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        net = nu.restate(M, sim.n, -1)
        W = check(sim, L, 6, R, -1, 0, M, "chambers", N=net, max_iter=5)
        assert W["counts"]["regions"] > 65536 and W["counts"]["status"] == 1 and W["counts"]["iterations"] == 5
        assert W["counts"]["inlet_regions"] > 0 and W["counts"]["outlet_regions"] > 0


def test_max_iter_stops_where_the_restatement_stops(pkg):
    lx, ly = 127, 121
    r, x, y = shape_scene(lx, ly)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        M = du.random_discs(lx, ly, sim.n, 12700)
        net = nu.restate(M, sim.n, -1)
        seen = []
        for k in (1, 7, 33, 0):
            W = check(sim, T, 4, B, -1, 0, M, "max_iter %d" % k, N=net, max_iter=k)
            seen.append((W["counts"]["status"], W["counts"]["iterations"]))
        assert seen[:3] == [(1, 1), (1, 7), (1, 33)] and seen[3][0] == 0 and seen[3][1] > 33


def test_readers_sizing_and_validity(pkg):
    import ctypes
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
        N0 = nu.restate(sim.obst, sim.n, -1)
        W = check(sim, T, 4, B, N=N0)
        Lb = pkg.load_library()
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        for who, what, want in (("lbmdem_download_netsolve_regions", "regions", W["regions"]),
                                ("lbmdem_download_netsolve_links", "links", W["links"])):
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
            assert roomy[:cnt.value].tobytes() == want.tobytes() and not roomy[cnt.value:].view(np.int64).any()
            assert call(sim._h, None, 0, None) == -1
        # arguments; a refused compute leaves no result
        text = lambda call: (pytest.raises(pkg.LbmDemError, call), sim._L.lbmdem_last_error().decode())[1]
        who = "lbmdem_netsolve_compute: "
        for kw, want in ((dict(frm=0), "from must be a mask of sides, B 1 | T 2 | L 4 | R 8, with at least one (0)"),
                         (dict(frm=16), "from must be a mask of sides, B 1 | T 2 | L 4 | R 8, with at least one (16)"),
                         (dict(to=0), "to must be a mask of sides, B 1 | T 2 | L 4 | R 8, with at least one (0)"),
                         (dict(to=16), "to must be a mask of sides, B 1 | T 2 | L 4 | R 8, with at least one (16)"),
                         (dict(band=0), "band must be at least 1 node (0)"),
                         (dict(level=2), "level must be 0 (between bodies) or 1 (between groups) (2)"),
                         (dict(level=-1), "level must be 0 (between bodies) or 1 (between groups) (-1)"),
                         (dict(merge=-2), "merge must be -1 (no merging) or a difference of radii >= 0 (-2)"),
                         (dict(model=2), "model must be 0 (plane Poiseuille from the saddle) or 1 (the caller's g) (2)"),
                         (dict(model=1), "model 1 needs g_user, one conductance per link"),
                         (dict(g=np.ones(len(W["links"]))), "g_user must be NULL with model 0"),
                         (dict(rtol=0.0), "rtol must lie strictly between 0 and 1 (0)"),
                         (dict(rtol=1.0), "rtol must lie strictly between 0 and 1 (1)"),
                         (dict(rtol=float("nan")), "rtol must lie strictly between 0 and 1 (nan)"),
                         (dict(max_iter=-1), "max_iter must not be negative, 0: the number of free regions (-1)")):
            check(sim, T, 4, B, N=N0)
            args = dict(dict(frm=T, band=4, to=B), **kw)
            assert text(lambda: sim.netsolve(**args)) == who + want, kw
            refused()
        g = np.ones(len(W["links"]))
        for k, v in ((2, 0.0), (1, -1.0), (3, np.inf), (0, np.nan)):
            bad = g.copy()
            bad[k] = v
            bad[-1] = -3.0          # (a later offender: the first is named)
            assert text(lambda: sim.netsolve(T, 4, B, model=1, g=bad)) == who + "g_user[%d] = %g: a conductance is finite and > 0" % (k, v)
        refused()
        bad = sim.obst.copy()
        bad[40, 3] = sim.n + 1
        assert text(lambda: sim.netsolve(T, 4, B, map=bad)) == (who + "map[%d] = %d (node 40, 3) is neither -1 (fluid), a grain "
                                                                "(0 .. %d) nor the wall (%d)" % (40 * ly + 3, sim.n + 1, sim.n - 1, sim.n))
        assert text(lambda: sim.set_netsolve_output(True, T, 0, B)) == "lbmdem_set_netsolve_output: band must be at least 1 node (0)"
        assert Lb.lbmdem_netsolve_compute(sim._h, None, -1, 0, T, 4, B, 0, None, 1e-8, 0, None, None) == -1
        refused()
        # a later network() takes the tables the results are aligned with away
        check(sim, T, 4, B)
        sim.network(None, -1)
        refused()
        # steps invalidate as they invalidate the network's readers, and the computes have disturbed nothing
        check(sim, T, 4, B)
        for call in readers_of(sim):                # reading does not invalidate
            call()
        sim.renderScene(sim.cfg.npDEM + 1); twin.renderScene(twin.cfg.npDEM + 1)
        refused()                                   # after coupled steps
        check(sim, L, 3, R, 1, 1)
        sim.dem_substep(); twin.dem_substep()
        refused()                                   # after a sub-step
        check(sim, L, 3, R)
        sim.lbm_step(); twin.lbm_step()
        refused()                                   # after a fluid step: the network's guard
        check(sim, T, 2, B)
        for what in ("f", "obst", "kinematics", "fhf"):
            assert np.array_equal(getattr(sim, what), getattr(twin, what)), what
        # the permeability: Q_in * L / W for one pair of opposite sides
        c, s = sim.netsolve(T, 4, B)
        assert sim.netsolve_permeability() == s["Q_in"] * ly / lx
        c, s = sim.netsolve(L, 4, R)
        assert sim.netsolve_permeability() == s["Q_in"] * lx / ly
        sim.netsolve(T, 4, L)
        with pytest.raises(ValueError):
            sim.netsolve_permeability()


def test_refusals(pkg, tmp_path):
    lx, ly = 64, 64
    r, x, y = shape_scene(lx, ly)
    calls = lambda s: ([("lbmdem_netsolve_compute", lambda: s.netsolve(T, 4, B))] + list(zip(READERS, readers_of(s))) +
                       [("lbmdem_write_netsolve", lambda: s.write_netsolve(str(tmp_path), 0)),
                        ("lbmdem_set_netsolve_output", lambda: s.set_netsolve_output(True))])

    def text(sim, call):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1, e.value
        return sim._L.lbmdem_last_error().decode()
    if os.path.exists(pkg.SP_LIB_PATH):
        with pkg.LbmDem(lx, ly, r, x, y, precision="f32") as sp:
            for who, call in calls(sp):
                assert text(sp, call) == "the network pressure analysis is not available in the single-precision build of the library", who
    with pkg.LbmDem(lx, ly, r, x, y, strip=(lx // 2, lx), halo=12) as strip:
        for who, call in calls(strip):
            assert text(strip, call) == who + WHOLE
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        missing = str(tmp_path / "missing")
        assert text(sim, lambda: sim.write_netsolve(missing, 0)) == f"cannot open '{missing}/netsolve_regions000000.dat' for writing"
        assert os.listdir(tmp_path) == []
        sim.set_netsolve_output(True, T, 4, B, 1, 1)
        assert text(sim, sim.dist_enable) == ("the network pressure analysis is not available with distributed grains "
                                              "(lbmdem_set_netsolve_output(h, 0, 0, 0, 0, 0, 0, 0., 0) first)")
        sim.set_netsolve_output(False)
        sim.dist_enable()
        for who, call in calls(sim):
            assert text(sim, call) == who + WHOLE


MERGE, LEVEL, FROM, BAND, TO = 1, 1, T, 4, B


@pytest.fixture(scope="module")
def scene(pkg, tmp_path_factory):
    """a packing through run_scene over two DEM events, with the network pressure output on and without"""
    lx, ly = 61, 59
    r, x, y = shape_scene(lx, ly)
    with_dir, without_dir = tmp_path_factory.mktemp("with"), tmp_path_factory.mktemp("without")
    steps = 8000
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.run_scene(steps, str(without_dir))
        end = {what: getattr(sim, what) for what in ("f", "obst", "kinematics", "fhf")}
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.set_netsolve_output(True, FROM, BAND, TO, MERGE, LEVEL)
        _, res = sim.run_scene(steps, str(with_dir))
        for what in end:
            assert np.array_equal(getattr(sim, what), end[what]), what
        # the last event is the run's last sub-step: the restatement of the state the run ends in
        W = su.restate(sim.obst, sim.n, FROM, BAND, TO, MERGE, LEVEL)
        t = sim.nbsteps * sim.config().dt
        n = sim.n
    return dict(lx=lx, ly=ly, r=r, x=x, y=y, n=n, with_dir=with_dir, without_dir=without_dir, steps=steps, W=W, t=t, nfile=res["nfile"])


NEW_FILES = ("netsolve_regions%06d.dat", "netsolve_links%06d.dat")


def test_run_scene_with_the_netsolve_output(pkg, scene, tmp_path):
    S = scene
    lx, ly, W, last = S["lx"], S["ly"], S["W"], S["nfile"]
    others = sorted(os.listdir(S["without_dir"]))
    numbers = sorted({int(name[3:9]) for name in others if name.startswith("DEM") and name.endswith(".dat")})
    assert last in numbers
    new = ["netsolve.data"] + [p % k for k in numbers for p in NEW_FILES]
    assert sorted(os.listdir(S["with_dir"])) == sorted(others + new)
    for name in others:
        assert (S["with_dir"] / name).read_bytes() == (S["without_dir"] / name).read_bytes(), name
    lines = (S["with_dir"] / "netsolve.data").read_text().splitlines()
    events = len((S["with_dir"] / "stats.data").read_text().splitlines())
    assert lines[0] + "\n" == su.DATA_HEADER and len(lines) == 1 + events and events == 2
    assert W["counts"]["regions"] >= 2
    pkg.write_netsolve_files(str(tmp_path), last, lx, ly, S["n"], MERGE, LEVEL, FROM, BAND, TO, W["table"], W["links"], W["region_body"],
                             W["regions"], W["counts"], W["sums"], S["t"])
    want = su.files_bytes(lx, ly, S["n"], MERGE, LEVEL, FROM, BAND, TO, W, S["t"], nfile=last)
    assert lines[-1] + "\n" == want.pop("netsolve.data").decode()
    for name, data in want.items():
        assert (S["with_dir"] / name).read_bytes() == data == (tmp_path / name).read_bytes(), name


def test_host_driver_writes_the_netsolve_files(po, scene, tmp_path):
    """`lbmdem <sample> --steps N --netsolve T --netsolve-to B --netsolve-band 4 --netsolve-level 1 --netsolve-merge 1` in a child
    process"""
    S = scene
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), S["r"] * 1e3, S["x"] * 1e3, S["y"] * 1e3)
    out = subprocess.run([EXE, str(sample), "--lx", str(S["lx"]), "--ly", str(S["ly"]), "--steps", str(S["steps"] + 1), "--netsolve", "T",
                          "--netsolve-to", "B", "--netsolve-band", str(BAND), "--netsolve-level", str(LEVEL), "--netsolve-merge", str(MERGE),
                          "--netsolve-rtol", "1e-8", "--netsolve-max-iter", "0"], capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    names = [name for name in os.listdir(S["with_dir"]) if name.startswith("netsolve")]
    assert "netsolve.data" in names and len(names) >= 3
    for name in names:
        assert (tmp_path / name).read_bytes() == (S["with_dir"] / name).read_bytes(), name
    refused = subprocess.run([EXE, str(sample), "--netsolve", "T", "--netsolve-to", "B", "--gpus", "2"], capture_output=True, text=True,
                             cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "--netsolve is a single-GPU mode" in refused.stderr
    refused = subprocess.run([EXE, str(sample), "--netsolve", "T"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "--netsolve FROM needs --netsolve-to TO" in refused.stderr
    refused = subprocess.run([EXE, str(sample), "--netsolve-band", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "need --netsolve FROM" in refused.stderr
    refused = subprocess.run([EXE, str(sample), "--netsolve", "X"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert refused.returncode != 0 and "--netsolve SIDES" in refused.stderr
