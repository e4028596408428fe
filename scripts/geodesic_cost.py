"""Cost of the geodesic analysis (lbmdem_geodesic_compute) on the flagship workload, 4096^2 / 50 000 grains after three coupled
steps, and on an all-fluid 4096^2 map as the other extreme: warmed calls, ms per call (the call ends in a synchronise), from T to
B with a band of 8 and from L to R, conn 4 and 8, with and without the backward pass, min_d2 0 and 16, and the launches of the two
relaxations. Every dist plane is certified on the host in one numpy pass: 0 on the seed, elsewhere equal to the least neighbour
plus the step (with positive steps that fixed point is the distance). What the call replaces, the download of the map plus
tests/geodesic_util.py's two statements, is timed on a 512 x 512 corner of the same map, where every output is compared too: at
4096^2 the Python statements take minutes to hours.
    python scripts/geodesic_cost.py"""
import json, os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench
import __graft_entry__ as ge
import drainage_util as du
import geodesic_util as gu
from test_gpu_pores import shape_scene
pkg = ge.load_package()
w = bench.workload("metric")
(r, x1, x2), _ = bench.make_sample(w)
sim = pkg.LbmDem(w["lx"], w["ly"], r, x1, x2)
sim.renderScene(3 * sim.cfg.npDEM); sim.sync()
fluid_map = np.full((sim.lx, sim.ly), -1, np.int32)
BAND = 8
res = {"grains": int(sim.n), "lattice": [sim.lx, sim.ly], "band": BAND}


def timed(call, reps):
    call()
    ms = []
    for rep in range(reps):
        sim.sync()
        t0 = time.perf_counter(); out = call(); t1 = time.perf_counter()
        ms.append(round(1e3 * (t1 - t0), 3))
    return ms, out


def certify(P, frm, conn, dist):
    """dist is the distance plane of the passable plane P: -1 off P, 0 on the seed, elsewhere the least neighbour plus the step"""
    lx, ly = P.shape
    D = np.full((lx + 2, ly + 2), gu.INF, np.int64)
    dist = dist.astype(np.int64)
    D[1:-1, 1:-1] = np.where(dist >= 0, dist, gu.INF)
    best = np.full((lx, ly), gu.INF, np.int64)
    for dx, dy, step in (gu.STEPS8 if conn == 8 else gu.STEPS4):
        np.minimum(best, D[1 + dx:lx + 1 + dx, 1 + dy:ly + 1 + dy] + step, out=best)
    seed = P & du.region(lx, ly, frm, BAND)
    want = np.where(P, np.where(seed, 0, np.where(best < gu.INF, best, -1)), -1)
    return bool(np.array_equal(want, dist))


for name, M in (("packing", None), ("all_fluid", fluid_map)):
    P = (sim.obst if M is None else M) == -1
    for frm, to in ((du.SIDE_T, du.SIDE_B), (du.SIDE_L, du.SIDE_R)):
        for conn in (4, 8):
            for back in (True, False):
                ms, c = timed(lambda: sim.geodesic(frm, BAND, to if back else 0, conn, 0, M), 3)
                ok = certify(P, frm, conn, sim.geodesic_planes()["dist"])
                key = "%s_from%d_conn%d_%s" % (name, frm, conn, "both" if back else "forward")
                res[key] = dict(ms=ms, rounds=sim.geodesic_rounds(), shortest=c["shortest"], dist_max=c["dist_max"],
                                reached=c["reached_nodes"], path_nodes=c["path_nodes"], certified=ok)
                print(key, res[key], flush=True)
                assert ok, key
    if M is None:
        ms, c = timed(lambda: sim.geodesic(du.SIDE_T, BAND, du.SIDE_B, 8, 16), 3)       # (the clearance result is reused from the second call on)
        d2, _ = sim.clearance_planes()
        ok = certify(d2 >= 16, du.SIDE_T, 8, sim.geodesic_planes()["dist"])
        res["packing_min_d2_16"] = dict(ms=ms, rounds=sim.geodesic_rounds(), shortest=c["shortest"], passable=c["passable_nodes"],
                                        reached=c["reached_nodes"], certified=ok)
        ms, _ = timed(lambda: (sim.dem_substep(), sim.geodesic(du.SIDE_T, BAND, du.SIDE_B, 8, 16))[1], 3)    # (a sub-step: the clearance again)
        res["packing_min_d2_16"]["with_clearance_and_substep_ms"] = ms
        print("packing_min_d2_16", res["packing_min_d2_16"], flush=True)
        assert ok
# what the call replaces, on a corner of the packing's map
t0 = time.perf_counter(); obst = sim.obst; t1 = time.perf_counter()
res["download_obst_ms"] = round(1e3 * (t1 - t0), 1)
side = 512
corner = np.ascontiguousarray(obst[:side, :side])
small = pkg.LbmDem(side, side, *shape_scene(side, side))
t0 = time.perf_counter(); W = gu.restate(corner, sim.n, du.SIDE_T, BAND, du.SIDE_B, 8, 0); t1 = time.perf_counter()
V = gu.brute_force(corner, sim.n, du.SIDE_T, BAND, du.SIDE_B, 8, 0); t2 = time.perf_counter()
corner_map = np.where(corner == -1, -1, 0).astype(np.int32)
ms, c = timed(lambda: small.geodesic(du.SIDE_T, BAND, du.SIDE_B, 8, 0, corner_map), 3)
D = dict(small.geodesic_planes(), counts=c, profile=small.geodesic_profile())
assert gu.same(D, W) is None and gu.same(V, W) is None, (gu.same(D, W), gu.same(V, W))
res["corner_512"] = dict(device_ms=ms, rounds=small.geodesic_rounds(), restate_ms=round(1e3 * (t1 - t0), 1), restate_sweeps=W["rounds"],
                         brute_force_ms=round(1e3 * (t2 - t1), 1), all_outputs_equal=True)
print("corner_512", res["corner_512"], flush=True)
print(json.dumps(res))
