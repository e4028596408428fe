"""Cost of the drainage analysis (lbmdem_drainage_compute) on the flagship workload, 4096^2 / 50 000 grains after three coupled
steps, from T to B with a band of 8, and on an all-fluid 4096^2 map as the other extreme: warmed calls, ms per call (the call ends
in a synchronise), with the network result there and without it, the launches of the relaxation, against what it replaces on the
same box -- the downloads of d2, the body plane and the tables plus tests/drainage_util.py's restatement over them -- with every
output compared; `trace`: a few calls of each for rocprofv3 --kernel-trace --stats.
    python scripts/drainage_cost.py [trace]"""
import json, os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench
import __graft_entry__ as ge
import drainage_util as du
pkg = ge.load_package()
w = bench.workload("metric")
(r, x1, x2), _ = bench.make_sample(w)
sim = pkg.LbmDem(w["lx"], w["ly"], r, x1, x2)
sim.renderScene(3 * sim.cfg.npDEM); sim.sync()
fluid_map = np.full((sim.lx, sim.ly), -1, np.int32)
FRM, BAND, TO = du.SIDE_T, 8, du.SIDE_B
trace_only = len(sys.argv) > 1 and sys.argv[1] == "trace"
if trace_only:
    for rep in range(3):
        c = sim.drainage(FRM, BAND, TO)
    for rep in range(2):
        c = sim.drainage(FRM, BAND, TO, fluid_map)
    print("trace run:", c)
    sys.exit(0)
res = {"grains": int(sim.n), "lattice": [sim.lx, sim.ly], "from": FRM, "band": BAND, "to": TO}


def timed(call, reps):
    call(); call()
    ms = []
    for rep in range(reps):
        sim.sync()
        t0 = time.perf_counter(); out = call(); t1 = time.perf_counter()
        ms.append(round(1e3 * (t1 - t0), 3))
    return ms, out


for name, M, reps in (("packing", None, 5), ("all_fluid", fluid_map, 3)):
    ms, c = timed(lambda: sim.drainage(FRM, BAND, TO, M), reps)        # (M None: the network result is reused from the second call on)
    res[name + "_ms"], res[name + "_counts"], res[name + "_rounds"] = ms, c, sim.drainage_rounds()
    print(name, "ms per call", ms, "relaxation launches", res[name + "_rounds"], c, flush=True)
    if M is None:
        ms, _ = timed(lambda: (sim.dem_substep(), sim.drainage(FRM, BAND, TO))[1], reps)      # (a sub-step: clearance and network again)
        res[name + "_with_network_and_substep_ms"] = ms
        ms, _ = timed(lambda: (sim.dem_substep(), sim.network())[1], reps)
        res[name + "_network_and_substep_ms"] = ms
        for frm, to in ((du.SIDE_L, du.SIDE_R), (15, 0)):
            ms, cc = timed(lambda: sim.drainage(frm, BAND, to), 3)
            res["%s_from%d_to%d" % (name, frm, to)] = dict(ms=ms, rounds=sim.drainage_rounds(), critical=cc["critical"])
        c = sim.drainage(FRM, BAND, TO)
        print(name, {k: v for k, v in res.items() if k.startswith(name + "_")}, flush=True)
    D = dict(counts=c, access=sim.drainage_plane(), A=sim.drainage_bodies(), passes=sim.drainage_links(), hist=sim.drainage_hist())
    t0 = time.perf_counter()
    d2, _ = sim.clearance_planes(); body, _ = sim.network_planes()
    net = dict(d2=d2, body=body, bodies=sim.network_bodies(), links0=sim.network_links(0))
    t1 = time.perf_counter()
    R = du.restate(sim.obst if M is None else M, sim.n, FRM, BAND, TO, N=net)
    t2 = time.perf_counter()
    res[name + "_host_download_ms"], res[name + "_host_restate_ms"] = round(1e3 * (t1 - t0), 1), round(1e3 * (t2 - t1), 1)
    res[name + "_host_jacobi_rounds"] = R["rounds"]
    assert du.same(D, R) is None, (name, du.same(D, R))
    print(name, "download ms", res[name + "_host_download_ms"], "restatement ms", res[name + "_host_restate_ms"], "rounds there",
          R["rounds"], "all outputs equal", flush=True)
print(json.dumps(res))
