"""Cost of the pore network analysis (lbmdem_network_compute) on the flagship workload, 4096^2 / 50 000 grains after three coupled
steps, with merge -1 and 1, and on the worst case of the ascent's chains, an all-fluid 4096^2 map: warmed calls, ms per call (the
call ends in a synchronise), with and without a clearance result to reuse, against what it replaces on the same box --
clearance_planes() plus tests/network_util.py's restatement over the downloaded d2 -- with every output compared; the counts of the
packing at merge -1, 0, 1, 2; `trace`: a few calls of each for rocprofv3 --kernel-trace --stats.
    python scripts/network_cost.py [trace]"""
import json, os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench
import __graft_entry__ as ge
import network_util as nu
pkg = ge.load_package()
w = bench.workload("metric")
(r, x1, x2), _ = bench.make_sample(w)
sim = pkg.LbmDem(w["lx"], w["ly"], r, x1, x2)
sim.renderScene(3 * sim.cfg.npDEM); sim.sync()
fluid_map = np.full((sim.lx, sim.ly), -1, np.int32)
trace_only = len(sys.argv) > 1 and sys.argv[1] == "trace"
if trace_only:
    for merge in (-1, 1):
        for rep in range(3):
            c = sim.network(None, merge)
    for rep in range(2):
        c = sim.network(fluid_map, 1)
    print("trace run:", c)
    sys.exit(0)
res = {"grains": int(sim.n), "lattice": [sim.lx, sim.ly]}


def timed(call, reps):
    call(); call()
    ms = []
    for rep in range(reps):
        sim.sync()
        t0 = time.perf_counter(); out = call(); t1 = time.perf_counter()
        ms.append(round(1e3 * (t1 - t0), 3))
    return ms, out


for name, M, merge, reps in (("packing_m-1", None, -1, 5), ("packing_m1", None, 1, 5), ("all_fluid_m1", fluid_map, 1, 3)):
    ms, c = timed(lambda: sim.network(M, merge), reps)            # (M None: the clearance result is reused from the second call on)
    res[name + "_ms"], res[name + "_counts"] = ms, c
    print(name, "ms per call", ms, c, flush=True)
    if M is None:
        ms, _ = timed(lambda: (sim.dem_substep(), sim.network(M, merge))[1], reps)      # (a sub-step: the clearance is made again)
        res[name + "_with_clearance_and_substep_ms"] = ms
        ms, _ = timed(lambda: (sim.dem_substep(), sim.clearance())[1], reps)
        res[name + "_clearance_and_substep_ms"] = ms
        c = sim.network(M, merge)
    t0 = time.perf_counter(); d2, _ = sim.clearance_planes(); t1 = time.perf_counter()
    H = sim.obst if M is None else M
    R = nu.finish_from(H, d2, merge)
    t2 = time.perf_counter()
    res[name + "_host_download_ms"], res[name + "_host_restate_ms"] = round(1e3 * (t1 - t0), 1), round(1e3 * (t2 - t1), 1)
    body, group = sim.network_planes()
    D = dict(counts=c, body=body, group=group, bodies=sim.network_bodies(), groups=sim.network_groups(), links0=sim.network_links(0),
             links1=sim.network_links(1))
    assert nu.same(D, R) is None, (name, nu.same(D, R))
    print(name, "download ms", res[name + "_host_download_ms"], "restatement ms", res[name + "_host_restate_ms"], "all outputs equal",
          flush=True)
for merge in (-1, 0, 1, 2):
    c = sim.network(None, merge)
    g = sim.network_groups()
    res["packing_counts_m%d" % merge] = dict(c, mean_group_degree=round(float(g["degree"].mean()), 3))
    print("merge", merge, res["packing_counts_m%d" % merge], flush=True)
print(json.dumps(res))
