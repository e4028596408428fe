"""Cost of the pore flux analysis (lbmdem_netflux_compute) on the flagship workload, 4096^2 / 50 000 grains after three coupled
steps: warmed calls at level 0 and 1, ms per call (the call ends in a synchronise), with the network result there and with it made
again (a fluid step in front), against what it replaces on the same box -- the downloads of f, the two planes and the tables plus
tests/netflux_util.py's restatement over them -- with every output compared; `trace`: a few calls for rocprofv3 --kernel-trace
--stats, from which k_nf_plane's share is read (its floor: one read of f where fluid, 72 B a node, and of the label plane, 4 B).
    python scripts/netflux_cost.py [trace]"""
import json, os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench
import __graft_entry__ as ge
import netflux_util as fu
pkg = ge.load_package()
w = bench.workload("metric")
(r, x1, x2), _ = bench.make_sample(w)
sim = pkg.LbmDem(w["lx"], w["ly"], r, x1, x2)
sim.renderScene(3 * sim.cfg.npDEM); sim.sync()
MERGE = 1
if len(sys.argv) > 1 and sys.argv[1] == "trace":
    for rep in range(4):
        c = sim.netflux(MERGE, rep & 1)
    print("trace run:", c)
    sys.exit(0)
res = {"grains": int(sim.n), "lattice": [sim.lx, sim.ly], "merge": MERGE}


def timed(call, reps):
    call(); call()
    ms = []
    for rep in range(reps):
        sim.sync()
        t0 = time.perf_counter(); out = call(); t1 = time.perf_counter()
        ms.append(round(1e3 * (t1 - t0), 3))
    return ms, out


for level in (0, 1):
    ms, c = timed(lambda: sim.netflux(MERGE, level), 5)                      # (the network result is reused)
    res["level%d_ms" % level], res["level%d_counts" % level] = ms, c
    print("level", level, "ms per call", ms, c, flush=True)
ms, _ = timed(lambda: (sim.lbm_step(), sim.netflux(MERGE, 0))[1], 3)        # (a fluid step: clearance and network again)
res["with_network_and_step_ms"] = ms
ms, _ = timed(lambda: (sim.lbm_step(), sim.network(None, MERGE))[1], 3)
res["network_and_step_ms"] = ms
ms, _ = timed(lambda: sim.lbm_step(), 3)
res["step_ms"] = ms
print({k: v for k, v in res.items() if k.endswith("_ms")}, flush=True)
for level in (0, 1):
    c = sim.netflux(MERGE, level)
    col, row = sim.netflux_profile()
    D = dict(counts=c, links=sim.netflux_links(), regions=sim.netflux_regions(), col=col, row=row)
    t0 = time.perf_counter()
    f = sim.f
    body, group = sim.network_planes()
    net = dict(body=body, group=group, bodies=sim.network_bodies(), groups=sim.network_groups(), links0=sim.network_links(0),
               links1=sim.network_links(1))
    t1 = time.perf_counter()
    W = fu.restate(sim.obst, f, sim.n, MERGE, level, N=net)
    t2 = time.perf_counter()
    res["level%d_host_download_ms" % level], res["level%d_host_restate_ms" % level] = round(1e3 * (t1 - t0), 1), round(1e3 * (t2 - t1), 1)
    assert fu.same(D, W) is None, (level, fu.same(D, W))
    print("level", level, "download ms", round(1e3 * (t1 - t0), 1), "restatement ms", round(1e3 * (t2 - t1), 1), "all outputs equal", flush=True)
print(json.dumps(res))
