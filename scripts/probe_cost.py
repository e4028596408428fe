"""Cost of the probe recorder (lbmdem_probe_*) on the flagship workload: renderScene at 4096^2 / 50 000 grains with the probes
off and on (every = 1, all fields), alternating, ms per coupled step; `trace`: a short probing run for rocprofv3 --kernel-trace --stats.
    python scripts/probe_cost.py [trace]"""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench
import __graft_entry__ as ge
pkg = ge.load_package()
w = bench.workload("metric")
(r, x1, x2), _ = bench.make_sample(w)
sim = pkg.LbmDem(w["lx"], w["ly"], r, x1, x2)
npdem = sim.cfg.npDEM
trace_only = len(sys.argv) > 1 and sys.argv[1] == "trace"
pts = [(17 + 61 * k, 5 + 63 * k) for k in range(64)]
if trace_only:
    sim.probe_enable(every=1, capacity=256, pressure_row=2, points=pts)
    sim.renderScene(100 * npdem); sim.sync()
    got = sim.probe_read()
    print("trace run:", len(got["step"]), "records", got["dropped"], "dropped")
    sys.exit(0)
sim.renderScene(40 * npdem); sim.sync()
K = 200
res = {"off": [], "on": []}
for rep in range(4):
    for mode in ("off", "on"):
        if mode == "on":
            sim.probe_enable(every=1, capacity=K + 8, pressure_row=2, points=pts)
        sim.sync()
        t0 = time.perf_counter(); sim.renderScene(K * npdem); sim.sync(); t1 = time.perf_counter()
        if mode == "on":
            got = sim.probe_read()
            assert len(got["step"]) == K and got["dropped"] == 0
            sim.probe_disable()
        res[mode].append(1e3 * (t1 - t0) / K)
        print(rep, mode, "%.4f ms per coupled step" % res[mode][-1], flush=True)
res["delta_us"] = [1e3 * (b - a) for a, b in zip(res["off"], res["on"])]
print(json.dumps(res))


