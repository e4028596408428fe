"""Cost of the pore clearance analysis (lbmdem_clearance_compute) on the flagship workload, 4096^2 / 50 000 grains after three
coupled steps, and on the worst case of the column walk, an all-fluid 4096^2 map: warmed calls, ms per call (the call ends in a
synchronise), against what it replaces on the same box -- download_obst plus scipy.ndimage.distance_transform_edt -- with d2
compared; `trace`: a few calls of each for rocprofv3 --kernel-trace --stats.
    python scripts/clearance_cost.py [trace]"""
import json, os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench
import __graft_entry__ as ge
pkg = ge.load_package()
w = bench.workload("metric")
(r, x1, x2), _ = bench.make_sample(w)
sim = pkg.LbmDem(w["lx"], w["ly"], r, x1, x2)
sim.renderScene(3 * sim.cfg.npDEM); sim.sync()
fluid_map = np.full((sim.lx, sim.ly), -1, np.int32)
trace_only = len(sys.argv) > 1 and sys.argv[1] == "trace"
if trace_only:
    for rep in range(4):
        c = sim.clearance()
    for rep in range(2):
        c = sim.clearance(fluid_map)
    print("trace run:", c)
    sys.exit(0)
res = {"grains": int(sim.n), "lattice": [sim.lx, sim.ly]}
for name, M, reps in (("packing", None, 7), ("all_fluid", fluid_map, 3)):
    sim.clearance(M); sim.clearance(M)
    ms = []
    for rep in range(reps):
        sim.sync()
        t0 = time.perf_counter(); c = sim.clearance(M); t1 = time.perf_counter()
        ms.append(1e3 * (t1 - t0))
    res[name + "_ms"] = [round(v, 3) for v in ms]
    res[name + "_counts"] = c
    print(name, "ms per call", res[name + "_ms"], c, flush=True)
    t0 = time.perf_counter(); d2, owner = sim.clearance_planes(); res[name + "_planes_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
    t0 = time.perf_counter(); tab = sim.throat_table(); res[name + "_table_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
    assert len(tab) == c["throats"] and int(tab["edges"].sum()) == c["ridge_edges"] and int((d2 > 0).sum()) == c["fluid_nodes"]
    from scipy import ndimage
    dl, edt = [], []
    for rep in range(2):
        t0 = time.perf_counter(); H = sim.obst if M is None else M; t1 = time.perf_counter()
        P = np.zeros((sim.lx + 2, sim.ly + 2), bool)
        P[1:-1, 1:-1] = H == -1
        ref = ndimage.distance_transform_edt(P)[1:-1, 1:-1]
        t2 = time.perf_counter()
        dl.append(round(1e3 * (t1 - t0), 1)); edt.append(round(1e3 * (t2 - t1), 1))
    assert np.array_equal(d2, np.rint(ref * ref).astype(np.int64)), name
    res[name + "_host_download_ms"], res[name + "_host_edt_ms"] = dl, edt
    print(name, "download ms", dl, "distance_transform_edt ms", edt, flush=True)
print(json.dumps(res))
