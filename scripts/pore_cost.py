"""Cost of the pore space analysis (lbmdem_pore_compute) on the flagship workload, 4096^2 / 50 000 grains after three coupled
steps: warmed calls of pores(4) and pores(8), ms per call (the call ends in a synchronise), against what it replaces on the same
box -- download_obst plus scipy.ndimage.label (tests/pore_util.py's restatement where scipy has no ndimage) -- with the component
count of the two compared; `trace`: a few calls for rocprofv3 --kernel-trace --stats.
    python scripts/pore_cost.py [trace]"""
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
trace_only = len(sys.argv) > 1 and sys.argv[1] == "trace"
if trace_only:
    for conn in (4, 8, 4, 8, 4, 8, 4, 8):
        c = sim.pores(conn)
    print("trace run:", c)
    sys.exit(0)
res = {"grains": int(sim.n), "lattice": [sim.lx, sim.ly]}
for conn in (4, 8):
    sim.pores(conn); sim.pores(conn)
    ms = []
    for rep in range(7):
        sim.sync()
        t0 = time.perf_counter(); c = sim.pores(conn); t1 = time.perf_counter()
        ms.append(1e3 * (t1 - t0))
    res["pores_%d_ms" % conn] = [round(v, 4) for v in ms]
    res["counts_%d" % conn] = c
    print(conn, "ms per call", res["pores_%d_ms" % conn], c, flush=True)
t0 = time.perf_counter(); lab = sim.pore_labels(); res["pore_labels_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
t0 = time.perf_counter(); tab = sim.pore_table(); res["pore_table_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
assert len(tab) == res["counts_8"]["components"] and int(tab["nodes"].sum()) == res["counts_8"]["fluid_nodes"] == int((lab >= 0).sum())
try:
    from scipy import ndimage
    how = "scipy.ndimage.label"
except ImportError:
    ndimage, how = None, "tests/pore_util.py components()"
import pore_util
res["host_path"] = how
for conn, structure in ((4, [[0, 1, 0], [1, 1, 1], [0, 1, 0]]), (8, [[1, 1, 1]] * 3)):
    dl, lb = [], []
    for rep in range(3):
        t0 = time.perf_counter(); M = sim.obst; t1 = time.perf_counter()
        if ndimage is not None:
            ref, count = ndimage.label(M == -1, structure=structure)
        else:
            count = len(np.unique(pore_util.components(M, conn))) - 1
        t2 = time.perf_counter()
        dl.append(round(1e3 * (t1 - t0), 1)); lb.append(round(1e3 * (t2 - t1), 1))
    assert count == res["counts_%d" % conn]["components"], (conn, count)
    res["host_%d_download_ms" % conn], res["host_%d_label_ms" % conn] = dl, lb
    print(conn, how, "download ms", dl, "label ms", lb, "components", count, flush=True)
print(json.dumps(res))
