"""Cost of the strain analysis (lbmdem_strain_mark, lbmdem_strain_compute) on the flagship workload, 4096^2 / 50 000 grains: the
mark after three coupled steps, the compute after three more, at cutoffs of 3 and 10 mean diameters; warmed calls, ms per call (both
calls end in a synchronise), against what they replace on the same box -- the download of the kinematics plus tests/strain_util.py's
restatement over the same mark -- with every output compared; `trace`: a few calls for rocprofv3 --kernel-trace --stats, from which
the split by kernel is read. The floor printed beside it: one read of the 32-byte records through the list at 8 TB/s.
    python scripts/strain_cost.py [trace]"""
import json, os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench
import __graft_entry__ as ge
import strain_util as su
pkg = ge.load_package()
w = bench.workload("metric")
(r, x1, x2), _ = bench.make_sample(w)
sim = pkg.LbmDem(w["lx"], w["ly"], r, x1, x2)
sim.renderScene(3 * sim.cfg.npDEM); sim.sync()
D = 2.0 * float(np.mean(r))
TRACE = len(sys.argv) > 1 and sys.argv[1] == "trace"
res = {"grains": int(sim.n), "lattice": [sim.lx, sim.ly], "mean_diameter": D}


def timed(call, reps):
    call(); call()
    ms = []
    for rep in range(reps):
        sim.sync()
        t0 = time.perf_counter(); out = call(); t1 = time.perf_counter()
        ms.append(round(1e3 * (t1 - t0), 3))
    return ms, out


k_mark = sim.kinematics
for cut in (3, 10):
    sim.kinematics = k_mark
    sim.structure(cut * D, 1, 1.0)
    if TRACE:
        sim.strain_mark()
        sim.renderScene(3 * sim.cfg.npDEM)
        for rep in range(4):
            c = sim.strain()
        print("trace run:", cut, c)
        continue
    ms_mark, entries = timed(sim.strain_mark, 7)
    sim.renderScene(3 * sim.cfg.npDEM); sim.sync()
    ms, c = timed(sim.strain, 7)
    floor_us = 1e6 * (32.0 * entries) / 8e12          # one read of a 32-byte record per entry (the lane walks the list twice)
    res["cut%d" % cut] = dict(entries=entries, mark_ms=ms_mark, compute_ms=ms, counts=c, floor_us=round(floor_us, 2))
    print("cut", cut, "entries", entries, "mark ms", ms_mark, "compute ms", ms, "floor us", round(floor_us, 2), c, flush=True)
    g = sim.strain_grains()
    ref = sim.strain_reference()
    t0 = time.perf_counter()
    k = sim.kinematics
    t1 = time.perf_counter()
    R = su.restate(ref["x0"], ref["y0"], ref["th0"], ref["offsets"], ref["nbr"], ref["rc2"], k[:, 0], k[:, 1], k[:, 2])
    t2 = time.perf_counter()
    assert c == R["counts"], (c, R["counts"])
    for name in su.INTS:
        assert np.array_equal(g[name], R["grains"][name]), name
    for name in su.DOUBLES:
        assert su.same_bits(g[name], R["grains"][name]), name
    res["cut%d" % cut].update(host_download_ms=round(1e3 * (t1 - t0), 2), host_restate_ms=round(1e3 * (t2 - t1), 1))
    print("cut", cut, "download ms", round(1e3 * (t1 - t0), 2), "restatement ms", round(1e3 * (t2 - t1), 1), "all outputs equal",
          flush=True)
if not TRACE:
    print(json.dumps(res))
