"""Cost of the network pressure analysis (lbmdem_netsolve_compute) on the flagship workload, 4096^2 / 50 000 grains after three
coupled steps: T -> B, band 8, rtol 1e-8, warmed calls at level 0 and 1 with the network result there -- iterations, launches, ms
per call (the call ends in a synchronise) and per iteration -- against what it replaces on the same box: the downloads of the
planes and the tables plus tests/netsolve_util.py's restatement over them, with every output compared on the bits, and
scipy.sparse.linalg's CG on the same matrix where scipy is installed.
    python scripts/netsolve_cost.py"""
import json, os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench
import __graft_entry__ as ge
import netsolve_util as su
pkg = ge.load_package()
w = bench.workload("metric")
(r, x1, x2), _ = bench.make_sample(w)
sim = pkg.LbmDem(w["lx"], w["ly"], r, x1, x2)
sim.renderScene(3 * sim.cfg.npDEM); sim.sync()
MERGE, FROM, BAND, TO, RTOL = 1, pkg.SIDE_T, 8, pkg.SIDE_B, 1e-8
res = {"grains": int(sim.n), "lattice": [sim.lx, sim.ly], "merge": MERGE, "band": BAND, "rtol": RTOL}


def timed(call, reps):
    call(); call()
    ms = []
    for rep in range(reps):
        sim.sync()
        t0 = time.perf_counter(); out = call(); t1 = time.perf_counter()
        ms.append(round(1e3 * (t1 - t0), 3))
    return ms, out


sim.network(None, MERGE)
for level in (0, 1):
    ms, (c, s) = timed(lambda: sim.netsolve(FROM, BAND, TO, MERGE, level, rtol=RTOL), 5)   # (the network result is reused)
    ms5, _ = timed(lambda: sim.netsolve(FROM, BAND, TO, MERGE, level, rtol=RTOL, max_iter=1), 5)   # (the build and one batch)
    rounds = sim.netsolve(FROM, BAND, TO, MERGE, level, rtol=RTOL) and sim.netsolve_rounds()
    per_iter = (min(ms) - min(ms5)) / max(1, rounds // 2 - 16)
    res["level%d" % level] = dict(ms=ms, ms_one_batch=ms5, counts=c, sums=s, launches=rounds, ms_per_iteration=round(per_iter, 4),
                                  permeability=sim.netsolve_permeability(), largest_degree=int(sim.netsolve_regions()["degree"].max()))
    print("level", level, res["level%d" % level], flush=True)
for level in (0, 1):
    c, s = sim.netsolve(FROM, BAND, TO, MERGE, level, rtol=RTOL)
    D = dict(counts=c, sums=s, regions=sim.netsolve_regions(), links=sim.netsolve_links())
    t0 = time.perf_counter()
    body, group = sim.network_planes()
    net = dict(body=body, group=group, bodies=sim.network_bodies(), groups=sim.network_groups(), links0=sim.network_links(0),
               links1=sim.network_links(1))
    t1 = time.perf_counter()
    W = su.restate(sim.obst, sim.n, FROM, BAND, TO, MERGE, level, rtol=RTOL, N=net)
    t2 = time.perf_counter()
    res["level%d_host_download_ms" % level], res["level%d_host_restate_ms" % level] = round(1e3 * (t1 - t0), 1), round(1e3 * (t2 - t1), 1)
    assert su.same(D, W) is None, (level, su.same(D, W))
    print("level", level, "download ms", round(1e3 * (t1 - t0), 1), "restatement ms", round(1e3 * (t2 - t1), 1), "all outputs equal", flush=True)
    try:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
    except ImportError:
        res["scipy"] = "not installed"
        continue
    t0 = time.perf_counter()
    R = len(W["regions"])
    f = np.nonzero(W["free"] & su.anchored(W))[0]
    A = sp.coo_matrix((np.concatenate([-W["g"], -W["g"]]), (np.concatenate([W["lo"], W["hi"]]), np.concatenate([W["hi"], W["lo"]]))),
                      shape=(R, R)).tocsr()
    A = (A - sp.diags(np.asarray(A.sum(axis=1)).ravel())).tocsr()[f][:, f]
    x, info = spl.cg(A, W["b"][f], rtol=RTOL, M=sp.diags(1.0 / A.diagonal()))
    res["level%d_scipy_cg_ms" % level] = round(1e3 * (time.perf_counter() - t0), 1)
    print("level", level, "scipy cg ms", res["level%d_scipy_cg_ms" % level], "info", info, "max |x - x_device|",
          float(np.abs(x - W["x"][f]).max()), flush=True)
print(json.dumps(res))
