"""Cost of the vibrating walls (lbmdem_set_vibration) on the flagship workload: 4096^2, the 50 000-grain row packing of
bench.py, coupled steps (npDEM sub-steps each), three handles stepped in interleaved rounds:
    off       the default handle
    off_noupd the default handle with lbmdem_set_obst_update(0) -- the map fast path vibration turns off, alone
    vib       vibrating walls (freq 2000 rad/s, amp 1e-9 m: the walls move, the packing is not crushed; Mgx moves ~1 % of a
              node over the run -- the cost measured is the mode's fixed per-step cost, which does not depend on the
              displacement, not that of a run whose walls shift the raster)
    python scripts/vib_cost.py [rounds] [steps per round]
Prints ms per coupled step per round, the medians, and the chain launches per fluid step of the vibrating handle."""
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
import samples  # noqa: E402

pkg = ge.load_package()
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
r, x, y = samples.row_packing(4096, 4096, 50000, seed=1234)
r, x1, x2 = samples.to_metres(r, x, y)
phys = pkg.Physics()
pkg.load_library().lbmdem_physics_defaults(__import__("ctypes").byref(phys))
phys.freq, phys.amp = 2000.0, 1e-9
sims = {name: pkg.LbmDem(4096, 4096, r, x1, x2, physics=phys) for name in ("off", "off_noupd", "vib")}
sims["off_noupd"].set_obst_update(False)
sims["vib"].set_vibration(True)
npdem = sims["off"].cfg.npDEM
for s in sims.values():   # warm-up: census, first list, first pictures
    s.renderScene(2 * npdem)
    s.sync()
times = {name: [] for name in sims}
l0 = sims["vib"].dem_chain_stats()[0]
for k in range(rounds):
    for name, s in sims.items():
        s.sync()
        t0 = time.perf_counter()
        s.renderScene(steps * npdem)
        s.sync()
        times[name].append((time.perf_counter() - t0) * 1e3 / steps)
    print("round", k, {n: round(v[-1], 4) for n, v in times.items()}, flush=True)
launches = sims["vib"].dem_chain_stats()[0] - l0
med = {n: statistics.median(v) for n, v in times.items()}
print("median ms per coupled step", {n: round(v, 4) for n, v in med.items()})
print("vib vs off: %+.2f %%, of which the map fast path (off_noupd vs off): %+.2f %%" %
      (100 * (med["vib"] / med["off"] - 1), 100 * (med["off_noupd"] / med["off"] - 1)))
print("chain launches per coupled step (vibrating):", launches / (rounds * steps), "walls", sims["vib"].walls())
