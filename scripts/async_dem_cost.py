"""What a write_DEM + write_forces event costs at 4096^2 / 50 000 grains and how long the step stream is held by one, with and
without lbmdem_set_async_dem. Run on an MI355X from the repository root: python scripts/async_dem_cost.py [outdir].
Under `rocprofv3 --kernel-trace --stats -- python scripts/async_dem_cost.py` the kernel table has k_dem_frame and k_dem_stats
(three launches of each from the events, three more from dem_stats()). Wall-clock times between two lbmdem_sync()s, ms."""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import __graft_entry__ as ge
import samples

pkg = ge.load_package()
lx = ly = 4096
r, x, y = samples.row_packing(lx, ly, 50000, seed=1234)
r, x1, x2 = samples.to_metres(r, x, y)
out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="tables_")
os.makedirs(out, exist_ok=True)
sim = pkg.LbmDem(lx, ly, r, x1, x2)
sim.renderScene(4000)     # the sub-step that reaches 4000 leaves the table
sim.sync()


def ms(fn):
    sim.sync()
    t0 = time.perf_counter()
    fn()
    sim.sync()
    return 1e3 * (time.perf_counter() - t0)


print("file system of %s: %s" % (out, os.popen("df -T %s | tail -1" % out).read().split()[1:2]))
print("write_DEM + write_forces, step stream held: %s ms" % ["%.1f" % ms(lambda: (sim.write_DEM(out, 0), sim.write_forces(out, 0))) for _ in range(3)])
print("dem_stats() (both kernels, a temporary, 176 bytes back): %s ms" % ["%.3f" % ms(sim.dem_stats) for _ in range(3)])
sim.set_async_dem(2)
for k in range(3):
    held = ms(lambda: sim.write_DEM_async(out, 1 + k))      # returns with the 22 numbers; the rest is the writer's
    t0 = time.perf_counter(); sim.output_drain(); t1 = time.perf_counter()
    print("write_DEM_async, step stream held: %.3f ms; drain afterwards %.1f ms" % (held, 1e3 * (t1 - t0)))
print(sim.output_stats_dem())
same = all(open(os.path.join(out, "DEM%06d.%s" % (k, e)), "rb").read() == open(os.path.join(out, "DEM000000.%s" % e), "rb").read()
           for k in (1, 2, 3) for e in ("dat", "ps"))
print("files identical to the synchronous writers':", same)
sim.close()
