"""How long a checkpoint holds its caller at 4096^2 / 50 000 grains, with lbmdem_checkpoint_save and with
lbmdem_checkpoint_save_async called with a free slot, and what a cadence inside lbmdem_run_scene costs per coupled step. Run on an
MI355X from the repository root: python scripts/async_checkpoint_cost.py [outdir] [cadence_substeps] [steps].
Under `rocprofv3 --kernel-trace --stats -- python scripts/async_checkpoint_cost.py` the kernel table has k_ckpt_frame.
Wall-clock times, ms; the run arms alternate."""
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
out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="ckpt_")
every = int(sys.argv[2]) if len(sys.argv) > 2 else 1200
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3600
os.makedirs(out, exist_ok=True)
sim = pkg.LbmDem(lx, ly, r, x1, x2)
sim.renderScene(120)
sim.sync()
print("file system of %s: %s" % (out, os.popen("df -T %s | tail -1" % out).read().split()[1:2]))
A, B = os.path.join(out, "sync.ckpt"), os.path.join(out, "async.ckpt")


def held(fn):
    sim.sync()
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


print("checkpoint_save, caller held: %s ms" % ["%.1f" % held(lambda: sim.checkpoint_save(A)) for _ in range(3)])
sim.set_async_checkpoint(1)
for k in range(3):
    h = held(lambda: sim.checkpoint_save_async(B))           # a free slot: returns behind the launch
    t0 = time.perf_counter(); sim.sync(); t1 = time.perf_counter(); sim.output_drain(); t2 = time.perf_counter()
    print("checkpoint_save_async, caller held: %.3f ms; step stream busy %.2f ms more; drain afterwards %.1f ms"
          % (h, 1e3 * (t1 - t0), 1e3 * (t2 - t1)))
print(sim.output_stats_checkpoint())
size = os.path.getsize(A)
body = open(B, "rb").read(size)
print("file %d bytes; async file = synchronous file + %d bytes of trailer: %s; verify: %s"
      % (size, os.path.getsize(B) - size, body == open(A, "rb").read(), pkg.LbmDem.checkpoint_verify(B)))
del body
print("measure_copy for the same bytes: %.0f GB/s read + written -> %.3f ms" % (sim.measure_copy(size), 2 * size / sim.measure_copy(size) * 1e-6))
sim.set_async_checkpoint(0)

# the cadence: run_scene without it, with it synchronously, with it in the background; alternating, two rounds
npdem = sim.cfg.npDEM
for rnd in range(2):
    for arm in ("off", "sync", "async"):
        sim.set_async_checkpoint(1 if arm == "async" else 0)
        sim.set_checkpoint_every(0 if arm == "off" else every, os.path.join(out, "cadence.ckpt"))
        sim.sync()
        t0 = time.perf_counter()
        sim.run_scene(steps)
        sim.sync()
        dt = time.perf_counter() - t0
        print("run_scene(%d), cadence %s: %.3f s = %.1f us per coupled step%s" % (
            steps, arm if arm == "off" else "%d %s" % (every, arm), dt, 1e6 * dt / (steps / npdem),
            "  " + str(sim.output_stats_checkpoint()) if arm == "async" else ""))
sim.close()
