"""What a VTK frame costs at 4096^2 / 50 000 grains, stage by stage, and how long the step stream is held by a frame with and
without lbmdem_set_async_output. Run on an MI355X from the repository root: python scripts/async_output_cost.py [outdir].
Under `rocprofv3 --kernel-trace --stats -- python scripts/async_output_cost.py` the kernel table has k_vtk_frame next to
k_vtk_fields (three launches each). Wall-clock times between two lbmdem_sync()s, milliseconds."""
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
out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="frames_")
os.makedirs(out, exist_ok=True)
sim = pkg.LbmDem(lx, ly, r, x1, x2)
sim.renderScene(4000)     # the sub-step that reaches 4000 leaves the diagnostics write_DEM needs
sim.sync()


def ms(fn):
    sim.sync()
    t0 = time.perf_counter()
    fn()
    sim.sync()
    return 1e3 * (time.perf_counter() - t0)


print("copy yardstick (lbmdem_measure_copy): %.0f GB/s" % sim.measure_copy())
print("file system of %s: %s" % (out, os.popen("df -T %s | tail -1" % out).read().split()[1:2]))
print("write_DEM + write_forces: %s ms" % ["%.1f" % ms(lambda: (sim.write_DEM(out, 0), sim.write_forces(out, 0))) for _ in range(3)])
print("vtk_fields() (k_vtk_fields + 5 pageable copies): %s ms" % ["%.1f" % ms(sim.vtk_fields) for _ in range(3)])
print("vtk_image() (k_vtk_frame + 1 pageable copy): %s ms" % ["%.1f" % ms(sim.vtk_image) for _ in range(3)])
print("write_vtk, step stream held: %s ms" % ["%.1f" % ms(lambda: sim.write_vtk(out, 0)) for _ in range(3)])
img = sim.vtk_image()
t0 = time.perf_counter(); pkg.write_vtk_image(out, 1, lx, ly, img); t1 = time.perf_counter()
print("write_vtk_image (file I/O alone): %.1f ms" % (1e3 * (t1 - t0)))
sim.set_async_output(2)
for k in range(3):
    held = ms(lambda: sim.write_vtk_async(out, 2 + k))      # returns behind the snapshot kernel; sync() waits for that kernel only
    t0 = time.perf_counter(); sim.output_drain(); t1 = time.perf_counter()
    print("write_vtk_async, step stream held: %.2f ms; drain afterwards %.1f ms" % (held, 1e3 * (t1 - t0)))
print(sim.output_stats())
sim.close()
