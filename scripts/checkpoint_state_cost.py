"""What a checkpoint that carries the optional state costs at 4096^2 / 50 000 grains: how long lbmdem_checkpoint_save_async holds
its caller and the step stream with nothing selected (lbmdem_set_checkpoint_contents(h, 0)) and with 65 536 tracers, the scalar
and a window of all eleven planes selected and present, the slots' growth between the two, and the files' sizes. Run on an
MI355X from the repository root: python scripts/checkpoint_state_cost.py [outdir]. Wall-clock times, ms."""
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import __graft_entry__ as ge
import samples

pkg = ge.load_package()
lx = ly = 4096
r, x, y = samples.row_packing(lx, ly, 50000, seed=1234)
r, x1, x2 = samples.to_metres(r, x, y)
out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="ckpt_state_")
os.makedirs(out, exist_ok=True)
sim = pkg.LbmDem(lx, ly, r, x1, x2)
sim.renderScene(120)
sim.set_async_checkpoint(1)
path = os.path.join(out, "state.ckpt")


def rounds(label, n=4):
    for k in range(n):
        sim.sync()
        t0 = time.perf_counter()
        sim.checkpoint_save_async(path)
        t1 = time.perf_counter(); sim.sync(); t2 = time.perf_counter(); sim.output_drain(); t3 = time.perf_counter()
        print("%s: caller held %.3f ms; step stream busy %.3f ms more; drain afterwards %.1f ms; file %d bytes, verify %s, %s"
              % (label, 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), os.path.getsize(path), pkg.LbmDem.checkpoint_verify(path),
                 pkg.LbmDem.checkpoint_contents(path)))
    print("   ", sim.output_stats_checkpoint())


rounds("nothing selected")
g = (np.arange(256) + 0.5) * (lx - 1) / 256
sim.set_tracers(np.stack([np.repeat(g, 256), np.tile(g, 256)], axis=1))
sim.set_scalar(np.ones((lx, ly)), 0.8)
sim.begin_mean(pkg.MEAN_ALL, 1)
sim.renderScene(4 * sim.cfg.npDEM)
rounds("selected 0, all three present")          # still the plain file
sim.set_checkpoint_contents(pkg.CKPT_ALL)
rounds("CKPT_ALL, all three present")            # the first call drains and makes the slot larger
sim.set_checkpoint_contents(pkg.CKPT_TRACERS)
rounds("CKPT_TRACERS alone", 2)
sim.close()
