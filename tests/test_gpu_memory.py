"""GPU: who frees what. Every device and pinned block of the library comes from a MemPool (2d-lbm-dem_amd/csrc/lbm_mem.h) that
counts, process-wide, the blocks it has handed out and their bytes; the experiment build exports the two numbers
(live_memory()). Each case reads them first and finds them again afterwards: a handle with every optional buffer in use, two
strips with distributed grains, the calls that take scratch for their own duration, a create that runs out of memory, and the
communicator. The cases run in fresh child processes with the experiment build, as the give-up tests of test_gpu_dem_chain.py."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB_LIB = os.path.join(ROOT, "2d-lbm-dem_amd", "liblbmdem_hip_ab.so")
SHIM = os.path.join(ROOT, "tests", "rccl_shim", "librccl.so.1")

PRELUDE = r"""
import os, sys
import ctypes as C
import numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import __graft_entry__ as ge
pkg = ge.load_package()
import torch
torch.cuda.init()
LA = (37, 50, np.array([0.62, 0.55, 0.70]) * 1e-3, np.array([0.35, 1.47, 2.60]) * 1e-3, np.array([1.30, 1.30, 4.75]) * 1e-3)
"""

HANDLE = PRELUDE + r"""
import golden_util as gu
out = sys.argv[1]
base = pkg.live_memory()
sim = pkg.LbmDem(64, 48, *gu.inputs_m("G5_dem_64x48"))
created = pkg.live_memory()
assert created[0] > base[0] and created[1] > base[1], (base, created)
sim.probe_enable(capacity=16, points=[(3, 4), (40, 30)])
first = pkg.live_memory()
sim.probe_enable(capacity=64, points=[(3, 4), (40, 30)])          # the old ring goes, a larger one comes
second = pkg.live_memory()
assert second[0] == first[0] == created[0] + 3 and second[1] > first[1], (created, first, second)
sim.set_diagnostics(True)
sim.set_vibration(True)
sim.set_change_mask(2)
for setter in (sim.set_async_output, sim.set_async_dem, sim.set_async_checkpoint):
    for slots in (2, 1, 0, 2):
        setter(slots)
npdem = sim.cfg.npDEM
sim.renderScene(npdem)
sim.write_vtk_async(out, 0)
sim.write_DEM_async(out, 0)
sim.checkpoint_save_async(os.path.join(out, "state.ckpt"))
sim.renderScene(npdem)
sim.output_drain()
names = set(os.listdir(out))
assert {"fluid_pressure_000000.vtk", "DEM000000.dat", "state.ckpt"} <= names, names
busy = pkg.live_memory()
assert busy[0] > second[0] and busy[1] > second[1], (second, busy)
sim.probe_disable()
assert pkg.live_memory()[0] == busy[0] - 3
sim.close()
assert pkg.live_memory() == base, (base, pkg.live_memory())
print("MEMORY-OK handle", base, created, busy)
"""

STRIPS = PRELUDE + r"""
lx, ly, r, x1, x2 = LA
base = pkg.live_memory()
cut = lx // 2
sims = [pkg.LbmDem(lx, ly, r, x1, x2, strip=s, halo=2) for s in ((0, cut), (cut, lx))]
plain = pkg.live_memory()
for s in sims:
    s.dist_enable(6)        # (a margin the 18 rows of a strip have room for: nothing is stepped here)
    s.dist_begin_period()
    s.sync()
dist = pkg.live_memory()
assert dist[0] > plain[0] > base[0], (base, plain, dist)
for s in sims:
    s.close()
assert pkg.live_memory() == base, (base, pkg.live_memory())
print("MEMORY-OK strips", base, plain, dist)
"""

CALLS = PRELUDE + r"""
import golden_util as gu
out = sys.argv[1]
c = gu.ALL_CASES["S_13x61"]
shapes = [LA, (13, 61, np.asarray(c["r_mm"]) * 1e-3, np.asarray(c["x_mm"]) * 1e-3, np.asarray(c["y_mm"]) * 1e-3)]
base = pkg.live_memory()
for lx, ly, r, x1, x2 in shapes:
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    sim.renderScene(sim.cfg.npDEM)
    held = pkg.live_memory()
    def same(what):
        assert pkg.live_memory() == held, (what, held, pkg.live_memory())
    assert sim.geometry_stats()["links"] > 0; same("geometry_stats")
    assert len(sim.download_links()) > 0; same("download_links")
    sim.write_densities(out, 0); same("write_densities")
    whole = sim.densities_text(); same("densities_text")
    sim.set_densities_staging(300)
    banded = sim.densities_text(); same("densities_text in bands")
    assert banded == whole and sim.densities_stats()[2] > 4, sim.densities_stats()
    sim.f = sim.f; same("upload_f, download_f")
    sim.macro(); sim.vtk_fields(); sim.vtk_image(); sim.final_density(); same("downloads")
    sim.close()
    assert pkg.live_memory() == base, (base, pkg.live_memory())
print("MEMORY-OK calls", base)
"""

FAILED_CREATE = PRELUDE + r"""
total = torch.cuda.get_device_properties(0).total_memory
side = int(np.ceil(np.sqrt(total / 72.0))) + 16       # 72 bytes of populations per node: f[0] alone is more than the device has
assert 72 * side * side > total
r, x1, x2 = LA[2:]
L = pkg.load_library()
cfg = pkg.derive(side, side, r)
base = pkg.live_memory()
h = C.c_void_p(0xdead)
rc = L.lbmdem_create(C.byref(cfg), r.ctypes.data_as(C.c_void_p), x1.ctypes.data_as(C.c_void_p), x2.ctypes.data_as(C.c_void_p), C.byref(h))
msg = L.lbmdem_last_error().decode()
assert rc == -4, (rc, msg)                            # LBMDEM_ENOMEM
assert not h.value, h.value
assert pkg.live_memory() == base, (base, pkg.live_memory())
sim = pkg.LbmDem(*LA)                                 # ... and the device is none the worse
sim.renderScene(3)
sim.close()
assert pkg.live_memory() == base
print("MEMORY-OK failed_create", side, msg)
"""

COMM = PRELUDE + r"""
import time, samples
strips = pkg.strips_module()
rank, world, idfile = int(os.environ["RANK"]), int(os.environ["WORLD"]), os.environ["IDFILE"]
lx, ly = 320 * world, 192
r, x, y = samples.row_packing(lx, ly, 230 * world, seed=21)
r, x1, x2 = samples.to_metres(r, x, y)
base = pkg.live_memory()
if rank == 0:
    uid = pkg.comm_unique_id()
    open(idfile + ".tmp", "wb").write(uid); os.rename(idfile + ".tmp", idfile)
else:
    t0 = time.time()
    while not os.path.exists(idfile):
        assert time.time() - t0 < 60
        time.sleep(0.01)
    uid = open(idfile, "rb").read()
comm = pkg.Comm(uid, rank, world, 0)
sim = pkg.LbmDem(lx, ly, r, x1, x2, strip=strips.partition(lx, world)[rank], halo=2)
sim.dist_enable(0)
comm.selftest(4096)
s = comm.allreduce_sum(np.array([rank + 1.0]))
assert s[0] == world * (world + 1) / 2, s
comm.run(sim, sim.cfg.npDEM)
sim.sync()
assert pkg.live_memory()[0] > base[0]
comm.close()
sim.close()
print("MEMORY-OK comm rank %d" % rank, base, pkg.live_memory())
assert pkg.live_memory() == base, (base, pkg.live_memory())
"""


def ab_env(**extra):
    if not os.path.exists(AB_LIB):
        pytest.skip("the experiment build (make -C 2d-lbm-dem_amd/csrc AB=1) is not there")
    return dict(os.environ, LBMDEM_HIP_LIBRARY=AB_LIB, **extra)


def run_case(script, what, *args):
    out = subprocess.run([sys.executable, "-c", script, *args], cwd=ROOT, env=ab_env(), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "MEMORY-OK " + what in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_a_handle_with_everything_on_gives_all_of_it_back(tmp_path):
    """64 x 48 with grains: probes enabled twice (the first ring is released), diagnostics, vibration, the verified change mask,
    frames, tables and checkpoints in the background with their slots resized 2 -> 1 -> 0 -> 2, one file of each kind, probes
    off again. Blocks and bytes are above the baseline while the handle is open and at it after close()."""
    run_case(HANDLE, "handle", str(tmp_path))


def test_strip_handles_with_distributed_grains():
    """two strips of a 37 x 50 lattice on one device, dist_enable() on both, one period begun"""
    run_case(STRIPS, "strips")


def test_calls_with_their_own_scratch_leave_nothing(tmp_path):
    """37 x 50 and 13 x 61: geometry_stats, download_links, write_densities, densities_text whole and in bands of a few hundred
    bytes, the state transfers -- the live numbers are the same before and after every call"""
    run_case(CALLS, "calls", str(tmp_path))


def test_a_create_that_runs_out_of_memory_leaves_nothing():
    """a lattice whose first population buffer alone is larger than the device's memory: LBMDEM_ENOMEM, a null handle, the
    live numbers untouched"""
    run_case(FAILED_CREATE, "failed_create")


def test_communicator_and_its_handle_with_two_ranks_on_one_gpu(tmp_path):
    """world 2 through tests/rccl_shim: one selftest, one all-reduce, one fluid period of lbmdem_comm_run; after comm.close()
    and sim.close() every rank is back at its baseline"""
    if not os.path.exists(SHIM):
        pytest.skip("tests/rccl_shim/librccl.so.1 is not built")
    env = ab_env(LBMDEM_RCCL_LIBRARY=SHIM, RCCL_SHIM_TIMEOUT_S="30", WORLD="2", IDFILE=str(tmp_path / "rccl_id"))
    procs = [subprocess.Popen([sys.executable, "-c", COMM], cwd=ROOT, env=dict(env, RANK=str(k)), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for k in range(2)]
    try:
        outs = [p.communicate(timeout=300) + (p.returncode,) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for k, (o, e, rc) in enumerate(outs):
        assert rc == 0 and "MEMORY-OK comm rank %d" % k in o, o[-1000:] + e[-3000:]
